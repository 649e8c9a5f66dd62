"""Cost of the voxel frame fill's per-pixel planes (sfrt_voxel_render_band_aux) at 4K.

    python tools/bench_voxel_aux.py [--warmup 10] [--frames 30] [--repeats 6]
                                    [--out profiles/voxel_aux_bench.json]

3840x2160, the default voxel world at the default pose (bench.py's "voxel_3840x2160" frame),
whole-frame bands on one stream, tile order off (the voxel renderer's default).  Three variants,
one world each, timed alternately in one process, `repeats` times each; every repeat warms
`warmup` frames and then times `frames` frames with a HIP event pair around each, the median
minus the empty pair's own time:

* plain:     sfrt_voxel_render_band -- the baseline, the same library in the same run;
* aux_depth: sfrt_voxel_render_band_aux, the depth plane only;
* aux_all:   sfrt_voxel_render_band_aux, depth, cell, face and steps.

The first repeat (the clock ramping up) is listed apart and left out of the medians.  No pass
threshold: the file records what the planes cost.  Each variant's bytes written per frame are
listed beside its times (4 bytes per pixel for the colour and for each plane).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sfml-software-raytracer_amd"))

WIDTH, HEIGHT = 3840, 2160
POSE = ((15.5, 1.9, 15.5), 0.0, 0.0)
VARIANTS = {"plain": (), "aux_depth": ("depth",), "aux_all": ("depth", "cell", "face", "steps")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_aux_bench.json"))
    a = ap.parse_args()
    if a.repeats < 2:
        raise SystemExit("bench_voxel_aux.py: --repeats must be at least 2 (the first is set apart)")

    import numpy as np
    import torch
    import sfrt
    import voxel_scenes as vs

    if sfrt.build_flavour() != "release":
        raise SystemExit("bench_voxel_aux.py times the release build only")
    stream = torch.cuda.Stream()
    pitch = 4 * WIDTH
    colour = torch.empty(HEIGHT, pitch, dtype=torch.uint8, device="cuda")
    planes = {p: torch.empty(HEIGHT, pitch, dtype=torch.uint8, device="cuda")
              for p in VARIANTS["aux_all"]}
    tex, dyn = vs.load_textures()
    scene = vs.default_world(*POSE)
    worlds = {}
    for name in VARIANTS:
        w = sfrt.VoxelWorld(0)
        w.load_assets(tex, dyn, vs.COLORS)
        w.set_scene(scene, WIDTH, HEIGHT)
        worlds[name] = w

    def fill(name):
        want = VARIANTS[name]
        if want:
            worlds[name].render_band_aux(colour.data_ptr(), pitch, 0, HEIGHT, stream.cuda_stream,
                                         **{p: (planes[p].data_ptr(), pitch) for p in want})
        else:
            worlds[name].render_band(colour.data_ptr(), pitch, 0, HEIGHT, stream.cuda_stream)

    def event_gap():
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                 for _ in range(64)]
        for x, y in pairs:
            x.record(stream)
            y.record(stream)
        torch.cuda.synchronize()
        return float(np.median([x.elapsed_time(y) for x, y in pairs]))

    def timed(name):
        for _ in range(a.warmup):
            fill(name)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(a.frames)]
        for x, y in ev:
            x.record(stream)
            fill(name)
            y.record(stream)
        torch.cuda.synchronize()
        worlds[name].check(stream.cuda_stream)
        raw = float(np.median([x.elapsed_time(y) for x, y in ev]))
        return round(max(0.0, raw - event_gap()) * 1e3, 2)

    runs = {name: [] for name in VARIANTS}
    for _ in range(a.repeats):
        for name in VARIANTS:
            runs[name].append(timed(name))
    frame_bytes = WIDTH * HEIGHT * 4
    base = float(np.median(runs["plain"][1:]))
    variants = {}
    for name, want in VARIANTS.items():
        kept = runs[name][1:]
        med = float(np.median(kept))
        variants[name] = {"planes": list(want), "bytes_written": frame_bytes * (1 + len(want)),
                          "first_repeat_us": runs[name][0], "kernel_us": kept,
                          "median_us": round(med, 2),
                          "range_us": round(max(kept) - min(kept), 2),
                          "vs_plain_percent": round(100.0 * (med / base - 1.0), 2)}
        print(f"{name:10s} {med:9.2f} us  range {variants[name]['range_us']:6.2f}  "
              f"first {runs[name][0]:9.2f}  {variants[name]['vs_plain_percent']:+6.2f} %  "
              f"{variants[name]['bytes_written'] / 1e6:6.1f} MB written")
    out = {"command": f"python tools/bench_voxel_aux.py --warmup {a.warmup} --frames {a.frames} "
                      f"--repeats {a.repeats}",
           "device": torch.cuda.get_device_name(0),
           "frame": {"width": WIDTH, "height": HEIGHT, "scene": "voxel default world",
                     "pose": [list(POSE[0]), POSE[1], POSE[2]], "tile_order": "off",
                     "bytes_per_plane": frame_bytes},
           "warmup": a.warmup, "frames": a.frames, "repeats": a.repeats,
           "timing": "HIP event pair around each frame, median over the frames minus the empty "
                     "pair's time, per repeat; variants alternate within each repeat; the first "
                     "repeat (clock ramp-up) is listed apart and not in the medians",
           "variants": variants}
    for w in worlds.values():
        w.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
