"""Cost of the frame fill's per-pixel planes (sfrt_world_render_band_aux) at 4K.

    python tools/bench_aux.py [--warmup 20] [--frames 40] [--repeats 5] [--rays 0]
                              [--out profiles/aux_planes_bench.json]

3840x2160, lcg64, pose (0, 0), whole-frame bands in the adaptive tile order on one stream.
Four variants, one world each (so each keeps its own tile-order chain and ray cache), timed
alternately in one process, `repeats` times each; every repeat warms `warmup` frames (the order
is live from the third) and then times `frames` frames with a HIP event pair around each, the
median minus the empty pair's own time:

* plain_nocache: sfrt_world_render_band with SFRT_OPT_RAY_CACHE_MB 0 -- the like-for-like
  baseline, since the aux kernels compute their ray directions;
* plain_cached:  sfrt_world_render_band with the ray cache on (the default);
* aux_depth:     sfrt_world_render_band_aux, the depth plane only;
* aux_all:       sfrt_world_render_band_aux, depth, sphere and steps.

--rays R forces R pixels per lane (SFRT_OPT_RAYS_PER_LANE) on every variant; 0, the default,
leaves the kernel table's choice (R = 4 for this frame).

No pass threshold: the file records what the planes cost.  Each variant's bytes written per
frame are listed beside its times (4 bytes per pixel for the colour and for each plane).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sfml-software-raytracer_amd"))

WIDTH, HEIGHT, SCENE, POSE = 3840, 2160, "lcg64", (0.0, 0.0)
VARIANTS = {"plain_nocache": (), "plain_cached": (), "aux_depth": ("depth",),
            "aux_all": ("depth", "sphere", "steps")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rays", type=int, default=0, help="SFRT_OPT_RAYS_PER_LANE of every variant")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_planes_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import scenes
    import sfrt

    if sfrt.build_flavour() != "release":
        raise SystemExit("bench_aux.py times the release build only")
    stream = torch.cuda.Stream()
    pitch = 4 * WIDTH
    colour = torch.empty(HEIGHT, pitch, dtype=torch.uint8, device="cuda")
    planes = {p: torch.empty(HEIGHT, pitch, dtype=torch.uint8, device="cuda")
              for p in ("depth", "sphere", "steps")}
    floor = scenes.load_floor()
    worlds = {}
    for name in VARIANTS:
        w = sfrt.World(0)
        w.load_texture(*floor)
        w.set_scene(scenes.SCENES[SCENE]().posed(*POSE), WIDTH, HEIGHT)
        w.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, a.rays)
        if name == "plain_nocache":
            w.set_option(sfrt.SFRT_OPT_RAY_CACHE_MB, 0)
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
    base = float(np.median(runs["plain_nocache"]))
    variants = {}
    for name, want in VARIANTS.items():
        med = float(np.median(runs[name]))
        variants[name] = {"planes": list(want), "bytes_written": frame_bytes * (1 + len(want)),
                          "kernel_us": runs[name], "median_us": round(med, 2),
                          "range_us": round(max(runs[name]) - min(runs[name]), 2),
                          "vs_plain_nocache_percent": round(100.0 * (med / base - 1.0), 2)}
        print(f"{name:14s} {med:9.2f} us  range {variants[name]['range_us']:6.2f}  "
              f"{variants[name]['vs_plain_nocache_percent']:+6.2f} %  "
              f"{variants[name]['bytes_written'] / 1e6:6.1f} MB written")
    stats = worlds["plain_cached"].ray_cache_stats()
    out = {"command": f"python tools/bench_aux.py --warmup {a.warmup} --frames {a.frames} "
                      f"--repeats {a.repeats} --rays {a.rays}",
           "device": torch.cuda.get_device_name(0),
           "frame": {"width": WIDTH, "height": HEIGHT, "scene": SCENE, "pose": list(POSE),
                     "tile_order": "adaptive", "rays_per_lane": a.rays or "table (4)",
                     "bytes_per_plane": frame_bytes},
           "warmup": a.warmup, "frames": a.frames, "repeats": a.repeats,
           "timing": "HIP event pair around each frame, median over the frames minus the empty "
                     "pair's time, per repeat; variants alternate within each repeat",
           "plain_cached_ray_cache": stats,
           "aux_worlds_ray_cache": {n: worlds[n].ray_cache_stats() for n in ("aux_depth", "aux_all")},
           "variants": variants}
    for w in worlds.values():
        w.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
