"""Cost of a ray batch (sfrt_world_cast_rays_device) against the frame kernel on the same rays.

    python tools/bench_raycast.py [--warmup 5] [--frames 20] [--repeats 3]
                                  [--out profiles/raycast_bench.json]

The batch is the 3840x2160 lcg64 pose (0, 0) frame's own 8.29 M primary directions
(tests/raycast_ref.py pixel_dirs, the un-normalised r->dir of SphereWorld.cpp:106), from the
camera position (origins = NULL), in two orders:

* tile:     8x8-tile-major, so every wave holds one 8x8 pixel tile (coherent cones);
* shuffled: a seeded permutation (every wave is wide: no sphere is culled).

Each order is timed with rgba only and with all five outputs; the tile order also with
SFRT_OPT_CULL 0.  The yardstick is the frame kernel on the same rays: sfrt_world_render_band with
SFRT_OPT_RAYS_PER_LANE 1 and SFRT_OPT_RAY_CACHE_MB 0 (one ray per lane, directions computed),
with SFRT_OPT_CULL 1 and 0.  Before timing, the tile-order batch's rgba is checked against that
frame, byte for byte.

Method (as tools/bench_aux.py): every variant has its own world; the variants alternate in one
process, `repeats` times each; every repeat discards `warmup` calls and then times `frames` calls
with a HIP event pair around each, the median minus the empty pair's own time.  No pass
threshold: the file records what was measured, with the bytes each variant reads and writes per
ray beside its time.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sfml-software-raytracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WIDTH, HEIGHT, SCENE, POSE = 3840, 2160, "lcg64", (0.0, 0.0)
ALL = ("pos", "depth", "sphere", "steps", "rgba")
OUT_BYTES = {"pos": 12, "depth": 4, "sphere": 4, "steps": 4, "rgba": 4}
# name: (order or None for the frame kernel, outputs, SFRT_OPT_CULL)
VARIANTS = {
    "frame_r1_cull1": (None, ("rgba",), 1),
    "frame_r1_cull0": (None, ("rgba",), 0),
    "cast_tile_rgba": ("tile", ("rgba",), 1),
    "cast_tile_all": ("tile", ALL, 1),
    "cast_tile_rgba_cull0": ("tile", ("rgba",), 0),
    "cast_shuffled_rgba": ("shuffled", ("rgba",), 1),
    "cast_shuffled_all": ("shuffled", ALL, 1),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import raycast_ref
    import scenes
    import sfrt

    if sfrt.build_flavour() != "release":
        raise SystemExit("bench_raycast.py times the release build only")
    scene = scenes.SCENES[SCENE]().posed(*POSE)
    n = WIDTH * HEIGHT
    dirs = raycast_ref.pixel_dirs(scene, WIDTH, HEIGHT).reshape(n, 3)
    jj, ii = np.meshgrid(np.arange(HEIGHT), np.arange(WIDTH), indexing="ij")
    tile = ((jj // 8) * (WIDTH // 8) + ii // 8) * 64 + (jj % 8) * 8 + ii % 8
    perms = {"tile": np.argsort(tile.reshape(-1), kind="stable"),
             "shuffled": np.random.default_rng(7).permutation(n)}
    del jj, ii, tile
    stream = torch.cuda.Stream()
    d_dirs = {k: torch.from_numpy(np.ascontiguousarray(dirs[p])).to("cuda:0") for k, p in perms.items()}
    d_out = {k: torch.empty(n * OUT_BYTES[k], dtype=torch.uint8, device="cuda:0") for k in ALL}
    pitch = 4 * WIDTH
    colour = torch.empty(HEIGHT, pitch, dtype=torch.uint8, device="cuda:0")
    floor = scenes.load_floor()
    worlds = {}
    for name, (order, _, cull) in VARIANTS.items():
        w = sfrt.World(0)
        w.load_texture(*floor)
        w.set_scene(scene, WIDTH, HEIGHT)
        w.set_option(sfrt.SFRT_OPT_CULL, cull)
        if order is None:
            w.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, 1)
            w.set_option(sfrt.SFRT_OPT_RAY_CACHE_MB, 0)
        worlds[name] = w
    torch.cuda.synchronize()

    def call(name):
        order, outputs, _ = VARIANTS[name]
        if order is None:
            worlds[name].render_band(colour.data_ptr(), pitch, 0, HEIGHT, stream.cuda_stream)
        else:
            worlds[name].cast_rays_device(d_dirs[order].data_ptr(), None, n, stream.cuda_stream,
                                          **{k: d_out[k].data_ptr() for k in outputs})

    # the batch is the frame: same bytes
    call("frame_r1_cull1")
    call("cast_tile_rgba")
    worlds["cast_tile_rgba"].check(stream.cuda_stream)
    frame = colour.cpu().numpy().reshape(n, 4)
    got = d_out["rgba"].cpu().numpy().reshape(n, 4)
    if not np.array_equal(got, frame[perms["tile"]]):
        raise SystemExit("bench_raycast.py: the batch's rgba differs from the frame")

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
            call(name)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(a.frames)]
        for x, y in ev:
            x.record(stream)
            call(name)
            y.record(stream)
        torch.cuda.synchronize()
        worlds[name].check(stream.cuda_stream)
        raw = float(np.median([x.elapsed_time(y) for x, y in ev]))
        return round(max(0.0, raw - event_gap()) * 1e3, 2)

    runs = {name: [] for name in VARIANTS}
    for _ in range(a.repeats):
        for name in VARIANTS:
            runs[name].append(timed(name))
    base = float(np.median(runs["frame_r1_cull1"]))
    variants = {}
    for name, (order, outputs, cull) in VARIANTS.items():
        med = float(np.median(runs[name]))
        variants[name] = {"order": order or "frame kernel, 8x8 tiles, adaptive tile order",
                          "outputs": list(outputs), "cull": cull,
                          "bytes_read_per_ray": 0 if order is None else 12,
                          "bytes_written_per_ray": sum(OUT_BYTES[k] for k in outputs),
                          "kernel_us": runs[name], "median_us": round(med, 2),
                          "range_us": round(max(runs[name]) - min(runs[name]), 2),
                          "vs_frame_r1_cull1_percent": round(100.0 * (med / base - 1.0), 2)}
        print(f"{name:22s} {med:10.2f} us  range {variants[name]['range_us']:8.2f}  "
              f"{variants[name]['vs_frame_r1_cull1_percent']:+8.2f} %")
    out = {"command": f"python tools/bench_raycast.py --warmup {a.warmup} --frames {a.frames} "
                      f"--repeats {a.repeats}",
           "device": torch.cuda.get_device_name(0),
           "batch": {"rays": n, "source": f"{WIDTH}x{HEIGHT} {SCENE} pose {list(POSE)} primary "
                                          "directions, origins NULL"},
           "warmup": a.warmup, "frames": a.frames, "repeats": a.repeats,
           "timing": "HIP event pair around each call, median over the calls minus the empty "
                     "pair's time, per repeat; variants alternate within each repeat",
           "variants": variants}
    for w in worlds.values():
        w.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
