"""Cost of the voxel world's ray batches (sfrt_voxel_cast_rays_device,
sfrt_voxel_cast_shadow_rays_device) against the frame kernel, at 4K.

    python tools/bench_voxel_rays.py [--warmup 5] [--frames 20] [--repeats 5]
                                     [--out profiles/voxel_rays_bench.json]

The rays are the 3840x2160 default-world frame's 8.29 M primary rays (bench.py's
"voxel_3840x2160" frame: World.cpp:64-87 at the default pose), handed to the batch call as
directions and yscales in 8x8-tile-major order -- the order in which the frame kernel's waves
take them -- and once more shuffled.  Variants, one world each, timed alternately in one process,
`repeats` times each; every repeat warms `warmup` launches and then times `frames` launches with a
HIP event pair around each, the median minus the empty pair's own time:

* frame_aux:      sfrt_voxel_render_band_aux, colour and all four planes -- the baseline, the same
                  library in the same run (times of other runs are not comparable);
* rays_rgba:      the batch, colour only;
* rays_planes:    the batch, the frame call's own outputs (depth, cell, face, steps, rgba): what
                  it costs to take the rays from memory instead of the frame tables;
* rays_all:       the batch, all six outputs (pos, depth, cell, face, steps, rgba);
* rays_pick:      the batch, rgba = NULL (no shading): pos, depth, cell, face, steps;
* rays_all_shuffled / rays_pick_shuffled: the same rays in a random order;
* shadow:         sfrt_voxel_cast_shadow_rays_device, 8.29 M random segments through the default
                  world (both outputs), reported in segments per second as well.

The first repeat (the clock ramping up) is listed apart and left out of the medians.  No pass
threshold: the file records what the batches cost and their ratios to the frame kernel.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sfml-software-raytracer_amd"))

WIDTH, HEIGHT = 3840, 2160
POSE = ((15.5, 1.9, 15.5), 0.0, 0.0)
PLANES = ("depth", "cell", "face", "steps")
RAY_VARIANTS = {  # name: (outputs, shuffled)
    "rays_rgba": (("rgba",), False),
    "rays_planes": (("depth", "cell", "face", "steps", "rgba"), False),
    "rays_all": (("pos", "depth", "cell", "face", "steps", "rgba"), False),
    "rays_pick": (("pos", "depth", "cell", "face", "steps"), False),
    "rays_all_shuffled": (("pos", "depth", "cell", "face", "steps", "rgba"), True),
    "rays_pick_shuffled": (("pos", "depth", "cell", "face", "steps"), True),
}
ELEM = {"pos": 12, "depth": 4, "cell": 4, "face": 4, "steps": 4, "rgba": 4}


def frame_rays(scene, width, height):
    """World.cpp:64-87 in binary32 with the host libm: (dirs (n, 3), yscales (n,)), row-major."""
    import numpy as np
    import voxel_scenes as vs
    F = np.float32
    fov_h, fov_v, rot, hrot = F(scene.fov_h), F(scene.fov_v), F(scene.rotation), F(scene.hrotation)
    v_start, v_inc, v_off = fov_v / F(2), fov_v / F(height), vs.sinf(hrot)
    h_start, h_inc = rot - fov_h / F(2), fov_h / F(width)
    dx, dz = np.zeros(width, F), np.zeros(width, F)
    for i in range(width):
        hray = F(h_start + F(h_inc * F(i)))
        fix = vs.cosf(F(rot - hray))
        dx[i], dz[i] = F(vs.sinf(hray) / fix), F(vs.cosf(hray) / fix)
    dy, ys = np.zeros(height, F), np.zeros(height, F)
    for j in range(height):
        vray = F(v_start - F(F(j) * v_inc))
        dy[j], ys[j] = F(v_off + vs.sinf(vray)), vs.cosf(F(hrot + vray))
    col, row = np.tile(np.arange(width), height), np.repeat(np.arange(height), width)
    return np.stack([dx[col], dy[row], dz[col]], axis=1), ys[row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_rays_bench.json"))
    a = ap.parse_args()
    if a.repeats < 2:
        raise SystemExit("bench_voxel_rays.py: --repeats must be at least 2 (the first is set apart)")

    import numpy as np
    import torch
    import sfrt
    import voxel_scenes as vs

    if sfrt.build_flavour() != "release":
        raise SystemExit("bench_voxel_rays.py times the release build only")
    F = np.float32
    n = WIDTH * HEIGHT
    stream = torch.cuda.Stream()
    tex, dyn = vs.load_textures()
    scene = vs.default_world(*POSE)
    dirs, ys = frame_rays(scene, WIDTH, HEIGHT)
    jj, ii = np.divmod(np.arange(n), WIDTH)
    tile = np.lexsort((ii % 8, jj % 8, ii // 8, jj // 8))
    rng = np.random.default_rng(1)
    orders = {False: tile, True: rng.permutation(n)}
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    d_dirs = {k: dev(dirs[o]) for k, o in orders.items()}
    d_ys = {k: dev(ys[o]) for k, o in orders.items()}
    # shadow segments: starts in the rooms, ends up to ~40 away, normalised directions
    so = rng.uniform([1.2, 1.2, 1.2], [98.8, 8.8, 98.8], (n, 3)).astype(F)
    e = (rng.standard_normal((n, 3)) * rng.uniform(0.5, 14.0, (n, 1))).astype(F)
    ln = np.sqrt((e * e).sum(axis=1, dtype=F)).astype(F)
    d_so, d_sd, d_md = dev(so), dev((e / ln[:, None]).astype(F)), dev(np.minimum(ln, F(64.0)))
    out = {k: torch.empty(n * b, dtype=torch.uint8, device="cuda") for k, b in ELEM.items()}
    pitch = 4 * WIDTH
    colour = torch.empty(HEIGHT, pitch, dtype=torch.uint8, device="cuda")
    planes = {p: torch.empty(HEIGHT, pitch, dtype=torch.uint8, device="cuda") for p in PLANES}
    torch.cuda.synchronize()

    names = ["frame_aux"] + list(RAY_VARIANTS) + ["shadow"]
    worlds = {}
    for name in names:
        w = sfrt.VoxelWorld(0)
        w.load_assets(tex, dyn, vs.COLORS)
        w.set_scene(scene, WIDTH, HEIGHT)
        worlds[name] = w

    def launch(name):
        w = worlds[name]
        if name == "frame_aux":
            w.render_band_aux(colour.data_ptr(), pitch, 0, HEIGHT, stream.cuda_stream,
                              **{p: (planes[p].data_ptr(), pitch) for p in PLANES})
        elif name == "shadow":
            w.cast_shadow_rays_device(d_so.data_ptr(), d_sd.data_ptr(), d_md.data_ptr(), n,
                                      stream.cuda_stream, free=out["cell"].data_ptr(),
                                      steps=out["steps"].data_ptr())
        else:
            want, shuffled = RAY_VARIANTS[name]
            w.cast_rays_device(d_dirs[shuffled].data_ptr(), d_ys[shuffled].data_ptr(), 0, n,
                               stream.cuda_stream, **{k: out[k].data_ptr() for k in want})

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
            launch(name)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(a.frames)]
        for x, y in ev:
            x.record(stream)
            launch(name)
            y.record(stream)
        torch.cuda.synchronize()
        worlds[name].check(stream.cuda_stream)
        raw = float(np.median([x.elapsed_time(y) for x, y in ev]))
        return round(max(0.0, raw - event_gap()) * 1e3, 2)

    # the batch computes what the frame computes: colour and planes, pixel for pixel
    launch("frame_aux")
    launch("rays_all")
    torch.cuda.synchronize()
    frame_rgba = colour.cpu().numpy().reshape(n, 4)[tile]
    same = bool(np.array_equal(frame_rgba, out["rgba"].cpu().numpy().reshape(n, 4)))
    for p in PLANES:
        same &= bool(np.array_equal(planes[p].cpu().numpy().reshape(n, 4)[tile],
                                    out[p].cpu().numpy().reshape(n, 4)))
    if not same:
        raise SystemExit("bench_voxel_rays.py: the batch's outputs differ from the frame's")

    runs = {name: [] for name in names}
    for _ in range(a.repeats):
        for name in names:
            runs[name].append(timed(name))
    base = float(np.median(runs["frame_aux"][1:]))
    variants = {}
    for name in names:
        kept = runs[name][1:]
        med = float(np.median(kept))
        v = {"first_repeat_us": runs[name][0], "kernel_us": kept, "median_us": round(med, 2),
             "range_us": round(max(kept) - min(kept), 2)}
        if name == "shadow":
            v["segments_per_second"] = round(n / (med * 1e-6), 0)
            v["outputs"] = ["free", "steps"]
        else:
            v["ratio_to_frame_aux"] = round(med / base, 4)
            if name != "frame_aux":
                v["outputs"], v["order"] = list(RAY_VARIANTS[name][0]), \
                    "shuffled" if RAY_VARIANTS[name][1] else "8x8-tile-major"
                v["rays_per_second"] = round(n / (med * 1e-6), 0)
        variants[name] = v
        print(f"{name:20s} {med:9.2f} us  range {v['range_us']:6.2f}  first {runs[name][0]:9.2f}  "
              + (f"x{v['ratio_to_frame_aux']:.3f} of frame_aux" if "ratio_to_frame_aux" in v
                 else f"{v['segments_per_second'] / 1e9:.2f} G segments/s"))
    res = {"command": f"python tools/bench_voxel_rays.py --warmup {a.warmup} --frames {a.frames} "
                      f"--repeats {a.repeats}",
           "device": torch.cuda.get_device_name(0),
           "rays": {"count": n, "source": f"the {WIDTH}x{HEIGHT} frame of the voxel default world",
                    "pose": [list(POSE[0]), POSE[1], POSE[2]], "tile_order": "off"},
           "batch_equals_frame": same,
           "warmup": a.warmup, "frames": a.frames, "repeats": a.repeats,
           "timing": "HIP event pair around each launch, median over the launches minus the empty "
                     "pair's time, per repeat; variants alternate within each repeat; the first "
                     "repeat (clock ramp-up) is listed apart and not in the medians",
           "variants": variants}
    for w in worlds.values():
        w.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
