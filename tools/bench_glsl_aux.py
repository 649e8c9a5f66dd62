"""Cost of the GLSL renderer's per-pixel planes (sfrt_glsl_draw_aux) and of its ray batches
(sfrt_glsl_cast_rays_device) against the plain draw, at 4K.

    python tools/bench_glsl_aux.py [--warmup 10] [--frames 30] [--repeats 6]
                                   [--out profiles/glsl_aux_bench.json]

3840x2160, the default uniforms at pose (0.7, 0.3), whole-frame draws on one stream in the
adaptive tile order (the renderer's default).  Seven variants, one shader each, timed alternately
in one process, `repeats` times each; every repeat warms `warmup` calls and then times `frames`
calls with a HIP event pair around each, the median minus the empty pair's own time:

* plain:             sfrt_glsl_draw -- the baseline, the same library in the same run;
* aux_depth:         sfrt_glsl_draw_aux, the depth plane only;
* aux_all:           sfrt_glsl_draw_aux, depth, sphere and steps;
* cast_tile_rgba:    the frame's own 8.29 M rays as one 8x8-tile-major batch, colour only;
* cast_tile_all:     the same batch, all five outputs;
* cast_shuffled_rgba, cast_shuffled_all: the same rays in a seeded permutation (every wave's
                     directions scattered: the wall cull keeps every wall, the march diverges).

The batch's directions are main()'s (rayShader.frag:165-175) evaluated in numpy binary32; its
sin/cos may differ from the host library's in the last place, so the batch's colours are compared
with the frame's and the fraction that is equal is recorded, not required.

The first repeat (the clock ramping up) is listed apart and left out of the medians.  No pass
threshold: the file records what the planes and the batches cost against the plain draw of the
same run, with the bytes each variant reads and writes beside its times.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sfml-software-raytracer_amd"))

WIDTH, HEIGHT, POSE = 3840, 2160, (0.7, 0.3)
PLANES = ("depth", "sphere", "steps")
ALL = ("pos", "depth", "sphere", "steps", "rgba")
OUT_BYTES = {"pos": 12, "depth": 4, "sphere": 4, "steps": 4, "rgba": 4}
# name: ("draw", planes) or ("cast", order, outputs)
VARIANTS = {
    "plain": ("draw", ()),
    "aux_depth": ("draw", ("depth",)),
    "aux_all": ("draw", PLANES),
    "cast_tile_rgba": ("cast", "tile", ("rgba",)),
    "cast_tile_all": ("cast", "tile", ALL),
    "cast_shuffled_rgba": ("cast", "shuffled", ("rgba",)),
    "cast_shuffled_all": ("cast", "shuffled", ALL),
}


def frame_dirs(u, w, h):
    """main()'s un-normalised directions (:165-175) for every fragment, row 0 = top, binary32."""
    import numpy as np
    F = np.float32

    def rot_x(a, amount):
        s, c = F(np.sin(F(amount))), F(np.cos(F(amount)))
        return np.array([a[0], F(a[1] * c) - F(a[2] * s), F(a[1] * s) + F(a[2] * c)], F)

    def rot_y(a, amount):
        s, c = F(np.sin(F(amount))), F(np.cos(F(amount)))
        return np.array([F(a[0] * c) + F(a[2] * s), a[1], F(-a[0] * s) + F(a[2] * c)], F)

    rot = [F(v) for v in u["rotation"]]
    up = rot_y(rot_x(np.array([0, 1, 0], F), -rot[1]), rot[0])
    fwd = rot_y(rot_x(np.array([0, 0, 1], F), -rot[1]), rot[0])
    right = rot_y(np.array([1, 0, 0], F), rot[0])
    fx = np.arange(w, dtype=F)[None, :] + F(0.5)
    fy = (F(h - 1) - np.arange(h, dtype=F))[:, None] + F(0.5)
    hk = F(F(u["fov"][0]) / F(u["size"][0])) * F(2)
    vk = F(F(u["fov"][1]) / F(u["size"][1])) * F(2)
    ax = (-F(u["fov"][0]) + (hk * fx).astype(F)).astype(F)
    ay = (-F(u["fov"][1]) + (vk * fy).astype(F)).astype(F)
    d = np.empty((h, w, 3), F)
    for c in range(3):
        d[..., c] = ((fwd[c] + (right[c] * ax).astype(F)).astype(F) + (up[c] * ay).astype(F)).astype(F)
    return d.reshape(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glsl_aux_bench.json"))
    a = ap.parse_args()
    if a.repeats < 2:
        raise SystemExit("bench_glsl_aux.py: --repeats must be at least 2 (the first is set apart)")

    import numpy as np
    import torch
    import glsl_scenes as gs
    import scenes
    import sfrt

    if sfrt.build_flavour() != "release":
        raise SystemExit("bench_glsl_aux.py times the release build only")
    u = gs.default_uniforms(WIDTH, HEIGHT, *POSE)
    n = WIDTH * HEIGHT
    dirs = frame_dirs(u, WIDTH, HEIGHT)
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
    planes = {p: torch.empty(HEIGHT, pitch, dtype=torch.uint8, device="cuda:0") for p in PLANES}
    floor = scenes.load_floor()
    shaders = {}
    for name in VARIANTS:
        s = sfrt.GlslShader(0)
        s.set_ground(*floor)
        s.set_uniforms(u)
        shaders[name] = s
    torch.cuda.synchronize()

    def call(name):
        v = VARIANTS[name]
        if v[0] == "cast":
            shaders[name].cast_rays_device(d_dirs[v[1]].data_ptr(), n, stream.cuda_stream,
                                           **{k: d_out[k].data_ptr() for k in v[2]})
        elif v[1]:
            shaders[name].draw_aux(colour.data_ptr(), WIDTH, HEIGHT, pitch, 0, HEIGHT, stream.cuda_stream,
                                   **{p: (planes[p].data_ptr(), pitch) for p in v[1]})
        else:
            shaders[name].draw(colour.data_ptr(), WIDTH, HEIGHT, pitch, 0, HEIGHT, stream.cuda_stream)

    # the batch is the frame, up to numpy's sin/cos against the host library's
    call("plain")
    call("cast_tile_rgba")
    shaders["cast_tile_rgba"].check(stream.cuda_stream)
    frame = colour.cpu().numpy().reshape(n, 4)
    got = d_out["rgba"].cpu().numpy().reshape(n, 4)
    equal = float(np.mean((got == frame[perms["tile"]]).all(axis=1)))
    del frame, got

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
        shaders[name].check(stream.cuda_stream)
        raw = float(np.median([x.elapsed_time(y) for x, y in ev]))
        return round(max(0.0, raw - event_gap()) * 1e3, 2)

    runs = {name: [] for name in VARIANTS}
    for _ in range(a.repeats):
        for name in VARIANTS:
            runs[name].append(timed(name))
    base = float(np.median(runs["plain"][1:]))
    variants = {}
    for name, v in VARIANTS.items():
        kept = runs[name][1:]
        med = float(np.median(kept))
        if v[0] == "cast":
            what = {"order": v[1], "outputs": list(v[2]), "bytes_read": 12 * n,
                    "bytes_written": n * sum(OUT_BYTES[k] for k in v[2])}
        else:
            what = {"planes": list(v[1]), "bytes_read": 0, "bytes_written": 4 * n * (1 + len(v[1]))}
        variants[name] = {**what, "first_repeat_us": runs[name][0], "kernel_us": kept,
                          "median_us": round(med, 2), "range_us": round(max(kept) - min(kept), 2),
                          "vs_plain_percent": round(100.0 * (med / base - 1.0), 2)}
        print(f"{name:20s} {med:9.2f} us  range {variants[name]['range_us']:7.2f}  "
              f"first {runs[name][0]:9.2f}  {variants[name]['vs_plain_percent']:+7.2f} %  "
              f"{what['bytes_written'] / 1e6:6.1f} MB written")
    out = {"command": f"python tools/bench_glsl_aux.py --warmup {a.warmup} --frames {a.frames} "
                      f"--repeats {a.repeats}",
           "device": torch.cuda.get_device_name(0),
           "frame": {"width": WIDTH, "height": HEIGHT, "scene": "glsl default uniforms",
                     "pose": list(POSE), "tile_order": "adaptive", "bytes_per_plane": 4 * n},
           "batch": {"rays": n, "source": "the frame's own directions (main() in numpy binary32)",
                     "rgba_equal_to_frame_fraction": equal},
           "warmup": a.warmup, "frames": a.frames, "repeats": a.repeats,
           "timing": "HIP event pair around each call, median over the calls minus the empty "
                     "pair's time, per repeat; variants alternate within each repeat; the first "
                     "repeat (clock ramp-up) is listed apart and not in the medians",
           "variants": variants}
    for s in shaders.values():
        s.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
