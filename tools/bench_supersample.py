"""Cost of in-kernel supersampling (SFRT_OPT_SUPERSAMPLE) against the plain large frame.

    python tools/bench_supersample.py [--renderer sphere|voxel|glsl] [--warmup 50] [--frames 200]
                                      [--repeats 5] [--out profiles/supersample_bench.json]

Frames: lcg64 pose (0, 0) at 1920x1080 S=2, 1920x1080 S=4 and 3840x2160 S=2.  For each, in
one process, the supersampled W x H frame and the plain (S = 1) S*W x S*H frame -- the same
rays, a path this option does not change -- are timed alternately, `repeats` times each:

* kernel: render_band frames back to back on one stream (adaptive tile order), HIP events
  around every EVENT_EVERY-th frame, the empty event pair's own time subtracted (as
  bench.py times its headline); also the wall time per frame of the same loop;
* to host: submit_frame / wait_frame into pinned memory, two frames in flight, wall time
  per frame.

Expectation (stated before measuring): the supersampled kernel takes no longer than the
plain large frame's, within that plain frame's own run-to-run spread (max - min over the
repeats); the to-host time approaches 1 / S^2 of the plain large frame's.  The JSON holds
every repeat, the medians, the verdicts and the command line.  One supersampled frame per
case is also compared, on the device, with the box filter of the plain frame.

--renderer voxel / glsl (output profiles/supersample_voxel_bench.json / _glsl_bench.json): the
same three cases and the same alternation -- on one renderer object, its size and factor
switched between the two frames, so that both read the same allocations -- for
sfrt_voxel_render_band (default world, camera
defaults, row-major: the voxel default) and sfrt_glsl_draw (default uniforms, pose 0.7 / 0.3,
adaptive order: the GLSL default); to host is update_image / draw_image, synchronous, into
pageable memory, --host-frames (default 20) frames per repeat.  Their kernel expectation adds
the epilogue's share of the instruction stream: EPILOGUE_VALU over the per-ray VALU count of
profiles/r6j_voxel_traffic.json / r6j_glsl_traffic.json (SQ_INSTS_VALU per wave at 4K).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sfml-software-raytracer_amd"))

CASES = [(1920, 1080, 2), (1920, 1080, 4), (3840, 2160, 2)]
EVENT_EVERY = 8
# The filter epilogue's instructions, read off the new kernels' ISA against their S = 1 kernels
# (tools/isa_compare.py on the `make isa` listings: 24 / 23 more VALU and two swizzles at S = 4).
EPILOGUE_VALU = {"voxel": 26, "glsl": 25}
TRAFFIC = {"voxel": "r6j_voxel_traffic.json", "glsl": "r6j_glsl_traffic.json"}
DEFAULT_OUT = {"sphere": "supersample_bench.json", "voxel": "supersample_voxel_bench.json",
               "glsl": "supersample_glsl_bench.json"}


def epilogue_share(renderer):
    """EPILOGUE_VALU over the VALU instructions per ray (= per wave) of the 4K frame."""
    with open(os.path.join(ROOT, "profiles", TRAFFIC[renderer])) as f:
        per = json.load(f)["per_launch_pixels"]["8294400"]
    return EPILOGUE_VALU[renderer] / (per["SQ_INSTS_VALU"] / (8294400 / 64))


def bench_renderer(a):
    """--renderer voxel / glsl: see the module docstring."""
    import numpy as np
    import torch
    import sfrt

    stream = torch.cuda.Stream()
    share = epilogue_share(a.renderer)

    def event_gap():
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                 for _ in range(64)]
        for x, y in pairs:
            x.record(stream)
            y.record(stream)
        torch.cuda.synchronize()
        return float(np.median([x.elapsed_time(y) for x, y in pairs]))

    if a.renderer == "voxel":
        import voxel_scenes as vs
        tex, dyn = vs.load_textures()
        scene_name = "default world, camera defaults"

        def make():
            r = sfrt.VoxelWorld(0)
            r.load_assets(tex, dyn, vs.COLORS)
            return r

        def configure(r, width, height, s):
            r.set_scene(vs.default_world(), width, height)
            r.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)

        def fill(r, buf, width, height):
            r.render_band(buf.data_ptr(), width * 4, 0, height, stream.cuda_stream)

        def to_host(r, pixels, width, height):
            rc = sfrt.lib().sfrt_voxel_update_image(r._h, pixels.ctypes.data, 0, 1, 0, 1)
            assert rc == 0, rc
    else:
        import glsl_scenes as gs
        import scenes
        floor = scenes.load_floor()
        scene_name = "default uniforms, pose (0.7, 0.3)"

        def make():
            r = sfrt.GlslShader(0)
            r.set_ground(*floor)
            return r

        def configure(r, width, height, s):
            r.set_uniforms(gs.default_uniforms(width, height, 0.7, 0.3))
            r.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)

        def fill(r, buf, width, height):
            r.draw(buf.data_ptr(), width, height, width * 4, 0, height, stream.cuda_stream)

        def to_host(r, pixels, width, height):
            rc = sfrt.lib().sfrt_glsl_draw_image(r._h, pixels.ctypes.data, width, height)
            assert rc == 0, rc

    def kernel_time(r, buf, width, height):
        for _ in range(a.warmup):
            fill(r, buf, width, height)
        torch.cuda.synchronize()
        ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for k in range(0, a.frames, EVENT_EVERY)}
        t0 = time.perf_counter()
        for k in range(a.frames):
            if k in ev:
                ev[k][0].record(stream)
            fill(r, buf, width, height)
            if k in ev:
                ev[k][1].record(stream)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / a.frames
        r.check(stream.cuda_stream)
        raw = sum(x.elapsed_time(y) for x, y in ev.values()) / len(ev)
        return max(0.0, raw - event_gap()) * 1e3, wall * 1e6

    def host_time(r, pixels, width, height):
        to_host(r, pixels, width, height)  # warm: the device frame and the tables
        t0 = time.perf_counter()
        for _ in range(a.host_frames):
            to_host(r, pixels, width, height)
        return (time.perf_counter() - t0) / a.host_frames * 1e6

    out = {"command": "python " + " ".join([os.path.relpath(os.path.abspath(sys.argv[0]), ROOT)] +
                                            sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "build_flavour": sfrt.build_flavour(),
           "renderer": a.renderer, "scene": scene_name, "warmup": a.warmup, "frames": a.frames,
           "host_frames": a.host_frames, "repeats": a.repeats, "event_every": EVENT_EVERY,
           "first": a.first,
           "epilogue_valu": EPILOGUE_VALU[a.renderer], "epilogue_share": round(share, 5),
           "cases": []}
    cases = CASES if not a.cases else [tuple(int(v) for v in c.split("x")) for c in a.cases.split(",")]
    for width, height, s in cases:
        bw, bh = s * width, s * height
        # one object for both frames (the factor and the size switched between them): the same
        # grid, textures and tables under both -- two objects' allocations alone moved the 4K voxel
        # frame between 170 and 181 us from one process to the next
        r = make()
        small = torch.empty(height, width * 4, dtype=torch.uint8, device="cuda")
        big = torch.empty(bh, bw * 4, dtype=torch.uint8, device="cuda")
        rec = {"width": width, "height": height, "factor": s, "plain_width": bw, "plain_height": bh,
               "supersampled": {"kernel_us": [], "wall_us": [], "to_host_us": []},
               "plain_large": {"kernel_us": [], "wall_us": [], "to_host_us": []}}
        for _ in range(a.repeats):  # alternately, so that drift hits both alike
            pair = [("plain_large", big, bw, bh, 1), ("supersampled", small, width, height, s)]
            for key, buf, fw, fh, f in (pair if a.first == "plain" else pair[::-1]):
                configure(r, fw, fh, f)
                k_us, wall_us = kernel_time(r, buf, fw, fh)
                rec[key]["kernel_us"].append(round(k_us, 2))
                rec[key]["wall_us"].append(round(wall_us, 2))
        torch.cuda.synchronize()
        sums = big.view(height, s, width, s, 4).to(torch.int32).sum(dim=(1, 3))
        want = ((sums + s * s // 2) >> (2 if s == 2 else 4)).to(torch.uint8)
        rec["bytes_equal_filtered_plain"] = bool(torch.equal(want, small.view(height, width, 4)))
        del sums, want, big, small
        host_small = np.empty(width * height * 4, np.uint8)
        host_big = np.empty(bw * bh * 4, np.uint8)
        for _ in range(a.repeats):
            configure(r, bw, bh, 1)
            rec["plain_large"]["to_host_us"].append(round(host_time(r, host_big, bw, bh), 2))
            configure(r, width, height, s)
            rec["supersampled"]["to_host_us"].append(round(host_time(r, host_small, width, height), 2))
        r.close()
        p, q = rec["plain_large"], rec["supersampled"]
        for d in (p, q):
            for name in ("kernel_us", "wall_us", "to_host_us"):
                d[name + "_median"] = round(float(np.median(d[name])), 2)
        spread = max(p["kernel_us"]) - min(p["kernel_us"])
        bound = p["kernel_us_median"] * (1.0 + share) + spread
        rec["plain_kernel_spread_us"] = round(spread, 2)
        rec["kernel_bound_us"] = round(bound, 2)
        rec["kernel_ratio"] = round(q["kernel_us_median"] / p["kernel_us_median"], 4)
        rec["kernel_within_expectation"] = bool(q["kernel_us_median"] <= bound)
        rec["to_host_ratio"] = round(q["to_host_us_median"] / p["to_host_us_median"], 4)
        rec["to_host_ideal_ratio"] = round(1.0 / (s * s), 4)
        out["cases"].append(rec)
        print(f"{a.renderer} {width}x{height} S={s}: kernel {q['kernel_us_median']:.1f} us vs plain "
              f"{bw}x{bh} {p['kernel_us_median']:.1f} us (spread {spread:.1f}, bound {bound:.1f}); "
              f"to host {q['to_host_us_median']:.1f} vs {p['to_host_us_median']:.1f} us; "
              f"bytes {'ok' if rec['bytes_equal_filtered_plain'] else 'DIFFER'}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote " + a.out)
    if not all(c["bytes_equal_filtered_plain"] for c in out["cases"]):
        raise SystemExit("a supersampled frame differs from the filtered plain frame")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--renderer", choices=["sphere", "voxel", "glsl"], default="sphere")
    ap.add_argument("--host-frames", type=int, default=20,
                    help="voxel / glsl: update_image / draw_image frames per repeat")
    ap.add_argument("--cases", default="", help="voxel / glsl: WxHxS,... instead of the three cases")
    ap.add_argument("--first", choices=["plain", "supersampled"], default="plain",
                    help="voxel / glsl: which of the two frames each repeat times first")
    ap.add_argument("--out", default=None, help="default: profiles/supersample_bench.json, "
                    "supersample_voxel_bench.json or supersample_glsl_bench.json by renderer")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", DEFAULT_OUT[a.renderer])
    if a.warmup < 50 or a.frames < 200 or a.repeats < 5:
        raise SystemExit("at least 50 warm-up frames, 200 timed frames and 5 repeats")
    if a.renderer != "sphere":
        if a.host_frames < 10:
            raise SystemExit("at least 10 to-host frames per repeat")
        return bench_renderer(a)

    import numpy as np
    import torch
    import scenes
    import sfrt

    stream = torch.cuda.Stream()
    floor = scenes.load_floor()
    scene = scenes.lcg64().posed(0.0, 0.0)

    def event_gap():
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                 for _ in range(64)]
        for x, y in pairs:
            x.record(stream)
            y.record(stream)
        torch.cuda.synchronize()
        return float(np.median([x.elapsed_time(y) for x, y in pairs]))

    def world(width, height, s):
        w = sfrt.World(0)
        w.load_texture(*floor)
        w.set_scene(scene, width, height)
        w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
        return w

    def kernel_time(w, buf, width, height):
        """(kernel us per frame from events, wall us per frame) of one repeat."""
        for _ in range(a.warmup):
            w.render_band(buf.data_ptr(), width * 4, 0, height, stream.cuda_stream)
        torch.cuda.synchronize()
        sampled = [k for k in range(a.frames) if k % EVENT_EVERY == 0]
        ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for k in sampled}
        t0 = time.perf_counter()
        for k in range(a.frames):
            if k in ev:
                ev[k][0].record(stream)
            w.render_band(buf.data_ptr(), width * 4, 0, height, stream.cuda_stream)
            if k in ev:
                ev[k][1].record(stream)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / a.frames
        w.check(stream.cuda_stream)
        raw = sum(x.elapsed_time(y) for x, y in ev.values()) / len(ev)
        return max(0.0, raw - event_gap()) * 1e3, wall * 1e6

    def host_time(w, frames):
        """Wall us per frame of submit_frame / wait_frame with two frames in flight."""
        tickets = [w.submit_frame(frames[k % 2]) for k in range(2)]  # warm both slots
        for t in tickets:
            w.wait_frame(t)
        t0 = time.perf_counter()
        prev = None
        for k in range(a.frames):
            t = w.submit_frame(frames[k % 2])
            if prev is not None:
                w.wait_frame(prev)
            prev = t
        w.wait_frame(prev)
        return (time.perf_counter() - t0) / a.frames * 1e6

    def med(v):
        return float(np.median(v))

    out = {"command": "python " + " ".join([os.path.relpath(os.path.abspath(sys.argv[0]), ROOT)] +
                                            sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "build_flavour": sfrt.build_flavour(),
           "scene": "lcg64 pose (0, 0)", "warmup": a.warmup, "frames": a.frames,
           "repeats": a.repeats, "event_every": EVENT_EVERY, "cases": []}
    for width, height, s in CASES:
        bw, bh = s * width, s * height
        ws, wp = world(width, height, s), world(bw, bh, 1)
        small = torch.empty(height, width * 4, dtype=torch.uint8, device="cuda")
        big = torch.empty(bh, bw * 4, dtype=torch.uint8, device="cuda")
        rec = {"width": width, "height": height, "factor": s, "plain_width": bw, "plain_height": bh,
               "supersampled": {"kernel_us": [], "wall_us": [], "to_host_us": []},
               "plain_large": {"kernel_us": [], "wall_us": [], "to_host_us": []}}
        for _ in range(a.repeats):  # alternately, so that drift hits both alike
            for key, w, buf, fw, fh in (("plain_large", wp, big, bw, bh),
                                        ("supersampled", ws, small, width, height)):
                k_us, wall_us = kernel_time(w, buf, fw, fh)
                rec[key]["kernel_us"].append(round(k_us, 2))
                rec[key]["wall_us"].append(round(wall_us, 2))
        # bytes: the supersampled frame is the box filter of the plain one
        torch.cuda.synchronize()
        sums = big.view(height, s, width, s, 4).to(torch.int32).sum(dim=(1, 3))
        want = ((sums + s * s // 2) >> (2 if s == 2 else 4)).to(torch.uint8)
        rec["bytes_equal_filtered_plain"] = bool(torch.equal(want, small.view(height, width, 4)))
        host_small = [sfrt.HostFrame(width * height * 4) for _ in range(2)]
        host_big = [sfrt.HostFrame(bw * bh * 4) for _ in range(2)]
        for _ in range(a.repeats):
            rec["plain_large"]["to_host_us"].append(round(host_time(wp, host_big), 2))
            rec["supersampled"]["to_host_us"].append(round(host_time(ws, host_small), 2))
        for f in host_small + host_big:
            f.free()
        ws.close()
        wp.close()
        p, q = rec["plain_large"], rec["supersampled"]
        for d in (p, q):
            for name in ("kernel_us", "wall_us", "to_host_us"):
                d[name + "_median"] = round(med(d[name]), 2)
        spread = max(p["kernel_us"]) - min(p["kernel_us"])
        rec["plain_kernel_spread_us"] = round(spread, 2)
        rec["kernel_ratio"] = round(q["kernel_us_median"] / p["kernel_us_median"], 4)
        rec["kernel_within_expectation"] = bool(q["kernel_us_median"] <= p["kernel_us_median"] + spread)
        rec["to_host_ratio"] = round(q["to_host_us_median"] / p["to_host_us_median"], 4)
        rec["to_host_ideal_ratio"] = round(1.0 / (s * s), 4)
        out["cases"].append(rec)
        print(f"{width}x{height} S={s}: kernel {q['kernel_us_median']:.1f} us vs plain {bw}x{bh} "
              f"{p['kernel_us_median']:.1f} us (spread {spread:.1f}); to host "
              f"{q['to_host_us_median']:.1f} vs {p['to_host_us_median']:.1f} us; "
              f"bytes {'ok' if rec['bytes_equal_filtered_plain'] else 'DIFFER'}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote " + a.out)
    if not all(c["bytes_equal_filtered_plain"] for c in out["cases"]):
        raise SystemExit("a supersampled frame differs from the filtered plain frame")


if __name__ == "__main__":
    main()
