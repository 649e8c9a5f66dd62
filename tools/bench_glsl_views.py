"""Cost of a batch of camera views of the GLSL renderer in one launch (sfrt_glsl_render_views)
against the loops it replaces: set_uniform x 3 + draw per view.

    python tools/bench_glsl_views.py [--warmup 10] [--frames 30] [--repeats 5]
                                     [--out profiles/glsl_views_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_glsl_views.py --profile v64_320x180

Cases, all of the default uniforms (glsl_scenes.default_uniforms) with the floor texture: 64 views
of 320x180 from a circle round the origin inside the cave; the six 512x512 faces of a cube map
there, fov 90 degrees; a stereo pair and 16 views of 1920x1080.  Per case, one shader and one set of
targets per variant, the variants alternating within each repeat:

* loop:                  set_uniform("campos" / "rotation" / "fov") + draw per view on one stream,
                         SFRT_OPT_TILE_ORDER at its default (1: longest tiles first, wall cull);
* loop_order0:           the same with SFRT_OPT_TILE_ORDER 0 (row-major, four tiles a workgroup);
* loop_2streams:         the default loop, the views alternating between two streams; the window
                         opens on the first, which the second waits for, and closes on the first
                         once it has waited for the second;
* loop_2streams_order0:  the same with SFRT_OPT_TILE_ORDER 0;
* batch:                 one render_views call.

Every repeat warms `warmup` windows, then times `frames` windows with a HIP event pair around
each: the median, minus the empty pair's own time.  host_us is the median wall time of the
window's calls themselves, measured in a pass of its own with the device idle before each window
(submission only).  No threshold anywhere: the file records what came out.

--profile CASE runs, for a profiler, `frames` windows of loop and of batch.
--any-flavour lets a build with extra flags be timed (SFRT_LIB: the batch kernels' other form,
-DSFRT_GLSL_VIEWS_CULL=0); the file records the flavour.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sfml-software-raytracer_amd"))

CASES = {  # name: (views, width, height, kind)
    "v64_320x180": (64, 320, 180, "circle"),
    "cube6_512": (6, 512, 512, "cube"),
    "stereo2_1080p": (2, 1920, 1080, "stereo"),
    "v16_1080p": (16, 1920, 1080, "circle"),
}
VARIANTS = ("loop", "loop_order0", "loop_2streams", "loop_2streams_order0", "batch")
CENTRE = (0.0, 0.0, 0.0)  # SphereWorld's camera; the cave's walls hold a ball of radius 1 round it


def cameras(case):
    import glsl_scenes as gs
    import sfrt
    n, _, _, kind = CASES[case]
    u = gs.default_uniforms(16, 9)
    out = []
    for k in range(n):
        c = sfrt.Camera()
        c.fov_h, c.fov_v = float(u["fov"][0]), float(u["fov"][1])
        c.pos[0], c.pos[1], c.pos[2] = CENTRE
        if kind == "cube":  # four faces round the horizon, then up and down
            c.fov_h = c.fov_v = 1.0  # the shader's fov is the half angle's tangent: 90 degrees
            c.rotation = (k % 4) * math.pi / 2 if k < 4 else 0.0
            c.hrotation = 0.0 if k < 4 else (math.pi / 2 if k == 4 else -math.pi / 2)
        elif kind == "stereo":
            c.pos[0] = CENTRE[0] + (-0.0325 if k == 0 else 0.0325)
            c.rotation, c.hrotation = 0.7, 0.3
        else:  # a circle of radius 1 round the origin, each looking a little further round
            a = 2 * math.pi * k / n
            c.pos[0], c.pos[2] = CENTRE[0] + math.cos(a), CENTRE[2] + math.sin(a)
            c.pos[1] = CENTRE[1] + 0.3 * math.sin(3 * a)
            c.rotation, c.hrotation = a, 0.1 * math.cos(a)
        out.append(c)
    return out


def make_shader(case, order=None):
    import glsl_scenes as gs
    import scenes
    import sfrt
    _, width, height, _ = CASES[case]
    sh = sfrt.GlslShader(0)
    sh.set_ground(*scenes.load_floor())
    sh.set_uniforms(gs.default_uniforms(width, height, 0.7, 0.3))
    if order is not None:
        sh.set_option(sfrt.SFRT_OPT_TILE_ORDER, order)
    return sh


def run_loop(sh, cams, ptrs, width, height, pitch, streams):
    for k, c in enumerate(cams):
        sh.set_uniform("campos", (c.pos[0], c.pos[1], c.pos[2]))
        sh.set_uniform("rotation", (c.rotation, c.hrotation))
        sh.set_uniform("fov", (c.fov_h, c.fov_v))
        sh.draw(ptrs[k], width, height, pitch, 0, height, streams[k % len(streams)])


def bench(a):
    import numpy as np
    import torch
    import sfrt

    flavour = sfrt.build_flavour()
    if flavour != "release" and not a.any_flavour:
        raise SystemExit("bench_glsl_views.py times the release build only (--any-flavour)")
    stream, second = torch.cuda.Stream(), torch.cuda.Stream()
    st, st2 = stream.cuda_stream, second.cuda_stream

    def event_gap():
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                 for _ in range(64)]
        for x, y in pairs:
            x.record(stream)
            y.record(stream)
        torch.cuda.synchronize()
        return float(np.median([x.elapsed_time(y) for x, y in pairs]))

    cases = {}
    for case, (n, width, height, kind) in CASES.items():
        if a.cases and case not in a.cases:
            continue
        pitch = 4 * width
        frames = torch.zeros(n, height, pitch, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the launches on `stream`
        ptrs = [frames[k].data_ptr() for k in range(n)]
        cams = cameras(case)
        views = [sfrt.View(c, ptrs[k]) for k, c in enumerate(cams)]
        shaders = {v: make_shader(case, 0 if v.endswith("order0") else None) for v in VARIANTS}

        def calls(v, x=None):
            """The variant's calls; x: the event that opened the window on `stream`."""
            sh = shaders[v]
            if v.startswith("loop_2streams"):
                if x is not None:
                    second.wait_event(x)
                run_loop(sh, cams, ptrs, width, height, pitch, (st, st2))
                done = torch.cuda.Event()
                done.record(second)
                stream.wait_event(done)
            elif v.startswith("loop"):
                run_loop(sh, cams, ptrs, width, height, pitch, (st,))
            else:
                sh.render_views(views, width, height, pitch, stream=st)

        def timed(v):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(a.warmup + a.frames)]
            for x, y in ev:
                x.record(stream)
                calls(v, x)
                y.record(stream)
            torch.cuda.synchronize()
            shaders[v].check(st)
            raw = float(np.median([x.elapsed_time(y) for x, y in ev[a.warmup:]]))
            # the calls' own wall time, the device idle before each window (back to back the
            # host runs ahead until a staging ring is full and then waits for the device)
            host = []
            for _ in range(a.frames):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                calls(v)
                host.append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize()
            shaders[v].check(st)
            return (round(max(0.0, raw - event_gap()) * 1e3, 2), round(float(np.median(host)), 2))

        runs = {v: [] for v in VARIANTS}
        hosts = {v: [] for v in VARIANTS}
        for _ in range(a.repeats):
            for v in VARIANTS:
                dev, host = timed(v)
                runs[v].append(dev)
                hosts[v].append(host)
        loop = float(np.median(runs["loop"]))
        out = {"views": n, "width": width, "height": height, "scene": "default_uniforms + floor",
               "cameras": kind, "variants": {}}
        for v in VARIANTS:
            med = float(np.median(runs[v]))
            out["variants"][v] = {"window_us": runs[v], "median_us": round(med, 2),
                                  "range_us": round(max(runs[v]) - min(runs[v]), 2),
                                  "per_view_us": round(med / n, 2),
                                  "host_us": round(float(np.median(hosts[v])), 2),
                                  "of_loop": round(med / loop, 4)}
            print(f"{case:16s} {v:21s} {med:10.2f} us  range {out['variants'][v]['range_us']:8.2f}  "
                  f"host {out['variants'][v]['host_us']:9.2f} us  {med / loop:6.3f} of loop", flush=True)
        cases[case] = out
        for sh in shaders.values():
            sh.close()
        del frames
    doc = {"command": f"python tools/bench_glsl_views.py --warmup {a.warmup} --frames {a.frames} "
                      f"--repeats {a.repeats}",
           "device": torch.cuda.get_device_name(0), "build_flavour": flavour,
           "timing": "HIP event pair around each window on one stream, median over the windows "
                     "minus the empty pair's time, per repeat; variants alternate within each "
                     "repeat; host_us: wall time of the window's calls, the device idle before each",
           "warmup": a.warmup, "frames": a.frames, "repeats": a.repeats, "cases": cases}
    write(a.out, doc)


def profile(a):
    """`frames` windows of the one-stream loop, then of the batch, for a profiler."""
    import torch
    import sfrt
    n, width, height, _ = CASES[a.profile]
    pitch = 4 * width
    stream = torch.cuda.Stream()
    frames = torch.zeros(n, height, pitch, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptrs = [frames[k].data_ptr() for k in range(n)]
    cams = cameras(a.profile)
    views = [sfrt.View(c, ptrs[k]) for k, c in enumerate(cams)]
    sh = make_shader(a.profile)
    for _ in range(a.frames):
        run_loop(sh, cams, ptrs, width, height, pitch, (stream.cuda_stream,))
    sh.check(stream.cuda_stream)
    for _ in range(a.frames):
        sh.render_views(views, width, height, pitch, stream=stream.cuda_stream)
    sh.check(stream.cuda_stream)
    sh.close()


def write(path, doc):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glsl_views_bench.json"))
    ap.add_argument("--cases", nargs="*", choices=sorted(CASES), help="a subset of the cases")
    ap.add_argument("--any-flavour", action="store_true", help="time a build with extra flags too")
    ap.add_argument("--profile", choices=sorted(CASES), help="run the profiled windows of a case")
    a = ap.parse_args()
    if a.profile:
        profile(a)
    else:
        bench(a)


if __name__ == "__main__":
    main()
