"""Cost of a batch of camera views of the voxel world in one launch (sfrt_voxel_render_views)
against the loop it replaces: set_camera + render_band per view.

    python tools/bench_voxel_views.py [--warmup 10] [--frames 30] [--repeats 5]
                                      [--out profiles/voxel_views_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_voxel_views.py --profile v64_320x180

Cases, all of the default world (voxel_scenes.default_world, its list sorted for the first camera):
64 views of 320x180 from a circle round the default camera; the six 512x512 faces of a cube map
there, fov 90 degrees; a stereo pair and 16 views of 1920x1080.  Per case, one world and one set of
targets per variant, the variants alternating within each repeat:

* loop:           set_camera + render_band per view on one stream (the list as it stands);
* loop_2streams:  the same, the views alternating between two streams; the window opens on the
                  first, which the second waits for, and closes on the first once it has waited for
                  the second;
* loop_dynamics:  set_camera + set_dynamics(sort_dynamics(list, cam)) + render_band per view on one
                  stream: the loop SFRT_VOXEL_VIEWS_DYNAMICS replaces;
* batch:          one render_views call;
* batch_dynamics: one render_views call with SFRT_VOXEL_VIEWS_DYNAMICS.

Every repeat warms `warmup` windows, then times `frames` windows with a HIP event pair around
each: the median, minus the empty pair's own time.  host_us is the median wall time of the
window's calls themselves, measured in a pass of its own with the device idle before each window
(submission only).  No threshold anywhere: the file records what came out.

--profile CASE runs, for a profiler, `frames` windows of loop and of batch.
"""
import argparse
import dataclasses
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
VARIANTS = ("loop", "loop_2streams", "loop_dynamics", "batch", "batch_dynamics")
CENTRE = (15.5, 1.9, 15.5)  # World.h:9-19


def cameras(case):
    import sfrt
    import voxel_scenes as vs
    n, _, _, kind = CASES[case]
    out = []
    for k in range(n):
        c = sfrt.Camera()
        c.fov_h, c.fov_v = float(vs.deg2rad(75)), float(vs.deg2rad(47))
        c.pos[0], c.pos[1], c.pos[2] = CENTRE
        if kind == "cube":  # four faces round the horizon, then up and down
            c.fov_h = c.fov_v = float(vs.deg2rad(90))
            c.rotation = (k % 4) * math.pi / 2 if k < 4 else 0.0
            c.hrotation = 0.0 if k < 4 else (math.pi / 2 if k == 4 else -math.pi / 2)
        elif kind == "stereo":
            c.pos[0] = CENTRE[0] + (-0.0325 if k == 0 else 0.0325)
        else:  # a circle of radius 2 round the default camera, each looking a little further round
            a = 2 * math.pi * k / n
            c.pos[0], c.pos[2] = CENTRE[0] + 2 * math.cos(a), CENTRE[2] + 2 * math.sin(a)
            c.pos[1] = CENTRE[1] + 0.3 * math.sin(3 * a)
            c.rotation, c.hrotation = a, 0.1 * math.cos(a)
        out.append(c)
    return out


def make_world(case, cams):
    import sfrt
    import voxel_scenes as vs
    _, width, height, _ = CASES[case]
    tex, dyn = vs.load_textures()
    scene = vs.default_world(tuple(cams[0].pos), cams[0].rotation, cams[0].hrotation)
    scene = dataclasses.replace(scene, dyn=sfrt.sort_dynamics(scene.dyn, tuple(cams[0].pos)))
    w = sfrt.VoxelWorld(0)
    w.load_assets(tex, dyn, vs.COLORS)
    w.set_scene(scene, width, height)
    return w, scene


def run_loop(w, cams, ptrs, pitch, height, streams, dyn=None):
    import sfrt
    for k, c in enumerate(cams):
        w.set_camera(c)
        if dyn is not None:
            w.set_dynamics(sfrt.sort_dynamics(dyn, tuple(c.pos)))
        w.render_band(ptrs[k], pitch, 0, height, streams[k % len(streams)])


def bench(a):
    import numpy as np
    import torch
    import sfrt

    if sfrt.build_flavour() != "release":
        raise SystemExit("bench_voxel_views.py times the release build only")
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
        pitch = 4 * width
        frames = torch.zeros(n, height, pitch, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the launches on `stream`
        ptrs = [frames[k].data_ptr() for k in range(n)]
        cams = cameras(case)
        views = [sfrt.View(c, ptrs[k]) for k, c in enumerate(cams)]
        worlds, scene = {}, None
        for v in VARIANTS:
            worlds[v], scene = make_world(case, cams)

        def calls(v, x=None):
            """The variant's calls; x: the event that opened the window on `stream`."""
            w = worlds[v]
            if v == "loop_2streams":
                if x is not None:
                    second.wait_event(x)
                run_loop(w, cams, ptrs, pitch, height, (st, st2))
                done = torch.cuda.Event()
                done.record(second)
                stream.wait_event(done)
            elif v.startswith("loop"):
                run_loop(w, cams, ptrs, pitch, height, (st,),
                         dyn=scene.dyn if v == "loop_dynamics" else None)
            else:
                w.render_views(views, pitch, dynamics=(v == "batch_dynamics"), stream=st)

        def timed(v):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(a.warmup + a.frames)]
            for x, y in ev:
                x.record(stream)
                calls(v, x)
                y.record(stream)
            torch.cuda.synchronize()
            worlds[v].check(st)
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
            worlds[v].check(st)
            return (round(max(0.0, raw - event_gap()) * 1e3, 2), round(float(np.median(host)), 2))

        runs = {v: [] for v in VARIANTS}
        hosts = {v: [] for v in VARIANTS}
        for _ in range(a.repeats):
            for v in VARIANTS:
                dev, host = timed(v)
                runs[v].append(dev)
                hosts[v].append(host)
        loop = float(np.median(runs["loop"]))
        out = {"views": n, "width": width, "height": height, "scene": "default_world",
               "dynamics": int(scene.dyn.shape[0]), "lights": int(scene.lights.shape[0]),
               "cameras": kind, "variants": {}}
        for v in VARIANTS:
            med = float(np.median(runs[v]))
            out["variants"][v] = {"window_us": runs[v], "median_us": round(med, 2),
                                  "range_us": round(max(runs[v]) - min(runs[v]), 2),
                                  "per_view_us": round(med / n, 2),
                                  "host_us": round(float(np.median(hosts[v])), 2),
                                  "of_loop": round(med / loop, 4)}
            print(f"{case:16s} {v:15s} {med:10.2f} us  range {out['variants'][v]['range_us']:8.2f}  "
                  f"host {out['variants'][v]['host_us']:9.2f} us  {med / loop:6.3f} of loop", flush=True)
        cases[case] = out
        for w in worlds.values():
            w.close()
        del frames
    doc = {"command": f"python tools/bench_voxel_views.py --warmup {a.warmup} --frames {a.frames} "
                      f"--repeats {a.repeats}",
           "device": torch.cuda.get_device_name(0),
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
    w, _ = make_world(a.profile, cams)
    for _ in range(a.frames):
        run_loop(w, cams, ptrs, pitch, height, (stream.cuda_stream,))
    w.check(stream.cuda_stream)
    for _ in range(a.frames):
        w.render_views(views, pitch, stream=stream.cuda_stream)
    w.check(stream.cuda_stream)
    w.close()


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_views_bench.json"))
    ap.add_argument("--profile", choices=sorted(CASES), help="run the profiled windows of a case")
    a = ap.parse_args()
    if a.profile:
        profile(a)
    else:
        bench(a)


if __name__ == "__main__":
    main()
