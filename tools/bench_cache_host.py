"""The host cost of a launch that reads a chain's caches (csrc/sfrt_raycache.h ChainCaches), for
whatever library SFRT_LIB names.

    [SFRT_LIB=<lib>] python tools/bench_cache_host.py [--launches 20000] [--reps 5]

A still camera: after an uncached and a filling frame every render_band builds its keys, compares
them with the chain's, and queues the kernel that shades from the hit records -- the shortest
launch the library makes, so the one on which host work per launch shows first.  Per case (1080p
default10: the records in the kernel arguments; 4K lcg64: the largest key of the inline kernels)
`reps` loops of `launches` back-to-back launches on one stream, each timed by the host clock
around a final stream synchronise; one JSON line with every loop's microseconds per launch.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"1920x1080_default10": (1920, 1080, "default10"), "3840x2160_lcg64": (3840, 2160, "lcg64")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "sfml-software-raytracer_amd"))
    import torch
    import scenes
    import sfrt
    stream = torch.cuda.Stream()
    out = {"library": sfrt.LIB_PATH, "launches": a.launches, "us_per_launch": {}}
    for name, (width, height, scene) in CASES.items():
        with sfrt.World(0) as w:
            w.load_texture(*scenes.load_floor())
            w.set_scene(scenes.SCENES[scene](), width, height)
            buf = torch.empty(height, width * 4, dtype=torch.uint8, device="cuda")

            def loop(n):
                t0 = time.perf_counter()
                for _ in range(n):
                    w.render_band(buf.data_ptr(), width * 4, 0, height, stream.cuda_stream)
                stream.synchronize()
                return (time.perf_counter() - t0) / n * 1e6

            loop(2000)  # the uncached frame, the filling one, the clock's ramp
            hits0 = w.hit_cache_stats()["hits"]
            runs = [round(loop(a.launches), 3) for _ in range(a.reps)]
            w.check(stream.cuda_stream)
            if w.hit_cache_stats()["hits"] - hits0 != a.launches * a.reps:
                raise SystemExit(f"{name}: not every timed launch read the hit cache")
            out["us_per_launch"][name] = runs
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
