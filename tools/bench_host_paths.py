"""Wall clock of the synchronous host paths for several builds of libsfrt.so, interleaved.

    python tools/bench_host_paths.py --libs parent.so,new.so,parent_copy.so [--rounds 3] [--reps 100]

The device events of tools/ab_libs.py do not see these calls' host side (staging, scatter, the
status read), so each is timed around the call itself, which ends in a device sync: update_image
at 1080p for the sphere and the voxel world, draw_image at 1080p for the GLSL renderer, and a host
cast_rays of 100,000 rays for each renderer.  Each round starts one process per library
(SFRT_LIB=<lib>) in turn; every case runs `reps` warm calls; the table gives the median over all
rounds' calls in microseconds and one output hash per case, which must agree between libraries.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("world_update_image", "voxel_update_image", "glsl_draw_image", "world_cast_rays",
         "voxel_cast_rays", "glsl_cast_rays")


def child(reps):
    sys.path.insert(0, os.path.join(ROOT, "sfml-software-raytracer_amd"))
    import numpy as np
    import glsl_scenes as gs
    import scenes
    import sfrt
    import voxel_scenes as vs
    w, h, n = 1920, 1080, 100_000
    dirs = np.random.default_rng(3).standard_normal((n, 3)).astype(np.float32)
    floor = scenes.load_floor()
    world = sfrt.World(0)
    world.load_texture(*floor)
    world.set_scene(scenes.default10(), w, h)
    vw = sfrt.VoxelWorld(0)
    tex, dyn = vs.load_textures()
    vw.load_assets(tex, dyn, vs.COLORS)
    vw.set_scene(vs.default_world((15.5, 1.9, 15.5), 0.0, 0.0), w, h)
    g = sfrt.GlslShader(0)
    g.set_ground(*floor)
    g.set_uniforms(gs.default_uniforms(w, h, 0.0, 0.0))
    frame = np.zeros(w * h * 4, np.uint8)
    calls = {
        "world_update_image": lambda: world.update_image(frame),
        "voxel_update_image": lambda: vw.update_image(frame),
        "glsl_draw_image": lambda: g.draw_image(w, h),
        "world_cast_rays": lambda: world.cast_rays(dirs)["rgba"],
        "voxel_cast_rays": lambda: vw.cast_rays(dirs)["rgba"],
        "glsl_cast_rays": lambda: g.cast_rays(dirs)["rgba"],
    }
    out = {}
    for name in CASES:
        fn = calls[name]
        for _ in range(10):
            res = fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        out[name] = {"us": t, "hash": hashlib.sha256(np.asarray(res).tobytes()).hexdigest()[:16]}
    for o in (world, vw, g):
        o.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.reps)
        return
    libs = a.libs.split(",")
    times = {lib: {c: [] for c in CASES} for lib in libs}
    per_round = {lib: {c: [] for c in CASES} for lib in libs}  # each process's own median
    hashes = {}
    for _ in range(a.rounds):
        for lib in libs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=600,
                               env=dict(os.environ, SFRT_LIB=os.path.abspath(lib)))
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(r.stdout[-2000:], r.stderr[-2000:])
                raise SystemExit(f"{lib}: child failed")
            d = json.loads(line[0][7:])
            for c in CASES:
                times[lib][c] += d[c]["us"]
                per_round[lib][c].append(round(sorted(d[c]["us"])[len(d[c]["us"]) // 2], 1))
                if hashes.setdefault(c, d[c]["hash"]) != d[c]["hash"]:
                    raise SystemExit(f"{lib}: {c} output differs")
    print(f"{'median us':40s} " + "  ".join(f"{c:>18s}" for c in CASES))
    for lib in libs:
        med = [sorted(times[lib][c])[len(times[lib][c]) // 2] for c in CASES]
        print(f"{lib:40s} " + "  ".join(f"{m:18.1f}" for m in med))
    print(json.dumps({"per_round_median_us": per_round}))


if __name__ == "__main__":
    main()
