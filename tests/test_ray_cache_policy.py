"""The ray cache's policy (csrc/sfrt_raycache.h: when a chain fills, reads or leaves its cache of
primary ray directions) as a stand-alone host program, tests/native/raycache_check.cpp, built
with the host sanitizers: fill only on the second consecutive equal key, read on an equal key,
a miss on every single key field, no fill while the key keeps changing, the budget, and
invalidation by a failed launch.  No GPU, no HIP."""
import os
import subprocess

from conftest import ROOT


def test_ray_cache_policy_native(tmp_path):
    exe = tmp_path / "raycache_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "sfml-software-raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "raycache_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "raycache_check ok" in r.stdout, r.stdout + r.stderr
