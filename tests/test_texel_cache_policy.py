"""The texel cache's policy and record (csrc/sfrt_raycache.h TexelRec, TexKey, the texel layer of
ChainCaches: when a chain stores, reads or leaves its cache of per-ray texel indices) as a
stand-alone host program, tests/native/texelcache_check.cpp, built with the host sanitizers: the
rest sequence, a miss and the later refill on every field of the key, texels that change under an
unchanged key, a hit-layer refill that drops the layer, the shared budget, a refused allocation,
failed launches, a takeover, two chains, and the packing of the sentinel and of the moving bit in
the brightness' sign.  No GPU, no HIP."""
import os
import subprocess

from conftest import ROOT


def test_texel_cache_policy_native(tmp_path):
    exe = tmp_path / "texelcache_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "sfml-software-raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "texelcache_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "texelcache_check ok" in r.stdout, r.stdout + r.stderr
