"""The pixel layer's policy (csrc/sfrt_raycache.h PixelKey, the pixel layer of ChainCaches) as a
stand-alone host program, tests/native/pixelcache_check.cpp, built with the host sanitizers: the
rest sequence up to the pixel read (over the compact layer, over the texel layer, supersampled), a
miss and the later refill for the texel generation and for every field of the key, a generation
change that keeps the lower layers, a reload on every frame that never fills, a lower refill that
drops the layer, a launch that takes no part, the option, the shared budget (exactly enough, a
byte short, lower layers never displaced, another chain's bytes, two 4K chains at the default), a
refused allocation, failed launches, a takeover, no leak.  The six earlier native checks share
chain_harness.h and ChainCaches::begin's earlier signature: they are built and run by their own
tests, unchanged.  No GPU, no HIP."""
import os
import subprocess

from conftest import ROOT


def test_pixel_policy_native(tmp_path):
    exe = tmp_path / "pixelcache_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "sfml-software-raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "pixelcache_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pixelcache_check ok" in r.stdout, r.stdout + r.stderr
