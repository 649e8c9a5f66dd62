"""The tile records of the ray cache (csrc/sfrt_raycache.h TileRec, CacheBuf) as a stand-alone
host program, tests/native/tilerec_check.cpp, built with the host sanitizers: the record's size,
alignment and field offsets as the fill kernel and the trace kernels share them through that
header, and a chain's bookkeeping of its two buffers -- allocated with the fill, kept while the
key is read and across a position change, refilled in place after a basis change, regrown for a
larger grid, never read after a failed launch -- driven through ChainCaches::begin and end.
No GPU, no HIP."""
import os
import subprocess

from conftest import ROOT


def test_tile_record_layout_and_bookkeeping_native(tmp_path):
    exe = tmp_path / "tilerec_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "sfml-software-raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "tilerec_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tilerec_check ok" in r.stdout, r.stdout + r.stderr
