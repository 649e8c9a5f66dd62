"""The compact layer's record, brightness classes and policy (csrc/sfrt_raycache.h CompactRec,
BrightClasses, the compact layer of ChainCaches) as a stand-alone host program,
tests/native/compactrec_check.cpp, built with the host sanitizers and -ffp-contract=off (one
rounding per product, as the kernels are built): the class table against its definition and an
independent recount, class_of at its edges and over 10^7 random pairs, the record's packing, and
the chain -- the rest sequence, a miss and the later refill on the key's fields, eligibility at
65,535 and 65,536 texels and when supersampled, a texel refill that drops the layer, the shared
budget, a refused allocation, failed launches, two chains, no leak.  The five earlier native checks
share chain_harness.h and ChainCaches::begin's earlier signature: they are built and run by their
own tests, unchanged.  No GPU, no HIP."""
import os
import subprocess

from conftest import ROOT


def test_compact_policy_native(tmp_path):
    exe = tmp_path / "compactrec_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "sfml-software-raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "compactrec_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "compactrec_check ok" in r.stdout, r.stdout + r.stderr
