"""tests/voxel_ref.py, the numpy binary32 restatement of World::UpdateImage / Raycast / LRaycast
(World.cpp:62-87, 302-491) that the voxel aux-plane tests compare against, pinned on the CPU.

The voxel oracle (oracle/voxelworld_oracle.c) exposes no per-pixel intermediates, so the planes of
sfrt_voxel_render_band_aux (depth, cell, face, steps) are held to voxel_ref -- which is trusted
only because its colour frame equals the oracle's byte for byte here.  The planes are by-products
of the march that produces that colour.  Also: the coverage of the GPU tests' cases
(tests/voxel_aux_cases.py) asserted on the reference side, the committed hashes of their reference
planes, the supersampling identity, and the new calls' null-handle answers.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import oracle
import voxel_aux_cases as vc
import voxel_ref
import voxel_scenes as vs
from conftest import ROOT, host_threads

GOLDEN = os.path.join(ROOT, "tests", "golden", "voxel_aux.json")


@pytest.fixture(scope="module")
def assets():
    oracle.build()
    return vc.assets()


def pin(scene, w, h, assets):
    """voxel_ref's frame against the oracle's: (differing pixels, voxel_ref's and the oracle's
    counts of texel reads outside a texture)."""
    o = oracle.VoxelOracle(scene, w, h, assets[0], assets[1], vs.COLORS)
    before = oracle.VoxelOracle.bad_texel_reads()
    want = o.render(host_threads()).reshape(h, w, 4)
    counted = oracle.VoxelOracle.bad_texel_reads() - before
    ref = voxel_ref.render(scene, w, h, assets[0], assets[1], vs.COLORS)
    return int(np.any(ref["rgba"] != want, axis=2).sum()), ref["bad_texels"], counted


@pytest.mark.parametrize("pose", vc.DEFAULT_POSES, ids=lambda p: p[3])
def test_pin_default_poses(assets, pose):
    p, r, hr, _ = pose
    diff, bad, counted = pin(vs.default_world(p, r, hr), 96, 54, assets)
    assert diff == 0 and bad == counted == 0


@pytest.mark.parametrize("pose", vc.EDGE_POSES, ids=lambda p: p[3])
def test_pin_edge_poses(assets, pose):
    """Every pose of VOXEL_EDGE_CASES (tests/test_voxel.py), the ones that read outside a texture
    (the oracle's magenta and its count) and the ones beyond 2^30 included."""
    p, r, hr, _ = pose
    diff, bad, counted = pin(vs.default_world(p, r, hr), 64, 36, assets)
    assert diff == 0 and bad == counted


def test_edge_poses_are_test_voxels():
    """The copied tuples are the poses of tests/test_voxel.py's VOXEL_EDGE_CASES."""
    import test_voxel
    assert [(p, r, hr, n) for p, r, hr, n in vc.EDGE_POSES] == \
        [(c[2], c[3], c[4], c[5]) for c in test_voxel.VOXEL_EDGE_CASES]


@pytest.mark.parametrize("seed", list(range(16)))
def test_pin_random_worlds(assets, seed):
    scene, _, _ = vs.random_world(seed)
    diff, bad, counted = pin(scene, 72, 40, assets)
    assert diff == 0 and bad == counted


def test_pin_supersampled_sample_frame(assets):
    """S = 2 of a 64 x 36 frame: the samples are the pixels of the 128 x 72 frame."""
    p, r, hr, _ = vc.DEFAULT_POSES[1]
    diff, bad, counted = pin(vs.default_world(p, r, hr), 128, 72, assets)
    assert diff == 0 and bad == counted == 0


def test_gpu_cases_cover_every_outcome():
    """The cases the GPU tests render (101 x 37), on the reference side: every face value (the
    issue's list: -3..-1, 0, 1..3 and 4), a ray with a zero direction component (its wave takes
    the guarded DDA), a read outside a texture (SFRT_E_TEXEL) and steps from 1 to maxiter."""
    faces, zero, texel, lo, full = set(), False, False, 1 << 30, False
    for name in vc.NAMES:
        ref = vc.reference(name)
        faces |= set(np.unique(ref["face"]).tolist())
        zero |= ref["zero_dir"]
        texel |= ref["bad_texels"] > 0
        lo = min(lo, int(ref["steps"].min()))
        full |= int(ref["steps"].max()) == ref["maxiter"]
        hit = (ref["face"] != 0) & (ref["face"] != 4)
        assert (ref["cell"][hit] >= 0).all() and (ref["cell"][ref["face"] == 0] == -1).all(), name
        assert (ref["steps"] >= 0).all() and (ref["steps"] <= ref["maxiter"]).all(), name
    assert faces == {-3, -2, -1, 0, 1, 2, 3, 4}
    assert zero and texel and lo <= 1 and full
    assert vc.reference("negative_coordinates")["bad_texels"] > 0  # the GPU error test's pose
    assert vc.reference("axis_parallel_column")["zero_dir"]


def test_reference_planes_match_committed_hashes():
    """A later edit of the restatement that moves a plane is noticed (tests/golden/voxel_aux.json:
    FNV-1a 64 of each reference plane's bytes, per case)."""
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(vc.NAMES)
    for name in vc.NAMES:
        ref = vc.reference(name)
        got = {k: oracle.fnv1a64(np.ascontiguousarray(ref[k]).view(np.uint8)) for k in voxel_ref.PLANES}
        assert got == golden[name], name


# What fraction of the LAST sample's planes (sample (S*i + S-1, S*j + S-1)) differs from the 1x
# planes, at least, in every supersampling case: the GPU test's guard that "first sample" is not
# vacuous.  Measured here with voxel_ref: depth >= 0.999 of the pixels, the others >= 0.009.
LAST_SAMPLE_DIFFERS = {"depth": 0.99, "cell": 0.005, "face": 0.005, "steps": 0.005}


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("name", vc.SS_NAMES)
def test_first_sample_planes_equal_the_1x_planes(name, s):
    """fov / (S * W) is the 1x increment divided by a power of two, so hray and vray of sample
    (S*i, S*j) are the 1x pixel's bit for bit and so are its planes (0 pixels differ); the last
    sample's planes differ."""
    one, big = vc.reference(name), vc.reference(name, s)
    first = voxel_ref.first_sample(big, s)
    for k in voxel_ref.PLANES:
        assert np.array_equal(first[k].view(np.uint32), one[k].view(np.uint32)), k
        last = big[k][s - 1::s, s - 1::s]
        frac = float((last.view(np.uint32) != one[k].view(np.uint32)).mean())
        print(f"{name} S={s} {k}: last sample differs in {frac:.4f} of the pixels")
        assert frac >= LAST_SAMPLE_DIFFERS[k], (k, frac)


def test_box_filter_rule():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (8, 12, 4), dtype=np.uint8)
    for s in (2, 4):
        got = voxel_ref.box_filter(a, s)
        want = (a.reshape(8 // s, s, 12 // s, s, 4).astype(int).sum(axis=(1, 3)) + s * s // 2) >> (2 * (s // 2))
        assert np.array_equal(got, want.astype(np.uint8))


def test_null_handle_is_invalid(built):
    import sfrt
    L = sfrt.lib()
    assert L.sfrt_version() >= 8
    planes = sfrt.VoxelAuxPlanes()
    buf = (ctypes.c_uint8 * 16)()
    assert L.sfrt_voxel_render_band_aux(None, buf, 16, ctypes.byref(planes), 0, 1, None) == -1
    assert L.sfrt_voxel_update_image_aux(None, buf, buf, buf, buf, buf, 0, 1, 0, 1) == -1
