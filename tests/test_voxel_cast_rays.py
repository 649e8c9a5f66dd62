"""Batched ray queries of the voxel world: sfrt_voxel_cast_rays (World::Raycast) and
sfrt_voxel_cast_shadow_rays (World::LRaycast) for caller-supplied rays (include/sfrt.h).

The reference is tests/voxel_rays_ref.py, the numpy binary32 restatement.  It is trusted only
because the CPU tests here pin it: on the frame's own rays to voxel_ref.render (itself pinned to
the oracle in tests/test_voxel_ref.py) and to the oracle's frame, in own-origin mode to the same
code, and its shadow march to the booleans voxel_ref's colour path computes.  Every comparison is
on bit patterns.  The GPU tests use W x H = 101 x 37 rays: 58 full waves and a 25-lane tail.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import voxel_aux_cases as vc
import voxel_rays_ref as vrr
import voxel_ref
import voxel_scenes as vs
from conftest import ROOT, host_threads, poisoned
from voxel_aux_cases import W, H

F = np.float32
N = W * H
POISON = 0xA5
PAD = 64  # canary bytes past every device output
E_INVALID, E_EMPTY, E_TEXEL = -1, -2, -7
OUT = vrr.OUTPUTS
ELEM = {"pos": 12, "depth": 4, "cell": 4, "face": 4, "steps": 4, "rgba": 4, "free": 4}
DTYPE = {"pos": np.float32, "depth": np.float32, "cell": np.int32, "face": np.int32,
         "steps": np.int32, "rgba": np.uint8, "free": np.int32}
PIN_CASES = ["default", "default_turned", "axis_parallel_column", "negative_coordinates",
             "camera_at_int_limit", "random_3"]
INT_LIMIT = 2147483520.0  # the largest float below 2^31


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


def _assert_equal(got, want, what, names=None):
    for k in (names or got):
        assert len(got[k]) == len(want[k]), (what, k, len(got[k]), len(want[k]))
        if len(got[k]) == 0:
            continue
        g, w = _bits(got[k]).reshape(len(got[k]), -1), _bits(want[k]).reshape(len(want[k]), -1)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, (f"{what}: {k}: {bad.size} rays differ, first {bad[0]}: got "
                               f"{got[k][bad[0]]} want {want[k][bad[0]]}")


# ---------------------------------------------------------------- the ray sets and references

@functools.lru_cache(maxsize=None)
def frame_set(name):
    d, ys = vrr.frame_ray_set(vc.scene(name), W, H)
    d.setflags(write=False)
    ys.setflags(write=False)
    return d, ys


def _ref(scene, dirs, yscales, origins, shade=True):
    tex, dyn = vc.assets()
    r = vrr.raycast(scene, dirs, yscales, origins, tex, dyn, vs.COLORS, shade=shade)
    for k in OUT:
        if r[k] is not None:
            r[k].setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def frame_ref(name):
    """The restatement on the frame's own rays of `name`, row-major.  Shared: read only."""
    return _ref(vc.scene(name), *frame_set(name), None)


def _pow2(rng, n, lo=-70, hi=70):
    return np.ldexp(F(1), rng.integers(lo, hi + 1, n)).astype(F)


@functools.lru_cache(maxsize=None)
def arbitrary_set(name, seed=7):
    """N rays for scene `name`: a third of its frame's rays (they reach what a frame reaches,
    billboards included), random un-normalised directions with magnitudes across 2^-70 .. 2^70
    as a whole and per component (both sides of recip_ok's [2^-60, 2^60]), moderate ones,
    axis-parallel ones with one or two zero components (+0 and -0), and random yscales (some
    zero or negative); then shuffled, so waves mix every kind."""
    rng = np.random.default_rng(seed)
    fd, fy = frame_set(name)
    pick = rng.choice(N, 1200, replace=False)
    g = lambda n: rng.standard_normal((n, 3)).astype(F)
    whole = g(900) * _pow2(rng, 900)[:, None]
    comp = g(600) * np.stack([_pow2(rng, 600) for _ in range(3)], axis=1)
    mid = g(600) * rng.uniform(0.25, 4.0, (600, 1)).astype(F)
    axis = g(N - 3300) * rng.uniform(0.5, 2.0, (N - 3300, 1)).astype(F)
    zero = rng.integers(0, 3, axis.shape[0])
    axis[np.arange(axis.shape[0]), zero] = np.where(rng.random(axis.shape[0]) < 0.5, F(0.0), F(-0.0))
    two = rng.random(axis.shape[0]) < 0.3
    axis[two, (zero[two] + 1) % 3] = F(0.0)
    d = np.concatenate([fd[pick], whole, comp, mid, axis]).astype(F)
    ys = np.concatenate([fy[pick], rng.uniform(0.2, 2.5, N - 1200).astype(F)])
    ys[rng.choice(N, 20, replace=False)] = F(0.0)
    ys[rng.choice(N, 20, replace=False)] *= F(-1.0)
    perm = rng.permutation(N)
    d, ys = np.ascontiguousarray(d[perm]), np.ascontiguousarray(ys[perm])
    assert d.shape == (N, 3) and np.isfinite(d).all() and np.isfinite(ys).all()
    d.setflags(write=False)
    ys.setflags(write=False)
    return d, ys


@functools.lru_cache(maxsize=None)
def origin_set(name, seed=11):
    """N origins for scene `name`: inside and around its grid (negative coordinates included), on
    integer positions, far outside (1.5e9 on one axis) and at the int limit (2147483520.0f) --
    the last two are where a wrongly taken plain conversion differs from the guarded one."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = vc.scene(name).blocks.shape
    o = rng.uniform([-3.0, -2.0, -3.0], [nx + 3.0, ny + 2.0, nz + 3.0], (N, 3)).astype(F)
    kind = rng.integers(0, 10, N)
    o[kind == 0] = np.floor(o[kind == 0])                       # integer positions
    far = np.flatnonzero(kind == 1)
    o[far, rng.integers(0, 3, far.size)] = F(1.5e9) * np.where(rng.random(far.size) < 0.5, F(1), F(-1))
    lim = np.flatnonzero(kind == 2)
    o[lim, rng.integers(0, 3, lim.size)] = F(INT_LIMIT) * np.where(rng.random(lim.size) < 0.7, F(1), F(-1))
    assert np.isfinite(o).all()
    o.setflags(write=False)
    return o


ARB_CAMERA = ["random_3", "negative_coordinates"]  # billboards; reads outside a texture
ARB_OWN = ["default", "random_3"]


@functools.lru_cache(maxsize=None)
def arbitrary_ref(name, own):
    d, ys = arbitrary_set(name)
    return _ref(vc.scene(name), d, ys, origin_set(name) if own else None)


@functools.lru_cache(maxsize=None)
def shadow_set(seed=5):
    """N segments through the default world: random starts in the rooms, random ends up to 40
    away (max_dist <= 64 everywhere), the direction normalised as the reference passes it; an
    eighth with un-normalised directions across 2^-70 .. 2^70 and some zero components."""
    rng = np.random.default_rng(seed)
    o = rng.uniform([1.2, 1.2, 1.2], [98.8, 8.8, 98.8], (N, 3)).astype(F)
    e = (rng.standard_normal((N, 3)) * rng.uniform(0.5, 14.0, (N, 1))).astype(F)
    ln = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]).astype(F)
    d = (e / ln[:, None]).astype(F)
    md = np.minimum(ln, F(64.0)).astype(F)
    odd = rng.random(N) < 0.125
    d[odd] = d[odd] * _pow2(rng, int(odd.sum()))[:, None]
    z = rng.random(N) < 0.03
    d[z, rng.integers(0, 3, int(z.sum()))] = F(0.0)
    for a in (o, d, md):
        a.setflags(write=False)
    return o, d, md


@functools.lru_cache(maxsize=None)
def shadow_ref():
    r = vrr.shadow_rays(vc.scene("default"), *shadow_set())
    for k in ("free", "steps"):
        r[k].setflags(write=False)
    return r


def _no_dyn(scene):
    import dataclasses
    return dataclasses.replace(scene, dyn=scene.dyn[:0])


# ---------------------------------------------------------------- CPU: the restatement is pinned

@pytest.mark.parametrize("name", PIN_CASES)
def test_restatement_equals_voxel_ref_on_the_frames_rays(name):
    """1. The frame's own rays (origins None) give voxel_ref.render's planes and colour."""
    tex, dyn = vc.assets()
    want = voxel_ref.render(vc.scene(name), W, H, tex, dyn, vs.COLORS, shade=True)
    got = frame_ref(name)
    for k in ("depth", "cell", "face", "steps"):
        assert np.array_equal(_bits(got[k]), _bits(want[k].reshape(N))), (name, k)
    assert np.array_equal(got["rgba"], want["rgba"].reshape(N, 4)), name
    assert got["bad_texels"] == want["bad_texels"] and got["maxiter"] == want["maxiter"]


@pytest.mark.parametrize("name", ["default", "random_3"])
def test_restatement_equals_the_oracles_frame(built, name):
    """1. ... and the voxel oracle's bytes (random_3 has billboards)."""
    import oracle
    tex, dyn = vc.assets()
    want = oracle.VoxelOracle(vc.scene(name), W, H, tex, dyn, vs.COLORS).render(host_threads())
    assert np.array_equal(frame_ref(name)["rgba"], want.reshape(N, 4)), name


@pytest.mark.parametrize("name", ["default", "random_3"])
def test_own_origins_at_the_camera_are_the_camera_mode(name):
    """2. With the dynamics removed, own origins all equal to cam.pos give the camera-mode
    answer bit for bit: origins mode is the same code."""
    scene = _no_dyn(vc.scene(name))
    d, ys = arbitrary_set(name)
    cam = np.broadcast_to(np.array(scene.cam_pos, dtype=F), (N, 3))
    a, b = _ref(scene, d, ys, None), _ref(scene, d, ys, cam)
    _assert_equal(a, b, name, OUT)
    assert a["bad_texels"] == b["bad_texels"]


def test_shadow_restatement_agrees_with_the_colour_path(monkeypatch):
    """3. On the (pos, dir, maxDist) triples voxel_ref's light loop passes to _lraycast for
    `default` at 101 x 37, vrr.lraycast returns the same booleans.  Its `steps` have no oracle
    behind them: the restatement defines them (here only: at least one trip wherever the loop
    can run, and never more than the trip limit)."""
    calls = []
    real = voxel_ref._lraycast

    def spy(blocks, pos, d, max_dist):
        r = real(blocks, pos, d, max_dist)
        calls.append((pos.copy(), d.copy(), max_dist.copy(), r.copy()))
        return r

    monkeypatch.setattr(voxel_ref, "_lraycast", spy)
    tex, dyn = vc.assets()
    voxel_ref.render(vc.scene("default"), W, H, tex, dyn, vs.COLORS, shade=True)
    monkeypatch.undo()
    pos, d, md, want = (np.concatenate([c[k] for c in calls]) for k in range(4))
    assert want.size > 1000 and want.any() and not want.all()
    free, steps = vrr.lraycast(vc.scene("default").blocks, pos, d, md)
    assert np.array_equal(free, want)
    limit = voxel_ref.to_u32(np.maximum(md * F(2), F(20.0)))
    assert (steps >= (md > 0)).all() and (steps <= limit).all()


def test_ray_sets_are_not_vacuous():
    """4. On the reference side: the arbitrary camera-mode rays reach every face value, have a
    zero direction component, steps from <= 1 up to maxiter and a texel read outside a texture;
    the own-origin rays never meet a billboard; the shadow set has both answers often."""
    faces, lo, full, texel, zero = set(), 1 << 30, False, False, False
    for name in ARB_CAMERA:
        r = arbitrary_ref(name, False)
        faces |= set(np.unique(r["face"]).tolist())
        lo = min(lo, int(r["steps"].min()))
        full |= int(r["steps"].max()) == r["maxiter"]
        texel |= r["bad_texels"] > 0
        zero |= bool((arbitrary_set(name)[0] == 0).any())
        assert r["valid"].all()
    assert faces == {-3, -2, -1, 0, 1, 2, 3, 4}, faces
    assert zero and lo <= 1 and full and texel
    # random_3's status stays clean in both modes: the batches of the status-sensitive tests
    assert arbitrary_ref("random_3", False)["bad_texels"] == arbitrary_ref("random_3", True)["bad_texels"] == 0
    assert arbitrary_ref("default", True)["bad_texels"] > 0
    for name in ARB_OWN:
        r = arbitrary_ref(name, True)
        assert 4 not in set(np.unique(r["face"]).tolist()), name
        assert {-3, -2, -1, 0, 1, 2, 3} <= set(np.unique(r["face"]).tolist()), name
        o = origin_set(name)
        assert (o < 0).any() and (o == np.floor(o)).all(axis=1).any()
        assert (np.abs(o) == F(1.5e9)).any() and (o == F(INT_LIMIT)).any()
    assert len(vc.scene("default").dyn) > 0  # "never 4" is not for want of billboards
    s = shadow_ref()
    assert (s["free"] == 1).mean() >= 0.10 and (s["free"] == 0).mean() >= 0.10, \
        ((s["free"] == 1).mean(), (s["free"] == 0).mean())
    assert float(shadow_set()[2].max()) <= 64.0 and s["valid"].all()


def test_entry_points_are_declared_and_exported(built):
    """5. The four entry points are in include/sfrt.h, in the bindings' table and in the library;
    a NULL world is refused before anything touches a device."""
    import sfrt
    lib = sfrt.lib()
    assert lib.sfrt_version() >= 9
    header = open(os.path.join(ROOT, "include", "sfrt.h")).read()
    for name in ("sfrt_voxel_cast_rays", "sfrt_voxel_cast_rays_device",
                 "sfrt_voxel_cast_shadow_rays", "sfrt_voxel_cast_shadow_rays_device"):
        assert name in sfrt.ABI_SYMBOLS and hasattr(lib, name) and f"{name}(" in header
    assert "#define SFRT_VOXEL_MAX_SHADOW_DIST 4096.0f" in header
    assert ctypes.sizeof(sfrt.VoxelRayHits) == 6 * ctypes.sizeof(ctypes.c_void_p)
    hits = sfrt.VoxelRayHits(pos=4)
    assert lib.sfrt_voxel_cast_rays(None, 4, None, None, 1, ctypes.byref(hits)) == E_INVALID
    assert lib.sfrt_voxel_cast_rays_device(None, 4, None, None, 1, ctypes.byref(hits), None) == E_INVALID
    assert lib.sfrt_voxel_cast_shadow_rays(None, 4, 4, 4, 1, 4, None) == E_INVALID
    assert lib.sfrt_voxel_cast_shadow_rays_device(None, 4, 4, 4, 1, 4, None, None) == E_INVALID


def _build_cpp_check(tmp_path):
    lib_dir = os.path.join(ROOT, "sfml-software-raytracer_amd")
    exe = tmp_path / "cpp_voxel_raycast_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "cpp_voxel_raycast_check.cpp"), "-L", lib_dir,
                    "-lsfrt", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath-link,/opt/rocm/lib",
                    "-o", str(exe)], check=True)
    return exe


def test_cpp_voxel_raycast_builds(built, tmp_path):
    """5. sfrt::Ray's new members, VoxelWorld::Raycast / LRaycast / CastRays / CastShadowRays of
    include/sfrt.hpp compile and link."""
    assert _build_cpp_check(tmp_path).exists()


# ---------------------------------------------------------------- GPU helpers

@pytest.fixture(scope="module")
def vworld(built):
    import sfrt
    tex, dyn = vc.assets()
    w = sfrt.VoxelWorld(0)
    w.load_assets(tex, dyn, vs.COLORS)
    yield w
    w.close()


@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream()


def _dev(a):
    """A device copy of a float32 array (at least one element, so its pointer is not NULL)."""
    import torch
    if a is None:
        return None
    a = np.array(a, dtype=F).ravel()  # a writable copy: torch refuses read-only arrays
    t = torch.from_numpy(a if a.size else np.zeros(1, dtype=F)).to("cuda:0")
    torch.cuda.current_stream().synchronize()
    return t


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _read(bufs, n):
    """The outputs' first n elements; asserts every byte past them is still the poison."""
    out = {}
    for k, b in bufs.items():
        a = b.cpu().numpy()
        assert (a[n * ELEM[k]:] == POISON).all(), f"{k}: written past ray {n}"
        a = np.ascontiguousarray(a[:n * ELEM[k]]).view(DTYPE[k])
        out[k] = a.reshape(n, 3) if k == "pos" else a.reshape(n, 4) if k == "rgba" else a
    return out


def _status(world, stream):
    import sfrt
    try:
        world.check(stream.cuda_stream)
    except sfrt.SfrtError as e:
        return e.code
    return 0


def dev_cast(world, stream, dirs, yscales=None, origins=None, outputs=OUT, count=None):
    """sfrt_voxel_cast_rays_device on `stream` into poisoned, canaried buffers; returns
    ({name: array}, status of sfrt_voxel_check)."""
    n = len(dirs) if count is None else count
    ins = [_dev(dirs), _dev(yscales), _dev(origins)]
    bufs = {k: poisoned((n * ELEM[k] + PAD,), POISON) for k in outputs}
    world.cast_rays_device(_ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), n, stream.cuda_stream,
                           **{k: b.data_ptr() for k, b in bufs.items()})
    st = _status(world, stream)  # waits for the stream
    return _read(bufs, n), st


def dev_shadow(world, stream, o, d, md, outputs=("free", "steps"), count=None):
    n = len(md) if count is None else count
    ins = [_dev(o), _dev(d), _dev(md)]
    bufs = {k: poisoned((n * 4 + PAD,), POISON) for k in outputs}
    world.cast_shadow_rays_device(_ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), n, stream.cuda_stream,
                                  **{k: b.data_ptr() for k, b in bufs.items()})
    st = _status(world, stream)
    return _read(bufs, n), st


def _orders():
    """Row-major, 8x8-tile-major and shuffled orders of the frame's pixels."""
    row_major = np.arange(N)
    jj, ii = np.divmod(row_major, W)
    tile = np.lexsort((ii % 8, jj % 8, ii // 8, jj // 8))
    return {"row_major": row_major, "tile_major": tile,
            "shuffled": np.random.default_rng(3).permutation(N)}


# ---------------------------------------------------------------- GPU: Raycast

@pytest.mark.gpu
@pytest.mark.parametrize("name", PIN_CASES)
def test_pixel_rays_equal_the_reference_in_every_order(vworld, stream, name):
    """6. The frame's rays as a batch, in three orders (shuffled waves mix fast-path and guarded
    lanes), give the reference's six outputs; the texel status is the reference's."""
    d, ys = frame_set(name)
    want = frame_ref(name)
    vworld.set_scene(vc.scene(name), W, H)
    for what, order in _orders().items():
        got, st = dev_cast(vworld, stream, d[order], ys[order])
        assert st == (E_TEXEL if want["bad_texels"] else 0), (name, what, st)
        _assert_equal(got, {k: want[k][order] for k in OUT}, f"{name} {what}")


@pytest.mark.gpu
@pytest.mark.parametrize("own", [False, True], ids=["camera", "own_origins"])
def test_arbitrary_rays_equal_the_restatement(vworld, stream, own):
    """7. Un-normalised directions across 2^-70 .. 2^70, axis-parallel ones, random yscales; from
    the camera (with billboards) and from own origins (negative, integer, 1.5e9, the int limit)."""
    for name in (ARB_OWN if own else ARB_CAMERA):
        d, ys = arbitrary_set(name)
        want = arbitrary_ref(name, own)
        vworld.set_scene(vc.scene(name), W, H)
        got, st = dev_cast(vworld, stream, d, ys, origin_set(name) if own else None)
        assert st == (E_TEXEL if want["bad_texels"] else 0), (name, st)
        _assert_equal(got, want, name)
        # yscales NULL is 1.0f for every ray
        got1, _ = dev_cast(vworld, stream, d[:200], None, origin_set(name)[:200] if own else None)
        want1 = _ref(vc.scene(name), d[:200], None, origin_set(name)[:200] if own else None)
        _assert_equal(got1, want1, name + " yscales NULL")


@pytest.mark.gpu
@pytest.mark.parametrize("own", [False, True], ids=["camera", "own_origins"])
def test_invalid_rays_are_answered_and_disturb_nothing(vworld, stream, own):
    """8. NaN and +-inf in each component of dir, origin and yscale, interleaved inside full
    waves: the defined answers, the neighbours as in the same batch without them, no status bit
    (random_3's arbitrary rays read no texel outside a texture: asserted on the reference side)."""
    name = "random_3"
    d, ys = (a.copy() for a in arbitrary_set(name))
    o = origin_set(name).copy() if own else None
    vworld.set_scene(vc.scene(name), W, H)
    clean, st = dev_cast(vworld, stream, d, ys, o)
    assert st == 0
    bad_vals = [np.nan, np.inf, -np.inf]
    fields = [(d, 0), (d, 1), (d, 2), (ys, None)] + ([(o, 0), (o, 1), (o, 2)] if own else [])
    at = 5  # every 11th ray from here: several per wave, waves 0..
    hit = []
    for arr, c in fields:
        for v in bad_vals:
            if c is None:
                arr[at] = v
            else:
                arr[at, c] = v
            hit.append(at)
            at += 11
    hit = np.array(hit)
    assert hit.max() < 64 * 6 and np.unique(hit // 64).size >= 2
    got, st = dev_cast(vworld, stream, d, ys, o)
    assert st == 0
    want = _ref(vc.scene(name), d, ys, o)
    assert not want["valid"][hit].any() and want["valid"].sum() == N - hit.size
    _assert_equal(got, want, "with invalid rays")
    assert (got["face"][hit] == 0).all() and (got["cell"][hit] == -1).all()
    assert (got["steps"][hit] == 0).all() and not _bits(got["pos"][hit]).any()
    assert not _bits(got["depth"][hit]).any() and not got["rgba"][hit].any()
    ok = np.setdiff1d(np.arange(N), hit)
    _assert_equal({k: got[k][ok] for k in OUT}, {k: clean[k][ok] for k in OUT}, "neighbours")


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, N])
def test_counts_and_canaries(vworld, stream, count):
    """9. Batches of 0, 1, 63, 64, 65 and N rays write exactly `count` elements of every output
    (poisoned canaries past them), each output alone gives the same values, and rgba = NULL
    leaves the other outputs unchanged."""
    name = "random_3"
    d, ys = arbitrary_set(name)
    want = arbitrary_ref(name, False)
    vworld.set_scene(vc.scene(name), W, H)
    got, st = dev_cast(vworld, stream, d, ys, None, count=count)
    assert st == 0
    _assert_equal(got, {k: want[k][:count] for k in OUT}, f"count {count}")
    for k in OUT:
        alone, _ = dev_cast(vworld, stream, d, ys, None, outputs=(k,), count=count)
        _assert_equal(alone, {k: want[k][:count]}, f"count {count}, {k} alone")
    pick, _ = dev_cast(vworld, stream, d, ys, None, outputs=OUT[:-1], count=count)
    _assert_equal(pick, {k: want[k][:count] for k in OUT[:-1]}, f"count {count}, rgba NULL")
    o = origin_set(name)
    pick, _ = dev_cast(vworld, stream, d, ys, o, outputs=OUT[:-1], count=count)
    wo = arbitrary_ref(name, True)
    _assert_equal(pick, {k: wo[k][:count] for k in OUT[:-1]}, f"count {count}, own, rgba NULL")


# ---------------------------------------------------------------- GPU: LRaycast

@pytest.mark.gpu
def test_shadow_rays_equal_the_restatement(vworld, stream):
    """10. Random segments through the default world: free and steps."""
    vworld.set_scene(vc.scene("default"), W, H)
    got, st = dev_shadow(vworld, stream, *shadow_set())
    assert st == 0
    _assert_equal(got, shadow_ref(), "shadow rays", ("free", "steps"))


@pytest.mark.gpu
def test_shadow_ray_edge_cases(vworld, stream):
    """10. max_dist <= 0 (free, no trip), a zero direction, invalid rays (NaN, +-inf in every
    field, max_dist just above 4096) and the largest valid max_dist on a ray that starts inside a
    block (so it ends on trip 1), interleaved with ordinary rays whose answers do not change."""
    scene = vc.scene("default")
    vworld.set_scene(scene, W, H)
    o, d, md = (a[:256].copy() for a in shadow_set())
    clean, _ = dev_shadow(vworld, stream, o, d, md)
    at = iter(range(3, 256, 7))
    special = {}
    for v in (0.0, -0.0, -1.0, -64.0):
        k = next(at); md[k] = v; special[k] = (1, 0)
    k = next(at); d[k] = 0.0
    zero_dir = k
    invalid = []
    for arr, cols in ((o, 3), (d, 3), (md, 1)):
        for c in range(cols):
            for v in (np.nan, np.inf, -np.inf):
                k = next(at)
                if cols == 1:
                    arr[k] = v
                else:
                    arr[k, c] = v
                invalid.append(k)
    k = next(at); md[k] = np.nextafter(F(4096.0), F(np.inf)); invalid.append(k)
    k = next(at); md[k] = F(4096.0); o[k] = (0.5, 0.5, 0.5)   # inside the floor's corner block
    assert scene.blocks[0, 0, 0] != vs.EMPTY
    special[k] = (0, 1)
    got, st = dev_shadow(vworld, stream, o, d, md)
    assert st == 0
    want = vrr.shadow_rays(scene, o, d, md)
    _assert_equal(got, want, "edge cases", ("free", "steps"))
    for k, (fr, stp) in special.items():
        assert (got["free"][k], got["steps"][k]) == (fr, stp), k
    assert (got["free"][invalid] == -1).all() and (got["steps"][invalid] == 0).all()
    assert got["free"][zero_dir] in (0, 1)
    touched = np.array(list(special) + invalid + [zero_dir])
    ok = np.setdiff1d(np.arange(256), touched)
    _assert_equal({k: got[k][ok] for k in got}, {k: clean[k][ok] for k in got}, "neighbours")


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, N])
def test_shadow_counts_and_canaries(vworld, stream, count):
    """10. Counts and canaries as for cast_rays; each output alone."""
    vworld.set_scene(vc.scene("default"), W, H)
    want = shadow_ref()
    got, _ = dev_shadow(vworld, stream, *shadow_set(), count=count)
    _assert_equal(got, {k: want[k][:count] for k in got}, f"count {count}")
    for k in ("free", "steps"):
        alone, _ = dev_shadow(vworld, stream, *shadow_set(), outputs=(k,), count=count)
        _assert_equal(alone, {k: want[k][:count]}, f"count {count}, {k} alone")


# ---------------------------------------------------------------- GPU: host calls, streams, snapshots

@pytest.mark.gpu
def test_host_calls_equal_the_device_calls(vworld, stream):
    """11. sfrt_voxel_cast_rays and sfrt_voxel_cast_shadow_rays (staged through the world's
    buffers, grown on demand: a small batch, the whole, a small one again)."""
    name = "random_3"
    d, ys = arbitrary_set(name)
    o = origin_set(name)
    vworld.set_scene(vc.scene(name), W, H)
    for n in (100, N, 65):
        for own in (False, True):
            want = arbitrary_ref(name, own)
            got = vworld.cast_rays(d[:n], ys[:n], o[:n] if own else None)
            _assert_equal(got, {k: want[k][:n] for k in OUT}, f"host cast_rays {n} own={own}")
        got = vworld.cast_rays(d[:n], ys[:n], None, outputs=("face", "cell"))
        assert set(got) == {"face", "cell"}
        _assert_equal(got, {k: arbitrary_ref(name, False)[k][:n] for k in got}, f"host picking {n}")
    vworld.set_scene(vc.scene("default"), W, H)
    so, sd, smd = shadow_set()
    for n in (100, N, 65):
        got = vworld.cast_shadow_rays(so[:n], sd[:n], smd[:n])
        _assert_equal(got, {k: shadow_ref()[k][:n] for k in got}, f"host shadow rays {n}")
    assert vworld.cast_rays(d[:0], None, None)["face"].size == 0
    assert vworld.cast_shadow_rays(so[:0], sd[:0], smd[:0], outputs=("free",))["free"].size == 0


@pytest.mark.gpu
def test_two_streams_each_get_their_own_batch(vworld):
    """11. Two batches queued on two streams before either is waited for."""
    import torch
    name = "random_3"
    d, ys = arbitrary_set(name)
    want = arbitrary_ref(name, False)
    vworld.set_scene(vc.scene(name), W, H)
    halves = [(0, 2000), (2000, N)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    keep = []
    for (a, b), s in zip(halves, streams):
        ins = [_dev(d[a:b]), _dev(ys[a:b])]
        bufs = {k: poisoned(((b - a) * ELEM[k] + PAD,), POISON) for k in OUT}
        vworld.cast_rays_device(ins[0].data_ptr(), ins[1].data_ptr(), 0, b - a, s.cuda_stream,
                                **{k: t.data_ptr() for k, t in bufs.items()})
        keep.append((ins, bufs))
    for (a, b), s, (_, bufs) in zip(halves, streams, keep):
        assert _status(vworld, s) == 0
        _assert_equal(_read(bufs, b - a), {k: want[k][a:b] for k in OUT}, f"stream of rays {a}..{b}")


@pytest.mark.gpu
def test_queued_batch_keeps_the_camera_and_blocks_of_its_call(vworld, stream):
    """11. The scene, camera and view distances are snapshotted at the call: set_blocks (an
    empty world) and another camera right after a queued batch change nothing of its answers."""
    name = "random_3"
    d, ys = arbitrary_set(name)
    want = arbitrary_ref(name, False)
    vworld.set_scene(vc.scene(name), W, H)
    ins = [_dev(d), _dev(ys)]
    bufs = {k: poisoned((N * ELEM[k] + PAD,), POISON) for k in OUT}
    vworld.cast_rays_device(ins[0].data_ptr(), ins[1].data_ptr(), 0, N, stream.cuda_stream,
                            **{k: t.data_ptr() for k, t in bufs.items()})
    so, sd, smd = (_dev(a) for a in shadow_set())
    sb = {k: poisoned((N * 4 + PAD,), POISON) for k in ("free", "steps")}
    vworld.cast_shadow_rays_device(so.data_ptr(), sd.data_ptr(), smd.data_ptr(), N, stream.cuda_stream,
                                   **{k: t.data_ptr() for k, t in sb.items()})
    vworld.set_scene(vc.scene("default"), W, H)  # camera, view distances, blocks, dynamics, lights
    assert _status(vworld, stream) == 0
    _assert_equal(_read(bufs, N), want, "queued batch")
    _assert_equal(_read(sb, N), vrr.shadow_rays(vc.scene(name), *shadow_set()), "queued shadow batch",
                  ("free", "steps"))
    # and the next batches see the new world
    got, _ = dev_cast(vworld, stream, *arbitrary_set("default"))
    _assert_equal(got, arbitrary_ref("default", False), "after set_scene")
    got, _ = dev_shadow(vworld, stream, *shadow_set())
    _assert_equal(got, shadow_ref(), "shadow rays after set_scene", ("free", "steps"))


# ---------------------------------------------------------------- GPU: errors and status

@pytest.mark.gpu
def test_argument_errors_write_nothing(vworld, stream):
    """12. SFRT_E_INVALID for every listed argument error, with the outputs untouched."""
    import sfrt
    L = sfrt.lib()
    vworld.set_scene(vc.scene("default"), W, H)
    d, ys = arbitrary_set("default")
    dd, dy = _dev(d[:64]), _dev(ys[:64])
    bufs = {k: poisoned((64 * ELEM[k] + PAD,), POISON) for k in OUT}
    hits = sfrt.VoxelRayHits(**{k: b.data_ptr() for k, b in bufs.items()})
    s = ctypes.c_void_p(stream.cuda_stream)
    h, ref = vworld._h, ctypes.byref(hits)
    P = ctypes.c_void_p
    assert L.sfrt_voxel_cast_rays_device(h, None, P(dy.data_ptr()), None, 64, ref, s) == E_INVALID
    assert L.sfrt_voxel_cast_rays_device(h, P(dd.data_ptr()), None, None, -1, ref, s) == E_INVALID
    assert L.sfrt_voxel_cast_rays_device(h, P(dd.data_ptr()), None, None, 1 << 31, ref, s) == E_INVALID
    assert L.sfrt_voxel_cast_rays_device(h, P(dd.data_ptr() + 2), None, None, 8, ref, s) == E_INVALID
    assert L.sfrt_voxel_cast_rays_device(h, P(dd.data_ptr()), P(dy.data_ptr() + 1), None, 8, ref, s) == E_INVALID
    assert L.sfrt_voxel_cast_rays_device(h, P(dd.data_ptr()), None, P(dd.data_ptr() + 3), 8, ref, s) == E_INVALID
    assert L.sfrt_voxel_cast_rays_device(h, P(dd.data_ptr()), None, None, 8, None, s) == E_INVALID
    none = sfrt.VoxelRayHits()
    assert L.sfrt_voxel_cast_rays_device(h, P(dd.data_ptr()), None, None, 8, ctypes.byref(none), s) == E_INVALID
    odd = sfrt.VoxelRayHits(rgba=bufs["rgba"].data_ptr() + 1)
    assert L.sfrt_voxel_cast_rays_device(h, P(dd.data_ptr()), None, None, 8, ctypes.byref(odd), s) == E_INVALID
    fr, stp = P(bufs["cell"].data_ptr()), P(bufs["steps"].data_ptr())
    a = P(dd.data_ptr())
    assert L.sfrt_voxel_cast_shadow_rays_device(h, None, a, P(dy.data_ptr()), 8, fr, stp, s) == E_INVALID
    assert L.sfrt_voxel_cast_shadow_rays_device(h, a, None, P(dy.data_ptr()), 8, fr, stp, s) == E_INVALID
    assert L.sfrt_voxel_cast_shadow_rays_device(h, a, a, None, 8, fr, stp, s) == E_INVALID
    assert L.sfrt_voxel_cast_shadow_rays_device(h, a, a, P(dy.data_ptr()), -1, fr, stp, s) == E_INVALID
    assert L.sfrt_voxel_cast_shadow_rays_device(h, a, a, P(dy.data_ptr()), 1 << 31, fr, stp, s) == E_INVALID
    assert L.sfrt_voxel_cast_shadow_rays_device(h, a, a, P(dy.data_ptr()), 8, None, None, s) == E_INVALID
    assert L.sfrt_voxel_cast_shadow_rays_device(h, a, a, P(dy.data_ptr() + 2), 8, fr, stp, s) == E_INVALID
    assert L.sfrt_voxel_cast_shadow_rays_device(h, a, a, P(dy.data_ptr()), 8, P(fr.value + 1), stp, s) == E_INVALID
    # the host calls share the checks
    host = np.full(64, POISON, dtype=np.uint8)
    hh = sfrt.VoxelRayHits(face=host.ctypes.data)
    assert L.sfrt_voxel_cast_rays(h, None, None, None, 4, ctypes.byref(hh)) == E_INVALID
    assert L.sfrt_voxel_cast_rays(h, d.ctypes.data, None, None, -1, ctypes.byref(hh)) == E_INVALID
    assert L.sfrt_voxel_cast_shadow_rays(h, d.ctypes.data, d.ctypes.data, None, 4, host.ctypes.data, None) == E_INVALID
    assert _status(vworld, stream) == 0
    assert (host == POISON).all()
    for k, b in bufs.items():
        assert (b.cpu().numpy() == POISON).all(), k


@pytest.mark.gpu
def test_empty_world_is_refused(built, stream):
    """12. SFRT_E_EMPTY without blocks, from all four calls; count == 0 is SFRT_OK even then."""
    import sfrt
    d, ys = arbitrary_set("default")
    with sfrt.VoxelWorld(0) as w:
        with pytest.raises(sfrt.SfrtError) as e:
            w.cast_rays(d[:8], ys[:8])
        assert e.value.code == E_EMPTY
        with pytest.raises(sfrt.SfrtError) as e:
            w.cast_shadow_rays(d[:8], d[:8], ys[:8])
        assert e.value.code == E_EMPTY
        dd, dy = _dev(d[:8]), _dev(ys[:8])
        buf = poisoned((8 * 4 + PAD,), POISON)
        with pytest.raises(sfrt.SfrtError) as e:
            w.cast_rays_device(dd.data_ptr(), 0, 0, 8, stream.cuda_stream, face=buf.data_ptr())
        assert e.value.code == E_EMPTY
        with pytest.raises(sfrt.SfrtError) as e:
            w.cast_shadow_rays_device(dd.data_ptr(), dd.data_ptr(), dy.data_ptr(), 8, stream.cuda_stream,
                                      free=buf.data_ptr())
        assert e.value.code == E_EMPTY
        w.cast_rays_device(dd.data_ptr(), 0, 0, 0, stream.cuda_stream, face=buf.data_ptr())
        stream.synchronize()
        assert (buf.cpu().numpy() == POISON).all()


@pytest.mark.gpu
def test_texel_status(vworld, stream):
    """12. A read outside a texture: the host call returns SFRT_E_TEXEL and writes no output; the
    device call writes the defined outputs and reports it through sfrt_voxel_check."""
    import sfrt
    name = "negative_coordinates"
    d, ys = frame_set(name)
    want = frame_ref(name)
    assert want["bad_texels"] > 0
    vworld.set_scene(vc.scene(name), W, H)
    host = {k: np.full((N, 3) if k == "pos" else (N, 4) if k == "rgba" else (N,), POISON,
                       dtype=np.uint8 if k == "rgba" else DTYPE[k]) for k in OUT}
    before = {k: v.copy() for k, v in host.items()}
    hits = sfrt.VoxelRayHits(**{k: v.ctypes.data for k, v in host.items()})
    rc = sfrt.lib().sfrt_voxel_cast_rays(vworld._h, d.ctypes.data, ys.ctypes.data, None, N,
                                         ctypes.byref(hits))
    assert rc == E_TEXEL
    for k in OUT:
        assert np.array_equal(_bits(host[k]), _bits(before[k])), k
    got, st = dev_cast(vworld, stream, d, ys)
    assert st == E_TEXEL
    _assert_equal(got, want, name)
    assert _status(vworld, stream) == 0  # reported once


# ---------------------------------------------------------------- GPU: the tile-order chain

@pytest.mark.gpu
def test_batches_leave_the_tile_order_chain_alone(built, stream):
    """13. With SFRT_OPT_TILE_ORDER on, batches between sfrt_voxel_render_band calls leave the
    frames' bytes as they are without the batches.  The chain's recorded costs are not readable
    through the ABI; they are held to this: a chain run with batches in between produces, frame
    for frame, the bytes of a chain run without them -- the third frame of each is the first
    dispatched in the order sorted from the first frame's recorded costs."""
    import sfrt
    name = "default_turned"
    d, ys = frame_set(name)
    tex, dyn = vc.assets()

    def chain(with_batches):
        frames = []
        with sfrt.VoxelWorld(0) as w:
            w.load_assets(tex, dyn, vs.COLORS)
            w.set_scene(vc.scene(name), W, H)
            w.set_option(sfrt.SFRT_OPT_TILE_ORDER, 1)
            for _ in range(4):
                buf = poisoned((H, 4 * W), POISON)
                w.render_band(buf.data_ptr(), 4 * W, 0, H, stream.cuda_stream)
                if with_batches:
                    got, st = dev_cast(w, stream, d, ys)
                    assert st == 0
                    sg, _ = dev_shadow(w, stream, *shadow_set(), count=640)
                    w.cast_rays(d[:100], ys[:100], outputs=("face",))
                assert _status(w, stream) == 0
                frames.append(buf.cpu().numpy().copy())
            assert w.get_option(sfrt.SFRT_OPT_TILE_ORDER) == 1
        return frames, (got if with_batches else None)

    plain, _ = chain(False)
    mixed, got = chain(True)
    for k, (a, b) in enumerate(zip(plain, mixed)):
        assert np.array_equal(a, b), f"frame {k}"
    assert np.array_equal(plain[0].reshape(N, 4), frame_ref(name)["rgba"])
    assert np.array_equal(got["rgba"], frame_ref(name)["rgba"])


# ---------------------------------------------------------------- GPU: the C++ mirror

@pytest.mark.gpu
def test_cpp_voxel_raycast_runs(built, tmp_path):
    """14. tests/native/cpp_voxel_raycast_check.cpp: Raycast(Ray*) of a pixel's ray gives the
    frame's pixel, CastRays the same, LRaycast both answers."""
    exe = _build_cpp_check(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "failures=0" in r.stdout, r.stdout + r.stderr
