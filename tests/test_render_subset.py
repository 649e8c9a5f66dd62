"""UpdateImage's pixel subsets in place in a device-resident frame (include/sfrt.h
sfrt_world_render_subset, sfrt_voxel_render_subset and their _aux forms).

Every comparison is byte for byte.  The reference of the colour is the oracle's own
update_image into a poisoned host canvas with the same arguments (supersampled: the box filter of
the oracle's S*W x S*H frame, tests/test_supersample.py::reference); the reference of the planes
is the host update_image_aux, which tests/test_aux_planes.py and tests/test_voxel_aux.py pin to
the oracle.  Device canvases are poisoned with 0xA5 and have padded pitches: a whole canvas,
padding included, must equal the poisoned host canvas the reference wrote into.

Frames: 45x23 (ragged against the 8- and the 32-pixel tile widths), 100x37 for the list kernels,
64x36 for the voxel world.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import scenes
import voxel_scenes as vs
from conftest import ROOT, host_threads, poisoned
from test_supersample import reference as filtered_reference

pytestmark = pytest.mark.gpu

POISON = 0xA5
E_INVALID, E_EMPTY, E_NO_TEXTURE = -1, -2, -3
W, H, PAD = 45, 23, 32
LW, LH = 100, 37  # the list kernels' frame
# (ystart, yadd, xstart, xadd)
SUBSETS = [(0, 8, 0, 4), (3, 8, 2, 4), (7, 8, 3, 4), (1, 3, 0, 1), (0, 1, 5, 7), (22, 1, 44, 1),
           (5, 1000, 0, 1), (0, 1, 45, 1)]
SS_SUBSETS = [(1, 3, 2, 4), (0, 1, 0, 1), (0, 1, 3, 1000)]
CYCLE_POSES = [(0.7, 0.3), (0.74, 0.31), (0.79, 0.29), (0.85, 0.33)]
PHASES = [0, 3, 2, 1]  # cycle = (cycle + 3) % 4 from 0 (Source.cpp:23)
PLANES = ("depth", "sphere", "steps")
DTYPES = {"depth": np.float32, "sphere": np.int32, "steps": np.int32}
PLANE_PADS = {"depth": 4, "sphere": 8, "steps": 12}


@functools.lru_cache(maxsize=None)
def _floor():
    tex, tw, th = scenes.load_floor()
    tex = np.array(tex, dtype=np.uint8).ravel()
    tex.setflags(write=False)
    return tex, tw, th


@functools.lru_cache(maxsize=None)
def _scene(name, pose=(0.7, 0.3)):
    if name == "lcg65":
        sc = scenes.Scene(name, scenes.sort_spheres(scenes.lcg_spheres(count=64)))
    elif name == "lcg199":
        sc = scenes.Scene(name, scenes.sort_spheres(scenes.lcg_spheres(count=198)))
    else:
        sc = scenes.SCENES[name]()
    return sc.posed(*pose)


def _size(name):
    return (W, H) if name == "default10" else (LW, LH)


def _subsets(name):
    """SUBSETS, plus at the list kernels' frame size its own last pixel and its own empty subset."""
    w, h = _size(name)
    return SUBSETS if (w, h) == (W, H) else SUBSETS + [(h - 1, 1, w - 1, 1), (0, 1, w, 1)]


@functools.lru_cache(maxsize=None)
def _oracle(name, pose=(0.7, 0.3), tex=None):
    import oracle
    w, h = _size(name)
    return oracle.Oracle.from_scene(_scene(name, pose), w, h, *(_floor() if tex is None else tex))


@functools.lru_cache(maxsize=None)
def oracle_canvas(name, subset):
    """The poisoned (h, 4w) host canvas after Oracle.update_image(*subset); shared, read-only."""
    w, h = _size(name)
    canvas = np.full((h, 4 * w), POISON, dtype=np.uint8)
    _oracle(name).update_image(canvas, *subset)
    canvas.setflags(write=False)
    return canvas


def _world(name, pose=(0.7, 0.3), s=1):
    import sfrt
    w = sfrt.World(0)
    w.load_texture(*_floor())
    w.set_scene(_scene(name, pose), *_size(name))
    w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
    return w


@pytest.fixture(scope="module")
def stream(built):
    import torch
    return torch.cuda.Stream()


def _assert_canvas(dev, want, what=""):
    """The device canvas (rows, pitch) equals `want` (rows, 4w) and its padding is poison."""
    got = dev.cpu().numpy()
    n = want.shape[1]
    bad = np.argwhere(got[:, :n] != want)
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} bytes differ, first (row, byte) {tuple(bad[0])}"
    assert (got[:, n:] == POISON).all(), f"{what}: padding written"


def _addressed(subset, w, h):
    ystart, yadd, xstart, xadd = subset
    m = np.zeros((h, w), dtype=bool)
    m[ystart::yadd, xstart::xadd] = True
    return m


# ---------------------------------------------------------------- 1: addressed pixels only

@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("rays", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("name", ["default10", "lcg65", "lcg199"])
def test_addressed_pixels_only(stream, name, rays, cull):
    """Every subset into its own poisoned canvas of pitch 4w + 32: the whole canvas equals the
    oracle's.  rays 0 is the kernel table's own choice; 65 and 199 spheres run the list kernels."""
    import sfrt
    w, h = _size(name)
    pitch = 4 * w + PAD
    with _world(name) as world:
        world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
        world.set_option(sfrt.SFRT_OPT_CULL, cull)
        subsets = _subsets(name)
        canvases = poisoned((len(subsets), h, pitch), POISON)
        for k, sub in enumerate(subsets):
            world.render_subset(canvases[k].data_ptr(), pitch, *sub, stream=stream.cuda_stream)
        world.check(stream.cuda_stream)
        for k, sub in enumerate(subsets):
            _assert_canvas(canvases[k], oracle_canvas(name, sub), f"{name} {sub}")
    # the last subset addresses nothing, the others something
    assert (oracle_canvas(name, subsets[-1]) == POISON).all()
    assert all((oracle_canvas(name, s) != POISON).any() for s in subsets[:-1])


def test_strides_up_to_int_max(stream, vworld):
    """A stride of INT_MAX addresses the start pixel alone, as any stride past the frame does."""
    big = 2 ** 31 - 1
    pitch = 4 * W + PAD
    with _world("default10") as world:
        dev = poisoned((H, pitch), POISON)
        world.render_subset(dev.data_ptr(), pitch, 2, big, 3, big, stream.cuda_stream)
        world.check(stream.cuda_stream)
        _assert_canvas(dev, oracle_canvas("default10", (2, 1000, 3, 1000)), "INT_MAX strides")
    vworld.set_scene(vs.default_world(*VOXEL_POSE), VW, VH)
    vpitch = 4 * VW + PAD
    dev = poisoned((VH, vpitch), POISON)
    vworld.render_subset(dev.data_ptr(), vpitch, 2, big, 3, big, stream.cuda_stream)
    vworld.check(stream.cuda_stream)
    _assert_canvas(dev, voxel_canvas((2, 1000, 3, 1000)), "voxel INT_MAX strides")


# ---------------------------------------------------------------- 2: a full cycle, moving camera

@functools.lru_cache(maxsize=None)
def cycle_canvas():
    """The canvas after the four column phases, each with its own camera pose."""
    canvas = np.full((H, 4 * W), POISON, dtype=np.uint8)
    for pose, c in zip(CYCLE_POSES, PHASES):
        _oracle("default10", pose).update_image(canvas, 0, 1, c, 4)
    assert not (canvas.reshape(H, W, 4) == POISON).all(axis=-1).any()
    canvas.setflags(write=False)
    return canvas


@pytest.mark.parametrize("row_phases", [1, 8])
def test_full_cycle_with_a_moving_camera(stream, row_phases):
    """Phases 0, 3, 2, 1 with four poses on one stream (and the same as 8 row phases x 4 column
    phases, 32 calls): the canvas the four oracle calls leave; no poisoned pixel remains."""
    pitch = 4 * W + PAD
    with _world("default10") as world:
        dev = poisoned((H, pitch), POISON)
        for pose, c in zip(CYCLE_POSES, PHASES):
            world.set_scene(_scene("default10", pose), W, H)
            for r in range(row_phases):
                world.render_subset(dev.data_ptr(), pitch, r, row_phases, c, 4, stream.cuda_stream)
        world.check(stream.cuda_stream)
        _assert_canvas(dev, cycle_canvas(), f"{row_phases} row phases")
        px = dev.cpu().numpy()[:, :4 * W].reshape(H, W, 4)
        assert not (px == POISON).all(axis=-1).any()


# ---------------------------------------------------------------- 3: supersampled

@pytest.mark.parametrize("s", [2, 4])
def test_supersampled(stream, s):
    """Addressed pixels are the box filter of the oracle's S*W x S*H frame, all others untouched;
    (0, 1, 3, 1000) addresses one column, whose stride is not scaled."""
    want_frame = filtered_reference("default10", s, (0.7, 0.3), W, H)
    pitch = 4 * W + PAD
    with _world("default10", s=s) as world:
        for sub in SS_SUBSETS:
            dev = poisoned((H, pitch), POISON)
            world.render_subset(dev.data_ptr(), pitch, *sub, stream=stream.cuda_stream)
            world.check(stream.cuda_stream)
            want = np.full((H, W, 4), POISON, dtype=np.uint8)
            m = _addressed(sub, W, H)
            want[m] = want_frame[m]
            _assert_canvas(dev, want.reshape(H, 4 * W), f"S={s} {sub}")
    assert int(_addressed(SS_SUBSETS[2], W, H).sum()) == H  # one column


# ---------------------------------------------------------------- 4: planes

class Planes:
    """Poisoned whole-frame device planes, each with its own padded pitch."""

    def __init__(self, names, dtypes, pads, w, h):
        self.w, self.h, self.dtypes = w, h, dtypes
        self.pitch = {p: 4 * w + pads[p] for p in names}
        self.buf = {p: poisoned((h, self.pitch[p]), POISON) for p in names}

    def args(self):
        return {p: (b.data_ptr(), self.pitch[p]) for p, b in self.buf.items()}


def _host_planes(names, dtypes, w, h):
    return {p: np.full((h, 4 * w), POISON, dtype=np.uint8).view(dtypes[p]) for p in names}


@pytest.mark.parametrize("name,rays,s", [("default10", 0, 1), ("lcg65", 0, 1), ("default10", 4, 1),
                                         ("default10", 4, 2), ("lcg65", 4, 4), ("lcg65", 2, 2)])
def test_planes(stream, name, rays, s):
    """Each subset of test 1, the empty one included: every plane equals the host
    update_image_aux's poisoned plane (addressed elements written, the rest and the padding
    untouched; an empty subset writes nothing and returns SFRT_OK), the colour equals the host
    call's and, at S = 1, the oracle's.  Beyond the kernel table's own choice at S = 1: four pixels
    per lane (the 74-VGPR plane-writing kernels) and S = 2, 4, where the group's leader lane
    stores its first sample's values."""
    import sfrt
    w, h = _size(name)
    pitch = 4 * w + PAD
    with _world(name, s=s) as world:
        world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
        for sub in _subsets(name):
            planes = Planes(PLANES, DTYPES, PLANE_PADS, w, h)
            dev = poisoned((h, pitch), POISON)
            world.render_subset_aux(dev.data_ptr(), pitch, *sub, stream=stream.cuda_stream,
                                    **planes.args())
            world.check(stream.cuda_stream)
            host_rgba = np.full((h, 4 * w), POISON, dtype=np.uint8)
            host = _host_planes(PLANES, DTYPES, w, h)
            world.update_image_aux(host_rgba, *(host[p] for p in PLANES), *sub)
            for p in PLANES:
                _assert_canvas(planes.buf[p], host[p].view(np.uint8), f"{name} {sub} {p}")
            _assert_canvas(dev, host_rgba, f"{name} {sub} colour")
            if s == 1:
                assert np.array_equal(host_rgba, oracle_canvas(name, sub))
            if not _addressed(sub, w, h).any():
                assert bool((dev == POISON).all())
                assert all(bool((b == POISON).all()) for b in planes.buf.values())
    assert not _addressed(_subsets(name)[-1], w, h).any()


def test_null_planes_and_plane_refusals(stream):
    """A NULL plane is never written (its pitch is ignored); all-NULL, a pitch that is no multiple
    of 4 and a pitch below 4w are refused with every target untouched."""
    import sfrt
    sub = (3, 8, 2, 4)
    pitch = 4 * W + PAD
    with _world("default10") as world:
        host = _host_planes(PLANES, DTYPES, W, H)
        world.update_image_aux(np.full((H, 4 * W), POISON, dtype=np.uint8),
                               *(host[p] for p in PLANES), *sub)
        for wanted in [(p,) for p in PLANES] + [tuple(q for q in PLANES if q != p) for p in PLANES]:
            planes = Planes(wanted, DTYPES, PLANE_PADS, W, H)
            guard = poisoned((H, pitch), POISON)
            dev = poisoned((H, pitch), POISON)
            world.render_subset_aux(dev.data_ptr(), pitch, *sub, stream=stream.cuda_stream,
                                    **planes.args())
            world.check(stream.cuda_stream)
            for p in wanted:
                _assert_canvas(planes.buf[p], host[p].view(np.uint8), f"{wanted} {p}")
            _assert_canvas(dev, oracle_canvas("default10", sub), str(wanted))
            assert bool((guard == POISON).all())
        dev = poisoned((H, pitch), POISON)
        plane = poisoned((H, pitch), POISON)
        for kw in ({}, {"depth": (plane.data_ptr(), pitch + 2)}, {"steps": (plane.data_ptr(), 4 * W - 4)}):
            with pytest.raises(sfrt.SfrtError) as e:
                world.render_subset_aux(dev.data_ptr(), pitch, *sub, stream=stream.cuda_stream, **kw)
            assert e.value.code == E_INVALID, kw
        # a NULL aux record, which the Python wrapper never passes: the C entry point itself
        L = sfrt.lib()
        for sb in (sub, SUBSETS[-1]):
            assert L.sfrt_world_render_subset_aux(world._h, dev.data_ptr(), pitch, None, *sb,
                                                  stream.cuda_stream) == E_INVALID
        world.check(stream.cuda_stream)
        assert bool((dev == POISON).all()) and bool((plane == POISON).all())


# ---------------------------------------------------------------- 5: state is left alone

def _three_bands(world, stream, interpose):
    pitch = 4 * LW + 16
    bufs = [poisoned((LH, pitch), POISON) for _ in range(3)]
    side = poisoned((LH, pitch), POISON)
    for k, b in enumerate(bufs):
        world.render_band(b.data_ptr(), pitch, 0, LH, stream.cuda_stream)
        if interpose and k == 0:
            world.render_subset(side.data_ptr(), pitch, 0, 1, 3, 4, stream.cuda_stream)
    world.check(stream.cuda_stream)
    return [b.cpu().numpy() for b in bufs]


def test_state_is_left_alone(stream):
    """Ray-cache counters, the frames of the adaptive order and row_costs are the same with and
    without a render_subset between the bands."""
    with _world("lcg65") as a, _world("lcg65") as b:
        plain = _three_bands(a, stream, False)
        mixed = _three_bands(b, stream, True)
        for x, y in zip(plain, mixed):
            assert np.array_equal(x, y)
        assert a.ray_cache_stats() == b.ray_cache_stats()
        r0a, ca = a.row_costs()
        r0b, cb = b.row_costs()
        assert r0a == r0b and np.array_equal(ca, cb) and ca.size == LH
        before = b.ray_cache_stats()
        dev = poisoned((LH, 4 * LW), POISON)
        b.render_subset(dev.data_ptr(), 4 * LW, 0, 8, 0, 4, stream.cuda_stream)
        b.check(stream.cuda_stream)
        assert b.ray_cache_stats() == before
        r0c, cc = b.row_costs()
        assert r0c == r0b and np.array_equal(cc, cb)


# ---------------------------------------------------------------- 6: ordering behind a texture upload

def test_ordered_behind_the_texture_upload(stream):
    """load_texture with another texture, then render_subset on a non-default stream and
    check(stream): the new texture's bytes."""
    import oracle
    tex, tw, th = _floor()
    other = tex.copy()
    other[0::4] = 255 - other[0::4]
    other[1::4] = other[1::4] // 2
    sub = (0, 1, 1, 4)
    want = np.full((H, 4 * W), POISON, dtype=np.uint8)
    oracle.Oracle.from_scene(_scene("default10"), W, H, other, tw, th).update_image(want, *sub)
    assert not np.array_equal(want, oracle_canvas("default10", sub))
    pitch = 4 * W + PAD
    with _world("default10") as world:
        world.render()  # the first texture in use
        dev = poisoned((H, pitch), POISON)
        world.load_texture(other, tw, th)
        world.render_subset(dev.data_ptr(), pitch, *sub, stream=stream.cuda_stream)
        world.check(stream.cuda_stream)
        _assert_canvas(dev, want, "new texture")


# ---------------------------------------------------------------- 7: refusals

def test_refusals(stream):
    import sfrt
    pitch = 4 * W + PAD
    dev = poisoned((H, pitch), POISON)
    p = dev.data_ptr()
    with _world("default10") as world:
        bad = [(0, pitch, (-1, 1, 0, 1)), (0, pitch, (0, 1, -1, 1)), (0, pitch, (0, 0, 0, 1)),
               (0, pitch, (0, -2, 0, 1)), (0, pitch, (0, 1, 0, 0)), (0, pitch, (0, 1, 0, -1)),
               (0, pitch + 2, (0, 1, 0, 1)), (0, 4 * W - 4, (0, 1, 0, 1)), (1, pitch, (0, 1, 0, 1))]
        for null_frame, pb, sub in bad:
            with pytest.raises(sfrt.SfrtError) as e:
                world.render_subset(0 if null_frame else p, pb, *sub, stream=stream.cuda_stream)
            assert e.value.code == E_INVALID, (null_frame, pb, sub)
            with pytest.raises(sfrt.SfrtError) as e:
                world.render_subset_aux(0 if null_frame else p, pb, *sub, stream=stream.cuda_stream,
                                        depth=(p, pitch))
            assert e.value.code == E_INVALID, (null_frame, pb, sub)
        # an empty subset: SFRT_OK, nothing queued
        world.render_subset(p, pitch, H, 1, 0, 1, stream.cuda_stream)
        world.render_subset(p, pitch, 0, 1, W, 1, stream.cuda_stream)
        world.check(stream.cuda_stream)
    with sfrt.World(0) as world:  # no texture, then no sphere
        world.set_scene(_scene("default10"), W, H)
        with pytest.raises(sfrt.SfrtError) as e:
            world.render_subset(p, pitch, 0, 1, 0, 1, stream.cuda_stream)
        assert e.value.code == E_NO_TEXTURE
        world.load_texture(*_floor())
        world.set_spheres(np.zeros((0, 4), dtype=np.float32))
        with pytest.raises(sfrt.SfrtError) as e:
            world.render_subset(p, pitch, 0, 1, 0, 1, stream.cuda_stream)
        assert e.value.code == E_EMPTY
        world.check(stream.cuda_stream)
    assert bool((dev == POISON).all())


# ---------------------------------------------------------------- 8: the voxel world

VW, VH = 64, 36
# the default world, looking at the sprites of World.cpp:47-53 past lamp-lit walls
VOXEL_POSE = ((13.61, 1.99, 17.3), -0.36, 0.0)
VOXEL_CYCLE = [((13.61, 1.99, 17.3), -0.36, 0.0), ((13.63, 1.99, 17.32), -0.34, 0.0),
               ((13.66, 1.98, 17.35), -0.31, 0.01), ((13.7, 1.98, 17.37), -0.29, 0.01)]
VPLANES = ("depth", "cell", "face", "steps")
VDTYPES = {"depth": np.float32, "cell": np.int32, "face": np.int32, "steps": np.int32}
VPADS = {"depth": 4, "cell": 8, "face": 20, "steps": 12}


@functools.lru_cache(maxsize=None)
def _assets():
    return vs.load_textures()


@functools.lru_cache(maxsize=None)
def _voxel_oracle(pose, s=1):
    import oracle
    tex, dyn = _assets()
    return oracle.VoxelOracle(vs.default_world(*pose), s * VW, s * VH, tex, dyn, vs.COLORS)


def _clean(fn):
    """Runs an oracle call; the inputs must be ones for which it flags no texel."""
    import oracle
    before = oracle.VoxelOracle.bad_texel_reads()
    out = fn()
    assert oracle.VoxelOracle.bad_texel_reads() == before
    return out


@functools.lru_cache(maxsize=None)
def voxel_canvas(subset, pose=VOXEL_POSE):
    canvas = np.full((VH, 4 * VW), POISON, dtype=np.uint8)
    _clean(lambda: _voxel_oracle(pose).update_image(canvas, *subset))
    canvas.setflags(write=False)
    return canvas


VOXEL_SUBSETS = [(0, 8, 0, 4), (3, 8, 2, 4), (7, 8, 3, 4), (1, 3, 0, 1), (0, 1, 5, 7),
                 (VH - 1, 1, VW - 1, 1), (5, 1000, 0, 1), (0, 1, VW, 1)]


@pytest.fixture(scope="module")
def vworld(built):
    import sfrt
    tex, dyn = _assets()
    w = sfrt.VoxelWorld(0)
    w.load_assets(tex, dyn, vs.COLORS)
    yield w
    w.close()


def test_voxel_addressed_pixels_only(vworld, stream):
    import sfrt
    vworld.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 1)
    vworld.set_scene(vs.default_world(*VOXEL_POSE), VW, VH)
    pitch = 4 * VW + PAD
    canvases = poisoned((len(VOXEL_SUBSETS), VH, pitch), POISON)
    for k, sub in enumerate(VOXEL_SUBSETS):
        vworld.render_subset(canvases[k].data_ptr(), pitch, *sub, stream=stream.cuda_stream)
    vworld.check(stream.cuda_stream)
    for k, sub in enumerate(VOXEL_SUBSETS):
        _assert_canvas(canvases[k], voxel_canvas(sub), f"voxel {sub}")
    assert (voxel_canvas(VOXEL_SUBSETS[-1]) == POISON).all()


@pytest.mark.parametrize("row_phases", [1, 8])
def test_voxel_full_cycle_with_a_moving_camera(vworld, stream, row_phases):
    import sfrt
    vworld.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 1)
    want = np.full((VH, 4 * VW), POISON, dtype=np.uint8)
    for pose, c in zip(VOXEL_CYCLE, PHASES):
        _clean(lambda: _voxel_oracle(pose).update_image(want, 0, 1, c, 4))
    pitch = 4 * VW + PAD
    dev = poisoned((VH, pitch), POISON)
    for pose, c in zip(VOXEL_CYCLE, PHASES):
        vworld.set_scene(vs.default_world(*pose), VW, VH)
        for r in range(row_phases):
            vworld.render_subset(dev.data_ptr(), pitch, r, row_phases, c, 4, stream.cuda_stream)
    vworld.check(stream.cuda_stream)
    _assert_canvas(dev, want, f"voxel cycle, {row_phases} row phases")
    px = dev.cpu().numpy()[:, :4 * VW].reshape(VH, VW, 4)
    assert not (px == POISON).all(axis=-1).any()


def test_voxel_supersampled(vworld, stream):
    import sfrt
    s = 2
    big = _clean(lambda: _voxel_oracle(VOXEL_POSE, s).render(host_threads()))
    sums = big.reshape(VH, s, VW, s, 4).astype(np.uint32).sum(axis=(1, 3))
    want_frame = ((sums + s * s // 2) >> 2).astype(np.uint8)
    vworld.set_scene(vs.default_world(*VOXEL_POSE), VW, VH)
    vworld.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
    pitch = 4 * VW + PAD
    try:
        for sub in SS_SUBSETS:
            dev = poisoned((VH, pitch), POISON)
            vworld.render_subset(dev.data_ptr(), pitch, *sub, stream=stream.cuda_stream)
            vworld.check(stream.cuda_stream)
            want = np.full((VH, VW, 4), POISON, dtype=np.uint8)
            m = _addressed(sub, VW, VH)
            want[m] = want_frame[m]
            _assert_canvas(dev, want.reshape(VH, 4 * VW), f"voxel S={s} {sub}")
    finally:
        vworld.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 1)


@pytest.mark.parametrize("s", [1, 2])
def test_voxel_planes_every_subset(vworld, stream, s):
    """The planes of every subset, the empty one included, against the host update_image_aux;
    the colour against the host call's and, at S = 1, the oracle's.  S = 2: the plane-writing
    placing kernel's leader-lane store."""
    import sfrt
    vworld.set_scene(vs.default_world(*VOXEL_POSE), VW, VH)
    vworld.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
    pitch = 4 * VW + PAD
    try:
        for sub in VOXEL_SUBSETS:
            planes = Planes(VPLANES, VDTYPES, VPADS, VW, VH)
            dev = poisoned((VH, pitch), POISON)
            vworld.render_subset_aux(dev.data_ptr(), pitch, *sub, stream=stream.cuda_stream,
                                     **planes.args())
            vworld.check(stream.cuda_stream)
            host_rgba = np.full((VH, 4 * VW), POISON, dtype=np.uint8)
            host = _host_planes(VPLANES, VDTYPES, VW, VH)
            vworld.update_image_aux(host_rgba, *(host[p] for p in VPLANES), *sub)
            for p in VPLANES:
                _assert_canvas(planes.buf[p], host[p].view(np.uint8), f"voxel S={s} {sub} {p}")
            _assert_canvas(dev, host_rgba, f"voxel S={s} {sub} colour")
            if s == 1:
                assert np.array_equal(host_rgba, voxel_canvas(sub))
            if not _addressed(sub, VW, VH).any():
                assert bool((dev == POISON).all())
                assert all(bool((b == POISON).all()) for b in planes.buf.values())
    finally:
        vworld.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 1)
    assert not _addressed(VOXEL_SUBSETS[-1], VW, VH).any()


def test_voxel_planes(vworld, stream):
    """The pose shows a billboard (face 4) and lamp-lit walls, asserted on the host planes; a NULL
    plane is never written; NULL aux, all-NULL planes, bad pitches and bad strides are refused."""
    import sfrt
    vworld.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 1)
    vworld.set_scene(vs.default_world(*VOXEL_POSE), VW, VH)
    pitch = 4 * VW + PAD
    full = _host_planes(VPLANES, VDTYPES, VW, VH)
    rgba = np.zeros((VH, 4 * VW), dtype=np.uint8)
    vworld.update_image_aux(rgba, *(full[p] for p in VPLANES))
    assert int((full["face"] == 4).sum()) >= 1  # a billboard
    walls = (full["face"] != 4) & (full["face"] != 0)
    assert int((walls & (rgba.reshape(VH, VW, 4)[..., :3].astype(int).sum(-1) > 60)).sum()) > 500
    # a NULL plane is never written; all-NULL and bad pitches are refused, nothing written
    sub = VOXEL_SUBSETS[1]
    planes = Planes(("cell",), VDTYPES, VPADS, VW, VH)
    dev = poisoned((VH, pitch), POISON)
    guard = poisoned((VH, pitch), POISON)
    vworld.render_subset_aux(dev.data_ptr(), pitch, *sub, stream=stream.cuda_stream, **planes.args())
    vworld.check(stream.cuda_stream)
    _assert_canvas(dev, voxel_canvas(sub), "voxel cell only")
    assert bool((guard == POISON).all())
    for kw in ({}, {"depth": (guard.data_ptr(), pitch + 2)}, {"face": (guard.data_ptr(), 4 * VW - 4)}):
        with pytest.raises(sfrt.SfrtError) as e:
            vworld.render_subset_aux(guard.data_ptr(), pitch, *sub, stream=stream.cuda_stream, **kw)
        assert e.value.code == E_INVALID, kw
    for sb in (sub, VOXEL_SUBSETS[-1]):  # a NULL aux record: the C entry point itself
        assert sfrt.lib().sfrt_voxel_render_subset_aux(vworld._h, guard.data_ptr(), pitch, None, *sb,
                                                       stream.cuda_stream) == E_INVALID
    for pb, bad in ((pitch, (-1, 1, 0, 1)), (pitch, (0, 0, 0, 1)), (pitch, (0, 1, -1, 1)),
                    (pitch, (0, 1, 0, 0)), (pitch + 2, sub), (4 * VW - 4, sub)):
        with pytest.raises(sfrt.SfrtError) as e:
            vworld.render_subset(guard.data_ptr(), pb, *bad, stream=stream.cuda_stream)
        assert e.value.code == E_INVALID, (pb, bad)
    vworld.check(stream.cuda_stream)
    assert bool((guard == POISON).all())


# ---------------------------------------------------------------- 9: the C++ mirror

def test_cpp_render_cycles(built, tmp_path):
    """include/sfrt.hpp's RenderCycles on both world classes (tests/native/cpp_subset_check.cpp):
    four cycles from a poisoned device frame equal UpdateImage(host, 0, 1, 0, 1); one cycle
    leaves three of the four column phases poisoned and cycle == 3."""
    exe = tmp_path / "cpp_subset_check"
    lib_dir = os.path.join(ROOT, "sfml-software-raytracer_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I",
                    os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "native", "cpp_subset_check.cpp"), "-L", lib_dir,
                    "-lsfrt", f"-Wl,-rpath,{lib_dir}", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-lpthread",
                    "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe), os.path.join(lib_dir, "assets")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "failures=0" in r.stdout, r.stdout + r.stderr
