"""The voxel frame fill's per-pixel planes (include/sfrt.h sfrt_voxel_aux_planes): depth, cell,
face and DDA steps, written by the launch that writes the colour.

The reference of every plane is tests/voxel_ref.py, the numpy binary32 restatement that
tests/test_voxel_ref.py pins to the oracle's bytes on the CPU; the colour is compared with the
oracle itself and with the plain calls.  All four planes are compared exactly, depth as uint32 bit
patterns.  Frames are 101 x 37, ragged against the 8 x 8 tile; the cases (tests/voxel_aux_cases.py)
reach every face value, the guarded DDA, a texel read outside a texture and 1..maxiter steps
(asserted on the CPU).  Supersampled, the planes are those of sample pixel (S*i, S*j).
"""
import functools

import numpy as np
import pytest

import voxel_aux_cases as vc
import voxel_ref
import voxel_scenes as vs
from conftest import host_threads, poisoned
from voxel_aux_cases import W, H

pytestmark = pytest.mark.gpu

POISON = 0xA5
PLANES = voxel_ref.PLANES
DTYPES = {"depth": np.float32, "cell": np.int32, "face": np.int32, "steps": np.int32}
PADS = {"colour": 16, "depth": 4, "cell": 8, "face": 20, "steps": 12}  # every target its own pitch
TEXEL = -7  # SFRT_E_TEXEL


@functools.lru_cache(maxsize=None)
def oracle_frame(name, s=1):
    """The oracle's colour of `name` at 101 x 37 (s > 1: the box-filtered s-times larger frame) and
    whether the reference reads outside a texture there."""
    import oracle
    tex, dyn = vc.assets()
    o = oracle.VoxelOracle(vc.scene(name), s * W, s * H, tex, dyn, vs.COLORS)
    before = oracle.VoxelOracle.bad_texel_reads()
    rgba = o.render(host_threads()).reshape(s * H, s * W, 4)
    ub = oracle.VoxelOracle.bad_texel_reads() > before
    if s > 1:
        rgba = voxel_ref.box_filter(rgba, s)
    rgba.setflags(write=False)
    return rgba, ub


@pytest.fixture(scope="module")
def vworld(built):
    import sfrt
    tex, dyn = vc.assets()
    w = sfrt.VoxelWorld(0)
    w.load_assets(tex, dyn, vs.COLORS)
    yield w
    w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 1)
    w.set_option(sfrt.SFRT_OPT_TILE_ORDER, 0)
    w.close()


@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_planes(got, want, what="", rows=slice(None)):
    for p, a in got.items():
        bad = np.argwhere(_bits(a) != _bits(want[p][rows]))
        assert bad.shape[0] == 0, (f"{what}: plane {p}: {bad.shape[0]} pixels differ, first (i, j) = "
                                   f"({bad[0][1]}, {bad[0][0]}): got {a[tuple(bad[0])]} want "
                                   f"{want[p][rows][tuple(bad[0])]}")


class Band:
    """Poisoned device targets of one render_band_aux: colour and each wanted plane, every one
    with its own padded pitch."""

    def __init__(self, rows=H, planes=PLANES):
        self.rows = rows
        self.pitch = {k: 4 * W + PADS[k] for k in ("colour",) + tuple(planes)}
        self.buf = {k: poisoned((rows, p), POISON) for k, p in self.pitch.items()}
        self.planes = tuple(planes)

    def render(self, world, stream, row0=0, rows=None, at=0):
        """Rows [row0, row0 + rows) of the frame into rows [at, at + rows) of the targets."""
        rows = self.rows if rows is None else rows
        world.render_band_aux(self.buf["colour"][at].data_ptr(), self.pitch["colour"], row0, rows,
                              stream.cuda_stream,
                              **{p: (self.buf[p][at].data_ptr(), self.pitch[p]) for p in self.planes})

    def read(self):
        """(rgba (rows, W, 4), {plane: (rows, W)}); asserts the padding of every target untouched."""
        out = {}
        for k, b in self.buf.items():
            a = b.cpu().numpy()
            assert (a[:, 4 * W:] == POISON).all(), f"{k}: padding written"
            a = np.ascontiguousarray(a[:, :4 * W])
            out[k] = a.reshape(self.rows, W, 4) if k == "colour" else \
                a.view(DTYPES[k]).reshape(self.rows, W)
        return out.pop("colour"), out


def _check(world, stream, ub):
    import sfrt
    if ub:
        with pytest.raises(sfrt.SfrtError) as e:
            world.check(stream.cuda_stream)
        assert e.value.code == TEXEL, e.value
    else:
        world.check(stream.cuda_stream)


def _plain(world, stream):
    dev = poisoned((H, W * 4), POISON)
    world.render_band(dev.data_ptr(), W * 4, 0, H, stream.cuda_stream)
    return dev


@pytest.mark.parametrize("name", vc.NAMES)
def test_whole_frame_all_planes(vworld, stream, name):
    """All four planes of every case equal voxel_ref's, each over its own padded pitch with the
    padding untouched; the colour equals the plain render_band's bytes and the oracle's."""
    want_rgba, ub = oracle_frame(name)
    vworld.set_scene(vc.scene(name), W, H)
    band = Band()
    band.render(vworld, stream)
    _check(vworld, stream, ub)
    plain = _plain(vworld, stream)
    _check(vworld, stream, ub)
    rgba, got = band.read()
    _assert_planes(got, vc.reference(name), name)
    assert np.array_equal(rgba, plain.cpu().numpy().reshape(H, W, 4)), name
    assert np.array_equal(rgba, want_rgba), name


def test_null_combinations(vworld, stream):
    """Each plane alone and each plane left out: the same values; a left-out plane's pitch is
    ignored (garbage) and nothing but the wanted targets is written."""
    name = "random_11"  # blocks, billboards and march-outs
    want = vc.reference(name)
    vworld.set_scene(vc.scene(name), W, H)
    for planes in [(p,) for p in PLANES] + [tuple(q for q in PLANES if q != p) for p in PLANES]:
        band = Band(planes=planes)
        guard = poisoned((H, 4 * W), POISON)  # a neighbour no call may touch
        band.render(vworld, stream)
        vworld.check(stream.cuda_stream)
        rgba, got = band.read()
        assert set(got) == set(planes)
        _assert_planes(got, want, str(planes))
        assert np.array_equal(rgba, oracle_frame(name)[0]), planes
        assert (guard.cpu().numpy() == POISON).all()


def test_bands_tile_the_frame(vworld, stream):
    name = "default_turned"
    want = vc.reference(name)
    vworld.set_scene(vc.scene(name), W, H)
    band = Band()
    for r0, r1 in [(0, 13), (13, 14), (14, 37)]:
        band.render(vworld, stream, r0, r1 - r0, at=r0)
    vworld.check(stream.cuda_stream)
    rgba, got = band.read()
    _assert_planes(got, want, "bands")
    assert np.array_equal(rgba, oracle_frame(name)[0])


def _host_canvas():
    rgba = np.full((H, W, 4), POISON, dtype=np.uint8)
    return rgba, {p: np.full((H, W, 4), POISON, dtype=np.uint8).view(DTYPES[p]).reshape(H, W)
                  for p in PLANES}


def test_update_image_aux_strides_and_pick(vworld):
    """update_image_aux addresses pixels as update_image does: only the addressed elements change,
    in `pixels` and in every plane; a single-pixel pick is (j, height, i, width)."""
    name = "random_11"
    want, want_rgba = vc.reference(name), oracle_frame(name)[0]
    vworld.set_scene(vc.scene(name), W, H)
    face = want["face"]
    picks = [tuple(int(v) for v in np.argwhere(face == f)[0][::-1]) for f in (4, 0)] + [(W - 1, H - 1)]
    for ystart, yadd, xstart, xadd in [(0, 4, 1, 4), (3, 4, 0, 1), (0, 1, 7, 3)] + \
            [(j, H, i, W) for i, j in picks]:
        rgba, got = _host_canvas()
        vworld.update_image_aux(rgba, *(got[p] for p in PLANES), ystart, yadd, xstart, xadd)
        mask = np.zeros((H, W), dtype=bool)
        mask[ystart::yadd, xstart::xadd] = True
        assert mask.sum() == len(range(ystart, H, yadd)) * len(range(xstart, W, xadd))
        assert np.array_equal(rgba[mask], want_rgba[mask]) and (rgba[~mask] == POISON).all()
        for p in PLANES:
            assert np.array_equal(_bits(got[p])[mask], _bits(want[p])[mask]), (p, ystart, xstart)
            assert (got[p].view(np.uint8).reshape(H, W, 4)[~mask] == POISON).all(), p
    full = vworld.render_aux()
    assert np.array_equal(full[0], want_rgba)
    _assert_planes(dict(zip(PLANES, full[1:])), want, "render_aux")


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("name", vc.SS_NAMES)
def test_supersampled_planes_are_the_first_samples(vworld, stream, name, s):
    """S = 2, 4: the colour is the plain supersampled frame (and the box-filtered oracle's), the
    planes are those of sample (S*i, S*j); they differ from the last sample's, which the reference
    shows to differ (tests/test_voxel_ref.py LAST_SAMPLE_DIFFERS)."""
    import sfrt
    big = vc.reference(name, s)
    vworld.set_scene(vc.scene(name), W, H)
    vworld.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
    try:
        band = Band()
        band.render(vworld, stream)
        plain = _plain(vworld, stream)
        vworld.check(stream.cuda_stream)
        rgba, got = band.read()
        host = vworld.render_aux()
    finally:
        vworld.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 1)
    first = voxel_ref.first_sample(big, s)
    _assert_planes(got, first, f"{name} S={s}")
    _assert_planes(dict(zip(PLANES, host[1:])), first, f"{name} S={s} update_image_aux")
    assert np.array_equal(rgba, plain.cpu().numpy().reshape(H, W, 4))
    assert np.array_equal(rgba, oracle_frame(name, s)[0])
    assert np.array_equal(host[0], rgba)
    for p in PLANES:
        last = big[p][s - 1::s, s - 1::s]
        assert not np.array_equal(_bits(last), _bits(first[p])), p  # the reference's own guard
        assert not np.array_equal(_bits(got[p]), _bits(last)), p


@pytest.mark.parametrize("order", [1, 2])
def test_tile_order_same_planes(vworld, order):
    """SFRT_OPT_TILE_ORDER 1 and 2: four consecutive aux frames on one stream, then plain and aux
    alternating (one chain: the same tile key), equal the order-0 planes and colour; plain frames
    after aux frames still equal the oracle."""
    import sfrt
    import torch
    name = "default"
    want, want_rgba = vc.reference(name), oracle_frame(name)[0]
    vworld.set_scene(vc.scene(name), W, H)
    s = torch.cuda.Stream()
    vworld.set_option(sfrt.SFRT_OPT_TILE_ORDER, order)
    try:
        frames = []
        for kind in ["aux"] * 4 + ["plain", "aux"] * 3 + ["plain", "plain"]:
            if kind == "aux":
                b = Band()
                b.render(vworld, s)
            else:
                b = _plain(vworld, s)
            frames.append((kind, b))
        vworld.check(s.cuda_stream)
    finally:
        vworld.set_option(sfrt.SFRT_OPT_TILE_ORDER, 0)
    for k, (kind, b) in enumerate(frames):
        if kind == "aux":
            rgba, got = b.read()
            _assert_planes(got, want, f"order {order} frame {k}")
        else:
            rgba = b.cpu().numpy().reshape(H, W, 4)
        assert np.array_equal(rgba, want_rgba), (order, k, kind)


def test_errors(vworld, stream):
    import sfrt
    name = "negative_coordinates"
    want, (want_rgba, ub) = vc.reference(name), oracle_frame(name)
    assert ub
    vworld.set_scene(vc.scene(name), W, H)
    band = Band()
    col = band.buf["colour"].data_ptr()

    def code(**planes):
        with pytest.raises(sfrt.SfrtError) as e:
            vworld.render_band_aux(col, band.pitch["colour"], 0, H, stream.cuda_stream, **planes)
        return e.value.code

    assert code() == -1                                                   # all planes NULL
    assert code(depth=(band.buf["depth"].data_ptr(), 4 * W - 4)) == -1    # below 4 * width
    assert code(face=(band.buf["face"].data_ptr(), 4 * W + 2)) == -1      # not a multiple of 4
    assert code(depth=(band.buf["depth"].data_ptr(), band.pitch["depth"]),
                steps=(band.buf["steps"].data_ptr(), 4 * W - 4)) == -1
    rgba, got = _host_canvas()
    with pytest.raises(sfrt.SfrtError) as e:
        vworld.update_image_aux(rgba)
    assert e.value.code == -1
    vworld.check(stream.cuda_stream)
    for b in band.buf.values():
        assert (b.cpu().numpy() == POISON).all()
    # a world without blocks
    empty = sfrt.VoxelWorld(0)
    try:
        empty.width, empty.height = W, H
        sfrt._check(sfrt.lib().sfrt_voxel_set_size(empty._h, W, H), "set_size")
        with pytest.raises(sfrt.SfrtError) as e:
            band.render(empty, stream)
        assert e.value.code == -2
        with pytest.raises(sfrt.SfrtError) as e:
            empty.update_image_aux(rgba, *(got[p] for p in PLANES))
        assert e.value.code == -2
    finally:
        empty.close()
    for b in band.buf.values():
        assert (b.cpu().numpy() == POISON).all()
    # a read outside a texture: render_band_aux's planes are the reference's, check raises -7
    band.render(vworld, stream)
    _check(vworld, stream, True)
    dev_rgba, dev_planes = band.read()
    _assert_planes(dev_planes, want, name)
    assert np.array_equal(dev_rgba, want_rgba)
    # update_image_aux returns -7 and writes neither pixels nor any plane
    with pytest.raises(sfrt.SfrtError) as e:
        vworld.update_image_aux(rgba, *(got[p] for p in PLANES))
    assert e.value.code == TEXEL
    assert (rgba == POISON).all()
    for p in PLANES:
        assert (got[p].view(np.uint8) == POISON).all(), p
