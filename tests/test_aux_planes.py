"""The frame fill's per-pixel planes (include/sfrt.h sfrt_aux_planes): depth, sphere index and
march steps, written by the launch that writes the colour.

The reference of every plane comes from the oracle alone, one Oracle.dump(i, j) per pixel:
sphere = dump["draw"], steps = dump["iters"] (asserted equal to iteration_map()), and depth =
sqrtf((ex*ex + ey*ey) + ez*ez), e = dump["pos"] - cam, evaluated in numpy binary32 -- pinned to
the oracle by asserting 3.0f / max(depth, 3.0f) == dump["brightness"] bit for bit.  Depth is
compared as uint32 bit patterns, with no tolerance.  Frames are 101x37, ragged against every
tile width (as tests/test_supersample.py).  Supersampled, the planes are those of sample pixel
(S*i, S*j) of the S*W x S*H frame.
"""
import ctypes
import functools

import numpy as np
import pytest

import scenes
from conftest import host_threads, poisoned
from test_supersample import POSES, W, H, reference as colour_reference

F = np.float32
POISON = 0xA5
PLANES = ("depth", "sphere", "steps")
DTYPES = {"depth": np.float32, "sphere": np.int32, "steps": np.int32}
PADS = {"colour": 16, "depth": 4, "sphere": 8, "steps": 12}  # every target its own pitch
# Conditions on the references (checked on the CPU when the tests were written; asserted so that
# a scene change cannot make a test vacuous): distinct draw values, (min, max) steps.
EXPECT = {"default10": (4, (4, 13)), "lcg64": (17, (2, 50)), "lcg256": (29, (4, 54)),
          "near_wall": (1, (2, 6))}
FIXTURES = ("default10", "lcg64", "lcg256", "near_wall")


def _scene(name):
    if name == "near_wall":
        # inside the radius-4 sphere, 1.5 from its wall: most hit distances are below 3, where
        # the colour's brightness is 1 and only the unclamped depth tells the distance
        cam = (0.0, 0.0, 2.5)
        base = scenes.one_sphere()
        return scenes.Scene("near_wall", scenes.sort_spheres(base.spheres, cam), cam).posed(0.7, 0.3)
    return scenes.SCENES[name]().posed(*POSES[name])


@functools.lru_cache(maxsize=None)
def _floor():
    tex, tw, th = scenes.load_floor()
    tex = np.array(tex, dtype=np.uint8).ravel()
    tex.setflags(write=False)
    return tex, tw, th


def _depth_of(pos, cam):
    """VLength(pos - cam) (SphereWorld.cpp:375, :340-343) in binary32; pos (..., 3) float32."""
    e = pos - cam  # float32 - float32, per component
    return np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])


@functools.lru_cache(maxsize=None)
def planes_reference(name, s=1, off=0):
    """{"depth", "sphere", "steps"}: (H, W) arrays of the oracle's pixel (s*i + off, s*j + off)
    of the s*W x s*H frame (off = 0: the output pixel's first sample); computed once, shared,
    read-only."""
    import oracle
    sc = _scene(name)
    o = oracle.Oracle.from_scene(sc, s * W, s * H, *_floor())
    itmap = o.iteration_map(host_threads()).reshape(s * H, s * W)
    pos = np.zeros((H, W, 3), dtype=F)
    sphere = np.zeros((H, W), dtype=np.int32)
    steps = np.zeros((H, W), dtype=np.int32)
    bright = np.zeros((H, W), dtype=F)
    for j in range(H):
        for i in range(W):
            d = o.dump(s * i + off, s * j + off)
            pos[j, i] = d["pos"]
            sphere[j, i] = d["draw"]
            steps[j, i] = d["iters"]
            bright[j, i] = d["brightness"]
    assert pos.dtype == F
    depth = _depth_of(pos, np.asarray(sc.cam_pos, dtype=F))
    assert depth.dtype == F
    # the numpy restatement is the oracle's own value: its brightness, bit for bit
    assert np.array_equal((F(3.0) / np.maximum(depth, F(3.0))).view(np.uint32), bright.view(np.uint32))
    assert np.array_equal(steps, itmap[off::s, off::s])
    if s == 1:
        ndraw, (lo, hi) = EXPECT[name]
        assert len(np.unique(sphere)) == ndraw, (name, len(np.unique(sphere)))
        assert (int(steps.min()), int(steps.max())) == (lo, hi), (name, steps.min(), steps.max())
        if name == "near_wall":
            assert np.count_nonzero(depth < F(3.0)) >= depth.size // 2
    out = {"depth": depth, "sphere": sphere, "steps": steps}
    for a in out.values():
        a.setflags(write=False)
    return out


def _world(name, s=1):
    import sfrt
    w = sfrt.World(0)
    w.load_texture(*_floor())
    w.set_scene(_scene(name), W, H)
    w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
    return w


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_planes(got, want, what="", rows=slice(None)):
    for p, a in got.items():
        bad = int(np.count_nonzero(_bits(a) != _bits(want[p][rows])))
        assert bad == 0, f"{what}: plane {p}: {bad} pixels differ from the oracle"


def _host_aux(w, planes=PLANES, stride=(0, 1, 0, 1), canvas=None):
    """update_image_aux into poisoned host buffers (or `canvas`); (rgba (H, W, 4), {plane})."""
    if canvas is None:
        canvas = _host_canvas(planes)
    rgba, got = canvas
    w.update_image_aux(rgba, *(got.get(p) for p in PLANES), *stride)
    return rgba, got


def _host_canvas(planes=PLANES):
    rgba = np.full((H, W, 4), POISON, dtype=np.uint8)
    return rgba, {p: np.full((H, W, 4), POISON, dtype=np.uint8).view(DTYPES[p]).reshape(H, W)
                  for p in planes}


class Band:
    """Poisoned device targets of one render_band_aux: colour and each wanted plane, every one
    with its own pitch."""

    def __init__(self, rows=H, planes=PLANES):
        self.rows = rows
        self.pitch = {k: 4 * W + PADS[k] for k in ("colour",) + tuple(planes)}
        self.buf = {k: poisoned((rows, p), POISON) for k, p in self.pitch.items()}
        self.planes = tuple(planes)

    def args(self, row=0):
        """Plane keyword arguments of World.render_band_aux, the targets' row `row` first."""
        return {p: (self.buf[p].data_ptr() + row * self.pitch[p], self.pitch[p]) for p in self.planes}

    def colour_ptr(self, row=0):
        return self.buf["colour"].data_ptr() + row * self.pitch["colour"]

    def read(self):
        """(rgba (rows, W, 4), {plane: (rows, W)}); asserts the padding bytes untouched."""
        out = {}
        for k, b in self.buf.items():
            a = b.cpu().numpy()
            assert (a[:, 4 * W:] == POISON).all(), f"{k}: padding written"
            a = np.ascontiguousarray(a[:, :4 * W])
            out[k] = a.reshape(self.rows, W, 4) if k == "colour" else a.view(DTYPES[k])
        return out.pop("colour"), out

    def untouched(self):
        return all(bool((b == POISON).all()) for b in self.buf.values())


def _ordered_aux(w, frames=3, planes=PLANES):
    """`frames` render_band_aux fills back to back on one stream: the adaptive tile order is
    live from the second on."""
    import torch
    stream = torch.cuda.Stream()
    bands = [Band(planes=planes) for _ in range(frames)]
    for b in bands:
        w.render_band_aux(b.colour_ptr(), b.pitch["colour"], 0, H, stream.cuda_stream, **b.args())
    w.check(stream.cuda_stream)
    return [b.read() for b in bands]


# ---------------------------------------------------------------- CPU


def test_entry_points_exist_and_refuse_a_null_world(built):
    import sfrt
    lib = sfrt.lib()
    for name in ("sfrt_world_render_band_aux", "sfrt_world_update_image_aux"):
        assert hasattr(lib, name), name
        assert name in sfrt.ABI_SYMBOLS
    planes = sfrt.AuxPlanes()
    dummy = (ctypes.c_uint8 * 64)()
    planes.depth, planes.depth_pitch_bytes = ctypes.addressof(dummy), 64
    assert lib.sfrt_world_render_band_aux(None, ctypes.addressof(dummy), 64, ctypes.byref(planes),
                                          0, 1, None) == -1
    assert lib.sfrt_world_update_image_aux(None, ctypes.addressof(dummy), ctypes.addressof(dummy),
                                           None, None, 0, 1, 0, 1) == -1
    assert bytes(dummy) == bytes(64)
    assert ctypes.sizeof(sfrt.AuxPlanes) == 48
    assert lib.sfrt_version() >= 6


# ---------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_planes_equal_the_oracle(built, name):
    """update_image_aux (row-major) and three render_band_aux frames on one stream (ordered from
    the second): the three planes are the reference's, the colour the plain render()'s."""
    want = planes_reference(name)
    with _world(name) as w:
        plain = w.render().reshape(H, W, 4)
        rgba, got = _host_aux(w)
        assert np.array_equal(rgba, plain)
        _assert_planes(got, want, "update_image_aux")
        for k, (rgba, got) in enumerate(_ordered_aux(w)):
            assert np.array_equal(rgba, plain), k
            _assert_planes(got, want, f"render_band_aux frame {k}")
        # the convenience wrapper returns the same four arrays
        rgba, depth, sphere, steps = w.render_aux()
        assert np.array_equal(rgba, plain)
        _assert_planes({"depth": depth, "sphere": sphere, "steps": steps}, want, "render_aux")


@pytest.mark.gpu
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("rays", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["lcg64", "lcg256"])
def test_every_tile_shape_row_major_and_ordered(built, name, rays, cull):
    import sfrt
    want = planes_reference(name)
    colour = colour_reference(name, 1)
    with _world(name) as w:
        w.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
        w.set_option(sfrt.SFRT_OPT_CULL, cull)
        rgba, got = _host_aux(w)
        assert np.array_equal(rgba, colour)
        _assert_planes(got, want, "row-major")
        for k, (rgba, got) in enumerate(_ordered_aux(w)):
            assert np.array_equal(rgba, colour), k
            _assert_planes(got, want, f"ordered frame {k}")


SUBSETS = [tuple(p for p, bit in zip(PLANES, (1, 2, 4)) if m & bit) for m in range(1, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("planes", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_plane_subsets(built, planes):
    """Each non-empty NULL / non-NULL combination, device and host path: the wanted planes are
    the reference's and the colour is unchanged."""
    want = planes_reference("lcg64")
    colour = colour_reference("lcg64", 1)
    with _world("lcg64") as w:
        for k, (rgba, got) in enumerate(_ordered_aux(w, frames=2, planes=planes)):
            assert set(got) == set(planes)
            assert np.array_equal(rgba, colour), k
            _assert_planes(got, want, f"band {k}")
        rgba, got = _host_aux(w, planes)
        assert np.array_equal(rgba, colour)
        _assert_planes(got, want, "host")


@pytest.mark.gpu
def test_invalid_plane_arguments_write_nothing(built):
    import sfrt
    import torch
    with _world("lcg64") as w:
        stream = torch.cuda.Stream()
        b = Band()

        def refused(**planes):
            with pytest.raises(sfrt.SfrtError) as e:
                w.render_band_aux(b.colour_ptr(), b.pitch["colour"], 0, H, stream.cuda_stream, **planes)
            assert e.value.code == -1
            w.check(stream.cuda_stream)
            assert b.untouched()

        refused()  # all three NULL
        good = b.args()
        for p in PLANES:
            ptr, pitch = good[p]
            refused(**{**good, p: (ptr, 4 * W - 4)})  # short
            refused(**{**good, p: (ptr, pitch + 2)})  # not a multiple of 4
        # the plain call's own checks still apply
        with pytest.raises(sfrt.SfrtError) as e:
            w.render_band_aux(b.colour_ptr(), 4 * W - 4, 0, H, stream.cuda_stream, **good)
        assert e.value.code == -1
        with pytest.raises(sfrt.SfrtError) as e:
            w.render_band_aux(b.colour_ptr(), b.pitch["colour"], 1, H, stream.cuda_stream, **good)
        assert e.value.code == -1
        w.check(stream.cuda_stream)
        assert b.untouched()
        # host path: all planes NULL
        rgba = np.full((H, W, 4), POISON, dtype=np.uint8)
        with pytest.raises(sfrt.SfrtError) as e:
            w.update_image_aux(rgba)
        assert e.value.code == -1
        assert (rgba == POISON).all()
        # a NULL plane's pitch is ignored
        w.render_band_aux(b.colour_ptr(), b.pitch["colour"], 0, H, stream.cuda_stream,
                          depth=good["depth"], sphere=(0, 3))
        w.check(stream.cuda_stream)


@pytest.mark.gpu
def test_pixel_subsets_write_only_addressed_pixels(built):
    """The eight RenderThreads' interleave (Source.cpp:21-23): UpdateImage(num, 8, cycle, 4) for
    num < 8, cycle < 4.  Each call writes its addressed pixels only, in every plane; the 32
    calls assemble the reference."""
    want = planes_reference("lcg64")
    colour = colour_reference("lcg64", 1)
    canvas = _host_canvas()
    rgba, got = canvas
    done = np.zeros((H, W), dtype=bool)
    with _world("lcg64") as w:
        for num in range(8):
            for cycle in range(4):
                _host_aux(w, stride=(num, 8, cycle, 4), canvas=canvas)
                done[num::8, cycle::4] = True
                assert np.array_equal(rgba[done], colour[done])
                assert (rgba[~done] == POISON).all(), (num, cycle)
                for p in PLANES:
                    assert np.array_equal(_bits(got[p])[done], _bits(want[p])[done]), (p, num, cycle)
                    assert (got[p].view(np.uint8).reshape(H, W, 4)[~done] == POISON).all(), (p, num, cycle)
    assert done.all()
    _assert_planes(got, want, "assembled")


@pytest.mark.gpu
def test_bands_tile_all_four_outputs(built):
    """Bands of 5, 19 and 13 rows with global row indices tile the colour and the planes; a band
    alone writes its rows only."""
    import torch
    want = planes_reference("lcg256")
    colour = colour_reference("lcg256", 1)
    stream = torch.cuda.Stream()
    with _world("lcg256") as w:
        full, alone = Band(), Band()
        for row0, rows in ((0, 5), (5, 19), (24, 13)):
            w.render_band_aux(full.colour_ptr(row0), full.pitch["colour"], row0, rows,
                              stream.cuda_stream, **full.args(row0))
        w.render_band_aux(alone.colour_ptr(5), alone.pitch["colour"], 5, 19, stream.cuda_stream,
                          **alone.args(5))
        w.check(stream.cuda_stream)
        rgba, got = full.read()
        assert np.array_equal(rgba, colour)
        _assert_planes(got, want, "three bands")
        rgba, got = alone.read()
        assert np.array_equal(rgba[5:24], colour[5:24])
        assert (rgba[:5] == POISON).all() and (rgba[24:] == POISON).all()
        for p, a in got.items():
            assert np.array_equal(_bits(a[5:24]), _bits(want[p][5:24])), p
            raw = a.view(np.uint8)
            assert (raw[:5] == POISON).all() and (raw[24:] == POISON).all(), p


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("name", ["lcg64", "lcg256"])
def test_supersampled_planes_are_the_first_sample(built, name, s):
    """The colour is the box-filtered frame; the planes are the oracle's pixel (S*i, S*j) of the
    S*W x S*H frame.

    That reference cannot differ from the 1x planes: sample (S*i, S*j) of the S*W x S*H frame is
    the 1x pixel's own ray, bit for bit (hIncreaseBy = fovH / (S*W) * 2 is the 1x increment
    divided by the power of two S, exactly, and S*i undoes it before the product rounds; rows
    likewise) -- measured here: 0 of 3737 pixels differ in any plane, both scenes, both factors;
    asserted below as the property it is.  What tells a kernel that mishandles S is the rest of
    the group: the reference must differ from the planes of the group's LAST sample
    (S*i + S - 1, S*j + S - 1) in more than a handful of pixels, so a kernel that stored another
    lane's values, or a filtered one, fails (as does one that ignored S in the colour)."""
    want = planes_reference(name, s)
    colour = colour_reference(name, s)
    one = planes_reference(name, 1)
    last = planes_reference(name, s, s - 1)
    for p in PLANES:
        assert np.array_equal(_bits(want[p]), _bits(one[p])), p
        assert np.count_nonzero(_bits(want[p]) != _bits(last[p])) > 16, p
    assert np.count_nonzero((colour != colour_reference(name, 1)).any(axis=-1)) > 0.3 * W * H
    with _world(name, s) as w:
        rgba, got = _host_aux(w)
        assert np.array_equal(rgba, colour)
        _assert_planes(got, want, "row-major")
        for k, (rgba, got) in enumerate(_ordered_aux(w)):
            assert np.array_equal(rgba, colour), k
            _assert_planes(got, want, f"ordered frame {k}")


SMALL_W, SMALL_H = 40, 24  # partial tiles at every tile width; both factors divide both sides


def _small_scene(n):
    """n spheres: 64 travel in the kernel arguments, 65 are the fewest that take the list kernels."""
    spheres = scenes.sort_spheres(scenes.lcg_spheres(count=n - 1, seed=31 + n))
    return scenes.Scene(f"many{n}", spheres).posed(1.1, -0.2)


@functools.lru_cache(maxsize=None)
def _small_reference(n, s):
    """(colour (H, W, 4), planes) of the 40x24 frame at factor s, from the oracle alone: its
    s*W x s*H frame box-filtered, and the planes of each group's first sample (planes_reference's
    construction, the depth pinned to the oracle's brightness in the same way)."""
    import oracle
    sc = _small_scene(n)
    o = oracle.Oracle.from_scene(sc, s * SMALL_W, s * SMALL_H, *_floor())
    big = o.render(host_threads())
    sums = big.reshape(SMALL_H, s, SMALL_W, s, 4).astype(np.uint32).sum(axis=(1, 3))
    colour = ((sums + s * s // 2) >> {2: 2, 4: 4}[s]).astype(np.uint8)
    dumps = [[o.dump(s * i, s * j) for i in range(SMALL_W)] for j in range(SMALL_H)]
    pos = np.array([[d["pos"] for d in row] for row in dumps], dtype=F)
    bright = np.array([[d["brightness"] for d in row] for row in dumps], dtype=F)
    depth = _depth_of(pos, np.asarray(sc.cam_pos, dtype=F))
    assert depth.dtype == F
    assert np.array_equal((F(3.0) / np.maximum(depth, F(3.0))).view(np.uint32), bright.view(np.uint32))
    planes = {"depth": depth,
              "sphere": np.array([[d["draw"] for d in row] for row in dumps], dtype=np.int32),
              "steps": np.array([[d["iters"] for d in row] for row in dumps], dtype=np.int32)}
    assert len(np.unique(planes["sphere"])) > 1 and planes["steps"].max() > planes["steps"].min()
    for a in (colour, *planes.values()):
        a.setflags(write=False)
    return colour, planes


@pytest.mark.gpu
@pytest.mark.parametrize("rays", [1, 3, 4])
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("n", [64, 65])
def test_supersampled_planes_at_every_other_tile_shape(built, n, s, rays):
    """The supersampled aux kernels at R = 1, 3 and 4, for n <= 64 and above: the tests above
    reach them only at the kernel table's own choice, R = 2."""
    import sfrt
    colour, want = _small_reference(n, s)
    with sfrt.World(0) as w:
        w.load_texture(*_floor())
        w.set_scene(_small_scene(n), SMALL_W, SMALL_H)
        w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
        w.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
        rgba, depth, sphere, steps = w.render_aux()
    assert np.array_equal(rgba, colour)
    _assert_planes({"depth": depth, "sphere": sphere, "steps": steps}, want, f"n={n} s={s} R={rays}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default10", "lcg256"])
def test_ray_cache_left_alone(built, name):
    """plain, plain (the fill), aux, plain on one stream with one geometry: the aux launch
    neither fills, reads nor invalidates the cache, and counts nowhere."""
    import torch
    want = planes_reference(name)
    stream = torch.cuda.Stream()
    pitch = 4 * W

    def plain(w):
        buf = poisoned((H, pitch), POISON)
        w.render_band(buf.data_ptr(), pitch, 0, H, stream.cuda_stream)
        w.check(stream.cuda_stream)
        return buf.cpu().numpy()

    def stats(w):
        st = w.ray_cache_stats()
        return st["cached_frames"], st["fills"], st["bytes"]

    with _world(name) as w:
        first = plain(w)
        assert stats(w)[:2] == (0, 0)
        plain(w)
        filled = stats(w)
        assert filled[:2] == (1, 1) and filled[2] > 0
        b = Band()
        w.render_band_aux(b.colour_ptr(), b.pitch["colour"], 0, H, stream.cuda_stream, **b.args())
        w.check(stream.cuda_stream)
        assert stats(w) == filled
        rgba, got = b.read()
        _assert_planes(got, want, "aux between cached frames")
        last = plain(w)
        assert stats(w) == (2, 1, filled[2])
        assert np.array_equal(last, first)
        assert np.array_equal(rgba.reshape(H, pitch), first)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lcg64", "lcg256"])
def test_row_costs_after_an_aux_band(built, name):
    """sfrt_world_row_costs after an aux band equals the costs after a plain band of the same
    world and rows."""
    import torch
    stream = torch.cuda.Stream()
    pitch = 4 * W
    for row0, rows in ((0, H), (5, 19)):
        with _world(name) as w:
            buf = poisoned((rows, pitch), POISON)
            w.render_band(buf.data_ptr(), pitch, row0, rows, stream.cuda_stream)
            w.check(stream.cuda_stream)
            plain = w.row_costs()
        with _world(name) as w:
            b = Band(rows)
            w.render_band_aux(b.colour_ptr(), b.pitch["colour"], row0, rows, stream.cuda_stream,
                              **b.args())
            w.check(stream.cuda_stream)
            aux = w.row_costs()
        assert aux[0] == plain[0] == row0
        assert aux[1].size == rows and (aux[1] > 0).all()
        assert np.array_equal(aux[1], plain[1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lcg64", "lcg256"])
def test_agrees_with_trace_points(built, name):
    """64 listed pixels: the planes equal draw, iters and the depth derived from pos of
    sfrt_world_trace_points (the debug path)."""
    rng = np.random.default_rng(11)
    ij = np.stack([rng.integers(0, W, 64), rng.integers(0, H, 64)], axis=1)
    ij[:4] = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    with _world(name) as w:
        _, got = _host_aux(w)
        dumps = w.trace_points(ij)
        cam = np.asarray(_scene(name).cam_pos, dtype=F)
    for (i, j), d in zip(ij, dumps):
        assert got["sphere"][j, i] == d["draw"], (i, j)
        assert got["steps"][j, i] == d["iters"], (i, j)
        depth = _depth_of(np.asarray(d["pos"], dtype=F), cam)
        assert _bits(got["depth"][j, i:i + 1])[0] == _bits(np.asarray([depth], dtype=F))[0], (i, j)
