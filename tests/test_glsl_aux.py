"""The GLSL renderer's per-pixel planes: sfrt_glsl_draw_aux and sfrt_glsl_draw_image_aux
(include/sfrt.h "the draw's per-pixel planes").

depth is totalDist after rayShader.frag:117, sphere drawSphere after :118, steps the trips of the
metaball loop :94-112.  Every comparison is on bits, against the restatement's per-pixel dump
(oracle/glsl_oracle.c oglsl_pixel, tests/glsl_aux_cases.py).  Frames are 40x24 and 37x23: the
second has edge lanes in every tile row and column.
"""
import ctypes
import os

import numpy as np
import pytest

import glsl_aux_cases as gc
from conftest import ROOT, poisoned

E_INVALID = -1
POISON = 0xA5
PLANES = ("depth", "sphere", "steps")
DTYPE = {"depth": np.float32, "sphere": np.int32, "steps": np.int32}
SHAPES = [(n, w, h) for n in gc.CASES for (w, h) in gc.SIZES] + [(n, 37, 23) for n in gc.EDGE]
IDS = [f"{n}@{w}x{h}" for n, w, h in SHAPES]


# ---------------------------------------------------------------- CPU

def test_entry_points_are_declared_and_exported(built):
    """The two plane calls are in include/sfrt.h, in the bindings' table and in the library, and
    refuse a NULL shader before anything touches a device; the header no longer says the GLSL
    renderer has no planes."""
    import sfrt
    lib = sfrt.lib()
    assert lib.sfrt_version() >= 10
    header = open(os.path.join(ROOT, "include", "sfrt.h")).read()
    for name in ("sfrt_glsl_draw_aux", "sfrt_glsl_draw_image_aux"):
        assert name in sfrt.ABI_SYMBOLS and hasattr(lib, name) and f"{name}(" in header
    assert "GLSL renderer have no planes" not in " ".join(header.split())
    planes = sfrt.AuxPlanes(depth=4, depth_pitch_bytes=64)
    assert lib.sfrt_glsl_draw_aux(None, 4, 8, 8, 32, ctypes.byref(planes), 0, 8, None) == E_INVALID
    assert lib.sfrt_glsl_draw_image_aux(None, 4, 4, None, None, 8, 8) == E_INVALID


@pytest.mark.parametrize("name", list(gc.CASES))
def test_expected_frames_have_walls_balls_and_step_counts(name):
    """The frames the GPU tests compare with hold what they are meant to exercise."""
    for w, h in gc.SIZES:
        gc.check_content(name, w, h)


# ---------------------------------------------------------------- GPU helpers

@pytest.fixture(scope="module")
def shader(built):
    import sfrt
    s = sfrt.GlslShader(0)
    s.set_ground(*gc.floor())
    yield s
    s.close()


@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream()


def _canvas(w, h, pad):
    """A poisoned device canvas of h rows with a pitch of 4 * w + pad bytes."""
    return poisoned((h, 4 * w + pad), POISON)


def _plane(buf, w, name):
    """The plane's h x w elements out of its canvas; asserts the pad bytes kept the poison."""
    a = buf.cpu().numpy()
    assert (a[:, 4 * w:] == POISON).all(), f"{name}: pad bytes written"
    return np.ascontiguousarray(a[:, :4 * w]).view(DTYPE[name] if name in DTYPE else np.uint8)


def draw_aux(shader, stream, w, h, planes=PLANES, row0=0, rows=None, repeat=1, pads=None):
    """sfrt_glsl_draw_aux on `stream` into poisoned canvases, each target with its own padded
    pitch; returns ({rgba, plane: array}, canvases)."""
    rows = h - row0 if rows is None else rows
    pads = pads or {"rgba": 20, "depth": 4, "sphere": 36, "steps": 12}
    bufs = {k: _canvas(w, h, pads[k]) for k in ("rgba",) + tuple(planes)}
    for _ in range(repeat):
        shader.draw_aux(bufs["rgba"][row0].data_ptr(), w, h, bufs["rgba"].stride(0), row0, rows,
                        stream.cuda_stream,
                        **{k: (bufs[k][row0].data_ptr(), bufs[k].stride(0)) for k in planes})
    shader.check(stream.cuda_stream)
    return {k: _plane(b, w, k) for k, b in bufs.items()}, bufs


def draw_plain(shader, stream, w, h, repeat=1):
    b = _canvas(w, h, 0)
    for _ in range(repeat):
        shader.draw(b.data_ptr(), w, h, w * 4, 0, h, stream.cuda_stream)
    shader.check(stream.cuda_stream)
    return b.cpu().numpy().reshape(h, w, 4)


def assert_planes(got, name, w, h, scale=1, planes=PLANES):
    e = gc.expected(name, w, h, scale)
    for k in planes:
        bad = np.argwhere(gc.bits(got[k]).reshape(h, w) != gc.bits(e[k]))
        assert bad.size == 0, (f"{name}@{w}x{h} S={scale} {k}: {len(bad)} pixels differ, first "
                               f"(row {bad[0][0]}, col {bad[0][1]}): {got[k][tuple(bad[0])]} vs "
                               f"{e[k][tuple(bad[0])]}")


# ---------------------------------------------------------------- GPU: planes

@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h", SHAPES, ids=IDS)
def test_planes_equal_the_oracle_dump(shader, stream, name, w, h):
    """1. Every plane equals the dump for every pixel through draw_image_aux (row-major), draw_aux
    in the adaptive order (three draws, so the order is live) and draw_aux row-major; the colour
    equals the plain call's bytes and the restatement's frame."""
    import sfrt
    gc.check_content(name, w, h)
    shader.set_uniforms(gc.uniforms(name, w, h))
    want_rgba = gc.expected_rgba(name, w, h)
    img = shader.draw_image_aux(w, h)
    assert_planes(img, name, w, h)
    assert np.array_equal(img["rgba"], shader.draw_image(w, h))
    assert np.array_equal(img["rgba"].reshape(h, w, 4), want_rgba)
    for order in (1, 0):
        shader.set_option(sfrt.SFRT_OPT_TILE_ORDER, order)
        try:
            got, _ = draw_aux(shader, stream, w, h, repeat=3)
            plain = draw_plain(shader, stream, w, h)
        finally:
            shader.set_option(sfrt.SFRT_OPT_TILE_ORDER, 1)
        assert_planes(got, name, w, h)
        assert np.array_equal(got["rgba"].reshape(h, w, 4), plain), order
        assert np.array_equal(plain, want_rgba), order


SUBSETS = [tuple(p for k, p in enumerate(PLANES) if m >> k & 1) for m in range(1, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("planes", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_every_plane_subset(shader, stream, planes):
    """2. All seven subsets, every target with its own padded pitch: the requested planes are
    right, their pad bytes untouched (draw_aux's helper asserts it), and the memory a NULL plane
    would have used -- canvases handed to nobody -- keeps its poison; the host call likewise."""
    name, (w, h) = "posed", gc.SIZES[1]
    shader.set_uniforms(gc.uniforms(name, w, h))
    bystanders = {k: _canvas(w, h, 8) for k in PLANES if k not in planes}
    got, _ = draw_aux(shader, stream, w, h, planes=planes)
    assert_planes(got, name, w, h, planes=planes)
    assert np.array_equal(got["rgba"].reshape(h, w, 4), gc.expected_rgba(name, w, h))
    for k, b in bystanders.items():
        assert (b.cpu().numpy() == POISON).all(), k
    img = shader.draw_image_aux(w, h, **{k: k in planes for k in PLANES})
    assert set(img) == {"rgba", *planes}
    assert_planes(img, name, w, h, planes=planes)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", gc.SIZES)
def test_bands_tile_the_frame(shader, stream, w, h):
    """3. Bands (row0, rows) that tile the frame reproduce all four outputs; rows outside a band
    keep the poison."""
    name = "random3"
    shader.set_uniforms(gc.uniforms(name, w, h))
    pads = {"rgba": 20, "depth": 4, "sphere": 36, "steps": 12}
    bufs = {k: _canvas(w, h, pads[k]) for k in ("rgba",) + PLANES}
    edges = [0, 5, 8, 17, h]
    first = None
    for k, (r0, r1) in enumerate(zip(edges, edges[1:])):
        shader.draw_aux(bufs["rgba"][r0].data_ptr(), w, h, bufs["rgba"].stride(0), r0, r1 - r0,
                        stream.cuda_stream,
                        **{p: (bufs[p][r0].data_ptr(), bufs[p].stride(0)) for p in PLANES})
        if k == 0:
            shader.check(stream.cuda_stream)
            first = bufs["depth"].cpu().numpy()
    shader.check(stream.cuda_stream)
    assert (first[edges[1]:] == POISON).all(), "the first band wrote past its rows"
    got = {k: _plane(b, w, k) for k, b in bufs.items()}
    assert_planes(got, name, w, h)
    assert np.array_equal(got["rgba"].reshape(h, w, 4), gc.expected_rgba(name, w, h))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("name", ["posed", "random2"])
def test_supersampled_planes_are_the_first_sample(shader, stream, name, scale):
    """4. S = 2 and 4: the planes equal the dump of pixel (S*i, S*row) of the S*w x S*h target
    with `size` scaled by S; the colour equals the plain supersampled draw.  Ordered (three
    draws), row-major and the host call."""
    import sfrt
    w, h = gc.SIZES[1]
    shader.set_uniforms(gc.uniforms(name, w, h))
    shader.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, scale)
    try:
        for order in (1, 0):
            shader.set_option(sfrt.SFRT_OPT_TILE_ORDER, order)
            got, _ = draw_aux(shader, stream, w, h, repeat=3)
            plain = draw_plain(shader, stream, w, h)
            assert_planes(got, name, w, h, scale)
            assert np.array_equal(got["rgba"].reshape(h, w, 4), plain), order
        img = shader.draw_image_aux(w, h)
        assert_planes(img, name, w, h, scale)
        assert np.array_equal(img["rgba"], shader.draw_image(w, h))
        assert np.array_equal(img["rgba"].reshape(h, w, 4), plain)
    finally:
        shader.set_option(sfrt.SFRT_OPT_TILE_ORDER, 1)
        shader.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 1)
    # the first sample differs from the unsupersampled pixel somewhere: the test can tell them apart
    e1, es = gc.expected(name, w, h), gc.expected(name, w, h, scale)
    assert not np.array_equal(gc.bits(e1["depth"]), gc.bits(es["depth"]))


@pytest.mark.gpu
def test_invalid_arguments_write_nothing(shader, stream):
    """5. All planes NULL, a pitch that is no multiple of 4, a pitch below 4 * width: E_INVALID
    and every canvas keeps its poison; the plain call's own checks still apply."""
    import sfrt
    L, P = sfrt.lib(), ctypes.c_void_p
    w, h = gc.SIZES[0]
    shader.set_uniforms(gc.uniforms("default", w, h))
    bufs = {k: _canvas(w, h, 8) for k in ("rgba",) + PLANES}
    pitch = bufs["rgba"].stride(0)
    s = P(stream.cuda_stream)

    def call(planes, width=w, pix_pitch=pitch, row0=0, rows=h):
        return L.sfrt_glsl_draw_aux(shader._h, P(bufs["rgba"].data_ptr()), width, h, pix_pitch,
                                    ctypes.byref(planes) if planes is not None else None, row0,
                                    rows, s)

    def planes(**kw):
        a = sfrt.AuxPlanes()
        for k, pitch_k in kw.items():
            setattr(a, k, bufs[k].data_ptr())
            setattr(a, k + "_pitch_bytes", pitch_k)
        return a

    assert call(sfrt.AuxPlanes()) == E_INVALID
    assert call(None) == E_INVALID
    assert call(planes(depth=pitch, steps=pitch + 2)) == E_INVALID
    assert call(planes(sphere=4 * w - 4)) == E_INVALID
    assert call(planes(depth=pitch, sphere=pitch, steps=0)) == E_INVALID
    assert call(planes(depth=pitch), pix_pitch=4 * w - 4) == E_INVALID     # the plain call's checks
    assert call(planes(depth=pitch), row0=h - 1, rows=2) == E_INVALID
    host = np.full(w * h * 4, POISON, np.uint8)
    assert L.sfrt_glsl_draw_image_aux(shader._h, host.ctypes.data, None, None, None, w, h) == E_INVALID
    assert (host == POISON).all()
    shader.check(stream.cuda_stream)
    for k, b in bufs.items():
        assert (b.cpu().numpy() == POISON).all(), k
    # a NULL plane's pitch is ignored
    a = planes(depth=pitch)
    a.sphere_pitch_bytes = 3
    assert call(a) == 0
    shader.check(stream.cuda_stream)
    assert_planes({"depth": _plane(bufs["depth"], w, "depth")}, "default", w, h, planes=("depth",))


@pytest.mark.gpu
def test_plain_ordered_draw_after_an_aux_draw(shader, stream):
    """6. The aux draw joins its stream's tile chain as a plain draw does: plain and aux draws
    interleaved on one stream, the uniforms changing in between, all equal the restatement."""
    w, h = gc.SIZES[1]
    for name in ("posed", "random3", "posed"):
        shader.set_uniforms(gc.uniforms(name, w, h))
        got, _ = draw_aux(shader, stream, w, h, repeat=2)
        assert_planes(got, name, w, h)
        plain = draw_plain(shader, stream, w, h, repeat=2)
        assert np.array_equal(plain, gc.expected_rgba(name, w, h)), name
        got, _ = draw_aux(shader, stream, w, h)
        assert_planes(got, name, w, h)
        assert np.array_equal(got["rgba"].reshape(h, w, 4), plain), name
