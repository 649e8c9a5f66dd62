"""SFRT_OPT_SUPERSAMPLE on the voxel and GLSL renderers: S x S samples per pixel, box-filtered
inside the kernel (k_voxel_ordered_ss, k_glsl_ss, k_glsl_ordered_ss).

The reference of every case is the numpy box filter of the oracle's S*W x S*H frame,
out_c = (sum of the S*S sample bytes + S*S/2) >> log2(S*S) for each of the four channels
(include/sfrt.h), compared byte for byte: the samples of a supersampled voxel pixel are the
pixels of World::UpdateImage at the larger size, those of a GLSL pixel the fragments of the
larger render target (`size` scaled by S, nothing else changed).  Frames are 101x37: the sample
grids 202x74 and 404x148 are ragged against the 8x8 tile at both factors.
"""
import functools
import os
import re

import numpy as np
import pytest

import glsl_scenes as gs
import scenes
import voxel_scenes as vs
from conftest import ROOT, host_threads, poisoned

W, H = 101, 37
POISON = 0xA5
BANDS = ((0, 5), (5, 13), (18, 19))
SHIFT = {2: 2, 4: 4}


def box_filter(big, width, height, s):
    """(height, width, 4) uint8 from the flat RGBA8 frame of s*width x s*height pixels."""
    if s == 1:
        out = np.array(big, dtype=np.uint8).reshape(height, width, 4)
    else:
        sums = big.reshape(height, s, width, s, 4).astype(np.uint32).sum(axis=(1, 3))
        out = ((sums + s * s // 2) >> SHIFT[s]).astype(np.uint8)
    out.setflags(write=False)
    return out


def _diff(got, want):
    got = np.asarray(got).reshape(want.shape)
    return int(np.count_nonzero((got != want).any(axis=-1)))


def _device_frames(fill, frames=3, pad=16, rows=H):
    """`frames` fills back to back on one stream (the adaptive tile order sorts from the second
    on) into poisoned buffers with pitch 4 * W + pad; fill(ptr, pitch, stream).  (rows, pitch)
    arrays."""
    import torch
    pitch = 4 * W + pad
    stream = torch.cuda.Stream()
    bufs = [poisoned((rows, pitch), POISON) for _ in range(frames)]
    for b in bufs:
        fill(b.data_ptr(), pitch, stream.cuda_stream)
    stream.synchronize()
    return [b.cpu().numpy() for b in bufs], stream


def _check_option_semantics(obj, default_order):
    """Default 1, round trip, refusals that leave the stored factor alone, unknown options."""
    import sfrt
    assert obj.get_option(sfrt.SFRT_OPT_SUPERSAMPLE) == 1
    assert obj.get_option(sfrt.SFRT_OPT_TILE_ORDER) == default_order
    for s in (2, 4, 1, 2):
        obj.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
        assert obj.get_option(sfrt.SFRT_OPT_SUPERSAMPLE) == s
    for bad in (0, 3, 8, -1):
        with pytest.raises(sfrt.SfrtError) as e:
            obj.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, bad)
        assert e.value.code == -1  # SFRT_E_INVALID
        assert obj.get_option(sfrt.SFRT_OPT_SUPERSAMPLE) == 2
    for order in (2, 0, 1):
        obj.set_option(sfrt.SFRT_OPT_TILE_ORDER, order)
        assert obj.get_option(sfrt.SFRT_OPT_TILE_ORDER) == order
    assert obj.get_option(sfrt.SFRT_OPT_SUPERSAMPLE) == 2
    with pytest.raises(sfrt.SfrtError) as e:
        obj.get_option(99)
    assert e.value.code == -1
    with pytest.raises(sfrt.SfrtError):
        obj.set_option(99, 1)


# ---------------------------------------------------------------- voxel

VOXEL_POSES = [((15.5, 1.9, 15.5), 0.0, 0.0), ((20.5, 2.2, 40.5), 1.0, 0.1),
               ((30.25, 2.6, 12.75), 2.2, 0.25), ((47.5, 1.5, 60.1), 4.0, -0.3)]


@functools.lru_cache(maxsize=None)
def _assets():
    return vs.load_textures()


def _filtered_voxel(scene, width, height, s):
    """The filtered oracle frame; the oracle must have read no texel outside its texture."""
    import oracle
    tex, dyn = _assets()
    o = oracle.VoxelOracle(scene, s * width, s * height, tex, dyn, vs.COLORS)
    big = o.render(host_threads())
    assert o.bad_texel_reads() == 0, (s, width, height)
    return box_filter(big, width, height, s)


@functools.lru_cache(maxsize=None)
def voxel_reference(pose, s):
    return _filtered_voxel(vs.default_world(*VOXEL_POSES[pose]), W, H, s)


@functools.lru_cache(maxsize=None)
def voxel_random_reference(seed, s):
    return _filtered_voxel(vs.random_world(seed)[0], 67, 29, s)


def _voxel(scene, s, width=W, height=H):
    import sfrt
    tex, dyn = _assets()
    v = sfrt.VoxelWorld(0)
    v.load_assets(tex, dyn, vs.COLORS)
    v.set_scene(scene, width, height)
    v.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("pose", range(len(VOXEL_POSES)))
def test_voxel_full_frame_equals_filtered_oracle(built, pose, s):
    with _voxel(vs.default_world(*VOXEL_POSES[pose]), s) as v:
        assert _diff(v.render(), voxel_reference(pose, s)) == 0
    # the option is not ignored: the reference is not the 1x frame
    assert _diff(voxel_reference(pose, 1), voxel_reference(pose, s)) > 0.3 * W * H


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 4])
def test_voxel_ordered_kernel(built, s):
    """SFRT_OPT_TILE_ORDER 1 (the kernels that record the tile cost): three render_band fills
    back to back equal the reference, the pitch padding untouched."""
    import sfrt
    want = voxel_reference(2, s)
    with _voxel(vs.default_world(*VOXEL_POSES[2]), s) as v:
        v.set_option(sfrt.SFRT_OPT_TILE_ORDER, 1)
        frames, stream = _device_frames(lambda p, pitch, st: v.render_band(p, pitch, 0, H, st))
        v.check(stream.cuda_stream)
    for k, got in enumerate(frames):
        assert _diff(got[:, :4 * W], want) == 0, k
        assert (got[:, 4 * W:] == POISON).all(), k


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("stride", [(3, 8, 1, 4), (0, 1, 2, 3)])
def test_voxel_strides_address_output_pixels(built, stride, s):
    ystart, yadd, xstart, xadd = stride
    want = voxel_reference(1, s)
    canvas = np.full((H, W, 4), POISON, dtype=np.uint8)
    with _voxel(vs.default_world(*VOXEL_POSES[1]), s) as v:
        v.update_image(canvas.reshape(-1), ystart, yadd, xstart, xadd)
    hit = np.zeros((H, W), dtype=bool)
    hit[ystart::yadd, xstart::xadd] = True
    assert hit.sum() > 1
    assert np.array_equal(canvas[hit], want[hit])
    assert (canvas[~hit] == POISON).all()


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 4])
def test_voxel_bands_tile_the_frame(built, s):
    import torch
    want = voxel_reference(3, s)
    pitch = 4 * W
    stream = torch.cuda.Stream()
    with _voxel(vs.default_world(*VOXEL_POSES[3]), s) as v:
        frame = poisoned((H, pitch), POISON)
        for row0, rows in BANDS:
            v.render_band(frame.data_ptr() + row0 * pitch, pitch, row0, rows, stream.cuda_stream)
        alone = poisoned((H, pitch), POISON)
        v.render_band(alone.data_ptr() + 5 * pitch, pitch, 5, 13, stream.cuda_stream)
        v.check(stream.cuda_stream)
        assert _diff(frame.cpu().numpy(), want) == 0
        alone = alone.cpu().numpy().reshape(H, W, 4)
    assert np.array_equal(alone[5:18], want[5:18])
    assert (alone[:5] == POISON).all() and (alone[18:] == POISON).all()


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("seed", range(1, 9))
def test_voxel_random_worlds(built, seed, s):
    with _voxel(vs.random_world(seed)[0], s, 67, 29) as v:
        assert _diff(v.render(), voxel_random_reference(seed, s)) == 0


@pytest.mark.gpu
def test_voxel_factor_switching(built):
    """1 -> 2 -> 4 -> 1 on one object and one scene with no other setter in between: the
    per-sample tables are rebuilt at every change."""
    import sfrt
    with _voxel(vs.default_world(*VOXEL_POSES[2]), 1) as v:
        for s in (1, 2, 4, 1):
            v.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
            assert _diff(v.render(), voxel_reference(2, s)) == 0, s


@pytest.mark.gpu
def test_voxel_option_semantics(built):
    import sfrt
    with sfrt.VoxelWorld(0) as fresh:
        _check_option_semantics(fresh, 0)
    with _voxel(vs.default_world(*VOXEL_POSES[0]), 4) as v:
        fn = sfrt.lib().sfrt_voxel_update_image
        canvas = np.full(64, POISON, dtype=np.uint8)
        # S * width does not fit an int (one addressed pixel: the canvas would be large enough)
        assert sfrt.lib().sfrt_voxel_set_size(v._h, 0x30000000, 1) == 0
        assert fn(v._h, canvas.ctypes.data, 0, 1, 0, 0x30000000) == -1
        # S * width and S * height fit, their 2^16 x 2^16 tiles are more than one launch takes
        assert sfrt.lib().sfrt_voxel_set_size(v._h, 1 << 17, 1 << 17) == 0
        assert fn(v._h, canvas.ctypes.data, 0, 1, 0, 1) == -1
        assert (canvas == POISON).all()
        v.set_scene(vs.default_world(*VOXEL_POSES[0]), W, H)  # and renders again afterwards
        assert _diff(v.render(), voxel_reference(0, 4)) == 0


# ---------------------------------------------------------------- GLSL

def _no_walls(w, h):
    """Nothing at all: no wall to cull, no ball to march."""
    u = gs.random_uniforms(9, 1, 0, 0, w, h)
    u["sphere_count"] = u["all_spheres_count"] = 0
    return u


def _walls_only(w, h):
    return gs.random_uniforms(8, 9, 0, 0, w, h)


def _balls_without_walls(w, h):
    u = gs.random_uniforms(7, 1, 1, 6, w, h)
    u["spheres"][:-1] = u["spheres"][1:].copy()     # drop the wall: sphereCount 0
    u["uvs"][:-1] = u["uvs"][1:].copy()
    u["lights"][:-1] = u["lights"][1:].copy()
    u["sphere_count"], u["all_spheres_count"] = 0, int(u["all_spheres_count"]) - 1
    return u


def _camera_outside(w, h):
    u = gs.default_uniforms(w, h, 0.2, 0.1)
    u["campos"] = (30.0, 2.0, -25.0)
    return u


GLSL_SETS = {
    "default": lambda w, h: gs.default_uniforms(w, h, 0.7, 0.3),
    "default300": lambda w, h: gs.default_uniforms(w, h, 5.5, -0.4, frames=300),
    "random2": lambda w, h: gs.random_uniforms(2, 12, 2, 14, w, h),
    "random4": lambda w, h: gs.random_uniforms(4, 5, 0, 9, w, h),
    "no_walls": _no_walls,
    "walls_only": _walls_only,
    "balls_without_walls": _balls_without_walls,
    "camera_outside": _camera_outside,
}
MAIN_SETS = ["default", "default300", "random2", "random4"]


@functools.lru_cache(maxsize=None)
def _floor():
    tex, tw, th = scenes.load_floor()
    tex = np.array(tex, dtype=np.uint8).ravel()
    tex.setflags(write=False)
    return tex, tw, th


@functools.lru_cache(maxsize=None)
def glsl_reference(name, s, width=W, height=H):
    import oracle
    u = GLSL_SETS[name](s * width, s * height)
    big = oracle.GlslOracle(u, *_floor()).render(s * width, s * height, host_threads())
    return box_filter(big, width, height, s)


def _shader(name, s, width=W, height=H):
    import sfrt
    g = sfrt.GlslShader(0)
    g.set_ground(*_floor())
    g.set_uniforms(GLSL_SETS[name](width, height))
    g.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
    return g


def test_glsl_uniform_sets_differ_in_size_only():
    """What makes the filtered oracle frame at (S*w, S*h) the reference of a draw at (w, h)."""
    for name, make in GLSL_SETS.items():
        a, b = make(W, H), make(4 * W, 4 * H)
        assert tuple(b["size"]) == (4.0 * W, 4.0 * H), name
        b["size"] = a["size"]
        assert a.tobytes() == b.tobytes(), name


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("name", MAIN_SETS)
def test_glsl_row_major_kernel(built, name, s):
    with _shader(name, s) as g:
        assert _diff(g.draw_image(W, H), glsl_reference(name, s)) == 0
    assert (glsl_reference(name, s)[..., 3] == 255).all()
    assert _diff(glsl_reference(name, 1), glsl_reference(name, s)) > 0.3 * W * H


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("name", ["default", "random2"])
def test_glsl_draw_into_device_frame(built, name, s, order):
    """sfrt_glsl_draw, adaptive order (k_glsl_ordered_ss) and row-major (k_glsl_ss): three draws
    back to back equal the reference, the pitch padding untouched."""
    import sfrt
    want = glsl_reference(name, s)
    with _shader(name, s) as g:
        g.set_option(sfrt.SFRT_OPT_TILE_ORDER, order)
        frames, stream = _device_frames(lambda p, pitch, st: g.draw(p, W, H, pitch, 0, H, st))
        g.check(stream.cuda_stream)
    for k, got in enumerate(frames):
        assert _diff(got[:, :4 * W], want) == 0, k
        assert (got[:, 4 * W:] == POISON).all(), k


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 4])
def test_glsl_bands_tile_the_frame(built, s):
    import torch
    want = glsl_reference("default300", s)
    pitch = 4 * W
    stream = torch.cuda.Stream()
    with _shader("default300", s) as g:
        frame = poisoned((H, pitch), POISON)
        for row0, rows in BANDS:
            g.draw(frame.data_ptr() + row0 * pitch, W, H, pitch, row0, rows, stream.cuda_stream)
        alone = poisoned((H, pitch), POISON)
        g.draw(alone.data_ptr() + 5 * pitch, W, H, pitch, 5, 13, stream.cuda_stream)
        g.check(stream.cuda_stream)
        assert _diff(frame.cpu().numpy(), want) == 0
        alone = alone.cpu().numpy().reshape(H, W, 4)
    assert np.array_equal(alone[5:18], want[5:18])
    assert (alone[:5] == POISON).all() and (alone[18:] == POISON).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["no_walls", "walls_only", "balls_without_walls",
                                  "camera_outside"])
def test_glsl_culling_special_cases(built, name):
    """The wall cull's and the march's degenerate inputs, S = 2, both kernels."""
    import sfrt
    want = glsl_reference(name, 2)
    with _shader(name, 2) as g:
        assert _diff(g.draw_image(W, H), want) == 0
        g.set_option(sfrt.SFRT_OPT_TILE_ORDER, 1)
        frames, stream = _device_frames(lambda p, pitch, st: g.draw(p, W, H, pitch, 0, H, st),
                                        frames=1, pad=0)
        g.check(stream.cuda_stream)
    assert _diff(frames[0], want) == 0


@pytest.mark.gpu
def test_glsl_factor_switching_and_size(built):
    """1 -> 2 -> 4 -> 1 on one shader with no other setter in between, then `size` set by name
    after the option: the frame is the reference for the new size."""
    import sfrt
    with _shader("default", 1) as g:
        for s in (1, 2, 4, 1):
            g.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
            assert _diff(g.draw_image(W, H), glsl_reference("default", s)) == 0, s
        g.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 2)
        g.set_uniform("size", (67.0, 29.0))
        assert _diff(g.draw_image(67, 29), glsl_reference("default", 2, 67, 29)) == 0


@pytest.mark.gpu
def test_glsl_option_semantics(built):
    import sfrt
    with sfrt.GlslShader(0) as fresh:
        _check_option_semantics(fresh, 1)
    with _shader("default", 2) as g:
        # S * width reaches 2^24: refused, nothing written (the buffer holds the whole row)
        width = 1 << 23
        row = poisoned((1, 4 * width), POISON)
        with pytest.raises(sfrt.SfrtError) as e:
            g.draw(row.data_ptr(), width, 1, 4 * width, 0, 1)
        assert e.value.code == -1
        with pytest.raises(sfrt.SfrtError) as e:
            g.draw_image(1, 1 << 23)
        assert e.value.code == -1
        g.check()
        assert bool((row == POISON).all())
        assert _diff(g.draw_image(W, H), glsl_reference("default", 2)) == 0


# ---------------------------------------------------------------- ABI (no GPU)

def test_get_option_entry_points_are_exported_and_declared(built):
    import sfrt
    text = open(os.path.join(ROOT, "include", "sfrt.h")).read()
    for sym, handle in (("sfrt_voxel_get_option", "sfrt_voxel"), ("sfrt_glsl_get_option", "sfrt_glsl")):
        assert hasattr(sfrt.lib(), sym)
        assert sym in sfrt.ABI_SYMBOLS
        assert re.search(rf"SFRT_API\s+int\s+{sym}\(const\s+{handle}\*\s*\w+,\s*int\s+option,\s*"
                         rf"int\*\s*value\);", text)
    assert sfrt.lib().sfrt_version() >= 4
