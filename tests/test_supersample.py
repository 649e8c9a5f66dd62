"""SFRT_OPT_SUPERSAMPLE: S x S samples per pixel, box-filtered inside the frame-fill kernel.

The reference of every case is the numpy box filter of the oracle's S*W x S*H frame,
out_c = (sum of the S*S sample bytes + S*S/2) >> log2(S*S) for each of the four channels
(include/sfrt.h): the samples of a supersampled pixel are the reference's own pixels of the
larger frame, so the comparison is byte for byte.  Frames are 101x37, ragged against every
tile width at both factors (sample grids 202x74 and 404x148).
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import scenes
from conftest import ROOT, host_threads, poisoned

W, H = 101, 37
POSES = {"one_sphere": (0.0, 0.0), "default10": (0.7, 0.3), "lcg64": (1.1, -0.2),
         "lcg256": (2.0, 0.4)}
POISON = 0xA5


def _scene(name, pose=None):
    return scenes.SCENES[name]().posed(*(POSES[name] if pose is None else pose))


@functools.lru_cache(maxsize=None)
def _floor(opaque=False):
    tex, tw, th = scenes.load_floor()
    tex = np.array(tex, dtype=np.uint8).ravel()
    if opaque:
        tex[3::4] = 255
    tex.setflags(write=False)
    return tex, tw, th


@functools.lru_cache(maxsize=None)
def reference(name, s, pose=None, width=W, height=H, opaque=False):
    """(height, width, 4) uint8: the oracle's s*width x s*height frame, box-filtered."""
    import oracle
    big = oracle.Oracle.from_scene(_scene(name, pose), s * width, s * height,
                                   *_floor(opaque)).render(host_threads())
    if s == 1:
        out = big.reshape(height, width, 4).copy()
    else:
        sums = big.reshape(height, s, width, s, 4).astype(np.uint32).sum(axis=(1, 3))
        out = ((sums + s * s // 2) >> {2: 2, 4: 4}[s]).astype(np.uint8)
    out.setflags(write=False)
    return out


def _world(name, s, pose=None, width=W, height=H, opaque=False):
    import sfrt
    w = sfrt.World(0)
    w.load_texture(*_floor(opaque))
    w.set_scene(_scene(name, pose), width, height)
    w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
    return w


def _diff(got, want):
    got = np.asarray(got).reshape(want.shape)
    return int(np.count_nonzero((got != want).any(axis=-1)))


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("name", ["one_sphere", "default10", "lcg64", "lcg256"])
def test_full_frame_equals_filtered_oracle(built, name, s):
    """update_image of every fixture scene (inline and list kernels, both reduction depths)."""
    with _world(name, s) as w:
        assert _diff(w.render(), reference(name, s)) == 0
    # the option is not ignored: the reference is not the 1x frame
    assert _diff(reference(name, 1), reference(name, s)) > 0.3 * W * H


def _ordered_frames(w, frames=3, pad=16, row0=0, rows=H):
    """`frames` render_band fills back to back on one stream (the adaptive tile order sorts
    from the second on) into poisoned buffers with pitch > 4 * W; (rows, pitch) arrays."""
    import torch
    pitch = 4 * W + pad
    stream = torch.cuda.Stream()
    bufs = [poisoned((rows, pitch), POISON) for _ in range(frames)]
    for b in bufs:
        w.render_band(b.data_ptr(), pitch, row0, rows, stream.cuda_stream)
    w.check(stream.cuda_stream)
    return [b.cpu().numpy() for b in bufs]


@pytest.mark.gpu
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("rays", [1, 2, 3, 4])
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("name", ["lcg64", "lcg256"])
def test_every_tile_shape_row_major_and_ordered(built, name, s, rays, cull):
    """SFRT_OPT_RAYS_PER_LANE 1..4, culling on and off: update_image (row-major) and three
    render_band frames in the adaptive order give the reference, pitch padding untouched."""
    import sfrt
    want = reference(name, s)
    with _world(name, s) as w:
        w.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
        w.set_option(sfrt.SFRT_OPT_CULL, cull)
        assert _diff(w.render(), want) == 0
        for k, got in enumerate(_ordered_frames(w)):
            assert _diff(got[:, :4 * W], want) == 0, k
            assert (got[:, 4 * W:] == POISON).all(), k


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("stride", [(3, 8, 1, 4), (0, 1, 2, 3)])
@pytest.mark.parametrize("name", ["lcg64", "lcg256"])
def test_strides_address_output_pixels(built, name, stride, s):
    """update_image(ystart, yadd, xstart, xadd): the addressed output pixels are the
    reference's, every other byte of the caller's canvas is untouched."""
    ystart, yadd, xstart, xadd = stride
    want = reference(name, s)
    canvas = np.full((H, W, 4), POISON, dtype=np.uint8)
    with _world(name, s) as w:
        w.update_image(canvas.reshape(-1), ystart, yadd, xstart, xadd)
    hit = np.zeros((H, W), dtype=bool)
    hit[ystart::yadd, xstart::xadd] = True
    assert hit.sum() > 1
    assert np.array_equal(canvas[hit], want[hit])
    assert (canvas[~hit] == POISON).all()


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 4])
def test_bands_tile_the_frame(built, s):
    """render_band rows (0,5), (5,13), (18,19) into one frame equal the full reference; a band
    rendered alone writes its rows only."""
    import torch
    want = reference("lcg64", s)
    pitch = 4 * W
    stream = torch.cuda.Stream()
    with _world("lcg64", s) as w:
        frame = poisoned((H, pitch), POISON)
        for row0, rows in ((0, 5), (5, 13), (18, 19)):
            w.render_band(frame.data_ptr() + row0 * pitch, pitch, row0, rows, stream.cuda_stream)
        alone = poisoned((H, pitch), POISON)
        w.render_band(alone.data_ptr() + 5 * pitch, pitch, 5, 13, stream.cuda_stream)
        w.check(stream.cuda_stream)
        assert _diff(frame.cpu().numpy(), want) == 0
        alone = alone.cpu().numpy().reshape(H, W, 4)
        assert np.array_equal(alone[5:18], want[5:18])
        assert (alone[:5] == POISON).all() and (alone[18:] == POISON).all()


@pytest.mark.gpu
def test_two_frames_in_flight(built):
    """submit_frame twice (different poses) before the first wait_frame, S = 2."""
    import sfrt
    poses = [(1.1, -0.2), (0.4, 0.1)]
    sc = _scene("lcg64")
    frames = [sfrt.HostFrame(W * H * 4) for _ in poses]
    try:
        with _world("lcg64", 2) as w:
            tickets = []
            for f, p in zip(frames, poses):
                f.array[:] = POISON
                w.set_camera(sc.cam_pos, *p)
                tickets.append(w.submit_frame(f))
            for f, p, t in zip(frames, poses, tickets):
                w.wait_frame(t)
                assert _diff(f.array, reference("lcg64", 2, p)) == 0, p
    finally:
        for f in frames:
            f.free()


@pytest.mark.gpu
def test_default_and_invalid_values(built):
    import sfrt
    with _world("default10", 1) as w:
        fresh = sfrt.World(0)
        assert fresh.get_option(sfrt.SFRT_OPT_SUPERSAMPLE) == 1
        fresh.close()
        w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 2)
        assert w.get_option(sfrt.SFRT_OPT_SUPERSAMPLE) == 2
        assert _diff(w.render(), reference("default10", 2)) == 0
        for bad in (0, 3, 8, -1):
            with pytest.raises(sfrt.SfrtError) as e:
                w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, bad)
            assert e.value.code == -1
            assert w.get_option(sfrt.SFRT_OPT_SUPERSAMPLE) == 2
        w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 1)
        assert w.get_option(sfrt.SFRT_OPT_SUPERSAMPLE) == 1
        assert _diff(w.render(), reference("default10", 1)) == 0
        # the other options read back too
        w.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, 3)
        w.set_option(sfrt.SFRT_OPT_CULL, 0)
        w.set_option(sfrt.SFRT_OPT_TILE_ORDER, 0)
        assert [w.get_option(o) for o in (sfrt.SFRT_OPT_CULL, sfrt.SFRT_OPT_RAYS_PER_LANE,
                                          sfrt.SFRT_OPT_TILE_ORDER)] == [0, 3, 0]
        with pytest.raises(sfrt.SfrtError):
            w.get_option(99)
        # a sample frame wider than an int is refused before anything is queued
        w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 4)
        w.set_size(1 << 30, 1)
        dummy = poisoned((64,), POISON)
        with pytest.raises(sfrt.SfrtError) as e:
            w.render_band(dummy.data_ptr(), 4 << 30, 0, 1)
        assert e.value.code == -1
        assert (dummy.cpu().numpy() == POISON).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lcg64", "lcg256"])
def test_row_costs_are_per_output_row(built, name):
    """After ordered S = 2 fills: (row0, rows) of the band in output rows, positive costs,
    constant over each group of 8 / S = 4 rows (one tile row of samples); a fill at another
    factor is never read back."""
    import sfrt
    with _world(name, 2) as w:
        for row0, rows in ((0, H), (5, 13)):
            _ordered_frames(w, row0=row0, rows=rows)
            r0, cost = w.row_costs()
            assert (r0, cost.size) == (row0, rows)
            assert (cost > 0).all()
            for g in range(0, rows, 4):
                assert (cost[g:g + 4] == cost[g]).all(), (row0, g)
        w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 4)
        with pytest.raises(sfrt.SfrtError):
            w.row_costs()


def _rank_alpha_binary(m, rank):
    import sfrt
    wh, b = ctypes.c_void_p(), ctypes.c_int()
    assert sfrt.lib().sfrt_multi_world(m._h, rank, ctypes.byref(wh)) == 0
    assert sfrt.lib().sfrt_world_alpha_binary(wh, ctypes.byref(b)) == 0
    return bool(b.value)


@pytest.mark.gpu
def test_multi_renders_and_packs_only_uniform_alpha(built):
    """Multi([0, 0], peer copies) at 101x40, S = 2: averaged alphas are not binary, so AUTO
    sends RGBA and PACKED is refused; with every texel's alpha 255 AUTO packs again."""
    import sfrt
    height = 40
    sc = _scene("lcg64")
    for opaque in (False, True):
        want = reference("lcg64", 2, None, W, height, opaque)
        with sfrt.Multi([0, 0], sfrt.SFRT_MULTI_PEER) as m:
            m.load_texture(*_floor(opaque))
            m.set_scene(sc, W, height)
            assert _rank_alpha_binary(m, 1)  # 1x: the Floor texture's alphas are 0 or 255
            m.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, 2)
            assert _rank_alpha_binary(m, 0) == opaque and _rank_alpha_binary(m, 1) == opaque
            assert _diff(m.update_image(), want) == 0
            assert m.transfer() == (sfrt.SFRT_TRANSFER_AUTO, opaque)
            m.set_transfer(sfrt.SFRT_TRANSFER_PACKED)
            if opaque:
                assert _diff(m.update_image(), want) == 0
                assert m.transfer() == (sfrt.SFRT_TRANSFER_PACKED, True)
            else:
                with pytest.raises(sfrt.SfrtError) as e:
                    m.update_image()
                assert e.value.code == -1
            cost = m.row_costs()
            assert cost.size == height and (cost > 0).all()
        with _world("lcg64", 2, None, W, height, opaque) as w:
            assert w.alpha_binary() == opaque
    # the averaged frame really holds alphas other than 0 and 255
    assert len(np.unique(reference("lcg64", 2, None, W, height, False)[..., 3])) > 2


def test_constant_header_and_export(built):
    import sfrt
    assert sfrt.SFRT_OPT_SUPERSAMPLE == 4
    text = open(os.path.join(ROOT, "include", "sfrt.h")).read()
    assert re.search(r"^#define\s+SFRT_OPT_SUPERSAMPLE\s+4\s*$", text, re.M)
    assert hasattr(sfrt.lib(), "sfrt_world_get_option")
    assert "sfrt_world_get_option" in sfrt.ABI_SYMBOLS
