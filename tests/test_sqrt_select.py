"""sqrt_cr_normal (csrc/sfrt_device.h) picks the correctly rounded root among v_sqrt_f32's result
and its two neighbours by the sign bits of two fma residuals (csrc/sfrt_math.h sqrt_select).

- the selection itself on the host, for the correctly rounded root and both neighbours as r
  (tests/native/sqrt_select_host_check.cpp; no GPU);
- the device function against the compare-and-select form it replaced, every binary32 pattern
  from 2^-96 to +inf, and the pass body's `rad - q` below 2^-96
  (tests/native/sqrt_select_check.hip);
- small frames against the oracles: 72x20 and 33x9 hold partial 32x8 tiles and clamped edge
  lanes, at four pixels per lane and at the width the library picks; one_sphere marches from
  the SGPR slots, default10 and lcg64 through the window, lcg256 through the culled list, lcg64
  with culling off through every sphere.  Four frames of one view: the first runs the uncached
  kernel in row-major order, the second fills the ray cache and is the cached kernel in
  row-major order, the third and fourth are the cached kernel in the sorted tile order
  (sfrt_world_ray_cache_stats tells); with SFRT_OPT_TILE_ORDER off the uncached kernel serves
  every frame.  Then the GLSL and voxel default scenes at 64x36.
"""
import os
import subprocess

import numpy as np
import pytest

import test_ray_cache as rc
from conftest import ROOT, host_threads, poisoned

CSRC = os.path.join(ROOT, "sfml-software-raytracer_amd", "csrc")


def test_selection_on_the_host(tmp_path):
    exe = tmp_path / "sqrt_select_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "sqrt_select_host_check.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mismatches=0" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_device_root_matches_the_select_form(tmp_path):
    exe = tmp_path / "sqrt_select_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                    os.path.join(ROOT, "tests", "native", "sqrt_select_check.hip"),
                    "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mismatches=0" in r.stdout, r.stdout + r.stderr


# --- frames ------------------------------------------------------------------------------------
POSES = {"one_sphere": (0.0, 0.0), "default10": (0.7, 0.3), "lcg64": (0.0, 0.0),
         "lcg256": (2.0, 0.4)}
SCENES = [("one_sphere", 1), ("default10", 1), ("lcg64", 1), ("lcg256", 1), ("lcg64", 0)]  # name, cull
SIZES = [(72, 20), (33, 9)]


def render_frames(name, cull, width, height, rays, order, count):
    """`count` frames of one view on one stream: [(bytes, (cached_frames, fills))]."""
    import sfrt
    import torch
    out = []
    with sfrt.World(0) as w:
        w.load_texture(*rc._floor(0))
        w.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
        w.set_option(sfrt.SFRT_OPT_CULL, cull)
        w.set_option(sfrt.SFRT_OPT_TILE_ORDER, order)
        w.set_scene(rc._scene(name, POSES[name]), width, height)
        stream = torch.cuda.Stream()
        pitch = 4 * width + 16
        for _ in range(count):
            buf = poisoned((height, pitch), rc.POISON)
            w.render_band(buf.data_ptr(), pitch, 0, height, stream.cuda_stream)
            w.check(stream.cuda_stream)
            got = buf.cpu().numpy()
            assert (got[:, 4 * width:] == rc.POISON).all()
            st = w.ray_cache_stats()
            out.append((got[:, :4 * width].reshape(height, width, 4),
                        (st["cached_frames"], st["fills"])))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rays", [0, 4], ids=["auto", "r4"])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("name,cull", SCENES, ids=[n + ("" if c else "-nocull") for n, c in SCENES])
def test_small_frames_match_the_oracle(built, name, cull, size, rays):
    width, height = size
    want = rc.reference(name, 1, width, height, POSES[name])
    frames = render_frames(name, cull, width, height, rays, 1, 4)
    assert [st for _, st in frames] == [(0, 0), (1, 1), (2, 1), (3, 1)]
    for k, (got, _) in enumerate(frames):
        bad = int(np.count_nonzero((got != want).any(axis=-1)))
        assert bad == 0, f"frame {k + 1}: {bad} pixels differ from the oracle"
    for k, (got, st) in enumerate(render_frames(name, cull, width, height, rays, 0, 2)):
        assert st == (0, 0)
        bad = int(np.count_nonzero((got != want).any(axis=-1)))
        assert bad == 0, f"row-major frame {k + 1}: {bad} pixels differ from the oracle"


@pytest.mark.gpu
def test_glsl_default_scene_64x36(built):
    import glsl_scenes as gs
    import oracle
    import sfrt
    w, h = 64, 36
    tex, tw, th = rc._floor(0)
    u = gs.default_uniforms(w, h, 0.3, 0.1, frames=20)
    shader = sfrt.GlslShader(0)
    try:
        shader.set_ground(tex, tw, th)
        shader.set_uniforms(u)
        got = shader.draw_image(w, h)
    finally:
        shader.close()
    want = oracle.GlslOracle(u, tex, tw, th).render(w, h, host_threads())
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_voxel_default_scene_64x36(built):
    import oracle
    import sfrt
    import voxel_scenes as vs
    w, h = 64, 36
    vtex, vdyn = vs.load_textures()
    scene = vs.default_world((20.5, 2.2, 40.5), 1.0, 0.1)
    vw = sfrt.VoxelWorld(0)
    try:
        vw.load_assets(vtex, vdyn, vs.COLORS)
        vw.set_scene(scene, w, h)
        got = vw.render()
    finally:
        vw.close()
    want = oracle.VoxelOracle(scene, w, h, vtex, vdyn, vs.COLORS).render(host_threads())
    assert np.array_equal(got, want)
