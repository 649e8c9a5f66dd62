"""The GLSL view batch's entry points (include/sfrt.h sfrt_glsl_render_views and its _aux form)
without a GPU: exported, declared, listed, a NULL shader refused before any device use, the C++
mirror compiled and linked, and the reference-side facts that keep the GPU comparisons of
tests/test_glsl_views.py from being vacuous (on the restatement alone).
"""
import ctypes
import os
import subprocess

import numpy as np

import glsl_views_cases as gc
from conftest import ROOT

E_INVALID = -1
NAMES = ("sfrt_glsl_render_views", "sfrt_glsl_render_views_aux")


def test_symbols_resolve_and_are_declared(built):
    import sfrt
    lib = sfrt.lib()
    header = open(os.path.join(ROOT, "include", "sfrt.h")).read()
    assert lib.sfrt_version() >= 18
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in sfrt.ABI_SYMBOLS, name
        assert f"SFRT_API int {name}(" in header, name
    assert hasattr(sfrt.GlslShader, "render_views") and hasattr(sfrt.GlslShader, "render_views_aux")
    hpp = open(os.path.join(ROOT, "include", "sfrt.hpp")).read()
    assert "void drawViews(" in hpp and "void drawViewsAux(" in hpp


def test_null_shader_is_refused(built):
    """Checked first: no device is touched (this test runs without one)."""
    import sfrt
    lib = sfrt.lib()
    frame = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(frame)
    views = (sfrt.View * 2)()
    for v in views:
        v.dev_pixels = p
        v.cam.fov_h, v.cam.fov_v = 1.0, 0.5
    planes = (sfrt.AuxPlanes * 2)()
    for q in planes:
        q.depth, q.depth_pitch_bytes = p, 16
    assert lib.sfrt_glsl_render_views(None, views, 2, 4, 1, 16, 0, None) == E_INVALID
    assert lib.sfrt_glsl_render_views_aux(None, views, planes, 2, 4, 1, 16, 0, None) == E_INVALID
    assert lib.sfrt_glsl_render_views(None, views, 0, 4, 1, 16, 0, None) == E_INVALID
    assert bytes(frame) == bytes(64)


def test_cpp_mirror_compiles_and_links(built, tmp_path):
    """tests/native/cpp_glsl_views_check.cpp uses Shader::drawViews and drawViewsAux; it compiles
    with warnings as errors and links against libsfrt.so.  Run without arguments it calls the C
    entry points with a NULL shader alone, which needs no device."""
    exe = tmp_path / "cpp_glsl_views_check"
    lib_dir = os.path.join(ROOT, "sfml-software-raytracer_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "cpp_glsl_views_check.cpp"), "-L", lib_dir,
                    "-lsfrt", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath-link,/opt/rocm/lib",
                    "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", str(exe)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "failures=0" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- the reference side

def test_expected_frames_are_pairwise_different():
    """Eight cameras, eight frames; gc.frame raises if a pixel of a view reaches the march cap."""
    frames = [gc.frame(k).tobytes() for k in range(len(gc.CAMS))]
    assert len(gc.CAMS) == 8 and len(set(frames)) == 8


def test_views_hold_walls_balls_and_step_counts():
    """Views 0, 1, 2, 6 and 7 each hold a wall pixel, a ball pixel and two distinct step counts.
    Measured on the restatement: wall / ball pixels 565 / 286, 499 / 352, 845 / 6, 714 / 137,
    722 / 129."""
    for k in (0, 1, 2, 6, 7):
        e = gc.planes(k)
        walls, balls = int((e["checkstep"] == 1).sum()), int((e["checkstep"] == 0).sum())
        assert walls > 0 and balls > 0 and len(np.unique(e["steps"])) >= 2, (k, walls, balls)


def test_wall_start_differs_over_the_views():
    u = gc.base_uniforms()
    sc = int(u["sphere_count"])
    starts = [gc.wall_start(u, cam[0]) for cam in gc.CAMS]
    assert len(set(starts)) >= 3, starts
    assert starts[3] == 3 * sc and starts[2] != starts[0], starts
    assert any(np.signbit(np.float32(c)) and c == 0 for c in gc.CAMS[4][0])


def test_lit_shortcut_differs_over_the_views():
    """View 5 is at least 1000 from every shadow ball (no pair may keep the shortcut there), view 0
    has a pair that keeps it: a batch holding both must not shade one with the other's table."""
    u = gc.base_uniforms()
    far = gc.shadow_pairs(u, gc.CAMS[5][0])
    assert far and all(dcam >= 1000.0 for _, dcam in far), far
    near = gc.shadow_pairs(u, gc.CAMS[0][0])
    assert any(0.0 < sanglet < 1.0 and dcam < 1000.0 for sanglet, dcam in near), near


def test_extra_scenes_and_supersampled_views_render():
    """The three extra scenes from three cameras each and the S = 2 views stay below the march cap
    (gc.frame raises otherwise) and differ per camera; many_walls has more than 64 walls.  Without
    walls the wall distance is 0 and the march never starts: one flat frame from every camera."""
    for name in gc.EXTRA:
        frames = [gc.frame(k, 1, name).tobytes() for k in range(3)]
        assert len(set(frames)) == (1 if name == "no_walls" else 3), name
    assert int(gc.EXTRA["many_walls"]()["sphere_count"]) > 64
    assert int(gc.EXTRA["no_walls"]()["sphere_count"]) == 0
    for k in gc.SS_VIEWS:
        assert gc.frame(k, 2).tobytes() != gc.frame(k).tobytes(), k
