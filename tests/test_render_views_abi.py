"""The view batch's entry points (include/sfrt.h sfrt_world_render_views and its _aux form) without
a GPU: exported, declared, listed, a NULL world refused before any device use, and the C++ mirror
with its new members compiles.
"""
import ctypes
import os
import subprocess

from conftest import ROOT

E_INVALID = -1
NAMES = ("sfrt_world_render_views", "sfrt_world_render_views_aux")


def test_symbols_resolve_and_are_declared(built):
    import sfrt
    lib = sfrt.lib()
    header = open(os.path.join(ROOT, "include", "sfrt.h")).read()
    assert lib.sfrt_version() >= 12
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in sfrt.ABI_SYMBOLS, name
        assert f"SFRT_API int {name}(" in header, name
    assert "#define SFRT_MAX_VIEWS 1024" in header and sfrt.SFRT_MAX_VIEWS == 1024
    assert "#define SFRT_VIEWS_SORT 1" in header and sfrt.SFRT_VIEWS_SORT == 1
    # sfrt_view: the camera's seven floats, padding, the pointer
    assert ctypes.sizeof(sfrt.View) == 40 and sfrt.View.dev_pixels.offset == 32


def test_null_world_is_refused(built):
    """Checked first: no device is touched (this test runs without one)."""
    import sfrt
    lib = sfrt.lib()
    frame = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(frame)
    views = (sfrt.View * 2)()
    for v in views:
        v.dev_pixels = p
    planes = (sfrt.AuxPlanes * 2)()
    for q in planes:
        q.depth, q.depth_pitch_bytes = p, 16
    for flags in (0, sfrt.SFRT_VIEWS_SORT):
        assert lib.sfrt_world_render_views(None, views, 2, 16, flags, None) == E_INVALID
        assert lib.sfrt_world_render_views_aux(None, views, planes, 2, 16, flags, None) == E_INVALID
    assert lib.sfrt_world_render_views(None, views, 0, 16, 0, None) == E_INVALID
    assert bytes(frame) == bytes(64)


def test_cpp_mirror_compiles(tmp_path):
    """include/sfrt.hpp with SphereWorld::RenderViews and RenderViewsAux: a translation unit that
    uses both passes g++ -fsyntax-only."""
    src = tmp_path / "use_views.cpp"
    src.write_text("""
#include "sfrt.hpp"
void stereo(sfrt::SphereWorld& w, void* left, void* right, void* depth, void* stream) {
  std::vector<sfrt_view> views(2);
  views[0].cam = sfrt::to_c(w.cam);
  views[0].dev_pixels = left;
  views[1] = views[0];
  views[1].cam.pos[0] += 0.065f;
  views[1].dev_pixels = right;
  w.RenderViews(views, 4 * w.width, false, stream);
  w.RenderViews(views, 4 * w.width, true, stream);
  std::vector<sfrt_aux_planes> planes(2);
  planes[0].depth = depth;
  planes[0].depth_pitch_bytes = 4 * w.width;
  planes[1] = planes[0];
  w.RenderViewsAux(views, planes, 4 * w.width, true, stream);
  static_assert(SFRT_MAX_VIEWS == 1024 && SFRT_VIEWS_SORT == 1, "sfrt.h");
}
""")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), str(src)], check=True)
