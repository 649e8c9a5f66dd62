"""The in-place subset fill's entry points (include/sfrt.h sfrt_world_render_subset and its three
siblings) without a GPU: exported, declared, a NULL world refused before any device use, and the
C++ mirror with its new members compiles.
"""
import ctypes
import os
import subprocess

from conftest import ROOT

E_INVALID = -1
NAMES = ("sfrt_world_render_subset", "sfrt_world_render_subset_aux",
         "sfrt_voxel_render_subset", "sfrt_voxel_render_subset_aux")


def test_symbols_resolve_and_are_declared(built):
    import sfrt
    lib = sfrt.lib()
    header = open(os.path.join(ROOT, "include", "sfrt.h")).read()
    assert lib.sfrt_version() >= 11
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in sfrt.ABI_SYMBOLS, name
        assert f"SFRT_API int {name}(" in header, name


def test_null_world_is_refused(built):
    """Checked first: no device is touched (this test runs without one)."""
    import sfrt
    lib = sfrt.lib()
    frame = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(frame)
    planes = sfrt.AuxPlanes(depth=p, depth_pitch_bytes=16)
    vplanes = sfrt.VoxelAuxPlanes(depth=p, depth_pitch_bytes=16)
    assert lib.sfrt_world_render_subset(None, p, 16, 0, 1, 0, 1, None) == E_INVALID
    assert lib.sfrt_world_render_subset_aux(None, p, 16, ctypes.byref(planes), 0, 1, 0, 1,
                                            None) == E_INVALID
    assert lib.sfrt_voxel_render_subset(None, p, 16, 0, 1, 0, 1, None) == E_INVALID
    assert lib.sfrt_voxel_render_subset_aux(None, p, 16, ctypes.byref(vplanes), 0, 1, 0, 1,
                                            None) == E_INVALID
    assert bytes(frame) == bytes(64)


def test_cpp_mirror_compiles(tmp_path):
    """include/sfrt.hpp with UpdateImageDevice[Aux], RenderCycles, fullCycles and cycle on both
    world classes: a translation unit that uses every new member passes g++ -fsyntax-only."""
    src = tmp_path / "use_subset.cpp"
    src.write_text("""
#include "sfrt.hpp"
template <class World, class Planes>
int use(World& w, void* frame, void* stream) {
  Planes planes{};
  planes.depth = frame;
  planes.depth_pitch_bytes = 4 * w.width;
  w.UpdateImageDevice(frame, 4 * w.width, 0, 8, 3, 4, stream);
  w.UpdateImageDeviceAux(frame, 4 * w.width, planes, 0, 8, 3, 4, stream);
  w.fullCycles = 4;
  w.cycle = 0;
  w.RenderCycles(frame, 4 * w.width, 4, stream);
  return w.cycle;
}
int both(sfrt::SphereWorld& s, sfrt::VoxelWorld& v, void* frame) {
  return use<sfrt::SphereWorld, sfrt_aux_planes>(s, frame, nullptr) +
         use<sfrt::VoxelWorld, sfrt_voxel_aux_planes>(v, frame, nullptr);
}
""")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), str(src)], check=True)
