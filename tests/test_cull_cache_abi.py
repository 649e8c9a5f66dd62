"""The cull cache's entry point (include/sfrt.h sfrt_world_cull_cache_stats) without a GPU:
exported, declared, listed, null arguments refused before any device use."""
import ctypes
import os

from conftest import ROOT

E_INVALID = -1


def test_symbol_resolves_and_is_declared(built):
    import sfrt
    lib = sfrt.lib()
    header = open(os.path.join(ROOT, "include", "sfrt.h")).read()
    assert lib.sfrt_version() >= 13
    assert hasattr(lib, "sfrt_world_cull_cache_stats")
    assert "sfrt_world_cull_cache_stats" in sfrt.ABI_SYMBOLS
    assert "SFRT_API int sfrt_world_cull_cache_stats(" in header
    hpp = open(os.path.join(ROOT, "include", "sfrt.hpp")).read()
    assert "GetCullCacheStats" in hpp


def test_null_arguments_are_refused(built):
    import sfrt
    lib = sfrt.lib()
    v = ctypes.c_int64()
    p = ctypes.byref(v)
    assert lib.sfrt_world_cull_cache_stats(None, p, p, p) == E_INVALID
