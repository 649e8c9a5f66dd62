"""Python plumbing over libsfrt.so (the C ABI in include/sfrt.h).

Used by bench.py, __graft_entry__.py and the tests.  The class ``World``
mirrors the reference's ``SphereWorld`` surface for this path
(/root/reference/Raytracing/SphereWorld.h:40-78): ``width``/``height``,
``cam``, ``AddSphere``, ``UpdateSpheres`` and ``UpdateImage(ystart, yadd,
xstart, xadd)``, plus the device-resident ``render_band`` used by the display
and multi-GPU paths.  There is no CPU fallback: if libsfrt.so is missing or
has no HIP device, construction raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SFRT_LIB: another build of the same library (build-flag A/B timing in tools/ only;
# bench.py refuses any library whose build_flavour() is not "release").
LIB_PATH = os.environ.get("SFRT_LIB") or os.path.join(HERE, "libsfrt.so")

SFRT_OPT_CULL = 1
SFRT_OPT_RAYS_PER_LANE = 2
SFRT_OPT_TILE_ORDER = 3
SFRT_OPT_SUPERSAMPLE = 4  # 1 (default), 2 or 4: S x S samples per pixel, box-filtered in the kernel
SFRT_OPT_RAY_CACHE_MB = 5  # MiB per world for cached primary ray directions (512 default, 0 off)
SFRT_OPT_HIT_CACHE_MB = 6  # MB (10^6 B) per world for cached march results, a budget of its own (512, 0 off)
SFRT_OPT_TEXEL_CACHE = 7  # the texel cache on the hit cache, under the hit cache's budget (1 default, 0 off)
SFRT_OPT_COMPACT_TEXELS = 8  # the 4-byte compact layer on the texel cache (0 off, 1 default: 4 px per lane and <= 64 spheres, 2 every eligible launch)
SFRT_OPT_PIXEL_CACHE = 9  # the finished pixels of a scene at rest, copied until a texture is loaded (0 off, 1 default: no supersampling, <= 64 spheres, an atlas the compact layer can index; 2 every plain band)
ERRORS = {
    0: "SFRT_OK", -1: "SFRT_E_INVALID", -2: "SFRT_E_EMPTY", -3: "SFRT_E_NO_TEXTURE",
    -4: "SFRT_E_TOO_MANY", -5: "SFRT_E_HIP", -6: "SFRT_E_MARCH_LIMIT", -7: "SFRT_E_TEXEL",
}

# Every symbol include/sfrt.h declares (checked by tests/test_abi.py).
ABI_SYMBOLS = (
    "sfrt_world_create", "sfrt_world_destroy", "sfrt_world_set_size", "sfrt_world_get_size",
    "sfrt_world_set_camera", "sfrt_world_get_camera", "sfrt_world_load_texture",
    "sfrt_world_add_sphere", "sfrt_world_set_spheres", "sfrt_world_get_spheres",
    "sfrt_world_set_sphere_textures", "sfrt_world_get_sphere_textures",
    "sfrt_world_update_spheres", "sfrt_world_update_image", "sfrt_world_render_band",
    "sfrt_world_check", "sfrt_world_trace_points", "sfrt_world_set_option",
    "sfrt_world_submit_frame", "sfrt_world_wait_frame", "sfrt_host_alloc", "sfrt_host_free",
    "sfrt_sort_spheres", "sfrt_deg_to_rad", "sfrt_pass_threshold", "sfrt_error_string",
    "sfrt_version", "sfrt_build_flavour",
    "sfrt_voxel_create", "sfrt_voxel_destroy", "sfrt_voxel_set_size", "sfrt_voxel_set_camera",
    "sfrt_voxel_set_view", "sfrt_voxel_set_blocks", "sfrt_voxel_load_texture",
    "sfrt_voxel_load_dyn_texture", "sfrt_voxel_set_colors", "sfrt_voxel_set_dynamics",
    "sfrt_voxel_set_lights", "sfrt_voxel_light_dd_pass", "sfrt_voxel_update_image",
    "sfrt_voxel_render_band",
    "sfrt_voxel_check", "sfrt_voxel_set_option",
    "sfrt_glsl_create", "sfrt_glsl_destroy", "sfrt_glsl_set_ground", "sfrt_glsl_set_uniforms",
    "sfrt_glsl_get_uniforms", "sfrt_glsl_set_uniform", "sfrt_glsl_set_uniform_int",
    "sfrt_glsl_draw", "sfrt_glsl_draw_image", "sfrt_glsl_check", "sfrt_glsl_set_option",
    "sfrt_png_info", "sfrt_png_decode",
    "sfrt_multi_create", "sfrt_multi_destroy", "sfrt_multi_count", "sfrt_multi_world",
    "sfrt_multi_set_size", "sfrt_multi_set_camera", "sfrt_multi_load_texture",
    "sfrt_multi_set_spheres", "sfrt_multi_add_sphere", "sfrt_multi_update_spheres",
    "sfrt_multi_set_sphere_textures", "sfrt_multi_set_option", "sfrt_multi_set_bands",
    "sfrt_multi_bands", "sfrt_multi_render", "sfrt_multi_check", "sfrt_multi_update_image",
    "sfrt_world_row_costs", "sfrt_multi_cost_bands", "sfrt_multi_row_costs", "sfrt_multi_balance",
    "sfrt_multi_set_transfer", "sfrt_multi_get_transfer", "sfrt_band_packed_bytes", "sfrt_band_pack",
    "sfrt_band_unpack", "sfrt_world_alpha_binary", "sfrt_multi_transport_library",
    "sfrt_multi_use_test_transport", "sfrt_world_get_option",
    "sfrt_voxel_get_option", "sfrt_glsl_get_option", "sfrt_world_ray_cache_stats",
    "sfrt_world_tile_record_bytes", "sfrt_world_render_band_aux", "sfrt_world_update_image_aux",
    "sfrt_world_cast_rays", "sfrt_world_cast_rays_device",
    "sfrt_voxel_render_band_aux", "sfrt_voxel_update_image_aux",
    "sfrt_voxel_cast_rays", "sfrt_voxel_cast_rays_device",
    "sfrt_voxel_cast_shadow_rays", "sfrt_voxel_cast_shadow_rays_device",
    "sfrt_glsl_draw_aux", "sfrt_glsl_draw_image_aux",
    "sfrt_glsl_cast_rays", "sfrt_glsl_cast_rays_device",
    "sfrt_world_render_subset", "sfrt_world_render_subset_aux",
    "sfrt_voxel_render_subset", "sfrt_voxel_render_subset_aux",
    "sfrt_world_render_views", "sfrt_world_render_views_aux",
    "sfrt_world_cull_cache_stats", "sfrt_world_hit_cache_stats",
    "sfrt_voxel_render_views", "sfrt_voxel_render_views_aux", "sfrt_voxel_sort_dynamics",
    "sfrt_world_texel_cache_stats", "sfrt_world_compact_cache_stats",
    "sfrt_world_pixel_cache_stats",
    "sfrt_glsl_render_views", "sfrt_glsl_render_views_aux",
)

SFRT_MAX_VIEWS = 1024
SFRT_VIEWS_SORT = 1
SFRT_VOXEL_VIEWS_DYNAMICS = 1

SFRT_MULTI_AUTO, SFRT_MULTI_RCCL, SFRT_MULTI_PEER = 0, 1, 2
SFRT_TRANSFER_AUTO, SFRT_TRANSFER_RGBA, SFRT_TRANSFER_PACKED = 0, 1, 2


class SfrtError(RuntimeError):
    def __init__(self, code: int, what: str):
        self.code = code
        super().__init__(f"{what}: {ERRORS.get(code, code)} ({code})")


class Sphere(ctypes.Structure):
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float), ("z", ctypes.c_float),
                ("radius", ctypes.c_float)]


class Camera(ctypes.Structure):
    _fields_ = [("pos", ctypes.c_float * 3), ("rotation", ctypes.c_float),
                ("hrotation", ctypes.c_float), ("fov_h", ctypes.c_float),
                ("fov_v", ctypes.c_float)]


class PixelDump(ctypes.Structure):
    _fields_ = [("pos", ctypes.c_float * 3), ("draw", ctypes.c_int32), ("iters", ctypes.c_int32),
                ("xcoord", ctypes.c_float), ("ycoord", ctypes.c_float),
                ("brightness", ctypes.c_float), ("texel", ctypes.c_uint32 * 2),
                ("rgba", ctypes.c_uint32)]


class AuxPlanes(ctypes.Structure):
    """sfrt_aux_planes: device planes of sfrt_world_render_band_aux (None = not wanted)."""
    _fields_ = [("depth", ctypes.c_void_p), ("depth_pitch_bytes", ctypes.c_int64),
                ("sphere", ctypes.c_void_p), ("sphere_pitch_bytes", ctypes.c_int64),
                ("steps", ctypes.c_void_p), ("steps_pitch_bytes", ctypes.c_int64)]


class View(ctypes.Structure):
    """sfrt_view: one view of sfrt_world_render_views, its camera and its device target."""
    _fields_ = [("cam", Camera), ("dev_pixels", ctypes.c_void_p)]


class VoxelAuxPlanes(ctypes.Structure):
    """sfrt_voxel_aux_planes: device planes of sfrt_voxel_render_band_aux (None = not wanted)."""
    _fields_ = [("depth", ctypes.c_void_p), ("depth_pitch_bytes", ctypes.c_int64),
                ("cell", ctypes.c_void_p), ("cell_pitch_bytes", ctypes.c_int64),
                ("face", ctypes.c_void_p), ("face_pitch_bytes", ctypes.c_int64),
                ("steps", ctypes.c_void_p), ("steps_pitch_bytes", ctypes.c_int64)]


VOXEL_PLANES = (("depth", np.float32), ("cell", np.int32), ("face", np.int32), ("steps", np.int32))


class RayHits(ctypes.Structure):
    """sfrt_ray_hits: the per-ray outputs of sfrt_world_cast_rays[_device] (None = not wanted)."""
    _fields_ = [("pos", ctypes.c_void_p), ("depth", ctypes.c_void_p), ("sphere", ctypes.c_void_p),
                ("steps", ctypes.c_void_p), ("rgba", ctypes.c_void_p)]


RAY_OUTPUTS = ("pos", "depth", "sphere", "steps", "rgba")


class VoxelRayHits(ctypes.Structure):
    """sfrt_voxel_ray_hits: the per-ray outputs of sfrt_voxel_cast_rays[_device] (None = not
    wanted)."""
    _fields_ = [("pos", ctypes.c_void_p), ("depth", ctypes.c_void_p), ("cell", ctypes.c_void_p),
                ("face", ctypes.c_void_p), ("steps", ctypes.c_void_p), ("rgba", ctypes.c_void_p)]


VOXEL_RAY_OUTPUTS = ("pos", "depth", "cell", "face", "steps", "rgba")
VOXEL_SHADOW_OUTPUTS = ("free", "steps")
SFRT_VOXEL_MAX_SHADOW_DIST = 4096.0

_lib = None


def lib() -> ctypes.CDLL:
    """Load libsfrt.so (raises if it was not built: no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built: run __graft_entry__.build() (make -C "
                           f"sfml-software-raytracer_amd)")
    # torch wheels bundle their own libamdhip64 (same soname).  Loading torch first
    # lets libsfrt.so bind to that one, so a process has ONE HIP runtime and torch
    # tensors / streams can be handed to render_band.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    P, c_int, c_float, vp = ctypes.POINTER, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    W = vp  # opaque sfrt_world*
    sig = {
        "sfrt_world_create": ([c_int, P(vp)], c_int),
        "sfrt_world_destroy": ([W], None),
        "sfrt_world_set_size": ([W, c_int, c_int], c_int),
        "sfrt_world_get_size": ([W, P(c_int), P(c_int)], c_int),
        "sfrt_world_set_camera": ([W, P(Camera)], c_int),
        "sfrt_world_get_camera": ([W, P(Camera)], c_int),
        "sfrt_world_load_texture": ([W, c_int, vp, c_int, c_int], c_int),
        "sfrt_world_add_sphere": ([W, c_float, c_float, c_float, c_float], c_int),
        "sfrt_world_set_spheres": ([W, vp, c_int], c_int),
        "sfrt_world_get_spheres": ([W, vp, c_int, P(c_int)], c_int),
        "sfrt_world_set_sphere_textures": ([W, vp, c_int], c_int),
        "sfrt_world_get_sphere_textures": ([W, vp, c_int, P(c_int)], c_int),
        "sfrt_world_update_spheres": ([W], c_int),
        "sfrt_world_update_image": ([W, vp, c_int, c_int, c_int, c_int], c_int),
        "sfrt_world_render_band": ([W, vp, ctypes.c_int64, c_int, c_int, vp], c_int),
        "sfrt_world_render_subset": ([W, vp, ctypes.c_int64, c_int, c_int, c_int, c_int, vp], c_int),
        "sfrt_world_render_subset_aux": ([W, vp, ctypes.c_int64, P(AuxPlanes), c_int, c_int, c_int,
                                          c_int, vp], c_int),
        "sfrt_world_render_views": ([W, P(View), c_int, ctypes.c_int64, c_int, vp], c_int),
        "sfrt_world_render_views_aux": ([W, P(View), P(AuxPlanes), c_int, ctypes.c_int64, c_int, vp],
                                        c_int),
        "sfrt_voxel_render_subset": ([vp, vp, ctypes.c_int64, c_int, c_int, c_int, c_int, vp], c_int),
        "sfrt_voxel_render_subset_aux": ([vp, vp, ctypes.c_int64, P(VoxelAuxPlanes), c_int, c_int,
                                          c_int, c_int, vp], c_int),
        "sfrt_world_render_band_aux": ([W, vp, ctypes.c_int64, P(AuxPlanes), c_int, c_int, vp],
                                       c_int),
        "sfrt_world_update_image_aux": ([W, vp, vp, vp, vp, c_int, c_int, c_int, c_int], c_int),
        "sfrt_world_cast_rays": ([W, vp, vp, ctypes.c_int64, P(RayHits)], c_int),
        "sfrt_world_cast_rays_device": ([W, vp, vp, ctypes.c_int64, P(RayHits), vp], c_int),
        "sfrt_world_check": ([W, vp], c_int),
        "sfrt_world_row_costs": ([W, vp, c_int, P(c_int), P(c_int)], c_int),
        "sfrt_multi_cost_bands": ([vp, c_int, c_int, c_float, vp, vp], c_int),
        "sfrt_multi_row_costs": ([vp, vp, c_int], c_int),
        "sfrt_multi_balance": ([vp, c_float], c_int),
        "sfrt_world_trace_points": ([W, vp, c_int, vp], c_int),
        "sfrt_world_set_option": ([W, c_int, c_int], c_int),
        "sfrt_world_get_option": ([W, c_int, P(c_int)], c_int),
        "sfrt_world_ray_cache_stats": ([W, P(ctypes.c_int64), P(ctypes.c_int64),
                                        P(ctypes.c_int64)], c_int),
        "sfrt_world_tile_record_bytes": ([W, P(ctypes.c_int64)], c_int),
        "sfrt_world_cull_cache_stats": ([W, P(ctypes.c_int64), P(ctypes.c_int64),
                                         P(ctypes.c_int64)], c_int),
        "sfrt_world_hit_cache_stats": ([W, P(ctypes.c_int64), P(ctypes.c_int64),
                                        P(ctypes.c_int64)], c_int),
        "sfrt_world_texel_cache_stats": ([W, P(ctypes.c_int64), P(ctypes.c_int64),
                                          P(ctypes.c_int64)], c_int),
        "sfrt_world_compact_cache_stats": ([W, P(ctypes.c_int64), P(ctypes.c_int64),
                                            P(ctypes.c_int64)], c_int),
        "sfrt_world_pixel_cache_stats": ([W, P(ctypes.c_int64), P(ctypes.c_int64),
                                          P(ctypes.c_int64)], c_int),
        "sfrt_world_submit_frame": ([W, vp, P(ctypes.c_int64)], c_int),
        "sfrt_world_wait_frame": ([W, ctypes.c_int64], c_int),
        "sfrt_host_alloc": ([P(vp), ctypes.c_int64], c_int),
        "sfrt_host_free": ([vp], c_int),
        "sfrt_sort_spheres": ([vp, c_int, vp], c_int),
        "sfrt_deg_to_rad": ([c_float], c_float),
        "sfrt_pass_threshold": ([c_float], c_float),
        "sfrt_error_string": ([c_int], ctypes.c_char_p),
        "sfrt_version": ([], c_int),
        "sfrt_build_flavour": ([], ctypes.c_char_p),
        "sfrt_voxel_create": ([c_int, P(vp)], c_int),
        "sfrt_voxel_destroy": ([vp], None),
        "sfrt_voxel_set_size": ([vp, c_int, c_int], c_int),
        "sfrt_voxel_set_camera": ([vp, P(Camera)], c_int),
        "sfrt_voxel_set_view": ([vp, c_float, c_float], c_int),
        "sfrt_voxel_set_blocks": ([vp, vp, c_int, c_int, c_int], c_int),
        "sfrt_voxel_load_texture": ([vp, c_int, vp, c_int, c_int], c_int),
        "sfrt_voxel_load_dyn_texture": ([vp, c_int, vp, c_int, c_int], c_int),
        "sfrt_voxel_set_colors": ([vp, vp, c_int], c_int),
        "sfrt_voxel_set_dynamics": ([vp, vp, c_int], c_int),
        "sfrt_voxel_set_lights": ([vp, vp, c_int], c_int),
        "sfrt_voxel_light_dd_pass": ([ctypes.c_float], ctypes.c_float),
        "sfrt_voxel_update_image": ([vp, vp, c_int, c_int, c_int, c_int], c_int),
        "sfrt_voxel_render_band": ([vp, vp, ctypes.c_int64, c_int, c_int, vp], c_int),
        "sfrt_voxel_render_band_aux": ([vp, vp, ctypes.c_int64, P(VoxelAuxPlanes), c_int, c_int, vp],
                                       c_int),
        "sfrt_voxel_update_image_aux": ([vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int], c_int),
        "sfrt_voxel_cast_rays": ([vp, vp, vp, vp, ctypes.c_int64, P(VoxelRayHits)], c_int),
        "sfrt_voxel_cast_rays_device": ([vp, vp, vp, vp, ctypes.c_int64, P(VoxelRayHits), vp], c_int),
        "sfrt_voxel_cast_shadow_rays": ([vp, vp, vp, vp, ctypes.c_int64, vp, vp], c_int),
        "sfrt_voxel_cast_shadow_rays_device": ([vp, vp, vp, vp, ctypes.c_int64, vp, vp, vp], c_int),
        "sfrt_voxel_render_views": ([vp, P(View), c_int, ctypes.c_int64, c_int, vp], c_int),
        "sfrt_voxel_render_views_aux": ([vp, P(View), P(VoxelAuxPlanes), c_int, ctypes.c_int64, c_int,
                                         vp], c_int),
        "sfrt_voxel_sort_dynamics": ([vp, c_int, vp], c_int),
        "sfrt_voxel_check": ([vp, vp], c_int),
        "sfrt_voxel_set_option": ([vp, c_int, c_int], c_int),
        "sfrt_voxel_get_option": ([vp, c_int, P(c_int)], c_int),
        "sfrt_glsl_create": ([c_int, P(vp)], c_int),
        "sfrt_glsl_destroy": ([vp], None),
        "sfrt_glsl_set_ground": ([vp, vp, c_int, c_int], c_int),
        "sfrt_glsl_set_uniforms": ([vp, vp], c_int),
        "sfrt_glsl_get_uniforms": ([vp, vp], c_int),
        "sfrt_glsl_set_uniform": ([vp, ctypes.c_char_p, vp, c_int], c_int),
        "sfrt_glsl_set_uniform_int": ([vp, ctypes.c_char_p, c_int], c_int),
        "sfrt_glsl_draw": ([vp, vp, c_int, c_int, ctypes.c_int64, c_int, c_int, vp], c_int),
        "sfrt_glsl_draw_image": ([vp, vp, c_int, c_int], c_int),
        "sfrt_glsl_draw_aux": ([vp, vp, c_int, c_int, ctypes.c_int64, P(AuxPlanes), c_int, c_int, vp],
                               c_int),
        "sfrt_glsl_draw_image_aux": ([vp, vp, vp, vp, vp, c_int, c_int], c_int),
        "sfrt_glsl_cast_rays": ([vp, vp, ctypes.c_int64, P(RayHits)], c_int),
        "sfrt_glsl_cast_rays_device": ([vp, vp, ctypes.c_int64, P(RayHits), vp], c_int),
        "sfrt_glsl_render_views": ([vp, P(View), c_int, c_int, c_int, ctypes.c_int64, c_int, vp],
                                   c_int),
        "sfrt_glsl_render_views_aux": ([vp, P(View), P(AuxPlanes), c_int, c_int, c_int,
                                        ctypes.c_int64, c_int, vp], c_int),
        "sfrt_glsl_check": ([vp, vp], c_int),
        "sfrt_glsl_set_option": ([vp, c_int, c_int], c_int),
        "sfrt_glsl_get_option": ([vp, c_int, P(c_int)], c_int),
        "sfrt_png_info": ([vp, ctypes.c_int64, P(c_int), P(c_int)], c_int),
        "sfrt_png_decode": ([vp, ctypes.c_int64, vp, ctypes.c_int64, P(c_int), P(c_int)], c_int),
        "sfrt_multi_create": ([vp, c_int, c_int, P(vp)], c_int),
        "sfrt_multi_destroy": ([vp], None),
        "sfrt_multi_count": ([vp, P(c_int), P(c_int)], c_int),
        "sfrt_multi_world": ([vp, c_int, P(vp)], c_int),
        "sfrt_multi_set_size": ([vp, c_int, c_int], c_int),
        "sfrt_multi_set_camera": ([vp, P(Camera)], c_int),
        "sfrt_multi_load_texture": ([vp, c_int, vp, c_int, c_int], c_int),
        "sfrt_multi_set_spheres": ([vp, vp, c_int], c_int),
        "sfrt_multi_add_sphere": ([vp, c_float, c_float, c_float, c_float], c_int),
        "sfrt_multi_update_spheres": ([vp], c_int),
        "sfrt_multi_set_sphere_textures": ([vp, vp, c_int], c_int),
        "sfrt_multi_set_option": ([vp, c_int, c_int], c_int),
        "sfrt_multi_set_bands": ([vp, vp, c_int], c_int),
        "sfrt_multi_bands": ([c_int, c_int, c_float, vp, vp], c_int),
        "sfrt_multi_render": ([vp, vp, ctypes.c_int64, vp], c_int),
        "sfrt_multi_check": ([vp], c_int),
        "sfrt_multi_set_transfer": ([vp, c_int], c_int),
        "sfrt_multi_get_transfer": ([vp, P(c_int), P(c_int)], c_int),
        "sfrt_band_packed_bytes": ([ctypes.c_int64], ctypes.c_int64),
        "sfrt_band_pack": ([vp, ctypes.c_int64, vp, vp], c_int),
        "sfrt_band_unpack": ([vp, ctypes.c_int64, vp, vp], c_int),
        "sfrt_world_alpha_binary": ([W, P(c_int)], c_int),
        "sfrt_multi_update_image": ([vp, vp], c_int),
        "sfrt_multi_transport_library": ([ctypes.c_char_p, c_int], c_int),
        "sfrt_multi_use_test_transport": ([ctypes.c_char_p], c_int),
    }
    for name, (args, res) in sig.items():
        if os.environ.get("SFRT_LIB") and not hasattr(L, name):
            continue  # an older build under A/B (tools/ab_libs.py) lacks the newer entry points
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise SfrtError(rc, what)


def _f32_rows(spheres) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(spheres, dtype=np.float32).reshape(-1, 4))


def sort_spheres(spheres, cam_pos=(0.0, 0.0, 0.0)) -> np.ndarray:
    s = _f32_rows(spheres).copy()
    cam = (ctypes.c_float * 3)(*[float(c) for c in cam_pos])
    _check(lib().sfrt_sort_spheres(s.ctypes.data, s.shape[0], cam), "sfrt_sort_spheres")
    return s


def sort_dynamics(dyn, cam_pos) -> np.ndarray:
    """A copy of `dyn` (voxel_scenes.DYN_DTYPE records) with dist_to_camera set for cam_pos and in
    the stable ascending order of sfrt_voxel_sort_dynamics: the list a camera at rest sees."""
    d = np.array(dyn, copy=True)
    if d.ndim != 1 or d.dtype.itemsize != 40 or not d.flags.c_contiguous:
        raise ValueError("dyn must be a contiguous 1-D array of sfrt_dynamic records (40 bytes)")
    if len(cam_pos) != 3:
        raise ValueError("cam_pos must have three components")
    cam = (ctypes.c_float * 3)(*[float(c) for c in cam_pos])
    _check(lib().sfrt_voxel_sort_dynamics(d.ctypes.data, d.shape[0], cam), "sfrt_voxel_sort_dynamics")
    return d


def build_flavour() -> str:
    """sfrt_build_flavour: "release" for the shipped library, "diagnostic" / "ab" otherwise."""
    return lib().sfrt_build_flavour().decode()


def deg_to_rad(deg: float) -> float:
    return lib().sfrt_deg_to_rad(float(deg))


def pass_threshold(radius: float) -> float:
    return lib().sfrt_pass_threshold(float(radius))


class HostFrame:
    """Pinned host RGBA8 frame (sfrt_host_alloc), viewable as a numpy array."""

    def __init__(self, nbytes: int):
        p = ctypes.c_void_p()
        _check(lib().sfrt_host_alloc(ctypes.byref(p), int(nbytes)), "sfrt_host_alloc")
        self.ptr = p.value
        self.nbytes = int(nbytes)
        self.array = np.ctypeslib.as_array((ctypes.c_uint8 * self.nbytes).from_address(self.ptr))

    def free(self) -> None:
        if self.ptr:
            self.array = None
            lib().sfrt_host_free(ctypes.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class World:
    """Device-backed mirror of ``SphereWorld`` for the frame-fill path."""

    def __init__(self, device: int = 0):
        h = ctypes.c_void_p()
        _check(lib().sfrt_world_create(int(device), ctypes.byref(h)), "sfrt_world_create")
        self._h = h
        self.device = device

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().sfrt_world_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # --- state ---
    def set_size(self, width: int, height: int) -> None:
        _check(lib().sfrt_world_set_size(self._h, int(width), int(height)), "set_size")

    @property
    def size(self) -> tuple[int, int]:
        w, h = ctypes.c_int(), ctypes.c_int()
        _check(lib().sfrt_world_get_size(self._h, ctypes.byref(w), ctypes.byref(h)), "get_size")
        return w.value, h.value

    def set_camera(self, pos=(0.0, 0.0, 0.0), rotation=0.0, hrotation=0.0, fov_h=None,
                   fov_v=None) -> None:
        cur = self.camera
        cam = Camera()
        for k in range(3):
            cam.pos[k] = float(pos[k])
        cam.rotation, cam.hrotation = float(rotation), float(hrotation)
        cam.fov_h = float(fov_h) if fov_h is not None else cur.fov_h
        cam.fov_v = float(fov_v) if fov_v is not None else cur.fov_v
        _check(lib().sfrt_world_set_camera(self._h, ctypes.byref(cam)), "set_camera")

    @property
    def camera(self) -> Camera:
        cam = Camera()
        _check(lib().sfrt_world_get_camera(self._h, ctypes.byref(cam)), "get_camera")
        return cam

    def load_texture(self, rgba, tex_w: int, tex_h: int, slot: int = 0) -> None:
        buf = np.ascontiguousarray(np.asarray(rgba, dtype=np.uint8).ravel())
        if buf.size != tex_w * tex_h * 4:
            raise ValueError("texture size mismatch")
        _check(lib().sfrt_world_load_texture(self._h, slot, buf.ctypes.data, tex_w, tex_h),
               "load_texture")

    def add_sphere(self, x, y, z, radius) -> None:
        _check(lib().sfrt_world_add_sphere(self._h, float(x), float(y), float(z), float(radius)),
               "add_sphere")

    def set_spheres(self, spheres) -> None:
        s = _f32_rows(spheres)
        _check(lib().sfrt_world_set_spheres(self._h, s.ctypes.data, s.shape[0]), "set_spheres")

    @property
    def spheres(self) -> np.ndarray:
        n = ctypes.c_int()
        _check(lib().sfrt_world_get_spheres(self._h, None, 0, ctypes.byref(n)), "get_spheres")
        out = np.zeros((n.value, 4), dtype=np.float32)
        _check(lib().sfrt_world_get_spheres(self._h, out.ctypes.data, n.value, ctypes.byref(n)),
               "get_spheres")
        return out

    def set_sphere_textures(self, slots) -> None:
        """Texture slot per sphere (current order): the "all textures" extension."""
        a = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).ravel())
        _check(lib().sfrt_world_set_sphere_textures(self._h, a.ctypes.data, a.size),
               "set_sphere_textures")

    @property
    def sphere_textures(self) -> np.ndarray:
        n = ctypes.c_int()
        _check(lib().sfrt_world_get_sphere_textures(self._h, None, 0, ctypes.byref(n)),
               "get_sphere_textures")
        out = np.zeros(n.value, dtype=np.int32)
        _check(lib().sfrt_world_get_sphere_textures(self._h, out.ctypes.data, n.value,
                                                    ctypes.byref(n)), "get_sphere_textures")
        return out

    def update_spheres(self) -> None:
        _check(lib().sfrt_world_update_spheres(self._h), "update_spheres")

    def set_option(self, option: int, value: int) -> None:
        _check(lib().sfrt_world_set_option(self._h, option, value), "set_option")

    def get_option(self, option: int) -> int:
        v = ctypes.c_int()
        _check(lib().sfrt_world_get_option(self._h, option, ctypes.byref(v)), "get_option")
        return v.value

    def ray_cache_stats(self) -> dict:
        """The ray cache's counters (sfrt_world_ray_cache_stats): launches that read a cache
        (the filling one included), fills, and the device bytes the caches hold now."""
        c, f, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(lib().sfrt_world_ray_cache_stats(self._h, ctypes.byref(c), ctypes.byref(f),
                                                ctypes.byref(b)), "ray_cache_stats")
        return {"cached_frames": c.value, "fills": f.value, "bytes": b.value}

    def tile_record_bytes(self) -> int:
        """Device bytes of the tile records that ride with the cached directions
        (sfrt_world_tile_record_bytes): 32 per tile of every filled cache, 0 when off."""
        b = ctypes.c_int64()
        _check(lib().sfrt_world_tile_record_bytes(self._h, ctypes.byref(b)), "tile_record_bytes")
        return b.value

    def cull_cache_stats(self) -> dict:
        """The cull cache's counters (sfrt_world_cull_cache_stats): launches preceded by a fill,
        launches that loaded their culling from a cache filled earlier, and the device bytes the
        cull caches hold now."""
        f, h, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(lib().sfrt_world_cull_cache_stats(self._h, ctypes.byref(f), ctypes.byref(h),
                                                 ctypes.byref(b)), "cull_cache_stats")
        return {"fills": f.value, "hits": h.value, "bytes": b.value}

    def hit_cache_stats(self) -> dict:
        """The hit cache's counters (sfrt_world_hit_cache_stats): launches that stored their march
        results, launches that shaded from stored results without marching, and the device bytes
        the hit caches hold now."""
        f, h, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(lib().sfrt_world_hit_cache_stats(self._h, ctypes.byref(f), ctypes.byref(h),
                                                ctypes.byref(b)), "hit_cache_stats")
        return {"fills": f.value, "hits": h.value, "bytes": b.value}

    def texel_cache_stats(self) -> dict:
        """The texel cache's counters (sfrt_world_texel_cache_stats): launches that shaded from the
        hit cache and stored their texel indices, launches that shaded from stored indices, and the
        device bytes the texel caches hold now."""
        f, h, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(lib().sfrt_world_texel_cache_stats(self._h, ctypes.byref(f), ctypes.byref(h),
                                                  ctypes.byref(b)), "texel_cache_stats")
        return {"fills": f.value, "hits": h.value, "bytes": b.value}

    def compact_cache_stats(self) -> dict:
        """The compact layer's counters (sfrt_world_compact_cache_stats): launches that shaded from
        the texel cache and stored their 4-byte records, launches that shaded from those, and the
        device bytes the compact records hold now."""
        f, h, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(lib().sfrt_world_compact_cache_stats(self._h, ctypes.byref(f), ctypes.byref(h),
                                                    ctypes.byref(b)), "compact_cache_stats")
        return {"fills": f.value, "hits": h.value, "bytes": b.value}

    def pixel_cache_stats(self) -> dict:
        """The pixel layer's counters (sfrt_world_pixel_cache_stats): launches whose band was copied
        into the layer, launches that were a copy out of it, and the device bytes the cached pixels
        hold now."""
        f, h, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(lib().sfrt_world_pixel_cache_stats(self._h, ctypes.byref(f), ctypes.byref(h),
                                                  ctypes.byref(b)), "pixel_cache_stats")
        return {"fills": f.value, "hits": h.value, "bytes": b.value}

    def set_scene(self, scene, width: int, height: int) -> None:
        """Load a scenes.Scene (spheres verbatim, camera pose) at width x height."""
        self.set_size(width, height)
        self.set_camera(scene.cam_pos, scene.rotation, scene.hrotation, scene.fov_h, scene.fov_v)
        self.set_spheres(scene.spheres)

    # --- frame fill ---
    def update_image(self, pixels: np.ndarray, ystart=0, yadd=1, xstart=0, xadd=1) -> np.ndarray:
        """SphereWorld::UpdateImage into a host RGBA8 buffer (width*height*4 bytes)."""
        w, h = self.size
        if pixels.dtype != np.uint8 or pixels.size != w * h * 4 or not pixels.flags.c_contiguous:
            raise ValueError("pixels must be a contiguous uint8 array of width*height*4")
        _check(lib().sfrt_world_update_image(self._h, pixels.ctypes.data, ystart, yadd, xstart,
                                             xadd), "update_image")
        return pixels

    def render(self) -> np.ndarray:
        w, h = self.size
        out = np.zeros(w * h * 4, dtype=np.uint8)
        return self.update_image(out)

    def render_band(self, dev_ptr: int, pitch_bytes: int, row0: int, rows: int,
                    stream: int = 0) -> None:
        """Asynchronous device fill of rows [row0, row0+rows) at dev_ptr on `stream`."""
        _check(lib().sfrt_world_render_band(self._h, ctypes.c_void_p(dev_ptr), int(pitch_bytes),
                                            int(row0), int(rows), ctypes.c_void_p(stream or None)),
               "render_band")

    def render_band_aux(self, dev_ptr: int, pitch_bytes: int, row0: int, rows: int,
                        stream: int = 0, depth=None, sphere=None, steps=None) -> None:
        """render_band plus the per-pixel planes (sfrt_world_render_band_aux): depth (float32),
        sphere and steps (int32), each None or a (device pointer, pitch in bytes) pair."""
        planes = AuxPlanes()
        for name, plane in (("depth", depth), ("sphere", sphere), ("steps", steps)):
            if plane is not None:
                setattr(planes, name, int(plane[0]))
                setattr(planes, name + "_pitch_bytes", int(plane[1]))
        _check(lib().sfrt_world_render_band_aux(self._h, ctypes.c_void_p(dev_ptr), int(pitch_bytes),
                                                ctypes.byref(planes), int(row0), int(rows),
                                                ctypes.c_void_p(stream or None)),
               "render_band_aux")

    def render_subset(self, dev_ptr: int, pitch_bytes: int, ystart: int = 0, yadd: int = 1,
                      xstart: int = 0, xadd: int = 1, stream: int = 0) -> None:
        """update_image's pixel subset in place in the whole width x height device frame at
        dev_ptr (sfrt_world_render_subset): only the addressed pixels are written; asynchronous
        on `stream`."""
        _check(lib().sfrt_world_render_subset(self._h, ctypes.c_void_p(dev_ptr), int(pitch_bytes),
                                              int(ystart), int(yadd), int(xstart), int(xadd),
                                              ctypes.c_void_p(stream or None)),
               "render_subset")

    def render_subset_aux(self, dev_ptr: int, pitch_bytes: int, ystart: int = 0, yadd: int = 1,
                          xstart: int = 0, xadd: int = 1, stream: int = 0, depth=None, sphere=None,
                          steps=None) -> None:
        """render_subset plus the same elements of the whole-frame planes (render_band_aux's
        pairs: device pointer, pitch in bytes)."""
        planes = AuxPlanes()
        for name, plane in (("depth", depth), ("sphere", sphere), ("steps", steps)):
            if plane is not None:
                setattr(planes, name, int(plane[0]))
                setattr(planes, name + "_pitch_bytes", int(plane[1]))
        _check(lib().sfrt_world_render_subset_aux(self._h, ctypes.c_void_p(dev_ptr), int(pitch_bytes),
                                                  ctypes.byref(planes), int(ystart), int(yadd),
                                                  int(xstart), int(xadd),
                                                  ctypes.c_void_p(stream or None)),
               "render_subset_aux")

    @staticmethod
    def _view_array(views):
        """A ctypes array of View from View objects or (Camera, device pointer) pairs."""
        arr = (View * max(1, len(views)))()
        for k, v in enumerate(views):
            if not isinstance(v, View):
                v = View(v[0], int(v[1]) or None)
            arr[k] = v
        return arr

    def render_views(self, views, pitch_bytes: int, sort: bool = False, stream: int = 0) -> None:
        """A batch of whole frames of this world in one launch (sfrt_world_render_views): view k
        is the frame set_camera(views[k].cam) [+ update_spheres with sort] + render_band would
        write at views[k].dev_pixels; the world itself is left as it was.  views: View objects
        or (Camera, device pointer) pairs.  Asynchronous on `stream`."""
        arr = self._view_array(views)
        _check(lib().sfrt_world_render_views(self._h, arr, len(views), int(pitch_bytes),
                                             SFRT_VIEWS_SORT if sort else 0,
                                             ctypes.c_void_p(stream or None)), "render_views")

    def render_views_aux(self, views, planes, pitch_bytes: int, sort: bool = False,
                         stream: int = 0) -> None:
        """render_views plus each view's planes (sfrt_world_render_views_aux): planes[k] is an
        AuxPlanes, or a dict of render_band_aux's (device pointer, pitch in bytes) pairs under
        "depth", "sphere" and "steps"."""
        if len(planes) != len(views):
            raise ValueError("one planes entry per view")
        arr = self._view_array(views)
        pl = (AuxPlanes * max(1, len(views)))()
        for k, p in enumerate(planes):
            if not isinstance(p, AuxPlanes):
                q = AuxPlanes()
                for name, plane in p.items():
                    if plane is not None:
                        setattr(q, name, int(plane[0]))
                        setattr(q, name + "_pitch_bytes", int(plane[1]))
                p = q
            pl[k] = p
        _check(lib().sfrt_world_render_views_aux(self._h, arr, pl, len(views), int(pitch_bytes),
                                                 SFRT_VIEWS_SORT if sort else 0,
                                                 ctypes.c_void_p(stream or None)),
               "render_views_aux")

    def update_image_aux(self, pixels: np.ndarray, depth=None, sphere=None, steps=None,
                         ystart=0, yadd=1, xstart=0, xadd=1) -> np.ndarray:
        """update_image plus host planes of width*height elements (sfrt_world_update_image_aux):
        depth float32, sphere and steps int32, each a contiguous array or None."""
        w, h = self.size
        if pixels.dtype != np.uint8 or pixels.size != w * h * 4 or not pixels.flags.c_contiguous:
            raise ValueError("pixels must be a contiguous uint8 array of width*height*4")
        ptrs = []
        for plane, dtype in ((depth, np.float32), (sphere, np.int32), (steps, np.int32)):
            if plane is not None and (plane.dtype != dtype or plane.size != w * h or
                                      not plane.flags.c_contiguous):
                raise ValueError(f"a plane must be a contiguous {np.dtype(dtype).name} array of "
                                 "width*height")
            ptrs.append(None if plane is None else plane.ctypes.data)
        _check(lib().sfrt_world_update_image_aux(self._h, pixels.ctypes.data, *ptrs, ystart, yadd,
                                                 xstart, xadd), "update_image_aux")
        return pixels

    def render_aux(self) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(rgba (h, w, 4) uint8, depth (h, w) float32, sphere (h, w) int32, steps (h, w) int32)
        of the whole frame."""
        w, h = self.size
        rgba = np.zeros((h, w, 4), dtype=np.uint8)
        depth = np.zeros((h, w), dtype=np.float32)
        sphere = np.zeros((h, w), dtype=np.int32)
        steps = np.zeros((h, w), dtype=np.int32)
        self.update_image_aux(rgba, depth, sphere, steps)
        return rgba, depth, sphere, steps

    # --- ray queries ---
    def cast_rays(self, dirs, origins=None, outputs=RAY_OUTPUTS) -> dict:
        """SphereWorld::Raycast for a batch of caller-supplied rays (sfrt_world_cast_rays).

        dirs: (N, 3) float32, un-normalised; origins: (N, 3) float32, or None for the world's
        camera position.  Returns {name: array} for the requested outputs: pos (N, 3) float32,
        depth (N,) float32, sphere and steps (N,) int32, rgba (N, 4) uint8.  An invalid ray
        (non-finite component, zero / underflowing / overflowing length) has sphere == -1 and
        zeros elsewhere."""
        dirs = np.ascontiguousarray(np.asarray(dirs, dtype=np.float32).reshape(-1, 3))
        n = dirs.shape[0]
        if origins is not None:
            origins = np.ascontiguousarray(np.asarray(origins, dtype=np.float32).reshape(-1, 3))
            if origins.shape[0] != n:
                raise ValueError("origins must hold one position per direction")
        shapes = {"pos": ((n, 3), np.float32), "depth": ((n,), np.float32),
                  "sphere": ((n,), np.int32), "steps": ((n,), np.int32), "rgba": ((n, 4), np.uint8)}
        res = {name: np.zeros(*shapes[name]) for name in outputs}
        hits = RayHits()
        for name, arr in res.items():
            # an empty array's pointer still says "requested"
            setattr(hits, name, arr.ctypes.data if n else 4)
        _check(lib().sfrt_world_cast_rays(self._h, dirs.ctypes.data if n else 4,
                                          None if origins is None else (origins.ctypes.data if n else 4),
                                          n, ctypes.byref(hits)), "cast_rays")
        return res

    def cast_rays_device(self, dirs_ptr: int, origins_ptr, count: int, stream: int = 0, pos=None,
                         depth=None, sphere=None, steps=None, rgba=None) -> None:
        """Asynchronous sfrt_world_cast_rays_device on `stream`: device pointers (ints) to
        count*3 float32 directions and origins (origins_ptr None or 0: the camera position) and
        to each wanted output; the status is left to check(stream)."""
        hits = RayHits()
        for name, ptr in zip(RAY_OUTPUTS, (pos, depth, sphere, steps, rgba)):
            if ptr:
                setattr(hits, name, int(ptr))
        _check(lib().sfrt_world_cast_rays_device(self._h, ctypes.c_void_p(dirs_ptr or None),
                                                 ctypes.c_void_p(origins_ptr or None), int(count),
                                                 ctypes.byref(hits), ctypes.c_void_p(stream or None)),
               "cast_rays_device")

    def submit_frame(self, frame: "HostFrame") -> int:
        """Pipelined full-frame fill into a pinned HostFrame; returns a ticket."""
        w, h = self.size
        if frame.nbytes < w * h * 4:
            raise ValueError("host frame too small")
        t = ctypes.c_int64()
        _check(lib().sfrt_world_submit_frame(self._h, ctypes.c_void_p(frame.ptr), ctypes.byref(t)),
               "submit_frame")
        return t.value

    def wait_frame(self, ticket: int) -> None:
        _check(lib().sfrt_world_wait_frame(self._h, int(ticket)), "wait_frame")

    def check(self, stream: int = 0) -> None:
        _check(lib().sfrt_world_check(self._h, ctypes.c_void_p(stream or None)), "check")

    def row_costs(self) -> tuple[int, np.ndarray]:
        """(row0, per-row ray-steps) of the last ordered frame fill (sfrt_world_row_costs)."""
        _, h = self.size
        out = np.zeros(max(h, 1), dtype=np.float32)
        r0, n = ctypes.c_int(), ctypes.c_int()
        _check(lib().sfrt_world_row_costs(self._h, out.ctypes.data, out.size, ctypes.byref(r0),
                                          ctypes.byref(n)), "row_costs")
        return r0.value, out[:n.value].copy()

    def alpha_binary(self) -> bool:
        """sfrt_world_alpha_binary: every loaded texel's alpha is 0 or 255 (bands pack)."""
        b = ctypes.c_int()
        _check(lib().sfrt_world_alpha_binary(self._h, ctypes.byref(b)), "alpha_binary")
        return bool(b.value)

    def trace_points(self, ij) -> list[dict]:
        ij = np.ascontiguousarray(np.asarray(ij, dtype=np.int32).reshape(-1, 2))
        out = (PixelDump * ij.shape[0])()
        _check(lib().sfrt_world_trace_points(self._h, ij.ctypes.data, ij.shape[0],
                                             ctypes.cast(out, ctypes.c_void_p)), "trace_points")
        res = []
        for d in out:
            rgba = d.rgba
            res.append({"pos": list(d.pos), "draw": d.draw, "iters": d.iters,
                        "xcoord": d.xcoord, "ycoord": d.ycoord, "brightness": d.brightness,
                        "texel": list(d.texel),
                        "rgba": [rgba & 255, (rgba >> 8) & 255, (rgba >> 16) & 255, rgba >> 24]})
        return res


class VoxelWorld:
    """Device-backed mirror of the reference's voxel ``World`` frame fill
    (World.h:58-97); the scene is a voxel_scenes.VoxelScene snapshot."""

    def __init__(self, device: int = 0):
        h = ctypes.c_void_p()
        _check(lib().sfrt_voxel_create(int(device), ctypes.byref(h)), "sfrt_voxel_create")
        self._h = h
        self.width = self.height = 0

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().sfrt_voxel_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def load_assets(self, textures, dyn_textures, colors) -> None:
        for k, (rgba, w, h) in enumerate(textures):
            buf = np.ascontiguousarray(rgba, dtype=np.uint8)
            _check(lib().sfrt_voxel_load_texture(self._h, k, buf.ctypes.data, w, h), "load_texture")
        for k, (rgba, w, h) in enumerate(dyn_textures):
            buf = np.ascontiguousarray(rgba, dtype=np.uint8)
            _check(lib().sfrt_voxel_load_dyn_texture(self._h, k, buf.ctypes.data, w, h),
                   "load_dyn_texture")
        col = np.ascontiguousarray(colors, dtype=np.uint8)
        _check(lib().sfrt_voxel_set_colors(self._h, col.ctypes.data, col.shape[0]), "set_colors")

    def load_texture(self, slot: int, rgba, w: int, h: int) -> None:
        """textures[slot] (World.h:90) alone: sfrt_voxel_load_texture, stream-ordered."""
        buf = np.ascontiguousarray(rgba, dtype=np.uint8)
        _check(lib().sfrt_voxel_load_texture(self._h, int(slot), buf.ctypes.data, int(w), int(h)),
               "load_texture")

    def set_scene(self, scene, width: int, height: int) -> None:
        self.width, self.height = int(width), int(height)
        _check(lib().sfrt_voxel_set_size(self._h, self.width, self.height), "set_size")
        cam = Camera()
        for k in range(3):
            cam.pos[k] = float(scene.cam_pos[k])
        cam.rotation, cam.hrotation = float(scene.rotation), float(scene.hrotation)
        cam.fov_h, cam.fov_v = float(scene.fov_h), float(scene.fov_v)
        _check(lib().sfrt_voxel_set_camera(self._h, ctypes.byref(cam)), "set_camera")
        _check(lib().sfrt_voxel_set_view(self._h, float(scene.shadow_distance),
                                         float(scene.view_distance)), "set_view")
        b = np.ascontiguousarray(scene.blocks, dtype=np.int16)
        _check(lib().sfrt_voxel_set_blocks(self._h, b.ctypes.data, *b.shape), "set_blocks")
        d = np.ascontiguousarray(scene.dyn)
        _check(lib().sfrt_voxel_set_dynamics(self._h, d.ctypes.data, d.shape[0]), "set_dynamics")
        l = np.ascontiguousarray(scene.lights)
        _check(lib().sfrt_voxel_set_lights(self._h, l.ctypes.data, l.shape[0]), "set_lights")

    def update_image(self, pixels: np.ndarray, ystart=0, yadd=1, xstart=0, xadd=1) -> np.ndarray:
        if pixels.dtype != np.uint8 or pixels.size != self.width * self.height * 4:
            raise ValueError("pixels must be uint8 width*height*4")
        _check(lib().sfrt_voxel_update_image(self._h, pixels.ctypes.data, ystart, yadd, xstart,
                                             xadd), "voxel_update_image")
        return pixels

    def render(self) -> np.ndarray:
        return self.update_image(np.zeros(self.width * self.height * 4, np.uint8))

    def render_band(self, dev_ptr: int, pitch_bytes: int, row0: int, rows: int,
                    stream: int = 0) -> None:
        _check(lib().sfrt_voxel_render_band(self._h, ctypes.c_void_p(dev_ptr), int(pitch_bytes),
                                            int(row0), int(rows), ctypes.c_void_p(stream or None)),
               "voxel_render_band")

    def render_band_aux(self, dev_ptr: int, pitch_bytes: int, row0: int, rows: int,
                        stream: int = 0, depth=None, cell=None, face=None, steps=None) -> None:
        """render_band plus the per-pixel planes (sfrt_voxel_render_band_aux): depth (float32),
        cell, face and steps (int32), each None or a (device pointer, pitch in bytes) pair."""
        planes = VoxelAuxPlanes()
        for name, plane in (("depth", depth), ("cell", cell), ("face", face), ("steps", steps)):
            if plane is not None:
                setattr(planes, name, int(plane[0]))
                setattr(planes, name + "_pitch_bytes", int(plane[1]))
        _check(lib().sfrt_voxel_render_band_aux(self._h, ctypes.c_void_p(dev_ptr), int(pitch_bytes),
                                                ctypes.byref(planes), int(row0), int(rows),
                                                ctypes.c_void_p(stream or None)),
               "voxel_render_band_aux")

    def render_subset(self, dev_ptr: int, pitch_bytes: int, ystart: int = 0, yadd: int = 1,
                      xstart: int = 0, xadd: int = 1, stream: int = 0) -> None:
        """update_image's pixel subset in place in the whole width x height device frame at
        dev_ptr (sfrt_voxel_render_subset): only the addressed pixels are written."""
        _check(lib().sfrt_voxel_render_subset(self._h, ctypes.c_void_p(dev_ptr), int(pitch_bytes),
                                              int(ystart), int(yadd), int(xstart), int(xadd),
                                              ctypes.c_void_p(stream or None)),
               "voxel_render_subset")

    def render_subset_aux(self, dev_ptr: int, pitch_bytes: int, ystart: int = 0, yadd: int = 1,
                          xstart: int = 0, xadd: int = 1, stream: int = 0, depth=None, cell=None,
                          face=None, steps=None) -> None:
        """render_subset plus the same elements of the whole-frame planes (render_band_aux's
        pairs: device pointer, pitch in bytes)."""
        planes = VoxelAuxPlanes()
        for name, plane in (("depth", depth), ("cell", cell), ("face", face), ("steps", steps)):
            if plane is not None:
                setattr(planes, name, int(plane[0]))
                setattr(planes, name + "_pitch_bytes", int(plane[1]))
        _check(lib().sfrt_voxel_render_subset_aux(self._h, ctypes.c_void_p(dev_ptr), int(pitch_bytes),
                                                  ctypes.byref(planes), int(ystart), int(yadd),
                                                  int(xstart), int(xadd),
                                                  ctypes.c_void_p(stream or None)),
               "voxel_render_subset_aux")

    def set_camera(self, cam: Camera) -> None:
        """World::cam alone (sfrt_voxel_set_camera); set_scene sets it with everything else."""
        _check(lib().sfrt_voxel_set_camera(self._h, ctypes.byref(cam)), "voxel_set_camera")

    def set_dynamics(self, dyn) -> None:
        """The `dyn` list alone, in list order (sfrt_voxel_set_dynamics; voxel_scenes.DYN_DTYPE)."""
        d = np.ascontiguousarray(dyn)
        if d.ndim != 1 or d.dtype.itemsize != 40:
            raise ValueError("dyn must be a 1-D array of sfrt_dynamic records (40 bytes)")
        _check(lib().sfrt_voxel_set_dynamics(self._h, d.ctypes.data, d.shape[0]), "voxel_set_dynamics")

    def render_views(self, views, pitch_bytes: int, dynamics: bool = False, stream: int = 0) -> None:
        """A batch of whole frames of this world in one launch (sfrt_voxel_render_views): view k
        is the frame set_camera(views[k].cam) [+ the list sorted for that camera with dynamics] +
        render_band would write at views[k].dev_pixels; the world itself is left as it was.
        views: View objects or (Camera, device pointer) pairs.  Asynchronous on `stream`."""
        if len(views) > SFRT_MAX_VIEWS:
            raise ValueError(f"at most {SFRT_MAX_VIEWS} views")
        arr = World._view_array(views)
        _check(lib().sfrt_voxel_render_views(self._h, arr, len(views), int(pitch_bytes),
                                             SFRT_VOXEL_VIEWS_DYNAMICS if dynamics else 0,
                                             ctypes.c_void_p(stream or None)), "voxel_render_views")

    def render_views_aux(self, views, planes, pitch_bytes: int, dynamics: bool = False,
                         stream: int = 0) -> None:
        """render_views plus each view's planes (sfrt_voxel_render_views_aux): planes[k] is a
        VoxelAuxPlanes, or a dict of render_band_aux's (device pointer, pitch in bytes) pairs
        under "depth", "cell", "face" and "steps"."""
        if len(views) > SFRT_MAX_VIEWS:
            raise ValueError(f"at most {SFRT_MAX_VIEWS} views")
        if len(planes) != len(views):
            raise ValueError("one planes entry per view")
        arr = World._view_array(views)
        pl = (VoxelAuxPlanes * max(1, len(views)))()
        for k, p in enumerate(planes):
            if not isinstance(p, VoxelAuxPlanes):
                q = VoxelAuxPlanes()
                for name, plane in p.items():
                    if name not in ("depth", "cell", "face", "steps"):
                        raise ValueError(f"unknown plane {name!r}")
                    if plane is not None:
                        setattr(q, name, int(plane[0]))
                        setattr(q, name + "_pitch_bytes", int(plane[1]))
                p = q
            pl[k] = p
        _check(lib().sfrt_voxel_render_views_aux(self._h, arr, pl, len(views), int(pitch_bytes),
                                                 SFRT_VOXEL_VIEWS_DYNAMICS if dynamics else 0,
                                                 ctypes.c_void_p(stream or None)),
               "voxel_render_views_aux")

    def update_image_aux(self, pixels: np.ndarray, depth=None, cell=None, face=None, steps=None,
                         ystart=0, yadd=1, xstart=0, xadd=1) -> np.ndarray:
        """update_image plus host planes of width*height elements (sfrt_voxel_update_image_aux):
        depth float32, cell, face and steps int32, each a contiguous array or None.  A pick of
        pixel (i, j) is xstart=i, xadd=width, ystart=j, yadd=height."""
        n = self.width * self.height
        if pixels.dtype != np.uint8 or pixels.size != n * 4 or not pixels.flags.c_contiguous:
            raise ValueError("pixels must be a contiguous uint8 array of width*height*4")
        ptrs = []
        for plane, (_, dtype) in zip((depth, cell, face, steps), VOXEL_PLANES):
            if plane is not None and (plane.dtype != dtype or plane.size != n or
                                      not plane.flags.c_contiguous):
                raise ValueError(f"a plane must be a contiguous {np.dtype(dtype).name} array of "
                                 "width*height")
            ptrs.append(None if plane is None else plane.ctypes.data)
        _check(lib().sfrt_voxel_update_image_aux(self._h, pixels.ctypes.data, *ptrs, ystart, yadd,
                                                 xstart, xadd), "voxel_update_image_aux")
        return pixels

    def render_aux(self):
        """(rgba (h, w, 4) uint8, depth (h, w) float32, cell, face, steps (h, w) int32) of the
        whole frame."""
        w, h = self.width, self.height
        rgba = np.zeros((h, w, 4), dtype=np.uint8)
        planes = [np.zeros((h, w), dtype=dt) for _, dt in VOXEL_PLANES]
        self.update_image_aux(rgba, *planes)
        return (rgba, *planes)

    # --- ray queries ---
    def cast_rays(self, dirs, yscales=None, origins=None, outputs=VOXEL_RAY_OUTPUTS) -> dict:
        """World::Raycast for a batch of caller-supplied rays (sfrt_voxel_cast_rays).

        dirs: (N, 3) float32, used verbatim; yscales: (N,) float32 or None (1.0); origins: (N, 3)
        float32, or None for the camera position (then with the billboards).  Returns
        {name: array} for the requested outputs: pos (N, 3) float32, depth (N,) float32, cell,
        face and steps (N,) int32, rgba (N, 4) uint8.  An invalid ray (a non-finite component) has
        face 0, cell -1, steps 0 and zeros elsewhere."""
        dirs = np.ascontiguousarray(np.asarray(dirs, dtype=np.float32).reshape(-1, 3))
        n = dirs.shape[0]
        if yscales is not None:
            yscales = np.ascontiguousarray(np.asarray(yscales, dtype=np.float32).ravel())
            if yscales.shape[0] != n:
                raise ValueError("yscales must hold one value per direction")
        if origins is not None:
            origins = np.ascontiguousarray(np.asarray(origins, dtype=np.float32).reshape(-1, 3))
            if origins.shape[0] != n:
                raise ValueError("origins must hold one position per direction")
        shapes = {"pos": ((n, 3), np.float32), "depth": ((n,), np.float32), "cell": ((n,), np.int32),
                  "face": ((n,), np.int32), "steps": ((n,), np.int32), "rgba": ((n, 4), np.uint8)}
        res = {name: np.zeros(*shapes[name]) for name in outputs}
        hits = VoxelRayHits()
        for name, arr in res.items():
            # an empty array's pointer still says "requested"
            setattr(hits, name, arr.ctypes.data if n else 4)
        ptr = lambda a: None if a is None else (a.ctypes.data if n else 4)
        _check(lib().sfrt_voxel_cast_rays(self._h, ptr(dirs), ptr(yscales), ptr(origins), n,
                                          ctypes.byref(hits)), "voxel_cast_rays")
        return res

    def cast_rays_device(self, dirs_ptr: int, yscales_ptr, origins_ptr, count: int, stream: int = 0,
                         pos=None, depth=None, cell=None, face=None, steps=None, rgba=None) -> None:
        """Asynchronous sfrt_voxel_cast_rays_device on `stream`: device pointers (ints) to count*3
        float32 directions, count yscales (None or 0: 1.0), count*3 origins (None or 0: the
        camera position) and to each wanted output; the status is left to check(stream)."""
        hits = VoxelRayHits()
        for name, ptr in zip(VOXEL_RAY_OUTPUTS, (pos, depth, cell, face, steps, rgba)):
            if ptr:
                setattr(hits, name, int(ptr))
        _check(lib().sfrt_voxel_cast_rays_device(self._h, ctypes.c_void_p(dirs_ptr or None),
                                                 ctypes.c_void_p(yscales_ptr or None),
                                                 ctypes.c_void_p(origins_ptr or None), int(count),
                                                 ctypes.byref(hits), ctypes.c_void_p(stream or None)),
               "voxel_cast_rays_device")

    def cast_shadow_rays(self, origins, dirs, max_dists, outputs=VOXEL_SHADOW_OUTPUTS) -> dict:
        """World::LRaycast for a batch of rays (sfrt_voxel_cast_shadow_rays): origins and dirs
        (N, 3) float32 (dirs verbatim), max_dists (N,) float32.  Returns {name: (N,) int32} for
        the requested outputs: free (1 free, 0 blocked or out of trips, -1 invalid ray) and steps
        (trips of the loop's body).  max_dist above SFRT_VOXEL_MAX_SHADOW_DIST is invalid."""
        origins = np.ascontiguousarray(np.asarray(origins, dtype=np.float32).reshape(-1, 3))
        dirs = np.ascontiguousarray(np.asarray(dirs, dtype=np.float32).reshape(-1, 3))
        max_dists = np.ascontiguousarray(np.asarray(max_dists, dtype=np.float32).ravel())
        n = dirs.shape[0]
        if origins.shape[0] != n or max_dists.shape[0] != n:
            raise ValueError("origins, dirs and max_dists must hold one entry per ray")
        res = {name: np.zeros(n, dtype=np.int32) for name in outputs}
        ptr = lambda a: None if a is None else (a.ctypes.data if n else 4)
        _check(lib().sfrt_voxel_cast_shadow_rays(self._h, ptr(origins), ptr(dirs), ptr(max_dists), n,
                                                 ptr(res.get("free")), ptr(res.get("steps"))),
               "voxel_cast_shadow_rays")
        return res

    def cast_shadow_rays_device(self, origins_ptr: int, dirs_ptr: int, max_dists_ptr: int, count: int,
                                stream: int = 0, free=None, steps=None) -> None:
        """Asynchronous sfrt_voxel_cast_shadow_rays_device on `stream` (device pointers as ints)."""
        _check(lib().sfrt_voxel_cast_shadow_rays_device(
            self._h, ctypes.c_void_p(origins_ptr or None), ctypes.c_void_p(dirs_ptr or None),
            ctypes.c_void_p(max_dists_ptr or None), int(count), ctypes.c_void_p(free or None),
            ctypes.c_void_p(steps or None), ctypes.c_void_p(stream or None)),
            "voxel_cast_shadow_rays_device")

    def check(self, stream: int = 0) -> None:
        _check(lib().sfrt_voxel_check(self._h, ctypes.c_void_p(stream or None)), "voxel_check")

    def set_option(self, option: int, value: int) -> None:
        _check(lib().sfrt_voxel_set_option(self._h, option, value), "voxel_set_option")

    def get_option(self, option: int) -> int:
        """SFRT_OPT_TILE_ORDER (0/1/2) or SFRT_OPT_SUPERSAMPLE (the factor 1, 2 or 4)."""
        v = ctypes.c_int(0)
        _check(lib().sfrt_voxel_get_option(self._h, option, ctypes.byref(v)), "voxel_get_option")
        return int(v.value)


def band_packed_bytes(pixels: int) -> int:
    """sfrt_band_packed_bytes: bytes of a packed band of `pixels` pixels (3.125 B each)."""
    b = lib().sfrt_band_packed_bytes(int(pixels))
    if b < 0:
        raise SfrtError(int(b), "band_packed_bytes")
    return int(b)


def band_pack(src_ptr: int, pixels: int, dst_ptr: int, stream: int = 0) -> None:
    """sfrt_band_pack: RGBA8 device pixels -> the packed transfer format (asynchronous)."""
    _check(lib().sfrt_band_pack(ctypes.c_void_p(src_ptr), int(pixels), ctypes.c_void_p(dst_ptr),
                                ctypes.c_void_p(stream or None)), "band_pack")


def band_unpack(src_ptr: int, pixels: int, dst_ptr: int, stream: int = 0) -> None:
    """sfrt_band_unpack: the packed transfer format -> RGBA8 device pixels (asynchronous)."""
    _check(lib().sfrt_band_unpack(ctypes.c_void_p(src_ptr), int(pixels), ctypes.c_void_p(dst_ptr),
                                  ctypes.c_void_p(stream or None)), "band_unpack")


def multi_transport_library() -> str:
    """sfrt_multi_transport_library: "" before the first RCCL context, else the library behind
    SFRT_MULTI_RCCL ("librccl.so.1", or "test:<path>" for a test transport)."""
    buf = ctypes.create_string_buffer(4096)
    _check(lib().sfrt_multi_transport_library(buf, len(buf)), "sfrt_multi_transport_library")
    return buf.value.decode()


def use_test_transport(path: str) -> None:
    """TEST ONLY (sfrt_multi_use_test_transport): the RCCL C API from `path`, before the
    process's first RCCL context."""
    _check(lib().sfrt_multi_use_test_transport(path.encode()), "sfrt_multi_use_test_transport")


def multi_bands(height: int, n: int, root_factor: float = 1.0) -> list[tuple[int, int]]:
    """sfrt_multi_bands: (row0, rows) per rank, rank 0 ~root_factor x the others' rows."""
    row0 = np.zeros(n, dtype=np.int32)
    rows = np.zeros(n, dtype=np.int32)
    _check(lib().sfrt_multi_bands(int(height), int(n), float(root_factor), row0.ctypes.data,
                                  rows.ctypes.data), "sfrt_multi_bands")
    return [(int(a), int(b)) for a, b in zip(row0, rows)]


def multi_cost_bands(row_cost, n: int, root_factor: float = 1.0) -> list[tuple[int, int]]:
    """sfrt_multi_cost_bands: (row0, rows) per rank, rank 0 ~root_factor x the others' cost."""
    c = np.ascontiguousarray(np.asarray(row_cost, dtype=np.float32))
    row0 = np.zeros(n, dtype=np.int32)
    rows = np.zeros(n, dtype=np.int32)
    _check(lib().sfrt_multi_cost_bands(c.ctypes.data if c.size else None, int(c.size), int(n),
                                       float(root_factor), row0.ctypes.data, rows.ctypes.data),
           "sfrt_multi_cost_bands")
    return [(int(a), int(b)) for a, b in zip(row0, rows)]


class Multi:
    """One frame over several GPUs of this node through the C ABI (sfrt_multi_*): the scene
    setters of ``World`` broadcast to one world per device, the frame is rendered in row
    bands and gathered on devices[0] (RCCL or peer copies)."""

    def __init__(self, devices, transport: int = SFRT_MULTI_AUTO):
        devs = np.ascontiguousarray(np.asarray(devices, dtype=np.int32))
        h = ctypes.c_void_p()
        _check(lib().sfrt_multi_create(devs.ctypes.data, devs.size, int(transport),
                                       ctypes.byref(h)), "sfrt_multi_create")
        self._h = h
        self.devices = [int(d) for d in devs]
        self.width = self.height = 0

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().sfrt_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def transport(self) -> int:
        n, t = ctypes.c_int(), ctypes.c_int()
        _check(lib().sfrt_multi_count(self._h, ctypes.byref(n), ctypes.byref(t)), "multi_count")
        return t.value

    def load_texture(self, rgba, tex_w: int, tex_h: int, slot: int = 0) -> None:
        buf = np.ascontiguousarray(np.asarray(rgba, dtype=np.uint8).ravel())
        _check(lib().sfrt_multi_load_texture(self._h, slot, buf.ctypes.data, tex_w, tex_h),
               "multi_load_texture")

    def set_camera(self, pos, rotation=0.0, hrotation=0.0, fov_h=None, fov_v=None) -> None:
        cam = Camera()
        for k in range(3):
            cam.pos[k] = float(pos[k])
        cam.rotation, cam.hrotation = float(rotation), float(hrotation)
        cam.fov_h = float(fov_h) if fov_h is not None else float(deg_to_rad(75.0))
        cam.fov_v = float(fov_v) if fov_v is not None else float(deg_to_rad(47.0))
        _check(lib().sfrt_multi_set_camera(self._h, ctypes.byref(cam)), "multi_set_camera")

    def set_scene(self, scene, width: int, height: int) -> None:
        self.width, self.height = int(width), int(height)
        _check(lib().sfrt_multi_set_size(self._h, self.width, self.height), "multi_set_size")
        self.set_camera(scene.cam_pos, scene.rotation, scene.hrotation, scene.fov_h, scene.fov_v)
        s = _f32_rows(scene.spheres)
        _check(lib().sfrt_multi_set_spheres(self._h, s.ctypes.data, s.shape[0]), "multi_set_spheres")

    def set_option(self, option: int, value: int) -> None:
        _check(lib().sfrt_multi_set_option(self._h, option, value), "multi_set_option")

    def set_transfer(self, fmt: int) -> None:
        """sfrt_multi_set_transfer: SFRT_TRANSFER_AUTO / _RGBA / _PACKED."""
        _check(lib().sfrt_multi_set_transfer(self._h, int(fmt)), "multi_set_transfer")

    def transfer(self) -> tuple[int, bool]:
        """(the transfer setting, whether the last render packed its bands)."""
        f, p = ctypes.c_int(), ctypes.c_int()
        _check(lib().sfrt_multi_get_transfer(self._h, ctypes.byref(f), ctypes.byref(p)),
               "multi_get_transfer")
        return f.value, bool(p.value)

    def set_bands(self, rows=None) -> None:
        if rows is None:
            _check(lib().sfrt_multi_set_bands(self._h, None, 0), "multi_set_bands")
            return
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int32))
        _check(lib().sfrt_multi_set_bands(self._h, r.ctypes.data, r.size), "multi_set_bands")

    def row_costs(self) -> np.ndarray:
        """Per-row ray-steps of the last frame, from every rank's band (sfrt_multi_row_costs)."""
        out = np.zeros(self.height, dtype=np.float32)
        _check(lib().sfrt_multi_row_costs(self._h, out.ctypes.data, self.height), "multi_row_costs")
        return out

    def band_costs(self, rank: int) -> tuple[int, np.ndarray]:
        """(row0, per-row ray-steps) of rank `rank`'s last band (its world's row costs)."""
        wh = ctypes.c_void_p()
        _check(lib().sfrt_multi_world(self._h, int(rank), ctypes.byref(wh)), "multi_world")
        out = np.zeros(max(self.height, 1), dtype=np.float32)
        r0, n = ctypes.c_int(), ctypes.c_int()
        _check(lib().sfrt_world_row_costs(wh, out.ctypes.data, out.size, ctypes.byref(r0),
                                          ctypes.byref(n)), "row_costs")
        return r0.value, out[:n.value].copy()

    def balance(self, root_factor: float = 1.0) -> None:
        """Cost-weighted bands from the last frame (sfrt_multi_balance)."""
        _check(lib().sfrt_multi_balance(self._h, float(root_factor)), "multi_balance")

    def render(self, dev_ptr: int, pitch_bytes: int, stream: int = 0) -> None:
        _check(lib().sfrt_multi_render(self._h, ctypes.c_void_p(dev_ptr), int(pitch_bytes),
                                       ctypes.c_void_p(stream or None)), "multi_render")

    def check(self) -> None:
        _check(lib().sfrt_multi_check(self._h), "multi_check")

    def update_image(self, pixels=None) -> np.ndarray:
        if pixels is None:
            pixels = np.zeros(self.width * self.height * 4, dtype=np.uint8)
        if pixels.dtype != np.uint8 or pixels.size != self.width * self.height * 4:
            raise ValueError("pixels must be uint8 width*height*4")
        _check(lib().sfrt_multi_update_image(self._h, pixels.ctypes.data), "multi_update_image")
        return pixels


def decode_png(data: bytes) -> tuple[np.ndarray, int, int]:
    """PNG bytes -> (RGBA8 uint8 array, width, height), as sf::Image::loadFromFile."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    w, h = ctypes.c_int(), ctypes.c_int()
    _check(lib().sfrt_png_info(buf.ctypes.data, buf.size, ctypes.byref(w), ctypes.byref(h)),
           "png_info")
    out = np.empty(w.value * h.value * 4, dtype=np.uint8)
    _check(lib().sfrt_png_decode(buf.ctypes.data, buf.size, out.ctypes.data, out.size,
                                 ctypes.byref(w), ctypes.byref(h)), "png_decode")
    return out, w.value, h.value


class GlslShader:
    """Device-backed rayShader.frag: the uniform state of
    ``SphereWorld::shader`` plus ``rt.draw(sp, &shader)``.  Uniform blocks are
    glsl_scenes.UNIFORM_DTYPE records (the layout of sfrt_glsl_uniforms)."""

    def __init__(self, device: int = 0):
        h = ctypes.c_void_p()
        _check(lib().sfrt_glsl_create(int(device), ctypes.byref(h)), "sfrt_glsl_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().sfrt_glsl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_ground(self, rgba, w: int, h: int) -> None:
        buf = np.ascontiguousarray(rgba, dtype=np.uint8)
        if buf.size != w * h * 4:
            raise ValueError("ground size mismatch")
        _check(lib().sfrt_glsl_set_ground(self._h, buf.ctypes.data, int(w), int(h)), "set_ground")

    def set_uniforms(self, u) -> None:
        rec = np.ascontiguousarray(np.asarray(u).reshape(()))
        _check(lib().sfrt_glsl_set_uniforms(self._h, rec.ctypes.data), "set_uniforms")

    def get_uniforms(self, dtype):
        rec = np.zeros((), dtype=dtype)
        _check(lib().sfrt_glsl_get_uniforms(self._h, rec.ctypes.data), "get_uniforms")
        return rec

    def set_uniform(self, name: str, value) -> None:
        """sf::Shader::setUniform: floats/vectors by name, ints for the counts."""
        if isinstance(value, (int, np.integer)):
            _check(lib().sfrt_glsl_set_uniform_int(self._h, name.encode(), int(value)), name)
            return
        v = np.ascontiguousarray(np.atleast_1d(np.asarray(value, dtype=np.float32)))
        _check(lib().sfrt_glsl_set_uniform(self._h, name.encode(), v.ctypes.data, v.size), name)

    def draw(self, dev_ptr: int, width: int, height: int, pitch_bytes: int, row0: int = 0,
             rows: int | None = None, stream: int = 0) -> None:
        rows = height - row0 if rows is None else rows
        _check(lib().sfrt_glsl_draw(self._h, ctypes.c_void_p(dev_ptr), int(width), int(height),
                                    int(pitch_bytes), int(row0), int(rows),
                                    ctypes.c_void_p(stream or None)), "glsl_draw")

    def draw_image(self, width: int, height: int) -> np.ndarray:
        out = np.zeros(width * height * 4, dtype=np.uint8)
        _check(lib().sfrt_glsl_draw_image(self._h, out.ctypes.data, int(width), int(height)),
               "glsl_draw_image")
        return out

    def draw_aux(self, dev_ptr: int, width: int, height: int, pitch_bytes: int, row0: int = 0,
                 rows: int | None = None, stream: int = 0, depth=None, sphere=None,
                 steps=None) -> None:
        """draw plus the per-pixel planes (sfrt_glsl_draw_aux): depth (float32), sphere and steps
        (int32), each None or a (device pointer, pitch in bytes) pair."""
        rows = height - row0 if rows is None else rows
        planes = AuxPlanes()
        for name, plane in (("depth", depth), ("sphere", sphere), ("steps", steps)):
            if plane is not None:
                setattr(planes, name, int(plane[0]))
                setattr(planes, name + "_pitch_bytes", int(plane[1]))
        _check(lib().sfrt_glsl_draw_aux(self._h, ctypes.c_void_p(dev_ptr), int(width), int(height),
                                        int(pitch_bytes), ctypes.byref(planes), int(row0),
                                        int(rows), ctypes.c_void_p(stream or None)),
               "glsl_draw_aux")

    def draw_image_aux(self, width: int, height: int, depth: bool = True, sphere: bool = True,
                       steps: bool = True) -> dict:
        """draw_image plus the wanted planes (sfrt_glsl_draw_image_aux): {"rgba": uint8
        (width*height*4,), "depth": float32 (height, width), "sphere", "steps": int32}."""
        res = {"rgba": np.zeros(width * height * 4, dtype=np.uint8)}
        for name, want, dtype in (("depth", depth, np.float32), ("sphere", sphere, np.int32),
                                  ("steps", steps, np.int32)):
            if want:
                res[name] = np.zeros((height, width), dtype=dtype)
        ptrs = [res[name].ctypes.data if name in res else None
                for name in ("depth", "sphere", "steps")]
        _check(lib().sfrt_glsl_draw_image_aux(self._h, res["rgba"].ctypes.data, *ptrs, int(width),
                                              int(height)), "glsl_draw_image_aux")
        return res

    # --- view batches ---
    def render_views(self, views, width: int, height: int, pitch_bytes: int,
                     stream: int = 0) -> None:
        """A batch of whole frames of this shader in one launch (sfrt_glsl_render_views): view k
        is the frame set_uniform("campos" / "rotation" / "fov" from views[k].cam) + draw would
        write at views[k].dev_pixels; the shader itself is left as it was.  views: View objects
        or (Camera, device pointer) pairs.  Asynchronous on `stream`."""
        arr = World._view_array(views)
        _check(lib().sfrt_glsl_render_views(self._h, arr, len(views), int(width), int(height),
                                            int(pitch_bytes), 0, ctypes.c_void_p(stream or None)),
               "glsl_render_views")

    def render_views_aux(self, views, planes, width: int, height: int, pitch_bytes: int,
                         stream: int = 0) -> None:
        """render_views plus each view's planes (sfrt_glsl_render_views_aux): planes[k] is an
        AuxPlanes, or a dict of draw_aux's (device pointer, pitch in bytes) pairs under "depth",
        "sphere" and "steps"."""
        if len(planes) != len(views):
            raise ValueError("one planes entry per view")
        arr = World._view_array(views)
        pl = (AuxPlanes * max(1, len(views)))()
        for k, p in enumerate(planes):
            if not isinstance(p, AuxPlanes):
                q = AuxPlanes()
                for name, plane in p.items():
                    if plane is not None:
                        setattr(q, name, int(plane[0]))
                        setattr(q, name + "_pitch_bytes", int(plane[1]))
                p = q
            pl[k] = p
        _check(lib().sfrt_glsl_render_views_aux(self._h, arr, pl, len(views), int(width),
                                                int(height), int(pitch_bytes), 0,
                                                ctypes.c_void_p(stream or None)),
               "glsl_render_views_aux")

    # --- ray queries ---
    def cast_rays(self, dirs, outputs=RAY_OUTPUTS) -> dict:
        """The shader's Raycast(campos, dir, 1) for a batch of caller-supplied directions
        (sfrt_glsl_cast_rays); every ray starts at the campos uniform.

        dirs: (N, 3) float32, un-normalised.  Returns {name: array} for the requested outputs:
        pos (N, 3) float32, depth (N,) float32, sphere and steps (N,) int32, rgba (N, 4) uint8.
        An invalid ray (non-finite component, zero / underflowing / overflowing length) has
        sphere == -1 and zeros elsewhere."""
        dirs = np.ascontiguousarray(np.asarray(dirs, dtype=np.float32).reshape(-1, 3))
        n = dirs.shape[0]
        shapes = {"pos": ((n, 3), np.float32), "depth": ((n,), np.float32),
                  "sphere": ((n,), np.int32), "steps": ((n,), np.int32), "rgba": ((n, 4), np.uint8)}
        res = {name: np.zeros(*shapes[name]) for name in outputs}
        hits = RayHits()
        for name, arr in res.items():
            # an empty array's pointer still says "requested"
            setattr(hits, name, arr.ctypes.data if n else 4)
        _check(lib().sfrt_glsl_cast_rays(self._h, dirs.ctypes.data if n else 4, n,
                                         ctypes.byref(hits)), "glsl_cast_rays")
        return res

    def cast_rays_device(self, dirs_ptr: int, count: int, stream: int = 0, pos=None, depth=None,
                         sphere=None, steps=None, rgba=None) -> None:
        """Asynchronous sfrt_glsl_cast_rays_device on `stream`: device pointers (ints) to count*3
        float32 directions and to each wanted output; the status is left to check(stream)."""
        hits = RayHits()
        for name, ptr in zip(RAY_OUTPUTS, (pos, depth, sphere, steps, rgba)):
            if ptr:
                setattr(hits, name, int(ptr))
        _check(lib().sfrt_glsl_cast_rays_device(self._h, ctypes.c_void_p(dirs_ptr or None),
                                                int(count), ctypes.byref(hits),
                                                ctypes.c_void_p(stream or None)),
               "glsl_cast_rays_device")

    def check(self, stream: int = 0) -> None:
        _check(lib().sfrt_glsl_check(self._h, ctypes.c_void_p(stream or None)), "glsl_check")

    def set_option(self, option: int, value: int) -> None:
        _check(lib().sfrt_glsl_set_option(self._h, option, value), "glsl_set_option")

    def get_option(self, option: int) -> int:
        """SFRT_OPT_TILE_ORDER (0/1/2) or SFRT_OPT_SUPERSAMPLE (the factor 1, 2 or 4)."""
        v = ctypes.c_int(0)
        _check(lib().sfrt_glsl_get_option(self._h, option, ctypes.byref(v)), "glsl_get_option")
        return int(v.value)
