"""The cases of the voxel aux-plane tests (tests/test_voxel_ref.py on the CPU, tests/test_voxel_aux.py
on the GPU) and their reference planes, computed once per process by tests/voxel_ref.py.

The GPU tests render these scenes at 101 x 37, ragged against the 8 x 8 tile; the CPU test asserts
on the reference side that they reach every face value, a zero direction component, a texel read
outside a texture and step counts from 1 to maxiter, so that no GPU comparison is vacuous."""
import functools

import voxel_ref
import voxel_scenes as vs

W, H = 101, 37

DEFAULT_POSES = [  # (cam_pos, rotation, hrotation, name)
    ((15.5, 1.9, 15.5), 0.0, 0.0, "default"),
    ((30.25, 2.6, 12.75), 2.2, 0.25, "default_turned"),
]

# the poses of VOXEL_EDGE_CASES in tests/test_voxel.py
EDGE_POSES = [
    ((15.5, 1.9, 15.5), float(vs.deg2rad(75)) / 2, 0.0, "axis_parallel_column"),
    ((-1.5, 1.9, -1.5), 0.785, 0.0, "negative_coordinates"),
    ((-3.5, 4.5, 20.5), 1.5708, 0.0, "negative_x_facing_wall"),
    ((50.5, 11.5, 50.5), 0.3, -1.2, "above_the_grid"),
    ((50.5, 10.25, 50.5), 0.3, -0.9, "just_above_the_ceiling"),
    ((16.0, 2.0, 16.0), 1.0, 0.2, "integer_position"),
    ((1.5, 0.5, 1.5), 0.785398, 0.0, "long_walks"),
    ((1.5e9, 1.9, 15.5), 3.14159, 0.0, "far_camera"),
    ((2147483520.0, 1.9, 15.5), 0.0, 0.0, "camera_at_int_limit"),
    ((2147483520.0, 1.9, 15.5), 3.14159, 0.0, "camera_at_int_limit_back"),
]

SEEDS = list(range(12))

NAMES = [p[3] for p in DEFAULT_POSES + EDGE_POSES] + [f"random_{s}" for s in SEEDS]
SS_NAMES = ["default_turned", "random_3"]  # the supersampling cases (random_3 has billboards)


@functools.lru_cache(maxsize=None)
def scene(name):
    for p, r, hr, n in DEFAULT_POSES + EDGE_POSES:
        if n == name:
            return vs.default_world(p, r, hr)
    return vs.random_world(int(name.split("_")[1]))[0]


@functools.lru_cache(maxsize=None)
def assets():
    return vs.load_textures()


@functools.lru_cache(maxsize=None)
def reference(name, s=1):
    """voxel_ref's planes of `name` at (s * W) x (s * H), without the colour.  Shared: read only."""
    tex, dyn = assets()
    ref = voxel_ref.render(scene(name), s * W, s * H, tex, dyn, vs.COLORS, shade=False)
    for k in voxel_ref.PLANES:
        ref[k].setflags(write=False)
    return ref
