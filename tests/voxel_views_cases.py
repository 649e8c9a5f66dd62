"""The cases of the voxel view-batch tests (tests/test_voxel_views_abi.py on the CPU,
tests/test_voxel_views.py on the GPU) and their references, each computed once per process.

The world is voxel_scenes.default_world() with its billboard list replaced by the list sorted for
camera 0 (sort_dynamics below: the numpy statement of sfrt_voxel_sort_dynamics).  View k is that
world seen from CAMS[k]: `stale` with the list as it stands (the batch without the flag), sorted
with the list re-sorted for CAMS[k] (SFRT_VOXEL_VIEWS_DYNAMICS).  Frames are 101 x 37, ragged
against the 8 x 8 tile.  Cameras 5 and 6 are beyond the fast DDA's bound (dda_qlim == 0, restated
below from sfrt_voxel.cpp) beside views that take the fast DDA.
"""
import dataclasses
import functools

import numpy as np

import voxel_ref
import voxel_scenes as vs

F = np.float32
W, H = 101, 37

CAMS = [  # (cam_pos, rotation, hrotation)
    ((13.0, 1.6, 16.5), 0.0, 0.0),
    ((13.06, 1.6, 16.5), 0.0, 0.0),
    ((12.9, 1.5, 20.5), 3.14159, 0.0),
    ((15.5, 1.9, 15.5), -0.6, 0.0),
    ((10.5, 1.9, 18.4), 1.5708, 0.1),
    ((1.5e9, 1.9, 15.5), 3.14159, 0.0),
    ((2147483520.0, 1.9, 15.5), 0.0, 0.0),
    ((16.0, 2.0, 16.0), 1.0, 0.2),
]
SS_VIEWS = (0, 2, 4)  # the supersampled views: billboards from the front, from behind, tilted


def distances(dyn, cam_pos):
    """distToCamera of World.cpp:226-227 for every element, binary32."""
    cam = np.array(cam_pos, dtype=F)
    out = np.empty(dyn.shape[0], dtype=F)
    for i, p in enumerate(dyn["pos"]):
        x, z = F(p[0] - cam[0]), F(p[2] - cam[2])
        out[i] = vs.sqrtf(F(F(x * x) + F(z * z)))
    return out


def sort_dynamics(dyn, cam_pos):
    """The list for a camera at rest: distances set, stable ascending order (no NaN)."""
    d = dyn.copy()
    d["dist_to_camera"] = distances(d, cam_pos)
    assert not np.isnan(d["dist_to_camera"]).any()
    return d[np.argsort(d["dist_to_camera"], kind="stable")]


def insertion_order(dist):
    """The rule itself, for lists with a NaN distance: element i goes before the first already
    placed element whose distance is greater (World.cpp:229's `<`).  Returns the permutation."""
    placed = []
    for i, e in enumerate(dist):
        j = 0
        while j < len(placed) and not (e < dist[placed[j]]):
            j += 1
        placed.insert(j, i)
    return placed


@functools.lru_cache(maxsize=None)
def assets():
    return vs.load_textures()


@functools.lru_cache(maxsize=None)
def base_scene():
    """default_world() with the list sorted for camera 0 and camera 0's pose."""
    sc = vs.default_world()
    pos, rot, hrot = CAMS[0]
    return dataclasses.replace(sc, dyn=sort_dynamics(sc.dyn, pos), cam_pos=pos, rotation=rot,
                               hrotation=hrot)


def with_camera(scene, cam, dynamics):
    pos, rot, hrot = cam
    dyn = sort_dynamics(scene.dyn, pos) if dynamics else scene.dyn
    return dataclasses.replace(scene, cam_pos=pos, rotation=rot, hrotation=hrot, dyn=dyn)


@functools.lru_cache(maxsize=None)
def view_scene(k, dynamics):
    return with_camera(base_scene(), CAMS[k], dynamics)


def _freeze(ref):
    for k in voxel_ref.PLANES:
        ref[k].setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(k, dynamics, s=1):
    """voxel_ref's planes of view k at (s * W) x (s * H), without the colour.  Read only."""
    tex, dyn = assets()
    return _freeze(voxel_ref.render(view_scene(k, dynamics), s * W, s * H, tex, dyn, vs.COLORS,
                                    shade=False))


def oracle_render(scene, w, h, s=1):
    """(rgba (h, w, 4), the reference read outside a texture) by oracle.VoxelOracle; s > 1: the
    box-filtered s-times larger frame."""
    import oracle
    from conftest import host_threads
    tex, dyn = assets()
    o = oracle.VoxelOracle(scene, s * w, s * h, tex, dyn, vs.COLORS)
    before = oracle.VoxelOracle.bad_texel_reads()
    rgba = o.render(host_threads()).reshape(s * h, s * w, 4)
    ub = oracle.VoxelOracle.bad_texel_reads() > before
    if s > 1:
        rgba = voxel_ref.box_filter(rgba, s)
    rgba.setflags(write=False)
    return rgba, ub


@functools.lru_cache(maxsize=None)
def oracle_frame(k, dynamics, s=1):
    return oracle_render(view_scene(k, dynamics), W, H, s)


# ---- random worlds: four cameras inside the scene's own empty cell

@functools.lru_cache(maxsize=None)
def random_scene(seed):
    return vs.random_world(seed)[0]


def random_cams(seed):
    """Four poses in the cell the scene's camera stands in (empty by construction)."""
    sc = random_scene(seed)
    cell = np.floor(np.array(sc.cam_pos, dtype=np.float64))
    offs = [(0.5, 0.5, 0.5), (0.2, 0.7, 0.3), (0.8, 0.3, 0.6), (0.35, 0.55, 0.85)]
    turns = [(sc.rotation, sc.hrotation), (sc.rotation + 1.7, 0.1), (sc.rotation - 2.3, -0.2),
             (sc.rotation + 3.1, 0.3)]
    return [(tuple(float(F(c + o)) for c, o in zip(cell, off)), float(F(r)), float(F(hr)))
            for off, (r, hr) in zip(offs, turns)]


@functools.lru_cache(maxsize=None)
def random_reference(seed, k, dynamics):
    tex, dyn = assets()
    sc = with_camera(random_scene(seed), random_cams(seed)[k], dynamics)
    return _freeze(voxel_ref.render(sc, W, H, tex, dyn, vs.COLORS, shade=False))


@functools.lru_cache(maxsize=None)
def random_oracle(seed, k, dynamics):
    return oracle_render(with_camera(random_scene(seed), random_cams(seed)[k], dynamics), W, H)


# ---- dda_qlim, restated from sfrt_voxel.cpp (doubles, then rounded down to binary32)

def dda_qlim(scene, w, h):
    dx, dz, _, dy, _ = voxel_ref.frame_rays(scene, w, h)
    comps = np.abs(np.concatenate([dx, dz, dy])).astype(np.float64)
    xmax = float(comps[np.isfinite(comps)].max(initial=0.0))
    p = max(abs(float(F(c))) for c in scene.cam_pos)
    maxiter = int(voxel_ref.to_u32(F(scene.view_distance) * F(1.5)))
    q = ((1073741824.0 - p) / (maxiter + 1.0) - 33.0 - 0.003 * xmax) / 2.001
    if not q > 1.0:
        return 0.0
    return float(q)  # > 0: the fast DDA is open to waves within the bound (the value's rounding aside)
