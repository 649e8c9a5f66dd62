"""One fixed list of degenerate voxel worlds for every voxel kernel family (no GPU).

The worlds are `voxel_scenes.random_world`, tests/test_parity_sweep.py's `_voxel_adversarial` and
the sweep's `seed % 4 == 1` branch (the default world from a random empty cell), each imported
where it lives so that a seed stays the same world, plus hand-built corner worlds neither
generator produces (CORNERS): adversarial worlds seen from negative coordinates, cameras above the
ceiling and beside a wall, cameras at 1.5e9 and at 2147483520.0 in x with billboards and shadow
lights (dda_qlim == 0: every wave takes the slow DDA; the four cases before each borrow that
camera, so their view batches mix both marches), a billboard at the camera's own x, z, four
billboards at bitwise equal distances, lights inside a solid block, on a cell corner and at the
camera, long light and billboard lists, and the view distances 0 and 64.

include/sfrt.h sets no maximum for the light and billboard counts and none for the view distance
but that it is finite and >= 0.  `max_dyn` is therefore the default world's own 133 billboards or
more, `max_lights` 64 lights or more, and `long_view` the sweep's largest, 64: the march's trip
count grows with the view distance (maxiter = 1.5 * view_distance), so a frame at the largest
finite float would never end.

A case is (id, scene, width, height, tile_order, tags): the voxel world has no pixels-per-lane
option.  The frame size is one of SIZES and SFRT_OPT_TILE_ORDER alternates, both by the case's
index.  The tags come from the scene's numbers (`tags_of`), never from a generator's draws.
"""
import dataclasses
import functools
from typing import NamedTuple

import numpy as np

import voxel_ref
import voxel_scenes as vs
import voxel_views_cases as vv

F = np.float32
SIZES = [(101, 37), (72, 20), (40, 9), (133, 17), (24, 40)]
INT_LIMIT = 2147483520.0  # the largest float below 2^31
MAX_DYN, MAX_LIGHTS, LONG_VIEW = 133, 64, 64.0

RANDOM_SEEDS = [20000, 20002, 20003, 20004, 20006, 20007, 20008, 20010, 20011, 20012, 20014,
                20015, 20016, 20018, 20019, 20020]
DEFAULT_SEEDS = [20001, 20005, 20009, 20013]  # the sweep's seed % 4 == 1 branch
ADVERSARIAL_SEEDS = [50000, 50001, 50002, 50003, 50004, 50006, 50007, 50008, 50009, 50010, 50011,
                     50012, 50013, 50014, 50016, 50021]
ADVERSARIAL_CLASSES = ("cam_integer", "cam_half", "quarter_turn", "zero_tilt", "light_on_corner",
                       "long_view")
OTHER_TAGS = ("cam_negative", "cam_outside_grid", "cam_far", "light_in_block", "light_at_cam",
              "billboard_at_cam", "equal_billboards", "max_lights", "max_dyn", "texel_outside")
CORNERS = {4: "negative_a", 9: "negative_b", 14: "above_ceiling", 19: "beside_wall",
           23: "far_1.5e9", 27: "far_int_limit", 31: "billboard_at_cam", 35: "equal_billboards",
           38: "lights", 41: "long_lists", 44: "view_0", 47: "view_64"}
QUARTER_TURNS = {float(F(0.0)), float(F(np.pi / 2)), float(F(np.pi)), float(F(-np.pi / 2)),
                 float(F(2 * np.pi))}


class Case(NamedTuple):
    id: str
    scene: vs.VoxelScene
    width: int
    height: int
    tile_order: int
    tags: frozenset


@functools.lru_cache(maxsize=None)
def assets():
    return vs.load_textures()


# ---------------------------------------------------------------- the generators

def default_from_a_cell(seed):
    """test_voxel_sweep's seed % 4 == 1 branch: the default world from a random empty cell."""
    r4 = np.random.default_rng(seed)
    blocks = vs.default_blocks()
    while True:
        c = (int(r4.integers(1, 99)), int(r4.integers(1, 9)), int(r4.integers(1, 99)))
        if blocks[c] == vs.EMPTY:
            break
    return vs.default_world(tuple(float(F(c[k] + r4.uniform(0.05, 0.95))) for k in range(3)),
                            float(r4.uniform(0, 6.28)), float(r4.uniform(-0.6, 0.6)))


def generated(mode, seed):
    """The world the sweep of `mode` ("random" / "adversarial") draws for `seed`."""
    from test_parity_sweep import _voxel_adversarial
    if seed % 4 == 1 and mode == "random":
        return default_from_a_cell(seed)
    return (vs.random_world(seed) if mode == "random" else _voxel_adversarial(seed))[0]


# ---------------------------------------------------------------- the corner worlds

def _dyn(entries):
    """entries: (pos, size, (r, g, b), texture_id); dist_to_camera is set by the caller."""
    d = np.zeros(len(entries), dtype=vs.DYN_DTYPE)
    for k, (pos, size, rgb, tex) in enumerate(entries):
        d[k]["pos"], d[k]["size"] = pos, size
        d[k]["r"], d[k]["g"], d[k]["b"] = rgb
        d[k]["texture_id"] = tex
    return d


def _light(pos, intensity=6.0, rgb=(1.0, 0.8, 0.6), shadows=1):
    L = np.zeros(1, dtype=vs.LIGHT_DTYPE)
    L[0]["pos"], L[0]["intensity"], L[0]["shadows"] = pos, intensity, shadows
    L[0]["r"], L[0]["g"], L[0]["b"] = rgb
    return L


def _sorted_for_own_camera(sc):
    return dataclasses.replace(sc, dyn=vv.sort_dynamics(sc.dyn, sc.cam_pos))


def _negative(seed, whole):
    """An adversarial world seen from negative coordinates: the camera moved out along -x (and
    -z and -y with `whole`) by whole cells, facing the grid."""
    from test_parity_sweep import _voxel_adversarial
    sc = _voxel_adversarial(seed)[0]
    cam = np.array(sc.cam_pos, dtype=F)
    cam[0] = F(cam[0] - np.floor(cam[0]) - F(2))
    if whole:
        cam[1] = F(cam[1] - np.floor(cam[1]) - F(1))
        cam[2] = F(cam[2] - np.floor(cam[2]) - F(3))
    return _sorted_for_own_camera(dataclasses.replace(
        sc, cam_pos=tuple(float(c) for c in cam), rotation=float(F(0.9 if whole else np.pi / 2)),
        hrotation=float(F(0.2 if whole else 0.0))))


def _outside(seed, above):
    sc = vs.random_world(seed)[0]
    nx, ny, nz = sc.blocks.shape
    cam = np.array(sc.cam_pos, dtype=F)
    if above:
        cam[1] = F(ny + 1.5)
        return _sorted_for_own_camera(dataclasses.replace(sc, cam_pos=tuple(float(c) for c in cam),
                                                          hrotation=float(F(-0.9))))
    cam[0] = F(nx + 2.25)
    return _sorted_for_own_camera(dataclasses.replace(
        sc, cam_pos=tuple(float(c) for c in cam), rotation=float(F(-np.pi / 2)), hrotation=0.0))


def _far(seed, x):
    """A random world with billboards and shadow lights seen from x: three more billboards stand
    at the camera's own x (the spacing of binary32 there is 64 or more), so the far frame draws
    some."""
    sc = vs.random_world(seed)[0]
    assert sc.dyn.shape[0] >= 2 and (sc.lights["shadows"] == 1).any()
    cam = (float(F(x)), sc.cam_pos[1], sc.cam_pos[2])
    near = _dyn([((x, cam[1], cam[2] + 2.0), (0.4, 0.6), (1.0, 0.5, 0.25), 0),
                 ((x, cam[1] + 0.25, cam[2] - 3.0), (0.5, 0.5), (0.5, 1.0, 1.5), 1),
                 ((x, cam[1], cam[2] + 5.5), (0.3, 0.8), (2.0, 2.0, 0.5), 0)])
    return _sorted_for_own_camera(dataclasses.replace(
        sc, cam_pos=cam, rotation=0.0, hrotation=0.0, dyn=np.concatenate([sc.dyn, near])))


def _billboard_at_cam():
    sc = vs.random_world(20103)[0]
    cam = sc.cam_pos
    here = _dyn([((cam[0], cam[1] - 0.125, cam[2]), (0.4, 0.6), (1.0, 1.0, 1.0), 0),
                 ((cam[0] + 1.5, cam[1], cam[2] + 1.5), (0.4, 0.6), (0.5, 1.5, 1.0), 1)])
    return _sorted_for_own_camera(dataclasses.replace(sc, dyn=np.concatenate([here, sc.dyn])))


def _equal_billboards():
    """The camera on half coordinates; four billboards one cell away along +-x and +-z (their
    binary32 distances are all exactly 1) and two pairs at equal distances further out, in a list
    order a stable sort keeps and an unstable one need not."""
    sc = vs.random_world(20104)[0]
    cam = tuple(float(F(np.floor(c) + 0.5)) for c in sc.cam_pos)
    x, y, z = cam
    ring = _dyn([((x + 1, y, z), (0.3, 0.5), (2.0, 0.0, 0.0), 0),
                 ((x + 2, y, z + 2), (0.5, 0.7), (0.0, 0.0, 2.0), 1),
                 ((x, y, z + 1), (0.3, 0.5), (0.0, 2.0, 0.0), 1),
                 ((x - 1, y, z), (0.3, 0.5), (0.0, 0.0, 2.0), 0),
                 ((x - 2, y, z - 2), (0.5, 0.7), (2.0, 2.0, 0.0), 0),
                 ((x, y, z - 1), (0.3, 0.5), (2.0, 2.0, 2.0), 1),
                 ((x + 2, y + 0.25, z + 2), (0.5, 0.7), (2.0, 0.0, 2.0), 0)])
    return _sorted_for_own_camera(dataclasses.replace(sc, cam_pos=cam, dyn=ring))


def _lights():
    """A light inside a solid block, one on a cell corner, one at the camera position, and 61
    more around the camera."""
    sc = vs.random_world(20105)[0]
    solid = np.argwhere(sc.blocks != vs.EMPTY)
    cam = np.array(sc.cam_pos)
    cell = solid[np.argmin(np.linalg.norm(solid + 0.5 - cam, axis=1))]
    rng = np.random.default_rng(5)
    nx, ny, nz = sc.blocks.shape
    more = [_light(tuple(np.clip(cam + rng.uniform(-6, 6, 3), 0.2, [nx - 0.2, ny - 0.2, nz - 0.2])),
                   rng.uniform(1, 6), tuple(rng.uniform(0.2, 1.0, 3)), int(k % 2))
            for k in range(MAX_LIGHTS - 3)]
    lights = np.concatenate([_light(tuple(cell + 0.5)), _light(tuple(np.round(cam) + [1.0, 0.0, 1.0]), 9.0),
                             _light(sc.cam_pos, 4.0, (0.5, 1.0, 1.0))] + more)
    return dataclasses.replace(sc, lights=lights)


def _long_lists():
    """64 lights (the first at the camera position) and 140 billboards (the first at the camera's
    own x, z) around the camera of a random world."""
    sc = vs.random_world(20106)[0]
    rng = np.random.default_rng(9)
    nx, ny, nz = sc.blocks.shape
    cam = np.array(sc.cam_pos)
    lights = np.concatenate([
        _light(tuple(np.clip(cam + rng.uniform(-7, 7, 3), 0.2, [nx - 0.2, ny - 0.2, nz - 0.2])),
               rng.uniform(1, 8), tuple(rng.uniform(0.2, 1.0, 3)), int(k % 4 == 0))
        for k in range(MAX_LIGHTS)])
    lights[0]["pos"] = sc.cam_pos
    entries = [((cam[0], cam[1] + 0.25, cam[2]), (0.2, 0.3), (1.0, 1.0, 1.0), 1)]
    for k in range(139):
        a, r = rng.uniform(0, 2 * np.pi), rng.uniform(1.0, 9.0)
        entries.append(((cam[0] + r * np.sin(a), rng.uniform(0.3, ny - 0.7), cam[2] + r * np.cos(a)),
                        (rng.uniform(0.05, 0.3), rng.uniform(0.1, 0.5)), tuple(rng.uniform(0, 2, 3)),
                        int(k % 2)))
    return _sorted_for_own_camera(dataclasses.replace(sc, lights=lights, dyn=_dyn(entries)))


_CORNER_WORLDS = {
    "negative_a": lambda: _negative(50101, False),
    "negative_b": lambda: _negative(50102, True),
    "above_ceiling": lambda: _outside(20101, True),
    "beside_wall": lambda: _outside(20102, False),
    "far_1.5e9": lambda: _far(20003, 1.5e9),
    "far_int_limit": lambda: _far(20010, INT_LIMIT),
    "billboard_at_cam": _billboard_at_cam,
    "equal_billboards": _equal_billboards,
    "lights": _lights,
    "long_lists": _long_lists,
    "view_0": lambda: dataclasses.replace(vs.random_world(20107)[0], view_distance=0.0),
    "view_64": lambda: dataclasses.replace(vs.default_world((1.5, 1.5, 1.5), 0.785398, 0.0),
                                           view_distance=LONG_VIEW),
}


# ---------------------------------------------------------------- the tags

def tags_of(scene, w, h):
    """The classes a world belongs to, from its numbers alone (`texel_outside`: from the
    restatement's count of texel reads outside a texture for the w x h frame)."""
    cam = np.array(scene.cam_pos, dtype=F)
    dims = np.array(scene.blocks.shape)
    tags = set()
    if (cam == np.floor(cam)).all():
        tags.add("cam_integer")
    if (cam - np.floor(cam) == F(0.5)).all():
        tags.add("cam_half")
    if (cam < 0).any():
        tags.add("cam_negative")
    if ((cam < 0) | (cam >= dims)).any():
        tags.add("cam_outside_grid")
    if vv.dda_qlim(scene, w, h) == 0.0:
        tags.add("cam_far")
    if float(F(scene.rotation)) in QUARTER_TURNS:
        tags.add("quarter_turn")
    if F(scene.hrotation) == 0:
        tags.add("zero_tilt")
    lp = np.asarray(scene.lights["pos"], dtype=F).reshape(-1, 3)
    for p in lp:
        if (p == np.floor(p)).all():
            tags.add("light_on_corner")
        c = np.floor(p).astype(np.int64)
        if ((c >= 0) & (c < dims)).all() and scene.blocks[tuple(c)] != vs.EMPTY:
            tags.add("light_in_block")
        if (p.view(np.uint32) == cam.view(np.uint32)).all():
            tags.add("light_at_cam")
    dp = np.asarray(scene.dyn["pos"], dtype=F).reshape(-1, 3)
    if dp.shape[0] and ((dp[:, 0] == cam[0]) & (dp[:, 2] == cam[2])).any():
        tags.add("billboard_at_cam")
    if dp.shape[0]:
        dist = vv.distances(scene.dyn, scene.cam_pos)
        if len(np.unique(dist.view(np.uint32))) < dist.size:
            tags.add("equal_billboards")
    if lp.shape[0] >= MAX_LIGHTS:
        tags.add("max_lights")
    if dp.shape[0] >= MAX_DYN:
        tags.add("max_dyn")
    if F(scene.view_distance) >= F(LONG_VIEW):
        tags.add("long_view")
    if reference(scene, w, h)["bad_texels"] > 0:
        tags.add("texel_outside")
    return frozenset(tags)


def reference(scene, w, h, shade=True):
    """voxel_ref.render of the scene: the planes, the colour and the count of bad texel reads."""
    tex, dyn = assets()
    return voxel_ref.render(scene, w, h, tex, dyn, vs.COLORS, shade=shade)


# ---------------------------------------------------------------- the list

def make_case(kind, name, scene, index):
    w, h = SIZES[index % len(SIZES)]
    return Case(f"{kind}-{name}", scene, w, h, index % 2, tags_of(scene, w, h) | {kind})


@functools.lru_cache(maxsize=None)
def cases():
    """The fixed ordered list: random (the default world for every fourth) and adversarial seeds
    alternating, the corner worlds at CORNERS."""
    rand = sorted(RANDOM_SEEDS + DEFAULT_SEEDS)
    order = []
    for k in range(max(len(rand), len(ADVERSARIAL_SEEDS))):
        if k < len(rand):
            order.append(("default" if rand[k] % 4 == 1 else "random", rand[k]))
        if k < len(ADVERSARIAL_SEEDS):
            order.append(("adversarial", ADVERSARIAL_SEEDS[k]))
    for at in sorted(CORNERS):
        order.insert(at, ("corner", CORNERS[at]))
    out = []
    for index, (kind, v) in enumerate(order):
        if kind == "corner":
            sc = _CORNER_WORLDS[v]()
        else:
            sc = generated("adversarial" if kind == "adversarial" else "random", v)
        out.append(make_case(kind, str(v), sc, index))
    return tuple(out)


def camera_of(sc):
    """(cam_pos, rotation, hrotation) of a scene as Python floats of binary32 values: the camera
    of voxel_views_cases.with_camera."""
    return (tuple(float(F(x)) for x in sc.cam_pos), float(F(sc.rotation)), float(F(sc.hrotation)))


def other_scenes(index, count=4):
    """The scenes of the next `count` cases of the fixed list (the list wraps round)."""
    cs = cases()
    return [cs[(index + q) % len(cs)].scene for q in range(1, count + 1)]


def borrowed_cameras(others):
    return [camera_of(o) for o in others[:4]]
