"""One fixed list of degenerate sphere scenes for every sphere kernel family (no GPU).

The scenes are tests/test_gpu_parity.py's `_fuzz_scene` and tests/test_parity_sweep.py's
`_sphere_adversarial`, imported where they live so that a seed stays the same scene, plus four
"swarm" scenes neither generator produces: 130, 200, 257 and 1024 spheres in caller (unsorted)
order with the camera strictly inside more than 64 of them.  A sphere that holds the apex of a
wave's cone can never be culled, so every wave of a swarm frame overflows the 64 entries of its
culled list (`count + cw > 64` in cull_wave) and marches the full list.

A case is (id, scene, width, height, rays_per_lane, tags).  The frame size overrides the
generator's with one of SIZES (ragged both ways, narrower and wider than a tile row), and
SFRT_OPT_RAYS_PER_LANE cycles through 0..4, both by the case's index.  The tags are computed
from the scene's numbers (`tags_of`), never from the generator's random draws.  The seeds were
picked once, on the CPU, so that every tag tests/test_sphere_family_fuzz.py asks for is present
and the oracle alone gives every case a defined answer (no march reaches the kernels' guard of
2^20 steps, at 1, 2x2 and 4x4 samples per pixel, nor from the four other cameras the views test
borrows).
"""
import functools
from typing import NamedTuple

import numpy as np

if __name__ == "__main__":
    import conftest  # noqa: F401  run as a script (below): the import path of the tests
import scenes

F = np.float32
SIZES = [(72, 20), (40, 9), (97, 33), (133, 17), (256, 8), (24, 40)]
MARCH_GUARD = 1 << 20   # the kernels' march guard (SFRT_E_MARCH_LIMIT)
MAX_SPHERES = 1024      # SFRT_MAX_SPHERES
FUZZ_COUNTS = (1, 2, 3, 7, 16, 17, 33, 64, 65, 130)  # _fuzz_scene's list
CAMERA_MODES = ("cam_centre", "cam_near_surface", "cam_inside", "cam_outside")
ADVERSARIAL_CLASSES = ("cam_centre", "cam_on_surface", "quarter_turn", "tangent_pair", "duplicate",
                       "threshold_radius", "x1000", "fov_1e-4")

# _fuzz_scene(seed), from 20000 upward
RANDOM_SEEDS = [20000, 20001, 20002, 20003, 20004, 20005, 20006, 20007, 20008, 20009, 20010,
                20011, 20013, 20014, 20015, 20016, 20017, 20018, 20020, 20022, 20023, 20027]
# _sphere_adversarial(seed), from 50000 upward
ADVERSARIAL_SEEDS = [50001, 50002, 50003, 50004, 50005, 50056, 50007, 50008, 50009, 50010, 50011,
                     50012, 50013, 50014, 50015, 50017, 50018, 50020, 50021, 50035, 50081, 50098]
SWARM_COUNTS = (130, 200, 257, MAX_SPHERES)
SWARM_AT = (9, 20, 31, 47)  # their positions in the list


class Case(NamedTuple):
    id: str
    scene: scenes.Scene
    width: int
    height: int
    rays_per_lane: int
    tags: frozenset


def swarm_scene(n):
    """n spheres around the camera, in caller order.  Every sphere's radius exceeds its centre's
    distance from the camera by at least a quarter, so the camera is strictly inside all of them;
    the counts 200 and 1024 have integer centres and radii and their second half repeats the
    first (duplicated spheres)."""
    rng = np.random.default_rng(7000 + n)
    cam = np.array([0.5, -0.25, 0.125], dtype=F) if n in (200, MAX_SPHERES) else \
        rng.uniform(-3, 3, 3).astype(F)
    off = rng.uniform(-6, 6, size=(n, 3))
    if n in (200, MAX_SPHERES):
        c = np.round(off)
        r = np.ceil(np.linalg.norm(c - cam.astype(np.float64), axis=1) + rng.uniform(1, 9, n))
        sp = np.concatenate([c, r[:, None]], axis=1).astype(F)
        sp[n // 2:] = sp[: n - n // 2]
    else:
        c = cam.astype(np.float64) + off
        r = np.linalg.norm(off, axis=1) + rng.uniform(0.25, 9, n)
        sp = np.concatenate([c, r[:, None]], axis=1).astype(F)
    return scenes.Scene(f"swarm{n}", sp, cam_pos=tuple(float(x) for x in cam),
                        rotation=float(F(rng.uniform(-3, 3))), hrotation=float(F(rng.uniform(-0.6, 0.6))))


def spheres_holding_camera(scene):
    """How many spheres have |cam - c| < r, in float64."""
    sp = np.asarray(scene.spheres, dtype=np.float64)
    d = np.linalg.norm(sp[:, :3] - np.asarray(scene.cam_pos, dtype=np.float64), axis=1)
    return int(np.count_nonzero(d < sp[:, 3]))


def tags_of(scene):
    """The classes a scene belongs to, from its numbers alone."""
    sp32 = np.ascontiguousarray(np.asarray(scene.spheres, dtype=F).reshape(-1, 4))
    cam32 = np.asarray(scene.cam_pos, dtype=F)
    sp, cam = sp32.astype(np.float64), cam32.astype(np.float64)
    n = sp.shape[0]
    eps = float(np.finfo(F).eps)
    tags = {f"n{n}"}
    d = np.linalg.norm(sp[:, :3] - cam, axis=1)
    scale = np.maximum(np.maximum(sp[:, 3], np.abs(cam).max()), np.abs(sp[:, :3]).max(axis=1))
    # the camera: exactly one of CAMERA_MODES
    if (sp32[:, :3].view(np.uint32) == cam32.view(np.uint32)).all(axis=1).any():
        tags.add("cam_centre")       # cam == spheres[k, :3] bitwise
    elif (np.abs(d - sp[:, 3]) <= 2e-3 * sp[:, 3]).any():
        tags.add("cam_near_surface")  # _fuzz_scene puts it at 0.999 r
    elif (d < sp[:, 3]).any():
        tags.add("cam_inside")
    else:
        tags.add("cam_outside")
    # on a surface: one axis off a centre by the radius, to binary32's rounding of that sum
    one_axis = np.count_nonzero(sp32[:, :3] != cam32, axis=1) == 1
    if (one_axis & (np.abs(d - sp[:, 3]) <= 4 * eps * scale)).any():
        tags.add("cam_on_surface")
    quarter = {float(F(k * np.pi / 2)) for k in (-1, 0, 1, 2, 4)}
    if float(F(scene.rotation)) in quarter and float(F(scene.hrotation)) in quarter:
        tags.add("quarter_turn")
    rows = {r.tobytes() for r in sp32}
    if len(rows) < n:
        tags.add("duplicate")
    if n > 1:  # a tangent pair: centres apart along one axis by the sum of the radii
        k = np.arange(1, n)
        gap = np.linalg.norm(sp[k, :3] - sp[k - 1, :3], axis=1)
        axis = np.count_nonzero(sp32[k, :3] != sp32[k - 1, :3], axis=1) == 1
        tol = 4 * eps * np.maximum(scale[k], scale[k - 1])
        if (axis & (np.abs(gap - (sp[k, 3] + sp[k - 1, 3])) <= tol)).any():
            tags.add("tangent_pair")
    if np.isin(sp32[:, 3], [F(0.01), np.nextafter(F(0.01), F(1))]).any():
        tags.add("threshold_radius")
    if np.abs(sp[:, :3]).max() >= 1000.0:  # the generators stay within 60 otherwise
        tags.add("x1000")
    if F(scene.fov_h) == F(1e-4) or F(scene.fov_v) == F(1e-4):
        tags.add("fov_1e-4")
    if spheres_holding_camera(scene) > 64:
        tags.add("holds_camera_65")
    return frozenset(tags)


def make_case(kind, scene, index):
    """The case of `scene` at position `index` of a list: its size and pixels per lane."""
    w, h = SIZES[index % len(SIZES)]
    return Case(f"{kind}-{scene.name}", scene, w, h, index % 5, tags_of(scene) | {kind})


def generated(kind, seed):
    """The scene of a seed: kind "random" is _fuzz_scene, "adversarial" _sphere_adversarial."""
    from test_gpu_parity import _fuzz_scene
    from test_parity_sweep import _sphere_adversarial
    sc, _, _ = (_fuzz_scene if kind == "random" else _sphere_adversarial)(seed)
    if kind == "adversarial":
        sc.name = f"adv{seed}"
    sc.spheres = np.ascontiguousarray(np.asarray(sc.spheres, dtype=F))
    return sc


@functools.lru_cache(maxsize=None)
def cases():
    """The fixed ordered list: random and adversarial seeds alternating, the swarms at
    SWARM_AT (four different frame sizes and pixels per lane)."""
    order = []
    for k in range(max(len(RANDOM_SEEDS), len(ADVERSARIAL_SEEDS))):
        if k < len(RANDOM_SEEDS):
            order.append(("random", RANDOM_SEEDS[k]))
        if k < len(ADVERSARIAL_SEEDS):
            order.append(("adversarial", ADVERSARIAL_SEEDS[k]))
    for at, n in zip(SWARM_AT, SWARM_COUNTS):
        order.insert(at, ("swarm", n))
    out = []
    for index, (kind, v) in enumerate(order):
        sc = swarm_scene(v) if kind == "swarm" else generated(kind, v)
        out.append(make_case(kind, sc, index))
    return tuple(out)


def textured(index):
    """Every seventh case draws from the six shipped textures with random per-sphere slots."""
    return index % 7 == 3


def slots_of(case, index):
    """The texture slot per sphere (all 0 unless textured(index)), as the parity sweep draws them."""
    n = case.scene.spheres.shape[0]
    if not textured(index):
        return np.zeros(n, np.int32)
    return np.random.default_rng(20261021 + index).integers(0, len(scenes.ALL_TEXTURES), n).astype(np.int32)


def camera_of(sc):
    """(cam_pos, rotation, hrotation, fov_h, fov_v) of a scene, as Python floats of binary32 values."""
    return (tuple(float(F(x)) for x in sc.cam_pos), float(F(sc.rotation)), float(F(sc.hrotation)),
            float(F(sc.fov_h)), float(F(sc.fov_v)))


def borrowed_cameras(scene, others):
    """The cameras the views test renders `scene` from besides its own: the positions and poses of
    the scenes `others`, with this scene's own field of view."""
    own = camera_of(scene)
    return [camera_of(o)[:3] + own[3:] for o in others]


def other_scenes(index, count=4):
    """The scenes of the next `count` cases of the fixed list (the list wraps round)."""
    cs = cases()
    return [cs[(index + q) % len(cs)].scene for q in range(1, count + 1)]


def stepped_camera(scene, others):
    """The one-step cache test's camera: the next scene's position under this scene's own pose."""
    own = camera_of(scene)
    return (camera_of(others[0])[0],) + own[1:]


def nudged_spheres(scene):
    """The scene's spheres with sphere 0 moved by one ulp in x."""
    sp = np.array(scene.spheres, dtype=F)
    sp[0, 0] = np.nextafter(sp[0, 0], F(np.inf))
    return sp


def march_lengths(case, others, floor, threads=1):
    """{configuration: the oracle's longest march}, for every frame a family test asks the oracle
    for: the case's own camera at 1, 2x2 and 4x4 samples per pixel, the borrowed cameras, the
    stepped camera (at 1 and 2x2) and the nudged sphere."""
    import oracle
    sc = case.scene

    def longest(s, cam, spheres=None):
        o = oracle.Oracle(s * case.width, s * case.height, sc.spheres if spheres is None else spheres,
                          *floor, *cam)
        return int(o.iteration_map(threads).max())

    own = camera_of(sc)
    out = {f"own-s{s}": longest(s, own) for s in (1, 2, 4)}
    for q, cam in enumerate(borrowed_cameras(sc, others)):
        out[f"view{q + 1}"] = longest(1, cam)
        out[f"view{q + 1}-sorted"] = longest(1, cam, oracle.sort_spheres(sc.spheres, cam[0]))
    for s in (1, 2):
        out[f"step-s{s}"] = longest(s, stepped_camera(sc, others))
        out[f"nudge-s{s}"] = longest(s, own, nudged_spheres(sc))
    return out


if __name__ == "__main__":
    # `python tests/sphere_fuzz_cases.py random|adversarial <seed> <index>`: march_lengths of the
    # scene of a seed with the next four seeds' cameras, as JSON (the on-demand sweep runs this
    # in a child process under a time limit: the oracle's march has no guard of its own)
    import json
    import sys
    mode, seed0, at = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    probe = make_case(mode, generated(mode, seed0), at)
    print(json.dumps(march_lengths(probe, [generated(mode, seed0 + q) for q in range(1, 5)],
                                   scenes.load_floor())))
