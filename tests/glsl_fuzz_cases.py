"""One fixed list of degenerate uniform blocks for every GLSL kernel family (no GPU).

The blocks are `glsl_scenes.random_uniforms` with the argument draws of
tests/test_parity_sweep.py::test_glsl_sweep (`sweep_draws` replays that test's one running
generator, so a seed is the block the sweep draws for it), the sweep's `seed % 4 == 1` branch (the
reference's own world after k UpdateWorld steps in a random pose) and `_glsl_adversarial`, each
imported where it lives, plus hand-built corner blocks neither generator produces (CORNERS): 64, 65
and 70 walls with the adversarial edits (both sides of the `sc <= 64` wall cull), a shadow ball
whose binary32 distance from campos is the last value below 1000 or exactly 1000 (the lit
shortcut's bound), everything multiplied by 1000, a negative radius, a shadow ball larger than its
distance to a light (sanglet >= 1), shadow balls without a light, and SFRT_GLSL_MAX_SPHERES entries.

A case is (id, uniforms, width, height, tile_order, tags).  The frame size is one of SIZES and
SFRT_OPT_TILE_ORDER alternates, both by the case's index; `size` in the block is set to match.
The tags come from the block's numbers (`tags_of`), never from a generator's draws.  The seeds
were picked once, on the CPU, so that every tag has its cases and the restatement alone gives
every frame a family check asks for a defined answer (no pixel reaches the march cap).
"""
import functools
from typing import NamedTuple

import numpy as np

import glsl_scenes as gs
import glsl_views_cases as gv

F = np.float32
SIZES = [(37, 23), (40, 24), (72, 9), (133, 17), (24, 40)]
MAX_SPHERES = gs.MAX_SPHERES  # SFRT_GLSL_MAX_SPHERES
RANDOM_SEED0, ADVERSARIAL_SEED0 = 20000, 50000  # test_parity_sweep.SEED0 of the two modes

# random_uniforms with the sweep's draws; a seed with seed % 4 == 1 is the sweep's world branch
RANDOM_SEEDS = [20000, 20002, 20003, 20004, 20006, 20007, 20008, 20010, 20011, 20012, 20014,
                20015, 20016, 20018, 20019, 20020]
WORLD_SEEDS = [20001, 20005, 20009, 20013]
# _glsl_adversarial(seed, w, h)
ADVERSARIAL_SEEDS = [50000, 50001, 50002, 50004, 50008, 50011, 50016, 50018, 50021, 50035, 50037,
                     50041, 50043, 50046, 50051, 50072]
ADVERSARIAL_CLASSES = ("cam_at_wall_centre", "cam_negzero", "quarter_turn", "half_grid",
                       "ball_on_light_segment", "ball_on_light", "zero_radius", "duplicate_ball")
OTHER_TAGS = ("cam_outside_walls", "walls_gt_64", "far_ball", "x1000", "neg_radius", "sanglet_ge_1",
              "no_lights", "max_spheres", "wide_fov")
# the corner blocks and their positions in the list
CORNERS = {4: "walls64", 9: "walls65", 14: "walls70", 19: "far_below", 23: "far_above",
           27: "x1000_random", 31: "x1000_adversarial", 35: "neg_radius", 38: "sanglet_ge_1",
           41: "no_lights", 44: "max_spheres_a", 47: "max_spheres_b"}
QUARTER_TURNS = {float(F(k * np.pi / 2)) for k in (-1, 0, 1, 2, 4)}


class Case(NamedTuple):
    id: str
    uniforms: np.ndarray
    width: int
    height: int
    tile_order: int
    tags: frozenset


# ---------------------------------------------------------------- the sweep's draws

@functools.lru_cache(maxsize=None)
def sweep_draws(seed0, count):
    """test_glsl_sweep's draws from its one generator default_rng(seed0), per seed
    seed0 .. seed0 + count - 1: (nw, nl, nb), the world branch's (frame, rotation, hrotation) for
    seed % 4 == 1, the wide field of view for seed % 4 == 0."""
    rng = np.random.default_rng(seed0)
    out = {}
    for seed in range(seed0, seed0 + count):
        d = {"counts": (int(rng.integers(3, 61)), int(rng.integers(0, 4)), int(rng.integers(0, 12)))}
        if seed % 4 == 1:
            d["world"] = (int(rng.integers(0, 600)), F(rng.uniform(0, 6.28)), F(rng.uniform(-0.6, 0.6)))
        if seed % 4 == 0:
            d["fov"] = (F(rng.uniform(1.5, 2.6)), F(rng.uniform(1.0, 2.0)))
        out[seed] = d
    return out


@functools.lru_cache(maxsize=None)
def world_frames():
    """The sweep's 600 uniform blocks of the constructor's world under UpdateWorld."""
    sw = gs.ShaderWorld(0)
    frames = []
    for _ in range(600):
        frames.append(sw.uniforms(16, 16))
        sw.update_world()
    return tuple(frames)


def generated(mode, seed, w, h):
    """The block the sweep of `mode` ("random" / "adversarial") draws for `seed`, at w x h."""
    from test_parity_sweep import _glsl_adversarial
    seed0 = RANDOM_SEED0 if mode == "random" else ADVERSARIAL_SEED0
    d = sweep_draws(seed0, max(400, seed - seed0 + 1))[seed]
    if mode == "random" and seed % 4 == 1:
        k, rot, hrot = d["world"]
        u = world_frames()[k].copy()
        u["rotation"] = (rot, hrot)
        u["size"] = (F(w), F(h))
    elif mode == "random":
        u = gs.random_uniforms(seed, *d["counts"], w, h)
    else:
        u, _ = _glsl_adversarial(seed, w, h)
    if seed % 4 == 0:
        u["fov"] = d["fov"]
    return u


# ---------------------------------------------------------------- the corner blocks

def _edited(u):
    """The edits of _glsl_adversarial, all of them and without a draw: the 0.5 grid, every shadow
    ball on a segment from a light to campos (t = 0.25, 0.5, 0.75, 1.5 in turn), one zero radius,
    the last ball a duplicate of the one before."""
    sc, lc, al = int(u["sphere_count"]), int(u["light_count"]), int(u["all_spheres_count"])
    S = u["spheres"]
    S[:al] = (np.round(S[:al] * 2) / 2).astype(F)
    S[:sc, 3] = np.maximum(S[:sc, 3], F(1))
    cam = np.array(u["campos"], dtype=F)
    for n, j in enumerate(range(sc + lc, al)):
        i = sc + n % lc
        t = F((0.25, 0.5, 0.75, 1.5)[n % 4])
        S[j, :3] = (S[i, :3] + t * (cam - S[i, :3])).astype(F)
        # ... and clear of campos where an eighth fits, so that the frame is not one ball's inside
        S[j, 3] = min(S[j, 3], max(F(0.125), np.floor(_dcam(cam, S[j]) * F(4)) / F(8)))
    S[sc + lc + 1, 3] = F(0)
    S[al - 1] = S[al - 2]
    return u


def _dcam(cam, b):
    c = np.asarray(cam, F) - np.asarray(b, F)[:3]
    return np.sqrt(F(F(c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]))


def _far(above):
    """Wall 0 (radius 6) holds campos; three far shadow balls besides the near ones: one along +x
    whose binary32 distance from campos is the last value below 1000 (above: exactly 1000), one
    along -x at the last value below 1000, one 1500 up."""
    u = gs.random_uniforms(31, 6, 2, 5, 16, 16)
    sc, lc, al = int(u["sphere_count"]), int(u["light_count"]), int(u["all_spheres_count"])
    cam = np.array([0.25, 0.5, -0.25], dtype=F)
    u["campos"] = cam
    u["rotation"] = (F(0.4), F(0.1))
    S = u["spheres"]
    S[sc, :3] = (1.0, 1.5, 0.5)  # the lights stay clear of campos
    S[sc + 1, :3] = (-1.5, 0.5, -1.0)

    def along_x(sign, want_below):
        x = F(cam[0] + F(sign) * F(1000))
        for _ in range(64):  # walk towards campos until the distance is below 1000
            if _dcam(cam, (x, cam[1], cam[2])) < F(1000):
                break
            x = np.nextafter(x, cam[0])
        assert _dcam(cam, (x, cam[1], cam[2])) < F(1000)
        if not want_below:  # one step back out: the first value not below 1000
            x = np.nextafter(x, F(sign) * F(np.inf))
            assert _dcam(cam, (x, cam[1], cam[2])) >= F(1000)
        return x

    for k, centre in enumerate([(along_x(1, not above), cam[1], cam[2]),
                                (along_x(-1, True), cam[1], cam[2]),
                                (cam[0], F(cam[1] + F(1500)), cam[2])]):
        S[al + k] = (*centre, 0.75)
        u["lights"][al + k] = (0.5, 1.0, 1.0, 1.0)
        u["uvs"][al + k] = (0.5, 1.0, 0.5, 0.0)
    u["all_spheres_count"] = al + 3
    return u


def _x1000(u):
    al = int(u["all_spheres_count"])
    u["spheres"][:al] = (u["spheres"][:al] * F(1000)).astype(F)
    u["campos"] = (np.array(u["campos"], F) * F(1000)).astype(F)
    return u


def _neg_radius():
    u = gs.random_uniforms(41, 8, 2, 6, 16, 16)
    sc, lc = int(u["sphere_count"]), int(u["light_count"])
    u["spheres"][sc + lc + 1, 3] = -u["spheres"][sc + lc + 1, 3]
    u["spheres"][sc + lc + 4, 3] = F(-2.5)
    u["campos"] = (30.0, 2.0, -25.0)  # outside every wall
    return u


def _sanglet_ge_1():
    """Two shadow balls larger than their distance to light 0 (atan2(r, dist) >= 1), one of them
    holding the light."""
    u = gs.random_uniforms(43, 9, 2, 6, 16, 16)
    sc, lc = int(u["sphere_count"]), int(u["light_count"])
    S = u["spheres"]
    S[sc + lc, :3] = S[sc, :3] + F([0.25, 0.0, 0.0])
    S[sc + lc, 3] = F(0.5)
    S[sc + lc + 2, :3] = S[sc, :3] + F([0.0, -0.25, 0.125])
    S[sc + lc + 2, 3] = F(0.25)
    return u


def _no_lights():
    u = gs.random_uniforms(47, 10, 0, 7, 16, 16)
    u["spheres"][int(u["sphere_count"]) + 2, 3] = F(-0.25)
    u["campos"] = (-20.0, 9.0, 14.0)  # outside every wall
    u["rotation"] = (F(2.2), F(-0.3))  # facing the walls
    return u


def _max_spheres_b():
    u = gs.random_uniforms(53, 70, 3, 27, 16, 16)
    sc, lc = int(u["sphere_count"]), int(u["light_count"])
    u["spheres"][sc + lc + 5, 3] = F(-0.5)
    u["spheres"][sc + lc + 7, :3] = u["spheres"][sc + 1, :3] + F([0.125, 0.0, 0.0])
    return u


_CORNER_BLOCKS = {
    "walls64": lambda: _edited(gs.random_uniforms(11, 64, 2, 8, 16, 16)),
    "walls65": lambda: _edited(gs.random_uniforms(12, 65, 2, 8, 16, 16)),
    "walls70": lambda: _edited(gs.random_uniforms(13, 70, 3, 9, 16, 16)),
    "far_below": lambda: _far(False),
    "far_above": lambda: _far(True),
    "x1000_random": lambda: _x1000(gs.random_uniforms(21, 12, 2, 7, 16, 16)),
    "x1000_adversarial": lambda: _x1000(_edited(gs.random_uniforms(22, 9, 3, 8, 16, 16))),
    "neg_radius": _neg_radius,
    "sanglet_ge_1": _sanglet_ge_1,
    "no_lights": _no_lights,
    "max_spheres_a": lambda: gs.random_uniforms(51, 40, 4, 56, 16, 16),
    "max_spheres_b": _max_spheres_b,
}


def corner(name, w, h):
    u = _CORNER_BLOCKS[name]()
    u["size"] = (F(w), F(h))
    return u


# ---------------------------------------------------------------- the tags

def tags_of(u):
    """The classes a block belongs to, from its numbers alone."""
    sc, lc, al = int(u["sphere_count"]), int(u["light_count"]), int(u["all_spheres_count"])
    S = np.asarray(u["spheres"], dtype=F)
    cam = np.asarray(u["campos"], dtype=F)
    tags = set()
    negzero = bool(((cam == 0) & np.signbit(cam)).any())
    if sc and (S[:sc, :3].view(np.uint32) == cam.view(np.uint32)).all(axis=1).any():
        tags.add("cam_at_wall_centre")
    if negzero:
        tags.add("cam_negzero")
    if sc and not negzero and gv.wall_start(u, cam) == 3 * sc:
        tags.add("cam_outside_walls")
    if float(F(u["rotation"][0])) in QUARTER_TURNS and float(F(u["rotation"][1])) in (0.0, 0.5):
        tags.add("quarter_turn")
    if al and (S[:al] * 2 == np.round(S[:al] * 2)).all():
        tags.add("half_grid")
    shadow = S[sc + lc:al].astype(np.float64)
    lights = S[sc:sc + lc].astype(np.float64)
    for b in shadow:  # collinear with a light and campos, to rounding
        for a in lights:
            p, q = b[:3] - a[:3], cam.astype(np.float64) - a[:3]
            scale = np.linalg.norm(p) * np.linalg.norm(q)
            if scale > 0 and np.linalg.norm(np.cross(p, q)) <= 1e-5 * scale:
                tags.add("ball_on_light_segment")
            if (b[:3] == a[:3]).all():
                tags.add("ball_on_light")
    if al > sc and (S[sc:al, 3] == 0).any():
        tags.add("zero_radius")
    if len({r.tobytes() for r in S[sc:al]}) < al - sc:
        tags.add("duplicate_ball")
    if sc > 64:
        tags.add("walls_gt_64")
    pairs = gv.shadow_pairs(u, cam)
    if any(999.0 <= d <= 1001.0 for _, d in pairs):  # a pair at the lit shortcut's bound
        tags.add("far_ball")
    if sc and np.abs(S[:sc]).max() >= 1000.0:  # the generators stay within 13 otherwise
        tags.add("x1000")
    if (S[sc + lc:al, 3] < 0).any():
        tags.add("neg_radius")
    if any(s >= 1.0 for s, _ in pairs):
        tags.add("sanglet_ge_1")
    if lc == 0 and al > sc:
        tags.add("no_lights")
    if al == MAX_SPHERES:
        tags.add("max_spheres")
    if F(u["fov"][0]) >= F(1.5):  # random_uniforms' own is FOV_H < 1.5
        tags.add("wide_fov")
    return frozenset(tags)


# ---------------------------------------------------------------- the list

def make_case(kind, name, make, index):
    """The case at position `index` of a list: make(w, h) is its block."""
    w, h = SIZES[index % len(SIZES)]
    u = np.array(make(w, h), copy=True)
    assert tuple(u["size"]) == (w, h)
    u.setflags(write=False)
    return Case(f"{kind}-{name}", u, w, h, index % 2, tags_of(u) | {kind})


@functools.lru_cache(maxsize=None)
def cases():
    """The fixed ordered list: random (a world block for every fourth) and adversarial seeds
    alternating, the corner blocks at CORNERS."""
    rand = sorted(RANDOM_SEEDS + WORLD_SEEDS)
    order = []
    for k in range(max(len(rand), len(ADVERSARIAL_SEEDS))):
        if k < len(rand):
            order.append(("world" if rand[k] % 4 == 1 else "random", rand[k]))
        if k < len(ADVERSARIAL_SEEDS):
            order.append(("adversarial", ADVERSARIAL_SEEDS[k]))
    for at in sorted(CORNERS):
        order.insert(at, ("corner", CORNERS[at]))
    out = []
    for index, (kind, v) in enumerate(order):
        if kind == "corner":
            out.append(make_case(kind, v, functools.partial(corner, v), index))
        else:
            mode = "adversarial" if kind == "adversarial" else "random"
            out.append(make_case(kind, str(v), functools.partial(generated, mode, v), index))
    return tuple(out)


def camera_of(u):
    """((campos), (rotation, hrotation), (fov_h, fov_v)) of a block, as Python floats of its
    binary32 values (a -0.0 stays one): the camera of glsl_views_cases.with_camera."""
    return (tuple(float(x) for x in u["campos"]), tuple(float(x) for x in u["rotation"]),
            tuple(float(x) for x in u["fov"]))


def other_blocks(index, count=4):
    """The blocks of the next `count` cases of the fixed list (the list wraps round)."""
    cs = cases()
    return [cs[(index + q) % len(cs)].uniforms for q in range(1, count + 1)]


def borrowed_cameras(others):
    """The cameras a view batch borrows: (campos, rotation, fov) of the next four blocks."""
    return [camera_of(o) for o in others[:4]]


def borrowed_rotations(u, others):
    """The cameras whose pixel directions a ray batch borrows: the case's own campos and fov under
    the rotation of the next two blocks."""
    own = camera_of(u)
    return [(own[0], camera_of(o)[1], own[2]) for o in others[:2]]


def asked_frames(case, others):
    """{name: (block, width, height)} of every frame a family check asks the restatement for: the
    own camera at S = 1, 2, 4, each borrowed camera, each borrowed rotation."""
    u, w, h = case.uniforms, case.width, case.height
    own = camera_of(u)
    out = {f"own-s{s}": (gv.with_camera(u, own, s), s * w, s * h) for s in (1, 2, 4)}
    for q, cam in enumerate(borrowed_cameras(others)):
        out[f"view{q + 1}"] = (gv.with_camera(u, cam), w, h)
    for q, cam in enumerate(borrowed_rotations(u, others)):
        out[f"rotation{q + 1}"] = (gv.with_camera(u, cam), w, h)
    return out


def capped_frames(case, others, floor, threads=1):
    """The names of asked_frames for which the restatement reaches its march cap."""
    import oracle
    bad = []
    for name, (u, w, h) in asked_frames(case, others).items():
        try:
            oracle.GlslOracle(u, *floor).render(w, h, threads)
        except RuntimeError:
            bad.append(name)
    return bad
