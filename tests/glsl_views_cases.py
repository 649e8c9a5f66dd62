"""Shared cases and expected values of tests/test_glsl_views.py and tests/test_glsl_views_abi.py
(not a test module): one scene, eight cameras, and per camera the restatement's frame and per-pixel
dump (oracle/glsl_oracle.c) for the uniform block that has the camera's three uniforms -- campos,
rotation, fov -- substituted, computed once per session and never modified.

The scene is gs.default_uniforms(W, H, 0.7, 0.3) at 37 x 23: 5 x 3 tiles, so edge lanes in every
tile row and column, and 15 tiles, so the last four-tile workgroup of a row-major launch has a tail
wave.  Its ten walls are sorted by the distance from the origin; the origin lies in wall 2 first.

The cameras (position, (rotation, hrotation), (fov_h, fov_v)):
  0  the scene's own campos / rotation / fov
  1  the same position, another rotation and hrotation, fov halved in x only
  2  inside wall 4 first (view 0: wall 2): another wall_start
  3  (30, 2, -25), outside every wall: wall_start 3 * sphereCount, no lane ever moves
  4  a -0.0 component: the wall pass's literal update from iteration 0
  5  (1500, 0, 0), at least 1000 from every shadow ball: no pair may keep the lit shortcut
  6, 7  inside the cave, facing the balls
Three more scenes with three cameras each: tests/test_glsl.py's _no_walls and _walls_only, and
gs.random_uniforms(5, 70, 2, 10, W, H) with more than 64 walls (no wall cull).
"""
import functools

import numpy as np

import glsl_scenes as gs
import oracle
import scenes
import test_glsl as tg
from conftest import host_threads

F = np.float32
W, H = 37, 23
SS_VIEWS = (0, 1, 2)   # the views rendered with S = 2


def base_uniforms():
    return gs.default_uniforms(W, H, 0.7, 0.3)


_B = base_uniforms()
_HALF_FOV = (float(F(_B["fov"][0]) / F(2)), float(_B["fov"][1]))
_FOV = (float(_B["fov"][0]), float(_B["fov"][1]))
CAMS = [
    (tuple(float(c) for c in _B["campos"]), (float(_B["rotation"][0]), float(_B["rotation"][1])), _FOV),
    ((0.0, 0.0, 0.0), (0.9, 0.45), _HALF_FOV),
    ((-7.5, 0.5, 1.5), (0.7, 0.3), _FOV),
    ((30.0, 2.0, -25.0), (0.2, 0.1), _FOV),
    ((-0.0, 0.25, 0.5), (0.4, 0.1), _FOV),
    ((1500.0, 0.0, 0.0), (1.0, 0.0), _FOV),
    ((1.0, 0.5, -1.0), (5.5, -0.3), _FOV),
    ((-1.5, -0.5, 1.5), (1.3, 0.3), _FOV),
]

EXTRA = {
    "no_walls": lambda: tg._no_walls(W, H),
    "walls_only": lambda: tg._walls_only(W, H),
    "many_walls": lambda: gs.random_uniforms(5, 70, 2, 10, W, H),
}


def extra_cams(name):
    """Three cameras for an extra scene: its own, and two near it turned elsewhere."""
    u = EXTRA[name]()
    pos = tuple(float(c) for c in u["campos"])
    rot = (float(u["rotation"][0]), float(u["rotation"][1]))
    fov = (float(u["fov"][0]), float(u["fov"][1]))
    return [(pos, rot, fov),
            ((float(F(pos[0]) + F(0.25)), pos[1], float(F(pos[2]) - F(0.125))),
             (float(F(rot[0]) + F(1.5)), float(-F(rot[1]))), fov),
            ((pos[0], float(F(pos[1]) - F(0.25)), pos[2]), (float(F(rot[0]) + F(3.0)), 0.25),
             (float(F(fov[0]) * F(0.75)), fov[1]))]


@functools.lru_cache(maxsize=None)
def floor():
    return scenes.load_floor()


def with_camera(u, cam, scale=1):
    """The block with the camera's three uniforms substituted; scale S: the block the supersampled
    fragments see, `size` scaled by S (exact in binary32)."""
    pos, rot, fov = cam
    v = np.array(u, copy=True)
    v["campos"] = pos
    v["rotation"] = rot
    v["fov"] = fov
    if scale != 1:
        v["size"] = (F(v["size"][0]) * F(scale), F(v["size"][1]) * F(scale))
    return v


def _scene(name):
    return base_uniforms() if name == "base" else EXTRA[name]()


def cams_of(name):
    return CAMS if name == "base" else extra_cams(name)


def view_uniforms(k, scale=1, name="base"):
    return with_camera(_scene(name), cams_of(name)[k], scale)


def _box(big, s):
    """(H, W, 4) uint8 from the flat RGBA8 frame of s*W x s*H pixels: the S x S box, rounded half
    up (the rule stated for SFRT_OPT_SUPERSAMPLE)."""
    if s == 1:
        return np.array(big, dtype=np.uint8).reshape(H, W, 4)
    sums = big.reshape(H, s, W, s, 4).astype(np.uint32).sum(axis=(1, 3))
    return ((sums + s * s // 2) >> {2: 2, 4: 4}[s]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def frame(k, scale=1, name="base"):
    """View k's expected (H, W, 4) colours; raises if a pixel reaches the march cap."""
    o = oracle.GlslOracle(view_uniforms(k, scale, name), *floor())
    a = _box(o.render(scale * W, scale * H, host_threads()), scale)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def planes(k, scale=1, name="base"):
    """{depth, sphere, steps, checkstep: (H, W)} for output pixel (i, row) of view k: the dump of
    pixel (scale * i, scale * row) of the scale*W x scale*H target (the first sample)."""
    o = oracle.GlslOracle(view_uniforms(k, scale, name), *floor())
    out = {"depth": np.zeros((H, W), F), "sphere": np.zeros((H, W), np.int32),
           "steps": np.zeros((H, W), np.int32), "checkstep": np.zeros((H, W), np.int32)}
    for row in range(H):
        for i in range(W):
            d = o.pixel(scale * W, scale * H, scale * i, scale * row)
            out["depth"][row, i] = d["total_dist"]
            out["sphere"][row, i] = d["draw_sphere"]
            out["steps"][row, i] = d["march_steps"]
            out["checkstep"][row, i] = d["checkstep"]
    for a in out.values():
        a.setflags(write=False)
    return out


def wall_start(u, pos):
    """sfrt_glsl.cpp's wall_start in numpy, with the kernel's containment test
    step(length(rpos), r) on binary32 values: the first wall that holds the camera, 3 * sphereCount
    when none does, 0 with a -0.0 component."""
    cam = np.asarray(pos, F)
    sc = int(u["sphere_count"])
    if any(np.signbit(c) and c == 0 for c in cam):
        return 0
    for j in range(sc):
        r = cam - np.asarray(u["spheres"][j, :3], F)
        s = F(F(r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
        if np.sqrt(s) <= F(u["spheres"][j, 3]):
            return j
    return 3 * sc


def shadow_pairs(u, pos):
    """Per (light, shadow ball) pair: (sanglet, |campos - ball|) in binary32, as the host's pair
    table computes them (atan2 in double, rounded: the bound below is not near a rounding)."""
    sc, lc, al = int(u["sphere_count"]), int(u["light_count"]), int(u["all_spheres_count"])
    cam = np.asarray(pos, F)
    out = []
    for li in range(lc):
        a = np.asarray(u["spheres"][sc + li], F)
        for k in range(sc + lc, al):
            b = np.asarray(u["spheres"][k], F)
            q = a[:3] - b[:3]
            dist = np.sqrt(F(F(q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]))
            c = cam - b[:3]
            dcam = np.sqrt(F(F(c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]))
            out.append((float(np.arctan2(np.float64(b[3]), np.float64(dist))), float(dcam)))
    return out
