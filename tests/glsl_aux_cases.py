"""Shared cases and expected values of tests/test_glsl_aux.py and tests/test_glsl_cast_rays.py
(not a test module): the uniform blocks, and per block and size the restatement's per-pixel dump
(oracle/glsl_oracle.c oglsl_pixel) as arrays, computed once per session and never modified.

What the planes and the ray outputs must equal, bit for bit (rayShader.frag line numbers):
  depth   oglsl_dump.total_dist   totalDist after :117
  sphere  oglsl_dump.draw_sphere  drawSphere after :118
  steps   oglsl_dump.march_steps  trips of the metaball loop :94-112
  pos     :119 rebuilt in binary32 from the dump: checkstep * wall_pos + (1 - checkstep) *
          (campos + dir * ball_dist), each product and sum rounded, no contraction
  rgba    the restatement's frame
"""
import functools

import numpy as np

import glsl_scenes as gs
import oracle
import scenes
import test_glsl as tg

F = np.float32
SIZES = [(40, 24), (37, 23)]   # 37x23: edge lanes in every tile row and column; 851 rays = 13 waves + 19

CASES = {
    "default": lambda w, h: gs.default_uniforms(w, h),
    "posed": lambda w, h: gs.default_uniforms(w, h, 0.7, 0.3),
    "random2": lambda w, h: gs.random_uniforms(2, 12, 2, 14, w, h),
    "random3": lambda w, h: gs.random_uniforms(3, 40, 4, 50, w, h),
}
# the edge uniforms of tests/test_glsl.py; exempt from the content rule where they cannot meet it
EDGE = {
    "no_walls": tg._no_walls, "walls_only": tg._walls_only, "empty": tg._empty,
    "negzero_cam": tg._negzero_cam, "camera_outside": tg._camera_outside,
}
ALL = {**CASES, **EDGE}
# ball pixels of the four named cases at 40x24 (measured on the restatement)
BALL_PIXELS_40x24 = {"default": 171, "posed": 323, "random2": 210, "random3": 799}


@functools.lru_cache(maxsize=None)
def floor():
    return scenes.load_floor()


def uniforms(name, w, h, scale=1):
    """The block of case `name` for a w x h target; scale S: the block the supersampled
    fragments see, `size` scaled by S (exact in binary32)."""
    u = np.array(ALL[name](w, h), copy=True)
    if scale != 1:
        u["size"] = (F(u["size"][0]) * F(scale), F(u["size"][1]) * F(scale))
    return u


def _freeze(d):
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def expected(name, w, h, scale=1):
    """{depth, sphere, steps, checkstep, dir, pos: (h, w[, 3])} for output pixel (i, row): the
    dump of pixel (scale * i, scale * row) of the scale*w x scale*h target with `size` scaled."""
    u = uniforms(name, w, h, scale)
    o = oracle.GlslOracle(u, *floor())
    out = {"depth": np.zeros((h, w), F), "sphere": np.zeros((h, w), np.int32),
           "steps": np.zeros((h, w), np.int32), "checkstep": np.zeros((h, w), np.int32),
           "dir": np.zeros((h, w, 3), F), "pos": np.zeros((h, w, 3), F)}
    cam = np.asarray(u["campos"], F)
    for row in range(h):
        for i in range(w):
            d = o.pixel(scale * w, scale * h, scale * i, scale * row)
            out["depth"][row, i] = d["total_dist"]
            out["sphere"][row, i] = d["draw_sphere"]
            out["steps"][row, i] = d["march_steps"]
            out["checkstep"][row, i] = d["checkstep"]
            dr = np.asarray(d["dir"], F)
            out["dir"][row, i] = dr
            cs = F(d["checkstep"])
            ball = (cam + (dr * F(d["ball_dist"])).astype(F)).astype(F)          # :119
            out["pos"][row, i] = ((cs * np.asarray(d["wall_pos"], F)).astype(F) +
                                  ((F(1) - cs) * ball).astype(F)).astype(F)
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def expected_rgba(name, w, h):
    a = oracle.GlslOracle(uniforms(name, w, h), *floor()).render(w, h, 1).reshape(h, w, 4)
    a.setflags(write=False)
    return a


def check_content(name, w, h):
    """Each expected frame of a named case holds a wall pixel, a ball pixel and two distinct step
    counts; an edge case is held to what its uniforms allow."""
    e = expected(name, w, h)
    walls, balls = int((e["checkstep"] == 1).sum()), int((e["checkstep"] == 0).sum())
    nsteps = len(np.unique(e["steps"]))
    if name in CASES:
        assert walls > 0 and balls > 0 and nsteps >= 2, (name, walls, balls, nsteps)
        if (w, h) == (40, 24):
            assert balls == BALL_PIXELS_40x24[name], (name, balls)
    else:  # no walls, no balls or nothing in view: whatever the restatement gives
        assert walls + balls == w * h
    return walls, balls, nsteps


def bits(a):
    """The array's 4-byte elements as uint32, for comparisons on bits (NaN payloads, -0.0)."""
    return np.ascontiguousarray(a).view(np.uint32)
