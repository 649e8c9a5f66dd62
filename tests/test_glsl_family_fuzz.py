"""Every GLSL kernel family against the restatement on the degenerate blocks of
tests/glsl_fuzz_cases.py: the planes, the tile orders, in-kernel supersampling, the view batches
and the ray batches.

Every comparison is on bit patterns, with no tolerance, and no case is skipped.  The references
are oracle.GlslOracle's own: its frame for the colour (box-filtered for S > 1, the filter of
tests/glsl_views_cases.py) and one per-pixel dump per output pixel for depth / sphere / steps / pos,
by the method of glsl_aux_cases.expected (S > 1: the first sample's).  Device targets are
0xA5-poisoned with a pitch per target (the ray batches: canary bytes past the count), and a whole
canvas, padding included, must equal the expected one.

The checks are functions of a `Ctx` (a case and the blocks it borrows cameras from), so that
tests/test_parity_sweep.py::test_glsl_family_sweep can run them over any seeds.
"""
import functools

import numpy as np
import pytest

import glsl_fuzz_cases as fuzz
import glsl_scenes as gs
import glsl_views_cases as gv
from conftest import host_threads, poisoned
from test_glsl_cast_rays import OUT, assert_rays, dev_cast, frame_dirs, length32

F = np.float32
POISON = 0xA5
PLANES = ("depth", "sphere", "steps")
PADS = {"colour": 20, "depth": 4, "sphere": 36, "steps": 12}  # every target its own pitch
CUT = 5  # the row two bands are cut at: no edge of the 8-row tiles
CHUNK = 8
CHUNKS = [range(a, min(a + CHUNK, 48)) for a in range(0, 48, CHUNK)]
chunks = pytest.mark.parametrize("chunk", CHUNKS, ids=[f"cases{c.start}-{c.stop - 1}" for c in CHUNKS])
# non-finite and unusable directions, answered with sphere -1 and zeros; 1e-20 and 1e20 scale a
# unit direction to a squared length that is no finite normal number
INVALID = [F([0, 0, 0]), F([-0.0, 0.0, -0.0]), F([np.nan, 0, 1]), F([0, -np.inf, 0]), 1e-20, 1e20]


def _box(big, w, h, s):
    """glsl_views_cases._box for any size: (h, w, 4) from the flat frame of s*w x s*h pixels."""
    if s == 1:
        return np.array(big, dtype=np.uint8).reshape(h, w, 4)
    sums = big.reshape(h, s, w, s, 4).astype(np.uint32).sum(axis=(1, 3))
    return ((sums + s * s // 2) >> {2: 2, 4: 4}[s]).astype(np.uint8)


def dump_planes(u, w, h, s=1):
    """glsl_aux_cases.expected for a block: {depth, sphere, steps, checkstep, dir, pos} of output
    pixel (i, row), the dump of pixel (s * i, s * row) of the s*w x s*h target; `u` holds the
    scaled `size` already.  The same per-pixel call (oglsl_pixel) and the same binary32
    expression for pos (:119), with the rows shared among threads and pos evaluated on arrays."""
    import ctypes
    from concurrent.futures import ThreadPoolExecutor
    import oracle
    o = oracle.GlslOracle(u, *gv.floor())
    pixel, args = oracle.lib().oglsl_pixel, o._args()
    out = {"depth": np.zeros((h, w), F), "sphere": np.zeros((h, w), np.int32),
           "steps": np.zeros((h, w), np.int32), "checkstep": np.zeros((h, w), np.int32),
           "dir": np.zeros((h, w, 3), F)}
    wall_pos, ball_dist = np.zeros((h, w, 3), F), np.zeros((h, w), F)

    def rows(part):
        d = oracle.OglslDump()
        ref = ctypes.byref(d)
        for row in part:
            for i in range(w):
                pixel(*args, s * w, s * h, s * i, s * row, ref)
                out["depth"][row, i], out["sphere"][row, i] = d.total_dist, d.draw_sphere
                out["steps"][row, i], out["checkstep"][row, i] = d.march_steps, d.checkstep
                out["dir"][row, i] = d.dir[:]
                wall_pos[row, i], ball_dist[row, i] = d.wall_pos[:], d.ball_dist

    threads = min(8, host_threads(), h)
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(rows, [range(k, h, threads) for k in range(threads)]))
    cam = np.asarray(u["campos"], F)
    cs = out["checkstep"].astype(F)[..., None]
    with np.errstate(all="ignore"):
        ball = (cam + (out["dir"] * ball_dist[..., None]).astype(F)).astype(F)          # :119
        out["pos"] = ((cs * wall_pos).astype(F) + ((F(1) - cs) * ball).astype(F)).astype(F)
    assert out["pos"].dtype == F
    for a in out.values():
        a.setflags(write=False)
    return out


class Ctx:
    """A case, the blocks whose cameras it borrows, and its references, each computed once."""

    def __init__(self, case, index, others):
        self.case, self.index, self.others = case, index, list(others)
        self.u, self.w, self.h = case.uniforms, case.width, case.height
        self.cam = fuzz.camera_of(self.u)
        self.cams = [self.cam] + fuzz.borrowed_cameras(self.others)
        self.turned = fuzz.borrowed_rotations(self.u, self.others)
        self._memo = {}

    def memo(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def block(self, s=1, cam=None):
        return gv.with_camera(self.u, self.cam if cam is None else cam, s)

    def frame(self, s=1, cam=None):
        """(h, w, 4): the restatement's frame (box-filtered for s > 1); shared, read-only."""
        import oracle

        def make():
            o = oracle.GlslOracle(self.block(s, cam), *gv.floor())
            a = _box(o.render(s * self.w, s * self.h, host_threads()), self.w, self.h, s)
            a.setflags(write=False)
            return a
        return self.memo(("frame", s, cam), make)

    def planes(self, s=1, cam=None):
        return self.memo(("planes", s, cam), lambda: dump_planes(self.block(s, cam), self.w, self.h, s))


@functools.lru_cache(maxsize=None)
def ctx(index):
    """The Ctx of case `index` of the fixed list."""
    return Ctx(fuzz.cases()[index], index, fuzz.other_blocks(index))


# ---------------------------------------------------------------- CPU: the list

def test_the_list_meets_its_conditions(built):
    cs = fuzz.cases()
    assert 40 <= len(cs) <= 48 and len({c.id for c in cs}) == len(cs)
    assert cs is fuzz.cases()  # fixed
    for k, c in enumerate(cs):
        assert (c.width, c.height) == fuzz.SIZES[k % len(fuzz.SIZES)] and c.tile_order == k % 2
        assert tuple(c.uniforms["size"]) == (c.width, c.height)
        assert c.tags == fuzz.tags_of(c.uniforms) | {c.id.split("-")[0]}
    kinds = {kind: [c for c in cs if kind in c.tags] for kind in ("random", "world", "adversarial", "corner")}
    assert len(kinds["random"]) >= 16 and len(kinds["adversarial"]) >= 16 and len(kinds["world"]) >= 2
    assert [int(c.id.split("-")[1]) for c in kinds["random"]] == fuzz.RANDOM_SEEDS
    assert [int(c.id.split("-")[1]) for c in kinds["world"]] == fuzz.WORLD_SEEDS
    assert [int(c.id.split("-")[1]) for c in kinds["adversarial"]] == fuzz.ADVERSARIAL_SEEDS
    assert min(fuzz.RANDOM_SEEDS + fuzz.WORLD_SEEDS) >= 20000 and min(fuzz.ADVERSARIAL_SEEDS) >= 50000
    assert all(s % 4 == 1 for s in fuzz.WORLD_SEEDS) and all(s % 4 != 1 for s in fuzz.RANDOM_SEEDS)
    assert {k: cs[k].id for k in fuzz.CORNERS} == {k: f"corner-{v}" for k, v in fuzz.CORNERS.items()}
    for name, count in (("walls64", 64), ("walls65", 65), ("walls70", 70)):
        (c,) = [c for c in cs if c.id == f"corner-{name}"]
        assert int(c.uniforms["sphere_count"]) == count
    for tag in fuzz.ADVERSARIAL_CLASSES:
        assert sum(tag in c.tags for c in kinds["adversarial"]) >= 3, tag
    for tag in fuzz.ADVERSARIAL_CLASSES + fuzz.OTHER_TAGS:
        assert sum(tag in c.tags for c in cs) >= 2, tag
    # the restatement alone gives every asked frame a defined answer: no march reaches the cap
    for k, c in enumerate(cs):
        assert fuzz.capped_frames(c, fuzz.other_blocks(k), gv.floor(), host_threads()) == [], c.id


def test_the_frames_hold_what_the_checks_are_for(built):
    """Non-vacuity, from the dumps of the cases' own frames and the pair tables."""
    cs = fuzz.cases()
    both = three = 0
    for k, c in enumerate(cs):
        e = ctx(k).planes()
        walls, balls = e["checkstep"] == 1, e["checkstep"] == 0
        both += bool(walls.any() and balls.any())
        three += len(np.unique(e["steps"])) >= 3
        if "far_ball" in c.tags:
            assert (walls & (e["depth"] < F(1000))).any(), c.id
            near = [d < 1000.0 for _, d in gv.shadow_pairs(c.uniforms, c.uniforms["campos"])]
            assert any(near) and not all(near), c.id
            # a borrowed camera changes, for some pair, whether every camera of the batch is near
            views = [[d < 1000.0 for _, d in gv.shadow_pairs(c.uniforms, cam[0])] for cam in ctx(k).cams[1:]]
            assert any(own and not all(v[p] for v in views) for p, own in enumerate(near)), c.id
    assert 2 * both >= len(cs), both
    assert three >= 10, three


# ---------------------------------------------------------------- GPU: helpers

def _shader(c, s=1, order=None):
    import sfrt
    sh = sfrt.GlslShader(0)
    sh.set_ground(*gv.floor())
    sh.set_uniforms(c.u)
    sh.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
    sh.set_option(sfrt.SFRT_OPT_TILE_ORDER, c.case.tile_order if order is None else order)
    return sh


def _camera(cam):
    import sfrt
    pos, rot, fov = cam
    c = sfrt.Camera()
    for q in range(3):
        c.pos[q] = pos[q]
    c.rotation, c.hrotation = rot
    c.fov_h, c.fov_v = fov
    return c


def _stream():
    import torch
    return torch.cuda.Stream()


def _same_canvas(got, content, what):
    """got (h, pitch) uint8 equals `content` ((h, w) 4-byte elements or (h, w, 4) bytes) and
    POISON in the padding past 4w."""
    h, w = content.shape[:2]
    want = np.full(got.shape, POISON, dtype=np.uint8)
    want[:, :4 * w] = np.ascontiguousarray(content).view(np.uint8).reshape(h, 4 * w)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} bytes differ, first (row, byte) {tuple(bad[0])}"


class Targets:
    """Poisoned whole-frame device targets: the colour and each plane, every one its own pitch."""

    def __init__(self, w, h, planes=PLANES):
        self.planes = tuple(planes)
        self.pitch = {k: 4 * w + PADS[k] for k in ("colour",) + self.planes}
        self.buf = {k: poisoned((h, p), POISON) for k, p in self.pitch.items()}

    def args(self, row=0):
        return {p: (self.buf[p].data_ptr() + row * self.pitch[p], self.pitch[p]) for p in self.planes}

    def colour_ptr(self, row=0):
        return self.buf["colour"].data_ptr() + row * self.pitch["colour"]

    def check(self, colour, planes, what):
        want = {"colour": colour, **{p: planes[p] for p in self.planes}}
        for k, b in self.buf.items():
            _same_canvas(b.cpu().numpy(), want[k], f"{what}: {k}")


# ---------------------------------------------------------------- the family checks

def check_planes(c, s=1):
    """draw_aux (the whole frame, and two bands cut at row CUT) and draw_image_aux: the colour is
    the restatement's frame, the planes its dumps (s > 1: the first sample's)."""
    what = f"{c.case.id} planes S={s}"
    colour, want = c.frame(s), c.planes(s)
    stream = _stream()
    with _shader(c, s) as sh:
        whole, banded = Targets(c.w, c.h), Targets(c.w, c.h)
        sh.draw_aux(whole.colour_ptr(), c.w, c.h, whole.pitch["colour"], 0, c.h, stream.cuda_stream,
                    **whole.args())
        for row0, rows in ((0, CUT), (CUT, c.h - CUT)):
            sh.draw_aux(banded.colour_ptr(row0), c.w, c.h, banded.pitch["colour"], row0, rows,
                        stream.cuda_stream, **banded.args(row0))
        sh.check(stream.cuda_stream)
        whole.check(colour, want, what + " whole frame")
        banded.check(colour, want, what + " two bands")
        img = sh.draw_image_aux(c.w, c.h)
        _same_canvas(img["rgba"].reshape(c.h, 4 * c.w), colour, what + " draw_image_aux: colour")
        for p in PLANES:
            _same_canvas(img[p].view(np.uint8).reshape(c.h, 4 * c.w), want[p],
                         f"{what} draw_image_aux: {p}")


def check_orders(c):
    """Three draws on one shader (the adaptive order is in use from the third) under the case's
    SFRT_OPT_TILE_ORDER and under the other value, and draw_image, the row-major kernel without
    the wall cull: every frame is the restatement's."""
    colour = c.frame()
    stream = _stream()
    pitch = 4 * c.w + 16
    for order in (c.case.tile_order, 1 - c.case.tile_order):
        with _shader(c, 1, order) as sh:
            for k in range(3):
                buf = poisoned((c.h, pitch), POISON)
                sh.draw(buf.data_ptr(), c.w, c.h, pitch, 0, c.h, stream.cuda_stream)
                sh.check(stream.cuda_stream)
                _same_canvas(buf.cpu().numpy(), colour, f"{c.case.id} order {order} draw {k + 1}")
            got = sh.draw_image(c.w, c.h).reshape(c.h, 4 * c.w)
            _same_canvas(got, colour, f"{c.case.id} order {order} draw_image")


def check_supersample(c):
    """S = 2 and 4 through draw and draw_image against the box-filtered frame of the S*w x S*h
    target with `size` scaled, and with planes: those of the group's first sample."""
    for s in (2, 4):
        what = f"{c.case.id} S={s}"
        colour = c.frame(s)
        stream = _stream()
        with _shader(c, s) as sh:
            pitch = 4 * c.w + 16
            buf = poisoned((c.h, pitch), POISON)
            sh.draw(buf.data_ptr(), c.w, c.h, pitch, 0, c.h, stream.cuda_stream)
            sh.check(stream.cuda_stream)
            _same_canvas(buf.cpu().numpy(), colour, what + " draw")
            _same_canvas(sh.draw_image(c.w, c.h).reshape(c.h, 4 * c.w), colour, what + " draw_image")
        check_planes(c, s)


def check_views(c):
    """The case's camera and four borrowed ones as one render_views_aux batch, and as a
    render_views batch in the reverse order: each view is the restatement's of the block with
    that camera substituted.  Afterwards a draw with no setter between gives the shader's own
    frame and the uniform block reads back bytewise unchanged."""
    stream = _stream()
    with _shader(c) as sh:
        before = sh.get_uniforms(gs.UNIFORM_DTYPE).tobytes()
        assert before == np.ascontiguousarray(c.u).tobytes()
        views = [Targets(c.w, c.h) for _ in c.cams]
        pitch = views[0].pitch["colour"]
        sh.render_views_aux([(_camera(cam), t.colour_ptr()) for cam, t in zip(c.cams, views)],
                            [t.args() for t in views], c.w, c.h, pitch, stream=stream.cuda_stream)
        sh.check(stream.cuda_stream)
        for k, (cam, t) in enumerate(zip(c.cams, views)):
            t.check(c.frame(1, cam), c.planes(1, cam), f"{c.case.id} aux view {k}")
        back = list(reversed(c.cams))
        plain = [poisoned((c.h, pitch), POISON) for _ in back]
        sh.render_views([(_camera(cam), b.data_ptr()) for cam, b in zip(back, plain)], c.w, c.h,
                        pitch, stream=stream.cuda_stream)
        sh.check(stream.cuda_stream)
        for k, (cam, b) in enumerate(zip(back, plain)):
            _same_canvas(b.cpu().numpy(), c.frame(1, cam), f"{c.case.id} reversed view {k}")
        buf = poisoned((c.h, pitch), POISON)
        sh.draw(buf.data_ptr(), c.w, c.h, pitch, 0, c.h, stream.cuda_stream)
        sh.check(stream.cuda_stream)
        _same_canvas(buf.cpu().numpy(), c.frame(), f"{c.case.id}: the shader's own draw after the batches")
        assert sh.get_uniforms(gs.UNIFORM_DTYPE).tobytes() == before, c.case.id


def frame_rays(c, cam=None):
    """(dirs, expected) of the rays of the frame from `cam` (None: the case's own), row-major.
    A batch normalises what it is given (:65), so a ray reproduces its pixel where that division
    changes nothing: with the rotation (0, 0) every pixel, from test_glsl_cast_rays.frame_dirs'
    un-normalised directions (pinned there to the restatement's `dir`); under any other rotation
    the pixels whose normalised `dir` has the binary32 length exactly 1, as
    test_unit_direction_rays_of_other_rotations selects them."""
    def make():
        e, rgba = c.planes(1, cam), c.frame(1, cam).reshape(-1, 4)
        block = c.block(1, cam)
        unit = e["dir"].reshape(-1, 3)
        if tuple(block["rotation"]) == (0.0, 0.0):
            keep = np.arange(c.w * c.h)
            dirs = frame_dirs(block, c.w, c.h)
            with np.errstate(all="ignore"):
                assert np.array_equal((dirs / length32(dirs)[:, None]).astype(F).view(np.uint32),
                                      unit.view(np.uint32)), c.case.id
        else:
            keep = np.nonzero(length32(unit) == F(1))[0]
            dirs = unit[keep]
        want = {"pos": e["pos"].reshape(-1, 3)[keep], "depth": e["depth"].ravel()[keep],
                "sphere": e["sphere"].ravel()[keep], "steps": e["steps"].ravel()[keep],
                "rgba": rgba[keep]}
        return np.ascontiguousarray(dirs), {k: np.ascontiguousarray(v) for k, v in want.items()}
    return c.memo(("rays", cam), make)


def _tail(dirs, want):
    """The set cut by one ray where its count would fill its last wave."""
    n = len(dirs) - (len(dirs) % 64 == 0)
    return dirs[:n], {k: v[:n] for k, v in want.items()}


def _scaled(dirs, seed):
    """Each ray times a power of two in 2^-40 .. 2^40: exact, so the normalised direction stays."""
    k = np.random.default_rng(seed).integers(-40, 41, len(dirs))
    out = (dirs * np.exp2(k).astype(F)[:, None]).astype(F)
    assert np.array_equal(np.ldexp(out.astype(np.float64), -k[:, None]), dirs.astype(np.float64))
    return out


def check_rays(c):
    """cast_rays_device with all five outputs: the frame's own rays row-major and shuffled, each
    scaled by a power of two; the rays of the two borrowed rotations from the case's campos; and
    unusable directions at fixed places in six different waves, answered with sphere -1 and zeros.
    Every count leaves a tail wave; dev_cast asserts the canary bytes past the count."""
    stream = _stream()
    with _shader(c) as sh:
        dirs, want = _tail(*frame_rays(c))
        assert len(dirs) >= c.w * c.h // 4, (c.case.id, len(dirs))
        got = dev_cast(sh, stream, _scaled(dirs, 3 + c.index))
        assert_rays(got, want, what=f"{c.case.id}: own rays, row-major")
        shuffle = np.random.default_rng(7).permutation(len(dirs))
        got = dev_cast(sh, stream, _scaled(dirs, 5 + c.index)[shuffle])
        assert_rays(got, want, shuffle, what=f"{c.case.id}: own rays, shuffled")
        for q, cam in enumerate(c.turned):
            td, tw = _tail(*frame_rays(c, cam))
            assert len(td) >= c.w * c.h // 4, (c.case.id, q, len(td))
            assert_rays(dev_cast(sh, stream, td), tw, what=f"{c.case.id}: rays of borrowed rotation {q + 1}")
        # the own rays repeated to six waves and a tail, an unusable direction in each wave
        reps = -(-(6 * 64 + 19) // len(dirs))
        idx = np.tile(np.arange(len(dirs)), reps)
        idx = idx[:len(idx) - (len(idx) % 64 == 0)]
        d = np.array(dirs[idx], copy=True)
        waves = len(d) // 64
        where = [64 * (k * waves // 6) + 7 * k + 3 for k in range(6)]
        assert len({at // 64 for at in where}) == 6
        with np.errstate(all="ignore"):
            for at, bad in zip(where, INVALID):
                d[at] = bad if isinstance(bad, np.ndarray) else (d[at] * F(bad)).astype(F)
        valid = np.setdiff1d(np.arange(len(d)), where)
        got = dev_cast(sh, stream, d)
        assert_rays({k: v[valid] for k, v in got.items()}, want, idx[valid],
                    what=f"{c.case.id}: valid rays beside unusable ones")
        assert (got["sphere"][where] == -1).all(), c.case.id
        for name in ("pos", "depth", "steps", "rgba"):
            assert not np.ascontiguousarray(got[name][where]).view(np.uint8).any(), (c.case.id, name)
    assert set(OUT) == set(got)


FAMILIES = {"planes": check_planes, "orders": check_orders, "supersample": check_supersample,
            "views": check_views, "rays": check_rays}


# ---------------------------------------------------------------- GPU: the tests

@pytest.mark.gpu
@chunks
def test_planes(built, chunk):
    for k in chunk:
        check_planes(ctx(k))


@pytest.mark.gpu
@chunks
def test_tile_orders(built, chunk):
    for k in chunk:
        check_orders(ctx(k))


@pytest.mark.gpu
@chunks
def test_supersampling(built, chunk):
    for k in chunk:
        check_supersample(ctx(k))


@pytest.mark.gpu
@chunks
def test_views(built, chunk):
    for k in chunk:
        check_views(ctx(k))


@pytest.mark.gpu
@chunks
def test_ray_batches(built, chunk):
    for k in chunk:
        check_rays(ctx(k))
