"""Every voxel kernel family against the oracle on the degenerate worlds of
tests/voxel_fuzz_cases.py: the planes, the tile orders, in-kernel supersampling, the placing
kernels of render_subset, the view batches, the ray batches and the shadow-ray batches.

Every comparison is on bit patterns, with no tolerance, and no case is skipped.  The colour is
oracle.VoxelOracle's (box-filtered for S > 1), the planes tests/voxel_ref.py's, the ray outputs
tests/voxel_rays_ref.py's; the CPU tests below pin voxel_ref to the oracle's bytes and
voxel_rays_ref to voxel_ref on every pixel's ray of every case.  Where the reference reads outside
a texture both sides read the stand-in texel and the library's status must be SFRT_E_TEXEL
exactly when the oracle's bad_texel_reads rose (a host call then returns it and writes nothing).
Device targets are 0xA5-poisoned with a pitch per target (the ray batches: canary bytes past the
count), and a whole canvas, padding included, must equal the expected one.

The checks are functions of a `Ctx` (a case and the scenes it borrows cameras from), so that
tests/test_parity_sweep.py::test_voxel_family_sweep can run them over any seeds.
"""
import functools

import numpy as np
import pytest

import voxel_fuzz_cases as fuzz
import voxel_rays_ref as vrr
import voxel_ref
import voxel_scenes as vs
import voxel_views_cases as vv
from conftest import host_threads, poisoned

F = np.float32
POISON = 0xA5
TEXEL = -7  # SFRT_E_TEXEL
PLANES = voxel_ref.PLANES
DTYPES = {"depth": np.float32, "cell": np.int32, "face": np.int32, "steps": np.int32}
PADS = {"colour": 16, "depth": 4, "cell": 8, "face": 20, "steps": 12}  # every target its own pitch
CUT = 5  # the row two bands are cut at: no edge of the 8-row tiles
SUBSETS = [(3, 8, 2, 4), (1, 3, 0, 1), (0, 1, 5, 7)]  # (ystart, yadd, xstart, xadd)
MAX_SHADOW_DIST = F(4096.0)  # SFRT_VOXEL_MAX_SHADOW_DIST
RAYS = 16 * 64 + 37
FAR = [1.5e9, fuzz.INT_LIMIT, 2147483648.0, 3e9, -1.5e9, 4294967296.0]  # own_origin_rays
CHUNK = 8
CHUNKS = [range(a, min(a + CHUNK, 48)) for a in range(0, 48, CHUNK)]
chunks = pytest.mark.parametrize("chunk", CHUNKS, ids=[f"cases{c.start}-{c.stop - 1}" for c in CHUNKS])


class Ctx:
    """A case, the scenes whose cameras it borrows, and its references, each computed once."""

    def __init__(self, case, index, others):
        self.case, self.index, self.others = case, index, list(others)
        self.sc, self.w, self.h = case.scene, case.width, case.height
        self.cam = fuzz.camera_of(self.sc)
        self.cams = [self.cam] + fuzz.borrowed_cameras(self.others)
        self._memo = {}

    def memo(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def scene(self, cam=None, dynamics=False):
        return self.sc if cam is None else vv.with_camera(self.sc, cam, dynamics)

    def frame(self, s=1, cam=None, dynamics=False):
        """((h, w, 4) colour of the oracle, box-filtered for s > 1; whether the reference read
        outside a texture).  Shared, read-only."""
        return self.memo(("frame", s, cam, dynamics),
                         lambda: vv.oracle_render(self.scene(cam, dynamics), self.w, self.h, s))

    def planes(self, s=1, cam=None, dynamics=False):
        """voxel_ref's planes (s > 1: of each output pixel's first sample)."""
        def make():
            ref = fuzz.reference(self.scene(cam, dynamics), s * self.w, s * self.h, shade=False)
            ref = voxel_ref.first_sample(ref, s)
            for a in ref.values():
                a.setflags(write=False)
            return ref
        return self.memo(("planes", s, cam, dynamics), make)

    def subset(self, sub, s=1):
        """(the poisoned (h, w, 4) canvas after the oracle's update_image(*sub), whether the
        reference read outside a texture for the addressed pixels); s > 1: the addressed pixels
        of the filtered frame, the status that of their samples."""
        import oracle

        def make():
            tex, dyn = fuzz.assets()
            ystart, yadd, xstart, xadd = sub
            canvas = np.full((self.h, self.w, 4), POISON, dtype=np.uint8)
            o = oracle.VoxelOracle(self.sc, s * self.w, s * self.h, tex, dyn, vs.COLORS)
            before = oracle.VoxelOracle.bad_texel_reads()
            if s == 1:
                o.update_image(canvas.reshape(-1), *sub)
            else:
                scratch = np.zeros(s * s * self.w * self.h * 4, dtype=np.uint8)
                for a in range(s):
                    for b in range(s):
                        o.update_image(scratch, s * ystart + a, s * yadd, s * xstart + b, s * xadd)
                m = _addressed(sub, self.w, self.h)
                canvas[m] = self.frame(s)[0][m]
            ub = oracle.VoxelOracle.bad_texel_reads() > before
            canvas.setflags(write=False)
            return canvas, ub
        return self.memo(("subset", sub, s), make)


def _addressed(sub, w, h):
    ystart, yadd, xstart, xadd = sub
    m = np.zeros((h, w), dtype=bool)
    m[ystart::yadd, xstart::xadd] = True
    return m


@functools.lru_cache(maxsize=None)
def ctx(index):
    """The Ctx of case `index` of the fixed list."""
    return Ctx(fuzz.cases()[index], index, fuzz.other_scenes(index))


# ---------------------------------------------------------------- CPU: the list and the restatements

def test_the_list_meets_its_conditions(built):
    cs = fuzz.cases()
    assert 40 <= len(cs) <= 48 and len({c.id for c in cs}) == len(cs)
    assert cs is fuzz.cases()  # fixed
    for k, c in enumerate(cs):
        assert (c.width, c.height) == fuzz.SIZES[k % len(fuzz.SIZES)] and c.tile_order == k % 2
        assert c.tags == fuzz.tags_of(c.scene, c.width, c.height) | {c.id.split("-")[0]}
    kinds = {kind: [c for c in cs if kind in c.tags] for kind in ("random", "default", "adversarial")}
    assert len(kinds["random"]) >= 16 and len(kinds["adversarial"]) >= 16 and len(kinds["default"]) >= 2
    assert [int(c.id.split("-")[1]) for c in kinds["random"]] == fuzz.RANDOM_SEEDS
    assert [int(c.id.split("-")[1]) for c in kinds["default"]] == fuzz.DEFAULT_SEEDS
    assert [int(c.id.split("-")[1]) for c in kinds["adversarial"]] == fuzz.ADVERSARIAL_SEEDS
    assert min(fuzz.RANDOM_SEEDS + fuzz.DEFAULT_SEEDS) >= 20000 and min(fuzz.ADVERSARIAL_SEEDS) >= 50000
    assert all(s % 4 == 1 for s in fuzz.DEFAULT_SEEDS) and all(s % 4 != 1 for s in fuzz.RANDOM_SEEDS)
    assert {k: cs[k].id for k in fuzz.CORNERS} == {k: f"corner-{v}" for k, v in fuzz.CORNERS.items()}
    for tag in fuzz.ADVERSARIAL_CLASSES:
        assert sum(tag in c.tags for c in kinds["adversarial"]) >= 3, tag
    for tag in fuzz.ADVERSARIAL_CLASSES + fuzz.OTHER_TAGS:
        assert sum(tag in c.tags for c in cs) >= 2, tag
    assert sum("texel_outside" in c.tags for c in cs) <= 6
    # both far cameras, and a batch that mixes the fast and the slow DDA: a case whose own camera
    # is within the bound borrows one beyond it
    assert {float(F(c.scene.cam_pos[0])) for c in cs if "cam_far" in c.tags} >= {1.5e9, fuzz.INT_LIMIT}
    mixed = 0
    for k, c in enumerate(cs):
        own = vv.dda_qlim(c.scene, c.width, c.height)
        lent = [vv.dda_qlim(ctx(k).scene(cam), c.width, c.height) for cam in ctx(k).cams[1:]]
        mixed += own > 0 and min(lent) == 0.0
    assert mixed >= 2
    # corner worlds: what their names say, in numbers
    by_id = {c.id: c for c in cs}
    eq = by_id["corner-equal_billboards"].scene
    dist = vv.distances(eq.dyn, eq.cam_pos)
    assert (dist == F(1)).sum() == 4 and len(np.unique(dist)) <= dist.size - 4
    assert F(by_id["corner-view_0"].scene.view_distance) == 0
    assert vv.distances(by_id["corner-billboard_at_cam"].scene.dyn,
                        by_id["corner-billboard_at_cam"].scene.cam_pos).min() == 0
    for name in ("corner-far_1.5e9", "corner-far_int_limit"):
        sc = by_id[name].scene
        assert sc.dyn.shape[0] >= 3 and (sc.lights["shadows"] == 1).any()


def test_the_frames_hold_what_the_checks_are_for(built):
    """Over the list: every face value the renderer defines, step counts from 1 (and 0, at the
    view distance 0) up to maxiter, billboards drawn in the far frames and in the frame of equal
    distances; `texel_outside` is what the oracle's counter says."""
    faces, lo, full = set(), 1 << 30, False
    for k, c in enumerate(fuzz.cases()):
        ref = fuzz.reference(c.scene, c.width, c.height, shade=False)
        faces |= set(np.unique(ref["face"]).tolist())
        if ref["maxiter"] > 0:
            lo = min(lo, int(ref["steps"].min()))
        full |= ref["maxiter"] > 0 and int(ref["steps"].max()) == ref["maxiter"]
        if "cam_far" in c.tags or c.id == "corner-equal_billboards":
            assert (ref["face"] == 4).any(), c.id
        assert ctx(k).frame()[1] == ("texel_outside" in c.tags), c.id
    assert faces == {-3, -2, -1, 0, 1, 2, 3, 4}, faces
    assert lo == 1 and full


@chunks
def test_restatements_are_pinned_on_every_case(built, chunk):
    """tests/voxel_ref.py equals VoxelOracle.render byte for byte, and tests/voxel_rays_ref.py
    equals voxel_ref in every output on every pixel's ray, on every case (tests/test_voxel_ref.py
    and tests/test_voxel_cast_rays.py pin them on their named scenes)."""
    for k in chunk:
        c = ctx(k)
        ref = fuzz.reference(c.sc, c.w, c.h)
        rgba, ub = c.frame()
        assert np.array_equal(ref["rgba"], rgba), c.case.id
        assert (ref["bad_texels"] > 0) == ub, c.case.id
        got = frame_rays(c)[2]
        n = c.w * c.h
        for name in PLANES:
            assert np.array_equal(np.ascontiguousarray(got[name]).view(np.uint32),
                                  np.ascontiguousarray(ref[name].reshape(n)).view(np.uint32)), (c.case.id, name)
        assert np.array_equal(got["rgba"], ref["rgba"].reshape(n, 4)), c.case.id
        assert got["bad_texels"] == ref["bad_texels"] and got["maxiter"] == ref["maxiter"]


# ---------------------------------------------------------------- the ray sets

def frame_rays(c):
    """(dirs, yscales, voxel_rays_ref's answer) of the frame's own rays, row-major."""
    def make():
        tex, dyn = fuzz.assets()
        d, ys = vrr.frame_ray_set(c.sc, c.w, c.h)
        ref = vrr.raycast(c.sc, d, ys, None, tex, dyn, vs.COLORS)
        for a in (d, ys, *(ref[k] for k in vrr.OUTPUTS)):
            a.setflags(write=False)
        return d, ys, ref
    return c.memo("frame rays", make)


def own_origin_rays(c):
    """RAYS rays with an origin each, and voxel_rays_ref's answer.  Origins in turn: a cell centre,
    on a cell face, on a cell corner, the camera, outside the grid, and -- in waves 3 and 9, in
    every fourth lane but never the first -- a cell centre with FAR's values in x or y, beside
    origins near the grid in the same wave: such a wave must not take the fast DDA, whose plain
    conversion differs from World.cpp's (INT_MIN, so cell 0 of that axis) from 2^31 on.
    Directions axis-parallel (a third), random with one zero component (a sixth) or random; a
    zero component keeps its whole wave off the fast DDA, so waves 3, 5 and 9 have none (wave 5,
    all of whose origins are near the grid, takes it).
    A NaN, an infinite and a -inf component in dir, origin and yscale at fixed indices."""
    def make():
        tex, dyn = fuzz.assets()
        rng = np.random.default_rng(77 + c.index)
        nx, ny, nz = c.sc.blocks.shape
        cell = np.stack([rng.integers(0, nx, RAYS), rng.integers(0, ny, RAYS), rng.integers(0, nz, RAYS)], axis=1)
        kind = np.arange(RAYS) % 5
        o = (cell + 0.5).astype(F)
        face = np.flatnonzero(kind == 1)
        o[face, rng.integers(0, 3, face.size)] -= F(0.5)
        o[kind == 2] = cell[kind == 2].astype(F)
        o[kind == 3] = np.array(c.cam[0], dtype=F)
        out = np.flatnonzero(kind == 4)
        o[out] = (o[out] + rng.choice([-1.0, 1.0], (out.size, 3)) * (np.array([nx, ny, nz]) + 2.5)).astype(F)
        for wave, first in ((3, 1), (9, 2)):  # never the wave's first lane
            lanes = 64 * wave + np.arange(first, 64, 4)
            o[lanes] = (cell[lanes] + 0.5).astype(F)
            o[lanes, np.arange(lanes.size) % 2] = F(FAR)[np.arange(lanes.size) % len(FAR)]
        d = rng.standard_normal((RAYS, 3)).astype(F)
        axis = np.arange(RAYS) % 3 == 0
        d[axis] = np.eye(3, dtype=F)[rng.integers(0, 3, int(axis.sum()))] * rng.choice(F([-1, 1]), int(axis.sum()))[:, None]
        zero = np.flatnonzero(np.arange(RAYS) % 6 == 1)
        d[zero, rng.integers(0, 3, zero.size)] = rng.choice(F([0.0, -0.0]), zero.size)
        for wave in (3, 5, 9):  # directions that let a wave of near origins take the fast DDA
            q = slice(64 * wave, 64 * wave + 64)
            d[q] = (rng.uniform(0.2, 1.0, (64, 3)) * rng.choice([-1.0, 1.0], (64, 3))).astype(F)
        ys = rng.uniform(0.2, 2.5, RAYS).astype(F)
        bad = [5, 64 + 27, 2 * 64 + 40, 5 * 64 + 1, 7 * 64 + 63, 11 * 64 + 9, RAYS - 3]
        d[bad[0], 0], d[bad[1], 2], d[bad[2], 1] = np.nan, np.inf, -np.inf
        o[bad[3], 1], o[bad[4], 0] = np.nan, np.inf
        ys[bad[5]], ys[bad[6]] = np.nan, -np.inf
        ref = vrr.raycast(c.sc, d, ys, o, tex, dyn, vs.COLORS)
        assert not ref["valid"][bad].any() and ref["valid"].sum() == RAYS - len(bad)
        bad = np.array(bad)
        for a in (d, ys, o, bad, *(ref[k] for k in vrr.OUTPUTS)):
            a.setflags(write=False)
        return d, ys, o, bad, ref
    return c.memo("own rays", make)


def shadow_segments(c):
    """Segments from own_origin_rays' origins (the unusable ones replaced by the camera) to the
    world's first four lights in turn (no light: to the camera), the direction normalised as the
    reference passes it; with a zero-length segment, one of exactly SFRT_VOXEL_MAX_SHADOW_DIST,
    and one just over it, which is refused with free = -1.  A segment from 1.5e9 is longer still."""
    def make():
        o = np.array(own_origin_rays(c)[2], copy=True)
        o[~np.isfinite(o).all(axis=1)] = np.array(c.cam[0], dtype=F)
        targets = np.asarray(c.sc.lights["pos"], dtype=F).reshape(-1, 3)[:4]
        if targets.shape[0] == 0:
            targets = np.array([c.cam[0]], dtype=F)
        e = (targets[np.arange(RAYS) % targets.shape[0]] - o).astype(F)
        with np.errstate(all="ignore"):
            ln = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]).astype(F)
            d = (e / ln[:, None]).astype(F)
        still = ~np.isfinite(d).all(axis=1)       # an origin on its light: a zero-length segment
        d[still] = F([0.0, 1.0, 0.0])
        md = ln.copy()
        md[~np.isfinite(md)] = F(1.0)
        zero, exact, over = 6, 64 + 13, 2 * 64 + 50
        md[zero], md[exact], md[over] = F(0.0), MAX_SHADOW_DIST, np.nextafter(MAX_SHADOW_DIST, F(np.inf))
        ref = vrr.shadow_rays(c.sc, o, d, md)
        assert ref["free"][zero] == 1 and ref["steps"][zero] == 0
        assert ref["free"][exact] in (0, 1) and ref["free"][over] == -1
        assert (ref["free"][md > MAX_SHADOW_DIST] == -1).all() and (md > F(1e9)).any()
        for a in (o, d, md, ref["free"], ref["steps"]):
            a.setflags(write=False)
        return o, d, md, ref
    return c.memo("shadow", make)


# ---------------------------------------------------------------- GPU: helpers

def _world(c, s=1, order=None):
    import sfrt
    tex, dyn = fuzz.assets()
    w = sfrt.VoxelWorld(0)
    w.load_assets(tex, dyn, vs.COLORS)
    w.set_scene(c.sc, c.w, c.h)
    w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
    w.set_option(sfrt.SFRT_OPT_TILE_ORDER, c.case.tile_order if order is None else order)
    return w


def _camera(cam, scene):
    import sfrt
    pos, rot, hrot = cam
    c = sfrt.Camera()
    for q in range(3):
        c.pos[q] = pos[q]
    c.rotation, c.hrotation = rot, hrot
    c.fov_h, c.fov_v = float(scene.fov_h), float(scene.fov_v)
    return c


def _stream():
    import torch
    return torch.cuda.Stream()


def _status(world, stream, ub, what):
    """check(stream) raises SFRT_E_TEXEL exactly when the reference read outside a texture."""
    import sfrt
    try:
        world.check(stream.cuda_stream)
        got = 0
    except sfrt.SfrtError as e:
        got = e.code
    assert got == (TEXEL if ub else 0), (what, got, ub)


def _same_canvas(got, content, mask, what):
    """got (h, pitch) uint8 equals `content` ((h, w) 4-byte elements or (h, w, 4) bytes) where
    mask is set (None: everywhere) and POISON everywhere else, the padding past 4w included."""
    h, w = content.shape[:2]
    want = np.full(got.shape, POISON, dtype=np.uint8)
    inner = want[:, :4 * w].reshape(h, w, 4)
    src = np.ascontiguousarray(content).view(np.uint8).reshape(h, w, 4)
    if mask is None:
        inner[:] = src
    else:
        inner[mask] = src[mask]
    want[:, :4 * w] = inner.reshape(h, 4 * w)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} bytes differ, first (row, byte) {tuple(bad[0])}"


class Targets:
    """Poisoned whole-frame device targets: the colour and each plane, every one its own pitch."""

    def __init__(self, w, h):
        self.pitch = {k: 4 * w + PADS[k] for k in ("colour",) + PLANES}
        self.buf = {k: poisoned((h, p), POISON) for k, p in self.pitch.items()}

    def args(self, row=0):
        return {p: (self.buf[p].data_ptr() + row * self.pitch[p], self.pitch[p]) for p in PLANES}

    def colour_ptr(self, row=0):
        return self.buf["colour"].data_ptr() + row * self.pitch["colour"]

    def check(self, colour, planes, what, mask=None):
        want = {"colour": colour, **{p: planes[p] for p in PLANES}}
        for k, b in self.buf.items():
            _same_canvas(b.cpu().numpy(), want[k], mask, f"{what}: {k}")


def _host_aux(world, c, ub, colour, want, what):
    """update_image_aux into poisoned host arrays: the references' bytes, or SFRT_E_TEXEL and
    nothing written."""
    import sfrt
    rgba = np.full((c.h, c.w, 4), POISON, dtype=np.uint8)
    planes = {p: np.full((c.h, c.w, 4), POISON, dtype=np.uint8).view(DTYPES[p]).reshape(c.h, c.w)
              for p in PLANES}
    try:
        world.update_image_aux(rgba, *(planes[p] for p in PLANES))
        code = 0
    except sfrt.SfrtError as e:
        code = e.code
    assert code == (TEXEL if ub else 0), (what, code, ub)
    if ub:
        assert (rgba == POISON).all() and all((planes[p].view(np.uint8) == POISON).all() for p in PLANES), what
        return
    _same_canvas(rgba.reshape(c.h, 4 * c.w), colour, None, f"{what}: colour")
    for p in PLANES:
        _same_canvas(planes[p].view(np.uint8).reshape(c.h, 4 * c.w), want[p], None, f"{what}: {p}")


def _host_plain(world, c, ub, colour, what):
    import sfrt
    rgba = np.full(c.w * c.h * 4, POISON, dtype=np.uint8)
    try:
        world.update_image(rgba)
        code = 0
    except sfrt.SfrtError as e:
        code = e.code
    assert code == (TEXEL if ub else 0), (what, code, ub)
    if ub:
        assert (rgba == POISON).all(), what
    else:
        _same_canvas(rgba.reshape(c.h, 4 * c.w), colour, None, what)


# ---------------------------------------------------------------- the family checks

def check_planes(c, s=1):
    """render_band_aux (the whole frame, and two bands cut at row CUT) and update_image_aux: the
    colour is the oracle's frame, the planes voxel_ref's (s > 1: the first sample's)."""
    what = f"{c.case.id} planes S={s}"
    (colour, ub), want = c.frame(s), c.planes(s)
    stream = _stream()
    with _world(c, s) as w:
        whole, banded = Targets(c.w, c.h), Targets(c.w, c.h)
        w.render_band_aux(whole.colour_ptr(), whole.pitch["colour"], 0, c.h, stream.cuda_stream,
                          **whole.args())
        _status(w, stream, ub, what + " whole frame")
        for row0, rows in ((0, CUT), (CUT, c.h - CUT)):
            w.render_band_aux(banded.colour_ptr(row0), banded.pitch["colour"], row0, rows,
                              stream.cuda_stream, **banded.args(row0))
        _status(w, stream, ub, what + " two bands")
        whole.check(colour, want, what + " whole frame")
        banded.check(colour, want, what + " two bands")
        _host_aux(w, c, ub, colour, want, what + " update_image_aux")


def check_orders(c):
    """Three render_band frames (the order is in use from the third) under SFRT_OPT_TILE_ORDER 0
    and 1, and update_image: every frame is the oracle's."""
    colour, ub = c.frame()
    stream = _stream()
    pitch = 4 * c.w + 16
    for order in (c.case.tile_order, 1 - c.case.tile_order):
        with _world(c, 1, order) as w:
            for k in range(3):
                what = f"{c.case.id} order {order} frame {k + 1}"
                buf = poisoned((c.h, pitch), POISON)
                w.render_band(buf.data_ptr(), pitch, 0, c.h, stream.cuda_stream)
                _status(w, stream, ub, what)
                _same_canvas(buf.cpu().numpy(), colour, None, what)
            _host_plain(w, c, ub, colour, f"{c.case.id} order {order} update_image")


def check_supersample(c):
    """S = 2 and 4 through render_band and update_image against the box-filtered oracle frame,
    and with planes: those of the group's first sample."""
    for s in (2, 4):
        what = f"{c.case.id} S={s}"
        colour, ub = c.frame(s)
        stream = _stream()
        with _world(c, s) as w:
            pitch = 4 * c.w + 16
            buf = poisoned((c.h, pitch), POISON)
            w.render_band(buf.data_ptr(), pitch, 0, c.h, stream.cuda_stream)
            _status(w, stream, ub, what + " render_band")
            _same_canvas(buf.cpu().numpy(), colour, None, what + " render_band")
            _host_plain(w, c, ub, colour, what + " update_image")
        check_planes(c, s)


def check_subsets(c):
    """render_subset and render_subset_aux with SUBSETS at S = 1 and 2 into poisoned whole-frame
    targets: the addressed pixels are the oracle's update_image bytes and voxel_ref's planes,
    every other byte is the poison."""
    stream = _stream()
    for s in (1, 2):
        want = c.planes(s)
        with _world(c, s) as w:
            for sub in SUBSETS:
                what = f"{c.case.id} subset {sub} S={s}"
                mask = _addressed(sub, c.w, c.h)
                colour, ub = c.subset(sub, s)
                pitch = 4 * c.w + 32
                plain = poisoned((c.h, pitch), POISON)
                t = Targets(c.w, c.h)
                w.render_subset(plain.data_ptr(), pitch, *sub, stream=stream.cuda_stream)
                _status(w, stream, ub, what + " render_subset")
                w.render_subset_aux(t.colour_ptr(), t.pitch["colour"], *sub, stream=stream.cuda_stream,
                                    **t.args())
                _status(w, stream, ub, what + " render_subset_aux")
                _same_canvas(plain.cpu().numpy(), colour, None, what + " render_subset")
                t.check(colour, want, what + " render_subset_aux", mask)
                assert (colour[~mask] == POISON).all()


def check_views(c):
    """The case's camera and four borrowed ones as one render_views_aux batch, without and with
    SFRT_VOXEL_VIEWS_DYNAMICS: each view is the references' of that camera on the stale list, or
    on the list sorted for the view.  Afterwards the world's own band is unchanged, and its
    billboard cells still index the world's own list."""
    stream = _stream()
    with _world(c) as w:
        for dynamics in (False, True):
            views = [Targets(c.w, c.h) for _ in c.cams]
            pitch = views[0].pitch["colour"]
            w.render_views_aux([(_camera(cam, c.sc), t.colour_ptr()) for cam, t in zip(c.cams, views)],
                               [t.args() for t in views], pitch, dynamics=dynamics,
                               stream=stream.cuda_stream)
            frames = [c.frame(1, cam, dynamics) for cam in c.cams]
            _status(w, stream, any(ub for _, ub in frames), f"{c.case.id} views dynamics={dynamics}")
            for k, (cam, t) in enumerate(zip(c.cams, views)):
                t.check(frames[k][0], c.planes(1, cam, dynamics),
                        f"{c.case.id} view {k} dynamics={dynamics}")
        own = Targets(c.w, c.h)
        w.render_band_aux(own.colour_ptr(), own.pitch["colour"], 0, c.h, stream.cuda_stream, **own.args())
        _status(w, stream, c.frame()[1], f"{c.case.id}: the world's own band after the batches")
        own.check(c.frame()[0], c.planes(), f"{c.case.id}: the world's own band after the batches")


def check_rays(c):
    """cast_rays_device with all six outputs: the frame's own rays row-major and shuffled, and
    own_origin_rays, against voxel_rays_ref; unusable rays are answered face 0, cell -1 and zeros.
    cast_shadow_rays_device on shadow_segments.  dev_cast asserts the canaries past the count."""
    from test_voxel_cast_rays import OUT, _assert_equal, dev_cast, dev_shadow
    stream = _stream()
    with _world(c) as w:
        d, ys, ref = frame_rays(c)
        n = len(d) - (len(d) % 64 == 0)  # a tail wave
        want = {k: ref[k][:n] for k in OUT}
        ub = ref["bad_texels"] > 0
        # the status is the whole frame's; a set cut by its last ray may have lost the one read
        allowed = (TEXEL if ub else 0,) if n == len(d) else ((0, TEXEL) if ub else (0,))
        got, st = dev_cast(w, stream, d[:n], ys[:n])
        assert st in allowed, (c.case.id, st)
        _assert_equal(got, want, f"{c.case.id}: pixel rays, row-major")
        shuffle = np.random.default_rng(7).permutation(n)
        got, st = dev_cast(w, stream, d[:n][shuffle], ys[:n][shuffle])
        assert st in allowed, (c.case.id, st)
        _assert_equal(got, {k: v[shuffle] for k, v in want.items()}, f"{c.case.id}: pixel rays, shuffled")
        rd, rys, ro, bad, rref = own_origin_rays(c)
        got, st = dev_cast(w, stream, rd, rys, ro)
        assert st == (TEXEL if rref["bad_texels"] > 0 else 0), (c.case.id, st)
        _assert_equal(got, {k: rref[k] for k in OUT}, f"{c.case.id}: rays with their own origins")
        assert (got["face"][bad] == 0).all() and (got["cell"][bad] == -1).all(), c.case.id
        for name in ("pos", "depth", "steps", "rgba"):
            assert not np.ascontiguousarray(got[name][bad]).view(np.uint8).any(), (c.case.id, name)
        so, sd, smd, sref = shadow_segments(c)
        got, st = dev_shadow(w, stream, so, sd, smd)
        assert st == 0, (c.case.id, st)
        _assert_equal(got, sref, f"{c.case.id}: shadow segments", ("free", "steps"))


FAMILIES = {"planes": check_planes, "orders": check_orders, "supersample": check_supersample,
            "subsets": check_subsets, "views": check_views, "rays": check_rays}


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
def test_subsets_in_place(built, chunk):
    for k in chunk:
        check_subsets(ctx(k))


@pytest.mark.gpu
@chunks
def test_views(built, chunk):
    for k in chunk:
        check_views(ctx(k))


@pytest.mark.gpu
@chunks
def test_ray_and_shadow_batches(built, chunk):
    for k in chunk:
        check_rays(ctx(k))
