"""Every sphere kernel family against the oracle on the degenerate scenes of
tests/sphere_fuzz_cases.py: the planes, in-kernel supersampling, the placing kernels of
render_subset, the view batches, the ray batches and the four cache layers.

Every comparison is on bit patterns, with no tolerance, and no case is skipped.  The references
are the oracle's own (Oracle.render, Oracle.update_image, one Oracle.dump per pixel with
test_aux_planes' `_depth_of`, the box filter of test_supersample) and, for rays that are no pixel
of a frame, tests/raycast_ref.py, which the CPU test below pins to the oracle on every pixel of
every case.  Device targets are 0xA5-poisoned with padded pitches (the ray batches: canary
elements past the count), and a whole target, padding included, must equal the expected one.

The checks are functions of a `Ctx` (a case, its textures and the scenes it borrows cameras from),
so that tests/test_parity_sweep.py::test_sphere_family_sweep can run them over any seeds.
"""
import functools

import numpy as np
import pytest

import raycast_ref
import scenes
import sphere_fuzz_cases as fuzz
from conftest import host_threads, poisoned
from test_aux_planes import DTYPES, PADS, PLANES, _depth_of

F = np.float32
POISON = 0xA5
CHUNK = 8
CHUNKS = [range(a, min(a + CHUNK, 48)) for a in range(0, 48, CHUNK)]
chunks = pytest.mark.parametrize("chunk", CHUNKS, ids=[f"cases{c.start}-{c.stop - 1}" for c in CHUNKS])
SUBSETS = [(3, 8, 2, 4), (1, 3, 0, 1), (0, 1, 5, 7)]  # (ystart, yadd, xstart, xadd)
# slot 0 of the cache test: one texel, one column, the two sides of 256, the widest row
CACHE_SIZES = ["sized1x1", "sized1x7", "sized255x257", "row65535"]
RAYS = 2048


@functools.lru_cache(maxsize=None)
def _all_textures():
    out = []
    for rgba, tw, th in scenes.load_all_textures():
        rgba = np.array(rgba, dtype=np.uint8).ravel()
        rgba.setflags(write=False)
        out.append((rgba, tw, th))
    return tuple(out)


def _box(big, w, h, s):
    """test_supersample.reference's filter: (h, w, 4) from the oracle's s*w x s*h frame."""
    if s == 1:
        return big.reshape(h, w, 4).copy()
    sums = big.reshape(h, s, w, s, 4).astype(np.uint32).sum(axis=(1, 3))
    return ((sums + s * s // 2) >> {2: 2, 4: 4}[s]).astype(np.uint8)


class Ctx:
    """A case with its textures and slots, the scenes whose cameras it borrows, and its oracle
    references, each computed once."""

    def __init__(self, case, index, others):
        self.case, self.index, self.others = case, index, list(others)
        self.sc, self.w, self.h = case.scene, case.width, case.height
        self.spheres = np.ascontiguousarray(np.asarray(self.sc.spheres, dtype=F))
        self.textured = fuzz.textured(index)
        self.textures = _all_textures() if self.textured else _all_textures()[:1]
        self.slots = fuzz.slots_of(case, index)
        self.cam = fuzz.camera_of(self.sc)
        self.cams = [self.cam] + fuzz.borrowed_cameras(self.sc, self.others)
        self._memo = {}

    def memo(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def oracle(self, s=1, cam=None, spheres=None, slots=None, tex0=None):
        import oracle
        cam = self.cam if cam is None else cam
        tex = (self.textures[0] if tex0 is None else tex0)
        extra = {}
        if self.textured:
            extra = {"sphere_tex": self.slots if slots is None else slots,
                     "textures": {k: self.textures[k] for k in range(1, len(self.textures))}}
        return oracle.Oracle(s * self.w, s * self.h, self.spheres if spheres is None else spheres,
                             *tex, *cam, **extra)

    def sorted_for(self, cam):
        """(spheres, slots) as update_spheres orders them for `cam`: oracle.sort_spheres, and the
        slots moved with their spheres by the same stable order."""
        import oracle
        def make():
            sp = oracle.sort_spheres(self.spheres, cam[0])
            e = self.spheres[:, :3] - np.asarray(cam[0], dtype=F)
            key = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) + self.spheres[:, 3]
            assert key.dtype == F
            perm = np.argsort(key, kind="stable")
            assert np.array_equal(self.spheres[perm].view(np.uint32), sp.view(np.uint32))
            return sp, self.slots[perm]
        return self.memo(("sorted", cam), make)

    def _view(self, cam, sort):
        return self.sorted_for(cam) if sort else (self.spheres, self.slots)

    def frame(self, s=1, cam=None, sort=False, spheres=None, tex0=None, tex_name=None):
        """(h, w, 4): the oracle's frame (box-filtered for s > 1); shared, read-only."""
        cam = self.cam if cam is None else cam

        def make():
            sp, sl = self._view(cam, sort)
            if spheres is not None:
                sp = spheres
            out = _box(self.oracle(s, cam, sp, sl, tex0).render(host_threads()), self.w, self.h, s)
            out.setflags(write=False)
            return out
        key = ("frame", s, cam, sort, None if spheres is None else spheres.tobytes(), tex_name)
        return self.memo(key, make)

    def planes(self, s=1, cam=None, sort=False):
        """test_aux_planes.planes_reference's method: one Oracle.dump per output pixel's first
        sample, the depth restated by _depth_of and pinned to the oracle's brightness."""
        cam = self.cam if cam is None else cam

        def make():
            o = self.oracle(s, cam, *self._view(cam, sort))
            return _dump_planes(o, self.w, self.h, s, cam[0])
        return self.memo(("planes", s, cam, sort), make)

    def subset_colour(self, sub, s=1):
        """The poisoned (h, w, 4) canvas after the oracle's update_image(*sub) (s > 1: the
        addressed pixels of the filtered frame)."""
        def make():
            canvas = np.full((self.h, self.w, 4), POISON, dtype=np.uint8)
            if s == 1:
                self.oracle().update_image(canvas.reshape(-1), *sub)
            else:
                m = _addressed(sub, self.w, self.h)
                canvas[m] = self.frame(s)[m]
            canvas.setflags(write=False)
            return canvas
        return self.memo(("subset", sub, s), make)


def _dump_planes(o, w, h, s, cam_pos):
    pos = np.zeros((h, w, 3), dtype=F)
    sphere = np.zeros((h, w), dtype=np.int32)
    steps = np.zeros((h, w), dtype=np.int32)
    bright = np.zeros((h, w), dtype=F)
    rgba = np.zeros((h, w, 4), dtype=np.uint8)
    for j in range(h):
        for i in range(w):
            d = o.dump(s * i, s * j)
            pos[j, i], sphere[j, i], steps[j, i], bright[j, i] = d["pos"], d["draw"], d["iters"], d["brightness"]
            rgba[j, i] = d["rgba"]
    with np.errstate(all="ignore"):
        depth = _depth_of(pos, np.asarray(cam_pos, dtype=F))
        assert depth.dtype == F
        pinned = F(3.0) / np.where(depth < F(3.0), F(3.0), depth)  # :375's ternary
    # the numpy restatement is the oracle's own value: its brightness, bit for bit (a NaN is a NaN)
    same = (pinned.view(np.uint32) == bright.view(np.uint32)) | (np.isnan(pinned) & np.isnan(bright))
    assert same.all()
    out = {"depth": depth, "sphere": sphere, "steps": steps, "pos": pos, "first_rgba": rgba}
    for a in out.values():
        a.setflags(write=False)
    return out


def _addressed(sub, w, h):
    ystart, yadd, xstart, xadd = sub
    m = np.zeros((h, w), dtype=bool)
    m[ystart::yadd, xstart::xadd] = True
    return m


@functools.lru_cache(maxsize=None)
def ctx(index):
    """The Ctx of case `index` of the fixed list."""
    return Ctx(fuzz.cases()[index], index, fuzz.other_scenes(index))


# ---------------------------------------------------------------- CPU: the list and the restatement

def test_the_list_meets_its_conditions(built, floor):
    cs = fuzz.cases()
    assert 44 <= len(cs) <= 52 and len({c.id for c in cs}) == len(cs)
    assert cs is fuzz.cases()  # fixed
    for k, c in enumerate(cs):
        assert (c.width, c.height) == fuzz.SIZES[k % len(fuzz.SIZES)] and c.rays_per_lane == k % 5
        assert c.tags == fuzz.tags_of(c.scene) | {c.id.split("-")[0]}
    assert {(c.width, c.height) for c in cs} == set(fuzz.SIZES)
    assert sum(fuzz.textured(k) for k in range(len(cs))) >= len(cs) // 7
    rand = [c for c in cs if "random" in c.tags]
    adv = [c for c in cs if "adversarial" in c.tags]
    swarm = [c for c in cs if "swarm" in c.tags]
    assert len(rand) >= 20 and len(adv) >= 20 and len(swarm) == 4
    assert [int(c.scene.name[4:]) for c in rand] == fuzz.RANDOM_SEEDS and min(fuzz.RANDOM_SEEDS) >= 20000
    assert [int(c.scene.name[3:]) for c in adv] == fuzz.ADVERSARIAL_SEEDS and min(fuzz.ADVERSARIAL_SEEDS) >= 50000
    for n in fuzz.FUZZ_COUNTS:  # every sphere count of _fuzz_scene's list
        assert any(f"n{n}" in c.tags for c in rand + adv), n
    for mode in fuzz.CAMERA_MODES:
        assert sum(mode in c.tags for c in cs) >= 3, mode
        assert all(sum(m in c.tags for m in fuzz.CAMERA_MODES) == 1 for c in cs)
    for cls in fuzz.ADVERSARIAL_CLASSES:
        assert sum(cls in c.tags for c in adv) >= 3, cls
    assert sorted(c.scene.spheres.shape[0] for c in swarm) == sorted(fuzz.SWARM_COUNTS)
    assert max(fuzz.SWARM_COUNTS) == fuzz.MAX_SPHERES
    for c in swarm:  # the camera strictly inside more than 64 spheres, in float64
        assert fuzz.spheres_holding_camera(c.scene) > 64, c.id
    both = [c for c in swarm if "duplicate" in c.tags and
            (c.scene.spheres[:, :3] == np.round(c.scene.spheres[:, :3])).all()]
    assert len(both) == 2
    # the oracle alone gives every case a defined answer: no march reaches the kernels' guard
    for k, c in enumerate(cs):
        lengths = fuzz.march_lengths(c, fuzz.other_scenes(k), floor, host_threads())
        assert {"own-s1", "own-s2", "own-s4"} <= set(lengths)
        assert max(lengths.values()) < fuzz.MARCH_GUARD, (c.id, lengths)


@chunks
def test_restatement_is_pinned_to_the_oracle_on_every_case(built, chunk):
    """tests/raycast_ref.py on the frame's own rays: position, draw, iterations and rgba equal
    Oracle.dump bit for bit on every pixel of every case (as tests/test_cast_rays.py pins it on
    three named scenes)."""
    for k in chunk:
        c = ctx(k)
        want = c.planes()
        dirs = raycast_ref.pixel_dirs(c.sc, c.w, c.h).reshape(-1, 3)
        ref = raycast_ref.raycast(c.spheres, c.cam[0], dirs, textures=dict(enumerate(c.textures)),
                                  sphere_tex=c.slots)
        assert ref["valid"].all() and ref["inside"].all(), c.case.id
        for name, a in (("pos", want["pos"]), ("sphere", want["sphere"]), ("steps", want["steps"]),
                        ("depth", want["depth"]), ("rgba", want["first_rgba"])):
            g = np.ascontiguousarray(ref[name]).reshape(-1).view(np.uint8)
            w = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
            assert np.array_equal(g, w), f"{c.case.id}: {name}"
        assert np.array_equal(want["first_rgba"], c.frame()), c.case.id  # dump and render agree


# ---------------------------------------------------------------- GPU: helpers

def _world(c, s=1):
    import sfrt
    w = sfrt.World(0)
    for slot, (rgba, tw, th) in enumerate(c.textures):
        w.load_texture(rgba, tw, th, slot=slot)
    w.set_scene(c.sc, c.w, c.h)
    w.set_sphere_textures(c.slots)
    w.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, c.case.rays_per_lane)
    w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
    return w


def _camera(cam):
    import sfrt
    c = sfrt.Camera()
    for q in range(3):
        c.pos[q] = cam[0][q]
    c.rotation, c.hrotation, c.fov_h, c.fov_v = cam[1:]
    return c


def _stream():
    import torch
    return torch.cuda.Stream()


class Targets:
    """Poisoned whole-frame device targets: the colour and each plane, every one its own pitch."""

    def __init__(self, w, h, planes=PLANES):
        self.w, self.h, self.planes = w, h, tuple(planes)
        self.pitch = {k: 4 * w + PADS[k] for k in ("colour",) + self.planes}
        self.buf = {k: poisoned((h, p), POISON) for k, p in self.pitch.items()}

    def args(self, row=0):
        return {p: (self.buf[p].data_ptr() + row * self.pitch[p], self.pitch[p]) for p in self.planes}

    def colour_ptr(self, row=0):
        return self.buf["colour"].data_ptr() + row * self.pitch["colour"]

    def check(self, colour, planes, what, mask=None):
        """Every target, padding included, is the expected one: `colour` (h, w, 4) and `planes`
        where `mask` (h, w) is set (None: everywhere), poison elsewhere."""
        want = {"colour": colour, **{p: planes[p] for p in self.planes}}
        for k, b in self.buf.items():
            _same_canvas(b.cpu().numpy(), want[k], mask, f"{what}: {k}")


def _as_bytes(a, h, w):
    return np.ascontiguousarray(a).view(np.uint8).reshape(h, w, 4)


def _same_canvas(got, content, mask, what):
    """got (h, pitch) uint8 equals `content` ((h, w) 4-byte elements or (h, w, 4) bytes) where
    mask is set and POISON everywhere else, the padding past 4w included."""
    h, w = content.shape[:2]
    want = np.full(got.shape, POISON, dtype=np.uint8)
    inner = want[:, :4 * w].reshape(h, w, 4)
    src = _as_bytes(content, h, w)
    if mask is None:
        inner[:] = src
    else:
        inner[mask] = src[mask]
    want[:, :4 * w] = inner.reshape(h, 4 * w)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} bytes differ, first (row, byte) {tuple(bad[0])}"


def _host_aux(world, c, sub=(0, 1, 0, 1)):
    rgba = np.full((c.h, c.w, 4), POISON, dtype=np.uint8)
    planes = {p: np.full((c.h, c.w, 4), POISON, dtype=np.uint8).view(DTYPES[p]).reshape(c.h, c.w)
              for p in PLANES}
    world.update_image_aux(rgba, *(planes[p] for p in PLANES), *sub)
    return rgba, planes


def _check_host(rgba, planes, colour, want, what, mask=None):
    h, w = rgba.shape[:2]
    _same_canvas(rgba.reshape(h, 4 * w), colour, mask, f"{what}: colour")
    for p in PLANES:
        _same_canvas(planes[p].view(np.uint8).reshape(h, 4 * w), want[p], mask, f"{what}: {p}")


# ---------------------------------------------------------------- the family checks

def check_planes(c, s=1):
    """render_band_aux (the whole frame, and two bands cut at row 5) and update_image_aux: the
    colour is the oracle's frame, the planes its dumps (s > 1: the first sample's)."""
    what = f"{c.case.id} planes S={s}"
    colour, want = c.frame(s), c.planes(s)
    stream = _stream()
    with _world(c, s) as w:
        whole, banded = Targets(c.w, c.h), Targets(c.w, c.h)
        w.render_band_aux(whole.colour_ptr(), whole.pitch["colour"], 0, c.h, stream.cuda_stream,
                          **whole.args())
        for row0, rows in ((0, 5), (5, c.h - 5)):
            w.render_band_aux(banded.colour_ptr(row0), banded.pitch["colour"], row0, rows,
                              stream.cuda_stream, **banded.args(row0))
        w.check(stream.cuda_stream)
        whole.check(colour, want, what + " whole frame")
        banded.check(colour, want, what + " two bands")
        rgba, planes = _host_aux(w, c)
        _check_host(rgba, planes, colour, want, what + " update_image_aux")


def check_supersample(c):
    """S = 2 and 4 through render_band and update_image against the box-filtered oracle frame,
    and with planes: those of the group's first sample."""
    for s in (2, 4):
        what = f"{c.case.id} S={s}"
        colour = c.frame(s)
        stream = _stream()
        with _world(c, s) as w:
            pitch = 4 * c.w + 16
            buf = poisoned((c.h, pitch), POISON)
            w.render_band(buf.data_ptr(), pitch, 0, c.h, stream.cuda_stream)
            w.check(stream.cuda_stream)
            _same_canvas(buf.cpu().numpy(), colour, None, what + " render_band")
            got = w.render().reshape(c.h, 4 * c.w)
            _same_canvas(got, colour, None, what + " update_image")
        check_planes(c, s)


def check_subsets(c):
    """render_subset and render_subset_aux with SUBSETS at S = 1 and 2 into poisoned whole-frame
    targets: the addressed pixels are the oracle's update_image bytes (and its dumps), every other
    byte is the poison."""
    stream = _stream()
    for s in (1, 2):
        want = c.planes(s)
        with _world(c, s) as w:
            for sub in SUBSETS:
                what = f"{c.case.id} subset {sub} S={s}"
                mask = _addressed(sub, c.w, c.h)
                colour = c.subset_colour(sub, s)
                pitch = 4 * c.w + 32
                plain = poisoned((c.h, pitch), POISON)
                t = Targets(c.w, c.h)
                w.render_subset(plain.data_ptr(), pitch, *sub, stream=stream.cuda_stream)
                w.render_subset_aux(t.colour_ptr(), t.pitch["colour"], *sub, stream=stream.cuda_stream,
                                    **t.args())
                w.check(stream.cuda_stream)
                _same_canvas(plain.cpu().numpy(), colour, None, what + " render_subset")
                t.check(colour, want, what + " render_subset_aux", mask)
                assert (colour[~mask] == POISON).all()


def check_views(c):
    """The case's camera and four borrowed ones as one render_views_aux batch, without and with
    SFRT_VIEWS_SORT: each view is the oracle's of that camera (sorted: on oracle.sort_spheres'
    order); afterwards the world's own render_band is still its own oracle frame."""
    stream = _stream()
    with _world(c) as w:
        for sort in (False, True):
            views = [Targets(c.w, c.h) for _ in c.cams]
            pitch = views[0].pitch["colour"]
            w.render_views_aux([(_camera(cam), t.colour_ptr()) for cam, t in zip(c.cams, views)],
                               [t.args() for t in views], pitch, sort=sort, stream=stream.cuda_stream)
            w.check(stream.cuda_stream)
            for k, (cam, t) in enumerate(zip(c.cams, views)):
                t.check(c.frame(1, cam, sort), c.planes(1, cam, sort),
                        f"{c.case.id} view {k} sort={sort}")
        buf = poisoned((c.h, pitch), POISON)
        w.render_band(buf.data_ptr(), pitch, 0, c.h, stream.cuda_stream)
        w.check(stream.cuda_stream)
        _same_canvas(buf.cpu().numpy(), c.frame(), None, f"{c.case.id}: the world's own band after the batches")


def own_origin_rays(c):
    """RAYS rays with an origin each, and raycast_ref's answer: origins at sphere centres, on
    sphere surfaces (a centre plus the radius along an axis) and around the camera (inside the
    swarm, for a swarm case); directions axis-parallel or random, a quarter of them scaled by
    1e-18 or 1e18 (valid) and every 32nd by 1e-20 or 1e20, whose squared length is no finite
    normal number; a zero, a NaN and an infinite direction and a NaN origin among them."""
    def make():
        rng = np.random.default_rng(99 + c.index)
        n = c.spheres.shape[0]
        k = rng.integers(0, n, RAYS)
        kind = np.arange(RAYS) % 3
        axes = np.eye(3, dtype=F)[rng.integers(0, 3, RAYS)] * rng.choice(F([-1, 1]), RAYS)[:, None]
        origins = c.spheres[k, :3].copy()
        origins[kind == 1] = (origins + axes * c.spheres[k, 3:4])[kind == 1]
        cam = np.asarray(c.cam[0], dtype=F)
        near = (cam + rng.uniform(-0.5, 0.5, (RAYS, 3)).astype(F) * F(min(1.0, float(c.spheres[:, 3].max()))))
        origins[kind == 2] = near.astype(F)[kind == 2]
        dirs = np.eye(3, dtype=F)[rng.integers(0, 3, RAYS)] * rng.choice(F([-1, 1]), RAYS)[:, None]
        free = rng.random(RAYS) < 0.5
        free[7::32] = False  # the 1e-20 / 1e20 ones stay axis-parallel: invalid whatever was drawn
        dirs[free] = rng.standard_normal((RAYS, 3)).astype(F)[free]
        scale = np.ones(RAYS, dtype=F)
        scale[3::4] = rng.choice(F([1e-18, 1e18]), RAYS)[3::4]
        scale[7::32] = rng.choice(F([1e-20, 1e20]), RAYS)[7::32]
        dirs = (dirs * scale[:, None]).astype(F)
        bad = {5: F([0, 0, 0]), 64 + 27: F([np.nan, 1, 0]), 7 * 64: F([1, np.inf, 0]),
               RAYS - 3: F([-0.0, 0, 0])}
        for at, d in bad.items():
            dirs[at] = d
        origins[3 * 64 + 1, 1] = np.nan
        meant = np.array(sorted(list(bad) + [3 * 64 + 1] + list(range(7, RAYS, 32))))
        ref = raycast_ref.raycast(c.spheres, cam, dirs, origins, textures=dict(enumerate(c.textures)),
                                  sphere_tex=c.slots, max_steps=fuzz.MARCH_GUARD)
        assert not ref["valid"][meant].any() and ref["inside"].all()
        invalid = np.flatnonzero(~ref["valid"])  # (a short random direction times 1e-18 as well)
        assert meant.size <= invalid.size <= meant.size + 8
        for a in (dirs, origins, invalid, *ref.values()):
            a.setflags(write=False)
        return dirs, origins, invalid, ref
    return c.memo("rays", make)


def check_rays(c):
    """cast_rays_device: the frame's own primary directions, row-major and shuffled, against the
    oracle in all five outputs; own_origin_rays against raycast_ref; invalid rays are answered
    with sphere -1 and zeros."""
    from test_cast_rays import OUTPUTS, _device_cast, _same, _unpermute
    want = c.planes()
    n = c.w * c.h
    frame = {"pos": want["pos"].reshape(n, 3), "depth": want["depth"].reshape(n),
             "sphere": want["sphere"].reshape(n), "steps": want["steps"].reshape(n),
             "rgba": c.frame().reshape(n, 4)}
    dirs = raycast_ref.pixel_dirs(c.sc, c.w, c.h).reshape(n, 3)
    shuffle = np.random.default_rng(7).permutation(n)
    stream = _stream()
    with _world(c) as w:
        _same(_device_cast(w, dirs, stream=stream), frame, f"{c.case.id}: pixel rays, row-major")
        got = _unpermute(_device_cast(w, dirs[shuffle], stream=stream), shuffle)
        _same(got, frame, f"{c.case.id}: pixel rays, shuffled")
        rd, ro, invalid, ref = own_origin_rays(c)
        got = _device_cast(w, rd, ro, stream=stream)
        _same(got, {k: ref[k] for k in OUTPUTS}, f"{c.case.id}: rays with their own origins")
        assert (got["sphere"][invalid] == -1).all(), c.case.id
        for name in ("pos", "depth", "steps", "rgba"):
            assert not np.ascontiguousarray(got[name][invalid]).view(np.uint8).any(), (c.case.id, name)


@functools.lru_cache(maxsize=None)
def _cache_rigs():
    """CaseRig and CaseTrio: test_hit_cache.HitRig and test_texel_cache.Trio on a case (built on
    first use: only the GPU tests and the sweep need the cache tests' modules)."""
    import test_hit_fractions  # noqa: F401  registers the sized textures in test_hit_cache.TEXTURES
    from test_hit_cache import TEXTURES, HitRig
    from test_texel_cache import Trio

    class CaseRig(HitRig):
        def __init__(self, c, s=1):
            import sfrt
            self.sfrt, self.c = sfrt, c
            self.spheres, self.slots = c.spheres.copy(), c.slots.copy()
            self.cam, self.s = c.cam, s
            self.width, self.height, self.row0, self.rows = c.w, c.h, 0, c.h
            # an ordered launch of a small frame at rays 0 uses two pixels per lane (trace_rays)
            self.rays = c.case.rays_per_lane or 2
            self.tex_key = None  # slot 0 holds the case's own texture
            self.w = _world(c, s)
            self.stream = _stream()

        def push(self):
            self.w.set_size(self.width, self.height)
            self.w.set_camera(*self.cam)
            self.w.set_spheres(self.spheres)
            self.w.set_sphere_textures(self.slots)

        def load(self, slot, name):
            assert slot == 0
            tex = self.c.textures[0] if name is None else TEXTURES[name]()
            self.w.load_texture(*tex, slot=0)
            self.tex_key, self.tex0_size = name, tex[1:]

        def w_h_of_slot_0(self):
            return self.tex0_size

        def want(self):
            tex0 = None if self.tex_key is None else TEXTURES[self.tex_key]()
            moved = None if np.array_equal(self.spheres, self.c.spheres) else self.spheres
            return self.c.frame(self.s, self.cam, spheres=moved, tex0=tex0, tex_name=self.tex_key)

    class CaseTrio(Trio):
        def __init__(self, c, s=1):
            self.r, self.m, self.h = CaseRig(c, s), CaseRig(c, s), CaseRig(c, s)
            self.m.w.set_option(self.m.sfrt.SFRT_OPT_HIT_CACHE_MB, 0)
            self.h.w.set_option(self.h.sfrt.SFRT_OPT_TEXEL_CACHE, 0)
            self.hfills = self.hhits = self.tfills = self.thits = 0
            self.hheld = self.theld = 0
            assert self.tstats(self.r) == (0, 0, 0)

        def same_status_frame(self, what, launch):
            """test_one_row_textures_same_status' rule: the status and the bytes of the marching
            world, the oracle's bytes whenever that status is 0."""
            from test_hit_cache import _status_and_frame
            got, frame = _status_and_frame(self.r)
            want, marched = _status_and_frame(self.m)
            hit, other = _status_and_frame(self.h)
            assert got == want and hit == want, (what, got, hit, want)
            assert np.array_equal(frame, marched) and np.array_equal(other, marched), what
            if want == 0:
                assert np.array_equal(frame, self.r.want()), what
            self.counted(what, launch)

    return CaseRig, CaseTrio


def check_caches(c, s=1):
    """Six frames at rest, four texture sizes in slot 0, a camera step and back, one sphere moved
    by an ulp: every frame is the oracle's and the launch the counters say (the module docstrings
    of tests/test_texel_cache.py and tests/test_hit_cache.py)."""
    from test_texel_cache import HIT, HIT_FILL, MARCH, TEXEL, TEXEL_FILL
    _, CaseTrio = _cache_rigs()
    what = f"{c.case.id} S={s}"
    with CaseTrio(c, s) as p:
        six = p.frames(what + " rest", MARCH, HIT_FILL, TEXEL_FILL, TEXEL, TEXEL, TEXEL)
        assert all(np.array_equal(six[0], f) for f in six[1:]), what
        assert (p.hfills, p.hhits, p.tfills, p.thits) == (1, 4, 1, 3)
        assert p.r.stats() == (1, 4) and p.r.w.ray_cache_stats()["cached_frames"] == 5, what
        assert p.h.hstats() == (1, 4, p.h.hit_bytes()), what
        texels = c.textures[0][1] * c.textures[0][2]
        for name in CACHE_SIZES + [None]:  # ... and the case's own texture again
            p.all(lambda rig: rig.load(0, name))
            # The texel key holds the drawn records' texture offsets and sizes (TexKey): it
            # changes when a sphere draws from slot 0, or when slot 0's texel count moves the
            # later slots that spheres draw from.  (255x257 and 65535x1 are both 65535 texels:
            # a textured case none of whose spheres is in slot 0 rightly keeps its records.)
            tw, th = p.r.w_h_of_slot_0()
            new_key = bool((c.slots == 0).any()) or tw * th != texels
            texels = tw * th
            for k, launch in enumerate((HIT, TEXEL_FILL, TEXEL) if new_key else (TEXEL,) * 3):
                p.same_status_frame(f"{what} {name} in slot 0, frame {k + 1}", launch)
        assert p.hfills == 1, what  # the hit records served every size
        # one step: to the next case's camera position and back
        home, away = c.cam, fuzz.stepped_camera(c.sc, c.others)
        assert away[0] != home[0]

        def cam(rig, to):
            rig.cam = to
            rig.push()
        p.all(lambda rig: cam(rig, away))
        p.frame(what + " one step", MARCH)
        p.all(lambda rig: cam(rig, home))
        p.frame(what + " back: the old records", TEXEL)

        def nudge(rig):
            rig.spheres = fuzz.nudged_spheres(c.sc)
            rig.push()
        p.all(nudge)
        p.frame(what + " sphere 0 moved by one ulp in x", MARCH)


FAMILIES = {"planes": check_planes, "supersample": check_supersample, "subsets": check_subsets,
            "views": check_views, "rays": check_rays, "caches": check_caches}


def check_case(c, s2_caches=False):
    """Every family check of one case."""
    for check in FAMILIES.values():
        check(c)
    if s2_caches:
        check_caches(c, 2)


# ---------------------------------------------------------------- GPU: the tests

@pytest.mark.gpu
@chunks
def test_planes(built, chunk):
    for k in chunk:
        check_planes(ctx(k))


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
def test_ray_batches(built, chunk):
    for k in chunk:
        assert int(own_origin_rays(ctx(k))[3]["steps"].max()) > 1  # some of the rays do march
        check_rays(ctx(k))


@pytest.mark.gpu
@chunks
def test_caches_at_rest_and_under_one_step(built, chunk):
    for k in chunk:
        check_caches(ctx(k))
        if k % 4 == 0:
            check_caches(ctx(k), 2)
