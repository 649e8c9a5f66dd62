"""The pixel layer (csrc/sfrt_raycache.h PixelKey, ChainCaches; DESIGN.md 5 "Pixel layer"): on top
of the texel cache and the compact layer, while the scene is at rest and no texture is loaded, a
chain keeps the finished RGBA8 band and its plain render_band launches are one copy of it into the
caller's frame (k_pixels_copy).

Every frame of three worlds -- every cache at SFRT_OPT_PIXEL_CACHE 2 (every plain band; the default,
1, serves launches that are not supersampled, have at most 64 spheres and an atlas the compact layer
can index), SFRT_OPT_PIXEL_CACHE 0 (it stays on the layer under it) and SFRT_OPT_HIT_CACHE_MB 0 (it
marches every frame) -- is
compared byte for byte with the other two and with the CPU oracle of its own state; the status is
equal in all three; and the hit, texel, compact and pixel counters are asserted after every frame:
each frame names the launch it expects, as one letter per layer (hit, texel, compact, pixel: T it
takes no part, F filled, R read).  Shapes: tests/test_compact_cache.py's -- 72x20 and 40x9 at one to
four pixels per lane, two bands with row0 > 0, 10 spheres and 65, a pitch of 4 * width + 16, a base
4 and 12 bytes off 16-byte alignment -- and widths that are no multiple of four pixels (the copy's
per-pixel row tail), narrower than one chunk included.

The status bits.  test_the_march_guard_status_in_every_frame runs a scene whose rays stop moving
short of their surface (coordinates of 10^6, where a step of 0.01 to 0.03 is below half an ulp): every
launch of it ends in SFRT_E_MARCH_LIMIT, the filling launch and every copy included.  No scene of
this renderer raises the texel bit: tests/test_hit_cache_texel_bound.py proves that for no size a
texture can have an index leaves its texture, so that bit has no case here.
"""
import functools

import numpy as np
import pytest

import test_hit_fractions  # noqa: F401  registers the sized textures in test_hit_cache.TEXTURES
from test_compact_cache import GEOMS as COMPACT_GEOMS
from test_compact_cache import CompactRig, Counters, _PlainRig
from test_cull_cache import CAM
from test_hit_cache import TEXTURES, _aux_band, _status_and_frame
from test_hit_fractions import _sized

pytestmark = pytest.mark.gpu

# hit, texel, compact, pixel
MARCH, HIT_FILL, HIT, TEXEL_FILL, TEXEL = "TTTT", "FTTT", "RTTT", "RFTT", "RRTT"
COMPACT_FILL, COMPACT, PIXEL_FILL, PIXEL = "RRFT", "RRRT", "RRRF", "RRRR"
TEXEL_PIXEL_FILL, TEXEL_PIXEL = "RRTF", "RRTR"  # where the launch has no compact layer
REST = (MARCH, HIT_FILL, TEXEL_FILL, COMPACT_FILL, PIXEL_FILL, PIXEL)
TEXEL_REST = (MARCH, HIT_FILL, TEXEL_FILL, TEXEL_PIXEL_FILL, TEXEL_PIXEL)

ALL_SHAPES = [(s, g) for g in COMPACT_GEOMS for s in ("n10", "n65")]
all_shapes = pytest.mark.parametrize("scene,geom", ALL_SHAPES, ids=[f"{s}-{g}" for s, g in ALL_SHAPES])
SHAPES = [("n10", "72x20-r4"), ("n65", "72x20-r4"), ("n10", "40x9-r1"), ("n65", "40x9-r3"), ("n10", "band-r3")]
shapes = pytest.mark.parametrize("scene,geom", SHAPES, ids=[f"{s}-{g}" for s, g in SHAPES])

TEXTURES.setdefault("sized256x256", functools.partial(_sized, 256, 256))


class PixelRig(CompactRig):
    def pixel_bytes(self):
        return self.width * self.rows * 4  # output pixels, whatever the supersampling factor

    def pstats(self):
        st = self.w.pixel_cache_stats()
        return st["fills"], st["hits"], st["bytes"]

    def sizes(self):
        return self.hit_bytes(), self.texel_bytes(), self.compact_bytes(), self.pixel_bytes()

    def all_stats(self):
        return [self.hstats(), self.tstats(), self.cstats(), self.pstats()]


class _PlainPixelRig(PixelRig):
    """PixelRig with HitRig's own target (test_hit_cache._aux_band reads it that way)."""

    def __init__(self, scene, geom, base_off=0):
        super().__init__(scene, geom, 0)

    queue = _PlainRig.queue
    bytes_of = _PlainRig.bytes_of


class Trio:
    """A world with every cache, one without the pixel layer and one that marches every frame, in
    the same state; and the counters the first two are expected to show."""

    def __init__(self, scene, geom, s=1, base_off=0, rig=PixelRig, shape=None):
        self.r, self.o, self.m = (rig(scene, geom, base_off) for _ in range(3))
        if shape is not None:
            for r in self.rigs():
                r.width, r.height, r.row0, r.rows = shape
                r.push()
        self.setup(s)

    def setup(self, s=1):
        opt = self.r.sfrt
        assert self.r.w.get_option(opt.SFRT_OPT_PIXEL_CACHE) == 1
        # 2: every plain band (the default serves the proven shapes only:
        # test_the_default_serves_the_proven_shapes_only)
        self.r.w.set_option(opt.SFRT_OPT_PIXEL_CACHE, 2)
        for rig in (self.r, self.o):
            rig.w.set_option(opt.SFRT_OPT_COMPACT_TEXELS, 2)  # every eligible launch, whatever its shape
        self.o.w.set_option(opt.SFRT_OPT_PIXEL_CACHE, 0)
        self.m.w.set_option(opt.SFRT_OPT_HIT_CACHE_MB, 0)
        assert self.o.w.get_option(opt.SFRT_OPT_PIXEL_CACHE) == 0
        if s != 1:
            for rig in self.rigs():
                rig.s = s
                rig.w.set_option(opt.SFRT_OPT_SUPERSAMPLE, s)
        self.n = [[0, 0, 0] for _ in range(4)]  # fills, hits, bytes of the hit, texel, compact and pixel layers
        assert self.r.pstats() == (0, 0, 0)

    def rigs(self):
        return self.r, self.o, self.m

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for rig in self.rigs():
            rig.w.close()

    def all(self, change):
        for rig in self.rigs():
            change(rig)

    def frame(self, what, launch, same_status=False):
        """One frame of all three worlds; `launch` is what the first world's is expected to be.
        same_status (tests/test_hit_cache.py's rule for degenerate scenes): the status and bytes of
        the marching world, the oracle's bytes whenever that status is 0."""
        got, frame = _status_and_frame(self.r)
        off, other = _status_and_frame(self.o)
        want, marched = _status_and_frame(self.m)
        self.status = want
        if not same_status:
            assert want == 0, (what, want)
        assert got == want and off == want, (what, got, off, want)
        assert np.array_equal(frame, marched), (what, "the marching world")
        assert np.array_equal(other, marched), (what, "the world without the pixel layer")
        if want == 0:
            assert np.array_equal(frame, self.r.want()), what
        self.counted(what, launch)
        return frame

    def counted(self, what, launch):
        sizes = self.r.sizes()
        for k, action in enumerate(launch):
            if action == "F":
                self.n[k][0] += 1
                self.n[k][2] = sizes[k]
                for up in range(k + 1, 4):  # a fill frees what rides on the layer first
                    self.n[up][2] = 0
            elif action == "R":
                self.n[k][1] += 1
        want = [tuple(v) for v in self.n]
        assert self.r.all_stats() == want, (what, launch, self.r.all_stats(), want)
        # the world without the layer: the same launches of the layers under it
        assert self.o.all_stats() == want[:3] + [(0, 0, 0)], (what, launch, self.o.all_stats())
        assert self.m.all_stats() == [(0, 0, 0)] * 4, what

    def frames(self, what, *launches, same_status=False):
        return [self.frame(f"{what}, frame {k + 1}", launch, same_status) for k, launch in enumerate(launches)]

    def start(self):
        """The rest sequence up to the first launch that is a copy of the cached pixels."""
        self.frames("start", *REST)


@all_shapes
def test_eight_frames_at_rest(built, scene, geom):
    with Trio(scene, geom) as p:
        eight = p.frames("rest", *REST, PIXEL, PIXEL)
        assert all(np.array_equal(eight[0], f) for f in eight[1:])
        assert [v[:2] for v in p.n] == [[1, 6], [1, 5], [1, 4], [1, 3]]
        # a pixel read counts as a read of the five layers under it
        assert p.r.stats() == (1, 6) and p.r.w.ray_cache_stats()["cached_frames"] == 7
        assert p.n[3][2] == p.r.width * p.r.rows * 4


@pytest.mark.parametrize("scene,geom", [("n10", "72x20-r4"), ("n65", "72x20-r4"), ("n10", "40x9-r3"),
                                        ("n65", "40x9-r2"), ("n10", "band-r4")])
def test_a_base_off_alignment(built, scene, geom):
    """The copy's chunks promise no alignment beyond a pixel's: base + 4 and base + 12 with a pitch
    of 4 * width + 16 put every row 4 bytes off a 16-byte boundary."""
    for off in (4, 12):
        with Trio(scene, geom, base_off=off) as p:
            p.frames(f"base + {off}", *REST, PIXEL)


# width, height, row0, rows: rows of 73, 41, 42 and 39 pixels end in a tail of 1, 1, 2 and 3 pixels
# (the layer's packed rows then start 4, 8 or 12 bytes off a 16-byte boundary); 3 is narrower than a
# chunk, 4 exactly one
TAILS = {"73x20": (73, 20, 0, 20), "41x9": (41, 9, 0, 9), "42x12+8": (42, 28, 8, 12), "39x9": (39, 9, 0, 9),
         "3x9": (3, 9, 0, 9), "4x5": (4, 5, 0, 5), "1x1": (1, 1, 0, 1)}


@pytest.mark.parametrize("scene,geom", [("n10", "72x20-r4"), ("n65", "40x9-r3"), ("n10", "40x9-r1")])
@pytest.mark.parametrize("shape", list(TAILS))
def test_row_tails(built, scene, geom, shape):
    for off in (0, 4):
        with Trio(scene, geom, base_off=off, shape=TAILS[shape]) as p:
            p.frames(f"{shape} base + {off}", *REST, PIXEL)


@pytest.mark.parametrize("scene,geom", [("n65", "72x20-r4"), ("n10", "40x9-r1"), ("n10", "band-r3")])
@pytest.mark.parametrize("s", [2, 4])
def test_supersampled(built, scene, geom, s):
    """No compact layer when supersampled: the fill rides on the texel reader, and the layer holds
    output pixels."""
    with Trio(scene, geom, s=s) as p:
        p.frames(f"{s}x", *TEXEL_REST, TEXEL_PIXEL, TEXEL_PIXEL)
        assert p.r.cstats() == (0, 0, 0) and p.r.pstats()[2] == p.r.width * p.r.rows * 4


def test_supersampled_row_tail(built):
    with Trio("n10", "40x9-r2", s=2, shape=TAILS["41x9"], base_off=12) as p:
        p.frames("2x 41x9", *TEXEL_REST, TEXEL_PIXEL)


@shapes
def test_a_texture_too_large_for_the_compact_layer(built, scene, geom):
    """256x256 ends at texel 65,536: the chain has no compact layer and the fill comes from the
    texel reader.  65535x1 ends at 65,535: all six layers."""
    with Trio(scene, geom) as p:
        p.all(lambda rig: rig.load(0, "sized256x256"))
        p.frames("256x256", *TEXEL_REST, TEXEL_PIXEL)
        assert p.r.cstats() == (0, 0, 0)
        p.all(lambda rig: rig.load(0, "row65535"))
        p.frames("65535x1", HIT, TEXEL_FILL, COMPACT_FILL, PIXEL_FILL, PIXEL, PIXEL)
        p.all(lambda rig: rig.load(0, "sized256x256"))
        p.frames("256x256 again", HIT, TEXEL_FILL, TEXEL_PIXEL_FILL, TEXEL_PIXEL)


@shapes
def test_new_texels_of_the_same_size(built, scene, geom):
    """The very next frame shows the new texels, shaded from the layer under this one, which stays;
    the frame after it is copied into the layer, the one after that is a copy out of it."""
    with Trio(scene, geom) as p:
        p.start()
        a = p.frame("floor", PIXEL)
        p.all(lambda rig: rig.load(0, "green"))
        b = p.frame("green texels in slot 0", COMPACT)
        assert not np.array_equal(a, b)
        c, d = p.frames("green at rest", PIXEL_FILL, PIXEL)
        assert np.array_equal(b, c) and np.array_equal(b, d)
        p.all(lambda rig: rig.load(0, "floor"))
        e = p.frame("the floor again", COMPACT)
        assert np.array_equal(a, e)
        p.frames("the floor at rest", PIXEL_FILL, PIXEL)
        assert [v[0] for v in p.n] == [1, 1, 1, 3]


@shapes
def test_a_reload_on_every_frame_never_fills(built, scene, geom):
    with Trio(scene, geom) as p:
        p.start()
        held = p.r.pstats()
        for k in range(5):
            p.all(lambda rig: rig.load(0, "green" if k % 2 == 0 else "floor"))
            p.frame(f"reload {k}", COMPACT)
        assert p.r.pstats() == held
        # the same texels loaded again are a reload too: the library compares no texel
        p.all(lambda rig: rig.load(0, "floor"))
        p.frames("the same texels", COMPACT, PIXEL_FILL, PIXEL)


@shapes
def test_a_reload_of_a_slot_no_sphere_draws(built, scene, geom):
    """Slot 1 is loaded and undrawn: new texels there change no pixel, and the library does not look
    -- the generation counts every load."""
    with Trio(scene, geom) as p:
        p.start()
        a = p.frame("before", PIXEL)
        p.all(lambda rig: rig.load(1, "green"))
        b, c, d = p.frames("slot 1 reloaded", COMPACT, PIXEL_FILL, PIXEL)
        assert all(np.array_equal(a, f) for f in (b, c, d))


@shapes
def test_slot_changes(built, scene, geom):
    def slots(rig, values):
        rig.slots = np.asarray(values, dtype=np.int32)
        rig.push()

    with Trio(scene, geom) as p:
        p.start()
        n = p.r.spheres.shape[0]
        p.all(lambda rig: slots(rig, np.arange(n) % 2))
        p.frames("every other sphere in slot 1", HIT, TEXEL_FILL, COMPACT_FILL, PIXEL_FILL, PIXEL)
        p.all(lambda rig: slots(rig, np.arange(n) % 2))
        p.frame("the same slots pushed again", PIXEL)
        p.all(lambda rig: slots(rig, np.zeros(n)))
        p.frames("every sphere in slot 0 again", HIT, TEXEL_FILL, COMPACT_FILL, PIXEL_FILL, PIXEL)


@shapes
def test_camera_step_and_return(built, scene, geom):
    def cam(rig, c):
        rig.cam = c
        rig.push()

    with Trio(scene, geom) as p:
        p.start()
        p.all(lambda rig: cam(rig, (CAM[0] + 0.03, CAM[1], CAM[2] + 0.02)))
        p.frame("one step", MARCH)
        p.all(lambda rig: cam(rig, CAM))
        p.frame("back: nothing was rewritten", PIXEL)
        p.all(lambda rig: cam(rig, (CAM[0] + 0.03, CAM[1], CAM[2] + 0.02)))
        p.frames("the step again, to stay", *REST)
        assert [v[0] for v in p.n] == [2, 2, 2, 2]


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_aux_band_between_pixel_reads(built, scene):
    with Trio(scene, "72x20-r4", rig=_PlainPixelRig) as p:
        p.start()
        first = p.frame("before", PIXEL)
        before = p.r.all_stats(), p.r.stats(), p.r.w.ray_cache_stats()
        aux = _aux_band(p.r)
        assert (p.r.all_stats(), p.r.stats(), p.r.w.ray_cache_stats()) == before
        last = p.frame("after", PIXEL)
        assert np.array_equal(aux, first) and np.array_equal(last, first)


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_option_off_and_on(built, scene):
    with Trio(scene, "72x20-r4") as p:
        opt = p.r.sfrt.SFRT_OPT_PIXEL_CACHE
        p.start()
        p.r.w.set_option(opt, 0)  # frees that layer only
        p.n[3][2] = 0
        assert p.r.all_stats() == [tuple(v) for v in p.n]
        assert p.r.w.get_option(opt) == 0
        p.frames("off", COMPACT, COMPACT)
        p.r.w.set_option(opt, 2)
        p.frames("on again", COMPACT, PIXEL_FILL, PIXEL)
        for bad in (-1, 3):
            with pytest.raises(p.r.sfrt.SfrtError):
                p.r.w.set_option(opt, bad)
        assert p.r.w.get_option(opt) == 2
        p.frame("still on", PIXEL)
        # the compact option frees both layers and nothing under them
        for rig in (p.r, p.o):
            rig.w.set_option(p.r.sfrt.SFRT_OPT_COMPACT_TEXELS, 0)
        p.n[2][2] = p.n[3][2] = 0
        assert p.r.all_stats() == [tuple(v) for v in p.n]
        p.frames("compact layer off", TEXEL, TEXEL_PIXEL_FILL, TEXEL_PIXEL)


@pytest.mark.parametrize("scene,geom,s,tex,served", [
    ("n10", "72x20-r4", 1, None, True), ("n10", "40x9-r1", 1, None, True), ("n65", "72x20-r4", 1, None, False),
    ("n10", "72x20-r4", 2, None, False), ("n10", "72x20-r4", 1, "sized256x256", False)])
def test_the_default_serves_the_proven_shapes_only(built, scene, geom, s, tex, served):
    """SFRT_OPT_PIXEL_CACHE 1, the default: no supersampling, at most 64 spheres and an atlas the
    compact layer can index fill the layer; other shapes stay on the layer under it until the option
    is 2, and lowering 2 to 1 frees pixels of a shape that 1 does not serve."""
    with Trio(scene, geom, s=s) as p:
        opt = p.r.sfrt.SFRT_OPT_PIXEL_CACHE
        p.r.w.set_option(opt, 1)
        if tex:
            p.all(lambda rig: rig.load(0, tex))
        compact = s == 1 and tex is None
        rest, below = (REST, COMPACT) if compact else (TEXEL_REST, TEXEL)
        fill, read = (PIXEL_FILL, PIXEL) if compact else (TEXEL_PIXEL_FILL, TEXEL_PIXEL)
        if served:
            p.frames("default", *rest, read)
        else:
            p.frames("default", *rest[:-2], below, below, below)
            assert p.r.pstats() == (0, 0, 0)
            p.r.w.set_option(opt, 2)
            p.frames("every plain band", below, fill, read)
            p.r.w.set_option(opt, 1)
            p.n[3][2] = 0
            assert p.r.all_stats() == [tuple(v) for v in p.n]
            p.frames("the default again", below, below)


def _stuck(rig):
    """One sphere of radius 4 around (10^6, 10^6, 10^6) and the camera half a unit from its centre:
    a coordinate's ulp is 0.0625 there, so a ray that lands where the sphere's wall is 0.01 to 0.03
    away steps by less than half an ulp in every component, stays where it is with a step above 0,
    and ends at the march guard."""
    rig.spheres = np.array([[1e6, 1e6, 1e6, 4.0]], dtype=np.float32)
    rig.slots = np.zeros(1, np.int32)
    rig.cam = (1e6 + 0.5, 1e6, 1e6)
    rig.push()


def test_the_march_guard_status_in_every_frame(built):
    """SFRT_E_MARCH_LIMIT (-6) from the marching world in every frame, and the same status and bytes
    from the other two in every frame: the launches that fill each layer, the launch whose band is
    copied into the pixel layer, and the copies out of it."""
    with Trio("n10", "40x9-r2") as p:
        p.all(_stuck)
        for k, launch in enumerate(REST + (PIXEL, PIXEL)):
            p.frame(f"stuck rays, frame {k + 1}", launch, same_status=True)
            assert p.status == -6, (k, p.status)
        # a step away the rays of this frame end: the word of the layer is the key's, not the world's
        p.all(lambda rig: (setattr(rig, "spheres", np.array([[0.0, 0.0, 0.0, 4.0]], dtype=np.float32)),
                           setattr(rig, "cam", CAM), rig.push()))
        p.frames("a scene that ends", *REST, PIXEL)
        p.all(_stuck)
        p.frames("stuck again", MARCH, same_status=True)
        assert p.status == -6


def test_budget_shared_with_the_layers_under_it(built):
    """404x236 at 16x8 tiles: 1,597,440 + 798,720 + 399,360 B of records and 381,376 B of pixels.  3 MB
    admits the records alone (2,795,520 B), 4 MB all four, 2 MB the hit records only; the byte-exact edges are
    tests/native/pixelcache_check.cpp's."""
    with Trio("n10", "40x9-r2", shape=(404, 236, 0, 236)) as p:
        assert p.r.sizes() == (1597440, 798720, 399360, 381376)
        opt = p.r.sfrt.SFRT_OPT_HIT_CACHE_MB
        for rig in (p.r, p.o):
            rig.w.set_option(opt, 3)
        p.frames("budget 3", MARCH, HIT_FILL, TEXEL_FILL, COMPACT_FILL, COMPACT, COMPACT)
        for rig in (p.r, p.o):
            rig.w.set_option(opt, 4)
        p.frames("budget 4", PIXEL_FILL, PIXEL)
        for rig in (p.r, p.o):
            rig.w.set_option(opt, 2)  # lowered below what either world holds: every layer goes
        for v in p.n:
            v[2] = 0
        assert p.r.all_stats() == [tuple(v) for v in p.n]
        p.frames("budget 2", MARCH, HIT_FILL, HIT)


# ---- the degenerate scenes of tests/sphere_fuzz_cases.py: NaN brightness, indices outside ----

FUZZ_TAGS = {"cam_centre", "cam_on_surface", "x1000", "fov_1e-4", "threshold_radius"}
FUZZ_CHUNKS = 6


@functools.lru_cache(maxsize=None)
def _fuzz_selection():
    import sphere_fuzz_cases as fuzz
    return tuple(k for k, c in enumerate(fuzz.cases()) if c.tags & FUZZ_TAGS)


@pytest.mark.parametrize("chunk", range(FUZZ_CHUNKS))
def test_degenerate_scenes(built, chunk):
    """tests/test_compact_cache.py's selection, at rest for seven frames: the status and the bytes
    of the marching world in every frame, the last two of them copies."""
    from test_sphere_family_fuzz import _cache_rigs, ctx
    CaseRig, _ = _cache_rigs()

    class Rig(Counters, CaseRig):
        pixel_bytes = PixelRig.pixel_bytes
        pstats = PixelRig.pstats
        sizes = PixelRig.sizes
        all_stats = PixelRig.all_stats

    class CaseTrio(Trio):
        def __init__(self, c):
            self.r, self.o, self.m = Rig(c), Rig(c), Rig(c)
            self.setup()

    picked = _fuzz_selection()
    assert len(picked) >= FUZZ_CHUNKS
    for k in picked[chunk::FUZZ_CHUNKS]:
        c = ctx(k)
        # the atlas holds the slots back to back; a record's texture ends at its offset + size
        sizes = [tw * th for _, tw, th in c.textures]
        ends = np.cumsum(sizes)
        eligible = max(int(ends[k]) for k in set(int(v) for v in c.slots) | ({0} if not c.textured else set())) <= 0xFFFF
        with CaseTrio(c) as p:
            rest = REST + (PIXEL,) if eligible else TEXEL_REST + (TEXEL_PIXEL, TEXEL_PIXEL)
            p.frames(f"{c.case.id} rest", *rest, same_status=True)
