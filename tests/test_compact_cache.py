"""The compact layer (csrc/sfrt_raycache.h CompactRec, BrightClasses, ChainCaches; DESIGN.md 5
"Compact layer"): on top of the texel cache, while no drawn texture ends beyond texel 65,535 of the
atlas and the world is not supersampled, a chain stores each ray in 4 bytes -- the texel's index
and the class of its brightness -- and its launches read those (k_shade_compact: a lane owns R
consecutive pixels of a row and stores them with one instruction).

Every frame of three worlds -- every cache at SFRT_OPT_COMPACT_TEXELS 2 (every eligible launch; the
default, 1, serves four pixels per lane and at most 64 spheres), SFRT_OPT_COMPACT_TEXELS 0 (it stays on the texel
cache) and SFRT_OPT_HIT_CACHE_MB 0 (it marches every frame) -- is compared byte for byte with the
other two and with the CPU oracle of its own state; the status is 0; and the hit, texel and compact
counters are asserted after every frame: each frame names the launch it expects.  The sequence is
tests/test_texel_cache.py's with the compact fill in the fourth frame.  Shapes: 72x20 and 40x9 at
one to four pixels per lane (72 and 40 leave a partial edge tile at every one of them), 10 spheres
(records in the arguments) and 65 (the list kernels); every target has a pitch of 4 * width + 16
bytes, and a band with row0 > 0 and a base 4 bytes off 16-byte alignment run beside them.
"""
import functools

import numpy as np
import pytest

import test_hit_fractions  # noqa: F401  registers the sized textures in test_hit_cache.TEXTURES
from conftest import poisoned
from test_cull_cache import CAM, POISON
from test_hit_cache import TEXTURES, HitRig, _aux_band, _status_and_frame
from test_hit_fractions import _name, _sized

pytestmark = pytest.mark.gpu

MARCH, HIT_FILL, HIT, TEXEL_FILL, TEXEL = "march", "hit fill", "hit", "texel fill", "texel"
COMPACT_FILL, COMPACT = "compact fill", "compact"
REST = (MARCH, HIT_FILL, TEXEL_FILL, COMPACT_FILL, COMPACT)

# width, height, row0, rows, pixels per lane
GEOMS = {f"{w}x{h}-r{r}": (w, h, 0, h, r) for w, h in ((72, 20), (40, 9)) for r in (1, 2, 3, 4)}
GEOMS["band-r4"] = (72, 40, 8, 12, 4)
GEOMS["band-r3"] = (72, 40, 16, 9, 3)
ALL_SHAPES = [(s, g) for g in GEOMS for s in ("n10", "n65")]
all_shapes = pytest.mark.parametrize("scene,geom", ALL_SHAPES, ids=[f"{s}-{g}" for s, g in ALL_SHAPES])
SHAPES = [("n10", "72x20-r4"), ("n65", "72x20-r4"), ("n10", "40x9-r1"), ("n65", "40x9-r3"), ("n10", "72x20-r2")]
shapes = pytest.mark.parametrize("scene,geom", SHAPES, ids=[f"{s}-{g}" for s, g in SHAPES])

# 256x256: 65,536 texels, one more than a compact record can index
TEXTURES.setdefault("sized256x256", functools.partial(_sized, 256, 256))


class Counters:
    """The upper layers' sizes and counters of a HitRig."""

    def compact_bytes(self):
        return self.tiles() * self.rays * 64 * 4

    def texel_bytes(self):
        return self.tiles() * self.rays * 64 * 8

    def tstats(self):
        st = self.w.texel_cache_stats()
        return st["fills"], st["hits"], st["bytes"]

    def cstats(self):
        st = self.w.compact_cache_stats()
        return st["fills"], st["hits"], st["bytes"]


class CompactRig(Counters, HitRig):
    """HitRig on this module's geometries; base_off: bytes the target's base is moved off its
    allocation's alignment."""

    def __init__(self, scene, geom, base_off=0):
        super().__init__(scene, "72x20-r4")
        self.width, self.height, self.row0, self.rows, self.rays = GEOMS[geom]
        self.base_off = base_off
        self.w.set_option(self.sfrt.SFRT_OPT_RAYS_PER_LANE, self.rays)
        self.push()

    def queue(self, stream=None):
        stream = self.stream if stream is None else stream
        pitch = 4 * self.width + 16
        buf = poisoned((self.rows + 1, pitch), POISON)
        self.w.render_band(buf.data_ptr() + self.base_off, pitch, self.row0, self.rows, stream.cuda_stream)
        return buf

    def bytes_of(self, buf):
        pitch = 4 * self.width + 16
        flat = buf.cpu().numpy().reshape(-1)
        assert (flat[:self.base_off] == POISON).all()
        got = flat[self.base_off:self.base_off + self.rows * pitch].reshape(self.rows, pitch)
        assert (got[:, 4 * self.width:] == POISON).all()  # the last row's padding runs into the spare row
        assert (flat[self.base_off + self.rows * pitch:] == POISON).all()
        return got[:, :4 * self.width].reshape(self.rows, self.width, 4)


class _PlainRig(CompactRig):
    """CompactRig with HitRig's own target (test_hit_cache._aux_band reads it that way)."""

    def __init__(self, scene, geom, base_off=0):
        super().__init__(scene, geom, 0)

    queue = HitRig.queue
    bytes_of = HitRig.bytes_of


class Trio:
    """A world with every cache, one that stays on the texel cache and one that marches every
    frame, in the same state; and the counters the first two are expected to show."""

    def __init__(self, scene, geom, s=1, base_off=0, rig=CompactRig):
        self.r, self.t, self.m = (rig(scene, geom, base_off) for _ in range(3))
        self.setup(s)

    def setup(self, s=1):
        opt = self.r.sfrt
        assert self.r.w.get_option(opt.SFRT_OPT_COMPACT_TEXELS) == 1
        # 2: every eligible launch (the default serves four pixels per lane and <= 64 spheres only:
        # test_the_default_serves_the_proven_shape_only)
        self.r.w.set_option(opt.SFRT_OPT_COMPACT_TEXELS, 2)
        self.t.w.set_option(opt.SFRT_OPT_COMPACT_TEXELS, 0)
        self.m.w.set_option(opt.SFRT_OPT_HIT_CACHE_MB, 0)
        assert self.r.w.get_option(opt.SFRT_OPT_COMPACT_TEXELS) == 2
        assert self.t.w.get_option(opt.SFRT_OPT_COMPACT_TEXELS) == 0
        if s != 1:
            for rig in self.rigs():
                rig.s = s
                rig.w.set_option(opt.SFRT_OPT_SUPERSAMPLE, s)
        self.h = [0, 0, 0]  # fills, hits, bytes of the hit, texel and compact layers
        self.x = [0, 0, 0]
        self.c = [0, 0, 0]
        assert self.r.cstats() == (0, 0, 0)

    def rigs(self):
        return self.r, self.t, self.m

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
        texel, other = _status_and_frame(self.t)
        want, marched = _status_and_frame(self.m)
        if not same_status:
            assert want == 0, (what, want)
        assert got == want and texel == want, (what, got, texel, want)
        assert np.array_equal(frame, marched), (what, "the marching world")
        assert np.array_equal(other, marched), (what, "the texel-cache world")
        if want == 0:
            assert np.array_equal(frame, self.r.want()), what
        self.counted(what, launch)
        return frame

    def counted(self, what, launch):
        h, x, c = self.h, self.x, self.c
        if launch == HIT_FILL:
            h[0] += 1
            h[2], x[2], c[2] = self.r.hit_bytes(), 0, 0  # a hit refill frees what rides on it
        elif launch != MARCH:
            h[1] += 1
            if launch == TEXEL_FILL:
                x[0] += 1
                x[2], c[2] = self.r.texel_bytes(), 0  # a texel refill frees the compact records first
            elif launch != HIT:
                x[1] += 1  # a compact launch counts as a read of the texel layer
                if launch == COMPACT_FILL:
                    c[0] += 1
                    c[2] = self.r.compact_bytes()
                elif launch == COMPACT:
                    c[1] += 1
        assert self.r.hstats() == tuple(h), (what, launch)
        assert self.r.tstats() == tuple(x), (what, launch)
        assert self.r.cstats() == tuple(c), (what, launch)
        # the world without the layer: the same launches of the layers under it
        assert self.t.hstats() == tuple(h) and self.t.tstats() == tuple(x), (what, launch)
        assert self.t.cstats() == (0, 0, 0), what
        assert self.m.hstats() == (0, 0, 0) and self.m.tstats() == (0, 0, 0) and self.m.cstats() == (0, 0, 0), what

    def frames(self, what, *launches, same_status=False):
        return [self.frame(f"{what}, frame {k + 1}", launch, same_status) for k, launch in enumerate(launches)]

    def start(self):
        """The rest sequence up to the first launch that reads the compact records."""
        self.frames("start", *REST)


@all_shapes
def test_seven_frames_at_rest(built, scene, geom):
    with Trio(scene, geom) as p:
        seven = p.frames("rest", *REST, COMPACT, COMPACT)
        assert all(np.array_equal(seven[0], f) for f in seven[1:])
        assert (p.h[:2], p.x[:2], p.c[:2]) == ([1, 5], [1, 4], [1, 3])
        # a compact read counts as a read of the four layers under it
        assert p.r.stats() == (1, 5) and p.r.w.ray_cache_stats()["cached_frames"] == 6
        assert p.c[2] == p.r.tiles() * p.r.rays * 64 * 4 and 2 * p.c[2] == p.x[2] and 4 * p.c[2] == p.h[2]


@pytest.mark.parametrize("scene,geom", [("n10", "72x20-r4"), ("n65", "72x20-r4"), ("n10", "40x9-r3"),
                                        ("n65", "40x9-r2"), ("n10", "band-r4")])
def test_a_base_four_bytes_off_alignment(built, scene, geom):
    """The whole-line stores promise no alignment beyond a pixel's: base + 4 and base + 12 with a
    pitch of 4 * width + 16 put every row 4 bytes off a 16-byte boundary."""
    for off in (4, 12):
        with Trio(scene, geom, base_off=off) as p:
            p.frames(f"base + {off}", *REST, COMPACT)


@shapes
def test_new_texels_of_the_same_size_keep_the_layer(built, scene, geom):
    with Trio(scene, geom) as p:
        p.start()
        a = p.frame("floor", COMPACT)
        p.all(lambda rig: rig.load(0, "green"))
        b = p.frame("green texels in slot 0", COMPACT)
        assert not np.array_equal(a, b)
        p.all(lambda rig: rig.load(0, "floor"))
        c = p.frame("the floor again", COMPACT)
        assert np.array_equal(a, c)
        assert p.c[0] == 1 and p.x[0] == 1


@shapes
def test_the_largest_texture_fills_and_one_texel_more_never_does(built, scene, geom):
    """65535x1 in slot 0 ends at texel 65,535: the layer fills.  256x256 ends at 65,536: the chain
    stays on the texel cache, the compact counters stand, the frames stay right.  The floor again
    fills again."""
    with Trio(scene, geom) as p:
        p.start()
        p.all(lambda rig: rig.load(0, "row65535"))
        p.frames("65535x1", HIT, TEXEL_FILL, COMPACT_FILL, COMPACT)
        held = tuple(p.c)
        p.all(lambda rig: rig.load(0, "sized256x256"))
        p.frames("256x256", HIT, TEXEL_FILL, TEXEL, TEXEL, TEXEL)
        assert tuple(p.c) == (held[0], held[1], 0)
        p.all(lambda rig: rig.load(0, _name((255, 257))))
        p.frames("255x257", HIT, TEXEL_FILL, COMPACT_FILL, COMPACT)
        p.all(lambda rig: rig.load(0, "floor"))
        p.frames("the floor again", HIT, TEXEL_FILL, COMPACT_FILL, COMPACT)
        assert p.h[0] == 1  # the hit records served every size


def test_a_world_that_only_ever_had_too_many_texels(built):
    """256x256 from the start: the compact stats stay 0."""
    with Trio("n10", "72x20-r4") as p:
        p.all(lambda rig: rig.load(0, "sized256x256"))
        p.frames("256x256", MARCH, HIT_FILL, TEXEL_FILL, TEXEL, TEXEL, TEXEL)
        assert p.r.cstats() == (0, 0, 0)


@shapes
def test_slot_changes(built, scene, geom):
    def slots(rig, values):
        rig.slots = np.asarray(values, dtype=np.int32)
        rig.push()

    with Trio(scene, geom) as p:
        p.start()
        n = p.r.spheres.shape[0]
        p.all(lambda rig: rig.load(1, _name((1, 7))))  # after slot 0 in the atlas: slot 0 stays where it is
        p.frame("a texture in a slot no sphere uses", COMPACT)
        p.all(lambda rig: slots(rig, np.arange(n) % 2))
        p.frames("every other sphere in slot 1", HIT, TEXEL_FILL, COMPACT_FILL, COMPACT)
        p.all(lambda rig: slots(rig, np.arange(n) % 2))
        p.frame("the same slots pushed again", COMPACT)
        p.all(lambda rig: slots(rig, np.zeros(n)))
        p.frames("every sphere in slot 0 again", HIT, TEXEL_FILL, COMPACT_FILL, COMPACT)


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
        p.frame("back: nothing was rewritten", COMPACT)
        p.all(lambda rig: cam(rig, (CAM[0] + 0.03, CAM[1], CAM[2] + 0.02)))
        p.frames("the step again, to stay", *REST)
        assert (p.h[0], p.x[0], p.c[0]) == (2, 2, 2)


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_aux_band_between_compact_reads(built, scene):
    with Trio(scene, "72x20-r4", rig=_PlainRig) as p:
        p.start()
        first = p.frame("before", COMPACT)
        before = p.r.hstats(), p.r.tstats(), p.r.cstats(), p.r.stats(), p.r.w.ray_cache_stats()
        aux = _aux_band(p.r)
        assert (p.r.hstats(), p.r.tstats(), p.r.cstats(), p.r.stats(), p.r.w.ray_cache_stats()) == before
        last = p.frame("after", COMPACT)
        assert np.array_equal(aux, first) and np.array_equal(last, first)


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_option_off_and_on(built, scene):
    with Trio(scene, "72x20-r4") as p:
        opt = p.r.sfrt.SFRT_OPT_COMPACT_TEXELS
        p.start()
        p.r.w.set_option(opt, 0)  # frees that layer only
        p.c[2] = 0
        assert p.r.cstats() == tuple(p.c) and p.r.tstats() == tuple(p.x) and p.r.hstats() == tuple(p.h)
        assert p.r.w.get_option(opt) == 0
        p.frames("off", TEXEL, TEXEL)
        p.r.w.set_option(opt, 2)
        p.frames("on again: the launches with the option off were the key's too", COMPACT_FILL, COMPACT)
        for bad in (-1, 3):
            with pytest.raises(p.r.sfrt.SfrtError):
                p.r.w.set_option(opt, bad)
        assert p.r.w.get_option(opt) == 2
        p.frame("still on", COMPACT)
        # the texel option frees both layers and nothing under them
        p.r.w.set_option(p.r.sfrt.SFRT_OPT_TEXEL_CACHE, 0)
        p.t.w.set_option(p.r.sfrt.SFRT_OPT_TEXEL_CACHE, 0)
        p.x[2] = p.c[2] = 0
        assert p.r.cstats() == tuple(p.c) and p.r.tstats() == tuple(p.x) and p.r.hstats() == tuple(p.h)
        p.frames("texel cache off", HIT, HIT)


@pytest.mark.parametrize("scene,geom,served", [("n10", "72x20-r4", True), ("n65", "72x20-r4", False),
                                               ("n10", "72x20-r2", False), ("n10", "40x9-r1", False)])
def test_the_default_serves_the_proven_shape_only(built, scene, geom, served):
    """SFRT_OPT_COMPACT_TEXELS 1, the default: four pixels per lane with the records in the
    arguments fill the layer, other shapes stay on the texel cache; lowering 2 to 1 frees records
    of a shape that 1 does not serve."""
    with Trio(scene, geom) as p:
        p.r.w.set_option(p.r.sfrt.SFRT_OPT_COMPACT_TEXELS, 1)
        if served:
            p.frames("default", *REST, COMPACT)
        else:
            p.frames("default", MARCH, HIT_FILL, TEXEL_FILL, TEXEL, TEXEL)
            assert p.r.cstats() == (0, 0, 0)
            p.r.w.set_option(p.r.sfrt.SFRT_OPT_COMPACT_TEXELS, 2)
            p.frames("every eligible launch", COMPACT_FILL, COMPACT)
            p.r.w.set_option(p.r.sfrt.SFRT_OPT_COMPACT_TEXELS, 1)
            p.c[2] = 0
            assert p.r.cstats() == tuple(p.c)
            p.frames("the default again", TEXEL, TEXEL)


def test_budget_shared_with_the_hit_and_texel_records(built):
    """404x236 at 16x8 tiles (test_texel_cache's geometry): 1,597,440 B of hit records, 798,720 B of
    texel records, 399,360 B of compact records.  2 MB admits the first alone, 3 MB all three
    (2,795,520 B); the byte-exact edges are tests/native/compactrec_check.cpp's."""
    with Trio("n10", "40x9-r2") as p:
        def big(rig):
            rig.width, rig.height, rig.row0, rig.rows = 404, 236, 0, 236
            rig.push()

        p.all(big)
        assert (p.r.hit_bytes(), p.r.texel_bytes(), p.r.compact_bytes()) == (1597440, 798720, 399360)
        opt = p.r.sfrt.SFRT_OPT_HIT_CACHE_MB
        for rig in (p.r, p.t):
            rig.w.set_option(opt, 2)
        p.frames("budget 2", MARCH, HIT_FILL, HIT, HIT)
        for rig in (p.r, p.t):
            rig.w.set_option(opt, 3)
        p.frames("budget 3", TEXEL_FILL, COMPACT_FILL, COMPACT)
        for rig in (p.r, p.t):
            rig.w.set_option(opt, 2)  # lowered below what is held: all three go
        p.h[2] = p.x[2] = p.c[2] = 0
        assert p.r.cstats() == tuple(p.c) and p.r.tstats() == tuple(p.x) and p.r.hstats() == tuple(p.h)
        p.frames("budget 2 again", MARCH, HIT_FILL, HIT)


@pytest.mark.parametrize("scene,geom", [("n65", "72x20-r4"), ("n10", "40x9-r1")])
def test_supersample_2_never_fills(built, scene, geom):
    with Trio(scene, geom, s=2) as p:
        p.frames("2x", MARCH, HIT_FILL, TEXEL_FILL, TEXEL, TEXEL, TEXEL)
        assert p.r.cstats() == (0, 0, 0)


@pytest.mark.parametrize("scene,geom", [("n10", "72x20-r4"), ("n65", "40x9-r3")])
def test_camera_within_distance_3_of_a_hit(built, scene, geom):
    """Brightness 3 / max(d, 3) = 1.0 for every hit nearer than 3: the last class.  The camera sits
    0.5 from the wall of the sphere {0, 0, 0, 4} that holds it, so the rays around that point end
    within 3 and the rest do not."""
    def near(rig):
        rig.cam = (3.5, 0.0, 0.0)
        rig.push()

    with Trio(scene, geom) as p:
        p.all(near)
        frames = p.frames("near the wall", *REST, COMPACT)
        tex = np.frombuffer(TEXTURES["floor"]()[0], dtype=np.uint8).reshape(-1, 4)
        texels = {t.tobytes() for t in tex}
        unshaded = sum(px.tobytes() in texels for px in frames[0].reshape(-1, 4))
        assert 0 < unshaded  # some pixels are their texel itself: brightness exactly 1.0


# ---- the degenerate scenes of tests/sphere_fuzz_cases.py: NaN brightness, indices outside ----

FUZZ_TAGS = {"cam_centre", "cam_on_surface", "x1000", "fov_1e-4", "threshold_radius"}
FUZZ_CHUNKS = 6


@functools.lru_cache(maxsize=None)
def _fuzz_selection():
    import sphere_fuzz_cases as fuzz
    return tuple(k for k, c in enumerate(fuzz.cases()) if c.tags & FUZZ_TAGS)


@pytest.mark.parametrize("chunk", range(FUZZ_CHUNKS))
def test_degenerate_scenes(built, chunk):
    """The cases whose camera sits on a centre or a surface, whose coordinates reach 1000 or whose
    field of view is 1e-4 -- where the brightness is NaN or the index falls outside the texture --
    at rest for six frames: the status and the bytes of the marching world in every frame."""
    from test_sphere_family_fuzz import _cache_rigs, ctx
    CaseRig, _ = _cache_rigs()

    class Rig(Counters, CaseRig):
        pass

    class CaseTrio(Trio):
        def __init__(self, c):
            self.r, self.t, self.m = Rig(c), Rig(c), Rig(c)
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
            rest = REST + (COMPACT,) if eligible else (MARCH, HIT_FILL, TEXEL_FILL, TEXEL, TEXEL, TEXEL)
            p.frames(f"{c.case.id} rest", *rest, same_status=True)
