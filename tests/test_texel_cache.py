"""The texel cache (csrc/sfrt_raycache.h TexelRec, TexKey, ChainCaches; DESIGN.md 5 "Texel cache"): on
top of the hit cache, a chain stores each ray's texel index and brightness while the texture sizes
and the spheres' texture slots stand still as well, and its launches then read 8 bytes per ray and
no sphere record.  The texels themselves are read every frame.

Every frame is compared byte for byte with the CPU oracle of its own state, with a second world
whose SFRT_OPT_HIT_CACHE_MB is 0 (it marches every frame) and with a third whose
SFRT_OPT_TEXEL_CACHE is 0 (it stays on the hit cache); the status is 0, and
sfrt_world_hit_cache_stats and sfrt_world_texel_cache_stats are asserted after every frame: each
frame names the launch it expects (MARCH, HIT_FILL, HIT, TEXEL_FILL, TEXEL).  The rig, the shapes
and the scenes are tests/test_hit_cache.py's smallest: 72x20 at four pixels per lane (clamped edge
lanes both ways, tile_x > 0) and 40x9 at one; 10 spheres run the kernels whose records travel in the
arguments, 65 the list ones.
"""
import numpy as np
import pytest

from test_cull_cache import CAM
from test_hit_cache import TEXTURES, HitRig, _aux_band, _status_and_frame
from test_hit_fractions import SIZES, _name

pytestmark = pytest.mark.gpu

MARCH, HIT_FILL, HIT, TEXEL_FILL, TEXEL = "march", "hit fill", "hit", "texel fill", "texel"
SHAPES = [("n10", "72x20-r4"), ("n65", "72x20-r4"), ("n10", "40x9-r1"), ("n65", "40x9-r1")]
shapes = pytest.mark.parametrize("scene,geom", SHAPES, ids=[f"{s}-{g}" for s, g in SHAPES])


class Trio:
    """A world with every cache, one that marches every frame and one that stays on the hit cache,
    in the same state; and the counters the first is expected to show."""

    def __init__(self, scene, geom, s=1):
        self.r, self.m, self.h = HitRig(scene, geom), HitRig(scene, geom), HitRig(scene, geom)
        self.m.w.set_option(self.m.sfrt.SFRT_OPT_HIT_CACHE_MB, 0)
        self.h.w.set_option(self.h.sfrt.SFRT_OPT_TEXEL_CACHE, 0)
        assert self.r.w.get_option(self.r.sfrt.SFRT_OPT_TEXEL_CACHE) == 1
        assert self.h.w.get_option(self.h.sfrt.SFRT_OPT_TEXEL_CACHE) == 0
        if s != 1:
            for rig in self.rigs():
                rig.s = s
                rig.w.set_option(rig.sfrt.SFRT_OPT_SUPERSAMPLE, s)
        self.hfills = self.hhits = self.tfills = self.thits = 0
        self.hheld = self.theld = 0
        assert self.tstats(self.r) == (0, 0, 0)

    def rigs(self):
        return self.r, self.m, self.h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for rig in self.rigs():
            rig.w.close()

    def all(self, change):
        for rig in self.rigs():
            change(rig)

    def texel_bytes(self):
        return self.r.tiles() * self.r.rays * 64 * 8

    @staticmethod
    def tstats(rig):
        st = rig.w.texel_cache_stats()
        return st["fills"], st["hits"], st["bytes"]

    def frame(self, what, launch):
        """One frame of all three worlds; `launch` is what the first world's is expected to be."""
        got, frame = _status_and_frame(self.r)
        for rig, name in ((self.m, "the marching world"), (self.h, "the hit-cache world")):
            code, other = _status_and_frame(rig)
            assert code == 0, (what, name, code)
            assert np.array_equal(frame, other), (what, name)
        assert got == 0, (what, got)
        assert np.array_equal(frame, self.r.want()), what
        self.counted(what, launch)
        return frame

    def counted(self, what, launch):
        """The counters of the three worlds after a frame whose first world's launch was `launch`."""
        if launch == HIT_FILL:
            self.hfills += 1
            self.hheld, self.theld = self.r.hit_bytes(), 0  # a hit refill frees the texel records
        elif launch != MARCH:
            self.hhits += 1
            self.tfills += launch == TEXEL_FILL
            self.thits += launch == TEXEL
            if launch == TEXEL_FILL:
                self.theld = self.texel_bytes()
        assert self.r.hstats() == (self.hfills, self.hhits, self.hheld), (what, launch)
        assert self.tstats(self.r) == (self.tfills, self.thits, self.theld), (what, launch)
        assert self.m.hstats() == (0, 0, 0) and self.tstats(self.m) == (0, 0, 0), what
        assert self.tstats(self.h) == (0, 0, 0), what

    def frames(self, what, *launches):
        return [self.frame(f"{what}, frame {k + 1}", launch) for k, launch in enumerate(launches)]

    def start(self):
        """The rest sequence up to the first launch that reads the texel records."""
        self.frames("start", MARCH, HIT_FILL, TEXEL_FILL, TEXEL)


@shapes
def test_six_frames_at_rest(built, scene, geom):
    with Trio(scene, geom) as p:
        six = p.frames("rest", MARCH, HIT_FILL, TEXEL_FILL, TEXEL, TEXEL, TEXEL)
        assert all(np.array_equal(six[0], f) for f in six[1:])
        assert (p.hfills, p.hhits, p.tfills, p.thits) == (1, 4, 1, 3)
        # a texel read counts as a read of the three layers under it; the third world read its hit cache
        assert p.r.stats() == (1, 4) and p.r.w.ray_cache_stats()["cached_frames"] == 5
        assert p.h.hstats() == (1, 4, p.h.hit_bytes())
        assert p.theld == p.r.tiles() * p.r.rays * 64 * 8 and 2 * p.theld == p.hheld


@shapes
def test_new_texels_of_the_same_size_keep_the_layer(built, scene, geom):
    """The texels are read every frame: another texture of the same size between two texel-reading
    launches shows in the next frame, which is still a texel hit."""
    with Trio(scene, geom) as p:
        p.start()
        a = p.frame("floor", TEXEL)
        p.all(lambda rig: rig.load(0, "green"))
        b = p.frame("green texels in slot 0", TEXEL)
        assert not np.array_equal(a, b)
        p.all(lambda rig: rig.load(0, "floor"))
        c = p.frame("the floor again", TEXEL)
        assert np.array_equal(a, c)
        assert p.tfills == 1


def _sizes_in_slot_0(p):
    p.start()
    seen = set()
    for size in SIZES:
        p.all(lambda rig: rig.load(0, _name(size)))
        three = p.frames("%dx%d in slot 0" % size, HIT, TEXEL_FILL, TEXEL)
        assert np.array_equal(three[0], three[1]) and np.array_equal(three[0], three[2])
        seen.add(three[0].tobytes())
    assert len(seen) > 1  # the frames do depend on the texture
    p.all(lambda rig: rig.load(0, "floor"))
    p.frames("the floor again", HIT, TEXEL_FILL, TEXEL)
    assert p.hfills == 1  # the hit records served every size


@shapes
def test_texture_sizes(built, scene, geom):
    """test_hit_fractions' sizes in slot 0: the launch of the change reads the hit cache, which was
    kept for it, the next stores the indices of the new size, the one after reads them."""
    with Trio(scene, geom) as p:
        _sizes_in_slot_0(p)


@pytest.mark.parametrize("s,scene,geom", [(2, "n65", "72x20-r4"), (4, "n10", "40x9-r1")],
                         ids=["2x-n65-72x20-r4", "4x-n10-40x9-r1"])
def test_supersampled(built, s, scene, geom):
    with Trio(scene, geom, s=s) as p:
        p.start()
        p.all(lambda rig: rig.load(0, _name((255, 257))))
        p.frames("255x257", HIT, TEXEL_FILL, TEXEL)
        p.all(lambda rig: rig.load(0, "green"))
        p.frames("green", HIT, TEXEL_FILL, TEXEL, TEXEL)
        assert p.theld == p.r.tiles() * p.r.rays * 64 * 8  # per sample


@shapes
def test_slot_changes(built, scene, geom):
    """set_sphere_textures over slots whose textures differ in size: every new assignment is a new
    key; the same assignment again is not."""
    def slots(rig, values):
        rig.slots = np.asarray(values, dtype=np.int32)
        rig.push()

    with Trio(scene, geom) as p:
        p.start()
        n = p.r.spheres.shape[0]
        p.all(lambda rig: rig.load(1, _name((1, 7))))  # after slot 0 in the atlas: slot 0 stays where it is
        p.frame("a texture in a slot no sphere uses", TEXEL)
        p.all(lambda rig: slots(rig, np.arange(n) % 2))
        p.frames("every other sphere in slot 1", HIT, TEXEL_FILL, TEXEL)
        p.all(lambda rig: slots(rig, np.arange(n) % 2))
        p.frame("the same slots pushed again", TEXEL)
        p.all(lambda rig: slots(rig, np.arange(n) % 3 == 0))
        p.frames("every third sphere in slot 1", HIT, TEXEL_FILL, TEXEL)
        p.all(lambda rig: slots(rig, np.zeros(n)))
        p.frames("every sphere in slot 0 again", HIT, TEXEL_FILL, TEXEL)


@shapes
def test_a_load_that_moves_the_drawn_slot(built, scene, geom):
    """Every sphere draws from slot 1; a texture of another size in slot 0 moves slot 1's texels in
    the atlas (its tex_off), though slot 1 itself was not touched."""
    def slot_1(rig):
        rig.slots[:] = 1
        rig.push()

    with Trio(scene, geom) as p:
        p.all(slot_1)
        p.start()
        p.all(lambda rig: rig.load(0, "small"))
        p.frames("48x20 in slot 0", HIT, TEXEL_FILL, TEXEL)
        p.all(lambda rig: rig.load(0, "green"))
        p.frames("the floor's size in slot 0 again", HIT, TEXEL_FILL, TEXEL)
        p.all(lambda rig: rig.load(0, "floor"))
        p.frame("other texels of that size in slot 0", TEXEL)


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
        p.frame("back: nothing was rewritten", TEXEL)
        p.all(lambda rig: cam(rig, (CAM[0] + 0.03, CAM[1], CAM[2] + 0.02)))
        p.frames("the step again, to stay", MARCH, HIT_FILL, TEXEL_FILL, TEXEL)
        assert (p.hfills, p.tfills) == (2, 2)


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_aux_band_between_texel_reads(built, scene):
    """A launch that takes no part in the caches between two texel-reading launches."""
    with Trio(scene, "72x20-r4") as p:
        p.start()
        first = p.frame("before", TEXEL)
        before = p.r.hstats(), p.tstats(p.r), p.r.stats(), p.r.w.ray_cache_stats()
        aux = _aux_band(p.r)
        assert (p.r.hstats(), p.tstats(p.r), p.r.stats(), p.r.w.ray_cache_stats()) == before
        last = p.frame("after", TEXEL)
        assert np.array_equal(aux, first) and np.array_equal(last, first)


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_option_off_and_on(built, scene):
    with Trio(scene, "72x20-r4") as p:
        opt = p.r.sfrt.SFRT_OPT_TEXEL_CACHE
        p.start()
        p.r.w.set_option(opt, 0)  # frees that layer only
        p.theld = 0
        assert p.tstats(p.r) == (1, 1, 0) and p.r.hstats() == (1, 2, p.r.hit_bytes())
        assert p.r.w.get_option(opt) == 0
        p.frames("off", HIT, HIT)
        p.r.w.set_option(opt, 1)
        p.frames("on again", HIT, TEXEL_FILL, TEXEL)
        with pytest.raises(p.r.sfrt.SfrtError):
            p.r.w.set_option(opt, -1)
        assert p.r.w.get_option(opt) == 1
        p.frame("still on", TEXEL)


def test_budget_shared_with_the_hit_records(built):
    """404x236 at 16x8 tiles (test_hit_cache.test_budgets' geometry): 1,597,440 B of hit records and
    798,720 B of texel records.  2 MB admits the first but not both; 3 MB admits both."""
    with Trio("n10", "40x9-r2") as p:
        def big(rig):
            rig.width, rig.height, rig.row0, rig.rows = 404, 236, 0, 236
            rig.push()

        p.all(big)
        assert p.r.hit_bytes() == 1597440 and p.texel_bytes() == 798720
        opt = p.r.sfrt.SFRT_OPT_HIT_CACHE_MB
        p.r.w.set_option(opt, 2)
        p.frames("budget 2", MARCH, HIT_FILL, HIT, HIT, HIT)
        assert p.tstats(p.r) == (0, 0, 0)
        p.r.w.set_option(opt, 3)
        p.frames("budget 3", TEXEL_FILL, TEXEL)
        p.r.w.set_option(opt, 2)  # lowered below what is held: the hit cache's bytes go, texel records included
        p.hheld = p.theld = 0
        assert p.r.hstats() == (1, 5, 0) and p.tstats(p.r) == (1, 1, 0)
        p.frames("budget 2 again", MARCH, HIT_FILL, HIT)
