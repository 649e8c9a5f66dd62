"""The hit cache's record holds the two texture fractions and the brightness (csrc/sfrt_raycache.h
HitRec; DESIGN.md 5 "Hit cache"), not the position: what shade_texel has just before it reads the
texture's size.  A reading launch multiplies the stored fractions by the size of the moment, so
the texture sizes here are those at which that product matters -- one texel, one row, one column,
the two sides of 256 and the largest side a texture can have, both ways -- loaded between reading
launches that never refill.

After every change the reading launch leaves the status and the bytes of a marching launch of a
second world with SFRT_OPT_HIT_CACHE_MB 0, and both are the oracle's frame of that state; the
status is clear (tests/test_hit_cache_texel_bound.py: no size lets the index leave the texture).
The rig, the shapes and the scenes are tests/test_hit_cache.py's: 72x20 at four pixels per lane and
40x9 at one; 10 spheres run the kernels whose records travel in the arguments, 65 the list ones.
"""
import functools

import numpy as np
import pytest

from test_cull_cache import F
from test_hit_cache import TEXTURES, HitRig, _status_and_frame

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (3, 1), (1, 7), (255, 257), (257, 255), (65535, 1), (1, 65535))


@functools.lru_cache(maxsize=None)
def _sized(tw, th):
    """A tw x th texture whose neighbouring texels differ, along rows and along columns."""
    k = np.arange(tw * th, dtype=np.uint32)
    x, y = k % tw, k // tw
    t = np.stack([(x * 37 + y * 11 + 1) & 255, (x * 5 + y * 59 + 7) & 255, (k * 17 + 3) & 255,
                  np.full_like(k, 255)], axis=1).astype(np.uint8).ravel()
    t.setflags(write=False)
    return t, tw, th


def _name(size):
    return "sized%dx%d" % size


# HitRig.load and its oracle look textures up by name in test_hit_cache's table
TEXTURES.update({_name(size): functools.partial(_sized, *size) for size in SIZES})


class Pair:
    """A world that reads its hit cache and one that marches every frame, in the same state."""

    def __init__(self, scene, geom, s=1):
        self.r, self.m = HitRig(scene, geom), HitRig(scene, geom)
        self.m.w.set_option(self.m.sfrt.SFRT_OPT_HIT_CACHE_MB, 0)
        for rig in (self.r, self.m):
            if s != 1:
                rig.s = s
                rig.w.set_option(rig.sfrt.SFRT_OPT_SUPERSAMPLE, s)
        self.fills = self.hits = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.r.w.close()
        self.m.w.close()

    def both(self, change):
        for rig in (self.r, self.m):
            change(rig)

    def start(self):
        """Three frames under the floor texture: the second stores, the third reads."""
        for rig in (self.r, self.m):
            for k in range(3):
                rig.check_frame(f"frame {k + 1}")
        self.fills, self.hits = 1, 1
        self.stats()

    def stats(self):
        assert self.r.hstats() == (self.fills, self.hits, self.r.hit_bytes())
        assert self.m.hstats() == (0, 0, 0)

    def reading_frame(self, what):
        """The next launch is a hit, never a refill, and equals the marching world and the oracle."""
        got, frame = _status_and_frame(self.r)
        want, marched = _status_and_frame(self.m)
        assert got == want == 0, (what, got, want)
        assert np.array_equal(frame, marched), what
        assert np.array_equal(frame, self.r.want()), what
        self.hits += 1
        self.stats()
        return frame


def _sizes_in_slot_0(p):
    p.start()
    seen = set()
    for size in SIZES:
        p.both(lambda rig: rig.load(0, _name(size)))
        seen.add(p.reading_frame("%dx%d in slot 0" % size).tobytes())
    assert len(seen) > 1  # the frames do depend on the texture
    p.both(lambda rig: rig.load(0, "floor"))
    p.reading_frame("the floor again")


@pytest.mark.parametrize("geom", ["72x20-r4", "40x9-r1"])
@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_texture_sizes_between_reading_launches(built, scene, geom):
    with Pair(scene, geom) as p:
        _sizes_in_slot_0(p)


def test_texture_sizes_supersample_two(built):
    with Pair("n65", "72x20-r4", s=2) as p:
        _sizes_in_slot_0(p)


@pytest.mark.parametrize("geom", ["72x20-r4", "40x9-r1"])
@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_slot_changes_between_reading_launches(built, scene, geom):
    """set_sphere_textures between reading launches, over slots whose textures differ in size."""
    def slots(rig, values):
        rig.slots = np.asarray(values, dtype=np.int32)
        rig.push()

    with Pair(scene, geom) as p:
        p.start()
        n = p.r.spheres.shape[0]
        p.both(lambda rig: rig.load(0, _name((255, 257))))
        p.both(lambda rig: rig.load(1, _name((1, 7))))
        p.reading_frame("every sphere in slot 0")
        p.both(lambda rig: slots(rig, np.arange(n) % 2))
        p.reading_frame("every other sphere in slot 1")
        p.both(lambda rig: slots(rig, (np.arange(n) % 3 == 0)))
        p.reading_frame("every third sphere in slot 1")
        p.both(lambda rig: rig.load(0, _name((65535, 1))))
        p.reading_frame("65535x1 in slot 0 under the same slots")
        p.both(lambda rig: slots(rig, np.ones(n)))
        p.reading_frame("every sphere in slot 1")
        p.both(lambda rig: slots(rig, np.zeros(n)))
        p.reading_frame("every sphere in slot 0 again")


def test_radius_change_drops_the_fractions(built):
    """The fractions depend on the drawn sphere's radius: the key drops the records with it.  The
    next frame marches, the one after stores again, later ones read; every frame is the oracle's."""
    def radius(rig):
        rig.spheres[min(3, len(rig.spheres) - 1), 3] *= F(1.05)
        rig.push()

    with Pair("n65", "72x20-r4") as p:
        p.start()
        p.both(lambda rig: rig.load(0, _name((257, 255))))
        p.reading_frame("257x255, old radius")
        p.both(radius)
        held = p.r.hit_bytes()
        for k in range(2):  # marches, then marches and stores
            a = p.r.check_frame(f"new radius, frame {k + 1}")
            b = p.m.check_frame(f"new radius, marching world, frame {k + 1}")
            assert np.array_equal(a, b)
            assert p.r.hstats() == (p.fills + k, p.hits, held) and p.m.hstats() == (0, 0, 0)
        p.fills += 1
        p.reading_frame("new radius, frame 3")
        p.both(lambda rig: rig.load(0, _name((1, 65535))))
        p.reading_frame("new radius, 1x65535")
