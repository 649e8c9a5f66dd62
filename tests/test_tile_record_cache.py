"""The tile records of the ray cache (csrc/sfrt_raycache.h TileRec): beside the directions, a
chain caches each tile's culling cone and grid position, which depend on the same key.

Every case renders the sequence uncached, fill, read, read (or a longer one) and compares each
frame byte for byte with the oracle and with a world whose SFRT_OPT_RAY_CACHE_MB is 0, whose
kernels compute the cone.  Shapes are the smallest that reach every path: 100x52 (a 13/7/5/4 x 7
grid at 8/16/24/32-pixel tiles, the last tile column and row holding clamped duplicates), a band
with row0 > 0, 404x236 at 16x8 tiles, 52x20 supersampled; default10 runs the kernel-argument
kernels, lcg256 the culled-list ones; R = 1, 2 take the cone from every ray, R = 3, 4 from the
tile's corner rays.  The rig, the poses and the shared, read-only oracle frames are those of
tests/test_ray_cache.py.
"""
import functools

import numpy as np
import pytest

import scenes
import test_ray_cache as rc
from conftest import host_threads

pytestmark = pytest.mark.gpu

REC = 32  # bytes per tile record
EDGE = (100, 52, 0, 52)   # width, height, row0, rows
BAND = (100, 52, 16, 20)  # rows 16..35: three tile rows, the last one half clamped
SMALL = (52, 20, 0, 20)


def tiles(width, rows, s, rays):
    return -(-width * s // (8 * rays)) * (-(-rows * s // 8))


def run_four(on, off, what=""):
    """uncached, fill, read, read: every frame the oracle's and the uncached world's."""
    expect = [(0, 0), (1, 1), (2, 1), (3, 1)]
    for k in range(4):
        a = on.check_frame(f"{what} frame {k + 1}")
        b = off.check_frame(f"{what} frame {k + 1}, cache off")
        assert np.array_equal(a, b), k
        assert on.stats() == expect[k], k
        recs = tiles(on.width, on.rows, on.s, on.rays) * REC
        assert on.w.tile_record_bytes() == (0 if k == 0 else recs)
        assert off.stats() == (0, 0) and off.held() == 0 and off.w.tile_record_bytes() == 0
    assert on.held() == rc.cache_bytes(on.width, on.rows, on.s, on.rays)  # directions only


class Rig(rc.Rig):
    def __init__(self, name, s=1, rays=0, geom="full", budget=None):
        self.rays = rays
        super().__init__(name, s, rays, geom, budget)


CASES = (
    # edge clamping, both cone variants, both kernel families
    [(name, 1, rays, EDGE) for name in ("default10", "lcg256") for rays in (1, 2, 3, 4)] +
    [("default10", 1, 2, (404, 236, 0, 236))] +
    # a subset: a row band with row0 > 0
    [(name, 1, rays, BAND) for name in ("default10", "lcg256") for rays in (2, 4)] +
    # supersampling
    [(name, s, rays, SMALL) for name in ("default10", "lcg256") for s in (2, 4) for rays in (2, 4)]
)


@pytest.mark.parametrize("name,s,rays,geom", CASES,
                         ids=[f"{n}-s{s}-r{r}-{g[0]}x{g[1]}+{g[2]}" for n, s, r, g in CASES])
def test_four_frames_of_one_pose(built, name, s, rays, geom):
    with Rig(name, s, rays, geom) as on, Rig(name, s, rays, geom, budget=0) as off:
        run_four(on, off)


# --- a wide tile -------------------------------------------------------------------------------
WIDE_FOV_H = 2.4  # half the image plane's horizontal extent at distance 1 (SphereWorld.cpp:85)


def wide_tiles(width, height, rays, fov_h, fov_v):
    """Per tile, whether some ray of it is more than 60 degrees off the tile's axis (the `wide`
    test of sphere_trace.hip's tile cones), from the host geometry in binary64: in camera space
    pixel (i, j) looks along (h, v, 1), h = -fov_h + 2 fov_h i / width, v likewise, and the axis
    looks through the tile's centre, columns past the frame's edge included."""
    tw = 8 * rays
    out = []
    for ty in range(-(-height // 8)):
        for tx in range(-(-width // tw)):
            def ray(i, j):
                d = np.array([-fov_h + 2.0 * fov_h * i / width,
                              -fov_v + 2.0 * fov_v * j / height, 1.0])
                return d / np.linalg.norm(d)
            axis = ray(tx * tw + 0.5 * tw - 0.5, ty * 8 + 3.5)
            cols = [min(tx * tw + c, width - 1) for c in range(tw)]
            rows = [min(ty * 8 + r, height - 1) for r in range(8)]
            out.append(min(float(ray(i, j) @ axis) for i in cols for j in rows))
    return np.array(out)


class WideRig(Rig):
    """The rig at a field of view no frame of the reference uses, its oracle frame its own."""

    def scene(self):
        sc = rc._scene(self.name, self.pose, self.cam_pos, self.drop)
        sc.fov_h = np.float32(WIDE_FOV_H)
        return sc

    def push(self):
        self.w.set_scene(self.scene(), self.width, self.height)

    def want(self):
        return wide_reference(self.name, self.width, self.height)[self.row0:self.row0 + self.rows]


@functools.lru_cache(maxsize=None)
def wide_reference(name, width, height):
    import oracle
    sc = rc._scene(name)
    sc.fov_h = np.float32(WIDE_FOV_H)
    out = oracle.Oracle.from_scene(sc, width, height, *rc._floor(0)).render(host_threads())
    out = out.reshape(height, width, 4).copy()
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("rays", [2, 4])
@pytest.mark.parametrize("name", ["default10", "lcg256"])
def test_a_wide_tile(built, name, rays):
    """A frame one tile and four pixels wide at a 2.4 rad half-extent: the first tile column's
    rays spread past 60 degrees of its axis (wide: not culled), the second's do not."""
    width, height = 8 * rays + 4, 12
    cos = wide_tiles(width, height, rays, WIDE_FOV_H, float(scenes.FOV_V))
    # far from the kernel's threshold of 0.5 on either side: binary32 cannot flip either
    assert (cos < 0.4).any() and (cos > 0.6).any() and not ((cos >= 0.4) & (cos <= 0.6)).any(), cos
    geom = (width, height, 0, height)
    with WideRig(name, 1, rays, geom) as on, WideRig(name, 1, rays, geom, budget=0) as off:
        run_four(on, off, "wide")


# --- key and position changes ---------------------------------------------------------------
@pytest.mark.parametrize("rays", [2, 4])
@pytest.mark.parametrize("name", ["default10", "lcg256"])
def test_position_change_keeps_the_records(built, name, rays):
    with Rig(name, 1, rays, EDGE) as on, Rig(name, 1, rays, EDGE, budget=0) as off:
        for k in range(3):  # uncached, fill, read
            on.check_frame(f"frame {k + 1}")
        assert on.stats() == (2, 1)
        held = on.w.tile_record_bytes()
        assert held == tiles(100, 52, 1, rays) * REC
        for k, pos in enumerate([(0.5, 0.2, -0.3), (0.9, -0.4, 0.6)]):
            for r in (on, off):
                r.cam_pos = pos
                r.push()
            a = on.check_frame(f"position {pos}")
            assert np.array_equal(a, off.check_frame(f"position {pos}, cache off"))
            assert on.stats() == (3 + k, 1) and on.w.tile_record_bytes() == held


@pytest.mark.parametrize("name", ["default10", "lcg256"])
def test_basis_change_drops_and_refills(built, name):
    with Rig(name, 1, 4, EDGE) as on, Rig(name, 1, 4, EDGE, budget=0) as off:
        for k in range(3):
            on.check_frame(f"frame {k + 1}")
        assert on.stats() == (2, 1)
        held = on.w.tile_record_bytes()
        turned = (rc.POSES[name][0] + 0.25, rc.POSES[name][1] - 0.1)
        for r in (on, off):
            r.pose = turned
            r.push()
        expect = [(2, 1), (3, 2), (4, 2)]  # a miss (no record of the old basis is read), fill, read
        for k in range(3):
            a = on.check_frame(f"turned, frame {k + 1}")
            assert np.array_equal(a, off.check_frame(f"turned, frame {k + 1}, cache off"))
            assert on.stats() == expect[k]
            assert on.w.tile_record_bytes() == held  # refilled in place
        for r in (on, off):
            r.pose = None
            r.push()
        a = on.check_frame("turned back")
        assert np.array_equal(a, off.check_frame("turned back, cache off"))
        assert on.stats() == (4, 2)  # the first basis' records are gone


@pytest.mark.parametrize("name", ["default10", "lcg256"])
def test_two_streams_alternating(built, name):
    """Each stream's chain has its own records."""
    import torch
    with Rig(name, 1, 4, EDGE) as on, Rig(name, 1, 4, EDGE, budget=0) as off:
        want = off.check_frame("cache off")
        streams = [on.stream, torch.cuda.Stream()]
        for k in range(8):
            assert np.array_equal(on.check_frame(f"frame {k}", streams[k % 2]), want)
        assert on.stats() == (6, 2)
        assert on.w.tile_record_bytes() == 2 * tiles(100, 52, 1, 4) * REC
        assert on.held() == 2 * rc.cache_bytes(100, 52, 1, 4)


@pytest.mark.parametrize("name", ["default10", "lcg256"])
def test_larger_grid_reallocates(built, name):
    """52x20 (2 x 3 tiles), then 100x52 (4 x 7) on the same stream: both buffers are replaced
    in stream order while the smaller frames may still be running; then back, into the larger
    buffers."""
    with Rig(name, 1, 4, SMALL) as on, Rig(name, 1, 4, SMALL, budget=0) as off:
        run_four(on, off, "52x20")
        for r in (on, off):
            r.width, r.height, r.row0, r.rows = EDGE
            r.push()
        expect = [(3, 1), (4, 2), (5, 2)]
        for k in range(3):
            a = on.check_frame(f"100x52, frame {k + 1}")
            assert np.array_equal(a, off.check_frame(f"100x52, frame {k + 1}, cache off"))
            assert on.stats() == expect[k]
            grid = (52, 20) if k == 0 else (100, 52)
            assert on.w.tile_record_bytes() == tiles(*grid, 1, 4) * REC
        assert on.held() == rc.cache_bytes(100, 52, 1, 4)
        for r in (on, off):
            r.width, r.height, r.row0, r.rows = SMALL
            r.push()
        for k in range(3):
            a = on.check_frame(f"52x20 again, frame {k + 1}")
            assert np.array_equal(a, off.check_frame(f"52x20 again, frame {k + 1}, cache off"))
        assert on.stats() == (7, 3)
        assert on.w.tile_record_bytes() == tiles(100, 52, 1, 4) * REC  # the buffers only grow


def test_option_zero_turns_the_records_off(built):
    with Rig("default10", 1, 4, EDGE) as r:
        frames = [r.check_frame(f"frame {k + 1}") for k in range(3)]
        assert r.stats() == (2, 1) and r.w.tile_record_bytes() == tiles(100, 52, 1, 4) * REC
        r.w.set_option(r.sfrt.SFRT_OPT_RAY_CACHE_MB, 0)
        assert r.w.tile_record_bytes() == 0 and r.held() == 0
        frames += [r.check_frame(f"off, frame {k + 1}") for k in range(3)]
        assert r.stats() == (2, 1) and r.w.tile_record_bytes() == 0
        r.w.set_option(r.sfrt.SFRT_OPT_RAY_CACHE_MB, 512)
        frames += [r.check_frame(f"on again, frame {k + 1}") for k in range(3)]
        # the key was committed while off: the first launch fills
        assert r.stats() == (5, 2) and r.w.tile_record_bytes() == tiles(100, 52, 1, 4) * REC
        assert all(np.array_equal(f, frames[0]) for f in frames)
