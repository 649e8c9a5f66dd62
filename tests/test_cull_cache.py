"""The cull cache (csrc/sfrt_raycache.h CullKey, ChainCaches; DESIGN.md 5 "Cull cache"): beside the ray
directions and the tile records, a chain caches what each tile's wave culls -- the mask of the
spheres that may pass and every sphere's march window -- while the view, the camera position,
the sphere count and every sphere's centre and radius stay.

Every frame is compared byte for byte with the CPU oracle, and sfrt_world_cull_cache_stats tells
which path ran.  Frames are 72x20 at four pixels per lane and 40x9 at one, two and three: every
tile width but 8 gets a clamped right edge, every frame a short last tile row.  Scenes of 10, 64,
65 and 200 random spheres run the kernel-argument kernels and the culled-list ones on both sides
of their boundary; `cluster` makes list waves overflow their 64 entries.
"""
import functools
import hashlib

import numpy as np
import pytest

import scenes
from conftest import host_threads, poisoned

pytestmark = pytest.mark.gpu

F = np.float32
CAM = (0.25, -0.5, 0.125)  # inside the sphere {0, 0, 0, 4} every scene starts with
POSE = (0.7, 0.3)
POISON = 0xA5
# width, height, row0, rows, pixels per lane
GEOMS = {"72x20-r4": (72, 20, 0, 20, 4), "40x9-r1": (40, 9, 0, 9, 1), "40x9-r2": (40, 9, 0, 9, 2),
         "40x9-r3": (40, 9, 0, 9, 3), "band": (72, 40, 8, 12, 4)}
BYTES_INLINE, BYTES_LIST = 16 + 64 * 8, 16 + 64 * 12  # per tile


def random_spheres(n):
    return scenes.sort_spheres(scenes.lcg_spheres(count=n - 1, seed=4242 + n))


def cluster_spheres():
    """152 spheres: {0,0,0,4} around the camera, {0,0,0,25} around everything, and 150 of radius
    2 with centres within 1 of (0, 0, 16) in x and y and within 2 in z.  Seen from CAM at
    rotation 0 every cluster centre is within 8 degrees of the forward axis.  Of the 72x20
    frame's 32-pixel tile columns the middle one's middle tile has its axis 23.5 degrees off
    forward and a half-angle of 34.6 degrees: every cluster sphere's centre lies inside its cone,
    152 > 64, the wave overflows and marches the full list.  The last column's cones (axis 58
    degrees off forward, half-angle 16 degrees) are more than 25 degrees away from every cluster
    sphere: those waves cull the cluster away."""
    rows = [(0.0, 0.0, 0.0, 4.0), (0.0, 0.0, 0.0, 25.0)]
    s = 99
    for _ in range(150):
        s, a = scenes.msvc_rand(s)
        s, b = scenes.msvc_rand(s)
        s, c = scenes.msvc_rand(s)
        rows.append(((a % 21 - 10) / 10.0, (b % 21 - 10) / 10.0, 16.0 + (c % 41 - 20) / 10.0, 2.0))
    return np.array(rows, dtype=F)


SCENES = {"n10": lambda: random_spheres(10), "n64": lambda: random_spheres(64),
          "n65": lambda: random_spheres(65), "n200": lambda: random_spheres(200),
          "cluster": cluster_spheres,
          # two of the named scenes (scenes.py), as they come: tests/test_hit_cache.py
          "default10": lambda: scenes.default10().spheres, "lcg256": lambda: scenes.lcg256().spheres}


@functools.lru_cache(maxsize=None)
def _textures():
    tex, tw, th = scenes.load_floor()
    tex = np.array(tex, dtype=np.uint8).ravel()
    other = tex.copy()
    other[0::4] = 255 - other[0::4]  # slot 1: the floor with red inverted
    for t in (tex, other):
        t.setflags(write=False)
    return (tex, tw, th), (other, tw, th)


@functools.lru_cache(maxsize=None)
def _reference(sph_bytes, slot_bytes, cam, pose, width, height, s):
    """(height, width, 4) uint8: the oracle's s*width x s*height frame, box-filtered; computed
    once per distinct frame, shared, read-only."""
    import oracle
    spheres = np.frombuffer(sph_bytes, dtype=F).reshape(-1, 4)
    slots = np.frombuffer(slot_bytes, dtype=np.int32)
    floor, other = _textures()
    big = oracle.Oracle(s * width, s * height, spheres, *floor, cam, float(F(pose[0])),
                        float(F(pose[1])), scenes.FOV_H, scenes.FOV_V, sphere_tex=slots,
                        textures={1: other}).render(host_threads())
    if s == 1:
        out = big.reshape(height, width, 4).copy()
    else:
        sums = big.reshape(height, s, width, s, 4).astype(np.uint32).sum(axis=(1, 3))
        out = ((sums + s * s // 2) >> {2: 2, 4: 4}[s]).astype(np.uint8)
    out.setflags(write=False)
    return out


class Rig:
    """A world, the state of its next frame, and that frame's oracle."""

    def __init__(self, scene, geom, pose=POSE):
        import sfrt
        import torch
        self.sfrt = sfrt
        self.spheres = SCENES[scene]().copy()
        self.slots = np.zeros(self.spheres.shape[0], np.int32)
        self.cam, self.pose, self.s = CAM, pose, 1
        self.width, self.height, self.row0, self.rows, self.rays = GEOMS[geom]
        self.w = sfrt.World(0)
        for slot, t in enumerate(_textures()):
            self.w.load_texture(*t, slot=slot)
        self.w.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, self.rays)
        self.stream = torch.cuda.Stream()
        self.push()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.w.close()

    def push(self):
        self.w.set_size(self.width, self.height)
        self.w.set_camera(self.cam, self.pose[0], self.pose[1], scenes.FOV_H, scenes.FOV_V)
        self.w.set_spheres(self.spheres)
        self.w.set_sphere_textures(self.slots)

    def queue(self, stream=None):
        stream = self.stream if stream is None else stream
        pitch = 4 * self.width + 16
        buf = poisoned((self.rows, pitch), POISON)
        self.w.render_band(buf.data_ptr(), pitch, self.row0, self.rows, stream.cuda_stream)
        return buf

    def bytes_of(self, buf):
        got = buf.cpu().numpy()
        assert (got[:, 4 * self.width:] == POISON).all()
        return got[:, :4 * self.width].reshape(self.rows, self.width, 4)

    def want(self):
        ref = _reference(self.spheres.tobytes(), self.slots.tobytes(), tuple(float(c) for c in self.cam),
                         self.pose, self.width, self.height, self.s)
        return ref[self.row0:self.row0 + self.rows]

    def check_frame(self, what, stream=None):
        stream = self.stream if stream is None else stream
        buf = self.queue(stream)
        self.w.check(stream.cuda_stream)
        got = self.bytes_of(buf)
        bad = int(np.count_nonzero((got != self.want()).any(axis=-1)))
        assert bad == 0, f"{what}: {bad} pixels differ from the oracle"
        return got

    def stats(self):
        st = self.w.cull_cache_stats()
        return st["fills"], st["hits"]

    def tiles(self):
        return -(-self.width * self.s // (8 * self.rays)) * (-(-self.rows * self.s // 8))

    def cache_bytes(self):
        return self.tiles() * (BYTES_LIST if self.spheres.shape[0] > 64 else BYTES_INLINE)

    def three_frames(self, what, fills=0, hits=0):
        """Three identical launches from (fills, hits): culls for itself, fills, hits."""
        expect = [(fills, hits), (fills + 1, hits), (fills + 1, hits + 1)]
        for k in range(3):
            self.check_frame(f"{what}, frame {k + 1}")
            assert self.stats() == expect[k], (what, k)
        return expect[2]


@pytest.mark.parametrize("geom", ["72x20-r4", "40x9-r1", "40x9-r2", "40x9-r3"])
@pytest.mark.parametrize("scene", ["n10", "n64", "n65", "n200", "cluster"])
def test_three_identical_frames(built, scene, geom):
    with Rig(scene, geom) as r:
        assert r.w.cull_cache_stats() == {"fills": 0, "hits": 0, "bytes": 0}
        r.check_frame("frame 1")
        assert r.w.cull_cache_stats() == {"fills": 0, "hits": 0, "bytes": 0}
        r.check_frame("frame 2")
        assert r.w.cull_cache_stats() == {"fills": 1, "hits": 0, "bytes": r.cache_bytes()}
        r.check_frame("frame 3")
        r.check_frame("frame 4")
        assert r.w.cull_cache_stats() == {"fills": 1, "hits": 2, "bytes": r.cache_bytes()}


def cluster_cones(width=72, height=20, rays=4):
    """Per tile of the frame at rotation 0, from the host geometry in binary64: how many cluster
    spheres have their centre inside the tile's cone, and the smallest angle (degrees) between
    the cone and the ball of a cluster sphere, the ball's angular radius taken off.  In camera
    space pixel (i, j) looks along (h, v, 1), h = -fov_h + 2 fov_h i / width, v likewise; the
    axis looks through the tile's centre, columns past the frame's edge included, and the
    half-angle holds every (clamped) ray of the tile, as sphere_trace.hip's tile cones do."""
    fh, fv = float(scenes.FOV_H), float(scenes.FOV_V)
    cluster = cluster_spheres()[2:].astype(np.float64)
    rel = cluster[:, :3] - np.array(CAM)
    dist = np.linalg.norm(rel, axis=1)
    dirs = rel / dist[:, None]
    ball = np.degrees(np.arcsin(cluster[:, 3] / dist))
    tw = 8 * rays
    out = []

    def ray(i, j):
        d = np.array([-fh + 2.0 * fh * i / width, -fv + 2.0 * fv * j / height, 1.0])
        return d / np.linalg.norm(d)
    for ty in range(-(-height // 8)):
        for tx in range(-(-width // tw)):
            axis = ray(tx * tw + 0.5 * tw - 0.5, ty * 8 + 3.5)
            cols = [min(tx * tw + c, width - 1) for c in (0, tw - 1)]
            rows = [min(ty * 8 + r, height - 1) for r in (0, 7)]
            half = max(np.degrees(np.arccos(min(1.0, float(ray(i, j) @ axis)))) for i in cols for j in rows)
            off = np.degrees(np.arccos(np.clip(dirs @ axis, -1.0, 1.0)))
            out.append((int(np.count_nonzero(off < half - 1.0)), float((off - half - ball).min())))
    return out


def test_cluster_overflows_at_rotation_zero(built):
    """The pose the cluster scene is laid out for.  A sphere whose centre lies inside a tile's
    cone is at distance 0 from it and is never culled, so a tile with more than 64 such centres
    (counted a degree inside the cone, far above binary32's error in it) overflows its wave's
    list: the frame's middle tile (tile 4 of the 3 x 3) does, with all 150.  A tile whose cone stays more than 10
    degrees clear of every cluster ball (the cull margin 0.026 is 0.1 degrees at the cluster's
    distance) culls all of them and keeps a list: the last column's tiles do.  Both kinds of
    record are therefore stored and read in this frame."""
    cones = cluster_cones()
    inside = [n for n, _ in cones]
    clear = [c for _, c in cones]
    assert inside[4] == 150, inside
    assert all(clear[t] > 10.0 for t in (2, 5, 8)), clear
    with Rig("cluster", "72x20-r4", pose=(0.0, 0.0)) as r:
        r.three_frames("cluster")


def _ulp(r):
    c = list(r.cam)
    c[1] = float(np.nextafter(F(c[1]), F(np.inf)))
    r.cam = tuple(c)


def _radius(r):
    r.spheres[min(3, len(r.spheres) - 1), 3] *= F(1.05)


def _centre(r):
    r.spheres[len(r.spheres) // 2, 0] += F(0.5)


def _reorder(r):
    r.spheres[[1, 2]] = r.spheres[[2, 1]]


CHANGES = {"camera position by one ulp": _ulp, "one radius": _radius, "one centre": _centre,
           "spheres reordered": _reorder}


@pytest.mark.parametrize("geom", ["72x20-r4", "40x9-r2"])
@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_changes_miss_then_refill(built, scene, geom):
    """After each change of an input of the cull the first frame is the oracle's and no hit,
    the second fills, the third hits."""
    with Rig(scene, geom) as r:
        fills, hits = r.three_frames("start")
        for what, change in CHANGES.items():
            change(r)
            r.push()
            fills, hits = r.three_frames(what, fills, hits)
        assert r.w.ray_cache_stats()["fills"] == 1  # the directions were never refilled


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_cull_option_off_and_on(built, scene):
    with Rig(scene, "72x20-r4") as r:
        fills, hits = r.three_frames("start")
        for value in (0, 1):
            r.w.set_option(r.sfrt.SFRT_OPT_CULL, value)
            fills, hits = r.three_frames(f"cull {value}", fills, hits)


@pytest.mark.parametrize("geom", ["72x20-r4", "40x9-r2"])
@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_supersampling_two(built, scene, geom):
    with Rig(scene, geom) as r:
        fills, hits = r.three_frames("1x")
        r.s = 2
        r.w.set_option(r.sfrt.SFRT_OPT_SUPERSAMPLE, 2)
        r.three_frames("2x", fills, hits)
        assert r.w.cull_cache_stats()["bytes"] == r.cache_bytes()


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_texture_slot_change_keeps_hitting(built, scene):
    with Rig(scene, "72x20-r4") as r:
        a = r.check_frame("frame 1")
        r.check_frame("frame 2")
        r.check_frame("frame 3")
        assert r.stats() == (1, 1)
        r.slots = (np.arange(r.spheres.shape[0]) % 2).astype(np.int32)
        r.push()
        r.check_frame("other slots")
        assert r.stats() == (1, 2)
        r.slots[:] = 1
        r.push()
        b = r.check_frame("every sphere in slot 1")
        assert r.stats() == (1, 3)
        assert not np.array_equal(a, b)  # the other texture shows


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_two_streams_a_chain_each(built, scene):
    import torch
    with Rig(scene, "72x20-r4") as r:
        streams = [r.stream, torch.cuda.Stream()]
        for k in range(8):
            r.check_frame(f"frame {k}", streams[k % 2])
        assert r.w.cull_cache_stats() == {"fills": 2, "hits": 4, "bytes": 2 * r.cache_bytes()}


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_band_of_some_rows(built, scene):
    with Rig(scene, "band") as r:
        r.three_frames("rows 8..19 of 40")
        assert r.w.cull_cache_stats()["bytes"] == r.cache_bytes()


def test_budget_refuses_the_cull_cache(built):
    """404x236 at 16x8 tiles: 1.14 MiB of directions and 0.39 MiB of cull cache.  A budget of
    1 MiB takes neither, but for the cull cache the limit is what is left beside the
    directions."""
    with Rig("n10", "40x9-r2") as r:
        r.width, r.height, r.row0, r.rows = 404, 236, 0, 236
        r.push()
        assert r.cache_bytes() == 26 * 30 * 528
        r.w.set_option(r.sfrt.SFRT_OPT_RAY_CACHE_MB, 1)
        for k in range(3):
            r.check_frame(f"budget 1, frame {k}")
        assert r.w.cull_cache_stats() == {"fills": 0, "hits": 0, "bytes": 0}
        r.w.set_option(r.sfrt.SFRT_OPT_RAY_CACHE_MB, 2)
        for k in range(3):
            r.check_frame(f"budget 2, frame {k}")
        assert r.w.cull_cache_stats() == {"fills": 1, "hits": 2, "bytes": r.cache_bytes()}
        r.w.set_option(r.sfrt.SFRT_OPT_RAY_CACHE_MB, 1)  # below what is held: everything goes
        assert r.w.cull_cache_stats()["bytes"] == 0 and r.w.ray_cache_stats()["bytes"] == 0
        r.w.set_option(r.sfrt.SFRT_OPT_RAY_CACHE_MB, 0)
        for k in range(3):
            r.check_frame(f"off, frame {k}")
        assert r.w.cull_cache_stats() == {"fills": 1, "hits": 2, "bytes": 0}


def test_twenty_cached_frames_320x240_lcg64(built):
    """The uncached frame, the filling one, then 20 frames queued back to back from the cache and
    one sfrt_world_check: every hash is the uncached frame's, which is the oracle's."""
    import oracle
    import sfrt
    import torch
    w, h = 320, 240
    scene = scenes.lcg64().posed(*POSE)
    tex, tw, th = scenes.load_floor()
    want = oracle.Oracle.from_scene(scene, w, h, tex, tw, th).render(host_threads())
    stream = torch.cuda.Stream()
    with sfrt.World(0) as world:
        world.load_texture(tex, tw, th)
        world.set_scene(scene, w, h)
        bufs = []
        for _ in range(22):
            buf = poisoned((h, 4 * w), POISON)
            world.render_band(buf.data_ptr(), 4 * w, 0, h, stream.cuda_stream)
            bufs.append(buf)
        world.check(stream.cuda_stream)
        assert world.cull_cache_stats()["fills"] == 1 and world.cull_cache_stats()["hits"] == 20
    hashes = [hashlib.sha256(b.cpu().numpy().tobytes()).hexdigest() for b in bufs]
    assert hashes[0] == hashlib.sha256(want.tobytes()).hexdigest()
    assert all(x == hashes[0] for x in hashes[1:]), hashes
