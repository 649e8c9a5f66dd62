"""The hit cache (csrc/sfrt_raycache.h HitRec, ChainCaches; DESIGN.md 5 "Hit cache"): on top of the cull
cache and under its key, a chain stores where each ray's march ended and on which sphere, and
while the key stays its launches do not march: they shade from the stored results with the
textures and texture slots of the moment.

Every frame is compared byte for byte with the CPU oracle of its own state, and
sfrt_world_hit_cache_stats is asserted after every frame.  Shapes, scenes and the rig are
tests/test_cull_cache.py's: 72x20 at four pixels per lane (2 1/4 x 2 1/2 tiles: clamped edge lanes
both ways, tile_x > 0) and 40x9 at one, two and three; 10 and 64 spheres run the kernels whose
records travel in the arguments, 65, 200 and the overflowing `cluster` the device-ring ones.

The texel status.  shade_texel's index is (a fraction in [0, 1)) * width, truncated, plus the same
for the row: it leaves the texture only if the binary32 product rounds up to the size itself, and
tests/test_hit_cache_texel_bound.py shows that for no size a texture can have it does.  So no
frame raises SFRT_E_TEXEL's bit from either kind of launch; test_one_row_textures_same_status runs
the shapes nearest to it -- one-row textures of widths that are no power of two under spheres of
radius <= 0.5 -- and asserts the same status, and the same bytes, from a reading launch, from a
marching launch of a world with SFRT_OPT_HIT_CACHE_MB 0, and from the oracle.
"""
import functools
import hashlib

import numpy as np
import pytest

import scenes
from conftest import host_threads, poisoned
from test_cull_cache import CAM, F, POISON, POSE, SCENES, Rig, _textures

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(sph_bytes, slot_bytes, cam, pose, width, height, s, tex_key):
    """As test_cull_cache._reference, with the two slots' textures of the moment (tex_key indexes
    TEXTURES); computed once per distinct frame, shared, read-only."""
    import oracle
    spheres = np.frombuffer(sph_bytes, dtype=F).reshape(-1, 4)
    slots = np.frombuffer(slot_bytes, dtype=np.int32)
    floor, other = TEXTURES[tex_key[0]](), TEXTURES[tex_key[1]]()
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


@functools.lru_cache(maxsize=None)
def _green():
    """The floor with green inverted: new texels of the same size."""
    tex, tw, th = _textures()[0]
    t = tex.copy()
    t[1::4] = 255 - t[1::4]
    t.setflags(write=False)
    return t, tw, th


@functools.lru_cache(maxsize=None)
def _small():
    """A 48x20 texture: another size (neither a power of two nor square)."""
    tw, th = 48, 20
    k = np.arange(tw * th, dtype=np.uint32)
    t = np.stack([(k * 7) & 255, (k * 13 + 5) & 255, (k * 3 + 90) & 255, np.full_like(k, 255)],
                 axis=1).astype(np.uint8).ravel()
    t.setflags(write=False)
    return t, tw, th


@functools.lru_cache(maxsize=None)
def _one_row(tw):
    """A tw x 1 texture."""
    k = np.arange(tw, dtype=np.uint32)
    t = np.stack([(k * 5 + 1) & 255, (k * 11 + 7) & 255, (k * 17 + 3) & 255, np.full_like(k, 255)],
                 axis=1).astype(np.uint8).ravel()
    t.setflags(write=False)
    return t, tw, 1


ONE_ROW_WIDTHS = (3, 7, 100, 1000, 65535)
TEXTURES = {"floor": lambda: _textures()[0], "other": lambda: _textures()[1], "green": _green,
            "small": _small, **{f"row{tw}": functools.partial(_one_row, tw) for tw in ONE_ROW_WIDTHS}}


class HitRig(Rig):
    """test_cull_cache.Rig with the textures of the moment in the oracle and the hit cache's stats."""

    def __init__(self, scene, geom, pose=POSE):
        self.tex_key = ("floor", "other")
        super().__init__(scene, geom, pose)

    def load(self, slot, name):
        self.w.load_texture(*TEXTURES[name](), slot=slot)
        key = list(self.tex_key)
        key[slot] = name
        self.tex_key = tuple(key)

    def want(self):
        ref = _reference(self.spheres.tobytes(), self.slots.tobytes(), tuple(float(c) for c in self.cam),
                         self.pose, self.width, self.height, self.s, self.tex_key)
        return ref[self.row0:self.row0 + self.rows]

    def hit_bytes(self):
        return self.tiles() * self.rays * 64 * 16

    def hstats(self):
        st = self.w.hit_cache_stats()
        return st["fills"], st["hits"], st["bytes"]

    def frames(self, what, fills=0, hits=0, held=0, count=3):
        """`count` identical launches of a new key from (fills, hits): the first runs what it would
        without a hit cache (and frees nothing: `held` bytes stay), the second stores, the others
        read.  Every frame is the oracle's."""
        for k in range(count):
            self.check_frame(f"{what}, frame {k + 1}")
            want = ((fills, hits, held) if k == 0 else
                    (fills + 1, hits + k - 1, self.hit_bytes()))
            assert self.hstats() == want, (what, k)
        return fills + 1, hits + count - 2


FIVE_FRAMES = [(scene, geom) for geom in ("72x20-r4", "40x9-r1", "40x9-r2", "40x9-r3")
               for scene in ("n10", "n64", "n65", "n200", "cluster")]
# ... and two named scenes with an aux band (sfrt_world_render_band_aux) after the third frame: a
# launch that takes no part in the caches, between two reading launches
AUX_BETWEEN = [("default10", "72x20-r4"), ("lcg256", "72x20-r4")]


def _aux_band(r):
    """One render_band_aux call of r's state on r's stream: its colour bytes, nothing else kept."""
    import torch
    pitch = 4 * r.width + 16
    buf = poisoned((r.rows, pitch), POISON)
    depth = torch.empty((r.rows, r.width), dtype=torch.float32, device="cuda")
    r.w.render_band_aux(buf.data_ptr(), pitch, r.row0, r.rows, r.stream.cuda_stream,
                        depth=(depth.data_ptr(), 4 * r.width))
    r.w.check(r.stream.cuda_stream)
    return r.bytes_of(buf)


@pytest.mark.parametrize("scene,geom", FIVE_FRAMES + AUX_BETWEEN,
                         ids=[f"{scene}-{geom}" for scene, geom in FIVE_FRAMES + AUX_BETWEEN])
def test_five_identical_frames(built, scene, geom):
    with HitRig(scene, geom) as r:
        assert r.w.get_option(r.sfrt.SFRT_OPT_HIT_CACHE_MB) == 512
        assert r.hstats() == (0, 0, 0)
        if (scene, geom) in AUX_BETWEEN:
            first = r.check_frame("frame 1")
            for k, want in ((2, (1, 0, r.hit_bytes())), (3, (1, 1, r.hit_bytes()))):
                r.check_frame(f"frame {k}")
                assert r.hstats() == want, k
            before = r.hstats(), r.stats(), r.w.ray_cache_stats()
            assert before[:2] == ((1, 1, r.hit_bytes()), (1, 1)) and before[2]["cached_frames"] == 2
            aux = _aux_band(r)
            assert (r.hstats(), r.stats(), r.w.ray_cache_stats()) == before  # no trace of it
            last = r.check_frame("the frame after the aux band")
            assert r.hstats() == (1, 2, r.hit_bytes())
            assert r.stats() == (1, 2) and r.w.ray_cache_stats()["cached_frames"] == 3
            assert np.array_equal(aux, first) and np.array_equal(last, first)
            return
        r.frames("five frames", count=5)
        assert r.hstats() == (1, 3, r.hit_bytes())
        # each reading launch counts as a cached frame and a cull-cache hit, as without the hit cache
        assert r.stats() == (1, 3) and r.w.ray_cache_stats()["cached_frames"] == 4


def test_cluster_at_rotation_zero(built):
    """The pose at which the cluster scene's middle tile overflows its list
    (test_cull_cache.test_cluster_overflows_at_rotation_zero): its full-list march is stored and
    read like any other."""
    with HitRig("cluster", "72x20-r4", pose=(0.0, 0.0)) as r:
        r.frames("cluster", count=4)


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


def _basis(r):
    r.pose = (r.pose[0] + 0.05, r.pose[1])


# (the change, whether it refills the directions: then the caches on them are freed first)
CHANGES = {"camera position by one ulp": (_ulp, False), "one radius": (_radius, False),
           "one centre": (_centre, False), "spheres reordered": (_reorder, False),
           "view basis": (_basis, True)}


@pytest.mark.parametrize("what", list(CHANGES))
@pytest.mark.parametrize("geom", ["72x20-r4", "40x9-r2"])
@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_key_change_misses_then_refills(built, scene, geom, what):
    """After a change of an input of the march the first frame is the new state's oracle and no
    hit, the second stores again, the third reads."""
    change, _ = CHANGES[what]
    with HitRig(scene, geom) as r:
        fills, hits = r.frames("start", count=4)
        change(r)
        r.push()
        fills, hits = r.frames(what, fills, hits, held=r.hit_bytes(), count=4)
        assert (fills, hits) == (2, 4)


@pytest.mark.parametrize("geom", ["72x20-r4", "40x9-r2"])
@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_texture_changes_keep_hitting(built, scene, geom):
    """What the key does not hold: new texels in a slot, a texture of another size in a slot, other
    slots for the spheres.  Every such frame is a hit and the oracle's frame of the new state."""
    with HitRig(scene, geom) as r:
        a = r.check_frame("frame 1")
        r.check_frame("frame 2")
        r.check_frame("frame 3")
        assert r.hstats() == (1, 1, r.hit_bytes())
        r.load(0, "green")
        b = r.check_frame("new texels in slot 0")
        assert r.hstats() == (1, 2, r.hit_bytes()) and not np.array_equal(a, b)
        r.load(0, "small")
        c = r.check_frame("a 48x20 texture in slot 0")
        assert r.hstats() == (1, 3, r.hit_bytes()) and not np.array_equal(b, c)
        r.slots = (np.arange(r.spheres.shape[0]) % 2).astype(np.int32)
        r.push()
        r.check_frame("every other sphere in slot 1")
        assert r.hstats() == (1, 4, r.hit_bytes())
        r.load(1, "green")
        r.slots[:] = 1
        r.push()
        r.check_frame("every sphere in slot 1, new texels there")
        assert r.hstats() == (1, 5, r.hit_bytes())
        assert r.w.ray_cache_stats()["fills"] == 1 and r.stats() == (1, 5)


def _status_and_frame(r):
    buf = r.queue()
    try:
        r.w.check(r.stream.cuda_stream)
        code = 0
    except r.sfrt.SfrtError as e:
        code = e.code
    return code, r.bytes_of(buf)


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_one_row_textures_same_status(built, scene):
    """The texture shapes nearest to an index outside the texture (the module's docstring): after
    each texture change the reading launch leaves the status and the bytes that a marching launch
    of a world without a hit cache leaves, and the oracle's frame when the status is clear."""
    with HitRig(scene, "72x20-r4") as r, HitRig(scene, "72x20-r4") as m:
        m.w.set_option(m.sfrt.SFRT_OPT_HIT_CACHE_MB, 0)
        for rig in (r, m):
            rig.spheres[2:, 3] = F(0.5)   # every sphere but the two around the camera
            rig.spheres[2::3, 3] = F(0.25)
            rig.push()
            for k in range(3):
                rig.check_frame(f"frame {k}")
        assert r.hstats() == (1, 1, r.hit_bytes()) and m.hstats() == (0, 0, 0)
        for n, tw in enumerate(ONE_ROW_WIDTHS):
            for rig in (r, m):
                rig.load(0, f"row{tw}")
            got, frame = _status_and_frame(r)
            want, marched = _status_and_frame(m)
            assert got == want, (tw, got, want)
            assert np.array_equal(frame, marched), tw
            if want == 0:
                assert np.array_equal(frame, r.want()), tw
            assert r.hstats() == (1, 2 + n, r.hit_bytes()) and m.hstats() == (0, 0, 0)


@pytest.mark.parametrize("geom", ["72x20-r4", "40x9-r2"])
@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_supersampling_two(built, scene, geom):
    with HitRig(scene, geom) as r:
        fills, hits = r.frames("1x")
        held = r.hit_bytes()
        r.s = 2
        r.w.set_option(r.sfrt.SFRT_OPT_SUPERSAMPLE, 2)
        # (the sample grid is a new view: its fill of the directions frees the caches on them)
        r.check_frame("2x, frame 1")
        assert r.hstats() == (fills, hits, held)
        r.check_frame("2x, frame 2")
        assert r.hstats() == (fills + 1, hits, r.hit_bytes())  # per sample: four times the records
        r.check_frame("2x, frame 3")
        r.check_frame("2x, frame 4")
        assert r.hstats() == (fills + 1, hits + 2, r.hit_bytes()) and r.hit_bytes() >= held


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_band_of_some_rows(built, scene):
    with HitRig(scene, "band") as r:
        r.frames("rows 8..19 of 40", count=4)


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_two_streams_a_chain_each(built, scene):
    import torch
    with HitRig(scene, "72x20-r4") as r:
        streams = [r.stream, torch.cuda.Stream()]
        for k in range(8):
            r.check_frame(f"frame {k}", streams[k % 2])
            done = (k + 1) // 2, (k + 2) // 2  # launches so far on stream 1, on stream 0
            fills = sum(1 for n in done if n >= 2)
            hits = sum(max(0, n - 2) for n in done)
            assert r.hstats() == (fills, hits, fills * r.hit_bytes()), k
        assert r.hstats() == (2, 4, 2 * r.hit_bytes())


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_cull_option_off_and_on(built, scene):
    with HitRig(scene, "72x20-r4") as r:
        fills, hits = r.frames("start")
        for value in (0, 1):
            r.w.set_option(r.sfrt.SFRT_OPT_CULL, value)
            fills, hits = r.frames(f"cull {value}", fills, hits, held=r.hit_bytes())


def test_budgets(built):
    """404x236 at 16x8 tiles: 26 x 30 tiles, 1.52 MiB of hit records."""
    with HitRig("n10", "40x9-r2") as r:
        r.width, r.height, r.row0, r.rows = 404, 236, 0, 236
        r.push()
        assert r.hit_bytes() == 26 * 30 * 2 * 64 * 16
        r.w.set_option(r.sfrt.SFRT_OPT_HIT_CACHE_MB, 1)  # too small: refused, the cull cache as without
        for k in range(4):
            r.check_frame(f"hit budget 1, frame {k}")
            assert r.hstats() == (0, 0, 0)
        assert r.w.cull_cache_stats() == {"fills": 1, "hits": 2, "bytes": r.cache_bytes()}
        r.w.set_option(r.sfrt.SFRT_OPT_HIT_CACHE_MB, 2)  # enough: the next launch of the key stores
        r.check_frame("hit budget 2, frame 0")
        assert r.hstats() == (1, 0, r.hit_bytes())
        r.check_frame("hit budget 2, frame 1")
        assert r.hstats() == (1, 1, r.hit_bytes())
        r.w.set_option(r.sfrt.SFRT_OPT_HIT_CACHE_MB, 1)  # lowered below what is held: freed
        assert r.hstats() == (1, 1, 0)
        assert r.w.cull_cache_stats()["bytes"] == r.cache_bytes()  # the other caches stay
        r.check_frame("lowered")
        assert r.hstats() == (1, 1, 0) and r.stats() == (1, 5)
        with pytest.raises(r.sfrt.SfrtError):
            r.w.set_option(r.sfrt.SFRT_OPT_HIT_CACHE_MB, -1)
        assert r.w.get_option(r.sfrt.SFRT_OPT_HIT_CACHE_MB) == 1
        r.w.set_option(r.sfrt.SFRT_OPT_HIT_CACHE_MB, 0)  # off
        for k in range(3):
            r.check_frame(f"off, frame {k}")
        assert r.hstats() == (1, 1, 0) and r.stats() == (1, 8)
        r.w.set_option(r.sfrt.SFRT_OPT_HIT_CACHE_MB, 512)
        r.check_frame("on again, frame 0")
        r.check_frame("on again, frame 1")
        assert r.hstats() == (2, 2, r.hit_bytes())
        r.w.set_option(r.sfrt.SFRT_OPT_RAY_CACHE_MB, 0)  # everything off, the hit cache with the rest
        assert r.hstats() == (2, 2, 0)
        for k in range(3):
            r.check_frame(f"ray cache 0, frame {k}")
        assert r.hstats() == (2, 2, 0) and r.w.ray_cache_stats()["bytes"] == 0


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_row_costs_stay_the_last_marching_launch(built, scene):
    with HitRig(scene, "72x20-r4") as r:
        r.check_frame("frame 1")
        r.check_frame("frame 2")  # the last launch that marches (it stores the results)
        row0, costs = r.w.row_costs()
        assert costs.size == r.rows and costs.max() > 0
        for k in range(3):
            r.check_frame(f"reading launch {k}")
            again0, again = r.w.row_costs()
            assert again0 == row0 and np.array_equal(again, costs)
        assert r.hstats() == (1, 3, r.hit_bytes())


@pytest.mark.parametrize("scene", ["n10", "n65"])
def test_adaptive_order_resumes_after_reading_launches(built, scene):
    """A camera that moves after a run of reading launches marches again, in the adaptive order
    continued from the last marching launch: frames equal the oracle and those of a world with
    SFRT_OPT_TILE_ORDER 0, which takes no part in any of this."""
    with HitRig(scene, "72x20-r4") as r, HitRig(scene, "72x20-r4") as plain:
        plain.w.set_option(plain.sfrt.SFRT_OPT_TILE_ORDER, 0)
        r.frames("rest", count=5)
        for step in range(4):
            for rig in (r, plain):
                rig.cam = (CAM[0] + 0.03 * (step + 1), CAM[1], CAM[2] + 0.02 * (step + 1))
                rig.push()
            a = r.check_frame(f"walking, frame {step}")
            b = plain.check_frame(f"walking row-major, frame {step}")
            assert np.array_equal(a, b)
            assert r.hstats() == (1, 3, r.hit_bytes())
        for rig in (r, plain):
            rig.cam = (CAM[0] + 0.2, CAM[1], CAM[2] + 0.1)
            rig.push()
        plain.check_frame("rest again, row-major")
        r.frames("rest again", 1, 3, held=r.hit_bytes(), count=4)
        assert plain.hstats() == (0, 0, 0)


def test_twenty_cached_frames_320x240_lcg64(built):
    """The uncached frame, the storing one, then 20 frames through submit_frame from the stored
    results: every frame is the oracle's."""
    import oracle
    import sfrt
    w, h = 320, 240
    scene = scenes.lcg64().posed(*POSE)
    tex, tw, th = scenes.load_floor()
    want = hashlib.sha256(oracle.Oracle.from_scene(scene, w, h, tex, tw, th).render(host_threads()).tobytes()).hexdigest()
    with sfrt.World(0) as world:
        world.load_texture(tex, tw, th)
        world.set_scene(scene, w, h)
        frames = [sfrt.HostFrame(w * h * 4) for _ in range(2)]
        try:
            for k in range(22):
                out = frames[k % 2]
                world.wait_frame(world.submit_frame(out))
                assert hashlib.sha256(out.array[:w * h * 4].tobytes()).hexdigest() == want, k
        finally:
            stats = world.hit_cache_stats()
            for fr in frames:
                fr.free()
        assert stats == {"fills": 1, "hits": 20, "bytes": 30 * 20 * 2 * 64 * 16}
