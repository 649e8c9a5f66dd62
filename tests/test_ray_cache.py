"""SFRT_OPT_RAY_CACHE_MB: a tile-order chain caches the primary ray directions of a view whose
rotation, fields of view, frame / band geometry, supersampling factor and tile shape stay put.

Every frame is compared byte for byte with the oracle (the box-filtered S*W x S*H frame when
supersampled, as tests/test_supersample.py), and sfrt_world_ray_cache_stats tells a frame
served from the cache from one where it never engaged.  Frames are 72x20 and the band
row0 = 8, rows = 12 of 72x40: partial tiles in both axes at every tile width (8, 16, 24, 32).
default10 runs the kernel-argument kernels, lcg256 the culled-list kernels.

A subset stride other than 1 reaches the kernels through update_image only, which joins no
chain and is never cached; that key field is covered on the host (test_ray_cache_policy.py).
"""
import functools

import numpy as np
import pytest

import scenes
from conftest import host_threads, poisoned

pytestmark = pytest.mark.gpu

POSES = {"default10": (0.7, 0.3), "lcg256": (2.0, 0.4)}
GEOMS = {"full": (72, 20, 0, 20), "band": (72, 40, 8, 12)}  # width, height, row0, rows
POISON = 0xA5


@functools.lru_cache(maxsize=None)
def _floor(variant=0):
    tex, tw, th = scenes.load_floor()
    tex = np.array(tex, dtype=np.uint8).ravel()
    if variant:
        tex[0::4] = 255 - tex[0::4]  # another texture: red inverted
    tex.setflags(write=False)
    return tex, tw, th


def _scene(name, pose=None, cam_pos=None, drop=0):
    sc = scenes.SCENES[name]().posed(*(POSES[name] if pose is None else pose))
    if cam_pos is not None:
        sc.cam_pos = tuple(cam_pos)
    if drop:  # other spheres: every radius 5 % larger
        sc.spheres = sc.spheres.copy()
        sc.spheres[:, 3] *= np.float32(1.05)
    return sc


@functools.lru_cache(maxsize=None)
def reference(name, s, width, height, pose=None, cam_pos=None, drop=0, tex=0):
    """(height, width, 4) uint8: the oracle's s*width x s*height frame, box-filtered (computed
    once per distinct frame, shared, read-only)."""
    import oracle
    big = oracle.Oracle.from_scene(_scene(name, pose, cam_pos, drop), s * width, s * height,
                                   *_floor(tex)).render(host_threads())
    if s == 1:
        out = big.reshape(height, width, 4).copy()
    else:
        sums = big.reshape(height, s, width, s, 4).astype(np.uint32).sum(axis=(1, 3))
        out = ((sums + s * s // 2) >> {2: 2, 4: 4}[s]).astype(np.uint8)
    out.setflags(write=False)
    return out


class Rig:
    """A world plus what the reference of its next frame needs."""

    def __init__(self, name, s=1, rays=0, geom="full", budget=None):
        import sfrt
        import torch
        self.sfrt = sfrt
        self.name, self.s = name, s
        self.width, self.height, self.row0, self.rows = GEOMS.get(geom, geom)
        self.pose, self.cam_pos, self.drop, self.tex = None, None, 0, 0
        self.w = sfrt.World(0)
        self.w.load_texture(*_floor(0))
        self.w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
        self.w.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
        if budget is not None:
            self.w.set_option(sfrt.SFRT_OPT_RAY_CACHE_MB, budget)
        self.stream = torch.cuda.Stream()
        self.push()

    def close(self):
        self.w.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def push(self):
        self.w.set_scene(_scene(self.name, self.pose, self.cam_pos, self.drop), self.width,
                         self.height)

    def frame(self, stream=None):
        """One render_band of the rig's band on `stream`; the (rows, width, 4) bytes."""
        stream = self.stream if stream is None else stream
        pitch = 4 * self.width + 16
        buf = poisoned((self.rows, pitch), POISON)
        self.w.render_band(buf.data_ptr(), pitch, self.row0, self.rows, stream.cuda_stream)
        self.w.check(stream.cuda_stream)
        got = buf.cpu().numpy()
        assert (got[:, 4 * self.width:] == POISON).all()
        return got[:, :4 * self.width].reshape(self.rows, self.width, 4)

    def want(self):
        ref = reference(self.name, self.s, self.width, self.height, self.pose, self.cam_pos,
                        self.drop, self.tex)
        return ref[self.row0:self.row0 + self.rows]

    def check_frame(self, what, stream=None):
        got = self.frame(stream)
        bad = int(np.count_nonzero((got != self.want()).any(axis=-1)))
        assert bad == 0, f"{what}: {bad} pixels differ from the oracle"
        return got

    def stats(self):
        st = self.w.ray_cache_stats()
        return st["cached_frames"], st["fills"]

    def held(self):
        return self.w.ray_cache_stats()["bytes"]


def cache_bytes(width, rows, s, rays):
    tiles = -(-width * s // (8 * rays)) * (-(-rows * s // 8))
    return tiles * rays * 64 * 12


@pytest.mark.parametrize("geom", ["full", "band"])
@pytest.mark.parametrize("rays", [1, 2, 3, 4])
@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("name", ["default10", "lcg256"])
def test_four_frames_of_one_pose(built, name, s, rays, geom):
    """Frame 1 renders as ever, frame 2 fills and reads, frames 3 and 4 read; every frame is
    the oracle's and the frame of a world with the option at 0."""
    with Rig(name, s, rays, geom) as on, Rig(name, s, rays, geom, budget=0) as off:
        assert on.w.get_option(on.sfrt.SFRT_OPT_RAY_CACHE_MB) == 512
        expect = [(0, 0), (1, 1), (2, 1), (3, 1)]
        for k in range(4):
            a = on.check_frame(f"frame {k + 1}")
            b = off.check_frame(f"frame {k + 1}, cache off")
            assert np.array_equal(a, b)
            assert on.stats() == expect[k], k
            assert off.stats() == (0, 0) and off.held() == 0
        assert on.held() == cache_bytes(on.width, on.rows, s, rays)


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("name", ["default10", "lcg256"])
def test_position_change_keeps_the_cache(built, name, s):
    """Walking: the position changes every frame, the rotation stays -- served from the cache,
    and each frame is the oracle's at the new position."""
    with Rig(name, s, 2, "band") as r:
        r.check_frame("first")
        r.check_frame("second")
        assert r.stats() == (1, 1)
        for k, pos in enumerate([(0.5, 0.2, -0.3), (0.9, -0.4, 0.6), (0.0, 0.0, 0.0)]):
            r.cam_pos = pos
            r.push()
            r.check_frame(f"position {pos}")
            assert r.stats() == (2 + k, 1)


@pytest.mark.parametrize("name", ["default10", "lcg256"])
def test_key_changes_drop_or_rebuild(built, name):
    """A rotation change, rotating back, and a change of frame size, band, supersampling
    factor or tile shape: none reads directions of another key, every frame is the oracle's."""
    with Rig(name, 1, 2, "band") as r:
        sfrt_opt = r.sfrt
        r.check_frame("first")
        r.check_frame("second")
        assert r.stats() == (1, 1)
        r.pose = (POSES[name][0] + 0.25, POSES[name][1])
        r.push()
        r.check_frame("rotated")
        assert r.stats() == (1, 1)  # a miss: today's kernel
        r.pose = None
        r.push()
        r.check_frame("rotated back")
        assert r.stats() == (2, 1)  # the cache of the first rotation still serves
        r.pose = (POSES[name][0] + 0.25, POSES[name][1])
        r.push()
        r.check_frame("rotated again")
        r.check_frame("rotated again, second frame")
        assert r.stats() == (3, 2)  # rebuilt for the new rotation
        r.pose = None
        r.push()
        r.check_frame("back after the rebuild")
        assert r.stats() == (3, 2)  # the old directions are gone
        steps = [
            ("frame size", lambda: setattr(r, "height", 44)),
            ("band", lambda: (setattr(r, "row0", 16), setattr(r, "rows", 20))),
            ("supersample", lambda: (setattr(r, "s", 2),
                                     r.w.set_option(sfrt_opt.SFRT_OPT_SUPERSAMPLE, 2))),
            ("tile shape", lambda: r.w.set_option(sfrt_opt.SFRT_OPT_RAYS_PER_LANE, 3)),
        ]
        cached, fills = r.stats()
        for what, change in steps:
            change()
            r.push()
            r.check_frame(what)
            assert r.stats() == (cached, fills), what
            r.check_frame(what + ", second frame")
            cached, fills = cached + 1, fills + 1
            assert r.stats() == (cached, fills), what
            r.check_frame(what + ", third frame")
            cached += 1
            assert r.stats() == (cached, fills), what


def test_turning_camera_never_fills(built):
    with Rig("default10", 1, 2, "full") as r:
        for k in range(6):
            r.pose = (0.7 + 0.004 * k, 0.3)
            r.push()
            r.check_frame(f"turn {k}")
        assert r.stats() == (0, 0) and r.held() == 0


@pytest.mark.parametrize("name", ["default10", "lcg256"])
def test_two_streams_alternating(built, name):
    """Two streams on one world: each stream's chain fills its own cache."""
    import torch
    with Rig(name, 1, 2, "band") as r:
        streams = [r.stream, torch.cuda.Stream()]
        for k in range(8):
            r.check_frame(f"frame {k}", streams[k % 2])
        assert r.stats() == (6, 2)
        assert r.held() == 2 * cache_bytes(r.width, r.rows, 1, 2)


def test_budget_below_the_cache_size(built):
    """404x236 at 16x8 tiles needs 26 * 30 * 1536 B = 1.14 MiB: a budget of 1 MiB refuses the
    fill, and the frames are the same bytes; 2 MiB takes it; lowering the budget frees it."""
    assert cache_bytes(404, 236, 1, 2) > 1 << 20
    with Rig("default10", 1, 2, (404, 236, 0, 236), budget=1) as r:
        frames = [r.check_frame(f"budget 1, frame {k}") for k in range(3)]
        assert r.stats() == (0, 0) and r.held() == 0
        r.w.set_option(r.sfrt.SFRT_OPT_RAY_CACHE_MB, 2)
        frames += [r.check_frame(f"budget 2, frame {k}") for k in range(2)]
        assert r.stats() == (2, 1) and r.held() == cache_bytes(404, 236, 1, 2)
        r.w.set_option(r.sfrt.SFRT_OPT_RAY_CACHE_MB, 1)
        assert r.held() == 0
        frames += [r.check_frame(f"budget 1 again, frame {k}") for k in range(3)]
        assert r.stats() == (2, 1) and r.held() == 0
        assert all(np.array_equal(f, frames[0]) for f in frames)
        with pytest.raises(r.sfrt.SfrtError):
            r.w.set_option(r.sfrt.SFRT_OPT_RAY_CACHE_MB, -1)
        assert r.w.get_option(r.sfrt.SFRT_OPT_RAY_CACHE_MB) == 1


@pytest.mark.parametrize("name", ["default10", "lcg256"])
def test_spheres_and_textures_are_not_frozen(built, name):
    """Between cached frames the spheres and the texture change: the frames change as the
    oracle says, still served from the cache."""
    with Rig(name, 1, 2, "band") as r:
        r.check_frame("first")
        a = r.check_frame("second")
        r.drop = 1
        r.push()
        b = r.check_frame("larger spheres")
        r.tex = 1
        r.w.load_texture(*_floor(1))
        c = r.check_frame("another texture")
        assert r.stats() == (3, 1)
        assert not np.array_equal(a, b) and not np.array_equal(b, c)
