"""A batch of camera views in one launch (include/sfrt.h sfrt_world_render_views and its _aux form).

Every comparison is byte for byte, with no case excluded.  View k must be the whole frame that
set_camera(views[k].cam) [+ update_spheres from the world's order] + render_band would write: the
reference is the oracle on the scene with that camera (with sort, on
scenes.sort_spheres(spheres, cam_pos)), or a second world stepping through that very loop.
Targets sit in 0xA5-poisoned canvases with padded pitch: the whole canvas, padding included, must
equal the expected one.

Frames: 45x23 (ragged against the 8-, 16- and 32-pixel tiles) for default10 and lcg64 (the last
size with the records beside the frame), 100x37 for lcg65 and lcg199 (the list kernels).
"""
import ctypes
import functools

import numpy as np
import pytest

import scenes
from conftest import host_threads, poisoned

pytestmark = pytest.mark.gpu

POISON = 0xA5
E_INVALID = -1
W, H, PAD = 45, 23, 32
LW, LH = 100, 37
NAMES = ["default10", "lcg64", "lcg65", "lcg199"]
# (cam_pos, rotation, hrotation): the last one is outside every sphere
CAMS = [((0.0, 0.0, 0.0), 0.7, 0.3), ((0.5, -0.3, 1.0), -0.4, 0.1), ((-1.0, 0.2, -0.5), 2.1, -0.2),
        ((2.0, 0.5, -1.5), 3.5, 0.25), ((100.0, 0.0, 0.0), -1.57, 0.0)]
PLANES = ("depth", "sphere", "steps")
DTYPES = {"depth": np.float32, "sphere": np.int32, "steps": np.int32}
PLANE_PADS = {"depth": 4, "sphere": 8, "steps": 12}


@functools.lru_cache(maxsize=None)
def _floor():
    tex, tw, th = scenes.load_floor()
    tex = np.array(tex, dtype=np.uint8).ravel()
    tex.setflags(write=False)
    return tex, tw, th


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "lcg65":  # as tests/test_render_subset.py builds them
        return scenes.Scene(name, scenes.sort_spheres(scenes.lcg_spheres(count=64)))
    if name == "lcg199":
        return scenes.Scene(name, scenes.sort_spheres(scenes.lcg_spheres(count=198)))
    return scenes.SCENES[name]()


def _size(name):
    return (W, H) if name in ("default10", "lcg64") else (LW, LH)


@functools.lru_cache(maxsize=None)
def _sorted(name, k):
    s = scenes.sort_spheres(_scene(name).spheres, CAMS[k][0])
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def oracle_frame(name, k, sort):
    """View k of the scene by the oracle, (h, 4w); shared, read-only."""
    import oracle
    w, h = _size(name)
    pos, rot, hrot = CAMS[k]
    sc = _scene(name)
    spheres = _sorted(name, k) if sort else sc.spheres
    o = oracle.Oracle(w, h, spheres, *_floor(), cam_pos=pos, rotation=float(np.float32(rot)),
                      hrotation=float(np.float32(hrot)), fov_h=sc.fov_h, fov_v=sc.fov_v)
    out = o.render(host_threads()).reshape(h, 4 * w)
    out.setflags(write=False)
    return out


def _cam(pos, rot, hrot):
    import sfrt
    c = sfrt.Camera()
    for q in range(3):
        c.pos[q] = pos[q]
    c.rotation, c.hrotation = rot, hrot
    c.fov_h, c.fov_v = float(scenes.FOV_H), float(scenes.FOV_V)
    return c


def _cams():
    return [_cam(*c) for c in CAMS]


def _world(name, s=1):
    import sfrt
    w = sfrt.World(0)
    w.load_texture(*_floor())
    w.set_scene(_scene(name), *_size(name))
    w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
    return w


@pytest.fixture(scope="module")
def stream(built):
    import torch
    return torch.cuda.Stream()


def _views(cams, canvases):
    import sfrt
    return [sfrt.View(c, canvases[k].data_ptr()) for k, c in enumerate(cams)]


def _loop(world, name, cams, canvases, pitch, sort, stream, slots=None, planes=None):
    """The definition, on a world of its own: per view set_camera [+ update_spheres from the
    original order, slots with their spheres] + render_band[_aux] of the whole frame."""
    h = _size(name)[1]
    for k, c in enumerate(cams):
        world.set_camera(tuple(c.pos), c.rotation, c.hrotation, c.fov_h, c.fov_v)
        if sort:
            world.set_spheres(_scene(name).spheres)
            if slots is not None:
                world.set_sphere_textures(slots)
            world.update_spheres()
        if planes is None:
            world.render_band(canvases[k].data_ptr(), pitch, 0, h, stream.cuda_stream)
        else:
            world.render_band_aux(canvases[k].data_ptr(), pitch, 0, h, stream.cuda_stream,
                                  **planes[k])
    world.check(stream.cuda_stream)


def _equal(got, want, what):
    got, want = got.cpu().numpy(), (want.cpu().numpy() if hasattr(want, "cpu") else want)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} bytes differ, first at {tuple(bad[0])}"


def _expected(frames, pitch):
    """Poisoned (views, h, pitch) canvases holding the (h, 4w) frames."""
    want = np.full((len(frames), frames[0].shape[0], pitch), POISON, dtype=np.uint8)
    for k, f in enumerate(frames):
        want[k, :, :f.shape[1]] = f
    return want


# ---------------------------------------------------------------- the views differ

@pytest.mark.parametrize("name", ["default10", "lcg64"])
def test_the_views_sort_differently(name):
    """The first four cameras give four different sphere orders; the last is outside every
    sphere (no first step, so no culling window)."""
    orders = {_sorted(name, k).tobytes() for k in range(4)}
    assert len(orders) == 4
    sph = _scene(name).spheres
    d = np.linalg.norm(sph[:, :3] - np.array(CAMS[4][0], dtype=np.float32), axis=1)
    assert (sph[:, 3] - d < 0).all()


# ---------------------------------------------------------------- 1: against the oracle

@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("rays", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_against_the_oracle(stream, name, sort, rays, cull):
    import sfrt
    w, h = _size(name)
    pitch = 4 * w + PAD
    if sort:
        assert _sorted(name, 0).tobytes() != _sorted(name, 1).tobytes()
    with _world(name) as world:
        world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
        world.set_option(sfrt.SFRT_OPT_CULL, cull)
        canvases = poisoned((len(CAMS), h, pitch), POISON)
        world.render_views(_views(_cams(), canvases), pitch, sort=sort, stream=stream.cuda_stream)
        world.check(stream.cuda_stream)
        want = _expected([oracle_frame(name, k, sort) for k in range(len(CAMS))], pitch)
        _equal(canvases, want, f"{name} sort={sort} rays={rays} cull={cull}")


# ---------------------------------------------------------------- 2: against the library's loop

@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("name", ["default10", "lcg64", "lcg65"])
def test_against_the_loop_supersampled(stream, name, sort, s):
    w, h = _size(name)
    pitch = 4 * w + PAD
    cams = _cams()
    with _world(name, s) as world, _world(name, s) as other:
        got = poisoned((len(cams), h, pitch), POISON)
        want = poisoned((len(cams), h, pitch), POISON)
        world.render_views(_views(cams, got), pitch, sort=sort, stream=stream.cuda_stream)
        world.check(stream.cuda_stream)
        _loop(other, name, cams, want, pitch, sort, stream)
        _equal(got, want, f"{name} S={s} sort={sort}")
        assert (want.cpu().numpy()[:, :, :4 * w] != POISON).any()


class Planes:
    """Poisoned device planes of one view, each with its own padded pitch."""

    def __init__(self, names, w, h):
        self.pitch = {p: 4 * w + PLANE_PADS[p] for p in names}
        self.buf = {p: poisoned((h, self.pitch[p]), POISON) for p in names}

    def args(self):
        return {p: (b.data_ptr(), self.pitch[p]) for p, b in self.buf.items()}


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("name", ["default10", "lcg64", "lcg65"])
def test_aux_against_the_loop(stream, name, sort, s):
    """All three planes of every view against render_band_aux; view 1 asks for steps alone, view
    2 for depth and sphere.  With sort the sphere plane indexes the view's own sorted order."""
    w, h = _size(name)
    pitch = 4 * w + PAD
    cams = _cams()
    asked = [PLANES, ("steps",), ("depth", "sphere"), PLANES, PLANES]
    with _world(name, s) as world, _world(name, s) as other:
        got = poisoned((len(cams), h, pitch), POISON)
        want = poisoned((len(cams), h, pitch), POISON)
        gp = [Planes(a, w, h) for a in asked]
        wp = [Planes(a, w, h) for a in asked]
        world.render_views_aux(_views(cams, got), [p.args() for p in gp], pitch, sort=sort,
                               stream=stream.cuda_stream)
        world.check(stream.cuda_stream)
        _loop(other, name, cams, want, pitch, sort, stream, planes=[p.args() for p in wp])
        _equal(got, want, f"{name} colour")
        for k, a in enumerate(asked):
            for p in a:
                _equal(gp[k].buf[p], wp[k].buf[p], f"{name} view {k} {p}")
        if sort:  # two views' sphere planes name different spheres for the same index
            assert _sorted(name, 0).tobytes() != _sorted(name, 3).tobytes()


def test_texture_slots_travel_with_their_spheres(stream):
    """Per-sphere texture slots under SFRT_VIEWS_SORT: each view's records carry the slot of the
    sphere they describe, as update_spheres moves them."""
    name = "default10"
    w, h = _size(name)
    pitch = 4 * w + PAD
    cams = _cams()
    textures = scenes.load_all_textures()
    slots = scenes.all_texture_slots(len(_scene(name).spheres))
    with _world(name) as world, _world(name) as other:
        for wd in (world, other):
            for k, (tex, tw, th) in enumerate(textures):
                wd.load_texture(tex, tw, th, slot=k)
            wd.set_sphere_textures(slots)
        got = poisoned((len(cams), h, pitch), POISON)
        want = poisoned((len(cams), h, pitch), POISON)
        plain = poisoned((len(cams), h, pitch), POISON)
        world.render_views(_views(cams, got), pitch, sort=True, stream=stream.cuda_stream)
        world.render_views(_views(cams, plain), pitch, sort=False, stream=stream.cuda_stream)
        world.check(stream.cuda_stream)
        assert (world.sphere_textures == slots).all()
        _loop(other, name, cams, want, pitch, True, stream, slots=slots)
        _equal(got, want, "sorted, six textures")
        assert (got != plain).any().item()


# ---------------------------------------------------------------- 3: one view

@pytest.mark.parametrize("name", ["default10", "lcg65"])
def test_one_view_equals_render_band(stream, name):
    w, h = _size(name)
    pitch = 4 * w + PAD
    cam = _cams()[1]
    with _world(name) as world:
        world.set_camera(tuple(cam.pos), cam.rotation, cam.hrotation, cam.fov_h, cam.fov_v)
        got = poisoned((1, h, pitch), POISON)
        want = poisoned((1, h, pitch), POISON)
        world.render_band(want[0].data_ptr(), pitch, 0, h, stream.cuda_stream)
        world.render_views(_views([cam], got), pitch, stream=stream.cuda_stream)
        world.check(stream.cuda_stream)
        _equal(got, want, name)
        _equal(got, _expected([oracle_frame(name, 1, False)], pitch), name + " oracle")


# ---------------------------------------------------------------- 4: SFRT_MAX_VIEWS

@pytest.mark.parametrize("sort", [False, True])
def test_max_views(stream, sort):
    """1024 views of 9x5 with cameras on a short path: the (view, tile) mapping at the limit."""
    import sfrt
    name, w, h = "default10", 9, 5
    pitch = 4 * w + 4
    n = sfrt.SFRT_MAX_VIEWS
    cams = [_cam((0.002 * k, 0.001 * k, -0.0015 * k), 0.7 + 0.003 * k, 0.3 - 0.0005 * k)
            for k in range(n)]
    with _world(name) as world, _world(name) as other:
        for wd in (world, other):
            wd.set_size(w, h)
        got = poisoned((n, h, pitch), POISON)
        want = poisoned((n, h, pitch), POISON)
        world.render_views(_views(cams, got), pitch, sort=sort, stream=stream.cuda_stream)
        world.check(stream.cuda_stream)
        for k, c in enumerate(cams):
            other.set_camera(tuple(c.pos), c.rotation, c.hrotation, c.fov_h, c.fov_v)
            if sort:
                other.set_spheres(_scene(name).spheres)
                other.update_spheres()
            other.render_band(want[k].data_ptr(), pitch, 0, h, stream.cuda_stream)
        other.check(stream.cuda_stream)
        _equal(got, want, f"{n} views")
        g = got.cpu().numpy()
        assert (g[0] != g[n - 1]).any() and (g[:, :, :4 * w] != POISON).any()


# ---------------------------------------------------------------- 5: side by side

def test_two_views_side_by_side_in_one_canvas(stream):
    name = "default10"
    w, h = _size(name)
    pitch = 8 * w + PAD
    cams = _cams()[:2]
    import sfrt
    with _world(name) as world:
        canvas = poisoned((h, pitch), POISON)
        views = [sfrt.View(cams[0], canvas.data_ptr()), sfrt.View(cams[1], canvas.data_ptr() + 4 * w)]
        world.render_views(views, pitch, stream=stream.cuda_stream)
        world.check(stream.cuda_stream)
        want = np.full((h, pitch), POISON, dtype=np.uint8)
        want[:, :4 * w] = oracle_frame(name, 0, False)
        want[:, 4 * w:8 * w] = oracle_frame(name, 1, False)
        _equal(canvas, want, "side by side")


# ---------------------------------------------------------------- 6: the world is untouched

def _costs(world):
    """sfrt_world_row_costs' answer, or its error code where the last fill recorded none."""
    import sfrt
    try:
        row0, costs = world.row_costs()
        return row0, costs.tobytes()
    except sfrt.SfrtError as e:
        return e.code

@pytest.mark.parametrize("name", ["default10", "lcg65"])
def test_the_world_is_untouched(stream, name):
    w, h = _size(name)
    pitch = 4 * w + PAD
    cams = _cams()
    with _world(name) as world:
        world.set_camera((0.1, 0.0, 0.2), 0.7, 0.3)
        slots = np.zeros(len(_scene(name).spheres), dtype=np.int32)
        before = poisoned((3, h, pitch), POISON)
        # two ordered frames on the stream (the tile-order chain and the ray cache warm up)
        for k in range(2):
            world.render_band(before[k].data_ptr(), pitch, 0, h, stream.cuda_stream)
        world.check(stream.cuda_stream)
        # a batch queued between two ordered frames of one stream
        frames = poisoned((2, h, pitch), POISON)
        batch = poisoned((len(cams), h, pitch), POISON)
        world.render_band(frames[0].data_ptr(), pitch, 0, h, stream.cuda_stream)

        def state():
            return (bytes(world.camera), world.spheres.tobytes(), world.sphere_textures.tobytes(),
                    world.ray_cache_stats(), world.tile_record_bytes(), _costs(world))

        state0 = state()
        world.render_views(_views(cams, batch), pitch, sort=True, stream=stream.cuda_stream)
        steps = [Planes(("steps",), w, h) for _ in cams]
        world.render_views_aux(_views(cams, batch), [p.args() for p in steps], pitch, sort=False,
                               stream=stream.cuda_stream)
        assert state() == state0
        world.render_band(frames[1].data_ptr(), pitch, 0, h, stream.cuda_stream)
        world.check(stream.cuda_stream)
        assert (world.sphere_textures == slots).all()
        _equal(frames[0], before[0], "band before the batch")
        _equal(frames[1], before[0], "band after the batch")
        _equal(before[1], before[0], "bands")
        _equal(batch, _expected([oracle_frame(name, k, False) for k in range(len(cams))], pitch),
               "the batch itself")


# ---------------------------------------------------------------- 7: refusals

def test_refusals_write_nothing(stream):
    import sfrt
    lib = sfrt.lib()
    name = "default10"
    w, h = _size(name)
    pitch = 4 * w + PAD
    s = ctypes.c_void_p(stream.cuda_stream)
    with _world(name) as world:
        canvases = poisoned((3, h, pitch), POISON)
        planes_buf = poisoned((3, h, pitch), POISON)

        def views(n=3, **change):
            arr = (sfrt.View * max(n, 1))()
            for k in range(min(n, 3)):
                arr[k] = sfrt.View(_cams()[k], canvases[k].data_ptr())
            for k in range(3, n):
                arr[k] = arr[0]
            for key, (k, v) in change.items():
                if key == "ptr":
                    arr[k].dev_pixels = v
                else:
                    setattr(arr[k].cam, key, v)
            return arr

        def planes(n=3, change=None):
            arr = (sfrt.AuxPlanes * max(n, 1))()
            for k in range(n):
                arr[k].steps, arr[k].steps_pitch_bytes = planes_buf[min(k, 2)].data_ptr(), pitch
            if change:
                k, fields = change
                for f, v in fields.items():
                    setattr(arr[k], f, v)
            return arr

        def plain(v, count=3, p=pitch, flags=0, wd=world._h):
            return lib.sfrt_world_render_views(wd, v, count, p, flags, s)

        def aux(v, pl, count=3, p=pitch, flags=0):
            return lib.sfrt_world_render_views_aux(world._h, v, pl, count, p, flags, s)

        nan, inf = float("nan"), float("inf")
        big = sfrt.SFRT_MAX_VIEWS + 1
        refused = {
            "NULL world": plain(views(), wd=None),
            "NULL views": plain(None),
            "count < 0": plain(views(), count=-1),
            "count > max": plain(views(big), count=big),
            "pitch % 4": plain(views(), p=pitch + 2),
            "pitch < 4w": plain(views(), p=4 * w - 4),
            "NULL target": plain(views(ptr=(1, None))),
            "unaligned target": plain(views(ptr=(2, canvases[2].data_ptr() + 2))),
            "NaN rotation, last view": plain(views(rotation=(2, nan))),
            "inf rotation": plain(views(hrotation=(0, inf))),
            "NaN fov": plain(views(fov_h=(1, nan))),
            "inf fov_v, sorted": plain(views(fov_v=(2, inf)), flags=sfrt.SFRT_VIEWS_SORT),
            "flag bit 1": plain(views(), flags=2),
            "flag bit 31": plain(views(), flags=-2 ** 31),
            "aux NULL planes": aux(views(), None),
            "aux all NULL": aux(views(), planes(change=(2, {"steps": None}))),
            "aux pitch % 4": aux(views(), planes(change=(1, {"steps_pitch_bytes": pitch + 1}))),
            "aux pitch < 4w": aux(views(), planes(change=(2, {"steps_pitch_bytes": 4 * w - 4}))),
            "aux depth pitch": aux(views(), planes(change=(0, {"depth": planes_buf[0].data_ptr(),
                                                               "depth_pitch_bytes": 8}))),
            "aux NaN camera": aux(views(rotation=(2, nan)), planes()),
        }
        # a NaN position component in the last view alone
        v = views()
        v[2].cam.pos[1] = nan
        refused["NaN pos"] = plain(v)
        # more than 2^31 - 1 workgroups: 1024 views of 16384 x 16384 (2048 x 2048 tiles each)
        world.set_size(16384, 16384)
        refused["grid"] = plain(views(1024), count=1024, p=4 * 16384)
        refused["grid, aux"] = aux(views(1024), planes(1024), count=1024, p=4 * 16384)
        world.set_size(w, h)
        assert {k: r for k, r in refused.items() if r != E_INVALID} == {}
        # count == 0 is fine and queues nothing; the world's own codes come unchanged
        assert plain(views(), count=0) == 0
        world.set_spheres(np.zeros((0, 4), dtype=np.float32))
        assert plain(views()) == -2  # SFRT_E_EMPTY
        world.set_spheres(_scene(name).spheres)
        world.check(stream.cuda_stream)
        assert (canvases.cpu().numpy() == POISON).all() and (planes_buf.cpu().numpy() == POISON).all()
        # and the same arguments, unchanged, are accepted
        assert plain(views()) == 0 and aux(views(), planes()) == 0
        world.check(stream.cuda_stream)
        _equal(canvases, _expected([oracle_frame(name, k, False) for k in range(3)], pitch), "accepted")
    with sfrt.World(0) as empty:  # no texture
        empty.set_scene(_scene(name), w, h)
        assert lib.sfrt_world_render_views(empty._h, views(), 3, pitch, 0, s) == -3
