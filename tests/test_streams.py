"""Many asynchronous fills in flight on several HIP streams at once.

Every renderer stages its per-launch tables (sphere records above 64
spheres, voxel column/row/object tables, GLSL wall/ball/pair tables) in a
ring of device slots guarded by events; a slot is never rewritten while a
launch on any stream may still read it.  Queue many launches with changing
scene state on three streams without synchronising, then compare every
frame with the same frame rendered alone.
"""
import os

import numpy as np
import pytest

import glsl_scenes as gs
import scenes
import voxel_scenes as vs
from conftest import poisoned


def _report(got, want, w):
    bad = np.nonzero(np.any(got.reshape(-1, 4) != want.reshape(-1, 4), axis=1))[0]
    if bad.size == 0:
        return ""
    rows = bad // w
    return f"{bad.size} pixels differ in rows {rows.min()}..{rows.max()}"


def _streams(n):
    import torch
    return [torch.cuda.Stream() for _ in range(n)]


@pytest.mark.gpu
def test_sphere_frames_in_flight(built, floor):
    import sfrt
    import torch
    w, h, k = 640, 360, 12
    spheres = scenes.sort_spheres(scenes.lcg_spheres(120, 4242))    # > 64: device ring path
    poses = [(0.25 * i, 0.05 * (i % 5) - 0.1) for i in range(k)]
    with sfrt.World(0) as world:
        world.load_texture(*floor)
        want = []
        for p in poses:
            world.set_scene(scenes.Scene("x", spheres).posed(*p), w, h)
            want.append(world.render())
        bufs = [torch.empty(h, w * 4, dtype=torch.uint8, device="cuda") for _ in poses]
        ss = _streams(3)
        for i, p in enumerate(poses):
            world.set_scene(scenes.Scene("x", spheres).posed(*p), w, h)
            world.render_band(bufs[i].data_ptr(), w * 4, 0, h, ss[i % 3].cuda_stream)
        torch.cuda.synchronize()
        for s in ss:
            world.check(s.cuda_stream)
    for i in range(k):
        got = bufs[i].cpu().numpy().ravel()
        assert np.array_equal(got, want[i]), f"frame {i}: {_report(got, want[i], w)}"


@pytest.mark.gpu
def test_voxel_frames_in_flight(built):
    import sfrt
    import torch
    w, h, k = 480, 270, 10
    tex, dyn = vs.load_textures()
    worlds = [vs.default_world((15.5 + 0.7 * i, 1.9, 15.5 + 0.3 * i), 0.4 * i, 0.02 * i)
              for i in range(k)]
    with sfrt.VoxelWorld(0) as v:
        v.load_assets(tex, dyn, vs.COLORS)
        want = []
        for scene in worlds:
            v.set_scene(scene, w, h)
            want.append(v.render())
        bufs = [torch.empty(h, w * 4, dtype=torch.uint8, device="cuda") for _ in worlds]
        ss = _streams(3)
        for i, scene in enumerate(worlds):
            v.set_scene(scene, w, h)
            v.render_band(bufs[i].data_ptr(), w * 4, 0, h, ss[i % 3].cuda_stream)
        torch.cuda.synchronize()
        for s in ss:
            v.check(s.cuda_stream)
    for i in range(k):
        got = bufs[i].cpu().numpy().ravel()
        assert np.array_equal(got, want[i]), f"frame {i}: {_report(got, want[i], w)}"


@pytest.mark.gpu
def test_glsl_frames_in_flight(built, floor):
    import sfrt
    import torch
    w, h, k = 480, 270, 10
    blocks = [gs.default_uniforms(w, h, 0.6 * i, 0.05 * i, frames=20 * i) for i in range(k)]
    with sfrt.GlslShader(0) as s:
        s.set_ground(*floor)
        want = []
        for u in blocks:
            s.set_uniforms(u)
            want.append(s.draw_image(w, h))
        bufs = [torch.empty(h, w * 4, dtype=torch.uint8, device="cuda") for _ in blocks]
        ss = _streams(3)
        for i, u in enumerate(blocks):
            s.set_uniforms(u)
            s.draw(bufs[i].data_ptr(), w, h, w * 4, 0, h, ss[i % 3].cuda_stream)
        torch.cuda.synchronize()
        for st in ss:
            s.check(st.cuda_stream)
    for i in range(k):
        got = bufs[i].cpu().numpy().ravel()
        assert np.array_equal(got, want[i]), f"frame {i}: {_report(got, want[i], w)}"


@pytest.mark.gpu
def test_sphere_tile_order_chains_more_streams_than_chains(built, floor):
    """The adaptive tile order keeps one chain per stream (sfrt_sched.h TileChains, 4
    chains): frames round-robin over 6 streams in the ordered render_band path -- chains
    taken over from other streams -- with the camera moving equal frames rendered alone."""
    import sfrt
    import torch
    w, h, k = 1600, 1200, 18
    sc = scenes.lcg64()
    poses = [(0.01 * i, 0.0) for i in range(k)]
    with sfrt.World(0) as world:
        world.load_texture(*floor)
        want = []
        for p in poses:
            world.set_scene(sc.posed(*p), w, h)
            want.append(world.render())
        bufs = [torch.empty(h, w * 4, dtype=torch.uint8, device="cuda") for _ in poses]
        ss = _streams(6)
        for rep in range(2):  # the second pass runs in orders built from the first
            for i, p in enumerate(poses):
                world.set_scene(sc.posed(*p), w, h)
                world.render_band(bufs[i].data_ptr(), w * 4, 0, h, ss[(i + rep) % 6].cuda_stream)
        torch.cuda.synchronize()
        for s in ss:
            world.check(s.cuda_stream)
    for i in range(k):
        got = bufs[i].cpu().numpy().ravel()
        assert np.array_equal(got, want[i]), f"frame {i}: {_report(got, want[i], w)}"


@pytest.mark.gpu
def test_growth_waits_for_no_other_stream(built, floor):
    """Buffers that grow between frames -- the sphere world's record ring (more spheres) and
    host-frame staging (a larger update_image), the voxel renderer's per-frame tables (a larger
    frame), the GLSL renderer's tables (more balls), the tile-order buffers of a new stream's
    chain, the pipelined display slots -- are reallocated without waiting for unrelated work:
    hipFree / hipHostFree wait for the whole device, so these paths use stream-ordered device
    memory and retire replaced pinned buffers (sfrt_host.h).  With ~50 ms of work queued on an
    unrelated stream, every call returns while that work is still pending, and the frames equal
    the same frames rendered on their own afterwards."""
    import sfrt
    import torch
    # high priority: the world's own stream (update_image) can never share its hardware queue,
    # where it would run behind the busy work whatever the library does (GPU_MAX_HW_QUEUES)
    busy_stream = torch.cuda.Stream(priority=-1)
    s1 = torch.cuda.Stream()

    def hold():
        torch.cuda.synchronize()
        with torch.cuda.stream(busy_stream):
            torch.cuda._sleep(100_000_000)

    def still_busy(what):
        assert not busy_stream.query(), f"{what} waited for an unrelated stream"

    checks = []
    with sfrt.World(0) as world:
        world.load_texture(*floor)
        world.set_scene(scenes.default10(), 320, 240)
        small = np.zeros(320 * 240 * 4, np.uint8)
        world.update_image(small)
        # the record ring grows (65 -> 300 spheres) and a new stream's chain is allocated
        sc = scenes.Scene("lcg300", scenes.sort_spheres(scenes.lcg_spheres(299, 77)))
        hold()
        world.set_scene(sc, 640, 360)
        dev = torch.empty((360, 640 * 4), dtype=torch.uint8, device="cuda:0")
        world.render_band(dev.data_ptr(), 640 * 4, 0, 360, s1.cuda_stream)
        still_busy("sphere record ring growth / new chain")
        checks.append(("sphere ring", dev, sc, 640, 360))
        # host-frame staging grows (update_image is synchronous on the world's own stream only)
        hold()
        big = np.zeros(640 * 360 * 4, np.uint8)
        world.update_image(big)
        still_busy("update_image staging growth")
        torch.cuda.synchronize()
        ref = np.zeros_like(big)
        world.update_image(ref)
        assert np.array_equal(big, ref)
        for name, buf, scx, w, h in checks:
            torch.cuda.synchronize()
            want = np.zeros(w * h * 4, np.uint8)
            world.set_scene(scx, w, h)
            world.update_image(want)
            assert np.array_equal(buf.cpu().numpy().ravel(), want), name
    # voxel tables grow with the frame
    vw = sfrt.VoxelWorld(0)
    try:
        tex, dyn = vs.load_textures()
        vw.load_assets(tex, dyn, vs.COLORS)
        scene = vs.default_world((20.5, 2.2, 40.5), 1.0, 0.1)
        vw.set_scene(scene, 160, 90)
        warm = torch.empty((90, 160 * 4), dtype=torch.uint8, device="cuda:0")
        vw.render_band(warm.data_ptr(), 160 * 4, 0, 90, s1.cuda_stream)
        hold()
        vw.set_scene(scene, 800, 450)
        vdev = torch.empty((450, 800 * 4), dtype=torch.uint8, device="cuda:0")
        vw.render_band(vdev.data_ptr(), 800 * 4, 0, 450, s1.cuda_stream)
        still_busy("voxel table growth")
        torch.cuda.synchronize()
        assert np.array_equal(vdev.cpu().numpy().ravel(), vw.render())
    finally:
        vw.close()
    # GLSL tables grow with the ball count
    g = sfrt.GlslShader(0)
    try:
        g.set_ground(*floor)
        u0 = gs.random_uniforms(2, 4, 1, 3, 320, 180)
        g.set_uniforms(u0)
        gw = torch.empty((180, 320 * 4), dtype=torch.uint8, device="cuda:0")
        g.draw(gw.data_ptr(), 320, 180, 320 * 4, 0, 180, s1.cuda_stream)
        hold()
        u1 = gs.random_uniforms(3, 40, 4, 50, 320, 180)
        g.set_uniforms(u1)
        g.draw(gw.data_ptr(), 320, 180, 320 * 4, 0, 180, s1.cuda_stream)
        still_busy("GLSL table growth")
        torch.cuda.synchronize()
        again = torch.empty_like(gw)
        g.draw(again.data_ptr(), 320, 180, 320 * 4, 0, 180, s1.cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(gw, again)
    finally:
        g.close()


def _world_frames(sfrt, floor, stack):
    world = stack.enter_context(sfrt.World(0))
    world.load_texture(*floor)

    def frame(w, h):
        world.set_scene(scenes.default10(), w, h)
        return world.render_aux()  # update_image_aux, all three planes
    return lambda: frame(320, 240), lambda: frame(640, 360)


def _voxel_frames(aux):
    def make(sfrt, floor, stack):
        vw = stack.enter_context(sfrt.VoxelWorld(0))
        vw.load_assets(*vs.load_textures(), vs.COLORS)
        scene = vs.default_world((20.5, 2.2, 40.5), 1.0, 0.1)

        def frame(w, h):
            vw.set_scene(scene, w, h)
            return vw.render_aux() if aux else (vw.render(),)  # update_image[_aux], four planes
        return lambda: frame(160, 90), lambda: frame(320, 180)
    return make


def _glsl_frames(sfrt, floor, stack):
    g = stack.enter_context(sfrt.GlslShader(0))
    g.set_ground(*floor)

    def frame(w, h):
        g.set_uniforms(gs.default_uniforms(w, h, 0.3, 0.1, frames=20))
        return tuple(g.draw_image_aux(w, h).values())
    return lambda: frame(160, 90), lambda: frame(320, 180)


def _rays(n, seed, center):
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((n, 3)).astype(np.float32)
    origins = (np.asarray(center, np.float32) + rng.uniform(-0.3, 0.3, (n, 3))).astype(np.float32)
    return dirs, origins


def _world_rays(own):
    def make(sfrt, floor, stack):
        world = stack.enter_context(sfrt.World(0))
        world.load_texture(*floor)
        sc = scenes.default10()
        world.set_scene(sc, 320, 240)

        def batch(n):
            dirs, origins = _rays(n, 11, sc.cam_pos)
            return tuple(world.cast_rays(dirs, origins if own else None).values())
        return lambda: batch(64), lambda: batch(4096)
    return make


def _voxel_rays(kind):
    def make(sfrt, floor, stack):
        vw = stack.enter_context(sfrt.VoxelWorld(0))
        vw.load_assets(*vs.load_textures(), vs.COLORS)
        vw.set_scene(vs.default_world((20.5, 2.2, 40.5), 1.0, 0.1), 160, 90)

        def batch(n):
            dirs, origins = _rays(n, 12, (20.5, 2.2, 40.5))
            if kind == "shadow":
                dists = np.linspace(1.0, 16.0, n, dtype=np.float32)
                return tuple(vw.cast_shadow_rays(origins, dirs, dists).values())
            return tuple(vw.cast_rays(dirs, None, origins if kind == "own" else None).values())
        return lambda: batch(64), lambda: batch(4096)
    return make


def _glsl_rays(sfrt, floor, stack):
    g = stack.enter_context(sfrt.GlslShader(0))
    g.set_ground(*floor)
    g.set_uniforms(gs.default_uniforms(160, 90, 0.3, 0.1, frames=20))
    return (lambda: tuple(g.cast_rays(_rays(64, 13, (0, 0, 0))[0]).values()),
            lambda: tuple(g.cast_rays(_rays(4096, 13, (0, 0, 0))[0]).values()))


HOST_GROWTH = {
    "world_update_image_aux": _world_frames,
    "voxel_update_image": _voxel_frames(False),
    "voxel_update_image_aux": _voxel_frames(True),
    "glsl_draw_image_aux": _glsl_frames,
    "world_cast_rays_origins": _world_rays(True),
    "world_cast_rays_camera": _world_rays(False),
    "voxel_cast_rays_origins": _voxel_rays("own"),
    "voxel_cast_rays_camera": _voxel_rays("camera"),
    "voxel_cast_shadow_rays": _voxel_rays("shadow"),
    "glsl_cast_rays": _glsl_rays,
}


@pytest.mark.gpu
@pytest.mark.parametrize("path", sorted(HOST_GROWTH))
def test_host_path_growth_waits_for_no_other_stream(built, floor, path):
    """The synchronous host paths test_growth_waits_for_no_other_stream does not reach, by the
    same scheme: the plane staging of update_image_aux (sphere, voxel) and draw_image_aux, the
    voxel update_image's device frame, and the staging of the host ray batches (sphere and voxel,
    with the caller's origins and from the camera; shadow; GLSL).  Each grows from a warm small
    call to one more than 1.5x larger -- past the pinned buffers' geometric capacity -- with
    ~50 ms of work queued on an unrelated stream: the call returns while that work is still
    pending, and its results equal the same call repeated on an idle device."""
    import contextlib
    import sfrt
    import torch
    busy_stream = torch.cuda.Stream(priority=-1)  # (as in the test above)
    with contextlib.ExitStack() as stack:
        small, large = HOST_GROWTH[path](sfrt, floor, stack)
        small()
        torch.cuda.synchronize()
        with torch.cuda.stream(busy_stream):
            torch.cuda._sleep(100_000_000)
        got = large()
        assert not busy_stream.query(), f"{path} waited for an unrelated stream"
        torch.cuda.synchronize()
        want = large()
        assert len(got) == len(want) and len(got) > 0
        for a, b in zip(got, want):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), path


@pytest.mark.gpu
def test_destroyed_stream_is_forgotten(built, floor):
    """A caller may destroy a stream once its frames are done (HIP leaves work still queued on a
    destroyed stream undefined).  The world's tile-order chain still remembers that stream as its last one: a larger
    frame on a seventeenth stream takes that chain over (sfrt_sched.h TileChains: sixteen chains,
    the least recently used one taken over) and reallocates its buffers.  Neither may pass the
    dead handle to HIP (a call on it crashed, profiles/r6y_dead_stream.txt), and the frames equal
    the same frames rendered alone."""
    import ctypes
    import sfrt
    import torch
    hip = ctypes.CDLL("libamdhip64.so")
    dead = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(dead)) == 0
    sc = scenes.default10()
    with sfrt.World(0) as world:
        world.load_texture(*floor)
        world.set_scene(sc, 320, 240)
        small = torch.empty((240, 320 * 4), dtype=torch.uint8, device="cuda:0")
        for _ in range(3):  # the chain's first launches, on the stream about to be destroyed
            world.render_band(small.data_ptr(), 320 * 4, 0, 240, dead.value)
        world.check(dead.value)
        assert hip.hipStreamDestroy(dead) == 0
        world.set_scene(sc, 640, 480)  # more tiles than the dead stream's chain holds
        n = 16
        big = [torch.empty((480, 640 * 4), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        ss = _streams(n)
        for rep in range(2):
            for i, s in enumerate(ss):  # the sixteenth new stream takes over the dead stream's chain
                world.render_band(big[i].data_ptr(), 640 * 4, 0, 480, s.cuda_stream)
        torch.cuda.synchronize()
        for s in ss:
            world.check(s.cuda_stream)
        want = world.render()
        world.set_scene(sc, 320, 240)
        want_small = world.render()
    assert np.array_equal(small.cpu().numpy().ravel(), want_small)
    for i in range(n):
        got = big[i].cpu().numpy().ravel()
        assert np.array_equal(got, want), f"stream {i}: {_report(got, want, 640)}"


@pytest.mark.gpu
def test_sphere_texture_load_is_stream_ordered(built, floor):
    """sfrt_world_load_texture without a device-wide wait: the new texels go into a new atlas,
    uploaded on the world's own stream, so a frame queued earlier on another stream (here behind
    ~50 ms of work on B) still reads the texels it was queued with and the call does not wait for
    it; a frame queued after the call, on another stream, reads the new ones.  A larger texture
    and a return to the first one included.  Each frame equals the same frame rendered on its own
    by a second world holding only that texture."""
    import sfrt
    import torch
    w, h = 320, 240
    rng = np.random.default_rng(5)
    texs = [floor, (rng.integers(0, 256, 128 * 128 * 4, dtype=np.uint8), 128, 128),
            (rng.integers(0, 256, 256 * 256 * 4, dtype=np.uint8), 256, 256), floor]
    sc = scenes.lcg64()
    # B at high priority: the world's stream, where the upload runs, never shares its hardware
    # queue (two streams that share one run in order, GPU_MAX_HW_QUEUES)
    a, b = torch.cuda.Stream(), torch.cuda.Stream(priority=-1)
    frames = []
    with sfrt.World(0) as world:
        world.load_texture(*texs[0])
        world.set_scene(sc, w, h)
        warm = torch.empty((h, w * 4), dtype=torch.uint8, device="cuda:0")
        world.render_band(warm.data_ptr(), w * 4, 0, h, a.cuda_stream)
        torch.cuda.synchronize()
        for k in range(1, len(texs)):
            old, new = poisoned((h, w * 4)), poisoned((h, w * 4))
            with torch.cuda.stream(b):
                torch.cuda._sleep(100_000_000)
            world.render_band(old.data_ptr(), w * 4, 0, h, b.cuda_stream)  # reads texs[k - 1]
            world.load_texture(*texs[k])
            busy = not b.query()
            world.render_band(new.data_ptr(), w * 4, 0, h, a.cuda_stream)  # reads texs[k]
            frames.append((texs[k - 1], old, texs[k], new, busy))
            torch.cuda.synchronize()
        world.check(a.cuda_stream)
        world.check(b.cuda_stream)
    for t_old, old, t_new, new, busy in frames:
        assert busy, "load_texture waited for the queued frame on B"
        for t, buf in ((t_old, old), (t_new, new)):
            with sfrt.World(0) as ref:
                ref.load_texture(*t)
                ref.set_scene(sc, w, h)
                want = ref.render()
            got = buf.cpu().numpy().ravel()
            assert np.array_equal(got, want), _report(got, want, w)


@pytest.mark.gpu
def test_check_waits_for_no_other_stream(built, floor):
    """check() reads a frame's status on the caller's stream.  A hipMemcpy there ran on the null
    stream, which also waits for every *blocking* stream of the process (hipStreamCreate's
    default, as a C++ caller of the ABI would create them) -- here one holding ~50 ms of work,
    at high priority so that no other stream shares its hardware queue."""
    import ctypes
    import sfrt
    import torch
    hip = ctypes.CDLL("libamdhip64.so")
    blk = ctypes.c_void_p()
    assert hip.hipStreamCreateWithPriority(ctypes.byref(blk), 0, -1) == 0  # flags 0: blocking
    ext = torch.cuda.ExternalStream(blk.value)
    s1 = torch.cuda.Stream()
    w, h = 320, 240
    buf = torch.empty((h, w * 4), dtype=torch.uint8, device="cuda:0")
    busy = {}
    tex, dyn = vs.load_textures()
    world, vw, g = sfrt.World(0), sfrt.VoxelWorld(0), sfrt.GlslShader(0)
    try:
        world.load_texture(*floor)
        world.set_scene(scenes.default10(), w, h)
        vw.load_assets(tex, dyn, vs.COLORS)
        vw.set_scene(vs.default_world((20.5, 2.2, 40.5), 1.0, 0.1), w, h)
        g.set_ground(*floor)
        g.set_uniforms(gs.default_uniforms(w, h, 0.4, 0.1))
        draws = {"sphere": lambda: world.render_band(buf.data_ptr(), w * 4, 0, h, s1.cuda_stream),
                 "voxel": lambda: vw.render_band(buf.data_ptr(), w * 4, 0, h, s1.cuda_stream),
                 "glsl": lambda: g.draw(buf.data_ptr(), w, h, w * 4, 0, h, s1.cuda_stream)}
        checks = {"sphere": world.check, "voxel": vw.check, "glsl": g.check}
        for name, draw in draws.items():
            draw()
            s1.synchronize()
            with torch.cuda.stream(ext):
                torch.cuda._sleep(100_000_000)
            checks[name](s1.cuda_stream)
            busy[name] = not ext.query()
            ext.synchronize()
    finally:
        torch.cuda.synchronize()
        world.close()
        vw.close()
        g.close()
        assert hip.hipStreamDestroy(blk) == 0
    assert all(busy.values()), f"check() waited for an unrelated blocking stream: {busy}"


def _interleaving_run(n_ops, seed, floor):
    """Random interleavings of scene, texture and size changes with draws on five streams (two
    at high priority, some behind queued busy work) and on short-lived streams (one in ten
    draws: created, drained and destroyed -- past sixteen streams an object's chains are taken
    over, sfrt_sched.h) across one sphere world, one voxel world
    and one GLSL shader, with no host synchronisation between the calls.  Returns the list of
    (kind, state, frame buffer) and the state pools; each frame must equal the state's frame
    rendered alone afterwards."""
    import ctypes
    import sfrt
    import torch
    hip = ctypes.CDLL("libamdhip64.so")
    rng = np.random.default_rng(seed)
    streams = [torch.cuda.Stream() for _ in range(3)] + [torch.cuda.Stream(priority=-1) for _ in range(2)]
    sizes = [(160, 90), (240, 136)]
    sph_scenes = [scenes.default10(), scenes.default10().posed(0.7, 0.3), scenes.lcg64(),
                  scenes.Scene("lcg100", scenes.sort_spheres(scenes.lcg_spheres(99, 31)))]
    r2 = np.random.default_rng(9)
    textures = [floor, (r2.integers(0, 256, 64 * 64 * 4, dtype=np.uint8), 64, 64),
                (r2.integers(0, 256, 256 * 128 * 4, dtype=np.uint8), 256, 128)]
    vox_tex, vox_dyn = vs.load_textures()
    vox_worlds = [vs.random_world(s)[0] for s in (3, 8, 21)]
    vox_alt = [vox_tex[0], (r2.integers(0, 256, 32 * 32 * 4, dtype=np.uint8), 32, 32)]
    glsl_u = [gs.random_uniforms(s, 12, 2, 6) for s in (4, 5)]
    grounds = [floor, textures[1]]
    world, vw, sh = sfrt.World(0), sfrt.VoxelWorld(0), sfrt.GlslShader(0)
    state = {"sphere": [0, 0, 0], "voxel": [0, 0, 0], "glsl": [0, 0, 0]}  # scene, texture, size
    world.load_texture(*textures[0])
    vw.load_assets(vox_tex, vox_dyn, vs.COLORS)
    sh.set_ground(*grounds[0])
    sh.set_uniforms(glsl_u[0])
    draws = []
    try:
        for _ in range(n_ops):
            kind = ["sphere", "voxel", "glsl"][int(rng.integers(3))]
            st = state[kind]
            op = rng.random()
            if op < 0.15:
                st[0] = int(rng.integers(len({"sphere": sph_scenes, "voxel": vox_worlds, "glsl": glsl_u}[kind])))
            elif op < 0.27:
                st[1] = int(rng.integers(len({"sphere": textures, "voxel": vox_alt, "glsl": grounds}[kind])))
                if kind == "sphere":
                    world.load_texture(*textures[st[1]])
                elif kind == "voxel":
                    vw.load_texture(0, *vox_alt[st[1]])
                else:
                    sh.set_ground(*grounds[st[1]])
                continue
            elif op < 0.35:
                st[2] = int(rng.integers(len(sizes)))
            elif op < 0.42:
                with torch.cuda.stream(streams[int(rng.integers(len(streams)))]):
                    torch.cuda._sleep(int(rng.integers(1, 8)) * 1_000_000)
                continue
            w, h = sizes[st[2]]
            if rng.random() < 0.08:  # a synchronous host frame (update_image / draw_image)
                if kind == "sphere":
                    world.set_scene(sph_scenes[st[0]], w, h)
                    host = world.render()
                elif kind == "voxel":
                    vw.set_scene(vox_worlds[st[0]], w, h)
                    host = vw.render()
                else:
                    sh.set_uniforms(glsl_u[st[0]])
                    host = sh.draw_image(w, h)
                draws.append((kind, tuple(st), host, None))
                continue
            raw = None
            if rng.random() < 0.1:  # a short-lived stream: created, drawn on, drained, destroyed
                raw = ctypes.c_void_p()
                assert hip.hipStreamCreateWithFlags(ctypes.byref(raw), 1) == 0
                s = torch.cuda.ExternalStream(raw.value)
            else:
                s = streams[int(rng.integers(len(streams)))]
            buf = torch.empty((h, w * 4), dtype=torch.uint8, device="cuda:0")
            with torch.cuda.stream(s):  # the poison on the draw's own stream, ahead of it
                buf.fill_(0xA5)
            if kind == "sphere":
                world.set_scene(sph_scenes[st[0]], w, h)
                world.render_band(buf.data_ptr(), w * 4, 0, h, s.cuda_stream)
            elif kind == "voxel":
                vw.set_scene(vox_worlds[st[0]], w, h)
                vw.render_band(buf.data_ptr(), w * 4, 0, h, s.cuda_stream)
            else:
                sh.set_uniforms(glsl_u[st[0]])
                sh.draw(buf.data_ptr(), w, h, w * 4, 0, h, s.cuda_stream)
            draws.append((kind, tuple(st), buf, s))
            if raw is not None:  # the objects remember it as a chain's last stream, by handle only
                assert hip.hipStreamSynchronize(raw) == 0 and hip.hipStreamDestroy(raw) == 0
        torch.cuda.synchronize()
        for s in streams:
            world.check(s.cuda_stream)
            vw.check(s.cuda_stream)
            sh.check(s.cuda_stream)
    finally:
        torch.cuda.synchronize()
        world.close()
        vw.close()
        sh.close()
    pools = dict(sizes=sizes, sph_scenes=sph_scenes, textures=textures, vox_tex=vox_tex,
                 vox_dyn=vox_dyn, vox_worlds=vox_worlds, vox_alt=vox_alt, glsl_u=glsl_u,
                 grounds=grounds)
    return draws, pools


def _interleaving_want(kind, st, p):
    """The frame of one state, rendered alone by a fresh object."""
    import sfrt
    w, h = p["sizes"][st[2]]
    if kind == "sphere":
        with sfrt.World(0) as r:
            r.load_texture(*p["textures"][st[1]])
            r.set_scene(p["sph_scenes"][st[0]], w, h)
            return r.render()
    if kind == "voxel":
        r = sfrt.VoxelWorld(0)
        try:
            tex = list(p["vox_tex"])
            tex[0] = p["vox_alt"][st[1]]
            r.load_assets(tex, p["vox_dyn"], vs.COLORS)
            r.set_scene(p["vox_worlds"][st[0]], w, h)
            return r.render()
        finally:
            r.close()
    r = sfrt.GlslShader(0)
    try:
        r.set_ground(*p["grounds"][st[1]])
        r.set_uniforms(p["glsl_u"][st[0]])
        return r.draw_image(w, h)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_random_interleavings(built, floor, seed):
    """The stream-ordering machinery under random schedules (sfrt_host.h TableSlot /
    SharedBuffer / PinnedStage, sfrt_sched.h TileChains, the sphere world's texture atlas):
    every frame equals its state's frame rendered alone."""
    draws, pools = _interleaving_run(160, seed, floor)
    kinds = {k for k, _, _, _ in draws}
    states = {(k, st) for k, st, _, _ in draws}
    print(f"{len(draws)} draws ({sum(s is None for *_, s in draws)} host frames), {len(states)} states")
    assert len(draws) >= 80 and kinds == {"sphere", "voxel", "glsl"} and len(states) >= 12
    cache = {}
    for i, (kind, st, buf, _) in enumerate(draws):
        if (kind, st) not in cache:
            cache[(kind, st)] = _interleaving_want(kind, st, pools)
        want = cache[(kind, st)]
        got = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy().ravel()
        assert np.array_equal(got, want), f"draw {i} ({kind}, state {st}): " \
                                          f"{_report(got, want, pools['sizes'][st[2]][0])}"


@pytest.mark.gpu
@pytest.mark.skipif(not os.environ.get("SFRT_INTERLEAVE_SEEDS"),
                    reason="on demand: SFRT_INTERLEAVE_SEEDS=<n> (400 operations per seed)")
def test_random_interleavings_long(built, floor):
    """test_random_interleavings over SFRT_INTERLEAVE_SEEDS seeds of 400 operations each."""
    total = 0
    seed0 = int(os.environ.get("SFRT_INTERLEAVE_SEED0", "100"))
    for seed in range(seed0, seed0 + int(os.environ["SFRT_INTERLEAVE_SEEDS"])):
        draws, pools = _interleaving_run(400, seed, floor)
        cache = {}
        for i, (kind, st, buf, _) in enumerate(draws):
            if (kind, st) not in cache:
                cache[(kind, st)] = _interleaving_want(kind, st, pools)
            got = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy().ravel()
            assert np.array_equal(got, cache[(kind, st)]), f"seed {seed} draw {i} ({kind}, {st})"
        total += len(draws)
        print(f"seed {seed}: {len(draws)} draws, {len(cache)} states, all equal", flush=True)
    print(f"{total} draws in all")


@pytest.mark.gpu
def test_random_display_pipeline(built, floor):
    """The display path (submit_frame / wait_frame into pinned host frames, two in flight) under
    random scene, size and texture changes between submissions: the pipeline slots grow with the
    frame and the record ring with the sphere count; every delivered frame equals its state's
    frame rendered alone."""
    import sfrt
    rng = np.random.default_rng(77)
    sizes = [(160, 90), (320, 180), (240, 136)]
    sph_scenes = [scenes.default10(), scenes.lcg64().posed(0.4, -0.1),
                  scenes.Scene("lcg90", scenes.sort_spheres(scenes.lcg_spheres(89, 5)))]
    r2 = np.random.default_rng(3)
    textures = [floor, (r2.integers(0, 256, 128 * 64 * 4, dtype=np.uint8), 128, 64)]
    frames = [sfrt.HostFrame(320 * 180 * 4) for _ in range(3)]
    pending, delivered = [], []
    st = [0, 0, 0]  # scene, texture, size
    try:
        with sfrt.World(0) as world:
            world.load_texture(*textures[0])
            for k in range(200):
                op = rng.random()
                if op < 0.2:
                    st[0] = int(rng.integers(len(sph_scenes)))
                elif op < 0.3:
                    st[1] = int(rng.integers(len(textures)))
                    world.load_texture(*textures[st[1]])
                elif op < 0.45:
                    st[2] = int(rng.integers(len(sizes)))
                w, h = sizes[st[2]]
                world.set_scene(sph_scenes[st[0]], w, h)
                if len(pending) == 2:  # at most two frames in flight
                    t, fr, s = pending.pop(0)
                    world.wait_frame(t)
                    delivered.append((tuple(s), fr.array[: sizes[s[2]][0] * sizes[s[2]][1] * 4].copy()))
                fr = frames[k % 3]
                pending.append((world.submit_frame(fr), fr, tuple(st)))
            for t, fr, s in pending:
                world.wait_frame(t)
                delivered.append((tuple(s), fr.array[: sizes[s[2]][0] * sizes[s[2]][1] * 4].copy()))
    finally:
        for fr in frames:
            fr.free()
    cache = {}
    for i, (s, got) in enumerate(delivered):
        if s not in cache:
            w, h = sizes[s[2]]
            with sfrt.World(0) as ref:
                ref.load_texture(*textures[s[1]])
                ref.set_scene(sph_scenes[s[0]], w, h)
                cache[s] = ref.render()
        assert np.array_equal(got, cache[s]), f"frame {i} (state {s}): {_report(got, cache[s], sizes[s[2]][0])}"
    assert len(delivered) == 200 and len(cache) >= 8
