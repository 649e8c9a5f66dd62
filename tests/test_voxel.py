"""Voxel World frame fill: World::UpdateImage/Raycast/LRaycast,
/root/reference/Raytracing/World.cpp:62-87, 302-491.

CPU: the restatement (oracle/voxelworld_oracle.c) is deterministic across
thread counts and interleaves, and matches its committed golden hashes
(tests/golden/golden.json "voxel").  GPU: libsfrt.so's voxel kernel equals the
restatement byte for byte (RGBA8).  The restatement itself is held to the
reference's own compiled World.cpp by tests/test_reference_pin.py.
"""
import json
import os

import numpy as np
import pytest

import oracle
import voxel_scenes as vs
from conftest import ROOT, host_threads, poisoned

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))

VOXEL_CASES = [  # (width, height, cam_pos, rotation, hrotation)
    (320, 180, (15.5, 1.9, 15.5), 0.0, 0.0),
    (1920, 1080, (15.5, 1.9, 15.5), 0.0, 0.0),
    (1920, 1080, (30.25, 2.6, 12.75), 2.2, 0.25),
    (3840, 2160, (47.5, 1.5, 60.1), 4.0, -0.3),
    (3840, 2160, (15.5, 1.9, 15.5), 0.0, 0.0),  # bench.py's "voxel_3840x2160" line
]


def case_key(c):
    w, h, p, r, hr = c
    return f"{w}x{h}@{p[0]:g},{p[1]:g},{p[2]:g}/{r:g},{hr:g}"


@pytest.fixture(scope="module")
def assets():
    oracle.build()
    return vs.load_textures()


def voxel_oracle(case, assets):
    w, h, p, r, hr = case
    scene = vs.default_world(p, r, hr)
    return scene, oracle.VoxelOracle(scene, w, h, assets[0], assets[1], vs.COLORS)


def test_default_world_layout():
    b = vs.default_blocks()
    assert b.shape == (100, 10, 100)
    assert (b[:, 0, :] == 1).all()                    # floor, World.cpp:9-10
    assert b[0, 5, 50] == 0 and b[99, 3, 7] == 0      # outer walls
    assert b[9, 5, 5] == 0                            # pillar x%9==0, z%5==0
    assert b[1, 4, 1] == 3 and b[3, 4, 1] != 3        # mid blocks y==4, x%3 != 0, z%4 != 0
    assert b[50, 9, 51] == 2                          # ceiling
    assert len(vs._lamps()) == 128
    s = vs.default_world()
    assert s.dyn.shape[0] == 133 and 0 < s.lights.shape[0] < 128


@pytest.mark.parametrize("case", VOXEL_CASES[:3], ids=case_key)
def test_voxel_oracle_golden_and_deterministic(assets, case):
    _, o = voxel_oracle(case, assets)
    a = o.render(host_threads())
    assert oracle.fnv1a64(a) == GOLDEN["voxel"][case_key(case)]["fnv1a64"]
    assert o.bad_texel_reads() == 0
    if case[0] <= 320:
        assert np.array_equal(a, o.render(1))
        canvas = np.zeros_like(a)
        for t in range(4):                            # World has rays[4] (World.h:96)
            for cyc in range(4):
                o.update_image(canvas, t, 4, cyc, 4)
        assert np.array_equal(canvas, a)


@pytest.fixture(scope="module")
def vworld(built, assets):
    import sfrt
    w = sfrt.VoxelWorld(0)
    w.load_assets(assets[0], assets[1], vs.COLORS)
    yield w
    w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", VOXEL_CASES, ids=case_key)
def test_voxel_gpu_matches_oracle(vworld, assets, case):
    scene, o = voxel_oracle(case, assets)
    vworld.set_scene(scene, case[0], case[1])
    got = vworld.render()
    want = o.render(host_threads())
    g, w = got.reshape(-1, 4), want.reshape(-1, 4)
    bad = np.nonzero(np.any(g != w, axis=1))[0]
    assert bad.size == 0, (f"{bad.size} pixels differ, first ({bad[0] % case[0]}, "
                           f"{bad[0] // case[0]}): gpu={g[bad[0]]} oracle={w[bad[0]]}")


@pytest.mark.gpu
def test_voxel_gpu_subsets_and_bands(vworld, assets):
    import torch
    case = (320, 180, (20.5, 2.2, 40.5), 1.0, 0.1)
    scene, o = voxel_oracle(case, assets)
    vworld.set_scene(scene, 320, 180)
    for ystart, yadd, xstart, xadd in [(0, 4, 1, 4), (3, 4, 0, 1), (0, 1, 7, 3)]:
        canvas = np.full(320 * 180 * 4, 0x5A, np.uint8)
        expect = canvas.copy()
        vworld.update_image(canvas, ystart, yadd, xstart, xadd)
        o.update_image(expect, ystart, yadd, xstart, xadd)
        assert np.array_equal(canvas, expect), (ystart, yadd, xstart, xadd)
    dev = torch.zeros(180, 320 * 4, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    for r0, r1 in [(0, 37), (37, 90), (90, 180)]:
        vworld.render_band(dev[r0].data_ptr(), 320 * 4, r0, r1 - r0, s)
    vworld.check(s)
    assert np.array_equal(dev.cpu().numpy().ravel(), o.render(1))


@pytest.mark.gpu
def test_voxel_adaptive_tile_order_same_bytes(vworld, assets):
    """SFRT_OPT_TILE_ORDER on the voxel renderer: frames rendered back to back through
    render_band (order from two frames back, poses and sizes changing, a row band) equal
    the row-major frames of update_image and the oracle."""
    import sfrt
    import torch
    seq = [((15.5, 1.9, 15.5), 0.0, 0.0, 640, 360, 0, 360)] * 4 + \
          [((30.25, 2.6, 12.75), 0.3 * k, 0.05 * k, 640, 360, 0, 360) for k in range(4)] + \
          [((47.5, 1.5, 60.1), 4.0, -0.3, 333, 211, 0, 211)] * 3 + \
          [((47.5, 1.5, 60.1), 4.0, -0.3, 640, 360, 40, 200)] * 3
    stream = torch.cuda.Stream()
    frames = []
    vworld.set_option(sfrt.SFRT_OPT_TILE_ORDER, 1)  # off by default for the voxel renderer
    try:
        with torch.cuda.stream(stream):
            for p, r, hr, width, height, r0, rows in seq:
                vworld.set_scene(vs.default_world(p, r, hr), width, height)
                b = poisoned((height, width * 4))
                vworld.render_band(b[r0].data_ptr(), width * 4, r0, rows, stream.cuda_stream)
                frames.append(b)
        vworld.check(stream.cuda_stream)
        torch.cuda.synchronize()
    finally:
        vworld.set_option(sfrt.SFRT_OPT_TILE_ORDER, 0)
    for k, ((p, r, hr, width, height, r0, rows), b) in enumerate(zip(seq, frames)):
        vworld.set_scene(vs.default_world(p, r, hr), width, height)
        want = np.full(width * height * 4, 0xA5, dtype=np.uint8)
        full = vworld.render()
        want[r0 * width * 4:(r0 + rows) * width * 4] = full[r0 * width * 4:(r0 + rows) * width * 4]
        assert np.array_equal(b.cpu().numpy().ravel(), want), (k, p, width, height, r0, rows)
        if k in (0, 11):
            o = oracle.VoxelOracle(vs.default_world(p, r, hr), width, height, assets[0], assets[1],
                                   vs.COLORS)
            assert np.array_equal(full, o.render(host_threads())), k


@pytest.mark.gpu
def test_voxel_tables_reused_across_streams(vworld, assets):
    """ADVICE r4 (sfrt_host.h TableSlot): tables staged on stream A behind queued work, then
    reused at once by a frame on stream B, with no host sync between: B's frame must wait for
    A's staging copy (hipStreamWaitEvent on the slot's event) and show the new scene, and the
    slot's event must then cover both users before it is restaged."""
    import dataclasses
    import torch
    w, h = 320, 180
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    base = vs.default_world((20.5, 2.2, 40.5), 1.0, 0.1)
    vworld.set_scene(base, w, h)
    buf0 = poisoned((h, w * 4))
    vworld.render_band(buf0.data_ptr(), w * 4, 0, h, a.cuda_stream)
    vworld.check(a.cuda_stream)
    scenes_ = []
    for k in range(3):  # three scene changes: each stages a new slot on A, read at once on B
        sc = dataclasses.replace(base, cam_pos=(20.5 + 0.75 * (k + 1), 2.2, 40.5), rotation=1.0 + 0.2 * k)
        vworld.set_scene(sc, w, h)
        ba = poisoned((h, w * 4))
        bb = poisoned((h, w * 4))
        torch.cuda.synchronize()
        with torch.cuda.stream(a):
            torch.cuda._sleep(100_000_000)  # ~50 ms of queued work ahead of A's staging copy
        vworld.render_band(ba.data_ptr(), w * 4, 0, h, a.cuda_stream)   # stages on A
        vworld.render_band(bb.data_ptr(), w * 4, 0, h, b.cuda_stream)   # reuses on B at once
        scenes_.append((sc, ba, bb))
    torch.cuda.synchronize()
    vworld.check(a.cuda_stream)
    vworld.check(b.cuda_stream)
    for sc, ba, bb in scenes_:
        want = oracle.VoxelOracle(sc, w, h, assets[0], assets[1], vs.COLORS).render(host_threads())
        assert np.array_equal(ba.cpu().numpy().ravel(), want)
        assert np.array_equal(bb.cpu().numpy().ravel(), want)


@pytest.mark.gpu
def test_voxel_tables_restaged_after_every_setter(vworld, assets):
    """The per-frame tables (columns, rows, billboards, lights) are staged once and reused
    while nothing they depend on changes (sfrt_voxel.cpp tables_version): each setter alone --
    camera, size, billboards, lights -- must be seen by the next frame, and a repeated frame
    must equal the first.  Every frame is compared with the oracle of the scene it was given."""
    import ctypes
    import dataclasses
    import sfrt
    import torch
    L = sfrt.lib()
    stream = torch.cuda.Stream()

    def frame(w, h):
        b = poisoned((h, w * 4))
        vworld.render_band(b.data_ptr(), w * 4, 0, h, stream.cuda_stream)
        vworld.check(stream.cuda_stream)
        return b.cpu().numpy().ravel()

    def want(scene, w, h):
        return oracle.VoxelOracle(scene, w, h, assets[0], assets[1], vs.COLORS).render(host_threads())

    base = vs.default_world((20.5, 2.2, 40.5), 1.0, 0.1)
    vworld.set_scene(base, 320, 180)
    first = frame(320, 180)
    assert np.array_equal(first, want(base, 320, 180))
    assert np.array_equal(frame(320, 180), first)          # reused tables
    # camera alone
    moved = dataclasses.replace(base, cam_pos=(21.25, 2.2, 39.5), rotation=1.3)
    cam = sfrt.Camera()
    for k in range(3):
        cam.pos[k] = float(moved.cam_pos[k])
    cam.rotation, cam.hrotation = float(moved.rotation), float(moved.hrotation)
    cam.fov_h, cam.fov_v = float(moved.fov_h), float(moved.fov_v)
    assert L.sfrt_voxel_set_camera(vworld._h, ctypes.byref(cam)) == 0
    assert np.array_equal(frame(320, 180), want(moved, 320, 180))
    # size alone
    assert L.sfrt_voxel_set_size(vworld._h, 200, 120) == 0
    vworld.width, vworld.height = 200, 120
    assert np.array_equal(frame(200, 120), want(moved, 200, 120))
    # billboards alone: every sprite 0.4 closer to the camera's row of the list
    dyn = moved.dyn.copy()
    dyn["dist_to_camera"] = dyn["dist_to_camera"] * np.float32(0.5)
    dyn["pos"][:, 1] = dyn["pos"][:, 1] + np.float32(0.25)
    d = np.ascontiguousarray(dyn)
    assert L.sfrt_voxel_set_dynamics(vworld._h, d.ctypes.data, d.shape[0]) == 0
    moved = dataclasses.replace(moved, dyn=dyn)
    assert np.array_equal(frame(200, 120), want(moved, 200, 120))
    # lights alone: the first half of the active lights
    lights = np.ascontiguousarray(moved.lights[: max(1, moved.lights.shape[0] // 2)])
    assert L.sfrt_voxel_set_lights(vworld._h, lights.ctypes.data, lights.shape[0]) == 0
    moved = dataclasses.replace(moved, lights=lights)
    got = frame(200, 120)
    assert np.array_equal(got, want(moved, 200, 120))
    assert np.array_equal(frame(200, 120), got)


VOXEL_EDGE_CASES = [  # (width, height, cam_pos, rotation, hrotation, what)
    # hray of column 0 is exactly 0: dir.x == 0, so those waves take the plain-division DDA
    # (raycast_t<false>, lraycast_t<false>) instead of the reciprocal one
    (320, 180, (15.5, 1.9, 15.5), float(vs.deg2rad(75)) / 2, 0.0, "axis_parallel_column"),
    # outside the grid at negative coordinates: negative map keys, truncation toward zero and the
    # reference's negative-fraction steps (World.cpp:330-350 with pos < 0)
    (320, 180, (-1.5, 1.9, -1.5), 0.785, 0.0, "negative_coordinates"),
    (320, 180, (-3.5, 4.5, 20.5), 1.5708, 0.0, "negative_x_facing_wall"),
    # above the grid looking down: cells with y >= ny, rays entering through the ceiling layer
    (320, 180, (50.5, 11.5, 50.5), 0.3, -1.2, "above_the_grid"),
    (320, 180, (50.5, 10.25, 50.5), 0.3, -0.9, "just_above_the_ceiling"),
    # integer camera position: every fraction starts at 0
    (320, 180, (16.0, 2.0, 16.0), 1.0, 0.2, "integer_position"),
    # looking straight along the floor far away: long DDA walks up to maxiter
    (320, 180, (1.5, 0.5, 1.5), 0.785398, 0.0, "long_walks"),
    # the fast primary DDA's host bound (sfrt_voxel.cpp dda_qlim) off: a camera beyond 2^30
    # sends every wave to the guarded conversions, and one just below 2^31 walks past it, where
    # the reference's cvttss2si gives INT_MIN (to_i32) and a plain conversion would saturate
    (320, 180, (1.5e9, 1.9, 15.5), 3.14159, 0.0, "far_camera"),
    (320, 180, (2147483520.0, 1.9, 15.5), 0.0, 0.0, "camera_at_int_limit"),
    (320, 180, (2147483520.0, 1.9, 15.5), 3.14159, 0.0, "camera_at_int_limit_back"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", VOXEL_EDGE_CASES, ids=lambda c: c[-1])
def test_voxel_gpu_edge_poses_match_oracle(vworld, assets, case):
    """Poses that reach the DDA's rarely taken paths, byte for byte against the restatement
    (oracle/voxelworld_oracle.c).  Reference: World::Raycast / LRaycast, World.cpp:302-491.
    From negative coordinates a hit in cell 0 can come from a position in (-1, 0) (truncation
    toward zero), whose negative fraction makes the reference read outside the texture (UB):
    the restatement substitutes magenta and counts the read; the kernel substitutes the same
    magenta and fails loudly (SFRT_E_TEXEL from check()), and its frame still equals the
    restatement's."""
    import sfrt
    import torch
    w, h, p, r, hr, _ = case
    scene = vs.default_world(p, r, hr)
    o = oracle.VoxelOracle(scene, w, h, assets[0], assets[1], vs.COLORS)
    before = oracle.VoxelOracle.bad_texel_reads()
    want = o.render(host_threads())
    ub = oracle.VoxelOracle.bad_texel_reads() > before
    vworld.set_scene(scene, w, h)
    stream = torch.cuda.Stream()
    dev = poisoned((h, w * 4))
    vworld.render_band(dev.data_ptr(), w * 4, 0, h, stream.cuda_stream)
    if ub:
        with pytest.raises(sfrt.SfrtError) as e:
            vworld.check(stream.cuda_stream)
        assert e.value.code == -7, e.value   # SFRT_E_TEXEL
    else:
        vworld.check(stream.cuda_stream)
    g, wv = dev.cpu().numpy().reshape(-1, 4), want.reshape(-1, 4)
    bad = np.nonzero(np.any(g != wv, axis=1))[0]
    assert bad.size == 0, (f"{bad.size} pixels differ, first ({bad[0] % w}, {bad[0] // w}): "
                           f"gpu={g[bad[0]]} oracle={wv[bad[0]]}")
    # the frame is not trivially empty: some pixel is not the background (far from the grid
    # every ray runs out of steps in empty space)
    if not case[-1].startswith(("far_", "camera_at_")):
        assert len(np.unique(g, axis=0)) > 4


def test_light_dd_pass_is_the_exact_threshold(built):
    """sfrt_voxel_light_dd_pass (the kernel's per-wave light skip): the light's test
    `intensity / dd - dd * 0.002f > 0` (World.cpp:425-426, binary32 as numpy evaluates it) holds
    just below the threshold and fails at it and at a spread of larger dd.  CPU only."""
    import sfrt
    f32 = np.float32
    L = sfrt.lib()
    rng = np.random.default_rng(11)
    intensities = np.concatenate([[2.0, 1.0, 0.5, 7.25, 1e-3, 1e6, 0.0, -1.0, np.inf],
                                  rng.random(200) * 50.0]).astype(f32)

    def adds(i, dd):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            return bool(f32(f32(i / dd) - f32(dd * f32(0.002))) > f32(0))

    for i in intensities:
        t = f32(L.sfrt_voxel_light_dd_pass(float(i)))
        if t == 0:
            assert not adds(i, f32(0)), i
            continue
        assert not adds(i, t), (i, t)
        assert adds(i, np.nextafter(t, f32(0))), (i, t)
        for m in (1.0001, 1.5, 10.0, 1e6):
            assert not adds(i, f32(t * f32(m))), (i, t, m)


def test_fast_dda_step_bound():
    """The fast primary DDA's bound (sfrt_voxel.cpp dda_qlim): one step of World::Raycast
    (World.cpp:330-350, binary32 as numpy evaluates it) moves each coordinate by at most
    2.001 Q + 0.003 X + 33 with X = max|d_k|, Q = X / min|d_k|, for positions below 2^30 --
    including negative positions, whose negative fractions give negative ray speeds, and
    directions with tiny components.  CPU only: random walks from cameras spread over
    [-2^29, 2^29] with directions spread over twenty binades."""
    f32 = np.float32
    rng = np.random.default_rng(7)
    n = 20000
    d = (rng.choice([-1.0, 1.0], (n, 3)) * 2.0 ** rng.uniform(-12, 8, (n, 3))).astype(f32)
    p = (rng.choice([-1.0, 1.0], (n, 3)) * 2.0 ** rng.uniform(-4, 29, (n, 3))).astype(f32)
    ad = np.abs(d)
    X = ad.max(axis=1).astype(np.float64)
    Q = X / ad.min(axis=1)
    S = 2.001 * Q + 0.003 * X + 33.0
    add = (d > 0).astype(f32)
    sgn = np.where(d > 0, f32(-1), f32(1))
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(40):
            ip = np.trunc(p)                               # (float)(int)pos, |pos| < 2^30
            ray = (add + sgn * (p - ip)).astype(f32) / ad  # xray, yray, zray
            ax = (ray[:, 0] <= ray[:, 1]) & (ray[:, 0] <= ray[:, 2])
            ay = ~ax & (ray[:, 1] <= ray[:, 0]) & (ray[:, 1] <= ray[:, 2])
            rs = np.where(ax, ray[:, 0], np.where(ay, ray[:, 1], ray[:, 2])).astype(f32)
            rs2 = (rs + f32(0.002)).astype(f32)
            step = np.stack([np.where(ax, rs2, rs), np.where(ay, rs2, rs),
                             np.where(ax | ay, rs, rs2)], axis=1).astype(f32)
            q = (p + (d * step).astype(f32)).astype(f32)
            live = np.all(np.abs(q) < 2.0 ** 30, axis=1) & np.all(np.abs(p) < 2.0 ** 30, axis=1)
            moved = np.abs(q.astype(np.float64) - p.astype(np.float64)).max(axis=1)
            assert np.all(moved[live] <= S[live]), moved[live][moved[live] > S[live]][:5]
            p = np.where(live[:, None], q, p)


def test_light_skip_fma_distance_bound():
    """The kernel's per-wave light skip tests ddf = fma(ex, ex, fma(ey, ey, ez * ez)) against
    dd_skip = RU(dd_pass / (1 - 2^-20)) (voxel_trace.h VoxLight): sound because the reference's
    dd = (ex*ex + ey*ey) + ez*ez (World.cpp:424, binary32) is never below ddf * (1 - 2^-20).
    CPU only: 10^6 random offsets over sixty binades, fma emulated in binary64 (the products of
    binary32 values are exact there)."""
    f32 = np.float32
    rng = np.random.default_rng(11)
    n = 1_000_000
    e = (rng.choice([-1.0, 1.0], (n, 3)) * 2.0 ** rng.uniform(-30, 30, (n, 3))).astype(f32)
    ex, ey, ez = (e[:, k] for k in range(3))
    dd = ((ex * ex + ey * ey).astype(f32) + ez * ez).astype(f32)
    zz = (ez * ez).astype(f32)
    inner = (ey.astype(np.float64) * ey + zz).astype(f32)
    ddf = (ex.astype(np.float64) * ex + inner).astype(f32)
    assert np.all(dd.astype(np.float64) >= ddf.astype(np.float64) * (1.0 - 2.0 ** -20))


@pytest.mark.gpu
def test_voxel_gpu_random_worlds(vworld, assets):
    """Random worlds (voxel_scenes.random_world: grid sizes 8-48 x 4-12 x 8-48, textures and
    colours, billboards near the camera, lights with and without shadows, random view and
    shadow distances, ragged frame sizes) rendered by the kernel against the restatement, byte
    for byte: the round-5 DDA (byte key space, one exit per step, the billboard stop through the
    step distance, the hit axis after the loop) on worlds the default snapshot does not cover."""
    import torch
    stream = torch.cuda.Stream()
    lit = billboards = 0
    for seed in range(24):
        scene, w, h = vs.random_world(seed)
        o = oracle.VoxelOracle(scene, w, h, assets[0], assets[1], vs.COLORS)
        want = o.render(host_threads())
        vworld.set_scene(scene, w, h)
        dev = poisoned((h, w * 4))
        vworld.render_band(dev.data_ptr(), w * 4, 0, h, stream.cuda_stream)
        vworld.check(stream.cuda_stream)
        g, wv = dev.cpu().numpy().reshape(-1, 4), want.reshape(-1, 4)
        bad = np.nonzero(np.any(g != wv, axis=1))[0]
        assert bad.size == 0, (seed, f"{bad.size} pixels differ, first ({bad[0] % w}, "
                               f"{bad[0] // w}): gpu={g[bad[0]]} oracle={wv[bad[0]]}")
        lit += scene.lights.shape[0] > 0
        billboards += scene.dyn.shape[0] > 0
    assert lit >= 12 and billboards >= 12


def test_random_worlds_oracle_deterministic(assets):
    """The random worlds of test_voxel_gpu_random_worlds on the CPU: the generator is
    deterministic, the restatement renders them the same with 1 and 8 threads, and none of
    them makes the reference read outside a texture (so the GPU test's frames are defined)."""
    for seed in (0, 5, 11, 17, 23):
        scene, w, h = vs.random_world(seed)
        again, w2, h2 = vs.random_world(seed)
        assert (w, h) == (w2, h2) and np.array_equal(scene.blocks, again.blocks)
        assert np.array_equal(scene.dyn, again.dyn) and np.array_equal(scene.lights, again.lights)
        o = oracle.VoxelOracle(scene, w, h, assets[0], assets[1], vs.COLORS)
        before = oracle.VoxelOracle.bad_texel_reads()
        a = o.render(8)
        assert oracle.VoxelOracle.bad_texel_reads() == before, seed
        assert np.array_equal(a, o.render(1)), seed


@pytest.mark.gpu
def test_voxel_blocks_rewrite_does_not_serialise_other_streams(built, assets):
    """VERDICT r5 item 2 (sfrt_voxel.cpp blocks_upload, sfrt_host.h SharedBuffer): new blocks
    while 4K sphere frames are in flight on stream A.  The voxel frame on stream B rewrites the
    grid stream-ordered -- behind the voxel launches that read the old grid, not behind A -- so
    the call returns and B's frame completes while A is still busy (the round-5 code's
    hipDeviceSynchronize held both until A drained).  The rewritten grid's frames equal the
    restatement: same dimensions, then smaller (the box of the old world cleared) and larger
    (100 x 10 x 100: a new allocation) worlds, each rewrite queued on A with a frame of the old
    world still queued on B."""
    import time
    import sfrt
    import scenes
    import torch
    w, h = 320, 180
    # B at high priority: HIP maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES), and two
    # streams that share one run in order whatever the library does; a high-priority stream comes
    # from another queue pool, so B never sits behind A's packets in hardware
    a, b = torch.cuda.Stream(), torch.cuda.Stream(priority=-1)
    tex, tw, th = scenes.load_floor()
    sphere = sfrt.World(0)
    vworld = sfrt.VoxelWorld(0)  # its own grid: the first world allocates it, the last grows it
    vworld.load_assets(assets[0], assets[1], vs.COLORS)
    try:
        sphere.load_texture(tex, tw, th)
        sphere.set_scene(scenes.lcg64(), 3840, 2160)
        frame4k = torch.empty((2160, 3840 * 4), dtype=torch.uint8, device="cuda:0")
        sphere.render_band(frame4k.data_ptr(), 3840 * 4, 0, 2160, a.cuda_stream)  # warm
        worlds = [vs.random_world(seed) for seed in (2, 9, 14)]
        first, fw, fh = worlds[0]
        vworld.set_scene(first, fw, fh)
        warm = torch.empty((fh, fw * 4), dtype=torch.uint8, device="cuda:0")
        vworld.render_band(warm.data_ptr(), fw * 4, 0, fh, b.cuda_stream)
        vworld.check(b.cuda_stream)
        torch.cuda.synchronize()
        # same dimensions, new blocks: no allocation on the way
        import dataclasses
        blocks2 = first.blocks.copy()
        textured = (blocks2 >= 0) & (blocks2 != vs.EMPTY)
        blocks2[textured] = (blocks2[textured] + 1) % 4  # the same cells, other textures
        second = dataclasses.replace(first, blocks=blocks2)
        got = poisoned((fh, fw * 4))  # filled before A is busy
        for _ in range(40):  # ~6 ms of sphere frames queued on A
            sphere.render_band(frame4k.data_ptr(), 3840 * 4, 0, 2160, a.cuda_stream)
        t0 = time.perf_counter()
        vworld.set_scene(second, fw, fh)
        vworld.render_band(got.data_ptr(), fw * 4, 0, fh, b.cuda_stream)
        done_b = torch.cuda.Event()
        done_b.record(b)
        call_s = time.perf_counter() - t0
        a_busy_after_call = not a.query()
        while not done_b.query():
            pass
        a_busy_after_b = not a.query()
        torch.cuda.synchronize()
        assert a_busy_after_call, f"the voxel call returned only after A drained ({call_s * 1e3:.2f} ms)"
        assert a_busy_after_b, "B's voxel frame waited for the sphere frames on A"
        vworld.check(b.cuda_stream)
        want = oracle.VoxelOracle(second, fw, fh, assets[0], assets[1], vs.COLORS).render(host_threads())
        assert np.array_equal(got.cpu().numpy().ravel(), want)
        # smaller and larger worlds, the previous world's frame queued on B ahead of each rewrite
        prev = (second, fw, fh)
        for scene, sw, sh in worlds[1:] + [(vs.default_world(), 320, 180)]:
            vworld.set_scene(prev[0], prev[1], prev[2])
            old = poisoned((prev[2], prev[1] * 4))
            with torch.cuda.stream(b):
                torch.cuda._sleep(20_000_000)  # the old world's frame still queued behind this
            vworld.render_band(old.data_ptr(), prev[1] * 4, 0, prev[2], b.cuda_stream)
            vworld.set_scene(scene, sw, sh)
            new = poisoned((sh, sw * 4))
            vworld.render_band(new.data_ptr(), sw * 4, 0, sh, a.cuda_stream)  # rewrite on A
            torch.cuda.synchronize()
            vworld.check(a.cuda_stream)
            vworld.check(b.cuda_stream)
            for sc, ww, hh, buf in ((prev[0], prev[1], prev[2], old), (scene, sw, sh, new)):
                want = oracle.VoxelOracle(sc, ww, hh, assets[0], assets[1], vs.COLORS).render(
                    host_threads())
                assert np.array_equal(buf.cpu().numpy().ravel(), want), (ww, hh, sc.blocks.shape)
            prev = (scene, sw, sh)
    finally:
        sphere.close()
        vworld.close()


def _aliasing_worlds():
    """Worlds at the key space's limits (nz = 1024, ny = 1024), where the reference's map key
    (x << 20) + (y << 10) + z (World.cpp:385) makes a cell past the last column alias the next
    row's first (z = 1024 is (x, y + 1, 0)) and a cell past the last row the next plane's (y = 1024
    is (x + 1, 0, z)): rays leaving the world there see those blocks, in the reference and -- as
    the grid is stored in that key space -- in the kernel."""
    E = vs.EMPTY
    out = []
    # nz = 1024: a floor, and blocks in the first columns z = 0..3 of rows y = 2..5, which the rays
    # crossing z = 1024 at rows 1..4 meet; the camera near the far end, looking along +z
    b = np.full((4, 8, 1024), E, dtype=np.int16)
    b[:, 0, :] = 1
    b[:, 2:6, 0:4] = 3
    b[0, :, :] = b[-1, :, :] = 0
    light = np.zeros(1, dtype=vs.LIGHT_DTYPE)
    light[0]["pos"], light[0]["intensity"] = (2.0, 3.0, 1020.0), 8.0
    light[0]["r"] = light[0]["g"] = light[0]["b"] = 1.0
    light[0]["shadows"] = 1
    out.append(("z_wraps_to_next_row",
                vs.VoxelScene(b, np.zeros(0, dtype=vs.DYN_DTYPE), light, (2.5, 2.5, 1019.5), 0.0, 0.1,
                              view_distance=40.0)))
    # ny = 1024: blocks on the floor of plane x = 2, which rays of plane x = 1 crossing y = 1024
    # meet; the camera high up in plane 1, looking up
    b = np.full((4, 1024, 8), E, dtype=np.int16)
    b[2, 0, :] = 2
    b[2, 1, 2:6] = -1
    b[1, 1020, 0] = 0
    out.append(("y_wraps_to_next_plane",
                vs.VoxelScene(b, np.zeros(0, dtype=vs.DYN_DTYPE), np.zeros(0, dtype=vs.LIGHT_DTYPE),
                              (1.5, 1021.5, 4.5), 0.3, 1.2, view_distance=40.0)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,scene", _aliasing_worlds(), ids=[n for n, _ in _aliasing_worlds()])
def test_voxel_gpu_key_aliasing_matches_oracle(built, assets, name, scene):
    """The key space's aliasing (_aliasing_worlds) byte for byte against the restatement, on a
    world object of its own (these grids are 4 MiB of keys; the rewrite clears them stream-ordered),
    and the aliasing really shows: the frame differs from the same world with the aliased blocks
    removed."""
    import sfrt
    import torch
    w, h = 256, 144
    vw = sfrt.VoxelWorld(0)
    try:
        vw.load_assets(assets[0], assets[1], vs.COLORS)
        frames = []
        for sc in (scene, None):
            if sc is None:  # the control: the aliased blocks gone
                b = scene.blocks.copy()
                if name.startswith("z_"):
                    b[:, 2:6, 0:4] = vs.EMPTY
                else:
                    b[2, 0, :] = vs.EMPTY
                    b[2, 1, 2:6] = vs.EMPTY
                import dataclasses
                sc = dataclasses.replace(scene, blocks=b)
            want = oracle.VoxelOracle(sc, w, h, assets[0], assets[1], vs.COLORS).render(host_threads())
            vw.set_scene(sc, w, h)
            stream = torch.cuda.Stream()
            dev = poisoned((h, w * 4))
            vw.render_band(dev.data_ptr(), w * 4, 0, h, stream.cuda_stream)
            vw.check(stream.cuda_stream)
            got = dev.cpu().numpy().ravel()
            g, wv = got.reshape(-1, 4), want.reshape(-1, 4)
            bad = np.nonzero(np.any(g != wv, axis=1))[0]
            assert bad.size == 0, (name, f"{bad.size} pixels differ, first ({bad[0] % w}, "
                                   f"{bad[0] // w}): gpu={g[bad[0]]} oracle={wv[bad[0]]}")
            frames.append(got)
        assert not np.array_equal(frames[0], frames[1]), f"{name}: no aliased block in view"
    finally:
        vw.close()


@pytest.mark.gpu
def test_voxel_texture_upload_is_stream_ordered(built, assets):
    """sfrt_voxel_load_texture without a device-wide wait (sfrt_voxel.cpp upload_texture,
    sfrt::SharedBuffer): a frame on stream B queued behind ~50 ms of work still reads the texture
    it was queued with when textures[0] is replaced right after; the call returns while B is busy;
    both frames equal the restatement with their own texture set, also for a larger texture (a new
    buffer)."""
    import sfrt
    import torch
    w, h = 320, 180
    case = (w, h, (20.5, 2.2, 40.5), 1.0, 0.1)
    scene, _ = voxel_oracle(case, assets)
    rng = np.random.default_rng(3)
    tex0 = list(assets[0])
    alt = [(rng.integers(0, 256, t[1] * t[2] * 4, dtype=np.uint8), t[1], t[2]) for t in tex0[:1]]
    big = (rng.integers(0, 256, 128 * 128 * 4, dtype=np.uint8), 128, 128)
    sets = [tex0, [alt[0]] + tex0[1:], [big] + tex0[1:], tex0]
    vw = sfrt.VoxelWorld(0)
    try:
        vw.load_assets(sets[0], assets[1], vs.COLORS)
        vw.set_scene(scene, w, h)
        # B at high priority: the object's own stream, where the upload runs, never shares B's
        # hardware queue (two streams that share one run in order, GPU_MAX_HW_QUEUES)
        a, b = torch.cuda.Stream(), torch.cuda.Stream(priority=-1)
        warm = torch.empty((h, w * 4), dtype=torch.uint8, device="cuda:0")
        vw.render_band(warm.data_ptr(), w * 4, 0, h, a.cuda_stream)
        torch.cuda.synchronize()
        frames = []
        for k in range(1, len(sets)):
            old, new = poisoned((h, w * 4)), poisoned((h, w * 4))  # filled before B is busy
            with torch.cuda.stream(b):
                torch.cuda._sleep(100_000_000)
            vw.render_band(old.data_ptr(), w * 4, 0, h, b.cuda_stream)    # reads sets[k - 1]
            rgba, tw, th = sets[k][0]
            vw.load_texture(0, rgba, tw, th)
            busy = not b.query()
            vw.render_band(new.data_ptr(), w * 4, 0, h, a.cuda_stream)    # reads sets[k]
            frames.append((sets[k - 1], old, sets[k], new, busy))
            torch.cuda.synchronize()
        vw.check(a.cuda_stream)
        vw.check(b.cuda_stream)
        for t_old, old, t_new, new, busy in frames:
            assert busy, "load_texture waited for the queued frame on B"
            for t, buf in ((t_old, old), (t_new, new)):
                want = oracle.VoxelOracle(scene, w, h, t, assets[1], vs.COLORS).render(host_threads())
                assert np.array_equal(buf.cpu().numpy().ravel(), want)
    finally:
        vw.close()
