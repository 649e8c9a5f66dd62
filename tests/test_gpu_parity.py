"""GPU parity: libsfrt.so (HIP, gfx950) against the CPU restatement, byte for byte.

Every frame here goes through the C ABI (sfrt.World -> libsfrt.so).  The
oracle (oracle/, TEST INFRASTRUCTURE) renders the same scene on the host
cores; frames too large for that in seconds are checked against the committed
golden hashes in tests/golden/golden.json instead.  Bar: RGBA8 bit-exact;
float intermediates (march position, xcoord, ycoord, brightness) within
1e-5 absolute (they are in fact expected to be identical) and integer ones
(drawSphere, iterations, texel) exact.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import scenes
from conftest import ROOT, host_threads, poisoned

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
FLOAT_TOL = 1e-5


@pytest.fixture(scope="module")
def world(built, floor):
    import sfrt
    w = sfrt.World(0)
    w.load_texture(*floor)
    yield w
    w.close()


def oracle_for(scene, width, height, floor):
    import oracle
    return oracle.Oracle.from_scene(scene, width, height, *floor)


def diff_report(got, want, width):
    g = got.reshape(-1, 4)
    w = want.reshape(-1, 4)
    bad = np.nonzero(np.any(g != w, axis=1))[0]
    if bad.size == 0:
        return ""
    k = int(bad[0])
    return (f"{bad.size} pixels differ; first at (i={k % width}, j={k // width}): "
            f"gpu={g[k].tolist()} oracle={w[k].tolist()}")


ORACLE_CASES = [
    ("c1_320x240_one_sphere", (0.0, 0.0)),
    ("c2_1920x1080_default10", (0.0, 0.0)),
    ("c2_1920x1080_default10", (0.7, 0.3)),
    ("c3_3840x2160_lcg64", (0.0, 0.0)),
    ("c3_3840x2160_lcg64", (1.1, -0.2)),
    ("c3_3840x2160_default10", (0.0, 0.0)),
]


@pytest.mark.parametrize("cfg,pose", ORACLE_CASES)
def test_full_frame_matches_oracle(world, floor, cfg, pose):
    width, height, sname, _ = scenes.CONFIGS[cfg]
    scene = scenes.SCENES[sname]().posed(*pose)
    world.set_scene(scene, width, height)
    got = world.render()
    want = oracle_for(scene, width, height, floor).render(host_threads())
    msg = diff_report(got, want, width)
    assert not msg, f"{cfg} pose={pose}: {msg}"


@pytest.mark.parametrize("key", sorted(
    k for k, g in GOLDEN["frames"].items()
    if (g["config"], tuple(g["pose"])) not in ORACLE_CASES))
def test_large_frame_matches_golden_hash(world, key):
    """Every golden frame the oracle does not render here in seconds -- 8K and 16384^2 (configs 4
    and 5, both scenes), the 3840 x 2160*N weak-scaling frames of bench.py --gpus N, the 256-sphere
    4K frame: device render, FNV-1a-64 vs the committed oracle hash."""
    import oracle
    g = GOLDEN["frames"][key]
    scene = scenes.SCENES[g["scene"]]().posed(*g["pose"])
    world.set_scene(scene, g["width"], g["height"])
    got = world.render()
    assert oracle.fnv1a64(got) == g["fnv1a64"], key


def test_cull_on_off_identical(world, floor):
    """Per-wave culling must not change a byte (A/B over the rotated 64-sphere 4K pose)."""
    import sfrt
    scene = scenes.lcg64().posed(1.1, -0.2)
    world.set_scene(scene, 3840, 2160)
    a = world.render()
    world.set_option(sfrt.SFRT_OPT_CULL, 0)
    try:
        b = world.render()
    finally:
        world.set_option(sfrt.SFRT_OPT_CULL, 1)
    assert diff_report(a, b, 3840) == ""


@pytest.mark.parametrize("rays", [1, 2, 3, 4])
def test_tile_shapes_identical(world, floor, rays):
    """Every shipped tile shape ((8R)x8 tiles, R pixels per lane, forced with
    SFRT_OPT_RAYS_PER_LANE; the kernel-argument kernel up to 64 spheres, the culled-list
    kernel above) produces the default kernel's bytes, in row-major order (update_image) and
    in the adaptive tile order (three render_band frames back to back), on ragged frames
    (64 spheres, 4K, rotated pose; random poses of four scenes, 256 spheres among them)."""
    import sfrt
    import torch
    cases = [(scenes.lcg64(), (1.1, -0.2), 3840, 2160)]
    rng = np.random.default_rng(rays)
    for sc in (scenes.lcg64(), scenes.default10(), scenes.one_sphere(), scenes.lcg256()):
        for _ in range(4 if sc.name != "lcg256" else 2):
            cases.append((sc, (float(rng.uniform(0, 6.3)), float(rng.uniform(-0.6, 0.6))), 1000, 563))
    stream = torch.cuda.Stream()
    for sc, pose, width, height in cases:
        world.set_scene(sc.posed(*pose), width, height)
        a = world.render()
        world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
        try:
            b = world.render()
            assert diff_report(a, b, width) == "", (sc.name, pose, "row-major")
            bufs = []
            for _ in range(3):
                buf = poisoned((height, width * 4))
                torch.cuda.synchronize()
                world.render_band(buf.data_ptr(), width * 4, 0, height, stream.cuda_stream)
                bufs.append(buf)
            world.check(stream.cuda_stream)
            torch.cuda.synchronize()
        finally:
            world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, 0)
        for k, buf in enumerate(bufs):
            assert diff_report(buf.cpu().numpy().ravel(), a, width) == "", (sc.name, pose, "ordered", k)


@pytest.mark.parametrize("count", [65, 120, 199, 1023])
def test_global_window_cull_on_off(world, floor, count):
    """n > 64 (8x8 tiles, multi-word culling masks, march windows in LDS): culling and the
    window on equal culling off (every sphere every step) for several poses, and the oracle
    for one of them."""
    import sfrt
    spheres = scenes.sort_spheres(scenes.lcg_spheres(count=count - 1, seed=31 + count))
    rng = np.random.default_rng(count)
    for q in range(4):
        pose = (float(rng.uniform(0, 6.3)), float(rng.uniform(-0.6, 0.6)))
        scene = scenes.Scene("many", spheres).posed(*pose)
        world.set_scene(scene, 1000, 563)
        a = world.render()
        world.set_option(sfrt.SFRT_OPT_CULL, 0)
        try:
            b = world.render()
        finally:
            world.set_option(sfrt.SFRT_OPT_CULL, 1)
        assert diff_report(a, b, 1000) == "", (count, pose)
        if q == 0 and count <= 200:
            want = oracle_for(scene, 1000, 563, floor).render(host_threads())
            assert diff_report(a, want, 1000) == "", (count, pose)


@pytest.mark.parametrize("ystart,yadd,xstart,xadd", [
    (0, 8, 0, 4), (3, 8, 2, 4), (7, 8, 3, 4),   # RenderThread interleave (Source.cpp:21,23)
    (1, 3, 0, 1), (0, 1, 5, 7), (239, 1, 319, 1), (5, 1000, 0, 1)])
def test_update_image_subset_writes_only_addressed(world, floor, ystart, yadd, xstart, xadd):
    width, height = 320, 240
    scene = scenes.default10().posed(0.7, 0.3)
    world.set_scene(scene, width, height)
    canvas = np.full(width * height * 4, 0xA5, dtype=np.uint8)
    expect = canvas.copy()
    world.update_image(canvas, ystart, yadd, xstart, xadd)
    oracle_for(scene, width, height, floor).update_image(expect, ystart, yadd, xstart, xadd)
    assert diff_report(canvas, expect, width) == ""


def test_row_bands_tile_the_frame(world, floor):
    """Multi-GPU row bands: bands rendered separately == the single-launch frame."""
    import torch
    width, height = 1920, 1080
    scene = scenes.lcg64().posed(0.3, 0.1)
    world.set_scene(scene, width, height)
    full = torch.zeros(height, width * 4, dtype=torch.uint8, device="cuda:0")
    bands = torch.zeros_like(full)
    stream = torch.cuda.current_stream().cuda_stream
    world.render_band(full.data_ptr(), width * 4, 0, height, stream)
    for r0, r1 in [(0, 1), (1, 270), (270, 541), (541, 1079), (1079, 1080)]:
        world.render_band(bands[r0].data_ptr(), width * 4, r0, r1 - r0, stream)
    world.check(stream)
    torch.cuda.synchronize()
    f = full.cpu().numpy().ravel()
    b = bands.cpu().numpy().ravel()
    assert diff_report(b, f, width) == ""
    want = oracle_for(scene, width, height, floor).render(host_threads())
    assert diff_report(f, want, width) == ""


def _check_dumps(world, floor, scene, width, height, n, seed, what):
    rng = np.random.default_rng(seed)
    ij = np.stack([rng.integers(0, width, n), rng.integers(0, height, n)], axis=1)
    ij[:4] = [[0, 0], [width - 1, height - 1], [width - 1, 0], [0, height - 1]]  # frame corners
    ij[4] = ij[5]  # a repeated pixel
    got = world.trace_points(ij)
    orc = oracle_for(scene, width, height, floor)
    identical = 0
    for (i, j), g in zip(ij.tolist(), got):
        w = orc.dump(i, j)
        assert (g["draw"], g["iters"], g["texel"], g["rgba"]) == \
               (w["draw"], w["iters"], w["texel"], w["rgba"]), (what, i, j, g, w)
        for k in ("xcoord", "ycoord", "brightness"):
            assert abs(g[k] - w[k]) <= FLOAT_TOL, (what, i, j, k, g[k], w[k])
        assert max(abs(a - b) for a, b in zip(g["pos"], w["pos"])) <= FLOAT_TOL, (what, i, j)
        identical += all(np.float32(g[k]) == np.float32(w[k]) for k in ("xcoord", "ycoord", "brightness")) \
            and all(np.float32(a) == np.float32(b) for a, b in zip(g["pos"], w["pos"]))
    return identical


# golden DUMP_CONFIGS (tests/golden/make_golden.py)
DUMP_CASES = [("c2_1920x1080_default10", (0.7, 0.3)), ("c3_3840x2160_lcg64", (0.0, 0.0))]


@pytest.mark.parametrize("cfg,pose", DUMP_CASES)
@pytest.mark.parametrize("rays", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("order", [1, 0])
def test_float_intermediates(world, floor, cfg, pose, rays, order):
    """north_star: float intermediates of SphereWorld.cpp:362-375 (march position, xcoord,
    ycoord, brightness) within 1e-5 of the oracle, integers (drawSphere, loop trips, texel,
    RGBA8) exact -- read out of the SHIPPED frame-fill kernel (its DUMP instantiation:
    sfrt_world_trace_points renders the whole frame through k_trace_window_r<R>), for every
    tile shape R (0 = the kernel table's pick) in the adaptive tile order (three launches,
    the last one sorted) and in row-major order."""
    import sfrt
    width, height, sname, _ = scenes.CONFIGS[cfg]
    scene = scenes.SCENES[sname]().posed(*pose)
    world.set_scene(scene, width, height)
    world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
    world.set_option(sfrt.SFRT_OPT_TILE_ORDER, order)
    try:
        same = _check_dumps(world, floor, scene, width, height, 1000, 1234 + rays, (cfg, rays, order))
    finally:
        world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, 0)
        world.set_option(sfrt.SFRT_OPT_TILE_ORDER, 1)
    assert same == 1000  # the tolerance is the bar; the floats are in fact identical


@pytest.mark.parametrize("rays", [0, 2, 4])
def test_float_intermediates_list_kernel(world, floor, rays):
    """n > 64 (256 spheres: the culled-list kernel k_trace_window_list<R>) in the adaptive
    tile order: the shipped kernel's intermediates against the oracle."""
    import sfrt
    scene = scenes.lcg256().posed(1.1, -0.2)
    world.set_scene(scene, 1600, 1200)
    world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
    try:
        same = _check_dumps(world, floor, scene, 1600, 1200, 600, 99 + rays, ("lcg256", rays))
    finally:
        world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, 0)
    assert same == 600


@pytest.mark.parametrize("rays", [1, 3])
def test_float_intermediates_list_kernel_other_tile_shapes(world, floor, rays):
    """k_trace_window_list_dump<R> at the two tile shapes the test above leaves out, on a 40x24
    frame (partial tiles at either width) of 65 spheres, the fewest that take the list kernel."""
    import sfrt
    spheres = scenes.sort_spheres(scenes.lcg_spheres(count=64, seed=96))
    scene = scenes.Scene("many65", spheres).posed(1.1, -0.2)
    world.set_scene(scene, 40, 24)
    world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
    try:
        same = _check_dumps(world, floor, scene, 40, 24, 200, 77 + rays, ("many65", rays))
    finally:
        world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, 0)
    assert same == 200


def test_trace_points_frame_equals_render(world, floor):
    """The DUMP instantiation writes the same frame as the shipped kernel: the rgba of every
    pixel of a small frame out of trace_points equals render()'s bytes."""
    scene = scenes.lcg64().posed(0.4, 0.2)
    width, height = 96, 40
    world.set_scene(scene, width, height)
    jj, ii = np.mgrid[0:height, 0:width]
    got = world.trace_points(np.stack([ii.ravel(), jj.ravel()], axis=1))
    frame = np.array([g["rgba"] for g in got], dtype=np.uint8).ravel()
    assert diff_report(frame, world.render(), width) == ""


def test_trace_points_16k_frame_listed_pixels(world, floor):
    """trace_points on the 16384^2 config-5 frame: memory and uploads are O(listed pixels)
    (sorted distinct pixel ids, binary-searched in the DUMP epilogue; no frame buffer), and the
    records of a few pixels -- corners, a repeat, random -- equal the oracle's dumps."""
    scene = scenes.lcg64()
    world.set_scene(scene, 16384, 16384)
    same = _check_dumps(world, floor, scene, 16384, 16384, 24, 7, "c5 lcg64")
    assert same == 24


def test_trace_points_leaves_row_costs_and_order(world, floor):
    """The dump runs on a private tile-order chain: the world's last fill (row costs) and the
    next frame's order are those of the caller's last render_band, before and after it."""
    import torch
    scene = scenes.lcg64().posed(1.1, -0.2)
    width, height = 1920, 1080
    world.set_scene(scene, width, height)
    buf = torch.empty(height, width * 4, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        world.render_band(buf.data_ptr(), width * 4, 200, 600)
    before = world.row_costs()
    world.trace_points(np.array([[5, 7], [600, 300], [1919, 1079]]))  # whole-frame DUMP passes
    after = world.row_costs()
    assert before[0] == after[0] == 200
    np.testing.assert_array_equal(before[1], after[1])
    world.render_band(buf.data_ptr(), width * 4, 200, 600)
    world.check()
    want = oracle_for(scene, width, height, floor).render_band(200, 600)
    assert np.array_equal(buf[:600].cpu().numpy().ravel(), want)


def test_camera_outside_every_sphere(world, floor):
    """largestDist == 0 on the first iteration: every pixel shades sphere 0 at cam.pos."""
    scene = scenes.Scene("outside", np.array([[50, 0, 0, 2], [0, 40, 0, 3]], np.float32),
                         cam_pos=(0.5, -0.25, 0.125))
    world.set_scene(scene, 160, 96)
    got = world.render()
    want = oracle_for(scene, 160, 96, floor).render(1)
    assert diff_report(got, want, 160) == ""


@pytest.mark.parametrize("case", ["far2^40", "far2^100", "tiny2^-30"])
def test_extreme_scale_scene_matches_oracle(world, floor, case):
    """Extreme coordinates, in both tile orders, against the oracle: sphere 0 of the default
    scene moved to ~2^40 or ~2^100 (sphere 0 is drawSphere for rays that leave every sphere,
    so the shading tail's division guards see huge or infinite operands, and the 2^100 frame
    has a non-finite reach: no culling), and the whole scene scaled by 2^-30 (every radius
    below the 0.01 pass threshold).  Scaling the whole scene up does not work as a test: at
    ~2^37 a step smaller than half an ulp of the position leaves it unchanged and the
    reference's loop (SphereWorld.cpp:362-371) never ends -- the oracle's neither."""
    import sfrt
    base = scenes.default10()
    sp = base.spheres.copy()
    cam = base.cam_pos
    if case == "tiny2^-30":
        sp[:, :4] *= np.float32(2.0 ** -30)
        cam = tuple(float(v) * 2.0 ** -30 for v in cam)
    else:
        far = 2.0 ** (40 if case == "far2^40" else 100)
        sp[0, :3] = np.float32([far, -far / 2, far])
    scene = scenes.Scene(f"default10_{case}", sp, cam_pos=cam)
    want = oracle_for(scene, 192, 108, floor).render(host_threads())
    for order in (0, 1):
        world.set_option(sfrt.SFRT_OPT_TILE_ORDER, order)
        world.set_scene(scene, 192, 108)
        got = world.render()
        assert diff_report(got, want, 192) == "", f"{case}, tile order {order}"
    world.set_option(sfrt.SFRT_OPT_TILE_ORDER, 1)


@pytest.mark.parametrize("pose", [(0.0, 0.0), (1.1, -0.2)])
def test_lcg256_ordered_frames_match_oracle(world, floor, pose):
    """256 spheres (the culled-list kernel, 32x8 tiles at 1600 x 1200 in the adaptive tile
    order, four frames back to back) against the oracle."""
    import torch
    width, height = 1600, 1200
    scene = scenes.lcg256().posed(*pose)
    world.set_scene(scene, width, height)
    want = oracle_for(scene, width, height, floor).render(host_threads())
    stream = torch.cuda.Stream()
    bufs = []
    with torch.cuda.stream(stream):
        for _ in range(4):
            b = poisoned((height, width * 4))
            world.render_band(b.data_ptr(), width * 4, 0, height, stream.cuda_stream)
            bufs.append(b)
    world.check(stream.cuda_stream)
    torch.cuda.synchronize()
    for k, b in enumerate(bufs):
        assert diff_report(b.cpu().numpy().ravel(), want, width) == "", (pose, k)
    assert diff_report(world.render(), want, width) == "", pose


def test_many_spheres_global_path(world, floor):
    """n > 64 takes the device-buffer kernel (culled list over multi-word masks)."""
    spheres = scenes.sort_spheres(scenes.lcg_spheres(count=199, seed=777))
    scene = scenes.Scene("lcg200", spheres).posed(0.4, -0.1)
    world.set_scene(scene, 640, 360)
    got = world.render()
    want = oracle_for(scene, 640, 360, floor).render(host_threads())
    assert diff_report(got, want, 640) == ""


@pytest.mark.parametrize("n_keep", [100, 127, 180])
def test_records_past_n_never_marched(built, floor, n_keep):
    """Device sphere slots keep records past n from an earlier, larger scene.

    Prime every slot of the ring with 192 records, then shrink the scene to
    its first n_keep spheres: a culling-mask word whose bit 31 is set must not
    widen to the stale indices above n (a sign-extended readfirstlane once
    did exactly that).  n_keep sits 4..63 past a 32-bit boundary of its word.
    """
    import sfrt
    full = scenes.sort_spheres(scenes.lcg_spheres(count=191, seed=4242))
    with sfrt.World(0) as w:
        w.load_texture(*floor)
        w.set_scene(scenes.Scene("prime", full).posed(0.0, 0.0), 64, 64)
        for _ in range(12):  # more renders than ring slots
            w.render()
        for pose in [(0.5, -0.1), (2.0, 0.05), (4.4, 0.1)]:
            scene = scenes.Scene("kept", full[:n_keep]).posed(*pose)
            w.set_scene(scene, 640, 360)
            want = oracle_for(scene, 640, 360, floor).render(host_threads())
            for _ in range(3):
                assert diff_report(w.render(), want, 640) == "", (n_keep, pose)


def test_ragged_sizes(world, floor):
    """Frame sizes that are not multiples of the 8x8 wave tile."""
    scene = scenes.lcg64().posed(2.0, 0.4)
    for width, height in [(1, 1), (7, 3), (333, 211), (1000, 9)]:
        world.set_scene(scene, width, height)
        got = world.render()
        want = oracle_for(scene, width, height, floor).render(host_threads())
        assert diff_report(got, want, width) == "", (width, height)


def test_errors_fail_loudly(world):
    import sfrt
    with pytest.raises(sfrt.SfrtError) as e:
        world.set_spheres(np.zeros((0, 4), np.float32))
        world.render()
    assert e.value.code == -2
    with pytest.raises(sfrt.SfrtError):
        world.set_spheres(np.array([[0, 0, 0, -1]], np.float32))
    with pytest.raises(sfrt.SfrtError):
        world.set_spheres(np.array([[0, 0, np.nan, 1]], np.float32))
    too_many = scenes.lcg_spheres(count=1024, seed=5)  # 1025 with the centre sphere
    assert too_many.shape[0] == 1025
    with pytest.raises(sfrt.SfrtError) as e:
        world.set_spheres(too_many)
    assert e.value.code == -4  # SFRT_E_TOO_MANY (SFRT_MAX_SPHERES = 1024)


def test_maximum_sphere_count_matches_oracle(world, floor):
    """SFRT_MAX_SPHERES = 1024 spheres (16 culling-mask words): equal to the oracle."""
    spheres = scenes.sort_spheres(scenes.lcg_spheres(count=1023, seed=99))
    assert spheres.shape[0] == 1024
    scene = scenes.Scene("lcg1024", spheres).posed(0.9, 0.1)
    world.set_scene(scene, 320, 180)
    want = oracle_for(scene, 320, 180, floor).render(host_threads())
    assert diff_report(world.render(), want, 320) == ""


@pytest.mark.parametrize("fn,arg", [("asinf", "1"), ("atanf", "1"), ("atan2f", "100000000"),
                                    ("sqrt_div", "16"), ("divpi", "1"), ("atan2f_x1", "1"), ("atan2f_wave", "400000000"),
                                    ("acosf", "1")])
def test_device_math_matches_libm(fn, arg, tmp_path):
    """sfrt_math on gfx950 vs host glibc: every binary32 input (atanf, asinf)."""
    exe = tmp_path / "math_gpu_check"
    src = os.path.join(ROOT, "tests", "native", "math_gpu_check.hip")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-fopenmp", src, "-o", str(exe)], check=True,
                   capture_output=True)
    env = dict(os.environ, OMP_NUM_THREADS=str(host_threads()))
    r = subprocess.run([str(exe), fn, arg], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "mismatches=0" in r.stdout, r.stdout + r.stderr


def test_device_div_recip(tmp_path):
    """sfrt_math::div_recip(a, b, 1/b) and sfrt::div_inrange(a, b) == a / b on gfx950
    (5 classes x 2^33 pairs)."""
    exe = tmp_path / "div_check"
    src = os.path.join(ROOT, "tests", "native", "div_check.hip")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                    "-ffp-contract=off", src, "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe), "33"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "mismatches=0" in r.stdout, r.stdout + r.stderr


def test_wave_helpers(tmp_path):
    """wave_min_u32 / wave_max_u32 / uniform_u64 (sfrt_device.h) against a lane loop, and
    sqrt_cr_normal in the march pass body for squared distances below 2^-96."""
    exe = tmp_path / "wave_check"
    src = os.path.join(ROOT, "tests", "native", "wave_check.hip")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                    src, "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mismatches=0" in r.stdout, r.stdout + r.stderr


def test_cpp_host_api(built, tmp_path):
    """include/sfrt.hpp driven from C++ like the reference drives SphereWorld and its
    shader (constructor scene, 8-thread RenderThread interleave, UpdateSpheres uniform
    uploads): frames equal the golden hashes (tests/native/cpp_api_check.cpp)."""
    exe = tmp_path / "cpp_api_check"
    lib_dir = os.path.join(ROOT, "sfml-software-raytracer_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "cpp_api_check.cpp"), "-L", lib_dir,
                    "-lsfrt", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath-link,/opt/rocm/lib",
                    "-lpthread", "-o", str(exe)], check=True, capture_output=True)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
    want_s = golden["frames"]["c2_1920x1080_default10@0,0"]["fnv1a64"]
    want_g = golden["glsl"]["default@320x180"]["fnv1a64"]
    r = subprocess.run([str(exe), os.path.join(lib_dir, "assets"), want_s, want_g],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "failures=0" in r.stdout, r.stdout + r.stderr


def test_pipelined_frames_match_oracle(world, floor):
    """Display path (the reference uploads the filled frame with
    screenTexture.loadFromImage, Source.cpp:141): two frames in flight through
    submit_frame / wait_frame into pinned host frames, the camera changing every frame.
    Each delivered frame equals the oracle's frame of its own pose, byte for byte."""
    import sfrt
    width, height = 640, 360
    scene = scenes.lcg64()
    poses = [(0.1 * k, 0.05 * (k % 3) - 0.05) for k in range(6)]
    want = {p: oracle_for(scene.posed(*p), width, height, floor).render(host_threads()) for p in poses}
    frames = [sfrt.HostFrame(width * height * 4) for _ in range(3)]
    world.set_scene(scene, width, height)
    tickets = []
    try:
        for k, pose in enumerate(poses):
            world.set_camera(scene.cam_pos, *pose)
            tickets.append((world.submit_frame(frames[k % 3]), k))
            if k >= 1:  # keep at most two frames in flight, check the older one
                t, kk = tickets.pop(0)
                world.wait_frame(t)
                assert diff_report(frames[kk % 3].array, want[poses[kk]], width) == "", kk
        for t, kk in tickets:
            world.wait_frame(t)
            assert diff_report(frames[kk % 3].array, want[poses[kk]], width) == "", kk
    finally:
        for fr in frames:
            fr.free()


def _fuzz_scene(seed):
    """A random scene/camera/frame: sphere counts on both sides of every kernel switch
    (8x8 vs pair kernel at 16, inline vs global at 64), caller (unsorted) order, cameras
    inside, outside, at a centre or near a surface, any pose and field of view."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([1, 2, 3, 7, 16, 17, 33, 64, 65, 130]))
    scale = float(rng.choice([5.0, 20.0, 60.0]))
    c = rng.uniform(-scale, scale, size=(n, 3))
    if rng.random() < 0.5:
        c = np.round(c)  # the reference's rand() scenes have integer centres
    r = rng.uniform(0.05, scale / 2, size=(n, 1))
    spheres = np.concatenate([c, r], axis=1).astype(np.float32)
    mode = int(rng.integers(4))
    k = int(rng.integers(n))
    if mode == 0:
        cam = spheres[k, :3]                                   # at a centre
    elif mode == 1:
        cam = spheres[k, :3] + rng.uniform(-0.5, 0.5, 3) * spheres[k, 3]  # inside
    elif mode == 2:
        d = rng.normal(size=3)
        cam = spheres[k, :3] + d / np.linalg.norm(d) * spheres[k, 3] * 0.999  # near the surface
    else:
        cam = rng.uniform(-2 * scale, 2 * scale, 3)            # anywhere (often outside)
    cam = tuple(float(x) for x in np.asarray(cam, dtype=np.float32))
    fov = (None, None) if rng.random() < 0.5 else (float(np.float32(rng.uniform(0.2, 1.5))),
                                                   float(np.float32(rng.uniform(0.2, 1.2))))
    sc = scenes.Scene(f"fuzz{seed}", spheres, cam_pos=cam,
                      rotation=float(np.float32(rng.uniform(-7, 7))),
                      hrotation=float(np.float32(rng.uniform(-1.5, 1.5))))
    if fov[0] is not None:
        sc.fov_h, sc.fov_v = np.float32(fov[0]), np.float32(fov[1])
    width, height = [(160, 90), (97, 61), (256, 8), (64, 200), (333, 41)][int(rng.integers(5))]
    return sc, width, height


@pytest.mark.parametrize("chunk", range(4))
def test_random_scenes_match_oracle(world, floor, chunk):
    """400 random scenes (100 per chunk) through the default kernels vs the oracle:
    culling, march windows and both tile shapes must never change a byte."""
    for seed in range(chunk * 100, chunk * 100 + 100):
        sc, width, height = _fuzz_scene(seed)
        world.set_scene(sc, width, height)
        got = world.render()
        want = oracle_for(sc, width, height, floor).render(host_threads())
        msg = diff_report(got, want, width)
        assert not msg, f"seed {seed} ({sc.spheres.shape[0]} spheres, cam {sc.cam_pos}, " \
                        f"{width}x{height}): {msg}"


@pytest.mark.parametrize("rays", [4, 3])
def test_random_scenes_match_oracle_wide_tiles(world, floor, rays):
    """The 4K headline's tile shapes on random scenes: R = 4 (32x8 tiles, the kernel the
    adaptive order picks for large frames) and R = 3 (24x8) forced on 150 scenes each (the
    default table gives these small frames 16x8 or 8x8 tiles), through update_image, vs the
    oracle byte for byte."""
    import sfrt
    world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
    try:
        for seed in range(1000 + 150 * rays, 1000 + 150 * rays + 150):
            sc, width, height = _fuzz_scene(seed)
            world.set_scene(sc, width, height)
            got = world.render()
            want = oracle_for(sc, width, height, floor).render(host_threads())
            msg = diff_report(got, want, width)
            assert not msg, f"R={rays} seed {seed} ({sc.spheres.shape[0]} spheres, cam {sc.cam_pos}, " \
                            f"{width}x{height}): {msg}"
    finally:
        world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, 0)


def test_random_subsets_match_oracle(world, floor):
    """UpdateImage(ystart, yadd, xstart, xadd) pixel subsets of random scenes (SphereWorld.cpp:94,97),
    on a poisoned canvas: the same bytes as the oracle's, and no other byte touched."""
    rng = np.random.default_rng(77)
    for seed in range(60):
        sc, width, height = _fuzz_scene(400 + seed)
        yadd, xadd = int(rng.integers(1, 9)), int(rng.integers(1, 5))
        ystart, xstart = int(rng.integers(0, yadd + 2)), int(rng.integers(0, xadd + 2))
        world.set_scene(sc, width, height)
        got = np.full(width * height * 4, 0xA5, dtype=np.uint8)
        world.update_image(got, ystart, yadd, xstart, xadd)
        want = np.full(width * height * 4, 0xA5, dtype=np.uint8)
        oracle_for(sc, width, height, floor).update_image(want, ystart, yadd, xstart, xadd)
        msg = diff_report(got, want, width)
        assert not msg, f"seed {seed} subset ({ystart},{yadd},{xstart},{xadd}): {msg}"


def test_adaptive_tile_order_same_bytes(world, floor):
    """SFRT_OPT_TILE_ORDER (render_band dispatches tiles longest-first by the march steps of
    two frames back): every frame of a sequence on a poisoned device buffer equals the
    row-major frame and the oracle -- static pose (exact order from frame 2 on), a pose
    changing every frame, scene size switches (16x8 <-> 8x8 tiles), bands and resolutions
    changing mid-sequence (stale orders must be dropped), two streams alternating."""
    import sfrt
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    seq = []
    for k in range(5):
        seq.append((scenes.lcg64(), (0.0, 0.0), 640, 360, 0, 360))
    for k in range(5):
        seq.append((scenes.lcg64(), (0.3 * k, -0.1 * k), 640, 360, 0, 360))
    for k in range(4):
        seq.append((scenes.default10(), (0.2 * k, 0.1), 640, 360, 0, 360))
    seq += [(scenes.lcg64(), (1.1, -0.2), 640, 360, 40, 200), (scenes.lcg64(), (1.1, -0.2), 640, 360, 40, 200),
            (scenes.lcg64(), (1.1, -0.2), 333, 211, 0, 211), (scenes.lcg64(), (1.1, -0.2), 640, 360, 40, 200),
            (scenes.lcg64(), (1.1, -0.2), 640, 360, 40, 200), (scenes.lcg64(), (1.1, -0.2), 640, 360, 0, 360)]
    ref = {}
    try:
        for k, (sc, pose, width, height, r0, rows) in enumerate(seq):
            scene = sc.posed(*pose)
            key = (sc.name, pose, width, height)
            if key not in ref:
                world.set_scene(scene, width, height)
                ref[key] = oracle_for(scene, width, height, floor).render(host_threads())
            world.set_scene(scene, width, height)
            stream = (s1 if k % 2 == 0 else s2)
            buf = poisoned((height, width * 4))
            torch.cuda.synchronize()
            world.set_option(sfrt.SFRT_OPT_TILE_ORDER, 1)
            world.render_band(buf[r0].data_ptr(), width * 4, r0, rows, stream.cuda_stream)
            world.check(stream.cuda_stream)
            torch.cuda.synchronize()
            got = buf.cpu().numpy().ravel()
            want = np.full(width * height * 4, 0xA5, dtype=np.uint8)
            want[r0 * width * 4:(r0 + rows) * width * 4] = ref[key][r0 * width * 4:(r0 + rows) * width * 4]
            assert diff_report(got, want, width) == "", (k, sc.name, pose, width, height, r0, rows)
    finally:
        world.set_option(sfrt.SFRT_OPT_TILE_ORDER, 1)


def test_adaptive_tile_order_4k_frames(world, floor):
    """Twelve back-to-back 4K frames on one stream without host syncs in between (the
    bench's pattern: the order sort overlaps the next frame), poses cycling through three
    values: each frame equals the same pose's row-major frame."""
    import sfrt
    import torch
    width, height = 3840, 2160
    poses = [(0.0, 0.0), (1.1, -0.2), (2.5, 0.3)]
    stream = torch.cuda.Stream()
    rowmajor = {}
    frames = []
    with torch.cuda.stream(stream):  # buffers filled on the render stream
        world.set_option(sfrt.SFRT_OPT_TILE_ORDER, 0)
        for p in poses:
            world.set_scene(scenes.lcg64().posed(*p), width, height)
            b = torch.empty(height, width * 4, dtype=torch.uint8, device="cuda:0")
            world.render_band(b.data_ptr(), width * 4, 0, height, stream.cuda_stream)
            rowmajor[p] = b
        world.set_option(sfrt.SFRT_OPT_TILE_ORDER, 1)
        for k in range(12):
            p = poses[(k // 2) % 3]
            world.set_scene(scenes.lcg64().posed(*p), width, height)
            b = poisoned((height, width * 4), 0x5A)
            world.render_band(b.data_ptr(), width * 4, 0, height, stream.cuda_stream)
            frames.append((p, b))
    world.check(stream.cuda_stream)
    torch.cuda.synchronize()
    for k, (p, b) in enumerate(frames):
        assert torch.equal(b, rowmajor[p]), (k, p)


@pytest.mark.parametrize("width,height", [(3333, 2111), (3900, 2170)])
def test_adaptive_order_ragged_wide_tiles(world, floor, width, height):
    """Large ragged frames through the ordered render_band path: 3333 x 2111 picks 24x8 tiles
    (27,720 tiles of 32x8 < 30,000 <= 36,696 of 24x8), 3900 x 2170 picks 32x8 tiles (33,184;
    3900 % 32 = 28 and 2170 % 8 = 2, so edge lanes in both directions).  Four frames back to
    back with two poses: every frame equals update_image's (the row-major 16x8 kernel) bytes,
    and one of them the oracle's."""
    import torch
    poses = [(0.4, 0.1), (2.0, -0.3)]
    want = {}
    for p in poses:
        world.set_scene(scenes.lcg64().posed(*p), width, height)
        want[p] = world.render()
    stream = torch.cuda.Stream()
    frames = []
    with torch.cuda.stream(stream):
        for k in range(4):
            p = poses[k // 2]
            world.set_scene(scenes.lcg64().posed(*p), width, height)
            b = poisoned((height, width * 4))
            world.render_band(b.data_ptr(), width * 4, 0, height, stream.cuda_stream)
            frames.append((p, b))
    world.check(stream.cuda_stream)
    torch.cuda.synchronize()
    for k, (p, b) in enumerate(frames):
        assert diff_report(b.cpu().numpy().ravel(), want[p], width) == "", (k, p)
    sc = scenes.lcg64().posed(*poses[1])
    assert diff_report(want[poses[1]], oracle_for(sc, width, height, floor).render(host_threads()),
                       width) == ""


def _division_guard_scenes():
    """Scenes whose pixels leave div_inrange's operand range ("Divisions without
    range scaling"), so that their waves take the compiler's full division: 256 x 256 frames
    with a power-of-two field of view (h_inc = v_inc = 2^-8) and the camera on the z axis:
    column 128's primary rays have x == +0 (primary_dir's guard), their hit points px == 0
    (atan2f_wave's general path), and row 128's hit points ey == 0 (the asinf argument's
    division).  (Scenes scaled far enough for |p - cam| >= 2^40 do not converge: the
    reference's march never ends once a step is below half an ulp of the position.)"""
    one = scenes.Scene("origin", np.array([[0, 0, 0, 4]], np.float32), cam_pos=(0.0, 0.0, 0.0),
                       fov_h=0.5, fov_v=0.5)
    two = scenes.Scene("axis2", np.array([[0, 0, 0, 4], [0, 0, 3, 2.5], [0, 0, -3, 1.5]],
                                         np.float32), cam_pos=(0.0, 0.0, 0.5), fov_h=1.0, fov_v=0.5)
    return [(one, 256, 256), (two, 256, 256), (two, 512, 256), (one.posed(0.3, 0.0), 256, 256)]


@pytest.mark.parametrize("case", range(4))
def test_division_guard_paths_match_oracle(world, floor, case):
    """Frames whose waves take the general division / atan2 paths equal the oracle's, through
    update_image (row-major, 8x8 / 16x8 tiles) and ordered render_band frames (the kernel
    table's choice, four back to back)."""
    import sfrt
    import torch
    sc, width, height = _division_guard_scenes()[case]
    world.set_scene(sc, width, height)
    want = oracle_for(sc, width, height, floor).render(host_threads())
    assert diff_report(world.render(), want, width) == ""
    for rays in (0, 4):  # 0: the kernel table's pick; 4: 32x8 tiles
        world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, rays)
        b = poisoned((height, width * 4))
        for _ in range(4):
            world.render_band(b.data_ptr(), width * 4, 0, height)
        world.check()
        assert diff_report(b.cpu().numpy().ravel(), want, width) == "", rays
    world.set_option(sfrt.SFRT_OPT_RAYS_PER_LANE, 0)
