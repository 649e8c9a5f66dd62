"""The oracle and the numpy restatements against the reference's own compiled code.

oracle/_ref/sphere_ref and oracle/_ref/voxel_ref (`make -C oracle ref`, run by build() where the
reference's sources exist) are the reference's unmodified SphereWorld.cpp and World.cpp, compiled
with gcc against the hand-written stand-in oracle/ref/SFML/Graphics.hpp and driven by
oracle/ref/*_ref_main.cpp.  Three kinds of test:

  live      (CPU) oracle.Oracle, oracle.VoxelOracle, tests/raycast_ref.py, tests/voxel_ref.py,
            tests/voxel_rays_ref.py and glsl_scenes.ShaderWorld against what the drivers compute
            now.  Where the reference's sources exist and the drivers do not, these FAIL; they skip
            only where neither exists.
  recorded  (CPU, everywhere) the same comparisons against tests/golden/reference/, which
            tests/golden/make_reference_golden.py wrote from the drivers; and, live, that those
            files are what the drivers produce now.
  gpu       the kernels against the recorded files (they never read the reference tree).

Every comparison is on bytes and bit patterns: the tolerance is zero.  The shared exclusion rule:
a pixel or ray for which the reference read outside a texture (the stand-in flags the read and
returns magenta instead of indexing memory) is left out of the byte comparison, and the number of
such pixels or rays must equal the restatement's count of reads outside a texture.  Every
left-out count is printed (run with -s).

What this holds: the reference's own arithmetic, as gcc compiles it for x86-64 with
-ffp-contract=off against a stand-in for SFML's containers.  What it does not hold: MSVC's code
generation, real SFML and stb, the GL output of rayShader.frag, and intermediates the reference
does not expose.  Where a float outside int range is converted (far_camera, camera_at_int_limit,
camera_at_int_limit_back, negative_coordinates' texel coordinates, the 1.5e9 and int-limit origins
of the own-origin ray sets) the reference's result is x86's cvttss2si: recorded behaviour of this
build, not of the language.
"""
import functools
import os
import zlib

import numpy as np
import pytest

import reference
import reference_cases as rc
import scenes
import voxel_aux_cases as vc
import voxel_scenes as vs
from conftest import ROOT, poisoned
from reference_cases import F, H, N, W, bits

POISON = 0xA5
PAD = 64  # canary bytes past every device output


def need_drivers():
    if reference.drivers_present():
        return
    if reference.sources_present():
        pytest.fail(f"the reference's sources are at {reference.REF_DIR} but oracle/_ref/ holds no "
                    "drivers: `make -C oracle ref` (build() runs it) failed or was not run")
    pytest.skip("neither the reference's sources nor oracle/_ref/ drivers here")


def same_outside(got, got_outside, want, want_bad, what, elem):
    """The exclusion rule: flagged rows are left out and their count is the restatement's."""
    flagged = np.asarray(got_outside).astype(bool)
    print(f"{what}: {int(flagged.sum())} of {flagged.size} left out (read outside a texture)")
    assert int(flagged.sum()) == int(want_bad), (what, int(flagged.sum()), int(want_bad))
    g = bits(got).reshape(flagged.size, -1)
    w = bits(want).reshape(flagged.size, -1)
    assert g.shape == w.shape and g.shape[1] * g.itemsize == elem, (what, g.shape, w.shape)
    bad = np.flatnonzero((g != w).any(axis=1) & ~flagged)
    assert bad.size == 0, f"{what}: {bad.size} differ, first {bad[0]}: reference {g[bad[0]]} restated {w[bad[0]]}"


oracle_sphere_frame = functools.lru_cache(maxsize=None)(rc.oracle_sphere_frame)
oracle_voxel_frame = functools.lru_cache(maxsize=None)(rc.oracle_voxel_frame)
restated_voxel_frame = functools.lru_cache(maxsize=None)(rc.restated_voxel_frame)
restated_uniforms = functools.lru_cache(maxsize=None)(rc.restated_uniforms)
SPHERE_CASES = list(rc.sphere_frame_cases())
VOXEL_CASES = rc.voxel_frame_cases()
RAY_MODES = [(n, own) for n in rc.SPHERE_RAY_SCENES for own in (False, True)]
ray_id = lambda p: f"{p[0]}-{'own' if p[1] else 'cam'}"


# ================================================================== live: restatement against reference

@pytest.mark.parametrize("case", SPHERE_CASES)
def test_live_sphere_frame(built, case):
    """oracle.Oracle against SphereWorld::UpdateImage(&img, 0, 1, 0, 1) on a snapshot world: c1 (also
    against the frame under tests/golden/), default10 in three poses, lcg64, 24 of the suite's
    random scenes and 12 of the parity sweep's adversarial ones (tangent spheres, the camera on a
    surface, radii at the 0.01 threshold, zero radii, duplicates) at 96 x 64."""
    need_drivers()
    frame, outside = rc.live_sphere_frame(case)
    _, w, h = rc.sphere_frame_cases()[case]
    same_outside(frame, outside, oracle_sphere_frame(case), 0, case, 4)
    if case == "c1_one_sphere":
        with open(os.path.join(ROOT, "tests", "golden", "frame_c1_320x240_one_sphere.rgba.zlib"), "rb") as f:
            assert frame.tobytes() == zlib.decompress(f.read())


def test_live_constructor_seed_0_is_default10(built):
    """srand(0) and the constructor's AddSphere sequence leave scenes.default10()'s walls, in
    UpdateSpheres order, and the constructor's fields of view."""
    need_drivers()
    r = reference.sphere(seed=0)
    assert np.array_equal(bits(r["spheres"]), bits(scenes.default10().spheres))
    assert np.array_equal(bits(r["cam"][5:]), bits(F([scenes.FOV_H, scenes.FOV_V])))


@pytest.mark.parametrize("mode", RAY_MODES, ids=ray_id)
def test_live_sphere_rays(built, mode):
    """tests/raycast_ref.py against SphereWorld::Raycast on tests/test_cast_rays.py's ray sets:
    the end position r->pos and the colour r->c, from the shared origin and from own origins.

    An own-origin ray is served by assigning cam.pos before the call, and raycast_ref measures its
    brightness from the ray's origin (depth = VLength(pos - o)), which is what SphereWorld.cpp:375
    then computes: so the colour is pinned in own-origin mode too.  Hit distance, drawSphere and
    the trip count cannot be observed without editing the reference: r->pos and r->c pin them only
    indirectly (a wrong sphere or trip count moves the end point or the texel).  Rays the ABI
    answers with sphere = -1 (zero, non-finite, underflowing or overflowing directions) are left
    out and counted: the reference divides by zero on them and its march does not end."""
    need_drivers()
    name, own = mode
    want = rc.restated_sphere_rays(name, own)
    got = rc.live_sphere_rays(name, own)
    v = want["valid"]
    print(f"{ray_id(mode)}: {int((~v).sum())} of {N} left out (invalid for the ABI)")
    assert 0 < int((~v).sum()) <= rc.LEFT_OUT_CAP * N
    assert (want["sphere"][~v] == -1).all() and want["inside"].all()
    same_outside(got["pos"][v], got["outside"][v], want["pos"][v], 0, ray_id(mode) + " pos", 12)
    same_outside(got["rgba"][v], got["outside"][v], want["rgba"][v], 0, ray_id(mode) + " rgba", 4)


@pytest.mark.parametrize("steps", rc.UNIFORM_STEPS)
def test_live_uniforms(built, steps):
    """glsl_scenes.ShaderWorld(0) against the uniforms SphereWorld uploads: srand(0), the
    constructor, `steps` UpdateWorld calls; every spheres[k], lights[k], uvs[k] ever set and the
    three counts, the last value of each.

    The driver stops the camera physics first (cam.airtime = 0, so UpdateWorld never calls Move):
    ShaderWorld does not replay Move, and with it the reference's camera falls to y = -3.58 within
    50 steps and UpdateSpheres sorts the walls differently.  The order in which gcc evaluates the
    rand() arguments of sf::Vector3f(rand()..., rand()..., rand()...) is the compiler's choice:
    this pins the replay (right to left) to this build's order.  The shader itself cannot run
    here: its GL output stays unpinned."""
    need_drivers()
    got, want = rc.live_uniforms(steps), restated_uniforms(steps)
    assert got.pop("ground") is None
    assert {"lightCount", "sphereCount", "allSpheresCount"} <= set(got) and len(got) > 60
    for name, value in got.items():
        assert want[name] == value, (steps, name, value, want[name])
    for name in set(want) - set(got):   # never uploaded: ShaderWorld must not have touched it
        assert not any(want[name]), (steps, name)


def _field_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for k in want.dtype.names:
        assert np.array_equal(bits(got[k]), bits(np.ascontiguousarray(want[k]))), (what, k)


@pytest.mark.parametrize("case", VOXEL_CASES)
def test_live_voxel_frame(built, case):
    """oracle.VoxelOracle and voxel_ref.render against World::UpdateImage(&img, 0, 1, 0, 1) at
    101 x 37.  The ctor_* cases run the reference's constructor, zero the sprites' directions, set
    the camera and run UpdateDyn twice -- what voxel_scenes.default_world replays -- and compare
    the resulting `dyn` (order, distToCamera, r, g, b and the rest), `alights` and block map with
    its arrays field by field; the other cases hand the driver a snapshot."""
    need_drivers()
    r = rc.live_voxel_frame(case)
    scene = rc.voxel_scene(case)
    if case in rc.CTOR_POSES:
        _field_equal(r["dyn"], scene.dyn.astype(reference.DYN_DTYPE), case + " dyn")
        _field_equal(r["lights"][r["alights"]], scene.lights.astype(reference.LIGHT_DTYPE), case + " alights")
        _field_equal(r["blocks"], np.sort(reference.block_records(scene.blocks), order="key"), case + " blocks")
        assert np.array_equal(bits(r["cam"][5:]), bits(F([scene.fov_h, scene.fov_v, 24.0, 16.0])))
    frame, bad = oracle_voxel_frame(case)
    same_outside(r["frame"], r["frame_outside"], frame, bad, case + " oracle", 4)
    frame, bad = restated_voxel_frame(case)
    same_outside(r["frame"], r["frame_outside"], frame, bad, case + " voxel_ref", 4)


@pytest.mark.parametrize("ray_set", rc.VOXEL_RAY_SETS, ids=ray_id)
def test_live_voxel_rays(built, ray_set):
    """tests/voxel_rays_ref.py's colour against World::Raycast's r->c for arbitrary_set: from the
    camera with the billboards, and from own origins (cam.pos assigned per ray) with `dyn` emptied."""
    need_drivers()
    name, own = ray_set
    want = rc.restated_voxel_rays(name, own)
    got = rc.live_voxel_rays(name, own)
    left = ~want["valid"]
    print(f"{ray_id(ray_set)}: {int(left.sum())} of {N} left out (invalid for the ABI)")
    assert left.sum() + got["outside"].astype(bool).sum() < rc.LEFT_OUT_CAP * N
    v = want["valid"]
    same_outside(got["rgba"][v], got["outside"][v], want["rgba"][v], want["bad_texels"], ray_id(ray_set), 4)


def test_live_shadow_rays(built):
    """tests/voxel_rays_ref.py's `free` against World::LRaycast's bool for shadow_set().  Until now
    nothing stood behind these answers but the restatement itself."""
    need_drivers()
    left = rc.shadow_left_out()
    print(f"shadow: {int(left.sum())} of {N} left out (the ABI's own definition)")
    assert left.sum() < rc.LEFT_OUT_CAP * N
    free, outside = rc.live_shadow()
    want = rc.restated_shadow()["free"]
    assert not outside.any()
    bad = np.flatnonzero((free != want) & ~left)
    assert bad.size == 0, (bad.size, bad[:5], free[bad[:5]], want[bad[:5]])
    assert (free[~left] == 1).any() and (free[~left] == 0).any()


# ================================================================== recorded: the pin without the drivers

def test_recorded_files_are_what_the_drivers_produce_now(built):
    need_drivers()
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "make_reference_golden", os.path.join(ROOT, "tests", "golden", "make_reference_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    now = mod.record()
    assert sorted(now) == sorted(os.listdir(rc.GOLDEN))
    for name, content in now.items():
        if name == "hashes.json":
            assert content == rc.load_hashes()
        elif name == "uniforms.json":
            assert content == rc.load_uniforms()
        elif name.endswith(".npz"):
            rec = rc.load_npz(name[:-4])
            assert sorted(rec.files) == sorted(content), name
            for k, a in content.items():
                assert np.array_equal(rec[k], a), (name, k)
        else:
            assert rc.load_frame(name[len("frame_"):-len(".rgba.zlib")]).tobytes() == content, name
        assert os.path.getsize(os.path.join(rc.GOLDEN, name)) <= \
            os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden.json")), name


@pytest.mark.parametrize("case", SPHERE_CASES)
def test_recorded_sphere_frame(built, case):
    """oracle.Oracle against the recorded hash of the reference's frame (the whole frame for c1
    and default10 at (0.7, 0.3)).  No sphere case reads outside the texture, so nothing is left out."""
    rec = rc.load_hashes()["sphere_frames"][case]
    frame = oracle_sphere_frame(case)
    assert rec["outside"] == 0
    assert rc.fnv1a64(frame) == rec["fnv1a64"], case
    if case in rc.RECORDED_FRAMES:
        assert np.array_equal(frame, rc.load_frame(case)), case


@pytest.mark.parametrize("case", VOXEL_CASES)
def test_recorded_voxel_frame(built, case):
    """oracle.VoxelOracle and voxel_ref.render against the recorded hash of the reference's frame;
    the constructor cases also voxel_scenes.default_world's dyn and active lights against the
    recorded hashes of the reference's.  A recorded frame holds magenta where the reference read
    outside a texture -- the colour the oracle and voxel_ref substitute as well -- so the hash
    covers those pixels too, and their count must be the restatements' count."""
    rec = rc.load_hashes()["voxel_frames"][case]
    for what, (frame, bad) in (("oracle", oracle_voxel_frame(case)), ("voxel_ref", restated_voxel_frame(case))):
        print(f"{case} {what}: {bad} pixels read outside a texture")
        assert bad == rec["outside"], (case, what, bad, rec["outside"])
        assert rc.fnv1a64(frame) == rec["fnv1a64"], (case, what)
        if case in rc.RECORDED_FRAMES:
            assert np.array_equal(np.asarray(frame).reshape(-1), rc.load_frame(case)), (case, what)
    if case in rc.CTOR_POSES:
        scene = rc.voxel_scene(case)
        assert rc.fnv1a64(np.frombuffer(scene.dyn.astype(reference.DYN_DTYPE).tobytes(), np.uint8)) == rec["dyn_fnv1a64"]
        assert rc.fnv1a64(np.frombuffer(scene.lights.astype(reference.LIGHT_DTYPE).tobytes(), np.uint8)) == rec["alights_fnv1a64"]


@pytest.mark.parametrize("mode", RAY_MODES, ids=ray_id)
def test_recorded_sphere_rays(built, mode):
    name, own = mode
    rec = rc.load_npz(f"sphere_rays_{name}")
    assert str(rec["input_fnv1a64"]) == rc.input_hash(*rc.sphere_ray_set(name)), "the ray set changed: record again"
    tag = "own" if own else "cam"
    want = rc.restated_sphere_rays(name, own)
    v = want["valid"]
    assert np.array_equal(rec[f"valid_{tag}"], v)
    print(f"{ray_id(mode)}: {int((~v).sum())} of {N} left out (invalid for the ABI)")
    assert 0 < int((~v).sum()) <= rc.LEFT_OUT_CAP * N
    same_outside(rec[f"pos_{tag}"][v], rec[f"outside_{tag}"][v], want["pos"][v], 0, ray_id(mode) + " pos", 12)
    same_outside(rec[f"rgba_{tag}"][v], rec[f"outside_{tag}"][v], want["rgba"][v], 0, ray_id(mode) + " rgba", 4)


@pytest.mark.parametrize("steps", rc.UNIFORM_STEPS)
def test_recorded_uniforms(steps):
    got, want = dict(rc.load_uniforms()[str(steps)]), restated_uniforms(steps)
    assert got.pop("ground") is None and len(got) > 60
    for name, value in got.items():
        assert want[name] == value, (steps, name, value, want[name])
    for name in set(want) - set(got):
        assert not any(want[name]), (steps, name)


@pytest.mark.parametrize("ray_set", rc.VOXEL_RAY_SETS, ids=ray_id)
def test_recorded_voxel_rays(ray_set):
    name, own = ray_set
    rec = rc.load_npz("voxel_rays")
    tag = f"{name}_{'own' if own else 'cam'}"
    assert str(rec[f"input_fnv1a64_{tag}"]) == rc.input_hash(*rc.voxel_ray_inputs(name, own)), \
        "the ray set changed: record again"
    want = rc.restated_voxel_rays(name, own)
    v = want["valid"]
    assert (~v).sum() + rec[f"outside_{tag}"].astype(bool).sum() < rc.LEFT_OUT_CAP * N
    same_outside(rec[f"rgba_{tag}"][v], rec[f"outside_{tag}"][v], want["rgba"][v], want["bad_texels"], tag, 4)


def test_recorded_shadow_rays():
    rec = rc.load_npz("voxel_rays")
    assert str(rec["input_fnv1a64_shadow"]) == rc.input_hash(*rc.shadow_inputs()), "the ray set changed: record again"
    left = rc.shadow_left_out()
    print(f"shadow: {int(left.sum())} of {N} left out (the ABI's own definition)")
    assert left.sum() < rc.LEFT_OUT_CAP * N
    free, want = rec["shadow_free"], rc.restated_shadow()["free"]
    assert np.array_equal(free[~left], want[~left])
    assert (free[~left] == 1).any() and (free[~left] == 0).any()


# ================================================================== gpu: kernels against the recorded files

def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a, dtype=F).ravel()).to("cuda:0")
    torch.cuda.current_stream().synchronize()
    return t


def _read(buf, nbytes, what):
    raw = buf.cpu().numpy()
    assert raw.size == nbytes + PAD and (raw[nbytes:] == POISON).all(), f"{what}: bytes past the output were written"
    return np.ascontiguousarray(raw[:nbytes])


def _band_frames(world, w, h, times=3):
    """`times` whole-frame render_band calls with the adaptive tile order on, back to back on one
    stream (the order of a frame comes from two frames back), each into a poisoned, canaried buffer."""
    import sfrt
    import torch
    stream = torch.cuda.Stream()
    before = world.get_option(sfrt.SFRT_OPT_TILE_ORDER)
    world.set_option(sfrt.SFRT_OPT_TILE_ORDER, 1)
    try:
        bufs = [poisoned((w * h * 4 + PAD,), POISON) for _ in range(times)]
        for b in bufs:
            world.render_band(b.data_ptr(), w * 4, 0, h, stream.cuda_stream)
        world.check(stream.cuda_stream)
    finally:
        world.set_option(sfrt.SFRT_OPT_TILE_ORDER, before)
    return [_read(b, w * h * 4, "render_band") for b in bufs]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["c1_one_sphere", "default10_0.7_0.3"])
def test_gpu_sphere_frame_equals_the_recorded_reference(built, case):
    import sfrt
    want = rc.load_frame(case)
    sc, w, h = rc.sphere_frame_cases()[case]
    with sfrt.World(0) as world:
        world.load_texture(*scenes.load_floor())
        world.set_scene(sc, w, h)
        assert np.array_equal(world.update_image(np.full(w * h * 4, POISON, np.uint8)), want), case
        for k, got in enumerate(_band_frames(world, w, h)):
            assert np.array_equal(got, want), (case, "render_band", k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["voxel_default", "voxel_random_3"])
def test_gpu_voxel_frame_equals_the_recorded_reference(built, case):
    import sfrt
    want = rc.load_frame(case)
    assert rc.load_hashes()["voxel_frames"][case]["outside"] == 0  # so check() stays clean
    tex, dyn = vc.assets()
    with sfrt.VoxelWorld(0) as world:
        world.load_assets(tex, dyn, vs.COLORS)
        world.set_scene(rc.voxel_scene(case), W, H)
        assert np.array_equal(world.update_image(np.full(N * 4, POISON, np.uint8)), want), case
        for k, got in enumerate(_band_frames(world, W, H)):
            assert np.array_equal(got, want), (case, "render_band", k)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", RAY_MODES, ids=ray_id)
def test_gpu_sphere_rays_equal_the_recorded_reference(built, mode):
    """sfrt_world_cast_rays_device on the recorded batch of 101 x 37 rays (58 full waves and a
    25-lane tail): end position and colour; the rays the ABI calls invalid are left out, counted,
    and must carry sphere = -1."""
    import sfrt
    import torch
    name, own = mode
    rec = rc.load_npz(f"sphere_rays_{name}")
    d, o = rc.sphere_ray_set(name)
    assert str(rec["input_fnv1a64"]) == rc.input_hash(d, o), "the ray set changed: record again"
    tag = "own" if own else "cam"
    v = rec[f"valid_{tag}"]
    stream = torch.cuda.Stream()
    with sfrt.World(0) as world:
        world.load_texture(*scenes.load_floor())
        world.set_scene(rc.sphere_ray_scene(name), W, H)
        ins = (_dev(d), _dev(o) if own else None)
        bufs = {k: poisoned((N * n + PAD,), POISON) for k, n in (("pos", 12), ("sphere", 4), ("rgba", 4))}
        world.cast_rays_device(ins[0].data_ptr(), ins[1].data_ptr() if own else None, N, stream.cuda_stream,
                               **{k: b.data_ptr() for k, b in bufs.items()})
        world.check(stream.cuda_stream)
        pos = _read(bufs["pos"], N * 12, "pos").view(F).reshape(N, 3)
        sphere = _read(bufs["sphere"], N * 4, "sphere").view(np.int32)
        rgba = _read(bufs["rgba"], N * 4, "rgba").reshape(N, 4)
    print(f"{ray_id(mode)}: {int((~v).sum())} of {N} left out (invalid for the ABI)")
    assert np.array_equal(sphere == -1, ~v)
    assert not rec[f"outside_{tag}"].any()
    assert np.array_equal(bits(pos[v]), bits(rec[f"pos_{tag}"][v]))
    assert np.array_equal(rgba[v], rec[f"rgba_{tag}"][v])


@pytest.mark.gpu
@pytest.mark.parametrize("ray_set", rc.VOXEL_RAY_SETS, ids=ray_id)
def test_gpu_voxel_rays_equal_the_recorded_reference(built, ray_set):
    """sfrt_voxel_cast_rays_device's colour on the recorded batches; rays for which the reference
    read outside a texture are left out, and the status word says SFRT_E_TEXEL exactly then."""
    import sfrt
    import torch
    name, own = ray_set
    rec = rc.load_npz("voxel_rays")
    tag = f"{name}_{'own' if own else 'cam'}"
    d, ys, o = rc.voxel_ray_inputs(name, own)
    assert str(rec[f"input_fnv1a64_{tag}"]) == rc.input_hash(d, ys, o), "the ray set changed: record again"
    outside = rec[f"outside_{tag}"].astype(bool)
    tex, dyn = vc.assets()
    stream = torch.cuda.Stream()
    with sfrt.VoxelWorld(0) as world:
        world.load_assets(tex, dyn, vs.COLORS)
        world.set_scene(vc.scene(name), W, H)
        ins = (_dev(d), _dev(ys), _dev(o) if own else None)
        buf = poisoned((N * 4 + PAD,), POISON)
        world.cast_rays_device(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr() if own else None, N,
                               stream.cuda_stream, rgba=buf.data_ptr())
        try:
            world.check(stream.cuda_stream)
            status = 0
        except sfrt.SfrtError as e:
            status = e.code
        rgba = _read(buf, N * 4, "rgba").reshape(N, 4)
    print(f"{tag}: {int(outside.sum())} of {N} left out (read outside a texture)")
    assert status == (-7 if outside.any() else 0), (tag, status)   # SFRT_E_TEXEL
    assert outside.sum() < rc.LEFT_OUT_CAP * N
    assert np.array_equal(rgba[~outside], rec[f"rgba_{tag}"][~outside]), tag


@pytest.mark.gpu
def test_gpu_shadow_rays_equal_the_recorded_reference(built):
    import sfrt
    import torch
    rec = rc.load_npz("voxel_rays")
    o, d, md = rc.shadow_inputs()
    assert str(rec["input_fnv1a64_shadow"]) == rc.input_hash(o, d, md), "the ray set changed: record again"
    left = rc.shadow_left_out()
    tex, dyn = vc.assets()
    stream = torch.cuda.Stream()
    with sfrt.VoxelWorld(0) as world:
        world.load_assets(tex, dyn, vs.COLORS)
        world.set_scene(vc.scene("default"), W, H)
        ins = (_dev(o), _dev(d), _dev(md))
        buf = poisoned((N * 4 + PAD,), POISON)
        world.cast_shadow_rays_device(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), N,
                                      stream.cuda_stream, free=buf.data_ptr())
        world.check(stream.cuda_stream)
        free = _read(buf, N * 4, "free").view(np.int32)
    print(f"shadow: {int(left.sum())} of {N} left out (the ABI's own definition)")
    assert np.array_equal(free[~left], rec["shadow_free"][~left])
