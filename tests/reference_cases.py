"""The cases of tests/test_reference_pin.py and tests/golden/make_reference_golden.py: what is
asked of the reference drivers (oracle/reference.py), and what the oracle and the numpy
restatements answer for the same input.  One place, so the live tests, the recorded fixtures and
the GPU tests speak about the same scenes and rays.

Helper module, not a test.  Nothing here reads the reference's sources; `live_*` functions run the
compiled drivers and are called only where they exist.
"""
import functools
import json
import os
import tempfile
import zlib

import numpy as np

import glsl_scenes as gs
import raycast_ref
import reference
import scenes
import voxel_aux_cases as vc
import voxel_rays_ref as vrr
import voxel_ref
import voxel_scenes as vs

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference")
W, H = vc.W, vc.H                # 101 x 37: 58 full waves and a 25-lane tail
N = W * H
SMALL = (96, 64)
DEFAULT10_POSES = [(0.0, 0.0), (0.7, 0.3), (-2.4, -0.9)]
FUZZ_SEEDS = list(range(24))                      # tests/test_gpu_parity.py _fuzz_scene
ADVERSARIAL_SEEDS = list(range(50000, 50012))     # tests/test_parity_sweep.py _sphere_adversarial
UNIFORM_STEPS = [0, 50, 300]
CTOR_POSES = {  # the constructor world's poses: vc.DEFAULT_POSES and one inside a room looking up
    "ctor_default": ((15.5, 1.9, 15.5), 0.0, 0.0),
    "ctor_default_turned": ((30.25, 2.6, 12.75), 2.2, 0.25),
    "ctor_room_looking_up": ((20.5, 2.2, 40.5), 1.0, 0.6),
}
RECORDED_FRAMES = ["c1_one_sphere", "default10_0.7_0.3", "voxel_default", "voxel_random_3"]
SPHERE_RAY_SCENES = ["default10", "lcg64", "lcg256"]
VOXEL_RAY_SETS = [("random_3", False), ("negative_coordinates", False), ("default", True),
                  ("random_3", True)]   # test_voxel_cast_rays.py ARB_CAMERA and ARB_OWN
LEFT_OUT_CAP = 0.05


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.itemsize == 1 else a.view(np.uint32)


def fnv1a64(buf) -> str:
    import oracle
    return oracle.fnv1a64(np.ascontiguousarray(buf).view(np.uint8))


# ------------------------------------------------------------------ sphere frames

@functools.lru_cache(maxsize=None)
def sphere_frame_cases():
    """{id: (scene, width, height)}."""
    from test_gpu_parity import _fuzz_scene
    from test_parity_sweep import _sphere_adversarial
    out = {"c1_one_sphere": (scenes.one_sphere(), 320, 240)}
    for rot, hrot in DEFAULT10_POSES:
        out[f"default10_{rot:g}_{hrot:g}"] = (scenes.default10().posed(rot, hrot), 320, 180)
    out["lcg64"] = (scenes.lcg64(), 160, 90)
    for s in FUZZ_SEEDS:
        out[f"fuzz_{s}"] = (_fuzz_scene(s)[0], *SMALL)
    for s in ADVERSARIAL_SEEDS:
        out[f"adversarial_{s}"] = (_sphere_adversarial(s)[0], *SMALL)
    return out


def oracle_sphere_frame(case):
    import oracle
    sc, w, h = sphere_frame_cases()[case]
    return oracle.Oracle.from_scene(sc, w, h, *scenes.load_floor()).render(4)


def live_sphere_frame(case):
    sc, w, h = sphere_frame_cases()[case]
    r = reference.sphere(spheres=sc.spheres, cam_pos=sc.cam_pos, rotation=sc.rotation,
                         hrotation=sc.hrotation, fov_h=sc.fov_h, fov_v=sc.fov_v, width=w, height=h)
    return r["frame"], r["frame_outside"]


# ------------------------------------------------------------------ sphere rays

@functools.lru_cache(maxsize=None)
def sphere_ray_set(name):
    """N rays for scene `name` (unposed): tests/test_cast_rays.py's arbitrary rays (1000, six
    axis-parallel ones among them), its denormal-component rays, its invalid rays (BAD_DIRS: NaN,
    inf, zero, overflowing and underflowing lengths) and, to fill the batch, pixel directions of
    the suite's posed frame; and the own origins: its 1000, then the camera moved by up to 0.5."""
    import test_cast_rays as tcr
    dirs, origins, _, _ = tcr.arbitrary_rays(name)
    denormal = F([[1e-39, 1, 0], [0, 1e-39, -1], [1, 1, 1e-41], [-1e-19, 1e-24, 1e-19]])
    fill = tcr.frame_dirs(name)[:N - 1000 - 4 - len(tcr.BAD_DIRS)]
    d = np.concatenate([dirs, denormal, tcr.BAD_DIRS, fill]).astype(F)
    cam = np.asarray(tcr._scene(name, posed=False).cam_pos, dtype=F)
    rng = np.random.default_rng(31)
    o = np.concatenate([origins, (cam + rng.uniform(-0.5, 0.5, (N - 1000, 3))).astype(F)]).astype(F)
    assert d.shape == o.shape == (N, 3)
    d.setflags(write=False)
    o.setflags(write=False)
    return d, o


def sphere_ray_scene(name):
    import test_cast_rays as tcr
    return tcr._scene(name, posed=False)


@functools.lru_cache(maxsize=None)
def restated_sphere_rays(name, own):
    d, o = sphere_ray_set(name)
    sc = sphere_ray_scene(name)
    r = raycast_ref.raycast(sc.spheres, sc.cam_pos, d, o if own else None,
                            textures={0: scenes.load_floor()})
    for k in ("pos", "rgba", "valid", "inside", "sphere"):
        r[k].setflags(write=False)
    return r


def live_sphere_rays(name, own):
    """The driver on the valid rays of the set (an invalid direction never ends the reference's
    march: its step is NaN or zero).  Returns pos, rgba, outside for all N rays (zeros where
    invalid) and the valid mask."""
    d, o = sphere_ray_set(name)
    sc = sphere_ray_scene(name)
    valid = restated_sphere_rays(name, own)["valid"]
    v = np.flatnonzero(valid)
    r = reference.sphere(spheres=sc.spheres, cam_pos=sc.cam_pos, fov_h=sc.fov_h, fov_v=sc.fov_v,
                         dirs=d[v], origins=o[v] if own else None)
    pos, rgba, outside = np.zeros((N, 3), F), np.zeros((N, 4), np.uint8), np.zeros(N, np.uint8)
    pos[v], rgba[v], outside[v] = r["pos"], r["rgba"], r["outside"]
    return {"pos": pos, "rgba": rgba, "outside": outside, "valid": valid}


# ------------------------------------------------------------------ GLSL uniforms

def uniform_state(dump):
    """A driver's uniform dump (every setUniform call in order) -> {name: last value}, vec4 as
    four uint32 bit patterns, int as the int."""
    last = {}
    for name, kind, v, i in dump:
        last[name] = [int(x) for x in bits(v)] if kind == 0 else int(i) if kind == 1 else None
    return last


def live_uniforms(steps):
    return uniform_state(reference.sphere(seed=0, steps=steps, uniforms=True)["uniforms"])


def restated_uniforms(steps):
    """glsl_scenes.ShaderWorld(0) after `steps` update_world calls, in uniform_state's form: every
    spheres[k], lights[k], uvs[k] of the block and the three counts."""
    w = gs.ShaderWorld(0)
    for _ in range(steps):
        w.update_world()
    out = {"lightCount": int(w.u["light_count"]), "sphereCount": int(w.u["sphere_count"]),
           "allSpheresCount": int(w.u["all_spheres_count"])}
    for arr in ("spheres", "lights", "uvs"):
        for k in range(gs.MAX_SPHERES):
            out[f"{arr}[{k}]"] = [int(x) for x in bits(w.u[arr][k])]
    return out


# ------------------------------------------------------------------ voxel frames

def voxel_frame_cases():
    """ids: the constructor world's three poses, then every snapshot of voxel_aux_cases (its
    default and edge poses -- the VOXEL_EDGE_CASES of tests/test_voxel.py -- and random_0..11)."""
    return list(CTOR_POSES) + [f"voxel_{n}" for n in vc.NAMES]


@functools.lru_cache(maxsize=None)
def voxel_scene(case):
    if case in CTOR_POSES:
        return vs.default_world(*CTOR_POSES[case])
    return vc.scene(case[len("voxel_"):])


@functools.lru_cache(maxsize=None)
def _private_oracle_lib():
    """A second copy of liboracle.so loaded from a file of its own, so with a counter of texel
    reads outside a texture of its own: the suite's library counts per process, and
    tests/test_voxel.py and tests/test_supersample_renderers.py assert on that count's absolute
    value, which the cases here (negative_coordinates reads outside 185 times) must not move."""
    import oracle
    oracle.lib()
    saved = oracle._lib, oracle.LIB_PATH
    fd, path = tempfile.mkstemp(prefix="liboracle_pin_", suffix=".so")
    try:
        with os.fdopen(fd, "wb") as dst, open(oracle.LIB_PATH, "rb") as src:
            dst.write(src.read())
        oracle._lib, oracle.LIB_PATH = None, path
        return oracle.lib()
    finally:
        oracle._lib, oracle.LIB_PATH = saved
        os.unlink(path)  # the mapping outlives the name


def oracle_voxel_frame(case):
    """(frame bytes, texel reads outside a texture) of oracle/voxelworld_oracle.c."""
    import oracle
    tex, dyn = vc.assets()
    private = _private_oracle_lib()
    saved = oracle._lib
    oracle._lib = private
    try:
        before = oracle.VoxelOracle.bad_texel_reads()
        frame = oracle.VoxelOracle(voxel_scene(case), W, H, tex, dyn, vs.COLORS).render(1)
        return frame, oracle.VoxelOracle.bad_texel_reads() - before
    finally:
        oracle._lib = saved


def restated_voxel_frame(case):
    tex, dyn = vc.assets()
    r = voxel_ref.render(voxel_scene(case), W, H, tex, dyn, vs.COLORS, shade=True)
    return r["rgba"].reshape(-1), r["bad_texels"]


def live_voxel_frame(case):
    """The driver's result: the constructor request for CTOR_POSES, a snapshot request otherwise."""
    if case in CTOR_POSES:
        p, rot, hrot = CTOR_POSES[case]
        return reference.voxel(cam_pos=p, rotation=rot, hrotation=hrot, width=W, height=H,
                               dump_blocks=True)
    return reference.voxel(scene=voxel_scene(case), colors=vs.COLORS, width=W, height=H)


# ------------------------------------------------------------------ voxel rays

def voxel_ray_inputs(name, own):
    import test_voxel_cast_rays as tv
    d, ys = tv.arbitrary_set(name)
    return d, ys, (tv.origin_set(name) if own else None)


def restated_voxel_rays(name, own):
    import test_voxel_cast_rays as tv
    return tv.arbitrary_ref(name, own)


def live_voxel_rays(name, own):
    d, ys, o = voxel_ray_inputs(name, own)
    return reference.voxel(scene=vc.scene(name), colors=vs.COLORS, raycast=(d, ys), origins=o,
                           empty_dyn=own)


def shadow_inputs():
    import test_voxel_cast_rays as tv
    return tv.shadow_set()


def shadow_left_out():
    """Rays of the shadow set whose answer is the ABI's own definition, not the reference's:
    non-finite rays, segments beyond SFRT_VOXEL_MAX_SHADOW_DIST.  (max_dist <= 0: the reference's
    loop at World.cpp:475 is not entered and `dist >= maxDist` holds, the restatement's answer
    too, so those rows stay in.)"""
    o, d, md = shadow_inputs()
    return ~(np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & np.isfinite(md) &
             (md <= vrr.MAX_SHADOW_DIST))


def restated_shadow():
    import test_voxel_cast_rays as tv
    return tv.shadow_ref()


def live_shadow():
    o, d, md = shadow_inputs()
    keep = np.flatnonzero(~shadow_left_out())
    r = reference.voxel(scene=vc.scene("default"), colors=vs.COLORS,
                        lraycast=(o[keep], d[keep], md[keep]))
    free = np.full(N, -1, dtype=np.int32)
    free[keep] = r["free"]
    return free, r["outside"]


# ------------------------------------------------------------------ the recorded fixtures

def load_hashes():
    with open(os.path.join(GOLDEN, "hashes.json")) as f:
        return json.load(f)


def load_frame(case):
    with open(os.path.join(GOLDEN, f"frame_{case}.rgba.zlib"), "rb") as f:
        return np.frombuffer(zlib.decompress(f.read()), dtype=np.uint8)


def load_npz(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def load_uniforms():
    with open(os.path.join(GOLDEN, "uniforms.json")) as f:
        return json.load(f)


def input_hash(*arrays) -> str:
    """FNV-1a-64 over the ray inputs a recorded batch belongs to: a change of a generator (or of
    numpy's streams) shows as this hash, not as a misleading mismatch."""
    return fnv1a64(np.concatenate([bits(a).reshape(-1).view(np.uint8) for a in arrays if a is not None]))
