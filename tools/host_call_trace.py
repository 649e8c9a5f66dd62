"""The ordered HIP runtime calls of every host entry point, for two builds of libsfrt.so.

    SFRT_LIB=<lib> rocprofv3 --hip-trace --output-format csv -d DIR -o NAME -- \
        python tools/host_call_trace.py run LABELS.txt
    python tools/host_call_trace.py compare OLD_hip_api_trace.csv OLD_LABELS NEW_hip_api_trace.csv \
        NEW_LABELS [OUT.txt]

`run` makes each host entry point's first call and one growing call (frames 320x240 -> 640x360 for
the sphere world, 160x90 -> 320x180 for the voxel and GLSL renderers, ray batches of 64 -> 4,096
rays: each more than 1.5 times larger, past the pinned buffers' geometric capacity), then the
sphere world's render_band sequence through every state of a chain's caches (sfrt_raycache.h), and
writes the entry points' labels in call order.  Before each it calls sfrt_world_create(-1) twice -- two
hipGetDeviceCount calls in a row, which no entry point makes -- so `compare` can cut the trace
into entry points.  `compare` prints both builds' call names per entry point and exits 1 if any
entry point's list differs.
"""
import copy
import csv
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = "hipGetDeviceCount"


def run(labels_path):
    sys.path.insert(0, os.path.join(ROOT, "sfml-software-raytracer_amd"))
    import numpy as np
    import glsl_scenes as gs
    import scenes
    import sfrt
    import voxel_scenes as vs
    import torch
    labels, frames = [], []
    # (before the first marker: the band sequence's device buffers, so that no allocator call of
    # torch's falls between two entry points)
    band_w, band_h = 72, 20
    band = torch.empty((band_h, band_w * 4), dtype=torch.uint8, device="cuda")
    band_depth = torch.empty((band_h, band_w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def entry(label, fn):
        out = ctypes.c_void_p()
        for _ in range(2):
            sfrt.lib().sfrt_world_create(-1, ctypes.byref(out))
        labels.append(label)
        return fn()

    rng = np.random.default_rng(5)
    dirs = rng.standard_normal((4096, 3)).astype(np.float32)
    floor = scenes.load_floor()

    world = entry("world_create", lambda: sfrt.World(0))
    entry("world_load_texture", lambda: world.load_texture(*floor))
    sc = scenes.default10()
    org = (np.asarray(sc.cam_pos, np.float32) + rng.uniform(-0.3, 0.3, (4096, 3))).astype(np.float32)
    for tag, (w, h) in (("first", (320, 240)), ("grown", (640, 360))):
        world.set_scene(sc, w, h)
        entry(f"world_update_image {tag}", world.render)
        entry(f"world_update_image_aux {tag}", world.render_aux)
        frame = entry(f"host_alloc {tag}", lambda: sfrt.HostFrame(w * h * 4))
        frames.append(frame)
        ticket = entry(f"world_submit_frame {tag}", lambda: world.submit_frame(frame))
        entry(f"world_wait_frame {tag}", lambda: world.wait_frame(ticket))
        entry(f"world_submit_frame {tag} second slot", lambda: world.submit_frame(frame))
        entry(f"world_wait_frame {tag} second slot", lambda: world.wait_frame(ticket + 1))
    for tag, n in (("first", 64), ("grown", 4096)):
        entry(f"world_cast_rays origins {tag}", lambda: world.cast_rays(dirs[:n], org[:n]))
        entry(f"world_cast_rays camera {tag}", lambda: world.cast_rays(dirs[:n]))
    # One pose at 72x20 (a clamped last tile column and row) on the null stream: an uncached, a
    # filling and three reading launches; an aux band, which takes no part; a moved camera twice
    # (a miss, then a refill over the directions); the first pose again; each budget lowered to 0.
    world.set_scene(sc, band_w, band_h)
    pos = tuple(sc.cam_pos)

    def draw():
        world.render_band(band.data_ptr(), band_w * 4, 0, band_h)

    for k, what in enumerate(("trace", "fill", "read", "read", "read")):
        entry(f"world_render_band {k + 1} {what}", draw)
    entry("world_render_band_aux between reads", lambda: world.render_band_aux(
        band.data_ptr(), band_w * 4, 0, band_h, depth=(band_depth.data_ptr(), band_w * 4)))
    world.set_camera((pos[0] + 0.25, pos[1], pos[2]), sc.rotation, sc.hrotation)
    entry("world_render_band moved 1", draw)
    entry("world_render_band moved 2", draw)
    world.set_camera(pos, sc.rotation, sc.hrotation)
    entry("world_render_band moved back", draw)
    entry("world_set_option hit cache 0", lambda: world.set_option(sfrt.SFRT_OPT_HIT_CACHE_MB, 0))
    entry("world_render_band hit cache 0", draw)
    entry("world_set_option ray cache 0", lambda: world.set_option(sfrt.SFRT_OPT_RAY_CACHE_MB, 0))
    entry("world_render_band ray cache 0", draw)
    entry("world_check after bands", world.check)
    entry("host_free", lambda: [f.free() for f in frames])
    entry("world_destroy", world.close)

    vw = entry("voxel_create", lambda: sfrt.VoxelWorld(0))
    tex, dyn = vs.load_textures()
    entry("voxel_load_assets", lambda: vw.load_assets(tex, dyn, vs.COLORS))
    scene = vs.default_world((20.5, 2.2, 40.5), 1.0, 0.1)
    part = copy.copy(scene)
    part.blocks = scene.blocks[:scene.blocks.shape[0] // 3]  # the grid and its staging grow too
    vorg = (np.asarray((20.5, 2.2, 40.5), np.float32) + rng.uniform(-0.3, 0.3, (4096, 3))).astype(np.float32)
    dists = np.linspace(1.0, 16.0, 4096, dtype=np.float32)
    for tag, sn, (w, h), n in (("first", part, (160, 90), 64), ("grown", scene, (320, 180), 4096)):
        vw.set_scene(sn, w, h)
        entry(f"voxel_update_image {tag}", vw.render)
        vw.set_scene(sn, w, h)  # (blocks set again: the second staging pair)
        entry(f"voxel_update_image_aux {tag}", vw.render_aux)
        # (the smaller batch first: 36 then 56 bytes per ray, both grow the shared staging)
        entry(f"voxel_cast_shadow_rays {tag}", lambda: vw.cast_shadow_rays(vorg[:n], dirs[:n], dists[:n]))
        entry(f"voxel_cast_rays origins {tag}", lambda: vw.cast_rays(dirs[:n], None, vorg[:n]))
        entry(f"voxel_cast_rays camera {tag}", lambda: vw.cast_rays(dirs[:n]))
    entry("voxel_destroy", vw.close)

    g = entry("glsl_create", lambda: sfrt.GlslShader(0))
    entry("glsl_set_ground", lambda: g.set_ground(*floor))
    for tag, (w, h), n in (("first", (160, 90), 64), ("grown", (320, 180), 4096)):
        g.set_uniforms(gs.default_uniforms(w, h, 0.3, 0.1, frames=20))
        entry(f"glsl_draw_image {tag}", lambda: g.draw_image(w, h))
        entry(f"glsl_draw_image_aux {tag}", lambda: g.draw_image_aux(w, h))
        entry(f"glsl_cast_rays {tag}", lambda: g.cast_rays(dirs[:n]))
    entry("glsl_set_ground again", lambda: g.set_ground(*floor))
    entry("glsl_destroy", g.close)
    entry("end", lambda: None)
    with open(labels_path, "w") as f:
        f.write("\n".join(labels) + "\n")


def entries(trace_csv, labels_path):
    """[(label, [HIP call names in order])] of one traced run."""
    rows = [r for r in csv.DictReader(open(trace_csv)) if r["Function"].startswith("hip")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Function"] for r in rows]
    cuts, k = [], 0
    while k < len(names) - 1:  # (a create after the marker starts with a third hipGetDeviceCount)
        if names[k] == MARK and names[k + 1] == MARK:
            cuts.append(k)
            k += 2
        else:
            k += 1
    labels = open(labels_path).read().split("\n")[:-1]
    # (torch's own initialisation, before the first entry point, counts the devices twice in a row)
    cuts = cuts[max(0, len(cuts) - len(labels)):]
    if len(cuts) != len(labels):
        raise SystemExit(f"{trace_csv}: {len(cuts)} markers for {len(labels)} labels")
    out = []
    for k, label in enumerate(labels):
        end = cuts[k + 1] if k + 1 < len(cuts) else cuts[k] + 2
        out.append((label, names[cuts[k] + 2:end]))
    return out[:-1]  # ("end", [])


def compare(old_csv, old_labels, new_csv, new_labels, out_path=None):
    old, new = entries(old_csv, old_labels), entries(new_csv, new_labels)
    if [l for l, _ in old] != [l for l, _ in new]:
        raise SystemExit("the two runs made different entry-point calls")
    lines, bad = [], 0
    for (label, a), (_, b) in zip(old, new):
        same = a == b
        bad += not same
        lines.append(f"{'same' if same else 'DIFF'} {label}: {len(a)} calls")
        lines.append("  parent: " + " ".join(a))
        if not same:
            lines.append("  new:    " + " ".join(b))
    lines.append(f"{len(old)} entry points, {bad} differ")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) >= 6 and sys.argv[1] == "compare":
        compare(*sys.argv[2:7])
    else:
        raise SystemExit(__doc__)
