"""Cost of in-kernel supersampling (SFRT_OPT_SUPERSAMPLE) against the plain large frame.

    python tools/bench_supersample.py [--warmup 50] [--frames 200] [--repeats 5]
                                      [--out profiles/supersample_bench.json]

Frames: lcg64 pose (0, 0) at 1920x1080 S=2, 1920x1080 S=4 and 3840x2160 S=2.  For each, in
one process, the supersampled W x H frame and the plain (S = 1) S*W x S*H frame -- the same
rays, a path this option does not change -- are timed alternately, `repeats` times each:

* kernel: render_band frames back to back on one stream (adaptive tile order), HIP events
  around every EVENT_EVERY-th frame, the empty event pair's own time subtracted (as
  bench.py times its headline); also the wall time per frame of the same loop;
* to host: submit_frame / wait_frame into pinned memory, two frames in flight, wall time
  per frame.

Expectation (stated before measuring): the supersampled kernel takes no longer than the
plain large frame's, within that plain frame's own run-to-run spread (max - min over the
repeats); the to-host time approaches 1 / S^2 of the plain large frame's.  The JSON holds
every repeat, the medians, the verdicts and the command line.  One supersampled frame per
case is also compared, on the device, with the box filter of the plain frame.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sfml-software-raytracer_amd"))

CASES = [(1920, 1080, 2), (1920, 1080, 4), (3840, 2160, 2)]
EVENT_EVERY = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "supersample_bench.json"))
    a = ap.parse_args()
    if a.warmup < 50 or a.frames < 200 or a.repeats < 5:
        raise SystemExit("at least 50 warm-up frames, 200 timed frames and 5 repeats")

    import numpy as np
    import torch
    import scenes
    import sfrt

    stream = torch.cuda.Stream()
    floor = scenes.load_floor()
    scene = scenes.lcg64().posed(0.0, 0.0)

    def event_gap():
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                 for _ in range(64)]
        for x, y in pairs:
            x.record(stream)
            y.record(stream)
        torch.cuda.synchronize()
        return float(np.median([x.elapsed_time(y) for x, y in pairs]))

    def world(width, height, s):
        w = sfrt.World(0)
        w.load_texture(*floor)
        w.set_scene(scene, width, height)
        w.set_option(sfrt.SFRT_OPT_SUPERSAMPLE, s)
        return w

    def kernel_time(w, buf, width, height):
        """(kernel us per frame from events, wall us per frame) of one repeat."""
        for _ in range(a.warmup):
            w.render_band(buf.data_ptr(), width * 4, 0, height, stream.cuda_stream)
        torch.cuda.synchronize()
        sampled = [k for k in range(a.frames) if k % EVENT_EVERY == 0]
        ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for k in sampled}
        t0 = time.perf_counter()
        for k in range(a.frames):
            if k in ev:
                ev[k][0].record(stream)
            w.render_band(buf.data_ptr(), width * 4, 0, height, stream.cuda_stream)
            if k in ev:
                ev[k][1].record(stream)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / a.frames
        w.check(stream.cuda_stream)
        raw = sum(x.elapsed_time(y) for x, y in ev.values()) / len(ev)
        return max(0.0, raw - event_gap()) * 1e3, wall * 1e6

    def host_time(w, frames):
        """Wall us per frame of submit_frame / wait_frame with two frames in flight."""
        tickets = [w.submit_frame(frames[k % 2]) for k in range(2)]  # warm both slots
        for t in tickets:
            w.wait_frame(t)
        t0 = time.perf_counter()
        prev = None
        for k in range(a.frames):
            t = w.submit_frame(frames[k % 2])
            if prev is not None:
                w.wait_frame(prev)
            prev = t
        w.wait_frame(prev)
        return (time.perf_counter() - t0) / a.frames * 1e6

    def med(v):
        return float(np.median(v))

    out = {"command": "python " + " ".join([os.path.relpath(os.path.abspath(sys.argv[0]), ROOT)] +
                                            sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "build_flavour": sfrt.build_flavour(),
           "scene": "lcg64 pose (0, 0)", "warmup": a.warmup, "frames": a.frames,
           "repeats": a.repeats, "event_every": EVENT_EVERY, "cases": []}
    for width, height, s in CASES:
        bw, bh = s * width, s * height
        ws, wp = world(width, height, s), world(bw, bh, 1)
        small = torch.empty(height, width * 4, dtype=torch.uint8, device="cuda")
        big = torch.empty(bh, bw * 4, dtype=torch.uint8, device="cuda")
        rec = {"width": width, "height": height, "factor": s, "plain_width": bw, "plain_height": bh,
               "supersampled": {"kernel_us": [], "wall_us": [], "to_host_us": []},
               "plain_large": {"kernel_us": [], "wall_us": [], "to_host_us": []}}
        for _ in range(a.repeats):  # alternately, so that drift hits both alike
            for key, w, buf, fw, fh in (("plain_large", wp, big, bw, bh),
                                        ("supersampled", ws, small, width, height)):
                k_us, wall_us = kernel_time(w, buf, fw, fh)
                rec[key]["kernel_us"].append(round(k_us, 2))
                rec[key]["wall_us"].append(round(wall_us, 2))
        # bytes: the supersampled frame is the box filter of the plain one
        torch.cuda.synchronize()
        sums = big.view(height, s, width, s, 4).to(torch.int32).sum(dim=(1, 3))
        want = ((sums + s * s // 2) >> (2 if s == 2 else 4)).to(torch.uint8)
        rec["bytes_equal_filtered_plain"] = bool(torch.equal(want, small.view(height, width, 4)))
        host_small = [sfrt.HostFrame(width * height * 4) for _ in range(2)]
        host_big = [sfrt.HostFrame(bw * bh * 4) for _ in range(2)]
        for _ in range(a.repeats):
            rec["plain_large"]["to_host_us"].append(round(host_time(wp, host_big), 2))
            rec["supersampled"]["to_host_us"].append(round(host_time(ws, host_small), 2))
        for f in host_small + host_big:
            f.free()
        ws.close()
        wp.close()
        p, q = rec["plain_large"], rec["supersampled"]
        for d in (p, q):
            for name in ("kernel_us", "wall_us", "to_host_us"):
                d[name + "_median"] = round(med(d[name]), 2)
        spread = max(p["kernel_us"]) - min(p["kernel_us"])
        rec["plain_kernel_spread_us"] = round(spread, 2)
        rec["kernel_ratio"] = round(q["kernel_us_median"] / p["kernel_us_median"], 4)
        rec["kernel_within_expectation"] = bool(q["kernel_us_median"] <= p["kernel_us_median"] + spread)
        rec["to_host_ratio"] = round(q["to_host_us_median"] / p["to_host_us_median"], 4)
        rec["to_host_ideal_ratio"] = round(1.0 / (s * s), 4)
        out["cases"].append(rec)
        print(f"{width}x{height} S={s}: kernel {q['kernel_us_median']:.1f} us vs plain {bw}x{bh} "
              f"{p['kernel_us_median']:.1f} us (spread {spread:.1f}); to host "
              f"{q['to_host_us_median']:.1f} vs {p['to_host_us_median']:.1f} us; "
              f"bytes {'ok' if rec['bytes_equal_filtered_plain'] else 'DIFFER'}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote " + a.out)
    if not all(c["bytes_equal_filtered_plain"] for c in out["cases"]):
        raise SystemExit("a supersampled frame differs from the filtered plain frame")


if __name__ == "__main__":
    main()
