"""Supersampled frames against the two ways a caller had before (GPU; not
bench.py, no gate).  For one scene, output size and grid n, in f32, with Cn
the output camera resized to n W x n H:

  ss        (a) rt_render_supersampled_device: n x n samples per pixel averaged
            in the frame kernel, one W x H frame written
  frame_avg (b) rt_render_device of Cn into a torch buffer, then
            torch.nn.functional.avg_pool2d over n x n (what a caller did)
  frame     (c) rt_render_device of Cn alone: the same sample rays, n^2 times
            the output

All three from one process on one GPU, alternating a, b, c for `--rounds`
rounds of `--steps` back-to-back launches each (torch events); the record
holds every round's ms per frame, the medians, and the spread of (c), which is
the margin for "(a) is no slower than (c) per sample ray".  Kernels as a warm
renderer runs them: per-scene builds made in line (RT_JIT_SYNC) where the
library takes them, `per_scene` says which.

--once launches each column once per case and prints the order, for a counter
run of its own around the script (rocprofv3 --pmc WRITE_SIZE, then FETCH_SIZE).

  python scripts/supersample_bench.py --out profiles/supersample.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracer-challenge-rs_amd"))
import rtc_amd  # noqa: E402
from rtc_amd import scene_io  # noqa: E402

CASES = [("three_sphere_scene", 1920, 1080), ("reflect_refract", 1920, 1080), ("cover", 3840, 2160)]


def timed(fn, steps, warmup):
    """Milliseconds per call of fn (device time, torch events on the current stream)."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def measure(ctx, scene, name, width, height, n, depth, steps, warmup, rounds, once):
    import torch
    import torch.nn.functional as F
    dev = torch.device("cuda", 0)
    cam = rtc_amd.camera_resize(scene.camera, width, height)
    cn = rtc_amd.camera_resize(scene.camera, n * width, n * height)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty((height, width, 3), dtype=torch.float32, device=dev)
    big = torch.empty((n * height, n * width, 3), dtype=torch.float32, device=dev)

    def ss():
        ctx.render_supersampled_device(cam, n, out.data_ptr(), stream, depth, "f32")

    def frame():
        ctx.render_device(cn, big.data_ptr(), stream, depth, "f32")

    def frame_avg():
        frame()
        return F.avg_pool2d(big.permute(2, 0, 1).unsqueeze(0), n)

    rec = {"scene": name, "width": width, "height": height, "grid": n, "depth": depth, "precision": "f32",
           "sample_rays": n * n * width * height, "steps": steps, "warmup": warmup, "rounds": rounds,
           "device": torch.cuda.get_device_name(0)}
    used = {}
    for key, fn in (("ss", ss), ("frame", frame)):  # builds land here, outside the timing
        fn()
        torch.cuda.synchronize()
        used[key] = ctx.jit_status()["used"]
    rec["per_scene"] = used
    pooled = frame_avg()[0].permute(1, 2, 0)
    ss()
    torch.cuda.synchronize()
    rec["ss_vs_frame_avg_max_abs_diff"] = float((pooled - out).abs().max())
    if once:
        for key, fn in (("ss", ss), ("frame_avg", frame_avg), ("frame", frame)):
            fn()
            torch.cuda.synchronize()
            print(f"once: {name} {width}x{height} n={n} {key}", flush=True)
        return rec
    ms = {"ss": [], "frame_avg": [], "frame": []}
    for _ in range(rounds):
        for key, fn in (("ss", ss), ("frame_avg", frame_avg), ("frame", frame)):
            ms[key].append(timed(fn, steps, warmup))
    for key, v in ms.items():
        rec[key] = {"ms_rounds": v, "ms": statistics.median(v),
                    "msample_s": rec["sample_rays"] / statistics.median(v) / 1e3}
    rec["frame_spread_ms"] = max(ms["frame"]) - min(ms["frame"])
    rec["ss_over_frame"] = rec["ss"]["ms"] / rec["frame"]["ms"]
    rec["ss_over_frame_avg"] = rec["ss"]["ms"] / rec["frame_avg"]["ms"]
    rec["ss_no_slower_than_frame"] = rec["ss"]["ms"] <= rec["frame"]["ms"] + rec["frame_spread_ms"]
    rec["ss_faster_than_frame_avg"] = rec["ss"]["ms"] < rec["frame_avg"]["ms"]
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", nargs="+", type=int, default=[2, 4])
    ap.add_argument("--depth", type=int, default=rtc_amd.RT_DEFAULT_MAX_DEPTH)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--jit", type=int, default=rtc_amd.RT_JIT_SYNC, help="rt_context_set_jit mode (0 = generic kernels)")
    ap.add_argument("--only", nargs="+", help="scene names to keep of the built-in cases")
    ap.add_argument("--once", action="store_true", help="one launch per column and case (a counter run)")
    ap.add_argument("--out", help="write the records to this JSON file as well")
    a = ap.parse_args()
    if rtc_amd.device_count() < 1:
        sys.exit("supersample_bench: no HIP device (there is no CPU path to time)")
    recs = []
    for name, width, height in CASES:
        if a.only and name not in a.only:
            continue
        scene = scene_io.load(os.path.join(ROOT, "tests", "golden", "scenes", f"{name}.json"))
        with rtc_amd.Context(0) as ctx:
            ctx.set_jit(a.jit)
            ctx.upload(scene)
            for n in a.grids:
                recs.append(measure(ctx, scene, name, width, height, n, a.depth, a.steps, a.warmup, a.rounds, a.once))
                print(json.dumps(recs[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "scripts/supersample_bench.py: ms per frame, f32, one GPU; ss = rt_render_supersampled_device, "
                               "frame_avg = rt_render_device of the n x size frame + avg_pool2d, frame = that frame alone",
                       "runs": recs}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
