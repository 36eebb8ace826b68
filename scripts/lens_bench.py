"""Lens frames against the supersampled frames they extend (GPU; not bench.py, no gate).

For one scene, output size and grid n, in f32, at aperture 0.1 and the focal distance given per scene:

  ss           rt_render_supersampled_device: the pinhole frame, what the library offered before
  lens_none    rt_render_lens_device, RT_JITTER_NONE: the lens points read from the launch's table
  lens_hashed  rt_render_lens_device, RT_JITTER_HASHED: the lens point hashed per lane

each with the generic kernels (rt_context_set_jit 0) and with the per-scene builds made in line (RT_JIT_SYNC)
on two contexts of one process on one GPU.  The columns alternate for `--rounds` rounds of `--steps`
back-to-back launches each (torch events); the record holds every round's ms per frame, the medians, the
ratios to ss and the A/A spread of ss (max - min over its rounds), the margin below which a ratio says nothing.
`per_scene` says which launches the library ran per-scene kernels for.

  python scripts/lens_bench.py --out profiles/lens.json
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

# scene, output size, focal distance (about the camera's distance to what it looks at)
CASES = [("three_sphere_scene", 1920, 1080, 5.0), ("reflect_refract", 1920, 1080, 5.0), ("cover", 3840, 2160, 10.0)]
APERTURE = 0.1


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


def measure(ctxs, scene, name, width, height, focal, n, depth, steps, warmup, rounds):
    import torch
    dev = torch.device("cuda", 0)
    cam = rtc_amd.camera_resize(scene.camera, width, height)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty((height, width, 3), dtype=torch.float32, device=dev)
    lenses = {"lens_none": rtc_amd.Lens(APERTURE, focal, False), "lens_hashed": rtc_amd.Lens(APERTURE, focal, True, 1)}
    cols = {}
    for kernels, ctx in ctxs.items():
        cols[f"{kernels}/ss"] = (ctx, lambda ctx=ctx: ctx.render_supersampled_device(cam, n, out.data_ptr(), stream,
                                                                                   depth, "f32"))
        for key, lens in lenses.items():
            cols[f"{kernels}/{key}"] = (ctx, lambda ctx=ctx, lens=lens: ctx.render_lens_device(
                cam, n, lens, out.data_ptr(), stream, depth, "f32"))
    rec = {"scene": name, "width": width, "height": height, "grid": n, "depth": depth, "precision": "f32",
           "aperture": APERTURE, "focal_distance": focal, "sample_rays": n * n * width * height, "steps": steps,
           "warmup": warmup, "rounds": rounds, "device": torch.cuda.get_device_name(0), "per_scene": {}}
    for key, (ctx, fn) in cols.items():  # builds land here, outside the timing
        fn()
        torch.cuda.synchronize()
        rec["per_scene"][key] = ctx.jit_status()["used"]
    ms = {key: [] for key in cols}
    for _ in range(rounds):
        for key, (_, fn) in cols.items():
            ms[key].append(timed(fn, steps, warmup))
    for key, v in ms.items():
        rec[key] = {"ms_rounds": v, "ms": statistics.median(v)}
    for kernels in ctxs:
        base = rec[f"{kernels}/ss"]
        rec[f"{kernels}/ss_spread_ms"] = max(base["ms_rounds"]) - min(base["ms_rounds"])
        for key in lenses:
            rec[f"{kernels}/{key}_over_ss"] = rec[f"{kernels}/{key}"]["ms"] / base["ms"]
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", nargs="+", type=int, default=[2, 4])
    ap.add_argument("--depth", type=int, default=rtc_amd.RT_DEFAULT_MAX_DEPTH)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", nargs="+", help="scene names to keep of the built-in cases")
    ap.add_argument("--out", help="write the records to this JSON file as well")
    a = ap.parse_args()
    if rtc_amd.device_count() < 1:
        sys.exit("lens_bench: no HIP device (there is no CPU path to time)")
    recs = []
    for name, width, height, focal in CASES:
        if a.only and name not in a.only:
            continue
        scene = scene_io.load(os.path.join(ROOT, "tests", "golden", "scenes", f"{name}.json"))
        with rtc_amd.Context(0) as generic, rtc_amd.Context(0) as per_scene:
            generic.set_jit(0)
            per_scene.set_jit(rtc_amd.RT_JIT_SYNC)
            for ctx in (generic, per_scene):
                ctx.upload(scene)
            for n in a.grids:
                recs.append(measure({"generic": generic, "per_scene": per_scene}, scene, name, width, height, focal, n,
                                    a.depth, a.steps, a.warmup, a.rounds))
                print(json.dumps(recs[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "scripts/lens_bench.py: ms per frame, f32, one GPU; ss = rt_render_supersampled_device, "
                               "lens_none / lens_hashed = rt_render_lens_device at aperture 0.1 with RT_JITTER_NONE / "
                               "RT_JITTER_HASHED, each with the generic and the per-scene kernels",
                       "runs": recs}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
