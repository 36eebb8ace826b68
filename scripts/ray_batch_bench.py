"""Throughput of the ray-batch path against the two older ways to the same
colours (GPU; not bench.py, no gate).  For one scene and canvas, in f32:

  trace_rays_device   rt_trace_rays_device on the camera's own rays, computed
                      on the device in torch and kept there (no host copy)
  color_at_host       rt_color_at on the same rays from the host (f64 up,
                      f64 back, a sync: the whole call's wall time, and the
                      kernel's own time from its stats)
  render_device       rt_render_device of the same frame (the generic kernel:
                      RT_JIT_OFF; --per-scene adds the per-scene build)

Rates are primary rays (= pixels) per second; `rays_per_frame` counts every
ray (shadow, reflected, refracted) for those who want the other rate.  Device
times are torch events around `--steps` back-to-back launches after
`--warmup`.  One JSON object per scene; --out collects them in one file
(profiles/ray_batch.json).

  python scripts/ray_batch_bench.py --scenes three_sphere_scene reflect_refract --out profiles/ray_batch.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracer-challenge-rs_amd"))
import rtc_amd  # noqa: E402
from rtc_amd import scene_io  # noqa: E402


def camera_rays_device(cam, device):
    """Camera::ray_for_pixel (camera.rs:52-68) for every pixel, row-major, as an (n, 6) f64 tensor."""
    import torch
    f = dict(dtype=torch.float64, device=device)
    y, x = torch.meshgrid(torch.arange(cam.height, **f), torch.arange(cam.width, **f), indexing="ij")
    wx = cam.half_width - (x.reshape(-1) + 0.5) * cam.pixel_size
    wy = cam.half_height - (y.reshape(-1) + 0.5) * cam.pixel_size
    m = torch.tensor(cam.inverse[:], **f).reshape(4, 4)
    origin = torch.tensor(cam.origin[:], **f)
    pixel = torch.stack([wx, wy, -torch.ones_like(wx), torch.ones_like(wx)], dim=1) @ m.T
    d = pixel[:, :3] - origin
    d = d / d.norm(dim=1, keepdim=True)
    return torch.cat([origin.expand_as(d), d], dim=1).contiguous()


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


def measure(name, width, height, depth, steps, warmup, per_scene):
    import torch
    scene = scene_io.load(os.path.join(ROOT, "tests", "golden", "scenes", f"{name}.json"))
    cam = rtc_amd.camera_resize(scene.camera, width, height)
    n = width * height
    dev = torch.device("cuda", 0)
    rec = {"scene": name, "width": width, "height": height, "depth": depth, "precision": "f32", "rays": n,
           "steps": steps, "warmup": warmup, "device": torch.cuda.get_device_name(0)}
    with rtc_amd.Context(0) as ctx:
        ctx.set_jit(rtc_amd.RT_JIT_OFF)
        ctx.upload(scene)
        rays64 = camera_rays_device(cam, dev)
        rays32 = rays64.float().contiguous()
        stream = torch.cuda.current_stream(dev).cuda_stream

        before = ctx.counters()
        rgb = ctx.trace_rays(rays32, depth)
        torch.cuda.synchronize()
        rec["rays_per_frame"] = ctx.counters()["rays"] - before["rays"]
        ms = timed(lambda: ctx.trace_rays(rays32, depth), steps, warmup)
        rec["trace_rays_device"] = {"ms": ms, "mray_s": n / ms / 1e3}

        frame = torch.empty((height, width, 3), dtype=torch.float32, device=dev)
        render = lambda: ctx.render_device(cam, frame.data_ptr(), stream, depth, "f32")  # noqa: E731
        ms = timed(render, steps, warmup)
        rec["render_device"] = {"ms": ms, "mray_s": n / ms / 1e3, "kernel": "generic"}
        diff = (rgb.reshape(frame.shape) - frame).abs().amax(dim=2)
        rec["trace_rays_vs_frame"] = {"max_abs_diff": float(diff.max()), "share_within_2_255": float((diff <= 2 / 255).float().mean())}

        host = rays64.cpu().numpy()
        walls, kernels = [], []
        for i in range(1 + 3):  # the first call sizes the staging buffer
            t0 = time.perf_counter()
            _, st = ctx.color_at(host, depth, precision="f32")
            if i:
                walls.append((time.perf_counter() - t0) * 1e3)
                kernels.append(st["kernel_ms"])
        rec["color_at_host"] = {"wall_ms": float(np.median(walls)), "mray_s": n / float(np.median(walls)) / 1e3,
                                "kernel_ms": float(np.median(kernels)),
                                "kernel_mray_s": n / float(np.median(kernels)) / 1e3}
        if per_scene:
            ctx.set_jit(rtc_amd.RT_JIT_SYNC)
            render()
            torch.cuda.synchronize()
            if ctx.jit_status()["used"]:
                ms = timed(render, steps, warmup)
                rec["render_device_per_scene"] = {"ms": ms, "mray_s": n / ms / 1e3, "kernel": "per-scene"}
            else:
                rec["render_device_per_scene"] = {"kernel": "per-scene build not used", "log": ctx.jit_status()["log"][-300:]}
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", nargs="+", default=["three_sphere_scene", "reflect_refract"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=rtc_amd.RT_DEFAULT_MAX_DEPTH)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--per-scene", action="store_true", help="also time rt_render_device with the per-scene kernel")
    ap.add_argument("--out", help="write the records to this JSON file as well")
    a = ap.parse_args()
    if rtc_amd.device_count() < 1:
        sys.exit("ray_batch_bench: no HIP device (there is no CPU path to time)")
    recs = []
    for name in a.scenes:
        recs.append(measure(name, a.width, a.height, a.depth, a.steps, a.warmup, a.per_scene))
        print(json.dumps(recs[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "scripts/ray_batch_bench.py: primary rays per second, f32, one GPU", "runs": recs}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
