"""Shutter frames of moving worlds against what they extend and what they replace (GPU; not bench.py, no gate).

For one moving world, grid n (2 and 4), pinhole and lens (aperture 0.1), f32, 1280 x 720, shutter [0, 1] at the
cell centres, the columns are ms per frame (torch events around `--steps` back-to-back launches):

  static        the same world without its velocities (SceneTables.at_time(0)) through rt_render_lens_device
                (rt_render_supersampled_device without a lens): the frame before there was time;
  shutter       the moving world through rt_render_shutter_device: shutter / static is the price of time;
  still         the moving world through the older entry point (rt_render_lens_device /
                rt_render_supersampled_device): what the motion build costs a caller who asks for no time;
  shutter_nocull the moving world on a context made under RTC_DEBUG=cull=0: what the displaced culls keep;
  host_average  what a caller had before: n^2 uploads of at_time(tau) worlds, each rendered with rt_render into a
                host array, averaged on the host; wall clock, upload and readback included.

The columns alternate for `--rounds` rounds; the record holds every round's ms, the medians, the ratios and the
A/A spread of `static` (max - min over its rounds), below which a ratio says nothing.  A timed ray batch of 2^20
camera rays (rt_trace_rays_timed_device, times uniform in [0, 1]) stands beside the same batch without times in
the static world.

Worlds: `casters` a checkered floor under 24 moving spheres, cubes and cylinders; `cover` the cover scene's
shapes with a third of the bounded ones moving; `tori` 125 instances of a 576-triangle torus, every second one
moving.

  python scripts/motion_bench.py --out profiles/motion.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import mesh_bench as B  # noqa: E402  (puts the package and tests/ on the path)
import mesh_worlds as M  # noqa: E402
import rtc_amd  # noqa: E402
from rtc_amd import scene_io  # noqa: E402
from rtc_amd import world as W  # noqa: E402

WIDTH, HEIGHT = 1280, 720
APERTURE, FOCUS = 0.1, 5.0


def casters():
    rng = np.random.default_rng(3)
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.9, 0.9, 0.9), (0.2, 0.3, 0.4)), specular=0.0))
    shapes = [floor]
    for k in range(24):
        mat = W.Material(color=tuple(rng.uniform(0.2, 0.9, 3)), specular=0.4)
        place = W.mat_mul(W.translation(*(rng.uniform(-3, 3), rng.uniform(0.4, 2.5), rng.uniform(-1, 4))),
                          W.scaling(*([rng.uniform(0.2, 0.45)] * 3)))
        s = (W.sphere(mat, place), W.cube(mat, place), W.cylinder(-1.0, 1.0, True, mat, place))[k % 3]
        s.velocity = tuple(rng.uniform(-1.5, 1.5, 3) * (1.0, 0.2, 1.0))
        shapes.append(s)
    cam = W.camera(WIDTH, HEIGHT, 0.9, (0.0, 1.5, -6.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0))
    return W.World([W.Light((-5.0, 8.0, -6.0))], shapes).tables(cam), 2


def cover():
    scene = scene_io.load(os.path.join(ROOT, "tests", "golden", "scenes", "cover.json"))
    rng = np.random.default_rng(4)
    bounded = [i for i, s in enumerate(scene.shapes) if s.kind != rtc_amd.SHAPE_KINDS["plane"]]
    movers = bounded[::3]
    motion = (rtc_amd.MotionDesc * len(movers))()
    for m, i in zip(motion, movers):
        m.target, m.index = rtc_amd.RT_MOVE_SHAPE, i
        m.velocity[:] = list(rng.uniform(-1.0, 1.0, 3))
    scene.motion = motion
    scene.camera = rtc_amd.camera_resize(scene.camera, WIDTH, HEIGHT)
    return scene, 5


def tori():
    mesh = B.mesh_of(*M.torus(24, 12))
    half, places = 2.0, []
    for i in range(5):
        for j in range(5):
            for k in range(5):
                places.append(W.mat_mul(W.translation(0.9 * (i - half), 0.9 * (j - half) + 0.6, 0.9 * (k - half) + 1.0),
                                        W.scaling(0.3, 0.3, 0.3)))
    rng = np.random.default_rng(5)
    inst = [W.instance(mesh, W.Material(color=(0.25, 0.6, 0.85), specular=0.5, shininess=60.0), p) for p in places]
    for it in inst[::2]:
        it.velocity = tuple(rng.uniform(-0.6, 0.6, 3))
    floor = W.plane(W.Material(color=(0.7, 0.7, 0.7), specular=0.0), transform=W.translation(0, -1.3, 0))
    cam = W.camera(WIDTH, HEIGHT, 0.9, (0.3, 1.7, -4.2), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0))
    return W.World([W.Light((-5.0, 6.0, -5.0))], [floor], inst).tables(cam), 3


WORLDS = {"casters": casters, "cover": cover, "tori": tori}


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


def host_average(ctx, scene, cam, n, depth):
    """Wall-clock ms of the caller's way before: n^2 displaced worlds uploaded, rendered, read back and averaged."""
    t0 = time.perf_counter()
    acc = np.zeros((cam.height, cam.width, 3), dtype=np.float32)
    for c in range(n * n):
        ctx.upload(scene.at_time((c + 0.5) / (n * n)))
        img, _ = ctx.render(cam, depth, precision="f32")
        acc += img
    acc *= 1.0 / (n * n)
    return (time.perf_counter() - t0) * 1e3


def measure(name, scene, depth, n, lens, a):
    import torch
    dev = torch.device("cuda", 0)
    cam = scene.camera
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty((cam.height, cam.width, 3), dtype=torch.float32, device=dev)
    L = rtc_amd.Lens(APERTURE, FOCUS) if lens else None
    sh = rtc_amd.Shutter(0.0, 1.0)
    ctxs = {"static": rtc_amd.Context(0), "moving": rtc_amd.Context(0), "nocull": B.context("cull=0"), "host": rtc_amd.Context(0)}
    for c in ctxs.values():
        c.set_jit(0)  # the generic kernels everywhere: a moving world has no per-scene build to compare with
    ctxs["static"].upload(scene.at_time(0.0))
    ctxs["moving"].upload(scene)
    ctxs["nocull"].upload(scene)

    def older(ctx):
        if L is None:
            return lambda: ctx.render_supersampled_device(cam, n, out.data_ptr(), stream, depth, "f32")
        return lambda: ctx.render_lens_device(cam, n, L, out.data_ptr(), stream, depth, "f32")

    def shutter(ctx):
        return lambda: ctx.render_shutter_device(cam, n, sh, out.data_ptr(), L, stream, depth, "f32")
    cols = {"static": older(ctxs["static"]), "shutter": shutter(ctxs["moving"]), "still": older(ctxs["moving"]),
            "shutter_nocull": shutter(ctxs["nocull"])}
    rec = {"world": name, "width": cam.width, "height": cam.height, "grid": n, "lens": bool(lens), "depth": depth,
           "precision": "f32", "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "motion": ctxs["moving"].motion_info()}
    ms = {key: [] for key in cols}
    ms["host_average"] = []
    for _ in range(a.rounds):
        for key, fn in cols.items():
            ms[key].append(timed(fn, a.steps, a.warmup))
        ms["host_average"].append(host_average(ctxs["host"], scene, cam, n, depth))
    for key, v in ms.items():
        rec[key] = {"ms_rounds": v, "ms": statistics.median(v)}
    base = rec["static"]["ms"]
    rec["static_spread_ms"] = max(ms["static"]) - min(ms["static"])
    rec["shutter_over_static"] = rec["shutter"]["ms"] / base
    rec["still_over_static"] = rec["still"]["ms"] / base
    rec["nocull_over_shutter"] = rec["shutter_nocull"]["ms"] / rec["shutter"]["ms"]
    rec["host_average_over_shutter"] = rec["host_average"]["ms"] / rec["shutter"]["ms"]
    for c in ctxs.values():
        c.close()
    return rec


def measure_rays(name, scene, depth, a):
    """2^20 camera rays of a 1024 x 1024 frame: timed in the moving world, untimed in the static one."""
    import torch
    cam = rtc_amd.camera_resize(scene.camera, 1024, 1024)
    rays = B.camera_rays(cam)
    times = torch.rand(rays.shape[0], dtype=torch.float32, device=rays.device, generator=torch.Generator(rays.device).manual_seed(1))
    with rtc_amd.Context(0) as still, rtc_amd.Context(0) as moving:
        still.upload(scene.at_time(0.0))
        moving.upload(scene)
        cols = {"static": lambda: still.trace_rays(rays, depth), "timed": lambda: moving.trace_rays(rays, depth, times=times),
                "untimed_on_moving": lambda: moving.trace_rays(rays, depth)}
        ms = {key: [] for key in cols}
        for _ in range(a.rounds):
            for key, fn in cols.items():
                ms[key].append(timed(fn, a.steps, a.warmup))
    rec = {"world": name, "rays": int(rays.shape[0]), "depth": depth, "precision": "f32"}
    for key, v in ms.items():
        rec[key] = {"ms_rounds": v, "ms": statistics.median(v)}
    rec["static_spread_ms"] = max(ms["static"]) - min(ms["static"])
    rec["timed_over_static"] = rec["timed"]["ms"] / rec["static"]["ms"]
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", nargs="+", type=int, default=[2, 4])
    ap.add_argument("--worlds", nargs="+", default=list(WORLDS))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", help="write the records to this JSON file as well")
    a = ap.parse_args()
    if rtc_amd.device_count() < 1:
        sys.exit("motion_bench: no HIP device (there is no CPU path to time)")
    frames, batches = [], []
    for name in a.worlds:
        scene, depth = WORLDS[name]()
        for n in a.grids:
            for lens in (False, True):
                frames.append(measure(name, scene, depth, n, lens, a))
                print(json.dumps(frames[-1]), flush=True)
        batches.append(measure_rays(name, scene, depth, a))
        print(json.dumps(batches[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "scripts/motion_bench.py: ms per frame, f32, 1280 x 720, one GPU, shutter [0, 1] at the cell "
                               "centres; static = the world without velocities through rt_render_lens_device / "
                               "rt_render_supersampled_device, shutter = rt_render_shutter_device, still = the moving world "
                               "through the older entry point, shutter_nocull = under RTC_DEBUG=cull=0, host_average = n^2 "
                               "uploads of at_time worlds rendered with rt_render and averaged on the host (wall clock)",
                       "frames": frames, "ray_batches": batches}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
