"""Mesh worlds with and without the triangle hierarchy (GPU; not bench.py, no
gate).  One process, one GPU: for every world a context with the default
upload (the tree) and one created under RTC_DEBUG=tri_tree=0
(the flat triangle loop: what the library ran before) alternate, device events
around `--steps` launches after `--warmup`; a second default context gives the
A/A spread.  A flat launch of a large mesh takes seconds, so a cell's step
count shrinks until the cell fits `--cell-ms` (never below 2; recorded).

Worlds: icospheres of 1280, 5120, 20 480 and 81 920 triangles over a plane
under one light, and a 5 x 5 x 5 grid of 576-triangle tori (many separated
subtrees).  Runs, f32 at 1920 x 1080: the opaque mesh (direct kernel), the
glass mesh at depth 4 (pool kernel and containers walk), rt_trace_rays_device
on the camera's own rays, and the host's upload time.

--leaf 2,4,8 repeats the tree cells with RTC_DEBUG=tri_leaf=N;
--small measures meshes of 16..256 triangles with the tree forced
(RTC_DEBUG=tri_min=1) against the flat context, which takes its per-scene
build where the library would (the comparison kTriTreeMin is set from).

  python scripts/mesh_bench.py --out profiles/mesh.json
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ray-tracer-challenge-rs_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import mesh_worlds as M  # noqa: E402
import rtc_amd  # noqa: E402
from rtc_amd import world as W  # noqa: E402

WIDTH, HEIGHT = 1920, 1080


def tables_of(meshes, material, transforms=None):
    """A plane, one light and the meshes' triangles (rt_mesh_triangles, baked) as SceneTables."""
    floor = W.plane(W.Material(color=(0.7, 0.7, 0.7), specular=0.0), transform=W.translation(0, -1.3, 0))
    base = W.World([W.Light((-5.0, 6.0, -5.0))], [floor, W.sphere(material)]).tables()
    descs = []
    for k, mesh in enumerate(meshes):
        t = None if transforms is None else [v for row in transforms[k] for v in row]
        descs.append(mesh.shape_descs(t, True, 1))
    n = 1 + sum(len(d) for d in descs)
    shapes = (rtc_amd.ShapeDesc * n)()
    shapes[0] = base.shapes[0]
    at = 1
    for d in descs:
        C.memmove(C.byref(shapes, at * C.sizeof(rtc_amd.ShapeDesc)), d, len(d) * C.sizeof(rtc_amd.ShapeDesc))
        at += len(d)
    cam = W.camera(WIDTH, HEIGHT, 0.9, (0.3, 1.7, -4.2), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0))
    return rtc_amd.SceneTables(shapes, base.materials, base.patterns, base.lights, cam)


def mesh_of(verts, faces):
    return rtc_amd.load_obj(M.obj_text(verts, faces))


def context(knobs):
    old = os.environ.get("RTC_DEBUG")
    if knobs:
        os.environ["RTC_DEBUG"] = knobs
    try:
        return rtc_amd.Context(0)
    finally:
        if knobs:
            if old is None:
                del os.environ["RTC_DEBUG"]
            else:
                os.environ["RTC_DEBUG"] = old


def timed(fn, steps, warmup, cell_ms):
    """(ms per call, steps used): device time over `steps` calls, fewer if one call is long."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = (time.perf_counter() - t0) * 1e3
    steps = int(max(2, min(steps, cell_ms / max(one, 1e-3))))
    for _ in range(min(warmup, steps) if 2 * one < cell_ms else 0):  # (the first call warmed a long cell)
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, steps


def runs_for(ctx, tables, depth, rays):
    """{run name: launch closure} on torch's current stream."""
    import torch
    dev = torch.device("cuda", 0)
    out = torch.empty((HEIGHT, WIDTH, 3), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cam = tables.camera
    return {"frame": lambda: ctx.render_device(cam, out.data_ptr(), stream, depth=depth, precision="f32"),
            "rays": lambda: ctx.trace_rays(rays, depth)}


def camera_rays(cam):
    import torch
    inv = np.array(cam.inverse[:]).reshape(4, 4)
    xs, ys = np.meshgrid(np.arange(cam.width), np.arange(cam.height))
    p = np.stack([cam.half_width - (xs + 0.5) * cam.pixel_size, cam.half_height - (ys + 0.5) * cam.pixel_size,
                  -np.ones(xs.shape), np.ones(xs.shape)], axis=-1).reshape(-1, 4)
    origin = (np.array([0.0, 0.0, 0.0, 1.0]) @ inv.T)[:3]
    d = (p @ inv.T)[:, :3] - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.concatenate([np.broadcast_to(origin, d.shape), d], axis=1).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(r)).cuda()


def measure(name, tables, depth, contexts, args, wait_jit=False):
    """One world on every context of `contexts` ({label: knobs}), alternating; ms per launch."""
    rays = camera_rays(tables.camera)
    ctxs, rec = {}, {"world": name, "triangles": len(tables.shapes) - 1, "depth": depth, "ms": {}, "steps": {},
                     "upload_ms": {}, "tree": {}}
    for label, knobs in contexts.items():
        c = context(knobs)
        t0 = time.perf_counter()
        c.upload(tables)
        rec["upload_ms"][label] = (time.perf_counter() - t0) * 1e3
        rec["tree"][label] = c.tree_info()
        ctxs[label] = c
    launches = {label: runs_for(c, tables, depth, rays) for label, c in ctxs.items()}
    if wait_jit:  # the flat context's per-scene build, as a warm renderer has it
        for label, c in ctxs.items():
            for _ in range(3):
                launches[label]["frame"]()
            c.jit_wait()
            launches[label]["frame"]()
            rec.setdefault("per_scene", {})[label] = c.jit_status()["used"]
    for run in ("frame", "rays"):
        for label in ctxs:
            ms, steps = timed(launches[label][run], args.steps, args.warmup, args.cell_ms)
            rec["ms"][f"{run}/{label}"] = ms
            rec["steps"][f"{run}/{label}"] = steps
    for c in ctxs.values():
        c.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh.json"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cell-ms", type=float, default=1500.0, help="a cell's launches fit this, steps permitting")
    ap.add_argument("--subdivisions", default="3,4,5,6")
    ap.add_argument("--leaf", default="", help="also tri_leaf=N contexts, e.g. 2,4,8")
    ap.add_argument("--small", action="store_true", help="meshes of 16..256 triangles, tree forced vs flat")
    ap.add_argument("--no-grid", action="store_true")
    ap.add_argument("--many-shapes", action="store_true",
                    help="the 300- and 1500-shape worlds of tests/test_gpu_random_worlds.py (a quarter triangles)")
    args = ap.parse_args()
    contexts = {"tree": "", "tree_again": "", "flat": "tri_tree=0"}
    for n in [int(v) for v in args.leaf.split(",") if v]:
        contexts[f"leaf{n}"] = f"tri_leaf={n}"
    opaque = W.Material(color=(0.25, 0.6, 0.85), specular=0.5, shininess=60.0)
    records = []
    if args.many_shapes:
        import test_gpu_random_worlds as R
        for n in (300, 1500):
            tables, cam = R._many_shapes_world(n, n)
            tables.camera = rtc_amd.camera_resize(cam, WIDTH, HEIGHT)
            rec = measure(f"many_shapes_{n}", tables, 4, contexts, args, wait_jit=True)
            rec["triangles"] = sum(1 for s in tables.shapes if s.kind == 5)
            records.append(rec)
    elif args.small:
        small = {"tree": "tri_min=1", "tree_again": "tri_min=1", "flat": "tri_tree=0"}
        for cells in ((4, 2), (4, 4), (8, 4), (8, 8), (16, 8)):  # 16, 32, 64, 128, 256 triangles
            verts, faces = M.height_field(16)
            n = 17
            keep = [f for f in faces.tolist() if all(v % n <= cells[0] and v // n <= cells[1] for v in f)]
            mesh = mesh_of(verts, np.array(keep))
            lift = W.mat_mul(W.translation(1.5, 0.0, 1.5), W.rotation_x(-0.6))
            records.append(measure(f"field{len(keep)}", tables_of([mesh], opaque, [lift]), 3, small, args, wait_jit=True))
    else:
        for s in [int(v) for v in args.subdivisions.split(",") if v]:
            mesh = mesh_of(*M.icosphere(s))
            records.append(measure(f"ico{s}_opaque", tables_of([mesh], opaque), 3, contexts, args))
            records.append(measure(f"ico{s}_glass", tables_of([mesh], M.glass()), 4, contexts, args))
        if not args.no_grid:
            torus = mesh_of(*M.torus(24, 12))
            place = [W.mat_mul(W.translation(0.9 * (i - 2), 0.9 * (j - 2) + 0.6, 0.9 * (k - 2) + 1.0),
                               W.scaling(0.3, 0.3, 0.3)) for i in range(5) for j in range(5) for k in range(5)]
            records.append(measure("tori_5x5x5", tables_of([torus] * 125, opaque, place), 3, contexts, args))
    out = {"what": "ms per launch, f32 1920x1080; tree = default upload, flat = RTC_DEBUG=tri_tree=0",
           "records": records}
    # growth of the tree's frame time with the triangle count, and the A/A spread
    ico = [r for r in records if r["world"].endswith("_opaque")]
    if len(ico) >= 2:
        a, b = ico[0], ico[-1]
        out["exponent_opaque_frame"] = (math.log(b["ms"]["frame/tree"] / a["ms"]["frame/tree"]) /
                                        math.log(b["triangles"] / a["triangles"]))
    spreads = [abs(r["ms"][f"{run}/tree"] - r["ms"][f"{run}/tree_again"]) / r["ms"][f"{run}/tree"]
               for r in records for run in ("frame", "rays")]
    if spreads:
        out["aa_spread_max"] = max(spreads)
        out["aa_spread_median"] = statistics.median(spreads)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
