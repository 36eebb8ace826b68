"""Smooth against flat uploads of the same mesh (GPU; not bench.py, no gate).
One process, one GPU, f32 at 1920 x 1080: for every world a context with the
smooth upload (rt_scene_upload_smooth: the instance build's kernels, one more
triangle test and nine loads per shaded hit on a smooth triangle, DESIGN.md
§3.11), a second one like it for the A/A spread, and one with the same tables
without the normals (the flat upload: the kernels the world ran before)
alternate, device events around `--steps` launches after `--warmup`, in the
style of scripts/mesh_bench.py.

Worlds: icospheres of 1280 and 20 480 triangles whose vertex normals are their
positions, opaque (direct kernel) and glass at depth 4 (pool kernel), over a
plane under one light; and the 5 x 5 x 5 grid of 576-triangle tori as 125
instances of one smooth mesh, opaque.  Runs: frames, rt_trace_rays_device on
the camera's own rays, the host's upload time, the device bytes of the normal
tables, and the frame's hit counts (what the smooth code's cost scales with).

  python scripts/smooth_bench.py --out profiles/smooth.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ray-tracer-challenge-rs_amd", "tests", "scripts"):
    sys.path.insert(0, os.path.join(ROOT, p))
import mesh_bench as B  # noqa: E402
import mesh_worlds as M  # noqa: E402
import rtc_amd  # noqa: E402
import smooth_worlds as S  # noqa: E402
from rtc_amd import world as W  # noqa: E402


def camera():
    return W.camera(B.WIDTH, B.HEIGHT, 0.9, (0.3, 1.7, -4.2), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0))


def floor_and_light():
    return [W.Light((-5.0, 6.0, -5.0))], [W.plane(W.Material(color=(0.7, 0.7, 0.7), specular=0.0),
                                                  transform=W.translation(0, -1.3, 0))]


def ico_world(subdivisions, material):
    lights, shapes = floor_and_light()
    mesh = S.load(rtc_amd, *S.icosphere(subdivisions))
    return W.World(lights, shapes + W.mesh(mesh, material, smooth=True)).tables(camera())


def tori_world(material):
    lights, shapes = floor_and_light()
    verts, faces = M.torus(24, 12)
    ring = np.stack([verts[:, 0], np.zeros(len(verts)), verts[:, 2]], axis=1)
    ring /= np.linalg.norm(ring, axis=1)[:, None]
    mesh = S.load(rtc_amd, verts, faces, (verts - ring) / 0.4)
    place = [W.mat_mul(W.translation(0.9 * (i - 2), 0.9 * (j - 2) + 0.6, 0.9 * (k - 2) + 1.0), W.scaling(0.3, 0.3, 0.3))
             for i in range(5) for j in range(5) for k in range(5)]
    return W.World(lights, shapes, [W.instance(mesh, material, transform=t, smooth=True) for t in place]).tables(camera())


def measure(name, tables, depth, args):
    flat = S.flat_of(rtc_amd, tables)
    uploads = {"smooth": tables, "smooth_again": tables, "flat": flat}
    rays = B.camera_rays(tables.camera)
    rec = {"world": name, "depth": depth, "ms": {}, "steps": {}, "upload_ms": {}}
    ctxs = {}
    for label, t in uploads.items():
        c = rtc_amd.Context(0)
        t0 = time.perf_counter()
        c.upload(t)
        rec["upload_ms"][label] = (time.perf_counter() - t0) * 1e3
        ctxs[label] = c
    rec["instance_info"] = {k: v for k, v in ctxs["smooth"].instance_info().items() if k != "build_ms"}
    rec["tree"] = ctxs["smooth"].tree_info()
    rec["frame_counts"] = {}
    for label in ("smooth", "flat"):  # (the normals change where glass sends its rays: the two frames differ)
        _, st = ctxs[label].render(tables.camera, depth, precision="f32")
        rec["frame_counts"][label] = {k: st[k] for k in ("primary", "shadow", "reflect", "refract", "shaded")}
    rec["smooth_info"] = ctxs["smooth"].smooth_info()
    launches = {label: B.runs_for(c, uploads[label], depth, rays) for label, c in ctxs.items()}
    for run in ("frame", "rays"):
        for label in ctxs:
            ms, steps = B.timed(launches[label][run], args.steps, args.warmup, args.cell_ms)
            rec["ms"][f"{run}/{label}"] = ms
            rec["steps"][f"{run}/{label}"] = steps
        rec.setdefault("smooth_over_flat", {})[run] = rec["ms"][f"{run}/smooth"] / rec["ms"][f"{run}/flat"]
        rec.setdefault("aa_spread", {})[run] = abs(rec["ms"][f"{run}/smooth"] - rec["ms"][f"{run}/smooth_again"]) / \
            rec["ms"][f"{run}/smooth"]
    for c in ctxs.values():
        c.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth.json"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cell-ms", type=float, default=1500.0, help="a cell's launches fit this, steps permitting")
    ap.add_argument("--subdivisions", default="3,5")
    ap.add_argument("--no-grid", action="store_true")
    args = ap.parse_args()
    records = []
    for s in [int(v) for v in args.subdivisions.split(",") if v]:
        records.append(measure(f"ico{s}_opaque", ico_world(s, S.opaque()), 3, args))
        records.append(measure(f"ico{s}_glass", ico_world(s, M.glass()), 4, args))
    if not args.no_grid:
        records.append(measure("tori_5x5x5_instanced", tori_world(S.opaque()), 3, args))
    spreads = [r["aa_spread"][run] for r in records for run in ("frame", "rays")]
    out = {"what": "ms per launch, f32 1920x1080; smooth = rt_scene_upload_smooth, flat = the same tables without "
                   "the normals, smooth_again = a second smooth context (A/A)",
           "records": records, "aa_spread_max": max(spreads), "aa_spread_median": statistics.median(spreads)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
