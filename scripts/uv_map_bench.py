"""Texture maps against the planar map and against a stripe pattern (GPU; not bench.py, no gate).
One process, one GPU, f32 at 1920 x 1080, in the style of scripts/texture_bench.py: for every world a context
per upload, all alternating, device events around `--steps` launches after `--warmup`, and a second context of
the first kind for the A/A spread.

Worlds:
  globe    a sphere that fills most of the frame over a plane under one light.  Uploads: the spherical map
           with a 256 x 256 and a 4096 x 4096 noise texture (the map build), the same tables with the planar
           map (the texture build), the planar map with a small spherically mapped sphere behind the camera
           (the same picture on the map build: the column that separates the maps' arithmetic from the
           difference between the builds), and a stripe pattern (the plain build);
  skybox   a cube of half side 12 that holds the camera and a light, a small sphere in it.  Uploads: a cube map
           of six noise textures, the planar map of one of them, the planar map on the map build, stripes.
Runs: frames and rt_trace_rays_device on the camera's own rays.  The figure of interest is what atan2 + acos
(the globe) and the face choice (the skybox) cost per patterned hit: (map - planar on the map build) / hits.

  python scripts/uv_map_bench.py --out profiles/uv_map.json
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
import rtc_amd  # noqa: E402
from rtc_amd import world as W  # noqa: E402


def noise(size, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(size, size, 3), dtype=np.uint8)


def behind_the_camera(image):
    """A small spherically mapped sphere no ray meets: its world runs the map build."""
    return W.sphere(W.Material(pattern=W.image_pattern(image, "bilinear", map="spherical")),
                    transform=W.mat_mul(W.translation(0.4, -40.0, -60.0), W.scaling(0.2, 0.2, 0.2)))


def globe(pattern, extra=()):
    cam = W.camera(B.WIDTH, B.HEIGHT, 0.9, (0.3, 1.2, -4.2), (0.0, 0.2, 0.0), (0.0, 1.0, 0.0))
    shapes = [W.plane(W.Material(color=(0.7, 0.7, 0.7), specular=0.0), transform=W.translation(0, -1.9, 0)),
              W.sphere(W.Material(pattern=pattern, specular=0.3), transform=W.mat_mul(W.translation(0.0, 0.2, 0.0), W.scaling(1.9, 1.9, 1.9)))]
    return W.World([W.Light((-5.0, 6.0, -5.0))], shapes + list(extra)).tables(cam)


def skybox(pattern, extra=()):
    cam = W.camera(B.WIDTH, B.HEIGHT, 1.2, (0.3, 0.5, -2.0), (0.0, 0.3, 1.0), (0.0, 1.0, 0.0))
    shapes = [W.cube(W.Material(pattern=pattern, specular=0.0, ambient=0.6), transform=W.scaling(12.0, 12.0, 12.0)),
              W.sphere(W.Material(color=(0.8, 0.3, 0.2)), transform=W.mat_mul(W.translation(0.0, 0.2, 2.0), W.scaling(0.6, 0.6, 0.6)))]
    return W.World([W.Light((-3.0, 5.0, -4.0))], shapes + list(extra)).tables(cam)


def measure(name, build, uploads, args):
    first = next(iter(uploads))
    uploads = dict(uploads)
    uploads[first + "_again"] = uploads[first]
    rays = B.camera_rays(uploads[first].camera)
    rec = {"world": name, "depth": 3, "ms": {}, "steps": {}, "upload_ms": {}, "map_info": {}, "frame_counts": {}}
    ctxs = {}
    for label, t in uploads.items():
        c = rtc_amd.Context(0)
        t0 = time.perf_counter()
        c.upload(t)
        rec["upload_ms"][label] = (time.perf_counter() - t0) * 1e3
        _, st = c.render(t.camera, 3, precision="f32")
        rec["frame_counts"][label] = {k: st[k] for k in ("primary", "shadow", "shaded", "lit_patterned")}
        rec["map_info"][label] = dict(c.map_info(), ran_textured=c.texture_info()["ran_textured"])
        ctxs[label] = c
    launches = {label: B.runs_for(c, uploads[label], 3, rays) for label, c in ctxs.items()}
    for run in ("frame", "rays"):
        for label in ctxs:
            ms, steps = B.timed(launches[label][run], args.steps, args.warmup, args.cell_ms)
            rec["ms"][f"{run}/{label}"] = ms
            rec["steps"][f"{run}/{label}"] = steps
        rec.setdefault("aa_spread", {})[run] = abs(rec["ms"][f"{run}/{first}"] - rec["ms"][f"{run}/{first}_again"]) / rec["ms"][f"{run}/{first}"]
        hits = rec["frame_counts"][first]["lit_patterned"]
        for size in args.size_list:
            a, b = rec["ms"].get(f"{run}/map_{size}"), rec["ms"].get(f"{run}/planar_{size}_map_build")
            if a is not None and b is not None:
                rec.setdefault("ns_per_patterned_hit_over_planar_on_the_map_build", {})[f"{run}/{size}"] = (a - b) * 1e6 / hits
    for c in ctxs.values():
        c.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_map.json"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cell-ms", type=float, default=1500.0, help="a cell's launches fit this, steps permitting")
    ap.add_argument("--sizes", default="256,4096")
    args = ap.parse_args()
    args.size_list = [int(s) for s in args.sizes.split(",") if s]
    a, b = (0.9, 0.3, 0.2), (0.2, 0.4, 0.8)
    records = []
    ups = {}
    for size in args.size_list:
        img = noise(size, size)
        ups[f"map_{size}"] = globe(W.image_pattern(img, "bilinear", map="spherical"))
        ups[f"planar_{size}"] = globe(W.image_pattern(img, "bilinear"))
        ups[f"planar_{size}_map_build"] = globe(W.image_pattern(img, "bilinear"), [behind_the_camera(noise(4, 1))])
    ups["stripes"] = globe(W.stripe_pattern(a, b).set_transformation(W.scaling(0.1, 1.0, 1.0)))
    records.append(measure("globe", globe, ups, args))
    ups = {}
    for size in args.size_list:
        faces = [noise(size, size + f) for f in range(6)]
        ups[f"map_{size}"] = skybox(W.cube_map_pattern(*faces, filter="bilinear"))
        ups[f"planar_{size}"] = skybox(W.image_pattern(faces[1], "bilinear").set_transformation(W.scaling(2.0, 2.0, 2.0)))
        ups[f"planar_{size}_map_build"] = skybox(W.image_pattern(faces[1], "bilinear").set_transformation(W.scaling(2.0, 2.0, 2.0)),
                                                 [behind_the_camera(noise(4, 1))])
    ups["stripes"] = skybox(W.stripe_pattern(a, b).set_transformation(W.scaling(0.1, 1.0, 1.0)))
    records.append(measure("skybox", skybox, ups, args))
    spreads = [r["aa_spread"][run] for r in records for run in ("frame", "rays")]
    out = {"what": "ms per launch, f32 1920x1080, bilinear filter; map_N = the spherical map (globe) or a cube map of six "
                   "textures (skybox) with N x N noise textures on the map build, planar_N = the same world under the planar map "
                   "(the texture build), planar_N_map_build = the planar map with a spherically mapped sphere no ray meets (the "
                   "map build), stripes = a stripe pattern (the plain build), *_again = a second context of the first kind (A/A)",
           "records": records, "aa_spread_max": max(spreads), "aa_spread_median": statistics.median(spreads)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
