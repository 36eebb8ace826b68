"""Textured against untextured uploads of the same mesh (GPU; not bench.py, no gate).
One process, one GPU, f32 at 1920 x 1080: for every world a context per texture
size (256 x 256: 256 KB of texels; 4096 x 4096: 64 MB, well beyond an XCD's
4 MiB L2) and filter (nearest: one dword per lane and shaded hit; bilinear:
four), a second context of the first kind for the A/A spread, and one with the
same tables without coordinates, textures and image pattern (the upload the
world ran before: the plain build where it has no instances) alternate; for
worlds without instances one more context holds those untextured tables with one
triangle named smooth with its own face normal three times (the same picture,
sent through the instance build: the column that separates the texture work
from the difference between the builds).  Device
events around `--steps` launches after `--warmup`, in the style of
scripts/smooth_bench.py.

Worlds: icospheres of 1280 and 20 480 triangles with a coordinate per vertex,
opaque (direct kernel) and glass at depth 4 (pool kernel), over a plane under
one light; and the 5 x 5 x 5 grid of 576-triangle tori as 125 instances of one
textured mesh, opaque.  Runs: frames, rt_trace_rays_device on the camera's own
rays, the host's upload time, and the device bytes of the coordinate tables and
the texels.

  python scripts/texture_bench.py --out profiles/texture.json
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
import smooth_bench as SB  # noqa: E402
import smooth_worlds as S  # noqa: E402
import texture_worlds as X  # noqa: E402
from rtc_amd import world as W  # noqa: E402


def noise(size, seed):
    """A size x size texture without structure: neighbouring lanes' texels share cache lines only by position."""
    return np.random.default_rng(seed).integers(0, 256, size=(size, size, 3), dtype=np.uint8)


def with_pattern(material, image, filt):
    material.pattern = W.image_pattern(image, filt)
    return material


def ico_world(subdivisions, material):
    lights, shapes = SB.floor_and_light()
    verts, faces = M.icosphere(subdivisions)
    mesh = X.load(rtc_amd, verts, faces, X.ico_coords(verts))
    return W.World(lights, shapes + W.mesh(mesh, material, textured=True)).tables(SB.camera())


def tori_world(material):
    lights, shapes = SB.floor_and_light()
    verts, faces = M.torus(24, 12)
    ang = np.arctan2(verts[:, 2], verts[:, 0]) / (2 * np.pi) + 0.5
    tube = np.arctan2(verts[:, 1], np.hypot(verts[:, 0], verts[:, 2]) - 1.0) / (2 * np.pi) + 0.5
    mesh = X.load(rtc_amd, verts, faces, np.stack([ang, tube], axis=1))
    place = [W.mat_mul(W.translation(0.9 * (i - 2), 0.9 * (j - 2) + 0.6, 0.9 * (k - 2) + 1.0), W.scaling(0.3, 0.3, 0.3))
             for i in range(5) for j in range(5) for k in range(5)]
    return W.World(lights, shapes, [W.instance(mesh, material, transform=t, textured=True) for t in place]).tables(SB.camera())


def through_the_instance_build(tables):
    """The same untextured tables with the first triangle named smooth with its face normal at every vertex: the
    same picture, run by the instance build (rt_scene_upload_smooth) instead of the plain one."""
    k = next(i for i, s in enumerate(tables.shapes) if s.kind == 5)
    e = rtc_amd.SmoothDesc(rtc_amd.RT_SMOOTH_SHAPES, k)
    e.normal_1[:] = e.normal_2[:] = e.normal_3[:] = list(tables.shapes[k].normal)
    return rtc_amd.SceneTables(tables.shapes, tables.materials, tables.patterns, tables.lights, tables.camera,
                               smooth=(rtc_amd.SmoothDesc * 1)(e))


def measure(name, build, material, depth, images, args):
    uploads = {}
    for size, image in images.items():
        for filt in ("nearest", "bilinear"):
            uploads[f"{size}_{filt}"] = build(with_pattern(material(), image, filt))
    first = next(iter(uploads))
    uploads[first + "_again"] = uploads[first]
    uploads["plain"] = X.without_textures(rtc_amd, uploads[first])
    if not uploads["plain"].instanced:
        uploads["plain_instance_build"] = through_the_instance_build(uploads["plain"])
    rays = B.camera_rays(uploads[first].camera)
    rec = {"world": name, "depth": depth, "ms": {}, "steps": {}, "upload_ms": {}, "texture_info": {}}
    ctxs = {}
    for label, t in uploads.items():
        c = rtc_amd.Context(0)
        t0 = time.perf_counter()
        c.upload(t)
        rec["upload_ms"][label] = (time.perf_counter() - t0) * 1e3
        rec["texture_info"][label] = c.texture_info()
        ctxs[label] = c
    rec["instance_info"] = {k: v for k, v in ctxs[first].instance_info().items() if k != "build_ms"}
    rec["tree"] = ctxs[first].tree_info()
    rec["frame_counts"] = {}
    for label in (first, "plain"):
        _, st = ctxs[label].render(uploads[label].camera, depth, precision="f32")
        rec["frame_counts"][label] = {k: st[k] for k in ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned")}
    launches = {label: B.runs_for(c, uploads[label], depth, rays) for label, c in ctxs.items()}
    for run in ("frame", "rays"):
        for label in ctxs:
            ms, steps = B.timed(launches[label][run], args.steps, args.warmup, args.cell_ms)
            rec["ms"][f"{run}/{label}"] = ms
            rec["steps"][f"{run}/{label}"] = steps
        base = "plain_instance_build" if "plain_instance_build" in uploads else "plain"
        for label in uploads:
            if label != "plain":
                rec.setdefault("over_plain", {})[f"{run}/{label}"] = rec["ms"][f"{run}/{label}"] / rec["ms"][f"{run}/plain"]
            if not label.startswith("plain"):  # against the untextured world on the build the textured one extends
                rec.setdefault("over_instance_build", {})[f"{run}/{label}"] = rec["ms"][f"{run}/{label}"] / rec["ms"][f"{run}/{base}"]
        rec.setdefault("aa_spread", {})[run] = abs(rec["ms"][f"{run}/{first}"] - rec["ms"][f"{run}/{first}_again"]) / \
            rec["ms"][f"{run}/{first}"]
    for c in ctxs.values():
        c.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture.json"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cell-ms", type=float, default=1500.0, help="a cell's launches fit this, steps permitting")
    ap.add_argument("--subdivisions", default="3,5")
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--no-grid", action="store_true")
    args = ap.parse_args()
    images = {f"tex{s}": noise(int(s), int(s)) for s in args.sizes.split(",") if s}
    records = []
    for s in [int(v) for v in args.subdivisions.split(",") if v]:
        records.append(measure(f"ico{s}_opaque", lambda m, s=s: ico_world(s, m), S.opaque, 3, images, args))
        records.append(measure(f"ico{s}_glass", lambda m, s=s: ico_world(s, m), M.glass, 4, images, args))
    if not args.no_grid:
        records.append(measure("tori_5x5x5_instanced", tori_world, S.opaque, 3, images, args))
    spreads = [r["aa_spread"][run] for r in records for run in ("frame", "rays")]
    out = {"what": "ms per launch, f32 1920x1080; texN_filter = rt_scene_upload_textured with an N x N noise texture, "
                   "plain = the same tables without coordinates, textures and image pattern, *_again = a second "
                   "context of the first kind (A/A), plain_instance_build = plain with one triangle named smooth with its "
                   "own face normal (the same picture through the instance build; worlds without instances only)",
           "records": records, "aa_spread_max": max(spreads), "aa_spread_median": statistics.median(spreads)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
