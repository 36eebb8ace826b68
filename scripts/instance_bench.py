"""Instanced worlds against their expansions (GPU; not bench.py, no gate).
One process, one GPU, f32 at 1920 x 1080: for every world a context with the
instanced upload (rt_scene_upload_instanced), a second one
like it (the A/A column) and one with the expansion uploaded through
rt_scene_upload alternate, device events around `--steps` launches after
`--warmup` as in scripts/mesh_bench.py (whose helpers this uses).

Worlds, each opaque (direct kernel, depth 3) and glass (pool kernel and the
containers walk, depth 4), over a plane under one light:
  tori_125      one 576-triangle torus placed 5 x 5 x 5 times
  ico5_27       27 icospheres of 20 480 triangles, 3 x 3 x 3
  ico3_1000     1000 icospheres of 1280 triangles, 10 x 10 x 10
Reported per world: ms per frame and per batch of the camera's own 2 M rays,
upload ms, and the device bytes of rt_scene_instance_info.

  python scripts/instance_bench.py --out profiles/instances.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import mesh_bench as B  # noqa: E402  (puts the package and tests/ on the path)
import mesh_worlds as M  # noqa: E402
import rtc_amd  # noqa: E402
from rtc_amd import world as W  # noqa: E402


def grid(n, pitch, scale, lift):
    half = (n - 1) / 2.0
    return [W.mat_mul(W.translation(pitch * (i - half), pitch * (j - half) + lift, pitch * (k - half) + 1.0),
                      W.scaling(scale, scale, scale)) for i in range(n) for j in range(n) for k in range(n)]


def tables_of(mesh, material, places):
    floor = W.plane(W.Material(color=(0.7, 0.7, 0.7), specular=0.0), transform=W.translation(0, -1.3, 0))
    cam = W.camera(B.WIDTH, B.HEIGHT, 0.9, (0.3, 1.7, -4.2), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0))
    return W.World([W.Light((-5.0, 6.0, -5.0))], [floor], [W.instance(mesh, material, p) for p in places]).tables(cam)


def measure(name, tables, depth, args):
    rays = B.camera_rays(tables.camera)
    t0 = time.perf_counter()
    flat = tables.expanded()
    expand_ms = (time.perf_counter() - t0) * 1e3
    rec = {"world": name, "instances": len(tables.instances), "triangles": len(flat.shapes) - len(tables.shapes),
           "depth": depth, "expand_ms": expand_ms, "ms": {}, "steps": {}, "upload_ms": {}, "info": None}
    ctxs = {}
    for label, t in (("instanced", tables), ("instanced_again", tables), ("expanded", flat)):
        c = rtc_amd.Context(0)
        t0 = time.perf_counter()
        c.upload(t)
        rec["upload_ms"][label] = (time.perf_counter() - t0) * 1e3
        if label == "instanced":
            rec["info"] = c.instance_info()
        if label == "expanded":
            rec["tree"] = c.tree_info()
        ctxs[label] = c
    launches = {label: B.runs_for(c, tables, depth, rays) for label, c in ctxs.items()}
    for run in ("frame", "rays"):
        for label in ctxs:
            ms, steps = B.timed(launches[label][run], args.steps, args.warmup, args.cell_ms)
            rec["ms"][f"{run}/{label}"] = ms
            rec["steps"][f"{run}/{label}"] = steps
    for c in ctxs.values():
        c.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instances.json"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cell-ms", type=float, default=1500.0, help="a cell's launches fit this, steps permitting")
    ap.add_argument("--worlds", default="tori_125,ico5_27,ico3_1000")
    ap.add_argument("--materials", default="opaque,glass")
    args = ap.parse_args()
    opaque = W.Material(color=(0.25, 0.6, 0.85), specular=0.5, shininess=60.0)
    worlds = {"tori_125": (lambda: B.mesh_of(*M.torus(24, 12)), grid(5, 0.9, 0.3, 0.6)),
              "ico5_27": (lambda: B.mesh_of(*M.icosphere(5)), grid(3, 1.5, 0.6, 0.6)),
              "ico3_1000": (lambda: B.mesh_of(*M.icosphere(3)), grid(10, 0.45, 0.18, 0.8))}
    records = []
    for name in [w for w in args.worlds.split(",") if w]:
        make, places = worlds[name]
        mesh = make()
        if "opaque" in args.materials.split(","):
            records.append(measure(f"{name}_opaque", tables_of(mesh, opaque, places), 3, args))
        if "glass" in args.materials.split(","):
            records.append(measure(f"{name}_glass", tables_of(mesh, M.glass(), places), 4, args))
    spreads = [abs(r["ms"][f"{run}/instanced"] - r["ms"][f"{run}/instanced_again"]) / r["ms"][f"{run}/instanced"]
               for r in records for run in ("frame", "rays")]
    out = {"what": "ms per launch, f32 1920x1080; instanced = rt_scene_upload_instanced, expanded = the same world "
                   "written out and uploaded through rt_scene_upload", "records": records}
    if spreads:
        out["aa_spread_max"] = max(spreads)
        out["aa_spread_median"] = statistics.median(spreads)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
