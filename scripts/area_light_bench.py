"""Area lights against their own expansions (GPU; not bench.py, no gate).  One process, one
GPU, f32 at 1920 x 1080.  For every world and light size (2 x 2, 4 x 4, 8 x 8 samples) these
contexts alternate, so every comparison is made on the same machine in the same call:

  area                  rt_scene_upload_lit, cell centres (the light-level caster cull on)
  area_again            a second context of the same kind: the A/A spread
  area_jitter           the same light with hashed jitter
  area_nocull           RTC_DEBUG=area_cull=0: every sample culls for itself
  expansion_generic     rt_lights_expand's point lights through the older entry point, per-scene
                        builds off: what the parent commit's generic kernels run
  expansion_per_scene   the same upload with the per-scene build (RT_JIT_EAGER, waited for up to
                        --jit-wait-ms); `per_scene_used` says whether the timed frames ran it (worlds
                        with instances have none)
The expansion keeps the world's instances: only the light list is expanded.

Worlds: a floor with a sphere, a cube and a cylinder, opaque (direct kernel) and with a mirror
floor and a glass sphere at depth 4 (pool kernel); cover's shapes (tests/golden/scenes/cover.json)
under one area light where its brightest light is; the 5 x 5 x 5 grid of 576-triangle tori as
125 instances.  Runs: frames, and rt_trace_rays_device on the camera's own rays.  Device events
around `--steps` launches after `--warmup` (scripts/mesh_bench.py timed).  Before timing, the
area frame is compared with the expansion's (the share of pixels within 2/255).

  python scripts/area_light_bench.py --out profiles/area_lights.json
"""
import argparse
import dataclasses
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
from rtc_amd import scene_io  # noqa: E402
from rtc_amd import world as W  # noqa: E402


def light(n, jitter=False, corner=(-1.5, 5.0, -4.0), u=(2.0, 0.0, 0.0), v=(0.0, 0.0, 2.0), intensity=(1.0, 1.0, 1.0)):
    return W.AreaLight(corner, u, v, n, n, intensity, jitter, 17)


def casters(mirror):
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.35, 0.35, 0.4)), specular=0.0,
                               reflectiveness=0.4 if mirror else 0.0), transform=W.translation(0, -1.3, 0))
    ball = W.sphere(M.glass() if mirror else W.Material(color=(0.9, 0.3, 0.25), specular=0.6, shininess=40.0),
                    transform=W.mat_mul(W.translation(-0.9, -0.3, 0.2), W.scaling(0.8, 0.8, 0.8)))
    box = W.cube(W.Material(color=(0.3, 0.5, 0.9), specular=0.3, shininess=20.0),
                 transform=W.mat_mul(W.translation(1.2, -0.8, 0.6), W.mat_mul(W.rotation_y(0.6), W.scaling(0.5, 0.5, 0.5))))
    rod = W.cylinder(-1.0, 1.0, True, W.Material(color=(0.4, 0.8, 0.4)),
                     W.mat_mul(W.translation(0.3, -0.3, 1.8), W.scaling(0.3, 1.0, 0.3)))
    return [floor, ball, box, rod]


def casters_world(mirror, n, jitter):
    return W.World([], casters(mirror), area_lights=[light(n, jitter)]).tables(SB.camera())


def cover_world(n, jitter):
    scene = scene_io.load(os.path.join(ROOT, "tests", "golden", "scenes", "cover.json"))
    cam = rtc_amd.camera_resize(scene.camera, B.WIDTH, B.HEIGHT)
    main = max(scene.lights, key=lambda lt: max(lt.intensity))
    total = tuple(sum(lt.intensity[c] for lt in scene.lights) for c in range(3))
    a = light(n, jitter, corner=(main.position[0] - 1.0, main.position[1], main.position[2] - 1.0), intensity=total)
    none = (rtc_amd.LightDesc * 0)()
    return dataclasses.replace(scene, lights=none, camera=cam, area_lights=(rtc_amd.AreaLightDesc * 1)(a.desc()))


def tori_world(n, jitter):
    _, shapes = SB.floor_and_light()
    mesh = rtc_amd.load_obj(M.obj_text(*M.torus(24, 12)))
    place = [W.mat_mul(W.translation(0.9 * (i - 2), 0.9 * (j - 2) + 0.6, 0.9 * (k - 2) + 1.0), W.scaling(0.3, 0.3, 0.3))
             for i in range(5) for j in range(5) for k in range(5)]
    return W.World([], shapes, [W.instance(mesh, S.opaque(), transform=t) for t in place],
                   area_lights=[light(n, jitter, corner=(-5.0, 6.0, -6.0))]).tables(SB.camera())


COUNTS = ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned")


def measure(name, build, depth, n, args):
    lit, jittered = build(n, False), build(n, True)
    # (the light list alone is expanded: an instanced world stays instanced, as its user uploads it today)
    flat = dataclasses.replace(lit, lights=lit.expanded_lights(), area_lights=None)
    uploads = {"area": (lit, ""), "area_again": (lit, ""), "area_jitter": (jittered, ""), "area_nocull": (lit, "area_cull=0"),
               "expansion_generic": (flat, ""), "expansion_per_scene": (flat, "")}
    rays = B.camera_rays(lit.camera)
    rec = {"world": name, "depth": depth, "light": f"{n}x{n}", "samples": n * n, "ms": {}, "steps": {}, "upload_ms": {}}
    ctxs = {}
    for label, (t, knobs) in uploads.items():
        c = B.context(knobs)
        c.set_jit(rtc_amd.RT_JIT_EAGER if label == "expansion_per_scene" and not args.no_per_scene else rtc_amd.RT_JIT_OFF)
        t0 = time.perf_counter()
        c.upload(t)
        rec["upload_ms"][label] = (time.perf_counter() - t0) * 1e3
        ctxs[label] = c
    rec["light_info"] = ctxs["area"].light_info()
    # results first (faster and different is not faster): the area frame against the expansion's
    a, sa = ctxs["area"].render(lit.camera, depth, precision="f32")
    e, se = ctxs["expansion_generic"].render(lit.camera, depth, precision="f32")
    rec["frame_counts"] = {"area": {k: sa[k] for k in COUNTS}, "expansion": {k: se[k] for k in COUNTS}}
    rec["share_within_2_255_of_the_expansion"] = M.share_within(a.astype(np.float64), e.astype(np.float64))
    rec["max_abs_diff_to_the_expansion"] = float(np.abs(a.astype(np.float64) - e).max())
    launches = {label: B.runs_for(c, uploads[label][0], depth, rays) for label, c in ctxs.items()}
    ps = ctxs["expansion_per_scene"]
    t0 = time.perf_counter()
    launches["expansion_per_scene"]["frame"]()  # (EAGER: the first large frame starts the build)
    pending = ps.jit_wait(args.jit_wait_ms)
    rec["per_scene_build_wait_ms"] = (time.perf_counter() - t0) * 1e3
    launches["expansion_per_scene"]["frame"]()
    import torch
    torch.cuda.synchronize()
    js = ps.jit_status()
    rec["per_scene_used"] = bool(js["used"])
    rec["per_scene_note"] = ("build still running after the wait" if pending else js["log"][:160])
    for run in ("frame", "rays"):
        for label in ctxs:
            ms, steps = B.timed(launches[label][run], args.steps, args.warmup, args.cell_ms)
            rec["ms"][f"{run}/{label}"] = ms
            rec["steps"][f"{run}/{label}"] = steps
        area = rec["ms"][f"{run}/area"]
        rec.setdefault("area_over_expansion_generic", {})[run] = area / rec["ms"][f"{run}/expansion_generic"]
        rec.setdefault("area_over_expansion_per_scene", {})[run] = area / rec["ms"][f"{run}/expansion_per_scene"]
        rec.setdefault("jitter_over_area", {})[run] = rec["ms"][f"{run}/area_jitter"] / area
        rec.setdefault("nocull_over_area", {})[run] = rec["ms"][f"{run}/area_nocull"] / area
        rec.setdefault("aa_spread", {})[run] = abs(area - rec["ms"][f"{run}/area_again"]) / area
    if pending:
        ps.jit_wait(120000.0)  # (leave no build running behind the next cell's timings)
    for c in ctxs.values():
        c.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "area_lights.json"))
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--cell-ms", type=float, default=600.0, help="a cell's launches fit this, steps permitting")
    ap.add_argument("--jit-wait-ms", type=float, default=60000.0)
    ap.add_argument("--no-per-scene", action="store_true", help="no per-scene build (an A/B of the area build alone)")
    ap.add_argument("--sizes", default="2,4,8")
    ap.add_argument("--worlds", default="casters,casters_mirror,cover,tori")
    args = ap.parse_args()
    worlds = {"casters": (lambda n, j: casters_world(False, n, j), 0),
              "casters_mirror": (lambda n, j: casters_world(True, n, j), 4),
              "cover": (cover_world, 6), "tori": (tori_world, 0)}
    records = []
    for name in [w for w in args.worlds.split(",") if w]:
        for n in [int(v) for v in args.sizes.split(",") if v]:
            records.append(measure(name, worlds[name][0], worlds[name][1], n, args))
            out = {"what": "ms per launch, f32 1920x1080; labels in scripts/area_light_bench.py's docstring; ratios "
                           "below 1 mean the numerator is faster",
                   "records": records,
                   "aa_spread_max": max(r["aa_spread"][run] for r in records for run in ("frame", "rays")),
                   "aa_spread_median": statistics.median(r["aa_spread"][run] for r in records for run in ("frame", "rays"))}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:  # (rewritten after every cell: a cut-off run keeps what it measured)
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
