"""f32 mesh frames and rays against the f64 oracle (GPU): the figures the
floors of tests/test_gpu_mesh.py come from.

For every world of tests/mesh_worlds.py WORLDS the share of the 80 x 60 f32
frame's pixels within 2/255 of oracle.render, and for the incoherent-ray
worlds the share of 2048 seeded rays within 2/255 of oracle.color_at.  The
record holds every figure and the two minima; the tests' floors are the
minima less 0.005.

  python scripts/mesh_parity.py --out profiles/mesh_parity.json
"""
import argparse
import json
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ray-tracer-challenge-rs_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import mesh_worlds as M  # noqa: E402
import pyoracle  # noqa: E402
import rtc_amd  # noqa: E402

RAY_WORLDS = ("ico3", "glass")  # tests/test_gpu_mesh.py test_incoherent_rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_parity.json"))
    args = ap.parse_args()
    tmp = pathlib.Path(tempfile.mkdtemp())
    frames, rays = {}, {}
    with rtc_amd.Context(0) as ctx:
        for key in M.WORLDS:
            tables, depth = M.build_world(rtc_amd, tmp, key)
            ref, _ = pyoracle.render(tables, tables.camera, depth, threads=8)
            ctx.upload(tables)
            img, _ = ctx.render(tables.camera, depth, precision="f32")
            frames[key] = M.share_within(img.astype(np.float64), ref)
            differ = np.argwhere(np.abs(img - ref).max(axis=2) > 2.0 / 255.0)
            print(f"{key}: frame {frames[key]:.5f} ({len(differ)} px differ), tree {ctx.tree_info()}", flush=True)
            if key in RAY_WORLDS:
                r = M.random_rays(2048, 1234)
                want, _ = pyoracle.color_at(tables, r, depth)
                got, _ = ctx.trace_rays(r, depth, precision="f32")
                rays[key] = M.share_within(got, want)
                print(f"{key}: rays {rays[key]:.5f}", flush=True)
    record = {"criterion": "share of pixels (rays) with every channel within 2/255 of the f64 oracle",
              "frame": list(M.FRAME), "frames": frames, "rays": rays,
              "frames_min": min(frames.values()), "rays_min": min(rays.values())}
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
