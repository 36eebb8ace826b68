"""f32 against the f64 device results for the textured worlds (GPU): the shares of
frame pixels and of random rays within 2/255 that tests/test_gpu_texture.py's
floors are set from (DESIGN.md §3.7's rule: the observed minimum less 0.005).

  python scripts/texture_parity.py --out profiles/texture_parity.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ray-tracer-challenge-rs_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import rtc_amd  # noqa: E402
import test_gpu_texture as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_parity.json"))
    args = ap.parse_args()
    with rtc_amd.Context(0) as ctx:
        shares = T.f32_parity(ctx, rtc_amd)
    out = {"what": "share of f32 results within 2/255 of the f64 device results of the same upload, 80x60 frames "
                   "and 4096 random rays (tests/test_gpu_texture.py f32_parity)",
           "worlds": {k: {"pixels": p, "rays": r} for k, (p, r) in shares.items()},
           "min_pixels": min(p for p, _ in shares.values()), "min_rays": min(r for _, r in shares.values()),
           "floors_in_the_test": {"pixels": T.F32_FLOOR_PIXELS, "rays": T.F32_FLOOR_RAYS}}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
