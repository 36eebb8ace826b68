"""f32 against the f64 device frames for the worlds with area lights (GPU): the share of frame pixels within
2/255, for the area upload and for its expansion uploaded through the older entry points; the expansion's
shares less 0.0005 are tests/f32_tolerance_area.py's floors.

  python scripts/area_light_parity.py --out profiles/area_light_parity.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ray-tracer-challenge-rs_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import rtc_amd  # noqa: E402
import test_gpu_area_lights as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "area_light_parity.json"))
    args = ap.parse_args()
    with rtc_amd.Context(0) as ctx:
        shares = T.f32_parity(ctx)
    out = {"what": "share of f32 frame pixels within 2/255 of the f64 device frame of the same upload, 64 x 32: the "
                   "area upload and its expansion through the older entry points (tests/test_gpu_area_lights.py "
                   "f32_parity)",
           "worlds": {k: {"area": a, "expansion": e} for k, (a, e) in shares.items()},
           "margin": T.F32A.MARGIN}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
