"""GPU measurement behind tests/test_gpu_trace_rays.py's f32 floor: for the
eight random worlds of that test, the share of the 2048 non-unit rays
(|d| from U(0.5, 1.25)) whose f32 colour from Context.trace_rays lies within
(2/255) x max(1, |ref|inf) of the f64 oracle's, and the f64 path's largest
relative error on the U(0.25, 2) rays.  Writes profiles/ray_batch_parity.json
(or the path given as the first argument)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ray-tracer-challenge-rs_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import rtc_amd  # noqa: E402
import test_gpu_trace_rays as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ray_batch_parity.json")
    shares, worst32, err64, biggest = [], [], [], []
    with rtc_amd.Context(0) as ctx:
        for seed in T.SEEDS:
            shares.append(T.f32_share(ctx, seed))
            got, _ = ctx.trace_rays(T._rays(seed, T.NARROW), 6, precision="f32")
            worst32.append(float(T._rel_err(got, T._oracle(seed, T.NARROW)[0]).max()))
            got, _ = ctx.trace_rays(T._rays(seed, T.WIDE), 6, precision="f64")
            ref = T._oracle(seed, T.WIDE)[0]
            err64.append(float(T._rel_err(got, ref).max()))
            biggest.append(float(np.abs(ref).max()))
    rec = {"what": "Context.trace_rays against the f64 oracle, random worlds of tests/test_gpu_trace_rays.py, "
                   "2048 rays each, depth 6",
           "seeds": T.SEEDS,
           "f32_direction_scale": list(T.NARROW),
           "criterion": "|got - ref|inf <= (2/255) x max(1, |ref|inf)",
           "share_within_2_255": shares,
           "min_share": min(shares),
           "f32_max_relative_error": worst32,
           "f64_direction_scale": list(T.WIDE),
           "f64_max_relative_error": err64,
           "f64_largest_reference_value": biggest}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
