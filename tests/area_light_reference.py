"""Area lights in numpy (include/rtc.h "Area lights"): the jitter hash, the jitter
and the sample positions, restated from the header's text for the tests to
compare the library against.  Everything is f64 and vectorised over rays.
"""
import numpy as np

U32 = np.uint32


def mix(x):
    """mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16, on uint32."""
    x = np.asarray(x).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    x = x ^ (x >> np.uint64(16))
    return x  # uint64 holding a uint32 value (numpy's uint32 products would warn on wraparound)


def jitter(seed, ray_id, remaining, area_index, k):
    """(ju, jv) of sample k for the given rays: multiples of 2^-24 in [0, 1)."""
    u = lambda v: np.asarray(v).astype(np.uint64) & np.uint64(0xFFFFFFFF)  # noqa: E731
    key = mix(mix(mix(u(seed) ^ u(ray_id)) ^ u(remaining)) ^ (((u(area_index) << np.uint64(8)) & np.uint64(0xFFFFFFFF)) | u(k)))
    ju = (key >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    jv = (mix(key ^ np.uint64(0x9E3779B9)) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return ju, jv


def position(light, area_index, ray_id, remaining, k):
    """Sample k of `light` (anything with corner, full_uvec, full_vvec, usteps, vsteps, jitter, seed) for each
    ray: (n, 3) f64.  pos = (corner + uvec * (i + ju)) + vvec * (j + jv), left to right."""
    ray_id = np.atleast_1d(np.asarray(ray_id))
    us, vs = int(light.usteps), int(light.vsteps)
    i, j = k % us, k // us
    if int(light.jitter):
        ju, jv = jitter(int(light.seed), ray_id, remaining, area_index, k)
    else:
        ju = jv = np.full(ray_id.shape, 0.5)
    out = np.empty(ray_id.shape + (3,), dtype=np.float64)
    for c in range(3):
        uvec = np.float64(light.full_uvec[c]) / np.float64(us)
        vvec = np.float64(light.full_vvec[c]) / np.float64(vs)
        out[..., c] = (np.float64(light.corner[c]) + uvec * (np.float64(i) + ju)) + vvec * (np.float64(j) + jv)
    return out

