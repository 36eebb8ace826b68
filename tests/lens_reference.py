"""The lens ray of include/rtc.h ("Thin-lens camera"), restated in numpy: f64, both jitter modes.

Written from the header's text, formula by formula, and vectorized over a whole frame.  numpy's f64
multiplies, adds, divisions and square roots are IEEE operations and nothing here fuses, so the rays equal
rt_lens_ray's and the f64 kernels' bit for bit.  Hash arithmetic is uint32 with wraparound (numpy arrays
wrap silently).
"""
import numpy as np

LENS_KEY = 0x4C454E53
U32 = np.uint32


def mix(x):
    """rtc.h "Hashed jitter": x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16."""
    x = np.asarray(x, dtype=U32).copy()
    x ^= x >> U32(16)
    x *= U32(0x7FEB352D)
    x ^= x >> U32(15)
    x *= U32(0x846CA68B)
    x ^= x >> U32(16)
    return x


def lens_cells(w, h, n, x, y, i, j, jitter, seed):
    """(ci, cj, ju, jv) of samples (i, j) of pixels (x, y) of a W x H frame (arrays of one shape; y the image row)."""
    x, y, i, j = (np.asarray(v, dtype=U32) for v in (x, y, i, j))
    if not jitter:
        half = np.full(x.shape, 0.5)
        return i.astype(np.float64), j.astype(np.float64), half, half
    n32, w32 = U32(n), U32(w)
    lk = mix(U32(seed) ^ U32(LENS_KEY))
    ray_id = (n32 * y + j) * (n32 * w32) + n32 * x + i
    key = mix(lk ^ ray_id)
    ju = (key >> U32(8)).astype(np.float64) * 2.0 ** -24
    jv = (mix(key ^ U32(0x9E3779B9)) >> U32(8)).astype(np.float64) * 2.0 ** -24
    r = mix(lk ^ mix(y * w32 + x)) % U32(n * n)
    k = (j * n32 + i + r) % U32(n * n)
    return (k % n32).astype(np.float64), (k // n32).astype(np.float64), ju, jv


def _point(inv, px, py, pz):
    """inverse * (px, py, pz, 1): each row the left fold (((0 + m0 x) + m1 y) + m2 z) + m3."""
    m = [float(v) for v in inv]
    return [(((0.0 + m[4 * r] * px) + m[4 * r + 1] * py) + m[4 * r + 2] * pz) + m[4 * r + 3] for r in range(3)]


def lens_rays(cn, w, h, n, aperture, focal, jitter=False, seed=0, x=None, y=None, i=None, j=None):
    """Rays (..., 6) = origin, direction.  `cn` is the SAMPLE camera (the output camera resized to n W x n H).
    Without x, y, i, j: the whole frame, shape (H, W, n, n, 6), indexed [y, x, j, i]."""
    if x is None:
        y, x, j, i = np.meshgrid(np.arange(h), np.arange(w), np.arange(n), np.arange(n), indexing="ij")
    x, y, i, j = (np.asarray(v, dtype=U32) for v in (x, y, i, j))
    px = (U32(n) * x + i).astype(np.float64)
    py = (U32(n) * y + j).astype(np.float64)
    wx = cn.half_width - (px + 0.5) * cn.pixel_size
    wy = cn.half_height - (py + 0.5) * cn.pixel_size
    ci, cj, ju, jv = lens_cells(w, h, n, x, y, i, j, jitter, seed)
    inv_n = 1.0 / float(n)
    a = 2.0 * ((ci + ju) * inv_n) - 1.0
    b = 2.0 * ((cj + jv) * inv_n) - 1.0
    ex = a * np.sqrt(1.0 - (b * b) * 0.5)
    ey = b * np.sqrt(1.0 - (a * a) * 0.5)
    f = float(focal)
    origin = _point(cn.inverse, aperture * ex, aperture * ey, np.zeros_like(ex))
    target = _point(cn.inverse, wx * f, wy * f, np.full_like(wx, -f))
    d = [t - o for t, o in zip(target, origin)]
    mag = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return np.stack(origin + [c / mag for c in d], axis=-1)


def ordered_mean(cols, h, w, n):
    """Colours (H W n n, 3) in ray order [y, x, j, i] to the frame: summed j outer and i inner, times 1 / n^2."""
    cols = np.asarray(cols, dtype=np.float64).reshape(h, w, n, n, 3)
    acc = np.zeros((h, w, 3), dtype=np.float64)
    for j in range(n):
        for i in range(n):
            acc = acc + cols[:, :, j, i]
    return acc * (1.0 / (n * n))


def traced_lens_frame(trace, tables, cn, w, h, n, aperture, focal, jitter, seed, tolerance, chunk=1024):
    """The lens frame of a numpy reference (smooth_reference.trace or texture_reference.trace: colours, hits
    and a decision margin per ray) over the lens rays, `chunk` rays at a time (every ray is traced on its own,
    so the chunks change no value).  Returns (frame (H, W, 3), sound (H, W): every one of the pixel's n^2 rays
    has a margin above `tolerance`, counts: the primary rays, the hits and the shadow rays, one per hit and
    light)."""
    from concurrent.futures import ThreadPoolExecutor
    rays = np.ascontiguousarray(lens_rays(cn, w, h, n, aperture, focal, jitter, seed).reshape(-1, 6))
    cols, margin, hits = np.zeros((len(rays), 3)), np.zeros(len(rays)), 0
    starts = range(0, len(rays), chunk)
    with ThreadPoolExecutor(max_workers=8) as pool:  # (numpy releases the interpreter lock in its loops)
        for a, (rgb, hit, m) in zip(starts, pool.map(lambda a: trace(tables, rays[a:a + chunk]), starts)):
            cols[a:a + chunk], margin[a:a + chunk] = rgb, m
            hits += int((hit["shape"] >= 0).sum())
    sound = (margin.reshape(h, w, n * n) > tolerance).all(axis=2)
    counts = {"primary": len(rays), "shaded": hits, "shadow": hits * len(tables.lights)}
    return ordered_mean(cols, h, w, n), sound, counts


def lens_frame(oracle, tables, cn, w, h, n, aperture, focal, jitter, seed, depth):
    """The oracle's lens frame: World::color_at over the rays, summed j outer and i inner, times 1 / n^2.
    Returns (frame (H, W, 3) f64, the oracle's stats of the whole ray set)."""
    rays = lens_rays(cn, w, h, n, aperture, focal, jitter, seed)
    cols, st = oracle.color_at(tables, np.ascontiguousarray(rays.reshape(-1, 6)), depth)
    cols = np.asarray(cols, dtype=np.float64).reshape(h, w, n, n, 3)
    acc = np.zeros((h, w, 3), dtype=np.float64)
    for j in range(n):
        for i in range(n):
            acc = acc + cols[:, :, j, i]
    return acc * (1.0 / (n * n)), st
