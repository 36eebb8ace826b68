"""The shutter time of include/rtc.h ("Motion blur"), restated in numpy, and the oracle over (ray, time) pairs.

Written from the header's text, formula by formula, vectorized over a whole frame: f64, both jitter modes.
numpy's f64 multiplies and adds are IEEE operations and nothing here fuses, so the times equal
rt_shutter_time's and the f64 kernels' bit for bit.  The sample rays and the ordered mean are
tests/lens_reference.py's (the pinhole's sample rays are its lens rays of aperture 0 and focal distance 1:
the lens point is the camera's origin and the focal point the pixel's point on the canvas).

The reference has no motion.  A ray of time tau in a moving world is that ray in the static world whose
movers are displaced by v tau, `scene.at_time(tau)` (rt_motion_displace): trace() groups the rays by their
time and asks the oracle once per distinct world.
"""
import numpy as np

from lens_reference import U32, lens_rays, mix, ordered_mean  # noqa: F401  (re-exported for the tests)

SHUTTER_KEY = 0x54494D45


def shutter_times(w, h, n, open_, close, jitter=False, seed=0, x=None, y=None, i=None, j=None):
    """tau of samples (i, j) of pixels (x, y) of a W x H frame (y the image row).  Without x, y, i, j: the
    whole frame, shape (H, W, n, n), indexed [y, x, j, i]."""
    if x is None:
        y, x, j, i = np.meshgrid(np.arange(h), np.arange(w), np.arange(n), np.arange(n), indexing="ij")
    x, y, i, j = (np.asarray(v, dtype=U32) for v in (x, y, i, j))
    n32, w32, n2 = U32(n), U32(w), U32(n * n)
    c = j * n32 + i
    jt = np.full(x.shape, 0.5)
    if jitter:
        tk = mix(U32(seed) ^ U32(SHUTTER_KEY))
        ray_id = (n32 * y + j) * (n32 * w32) + n32 * x + i
        key = mix(tk ^ ray_id)
        jt = (key >> U32(8)).astype(np.float64) * 2.0 ** -24
        r = mix(tk ^ mix(y * w32 + x)) % n2
        c = (c + r) % n2
    inv_n2 = 1.0 / float(n * n)
    u = (c.astype(np.float64) + jt) * inv_n2
    span = float(close) - float(open_)
    su = span * u  # multiply, then add
    return float(open_) + su


def sample_rays(cn, w, h, n, lens=None):
    """The sample rays (H, W, n, n, 6) of a shutter frame: lens = None (or an aperture of 0) the pinhole's,
    else (aperture, focal, jitter, seed)."""
    if lens is None or lens[0] == 0.0:
        return lens_rays(cn, w, h, n, 0.0, 1.0)
    return lens_rays(cn, w, h, n, *lens)


def trace(oracle, scene, rays, times, depth):
    """World::color_at of ray k in the world at times[k]: (colours (n, 3), the oracle's counters summed).
    One at_time world and one oracle call per distinct time."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    assert rays.shape[0] == times.shape[0]
    out = np.zeros((rays.shape[0], 3))
    total = {}
    for tau in np.unique(times):
        at = times == tau
        cols, st = oracle.color_at(scene.at_time(float(tau)).expanded(), rays[at], depth)
        out[at] = cols
        for k, v in st.items():
            if isinstance(v, (int, np.integer)):
                total[k] = total.get(k, 0) + int(v)
    return out, total


def trace_at_times(reference_trace, scene, rays, times):
    """A numpy restatement (smooth_reference.trace, texture_reference.trace: colours, the primary hits and a
    decision margin per ray) over (ray, time) pairs, where the oracle has nothing to say: ray k in
    scene.at_time(times[k]).expanded(), grouped by time as trace() groups them.  Returns (colours (n, 3),
    {"t", "shape"} of the primary hits, margins (n,))."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    assert rays.shape[0] == times.shape[0]
    n = rays.shape[0]
    out, margin = np.zeros((n, 3)), np.zeros(n)
    hit = {"t": np.full(n, np.inf), "shape": np.full(n, -1, dtype=np.int64)}
    for tau in np.unique(times):
        at = times == tau
        cols, h, m = reference_trace(scene.at_time(float(tau)).expanded(), rays[at])
        out[at], margin[at] = cols, m
        hit["t"][at], hit["shape"][at] = h["t"], h["shape"]
    return out, hit, margin


def frame(oracle, scene, cam, rtc, w, h, n, shutter, depth, lens=None):
    """The frame rt_render_shutter means: the ordered mean over the n^2 oracle colours of every pixel.
    shutter = (open, close, jitter, seed)."""
    c = rtc.camera_resize(cam, w, h)
    cn = rtc.camera_resize(c, n * w, n * h)
    rays = sample_rays(cn, w, h, n, lens).reshape(-1, 6)
    times = shutter_times(w, h, n, *shutter).reshape(-1)
    cols, st = trace(oracle, scene, rays, times, depth)
    return ordered_mean(cols, h, w, n), st
