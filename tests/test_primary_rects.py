"""CPU check of the direct kernel's primary cull (rtc_kernels.hip closest_hit /
wave_pixel_block, primary_rect.hpp): the host's screen
rectangle of a bounding ball must hold every pixel whose primary ray passes
the kernel's per-lane ball test, so a wave whose pixel block misses the
rectangle loses nothing by passing the shape by.

The model is the kernel's own f32 arithmetic: camera_ray (wx = half_width -
(x + 0.5) pixel_size, the direction through the f32 camera matrix, normalised
by a reciprocal square root) and wave_ball_may_hit's half-line test
((|oc|^2 kKeep - r^2) |d|^2 <= (oc.d)^2, front: oc.d >= 0 or |oc|^2 <= r^2),
with fused multiply-adds where the kernel fuses.  The rectangle comes from the
library (rt_camera_bound_rect), which runs the function a launch runs.

Random cameras (fov 0.3 .. 2.5, random view transforms, canvases from 64x48
to 1920x1080, ragged against the 64x4 tile and the 16x4 wave block) against
random balls: in front of the camera, straddling the eye plane, behind the
camera, around the camera, and unbounded (radius^2 = +inf).  Zero exceptions.
"""
import numpy as np
import pytest

F = np.float32
K_KEEP = F(1 - 1e-5)


def fma(a, b, c):
    # a f32 product is exact in f64; the sum rounds once more on the way back
    return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def camera_rays(cam):
    """camera_ray's f32 directions for every pixel: (H, W, 3)."""
    inv = np.array(cam.inverse[:12], np.float64).astype(F)
    hw, hh, ps = F(cam.half_width), F(cam.half_height), F(cam.pixel_size)
    x = np.arange(cam.width, dtype=np.uint32).astype(F)
    y = np.arange(cam.height, dtype=np.uint32).astype(F)
    wx = np.broadcast_to((hw - (x + F(0.5)) * ps).astype(F)[None, :], (cam.height, cam.width))
    wy = np.broadcast_to((hh - (y + F(0.5)) * ps).astype(F)[:, None], (cam.height, cam.width))
    wz = F(-1)
    row = lambda r: fma(np.full_like(wx, inv[4 * r + 2]), wz, fma(np.full_like(wx, inv[4 * r + 1]), wy, inv[4 * r] * wx))  # noqa: E731
    v = [row(0), row(1), row(2)]
    n2 = fma(v[2], v[2], fma(v[1], v[1], v[0] * v[0]))
    rs = (F(1) / np.sqrt(n2)).astype(F)
    return np.stack([(c * rs).astype(F) for c in v], axis=-1)


def ball_test(o, d, bound):
    """wave_ball_may_hit<float, true>, lane-wise."""
    oc = [(F(bound[i]) - o[i]).astype(F) if isinstance(o[i], np.ndarray) else F(F(bound[i]) - o[i]) for i in range(3)]
    dot = lambda a, b: fma(a[..., 2], b[2], fma(a[..., 0], b[0], a[..., 1] * b[1]))  # noqa: E731
    tc = dot(d, oc)
    oo = F(np.float64(oc[2]) * oc[2] + np.float64(F(np.float64(oc[0]) * oc[0] + np.float64(F(oc[1] * oc[1])))))
    dd = fma(d[..., 2], d[..., 2], fma(d[..., 0], d[..., 0], d[..., 1] * d[..., 1]))
    r2 = F(bound[3])
    with np.errstate(all="ignore"):
        lhs = (F(np.float64(oo) * np.float64(K_KEEP) - np.float64(r2)) * dd).astype(F)
        return ((tc >= 0) | (oo <= r2)) & (lhs <= (tc * tc).astype(F))


def random_camera(rtc, rng, size):
    w, h = size
    frm = rng.uniform(-8, 8, 3)
    to = frm + rng.normal(size=3) * rng.uniform(0.5, 10)
    up = rng.normal(size=3)
    return rtc.camera_make(w, h, float(rng.uniform(0.3, 2.5)), frm, to, up)


def random_ball(cam, rng, kind):
    """(centre, r^2) in world space, f32, from a camera-space recipe."""
    m = np.array(cam.inverse[:], np.float64).reshape(4, 4)
    ext = max(cam.half_width, cam.half_height)
    if kind in ("front", "inf"):
        b = rng.uniform(0.5, 40.0)
        r = b * rng.uniform(0.01, 0.6)
        # on the canvas, across its edges, or just off it
        c = np.array([rng.uniform(-1.6, 1.6) * ext * b, rng.uniform(-1.6, 1.6) * ext * b, -b])
    elif kind == "straddle":
        r = rng.uniform(0.5, 5.0)
        c = np.array([rng.uniform(-3, 3) * r, rng.uniform(-3, 3) * r, rng.uniform(-0.99, 0.99) * r])
        if np.linalg.norm(c) < r:  # keep the eye outside: `around` covers the rest
            c[0] += 2 * r
    elif kind == "behind":
        r = rng.uniform(0.1, 5.0)
        c = np.array([rng.uniform(-10, 10), rng.uniform(-10, 10), r * rng.uniform(1.001, 8.0)])
    else:  # around the camera
        r = rng.uniform(0.5, 20.0)
        c = rng.normal(size=3)
        c *= rng.uniform(0, 0.999) * r / np.linalg.norm(c)
    world = (m @ np.append(c, 1.0))[:3]
    r2 = np.inf if kind == "inf" else r * r
    return np.append(world, r2).astype(F)


SIZES = [(64, 48), (100, 75), (333, 201), (641, 363), (800, 450), (1279, 719), (1920, 1080)]
KINDS = ["front"] * 7 + ["straddle", "behind", "around", "inf"]


def test_rectangle_holds_every_pixel_the_ball_test_passes(rtc):
    rng = np.random.default_rng(20)
    pairs = fallbacks = tight = passed_pixels = empty_rects = 0
    for size in SIZES:
        for _ in range(3 if size[0] < 1000 else 2):
            cam = random_camera(rtc, rng, size)
            w, h = size
            d = camera_rays(cam)
            o = [F(cam.origin[i]) for i in range(3)]
            for kind in KINDS:
                bound = random_ball(cam, rng, kind)
                x0, y0, x1, y1 = rtc.camera_bound_rect(cam, bound)
                passes = ball_test(o, d, bound)
                outside = passes.copy()
                if x0 <= x1 and y0 <= y1:
                    assert x1 <= w - 1 and y1 <= h - 1
                    outside[y0:y1 + 1, x0:x1 + 1] = False
                else:
                    empty_rects += 1
                assert not outside.any(), (
                    f"{kind} ball {bound} camera {size} fov {cam.field_of_view}: {int(outside.sum())} pixels pass the "
                    f"ball test outside the rectangle {(x0, y0, x1, y1)}, first at {np.argwhere(outside)[0][::-1]}")
                pairs += 1
                full = (x0, y0, x1, y1) == (0, 0, w - 1, h - 1)
                fallbacks += full
                passed_pixels += int(passes.sum())
                if kind == "inf":
                    assert full and passes.all(), "an unbounded shape must keep the whole canvas"
                if kind == "behind":
                    assert not passes.any()
                if not full and x0 <= x1 and passes.any():
                    ys, xs = np.nonzero(passes)
                    # no looser than the one-pixel margin plus the kernel's own slack calls for: the
                    # rectangle stays within 3 pixels + 2 % of the extent of the pixels that pass
                    slack_x, slack_y = 3 + 0.02 * (x1 - x0), 3 + 0.02 * (y1 - y0)
                    tight += (xs.min() - x0 <= slack_x or x0 == 0) and (x1 - xs.max() <= slack_x or x1 == w - 1) and \
                             (ys.min() - y0 <= slack_y or y0 == 0) and (y1 - ys.max() <= slack_y or y1 == h - 1)
    assert pairs >= 150 and passed_pixels > 100000
    # the culls must come from the formula, not from falling back to the whole canvas
    assert fallbacks < 0.5 * pairs, f"{fallbacks} of {pairs} pairs fell back to the full canvas"
    assert empty_rects >= 10  # balls behind the camera and off the canvas
    assert tight >= 20, f"only {tight} rectangles hug the pixels that pass"


def test_three_sphere_frame_rectangles(rtc):
    """The headline frame: each sphere's rectangle holds its ball test's pixels and most 16x4 wave
    blocks of the 1080p frame overlap no rectangle (the blocks the primary cull passes by)."""
    from conftest import scene_fixture
    scene = scene_fixture("three_sphere_scene")
    cam = rtc.camera_resize(scene.camera, 1920, 1080)
    d = camera_rays(cam)
    o = [F(cam.origin[i]) for i in range(3)]
    shapes = [s for s in scene.shapes if int(s.kind) == 0]
    assert len(shapes) == 3
    overlap_any = np.zeros((1080 // 4, 1920 // 16), bool)
    for s in shapes:
        inv = np.array(s.inverse[:], np.float64).reshape(4, 4)
        fwd = np.linalg.inv(inv)
        centre = fwd[:3, 3]
        r = np.sqrt(np.abs(fwd[:3, :3].T @ fwd[:3, :3]).sum(axis=1).max())
        pad = 1e-3 * r + 1e-4 * (np.abs(centre).sum() + r) + 1e-4  # rtc_host.cpp bounding_sphere
        bound = np.append(centre, (r + pad) ** 2).astype(F)
        x0, y0, x1, y1 = rtc.camera_bound_rect(cam, bound)
        passes = ball_test(o, d, bound)
        assert passes.any()
        outside = passes.copy()
        outside[y0:y1 + 1, x0:x1 + 1] = False
        assert not outside.any()
        ys, xs = np.nonzero(passes)
        assert 1 <= xs.min() - x0 <= 4 and 1 <= x1 - xs.max() <= 4 and 1 <= ys.min() - y0 <= 4 and 1 <= y1 - ys.max() <= 4
        overlap_any[y0 // 4:y1 // 4 + 1, x0 // 16:x1 // 16 + 1] = True
    assert 0.6 < 1 - overlap_any.mean() < 0.8  # ~70 % of the frame's wave blocks pass every sphere by


def test_bad_arguments(rtc):
    from rtc_amd import _lib
    assert _lib.rt_camera_bound_rect(None, None, None) == -1
    cam = rtc.camera_make(0, 0, 1.0, (0, 0, -5), (0, 0, 0), (0, 1, 0))
    with pytest.raises(rtc.RenderError):
        rtc.camera_bound_rect(cam, (0, 0, 0, 1))
