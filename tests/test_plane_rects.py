"""CPU check of the direct kernel's primary cull of planes (rtc_kernels.hip
closest_hit under RTC_PLANE_RECTS, primary_rect.hpp plane_rect, DESIGN.md
§3.3): outside the host's rectangle of plane q no primary ray may have q's
entry as its nearest, so a wave whose pixel block misses the rectangle loses
nothing by passing the plane's test by.

The model is the kernel's plane step in f32 for every pixel: camera_ray's
direction (test_primary_rects.camera_rays), ld = the record's row 1 times the
direction (a product and two fused multiply-adds), the launch term h (the
origin's object-space height, launch_terms.hpp), the validity test
|ld| >= 8e-8f (bits 0x33abcc77), t = rcp(ld) * -h and the key order of
Nearest::offer: the bits of (valid ? t : -1) + 0, then the world index.  The
rectangle comes from the library (rt_camera_plane_rect), which runs the
functions a launch runs.

For every pixel outside the rectangle of plane q the model must show q's entry
invalid or negative, or another plane's valid entry at t >= 0 nearer by at
least 16 ulp of t (the device's v_rcp_f32 and v_rsq_f32 may differ from the
model's correctly rounded ones in the last bit; 16 ulp keeps the order whatever
they return).  Zero exceptions.

Random cameras (as test_primary_rects) on canvases from 64x48 to 1920x1080,
ragged against the 16x4 block, against sets of 2-4 planes whose inverses are
rotated, sheared and unevenly scaled, with the eye on either side, pairs that
are parallel, nearly parallel (1e-5 .. 1e-2 rad) or coincident, and an eye
within 1e-6 of a plane; then three_sphere's own planes and camera at 1080p.

Observed here: 89 of the 90 random cases cull something; three_sphere at
1920x1080 keeps 1.145 plane tests per 16x4 block (the geometry alone: 1.13).
"""
import numpy as np
import pytest

from test_primary_rects import SIZES, F, camera_rays, fma, random_camera

K_EPS_BITS = 0x33ABCC77  # 8e-8f


def kfma(m, x, acc):
    """kfma / launch_kfma: a zero matrix entry's term is dropped."""
    return acc if m == 0 else fma(np.asarray(m, F), x, acc)


def plane_keys(cam, d, rows):
    """(bits of (valid ? t : -1) + 0 as uint32, t) per plane: (n, H, W) each, from the f32 rows {n, inv[7]}."""
    assert np.float32(8e-8).view(np.uint32) == K_EPS_BITS
    o = [F(cam.origin[i]) for i in range(3)]
    bits, ts = [], []
    for m in rows:
        h = kfma(m[2], o[2], kfma(m[1], o[1], kfma(m[0], o[0], F(m[3]))))
        ld = m[0] * d[..., 0] if m[0] != 0 else np.zeros_like(d[..., 0])
        ld = kfma(m[2], d[..., 2], kfma(m[1], d[..., 1], ld.astype(F))).astype(F)
        with np.errstate(all="ignore"):
            valid = np.abs(ld).view(np.uint32) >= K_EPS_BITS
            t = ((F(1) / ld).astype(F) * F(-h)).astype(F)
            tv = (np.where(valid, t, F(-1)) + F(0)).astype(F)
        bits.append(tv.view(np.uint32).copy())
        ts.append(t)
    return np.stack(bits), np.stack(ts)


def check_rectangles(rtc, cam, rows):
    """Asserts the property for every plane of `rows`; returns the rectangles."""
    w, h = cam.width, cam.height
    d = camera_rays(cam)
    bits, t = plane_keys(cam, d, rows)
    front = bits <= 0x7F800000  # valid and t >= 0 (negative, invalid and NaN keys order above +inf)
    t64 = t.astype(np.float64)
    rects = []
    for q in range(len(rows)):
        rect = rtc.camera_plane_rect(cam, rows, q)
        rects.append(rect)
        x0, y0, x1, y1 = rect
        outside = np.ones((h, w), bool)
        if x0 <= x1 and y0 <= y1:
            assert x1 <= w - 1 and y1 <= h - 1
            outside[y0:y1 + 1, x0:x1 + 1] = False
        may_win = front[q] & outside
        if not may_win.any():
            continue
        with np.errstate(all="ignore"):
            gap = 16.0 * np.spacing(t[q]).astype(np.float64)
            for p in range(len(rows)):
                if p != q:
                    may_win &= ~(front[p] & (t64[p] + gap <= t64[q]))
        assert not may_win.any(), (
            f"plane {q} of {rows.tolist()}, camera {w}x{h} fov {cam.field_of_view} from {list(cam.origin)}: "
            f"{int(may_win.sum())} pixels outside {rect} where no other plane is clearly nearer, first at "
            f"{np.argwhere(may_win)[0][::-1]}")
    return rects


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    m = np.eye(4)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m[i, i] = m[j, j] = c
    m[i, j], m[j, i] = -s, s
    return m


def _translate(v):
    m = np.eye(4)
    m[:3, 3] = v
    return m


def random_transform(rng, plain=False):
    """A plane's transformation: translate . rotate . shear . scale."""
    m = _rot(0, rng.uniform(-np.pi, np.pi)) @ _rot(2, rng.uniform(-np.pi, np.pi)) @ _rot(1, rng.uniform(-np.pi, np.pi))
    if not plain:
        shear = np.eye(4)
        shear[0, 1], shear[1, 0], shear[1, 2], shear[2, 1] = rng.uniform(-0.8, 0.8, 4)
        m = m @ shear @ np.diag(np.append(10.0 ** rng.uniform(-2, 2, 3), 1.0))
    return _translate(rng.uniform(-10, 10, 3)) @ m


def row_of(transform):
    return np.linalg.inv(transform)[1].astype(F)


def through(transform, point, off=0.0):
    """`transform` moved along its plane's normal so that the plane passes `off` (world units) from `point`."""
    inv = np.linalg.inv(transform)
    n = inv[1, :3]
    height = n @ point + inv[1, 3]  # object-space y of the point
    step = n / (n @ n) * (height - off * np.linalg.norm(n))
    return _translate(step) @ transform


def random_planes(cam, rng, kind):
    eye = np.array(cam.origin[:3])
    n = int(rng.integers(2, 5))
    ts = [random_transform(rng, plain=rng.random() < 0.3) for _ in range(n)]
    if kind == "parallel":
        ts[1] = _translate(rng.uniform(-6, 6, 3)) @ ts[0]
    elif kind == "nearly_parallel":
        tilt = _rot(int(rng.integers(0, 3)), 10.0 ** rng.uniform(-5, -2))
        ts[1] = _translate(rng.uniform(-3, 3, 3)) @ tilt @ ts[0]
    elif kind == "coincident":
        ts[1] = ts[0].copy()
        if n > 2 and rng.random() < 0.5:  # the same plane from the other side
            ts[2] = ts[0] @ np.diag([1.0, -1.0, 1.0, 1.0])
    elif kind == "eye_near":
        ts[0] = through(ts[0], eye, float(rng.choice([-1, 1])) * 10.0 ** rng.uniform(-9, -6))
    elif kind == "eye_on":
        ts[0] = through(ts[0], eye)
    elif kind == "room":  # a floor and two walls around the eye, roughly as the reference scenes build them
        a = rng.uniform(-0.5, 0.5)
        ts = [_translate([0, eye[1] - rng.uniform(0.5, 4), 0]),
              _translate(eye + [0, 0, rng.uniform(2, 12)]) @ _rot(1, a - np.pi / 4) @ _rot(0, np.pi / 2),
              _translate(eye + [0, 0, rng.uniform(2, 12)]) @ _rot(1, a + np.pi / 4) @ _rot(0, np.pi / 2)]
    return np.stack([row_of(t) for t in ts])


KINDS = ["random", "random", "parallel", "nearly_parallel", "coincident", "eye_near", "eye_on", "room"]


def test_no_pixel_outside_a_rectangle_can_hit_its_plane_first(rtc):
    rng = np.random.default_rng(23)
    cases = culled = 0
    for size in SIZES:
        cams = [random_camera(rtc, rng, size) for _ in range(2 if size[0] < 1000 else 1)]
        for cam in cams:
            for kind in (KINDS if size[0] < 1000 else KINDS[1:5] + KINDS[7:]):
                rows = random_planes(cam, rng, kind)
                rects = check_rectangles(rtc, cam, rows)
                cases += 1
                culled += any(r != (0, 0, size[0] - 1, size[1] - 1) for r in rects)
    assert cases >= 50
    # not vacuous: the rectangles must come from the geometry, not from falling back to the whole canvas
    assert culled >= 0.2 * cases, f"only {culled} of {cases} cases cull anything"


def three_sphere_rows(scene):
    planes = [s for s in scene.shapes if int(s.kind) == 1]
    return np.stack([np.array(s.inverse[4:8], np.float64).astype(F) for s in planes])


def test_three_sphere_1080p(rtc):
    """The headline frame: 1.145 plane tests per 16x4 block are left of 3 (at most 1.3 asked)."""
    from conftest import scene_fixture
    scene = scene_fixture("three_sphere_scene")
    cam = rtc.camera_resize(scene.camera, 1920, 1080)
    rows = three_sphere_rows(scene)
    assert len(rows) == 3
    rects = check_rectangles(rtc, cam, rows)
    tests = np.zeros((1080 // 4, 1920 // 16))
    for x0, y0, x1, y1 in rects:
        assert x0 <= x1 and y0 <= y1  # each of the three is seen somewhere
        tests[y0 // 4:y1 // 4 + 1, x0 // 16:x1 // 16 + 1] += 1
    print(f"three_sphere 1080p: rectangles {rects}, {tests.mean():.4f} plane tests per block")
    assert tests.min() >= 1  # the room is closed: every pixel sees a plane
    assert tests.mean() <= 1.3


def test_bad_arguments(rtc):
    from rtc_amd import _lib
    assert _lib.rt_camera_plane_rect(None, None, 0, 0, None) == -1
    cam = rtc.camera_make(64, 48, 1.0, (0, 1, -5), (0, 0, 0), (0, 1, 0))
    rows = np.array([[0, 1, 0, 0]], F)
    x0, y0, x1, y1 = rtc.camera_plane_rect(cam, rows, 0)  # a floor alone: from the horizon (row 12) down
    assert (x0, x1, y1) == (0, 63, 47) and 8 <= y0 <= 12
    with pytest.raises(rtc.RenderError):
        rtc.camera_plane_rect(cam, rows, 1)  # q past the planes
    with pytest.raises(rtc.RenderError):
        rtc.camera_plane_rect(cam, np.zeros((9, 4), F), 0)  # past the cull's eight slots
    empty = rtc.camera_make(0, 0, 1.0, (0, 0, -5), (0, 0, 0), (0, 1, 0))
    with pytest.raises(rtc.RenderError):
        rtc.camera_plane_rect(empty, rows, 0)
    # a plane wholly behind the camera: never the nearest
    up = rtc.camera_make(64, 48, 0.8, (0, 1, 0), (0, 5, 0.001), (0, 0, 1))
    assert rtc.camera_plane_rect(up, rows, 0)[0] > rtc.camera_plane_rect(up, rows, 0)[2]
