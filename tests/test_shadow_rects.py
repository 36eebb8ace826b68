"""CPU check of the direct kernel's shadow cull by screen rectangles
(rtc_kernels.hip any_hit under shade_hit_const, primary_rect.hpp shadow_rect /
shadow_near): for a wave whose hits all lie on one plane the
launch says, per light and caster, whether the wave's 16 x 4 pixel block lies
outside the screen rectangle in which the caster's ball can shadow that plane,
and the wave then passes the caster by without its per-lane test.

The model is the kernel's own f32 arithmetic: camera_ray, the plane's entry
(object y of origin and direction, t by a reciprocal), p = o + t d, the normal
turned to the eye, the over-point at the flat kinds' offset and at the larger
3e-5 max(1, |p|inf) of the other kinds, tl = l - over, tt = |tl|^2, and both
forms of any_hit's ball cull: from the light's side, and the first form (the
ray from the over-point) that a wave takes when one of its lanes is farther
than kLightCullFar from the light.  Rectangles and spans come from the library
(rt_camera_shadow_rect, rt_camera_shadow_near), which runs the functions a
launch runs.

The first form's ball grows with the distance of the hit from the light, so
far enough away every ray passes it: the rectangle speaks for hits within
reach of the light, and the launch lets a block take it only in the columns or
rows that rt_camera_shadow_near reports as holding no hit beyond that reach.
What is asserted is what a launch relies on: in every block that may take the
rectangle, zero pixels outside the rectangle pass the form that any_hit takes
for a segment of their length (the light-side form up to kLightCullFar, the
first form beyond it), for either offset, and every hit of such a block is
nearer to the light than kLightCullFar, so its wave does take the light-side
form.  The same holds pixel by pixel for every hit within the reach, whatever
its block.

Random cameras (fov 0.3 .. 2.5, random views, canvases 64x48 .. 1920x1080,
ragged against 16x4), random planes, lights and balls: compact shadows,
shadows across the canvas edge, shadows that run to the horizon, and the
degenerate cases (the light in or on the ball, radius^2 infinite or negative,
the light or the eye on the plane, a singular camera matrix).
"""
import numpy as np
import pytest

from test_primary_rects import F, K_KEEP, camera_rays, fma, random_camera

FAR = F(100.0)           # any_hit kLightCullFar
REACH = 99.0           # primary_rect.hpp kShadowReach
FLAT_OFFSET, REL_OFFSET = F(1.9073486e-6), F(3e-5)
EMPTY = (0xFFFFFFFF, 0xFFFFFFFF, 0, 0)


def dot3(a, b):
    """dot(): rfma(a.z, b.z, rfma(a.x, b.x, a.y * b.y))"""
    return fma(a[2], b[2], fma(a[0], b[0], (a[1] * b[1]).astype(F)))


def sq3(a):
    """madd(z, z, madd(y, y, x * x))"""
    return fma(a[2], a[2], fma(a[1], a[1], (a[0] * a[0]).astype(F)))


def plane_hits(cam, d, plane):
    """The kernel's entry of plane (n, h) for every pixel's primary ray: hit mask, p, unit normal toward the eye."""
    n = [F(plane[i]) for i in range(3)]
    o = [F(cam.origin[i]) for i in range(3)]
    dd = [d[..., i] for i in range(3)]
    with np.errstate(all="ignore"):
        # xform_point / xform_vector, row 1 of the record's inverse = (n, -h)
        loy = fma(n[2], o[2], fma(n[1], o[1], fma(n[0], o[0], F(-plane[3]))))
        ldy = fma(n[2], dd[2], fma(n[1], dd[1], (n[0] * dd[0]).astype(F)))
        t = ((-loy) * (F(1) / ldy).astype(F)).astype(F)
        hit = ~(np.abs(ldy) < F(8e-8)) & (t > 0) & np.isfinite(t)
        p = [fma(dd[i], t, o[i]) for i in range(3)]
        rs = F(1) / np.sqrt(sq3(n))
        nu = [F(n[i] * rs) for i in range(3)]
        flip = dot3([np.full_like(t, nu[i]) for i in range(3)], [-dd[i] for i in range(3)]) < 0
        nn = [np.where(flip, -nu[i], nu[i]).astype(F) for i in range(3)]
    return hit, p, nn, o


def over_points(p, nn, o, rel):
    """Real<float>::surface_offset: the flat kinds' (rel = False) or the quadrics' 3e-5 max(1, |p|inf)."""
    with np.errstate(all="ignore"):
        mp = np.maximum(np.maximum(np.abs(p[0]), np.abs(p[1])), np.maximum(np.abs(p[2]), F(1)))
        if rel:
            off = (REL_OFFSET * mp).astype(F)
        else:
            mo = np.maximum(np.maximum(np.abs(o[0]), np.abs(o[1])), np.maximum(np.abs(o[2]), mp))
            off = (FLAT_OFFSET * mo).astype(F)
        return [fma(nn[i], off, p[i]) for i in range(3)]


def cull_passes(over, light, bound):
    """(light-side form, first form, tt) of any_hit's ball cull for the shadow ray over -> light, lane-wise."""
    l = [F(light[i]) for i in range(3)]
    c = [F(bound[i]) for i in range(3)]
    r2 = F(bound[3])
    with np.errstate(all="ignore"):
        tl = [(l[i] - over[i]).astype(F) for i in range(3)]
        tt = sq3(tl)
        # wave_ball_may_hit_from
        cl = [F(c[i] - l[i]) for i in range(3)]
        cc = F(np.float64(cl[2]) * cl[2] + np.float64(F(np.float64(cl[0]) * cl[0] + np.float64(F(cl[1] * cl[1])))))
        k = F(np.float64(cc) * np.float64(K_KEEP) - np.float64(r2))
        if not k > 0:
            from_light = np.ones(tt.shape, bool)
        else:
            tc = dot3([np.full_like(tt, cl[i]) for i in range(3)], tl)
            from_light = (tc <= 0) & ((k * tt).astype(F) <= (tc * tc).astype(F))
        # wave_ball_may_hit<float, true> along ld = normalized(to_light), |d|^2 formed from it
        rs = (F(1) / np.sqrt(tt)).astype(F)
        ld = [(tl[i] * rs).astype(F) for i in range(3)]
        oc = [(c[i] - over[i]).astype(F) for i in range(3)]
        tc1, oo = dot3(oc, ld), dot3(oc, oc)
        dd = dot3(ld, ld)
        lhs = (fma(oo, K_KEEP, -r2) * dd).astype(F)
        first = ((tc1 >= 0) | (oo <= r2)) & (lhs <= (tc1 * tc1).astype(F))
    return from_light, first, tt


def block_mask(lo, hi, n, cell):
    """Per pixel of one axis: its block lies wholly inside [lo, hi] (the canvas's last block ends with the canvas)."""
    idx = np.arange(n)
    first = idx // cell * cell
    last = np.minimum(first + cell - 1, n - 1)
    return (first >= lo) & (last <= hi) if lo <= hi else np.zeros(n, bool)


def eligible(span, w, h):
    """The pixels whose 16x4 block may take a rectangle's answer: the launch's rule (rtc_host.cpp)."""
    x0, y0, x1, y1 = span
    return block_mask(y0, y1, h, 4)[:, None] | block_mask(x0, x1, w, 16)[None, :]


def in_rect(rect, w, h):
    m = np.zeros((h, w), bool)
    x0, y0, x1, y1 = rect
    if x0 <= x1 and y0 <= y1:
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def check_rect(rect, w, h):
    x0, y0, x1, y1 = rect
    if rect == EMPTY:
        return
    assert x0 <= x1 < w and y0 <= y1 < h, f"reversed or off-canvas rectangle {rect} on {w}x{h}"


def check_pair(rtc, cam, hits, plane, light, bound, span, stats, what):
    """One (plane, light, caster) on one camera: the rectangle against the model."""
    w, h = cam.width, cam.height
    hit, p, nn, o = hits
    rect = rtc.camera_shadow_rect(cam, plane, light, bound)
    check_rect(rect, w, h)
    inside = in_rect(rect, w, h)
    elig = eligible(span, w, h)
    for rel in (False, True):
        over = over_points(p, nn, o, rel)
        a, b, tt = cull_passes(over, light, bound)
        with np.errstate(all="ignore"):
            passes = hit & np.where(tt <= FAR * FAR, a, b)  # the form any_hit takes for a segment of this length
            near_px = hit & (tt <= F(REACH * REACH))
        bad = passes & ~inside & (elig | near_px)
        assert not bad.any(), (
            f"{what}: {int(bad.sum())} pixels pass the cull outside {rect} (span {span}, offset class {int(rel)}), "
            f"first at {np.argwhere(bad)[0][::-1]}; plane {plane} light {light} bound {bound} "
            f"camera {w}x{h} fov {cam.field_of_view}")
        far_in = hit & elig & ~(tt < F(99.5) * F(99.5))
        assert not far_in.any(), f"{what}: a block inside span {span} holds a hit beyond kLightCullFar"
    stats["pairs"] += 1
    stats["full"] += rect == (0, 0, w - 1, h - 1)
    stats["empty"] += rect == EMPTY
    stats["passed"] += int(passes.sum())
    if rect not in ((0, 0, w - 1, h - 1), EMPTY) and (passes & elig).any():
        ys, xs = np.nonzero(passes & (elig | near_px))
        x0, y0, x1, y1 = rect
        # no looser than the one-pixel margin and the angle margins call for
        slack_x, slack_y = 4 + 0.05 * (x1 - x0), 4 + 0.05 * (y1 - y0)
        stats["tight"] += (xs.min() - x0 <= slack_x or x0 == 0) and (x1 - xs.max() <= slack_x or x1 == w - 1) and \
                          (ys.min() - y0 <= slack_y or y0 == 0) and (y1 - ys.max() <= slack_y or y1 == h - 1)
    return rect


def random_plane(cam, rng):
    """A plane the camera looks at: through a point ahead of the eye, tilted at random."""
    m = np.array(cam.inverse[:], np.float64).reshape(4, 4)
    ahead = (m @ np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.6, -0.1), -rng.uniform(2, 12), 1.0]))[:3]
    n = rng.normal(size=3)
    n /= np.linalg.norm(n)
    n *= rng.choice([1.0, 1.0, 0.37, 2.5])  # (a scaled plane's row is no unit vector)
    eye = np.array(cam.origin[:3])
    if n @ (eye - ahead) < 0:
        n = -n
    return np.append(n, n @ ahead).astype(F)


def random_light(plane, cam, rng, side=1.0):
    n = plane[:3].astype(np.float64)
    nu = n / np.linalg.norm(n)
    foot = (np.array(cam.origin[:3]) + rng.normal(size=3) * 4)
    foot -= (n @ foot - plane[3]) / (n @ n) * n
    return (foot + side * nu * rng.uniform(2, 15) + rng.normal(size=3)).astype(F)


def random_caster(plane, light, rng, family):
    """A ball between the light and the plane; `horizon`: low enough to throw its shadow to the plane's horizon."""
    n = plane[:3].astype(np.float64)
    nu = n / np.linalg.norm(n)
    l = light.astype(np.float64)
    height = abs(n @ l - plane[3]) / np.linalg.norm(n)
    if family == "horizon":
        r = rng.uniform(0.2, 1.0)
        side = rng.normal(size=3)
        side -= (side @ nu) * nu
        side /= np.linalg.norm(side)
        c = l + side * rng.uniform(2, 6) - np.sign(nu @ l - plane[3] / np.linalg.norm(n)) * nu * r * rng.uniform(-0.5, 0.5)
    else:
        r = rng.uniform(0.05, 0.25) * height
        target = l - np.sign(n @ l - plane[3]) * nu * height + rng.normal(size=3) * height * (0.3 if family == "compact" else 1.2)
        c = l + (target - l) * rng.uniform(0.3, 0.9)
    return np.append(c, r * r).astype(F)


SIZES = [(64, 48), (100, 75), (333, 201), (641, 363), (800, 450), (1279, 719), (1920, 1080)]


def test_rectangles_hold_every_pixel_that_passes_the_cull(rtc):
    rng = np.random.default_rng(29)
    stats = dict(pairs=0, full=0, empty=0, passed=0, tight=0)
    culling = spans = 0
    for size in SIZES:
        small = size[0] < 700  # (the large canvases once each: the model costs ~50 ns a pixel and pair)
        for _ in range(2 if small else 1):
            cam = random_camera(rtc, rng, size)
            d = camera_rays(cam)
            for _ in range(2 if small else 1):
                plane = random_plane(cam, rng)
                hits = plane_hits(cam, d, plane)
                light = random_light(plane, cam, rng)
                span = rtc.camera_shadow_near(cam, plane, light)
                spans += span[0] <= span[2] or span[1] <= span[3]
                for family in ("compact", "compact", "edge", "horizon"):
                    bound = random_caster(plane, light, rng, family)
                    rect = check_pair(rtc, cam, hits, plane, light, bound, span, stats, family)
                    culling += rect != (0, 0, size[0] - 1, size[1] - 1) and (span[0] <= span[2] or span[1] <= span[3])
    assert stats["pairs"] >= 70 and stats["passed"] > 20000, stats
    # the culls must come from the geometry, not from falling back to the whole canvas or to no span
    assert culling >= 0.3 * stats["pairs"], (culling, spans, stats)
    assert stats["tight"] >= 0.1 * stats["pairs"], stats  # (of the pairs whose shadow shows in blocks that may take it)


def test_degenerate_cases_keep_the_whole_canvas(rtc):
    rng = np.random.default_rng(31)
    cam = rtc.camera_make(333, 201, 1.0, (0, 1.5, -5), (0, 1, 0), (0, 1, 0))
    w, h = 333, 201
    full = (0, 0, w - 1, h - 1)
    d = camera_rays(cam)
    floor = np.array([0, 1, 0, 0], F)
    light = np.array([-10, 10, -10], F)
    stats = dict(pairs=0, full=0, empty=0, passed=0, tight=0)
    cases = {
        "light inside the ball": (floor, light, np.array([-9.5, 9.5, -9.5, 4.0], F)),
        "light on the ball": (floor, light, np.array([-10, 9, -10, 1.0], F)),
        "infinite radius": (floor, light, np.array([0, 1, 0, np.inf], F)),
        "negative radius": (floor, light, np.array([0, 1, 0, -1.0], F)),
        "NaN radius": (floor, light, np.array([0, 1, 0, np.nan], F)),
        "light on the plane": (floor, np.array([-3, 0, -3], F), np.array([0, 1, 0, 1.0], F)),
        "eye on the plane": (np.array([0, 1, 0, 1.5], F), light, np.array([0, 3, 0, 1.0], F)),
        "shadow to the horizon": (floor, np.array([-10, 1.0, 0], F), np.array([-5, 0.9, 0, 0.25], F)),
        "light far from the plane": (floor, np.array([0, 500, 0], F), np.array([0, 1, 0, 1.0], F)),
    }
    for what, (plane, lp, bound) in cases.items():
        hits = plane_hits(cam, d, plane)
        span = rtc.camera_shadow_near(cam, plane, lp)
        rect = check_pair(rtc, cam, hits, plane, lp, bound, span, stats, what)
        assert rect == full, (what, rect)
    # eye and light on opposite sides: whatever the rectangle, it holds the model's pixels
    below = np.array([2, -6, 1], F)
    hits = plane_hits(cam, d, floor)
    check_pair(rtc, cam, hits, floor, below, np.array([1, -2, 0.5, 0.49], F), rtc.camera_shadow_near(cam, floor, below), stats,
               "light below the floor")
    # a singular camera matrix, and one that is no rotation
    flat = cam.copy()
    for q in (8, 9, 10):
        flat.inverse[q] = 0.0
    assert rtc.camera_shadow_rect(flat, floor, light, (0, 1, 0, 1.0)) == full
    assert rtc.camera_shadow_near(flat, floor, light) == EMPTY
    skew = rtc.camera_make(w, h, 1.0, (0, 1.5, -5), (0, 1, 0), (0.6, 1, 0.2))
    ds = camera_rays(skew)
    hits = plane_hits(skew, ds, floor)
    rect = check_pair(rtc, skew, hits, floor, light, np.array([-0.5, 1, 0.5, 1.01], F),
                      rtc.camera_shadow_near(skew, floor, light), stats, "no rotation")
    assert rect != full and rect != EMPTY
    for _ in range(20):  # nothing not finite ever comes back reversed
        plane = rng.normal(size=4).astype(F) * F(rng.choice([1e-30, 1.0, 1e30]))
        r = rtc.camera_shadow_rect(cam, plane, rng.normal(size=3) * 1e3, np.append(rng.normal(size=3), rng.choice([1e-30, 1, 1e30])))
        check_rect(r, w, h)
        s = rtc.camera_shadow_near(cam, plane, rng.normal(size=3) * 1e3)
        assert all(v < max(w, h) or v == 0xFFFFFFFF for v in s)


def _f64_hits(cam, spheres, planes):
    """Nearest hit per pixel in f64: (slot, point), slot -1 = miss; spheres as (centre, r), planes as (n, h)."""
    m = np.array(cam.inverse[:], np.float64).reshape(4, 4)
    x = np.arange(cam.width) + 0.5
    y = np.arange(cam.height) + 0.5
    wx, wy = np.meshgrid(cam.half_width - x * cam.pixel_size, cam.half_height - y * cam.pixel_size)
    v = np.stack([wx, wy, -np.ones_like(wx)], axis=-1)
    d = v @ m[:3, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.array(cam.origin[:3], np.float64)
    best = np.full(wx.shape, np.inf)
    slot = np.full(wx.shape, -1)
    for i, (c, r) in enumerate(spheres):
        oc = o - c
        b = d @ oc
        disc = b * b - (oc @ oc - r * r)
        with np.errstate(invalid="ignore"):
            t = -b - np.sqrt(disc)
        ok = (disc >= 0) & (t > 0) & (t < best)
        best[ok], slot[ok] = t[ok], i
    for j, (n, hh) in enumerate(planes):
        with np.errstate(all="ignore"):
            t = (hh - n @ o) / (d @ n)
        ok = (t > 0) & (t < best)
        best[ok], slot[ok] = t[ok], len(spheres) + j
    return slot, o + best[..., None] * d


def test_three_sphere_rectangles_are_tight(rtc):
    """The headline frame at 1920x1080: over the (16x4 block that hits one plane throughout, sphere caster) pairs
    of an f64 brute-force hit classification, the launch's rule (rectangle and span) skips all but at most 5 %;
    the brute force itself, with balls padded by 1 % + 1e-3 (wider than the library's), keeps fewer than that."""
    from conftest import scene_fixture
    scene = scene_fixture("three_sphere_scene")
    cam = rtc.camera_resize(scene.camera, 1920, 1080)
    light = np.array(scene.lights[0].position[:3], np.float64)
    spheres, bounds, planes = [], [], []
    for s in scene.shapes:
        inv = np.array(s.inverse[:], np.float64).reshape(4, 4)
        if int(s.kind) == 0:
            fwd = np.linalg.inv(inv)
            centre, r = fwd[:3, 3], np.sqrt(np.abs(fwd[:3, :3].T @ fwd[:3, :3]).sum(axis=1).max())
            pad = 1e-3 * r + 1e-4 * (np.abs(centre).sum() + r) + 1e-4  # rtc_host.cpp bounding_sphere
            spheres.append((centre, r))
            bounds.append(np.append(centre, (r + pad) ** 2).astype(F))
        else:
            assert int(s.kind) == 1
            planes.append((inv[1, :3].copy(), -inv[1, 3]))
    assert len(spheres) == 3 and len(planes) == 3
    slot, p = _f64_hits(cam, spheres, planes)
    blocks = slot.reshape(270, 4, 120, 16).transpose(0, 2, 1, 3).reshape(270, 120, 64)
    tests = kept = brute = 0
    for j, (n, hh) in enumerate(planes):
        uniform = (blocks == 3 + j).all(axis=2)
        assert uniform.mean() > 0.15  # each wall and the floor fill a fifth of the frame's blocks or more
        plane = np.append(n, hh).astype(F)
        span = rtc.camera_shadow_near(cam, plane, light)
        elig = eligible(span, 1920, 1080)[::4, ::16]
        assert (elig & uniform).sum() > 0.98 * uniform.sum(), "the frame's plane blocks lie within reach of the light"
        for (c, r), bound in zip(spheres, bounds):
            x0, y0, x1, y1 = rtc.camera_shadow_rect(cam, plane, light, bound)
            assert (x0, y0, x1, y1) != (0, 0, 1919, 1079)
            overlap = np.zeros((270, 120), bool)
            if x0 <= x1:
                overlap[y0 // 4:y1 // 4 + 1, x0 // 16:x1 // 16 + 1] = True
            tests += int(uniform.sum())
            kept += int((uniform & (overlap | ~elig)).sum())
            # f64: the line from the light through the hit passes within the padded radius of the centre
            u = p - light
            cl = c - light
            tc = u @ cl
            dist2 = cl @ cl - tc * tc / np.einsum("...i,...i", u, u)
            shadow = (dist2 <= (1.01 * r + 1e-3) ** 2).reshape(270, 4, 120, 16).transpose(0, 2, 1, 3).reshape(270, 120, 64)
            brute += int((uniform & shadow.any(axis=2)).sum())
    assert tests > 60000
    print(f"three_sphere 1080p: {tests} (plane block, sphere) tests, rectangles keep {kept} ({kept / tests:.2%}), "
          f"f64 brute force {brute} ({brute / tests:.2%})")
    assert brute <= 0.05 * tests, f"the brute force keeps {brute / tests:.2%}"
    assert kept <= 0.05 * tests, f"the rectangles keep {kept / tests:.2%} of {tests} tests"


def test_bad_arguments(rtc):
    from rtc_amd import _lib
    assert _lib.rt_camera_shadow_rect(None, None, None, None, None) == -1
    assert _lib.rt_camera_shadow_near(None, None, None, None) == -1
    cam = rtc.camera_make(0, 0, 1.0, (0, 0, -5), (0, 0, 0), (0, 1, 0))
    with pytest.raises(rtc.RenderError):
        rtc.camera_shadow_rect(cam, (0, 1, 0, 0), (0, 5, 0), (0, 1, 0, 1))
    with pytest.raises(rtc.RenderError):
        rtc.camera_shadow_near(cam, (0, 1, 0, 0), (0, 5, 0))
