"""CPU check of the shadow any-hit's ball test from the light's side
(rtc_kernels.hip wave_ball_may_hit_from / any_hit), on the
kernel's own f32 arithmetic, in the style of tests/test_shadow_skips.py.

The per-scene f32 direct build tests the half-line from the light l through the surface
point instead of the shadow ray's own half-line: with cl = c - l and
tl = l - point, a lane may meet the ball iff
    (|cl|^2 kKeep - r^2) |tl|^2 <= (cl . tl)^2  and  cl . tl <= 0,
or the light is inside the ball.  A lane this rejects must be one where the
sphere's own roots (sphere_world, world space: oc = c - o, disc =
r^2 |d|^2 - |d x oc|^2, t = (d.oc -+ sqrt(disc)) / |d|^2) report no entry with
0 <= t < distance, for the ray the kernel traces: o = the point,
d = tl / |tl| by a reciprocal square root.  The ball is the sphere's own
padded bound (rtc_host.cpp bounding_sphere) or a cluster ball around it.
Points sit anywhere, and within 1e-6 .. 1e-3 (relative) of the sphere's
silhouette as the light sees it, in front of and behind the sphere; lights
sit outside, just outside and inside the ball.  Segments are at most
kLightCullFar = 100 long, the range any_hit applies the test in.
"""
import numpy as np

F = np.float32
K_KEEP = F(1 - 1e-5)
FAR = 100.0


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def dot(a, b):  # rtc_kernels.hip dot: fma(a.z, b.z, fma(a.x, b.x, a.y * b.y))
    return fma(a[..., 2], b[..., 2], fma(a[..., 0], b[..., 0], (a[..., 1] * b[..., 1]).astype(F)))


def cross(a, b):
    return np.stack([fma(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1]).astype(F)),
                     fma(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2]).astype(F)),
                     fma(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]).astype(F))], axis=-1)


def from_light_may_hit(ball, light, tl, tt):
    """wave_ball_may_hit_from, lane-wise."""
    cl = (ball[:3] - light).astype(F)
    k = fma(dot(cl, cl), K_KEEP, -ball[3])
    if not k > 0:
        return np.ones(tl.shape[0], bool)
    tc = dot(np.broadcast_to(cl, tl.shape), tl)
    return (tc <= 0) & ((k * tt).astype(F) <= (tc * tc).astype(F))


def line_from_point_may_hit(ball, o, d):
    """wave_ball_may_hit<float, false>, lane-wise: the line part of the test the new one replaces."""
    oc = (ball[:3] - o).astype(F)
    tc, oo, dd = dot(oc, d), dot(oc, oc), dot(d, d)
    return (fma(oo, K_KEEP, -ball[3]) * dd).astype(F) <= (tc * tc).astype(F)


def sphere_blocks(centre, r2, o, d, dist):
    """sphere_world's two roots and Blocker: some entry with 0 <= t < dist."""
    oc = (centre - o).astype(F)
    dd = dot(d, d)
    with np.errstate(all="ignore"):
        rdd = (F(1) / dd).astype(F)
        tc = dot(d, oc)
        c = cross(d, oc)
        disc = ((r2 * dd).astype(F) - dot(c, c)).astype(F)
        v = ~(disc < 0)
        root = np.sqrt(disc).astype(F)
        t1, t2 = ((tc - root) * rdd).astype(F), ((tc + root) * rdd).astype(F)
    hit = lambda t: v & (t >= 0) & (t < dist)  # noqa: E731
    return hit(t1) | hit(t2)


def padded_radius(centre, r):
    return r + 1e-3 * r + 1e-4 * (np.abs(centre).sum() + r) + 1e-4  # rtc_host.cpp bounding_sphere


def points_for(rng, centre, r, light, n):
    """Surface points: anywhere, and next to the sphere's silhouette seen from the light."""
    to_c = centre - light
    dc = np.linalg.norm(to_c)
    anywhere = centre + rng.normal(size=(n, 3)) * rng.uniform(0.2, 6.0, (n, 1)) * max(r, 0.5)
    if dc <= r * 1.0001:
        return anywhere
    axis = to_c / dc
    a = np.cross(axis, rng.normal(size=3))
    a /= np.linalg.norm(a)
    b = np.cross(axis, a)
    eps = rng.choice([0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3], n)
    sin_t = np.clip(r * (1 + eps) / dc, 0, 1)
    cos_t = np.sqrt(1 - sin_t * sin_t)
    phi = rng.uniform(0, 2 * np.pi, n)
    u = cos_t[:, None] * axis + sin_t[:, None] * (np.cos(phi)[:, None] * a + np.sin(phi)[:, None] * b)
    s = dc * rng.uniform(0.05, 3.0, n)  # before the tangent point, at it, and well behind the sphere
    near = light + u * s[:, None]
    pick = rng.random(n) < 0.6
    return np.where(pick[:, None], near, anywhere)


def test_light_side_cull_never_rejects_a_blocked_lane():
    rng = np.random.default_rng(5)
    lanes = rej_new = rej_old = blocked_n = inside_lights = 0
    for trial in range(300):
        centre = rng.uniform(-20, 20, 3)
        r = float(rng.choice([0.05, 0.33, 1.0, 2.5, 8.0])) * rng.uniform(0.8, 1.25)
        cf = centre.astype(F)
        r2f = F(r * r)  # the record's tri[3] (similar_sphere)
        if trial % 3 == 2:  # a cluster ball around the sphere's own ball, off centre
            off = rng.normal(size=3) * r * rng.uniform(0.2, 2.0)
            bc = centre + off
            br = (np.linalg.norm(off) + padded_radius(centre, r)) * rng.uniform(1.0, 1.3)
        else:
            bc, br = centre, padded_radius(centre, r)
        ball = np.append(bc, br * br).astype(F)
        kind = trial % 5
        dirn = rng.normal(size=3)
        dirn /= np.linalg.norm(dirn)
        if kind == 0:  # inside the ball
            light = bc + dirn * br * rng.uniform(0, 0.99)
            inside_lights += 1
        elif kind == 1:  # just outside it
            light = bc + dirn * br * (1 + float(rng.choice([1e-6, 1e-4, 1e-2])))
        else:
            light = bc + dirn * br * rng.uniform(1.2, 12.0)
        lf = light.astype(F)
        n = 4000
        p = points_for(rng, centre, r, light, n).astype(F)
        tl = (lf - p).astype(F)
        tt = fma(tl[:, 2], tl[:, 2], fma(tl[:, 1], tl[:, 1], (tl[:, 0] * tl[:, 0]).astype(F)))
        ok = (tt > 0) & (tt <= F(FAR * FAR))
        p, tl, tt = p[ok], tl[ok], tt[ok]
        dist = np.sqrt(tt).astype(F)
        d = (tl * (F(1) / np.sqrt(tt)).astype(F)[:, None]).astype(F)
        may = from_light_may_hit(ball, lf, tl, tt)
        blocked = sphere_blocks(cf, r2f, p, d, dist)
        bad = ~may & blocked
        assert not bad.any(), (f"trial {trial}: the light-side test rejected {int(bad.sum())} blocked lanes; first: point "
                               f"{p[bad][0]} light {lf} sphere {cf} r {r} ball {ball}")
        lanes += len(p)
        rej_new += int((~may).sum())
        rej_old += int((~line_from_point_may_hit(ball, p, d)).sum())
        blocked_n += int(blocked.sum())
    assert lanes > 500000 and blocked_n > 50000 and inside_lights >= 50
    # Not vacuous.  The old test's half-line starts at the point and runs through the light, the new
    # one's starts at the light and runs through the point: different ends, one line.  Whatever the
    # old test rejects because the LINE misses the ball the new one must reject too, up to the
    # sliver between the two margins (kKeep shrinks |oc|^2 there and |cl|^2 here: 1e-5 relative,
    # 1 % of lanes is generous even for this silhouette-heavy sample); its front test adds more.
    assert rej_old > 100000
    assert rej_new >= 0.99 * rej_old, (rej_new, rej_old)


def test_unbounded_ball_passes_every_lane():
    rng = np.random.default_rng(6)
    ball = np.array([1.0, 2.0, 3.0, np.inf], F)
    light = np.array([-10, 10, -10], F)
    p = rng.uniform(-30, 30, (1000, 3)).astype(F)
    tl = (light - p).astype(F)
    tt = dot(tl, tl)
    assert from_light_may_hit(ball, light, tl, tt).all()
