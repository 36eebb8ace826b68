"""A numpy f64 restatement of the smooth triangle's semantics (rtc.h
rt_scene_upload_smooth), the check of the kernels where the
oracle has nothing to say: opaque, unpatterned worlds of triangles (flat or
smooth) under point lights, one colour per ray.

  intersection   Triangle::local_intersect (triangle.rs:39-56) in its operation
                 order: dce2 = d x e2, det = e1 . dce2, u = (o - v1) . dce2 /
                 det, oce1 = (o - v1) x e1, v = d . oce1 / det, t = e2 . oce1 /
                 det; cross and dot with the reference's mul_add (vector.rs:
                 93-103), emulated below;
  hit            the first minimum t >= 0 in (t, world order);
  local normal   n2 u + n3 v + n1 (1 - u - v), left to right, plain products
                 and sums, with the u and v of the test; a flat triangle's own;
  world normal   normalize(inverse^T ln) (shape.rs:22-27), flipped when
                 n . eye < 0;
  over_point     p + n EPSILON, EPSILON = 8e-8;
  is_in_shadow   over every triangle whose material casts a shadow, an entry
                 with 0 <= t < distance (world.rs:98-112);
  lighting       calculate_lighting (material.rs:83-114) at the over point.

Besides the colours, trace() returns per ray the smallest distance of det, u,
v and u + v from the thresholds the accept decision compares them with
(|det| against EPSILON, u against 0 and 1, v against 0, u + v against 1) over
all triangles and over the primary and the shadow rays: a test that asserts it
above its tolerance knows no decision sat on the fence.

mul_add: numpy has no fused multiply-add.  fma() forms the product's rounding
error exactly (Veltkamp split, Dekker product) and the sum's (Knuth two-sum),
and adds the errors to the rounded sum: the correctly rounded result except in
rare double-rounding cases, where it is one ulp off (1e-16 relative: seven
orders below the tests' 1e-9).
"""
import numpy as np

EPSILON = 8e-8


def _split(a):
    c = 134217729.0 * a  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl  # a b = p + e exactly
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # p + c = s + err exactly
    return s + (err + e)


def dot(a, b):  # vector.rs:93-95
    return fma(a[..., 2], b[..., 2], fma(a[..., 0], b[..., 0], a[..., 1] * b[..., 1]))


def cross(a, b):  # vector.rs:97-103
    return np.stack([fma(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])),
                     fma(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     fma(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], axis=-1)


def normalized(v):  # vector.rs:84-91
    mag = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    return v / mag[..., None]


def magnitude(v):
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def mul_point(m, p):  # matrix.rs:332-346: per row a left fold from 0.0 over (x, y, z, 1)
    return np.stack([(((0.0 + m[..., r, 0] * p[..., 0]) + m[..., r, 1] * p[..., 1]) + m[..., r, 2] * p[..., 2]) +
                     m[..., r, 3] for r in range(3)], axis=-1)


def mul_vector(m, v):  # matrix.rs:348-362 (w = 0)
    return np.stack([((0.0 + m[..., r, 0] * v[..., 0]) + m[..., r, 1] * v[..., 1]) + m[..., r, 2] * v[..., 2]
                     for r in range(3)], axis=-1)


def mul_normal(m, n):  # transpose(inverse) * n (shape.rs:25), the 3 x 3 part
    return np.stack([((0.0 + m[..., 0, r] * n[..., 0]) + m[..., 1, r] * n[..., 1]) + m[..., 2, r] * n[..., 2]
                     for r in range(3)], axis=-1)


class Triangles:
    """The triangles of a world in world order, from SceneTables (shapes that are all triangles, or the
    triangles among them when `only_triangles`), its smooth list (entries with RT_SMOOTH_SHAPES) and materials."""

    def __init__(self, tables):
        sh = tables.shapes
        assert all(s.kind == 5 for s in sh), "the reference speaks for worlds of triangles"
        n = len(sh)
        self.inv = np.array([list(s.inverse) for s in sh], dtype=np.float64).reshape(n, 4, 4)
        self.v1 = np.array([list(s.vertex_1) for s in sh], dtype=np.float64)
        self.e1 = np.array([list(s.edge_1) for s in sh], dtype=np.float64)
        self.e2 = np.array([list(s.edge_2) for s in sh], dtype=np.float64)
        self.flat = np.array([list(s.normal) for s in sh], dtype=np.float64)
        self.smooth = np.zeros(n, dtype=bool)
        self.n1, self.n2, self.n3 = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        for e in (tables.smooth if tables.smooth is not None else []):
            assert e.list == 0xFFFFFFFF, "expand the tables first"
            self.smooth[e.index] = True
            self.n1[e.index], self.n2[e.index], self.n3[e.index] = list(e.normal_1), list(e.normal_2), list(e.normal_3)
        mats = [tables.materials[s.material] for s in sh]
        assert all(m.pattern < 0 and m.reflectiveness == 0.0 and m.transparency == 0.0 for m in mats)
        self.color = np.array([list(m.color) for m in mats], dtype=np.float64)
        self.ambient = np.array([m.ambient for m in mats])
        self.diffuse = np.array([m.diffuse for m in mats])
        self.specular = np.array([m.specular for m in mats])
        self.shininess = np.array([m.shininess for m in mats])
        self.casts = np.array([m.casts_shadow != 0 for m in mats])
        self.lights = [(np.array(list(lt.position)), np.array(list(lt.intensity))) for lt in tables.lights]


def intersect(tri, o, d):
    """Every ray (r, 3) against every triangle: t, u, v, valid (r, n) and the rays' decision margin (r,)."""
    lo = mul_point(tri.inv[None], o[:, None, :])
    ld = mul_vector(tri.inv[None], d[:, None, :])
    e1, e2, v1 = tri.e1[None], tri.e2[None], tri.v1[None]
    with np.errstate(all="ignore"):
        dce2 = cross(ld, np.broadcast_to(e2, ld.shape))
        det = dot(np.broadcast_to(e1, ld.shape), dce2)
        v1o = lo - v1
        u = dot(v1o, dce2) / det
        oce1 = cross(v1o, np.broadcast_to(e1, ld.shape))
        v = dot(ld, oce1) / det
        t = dot(np.broadcast_to(e2, ld.shape), oce1) / det
        ok_det = ~(np.abs(det) < EPSILON)
        ok_u = (u >= 0.0) & (u <= 1.0)
        valid = ok_det & ok_u & (v > 0.0) & (u + v < 1.0)
        # how far each compared value is from its threshold; a test further down the reference's early
        # returns only counts where the ones before it passed (it is not evaluated otherwise)
        big = np.full(det.shape, np.inf)
        m = np.abs(np.abs(det) - EPSILON)
        m = np.minimum(m, np.where(ok_det, np.minimum(np.abs(u), np.abs(u - 1.0)), big))
        m = np.minimum(m, np.where(ok_det & ok_u, np.minimum(np.abs(v), np.abs(u + v - 1.0)), big))
        m = np.where(np.isnan(m), 0.0, m)
    return t, u, v, valid, m.min(axis=1)


def first_hit(t, valid):
    """Index of the first minimum t >= 0 over valid entries per ray (-1: none) and that t."""
    key = np.where(valid & (t >= 0.0), t, np.inf)
    idx = np.argmin(key, axis=1)  # the first minimum: the lowest world index at equal t
    best = key[np.arange(len(idx)), idx]
    return np.where(np.isfinite(best), idx, -1), best


def trace(tables, rays):
    """Colours (r, 3), the primary hits' (t, shape, u, v) and the smallest decision margin per ray."""
    tri = Triangles(tables)
    rays = np.asarray(rays, dtype=np.float64)
    o, d = rays[:, :3], rays[:, 3:]
    t, u, v, valid, margin = intersect(tri, o, d)
    hit, th = first_hit(t, valid)
    rgb = np.zeros((len(rays), 3))
    rows = np.nonzero(hit >= 0)[0]
    hu, hv = np.zeros(len(rays)), np.zeros(len(rays))
    if len(rows):
        k = hit[rows]
        uu, vv = u[rows, k], v[rows, k]
        hu[rows], hv[rows] = uu, vv
        oo, dd, tt = o[rows], d[rows], th[rows]
        p = oo + dd * tt[:, None]
        w = (1.0 - uu) - vv
        ln = (tri.n2[k] * uu[:, None] + tri.n3[k] * vv[:, None]) + tri.n1[k] * w[:, None]
        ln = np.where(tri.smooth[k][:, None], ln, tri.flat[k])
        n = normalized(mul_normal(tri.inv[k], ln))
        eye = -dd
        n = np.where((dot(n, eye) < 0.0)[:, None], -n, n)
        over = p + n * EPSILON
        colour = np.zeros((len(rows), 3))
        for lpos, lint in tri.lights:
            to_light = lpos[None] - over
            dist = magnitude(to_light)
            ldir = normalized(to_light)
            st, _, _, sv, sm = intersect(tri, over, ldir)
            margin[rows] = np.minimum(margin[rows], sm)
            blocked = (sv & tri.casts[None] & (st >= 0.0) & (st < dist[:, None])).any(axis=1)
            eff = tri.color[k] * lint[None]
            c = eff * tri.ambient[k][:, None]
            ldn = dot(ldir, n)
            lit = ~blocked & ~(ldn < 0.0)
            diffuse = eff * tri.diffuse[k][:, None] * ldn[:, None]
            neg = -ldir
            refl = neg - (n * 2.0) * dot(neg, n)[:, None]  # vector.rs:105-107
            rde = dot(refl, eye)
            with np.errstate(all="ignore"):
                factor = np.where(rde > 0.0, np.power(np.where(rde > 0.0, rde, 1.0), tri.shininess[k]), 0.0)
            spec = lint[None] * tri.specular[k][:, None] * factor[:, None]
            c = c + np.where(lit[:, None], diffuse, 0.0)
            c = c + np.where((lit & (rde > 0.0))[:, None], spec, 0.0)
            colour = colour + c
        rgb[rows] = colour
    return rgb, {"t": th, "shape": hit, "u": hu, "v": hv}, margin


def known_answer():
    """The book's smooth-triangle answer (chapter 15): the triangle, the ray, u, v and the unit normal."""
    p = ((0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0))
    n = ((0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0))
    ray = (-0.2, 0.3, -2.0, 0.0, 0.0, 1.0)
    want = np.array([-0.2, 0.3, 0.0]) / np.sqrt(0.2 * 0.2 + 0.3 * 0.3)
    return p, n, ray, 0.45, 0.25, want
