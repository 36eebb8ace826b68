"""A numpy f64 restatement of the image texture's semantics (rtc.h
rt_scene_upload_textured) on smooth_reference's helpers: opaque
worlds of triangles (flat or smooth, with or without texture coordinates) under
point lights, one colour per ray.

  (u, v)     a triangle with coordinates: t2 u_b + t3 v_b + t1 (1 - u_b - v_b)
             per component, left to right, plain products and sums, with the
             u_b and v_b of the accepted hit; a component outside [0, 1] is
             wrapped by c - floor(c).  Any other hit: pp = pattern.inverse *
             (shape.inverse * over_point), u = pp.x - floor(pp.x), v = pp.z -
             floor(pp.z);
  sampling   x = u (w - 1), y = (1 - v) (h - 1); nearest: floor(x) + (x -
             floor(x) >= 0.5), the same for y; bilinear: (c00 (1 - fx) + c10 fx)
             (1 - fy) + (c01 (1 - fx) + c11 fx) fy; a texel is byte / 255.0.

trace() returns what smooth_reference.trace returns; its margin also takes in
the distance of x - floor(x) and y - floor(y) from 0.5 under the nearest filter
(where the texel changes), of every interpolated component from 0 and 1 (where
wrapping begins) and of every wrapped or planar-mapped component from the
nearest whole number (where floor jumps).
"""
import numpy as np

import smooth_reference as R

IMAGE, NEAREST, BILINEAR = 6, 0, 1


def sample(image, filt, u, v):
    """Colours (n, 3) of the texture at (u, v) in [0, 1], and per sample the distance of a nearest-filter
    decision from its threshold (inf for the bilinear filter)."""
    img = np.asarray(image)
    h, w = img.shape[:2]
    tex = img.astype(np.float64) / 255.0
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    x, y = u * (w - 1.0), (1.0 - v) * (h - 1.0)
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = x - xf, y - yf
    x0 = np.clip(xf.astype(np.int64), 0, w - 1)
    y0 = np.clip(yf.astype(np.int64), 0, h - 1)
    if filt == NEAREST:
        xi = np.minimum(x0 + (fx >= 0.5), w - 1)
        yi = np.minimum(y0 + (fy >= 0.5), h - 1)
        margin = np.minimum(np.abs(fx - 0.5) if w > 1 else np.inf, np.abs(fy - 0.5) if h > 1 else np.inf)
        return tex[yi, xi], np.broadcast_to(margin, u.shape)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    c00, c10, c01, c11 = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
    fx, fy = fx[:, None], fy[:, None]
    gx, gy = 1.0 - fx, 1.0 - fy
    return (c00 * gx + c10 * fx) * gy + (c01 * gx + c11 * fx) * fy, np.full(u.shape, np.inf)


def wrap(c):
    """A coordinate component as the kernels use it, and its distance from where that decision changes."""
    inside = (c >= 0.0) & (c <= 1.0)
    out = np.where(inside, c, c - np.floor(c))
    margin = np.minimum(np.abs(c), np.abs(c - 1.0))
    margin = np.where(inside, margin, np.minimum(margin, np.abs(c - np.round(c))))
    return out, margin


def uv_pattern_at(image, u, v, filt=NEAREST):
    """The book's uv_pattern_at for an image (one point)."""
    return sample(image, filt, np.array([u]), np.array([v]))[0][0]


def planar_map(p):
    """The book's planar map of a point: (u, v) = (x mod 1, z mod 1)."""
    p = np.asarray(p, np.float64)
    return p[..., 0] - np.floor(p[..., 0]), p[..., 2] - np.floor(p[..., 2])


class _Unpatterned:
    """The tables as smooth_reference.Triangles reads them, with every material's pattern taken off."""

    def __init__(self, tables):
        self.shapes, self.smooth, self.lights = tables.shapes, tables.smooth, tables.lights
        self.materials = type(tables.materials).from_buffer_copy(tables.materials)
        for m in self.materials:
            m.pattern = -1


def trace(tables, rays):
    """Colours (r, 3), the primary hits' (t, shape, u, v: the barycentric values) and the decision margin."""
    tri = R.Triangles(_Unpatterned(tables))
    n = len(tables.shapes)
    has_uv = np.zeros(n, dtype=bool)
    t1, t2, t3 = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    for e in (tables.uvs if tables.uvs is not None else []):
        assert e.list == 0xFFFFFFFF, "expand the tables first"
        has_uv[e.index] = True
        t1[e.index], t2[e.index], t3[e.index] = list(e.uv_1), list(e.uv_2), list(e.uv_3)
    pattern = np.array([tables.materials[s.material].pattern for s in tables.shapes])
    for p in set(pattern.tolist()) - {-1}:
        assert tables.patterns[p].kind == IMAGE, "the reference speaks for image patterns only"
    rays = np.asarray(rays, dtype=np.float64)
    o, d = rays[:, :3], rays[:, 3:]
    t, u, v, valid, margin = R.intersect(tri, o, d)
    hit, th = R.first_hit(t, valid)
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
        nrm = R.normalized(R.mul_normal(tri.inv[k], ln))
        eye = -dd
        nrm = np.where((R.dot(nrm, eye) < 0.0)[:, None], -nrm, nrm)
        over = p + nrm * R.EPSILON
        # the base colour: the material's, or the texture's at the hit's (u, v)
        base = tri.color[k].copy()
        tmargin = np.full(len(rows), np.inf)
        for pid in set(pattern[k].tolist()) - {-1}:
            pd = tables.patterns[pid]
            sel = np.nonzero(pattern[k] == pid)[0]
            ks = k[sel]
            tc = (t2[ks] * uu[sel, None] + t3[ks] * vv[sel, None]) + t1[ks] * w[sel, None]
            cu, mu = wrap(tc[:, 0])
            cv, mv = wrap(tc[:, 1])
            pinv = np.array(list(pd.inverse), dtype=np.float64).reshape(4, 4)
            pp = R.mul_point(pinv[None], R.mul_point(tri.inv[ks], over[sel]))
            pu, pv = planar_map(pp)
            pm = np.minimum(np.abs(pp[:, 0] - np.round(pp[:, 0])), np.abs(pp[:, 2] - np.round(pp[:, 2])))
            mapped = has_uv[ks]
            su, sv = np.where(mapped, cu, pu), np.where(mapped, cv, pv)
            colour, sm = sample(tables.textures[pd.sub_a], pd.reserved, su, sv)
            base[sel] = colour
            tmargin[sel] = np.minimum(sm, np.where(mapped, np.minimum(mu, mv), pm))
        margin[rows] = np.minimum(margin[rows], tmargin)
        colour = np.zeros((len(rows), 3))
        for lpos, lint in tri.lights:
            to_light = lpos[None] - over
            dist = R.magnitude(to_light)
            ldir = R.normalized(to_light)
            st, _, _, sv_, sm = R.intersect(tri, over, ldir)
            margin[rows] = np.minimum(margin[rows], sm)
            blocked = (sv_ & tri.casts[None] & (st >= 0.0) & (st < dist[:, None])).any(axis=1)
            eff = base * lint[None]
            c = eff * tri.ambient[k][:, None]
            ldn = R.dot(ldir, nrm)
            lit = ~blocked & ~(ldn < 0.0)
            diffuse = eff * tri.diffuse[k][:, None] * ldn[:, None]
            neg = -ldir
            refl = neg - (nrm * 2.0) * R.dot(neg, nrm)[:, None]
            rde = R.dot(refl, eye)
            with np.errstate(all="ignore"):
                factor = np.where(rde > 0.0, np.power(np.where(rde > 0.0, rde, 1.0), tri.shininess[k]), 0.0)
            spec = lint[None] * tri.specular[k][:, None] * factor[:, None]
            c = c + np.where(lit[:, None], diffuse, 0.0)
            c = c + np.where((lit & (rde > 0.0))[:, None], spec, 0.0)
            colour = colour + c
        rgb[rows] = colour
    return rgb, {"t": th, "shape": hit, "u": hu, "v": hv}, margin


# The book's known answers ("Texture mapping"): the 10 x 2 PPM of its uv_image scenario, whose pixels it lists
# as rows of grey levels and colours, and its planar-map table.
BOOK_PPM = """P3
10 10
10
0 0 0  1 1 1  2 2 2  3 3 3  4 4 4  5 5 5  6 6 6  7 7 7  8 8 8  9 9 9
1 1 1  2 2 2  3 3 3  4 4 4  5 5 5  6 6 6  7 7 7  8 8 8  9 9 9  0 0 0
2 2 2  3 3 3  4 4 4  5 5 5  6 6 6  7 7 7  8 8 8  9 9 9  0 0 0  1 1 1
3 3 3  4 4 4  5 5 5  6 6 6  7 7 7  8 8 8  9 9 9  0 0 0  1 1 1  2 2 2
4 4 4  5 5 5  6 6 6  7 7 7  8 8 8  9 9 9  0 0 0  1 1 1  2 2 2  3 3 3
5 5 5  6 6 6  7 7 7  8 8 8  9 9 9  0 0 0  1 1 1  2 2 2  3 3 3  4 4 4
6 6 6  7 7 7  8 8 8  9 9 9  0 0 0  1 1 1  2 2 2  3 3 3  4 4 4  5 5 5
7 7 7  8 8 8  9 9 9  0 0 0  1 1 1  2 2 2  3 3 3  4 4 4  5 5 5  6 6 6
8 8 8  9 9 9  0 0 0  1 1 1  2 2 2  3 3 3  4 4 4  5 5 5  6 6 6  7 7 7
9 9 9  0 0 0  1 1 1  2 2 2  3 3 3  4 4 4  5 5 5  6 6 6  7 7 7  8 8 8
"""
# (u, v) -> the grey level / 10 the book expects of uv_pattern_at on that image
BOOK_UV_ANSWERS = [((0.0, 0.0), 0.9), ((0.3, 0.0), 0.2), ((0.6, 0.3), 0.1), ((1.0, 1.0), 0.9)]
# point -> (u, v) of the book's planar mapping table
BOOK_PLANAR = [((0.25, 0.0, 0.5), (0.25, 0.5)), ((0.25, 0.0, -0.25), (0.25, 0.75)), ((0.25, 0.5, -0.25), (0.25, 0.75)),
               ((1.25, 0.0, 0.5), (0.25, 0.5)), ((0.25, 0.0, -1.75), (0.25, 0.25)), ((1.0, 0.0, -1.0), (0.0, 0.0)),
               ((0.0, 0.0, 0.0), (0.0, 0.0))]
