"""A numpy f64 restatement of the texture maps (rtc.h rt_scene_upload_mapped,
DESIGN.md 3.16) next to texture_reference, whose `sample` it reuses.

For a hit without texture coordinates, pp = pattern.inverse * (shape.inverse *
over_point):

  spherical    theta = atan2(pp.x, pp.z), r = sqrt((x^2 + y^2) + z^2),
               c = clamp(pp.y / r, -1, 1), phi = acos(c),
               u = 1 - (theta / (2 pi) + 0.5), v = 1 - phi / pi;
  cylindrical  u as above, v = pp.y - floor(pp.y);
  cube         a = max(|x|, |y|, |z|); the first true of a == x: right, a == -x:
               left, a == y: up, a == -y: down, a == z: front, else back; with
               m(c) = c - 2 floor(c / 2) the table of rtc.h, halved.

map_uv() returns (u, v, face, margin).  The margin of a point is its distance
from where a decision of the map changes: the seam theta = +-pi (in units of
u), a tie between two faces (|x| = |y| and the like), a jump of floor.
colour() adds the nearest filter's 0.5 thresholds (texture_reference.sample).
designed_rays() gives the rays of tests/test_gpu_uv_maps.py and the over points
the f64 kernel forms for them, shape by shape.
"""
import numpy as np

import texture_reference as T

PLANAR, SPHERICAL, CYLINDRICAL, CUBE = 0, 1, 2, 3
LEFT, FRONT, RIGHT, BACK, UP, DOWN = range(6)
FACE_NAMES = ("left", "front", "right", "back", "up", "down")
EPSILON = 0.00000008  # the f64 kernels' over-point offset


def _u_of_theta(x, z):
    theta = np.arctan2(x, z)
    u = 1.0 - (theta / (2.0 * np.pi) + 0.5)
    return u, (np.pi - np.abs(theta)) / (2.0 * np.pi)


def _mod2(c):
    """m(c) / 2 and the distance of c from the next jump of floor(c / 2)."""
    h = c / 2.0
    return (c - 2.0 * np.floor(h)) / 2.0, 2.0 * np.abs(h - np.round(h))


def cube_face(pp):
    """The face of each point (LEFT .. DOWN) and the gap between the largest and the second largest of |x|, |y|, |z|."""
    pp = np.asarray(pp, np.float64).reshape(-1, 3)
    x, y, z = pp[:, 0], pp[:, 1], pp[:, 2]
    ab = np.abs(pp)
    a = np.maximum(np.maximum(ab[:, 0], ab[:, 1]), ab[:, 2])
    face = np.select([a == x, a == -x, a == y, a == -y, a == z], [RIGHT, LEFT, UP, DOWN, FRONT], BACK)
    top2 = np.sort(ab, axis=1)
    return face, top2[:, 2] - top2[:, 1]


def map_uv(kind, pp):
    """(u, v, face, margin) of the pattern-space points `pp` (n, 3) under map `kind`; face is -1 but for a cube map."""
    pp = np.asarray(pp, np.float64).reshape(-1, 3)
    x, y, z = pp[:, 0], pp[:, 1], pp[:, 2]
    none = np.full(len(pp), -1)
    if kind == PLANAR:
        u, v = T.planar_map(pp)
        return u, v, none, np.minimum(np.abs(x - np.round(x)), np.abs(z - np.round(z)))
    if kind == SPHERICAL:
        u, seam = _u_of_theta(x, z)
        r = np.sqrt((x * x + y * y) + z * z)
        with np.errstate(divide="ignore", invalid="ignore"):  # (r = 0: the kernels divide too, and clamp)
            c = np.clip(y / r, -1.0, 1.0)
        return u, 1.0 - np.arccos(c) / np.pi, none, seam
    if kind == CYLINDRICAL:
        u, seam = _u_of_theta(x, z)
        return u, y - np.floor(y), none, np.minimum(seam, np.abs(y - np.round(y)))
    assert kind == CUBE
    face, tie = cube_face(pp)
    one = np.ones_like(x)
    cu = np.select([face == FRONT, face == BACK, face == LEFT, face == RIGHT], [x + one, one - x, z + one, one - z], x + one)
    cv = np.select([face == UP, face == DOWN], [one - z, z + one], y + one)
    (u, ju), (v, jv) = _mod2(cu), _mod2(cv)
    return u, v, face, np.minimum(tie, np.minimum(ju, jv))


def colour(kind, images, filt, pp):
    """The colour of each point: `images` is one texture, or for a cube map the six in the order left .. down.
    Returns (rgb (n, 3), margin)."""
    u, v, face, margin = map_uv(kind, pp)
    if kind != CUBE:
        rgb, sm = T.sample(images, filt, u, v)
        return rgb, np.minimum(margin, sm)
    rgb = np.zeros((len(u), 3))
    for f in range(6):
        sel = np.nonzero(face == f)[0]
        if len(sel):
            c, sm = T.sample(images[f], filt, u[sel], v[sel])
            rgb[sel] = c
            margin[sel] = np.minimum(margin[sel], sm)
    return rgb, margin


def mul_point(m, p):
    """A 4 x 4 matrix (nested lists or array) times points (n, 3), rows 0..2, left to right as the kernels sum."""
    m = np.asarray(m, np.float64).reshape(4, 4)
    return np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], axis=1)


def surface_points(shape, n, seed):
    """`n` seeded points of the unit sphere, of the side of the unit cylinder (|y| < 1) or of the unit cube's six
    faces, with the outward normal of each."""
    rng = np.random.default_rng(seed)
    if shape == "sphere":
        p = rng.normal(size=(n, 3))
        p /= np.linalg.norm(p, axis=1)[:, None]
        return p, p.copy()
    if shape == "cylinder":
        phi, y = rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.98, 0.98, n)
        p = np.stack([np.cos(phi), y, np.sin(phi)], axis=1)
        nrm = p.copy()
        nrm[:, 1] = 0.0
        return p, nrm
    assert shape == "cube"
    p = rng.uniform(-0.98, 0.98, size=(n, 3))
    axis, sign = rng.integers(0, 3, n), rng.choice([-1.0, 1.0], n)
    p[np.arange(n), axis] = sign
    nrm = np.zeros((n, 3))
    nrm[np.arange(n), axis] = sign
    return p, nrm


def designed_rays(shape, n, seed):
    """Rays from 2 p along -p at `n` surface points p of the unit `shape` at the origin (rows of origin,
    direction), and the over points of their hits: p + normal * EPSILON."""
    p, nrm = surface_points(shape, n, seed)
    d = -p / np.linalg.norm(p, axis=1)[:, None]
    rays = np.ascontiguousarray(np.concatenate([2.0 * p, d], axis=1))
    return rays, p + nrm * EPSILON


# The book's tables ("Texture mapping").
S2 = np.sqrt(2.0) / 2.0
BOOK_SPHERICAL = [((0, 0, -1), (0.0, 0.5)), ((1, 0, 0), (0.25, 0.5)), ((0, 0, 1), (0.5, 0.5)), ((-1, 0, 0), (0.75, 0.5)),
                  ((0, 1, 0), (0.5, 1.0)), ((0, -1, 0), (0.5, 0.0)), ((S2, S2, 0), (0.25, 0.75))]
BOOK_CYLINDRICAL = [((0, 0, -1), (0.0, 0.0)), ((0, 0.5, -1), (0.0, 0.5)), ((0, 1, -1), (0.0, 0.0)),
                    ((0.70711, 0.5, -0.70711), (0.125, 0.5)), ((1, 0.5, 0), (0.25, 0.5)), ((0.70711, 0.5, 0.70711), (0.375, 0.5)),
                    ((0, -0.25, 1), (0.5, 0.75)), ((-0.70711, 0.5, 0.70711), (0.625, 0.5)), ((-1, 1.25, 0), (0.75, 0.25)),
                    ((-0.70711, 0.5, -0.70711), (0.875, 0.5))]
BOOK_FACES = [((-1, 0.5, -0.25), LEFT), ((1.1, -0.75, 0.8), RIGHT), ((0.1, 0.6, 0.9), FRONT), ((-0.7, 0, -2), BACK),
              ((0.5, 1, 0.9), UP), ((-0.2, -1.3, 1.1), DOWN)]
BOOK_CUBE = [(FRONT, (-0.5, 0.5, 1), (0.25, 0.75)), (FRONT, (0.5, -0.5, 1), (0.75, 0.25)),
             (BACK, (0.5, 0.5, -1), (0.25, 0.75)), (BACK, (-0.5, -0.5, -1), (0.75, 0.25)),
             (LEFT, (-1, 0.5, -0.5), (0.25, 0.75)), (LEFT, (-1, -0.5, 0.5), (0.75, 0.25)),
             (RIGHT, (1, 0.5, 0.5), (0.25, 0.75)), (RIGHT, (1, -0.5, -0.5), (0.75, 0.25)),
             (UP, (-0.5, 1, -0.5), (0.25, 0.75)), (UP, (0.5, 1, 0.5), (0.75, 0.25)),
             (DOWN, (-0.5, -1, 0.5), (0.25, 0.75)), (DOWN, (0.5, -1, -0.5), (0.75, 0.25))]
