"""Worlds and rays that sit exactly on the tracer's decision boundaries.

The random worlds and ray batches of the GPU suite come from continuous
distributions, where a direction component that is exactly 0, a ray in a
cube's face plane, a discriminant that is exactly 0, a cap hit on the rim, two
surfaces at one t or a light in a surface's plane have measure zero.  Here
every transformation is an integer translation, a power-of-two scaling or one
rotation_x(pi/2), every origin a lattice point and every direction one of a few
lattice directions, so those cases are the rule.

    lattice_world(pool, room_first)  tables() of the world below
    lattice_rays()                   (25200, 6) unit rays for color_at
    exact_rays()                     (n, 6) dyadic rays for debug_intersect
    CAMERAS                          (from, to, up) of the lattice frames

A plain helper module (no fixtures): tests/test_lattice_inputs.py checks on the
CPU that these inputs do sit on decisions, tests/test_gpu_lattice.py runs them
on the GPU.
"""
import itertools
import math

import numpy as np

# (from, to, up); 96x72, fov pi/2, depth 5
CAMERAS = [((0, 0, -6), (0, 0, 0), (0, 1, 0)),
           ((-4, 3, -5), (0, 1, 0), (0, 1, 0)),
           ((0, 8, 0), (0, 0, 0), (0, 0, 1))]
FRAME = (96, 72, math.pi / 2)
DEPTH = 5


def lattice_world(pool: bool, room_first: bool):
    """Ten shapes that touch, share faces or coincide, two lights (one in the
    plane of the cube tops), inside a room cube whose floor face coincides
    with the floor plane.  pool: reflective and transparent materials (the
    pool kernel's worlds); room_first: the room is the world's first shape
    instead of its last (coincident surfaces tie on t, and the tie goes by
    world order)."""
    from rtc_amd import world as W

    def mat(color, reflect=0.0, transparency=0.0, n=1.0, pattern=None, casts_shadow=True):
        m = W.Material(color=color, ambient=0.1, diffuse=0.7, specular=0.5, shininess=50.0, pattern=pattern,
                       casts_shadow=casts_shadow)
        if pool:
            m.reflectiveness, m.transparency, m.refractive_index = reflect, transparency, n
        return m

    shapes = [
        W.plane(mat((1, 1, 1), reflect=0.25, pattern=W.checker_pattern((.9, .9, .9), (.1, .1, .1))),
                W.translation(0, -1, 0)),
        W.cube(mat((.2, .3, .9), reflect=0.1, transparency=0.7, n=1.5)),
        W.cube(mat((.9, .3, .2), pattern=W.stripe_pattern((1, 0, 0), (0, 0, 1))), W.translation(2, 0, 0)),
        W.sphere(mat((.3, .9, .3), reflect=0.2, transparency=0.6, n=1.5), W.translation(0, 2, 0)),
        W.sphere(mat((.9, .9, .2), reflect=0.5), W.translation(0, 4, 0)),
        W.cylinder(-1, 1, True, mat((.5, .2, .7), pattern=W.ring_pattern((1, 1, 0), (0, 1, 1))),
                   W.translation(-2, 0, 0)),
        W.cone(-1, 0, True, mat((.2, .7, .7), transparency=0.5, n=1.3), W.translation(2, 2, 0)),
        W.triangle((1, -1, -1), (3, -1, -1), (2, 1, -1), mat((.8, .8, .8), reflect=0.3)),
        W.plane(mat((.4, .4, .4), casts_shadow=False), W.mat_mul(W.translation(0, 0, 3), W.rotation_x(math.pi / 2))),
    ]
    room = W.cube(mat((.6, .6, .7)), W.mat_mul(W.translation(0, 7, 0), W.scaling(8, 8, 8)))
    shapes = [room] + shapes if room_first else shapes + [room]
    lights = [W.Light((-3, 1, -4), (.7, .7, .7)), W.Light((0, 6, -6), (.4, .4, .5))]
    return W.World(lights, shapes).tables()


def _normalize(d):
    """vector.rs:84-91: each component / sqrt of the sum of squares."""
    d = np.asarray(d, dtype=np.float64)
    mag = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return d / mag[:, None]


def _signed_permutations(v):
    out = set()
    for p in itertools.permutations(v):
        for s in itertools.product((1.0, -1.0), repeat=3):
            out.add(tuple(a * b + 0.0 for a, b in zip(p, s)))  # + 0.0: -0.0 -> 0.0
    return sorted(out)


def lattice_directions():
    """The 50 directions: 6 axes, 24 of (0.6, 0.8, 0), 12 of (1, 1, 0), 8 of (1, 1, 1)."""
    d = (_signed_permutations((1.0, 0.0, 0.0)) + _signed_permutations((0.6, 0.8, 0.0))
         + _signed_permutations((1.0, 1.0, 0.0)) + _signed_permutations((1.0, 1.0, 1.0)))
    assert len(d) == 50
    return _normalize(d)


def lattice_rays():
    """504 integer origins (x -4..4, y -1..5, z -5..2) x 50 directions."""
    o = np.array(list(itertools.product(range(-4, 5), range(-1, 6), range(-5, 3))), dtype=np.float64)
    d = lattice_directions()
    rays = np.concatenate([np.repeat(o, len(d), axis=0), np.tile(d, (len(o), 1))], axis=1)
    assert rays.shape == (25200, 6)
    return rays


def exact_rays():
    """Half-integer origins (x, y -2..2, z -3..-1) x every non-zero direction
    with components in {0, +-0.5, +-1, +-2}, not normalised: every input, and
    every product, sum and reciprocal the per-shape tests form from them
    before a square root, is a small dyadic number, exact in f32 as in f64."""
    h = lambda lo, hi: [k / 2.0 for k in range(2 * lo, 2 * hi + 1)]  # noqa: E731
    o = np.array(list(itertools.product(h(-2, 2), h(-2, 2), h(-3, -1))), dtype=np.float64)
    c = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
    d = np.array([v for v in itertools.product(c, repeat=3) if any(v)], dtype=np.float64)
    return np.concatenate([np.repeat(o, len(d), axis=0), np.tile(d, (len(o), 1))], axis=1)
