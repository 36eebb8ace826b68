"""Worlds of the motion tests (tests/test_motion_cpu.py, tests/test_gpu_motion.py).

Each world is built to break one consumer of a shape's world position if that consumer looks at the static
position (the position at tau = 0) instead of the displaced one:

  far(kind)      a small mover (sphere, cube, closed cylinder, lone triangle, instanced octahedron) that
                 crosses 6.6 units during the shutter [0, 1], more than 8 times its ball's radius, and is in
                 front of the camera only for the last third: a cull on the static ball loses it;
  shadow()       a static floor and a moving caster above the frame: only shadow rays meet it;
  plane()        a wall that crosses the light's side during the shutter: the plane-side skip;
  glass()        a glass sphere moving through a static glass cube, and two value-equal movers of different
                 velocity: the containers walk and the identity classes (the pool kernel, depth 5);
  pattern()      a striped mover and a spherically mapped mover: the pattern travels with the shape.  The
                 oracle samples no images, so the map's texture is the 2 x 1 texture [a b] under the nearest
                 filter, which coincides with the oracle's stripe_pattern(a, b) away from the plane x = 0
                 (tests/uv_map_worlds.py tie()): pattern(mapped=False) is the oracle's world;
  maps()         a unit cylinder under the cylindrical map and a unit cube under a cube map, both scaled, turned
                 about y and moving: the maps' points travel with their shapes too.  The textures are
                 tests/uv_map_worlds.py tie()'s, which coincide with the oracle's stripe_pattern(a, b) away from
                 the planes x = 0 and x = +-1 of the shape's own space; maps(mapped=False) is the oracle's world;
  area()         a mover under an area light: the light-level caster cull;
  tree()         72 static top-level triangles, enough for a triangle hierarchy, with a moving triangle that
                 must stay outside it, and two instances of one mesh with one placement and one material (a
                 value-equal pair, uploaded expanded) of which one moves: its plain records carry the velocity.

The f32 world-space paths are far("sphere") (a similarity sphere) and far("cube") (an axis-aligned cube).

glass(): at tau = 0 exactly the twins coincide, and the displaced static world, whose twins are then
value-equal, toggles one container entry for both, while the moving world keeps two classes at every time
(rtc.h: equal velocities are part of value equality).  The rays aimed at the twins therefore take their
times from TIMES without 0; every other ray of that world keeps all five.

Every world comes with `targets(tau)`: points (centre, reach) on or in its shapes at time tau that the ray
batches aim at, away from silhouettes by construction (a ray through a point within `reach` of the centre
of a ball of twice that radius meets it well inside its outline).
"""
import functools

import numpy as np

import rtc_amd
from rtc_amd import world as W

TIMES = (0.0, 0.25, 0.5, 0.75, 1.0)
N_RAYS = 2048
EYE = (0.0, 1.0, -5.0)
FAR_KINDS = ("sphere", "cube", "cylinder", "triangle", "instance")
V_FAR = (6.6, 0.0, 0.0)
X0 = -6.0  # the far mover's x at tau = 0: outside the frame until tau = 0.6

OCTAHEDRON = """v 1 0 0
v -1 0 0
v 0 1 0
v 0 -1 0
v 0 0 1
v 0 0 -1
f 1 3 5
f 3 2 5
f 2 4 5
f 4 1 5
f 3 1 6
f 2 3 6
f 4 2 6
f 1 4 6
"""


@functools.lru_cache(maxsize=None)
def octahedron():
    return rtc_amd.load_obj(OCTAHEDRON)


def camera(width=70, height=22):
    return W.camera(width, height, 0.8, EYE, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0))


def _floor():
    return W.plane(W.Material(pattern=W.checker_pattern((0.9, 0.9, 0.9), (0.2, 0.3, 0.4)), specular=0.0))


def _light():
    return W.Light((-3.0, 6.0, -6.0), (1.0, 1.0, 1.0))


def _tables(world):
    return world.tables(camera())


def _moving(centre0, v, reach):
    return lambda tau: (tuple(c + q * tau for c, q in zip(centre0, v)), reach)


def _still(centre, reach):
    return lambda tau: (centre, reach)


def _twin(target):
    """A target whose rays avoid tau = 0 (glass(), above)."""
    target.no_zero = True
    return target


def far(kind):
    """A mover of `kind`, of size 0.4, at (X0 + 6.6 tau, 1, 0)."""
    mat = W.Material(color=(0.9, 0.3, 0.2), specular=0.3)
    place = W.mat_mul(W.translation(X0, 1.0, 0.0), W.mat_mul(W.rotation_y(0.3), W.scaling(0.4, 0.4, 0.4)))
    world = W.World([_light()], [_floor()])
    if kind == "sphere":
        s = W.sphere(mat, W.mat_mul(W.translation(X0, 1.0, 0.0), W.scaling(0.4, 0.4, 0.4)))  # a similarity
    elif kind == "cube":
        s = W.cube(mat, W.mat_mul(W.translation(X0, 1.0, 0.0), W.scaling(0.4, 0.3, 0.35)))  # axis-aligned
    elif kind == "cylinder":
        s = W.cylinder(-1.0, 1.0, True, mat, place)
    elif kind == "triangle":
        s = W.triangle((X0 - 0.5, 0.6, 0.1), (X0 + 0.5, 0.6, -0.1), (X0, 1.6, 0.0), mat)
    else:
        s = None
        it = W.instance(octahedron(), mat, place)
        it.velocity = V_FAR
        world.instances.append(it)
    if s is not None:
        s.velocity = V_FAR
        world.shapes.append(s)
    # a static sphere beside the path, so that every batch has static hits too
    world.shapes.append(W.sphere(W.Material(color=(0.2, 0.5, 0.9)), W.mat_mul(W.translation(1.5, 0.5, 1.5), W.scaling(0.5, 0.5, 0.5))))
    reach = 0.08 if kind in ("triangle", "instance") else 0.15
    return _tables(world), [_moving((X0, 1.0, 0.0), V_FAR, reach), _still((1.5, 0.5, 1.5), 0.2), _still((0.3, 0.0, 0.7), 1.5)]


def shadow():
    """A caster above the frame (y = 4) that passes between the light and the floor in front of the camera."""
    world = W.World([W.Light((0.0, 8.0, 0.0), (1.0, 1.0, 1.0))], [_floor()])
    s = W.sphere(W.Material(), W.mat_mul(W.translation(-3.0, 4.0, 0.0), W.scaling(0.8, 0.8, 0.8)))
    s.velocity = (6.0, 0.0, 0.5)
    world.shapes.append(s)
    return _tables(world), [_still((0.2, 0.0, 0.6), 1.8)]


def plane():
    """A wall facing -x at x = -2 + 4 tau: the light (x = -0.3, on no sample's wall) changes its side of it
    during the shutter."""
    world = W.World([W.Light((-0.3, 3.0, -3.0), (1.0, 1.0, 1.0))], [_floor()])
    wall = W.plane(W.Material(color=(0.8, 0.7, 0.2), specular=0.0), W.mat_mul(W.translation(-2.0, 0.0, 0.0), W.rotation_z(np.pi / 2)))
    wall.velocity = (4.0, 0.0, 0.0)
    world.shapes.append(wall)
    world.shapes.append(W.sphere(W.Material(color=(0.3, 0.8, 0.4)), W.mat_mul(W.translation(-1.0, 0.6, 0.5), W.scaling(0.6, 0.6, 0.6))))
    return _tables(world), [_still((0.1, 0.0, 0.4), 1.6), _still((-1.0, 0.6, 0.5), 0.25), _still((0.3, 1.2, 0.0), 0.9)]


def _glass(**kw):
    return W.Material(color=(0.1, 0.1, 0.15), diffuse=0.2, ambient=0.05, reflectiveness=0.5, transparency=0.85, **kw)


def glass(twins=True):
    """A glass sphere (index 1.5) moving through a static glass cube (index 1.2), and two value-equal glass
    spheres (one transformation, one material value) whose velocities differ: apart from tau = 0 on.  The
    sphere passes beside the cube's centre, off the camera's axis: centred on it (at tau = 0.5 exactly) the
    world is a symmetric one whose rays tie, and the oracle's own frame changes by 0.19 when that time
    changes by 1e-13.  twins=False: the world without the twins ("glass_single"), which is its own static
    world at tau = 0."""
    world = W.World([_light()], [_floor()])
    world.shapes.append(W.cube(_glass(refractive_index=1.2), W.mat_mul(W.translation(0.0, 1.0, 0.0), W.scaling(0.9, 0.9, 0.9))))
    ball = W.sphere(_glass(refractive_index=1.5), W.mat_mul(W.translation(-1.3, 1.06, 0.07), W.scaling(0.5, 0.5, 0.5)))
    ball.velocity = (2.6, 0.0, 0.0)
    world.shapes.append(ball)
    twin = W.mat_mul(W.translation(0.0, 2.6, 0.5), W.scaling(0.45, 0.45, 0.45))
    a, b = W.sphere(_glass(refractive_index=1.4), twin), W.sphere(_glass(refractive_index=1.4), twin)
    a.velocity, b.velocity = (0.9, 0.0, 0.0), (-0.9, 0.1, 0.0)
    if not twins:
        return _tables(world), [_moving((-1.3, 1.06, 0.07), (2.6, 0.0, 0.0), 0.15), _still((0.0, 1.0, 0.0), 0.3),
                                _still((0.2, 0.0, 0.5), 1.5)]
    world.shapes += [a, b]
    return _tables(world), [_moving((-1.3, 1.06, 0.07), (2.6, 0.0, 0.0), 0.15), _still((0.0, 1.0, 0.0), 0.3),
                            _twin(_moving((0.0, 2.6, 0.5), (0.9, 0.0, 0.0), 0.15)),
                            _twin(_moving((0.0, 2.6, 0.5), (-0.9, 0.1, 0.0), 0.15)), _still((0.2, 0.0, 0.5), 1.5)]


A, B = (200, 40, 90), (30, 220, 140)
TWO_AB = np.array([[A, B]], dtype=np.uint8)


def pattern(mapped=True):
    """A striped mover and a spherically mapped mover (nearest filter): both patterns move with their shapes.
    mapped=False: the oracle's world, stripes in the map's place."""
    world = W.World([_light()], [_floor()])
    stripes = W.stripe_pattern((1.0, 0.2, 0.1), (0.1, 0.3, 1.0))
    stripes.transformation_inverse = W.inverse(W.mat_mul(W.rotation_z(0.4), W.scaling(0.37, 0.37, 0.37)))
    a = W.sphere(W.Material(pattern=stripes, specular=0.0), W.mat_mul(W.translation(-1.6, 0.8, 0.0), W.scaling(0.6, 0.6, 0.6)))
    a.velocity = (1.7, 0.0, 0.3)
    image = W.image_pattern(TWO_AB, "nearest", "spherical") if mapped else \
        W.stripe_pattern(tuple(c / 255.0 for c in A), tuple(c / 255.0 for c in B))
    b = W.sphere(W.Material(pattern=image, specular=0.0), W.mat_mul(W.translation(1.6, 1.4, 0.5), W.scaling(0.55, 0.55, 0.55)))
    b.velocity = (-1.3, 0.2, 0.0)
    world.shapes += [a, b]
    return _tables(world), [_moving((-1.6, 0.8, 0.0), (1.7, 0.0, 0.3), 0.2), _moving((1.6, 1.4, 0.5), (-1.3, 0.2, 0.0), 0.18),
                            _still((0.0, 0.0, 0.6), 1.5)]


ONE_A, ONE_B = np.array([[A]], dtype=np.uint8), np.array([[B]], dtype=np.uint8)
TWO_BA = np.array([[B, A]], dtype=np.uint8)
MAPS_CYLINDER = ((-1.2, 1.0, 0.5), (-0.24, 0.2, 1.1))  # its centre at tau = 0 and its velocity
MAPS_CUBE = ((1.3, 0.9, 0.8), (-0.9, 0.3, -0.4))


def maps(mapped=True, shift=None):
    """A closed unit cylinder under the cylindrical map with the 2 x 1 texture [a b] and a unit cube under a cube
    map of [a b] textures and their mirror images (tests/uv_map_worlds.py tie_pattern(): left a and right b
    alone, where the over point lies beyond the stripes' edge), nearest filter, both scaled and turned about y.
    mapped=False: the oracle's world, stripe_pattern(a, b) in both places; with `shift` the probe of
    tests/test_motion_random_cpu.py: the cylinder's stripes moved by it along x, the cube's twice as wide and
    moved by it (their edge is x = 0 alone: the cube's left and right faces lie 8e-8 beyond x = +-1 on purpose).

    The two patterns differ on the cylinder's lines x = +-1, where the over point's offset carries x past the
    stripes' edge.  The cylinder's x axis is turned square to the line from the eye to its centre and its
    velocity runs along that line (and along y), so both lines stay just behind its outline for every eye of the
    batches (within 0.2 of EYE, against a radius of 0.5) and of the lens frames, at every time."""
    world = W.World([_light()], [_floor()])
    a1, b1 = tuple(c / 255.0 for c in A), tuple(c / 255.0 for c in B)
    def stripes(wide=False):
        p = W.stripe_pattern(a1, b1)
        if shift is None:
            return p
        t = W.translation(shift, 0.0, 0.0)
        return p.set_transformation(W.mat_mul(t, W.scaling(2.0, 1.0, 1.0)) if wide else t)
    (cc, cv), (bc, bv) = MAPS_CYLINDER, MAPS_CUBE
    assert abs(cv[0] * (cc[2] - EYE[2]) - cv[2] * (cc[0] - EYE[0])) < 1e-12  # the velocity along the line of sight
    turn = -np.arctan2(-(cc[0] - EYE[0]), cc[2] - EYE[2])  # rotation_y(turn) (1, 0, 0) is square to that line
    tube = W.cylinder(-1.0, 1.0, True, W.Material(pattern=W.image_pattern(TWO_AB, "nearest", "cylindrical") if mapped else stripes(),
                                                  specular=0.2),
                      W.mat_mul(W.translation(*cc), W.mat_mul(W.rotation_y(turn), W.scaling(0.5, 0.45, 0.5))))
    tube.velocity = cv
    faces = W.cube_map_pattern(ONE_A, TWO_BA, ONE_B, TWO_AB, TWO_BA, TWO_BA, filter="nearest") if mapped else stripes(wide=True)
    box = W.cube(W.Material(pattern=faces, specular=0.2),
                 W.mat_mul(W.translation(*bc), W.mat_mul(W.rotation_y(0.5), W.scaling(0.45, 0.4, 0.5))))
    box.velocity = bv
    world.shapes += [tube, box]
    return _tables(world), [_moving(cc, cv, 0.2), _moving(bc, bv, 0.18), _still((0.0, 0.0, 0.6), 1.5)]


def area():
    """The far sphere's slower cousin under an area light of 2 x 2 samples (cell centres)."""
    world = W.World([], [_floor()])
    world.area_lights.append(W.AreaLight((-1.0, 5.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), 2, 2))
    s = W.sphere(W.Material(color=(0.9, 0.5, 0.2)), W.mat_mul(W.translation(-1.5, 1.2, 0.3), W.scaling(0.5, 0.5, 0.5)))
    s.velocity = (3.0, 0.0, 0.0)
    world.shapes.append(s)
    world.shapes.append(W.cube(W.Material(color=(0.3, 0.6, 0.3)), W.mat_mul(W.translation(1.2, 0.3, 1.0), W.scaling(0.3, 0.3, 0.3))))
    return _tables(world), [_moving((-1.5, 1.2, 0.3), (3.0, 0.0, 0.0), 0.18), _still((0.0, 0.0, 0.5), 1.6), _still((1.2, 0.3, 1.0), 0.1)]


def tree():
    """A bumpy ground of 72 triangles (a 6 x 6 height field, static, in the tree), the far triangle, and the
    twin octahedra, opaque: they coincide at tau = 0, where the tie goes to the first in world order."""
    ground = W.Material(color=(0.6, 0.7, 0.5), specular=0.0)
    world = W.World([_light()], [])
    vert = lambda i, j: (-3.0 + i, ((3 * i + 5 * j) % 4) / 8.0 - 0.4, -2.0 + j)  # noqa: E731
    for j in range(6):
        for i in range(6):
            a, b, c, d = vert(i, j), vert(i + 1, j), vert(i, j + 1), vert(i + 1, j + 1)
            world.shapes += [W.triangle(a, c, b, ground), W.triangle(b, c, d, ground)]
    mover = W.triangle((X0 - 0.5, 0.6, 0.1), (X0 + 0.5, 0.6, -0.1), (X0, 1.6, 0.0), W.Material(color=(0.9, 0.3, 0.2), specular=0.3))
    mover.velocity = V_FAR
    world.shapes.append(mover)
    place = W.mat_mul(W.translation(-0.8, 1.3, 0.8), W.mat_mul(W.rotation_y(0.3), W.scaling(0.4, 0.4, 0.4)))
    blue = W.Material(color=(0.2, 0.4, 0.9))
    first, second = W.instance(octahedron(), blue, place), W.instance(octahedron(), blue, place)
    second.velocity = (1.6, 0.0, 0.0)
    world.instances += [first, second]
    return _tables(world), [_moving((X0, 1.0, 0.0), V_FAR, 0.08), _still((-0.8, 1.3, 0.8), 0.08),
                            _moving((-0.8, 1.3, 0.8), (1.6, 0.0, 0.0), 0.08), _still((0.2, -0.2, 0.8), 1.4)]


WORLDS = {**{f"far_{k}": functools.partial(far, k) for k in FAR_KINDS},
          "shadow": shadow, "plane": plane, "glass": glass, "glass_single": functools.partial(glass, False),
          "pattern": pattern, "area": area, "tree": tree, "maps": maps}
DEPTH = {"glass": 5, "glass_single": 5}
POOL = ("glass", "glass_single")  # worlds with secondary rays: the pool kernel


@functools.lru_cache(maxsize=None)
def world(name):
    return WORLDS[name]()


@functools.lru_cache(maxsize=None)
def oracle_scene(name):
    """The tables the oracle traces for `name`: the world's own, but for pattern()'s and maps()'s stripes."""
    return {"pattern": pattern, "maps": maps}[name](mapped=False)[0] if name in ("pattern", "maps") else world(name)[0]


def depth(name):
    return DEPTH.get(name, 2)


@functools.lru_cache(maxsize=None)
def batch(name, n=N_RAYS, seed=11):
    """(rays (n, 6) f64, times (n,) f64): ray k leaves a point near the camera at TIMES[k mod 5] towards a
    point within its target's reach, the targets taken in turn."""
    _, targets = world(name)
    rng = np.random.default_rng(seed)
    rays, times = np.zeros((n, 6)), np.zeros(n)
    for k in range(n):
        tau = TIMES[k % len(TIMES)]
        target = targets[(k // len(TIMES)) % len(targets)]
        if tau == 0.0 and getattr(target, "no_zero", False):
            tau = TIMES[1 + (k // len(TIMES)) % (len(TIMES) - 1)]
        centre, reach = target(tau)
        u = rng.normal(size=3)
        point = np.array(centre) + reach * rng.uniform(0.0, 1.0) * u / np.linalg.norm(u)
        o = np.array(EYE) + rng.uniform(-0.2, 0.2, size=3)
        d = point - o
        rays[k, :3], rays[k, 3:], times[k] = o, d / np.linalg.norm(d), tau
    return rays, times
