"""The seeded random worlds of tests/test_gpu_random_worlds.py, and tests/random_moving_worlds.py's base worlds.

Each seed draws a world with every shape kind (world.rs:25-35 with shapes/*.rs), random transforms with
rotation, non-uniform scale and shear (shape.rs:22-27), random Phong materials with reflection, refraction and
Schlick mixing (world.rs:38-67, 114-157), every pattern kind but the test pattern (pattern.rs), shapes that cast
no shadow (world.rs:108-111), sometimes a value-identical copy of a shape (intersection.rs:47), one to three
lights, and a depth of 0 to 6.

The draws are fixed: tests/golden/random_worlds_sha256.json holds a hash of every table of seeds 0 to 47
(tests/test_motion_random_cpu.py), so that a change here that moves one draw shows.
"""
import math

import numpy as np


def random_world(seed, plain=False, allow_dup=True, light_scale=1.0):
    """(tables, camera, depth) of seed's world.  plain: no reflective or
    transparent material (the direct kernel's worlds); allow_dup=False: no
    value-identical copy; light_scale: brighter lights (the f32 pixel sums'
    fixed-point scale follows the world's brightness bound).  None of them
    changes the draws of the other parts."""
    from rtc_amd import world as W
    rng = np.random.default_rng(seed)

    def u(lo, hi):
        return float(rng.uniform(lo, hi))

    def color():
        return (u(0, 1), u(0, 1), u(0, 1))

    def transform(scale_lo=0.3, scale_hi=1.4):
        m = W.translation(u(-3, 3), u(0, 2.5), u(-3, 3))
        m = W.mat_mul(m, W.rotation_y(u(0, 2 * math.pi)))
        if rng.random() < 0.6:
            m = W.mat_mul(m, W.rotation_x(u(-1, 1)))
            m = W.mat_mul(m, W.rotation_z(u(-1, 1)))
        if rng.random() < 0.25:
            m = W.mat_mul(m, W.shearing(*[u(-0.3, 0.3) for _ in range(6)]))
        s = u(scale_lo, scale_hi)
        if rng.random() < 0.5:
            return W.mat_mul(m, W.scaling(s, s, s))
        return W.mat_mul(m, W.scaling(s, u(scale_lo, scale_hi), u(scale_lo, scale_hi)))

    def pattern():
        kind = int(rng.integers(0, 5))
        if kind == 4:
            p = W.complex_pattern(W.stripe_pattern(color(), color()), W.checker_pattern(color(), color()))
        else:
            p = (W.stripe_pattern, W.gradient_pattern, W.ring_pattern, W.checker_pattern)[kind](color(), color())
        if rng.random() < 0.5:
            p.set_transformation(W.mat_mul(W.rotation_y(u(0, 3)), W.scaling(u(0.2, 1), u(0.2, 1), u(0.2, 1))))
        return p

    def material():
        m = W.Material(color=color(), ambient=u(0, 0.3), diffuse=u(0.3, 1), specular=u(0, 1),
                       shininess=u(5, 300), casts_shadow=bool(rng.random() < 0.85))
        if rng.random() < 0.3:
            m.pattern = pattern()
        if rng.random() < 0.35:
            m.reflectiveness = u(0.1, 0.9)
        if rng.random() < 0.3:
            m.transparency = u(0.2, 1.0)
            m.refractive_index = u(1.0, 2.0)
        return m

    shapes = [W.plane(material(), W.translation(0, u(-1.5, -0.5), 0))]
    if rng.random() < 0.3:  # a back wall
        shapes.append(W.plane(material(), W.mat_mul(W.translation(0, 0, 6), W.rotation_x(math.pi / 2))))
    for _ in range(int(rng.integers(3, 9))):
        kind = int(rng.integers(0, 5))
        if kind == 0:
            shapes.append(W.sphere(material(), transform()))
        elif kind == 1:
            shapes.append(W.cube(material(), transform(0.2, 0.9)))
        elif kind == 2:
            lo = u(-1, 0.5)
            bounded = rng.random() < 0.8
            shapes.append(W.cylinder(lo if bounded else -W.F64_MAX, lo + u(0.2, 2) if bounded else W.F64_MAX,
                                     bool(rng.random() < 0.6), material(), transform(0.2, 0.9)))
        elif kind == 3:
            lo = u(-1.5, -0.2)
            shapes.append(W.cone(lo, u(-0.1, 1.0) if rng.random() < 0.5 else 0.0, bool(rng.random() < 0.6),
                                 material(), transform(0.3, 1.0)))
        else:
            c = (u(-3, 3), u(0, 2), u(-3, 3))
            pts = [tuple(c[q] + u(-1.2, 1.2) for q in range(3)) for _ in range(3)]
            shapes.append(W.triangle(*pts, material()))
    if rng.random() < 0.25:  # a value-identical copy (the containers walk's identity classes)
        import copy
        at, src = int(rng.integers(0, len(shapes))), int(rng.integers(1, len(shapes)))
        if allow_dup:
            shapes.insert(at, copy.deepcopy(shapes[src]))
    if plain:
        for sh in shapes:
            sh.material.reflectiveness = sh.material.transparency = 0.0
    lights = [W.Light((u(-8, 8), u(4, 10), u(-10, -2)),
                      (light_scale * u(0.3, 1), light_scale * u(0.3, 1), light_scale * u(0.3, 1)))
              for _ in range(int(rng.integers(1, 4)))]
    eye = (u(-4, 4), u(1.5, 4), u(-9, -6))
    cam = W.camera(96, 72, u(0.6, 1.2), eye, (0, 0.5, 0), (0, 1, 0))
    return W.World(lights, shapes).tables(), cam, int(rng.integers(0, 7))


def many_shapes_world(seed, n):
    """A world of n small shapes (spheres, cubes, closed cylinders, triangles)
    scattered over a floor, a fifth of them reflective or glass: past the
    per-scene builds' record limit (255 shapes) and the LDS world tables."""
    from rtc_amd import world as W
    rng = np.random.default_rng(seed)

    def u(lo, hi):
        return float(rng.uniform(lo, hi))

    shapes = [W.plane(W.Material(color=(0.8, 0.8, 0.7), reflectiveness=0.1), W.translation(0, -0.2, 0))]
    for _ in range(n):
        m = W.Material(color=(u(0, 1), u(0, 1), u(0, 1)), specular=u(0, 1), shininess=u(10, 200))
        r = rng.random()
        if r < 0.1:
            m.reflectiveness = u(0.2, 0.9)
        elif r < 0.2:
            m.transparency, m.refractive_index = u(0.5, 1.0), u(1.1, 1.8)
        s = u(0.05, 0.25)
        t = W.mat_mul(W.translation(u(-6, 6), u(0, 3), u(-4, 8)), W.rotation_y(u(0, 3)))
        k = int(rng.integers(0, 4))
        if k == 0:
            shapes.append(W.sphere(m, W.mat_mul(t, W.scaling(s, s, s))))
        elif k == 1:
            shapes.append(W.cube(m, W.mat_mul(t, W.scaling(s, s, s))))
        elif k == 2:
            shapes.append(W.cylinder(-1, 1, True, m, W.mat_mul(t, W.scaling(s, s, s))))
        else:
            c = (u(-6, 6), u(0, 3), u(-4, 8))
            shapes.append(W.triangle(*[tuple(c[q] + u(-0.3, 0.3) for q in range(3)) for _ in range(3)], m))
    lights = [W.Light((-10, 10, -10)), W.Light((8, 12, -4), (0.4, 0.4, 0.5))]
    cam = W.camera(80, 60, 1.1, (0, 2.5, -9), (0, 1, 2), (0, 1, 0))
    return W.World(lights, shapes).tables(), cam


def tables_sha256(tables, cam, depth=None):
    """A hash over every table of a world, its camera and its depth."""
    import hashlib
    h = hashlib.sha256()
    for part in (tables.shapes, tables.materials, tables.patterns, tables.lights, cam):
        h.update(bytes(part))
    h.update(repr(depth).encode())
    return h.hexdigest()
