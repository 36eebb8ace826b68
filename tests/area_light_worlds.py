"""Worlds with area lights for the area light tests (the reference has none; the
f64 oracle renders their expansions): a floor, a sphere and a cube under one
point light, a 2 x 2 and a 4 x 4 light, the same with a mirror floor and a glass
sphere, a mirror plane for the `remaining` test, and a textured, smooth,
instanced world.  Every light is wide enough, and close enough to its casters,
that its penumbra shows (tests/test_area_lights_cpu.py checks that).
"""
import dataclasses

import numpy as np

FRAME = (64, 32)
SMALL = (32, 16)


def eye(size=FRAME):
    from rtc_amd import world as W
    return W.camera(size[0], size[1], 0.95, (0.3, 3.2, -7.0), (0.1, 0.7, 0.0), (0.0, 1.0, 0.0))


def lights(jitter=False, seed=7):
    """One point light, a 2 x 2 light lying flat and a 4 x 4 light standing upright."""
    from rtc_amd import world as W
    point = [W.Light((-4.0, 6.0, -4.0), (0.35, 0.35, 0.4))]
    area = [W.AreaLight((1.5, 4.5, -2.5), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), 2, 2, (0.5, 0.5, 0.45), jitter, seed),
            W.AreaLight((-2.5, 2.5, -5.0), (2.5, 0.0, 0.5), (0.0, 2.0, 0.0), 4, 4, (0.4, 0.45, 0.5), jitter, seed + 1)]
    return point, area


def shapes(mirror=False):
    from rtc_amd import world as W
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.85, 0.85, 0.8), (0.35, 0.35, 0.4)), specular=0.0,
                               reflectiveness=0.4 if mirror else 0.0))
    ball = W.sphere(W.Material(color=(0.9, 0.3, 0.25), specular=0.6, shininess=40.0, diffuse=0.3 if mirror else 0.8,
                               transparency=0.8 if mirror else 0.0, reflectiveness=0.5 if mirror else 0.0,
                               refractive_index=1.5 if mirror else 1.0),
                    transform=W.mat_mul(W.translation(-0.9, 1.3, 0.2), W.scaling(0.8, 0.8, 0.8)))
    box = W.cube(W.Material(color=(0.3, 0.5, 0.9), specular=0.3, shininess=20.0),
                 transform=W.mat_mul(W.translation(1.3, 0.9, 0.6), W.mat_mul(W.rotation_y(0.6), W.scaling(0.5, 0.5, 0.5))))
    return [floor, ball, box]


def opaque(jitter=False, size=FRAME):
    """Floor, sphere and cube, all opaque: the direct kernel at any depth."""
    from rtc_amd import world as W
    point, area = lights(jitter)
    return W.World(point, shapes(), area_lights=area).tables(eye(size))


def mirror(jitter=False, size=FRAME):
    """The same with a mirror floor and a glass sphere: the pool kernel (depth 4)."""
    from rtc_amd import world as W
    point, area = lights(jitter)
    return W.World(point, shapes(True), area_lights=area).tables(eye(size))


def one_by_one(size=FRAME):
    """The opaque world under a single 1 x 1 light, and the same under the point light at its centre."""
    from rtc_amd import world as W
    a = W.AreaLight((1.0, 5.0, -3.0), (2.0, 0.0, 1.0), (0.0, 1.0, 2.0), 1, 1, (0.9, 0.8, 0.7))
    centre = tuple(a.corner[c] + 0.5 * a.full_uvec[c] + 0.5 * a.full_vvec[c] for c in range(3))
    return (W.World([], shapes(), area_lights=[a]).tables(eye(size)),
            W.World([W.Light(centre, a.intensity)], shapes()).tables(eye(size)))


def mirror_plane(jitter=True):
    """A mirror plane at y = 0 under a floating sphere and a cube, for the `remaining` test."""
    from rtc_amd import world as W
    floor = W.plane(W.Material(color=(0.7, 0.75, 0.8), specular=0.2, shininess=30.0, reflectiveness=0.6))
    ball = W.sphere(W.Material(color=(0.9, 0.4, 0.2), specular=0.5, shininess=50.0),
                    transform=W.mat_mul(W.translation(0.2, 1.6, 0.3), W.scaling(0.7, 0.7, 0.7)))
    box = W.cube(W.Material(color=(0.2, 0.7, 0.4), specular=0.1),
                 transform=W.mat_mul(W.translation(-1.6, 0.6, 0.8), W.scaling(0.4, 0.6, 0.4)))
    point, area = lights(jitter, seed=21)
    return W.World(point, [floor, ball, box], area_lights=area).tables(eye())


def plane_rays(n=256, seed=11):
    """n rays from above the mirror plane, aimed at points of it around the casters and passing clear of both
    (of the sphere, and of the ball around the cube): unit directions."""
    rng = np.random.default_rng(seed)
    m = 16 * n
    o = rng.uniform([-3.0, 2.5, -6.0], [3.0, 5.0, -3.0], size=(m, 3))
    target = np.concatenate([rng.uniform(-3.0, 3.0, size=(m, 1)), np.zeros((m, 1)), rng.uniform(-2.0, 3.0, size=(m, 1))], axis=1)
    d = target - o
    clear = np.ones(m, dtype=bool)
    for centre, radius in (((0.2, 1.6, 0.3), 0.7), ((-1.6, 0.6, 0.8), 0.83)):  # mirror_plane's casters
        v = np.array(centre) - o
        s = np.clip((v * d).sum(axis=1) / (d * d).sum(axis=1), 0.0, 1.0)
        clear &= np.linalg.norm(v - d * s[:, None], axis=1) > radius + 0.05
    o, d = o[clear][:n], d[clear][:n]
    assert len(o) == n
    d /= np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    return np.ascontiguousarray(np.concatenate([o, d], axis=1))


def seeded_rays(n, seed):
    """n unit rays from in front of the opaque world toward it."""
    rng = np.random.default_rng(seed)
    o = rng.uniform([-4.0, 0.5, -8.0], [4.0, 5.0, -4.0], size=(n, 3))
    target = rng.uniform([-3.0, 0.0, -2.0], [3.0, 2.0, 3.0], size=(n, 3))
    d = target - o
    d /= np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    return np.ascontiguousarray(np.concatenate([o, d], axis=1))


def with_area(tables, area):
    """`tables` with the area lights `area` (AreaLight values) beside its own lights."""
    from rtc_amd import AreaLightDesc
    return dataclasses.replace(tables, area_lights=(AreaLightDesc * len(area))(*[a.desc() for a in area]))


def textured_tori(rtc, smooth=True):
    """texture_worlds' three textured torus instances over a checkered floor, the tori smooth as well, lit by
    their two point lights and one 3 x 3 area light."""
    import mesh_worlds as M
    import texture_worlds as X
    from rtc_amd import world as W
    verts, faces = M.torus(24, 12)
    ang = np.arctan2(verts[:, 2], verts[:, 0]) / (2 * np.pi) + 0.5
    tube = np.arctan2(verts[:, 1], np.hypot(verts[:, 0], verts[:, 2]) - 1.0) / (2 * np.pi) + 0.5
    ring = np.stack([verts[:, 0], np.zeros(len(verts)), verts[:, 2]], axis=1)
    ring /= np.linalg.norm(ring, axis=1, keepdims=True)
    normals = verts - ring
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    mesh = X.load(rtc, verts, faces, np.stack([ang, tube], axis=1), normals=normals if smooth else None)
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                    transform=W.translation(0, -1.3, 0))
    pts = [W.Light((-5.0, 6.0, -5.0), (0.4, 0.4, 0.4)), W.Light((4.0, 5.0, -2.0), (0.2, 0.2, 0.2))]
    half = W.scaling(0.6, 0.6, 0.6)
    places = [W.mat_mul(W.translation(-1.1, 0.0, 0.3), half),
              W.mat_mul(W.translation(1.0, 0.3, 0.5), W.mat_mul(W.rotation_x(0.9), half)),
              W.mat_mul(W.translation(0.0, -0.4, -0.6), W.mat_mul(W.rotation_y(0.7), half))]
    pat = W.image_pattern(X.colors(5, 7), "bilinear")
    inst = [W.instance(mesh, W.Material(pattern=pat, specular=0.5, shininess=60.0), transform=p, textured=True,
                       smooth=smooth) for p in places]
    area = [W.AreaLight((-1.5, 3.0, -3.5), (3.0, 0.0, 0.0), (0.0, 0.5, 2.5), 3, 3, (0.5, 0.5, 0.5))]
    import smooth_worlds as S
    return W.World(pts, [floor], inst, area_lights=area).tables(S.camera())


def centre_lit(rtc, tables):
    """`tables` with every area light replaced by one point light of its full intensity at its centre: the
    world without a penumbra that the penumbra condition compares against."""
    rows = [(tuple(lt.position), tuple(lt.intensity)) for lt in tables.lights]
    for al in tables.area_lights:
        rows.append((tuple(al.corner[c] + 0.5 * al.full_uvec[c] + 0.5 * al.full_vvec[c] for c in range(3)),
                     tuple(al.intensity)))
    lts = (rtc.LightDesc * len(rows))()
    for d, (p, i) in zip(lts, rows):
        d.position[:] = p
        d.intensity[:] = i
    return dataclasses.replace(tables, lights=lts, area_lights=None)


def unjittered(tables):
    """`tables` with every area light sampled at its cells' centres."""
    from rtc_amd import AreaLightDesc
    area = (AreaLightDesc * len(tables.area_lights)).from_buffer_copy(tables.area_lights)
    for a in area:
        a.jitter = 0
    return dataclasses.replace(tables, area_lights=area)


def with_area_tables(tables, lit):
    """`tables` with the area lights of `lit`."""
    return dataclasses.replace(tables, area_lights=lit.area_lights)


def bright(intensity, area=True, size=SMALL):
    """The mirror floor, glass sphere and cube under one light of `intensity` in every channel: a 4 x 4 area
    light, or (area=False) the equal point light, for the brightness bound."""
    from rtc_amd import world as W
    i3 = (float(intensity),) * 3
    if area:
        return W.World([], shapes(True), area_lights=[W.AreaLight((-1.0, 5.0, -4.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0),
                                                                  4, 4, i3)]).tables(eye(size))
    return W.World([W.Light((0.0, 5.0, -3.0), i3)], shapes(True)).tables(eye(size))
