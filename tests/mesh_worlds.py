"""Triangle meshes for the mesh tests, generated from code (the reference has
none): an icosphere, a torus and a height field with dyadic vertices, as
vertex and face arrays, as OBJ text, and as worlds over a plane with a sphere
and two lights.

  icosphere(2), icosphere(3)  320 and 1280 triangles on the unit sphere
  torus(24, 12)               576 triangles, radii 1 and 0.4
  height_field(16)            512 triangles over [-2, 2]^2, every coordinate a
                              multiple of 1/8: rays with dyadic origins pass
                              through its edges and vertices exactly
"""
import math

import numpy as np

FRAME = (80, 60)  # partial tiles (RT_TILE_W = 64)
CAMERA = ((0.3, 1.7, -4.2), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0))
FOV = 0.9


def icosphere(subdivisions):
    t = (1.0 + math.sqrt(5.0)) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
             (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [tuple(c / math.sqrt(1 + t * t) for c in v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2),
             (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11),
             (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = [(verts[a][q] + verts[b][q]) / 2.0 for q in range(3)]
                n = math.sqrt(sum(c * c for c in m))
                verts.append(tuple(c / n for c in m))
                mid[key] = len(verts) - 1
            return mid[key]
        out = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.array(verts, dtype=np.float64), np.array(faces, dtype=np.int64)


def torus(nu=24, nv=12, major=1.0, minor=0.4):
    verts = []
    for i in range(nu):
        a = 2.0 * math.pi * i / nu
        for j in range(nv):
            b = 2.0 * math.pi * j / nv
            r = major + minor * math.cos(b)
            verts.append((r * math.cos(a), minor * math.sin(b), r * math.sin(a)))
    faces = []
    for i in range(nu):
        for j in range(nv):
            p, q = i * nv + j, i * nv + (j + 1) % nv
            r, s = ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv
            faces += [(p, q, s), (p, s, r)]
    return np.array(verts, dtype=np.float64), np.array(faces, dtype=np.int64)


def height_field(cells=16):
    """(cells + 1)^2 vertices at x, z = -2 + k / 4 with heights in {0, 1/8, 2/8, 3/8}; two triangles per cell."""
    n = cells + 1
    verts = [(-2.0 + i / 4.0, ((3 * i + 5 * j) % 4) / 8.0, -2.0 + j / 4.0) for j in range(n) for i in range(n)]
    faces = []
    for j in range(cells):
        for i in range(cells):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i, (j + 1) * n + i + 1
            faces += [(a, c, b), (b, c, d)]
    return np.array(verts, dtype=np.float64), np.array(faces, dtype=np.int64)


MESHES = {"ico2": lambda: icosphere(2), "ico3": lambda: icosphere(3), "torus": lambda: torus(24, 12),
          "field": lambda: height_field(16)}
TRIANGLES = {"ico2": 320, "ico3": 1280, "torus": 576, "field": 512}


def obj_text(verts, faces, newline="\n"):
    """OBJ text that round-trips the vertices exactly (repr of the f64 values)."""
    lines = ["# generated mesh", "o mesh"]
    lines += [f"v {x!r} {y!r} {z!r}" for x, y, z in verts.tolist()]
    lines += ["s off"]
    lines += [f"f {a + 1} {b + 1} {c + 1}" for a, b, c in faces.tolist()]
    return newline.join(lines) + newline


def load(rtc, tmp_path, name):
    """The named mesh written as an OBJ file under tmp_path and read back through rtc_amd.load_obj."""
    verts, faces = MESHES[name]()
    path = tmp_path / f"{name}.obj"
    path.write_text(obj_text(verts, faces))
    mesh = rtc.load_obj(str(path))
    assert mesh.triangles.shape == (TRIANGLES[name], 3) and np.array_equal(mesh.vertices, verts)
    return mesh


def camera():
    from rtc_amd import world as W
    return W.camera(*FRAME, FOV, *CAMERA)


def glass():
    from rtc_amd import world as W
    return W.Material(color=(0.1, 0.2, 0.3), diffuse=0.3, ambient=0.1, specular=0.8, shininess=100.0,
                      reflectiveness=0.3, transparency=0.8, refractive_index=1.5)


def world(mesh_shapes):
    """The mesh over a patterned plane, next to a sphere, under two lights."""
    from rtc_amd import world as W
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                    transform=W.translation(0, -1.3, 0))
    ball = W.sphere(W.Material(color=(0.9, 0.3, 0.2)), transform=W.mat_mul(W.translation(1.9, -0.7, 0.6),
                                                                         W.scaling(0.6, 0.6, 0.6)))
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    return W.World(lights, [floor, ball] + list(mesh_shapes)).tables(camera())


def same_world_by_triangle(mesh, material=None):
    """The shapes world.mesh gives, built face by face with world.triangle (the path that existed before)."""
    from rtc_amd import world as W
    v = mesh.vertices
    return [W.triangle(tuple(v[a]), tuple(v[b]), tuple(v[c]), material) for a, b, c in mesh.triangles.tolist()]


def _transform():
    from rtc_amd import world as W
    return W.mat_mul(W.rotation_y(0.7), W.shearing(0.3, 0.0, 0.0, 0.2, 0.0, 0.0))


WORLDS = ["ico2", "ico3", "torus", "field", "glass", "unbaked", "baked", "doubled", "coincident"]


def build_world(rtc, tmp_path, key):
    """(tables, depth) of a named mesh world of WORLDS."""
    from rtc_amd import world as W
    opaque = W.Material(color=(0.25, 0.6, 0.85), specular=0.5, shininess=60.0)
    get = lambda name: load(rtc, tmp_path, name)  # noqa: E731
    if key in MESHES:  # opaque: the direct kernel
        lift = W.translation(0, 0.35, 0) if key != "field" else W.translation(0, -0.2, 0.5)
        return world(W.mesh(get(key), opaque, transform=lift, bake=True)), 3
    if key == "glass":  # transparent and reflective: the pool kernel and the containers walk
        return world(W.mesh(get("ico2"), glass())), 4
    if key == "unbaked":  # rotation x shear, as set_transformation on every triangle
        return world(W.mesh(get("torus"), opaque, transform=_transform())), 3
    if key == "baked":  # ... and multiplied into the vertices
        return world(W.mesh(get("torus"), opaque, transform=_transform(), bake=True)), 3
    if key == "doubled":  # value-equal faces: one identity class per pair, the containers walk per class
        mesh, mat = get("ico2"), glass()
        return world(W.mesh(mesh, mat) + W.mesh(mesh, mat)), 4
    if key == "coincident":  # equal t across records of different materials: the lower world index wins
        mesh = get("torus")
        other = W.Material(color=(0.9, 0.8, 0.1), diffuse=0.7, specular=0.1)
        return world(W.mesh(mesh, opaque) + W.mesh(mesh, other)), 3
    raise KeyError(key)


def random_rays(n, seed):
    """Origins in a box around the mesh, directions uniform on the sphere, |d| from U(0.5, 1.25)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-2.5, 2.5, (n, 3))
    d = rng.normal(size=(n, 3))
    d *= (rng.uniform(0.5, 1.25, n) / np.linalg.norm(d, axis=1))[:, None]
    return np.ascontiguousarray(np.concatenate([o, d], axis=1))


def share_within(got, ref, tol=2.0 / 255.0):
    """Share of pixels (rays) whose colour is within tol of the reference's in every channel."""
    return float((np.abs(got - ref).max(axis=-1) <= tol).mean())
