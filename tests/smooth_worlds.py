"""Worlds with smooth triangles for the smooth tests (the reference has none):
OBJ text with vn lines and f i//k faces, an icosphere whose vertex normals are
its vertex positions, a 12-triangle box whose normals may be its faces' own
(degenerate: flat shading through the smooth code), the dyadic height field
with slanted normals, and the worlds the GPU tests share.
"""
import numpy as np

import mesh_worlds as M

FRAME = (80, 60)  # partial tiles (RT_TILE_W = 64)
# a camera off every symmetry plane of the icosphere, so no primary ray runs through an edge or a vertex
EYE = ((0.37, 0.83, -3.1), (0.03, -0.02, 0.0), (0.0, 1.0, 0.0))
FOV = 0.8


def obj_text(verts, faces, normals=None, face_normals=None, newline="\n"):
    """OBJ text that round-trips vertices and normals exactly (repr of the f64 values).  normals: (k, 3) vn
    lines; face_normals: per face its three 0-based normal indices (default: the vertex indices), written
    as f i//k; without normals the text is mesh_worlds.obj_text's."""
    if normals is None:
        return M.obj_text(verts, faces, newline)
    fn = faces if face_normals is None else face_normals
    lines = ["# generated mesh", "o mesh"]
    lines += [f"v {x!r} {y!r} {z!r}" for x, y, z in np.asarray(verts).tolist()]
    lines += [f"vn {x!r} {y!r} {z!r}" for x, y, z in np.asarray(normals).tolist()]
    lines += ["s 1"]
    lines += ["f " + " ".join(f"{a + 1}//{k + 1}" for a, k in zip(f, g))
              for f, g in zip(np.asarray(faces).tolist(), np.asarray(fn).tolist())]
    return newline.join(lines) + newline


def icosphere(subdivisions=2):
    """(verts, faces, normals): the unit icosphere; a vertex's normal is its position."""
    verts, faces = M.icosphere(subdivisions)
    return verts, faces, verts.copy()


def box(degenerate=True):
    """(verts, faces, normals, face_normals) of the cube [-1, 1]^3 as 12 triangles wound outwards.
    degenerate: every vertex normal is its face's axis normal, so the smooth box shades as the flat one;
    else the normals are the corners' directions (a rounded look)."""
    verts = np.array([(x, y, z) for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    quads = [((0, 1, 3, 2), (-1.0, 0.0, 0.0)), ((4, 6, 7, 5), (1.0, 0.0, 0.0)), ((0, 4, 5, 1), (0.0, -1.0, 0.0)),
             ((2, 3, 7, 6), (0.0, 1.0, 0.0)), ((0, 2, 6, 4), (0.0, 0.0, -1.0)), ((1, 5, 7, 3), (0.0, 0.0, 1.0))]
    faces, fnorm, normals = [], [], []
    for q, (corners, axis) in enumerate(quads):
        a, b, c, d = corners
        faces += [(a, b, c), (a, c, d)]
        if degenerate:
            normals.append(axis)
            fnorm += [(q, q, q), (q, q, q)]
        else:
            fnorm += [(a, b, c), (a, c, d)]
    if not degenerate:
        normals = (verts / np.sqrt(3.0)).tolist()
    # Triangle::new's normal is normalize(e2 x e1): wind the faces so that it is the outward axis
    faces, fnorm = np.array(faces), np.array(fnorm)
    for i, (f, (corners, axis)) in enumerate(zip(faces, [q for q in quads for _ in (0, 1)])):
        e1, e2 = verts[f[1]] - verts[f[0]], verts[f[2]] - verts[f[0]]
        if np.dot(np.cross(e2, e1), axis) < 0:
            faces[i] = f[[0, 2, 1]]
            fnorm[i] = fnorm[i][[0, 2, 1]]
    return verts, faces, np.array(normals, dtype=np.float64), fnorm


def height_field():
    """The dyadic height field of mesh_worlds with a slanted dyadic normal per vertex."""
    verts, faces = M.height_field(16)
    normals = np.array([(((3 * i) % 5 - 2) / 8.0, 1.0, ((7 * i) % 5 - 2) / 8.0) for i in range(len(verts))])
    return verts, faces, normals


def load(rtc, verts, faces, normals, face_normals=None):
    mesh = rtc.load_obj(obj_text(verts, faces, normals, face_normals), normals=True)
    assert mesh.n_smooth == len(faces) and np.array_equal(mesh.vertices, verts) and np.array_equal(mesh.normals, normals)
    return mesh


def camera(frame=FRAME, eye=EYE, fov=FOV):
    from rtc_amd import world as W
    return W.camera(*frame, fov, *eye)


def camera_rays(cam):
    """Camera::ray_for_pixel (camera.rs:52-68) for every pixel, row-major, in f64 and in the f64 kernel's
    operation order (as tests/test_gpu_trace_rays.py forms them)."""
    x, y = np.meshgrid(np.arange(cam.width, dtype=np.float64), np.arange(cam.height, dtype=np.float64))
    wx = cam.half_width - (x.ravel() + 0.5) * cam.pixel_size
    wy = cam.half_height - (y.ravel() + 0.5) * cam.pixel_size
    m = np.array(cam.inverse[:], dtype=np.float64)
    origin = np.array(cam.origin[:], dtype=np.float64)
    d = np.stack([(((0.0 + m[4 * r] * wx) + m[4 * r + 1] * wy) + m[4 * r + 2] * -1.0) + m[4 * r + 3] - origin[r]
                  for r in range(3)], axis=1)
    d /= np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(origin, d.shape), d], axis=1))


def opaque():
    from rtc_amd import world as W
    return W.Material(color=(0.25, 0.6, 0.85), specular=0.5, shininess=60.0)


def eye_light():
    """One light beside the eye."""
    from rtc_amd import world as W
    return W.Light((EYE[0][0] + 0.9, EYE[0][1] + 0.6, EYE[0][2] - 0.4), (1.0, 1.0, 1.0))


def ico_alone(rtc, smooth=True, extra=()):
    """The 320-triangle icosphere alone under one light beside the eye; smooth or the same faces flat."""
    from rtc_amd import world as W
    mesh = load(rtc, *icosphere(2))
    return W.World([eye_light()], W.mesh(mesh, opaque(), smooth=smooth) + list(extra)).tables(camera())


def glass_behind_the_camera():
    """A small glass sphere behind the camera, out of every light path: the world gets a transparent
    material (the pool kernel) and no ray of the frame, primary or shadow, meets the sphere."""
    from rtc_amd import world as W
    return W.sphere(M.glass(), transform=W.mat_mul(W.translation(0.4, -6.0, -9.0), W.scaling(0.2, 0.2, 0.2)))


def ico_over_plane(rtc, smooth=True, material=None):
    """The icosphere over a checkered plane under two lights (321 shapes: the triangle tree is built)."""
    from rtc_amd import world as W
    mesh = load(rtc, *icosphere(2))
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                    transform=W.translation(0, -1.3, 0))
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    return W.World(lights, [floor] + W.mesh(mesh, material or opaque(), smooth=smooth)).tables(camera())


def box_world(rtc, smooth=True, copies=1, normals_of_second=None, material_of_second=None):
    """The degenerate box as glass over a checkered plane (depth 4); copies = 2 doubles it (value-equal
    pairs), normals_of_second: the second copy's normal table (to make it differ in one component),
    material_of_second: its material (to make the flat copies differ by value)."""
    from rtc_amd import world as W
    verts, faces, normals, fnorm = box(True)
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                    transform=W.translation(0, -1.3, 0))
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    place = W.mat_mul(W.translation(0.1, 0.0, 0.3), W.mat_mul(W.rotation_y(0.5), W.scaling(0.8, 0.9, 0.7)))
    glass = M.glass()
    shapes = [floor]
    for c in range(copies):
        nn = normals if c == 0 or normals_of_second is None else normals_of_second
        mat = glass if c == 0 or material_of_second is None else material_of_second
        shapes += W.mesh(load(rtc, verts, faces, nn, fnorm), mat, transform=place, smooth=smooth)
    return W.World(lights, shapes).tables(camera())


def box_instances(rtc, smooth=True):
    """The box as one mesh with two instances (translation; rotation x shear), glass, over the plane."""
    from rtc_amd import world as W
    verts, faces, normals, fnorm = box(True)
    mesh = load(rtc, verts, faces, normals, fnorm)
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                    transform=W.translation(0, -1.3, 0))
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    small = W.scaling(0.5, 0.5, 0.5)
    places = [W.mat_mul(W.translation(-0.9, -0.2, 0.2), small),
              W.mat_mul(W.translation(0.9, 0.1, 0.4), W.mat_mul(W.mat_mul(W.rotation_y(0.7),
                                                                        W.shearing(0.3, 0.0, 0.0, 0.2, 0.0, 0.0)), small))]
    inst = [W.instance(mesh, M.glass(), transform=p, smooth=smooth) for p in places]
    return W.World(lights, [floor], inst).tables(camera())


def torus_instances(rtc, smooth=True):
    """Three instances of a smooth torus (576 triangles; normals point from the tube's centre line)."""
    from rtc_amd import world as W
    verts, faces = M.torus(24, 12)
    ring = np.stack([verts[:, 0], np.zeros(len(verts)), verts[:, 2]], axis=1)
    ring /= np.linalg.norm(ring, axis=1)[:, None]
    normals = (verts - ring) / 0.4
    mesh = load(rtc, verts, faces, normals)
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                    transform=W.translation(0, -1.3, 0))
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    half = W.scaling(0.6, 0.6, 0.6)
    places = [W.mat_mul(W.translation(-1.1, 0.0, 0.3), half),
              W.mat_mul(W.translation(1.0, 0.3, 0.5), W.mat_mul(W.rotation_x(0.9), half)),
              W.mat_mul(W.translation(0.0, -0.4, -0.6),
                        W.mat_mul(W.mat_mul(W.rotation_y(0.7), W.shearing(0.3, 0.0, 0.0, 0.2, 0.0, 0.0)), half))]
    mats = [opaque(), W.Material(color=(0.9, 0.8, 0.1), diffuse=0.7, specular=0.1), opaque()]
    inst = [W.instance(mesh, m, transform=p, smooth=smooth) for m, p in zip(mats, places)]
    return W.World(lights, [floor], inst).tables(camera())


def ico_instances(rtc, smooth=True, extra=()):
    """Two instances (a translation; a rotation x shear) of the 80-triangle icosphere, opaque, under the light
    beside the eye and nothing else: a world of triangles only, for which tests/smooth_reference.py speaks
    (torus_instances and box_instances stand over a plane, and the boxes are glass)."""
    from rtc_amd import world as W
    mesh = load(rtc, *icosphere(1))
    small = W.scaling(0.7, 0.7, 0.7)
    places = [W.mat_mul(W.translation(-0.8, 0.1, 0.2), small),
              W.mat_mul(W.translation(0.75, -0.1, 0.5), W.mat_mul(W.mat_mul(W.rotation_y(0.7),
                                                                            W.shearing(0.3, 0.0, 0.0, 0.2, 0.0, 0.0)), small))]
    mats = [opaque(), W.Material(color=(0.9, 0.8, 0.1), diffuse=0.7, specular=0.1)]
    inst = [W.instance(mesh, m, transform=p, smooth=smooth) for m, p in zip(mats, places)]
    return W.World([eye_light()], list(extra), inst).tables(camera())


# The thin lens of the lens tests of these worlds (tests/test_gpu_lens_builds.py): the icosphere's near side is
# 2.2 from the eye, the focal plane behind it, so that every part of the frame is out of focus.
LENS_APERTURE, LENS_FOCUS, LENS_SEED = 0.2, 5.0, 1


def flat_of(rtc, tables):
    """The same tables without the smooth list: every triangle flat."""
    return rtc.SceneTables(tables.shapes, tables.materials, tables.patterns, tables.lights, tables.camera,
                           meshes=tables.meshes, instances=tables.instances)
