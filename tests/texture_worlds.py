"""Worlds with image textures for the texture tests (the reference has none):
OBJ text with vt lines and f i/j or i/j/k faces, textures made with numpy, an
icosphere with a texture coordinate per vertex, a quad in the xz-plane, the
12-triangle box, and the worlds the GPU tests share.
"""
import numpy as np

import mesh_worlds as M
import smooth_worlds as S

FRAME = S.FRAME


def obj_text(verts, faces, texcoords, face_texcoords=None, normals=None, face_normals=None, newline="\n"):
    """OBJ text with vt lines that round-trips every number exactly.  texcoords: (k, 2) vt lines;
    face_texcoords: per face its three 0-based vt indices (default: the vertex indices), None entries write a
    face without coordinates; normals / face_normals as smooth_worlds.obj_text (f i/j/k)."""
    ft = [tuple(f) for f in np.asarray(faces).tolist()] if face_texcoords is None else list(face_texcoords)
    fn = None if normals is None else (faces if face_normals is None else face_normals)
    lines = ["# generated mesh", "o mesh"]
    lines += [f"v {x!r} {y!r} {z!r}" for x, y, z in np.asarray(verts).tolist()]
    lines += [f"vt {u!r} {v!r}" for u, v in np.asarray(texcoords).tolist()]
    if normals is not None:
        lines += [f"vn {x!r} {y!r} {z!r}" for x, y, z in np.asarray(normals).tolist()]
    for i, f in enumerate(np.asarray(faces).tolist()):
        words = []
        for c, a in enumerate(f):
            t = "" if ft[i] is None else str(ft[i][c] + 1)
            k = "" if fn is None else str(np.asarray(fn).tolist()[i][c] + 1)
            words.append(f"{a + 1}/{t}/{k}" if k else (f"{a + 1}/{t}" if t else f"{a + 1}"))
        lines.append("f " + " ".join(words))
    return newline.join(lines) + newline


def colors(width, height, seed=5):
    """A (height, width, 3) uint8 texture of distinct, well separated colours."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(height, width, 3), dtype=np.uint8)
    img[..., 0] = (np.arange(width * height).reshape(height, width) * 97 + 31) % 256  # no two texels alike
    return np.ascontiguousarray(img)


SIX = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]], [[255, 255, 0], [0, 255, 255], [255, 0, 255]]], dtype=np.uint8)


def uniform(width, height, rgb=(200, 120, 40)):
    return np.ascontiguousarray(np.broadcast_to(np.array(rgb, dtype=np.uint8), (height, width, 3)))


def ico_coords(verts, wrap=False):
    """A texture coordinate per icosphere vertex: inside (0.05, 0.95), or (wrap) from -0.7 to 1.9."""
    lo, span = (-0.7, 2.6) if wrap else (0.05, 0.9)
    return np.stack([lo + span * (0.5 + 0.5 * verts[:, 0]), lo + span * (0.5 + 0.5 * verts[:, 1])], axis=1)


def load(rtc, verts, faces, texcoords, face_texcoords=None, normals=None, face_normals=None):
    mesh = rtc.load_obj(obj_text(verts, faces, texcoords, face_texcoords, normals, face_normals), texcoords=True,
                        normals=normals is not None)
    assert np.array_equal(mesh.vertices, verts) and np.array_equal(mesh.texcoords, texcoords)
    return mesh


def textured_material(image, filter, **kw):
    from rtc_amd import world as W
    kw.setdefault("specular", 0.5)
    kw.setdefault("shininess", 60.0)
    return W.Material(pattern=W.image_pattern(image, filter), **kw)


def ico_alone(rtc, image, filter, extra=(), wrap=False, swap=False, subdivisions=2, smooth=False):
    """The icosphere alone under one light beside the eye with a coordinate per vertex; swap: the coordinates
    of vertices 0 and 1 exchanged."""
    from rtc_amd import world as W
    verts, faces = M.icosphere(subdivisions)
    tc = ico_coords(verts, wrap)
    if swap:
        tc[[0, 1]] = tc[[1, 0]]
    mesh = load(rtc, verts, faces, tc, normals=verts.copy() if smooth else None)
    assert mesh.n_textured == len(faces)
    shapes = W.mesh(mesh, textured_material(image, filter), textured=True, smooth=smooth)
    return W.World([S.eye_light()], shapes + list(extra)).tables(S.camera())


def ico_over_plane(rtc, image, filter, material=None, textured=True):
    """smooth_worlds.ico_over_plane with the icosphere textured (or, textured=False, the same material on
    triangles without coordinates and without pattern: the untextured upload)."""
    from rtc_amd import world as W
    verts, faces = M.icosphere(2)
    mesh = load(rtc, verts, faces, ico_coords(verts))
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                    transform=W.translation(0, -1.3, 0))
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    mat = material or (textured_material(image, filter) if textured else S.opaque())
    if textured and material is not None:
        mat.pattern = W.image_pattern(image, filter)
    return W.World(lights, [floor] + W.mesh(mesh, mat, textured=textured)).tables(S.camera())


def torus_instances(rtc, image, filter, textured=True):
    """Three instances of a torus (576 triangles) whose coordinates run around the ring and the tube."""
    from rtc_amd import world as W
    verts, faces = M.torus(24, 12)
    ang = np.arctan2(verts[:, 2], verts[:, 0]) / (2 * np.pi) + 0.5
    tube = np.arctan2(verts[:, 1], np.hypot(verts[:, 0], verts[:, 2]) - 1.0) / (2 * np.pi) + 0.5
    mesh = load(rtc, verts, faces, np.stack([ang, tube], axis=1))
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                    transform=W.translation(0, -1.3, 0))
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    half = W.scaling(0.6, 0.6, 0.6)
    places = [W.mat_mul(W.translation(-1.1, 0.0, 0.3), half),
              W.mat_mul(W.translation(1.0, 0.3, 0.5), W.mat_mul(W.rotation_x(0.9), half)),
              W.mat_mul(W.translation(0.0, -0.4, -0.6),
                        W.mat_mul(W.mat_mul(W.rotation_y(0.7), W.shearing(0.3, 0.0, 0.0, 0.2, 0.0, 0.0)), half))]
    pat = W.image_pattern(image, filter)
    mats = [W.Material(pattern=pat if textured else None, specular=0.5, shininess=60.0),
            W.Material(pattern=pat if textured else None, diffuse=0.7, specular=0.1),
            W.Material(pattern=pat if textured else None, specular=0.5, shininess=60.0)]
    inst = [W.instance(mesh, m, transform=p, textured=textured) for m, p in zip(mats, places)]
    return W.World(lights, [floor], inst).tables(S.camera())


QUAD = np.array([(-1.25, 0.0, -0.75), (1.5, 0.0, -0.75), (1.5, 0.0, 1.0), (-1.25, 0.0, 1.0)])


def quad(rtc, image, filter, mapped=True, eye=((0.2, 2.5, -2.0), (0.1, 0.0, 0.1), (0.0, 1.0, 0.0))):
    """A quad in the xz-plane, seen from above, whose coordinates are its vertices' (x, z) (mapped) or that has
    none (the planar map of the same points)."""
    from rtc_amd import world as W
    faces = np.array([(0, 1, 2), (0, 2, 3)])
    mesh = load(rtc, QUAD, faces, QUAD[:, [0, 2]], face_texcoords=None if mapped else [None, None])
    assert mesh.n_textured == (2 if mapped else 0)
    shapes = W.mesh(mesh, textured_material(image, filter), textured=True)
    return W.World([W.Light((-3.0, 6.0, -4.0))], shapes).tables(S.camera(eye=eye))


def box_world(rtc, image, filter, copies=1, coords_of_second=None, textured=True, color=None, image_of_second=None,
              smooth=False):
    """smooth_worlds.box_world's glass box (12 triangles, depth 4) with texture coordinates; copies = 2 doubles
    it (value-equal pairs) and coords_of_second gives the second copy other coordinates, image_of_second a
    pattern of its own over that array; textured=False: the oracle's world, glass of `color` without pattern;
    smooth: the vertex normals are the faces' own (smooth_worlds.box(True): flat shading through the smooth code)."""
    from rtc_amd import world as W
    verts, faces, normals, fnorm = S.box(True)
    tc = np.stack([0.5 + 0.25 * verts[:, 0] + 0.125 * verts[:, 2], 0.5 + 0.25 * verts[:, 1]], axis=1)
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                    transform=W.translation(0, -1.3, 0))
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    place = W.mat_mul(W.translation(0.1, 0.0, 0.3), W.mat_mul(W.rotation_y(0.5), W.scaling(0.8, 0.9, 0.7)))
    pat = W.image_pattern(image, filter) if textured else None
    shapes = [floor]
    for c in range(copies):
        glass = M.glass()
        glass.pattern = W.image_pattern(image_of_second, filter) if textured and c and image_of_second is not None else pat
        if color is not None:
            glass.color = tuple(color)
        t = tc if c == 0 or coords_of_second is None else coords_of_second
        mesh = load(rtc, verts, faces, t, normals=normals if smooth else None, face_normals=fnorm if smooth else None)
        shapes += W.mesh(mesh, glass, transform=place, textured=textured, smooth=smooth)
    return W.World(lights, shapes).tables(S.camera())


def without_textures(rtc, tables):
    """The same tables without coordinates, textures and image patterns (materials keep their colours)."""
    mats = type(tables.materials).from_buffer_copy(tables.materials)
    keep = [i for i, p in enumerate(tables.patterns) if p.kind != 6]
    renumber = {old: new for new, old in enumerate(keep)}
    pats = (rtc.PatternDesc * len(keep))(*[tables.patterns[i] for i in keep])
    for m in mats:
        m.pattern = renumber.get(m.pattern, -1)
    return rtc.SceneTables(tables.shapes, mats, pats, tables.lights, tables.camera, meshes=tables.meshes,
                           instances=tables.instances, smooth=tables.smooth)
