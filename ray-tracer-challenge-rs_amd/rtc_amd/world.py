"""Host-side world construction mirroring the reference's public Rust API.

    primitives/transformations.rs  translation, scaling, rotation_{x,y,z}, shearing, view_transform
    composites/material.rs         Material (Default, glass)
    shapes/*.rs                    Sphere, Plane, Cube, Cylinder, Cone, Triangle
    patterns/*.rs                  Stripe/Gradient/Ring/Checker/Complex/Test patterns
    primitives/light.rs            Light
    composites/world.rs            World (+ World.default(), world.rs:160-169)
    composites/camera.rs           Camera(h, v, fov).set_transformation(...)

Matrices are 4x4 f64 nested lists combined with the reference's left-fold
product (matrix.rs:317-330) and inverted by the C++ host (rt_matrix_inverse,
the cofactor inverse of matrix.rs:247-258), so the tables handed to the GPU
carry exactly the reference's f64 values.  `World.tables(camera)` flattens
the trait-object world into the rt_* descriptor arrays.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

from . import (AreaLightDesc, CameraDesc, InstanceDesc, LightDesc, MaterialDesc, MotionDesc, RT_MOVE_INSTANCE, RT_MOVE_SHAPE, PatternDesc, PATTERN_KINDS, RT_SMOOTH_SHAPES, TEXTURE_MAPS, UVMapDesc,
               SceneTables, ShapeDesc, SHAPE_KINDS, SmoothDesc, TEXTURE_FILTERS, UVDesc, camera_make, matrix_inverse)

F64_MAX = 1.7976931348623157e308
IDENTITY = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]


def mat_mul(a, b):
    """Matrix<4> * Matrix<4>: left fold from 0.0, no FMA (matrix.rs:317-330)."""
    r = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            acc = 0.0
            for k in range(4):
                acc = acc + a[i][k] * b[k][j]
            r[i][j] = acc
    return r


def translation(x, y, z):
    m = [row[:] for row in IDENTITY]
    m[0][3], m[1][3], m[2][3] = float(x), float(y), float(z)
    return m


def scaling(x, y, z):
    m = [row[:] for row in IDENTITY]
    m[0][0], m[1][1], m[2][2] = float(x), float(y), float(z)
    return m


def _rot(axis, theta):
    m = [row[:] for row in IDENTITY]
    c, s = math.cos(theta), math.sin(theta)
    if axis == 0:
        m[1][1], m[1][2], m[2][1], m[2][2] = c, -s, s, c
    elif axis == 1:
        m[0][0], m[0][2], m[2][0], m[2][2] = c, s, -s, c
    else:
        m[0][0], m[0][1], m[1][0], m[1][1] = c, -s, s, c
    return m


def rotation_x(t):
    return _rot(0, float(t))


def rotation_y(t):
    return _rot(1, float(t))


def rotation_z(t):
    return _rot(2, float(t))


def shearing(xy, xz, yx, yz, zx, zy):
    m = [row[:] for row in IDENTITY]
    m[0][1], m[0][2], m[1][0], m[1][2], m[2][0], m[2][1] = map(float, (xy, xz, yx, yz, zx, zy))
    return m


def inverse(m):
    return matrix_inverse([v for row in m for v in row]).tolist()


@dataclass
class Pattern:
    kind: str
    color_a: tuple = (1.0, 1.0, 1.0)
    color_b: tuple = (0.0, 0.0, 0.0)
    transformation_inverse: list = field(default_factory=lambda: [row[:] for row in IDENTITY])
    sub_a: "Pattern | None" = None
    sub_b: "Pattern | None" = None
    # an image pattern (rtc.h rt_scene_upload_textured): a uint8 array of shape (H, W, 3), row 0 at the top, and
    # the filter (TEXTURE_FILTERS); two patterns that hold the same array object share one texture of the upload
    image: object = field(default=None, compare=False)
    filter: int = 0
    # its texture map (rtc.h rt_scene_upload_mapped, TEXTURE_MAPS) and, for a cube map, the six faces' arrays
    # in the order left, front, right, back, up, down
    map: int = 0
    faces: object = field(default=None, compare=False)

    def set_transformation(self, m):
        self.transformation_inverse = inverse(m)
        return self


def stripe_pattern(a, b):
    return Pattern("stripe", tuple(a), tuple(b))


def gradient_pattern(a, b):
    return Pattern("gradient", tuple(a), tuple(b))


def ring_pattern(a, b):
    return Pattern("ring", tuple(a), tuple(b))


def checker_pattern(a, b):
    return Pattern("checker", tuple(a), tuple(b))


def complex_pattern(a: Pattern, b: Pattern):
    return Pattern("complex", sub_a=a, sub_b=b)


def _texture_array(image, who):
    import numpy as np
    img = np.ascontiguousarray(image, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] != 3 or not img.size:
        raise ValueError(f"{who} takes a uint8 array of shape (H, W, 3)")
    return img


def image_pattern(image, filter="nearest", map="planar"):
    """An image texture as a material's pattern (rtc.h rt_scene_upload_textured): `image` is a uint8 array of
    shape (H, W, 3), row 0 at the top (rtc_amd.read_image); a triangle with texture coordinates samples it at
    the interpolated (u, v), every other hit through `map` of the pattern-space point: "planar", "spherical"
    or "cylindrical" (rtc.h rt_scene_upload_mapped)."""
    if map not in ("planar", "spherical", "cylindrical"):
        raise ValueError("image_pattern: map is 'planar', 'spherical' or 'cylindrical' (cube_map_pattern makes a cube map)")
    return Pattern("image", image=_texture_array(image, "image_pattern"), filter=TEXTURE_FILTERS[filter],
                   map=TEXTURE_MAPS[map])


def cube_map_pattern(left, front, right, back, up, down, filter="nearest"):
    """A cube map (rtc.h RT_MAP_CUBE): six images, one per face of the cube |x|, |y|, |z| <= 1 in pattern
    space.  A triangle with texture coordinates samples `front`."""
    faces = [_texture_array(f, "cube_map_pattern") for f in (left, front, right, back, up, down)]
    return Pattern("image", image=faces[1], filter=TEXTURE_FILTERS[filter], map=TEXTURE_MAPS["cube"], faces=faces)


def test_pattern():
    return Pattern("test")


@dataclass
class Material:
    """material.rs:8-20; defaults material.rs:157-161."""
    color: tuple = (1.0, 1.0, 1.0)
    pattern: Pattern | None = None
    ambient: float = 0.1
    diffuse: float = 0.9
    specular: float = 0.9
    shininess: float = 200.0
    reflectiveness: float = 0.0
    refractive_index: float = 1.0
    transparency: float = 0.0
    casts_shadow: bool = True

    @staticmethod
    def glass() -> "Material":  # material.rs:148-154
        return Material(transparency=1.0, refractive_index=1.5)


@dataclass
class Shape:
    kind: str
    material: Material = field(default_factory=Material)
    transformation_inverse: list = field(default_factory=lambda: [row[:] for row in IDENTITY])
    minimum: float = -F64_MAX
    maximum: float = F64_MAX
    closed: bool = False
    triangle: tuple | None = None  # (v1, e1, e2, normal)
    normals: tuple | None = None   # a smooth triangle's (n1, n2, n3), used as given; None: flat
    uvs: tuple | None = None       # a triangle's texture coordinates (t1, t2, t3) of p1, p2, p3; None: none
    velocity: tuple | None = None  # world units per unit of time (rtc.h rt_scene_upload_moving); None: static

    def set_transformation(self, m):
        self.transformation_inverse = inverse(m)
        return self


def sphere(material=None, transform=None):
    s = Shape("sphere", material or Material())
    return s.set_transformation(transform) if transform is not None else s


def plane(material=None, transform=None):
    s = Shape("plane", material or Material())
    return s.set_transformation(transform) if transform is not None else s


def cube(material=None, transform=None):
    s = Shape("cube", material or Material())
    return s.set_transformation(transform) if transform is not None else s


def cylinder(minimum=-F64_MAX, maximum=F64_MAX, closed=False, material=None, transform=None):
    s = Shape("cylinder", material or Material(), minimum=float(minimum), maximum=float(maximum), closed=closed)
    return s.set_transformation(transform) if transform is not None else s


def cone(minimum=-F64_MAX, maximum=F64_MAX, closed=False, material=None, transform=None):
    s = Shape("cone", material or Material(), minimum=float(minimum), maximum=float(maximum), closed=closed)
    return s.set_transformation(transform) if transform is not None else s


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):  # vector.rs:97-103 (mul_add: exact via math.fma when available)
    fma = getattr(math, "fma", None)
    if fma is None:  # Python < 3.13: emulate a correctly rounded fma through fractions
        from fractions import Fraction

        def fma(x, y, z):
            r = Fraction(x) * Fraction(y) + Fraction(z)
            # an exact zero keeps IEEE's sign (-0 + -0 = -0, as mul_add gives): the product is then
            # exactly -z, so the plain float expression has no rounding and the right zero
            return float(r) if r != 0 else x * y + z
    return (fma(a[1], b[2], -a[2] * b[1]), fma(a[2], b[0], -a[0] * b[2]), fma(a[0], b[1], -a[1] * b[0]))


def triangle(p1, p2, p3, material=None):
    """triangle.rs:21-35: edges and normal = normalize(e2 x e1)."""
    e1, e2 = _sub(p2, p1), _sub(p3, p1)
    n = _cross(e2, e1)
    mag = math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    n = (n[0] / mag, n[1] / mag, n[2] / mag)
    return Shape("triangle", material or Material(), triangle=(tuple(map(float, p1)), e1, e2, n))


def smooth_triangle(p1, p2, p3, n1, n2, n3, material=None):
    """The book's smooth triangle: triangle(p1, p2, p3) with the vertex normals n1, n2, n3 of p1, p2, p3, used
    as given (rtc.h rt_scene_upload_smooth): the normal at a hit is n2 u + n3 v + n1 (1 - u - v)."""
    s = triangle(p1, p2, p3, material)
    s.normals = tuple(tuple(map(float, n)) for n in (n1, n2, n3))
    return s


def textured_triangle(p1, p2, p3, t1, t2, t3, material=None):
    """triangle(p1, p2, p3) with the texture coordinates t1, t2, t3 of p1, p2, p3 (rtc.h
    rt_scene_upload_textured): an image pattern is sampled at t2 u + t3 v + t1 (1 - u - v)."""
    s = triangle(p1, p2, p3, material)
    s.uvs = tuple(tuple(map(float, t)) for t in (t1, t2, t3))
    return s


def mesh(m, material=None, transform=None, bake=False, smooth=False, textured=False):
    """The faces of a Mesh (rtc_amd.load_obj) as Triangle shapes sharing `material`, through the host's
    rt_mesh_triangles: Triangle::new per face; with `transform` either set_transformation on every triangle
    (bake=False) or the vertices multiplied by it first (bake=True, identity inverse).  smooth=True makes the
    faces that name three normals (load_obj(..., normals=True)) smooth triangles; the others stay flat.
    textured=True gives the faces that name three texture coordinates (load_obj(..., texcoords=True)) theirs."""
    mat = material or Material()
    t = None if transform is None else [v for row in transform for v in row]
    out = []
    for d in m.shape_descs(t, bake):
        inv = [list(d.inverse[4 * i:4 * i + 4]) for i in range(4)]
        out.append(Shape("triangle", mat, transformation_inverse=inv,
                         triangle=(tuple(d.vertex_1), tuple(d.edge_1), tuple(d.edge_2), tuple(d.normal))))
    if smooth:
        for d in m.smooth_descs(t, bake):
            out[d.index].normals = (tuple(d.normal_1), tuple(d.normal_2), tuple(d.normal_3))
    if textured:
        for d in m.uv_descs():
            out[d.index].uvs = (tuple(d.uv_1), tuple(d.uv_2), tuple(d.uv_3))
    return out


@dataclass
class Instance:
    """One placement of a Mesh (rtc.h rt_instance_desc): in World.instances it stands for what
    mesh(m, material, transform) appends to World.shapes, triangle for triangle, after every shape."""
    mesh: object
    material: Material = field(default_factory=Material)
    transformation_inverse: list = field(default_factory=lambda: [row[:] for row in IDENTITY])
    smooth: bool = False  # the mesh's faces with three normals are smooth triangles (another mesh than its flat use)
    textured: bool = False  # the mesh's faces with three texture coordinates carry them (another mesh again)
    velocity: tuple | None = None  # the placement's velocity (rtc.h rt_scene_upload_moving); None: static


def instance(m, material=None, transform=None, smooth=False, textured=False):
    """A Mesh (rtc_amd.load_obj) placed by `transform` with `material`: an Instance for World.instances.
    The device keeps the mesh's triangles once however many instances place it.  smooth=True: the faces
    that name three normals are smooth triangles and keep their local normals under the placement;
    textured=True: the faces that name three texture coordinates keep them under every placement."""
    i = Instance(m, material or Material(), smooth=smooth, textured=textured)
    if transform is not None:
        i.transformation_inverse = inverse(transform)
    return i


@dataclass
class Light:
    position: tuple
    intensity: tuple = (1.0, 1.0, 1.0)


@dataclass
class AreaLight:
    """An area light (rtc.h rt_scene_upload_lit): the parallelogram corner + s full_uvec + t full_vvec, cut
    into usteps x vsteps cells with one sample each; jitter False = the cells' centres, True = hashed per ray
    with `seed`.  It means usteps * vsteps point lights of intensity / (usteps * vsteps)."""
    corner: tuple
    full_uvec: tuple
    full_vvec: tuple
    usteps: int = 1
    vsteps: int = 1
    intensity: tuple = (1.0, 1.0, 1.0)
    jitter: bool = False
    seed: int = 0

    def desc(self) -> AreaLightDesc:
        d = AreaLightDesc()
        d.corner[:] = list(map(float, self.corner))
        d.full_uvec[:] = list(map(float, self.full_uvec))
        d.full_vvec[:] = list(map(float, self.full_vvec))
        d.intensity[:] = list(map(float, self.intensity))
        d.usteps, d.vsteps = int(self.usteps), int(self.vsteps)
        d.jitter, d.seed = int(self.jitter), int(self.seed) & 0xFFFFFFFF
        return d


@dataclass
class World:
    lights: list = field(default_factory=list)
    shapes: list = field(default_factory=list)
    instances: list = field(default_factory=list)  # of Instance: their triangles follow the shapes in world order
    area_lights: list = field(default_factory=list)  # of AreaLight: their samples follow the lights in the light list

    @staticmethod
    def default() -> "World":
        """world.rs:160-169 with utils.rs:59-71."""
        s1 = sphere(Material(color=(0.8, 1.0, 0.6), diffuse=0.7, specular=0.2))
        s2 = sphere(transform=scaling(0.5, 0.5, 0.5))
        return World([Light((-10.0, 10.0, -10.0), (1.0, 1.0, 1.0))], [s1, s2])

    def tables(self, camera: CameraDesc | None = None) -> SceneTables:
        """Flatten into rt_* descriptor tables (one material entry per shape)."""
        pats: list[Pattern] = []

        def pat_index(p: Pattern | None) -> int:
            if p is None:
                return -1
            for i, q in enumerate(pats):
                if q is p:
                    return i
            pats.append(p)
            idx = len(pats) - 1
            if p.kind == "complex":
                pat_index(p.sub_a)
                pat_index(p.sub_b)
            return idx

        def put_material(md, m):
            md.color[:] = list(map(float, m.color))
            md.ambient, md.diffuse, md.specular, md.shininess = m.ambient, m.diffuse, m.specular, m.shininess
            md.reflectiveness, md.transparency, md.refractive_index = (m.reflectiveness, m.transparency,
                                                                       m.refractive_index)
            md.casts_shadow = int(m.casts_shadow)
            md.pattern = pat_index(m.pattern)

        shapes = (ShapeDesc * len(self.shapes))()
        # one material entry per shape, then one per instance
        mats = (MaterialDesc * (len(self.shapes) + len(self.instances)))()
        meshes, mesh_of, inst = [], [], (InstanceDesc * len(self.instances))()
        smooth = []  # SmoothDesc entries: the meshes' in mesh order, then the shapes'
        uvs = []     # UVDesc entries, in the same order
        textures = []  # the image patterns' arrays, one entry per array object
        for k, it in enumerate(self.instances):
            for j, seen in enumerate(mesh_of):
                if seen[0] is it.mesh and seen[1] == (bool(it.smooth), bool(it.textured)):
                    inst[k].mesh = j
                    break
            else:
                inst[k].mesh = len(meshes)
                mesh_of.append((it.mesh, (bool(it.smooth), bool(it.textured))))
                meshes.append(it.mesh.shape_descs())  # local triangles: identity inverse
                if it.smooth:
                    smooth.extend(it.mesh.smooth_descs(list_index=inst[k].mesh))
                if it.textured:
                    uvs.extend(it.mesh.uv_descs(list_index=inst[k].mesh))
            inst[k].material = len(self.shapes) + k
            inst[k].inverse[:] = [float(v) for row in it.transformation_inverse for v in row]
            put_material(mats[len(self.shapes) + k], it.material)
        for i, s in enumerate(self.shapes):
            d = shapes[i]
            d.kind = SHAPE_KINDS[s.kind]
            d.material = i
            d.inverse[:] = [float(v) for row in s.transformation_inverse for v in row]
            d.minimum, d.maximum, d.closed = s.minimum, s.maximum, int(s.closed)
            if s.triangle:
                d.vertex_1[:], d.edge_1[:], d.edge_2[:], d.normal[:] = [list(map(float, v)) for v in s.triangle]
            put_material(mats[i], s.material)
            if s.normals is not None:
                e = SmoothDesc(RT_SMOOTH_SHAPES, i)
                e.normal_1[:], e.normal_2[:], e.normal_3[:] = [list(map(float, n)) for n in s.normals]
                smooth.append(e)
            if s.uvs is not None:
                e = UVDesc(RT_SMOOTH_SHAPES, i)
                e.uv_1[:], e.uv_2[:], e.uv_3[:] = [list(map(float, t)) for t in s.uvs]
                uvs.append(e)
        maps = []  # UVMapDesc entries: the image patterns whose map is not the planar one

        def texture_index(image) -> int:
            for j, t in enumerate(textures):
                if t is image:
                    return j
            textures.append(image)
            return len(textures) - 1

        ptab = (PatternDesc * len(pats))()
        for i, p in enumerate(pats):
            d = ptab[i]
            d.kind = PATTERN_KINDS[p.kind]
            d.color_a[:] = list(map(float, p.color_a))
            d.color_b[:] = list(map(float, p.color_b))
            d.inverse[:] = [float(v) for row in p.transformation_inverse for v in row]
            d.sub_a = pats.index(p.sub_a) if p.sub_a is not None else -1
            d.sub_b = pats.index(p.sub_b) if p.sub_b is not None else -1
            if p.kind == "image":
                d.sub_a = texture_index(p.image)
                d.reserved = int(p.filter)
                if p.map:
                    e = UVMapDesc(i, int(p.map))
                    e.faces[:] = [texture_index(f) for f in p.faces] if p.faces is not None else [-1] * 6
                    maps.append(e)
        motion = []  # MotionDesc entries: the moving shapes in world order, then the moving instances
        for target, things in ((RT_MOVE_SHAPE, self.shapes), (RT_MOVE_INSTANCE, self.instances)):
            for i, s in enumerate(things):
                if s.velocity is not None:
                    e = MotionDesc(target, i)
                    e.velocity[:] = list(map(float, s.velocity))
                    motion.append(e)
        lts = (LightDesc * len(self.lights))()
        for i, lt in enumerate(self.lights):
            lts[i].position[:] = list(map(float, lt.position))
            lts[i].intensity[:] = list(map(float, lt.intensity))
        return SceneTables(shapes, mats, ptab, lts, camera if camera is not None else CameraDesc(),
                           meshes=meshes or None, instances=inst if len(inst) else None,
                           smooth=(SmoothDesc * len(smooth))(*smooth) if smooth else None,
                           uvs=(UVDesc * len(uvs))(*uvs) if uvs else None, textures=textures or None,
                           area_lights=(AreaLightDesc * len(self.area_lights))(*[a.desc() for a in self.area_lights])
                           if self.area_lights else None,
                           maps=(UVMapDesc * len(maps))(*maps) if maps else None,
                           motion=(MotionDesc * len(motion))(*motion) if motion else None)


def camera(width, height, fov, frm=(0, 0, 0), to=(0, 0, -1), up=(0, 1, 0)) -> CameraDesc:
    """Camera::new(width, height, fov).set_transformation(view_transform(from, to, up))."""
    return camera_make(width, height, fov, frm, to, up)
