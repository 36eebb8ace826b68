"""Worlds of the texture-map tests (tests/test_uv_maps_cpu.py, tests/test_gpu_uv_maps.py).

Frames are 64 x 48, ray batches 2048 rays.

designed(): one unit shape at the origin whose material shows its pattern alone (ambient 1, diffuse 0,
specular 0, one white light), for rays aimed at known surface points.

tie(): a shape over a checkered floor whose image pattern coincides with the oracle's stripe_pattern(a, b):
  a unit sphere under the spherical map and a unit cylinder under the cylindrical map with the 2 x 1 texture
  [a b] under the nearest filter: u < 0.5 exactly where x > 0, and stripe_pattern gives a there (floor(x) = 0);
  a unit cube under a cube map with front, up and down [b a] (u = (x + 1) / 2), back [a b] (u = (1 - x) / 2),
  left the 1 x 1 texture a (the over point's x is -1 - 8e-8, whose floor is -2) and right the 1 x 1 texture b
  (x = 1 + 8e-8, floor 1).
The two differ only on the planes x = 0 and x = +-1.  (rtc.h's u runs against x on the sphere, so the
sphere's and the cylinder's texture is [a b], not [b a].)
"""
import functools

import numpy as np

import mesh_worlds as M
import uv_map_reference as U

FRAME = (64, 48)
N_RAYS = 2048
SEED = 20
A, B = (200, 40, 90), (30, 220, 140)
A1, B1 = tuple(c / 255.0 for c in A), tuple(c / 255.0 for c in B)
TWO_AB = np.array([[A, B]], dtype=np.uint8)
TWO_BA = np.array([[B, A]], dtype=np.uint8)
ONE_A = np.array([[A]], dtype=np.uint8)
ONE_B = np.array([[B]], dtype=np.uint8)
SHAPES = ("sphere", "cylinder", "cube")
MAPS = ("spherical", "cylindrical", "cube")
# (shape, map, pattern turned) of the designed rays.  The cube under the cylindrical map with no pattern
# transformation is left out: the over points of its top and bottom faces have y = +-(1 + 8e-8), within 1e-6 of
# the jump of floor(y), so a third of the batch would have to be left out.
DESIGNED = [(s, m, t) for s in SHAPES for m in MAPS for t in (False, True) if (s, m, t) != ("cube", "cylindrical", False)]
NATURAL = {"sphere": "spherical", "cylinder": "cylindrical", "cube": "cube"}
KIND = {"planar": U.PLANAR, "spherical": U.SPHERICAL, "cylindrical": U.CYLINDRICAL, "cube": U.CUBE}
LENS = (0.05, 3.4)  # aperture and focal distance of the lens frames


def colors(width, height, seed):
    """A (height, width, 3) uint8 texture of distinct, well separated colours (texture_worlds.colors)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(height, width, 3), dtype=np.uint8)
    img[..., 0] = (np.arange(width * height).reshape(height, width) * 97 + 31 + 13 * seed) % 256
    return np.ascontiguousarray(img)


@functools.lru_cache(maxsize=None)
def face_images():
    """Six 5 x 7 textures, no two alike (left, front, right, back, up, down)."""
    return tuple(colors(5, 7, 40 + f) for f in range(6))


def turned():
    """A pattern transformation with a rotation and a non-uniform scale (its inverse orients the map)."""
    from rtc_amd import world as W
    return W.mat_mul(W.rotation_z(0.5), W.mat_mul(W.rotation_y(0.7), W.scaling(0.8, 1.3, 1.1)))


def mapped_pattern(map_name, filt, images=None, transform=None):
    from rtc_amd import world as W
    if map_name == "cube":
        p = W.cube_map_pattern(*(images if images is not None else face_images()), filter=filt)
    else:
        p = W.image_pattern(images if images is not None else face_images()[1], filt, map=map_name)
    return p.set_transformation(transform) if transform is not None else p


def unit_shape(shape, material, transform=None):
    from rtc_amd import world as W
    if shape == "sphere":
        return W.sphere(material, transform=transform)
    if shape == "cylinder":
        return W.cylinder(-1.0, 1.0, True, material, transform=transform)
    return W.cube(material, transform=transform)


def designed(shape, map_name, filt, transform=None):
    """The unit `shape` at the origin showing its pattern alone."""
    from rtc_amd import world as W
    mat = W.Material(ambient=1.0, diffuse=0.0, specular=0.0, pattern=mapped_pattern(map_name, filt, transform=transform))
    return W.World([W.Light((-4.0, 6.0, -5.0), (1.0, 1.0, 1.0))], [unit_shape(shape, mat)]).tables(camera())


def designed_reference(shape, map_name, filt, transform=None):
    """(rays, colours, margin) of the designed rays by the restatement; read-only."""
    from rtc_amd import world as W
    rays, over = U.designed_rays(shape, N_RAYS, SEED)
    pinv = W.inverse(transform) if transform is not None else np.eye(4)
    pp = U.mul_point(pinv, over)
    images = face_images() if map_name == "cube" else face_images()[1]
    rgb, margin = U.colour(KIND[map_name], images, 0 if filt == "nearest" else 1, pp)
    for a in (rays, rgb, margin):
        a.setflags(write=False)
    return rays, rgb, margin


def camera(eye=((0.9, 1.4, -4.3), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0)), fov=0.75):
    from rtc_amd import world as W
    return W.camera(*FRAME, fov, *eye)


def tie_pattern(shape, mapped, shift=0.0, probe=False):
    """The shape's pattern in the mapped world, or the oracle's stripes moved by `shift` along x; `probe`: the
    stripes twice as wide, whose only edge near the shape is the plane x = 0."""
    from rtc_amd import world as W
    if not mapped:
        t = W.translation(shift, 0.0, 0.0)
        return W.stripe_pattern(A1, B1).set_transformation(W.mat_mul(t, W.scaling(2.0, 1.0, 1.0)) if probe else t)
    if shape == "cube":
        return W.cube_map_pattern(ONE_A, TWO_BA, ONE_B, TWO_AB, TWO_BA, TWO_BA, filter="nearest")
    return W.image_pattern(TWO_AB, "nearest", map=NATURAL[shape])


def tie(shape, mapped, glass=False, area=False, shift=0.0, probe=False):
    """The shape, turned and moved, over a checkered floor; `glass`: a glass sphere between the camera and the
    shape (the pool kernel); `area`: a 2 x 2 area light in place of the point light."""
    from rtc_amd import world as W
    place = W.mat_mul(W.translation(0.1, 0.2, 0.3), W.mat_mul(W.rotation_y(0.45), W.rotation_x(-0.3)))
    if shape == "cylinder":
        # its lines x = +-1, where the over point's offset carries x beyond the stripes' edge along the whole
        # height, turned out of the camera's sight (the sphere has two such points, the cube's faces are meant)
        place = W.mat_mul(W.translation(0.1, 0.2, 0.3), W.rotation_y(-0.2))
    mat = W.Material(pattern=tie_pattern(shape, mapped, shift, probe), specular=0.3, shininess=40.0)
    shapes = [W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                      transform=W.translation(0.0, -1.6, 0.0)),
              unit_shape(shape, mat, place)]
    if glass:
        shapes.append(W.sphere(M.glass(), transform=W.mat_mul(W.translation(0.5, 0.7, -2.2), W.scaling(0.45, 0.45, 0.45))))
    lights = [W.Light((4.0, 5.0, -3.0), (0.35, 0.35, 0.3))]
    world = W.World(lights, shapes)
    if area:
        world.area_lights = [W.AreaLight((-5.5, 6.0, -5.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 2, 2, (0.7, 0.7, 0.7))]
    else:
        lights.append(W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)))
    return world.tables(camera())


def uniform(width, height, rgb):
    return np.ascontiguousarray(np.broadcast_to(np.array(rgb, dtype=np.uint8), (height, width, 3)))
