"""Moving smooth and textured triangles (tests/test_gpu_motion_meshes.py, tests/test_motion_random_cpu.py).

No oracle world can hold them: the references are the numpy restatements (tests/smooth_reference.py,
tests/texture_reference.py) applied to the world at each ray's time, motion_reference.trace_at_times.  Every
world is one of tests/smooth_worlds.py's or tests/texture_worlds.py's with a motion list attached:

  smooth_instance, flat_instance   ico_instances: two instances of the 80-triangle icosphere, the second one
                 (rotated and sheared) moving.  Smooth: the smooth_inst rows of a moving instance and the
                 displaced origin of prepare_hit's repeated triangle test, whose u and v weigh the vertex
                 normals.  Flat: the control, which never looks at u and v;
  smooth_tree    ico_alone: 320 top-level smooth triangles, enough for a triangle hierarchy, of which every 7th
                 moves along its own flat normal, 0.8 per unit of time.  Triangle::new's normal of these faces
                 points into the icosphere, so those movers sink into it and are seen through the holes they
                 leave; every 7th from the third on moves the other way, out towards the eye.  plan_triangles keeps the movers out of the
                 tree and puts them behind its leaves: their rows of smooth_plain are indexed after that reordering;
  texture_<filter>_<flat|smooth>   texture_worlds.ico_alone with an 8 x 4 texture and the same movers: the rows
                 of uv_plain, both filters, and smooth_plain beside them;
  texture_instance   two instances of the textured 80-triangle icosphere, the sheared one moving: uv_inst rows
                 of a moving instance.  (texture_worlds.torus_instances and box_world stand over a plane, for
                 which the restatements do not speak: this is smooth_worlds.ico_instances with coordinates.)

batch(name): the world's camera rays on 48 x 36 and 512 rays aimed at the movers (those that leave the
icosphere on the eye's side) where they are at the ray's time; ray k has time TIMES[k mod 4].
"""
import functools

import numpy as np

import mesh_worlds as M
import rtc_amd
import smooth_reference
import smooth_worlds as S
import texture_reference
import texture_worlds as T
from rtc_amd import world as W

TIMES = (0.25, 0.5, 0.75, 1.0)
RAY_FRAME = (48, 36)
AIMED = 512
DEPTH = 2
EVERY = 7
OUTWARD = 3
SPEED = 0.8
V_INSTANCE = (-0.9, 0.2, 0.3)
FENCE = 1e-9    # a ray whose reference margin is at most this sits on a decision fence and is left out
MAX_LEFT_OUT = 0.01


def _move_every_seventh(tables):
    """Every 7th top-level triangle (0, 7, ...) moves along its flat normal, and every 7th from the third on
    (3, 10, ...) against it."""
    movers = [i for i in range(len(tables.shapes)) if i % EVERY in (0, OUTWARD)]
    motion = (rtc_amd.MotionDesc * len(movers))()
    for e, i in zip(motion, movers):
        e.target, e.index = rtc_amd.RT_MOVE_SHAPE, i
        e.velocity[:] = [(SPEED if i % EVERY == 0 else -SPEED) * c for c in tables.shapes[i].normal]
    tables.motion = motion
    return tables


def _move_second_instance(tables):
    motion = (rtc_amd.MotionDesc * 1)()
    motion[0].target, motion[0].index = rtc_amd.RT_MOVE_INSTANCE, 1
    motion[0].velocity[:] = list(V_INSTANCE)
    tables.motion = motion
    return tables


def _textured_instances(filter):
    """smooth_worlds.ico_instances with a texture coordinate per vertex and the image pattern on both."""
    verts, faces = M.icosphere(1)
    mesh = T.load(rtc_amd, verts, faces, T.ico_coords(verts))
    small = W.scaling(0.7, 0.7, 0.7)
    places = [W.mat_mul(W.translation(-0.8, 0.1, 0.2), small),
              W.mat_mul(W.translation(0.75, -0.1, 0.5),
                        W.mat_mul(W.mat_mul(W.rotation_y(0.7), W.shearing(0.3, 0.0, 0.0, 0.2, 0.0, 0.0)), small))]
    pat = W.image_pattern(T.colors(8, 4), filter)
    mats = [W.Material(pattern=pat, specular=0.5, shininess=60.0), W.Material(pattern=pat, diffuse=0.7, specular=0.1)]
    inst = [W.instance(mesh, m, transform=p, textured=True) for m, p in zip(mats, places)]
    return W.World([S.eye_light()], [], inst).tables(S.camera())


WORLDS = {
    "smooth_instance": (lambda: _move_second_instance(S.ico_instances(rtc_amd, smooth=True)), smooth_reference.trace),
    "flat_instance": (lambda: _move_second_instance(S.ico_instances(rtc_amd, smooth=False)), smooth_reference.trace),
    "smooth_tree": (lambda: _move_every_seventh(S.ico_alone(rtc_amd)), smooth_reference.trace),
    "texture_nearest_flat": (lambda: _move_every_seventh(T.ico_alone(rtc_amd, T.colors(8, 4), "nearest", smooth=False)),
                             texture_reference.trace),
    "texture_nearest_smooth": (lambda: _move_every_seventh(T.ico_alone(rtc_amd, T.colors(8, 4), "nearest", smooth=True)),
                               texture_reference.trace),
    "texture_bilinear_flat": (lambda: _move_every_seventh(T.ico_alone(rtc_amd, T.colors(8, 4), "bilinear", smooth=False)),
                              texture_reference.trace),
    "texture_bilinear_smooth": (lambda: _move_every_seventh(T.ico_alone(rtc_amd, T.colors(8, 4), "bilinear", smooth=True)),
                                texture_reference.trace),
    "texture_instance": (lambda: _move_second_instance(_textured_instances("nearest")), texture_reference.trace),
}
NAMES = tuple(WORLDS)
TOP_LEVEL = tuple(n for n in NAMES if not n.endswith("instance"))
# the static twins whose recorded f32 shares the moving ones are compared with (profiles/smooth_parity.json,
# profiles/texture_parity.json; tests/f32_tolerance_motion.py STATIC_TWINS)


@functools.lru_cache(maxsize=None)
def world(name):
    return WORLDS[name][0]()


def mover_shapes(name):
    """The world indices (of the expansion) of the moving triangles."""
    tables = world(name)
    if name in TOP_LEVEL:
        return np.array([m.index for m in tables.motion])
    return np.arange(80, 160)  # the second instance's triangles follow the first one's


@functools.lru_cache(maxsize=None)
def batch(name):
    """(rays (1728 + 512, 6), times), read-only."""
    tables = world(name)
    cam = rtc_amd.camera_resize(tables.camera, *RAY_FRAME)
    eye_rays = S.camera_rays(cam)
    n = len(eye_rays) + AIMED
    times = np.array(TIMES)[np.arange(n) % len(TIMES)]
    rng = np.random.default_rng(31)
    eye = np.array(cam.origin[:])[:3]
    aimed = np.zeros((AIMED, 6))
    if name in TOP_LEVEL:  # the movers that leave the icosphere on the eye's side
        front = [m for m in tables.motion if m.index % EVERY == OUTWARD and
                 np.dot(tables.shapes[m.index].normal[:], np.array(tables.shapes[m.index].vertex_1[:]) - eye) > 0.5]
        assert len(front) >= 8, len(front)
    for j in range(AIMED):
        tau = times[len(eye_rays) + j]
        if name in TOP_LEVEL:
            m = front[j % len(front)]
            s = tables.shapes[m.index]
            a, b = rng.uniform(0.15, 0.4, size=2)  # well inside the triangle
            point = np.array(s.vertex_1[:]) + a * np.array(s.edge_1[:]) + b * np.array(s.edge_2[:])
            point = point + np.array(m.velocity[:]) * tau
        else:
            u = rng.normal(size=3)
            centre = np.linalg.inv(np.array(tables.instances[1].inverse[:]).reshape(4, 4))[:3, 3]
            point = centre + np.array(V_INSTANCE) * tau + 0.3 * rng.uniform(0.0, 1.0) * u / np.linalg.norm(u)
        o = eye + rng.uniform(-0.2, 0.2, size=3)
        d = point - o
        aimed[j, :3], aimed[j, 3:] = o, d / np.linalg.norm(d)
    rays = np.ascontiguousarray(np.concatenate([eye_rays, aimed], axis=0))
    rays.setflags(write=False)
    times.setflags(write=False)
    return rays, times


_REF = {}


def reference(name):
    """(colours, hits, margins, kept: the rays off every decision fence) of the restatement; computed once."""
    import motion_reference as MR
    if name not in _REF:
        rays, times = batch(name)
        cols, hit, margin = MR.trace_at_times(WORLDS[name][1], world(name), rays, times)
        for a in (cols, hit["t"], hit["shape"], margin):
            a.setflags(write=False)
        _REF[name] = (cols, hit, margin, margin > FENCE)
    return _REF[name]
