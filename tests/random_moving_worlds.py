"""Seeded random moving worlds (tests/test_motion_random_cpu.py, tests/test_gpu_motion_random.py).

The world of a seed is tests/random_worlds.py's random_world(seed) as it is, with a motion list attached to the
finished tables.  The list comes from a generator of its own (default_rng(7000 + seed)), so the base world of a
seed is the one the static tests render:

  - every shape, planes included, moves with probability 1/2, each velocity component uniform in [-2, 2] (three
    draws and one decision per shape in world order, taken whether or not the shape moves);
  - a shape that is value-equal to an earlier one (shape_identity.hpp's shape_eq before velocities, restated in
    classes() below) takes that shape's velocity or none: the pair stays one identity class that moves together,
    and the moving world and at_time(tau) have the same classes at every tau, 0 included;
  - at least one bounded shape moves: the first one is made to when the draw gave none;
  - five seeds (REDRAWN) take a later list of the same generator: their first one left less than 5 % of the
    batch's rays seeing the motion, a condition on the inputs that tests/test_motion_random_cpu.py holds;
  - seeds that are multiples of 3 carry their first light as a 2 x 2 area light of unit edges (1, 0, 0) and
    (0, 0, 1) centred on its position, cell centres, with the light's intensity: expanded() gives the oracle four
    point lights of a quarter of it.

batch(seed) is 2048 rays: 1024 camera rays (the seed's camera on 32 x 32) and 1024 rays from origins uniform in
the box [-4, 4] x [-1.5, 4] x [-6, 4] with random unit directions, so that origins lie inside movers and the
containers walk starts with entries at t < 0.  Ray k has time TIMES[k mod 4].
"""
import functools

import numpy as np

import motion_reference as MR
import rtc_amd
from random_worlds import random_world

SEEDS = tuple(range(24))
TIMES = (0.0, 0.3, 0.7, 1.0)
N_RAYS = 2048
FRAME = (70, 22)  # ragged against the 64 x 4 tile
GRID = 2
# Seeds whose first list left less than 5 % of the batch's rays seeing the motion (a few small movers away from
# the camera's centre; tests/test_motion_random_cpu.py holds that bar on the oracle alone): they take a later
# list of the same generator, the number says how many lists are drawn and dropped first.
REDRAWN = {2: 1, 4: 2, 11: 1, 13: 1, 23: 1}
KINDS = {0: "sphere", 1: "plane", 2: "cube", 3: "cylinder", 4: "cone", 5: "triangle"}
assert KINDS == {v: k for k, v in rtc_amd.SHAPE_KINDS.items()}


def _pattern_key(P, i, depth=0):
    if i < 0 or depth > 16:
        return None
    p = P[i]
    if p.kind == rtc_amd.PATTERN_KINDS["complex"]:
        return (p.kind, tuple(p.inverse), _pattern_key(P, p.sub_a, depth + 1), _pattern_key(P, p.sub_b, depth + 1))
    return (p.kind, tuple(p.inverse), tuple(p.color_a), tuple(p.color_b))


def _shape_key(tables, i):
    """The values shape_eq compares (f64 ==: tuples of floats compare -0 and +0 alike)."""
    s, m = tables.shapes[i], tables.materials[tables.shapes[i].material]
    key = [s.kind, tuple(s.inverse)]
    if KINDS[s.kind] in ("cylinder", "cone"):
        key += [s.minimum, s.maximum, s.closed != 0]
    if KINDS[s.kind] == "triangle":
        key += [tuple(s.vertex_1), tuple(s.edge_1), tuple(s.edge_2), tuple(s.normal)]
    key += [tuple(m.color), m.ambient, m.diffuse, m.specular, m.shininess, m.reflectiveness, m.transparency,
            m.refractive_index, m.casts_shadow != 0, _pattern_key(tables.patterns, m.pattern)]
    return tuple(key)


def classes(tables):
    """cls[i]: the smallest world index whose shape is value-equal to shape i (velocities aside)."""
    first, cls = {}, []
    for i in range(len(tables.shapes)):
        cls.append(first.setdefault(_shape_key(tables, i), i))
    return cls


@functools.lru_cache(maxsize=None)
def world(seed):
    """(tables with their motion list, the seed's camera, its depth); read-only."""
    tables, cam, depth = random_world(seed)
    rng = np.random.default_rng(7000 + seed)
    n = len(tables.shapes)
    cls = classes(tables)
    moves = np.zeros(n, dtype=bool)
    vel = np.zeros((n, 3))
    for _ in range(1 + REDRAWN.get(seed, 0)):
        for i in range(n):
            moves[i] = rng.random() < 0.5
            vel[i] = rng.uniform(-2.0, 2.0, size=3)
    for i in range(n):  # one class, one velocity
        moves[i], vel[i] = moves[cls[i]], vel[cls[i]]
    bounded = [i for i in range(n) if KINDS[tables.shapes[i].kind] != "plane"]
    if not moves[bounded].any():
        for i in range(n):
            if cls[i] == bounded[0]:
                moves[i] = True
    movers = np.nonzero(moves)[0]
    motion = (rtc_amd.MotionDesc * len(movers))()
    for e, i in zip(motion, movers):
        e.target, e.index = rtc_amd.RT_MOVE_SHAPE, int(i)
        e.velocity[:] = [float(c) for c in vel[i]]
    tables.motion = motion
    if seed % 3 == 0:
        first = tables.lights[0]
        area = rtc_amd.AreaLightDesc()
        area.corner[:] = [first.position[0] - 0.5, first.position[1], first.position[2] - 0.5]
        area.full_uvec[:] = [1.0, 0.0, 0.0]
        area.full_vvec[:] = [0.0, 0.0, 1.0]
        area.intensity[:] = list(first.intensity)
        area.usteps = area.vsteps = 2
        area.jitter = area.seed = 0
        tables.area_lights = (rtc_amd.AreaLightDesc * 1)(area)
        tables.lights = (rtc_amd.LightDesc * (len(tables.lights) - 1))(*list(tables.lights)[1:])
    return tables, cam, depth


def velocities(tables):
    """{world index: velocity (3,)} of the motion list."""
    return {m.index: np.array(m.velocity[:]) for m in tables.motion}


@functools.lru_cache(maxsize=None)
def batch(seed):
    """(rays (2048, 6), times (2048,)), read-only."""
    _, cam, _ = world(seed)
    half = N_RAYS // 2
    side = 32
    assert side * side == half
    eye = MR.sample_rays(rtc_amd.camera_resize(cam, side, side), side, side, 1).reshape(-1, 6)
    rng = np.random.default_rng(8000 + seed)
    o = rng.uniform([-4, -1.5, -6], [4, 4, 4], size=(half, 3))
    d = rng.normal(size=(half, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.ascontiguousarray(np.concatenate([eye, np.concatenate([o, d], axis=1)], axis=0))
    times = np.array(TIMES)[np.arange(N_RAYS) % len(TIMES)]
    rays.setflags(write=False)
    times.setflags(write=False)
    return rays, times


def lens(seed):
    """None for seeds 0 to 11 (the pinhole), else (aperture, focal distance = |eye|, hashed, seed 3)."""
    if seed < 12:
        return None
    eye = np.array(world(seed)[1].origin[:])
    return (0.05, float(np.sqrt((eye * eye).sum())), True, 3)


def shutter(seed):
    """(open, close, jitter, seed): the cell centres for seeds 0 to 11, hashed with seed 5 from 12 on."""
    return (0.0, 1.0, False, 0) if seed < 12 else (0.0, 1.0, True, 5)


_BATCH, _FRAME, _STATIC = {}, {}, {}


def batch_reference(oracle, seed):
    """(colours, counters) of the oracle over the seed's batch, each ray in the world at its time; computed once."""
    if seed not in _BATCH:
        tables, _, depth = world(seed)
        cols, st = MR.trace(oracle, tables, *batch(seed), depth)
        cols.setflags(write=False)
        _BATCH[seed] = (cols, st)
    return _BATCH[seed]


def static_reference(oracle, seed):
    """The oracle's colours of the batch's rays in the world at tau = 0; computed once."""
    if seed not in _STATIC:
        tables, _, depth = world(seed)
        _STATIC[seed] = oracle.color_at(tables.at_time(0.0).expanded(), batch(seed)[0], depth)[0]
    return _STATIC[seed]


def frame_reference(oracle, seed):
    """(frame, counters) of the oracle's mean over the seed's 70 x 22, n = 2 shutter frame; computed once."""
    if seed not in _FRAME:
        tables, cam, depth = world(seed)
        img, st = MR.frame(oracle, tables, cam, rtc_amd, *FRAME, GRID, shutter(seed), depth, lens(seed))
        img.setflags(write=False)
        _FRAME[seed] = (img, st)
    return _FRAME[seed]


def inside(tables, index, points):
    """Which of `points` (n, 3) lie strictly inside bounded shape `index` (a sphere, a cube, a bounded cylinder
    or a bounded cone) of static tables."""
    s = tables.shapes[index]
    inv = np.array(s.inverse[:]).reshape(4, 4)
    p = points @ inv[:3, :3].T + inv[:3, 3]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    kind = KINDS[s.kind]
    if kind == "sphere":
        return x * x + y * y + z * z < 1.0
    if kind == "cube":
        return np.abs(p).max(axis=1) < 1.0
    if kind in ("cylinder", "cone") and np.isfinite(s.minimum) and abs(s.minimum) < 1e300 and abs(s.maximum) < 1e300:
        side = x * x + z * z < (1.0 if kind == "cylinder" else y * y)
        return side & (y > s.minimum) & (y < s.maximum)
    return np.zeros(len(points), dtype=bool)
