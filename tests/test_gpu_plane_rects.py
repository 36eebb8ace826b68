"""The per-scene f32 direct kernel's primary cull of planes changes nothing.

A launch hands the kernel, per plane slot, the pixel blocks in which the
plane's entry lies behind the eye or another plane's entry in front is nearer
(primary_rect.hpp plane_rect, rtc_kernels.hip closest_hit under
RTC_PLANE_RECTS; tests/test_plane_rects.py checks the rectangles against the
kernel's arithmetic on the CPU).  A plane passed by could not have been the
nearest, so the frame must equal, bit for bit and counter for counter,

* the frame of the same kernel built with -DRTC_PLANE_RECTS=0 (a context
  created under RTC_DEBUG=jit_flags=...),
* the RT_FLAG_NO_SKIPS frame, and
* the generic kernel's frame (RT_JIT_OFF):

on the two direct reference scenes at 333x201 and 640x360, on one shard of
eight, for one context that renders camera A, camera B and camera A again (a
rectangle is its launch's: nothing of B may be left in the second A), and on
small worlds whose blocks straddle every boundary the rectangles draw: two
walls meeting in a corner over a floor, two parallel floors seen from above
and from between them, two coincident planes of different colours, an eye
lying on a plane and a hair off it, a plane behind the camera, a rolled camera
(a slanted horizon and slanted edges), a sphere across a floor-wall edge, and
nine slots (past the cap: the tables stay zero).

A world's three builds (default, RT_FLAG_NO_SKIPS, switched off) are compiled
side by side, as tests/test_gpu_launch_terms.py does.
"""
import numpy as np
import pytest

from conftest import scene_fixture
from test_gpu_parity import _counts
from test_gpu_uniform_hit import _salted

pytestmark = pytest.mark.gpu

OFFS = {"RTC_PLANE_RECTS=0": "jit_flags=-DRTC_PLANE_RECTS=0"}


def _frames(gpu_ctx, rtc, monkeypatch, scene, cams, salt, depth=6, shard=(0, 1)):
    """{build: [(frame, stats) per camera]} for the default build, the off-build, RT_FLAG_NO_SKIPS and the generic kernel."""
    kick = rtc.camera_resize(cams[0], 512, 128)  # 256 tiles: a frame that asks for a build
    out, offs = {}, []

    def render(ctx, cam, per_scene=True, **kw):
        f = ctx.render(cam, depth, precision="f32", shard=shard, **kw)
        assert bool(ctx.jit_status()["used"]) == per_scene, ctx.jit_status()
        return f

    try:
        gpu_ctx.upload(scene)
        gpu_ctx.set_jit(rtc.RT_JIT_EAGER)
        gpu_ctx.render(kick, depth, precision="f32")
        gpu_ctx.render(kick, depth, precision="f32", flags=rtc.RT_FLAG_NO_SKIPS)
        for i, knob in enumerate(OFFS.values()):
            monkeypatch.setenv("RTC_DEBUG", knob)
            off = rtc.Context(0)
            offs.append(off)
            off.set_jit(rtc.RT_JIT_EAGER)
            off.upload(_salted(rtc, scene, salt + 1e-3 * i))
            off.render(kick, depth, precision="f32")
        monkeypatch.delenv("RTC_DEBUG")
        for ctx in [gpu_ctx] + offs:
            assert ctx.jit_wait() == 0
        gpu_ctx.set_jit(rtc.RT_JIT_SYNC)
        out["default"] = [render(gpu_ctx, c) for c in cams]
        out["RT_FLAG_NO_SKIPS"] = [render(gpu_ctx, c, flags=rtc.RT_FLAG_NO_SKIPS) for c in cams]
        gpu_ctx.set_jit(rtc.RT_JIT_OFF)
        out["the generic kernel"] = [render(gpu_ctx, c, per_scene=False) for c in cams]
        for (name, knob), off in zip(OFFS.items(), offs):
            monkeypatch.setenv("RTC_DEBUG", knob)  # (a build made in line would be this context's kind too)
            off.set_jit(rtc.RT_JIT_SYNC)
            out[name] = [render(off, c) for c in cams]
        monkeypatch.delenv("RTC_DEBUG")
    finally:
        gpu_ctx.set_jit(rtc.RT_JIT_AUTO)
        for off in offs:
            off.close()
    return out


def _assert_same(frames, what):
    for i, (a, sa) in enumerate(frames["default"]):
        assert a.any()
        for name, others in frames.items():
            f, s = others[i]
            assert np.array_equal(a, f), f"{what}, camera {i}: {int((a != f).any(axis=2).sum())} px differ from {name}"
            assert _counts(sa) == _counts(s), (what, i, name)


def _plane_rects(rtc, tables, cam):
    """The launch's rectangles of the world's planes for `cam` (rt_camera_plane_rect), and the canvas's."""
    rows = np.array([list(s.inverse[4:8]) for s in tables.shapes if int(s.kind) == 1], np.float64).astype(np.float32)
    return [rtc.camera_plane_rect(cam, rows, q) for q in range(len(rows))], (0, 0, cam.width - 1, cam.height - 1)


@pytest.mark.parametrize("name", ["three_sphere_scene", "shadow_puppets"])
def test_reference_scenes(gpu_ctx, rtc, monkeypatch, name):
    scene = scene_fixture(name)
    cams = [rtc.camera_resize(scene.camera, *size) for size in [(333, 201), (640, 360)]]
    if name == "three_sphere_scene":  # the cull is at work here: every plane is passed by somewhere
        for cam in cams:
            rects, full = _plane_rects(rtc, scene, cam)
            assert len(rects) == 3 and all(r != full for r in rects)
    _assert_same(_frames(gpu_ctx, rtc, monkeypatch, scene, cams, 0.5772156 + len(name) * 1e-6), name)


def test_one_shard_of_eight(gpu_ctx, rtc, monkeypatch):
    scene = scene_fixture("three_sphere_scene")
    cam = rtc.camera_resize(scene.camera, 640, 360)
    shard, shards = 5, 8
    strips = _frames(gpu_ctx, rtc, monkeypatch, scene, [cam], 0.5772157, shard=(shard, shards))
    _assert_same(strips, "shard 5 of 8")
    gpu_ctx.set_jit(rtc.RT_JIT_SYNC)
    try:
        whole, _ = gpu_ctx.render(cam, 6, precision="f32")
        assert gpu_ctx.jit_status()["used"]
    finally:
        gpu_ctx.set_jit(rtc.RT_JIT_AUTO)
    owner, strip_row = rtc.shard_row_map(360, shards)
    mine = np.flatnonzero(owner == shard)
    assert len(mine) > 0
    got = strips["default"][0][0]
    assert np.array_equal(got[strip_row[mine]], whole[mine]), "the shard's strip differs from its rows of the frame"


def test_no_rectangle_outlives_its_launch(gpu_ctx, rtc):
    """Camera A, camera B, camera A again on one context: the A frames are one frame, and B is a fresh context's B."""
    from rtc_amd import world as W
    scene = scene_fixture("three_sphere_scene")
    cam_a = rtc.camera_resize(scene.camera, 333, 201)
    cam_b = W.camera(333, 201, 0.9, (3.5, 4.0, -2.0), (0, 0.5, 0), (0.1, 1, 0))  # another origin, side and height
    assert _plane_rects(rtc, scene, cam_a)[0] != _plane_rects(rtc, scene, cam_b)[0]
    gpu_ctx.upload(scene)
    gpu_ctx.set_jit(rtc.RT_JIT_SYNC)
    try:
        a1, s1 = gpu_ctx.render(cam_a, 6, precision="f32")
        b, sb = gpu_ctx.render(cam_b, 6, precision="f32")
        a2, s2 = gpu_ctx.render(cam_a, 6, precision="f32")
        assert gpu_ctx.jit_status()["used"]
        with rtc.Context(0) as fresh:
            fresh.set_jit(rtc.RT_JIT_SYNC)
            fresh.upload(scene)
            fb, sfb = fresh.render(cam_b, 6, precision="f32")
            assert fresh.jit_status()["used"]
        gpu_ctx.set_jit(rtc.RT_JIT_OFF)
        gb, sgb = gpu_ctx.render(cam_b, 6, precision="f32")
    finally:
        gpu_ctx.set_jit(rtc.RT_JIT_AUTO)
    assert np.array_equal(a1, a2) and _counts(s1) == _counts(s2)
    assert np.array_equal(b, fb) and _counts(sb) == _counts(sfb)
    assert np.array_equal(b, gb) and _counts(sb) == _counts(sgb)
    assert not np.array_equal(a1[:, :, 0], b[:, :, 0])


# ------------------------------------------------------------ the rectangles' edges
def _matte(W, color):
    return W.Material(color=color, specular=0.0)


def _ball(W, x, y, z, r, color=(0.1, 1.0, 0.5)):
    return W.sphere(W.Material(color=color, diffuse=0.7, specular=0.3), W.mat_mul(W.translation(x, y, z), W.scaling(r, r, r)))


def _wall(W, turn, z=5.0, color=(0.8, 0.8, 1.0)):
    """An upright wall through (0, 0, z), turned by `turn` about y (0: facing the -z side)."""
    return W.plane(_matte(W, color), W.mat_mul(W.translation(0, 0, z), W.mat_mul(W.rotation_y(turn), W.rotation_x(np.pi / 2))))


def _floor(W, y=0.0, color=(1.0, 0.9, 0.9)):
    return W.plane(_matte(W, color), W.translation(0, y, 0))


def _corner():
    """Two walls meeting in a corner on the screen, over a floor: every pair of planes shares an edge in view."""
    from rtc_amd import world as W
    shapes = [_floor(W), _wall(W, -np.pi / 4), _wall(W, np.pi / 4, color=(0.8, 1.0, 0.8)), _ball(W, -0.5, 1, 0.5, 1.0)]
    return W.World([W.Light((-10, 10, -10))], shapes), [((0, 1.5, -5), (0, 1, 0), (0, 1, 0)), ((2.5, 0.7, -3), (-1, 1.2, 2), (0, 1, 0))]


def _parallel_floors():
    """Two parallel floors, seen from above both (the lower one is never seen) and from between them."""
    from rtc_amd import world as W
    shapes = [_floor(W), _floor(W, -1.0, (0.6, 0.7, 1.0)), _wall(W, 0.0, 8.0), _ball(W, 0.4, 0.5, 0, 0.5)]
    return W.World([W.Light((-6, 8, -8))], shapes), [((0, 1.5, -5), (0, 0.5, 0), (0, 1, 0)), ((0, -0.4, -5), (0, -0.5, 0), (0, 1, 0))]


def _coincident():
    """Two coincident floors of different colours (the world index decides) and the same plane from the other side."""
    from rtc_amd import world as W
    shapes = [_floor(W, 0.0, (1.0, 0.2, 0.2)), _floor(W, 0.0, (0.2, 0.2, 1.0)),
              W.plane(_matte(W, (0.2, 1.0, 0.2)), W.scaling(1, -1, 1)), _wall(W, 0.3, 6.0), _ball(W, 0.5, 0.8, 0, 0.7)]
    return W.World([W.Light((-6, 8, -8))], shapes), [((0, 1.5, -5), (0, 0.5, 0), (0, 1, 0))]


def _eye_on_a_plane():
    """The eye exactly in the floor's plane, and 1e-7 above and below it; a wall ahead and one to the side."""
    from rtc_amd import world as W
    shapes = [_floor(W), _wall(W, 0.0, 6.0), _wall(W, np.pi / 2 - 0.2, 4.0, (0.8, 1.0, 0.8)), _ball(W, 0.7, 0.6, 0, 0.6)]
    level = lambda y: ((0, y, -5), (0, y, 0), (0, 1, 0))  # noqa: E731
    return W.World([W.Light((-6, 8, -8))], shapes), [level(0.0), level(1e-7), level(-1e-7)]


def _plane_behind():
    """A wall behind the camera (its rectangle is empty) and one ahead, over a floor."""
    from rtc_amd import world as W
    shapes = [_floor(W), _wall(W, 0.1, -9.0), _wall(W, -0.2, 7.0, (0.8, 1.0, 0.8)), _ball(W, -0.6, 0.7, 0.5, 0.7)]
    return W.World([W.Light((-10, 10, -8))], shapes), [((0, 1.5, -5), (0, 1, 0), (0, 1, 0))]


def _rolled_camera():
    """The corner seen with a rolled camera: the horizon and every edge cross the blocks at a slant."""
    world, _ = _corner()
    return world, [((0, 1.5, -5), (0, 1, 0), (0.6, 1, 0.1)), ((1, 2.5, -4), (0, 0.5, 1), (-1, 0.3, 0))]


def _sphere_on_an_edge():
    """A sphere across the floor-wall edge, and one across the walls' corner."""
    from rtc_amd import world as W
    shapes = [_floor(W), _wall(W, -np.pi / 4), _wall(W, np.pi / 4, color=(0.8, 1.0, 0.8)),
              _ball(W, -2.0, 0.1, 2.8, 0.6), _ball(W, 0.0, 1.6, 4.8, 0.7, (1.0, 0.4, 0.2))]
    return W.World([W.Light((-10, 10, -10))], shapes), [((0, 1.5, -5), (0, 1, 0), (0, 1, 0))]


def _nine_slots():
    """A floor, two walls and six balls: past the cap, the launch's tables stay zero."""
    from rtc_amd import world as W
    shapes = [_floor(W), _wall(W, -np.pi / 4), _wall(W, np.pi / 4)] + [
        _ball(W, 1.1 * (i - 2.5), 0.5, 0.4 * i, 0.5, (0.2 + 0.1 * i, 1.0 - 0.1 * i, 0.5)) for i in range(6)]
    return W.World([W.Light((-10, 10, -10))], shapes), [((0, 2.5, -8), (0, 0.5, 0), (0, 1, 0))]


EDGES = {"corner": (_corner, (320, 200)), "parallel_floors": (_parallel_floors, (203, 117)), "coincident": (_coincident, (160, 96)),
         "eye_on_a_plane": (_eye_on_a_plane, (203, 117)), "plane_behind": (_plane_behind, (160, 96)),
         "rolled_camera": (_rolled_camera, (320, 200)), "sphere_on_an_edge": (_sphere_on_an_edge, (203, 117)),
         "nine_slots": (_nine_slots, (160, 96))}
# the worlds whose first camera must see the cull at work, and how many of its planes' rectangles must be smaller than the canvas
CULLED = {"corner": 3, "parallel_floors": 2, "plane_behind": 2, "rolled_camera": 2, "sphere_on_an_edge": 3}


@pytest.mark.parametrize("which", list(EDGES))
def test_rectangle_edges(gpu_ctx, rtc, monkeypatch, which):
    from rtc_amd import world as W
    make, size = EDGES[which]
    world, views = make()
    cams = [W.camera(size[0], size[1], 1.0, *v) for v in views]
    tables = world.tables(cams[0])
    if which == "nine_slots":
        assert len(tables.shapes) == 9  # (past rtc_internal.hpp kPrimaryRectSlots)
    if which in CULLED:
        rects, full = _plane_rects(rtc, tables, cams[0])
        assert sum(r != full for r in rects) >= CULLED[which], rects
    if which == "plane_behind":
        rects, _ = _plane_rects(rtc, tables, cams[0])
        assert any(r[0] > r[2] for r in rects), rects  # the wall behind the camera: an empty rectangle
    frames = _frames(gpu_ctx, rtc, monkeypatch, tables, cams, 0.2020569 + len(which) * 1e-6)
    _assert_same(frames, which)
