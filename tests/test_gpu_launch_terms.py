"""The per-scene f32 direct kernel's launch terms and unit plane normals change nothing.

Every primary ray of a frame starts at the camera's origin, so what a test
forms from the origin alone (a plane's object-space height, the origin's part
of the offset scale) comes with the launch, worked out on the host in the
kernel's own f32 operations (launch_terms.hpp, rtc_kernels.hip closest_hit;
tests/test_launch_terms_cpu.py checks the host's bits on the CPU), the origin
stays a wave-uniform value in the other kinds' tests, and a plane's unit
normal is a constant of the build, evaluated once on the device (rtc_jit.cpp
unit_normals).  The same values by another road, so the frame must equal, bit
for bit and counter for counter,

* the frame of the same kernel built with -DRTC_LAUNCH_TERMS=0
  -DRTC_UNIT_NORMALS=0, and with each switch alone (contexts created under
  RTC_DEBUG=jit_flags=...),
* the RT_FLAG_NO_SKIPS frame, and
* the generic kernel's frame (RT_JIT_OFF),

and lie within the f32 tolerance of the oracle: on the two direct reference
scenes at 320x200 and 333x201 (ragged right and bottom tiles), on one shard of
eight, for one context that renders camera A, camera B and camera A again (the
terms are the launch's: nothing of B may be left in the second A), and on
small worlds aimed at the edges: the eye exactly on a plane and a hair either
side of it, a plane whose object-space height is -0, a sheared and unevenly
scaled plane (a normal far from unit length), a camera matrix that is no
rotation, an unevenly scaled sphere (the object-space test) beside a world
sphere, the eye inside a sphere's bound, nine slots (past the cap: no terms)
and a canvas 2064 pixels wide (beyond the cull tables, which the terms do not
depend on).

A world's five builds (default, RT_FLAG_NO_SKIPS, three switched off) are
compiled side by side: each context starts its build in the background on a
frame large enough to ask for one (RT_JIT_EAGER), then all are waited for.  An
off-context uploads the world with one more material that no shape uses
(test_gpu_uniform_hit._salted): a table, and so a build, of its own.
"""
import numpy as np
import pytest

from conftest import scene_fixture
from test_gpu_parity import F32_PIX_FRAC, _counts, _pix_agree
from test_gpu_uniform_hit import _salted

pytestmark = pytest.mark.gpu

OFFS = {
    "RTC_LAUNCH_TERMS=0 RTC_UNIT_NORMALS=0": "jit_flags=-DRTC_LAUNCH_TERMS=0 -DRTC_UNIT_NORMALS=0",
    "RTC_LAUNCH_TERMS=0": "jit_flags=-DRTC_LAUNCH_TERMS=0",
    "RTC_UNIT_NORMALS=0": "jit_flags=-DRTC_UNIT_NORMALS=0",
}
SIZES = [(320, 200), (333, 201)]


def _frames(gpu_ctx, rtc, monkeypatch, scene, cams, salt, depth=6, shard=(0, 1)):
    """{build: [(frame, stats) per camera]} for the default build, each off-build, RT_FLAG_NO_SKIPS and the generic kernel."""
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
        for name, others in frames.items():
            f, s = others[i]
            assert np.array_equal(a, f), f"{what}, camera {i}: {int((a != f).any(axis=2).sum())} px differ from {name}"
            assert _counts(sa) == _counts(s), (what, i, name)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["three_sphere_scene", "shadow_puppets"])
def test_launch_terms_are_exact(gpu_ctx, rtc, oracle, monkeypatch, name, size):
    scene = scene_fixture(name)
    cam = rtc.camera_resize(scene.camera, *size)
    frames = _frames(gpu_ctx, rtc, monkeypatch, scene, [cam], 0.4142135 + size[0] * 1e-6)
    _assert_same(frames, f"{name} {size}")
    a = frames["default"][0][0]
    assert a.any()
    ref, _ = oracle.render(scene, cam, 6, threads=8)
    assert _pix_agree(a, ref, oracle) >= F32_PIX_FRAC


def test_one_shard_of_eight(gpu_ctx, rtc, monkeypatch):
    scene = scene_fixture("three_sphere_scene")
    cam = rtc.camera_resize(scene.camera, 640, 400)
    shard, shards = 5, 8
    strips = _frames(gpu_ctx, rtc, monkeypatch, scene, [cam], 0.4142136, shard=(shard, shards))
    _assert_same(strips, "shard 5 of 8")
    gpu_ctx.set_jit(rtc.RT_JIT_SYNC)
    try:
        whole, _ = gpu_ctx.render(cam, 6, precision="f32")
        assert gpu_ctx.jit_status()["used"]
    finally:
        gpu_ctx.set_jit(rtc.RT_JIT_AUTO)
    owner, strip_row = rtc.shard_row_map(400, shards)
    mine = np.flatnonzero(owner == shard)
    assert len(mine) > 0
    got = strips["default"][0][0]
    assert np.array_equal(got[strip_row[mine]], whole[mine]), "the shard's strip differs from its rows of the frame"


def test_no_term_outlives_its_launch(gpu_ctx, rtc):
    """Camera A, camera B, camera A again on one context: the A frames are one frame, and B is a fresh context's B."""
    from rtc_amd import world as W
    scene = scene_fixture("three_sphere_scene")
    cam_a = rtc.camera_resize(scene.camera, 333, 201)
    cam_b = W.camera(333, 201, 0.9, (3.5, 4.0, -2.0), (0, 0.5, 0), (0.1, 1, 0))  # another origin, side and height
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


# ------------------------------------------------------------ the terms' edges
def _matte(W, color):
    return W.Material(color=color, specular=0.0)


def _ball(W, x, y, z, r, color=(0.1, 1.0, 0.5)):
    return W.sphere(W.Material(color=color, diffuse=0.7, specular=0.3), W.mat_mul(W.translation(x, y, z), W.scaling(r, r, r)))


def _back_wall(W, z=6.0):
    return W.plane(_matte(W, (0.8, 0.8, 1.0)), W.mat_mul(W.translation(0, 0, z), W.rotation_x(np.pi / 2)))


def _level(y):
    """A camera whose f32 origin is exactly (0, y, -5): a level view along +z."""
    return (0, y, -5), (0, y, 0), (0, 1, 0)


def _eye_on_a_plane():
    """The eye exactly in the floor's plane (lo.y == 0: the floor is seen edge-on), and 1e-7 above and below it."""
    from rtc_amd import world as W
    shapes = [W.plane(_matte(W, (1.0, 0.9, 0.9))), _back_wall(W), _ball(W, 0.7, 0.6, 0, 0.6), _ball(W, -0.9, -0.5, 1, 0.5, (1.0, 0.4, 0.2))]
    return W.World([W.Light((-6, 8, -8))], shapes), [_level(0.0), _level(1e-7), _level(-1e-7)]


def _minus_zero_height():
    """A floor mirrored in y (inverse: -1 on the diagonal, a translation of -0): the eye's object-space height is -0."""
    from rtc_amd import world as W
    shapes = [W.plane(_matte(W, (1.0, 0.9, 0.9)), W.scaling(1, -1, 1)), _back_wall(W), _ball(W, 0.5, 0.8, 0, 0.7)]
    return W.World([W.Light((-6, 8, -8))], shapes), [_level(0.0)]


def _sheared_plane():
    """A floor under uneven scaling and shear: its world normal is far from unit length (and a second, tilted one)."""
    from rtc_amd import world as W
    floor = W.plane(_matte(W, (1.0, 0.9, 0.9)), W.mat_mul(W.shearing(0.3, 0, 0.7, 0.2, 0, 0.4), W.scaling(7.0, 0.05, 0.3)))
    tilted = W.plane(_matte(W, (0.7, 1.0, 0.8)),
                     W.mat_mul(W.translation(0, 0, 8), W.mat_mul(W.rotation_x(1.1), W.scaling(0.01, 40.0, 3.0))))
    return W.World([W.Light((-10, 10, -10))], [floor, tilted, _ball(W, 0, 1, 0, 1.0)]), [((0.5, 2.5, -6), (0, 0.8, 0), (0, 1, 0))]


def _no_rotation():
    """`up` not at right angles to the view: the camera matrix is no rotation."""
    from rtc_amd import world as W
    shapes = [W.plane(_matte(W, (1.0, 0.9, 0.9))), _back_wall(W), _ball(W, -0.8, 1, 0, 1.0, (0.8, 1.0, 0.6)), _ball(W, 1.0, 0.5, -0.5, 0.5)]
    return W.World([W.Light((-10, 10, -10))], shapes), [((0, 1.5, -5), (0, 1, 0), (0.6, 1, 0.2))]


def _object_space_sphere():
    """An unevenly scaled sphere (no kShapeSimilar: the object-space test) beside a world sphere."""
    from rtc_amd import world as W
    egg = W.sphere(W.Material(color=(1.0, 0.5, 0.1), diffuse=0.7, specular=0.3),
                   W.mat_mul(W.translation(-1.2, 0.9, 0.3), W.mat_mul(W.rotation_z(0.4), W.scaling(0.5, 0.9, 0.7))))
    return W.World([W.Light((-10, 10, -10))], [W.plane(_matte(W, (1.0, 0.9, 0.9))), egg, _ball(W, 1.0, 0.8, 0, 0.8)]), \
        [((0, 1.5, -5), (0, 0.8, 0), (0, 1, 0))]


def _eye_in_a_bound():
    """The eye inside a large sphere (every ray a front ray of its ball), a small one in view."""
    from rtc_amd import world as W
    shell = W.sphere(W.Material(color=(0.6, 0.7, 1.0), diffuse=0.6, specular=0.1), W.scaling(9, 9, 9))
    return W.World([W.Light((-2, 5, -3))], [W.plane(_matte(W, (1.0, 0.9, 0.9))), shell, _ball(W, 0.5, 0.7, 0, 0.7)]), \
        [((0, 1.5, -5), (0, 1, 0), (0, 1, 0))]


def _nine_slots():
    """A floor and eight balls: past the cap, the launch brings no terms and the kernel asks for none."""
    from rtc_amd import world as W
    shapes = [W.plane(_matte(W, (1.0, 0.9, 0.9)))] + [
        _ball(W, 1.1 * (i - 3.5), 0.5, 0.4 * i, 0.5, (0.2 + 0.1 * i, 1.0 - 0.1 * i, 0.5)) for i in range(8)]
    return W.World([W.Light((-10, 10, -10))], shapes), [((0, 2.5, -8), (0, 0.5, 0), (0, 1, 0))]


EDGES = {"eye_on_a_plane": _eye_on_a_plane, "minus_zero_height": _minus_zero_height, "sheared_plane": _sheared_plane,
         "no_rotation": _no_rotation, "object_space_sphere": _object_space_sphere, "eye_in_a_bound": _eye_in_a_bound,
         "nine_slots": _nine_slots, "wide_canvas": _no_rotation}


@pytest.mark.parametrize("which", list(EDGES))
def test_term_edges(gpu_ctx, rtc, oracle, monkeypatch, which):
    from rtc_amd import world as W
    world, views = EDGES[which]()
    size = (2064, 40) if which == "wide_canvas" else (333, 201)  # (2064: past the 2048 pixels of the cull tables)
    cams = [W.camera(size[0], size[1], 1.0, *v) for v in views]
    tables = world.tables(cams[0])
    if which == "nine_slots":
        assert len(tables.shapes) == 9  # (past rtc_internal.hpp kPrimaryRectSlots)
    if which == "eye_on_a_plane":
        assert [np.float32(c.origin[1]) for c in cams] == [np.float32(0.0), np.float32(1e-7), np.float32(-1e-7)]
    if which == "minus_zero_height":
        # launch_terms: lo.y = fma(inv[5], o.y, inv[7]), the zero entries' terms dropped (kind 1: rtc.h RT_SHAPE_PLANE)
        inv = [np.float32(x) for x in [s for s in tables.shapes if s.kind == 1][0].inverse[:12]]
        assert inv[4] == 0 and inv[6] == 0 and inv[5] == -1 and inv[7] == 0 and np.signbit(inv[7])
        assert cams[0].origin[1] == 0.0 and not np.signbit(cams[0].origin[1])
    frames = _frames(gpu_ctx, rtc, monkeypatch, tables, cams, 0.7320508 + len(which) * 1e-6)
    _assert_same(frames, which)
    for cam, (a, _) in zip(cams, frames["default"]):
        assert a.any()
        ref, _ = oracle.render(tables, cam, 6, threads=8)
        assert _pix_agree(a, ref, oracle) >= F32_PIX_FRAC
