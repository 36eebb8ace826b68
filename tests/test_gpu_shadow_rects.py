"""The per-scene f32 direct kernel's shadow cull by screen rectangles changes nothing.

A wave of the frame kernel whose hits all lie on one plane passes a caster by,
in any_hit, when the launch's bits say that the wave's pixel block lies outside
the screen rectangle in which the caster's ball can shadow that plane from the
light (rtc_kernels.hip ShadowBits, primary_rect.hpp shadow_rect / shadow_near;
tests/test_shadow_rects.py checks the rectangles on the CPU).  Acceleration
only, so the frame must equal, bit for bit and counter for counter,

* the frame of the same kernel built with -DRTC_SHADOW_RECTS=0 (a context
  created under RTC_DEBUG=jit_flags=...),
* the RT_FLAG_NO_SKIPS frame (a per-scene build that takes no bits), and
* the generic kernel's frame (RT_JIT_OFF),

on the two direct reference scenes at 320x200 and 333x201 (ragged right and
bottom tiles), on one shard of eight, and on small worlds aimed at the cull's
edges, each also within the f32 tolerance of the oracle: a shadow across block
columns and rows, a shadow that runs to the horizon, a light below the floor,
a light inside a sphere's bound, two lights, a sphere resting on the plane, a
camera matrix that is no rotation, seven slots (past the cap: no bits) and a
canvas 2064 pixels wide (beyond the tables: no bits).

The RTC_SHADOW_RECTS=0 context uploads the world with one more material that
no shape uses (test_gpu_uniform_hit._salted): a table, and so a build, of its
own.
"""
import numpy as np
import pytest

from conftest import scene_fixture
from test_gpu_parity import F32_PIX_FRAC, _counts, _pix_agree
from test_gpu_uniform_hit import _salted

pytestmark = pytest.mark.gpu

OFF = "jit_flags=-DRTC_SHADOW_RECTS=0"
SIZES = [(320, 200), (333, 201)]
NAMES = ("RTC_SHADOW_RECTS=0", "RT_FLAG_NO_SKIPS", "the generic kernel")


def _frames(gpu_ctx, rtc, monkeypatch, scene, cam, salt, depth=6):
    """The default, RTC_SHADOW_RECTS=0, RT_FLAG_NO_SKIPS and generic frames with their stats."""
    gpu_ctx.upload(scene)
    gpu_ctx.set_jit(rtc.RT_JIT_SYNC)
    try:
        a, sa = gpu_ctx.render(cam, depth, precision="f32")
        assert gpu_ctx.jit_status()["used"], gpu_ctx.jit_status()
        n, sn = gpu_ctx.render(cam, depth, precision="f32", flags=rtc.RT_FLAG_NO_SKIPS)
        assert gpu_ctx.jit_status()["used"], gpu_ctx.jit_status()
        gpu_ctx.set_jit(rtc.RT_JIT_OFF)
        g, sg = gpu_ctx.render(cam, depth, precision="f32")
        assert not gpu_ctx.jit_status()["used"]
    finally:
        gpu_ctx.set_jit(rtc.RT_JIT_AUTO)
    monkeypatch.setenv("RTC_DEBUG", OFF)
    with rtc.Context(0) as off:
        off.set_jit(rtc.RT_JIT_SYNC)
        off.upload(_salted(rtc, scene, salt))
        b, sb = off.render(cam, depth, precision="f32")
        assert off.jit_status()["used"], off.jit_status()
    monkeypatch.delenv("RTC_DEBUG")
    return (a, sa), (b, sb), (n, sn), (g, sg)


def _assert_same(frames, what):
    (a, sa), rest = frames[0], frames[1:]
    for name, (f, s) in zip(NAMES, rest):
        assert np.array_equal(a, f), f"{what}: {int((a != f).any(axis=2).sum())} px differ from {name}"
        assert _counts(sa) == _counts(s), (what, name)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["three_sphere_scene", "shadow_puppets"])
def test_shadow_rects_are_exact(gpu_ctx, rtc, monkeypatch, name, size):
    scene = scene_fixture(name)
    cam = rtc.camera_resize(scene.camera, *size)
    frames = _frames(gpu_ctx, rtc, monkeypatch, scene, cam, 0.5772156 + size[0] * 1e-6)
    _assert_same(frames, f"{name} {size}")
    assert frames[0][0].any()


# ------------------------------------------------------------ the cull's edges
def _floor(W, **kw):
    return W.plane(W.Material(color=(1.0, 0.9, 0.9), specular=0.0, **kw))


def _ball(W, x, y, z, r, color=(0.1, 1.0, 0.5)):
    return W.sphere(W.Material(color=color, diffuse=0.7, specular=0.3), W.mat_mul(W.translation(x, y, z), W.scaling(r, r, r)))


def _across_blocks():
    """Seen from above, the shadow ellipse lies mid-frame, across several block columns and rows."""
    from rtc_amd import world as W
    return W.World([W.Light((-6, 10, -4))], [_floor(W), _ball(W, 0, 1.5, 0, 0.8)]), ((0, 9, -6), (0.5, 0, 0), (0, 1, 0))


def _to_the_horizon():
    """A low light behind a ball: the shadow runs off to the floor's horizon, which crosses the frame."""
    from rtc_amd import world as W
    return W.World([W.Light((0, 1.05, -6))], [_floor(W), _ball(W, 0.3, 1.0, -2, 0.5)]), ((3, 1.5, -8), (0, 1, 0), (0, 1, 0))


def _light_below_the_floor():
    """The eye above the floor, the light below it: the floor is lit by ambient light alone."""
    from rtc_amd import world as W
    shapes = [_floor(W), _ball(W, 0, 1, 0, 1.0), _ball(W, 1, -2, 0.5, 0.7, (1.0, 0.5, 0.1))]
    return W.World([W.Light((2, -6, 1))], shapes), ((0, 1.5, -5), (0, 1, 0), (0, 1, 0))


def _light_in_a_bound():
    """The light inside a sphere: every shadow ray starts toward a caster that holds its end."""
    from rtc_amd import world as W
    shapes = [_floor(W), _ball(W, -4, 5, -3, 1.5), _ball(W, 0.5, 0.5, 0, 0.5, (1.0, 0.3, 0.2))]
    return W.World([W.Light((-4, 5.5, -3))], shapes), ((0, 1.5, -5), (0, 1, 0), (0, 1, 0))


def _two_lights():
    from rtc_amd import world as W
    shapes = [_floor(W), _ball(W, -0.8, 1, 0, 1.0, (0.8, 1.0, 0.6)), _ball(W, 1.0, 0.5, -0.5, 0.5, (1.0, 0.5, 0.1))]
    return W.World([W.Light((-10, 10, -10)), W.Light((5, 8, -6), (0.3, 0.3, 0.4))], shapes), ((0, 1.5, -5), (0, 1, 0), (0, 1, 0))


def _resting_sphere():
    """The ball touches the floor: its shadow starts at the point of contact, inside the ball's own blocks."""
    from rtc_amd import world as W
    wall = W.plane(W.Material(color=(0.8, 0.8, 1.0), specular=0.0), W.mat_mul(W.translation(0, 0, 4), W.rotation_x(np.pi / 2)))
    return W.World([W.Light((-10, 10, -10))], [_floor(W), wall, _ball(W, 0, 1, 0, 1.0)]), ((0, 1.5, -5), (0, 1, 0), (0, 1, 0))


def _no_rotation():
    """`up` not at right angles to the view: the camera matrix is no rotation."""
    world, (frm, to, _) = _two_lights()
    return world, (frm, to, (0.6, 1, 0.2))


def _seven_slots():
    """A floor and six balls: past the cap, the launch sets no bits and the kernel asks for none."""
    from rtc_amd import world as W
    shapes = [_floor(W)] + [_ball(W, 1.3 * (i - 2.5), 0.5, 0.4 * i, 0.5, (0.2 + 0.12 * i, 1.0 - 0.1 * i, 0.5)) for i in range(6)]
    return W.World([W.Light((-10, 10, -10))], shapes), ((0, 2.5, -7), (0, 0.5, 0), (0, 1, 0))


EDGES = {"across_blocks": _across_blocks, "to_the_horizon": _to_the_horizon, "light_below_the_floor": _light_below_the_floor,
         "light_in_a_bound": _light_in_a_bound, "two_lights": _two_lights, "resting_sphere": _resting_sphere,
         "no_rotation": _no_rotation, "seven_slots": _seven_slots, "wide_canvas": _two_lights}


@pytest.mark.parametrize("which", list(EDGES))
def test_cull_edges(gpu_ctx, rtc, oracle, monkeypatch, which):
    from rtc_amd import world as W
    world, (frm, to, up) = EDGES[which]()
    size = (2064, 40) if which == "wide_canvas" else (333, 201)  # (2064: past the 2048 pixels of the tables)
    cam = W.camera(size[0], size[1], 1.0, frm, to, up)
    tables = world.tables(cam)
    frames = _frames(gpu_ctx, rtc, monkeypatch, tables, cam, 0.6931471 + len(which) * 1e-6)
    _assert_same(frames, which)
    a = frames[0][0]
    ref, _ = oracle.render(tables, cam, 6, threads=8)
    assert _pix_agree(a, ref, oracle) >= F32_PIX_FRAC
    if which == "seven_slots":
        assert len(tables.shapes) == 7  # (past rtc_internal.hpp kShadowRectSlots)
    floor = a[-8:].reshape(-1, 3)  # the bottom rows: floor, lit or (light below) in ambient light alone
    assert floor.any()
    if which in ("across_blocks", "two_lights", "resting_sphere", "no_rotation"):
        # the picture holds a shadow on the floor: floor pixels well below the lit floor's brightness
        lum = a.sum(axis=2)
        lit = np.median(lum[-8:])
        assert lit > 0 and (lum[size[1] // 3:] < 0.5 * lit).sum() > 50


def test_one_shard_of_eight_equals_its_rows_of_the_frame(gpu_ctx, rtc):
    import torch
    scene = scene_fixture("three_sphere_scene")
    cam = rtc.camera_resize(scene.camera, 640, 400)
    shard, shards = 5, 8
    gpu_ctx.upload(scene)
    gpu_ctx.set_jit(rtc.RT_JIT_SYNC)
    try:
        whole, _ = gpu_ctx.render(cam, 6, precision="f32")
        assert gpu_ctx.jit_status()["used"]
        rows = rtc.shard_rows(400, shards)
        strip = torch.zeros((rows, 640, 3), dtype=torch.float32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        gpu_ctx.render_device(cam, strip.data_ptr(), s, 6, "f32", "real", (shard, shards))
        assert gpu_ctx.jit_status()["used"]
        nos = torch.zeros_like(strip)
        gpu_ctx.render_device(cam, nos.data_ptr(), s, 6, "f32", "real", (shard, shards), rtc.RT_FLAG_NO_SKIPS)
        assert gpu_ctx.jit_status()["used"]
        torch.cuda.synchronize()
    finally:
        gpu_ctx.set_jit(rtc.RT_JIT_AUTO)
    owner, strip_row = rtc.shard_row_map(400, shards)
    mine = np.flatnonzero(owner == shard)
    assert len(mine) > 0
    got = strip.cpu().numpy()
    assert np.array_equal(got[strip_row[mine]], whole[mine]), "the shard's strip differs from its rows of the frame"
    assert np.array_equal(got, nos.cpu().numpy())
