"""The head and tail of the per-scene f32 direct kernel's tile loop change nothing.

Two pieces of rtc_kernels.hip direct_tile, each behind a build switch:

* RTC_EDGE_CLAMP: lanes past the canvas edge trace the clamped pixel, a pixel
  of a valid lane of the same block, instead of being masked off round the ray
  and the shading; `valid` guards the store and the counters alone.
* RTC_HEAD_CLAUSE: the launch words and the camera of one iteration come in
  one scalar load clause at its top (TileHead).

The same pixels by another road, so every frame must equal, bit for bit and
counter for counter, the frame of the same kernel with each switch off alone
and with both off (contexts created under RTC_DEBUG=jit_flags=...), the
RT_FLAG_NO_SKIPS frame and the generic kernel's frame (RT_JIT_OFF); the f32
frame must lie within the f32 floor of the oracle, and the rays counted must
be the oracle's: a clamped lane is counted nowhere.

Canvases are the smallest at which a piece can go wrong: 1x1; 15x3, less than
one 16x4 block; 16x4, one block; 17x5, one more column and row of blocks; 64x4,
one tile; 70x6, whose tile 2 has one ragged block and three wholly off the
canvas; 333x201, ragged right and bottom, as a frame, as shard 5 of 8 (strip
rows), as eight shards stored at their image rows of a canvas (image_rows = 1,
rt_render_to_canvas) and as a u8 frame; 2064x8, beyond the cull tables.  On
three_sphere_scene, shadow_puppets and a world whose sphere's silhouette
crosses the right and the bottom canvas edge at 17x5 and 70x6, so that clamped
lanes repeat sphere pixels in waves that are otherwise plane-uniform.

A world's five builds (default, RT_FLAG_NO_SKIPS, three switched off) are
compiled side by side, once for all its canvases (a build does not depend on
the camera), as in test_gpu_launch_terms; an off-context uploads the world with
one more material that no shape uses (test_gpu_uniform_hit._salted): a table,
and so a build, of its own.
"""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from conftest import scene_fixture
from test_gpu_parity import F32_PIX_FRAC, _counts, _pix_agree
from test_gpu_uniform_hit import _salted

pytestmark = pytest.mark.gpu

SWITCHES = ["RTC_EDGE_CLAMP", "RTC_HEAD_CLAUSE"]
OFFS = {f"{s}=0": f"jit_flags=-D{s}=0" for s in SWITCHES}
OFFS["both off"] = "jit_flags=" + " ".join(f"-D{s}=0" for s in SWITCHES)
DEPTH = 6


@contextmanager
def _rtc_debug(knob):
    old = os.environ.get("RTC_DEBUG")
    os.environ["RTC_DEBUG"] = knob
    try:
        yield
    finally:
        if old is None:
            del os.environ["RTC_DEBUG"]
        else:
            os.environ["RTC_DEBUG"] = old


# ------------------------------------------------------------------ the worlds
def _edge_view(w, h):
    """(fov, from, to, up): the sphere at the origin (radius 1) sits in the bottom right corner of a w x h frame."""
    fov = 1.0
    dist = 20 if w > 8 * h else 5  # (70x6: from far enough that six rows are taller than the sphere)
    half_w = np.tan(fov / 2)
    half_h = half_w * h / w
    # the view axis passes left of and above the sphere by the frame's half extent at the sphere's distance
    # (the oracle's frames: the sphere takes columns 13..16 of rows 1..4 at 17x5, columns 66..69 of rows 2..5 at 70x6)
    return fov, (0, 0, -dist), (-dist * half_w, dist * half_h, 0), (0, 1, 0)


def _edge_world():
    from rtc_amd import world as W
    ball = W.sphere(W.Material(color=(1.0, 0.1, 0.1), diffuse=0.7, specular=0.3))
    wall = W.plane(W.Material(color=(0.1, 0.1, 1.0), specular=0.0), W.mat_mul(W.translation(0, 0, 6), W.rotation_x(np.pi / 2)))
    floor = W.plane(W.Material(color=(0.1, 0.2, 0.9), specular=0.0), W.translation(0, -4, 0))
    return W.World([W.Light((-6, 8, -8))], [floor, wall, ball])


def _world(rtc, name):
    """(tables, camera(w, h)) of a world of this file."""
    if name == "edge_sphere":
        from rtc_amd import world as W
        tables = _edge_world().tables(W.camera(17, 5, *_edge_view(17, 5)))
        return tables, lambda w, h: W.camera(w, h, *_edge_view(w, h))
    scene = scene_fixture(name)
    return scene, lambda w, h: rtc.camera_resize(scene.camera, w, h)


class _Builds:
    """The contexts of one world: gpu_ctx (default, RT_FLAG_NO_SKIPS, generic) and one per entry of OFFS."""

    def __init__(self, gpu_ctx, rtc, name):
        self.name, self.ctx, self.rtc, self.offs = name, gpu_ctx, rtc, []
        self.scene, self.camera = _world(rtc, name)
        kick = self.camera(512, 128)  # 256 tiles: a frame that asks for a build
        try:
            gpu_ctx.upload(self.scene)
            gpu_ctx.set_jit(rtc.RT_JIT_EAGER)
            gpu_ctx.render(kick, DEPTH, precision="f32")
            gpu_ctx.render(kick, DEPTH, precision="f32", flags=rtc.RT_FLAG_NO_SKIPS)
            for i, knob in enumerate(OFFS.values()):
                with _rtc_debug(knob):
                    off = rtc.Context(0)
                    self.offs.append(off)
                    off.set_jit(rtc.RT_JIT_EAGER)
                    off.upload(_salted(rtc, self.scene, 0.5772156 + 1e-3 * i + 1e-5 * len(name)))
                    off.render(kick, DEPTH, precision="f32")
            for ctx in [gpu_ctx] + self.offs:
                assert ctx.jit_wait() == 0
        except BaseException:
            self.close()
            raise
        finally:
            gpu_ctx.set_jit(rtc.RT_JIT_AUTO)

    def close(self):
        for off in self.offs:
            off.close()
        self.offs = []

    def frames(self, render):
        """{build: render(ctx, per_scene, **kw)} for every build; `render` returns whatever is compared."""
        rtc, ctx, out = self.rtc, self.ctx, {}
        try:
            ctx.upload(self.scene)  # (the session's context: another test's world may be in it)
            ctx.set_jit(rtc.RT_JIT_SYNC)
            out["default"] = render(ctx, True)
            out["RT_FLAG_NO_SKIPS"] = render(ctx, True, flags=rtc.RT_FLAG_NO_SKIPS)
            ctx.set_jit(rtc.RT_JIT_OFF)
            out["the generic kernel"] = render(ctx, False)
            for (name, knob), off in zip(OFFS.items(), self.offs):
                with _rtc_debug(knob):  # (a build made in line would be this context's kind too)
                    off.set_jit(rtc.RT_JIT_SYNC)
                    out[name] = render(off, True)
        finally:
            ctx.set_jit(rtc.RT_JIT_AUTO)
        return out


@pytest.fixture(scope="module")
def builds(gpu_ctx, rtc):
    """builds(name): the world's contexts, compiled once for the tests of this file."""
    held = {}

    def get(name):
        if name not in held:
            held[name] = _Builds(gpu_ctx, rtc, name)
        return held[name]

    yield get
    for b in held.values():
        b.close()


def _frame(cam, shard=(0, 1), out_format="real"):
    def render(ctx, per_scene, **kw):
        f, st = ctx.render(cam, DEPTH, precision="f32", out_format=out_format, shard=shard, **kw)
        assert bool(ctx.jit_status()["used"]) == per_scene, ctx.jit_status()
        return f, _counts(st)
    return render


def _assert_same(frames, what):
    a, sa = frames["default"]
    for name, (f, s) in frames.items():
        assert np.array_equal(a, f), f"{what}: {int((a != f).any(axis=2).sum())} px differ from {name}"
        assert sa == s, (what, name, sa, s)


WORLDS = ["three_sphere_scene", "shadow_puppets", "edge_sphere"]
SIZES = [(1, 1), (15, 3), (16, 4), (17, 5), (64, 4), (70, 6), (333, 201), (2064, 8)]



@pytest.mark.parametrize("name,size", [(n, s) for n in WORLDS for s in SIZES],
                         ids=[f"{n}-{s[0]}x{s[1]}" for n in WORLDS for s in SIZES])
def test_frames_are_exact(builds, oracle, name, size):
    b = builds(name)
    cam = b.camera(*size)
    frames = b.frames(_frame(cam))
    _assert_same(frames, f"{name} {size}")
    a, counts = frames["default"]
    ref, ref_st = oracle.render(b.scene, cam, DEPTH, threads=8)
    assert counts == _counts(ref_st), (counts, _counts(ref_st))
    assert counts["primary"] == size[0] * size[1]
    assert _pix_agree(a, ref, oracle) >= F32_PIX_FRAC
    if name == "edge_sphere" and size in [(17, 5), (70, 6)]:
        ball = a[:, :, 0] > a[:, :, 2]  # (the sphere is red, the planes are blue)
        for edge, line in (("right", ball[:, -1]), ("bottom", ball[-1, :])):
            assert line.any() and not line.all(), f"the silhouette does not cross the {edge} edge at {size}"
        assert ball[-1, -1] and not ball[0, 0]


@pytest.mark.parametrize("name", WORLDS)
def test_u8_frame(builds, oracle, name):
    b = builds(name)
    cam = b.camera(333, 201)
    frames = b.frames(_frame(cam, out_format="u8"))
    _assert_same(frames, f"{name} u8")
    a, counts = frames["default"]
    assert a.dtype == np.uint8 and a.any()
    ref, ref_st = oracle.render(b.scene, cam, DEPTH, threads=8)
    assert counts == _counts(ref_st)
    d = np.abs(a.astype(int) - oracle.quantize(ref).astype(int)).max(axis=2)
    assert float((d <= 2).mean()) >= F32_PIX_FRAC


@pytest.mark.parametrize("name", WORLDS)
def test_one_shard_of_eight(builds, rtc, name):
    """Strip rows: shard 5 of 8 of 333x201 is its rows of the whole frame, and counts its own pixels alone."""
    b = builds(name)
    cam = b.camera(333, 201)
    shard, shards = 5, 8
    strips = b.frames(_frame(cam, shard=(shard, shards)))
    _assert_same(strips, f"{name} shard 5 of 8")
    whole, whole_counts = b.frames(_frame(cam))["default"]
    owner, strip_row = rtc.shard_row_map(201, shards)
    mine = np.flatnonzero(owner == shard)
    assert len(mine) > 0
    got, counts = strips["default"]
    assert np.array_equal(got[strip_row[mine]], whole[mine]), "the shard's strip differs from its rows of the frame"
    assert counts["primary"] == 333 * len(mine)


@pytest.mark.parametrize("name", WORLDS)
def test_image_rows_on_a_canvas(builds, rtc, name):
    """image_rows = 1 within one context: eight shards stored at their image rows of a canvas make the whole frame."""
    b = builds(name)
    cam = b.camera(333, 201)
    shards = 8

    def render(ctx, per_scene, **kw):
        if kw:  # (rt_render_to_canvas takes no flags: the RT_FLAG_NO_SKIPS frame is the plain one)
            return None
        before = _counts(ctx.counters())
        canvas, _ = ctx.canvas_create(333 * 201 * 3 * 4, shards, ipc=False)
        try:
            for shard in range(shards):
                ctx.render_to_canvas(cam, canvas, 1, DEPTH, "f32", "real", (shard, shards))
                assert bool(ctx.jit_status()["used"]) == per_scene, ctx.jit_status()
            ctx.canvas_wait(canvas, 1)
            img = ctx.canvas_read(canvas, (201, 333, 3), np.float32)
        finally:
            ctx.canvas_close(canvas)
        after = _counts(ctx.counters())
        return img, {k: after[k] - before[k] for k in after}

    frames = {k: v for k, v in b.frames(render).items() if v is not None}
    assert len(frames) == 2 + len(OFFS)
    _assert_same(frames, f"{name} canvas")
    whole, whole_counts = b.frames(_frame(cam))["default"]
    img, counts = frames["default"]
    assert np.array_equal(img, whole), f"{int((img != whole).any(axis=2).sum())} px of the canvas differ from the frame"
    assert counts == whole_counts, (counts, whole_counts)
