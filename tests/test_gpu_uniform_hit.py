"""The per-scene f32 direct kernel's wave-uniform slot dispatch changes nothing.

A wave of the frame kernel whose hits all lie on one shape shades them with
that shape's slot as a compile-time constant, from a scalar ladder
(rtc_kernels.hip shade_ray, jit_slot_ladder); every other wave keeps the per-lane
record tree.  Same source expressions either way, so the frame must equal,
bit for bit and counter for counter,

* the frame of the same kernel built with -DRTC_UNIFORM_HIT=0 (a context
  created under RTC_DEBUG=jit_flags=...),
* the RT_FLAG_NO_SKIPS frame (a per-scene build without the dispatch), and
* the generic kernel's frame (RT_JIT_OFF),

on the two direct reference scenes at 320x200 and 333x201 (ragged right and
bottom tiles: waves with invalid lanes), on small worlds aimed at the
dispatch's edges (each also within the f32 tolerance of the oracle), and on
one shard of eight.  Worlds of more than six slots (rtc_kernels.hip
kUniformHitSlots: shadow_puppets' eight, the nine spheres here) are past the
dispatch's cap and must come out the same through the per-lane tree.

The process keeps one build per world table whatever the flags, so the
RTC_UNIFORM_HIT=0 context uploads the world with one more material that no
shape uses (_salted): a table of its own, built under its own flags, and the
same picture.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import scene_fixture
from test_gpu_parity import F32_PIX_FRAC, _counts, _pix_agree

pytestmark = pytest.mark.gpu

OFF = "jit_flags=-DRTC_UNIFORM_HIT=0"
SIZES = [(320, 200), (333, 201)]


def _salted(rtc, scene, salt):
    """`scene` plus one matte material no shape refers to (ambient = salt)."""
    n = len(scene.materials)
    mats = (rtc.MaterialDesc * (n + 1))()
    C.memmove(mats, scene.materials, n * C.sizeof(rtc.MaterialDesc))
    extra = mats[n]
    extra.color[:] = [1.0, 1.0, 1.0]
    extra.ambient, extra.diffuse, extra.specular, extra.shininess = salt, 0.9, 0.0, 200.0
    extra.reflectiveness, extra.transparency, extra.refractive_index = 0.0, 0.0, 1.0
    extra.casts_shadow, extra.pattern = 1, -1
    return rtc.SceneTables(scene.shapes, mats, scene.patterns, scene.lights, scene.camera, scene.duplicate_shapes)


def _frames(gpu_ctx, rtc, monkeypatch, scene, cam, salt, depth=6):
    """The default, RTC_UNIFORM_HIT=0, RT_FLAG_NO_SKIPS and generic frames with their stats."""
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
    for name, (f, s) in zip(("RTC_UNIFORM_HIT=0", "RT_FLAG_NO_SKIPS", "the generic kernel"), rest):
        assert np.array_equal(a, f), f"{what}: {int((a != f).any(axis=2).sum())} px differ from {name}"
        assert _counts(sa) == _counts(s), (what, name)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["three_sphere_scene", "shadow_puppets"])
def test_uniform_hit_is_exact(gpu_ctx, rtc, monkeypatch, name, size):
    scene = scene_fixture(name)
    cam = rtc.camera_resize(scene.camera, *size)
    frames = _frames(gpu_ctx, rtc, monkeypatch, scene, cam, 0.3141592 + size[0] * 1e-6)
    _assert_same(frames, f"{name} {size}")
    assert frames[0][0].any()


# ------------------------------------------------------------ the dispatch's edges
def _blocks(img):
    """(block rows, block columns, 4, 16) hit flags of the whole 16x4 pixel blocks (a wave's pixels;
    a miss is exactly black, a hit is not: every material here has ambient light)."""
    hit = img.any(axis=2)
    h, w = hit.shape[0] // 4 * 4, hit.shape[1] // 16 * 16
    return hit[:h, :w].reshape(h // 4, 4, w // 16, 16).transpose(0, 2, 1, 3)


def _two_spheres():
    """No backdrop: blocks mix hits and misses.  The second sphere's silhouette starts inside a block
    column, so in its leftmost blocks the first active lane is not lane 0 (asserted by the test)."""
    from rtc_amd import world as W
    shapes = [W.sphere(W.Material(color=(0.8, 1.0, 0.6), diffuse=0.7, specular=0.2), W.translation(-1.2, 0, 0)),
              W.sphere(W.Material(color=(0.3, 0.4, 1.0)), W.mat_mul(W.translation(1.37, 0.2, 0.5), W.scaling(0.8, 0.8, 0.8)))]
    return W.World([W.Light((-10, 10, -10))], shapes), ((0, 0, -5), (0, 0, 0))


def _matte_and_shiny():
    """A matte floor (specular 0) and a shiny sphere on it share the blocks along the silhouette and the shadow."""
    from rtc_amd import world as W
    shapes = [W.plane(W.Material(color=(1.0, 0.9, 0.9), specular=0.0)),
              W.sphere(W.Material(color=(0.1, 1.0, 0.5), diffuse=0.7, specular=0.9, shininess=50.0), W.translation(0, 1, 0))]
    return W.World([W.Light((-10, 10, -10))], shapes), ((0, 1.5, -5), (0, 1, 0))


def _checkered_floor():
    """A checkered plane fills most blocks whole: pattern code under a constant slot."""
    from rtc_amd import world as W
    shapes = [W.plane(W.Material(pattern=W.checker_pattern((0.9, 0.9, 0.9), (0.2, 0.3, 0.2)), specular=0.0)),
              W.sphere(W.Material(color=(1.0, 0.3, 0.2), specular=0.4, shininess=5.0),
                       W.mat_mul(W.translation(0.5, 0.5, 0), W.scaling(0.5, 0.5, 0.5)))]
    return W.World([W.Light((-4.9, 4.9, -1))], shapes), ((0, 3, -4), (0, 0, 0))


def _two_lights():
    from rtc_amd import world as W
    shapes = [W.plane(W.Material(color=(0.9, 0.9, 1.0), specular=0.0)),
              W.sphere(W.Material(color=(0.8, 1.0, 0.6), diffuse=0.7, specular=0.2), W.translation(-0.8, 1, 0)),
              W.sphere(W.Material(color=(1.0, 0.5, 0.1)), W.mat_mul(W.translation(1.0, 0.5, -0.5), W.scaling(0.5, 0.5, 0.5)))]
    lights = [W.Light((-10, 10, -10)), W.Light((5, 8, -6), (0.3, 0.3, 0.4))]
    return W.World(lights, shapes), ((0, 1.5, -5), (0, 1, 0))


def _nine_spheres():
    """Nine slots: past the dispatch's cap, through the per-lane tree (the build must still be taken)."""
    from rtc_amd import world as W
    shapes = [W.sphere(W.Material(color=(0.2 + 0.1 * i, 1.0 - 0.1 * j, 0.5), specular=0.9 * ((i + j) % 2)),
                       W.mat_mul(W.translation(1.5 * (i - 1), 1.5 * (j - 1), 0), W.scaling(0.7, 0.7, 0.7)))
              for i in range(3) for j in range(3)]
    return W.World([W.Light((-10, 10, -10))], shapes), ((0, 0, -7), (0, 0, 0))


EDGES = {"two_spheres": _two_spheres, "matte_and_shiny": _matte_and_shiny, "checkered_floor": _checkered_floor,
         "two_lights": _two_lights, "nine_spheres": _nine_spheres}


@pytest.mark.parametrize("which", list(EDGES))
def test_dispatch_edges(gpu_ctx, rtc, oracle, monkeypatch, which):
    from rtc_amd import world as W
    world, (frm, to) = EDGES[which]()
    cam = W.camera(333, 201, 1.0, frm, to, (0, 1, 0))
    tables = world.tables(cam)
    frames = _frames(gpu_ctx, rtc, monkeypatch, tables, cam, 0.2718281 + len(which) * 1e-6)
    _assert_same(frames, which)
    a = frames[0][0]
    ref, _ = oracle.render(tables, cam, 6, threads=8)
    assert _pix_agree(a, ref, oracle) >= F32_PIX_FRAC
    blk = _blocks(a)
    whole = int(blk.all(axis=(2, 3)).sum())  # every pixel a hit
    mixed = int((blk.any(axis=(2, 3)) & ~blk.all(axis=(2, 3))).sum())
    if which == "two_spheres":
        assert mixed > 0
        # blocks with hits whose whole left column missed: the first active lane is not the block's first
        late = blk.any(axis=(2, 3)) & ~blk[:, :, :, 0].any(axis=2)
        right = late[:, late.shape[1] // 2:]  # (the second sphere's side of the picture)
        assert int(right.sum()) > 0
    elif which == "checkered_floor":
        assert whole > blk.shape[0] * blk.shape[1] // 2
    elif which == "nine_spheres":
        assert len(tables.shapes) == 9  # (past rtc_kernels.hip kUniformHitSlots)
    else:
        assert whole > 0 and mixed > 0


def test_one_shard_of_eight_equals_its_rows_of_the_frame(gpu_ctx, rtc):
    import torch
    scene = scene_fixture("three_sphere_scene")
    cam = rtc.camera_resize(scene.camera, 640, 400)
    shard, shards = 3, 8
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
