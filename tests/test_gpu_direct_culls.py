"""The per-scene f32 direct kernel's primary cull changes nothing, on the device.

A camera frame's launch hands the kernel one screen rectangle per shape slot
(primary_rect.hpp); a wave whose 16 x 4 pixel block misses a shape's rectangle
passes the shape by before the per-lane ball test (rtc_kernels.hip
closest_hit, wave_pixel_block).  Acceleration only, so the frame must equal,
bit for bit and counter for counter,

* the RT_FLAG_NO_SKIPS frame (a per-scene build without the rectangles), and
* the frame of a context under RTC_DEBUG=cull=0 (every bound +inf: every
  rectangle the whole canvas, every ball test passing),

at 320x200 and at 333x201 (ragged right and bottom tiles), with the camera
inside a sphere's ball, with every sphere behind the camera, on one shard of
eight (the block's rows go through the shard's row map), and on cover (the
pool kernel, which takes no rectangles).
"""
import numpy as np
import pytest

from conftest import scene_fixture
from test_gpu_parity import _counts

pytestmark = pytest.mark.gpu


def _three_ways(gpu_ctx, rtc, monkeypatch, scene, cam, what):
    gpu_ctx.upload(scene)
    gpu_ctx.set_jit(rtc.RT_JIT_SYNC)
    try:
        a, sa = gpu_ctx.render(cam, 6, precision="f32")
        assert gpu_ctx.jit_status()["used"], gpu_ctx.jit_status()
        b, sb = gpu_ctx.render(cam, 6, precision="f32", flags=rtc.RT_FLAG_NO_SKIPS)
        assert gpu_ctx.jit_status()["used"], gpu_ctx.jit_status()
    finally:
        gpu_ctx.set_jit(rtc.RT_JIT_AUTO)
    monkeypatch.setenv("RTC_DEBUG", "cull=0")
    with rtc.Context(0) as nocull:
        nocull.set_jit(rtc.RT_JIT_SYNC)
        nocull.upload(scene)
        c, sc = nocull.render(cam, 6, precision="f32")
        assert nocull.jit_status()["used"], nocull.jit_status()
    assert np.array_equal(a, b), f"{what}: the culls changed {int((a != b).any(axis=2).sum())} px against RT_FLAG_NO_SKIPS"
    assert np.array_equal(a, c), f"{what}: the culls changed {int((a != c).any(axis=2).sum())} px against cull=0"
    assert _counts(sa) == _counts(sb) == _counts(sc)
    return a


@pytest.mark.parametrize("size", [(320, 200), (333, 201)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["three_sphere_scene", "shadow_puppets"])
def test_direct_culls_are_exact(gpu_ctx, rtc, monkeypatch, name, size):
    scene = scene_fixture(name)
    cam = rtc.camera_resize(scene.camera, *size)
    a = _three_ways(gpu_ctx, rtc, monkeypatch, scene, cam, f"{name} {size}")
    assert a.any()


@pytest.mark.parametrize("where", ["inside", "behind"])
def test_camera_inside_a_sphere_and_facing_away(gpu_ctx, rtc, monkeypatch, where):
    """inside: the eye within the middle sphere (centre (-0.5, 1, 0.5), radius 1): its rectangle is
    the whole canvas; behind: the camera looks away from all three spheres: empty rectangles."""
    scene = scene_fixture("three_sphere_scene")
    if where == "inside":
        cam = rtc.camera_make(333, 201, 1.2, (-0.5, 1.0, 0.2), (1.5, 0.5, -0.5), (0, 1, 0))
        bound = (-0.5, 1.0, 0.5, 1.0)
        assert rtc.camera_bound_rect(cam, bound) == (0, 0, 332, 200)
    else:
        cam = rtc.camera_make(333, 201, 1.2, (0, 1.5, -5), (0, 1.0, -10), (0, 1, 0))
        x0, _, x1, _ = rtc.camera_bound_rect(cam, (-0.5, 1.0, 0.5, 1.0))
        assert x0 > x1
    _three_ways(gpu_ctx, rtc, monkeypatch, scene, cam, where)


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
        torch.cuda.synchronize()
    finally:
        gpu_ctx.set_jit(rtc.RT_JIT_AUTO)
    owner, strip_row = rtc.shard_row_map(400, shards)
    mine = np.flatnonzero(owner == shard)
    assert len(mine) > 0
    got = strip.cpu().numpy()
    assert np.array_equal(got[strip_row[mine]], whole[mine]), "the shard's strip differs from its rows of the frame"
    assert np.array_equal(got, nos.cpu().numpy())


def test_cover_pool_path_is_unchanged(gpu_ctx, rtc):
    scene = scene_fixture("cover")
    cam = rtc.camera_resize(scene.camera, 320, 200)
    gpu_ctx.upload(scene)
    gpu_ctx.set_jit(rtc.RT_JIT_SYNC)
    try:
        a, sa = gpu_ctx.render(cam, 6, precision="f32")
        b, sb = gpu_ctx.render(cam, 6, precision="f32", flags=rtc.RT_FLAG_NO_SKIPS)
    finally:
        gpu_ctx.set_jit(rtc.RT_JIT_AUTO)
    assert np.array_equal(a, b), f"cover: the skips changed {int((a != b).any(axis=2).sum())} px"
    assert _counts(sa) == _counts(sb)
