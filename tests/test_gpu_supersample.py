"""Supersampled frames (rt_render_supersampled*) on the GPU.

A supersampled frame of camera C (W x H) with grid n is the n x n box mean of
the frame of the sample camera Cn = camera_resize(C, n W, n H): sample (i, j)
of pixel (x, y) is Cn's pixel (n x + i, n y + j).  So the oracle of the
feature is pyoracle.render(scene, Cn) averaged in f64, its counters are the
counters, and the f32 kernels' sample colours are those of rt_render at Cn.

Shapes are ragged against the 64 x 4 tile and the 16 x 4 wave block: 70 x 22
and 130 x 10 outputs, plus 320 x 200 for the f32-against-oracle shares.
"""
import functools

import numpy as np
import pytest

from conftest import scene_fixture
from test_supersample_cpu import U8_CASES, box_mean, near_boundary

pytestmark = pytest.mark.gpu

ABS64 = 1e-9  # the project's f64 bar
COUNTERS = ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned", "refract_evals", "schlick_evals")
DIRECT = ("three_sphere_scene", "shadow_puppets")
POOL = ("reflect_refract", "refraction")
SHAPES = [(70, 22, 2), (70, 22, 3), (130, 10, 4)]
ALL_SCENES = ["three_sphere_scene", "reflect_refract", "cover", "table", "cylinders", "metal", "refraction",
              "shadow_puppets"]
RT_FLAG_STAMPS, RT_FLAG_NO_SKIPS = 8, 64

# f32 pool frames against the f64 box mean of rt_render's f32 frame of Cn:
# the largest |difference| observed per scene over SHAPES on MI355X
# (the test prints it; profiles/supersample_parity.json, "pool_f32_vs_plain").  Both sides are
# bit-deterministic; the test asserts twice this, and below (2/255)/4 always.
POOL_F32_OBSERVED = {
    "reflect_refract": 3.688037395477295e-07,
    "refraction": 1.0849907994270325e-07,
}
# f32 supersampled frames, 320 x 200, n = 2, against the averaged oracle:
# observed share of pixels within 2/255 after quantization (same file,
# "f32_vs_oracle"); the floor is the share minus 0.005.
F32_SHARE_OBSERVED = {
    "three_sphere_scene": 1.0,
    "reflect_refract": 0.999953125,
    "cover": 0.999984375,
    "table": 0.9999375,
    "cylinders": 0.9914375,
    "metal": 1.0,
    "refraction": 0.9933125,
    "shadow_puppets": 1.0,
}


def _counts(st):
    return {k: st[k] for k in COUNTERS}


@functools.lru_cache(maxsize=None)
def _dup_world():
    """The first seeded random world (tests/test_gpu_random_worlds.py) that holds a
    value-equal copy of a shape and secondary rays at a depth above 0."""
    from test_gpu_random_worlds import _random_world, depth_has_pool
    for seed in range(48):
        tables, cam, depth = _random_world(seed)
        copies = len(tables.shapes) - len(_random_world(seed, allow_dup=False)[0].shapes)
        if copies > 0 and depth > 0 and depth_has_pool(tables):
            return tables, cam, depth
    raise AssertionError("no seed with a value-equal copy")


def _world(name):
    """(tables, base camera, depth) of a reference scene or of the random world."""
    if name == "random_dup":
        return _dup_world()
    scene = scene_fixture(name)
    return scene, scene.camera, 6


@functools.lru_cache(maxsize=None)
def _oracle_frames(name, w, h, n, depth=None):
    """(averaged oracle frame, the Cn frame's stats), computed once per case; read-only."""
    import pyoracle
    import rtc_amd
    tables, cam, d = _world(name)
    cn = rtc_amd.camera_resize(cam, n * w, n * h)
    ref, st = pyoracle.render(tables, cn, d if depth is None else depth, threads=8)
    mean = box_mean(ref, n)
    mean.setflags(write=False)
    return mean, st


def _upload(ctx, name):
    tables, cam, depth = _world(name)
    ctx.upload(tables)
    return cam, depth


# ------------------------------------------------------------------ 1. f64 against the oracle
@pytest.mark.parametrize("w,h,n", SHAPES)
@pytest.mark.parametrize("name", DIRECT + POOL + ("random_dup",))
def test_f64_matches_the_averaged_oracle(gpu_ctx, rtc, name, w, h, n):
    cam, depth = _upload(gpu_ctx, name)
    c = rtc.camera_resize(cam, w, h)
    img, st = gpu_ctx.render_supersampled(c, n, depth, precision="f64")
    ref, rst = _oracle_frames(name, w, h, n)
    assert img.shape == (h, w, 3)
    err = float(np.abs(img - ref).max())
    print(f"{name} {w}x{h} n={n}: max |err| {err:.3g}")
    assert err < ABS64, err
    assert _counts(st) == _counts(rst) and st["primary"] == n * n * w * h


# ------------------------------------------------------------------ 2. n = 1 is rt_render
@pytest.mark.parametrize("jit", [0, 1])
@pytest.mark.parametrize("precision,out_format", [("f32", "real"), ("f64", "real"), ("f32", "u8"), ("f64", "u8")])
@pytest.mark.parametrize("name", ["three_sphere_scene", "reflect_refract"])
def test_grid_one_is_rt_render(gpu_ctx, rtc, name, precision, out_format, jit):
    cam, depth = _upload(gpu_ctx, name)
    c = rtc.camera_resize(cam, 70, 22)
    gpu_ctx.set_jit(jit)  # 0: generic kernels, 1: RT_JIT_SYNC
    try:
        a, sa = gpu_ctx.render(c, depth, precision=precision, out_format=out_format)
        b, sb = gpu_ctx.render_supersampled(c, 1, depth, precision=precision, out_format=out_format)
    finally:
        gpu_ctx.set_jit(2)
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert _counts(sa) == _counts(sb)


# ------------------------------------------------------------------ 3. u8
@pytest.mark.parametrize("name,w,h,n", U8_CASES)
def test_u8_is_quantized_once_after_the_mean(gpu_ctx, rtc, oracle, name, w, h, n):
    cam, depth = _upload(gpu_ctx, name)
    img, _ = gpu_ctx.render_supersampled(rtc.camera_resize(cam, w, h), n, depth, precision="f64", out_format="u8")
    ref, _ = _oracle_frames(name, w, h, n)
    exempt = near_boundary(ref, ABS64)
    assert exempt.mean() <= 0.001
    assert img.dtype == np.uint8
    assert np.array_equal(img[~exempt], oracle.quantize(ref)[~exempt])


# ------------------------------------------------------------------ 4. f32 against the shipped path
def _ordered_f32_mean(frame, n):
    """The direct kernel's sum of an f32 Cn frame: plain f32, j outer, i inner, one multiply."""
    acc = np.zeros((frame.shape[0] // n, frame.shape[1] // n, 3), dtype=np.float32)
    for j in range(n):
        for i in range(n):
            acc = acc + frame[j::n, i::n]
    return acc * (np.float32(1) / np.float32(n * n))


@pytest.mark.parametrize("w,h,n", SHAPES)
@pytest.mark.parametrize("name", DIRECT)
def test_f32_direct_is_the_ordered_sum_of_the_shipped_frame(gpu_ctx, rtc, name, w, h, n):
    cam, depth = _upload(gpu_ctx, name)
    plain, _ = gpu_ctx.render(rtc.camera_resize(cam, n * w, n * h), depth, precision="f32")
    img, _ = gpu_ctx.render_supersampled(rtc.camera_resize(cam, w, h), n, depth, precision="f32")
    want = _ordered_f32_mean(plain, n)
    assert want.dtype == np.float32 and img.dtype == np.float32
    bound = n * n * 2.0 ** -23 * np.maximum(1.0, np.abs(want.astype(np.float64)))
    d = np.abs(img.astype(np.float64) - want.astype(np.float64))
    print(f"{name} {w}x{h} n={n}: max |diff| {float(d.max()):.3g}, {int((d > 0).sum())} elements differ")
    assert (d <= bound).all(), float((d - bound).max())


@pytest.mark.parametrize("name", POOL)
def test_f32_pool_is_the_mean_of_the_shipped_frame(gpu_ctx, rtc, name):
    """Fixed-point rounding only: n^2 samples' contributions rounded into the
    pixel's sums here, each sample pixel's into its own there."""
    cam, depth = _upload(gpu_ctx, name)
    worst = 0.0
    for w, h, n in SHAPES:
        plain, _ = gpu_ctx.render(rtc.camera_resize(cam, n * w, n * h), depth, precision="f32")
        img, _ = gpu_ctx.render_supersampled(rtc.camera_resize(cam, w, h), n, depth, precision="f32")
        d = float(np.abs(img.astype(np.float64) - box_mean(plain, n)).max())
        print(f"{name} {w}x{h} n={n}: max |diff| {d:.3g}")
        worst = max(worst, d)
    assert worst < (2.0 / 255.0) / 4.0, worst  # anything larger is a bug, not rounding
    assert worst <= 2.0 * POOL_F32_OBSERVED[name], (worst, POOL_F32_OBSERVED[name])


# ------------------------------------------------------------------ 5. f32 against the oracle
@pytest.mark.parametrize("name", ALL_SCENES)
def test_f32_share_within_two_levels_of_the_oracle(gpu_ctx, rtc, oracle, name):
    import f32_tolerance
    cam, depth = _upload(gpu_ctx, name)
    w, h, n = 320, 200, 2
    img, st = gpu_ctx.render_supersampled(rtc.camera_resize(cam, w, h), n, depth, precision="f32")
    ref, rst = _oracle_frames(name, w, h, n)
    d = np.abs(oracle.quantize(img.astype(np.float64)).astype(int) - oracle.quantize(ref).astype(int)).max(axis=2)
    share = float((d <= 2).mean())
    print(f"{name}: {share:.6f} of pixels within 2/255")
    for k in ("primary", "shadow", "reflect", "refract"):
        assert abs(st[k] - rst[k]) <= max(3, f32_tolerance.KIND * rst[k]), (name, k, st[k], rst[k])
    assert st["primary"] == rst["primary"] == n * n * w * h
    assert share >= F32_SHARE_OBSERVED[name] - 0.005, (share, F32_SHARE_OBSERVED[name])


# ------------------------------------------------------------------ 6. exactness
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", ["three_sphere_scene", "reflect_refract", "random_dup"])
def test_no_skips_and_repeats_are_bit_identical(gpu_ctx, rtc, name, precision):
    cam, depth = _upload(gpu_ctx, name)
    c = rtc.camera_resize(cam, 70, 22)
    a, sa = gpu_ctx.render_supersampled(c, 2, depth, precision=precision)
    b, sb = gpu_ctx.render_supersampled(c, 2, depth, precision=precision, flags=RT_FLAG_NO_SKIPS)
    a2, sa2 = gpu_ctx.render_supersampled(c, 2, depth, precision=precision)
    assert a.tobytes() == b.tobytes() and _counts(sa) == _counts(sb)
    assert a.tobytes() == a2.tobytes() and _counts(sa) == _counts(sa2)


@pytest.mark.parametrize("flags", [0, RT_FLAG_NO_SKIPS])
@pytest.mark.parametrize("name,n", [("three_sphere_scene", 3), ("shadow_puppets", 2), ("metal", 2),
                                    ("reflect_refract", 2)])
def test_per_scene_kernels_are_bit_identical(gpu_ctx, rtc, name, n, flags):
    """The supersampled kernels built per scene (RT_JIT_SYNC) against the generic ones; the
    direct build takes no primary cull, so its frame is the RT_FLAG_NO_SKIPS frame too.
    Direct and pool builds of these scenes must be taken (rtc_jit.cpp kPoolSsScratchMax)."""
    cam, depth = _upload(gpu_ctx, name)
    c = rtc.camera_resize(cam, 70, 22)
    gpu_ctx.set_jit(0)
    try:
        a, sa = gpu_ctx.render_supersampled(c, n, depth, precision="f32")
        assert not gpu_ctx.jit_status()["used"]
        gpu_ctx.set_jit(1)
        b, sb = gpu_ctx.render_supersampled(c, n, depth, precision="f32", flags=flags)
        status = gpu_ctx.jit_status()
        assert status["used"], status["log"][:2000]
        b2, _ = gpu_ctx.render_supersampled(c, n, depth, precision="f32", flags=flags)
    finally:
        gpu_ctx.set_jit(2)
    assert a.tobytes() == b.tobytes() == b2.tobytes() and _counts(sa) == _counts(sb)


def test_refused_per_scene_build_falls_back_to_the_generic_kernel(rtc, monkeypatch):
    """A per-scene supersampled pool build that may use no scratch at all is refused (the
    library's own rule allows these some): the launch takes the generic supersampled
    kernel, says why, and renders the same frame."""
    scene = scene_fixture("reflect_refract")
    c = rtc.camera_resize(scene.camera, 70, 22)
    with rtc.Context(0) as ctx:
        ctx.upload(scene)
        ctx.set_jit(0)
        a, sa = ctx.render_supersampled(c, 2, 6, precision="f32")
    monkeypatch.setenv("RTC_DEBUG", "jit_ss_scratch=0")
    with rtc.Context(0) as ctx:
        ctx.upload(scene)
        ctx.set_jit(1)
        b, sb = ctx.render_supersampled(c, 2, 6, precision="f32")
        status = ctx.jit_status()
    assert not status["used"] and "supersampled pool kernel not used" in status["log"], status
    assert a.tobytes() == b.tobytes() and _counts(sa) == _counts(sb)


def test_plain_and_supersampled_launches_keep_their_own_tile_orders(rtc):
    """plain, ss, plain, ss of one camera on one context (a pool world: cost-ordered
    tiles) equal the frames of fresh contexts, and so do a few more of each."""
    scene = scene_fixture("reflect_refract")
    c = rtc.camera_resize(scene.camera, 70, 22)

    def fresh(ss):
        with rtc.Context(0) as ctx:
            ctx.upload(scene)
            return ctx.render_supersampled(c, 2, 6, precision="f32") if ss else ctx.render(c, 6, precision="f32")

    (plain, sp), (sup, ss) = fresh(False), fresh(True)
    with rtc.Context(0) as ctx:
        ctx.upload(scene)
        for rnd in range(3):
            a, sa = ctx.render(c, 6, precision="f32")
            b, sb = ctx.render_supersampled(c, 2, 6, precision="f32")
            assert a.tobytes() == plain.tobytes() and _counts(sa) == _counts(sp), rnd
            assert b.tobytes() == sup.tobytes() and _counts(sb) == _counts(ss), rnd


def test_supersampled_launch_leaves_the_plain_tile_costs_alone(rtc):
    """Frames do not depend on the tile order (fixed-point sums), so the separation is
    checked where it lives: the per-tile costs a plain pool launch recorded
    (rt_debug_tile_costs) are still there, word for word, after supersampled launches of
    the same camera, whose tiles cost n^2 samples each and go to costs of their own."""
    scene = scene_fixture("reflect_refract")
    c = rtc.camera_resize(scene.camera, 70, 22)
    tiles = ((70 + 63) // 64) * ((22 + 3) // 4)
    with rtc.Context(0) as ctx:
        ctx.upload(scene)
        ctx.render(c, 6, precision="f32")
        before = ctx.debug_tile_costs()
        assert len(before) >= tiles and (before[:tiles] > 0).all()
        for _ in range(3):  # (the second and third build an order from the first one's costs)
            ctx.render_supersampled(c, 4, 6, precision="f32")
        after = ctx.debug_tile_costs()
        assert np.array_equal(before, after)
        ctx.render(c, 6, precision="f32")
        again = ctx.debug_tile_costs()
        assert len(again) == len(before) and (again[:tiles] > 0).all()


# ------------------------------------------------------------------ 7. shards
@pytest.mark.parametrize("precision,out_format", [("f32", "real"), ("f32", "u8")])
@pytest.mark.parametrize("name", ["three_sphere_scene", "reflect_refract"])
def test_three_shards_assemble_to_the_whole_frame(gpu_ctx, rtc, name, precision, out_format):
    cam, depth = _upload(gpu_ctx, name)
    c = rtc.camera_resize(cam, 70, 22)
    whole, st = gpu_ctx.render_supersampled(c, 2, depth, precision=precision, out_format=out_format)
    shard_of, row_of = rtc.shard_row_map(c.height, 3)
    strips, primary = [], 0
    for s in range(3):
        strip, sst = gpu_ctx.render_supersampled(c, 2, depth, precision=precision, out_format=out_format,
                                                 shard=(s, 3))
        strips.append(strip)
        primary += sst["primary"]
    got = np.stack([strips[shard_of[y]][row_of[y]] for y in range(c.height)])
    assert got.tobytes() == whole.tobytes()
    assert primary == st["primary"] == 4 * 70 * 22


# ------------------------------------------------------------------ 8. pool bound
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_deepest_grid_never_overflows_the_pool(gpu_ctx, rtc, precision):
    """n = 4 at depth 16: 16 seedings of a tile into a pool whose bound is a plain
    frame's (rtc_internal.hpp pool_capacity_ss).  An overflow would raise RT_ERR_POOL."""
    cam, _ = _upload(gpu_ctx, "reflect_refract")
    img, st = gpu_ctx.render_supersampled(rtc.camera_resize(cam, 64, 8), 4, 16, precision=precision)
    ref, rst = _oracle_frames("reflect_refract", 64, 8, 4, 16)
    if precision == "f64":
        assert float(np.abs(img - ref).max()) < ABS64
        assert _counts(st) == _counts(rst)
    else:  # (f32: no error bit; its tolerance against the oracle is test_f32_share_within_two_levels_of_the_oracle's)
        assert np.isfinite(img).all() and st["primary"] == rst["primary"]


# ------------------------------------------------------------------ 9. refusals
def test_refusals(gpu_ctx, rtc):
    from rtc_amd import world as W
    from test_gpu_pool_range import _camera as tp_camera, _world as tp_world
    cam, depth = _upload(gpu_ctx, "three_sphere_scene")
    c = rtc.camera_resize(cam, 70, 22)
    for grid in (0, 5):
        with pytest.raises(rtc.RenderError) as e:
            gpu_ctx.render_supersampled(c, grid, depth)
        assert e.value.code == -1 and "outside 1..4" in str(e.value), str(e.value)
    huge = rtc.camera_resize(cam, 2 ** 31, 8)
    with pytest.raises(rtc.RenderError) as e:
        gpu_ctx.render_supersampled_device(huge, 2, 1, None, depth)
    assert e.value.code == -1 and "1..4" in str(e.value)
    with pytest.raises(rtc.RenderError) as e:
        gpu_ctx.render_supersampled(c, 2, depth, flags=RT_FLAG_STAMPS)
    assert e.value.code == -1 and "RT_FLAG_NO_SKIPS" in str(e.value)
    tp_cam = tp_camera(W)
    gpu_ctx.upload(tp_world(W, on_plane=True).tables(tp_cam))
    for precision in ("f32", "f64"):
        with pytest.raises(rtc.RenderError) as e:
            gpu_ctx.render_supersampled(tp_cam, 2, 6, precision=precision)
        assert "unbounded" in str(e.value)
    with rtc.Context(0) as fresh:
        with pytest.raises(rtc.RenderError) as e:
            fresh.render_supersampled(c, 2, depth)
        assert e.value.code == -4  # RT_ERR_NO_SCENE


def test_one_rank_group_is_accepted(rtc):
    scene = scene_fixture("three_sphere_scene")
    c = rtc.camera_resize(scene.camera, 70, 22)
    with rtc.Context(0) as single:
        single.upload(scene)
        want, sw = single.render_supersampled(c, 2, 6, precision="f32")
    with rtc.Context.multi([0]) as group:
        assert group.group()[0] == 1
        group.upload(scene)
        got, sg = group.render_supersampled(c, 2, 6, precision="f32")
    assert got.tobytes() == want.tobytes() and _counts(sg) == _counts(sw)


# ------------------------------------------------------------------ 10. device entry point
@pytest.mark.parametrize("name", ["reflect_refract", "three_sphere_scene"])
def test_device_entry_on_a_side_stream(gpu_ctx, rtc, name):
    """Into torch tensors on a stream of the caller's, no host sync; a host call on the
    context's stream right behind must wait for them (tests/test_gpu_streams.py's rule)."""
    import torch
    cam, depth = _upload(gpu_ctx, name)
    c = rtc.camera_resize(cam, 130, 10)
    ref, _ = gpu_ctx.render_supersampled(c, 4, depth, precision="f32")
    plain, _ = gpu_ctx.render(c, depth, precision="f32")
    side = torch.cuda.Stream()
    outs = [torch.empty((c.height, c.width, 3), dtype=torch.float32, device="cuda") for _ in range(4)]
    for rnd in range(2):
        for o in outs:
            gpu_ctx.render_supersampled_device(c, 4, o.data_ptr(), side.cuda_stream, depth, "f32")
        img, _ = gpu_ctx.render_supersampled(c, 4, depth, precision="f32")  # context stream, right away
        assert img.tobytes() == ref.tobytes(), rnd
        again, _ = gpu_ctx.render(c, depth, precision="f32")
        assert again.tobytes() == plain.tobytes(), rnd
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            assert o.cpu().numpy().tobytes() == ref.tobytes(), (rnd, i)
