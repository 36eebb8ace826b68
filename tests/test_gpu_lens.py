"""The thin-lens camera (rt_render_lens*) on the GPU.

A lens frame is the ordered mean of World::color_at over the lens rays of include/rtc.h, which
tests/lens_reference.py restates in numpy: that mean, formed with the f64 oracle, is the reference of the f64
kernels (1e-9, counters equal) and of the f32 kernels' shares.  Shapes are ragged against the 64 x 4 tile
and the 16 x 4 wave block: 70 x 22 with n = 2 and 3, 130 x 10 with n = 4.
"""
import numpy as np
import pytest

import f32_tolerance_lens
from conftest import scene_fixture
from test_lens_cpu import APERTURE, U8_CASES, U8_FOCUS, oracle_lens_frame, wall_world
from test_supersample_cpu import near_boundary

pytestmark = pytest.mark.gpu

ABS64 = 1e-9  # the project's f64 bar
COUNTERS = ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned", "refract_evals", "schlick_evals")
# scene -> focal distance (about the camera's distance to what it looks at)
FOCUS = {"three_sphere_scene": 5.0, "shadow_puppets": 20.0, "reflect_refract": 5.0, "refraction": 5.0}
DIRECT = ("three_sphere_scene", "shadow_puppets")
POOL = ("reflect_refract", "refraction")
SHAPES = [(70, 22, 2), (70, 22, 3), (130, 10, 4)]
SEED = 1
RT_FLAG_STAMPS, RT_FLAG_NO_SKIPS = 8, 64


def _counts(st):
    return {k: st[k] for k in COUNTERS}


def _upload(ctx, name):
    scene = scene_fixture(name)
    ctx.upload(scene)
    return scene.camera, 6


def _lens(rtc, name, jitter, seed=SEED, aperture=APERTURE):
    return rtc.Lens(aperture, FOCUS[name], jitter, seed)


# ------------------------------------------------------------------ 1. f64 against the oracle
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("w,h,n", SHAPES)
@pytest.mark.parametrize("name", DIRECT + POOL)
def test_f64_matches_the_oracle_mean_over_the_lens_rays(gpu_ctx, rtc, name, w, h, n, jitter):
    cam, depth = _upload(gpu_ctx, name)
    img, st = gpu_ctx.render_lens(rtc.camera_resize(cam, w, h), n, _lens(rtc, name, jitter), depth, precision="f64")
    ref, rst = oracle_lens_frame(name, w, h, n, APERTURE, FOCUS[name], jitter, SEED)
    assert img.shape == (h, w, 3)
    err = float(np.abs(img - ref).max())
    print(f"{name} {w}x{h} n={n} jitter {jitter}: max |err| {err:.3g}")
    assert err < ABS64, err
    assert _counts(st) == _counts(rst) and st["primary"] == n * n * w * h


def test_the_lens_changes_the_frame(gpu_ctx, rtc):
    """(the effect is there: a lens frame is not the pinhole frame)"""
    cam, depth = _upload(gpu_ctx, "three_sphere_scene")
    c = rtc.camera_resize(cam, 70, 22)
    a, _ = gpu_ctx.render_lens(c, 2, _lens(rtc, "three_sphere_scene", False), depth, precision="f64")
    b, _ = gpu_ctx.render_supersampled(c, 2, depth, precision="f64")
    assert float(np.abs(a - b).mean()) > 0.002


# ------------------------------------------------------------------ 2. aperture 0
@pytest.mark.parametrize("precision,out_format", [("f32", "real"), ("f64", "real"), ("f32", "u8"), ("f64", "u8")])
@pytest.mark.parametrize("name", ["three_sphere_scene", "reflect_refract"])
def test_aperture_zero_is_render_supersampled(gpu_ctx, rtc, name, precision, out_format):
    cam, depth = _upload(gpu_ctx, name)
    c = rtc.camera_resize(cam, 70, 22)
    for jitter in (False, True):
        lens = rtc.Lens(0.0, FOCUS[name], jitter, 3)
        a, sa = gpu_ctx.render_supersampled(c, 2, depth, precision=precision, out_format=out_format)
        b, sb = gpu_ctx.render_lens(c, 2, lens, depth, precision=precision, out_format=out_format)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes() and _counts(sa) == _counts(sb)
        p, sp = gpu_ctx.render(c, depth, precision=precision, out_format=out_format)
        q, sq = gpu_ctx.render_lens(c, 1, lens, depth, precision=precision, out_format=out_format)
        assert p.tobytes() == q.tobytes() and _counts(sp) == _counts(sq)


# ------------------------------------------------------------------ 3. focal plane identity
@pytest.mark.parametrize("jitter", [False, True])
def test_a_wall_at_the_focal_distance_is_sharp(gpu_ctx, rtc, jitter):
    tables = wall_world()
    lens = rtc.Lens(0.3, 5.0, jitter, 4)
    gpu_ctx.upload(tables)
    a, _ = gpu_ctx.render_lens(tables.camera, 2, lens, 6, precision="f64")
    b, _ = gpu_ctx.render_supersampled(tables.camera, 2, 6, precision="f64")
    err = float(np.abs(a - b).max())
    print(f"wall at focus, jitter {jitter}: max |lens - supersampled| {err:.3g}")
    assert err < ABS64
    ball = wall_world(True)
    gpu_ctx.upload(ball)
    a, _ = gpu_ctx.render_lens(ball.camera, 2, lens, 6, precision="f64")
    b, _ = gpu_ctx.render_supersampled(ball.camera, 2, 6, precision="f64")
    assert float(np.abs(a - b).max()) > 0.1


# ------------------------------------------------------------------ 4. exactness
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", ["three_sphere_scene", "reflect_refract"])
def test_no_skips_and_repeats_are_bit_identical(gpu_ctx, rtc, name, precision, jitter):
    """RT_FLAG_NO_SKIPS turns every cull off: equal bytes say that no cull downstream of the ray generation
    relies on primary rays that share an origin."""
    cam, depth = _upload(gpu_ctx, name)
    c = rtc.camera_resize(cam, 70, 22)
    lens = _lens(rtc, name, jitter)
    a, sa = gpu_ctx.render_lens(c, 3, lens, depth, precision=precision)
    b, sb = gpu_ctx.render_lens(c, 3, lens, depth, precision=precision, flags=RT_FLAG_NO_SKIPS)
    a2, sa2 = gpu_ctx.render_lens(c, 3, lens, depth, precision=precision)
    assert a.tobytes() == b.tobytes() and _counts(sa) == _counts(sb)
    assert a.tobytes() == a2.tobytes() and _counts(sa) == _counts(sa2)


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("name,n", [("three_sphere_scene", 3), ("shadow_puppets", 2), ("reflect_refract", 2)])
def test_per_scene_kernels_are_bit_identical(gpu_ctx, rtc, name, n, jitter):
    """The lens kernels built per scene (RT_JIT_SYNC) against the generic ones, direct and pool."""
    cam, depth = _upload(gpu_ctx, name)
    c = rtc.camera_resize(cam, 70, 22)
    lens = _lens(rtc, name, jitter)
    gpu_ctx.set_jit(0)
    try:
        a, sa = gpu_ctx.render_lens(c, n, lens, depth, precision="f32")
        assert not gpu_ctx.jit_status()["used"]
        gpu_ctx.set_jit(1)
        b, sb = gpu_ctx.render_lens(c, n, lens, depth, precision="f32")
        status = gpu_ctx.jit_status()
        assert status["used"], status["log"][:2000]
        b2, _ = gpu_ctx.render_lens(c, n, lens, depth, precision="f32", flags=RT_FLAG_NO_SKIPS)
    finally:
        gpu_ctx.set_jit(2)
    assert a.tobytes() == b.tobytes() == b2.tobytes() and _counts(sa) == _counts(sb)


@pytest.mark.parametrize("precision,out_format", [("f32", "real"), ("f64", "real"), ("f32", "u8")])
@pytest.mark.parametrize("name", ["three_sphere_scene", "reflect_refract"])
def test_three_shards_assemble_to_the_whole_frame(gpu_ctx, rtc, name, precision, out_format):
    """Hashed jitter: a shard hashes the whole frame's rows."""
    cam, depth = _upload(gpu_ctx, name)
    c = rtc.camera_resize(cam, 70, 22)
    lens = _lens(rtc, name, True)
    whole, st = gpu_ctx.render_lens(c, 2, lens, depth, precision=precision, out_format=out_format)
    shard_of, row_of = rtc.shard_row_map(c.height, 3)
    strips, primary = [], 0
    for s in range(3):
        strip, sst = gpu_ctx.render_lens(c, 2, lens, depth, precision=precision, out_format=out_format, shard=(s, 3))
        strips.append(strip)
        primary += sst["primary"]
    got = np.stack([strips[shard_of[y]][row_of[y]] for y in range(c.height)])
    assert got.tobytes() == whole.tobytes()
    assert primary == st["primary"] == 4 * 70 * 22


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", ["three_sphere_scene", "reflect_refract"])
def test_two_seeds_differ_and_a_seed_repeats(gpu_ctx, rtc, name, precision):
    cam, depth = _upload(gpu_ctx, name)
    c = rtc.camera_resize(cam, 70, 22)
    a, sa = gpu_ctx.render_lens(c, 2, _lens(rtc, name, True, 1), depth, precision=precision)
    b, _ = gpu_ctx.render_lens(c, 2, _lens(rtc, name, True, 2), depth, precision=precision)
    a2, sa2 = gpu_ctx.render_lens(c, 2, _lens(rtc, name, True, 1), depth, precision=precision)
    one, _ = gpu_ctx.render_lens(c, 1, _lens(rtc, name, True, 1), depth, precision=precision)
    assert a.tobytes() != b.tobytes()
    assert a.tobytes() == a2.tobytes() and _counts(sa) == _counts(sa2)
    assert one.tobytes() != gpu_ctx.render(c, depth, precision=precision)[0].tobytes()  # grid 1: a lens point per pixel


# ------------------------------------------------------------------ 5. u8
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("name,w,h,n", U8_CASES)
def test_u8_is_quantized_once_after_the_mean(gpu_ctx, rtc, oracle, name, w, h, n, jitter):
    cam, depth = _upload(gpu_ctx, name)
    lens = rtc.Lens(APERTURE, U8_FOCUS[name], jitter, SEED)
    img, _ = gpu_ctx.render_lens(rtc.camera_resize(cam, w, h), n, lens, depth, precision="f64", out_format="u8")
    ref, _ = oracle_lens_frame(name, w, h, n, APERTURE, U8_FOCUS[name], jitter, SEED)
    exempt = near_boundary(ref, ABS64)
    assert exempt.mean() <= 0.001
    assert img.dtype == np.uint8
    assert np.array_equal(img[~exempt], oracle.quantize(ref)[~exempt])


# ------------------------------------------------------------------ 6. f32 against the oracle
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("name", DIRECT + POOL)
def test_f32_share_within_two_levels_of_the_oracle(gpu_ctx, rtc, oracle, name, jitter):
    import f32_tolerance
    cam, depth = _upload(gpu_ctx, name)
    w, h, n = 320, 200, 2
    img, st = gpu_ctx.render_lens(rtc.camera_resize(cam, w, h), n, _lens(rtc, name, jitter), depth, precision="f32")
    ref, rst = oracle_lens_frame(name, w, h, n, APERTURE, FOCUS[name], jitter, SEED)
    d = np.abs(oracle.quantize(img.astype(np.float64)).astype(int) - oracle.quantize(ref).astype(int)).max(axis=2)
    share = float((d <= 2).mean())
    print(f"{name} jitter {jitter}: {share:.6f} of pixels within 2/255")
    for k in ("primary", "shadow", "reflect", "refract"):
        assert abs(st[k] - rst[k]) <= max(3, f32_tolerance.KIND * rst[k]), (name, k, st[k], rst[k])
    assert st["primary"] == rst["primary"] == n * n * w * h
    observed = f32_tolerance_lens.SHARE_OBSERVED[name, jitter]
    assert share >= observed - 0.005, (share, observed)


# ------------------------------------------------------------------ 7. area build
def test_area_build_matches_the_oracle_on_the_expansion(gpu_ctx, rtc, oracle):
    """An unjittered area light's world through a lens: the area build's lens kernel against the oracle's
    colours of the lens rays in the expansion's world."""
    import area_light_worlds as AW
    import lens_reference as LR
    t = AW.opaque(jitter=False, size=AW.SMALL)
    w, h = AW.SMALL
    n, focal = 2, 7.5
    gpu_ctx.upload(t)
    assert gpu_ctx.light_info()["area_lights"] == 2
    for jitter in (False, True):
        img, st = gpu_ctx.render_lens(t.camera, n, rtc.Lens(APERTURE, focal, jitter, SEED), 3, precision="f64")
        assert gpu_ctx.light_info()["ran_area"] == 1
        cn = rtc.camera_resize(t.camera, n * w, n * h)
        ref, rst = LR.lens_frame(oracle, t.expanded(), cn, w, h, n, APERTURE, focal, jitter, SEED, 3)
        err = float(np.abs(img - ref).max())
        print(f"area build, jitter {jitter}: max |err| {err:.3g}")
        assert err < ABS64 and _counts(st) == _counts(rst)


# ------------------------------------------------------------------ 8. device entry point
@pytest.mark.parametrize("name", ["reflect_refract", "three_sphere_scene"])
def test_device_entry_on_a_side_stream(gpu_ctx, rtc, name):
    """Into torch tensors on a stream of the caller's, no host sync; a host call on the context's stream
    right behind must wait for them (tests/test_gpu_streams.py's rule)."""
    import torch
    cam, depth = _upload(gpu_ctx, name)
    c = rtc.camera_resize(cam, 130, 10)
    lens = _lens(rtc, name, True)
    ref, _ = gpu_ctx.render_lens(c, 4, lens, depth, precision="f32")
    plain, _ = gpu_ctx.render(c, depth, precision="f32")
    side = torch.cuda.Stream()
    outs = [torch.empty((c.height, c.width, 3), dtype=torch.float32, device="cuda") for _ in range(4)]
    for rnd in range(2):
        for o in outs:
            gpu_ctx.render_lens_device(c, 4, lens, o.data_ptr(), side.cuda_stream, depth, "f32")
        img, _ = gpu_ctx.render_lens(c, 4, lens, depth, precision="f32")  # context stream, right away
        assert img.tobytes() == ref.tobytes(), rnd
        again, _ = gpu_ctx.render(c, depth, precision="f32")
        assert again.tobytes() == plain.tobytes(), rnd
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            assert o.cpu().numpy().tobytes() == ref.tobytes(), (rnd, i)


# ------------------------------------------------------------------ 9. pool bound
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_deepest_grid_never_overflows_the_pool(gpu_ctx, rtc, precision):
    """n = 4 at depth 16, hashed: an overflow would raise RT_ERR_POOL."""
    cam, _ = _upload(gpu_ctx, "reflect_refract")
    lens = _lens(rtc, "reflect_refract", True)
    img, st = gpu_ctx.render_lens(rtc.camera_resize(cam, 64, 8), 4, lens, 16, precision=precision)
    ref, rst = oracle_lens_frame("reflect_refract", 64, 8, 4, APERTURE, FOCUS["reflect_refract"], True, SEED, 16)
    if precision == "f64":
        assert float(np.abs(img - ref).max()) < ABS64
        assert _counts(st) == _counts(rst)
    else:
        assert np.isfinite(img).all() and st["primary"] == rst["primary"]


# ------------------------------------------------------------------ 10. refusals
def test_refusals(gpu_ctx, rtc):
    cam, depth = _upload(gpu_ctx, "three_sphere_scene")
    c = rtc.camera_resize(cam, 70, 22)
    lens = rtc.Lens(0.25, 5.0)
    for bad, text in ((None, "null lens"), (rtc.LensDesc(-1.0, 5.0, 0, 0), "aperture"),
                      (rtc.LensDesc(0.25, 0.0, 0, 0), "focal distance"), (rtc.LensDesc(0.25, 5.0, 7, 0), "jitter")):
        with pytest.raises(rtc.RenderError) as e:
            gpu_ctx.render_lens(c, 2, bad, depth)
        assert e.value.code == -1 and text in str(e.value), str(e.value)
        with pytest.raises(rtc.RenderError) as e:
            gpu_ctx.render_lens_device(c, 2, bad, 1, None, depth)
        assert e.value.code == -1 and text in str(e.value), str(e.value)
    for grid in (0, 5):  # ... and what rt_render_supersampled refuses, with its text, at aperture 0 too
        for ln in (lens, rtc.Lens(0.0, 5.0)):
            with pytest.raises(rtc.RenderError) as e:
                gpu_ctx.render_lens(c, grid, ln, depth)
            assert e.value.code == -1 and "outside 1..4" in str(e.value), str(e.value)
    with pytest.raises(rtc.RenderError) as e:
        gpu_ctx.render_lens(c, 2, lens, depth, flags=RT_FLAG_STAMPS)
    assert e.value.code == -1 and "RT_FLAG_NO_SKIPS" in str(e.value)
    with pytest.raises(rtc.RenderError) as e:
        gpu_ctx.render_lens_device(c, 2, lens, 0, None, depth)
    assert e.value.code == -1 and "null" in str(e.value)
    with rtc.Context(0) as fresh:
        with pytest.raises(rtc.RenderError) as e:
            fresh.render_lens(c, 2, lens, depth)
        assert e.value.code == -4  # RT_ERR_NO_SCENE
    if rtc.device_count() >= 2:
        with rtc.Context.multi([0, 1]) as group:
            group.upload(scene_fixture("three_sphere_scene"))
            with pytest.raises(rtc.RenderError) as e:
                group.render_lens(c, 2, lens, depth)
            assert e.value.code == -1 and "group of 2 ranks" in str(e.value)


def test_one_rank_group_is_accepted(rtc):
    scene = scene_fixture("three_sphere_scene")
    c = rtc.camera_resize(scene.camera, 70, 22)
    lens = rtc.Lens(0.25, 5.0, True, 2)
    with rtc.Context(0) as single:
        single.upload(scene)
        want, sw = single.render_lens(c, 2, lens, 6, precision="f32")
    with rtc.Context.multi([0]) as group:
        group.upload(scene)
        got, sg = group.render_lens(c, 2, lens, 6, precision="f32")
    assert got.tobytes() == want.tobytes() and _counts(sg) == _counts(sw)
