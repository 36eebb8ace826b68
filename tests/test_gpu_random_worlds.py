"""Seeded random worlds: the HIP path against the f64 oracle beyond the
reference's scenes.

The reference scenes hold no cone or triangle, no sheared or rotated
cylinder, no value-identical pair of shapes and no light count above two.
Each seed here draws a world with every shape kind (world.rs:25-35 with
shapes/*.rs), random transforms with rotation, non-uniform scale and shear
(shape.rs:22-27), random Phong materials with reflection, refraction and
Schlick mixing (world.rs:38-67, 114-157), every pattern kind but the test
pattern (pattern.rs), shapes that cast no shadow (world.rs:108-111),
sometimes a value-identical copy of a shape (intersection.rs:47), one to
three lights, and a depth of 0 to 6.  A small frame of it is rendered in
f64 (every pixel within 1e-9 of the oracle, every ray counter equal) and in
f32 (pixels within 2/255 after canvas.rs:117-123's quantization, a floor set
from the observed agreement of these seeds with a margin).
"""
import numpy as np
import pytest

from random_worlds import many_shapes_world as _many_shapes_world
from random_worlds import random_world as _random_world

pytestmark = pytest.mark.gpu

ABS64 = 1e-9
F32_PIX_FRAC = 0.99  # observed minimum over the 48 seeds: 0.9958 (round 6)
SEEDS = list(range(48))


def rtc_amd_error():
    import rtc_amd
    return rtc_amd.RenderError


def depth_has_pool(tables):
    """Some material reflective or transparent (the pool kernel's worlds)."""
    return any(m.reflectiveness != 0 or m.transparency != 0 for m in tables.materials)


def _counts(st):
    return {k: st[k] for k in ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned",
                               "refract_evals", "schlick_evals")}


@pytest.mark.parametrize("seed", SEEDS + [f"{s}x4" for s in range(8)])
def test_random_world_parity(gpu_ctx, oracle, seed):
    """Seeds "<s>x4": the same world with lights four times as bright."""
    if isinstance(seed, str):
        tables, cam, depth = _random_world(int(seed[:-2]), light_scale=4.0)
    else:
        tables, cam, depth = _random_world(seed)
    gpu_ctx.upload(tables)
    ref, rst = oracle.render(tables, cam, depth, threads=8)
    img, st = gpu_ctx.render(cam, depth, precision="f64")
    err = float(np.abs(img - ref).max())
    assert err < ABS64, f"seed {seed}: f64 max |err| {err:.3g}"
    assert _counts(st) == _counts(rst), f"seed {seed}"
    img32, _ = gpu_ctx.render(cam, depth, precision="f32")
    d = np.abs(oracle.quantize(img32).astype(int) - oracle.quantize(ref).astype(int)).max(axis=2)
    agree = float((d <= 2).mean())
    # the next frames are cost-ordered (heavy tiles split, raised priority): the same pixels
    for precision, first in (("f32", img32), ("f64", img)):
        again, _ = gpu_ctx.render(cam, depth, precision=precision)
        assert np.array_equal(again, first), f"seed {seed}: warm {precision} frame differs"
    print(f"seed {seed} depth {depth} shapes {len(tables.shapes)}: f64 {err:.2e}, f32 within 2/255 {agree:.4f}")
    assert agree >= F32_PIX_FRAC, f"seed {seed}: f32 {agree:.4f}"


PER_SCENE_USED = {}  # (seed, plain) -> the per-scene build was accepted and ran (filled by the test below)
PER_SCENE_CASES = 32
PER_SCENE_MIN_USED = 16  # round 6 recorded 21 of 32


@pytest.mark.parametrize("plain", [False, True], ids=["pool", "direct"])
@pytest.mark.parametrize("seed", list(range(16)))
def test_random_world_per_scene_kernel_equals_generic(rtc, seed, plain):
    """The per-scene (hipRTC) kernels the bench runs, built for each random
    world (constant shape records, clusters, world-space spheres and cubes,
    the acceleration skips), against the generic f32 kernel: the same
    frame bit for bit and the same counters.  (21 of these 32 builds were
    accepted in round 6; the others were refused for scratch.)"""
    tables, cam, depth = _random_world(seed, plain=plain, allow_dup=False)
    with rtc.Context(0) as gen, rtc.Context(0) as jit:
        gen.set_jit(rtc.RT_JIT_OFF)
        jit.set_jit(rtc.RT_JIT_SYNC)
        gen.upload(tables)
        jit.upload(tables)
        a, sa = gen.render(cam, depth, precision="f32")
        b, sb = jit.render(cam, depth, precision="f32")
        js = jit.jit_status()
        PER_SCENE_USED[(seed, plain)] = js["used"]
        if not js["used"]:
            # a build that spills or loses occupancy is refused (rtc_jit.cpp
            # jit_variant), with its reason in the log, and the frame falls
            # back to the generic kernel (checked below like an accepted one)
            assert "not used" in js["log"] and ("scratch" in js["log"] or "workgroups/CU" in js["log"]), js
        assert np.array_equal(a, b), f"seed {seed}: {int((a != b).any(axis=2).sum())} pixels differ"
        assert _counts(sa) == _counts(sb)


def test_random_world_per_scene_kernels_were_used():
    """The comparison above also passes when a build is refused and the frame
    falls back to the generic kernel.  Were every build refused it would
    compare the generic kernel with itself: at least half of the 32 builds
    must have been accepted and run (a condition against that vacuous pass,
    not a target).  Needs all 32 cases of the test above in this session."""
    if len(PER_SCENE_USED) < PER_SCENE_CASES:
        pytest.skip(f"only {len(PER_SCENE_USED)} of the {PER_SCENE_CASES} per-scene cases ran in this session")
    used = sum(PER_SCENE_USED.values())
    print(f"per-scene builds used: {used} of {PER_SCENE_CASES}")
    assert used >= PER_SCENE_MIN_USED, sorted(k for k, v in PER_SCENE_USED.items() if not v)


@pytest.mark.parametrize("seed", list(range(16)))
def test_random_world_color_at_random_rays(gpu_ctx, oracle, seed):
    """World::color_at (world.rs:89-93) on 2048 random rays per random world:
    origins anywhere in the scene's box, inside shapes included (the
    containers walk then starts with entries at t < 0), unit directions.
    f64 within 1e-9 of the oracle's color_at, counters equal.  (Non-unit
    directions are refused in worlds with secondary rays, rtc.h rt_color_at:
    the specular term grows as |d|^shininess past the pool's fixed-point
    range.)"""
    tables, _, _ = _random_world(seed)
    rng = np.random.default_rng(1000 + seed)
    n = 2048
    o = rng.uniform([-4, -1.5, -6], [4, 4, 4], size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], axis=1)
    gpu_ctx.upload(tables)
    if depth_has_pool(tables):
        bad = rays.copy()
        bad[7, 3:] *= 1.5
        with pytest.raises(rtc_amd_error(), match="unit length"):
            gpu_ctx.color_at(bad, 6, precision="f64")
    got, st = gpu_ctx.color_at(rays, 6, precision="f64")
    ref, rst = oracle.color_at(tables, rays, 6)
    err = float(np.abs(got - ref).max())
    assert err < ABS64, f"seed {seed}: max |err| {err:.3g} at ray {int(np.abs(got - ref).max(axis=1).argmax())}"
    assert _counts(st) == _counts(rst), f"seed {seed}"


@pytest.mark.parametrize("n", [300, 1500])
def test_many_shapes_world(gpu_ctx, oracle, rtc, n):
    """Hundreds to thousands of shapes: f64 within 1e-9 of the oracle with
    equal counters, f32 within 2/255, and the per-scene kernels (clusters,
    or the generic tables past 255 shapes) bit-equal to the generic one."""
    tables, cam = _many_shapes_world(n, n)
    gpu_ctx.upload(tables)
    ref, rst = oracle.render(tables, cam, 4, threads=8)
    img, st = gpu_ctx.render(cam, 4, precision="f64")
    assert float(np.abs(img - ref).max()) < ABS64
    assert _counts(st) == _counts(rst)
    img32, s32 = gpu_ctx.render(cam, 4, precision="f32")
    d = np.abs(oracle.quantize(img32).astype(int) - oracle.quantize(ref).astype(int)).max(axis=2)
    assert float((d <= 2).mean()) >= F32_PIX_FRAC
    with rtc.Context(0) as jit:
        jit.set_jit(rtc.RT_JIT_SYNC)
        jit.upload(tables)
        b, sb = jit.render(cam, 4, precision="f32")
        assert np.array_equal(img32, b) and _counts(s32) == _counts(sb), jit.jit_status()


@pytest.mark.parametrize("seed", list(range(24)))
def test_random_world_accelerations_are_exact(gpu_ctx, rtc, monkeypatch, seed):
    """The wave cull and the shadow/exit skips are acceleration only: on every
    random world the f32 and f64 frames with the cull off (RTC_DEBUG=cull=0,
    every shape unbounded) and with RT_FLAG_NO_SKIPS equal the default frame
    bit for bit, counters included.  (An f32 decision flipped on one pixel
    would pass the oracle's 2/255 floor; this catches it.)"""
    tables, cam, depth = _random_world(seed)
    gpu_ctx.upload(tables)
    monkeypatch.setenv("RTC_DEBUG", "cull=0")
    with rtc.Context(0) as nocull:
        nocull.upload(tables)
        for precision in ("f32", "f64"):
            a, sa = gpu_ctx.render(cam, depth, precision=precision)
            b, sb = nocull.render(cam, depth, precision=precision)
            c, sc = gpu_ctx.render(cam, depth, precision=precision, flags=rtc.RT_FLAG_NO_SKIPS)
            assert np.array_equal(a, b), f"seed {seed} {precision}: the cull changed {int((a != b).any(axis=2).sum())} px"
            assert np.array_equal(a, c), f"seed {seed} {precision}: the skips changed {int((a != c).any(axis=2).sum())} px"
            assert _counts(sa) == _counts(sb) == _counts(sc)
