"""Moving smooth and textured triangles on the GPU (tests/motion_mesh_worlds.py).

Every moving triangle of tests/test_gpu_motion.py is flat, and a flat triangle never looks at the u and v of
prepare_hit's repeated triangle test nor owns a row of smooth_plain, uv_plain, smooth_inst or uv_inst.  These
worlds do: the barycentrics of a moving smooth or textured triangle must be taken from the displaced origin, and
its row must be found after plan_triangles has put it behind the tree's leaves.

The references are the numpy restatements in the world at each ray's time (motion_reference.trace_at_times):
colours and hit t within 1e-9, the hit shape equal.  A ray whose reference margin is at most 1e-9 sits on a
decision fence and is left out, at most 1 % of them (tests/test_motion_random_cpu.py holds that cap on the
reference alone).  The f32 batches keep their recorded share of the f64 device batches, which the f64 tests have
checked: the project's way for worlds without an oracle.  The shutter frames are tied to the batches through
the ordered mean of the device's own timed rays.
"""
import os

import numpy as np
import pytest

import f32_tolerance_motion
import motion_mesh_worlds as MM
import motion_reference as MR

pytestmark = pytest.mark.gpu

ABS64 = 1e-9  # the project's f64 bar
COUNTERS = ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned", "refract_evals", "schlick_evals")


def _counts(st):
    return {k: st[k] for k in COUNTERS}


def _quantize(a):
    c = np.nan_to_num(np.clip(a, 0.0, 1.0), nan=0.0) * 255.0  # canvas.rs:117-123, as the oracle's quantize
    t = np.trunc(c)
    return (t + (c - t >= 0.5)).astype(int)


@pytest.mark.parametrize("name", MM.NAMES)
def test_moving_mesh_batches_match_the_reference_at_each_time(gpu_ctx, name):
    tables = MM.world(name)
    rays, times = MM.batch(name)
    ref, hit, margin, kept = MM.reference(name)
    assert (~kept).mean() <= MM.MAX_LEFT_OUT
    gpu_ctx.upload(tables)
    cols, t, shape, st = gpu_ctx.trace_rays(rays, MM.DEPTH, precision="f64", hits=True, times=times)
    info = gpu_ctx.motion_info()
    assert info["ran_motion"] == 1 and info["moving_shapes"] + info["moving_instances"] == len(tables.motion)
    err = np.abs(cols - ref).max(axis=1)[kept]
    on_mover = np.isin(hit["shape"], MM.mover_shapes(name)) & kept
    print(f"{name}: {int(kept.sum())} of {len(rays)} rays kept, {int(on_mover.sum())} on movers, max |err| {err.max():.3g}")
    assert err.max() < ABS64, (name, int((err >= ABS64).sum()), err.max())
    assert np.array_equal(shape[kept], hit["shape"][kept]), name
    has = kept & (hit["shape"] >= 0)
    assert np.abs(t[has] - hit["t"][has]).max() <= ABS64 and np.isinf(t[kept & ~has]).all(), name
    assert st["primary"] == len(rays)


def test_the_movers_stand_behind_a_tree_and_own_their_rows(gpu_ctx):
    """(the index case: a tree exists, every mover is outside it, and the smooth and uv tables have a row each)"""
    for name in MM.TOP_LEVEL:
        tables = MM.world(name)
        gpu_ctx.upload(tables)
        tree, info = gpu_ctx.tree_info(), gpu_ctx.motion_info()
        movers = len(tables.motion)
        assert movers == 46 + 46 and tree["nodes"] > 0, (name, tree)
        assert tree["records_outside"] == movers and tree["records_in_tree"] == 320 - movers, (name, tree)
        assert info["moving_shapes"] == movers and info["moving_instances"] == 0
        if "smooth" in name:
            assert gpu_ctx.smooth_info()["smooth_triangles"] == 320, gpu_ctx.smooth_info()
        if "texture" in name:
            assert gpu_ctx.texture_info()["textured_triangles"] == 320, gpu_ctx.texture_info()
    for name in ("smooth_instance", "texture_instance"):
        gpu_ctx.upload(MM.world(name))
        inst, info = gpu_ctx.instance_info(), gpu_ctx.motion_info()
        assert inst["instances"] == 2 and inst["expanded"] == 0 and info["moving_instances"] == 1, (name, inst, info)


def _everything(ctx, rtc, name):
    tables = MM.world(name)
    rays, times = MM.batch(name)
    ctx.upload(tables)
    out = []
    for precision in ("f32", "f64"):
        cols, t, shape, st = ctx.trace_rays(rays, MM.DEPTH, precision=precision, hits=True, times=times)
        img, fst = ctx.render_shutter(rtc.camera_resize(tables.camera, 70, 22), 2, rtc.Shutter(0.0, 1.0), None, MM.DEPTH,
                                      precision=precision)
        out += [cols, t, shape, _counts(st), img, _counts(fst)]
    return out


def test_the_tree_changes_no_bit_of_the_top_level_worlds(gpu_ctx, rtc):
    """RTC_DEBUG=tri_tree=0 (every triangle in the flat run, the movers where the upload found them): the same
    batches and frames bit for bit, f32 and f64, counters included."""
    plain = {name: _everything(gpu_ctx, rtc, name) for name in MM.TOP_LEVEL}
    before = os.environ.get("RTC_DEBUG")
    os.environ["RTC_DEBUG"] = "tri_tree=0" if not before else before + ",tri_tree=0"
    try:
        with rtc.Context(0) as ctx:  # (the knobs are read when a context is created)
            for name in MM.TOP_LEVEL:
                flat = _everything(ctx, rtc, name)
                assert ctx.tree_info()["nodes"] == 0
                assert len(flat) == len(plain[name]) and all(
                    np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(plain[name], flat)), name
    finally:
        if before is None:
            del os.environ["RTC_DEBUG"]
        else:
            os.environ["RTC_DEBUG"] = before


@pytest.mark.parametrize("name", MM.NAMES)
def test_moving_mesh_frames_are_the_mean_of_timed_rays(gpu_ctx, rtc, name):
    """70 x 22, n = 2, the cell centres: the shutter frame against rt_trace_rays_timed over the frame's own rays
    and times, which ties the frame kernels to the batches checked above."""
    w, h, n, sh = 70, 22, 2, (0.0, 1.0, False, 0)
    tables = MM.world(name)
    cam = rtc.camera_resize(tables.camera, w, h)
    gpu_ctx.upload(tables)
    img, st = gpu_ctx.render_shutter(cam, n, rtc.Shutter(*sh), None, MM.DEPTH, precision="f64")
    rays = MR.sample_rays(rtc.camera_resize(cam, n * w, n * h), w, h, n).reshape(-1, 6)
    times = MR.shutter_times(w, h, n, *sh).reshape(-1)
    cols, rst = gpu_ctx.trace_rays(np.ascontiguousarray(rays), MM.DEPTH, precision="f64", times=times)
    err = float(np.abs(img - MR.ordered_mean(cols, h, w, n)).max())
    print(f"{name}: frame against its timed rays, max |err| {err:.3g}, hits {st['shaded']}")
    assert err < ABS64 and _counts(st) == _counts(rst) and st["primary"] == n * n * w * h and st["shaded"] > 500


@pytest.mark.parametrize("name", MM.NAMES)
def test_f32_moving_mesh_batches_keep_their_share_of_the_f64_batches(gpu_ctx, name):
    rays, times = MM.batch(name)
    gpu_ctx.upload(MM.world(name))
    want, _ = gpu_ctx.trace_rays(rays, MM.DEPTH, precision="f64", times=times)
    got, _ = gpu_ctx.trace_rays(rays, MM.DEPTH, precision="f32", times=times)
    share = float((np.abs(_quantize(got) - _quantize(want)).max(axis=1) <= 2).mean())
    twin = f32_tolerance_motion.STATIC_TWINS[name]
    print(f"F32 mesh_batch {name} {share:.6f} (static twin {twin[0]}: {twin[1]:.6f})")
    assert share >= f32_tolerance_motion.SHARE_OBSERVED[("mesh_batch", name)] - 0.005, (name, share)
