"""Motion blur (rt_scene_upload_moving, rt_render_shutter*, rt_trace_rays_timed*) on the GPU.

The reference has no motion: a ray of time tau in a moving world is that ray in the static world whose movers
are displaced by v tau (SceneTables.at_time, rt_motion_displace), which the f64 oracle renders.  That is the
reference of the f64 kernels (1e-9, counters equal) and of the f32 kernels' shares; tests/motion_reference.py
restates the shutter's times in numpy and groups rays by time for the oracle.  The worlds are
tests/motion_worlds.py's, each built to break one consumer of a mover's static position.  Frames are ragged
against the 64 x 4 tile: 70 x 22 and 96 x 26, grids 2 and 3 (n^2 = 9: the cell rotation is no power of two).

The primary hit of a timed ray (shape and t) is checked against the device's own static path in the world at
that time (a static upload of at_time(tau), which tests/test_gpu_trace_rays.py checks against the device's
intersection tests): the oracle's interface gives colours and counters only.
"""
import os

import numpy as np
import pytest

import f32_tolerance_motion
import motion_reference as MR
import motion_worlds as MW

pytestmark = pytest.mark.gpu

ABS64 = 1e-9  # the project's f64 bar
COUNTERS = ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned", "refract_evals", "schlick_evals")
NAMES = tuple(MW.WORLDS)
DIRECT = tuple(n for n in NAMES if n not in MW.POOL)
SHUTTER = (0.0, 1.0, False, 0)
LENS = (0.05, 5.0, False, 0)  # aperture, focal distance (the camera's distance to what it looks at)
RT_FLAG_NO_SKIPS = 64


def _counts(st):
    return {k: st[k] for k in COUNTERS}


def _cam(rtc, w=70, h=22):
    return rtc.camera_resize(MW.camera(), w, h)


def _shutter(rtc, sh=SHUTTER):
    return rtc.Shutter(*sh)


def _lens(rtc, lens):
    return None if lens is None else rtc.Lens(*lens)


_REF = {}


def _batch_ref(oracle, name):
    """(colours, counters) of the oracle over the world's timed batch, computed once."""
    if name not in _REF:
        rays, times = MW.batch(name)
        cols, st = MR.trace(oracle, MW.oracle_scene(name), rays, times, MW.depth(name))
        assert np.isfinite(cols).all()  # no ray is left out: the oracle itself gives every one a finite colour
        _REF[name] = (cols, st)
    return _REF[name]


_FRAME = {}


def _frame_ref(oracle, rtc, name, w, h, n, sh, lens):
    key = (name, w, h, n, sh, lens)
    if key not in _FRAME:
        _FRAME[key] = MR.frame(oracle, MW.oracle_scene(name), MW.camera(), rtc, w, h, n, sh, MW.depth(name), lens)
    return _FRAME[key]


# ------------------------------------------------------------------ 1. timed ray batches, f64
@pytest.mark.parametrize("name", NAMES)
def test_timed_batches_match_the_oracle_in_the_world_at_each_time(gpu_ctx, oracle, name):
    scene, _ = MW.world(name)
    rays, times = MW.batch(name)
    depth = MW.depth(name)
    ref, rst = _batch_ref(oracle, name)
    gpu_ctx.upload(scene)
    cols, t, shape, st = gpu_ctx.trace_rays(rays, depth, precision="f64", hits=True, times=times)
    info = gpu_ctx.motion_info()
    err = np.abs(cols - ref).max(axis=1)
    print(f"{name}: {len(rays)} rays, max |err| {err.max():.3g}, moved {np.abs(cols - _static(oracle, name)).max():.3g}")
    assert err.max() < ABS64, (int((err >= ABS64).sum()), err.max())
    assert _counts(st) == _counts(rst) and st["primary"] == len(rays)
    assert info["ran_motion"] == 1 and info["moving_shapes"] + info["moving_instances"] == len(scene.motion)
    # the primary hits: the device's static path in the world at each time
    for tau in np.unique(times):
        at = times == tau
        gpu_ctx.upload(scene.at_time(float(tau)))
        _, t0, shape0, _ = gpu_ctx.trace_rays(rays[at], depth, precision="f64", hits=True)
        assert gpu_ctx.motion_info()["ran_motion"] == 0
        assert np.array_equal(shape[at], shape0), tau
        hit = shape0 >= 0
        assert np.all(np.abs(t[at][hit] - t0[hit]) <= ABS64) and np.isinf(t[at][~hit]).all(), tau


def _static(oracle, name):
    rays, _ = MW.batch(name)
    return oracle.color_at(MW.oracle_scene(name).at_time(0.0).expanded(), rays, MW.depth(name))[0]


def test_the_batches_see_the_motion(oracle):
    """(the effect is there: in every world a good share of the rays differ from the static world's)"""
    for name in NAMES:
        share = float((np.abs(_batch_ref(oracle, name)[0] - _static(oracle, name)).max(axis=1) > 1e-6).mean())
        assert share > 0.05, (name, share)


def test_the_tree_world_has_a_tree_and_an_expanded_moving_instance(gpu_ctx):
    """(the host paths the world is there for: the mover outside an existing tree, velocities on expanded records)"""
    scene = MW.world("tree")[0]
    gpu_ctx.upload(scene)
    tree, inst, info = gpu_ctx.tree_info(), gpu_ctx.instance_info(), gpu_ctx.motion_info()
    print(tree, inst, info)
    assert tree["nodes"] > 0 and inst["instances"] == 2 and inst["expanded"] == 2
    # the 72 static triangles and the static twin's 8 are in the tree; the moving triangle and the moving twin's 8 are not
    assert tree["records_in_tree"] == 72 + 8 and tree["records_outside"] == 1 + 8
    assert info["moving_shapes"] == 1 and info["moving_instances"] == 1


# ------------------------------------------------------------------ 2. shutter frames, f64, cell centres
FRAMES = [(name, 70, 22, 2) for name in NAMES] + [("far_sphere", 96, 26, 3), ("glass", 96, 26, 3), ("far_instance", 96, 26, 3)]


@pytest.mark.parametrize("lens", [None, LENS], ids=["pinhole", "lens"])
@pytest.mark.parametrize("name,w,h,n", FRAMES)
def test_f64_shutter_frames_match_the_oracle_mean(gpu_ctx, rtc, oracle, name, w, h, n, lens):
    gpu_ctx.upload(MW.world(name)[0])
    img, st = gpu_ctx.render_shutter(_cam(rtc, w, h), n, _shutter(rtc), _lens(rtc, lens), MW.depth(name), precision="f64")
    ref, rst = _frame_ref(oracle, rtc, name, w, h, n, SHUTTER, lens)
    err = float(np.abs(img - ref).max())
    print(f"{name} {w}x{h} n={n} lens {lens is not None}: max |err| {err:.3g}")
    assert img.shape == (h, w, 3) and err < ABS64, err
    assert _counts(st) == _counts(rst) and st["primary"] == n * n * w * h
    assert gpu_ctx.motion_info()["ran_motion"] == 1


# ------------------------------------------------------------------ 3. hashed shutter
@pytest.mark.parametrize("name", ["far_sphere", "glass"])
def test_hashed_frames_match_the_oracle_with_one_world_per_time(gpu_ctx, rtc, oracle, name):
    sh = (0.0, 1.0, True, 5)
    gpu_ctx.upload(MW.world(name)[0])
    img, st = gpu_ctx.render_shutter(_cam(rtc, 16, 10), 2, _shutter(rtc, sh), None, MW.depth(name), precision="f64")
    ref, rst = _frame_ref(oracle, rtc, name, 16, 10, 2, sh, None)
    times = MR.shutter_times(16, 10, 2, *sh)
    assert len(np.unique(times)) == times.size  # one world per ray
    assert float(np.abs(img - ref).max()) < ABS64 and _counts(st) == _counts(rst)


@pytest.mark.parametrize("lens", [None, (0.05, 5.0, True, 3)], ids=["pinhole", "lens"])
@pytest.mark.parametrize("name", ["far_sphere", "far_instance", "glass", "pattern"])
def test_hashed_frames_are_the_mean_of_timed_rays(gpu_ctx, rtc, name, lens):
    """70 x 22, n = 3: the frame against rt_trace_rays_timed over the reference's own rays and times."""
    w, h, n, sh = 70, 22, 3, (0.25, 1.0, True, 9)
    cam = _cam(rtc, w, h)
    gpu_ctx.upload(MW.world(name)[0])
    img, st = gpu_ctx.render_shutter(cam, n, _shutter(rtc, sh), _lens(rtc, lens), MW.depth(name), precision="f64")
    rays = MR.sample_rays(rtc.camera_resize(cam, n * w, n * h), w, h, n, lens).reshape(-1, 6)
    times = MR.shutter_times(w, h, n, *sh).reshape(-1)
    cols, rst = gpu_ctx.trace_rays(np.ascontiguousarray(rays), MW.depth(name), precision="f64", times=times)
    assert float(np.abs(img - MR.ordered_mean(cols, h, w, n)).max()) < ABS64
    assert _counts(st) == _counts(rst)


def test_seeds_differ_and_a_seed_repeats(gpu_ctx, rtc):
    gpu_ctx.upload(MW.world("far_sphere")[0])
    cam = _cam(rtc)
    for precision in ("f32", "f64"):
        a, _ = gpu_ctx.render_shutter(cam, 2, rtc.Shutter(0.0, 1.0, True, 1), None, 2, precision=precision)
        b, _ = gpu_ctx.render_shutter(cam, 2, rtc.Shutter(0.0, 1.0, True, 2), None, 2, precision=precision)
        c, _ = gpu_ctx.render_shutter(cam, 2, rtc.Shutter(0.0, 1.0, True, 1), None, 2, precision=precision)
        assert np.array_equal(a, c) and not np.array_equal(a, b)


# ------------------------------------------------------------------ 4. the frame depends on time
def test_the_frame_depends_on_time(gpu_ctx, rtc):
    """The far mover is in the frame for the last third of the shutter only: a closed shutter at 0 and the
    tau = 0 rule of the older entry points do not show it, the full shutter does, where it is at the end."""
    gpu_ctx.upload(MW.world("far_sphere")[0])
    cam = _cam(rtc)
    full, _ = gpu_ctx.render_shutter(cam, 2, rtc.Shutter(0.0, 1.0), None, 2, precision="f64")
    closed, _ = gpu_ctx.render_shutter(cam, 2, rtc.Shutter(0.0, 0.0), None, 2, precision="f64")
    still, _ = gpu_ctx.render_supersampled(cam, 2, 2, precision="f64")
    assert np.array_equal(closed, still)  # every sample at tau = 0 is the static frame
    assert (np.abs(full - closed).max(axis=2) > 1e-3).any()
    # where the mover is at tau = 0.875, the last of the full shutter's four sample times (a shutter closed there
    # shows its red; the static frame has no such pixel) ...
    late, _ = gpu_ctx.render_shutter(cam, 2, rtc.Shutter(0.875, 0.875), None, 2, precision="f64")
    red = lambda img: (img[..., 0] > 0.3) & (img[..., 0] > 2.0 * img[..., 2])  # noqa: E731
    assert red(late).sum() >= 4 and not red(still).any()
    # ... the full shutter has a quarter of it, and the older entry point none
    assert (np.abs(full - still).max(axis=2)[red(late)] > 1e-3).all()


# ------------------------------------------------------------------ 5. acceleration only
def _everything(ctx, rtc, name, flags=0):
    """Frames (pinhole and lens), timed batches and their counters, f32 and f64, of one world."""
    out = []
    ctx.upload(MW.world(name)[0])
    rays, times = MW.batch(name, 512)
    for precision in ("f32", "f64"):
        for lens in (None, LENS):
            img, st = ctx.render_shutter(_cam(rtc), 2, _shutter(rtc), _lens(rtc, lens), MW.depth(name), precision=precision, flags=flags)
            out += [img, _counts(st)]
        cols, t, shape, st = ctx.trace_rays(rays, MW.depth(name), precision=precision, hits=True, times=times, flags=flags)
        out += [cols, t, shape, _counts(st)]
    return out


def _same(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b)) and len(a) == len(b)


@pytest.fixture(scope="module")
def plain_results(gpu_ctx, rtc):
    return {name: _everything(gpu_ctx, rtc, name) for name in NAMES}


def test_no_skips_changes_nothing(gpu_ctx, rtc, plain_results):
    for name in NAMES:
        assert _same(plain_results[name], _everything(gpu_ctx, rtc, name, RT_FLAG_NO_SKIPS)), name


@pytest.mark.parametrize("knob", ["cull=0", "tri_tree=0", "area_cull=0", "lds_world=0"])
def test_debug_knobs_change_nothing(rtc, plain_results, knob):
    before = os.environ.get("RTC_DEBUG")
    os.environ["RTC_DEBUG"] = knob if not before else before + "," + knob
    try:
        with rtc.Context(0) as ctx:  # (the knobs are read when a context is created)
            for name in NAMES:
                assert _same(plain_results[name], _everything(ctx, rtc, name)), (knob, name)
    finally:
        if before is None:
            del os.environ["RTC_DEBUG"]
        else:
            os.environ["RTC_DEBUG"] = before


# ------------------------------------------------------------------ 6. degenerate forms
@pytest.mark.parametrize("precision,out_format", [("f32", "real"), ("f64", "real"), ("f32", "u8"), ("f64", "u8")])
@pytest.mark.parametrize("name", ["far_sphere", "glass"])
def test_a_world_without_movers_is_the_lens_frame(gpu_ctx, rtc, name, precision, out_format):
    still = MW.world(name)[0].at_time(0.0)  # (the same tables without a motion list)
    assert not still.moving
    gpu_ctx.upload(still)
    cam, d = _cam(rtc), MW.depth(name)
    a, sa = gpu_ctx.render_shutter(cam, 2, rtc.Shutter(0.0, 1.0, True, 4), rtc.Lens(*LENS), d, precision=precision, out_format=out_format)
    b, sb = gpu_ctx.render_lens(cam, 2, rtc.Lens(*LENS), d, precision=precision, out_format=out_format)
    assert np.array_equal(a, b) and _counts(sa) == _counts(sb)
    a, sa = gpu_ctx.render_shutter(cam, 2, rtc.Shutter(0.0, 1.0, True, 4), None, d, precision=precision, out_format=out_format)
    b, sb = gpu_ctx.render_supersampled(cam, 2, d, precision=precision, out_format=out_format)
    assert np.array_equal(a, b) and _counts(sa) == _counts(sb)
    assert gpu_ctx.motion_info() == {"moving_shapes": 0, "moving_instances": 0, "ran_motion": 0, "motion_bytes": 0}


@pytest.mark.parametrize("name", ["far_sphere", "far_instance", "glass_single", "pattern", "area"])
def test_older_entry_points_see_the_world_at_time_zero(gpu_ctx, rtc, name):
    """(glass_single: glass()'s twins are two classes in the moving world and one in its static world at 0)"""
    scene = MW.world(name)[0]
    cam, d = _cam(rtc), MW.depth(name)
    rays, _ = MW.batch(name, 512)

    def older(ctx):
        out = [ctx.render(cam, d, precision="f64"), ctx.render_supersampled(cam, 2, d, precision="f64"),
               ctx.render_lens(cam, 2, rtc.Lens(*LENS), d, precision="f64"), ctx.trace_rays(rays, d, precision="f64"),
               ctx.color_at(rays, d, precision="f64")]
        return out, ctx.motion_info()["ran_motion"]
    gpu_ctx.upload(scene)
    assert gpu_ctx.motion_info()["moving_shapes"] + gpu_ctx.motion_info()["moving_instances"] == len(scene.motion)
    moving, ran = older(gpu_ctx)
    assert ran == 0
    gpu_ctx.upload(scene.at_time(0.0))
    static, _ = older(gpu_ctx)
    for (a, sa), (b, sb) in zip(moving, static):
        assert float(np.abs(a - b).max()) < ABS64 and _counts(sa) == _counts(sb)


def test_zero_velocities_are_dropped_at_upload(gpu_ctx, rtc):
    """A list of zero velocities (+0 or -0) is no motion: the world is the static one, its build included."""
    scene = MW.world("far_sphere")[0].at_time(0.0)
    cam = _cam(rtc)
    gpu_ctx.upload(scene)
    want, wst = gpu_ctx.render_supersampled(cam, 2, 2, precision="f32")
    zero = (rtc.MotionDesc * 2)()
    zero[0].target, zero[0].index = rtc.RT_MOVE_SHAPE, 1
    zero[1].target, zero[1].index = rtc.RT_MOVE_SHAPE, 2
    zero[1].velocity[:] = [0.0, -0.0, 0.0]
    scene.motion = zero
    gpu_ctx.upload(scene)
    assert gpu_ctx.motion_info() == {"moving_shapes": 0, "moving_instances": 0, "ran_motion": 0, "motion_bytes": 0}
    got, gst = gpu_ctx.render_shutter(cam, 2, rtc.Shutter(0.0, 1.0), None, 2, precision="f32")
    assert np.array_equal(got, want) and _counts(gst) == _counts(wst) and gpu_ctx.motion_info()["ran_motion"] == 0
    scene.motion = None


def test_per_scene_builds_are_refused_with_their_reason(gpu_ctx, rtc):
    gpu_ctx.upload(MW.world("far_sphere")[0])
    gpu_ctx.set_jit(1)
    try:
        gpu_ctx.render(rtc.camera_resize(MW.camera(), 320, 200), 2, precision="f32")
        status = gpu_ctx.jit_status()
    finally:
        gpu_ctx.set_jit(2)
    assert not status["used"] and "moving shapes" in status["log"]


# ------------------------------------------------------------------ 7. plumbing
def test_three_shards_assemble_to_the_whole_frame(gpu_ctx, rtc):
    gpu_ctx.upload(MW.world("glass")[0])
    cam, sh = _cam(rtc), rtc.Shutter(0.0, 1.0, True, 6)
    for precision in ("f32", "f64"):
        whole, _ = gpu_ctx.render_shutter(cam, 2, sh, rtc.Lens(*LENS), 5, precision=precision)
        shard_of, row_of = rtc.shard_row_map(cam.height, 3)
        for s in range(3):
            strip, _ = gpu_ctx.render_shutter(cam, 2, sh, rtc.Lens(*LENS), 5, precision=precision, shard=(s, 3))
            rows = np.nonzero(shard_of == s)[0]
            assert np.array_equal(strip[row_of[rows]], whole[rows]), (precision, s)


def test_the_device_entry_runs_on_a_side_stream(gpu_ctx, rtc):
    import torch
    gpu_ctx.upload(MW.world("far_cube")[0])
    cam, sh = _cam(rtc), rtc.Shutter(0.0, 1.0)
    ref, _ = gpu_ctx.render_shutter(cam, 2, sh, None, 2, precision="f32")
    dev = torch.device("cuda", gpu_ctx.device)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        out = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device=dev)
        gpu_ctx.render_shutter_device(cam, 2, sh, out.data_ptr(), None, side.cuda_stream, 2, precision="f32")
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)


def test_u8_is_quantized_once_after_the_mean(gpu_ctx, rtc, oracle):
    gpu_ctx.upload(MW.world("far_sphere")[0])
    cam = _cam(rtc)
    real, _ = gpu_ctx.render_shutter(cam, 2, _shutter(rtc), None, 2, precision="f64")
    u8, _ = gpu_ctx.render_shutter(cam, 2, _shutter(rtc), None, 2, precision="f64", out_format="u8")
    assert u8.dtype == np.uint8 and np.array_equal(u8, oracle.quantize(real))


def test_the_deepest_grid_raises_no_pool_overflow(gpu_ctx, rtc):
    gpu_ctx.upload(MW.world("glass")[0])
    for precision in ("f32", "f64"):
        img, st = gpu_ctx.render_shutter(_cam(rtc), 4, rtc.Shutter(0.0, 1.0, True, 2), rtc.Lens(*LENS), 16, precision=precision)
        assert np.isfinite(img).all() and st["primary"] == 16 * 70 * 22


def test_a_one_rank_group_is_accepted_and_more_ranks_are_refused(rtc):
    with rtc.Context.multi([0]) as ctx:
        ctx.upload(MW.world("far_sphere")[0])
        img, _ = ctx.render_shutter(_cam(rtc), 2, _shutter(rtc), None, 2, precision="f32")
        assert img.shape == (22, 70, 3) and ctx.motion_info()["moving_shapes"] == 1
    if rtc.device_count() >= 2:
        with rtc.Context.multi([0, 1]) as ctx:
            with pytest.raises(rtc.RenderError, match="group of 2 ranks"):
                ctx.upload(MW.world("far_sphere")[0])
            ctx.upload(MW.world("far_sphere")[0].at_time(0.0))
            with pytest.raises(rtc.RenderError, match="not split across a group"):
                ctx.render_shutter(_cam(rtc), 2, _shutter(rtc), None, 2, precision="f32")


# ------------------------------------------------------------------ 8. f32
def f32_share(img, ref, oracle):
    q = lambda a: oracle.quantize(a).astype(int)  # noqa: E731
    return float((np.abs(q(img) - q(ref)).reshape(-1, 3).max(axis=1) <= 2).mean())


@pytest.mark.parametrize("name", NAMES)
def test_f32_batches_keep_their_share_of_the_oracle(gpu_ctx, oracle, name):
    rays, times = MW.batch(name)
    gpu_ctx.upload(MW.world(name)[0])
    cols, _ = gpu_ctx.trace_rays(rays, MW.depth(name), precision="f32", times=times)
    share = f32_share(cols, _batch_ref(oracle, name)[0], oracle)
    print(f"{name}: f32 batch share within 2/255 {share:.6f}")
    assert share >= f32_tolerance_motion.SHARE_OBSERVED[("batch", name)] - 0.005


@pytest.mark.parametrize("lens", [None, LENS], ids=["pinhole", "lens"])
@pytest.mark.parametrize("name", NAMES)
def test_f32_frames_keep_their_share_of_the_oracle(gpu_ctx, rtc, oracle, name, lens):
    gpu_ctx.upload(MW.world(name)[0])
    img, _ = gpu_ctx.render_shutter(_cam(rtc), 2, _shutter(rtc), _lens(rtc, lens), MW.depth(name), precision="f32")
    share = f32_share(img, _frame_ref(oracle, rtc, name, 70, 22, 2, SHUTTER, lens)[0], oracle)
    print(f"{name} lens {lens is not None}: f32 frame share within 2/255 {share:.6f}")
    assert share >= f32_tolerance_motion.SHARE_OBSERVED[("frame", name, lens is not None)] - 0.005
