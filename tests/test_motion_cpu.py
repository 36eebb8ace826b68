"""The host side of motion blur (include/rtc.h "Motion blur"), without a GPU.

  - every refusal of rt_scene_upload_moving, rt_render_shutter*, rt_shutter_time and rt_motion_displace and
    its text (the lists are checked before the context is looked at, so a null context reaches them);
  - rt_shutter_time against the numpy restatement (tests/motion_reference.py) for both jitter modes, over
    every (x, y, i, j) of a 7 x 5 frame, n = 1..4, bit for bit;
  - rt_motion_displace against numpy (inverse * translation(-v tau) as matrix.rs multiplies), a zero
    velocity and at_time(0) equal to the input bit for bit;
  - World.tables() emits the motion list; scene_io and dist carry it, and worlds without one serialise to
    the bytes they serialised to before;
  - tests/motion.cpp (stand-alone, its own main): value identity with velocities, the shutter's time in
    both precisions, the layouts the motion build relies on.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import motion_reference as MR
import motion_worlds as MW

HERE = os.path.dirname(os.path.abspath(__file__))


def _upload_error(rtc, scene, motion, n=None):
    """rt_scene_upload_moving with a null context: the lists' refusal, or "null context" when they pass."""
    args = list(scene.mapped_args())
    rc = rtc._lib.rt_scene_upload_moving(None, *args, motion, len(motion) if n is None else n)
    assert rc != 0
    return rtc._lib.rt_last_error().decode()


def _motion(rtc, *entries):
    m = (rtc.MotionDesc * len(entries))()
    for k, (target, index, v) in enumerate(entries):
        m[k].target, m[k].index = target, index
        m[k].velocity[:] = list(map(float, v))
    return m


def test_upload_refusals_have_their_own_texts(rtc):
    scene = MW.world("far_instance")[0]  # two shapes and one instance of an eight-triangle mesh: a world of ten shapes
    ns = len(scene.shapes)
    assert ns == 2 and len(scene.instances) == 1
    S, I = rtc.RT_MOVE_SHAPE, rtc.RT_MOVE_INSTANCE
    assert "null motion list with nonzero count" in _upload_error(rtc, scene, None, 2)
    assert "motion 0: unknown target" in _upload_error(rtc, scene, _motion(rtc, (2, 0, (1, 0, 0))))
    assert "motion 1: index out of range" in _upload_error(rtc, scene, _motion(rtc, (S, 0, (1, 0, 0)), (S, ns + 8, (1, 0, 0))))
    assert "motion 0: index out of range" in _upload_error(rtc, scene, _motion(rtc, (I, 1, (1, 0, 0))))
    assert "motion 1: target named twice" in _upload_error(rtc, scene, _motion(rtc, (S, 1, (1, 0, 0)), (S, 1, (2, 0, 0))))
    assert "motion 2: target named twice" in _upload_error(
        rtc, scene, _motion(rtc, (I, 0, (1, 0, 0)), (S, 0, (1, 0, 0)), (I, 0, (1, 0, 0))))
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert "motion 0: a velocity component that is not finite" in _upload_error(rtc, scene, _motion(rtc, (S, 0, (0, bad, 0))))
    for j in (0, 7):  # a triangle of the instance's mesh: world indices ns .. ns + 7
        assert "motion 0: the shape belongs to a mesh run" in _upload_error(rtc, scene, _motion(rtc, (S, ns + j, (1, 0, 0))))
    # the lists pass: the context is looked at last
    assert _upload_error(rtc, scene, _motion(rtc, (S, 0, (1, 0, 0)), (I, 0, (0, 0, 0)))) == "null context"
    assert _upload_error(rtc, scene, scene.motion) == "null context"
    # ... and after the other lists' own checks
    broken = MW.world("far_sphere")[0].at_time(0.0)  # (a copy of the tables)
    broken.shapes[1].material = len(broken.materials)
    rc = rtc._lib.rt_scene_upload_moving(None, *broken.mapped_args(), _motion(rtc, (2, 0, (1, 0, 0))), 1)
    assert rc != 0 and rtc._lib.rt_last_error().decode() == "shape 1: material index out of range"


def test_shutter_refusals_have_their_own_texts(rtc):
    cam = MW.camera(7, 5)
    opts = rtc.Context.options(2, "f64")
    out = np.zeros((5, 7, 3))

    def render(shutter, lens=None, device=False):
        fn = rtc._lib.rt_render_shutter_device if device else rtc._lib.rt_render_shutter
        rc = fn(None, C.byref(cam), C.byref(opts), 2, None if lens is None else C.byref(lens),
                None if shutter is None else C.byref(shutter), out.ctypes.data_as(C.c_void_p), None)
        assert rc != 0
        return rtc._lib.rt_last_error().decode()
    for device in (False, True):
        assert render(None, device=device) == "null shutter"
        for bad in (rtc.Shutter(float("nan"), 1), rtc.Shutter(0, float("inf"))):
            assert render(bad, device=device) == "shutter bound that is not finite"
        assert "open > close" in render(rtc.Shutter(1.0, 0.5), device=device)
        s = rtc.Shutter(0, 1)
        s.jitter = 2
        assert "shutter jitter 2 is neither RT_JITTER_NONE nor RT_JITTER_HASHED" in render(s, device=device)
        # after those, whatever rt_render_lens refuses, with its text: the lens, then the context
        assert render(rtc.Shutter(0, 1), rtc.Lens(-1.0, 5.0), device=device) == "lens aperture below 0 or not finite"
        assert render(rtc.Shutter(0, 1), rtc.Lens(0.1, 0.0), device=device) == "lens focal distance not above 0 or not finite"
        assert render(rtc.Shutter(0, 1), rtc.Lens(0.1, 5.0), device=device) == "null context"
        assert render(rtc.Shutter(0.5, 0.5), device=device) == "null context"  # open == close is a shutter
    with pytest.raises(rtc.RenderError, match="null shutter"):
        rtc.shutter_time(cam, 2, None, 0, 0, 0, 0)
    with pytest.raises(rtc.RenderError, match="open > close"):
        rtc.shutter_time(cam, 2, rtc.Shutter(2, 1), 0, 0, 0, 0)
    with pytest.raises(rtc.RenderError, match="sample grid 5 outside 1..4"):
        rtc.shutter_time(cam, 5, rtc.Shutter(0, 1), 0, 0, 0, 0)
    for x, y, i, j in ((7, 0, 0, 0), (0, 5, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2)):
        with pytest.raises(rtc.RenderError, match="pixel or sample out of range"):
            rtc.shutter_time(cam, 2, rtc.Shutter(0, 1), x, y, i, j)


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_shutter_time_equals_the_numpy_restatement(rtc, n, jitter):
    w, h, open_, close, seed = 7, 5, -0.375, 1.7, 12345
    cam = MW.camera(w, h)
    want = MR.shutter_times(w, h, n, open_, close, jitter, seed)
    sh = rtc.Shutter(open_, close, jitter, seed)
    got = np.array([[[[rtc.shutter_time(cam, n, sh, x, y, i, j) for i in range(n)] for j in range(n)] for x in range(w)]
                    for y in range(h)])
    assert np.array_equal(got, want)
    assert want.min() >= open_ and want.max() <= close
    if not jitter:  # the cell centres, j outer and i inner
        assert np.array_equal(want[0, 0].reshape(-1), open_ + (close - open_) * ((np.arange(n * n) + 0.5) * (1.0 / (n * n))))
    else:           # every pixel takes each of the n^2 cells once, rotated per pixel
        cells = np.floor((want - open_) / (close - open_) * (n * n)).astype(int).reshape(h, w, -1)
        assert np.array_equal(np.sort(cells, axis=2), np.broadcast_to(np.arange(n * n), cells.shape))
        if n > 1:
            assert len({tuple(c) for c in cells.reshape(-1, n * n)}) > 1
            other = MR.shutter_times(w, h, n, open_, close, True, seed + 1)
            assert not np.array_equal(other, want)


def _mat_mul(a, b):
    """matrix.rs:317-330: each element the left fold over the row and the column."""
    return np.array([[((a[r, 0] * b[0, c] + a[r, 1] * b[1, c]) + a[r, 2] * b[2, c]) + a[r, 3] * b[3, c]
                      for c in range(4)] for r in range(4)])


def test_motion_displace_equals_numpy_and_time_zero_is_the_input(rtc):
    for name in ("far_cylinder", "far_instance", "glass"):
        scene = MW.world(name)[0]
        assert scene.moving
        for tau in (0.25, -1.5, 1.0):
            at = scene.at_time(tau)
            assert not at.moving and len(at.shapes) == len(scene.shapes)
            moved = {(m.target, m.index): np.array(m.velocity[:]) for m in scene.motion}
            for target, before, after in ((rtc.RT_MOVE_SHAPE, scene.shapes, at.shapes),
                                          (rtc.RT_MOVE_INSTANCE, scene.instances or [], at.instances or [])):
                for i, (b, a) in enumerate(zip(before, after)):
                    inv = np.array(b.inverse[:]).reshape(4, 4)
                    if (target, i) in moved:
                        t = np.eye(4)
                        t[:3, 3] = -(moved[(target, i)] * tau)
                        inv = _mat_mul(inv, t)
                        assert not np.array_equal(inv, np.array(b.inverse[:]).reshape(4, 4))
                    assert np.array_equal(np.array(a.inverse[:]).reshape(4, 4), inv), (name, tau, target, i)
        zero = scene.at_time(0.0)
        assert bytes(zero.shapes) == bytes(scene.shapes)
        if scene.instances is not None:
            assert bytes(zero.instances) == bytes(scene.instances)
    # a zero velocity (+0 or -0) moves nothing at any time; bad lists are refused
    scene = MW.world("far_sphere")[0]
    still = _motion(rtc, (rtc.RT_MOVE_SHAPE, 1, (0.0, -0.0, 0.0)))
    out = (rtc.ShapeDesc * len(scene.shapes))()
    assert rtc._lib.rt_motion_displace(scene.shapes, len(scene.shapes), None, 0, still, 1, 3.0, out, None) == 0
    assert bytes(out) == bytes(scene.shapes)
    for bad, text in ((_motion(rtc, (5, 0, (1, 0, 0))), "unknown target"), (_motion(rtc, (0, 9, (1, 0, 0))), "index out of range")):
        assert rtc._lib.rt_motion_displace(scene.shapes, len(scene.shapes), None, 0, bad, 1, 1.0, out, None) != 0
        assert text in rtc._lib.rt_last_error().decode()
    assert rtc._lib.rt_motion_displace(scene.shapes, len(scene.shapes), None, 0, still, 1, float("nan"), out, None) != 0


def test_tables_emit_the_motion_list(rtc):
    scene = MW.world("glass")[0]
    assert [(m.target, m.index, tuple(m.velocity)) for m in scene.motion] == [
        (0, 2, (2.6, 0.0, 0.0)), (0, 3, (0.9, 0.0, 0.0)), (0, 4, (-0.9, 0.1, 0.0))]
    inst = MW.world("far_instance")[0]
    assert [(m.target, m.index, tuple(m.velocity)) for m in inst.motion] == [(1, 0, MW.V_FAR)]
    moving, mapped = inst.moving_args(), inst.mapped_args()
    assert len(moving) == len(mapped) + 2 and moving[-2] is inst.motion and moving[-1] == 1
    for a, b in zip(moving[:-2], mapped):  # (the descriptor arrays over meshes and textures are made per call)
        assert a is b or a == b or bytes(a) == bytes(b)
    assert not MW.world("glass")[0].at_time(0.5).moving


def test_serialisation_carries_the_list_and_leaves_other_worlds_bytes_alone(rtc):
    from rtc_amd import dist, scene_io
    moving = MW.world("glass")[0]
    still = moving.at_time(0.0)
    # without a list: the bytes and the JSON they always were
    assert "motion" not in scene_io.tables_to_dict(still)
    plain = dist.scene_to_bytes(still)
    assert len(plain) == dist._HEADER.itemsize + sum(len(bytes(t)) for t in (still.shapes, still.materials, still.patterns, still.lights)) + \
        C.sizeof(rtc.CameraDesc)
    assert not dist.scene_from_bytes(plain).moving
    # with one: round trips, bit for bit
    data = dist.scene_to_bytes(moving)
    assert data[:len(plain)] == plain and len(data) == len(plain) + 3 * C.sizeof(rtc.MotionDesc)
    back = dist.scene_from_bytes(data)
    assert bytes(back.motion) == bytes(moving.motion) and bytes(back.shapes) == bytes(moving.shapes)
    d = json.loads(json.dumps(scene_io.tables_to_dict(moving)))
    again = scene_io.tables_from_dict(d)
    assert bytes(again.motion) == bytes(moving.motion) and bytes(again.shapes) == bytes(moving.shapes)
    with pytest.raises(ValueError):
        dist.scene_from_bytes(data[:-1])
    # a tail of an entry's size that is no entry (a garbled broadcast) is refused as well
    for tail in (b"\xff" * 32, bytes(rtc.MotionDesc(0, len(moving.shapes))), bytes(rtc.MotionDesc(2, 0))):
        with pytest.raises(ValueError):
            dist.scene_from_bytes(plain + tail)


def test_exported_symbols_and_struct_sizes(rtc):
    assert C.sizeof(rtc.MotionDesc) == 32 and C.sizeof(rtc.ShutterDesc) == 24 and C.sizeof(rtc.MotionInfo) == 24
    for name in ("rt_scene_upload_moving", "rt_scene_motion_info", "rt_motion_displace", "rt_render_shutter",
                 "rt_render_shutter_device", "rt_shutter_time", "rt_trace_rays_timed", "rt_trace_rays_timed_device"):
        assert name in rtc.EXPORTED_SYMBOLS and hasattr(rtc._lib, name)
    assert rtc.abi_version() == 3


def test_motion_cpp(tmp_path):
    exe = tmp_path / "motion"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-o", str(exe), os.path.join(HERE, "motion.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "ok", out.stdout + out.stderr
