"""CPU checks of the thin-lens camera (rt_render_lens*, rt_lens_ray): no GPU.

* rt_lens_ray against the numpy restatement of the header (tests/lens_reference.py), bit for bit.
* The ray's geometry: aperture 0 is the pinhole ray, every origin lies on the lens disc, the hashed cell
  rotation is a permutation of the cells.
* The entry points' refusals that need no device, and the Python mirror.
* On the oracle alone: a matte wall at the focal distance renders as through a pinhole, and the u8 cases of
  tests/test_gpu_lens.py stay clear of rounding boundaries.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import lens_reference as LR
from conftest import PKG, ROOT, scene_fixture
from test_supersample_cpu import near_boundary

LIB = os.path.join(PKG, "rtc_amd", "_lib", "librtc.so")
RT_ERR_INVALID = -1
APERTURE = 0.25
# (scene, focal distance) x (W, H, n): the u8 cases, here and on the GPU
U8_FOCUS = {"shadow_puppets": 20.0, "refraction": 5.0}
U8_CASES = [(name, w, h, n) for name in U8_FOCUS for (w, h, n) in ((70, 22, 2), (70, 22, 3), (130, 10, 4))]


def random_camera(rtc, rng, w, h):
    frm = rng.uniform(-6.0, 6.0, size=3)
    to = frm + rng.uniform(-1.0, 1.0, size=3) + np.array([0.0, 0.0, 3.0])
    return rtc.camera_make(w, h, float(rng.uniform(0.3, 2.0)), tuple(frm), tuple(to), (0.0, 1.0, 0.0))


def wall_world(sphere=False):
    """A matte wall at z = 3 under one light, seen from (0, 0, -2): the wall is 5 from the camera along the
    view axis.  With `sphere`, a ball in front of it (out of focus at focus 5)."""
    from rtc_amd import world as W
    wall = W.plane(W.Material(color=(0.9, 0.8, 0.3), specular=0.0),
                   transform=W.mat_mul(W.translation(0.0, 0.0, 3.0), W.rotation_x(np.pi / 2)))
    shapes = [wall]
    if sphere:
        shapes.append(W.sphere(W.Material(color=(0.9, 0.2, 0.2), specular=0.0),
                               transform=W.mat_mul(W.translation(0.3, 0.1, 0.0), W.scaling(0.5, 0.5, 0.5))))
    cam = W.camera(70, 22, 0.9, (0.0, 0.0, -2.0), (0.0, 0.0, 3.0), (0.0, 1.0, 0.0))
    return W.World([W.Light((-3.0, 4.0, -5.0), (1.0, 1.0, 1.0))], shapes).tables(cam)


@functools.lru_cache(maxsize=None)
def oracle_lens_frame(name, w, h, n, aperture, focal, jitter, seed, depth=6):
    """(frame, stats) of the oracle's lens frame of a reference scene, once per case; read-only."""
    import pyoracle
    import rtc_amd
    tables = wall_world(name == "wall+sphere") if name.startswith("wall") else scene_fixture(name)
    cn = rtc_amd.camera_resize(tables.camera, n * w, n * h)
    img, st = LR.lens_frame(pyoracle, tables, cn, w, h, n, aperture, focal, jitter, seed, depth)
    img.setflags(write=False)
    return img, st


# ------------------------------------------------------------------ rt_lens_ray
@pytest.mark.parametrize("jitter", [False, True])
def test_lens_ray_equals_the_numpy_restatement_bit_for_bit(rtc, jitter):
    rng = np.random.default_rng(355)
    for case in range(12):
        n = 1 + case % 4
        w, h = int(rng.integers(1, 90)), int(rng.integers(1, 40))
        cam = random_camera(rtc, rng, w, h)
        cn = rtc.camera_resize(cam, n * w, n * h)
        aperture, focal = float(rng.uniform(0.0, 0.6)), float(rng.uniform(0.5, 30.0))
        for seed in (0, 1, 0xDEADBEEF):
            lens = rtc.Lens(aperture, focal, jitter, seed)
            want = LR.lens_rays(cn, w, h, n, aperture, focal, jitter, seed)
            picks = [(int(rng.integers(w)), int(rng.integers(h)), int(rng.integers(n)), int(rng.integers(n)))
                     for _ in range(24)] + [(0, 0, 0, 0), (w - 1, h - 1, n - 1, n - 1)]
            for x, y, i, j in picks:
                got = rtc.lens_ray(cam, n, lens, x, y, i, j)
                assert got.tobytes() == want[y, x, j, i].tobytes(), (case, seed, x, y, i, j, got, want[y, x, j, i])
            if not jitter:
                break  # (the seed is unread)


def test_aperture_zero_is_the_pinhole_ray(rtc, oracle):
    """Origin exactly, direction within 4 ulp of Cn's ray_for_pixel, an ulp being that of 1 (the directions
    are unit vectors).  The pinhole forms pixel - origin at distance 1 and the lens ray target - origin at
    distance f; each point transform's absolute error grows with |origin| and is divided by the ray's
    length, so the two directions differ by about (1 + |origin| (1 + 1 / f)) roundings.  The bar is therefore
    stated for cameras within 2.5 of the world origin per axis and f >= 2 (at most 4.75 such units, 0.72 ulp
    each at worst over 300 random cameras); a camera farther out loses those bits in both rays alike."""
    rng = np.random.default_rng(7)
    for case in range(8):
        n, w, h = 1 + case % 4, 33, 17
        frm = rng.uniform(-2.5, 2.5, size=3)
        to = frm + rng.uniform(-1.0, 1.0, size=3) + np.array([0.0, 0.0, 3.0])
        cam = rtc.camera_make(w, h, float(rng.uniform(0.3, 2.0)), tuple(frm), tuple(to), (0.0, 1.0, 0.0))
        cn = rtc.camera_resize(cam, n * w, n * h)
        focal = float(rng.uniform(2.0, 30.0))
        rays = LR.lens_rays(cn, w, h, n, 0.0, focal, bool(case & 1), 5)
        inv = np.array(cn.inverse[:]).reshape(4, 4)
        py, px = np.meshgrid(np.arange(n * h), np.arange(n * w), indexing="ij")
        wx = cn.half_width - (px + 0.5) * cn.pixel_size
        wy = cn.half_height - (py + 0.5) * cn.pixel_size
        pixel = LR._point(cn.inverse, wx, wy, np.full_like(wx, -1.0))
        d = np.stack([p - o for p, o in zip(pixel, cn.origin[:3])], axis=-1)
        d /= np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])[..., None]
        got = rays.transpose(0, 2, 1, 3, 4).reshape(n * h, n * w, 6)  # [y, j, x, i] -> sample-camera pixels
        assert (got[..., :3] == np.array(cn.origin[:3])).all()
        assert (got[..., :3] == inv[:3, 3]).all()
        worst = float(np.abs(got[..., 3:] - d).max() / np.spacing(1.0))
        assert worst <= 4.0, worst
        for x, y, i, j in ((0, 0, 0, 0), (w - 1, h - 1, n - 1, n - 1)):
            one = rtc.lens_ray(cam, n, rtc.Lens(0.0, focal, bool(case & 1), 5), x, y, i, j)
            assert one.tobytes() == rays[y, x, j, i].tobytes()


@pytest.mark.parametrize("jitter", [False, True])
def test_every_origin_lies_on_the_lens_disc(rtc, jitter):
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 4):
        w, h = 40, 12
        cam = random_camera(rtc, rng, w, h)
        cn = rtc.camera_resize(cam, n * w, n * h)
        aperture = float(rng.uniform(0.05, 0.8))
        rays = LR.lens_rays(cn, w, h, n, aperture, 4.0, jitter, 3).reshape(-1, 6)
        fwd = np.linalg.inv(np.array(cn.inverse[:]).reshape(4, 4))  # world -> camera
        local = rays[:, :3] @ fwd[:3, :3].T + fwd[:3, 3]
        assert np.abs(local[:, 2]).max() < 1e-12
        assert np.hypot(local[:, 0], local[:, 1]).max() <= aperture * (1.0 + 1e-12)
        # the unit directions aim at the focal plane's point of the pinhole ray
        assert np.abs(np.linalg.norm(rays[:, 3:], axis=1) - 1.0).max() < 1e-12
        if not jitter:  # n^2 distinct lens points in all, the same for every pixel
            assert len(np.unique(np.round(local[:, :2], 12), axis=0)) == n * n


def test_hashed_cell_rotation_is_a_permutation_of_the_cells():
    for n in (1, 2, 3, 4):
        w, h = 37, 9
        y, x, j, i = np.meshgrid(np.arange(h), np.arange(w), np.arange(n), np.arange(n), indexing="ij")
        rotations = set()
        for seed in (0, 9, 0xFFFFFFFF):
            ci, cj, ju, jv = LR.lens_cells(w, h, n, x, y, i, j, True, seed)
            cells = (cj * n + ci).astype(int).reshape(h, w, n * n)
            assert (np.sort(cells, axis=2) == np.arange(n * n)).all()
            assert ju.min() >= 0.0 and ju.max() < 1.0 and jv.min() >= 0.0 and jv.max() < 1.0
            rotations |= set(cells[:, :, 0].ravel())
        assert rotations == set(range(n * n))  # every rotation occurs


# ------------------------------------------------------------------ refusals, mirror
def test_entry_points_check_their_arguments_without_a_device(rtc):
    lib = C.CDLL(LIB)
    lib.rt_last_error.restype = C.c_char_p
    cam = rtc.camera_make(8, 8, 1.0, (0, 0, -5), (0, 0, 0), (0, 1, 0))
    ray = (C.c_double * 6)()

    def calls(lens):
        p = None if lens is None else C.byref(lens)
        yield lib.rt_render_lens(None, None, None, C.c_uint32(2), p, None, None)
        yield lib.rt_render_lens_device(None, None, None, C.c_uint32(2), p, None, None)
        yield lib.rt_lens_ray(C.byref(cam), C.c_uint32(2), p, 0, 0, 0, 0, ray)

    bad = [(None, b"null lens"),
           (rtc.LensDesc(-0.1, 5.0, 0, 0), b"aperture"), (rtc.LensDesc(float("nan"), 5.0, 0, 0), b"aperture"),
           (rtc.LensDesc(float("inf"), 5.0, 0, 0), b"aperture"),
           (rtc.LensDesc(0.1, 0.0, 0, 0), b"focal distance"), (rtc.LensDesc(0.1, -1.0, 0, 0), b"focal distance"),
           (rtc.LensDesc(0.1, float("inf"), 0, 0), b"focal distance"),
           (rtc.LensDesc(0.1, float("nan"), 0, 0), b"focal distance"),
           (rtc.LensDesc(0.1, 5.0, 2, 0), b"jitter")]
    texts = set()
    for lens, text in bad:
        for rc in calls(lens):
            assert rc == RT_ERR_INVALID and text in lib.rt_last_error(), (text, lib.rt_last_error())
        texts.add(lib.rt_last_error())
    assert len(texts) == 4  # each kind of refusal has its own text
    good = rtc.LensDesc(0.1, 5.0, 1, 3)
    for fn in (lib.rt_render_lens, lib.rt_render_lens_device):  # then rt_render_supersampled's checks
        assert fn(None, None, None, C.c_uint32(2), C.byref(good), None, None) == RT_ERR_INVALID
        assert b"null context" in lib.rt_last_error()
    for args in ((0, 0, 0, 0, 0), (5, 0, 0, 0, 0), (2, 8, 0, 0, 0), (2, 0, 8, 0, 0), (2, 0, 0, 2, 0), (2, 0, 0, 0, 2)):
        assert lib.rt_lens_ray(C.byref(cam), C.c_uint32(args[0]), C.byref(good), *args[1:], ray) == RT_ERR_INVALID
    assert lib.rt_lens_ray(None, C.c_uint32(2), C.byref(good), 0, 0, 0, 0, ray) == RT_ERR_INVALID
    assert lib.rt_lens_ray(C.byref(cam), C.c_uint32(2), C.byref(good), 7, 7, 1, 1, ray) == 0


def test_python_mirror(rtc):
    assert {"rt_render_lens", "rt_render_lens_device", "rt_lens_ray"} <= set(rtc.EXPORTED_SYMBOLS)
    assert callable(rtc.Context.render_lens) and callable(rtc.Context.render_lens_device) and callable(rtc.lens_ray)
    assert C.sizeof(rtc.LensDesc) == 24
    lens = rtc.Lens(0.25, 5.0, jitter=True, seed=9)
    assert (lens.aperture, lens.focal_distance, lens.jitter, lens.seed) == (0.25, 5.0, rtc.RT_JITTER_HASHED, 9)
    assert rtc.Lens(0.1, 2.0).jitter == rtc.RT_JITTER_NONE
    header = open(os.path.join(ROOT, "include", "rtc.h")).read()
    assert "typedef struct rt_lens_desc" in header and "#define RT_ABI_VERSION 3\n" in header
    assert rtc.abi_version() == 3


# ------------------------------------------------------------------ on the oracle alone
@pytest.mark.parametrize("jitter", [False, True])
def test_a_matte_wall_at_the_focal_distance_renders_as_through_a_pinhole(rtc, oracle, jitter):
    """Every lens ray of a sample meets the wall where the pinhole ray does, and a matte surface's colour
    does not depend on the eye."""
    tables = wall_world()
    w, h, n = 70, 22, 2
    cn = rtc.camera_resize(tables.camera, n * w, n * h)
    lens, _ = oracle_lens_frame("wall", w, h, n, 0.3, 5.0, jitter, 4)
    pin, _ = LR.lens_frame(oracle, tables, cn, w, h, n, 0.0, 5.0, False, 0, 6)
    err = float(np.abs(lens - pin).max())
    print(f"wall at focus, jitter {jitter}: max |lens - pinhole| {err:.3g}")
    assert err <= 1e-12
    blurred, _ = oracle_lens_frame("wall+sphere", w, h, n, 0.3, 5.0, jitter, 4)
    sharp, _ = LR.lens_frame(oracle, wall_world(True), cn, w, h, n, 0.0, 5.0, False, 0, 6)
    assert float(np.abs(blurred - sharp).max()) > 0.1


@pytest.mark.parametrize("name,w,h,n", U8_CASES)
def test_u8_cases_stay_clear_of_rounding_boundaries(name, w, h, n):
    for jitter in (False, True):
        ref, _ = oracle_lens_frame(name, w, h, n, APERTURE, U8_FOCUS[name], jitter, 1)
        exempt = near_boundary(ref)
        assert exempt.mean() <= 0.001, f"{name} {w}x{h} n={n} jitter {jitter}: {int(exempt.sum())} pixels near a boundary"
