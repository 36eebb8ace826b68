"""CPU checks of supersampled frames (rt_render_supersampled*): no GPU.

* The premise of the oracle comparison, so it comes first: the sample camera
  Cn = rt_camera_resize(C, n W, n H) keeps C's half_width and half_height bit
  for bit (n W / n H and W / H round to the same f64) and equals the oracle's
  camera of that size field by field, for random fields of view and sizes of
  aspect above and below 1 and n = 2..4.
* The pool kernel's seeding rule against its capacity rule
  (rtc_internal.hpp pool_capacity_ss): tests/pool_seed_model.cpp models seeds,
  pops and pushes for n = 1..4 at depths 0..16.
* The u8 test's premise: the averaged oracle frames of the scenes and sizes
  tests/test_gpu_supersample.py quantizes keep at most 0.1 % of their pixels
  within 1e-9 of a rounding boundary.
* The C entry points' argument checks that need no device, the Python
  mirror, and the CLI's --samples.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, scene_fixture

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(PKG, "rtc_amd", "_lib", "librtc.so")
CLI = os.path.join(PKG, "rtc_amd", "_lib", "rtc")
RT_ERR_INVALID = -1
MAX_DEPTH, MAX_GRID, BLOCK = 16, 4, 256


def box_mean(img, n):
    """(n H, n W, 3) f64 -> (H, W, 3): the mean of each n x n block, summed j outer, i inner."""
    h, w = img.shape[0] // n, img.shape[1] // n
    acc = np.zeros((h, w, 3), dtype=np.float64)
    for j in range(n):
        for i in range(n):
            acc = acc + img[j::n, i::n].astype(np.float64)
    return acc * (1.0 / (n * n))


def near_boundary(mean, tol=1e-9):
    """Pixels with a channel whose 255 x clamp(value) lies within 255 x tol of k + 0.5."""
    c = np.clip(mean, 0.0, 1.0) * 255.0
    return (np.abs(c - np.floor(c) - 0.5) <= 255.0 * tol).any(axis=2)


def test_sample_camera_keeps_the_half_extents(rtc, oracle):
    rng = np.random.default_rng(2024)
    frm, to, up = (1.0, 2.0, -5.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0)
    sizes = [(70, 22), (130, 10), (320, 200), (22, 70), (1, 1), (1920, 1080), (3840, 2160), (1080, 1920), (333, 333)]
    sizes += [(int(rng.integers(1, 5000)), int(rng.integers(1, 5000))) for _ in range(150)]
    assert any(w > h for w, h in sizes) and any(w < h for w, h in sizes)
    for w, h in sizes:
        fov = float(rng.uniform(0.05, 3.0))
        c = rtc.camera_make(w, h, fov, frm, to, up)
        for n in (2, 3, 4):
            cn = rtc.camera_resize(c, n * w, n * h)
            assert (cn.half_width, cn.half_height) == (c.half_width, c.half_height), (w, h, fov, n)
            assert cn.pixel_size == (c.half_width * 2.0) / (n * w), (w, h, fov, n)
            ref = oracle.camera(n * w, n * h, fov, frm, to, up)
            for f in ("width", "height", "field_of_view", "half_width", "half_height", "pixel_size"):
                assert getattr(cn, f) == getattr(ref, f), (f, w, h, fov, n)
            assert list(cn.inverse) == list(ref.inverse) and list(cn.origin) == list(ref.origin), (w, h, fov, n)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pool_seed_model") / "pool_seed_model"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", str(exe), os.path.join(HERE, "pool_seed_model.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split()[-1] == "ok", (out.returncode, out.stdout[-400:], out.stderr)
    table = {}
    for line in out.stdout.splitlines():
        if line.startswith("peak"):
            _, n, d, peak, rule = line.split()
            table[int(n), int(d)] = (int(peak), int(rule))
    return table


def test_pool_seeding_never_exceeds_the_capacity_rule(model):
    assert sorted(model) == [(n, d) for n in range(1, MAX_GRID + 1) for d in range(MAX_DEPTH + 1)]
    for (n, d), (peak, rule) in model.items():
        # the bound of a plain frame, whatever the grid; tight with two children everywhere
        assert rule == BLOCK + d * BLOCK, (n, d)
        assert peak <= rule and peak == (rule if d else BLOCK), (n, d, peak, rule)


# tests/test_gpu_supersample.py's u8 cases.  (three_sphere_scene and
# reflect_refract are not among them: their walls' colours sit on a boundary
# exactly, e.g. 0.1 x 255 = 25.5, in 1-7 % of the pixels at any size.)
U8_CASES = [("shadow_puppets", 70, 22, 2), ("shadow_puppets", 70, 22, 3), ("shadow_puppets", 130, 10, 4),
            ("refraction", 70, 22, 2), ("refraction", 70, 22, 3), ("refraction", 130, 10, 4)]


@pytest.mark.parametrize("name,w,h,n", U8_CASES)
def test_u8_cases_stay_clear_of_rounding_boundaries(rtc, oracle, name, w, h, n):
    scene = scene_fixture(name)
    cn = rtc.camera_resize(scene.camera, n * w, n * h)
    ref, _ = oracle.render(scene, cn, 6, threads=8)
    exempt = near_boundary(box_mean(ref, n))
    assert exempt.mean() <= 0.001, f"{name} {w}x{h} n={n}: {int(exempt.sum())} of {exempt.size} pixels near a boundary"


def test_entry_points_check_their_arguments_without_a_device():
    lib = C.CDLL(LIB)
    lib.rt_last_error.restype = C.c_char_p
    for fn in (lib.rt_render_supersampled, lib.rt_render_supersampled_device):
        assert fn(None, None, None, C.c_uint32(2), None, None) == RT_ERR_INVALID
        assert b"null context" in lib.rt_last_error()


def test_python_mirror(rtc):
    assert rtc.RT_MAX_SAMPLE_GRID == MAX_GRID
    assert {"rt_render_supersampled", "rt_render_supersampled_device"} <= set(rtc.EXPORTED_SYMBOLS)
    assert callable(rtc.Context.render_supersampled) and callable(rtc.Context.render_supersampled_device)
    header = open(os.path.join(ROOT, "include", "rtc.h")).read()
    assert f"#define RT_MAX_SAMPLE_GRID {MAX_GRID}\n" in header and "#define RT_ABI_VERSION 3\n" in header


def test_cli_samples_flag():
    r = subprocess.run([CLI], capture_output=True, text=True)
    assert r.returncode != 0 and "--samples N" in r.stderr
    for bad in ("0", "5", "two", "2x", "-1"):
        r = subprocess.run([CLI, "a.yaml", "b.png", "--samples", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "--samples takes a whole number from 1 to 4" in r.stderr, (bad, r.stderr)
    r = subprocess.run([CLI, "a.yaml", "b.png", "--samples"], capture_output=True, text=True)
    assert r.returncode == 2
