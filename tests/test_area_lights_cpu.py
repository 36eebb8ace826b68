"""Area lights without a GPU (include/rtc.h "Area lights"): the descriptor's layout, rt_lights_expand,
rt_area_light_sample against the numpy restatement, the validation texts, the Python surface, the CLI's
argument, and the penumbra condition of the worlds the GPU tests render (tests/area_light_worlds.py):
a world whose soft shadows did not show would let a kernel that samples one point pass them all.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import area_light_reference as ref
import area_light_worlds as AW


def _desc(rtc, corner=(-0.5, -0.5, -5.0), u=(1.0, 0.0, 0.0), v=(0.0, 1.0, 0.0), us=2, vs=2, intensity=(1.0, 0.5, 0.25),
          jitter=0, seed=0):
    d = rtc.AreaLightDesc()
    d.corner[:], d.full_uvec[:], d.full_vvec[:], d.intensity[:] = corner, u, v, intensity
    d.usteps, d.vsteps, d.jitter, d.seed = us, vs, jitter, seed
    return d


def test_the_descriptor_is_112_bytes(rtc):
    assert C.sizeof(rtc.AreaLightDesc) == 112
    assert rtc.AreaLightDesc.usteps.offset == 96 and rtc.AreaLightDesc.seed.offset == 108
    assert rtc.abi_version() == 3


def test_lights_expand_writes_the_samples_after_the_point_lights(rtc):
    lib = rtc._lib
    point = (rtc.LightDesc * 1)()
    point[0].position[:], point[0].intensity[:] = (1.0, 2.0, 3.0), (0.1, 0.2, 0.3)
    area = (rtc.AreaLightDesc * 1)(_desc(rtc))
    n = C.c_uint32(0)
    assert lib.rt_lights_expand(point, 1, area, 1, None, C.byref(n)) == rtc.RT_OK and n.value == 5
    out = (rtc.LightDesc * 5)()
    n = C.c_uint32(0)
    assert lib.rt_lights_expand(point, 1, area, 1, out, C.byref(n)) == rtc.RT_OK and n.value == 5
    assert tuple(out[0].position) == (1.0, 2.0, 3.0) and tuple(out[0].intensity) == (0.1, 0.2, 0.3)
    want = [(-0.25, -0.25, -5.0), (0.25, -0.25, -5.0), (-0.25, 0.25, -5.0), (0.25, 0.25, -5.0)]  # k = j * usteps + i
    for k in range(4):
        assert tuple(out[1 + k].position) == want[k], k
        assert tuple(out[1 + k].intensity) == (0.25, 0.125, 0.0625), k
    hashed = (rtc.AreaLightDesc * 1)(_desc(rtc, jitter=1))
    assert lib.rt_lights_expand(point, 1, hashed, 1, None, C.byref(n)) == rtc.RT_ERR_INVALID
    assert "hashed" in lib.rt_last_error().decode()
    assert lib.rt_lights_expand(None, 0, None, 0, None, C.byref(n)) == rtc.RT_OK and n.value == 0


def _keys(n=4096, seed=3):
    rng = np.random.default_rng(seed)
    ray_id = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    remaining = rng.integers(0, 17, size=n)
    area_index = rng.integers(0, 5, size=n)
    k = rng.integers(0, 256, size=n)
    seeds = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    ray_id[:4] = (2 ** 32 - 1, 0, 2 ** 32 - 1, 1)
    remaining[:4] = (0, 16, 16, 0)
    k[:4] = (255, 255, 0, 255)
    return ray_id, remaining, area_index, k, seeds


def test_sample_positions_equal_the_numpy_restatement_bit_for_bit(rtc):
    ray_id, remaining, area_index, k, seeds = _keys()
    worst = 0
    for mode in (1, 0):
        for n in range(len(k)):
            d = _desc(rtc, corner=(0.3, -1.7, 2.9), u=(1.1, 0.2, -0.3), v=(-0.4, 0.9, 1.3), us=16, vs=16, jitter=mode,
                      seed=int(seeds[n]))
            got = rtc.area_light_sample(d, int(area_index[n]), int(ray_id[n]), int(remaining[n]), int(k[n]))
            want = ref.position(d, int(area_index[n]), ray_id[n:n + 1], int(remaining[n]), int(k[n]))[0]
            worst += int(not np.array_equal(got.view(np.uint64), want.view(np.uint64)))
    assert worst == 0, f"{worst} of {2 * len(k)} samples differ from the restatement"
    # a 3 x 5 light: k = j * usteps + i with usteps = 3
    d = _desc(rtc, us=3, vs=5)
    for kk in range(15):
        assert np.array_equal(rtc.area_light_sample(d, 0, 0, 0, kk), ref.position(d, 0, [0], 0, kk)[0]), kk


def test_jitter_is_a_multiple_of_two_to_the_minus_24_in_the_unit_interval():
    ray_id, remaining, area_index, k, seeds = _keys()
    ju, jv = ref.jitter(seeds, ray_id, remaining, area_index, k)
    for j in (ju, jv):
        assert (j >= 0.0).all() and (j < 1.0).all()
        assert np.array_equal(j * 2.0 ** 24, np.floor(j * 2.0 ** 24))
        assert np.array_equal(j.astype(np.float32).astype(np.float64), j)  # exact in f32 too
    assert 0.4 < ju.mean() < 0.6 and 0.4 < jv.mean() < 0.6 and abs(np.corrcoef(ju, jv)[0, 1]) < 0.1
    # the library's own jitter, through a unit light whose sample is (ju, jv, 0)
    import rtc_amd as rtc
    d = _desc(rtc, corner=(0.0, 0.0, 0.0), us=1, vs=1, jitter=1, seed=99)
    for n in range(64):
        p = rtc.area_light_sample(d, int(area_index[n]), int(ray_id[n]), int(remaining[n]), 0)
        u, v = ref.jitter(99, ray_id[n:n + 1], int(remaining[n]), int(area_index[n]), 0)
        assert (p[0], p[1], p[2]) == (u[0], v[0], 0.0)


def test_every_refusal_has_its_own_text_and_needs_no_device(rtc):
    lib = rtc._lib
    t = AW.opaque()

    def refuse(area, n=1):
        args = t.textured_args() + ((rtc.AreaLightDesc * 1)(area) if area is not None else None, n)
        assert lib.rt_scene_upload_lit(None, *args) == rtc.RT_ERR_INVALID
        return lib.rt_last_error().decode()

    nan, inf = float("nan"), float("inf")
    texts = [refuse(None), refuse(_desc(rtc, us=0)), refuse(_desc(rtc, vs=17)), refuse(_desc(rtc, jitter=2)),
             refuse(_desc(rtc, corner=(0.0, nan, 0.0)))]
    assert len(set(texts)) == len(texts), texts
    assert "null" in texts[0] and "0" in texts[1] and "RT_LIGHT_MAX_STEPS" in texts[2] and "jitter" in texts[3] \
        and "finite" in texts[4], texts
    for bad in (_desc(rtc, u=(inf, 0.0, 0.0)), _desc(rtc, v=(0.0, 0.0, nan)), _desc(rtc, intensity=(1.0, -inf, 1.0))):
        assert refuse(bad) == texts[4]
    assert refuse(_desc(rtc, us=17)) == texts[2] and refuse(_desc(rtc, vs=0)) == texts[1]
    # a valid list reaches the context check; zero-length edges are allowed
    ok = t.textured_args() + ((rtc.AreaLightDesc * 1)(_desc(rtc, u=(0.0, 0.0, 0.0), v=(0.0, 0.0, 0.0), us=16, vs=16)), 1)
    assert lib.rt_scene_upload_lit(None, *ok) == rtc.RT_ERR_INVALID and lib.rt_last_error().decode() == "null context"
    n = C.c_uint32(0)
    assert lib.rt_lights_expand(None, 0, (rtc.AreaLightDesc * 1)(_desc(rtc, us=0)), 1, None, C.byref(n)) == rtc.RT_ERR_INVALID
    assert lib.rt_last_error().decode() == texts[1]
    with pytest.raises(rtc.RenderError):
        rtc.area_light_sample(_desc(rtc), 0, 0, 0, 4)  # k = usteps * vsteps


def test_the_python_surface_expands_like_the_library(rtc):
    t = AW.opaque()
    assert t.lit and len(t.area_lights) == 2 and len(t.lights) == 1
    flat = t.expanded()
    assert not flat.lit and len(flat.lights) == 1 + 4 + 16 and flat.shapes is t.shapes
    n = C.c_uint32(0)
    out = (rtc.LightDesc * 21)()
    assert rtc._lib.rt_lights_expand(t.lights, 1, t.area_lights, 2, out, C.byref(n)) == rtc.RT_OK and n.value == 21
    assert bytes(out) == bytes(flat.lights)
    for a, al in enumerate(t.area_lights):  # and like the restatement
        base = 1 + (0 if a == 0 else 4)
        for k in range(al.usteps * al.vsteps):
            assert np.array_equal(np.array(flat.lights[base + k].position[:]), ref.position(al, a, [0], 0, k)[0])
    with pytest.raises(rtc.RenderError, match="hashed"):
        AW.opaque(jitter=True).expanded()
    plain = AW.one_by_one()[1]
    assert not plain.lit and plain.expanded() is plain
    tori = AW.textured_tori(rtc)
    flat = tori.expanded()
    assert len(flat.lights) == 2 + 9 and len(flat.shapes) == 1 + 3 * 576 and flat.smoothed and flat.textured


def _penumbra_worlds(rtc):
    import texture_worlds as X
    tori = AW.textured_tori(rtc)
    return {"opaque": (AW.opaque(), 0), "mirror": (AW.mirror(), 4), "small opaque": (AW.opaque(size=AW.SMALL), 0),
            "mirror plane": (AW.unjittered(AW.mirror_plane()), 1),
            "bright": (AW.bright(1.0), 4),
            "tori": (AW.with_area_tables(X.without_textures(rtc, tori), tori), 3)}


@pytest.mark.parametrize("key", ["opaque", "mirror", "small opaque", "mirror plane", "bright", "tori"])
def test_the_gpu_worlds_show_a_penumbra(rtc, oracle, key):
    """The oracle's frame of the expansion against its frame under one point light of full intensity at each
    area light's centre: more than 1e-3 apart on at least 5 % of the pixels."""
    tables, depth = _penumbra_worlds(rtc)[key]
    soft, _ = oracle.render(tables.expanded(), tables.camera, depth)
    hard, _ = oracle.render(AW.centre_lit(rtc, tables).expanded(), tables.camera, depth)
    share = float((np.abs(soft - hard).max(axis=2) > 1e-3).mean())
    print(f"{key}: {share:.4f} of the pixels differ by more than 1e-3")
    assert share >= 0.05, f"{key}: only {share:.4f}"


def test_cli_refuses_a_malformed_area_light(rtc, tmp_path):
    import os

    from conftest import PKG, SCENES_YAML
    exe = os.path.join(PKG, "rtc_amd", "_lib", "rtc")
    scene = os.path.join(SCENES_YAML, sorted(os.listdir(SCENES_YAML))[0])
    for bad in ("0,5,0:1,0,0:0,0,1", "0,5,0:1,0,0:0,0,1:2by2", "0,5,0:1,0,0:0,0,1:2x2:wobble", "0,5:1,0,0:0,0,1:2x2"):
        r = subprocess.run([exe, scene, str(tmp_path / "o.ppm"), "--area-light", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "--area-light takes" in r.stderr, (bad, r.stderr[:200])


def test_the_area_build_keeps_the_register_caps(tmp_path):
    """The f32 tracer kernels of the area build (rtc::area::) hold the instance build's caps, read from the
    gfx950 code objects inside librtc.so as tests/test_isa_budget_texture.py reads them: trace_direct* at most
    64 VGPRs (8 waves per SIMD), trace_pool* at most 80 (6 waves)."""
    import re

    from test_isa_budget_texture import CAPS, all_kernels
    kernels = all_kernels(str(tmp_path))
    checked = 0
    for name, (vgpr, priv) in kernels.items():
        kind = re.search(r"\d+(trace_direct|trace_pool)(_ss)?If", name)
        if not name.startswith("_ZN3rtc4area") or not kind:
            continue
        print(name, vgpr, priv)
        assert vgpr <= CAPS[kind.group(1)], f"{name}: {vgpr} VGPRs > {CAPS[kind.group(1)]} (occupancy cliff)"
        checked += 1
    assert checked == 12  # direct x 2, pool x 4, and their supersampled twins
