"""Area lights on the GPU (include/rtc.h "Area lights"): an area light means its expansion
into point lights, so the f64 kernels are held to the oracle's render of rt_lights_expand's tables, within
1e-9 and with every counter equal; hashed jitter to the oracle's colour of each ray under that ray's own
samples, formed by the numpy restatement (tests/area_light_reference.py).

tests/test_area_lights_cpu.py shows that each world rendered here has a visible penumbra.
"""
import dataclasses
import functools
import json
import os

import numpy as np
import pytest

import area_light_reference as ref
import area_light_worlds as AW
import f32_tolerance_area as F32A
import mesh_worlds as M
from conftest import ROOT
from test_gpu_random_worlds import _counts

pytestmark = pytest.mark.gpu

TOL = 1e-9
EPSILON = 0.00000008  # consts.rs:2: the over_point offset of the f64 path


def _err(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max())


@functools.lru_cache(maxsize=None)
def _world(key):
    return {"opaque": AW.opaque, "mirror": AW.mirror}[key]()


@functools.lru_cache(maxsize=None)
def _oracle_frame(key, depth):
    import pyoracle
    t = _world(key)
    img, st = pyoracle.render(t.expanded(), t.camera, depth)
    img.setflags(write=False)
    return img, _counts(st)


# ------------------------------------------------------------------ 1: expansion parity, no jitter
@pytest.mark.parametrize("key,depth", [("opaque", 0), ("mirror", 4)])
def test_f64_frame_is_the_oracles_frame_of_the_expansion(gpu_ctx, key, depth):
    """64 x 32: the direct kernel (opaque, depth 0) and the pool kernel (mirror floor, glass sphere, depth 4)."""
    t = _world(key)
    gpu_ctx.upload(t)
    info = gpu_ctx.light_info()
    assert info["area_lights"] == 2 and info["samples"] == 20 and info["area_bytes"] == 2 * (64 + 112), info
    img, st = gpu_ctx.render(t.camera, depth, precision="f64")
    want, rst = _oracle_frame(key, depth)
    print(f"{key} depth {depth}: max |err| {_err(img, want):.3g}, shadow rays {st['shadow']}")
    assert _err(img, want) <= TOL
    assert _counts(st) == rst
    assert rst["shadow"] == 21 * rst["shaded"] and rst["lit_patterned"] % 21 == 0 and rst["lit_patterned"] > 0
    assert (rst["reflect"] > 0) == (key == "mirror")
    assert gpu_ctx.light_info()["ran_area"] == 1


@pytest.mark.parametrize("key,depth", [("opaque", 0), ("mirror", 4)])
def test_f64_ray_batches_and_color_at_are_the_oracles(gpu_ctx, oracle, key, depth):
    t = _world(key)
    rays = AW.seeded_rays(4096, 77)
    want, rst = oracle.color_at(t.expanded(), rays, depth)
    gpu_ctx.upload(t)
    got, ht, shape, st = gpu_ctx.trace_rays(rays, depth, precision="f64", hits=True)
    print(f"{key}: trace_rays max |err| {_err(got, want):.3g}, {int((shape >= 0).sum())} of 4096 rays hit")
    assert (shape >= 0).sum() > 2000 and len(set(shape.tolist())) == 4  # miss, floor, sphere, cube
    assert _err(got, want) <= TOL and _counts(st) == _counts(rst)
    got, st = gpu_ctx.color_at(rays, depth, precision="f64")
    print(f"{key}: color_at max |err| {_err(got, want):.3g}")
    assert _err(got, want) <= TOL and _counts(st) == _counts(rst)


@pytest.mark.parametrize("key,depth", [("opaque", 0), ("mirror", 4)])
def test_f64_supersampled_frame_is_the_mean_of_the_oracles_sample_frame(gpu_ctx, rtc, oracle, key, depth):
    """32 x 16 at grid 2: the samples are the pixels of the 64 x 32 camera."""
    t = _world(key)
    small = rtc.camera_resize(t.camera, *AW.SMALL)
    cn = rtc.camera_resize(small, 2 * AW.SMALL[0], 2 * AW.SMALL[1])
    fine, rst = oracle.render(t.expanded(), cn, depth)
    want = fine.reshape(AW.SMALL[1], 2, AW.SMALL[0], 2, 3).mean(axis=(1, 3))
    gpu_ctx.upload(t)
    img, st = gpu_ctx.render_supersampled(small, 2, depth, precision="f64")
    print(f"{key} grid 2: max |err| {_err(img, want):.3g}")
    assert _err(img, want) <= TOL and _counts(st) == _counts(rst)


def test_a_smooth_textured_instanced_world_equals_the_upload_of_its_expansion(gpu_ctx, rtc):
    """The oracle has no textures: the device's own upload of the expansion (flat triangles, point lights)
    through the older entry point is the reference."""
    t = AW.textured_tori(rtc)
    flat = t.expanded()
    assert not flat.lit and not flat.instanced and flat.smoothed and flat.textured and len(flat.lights) == 11
    rays = M.random_rays(2048, 99)
    gpu_ctx.upload(flat)
    assert gpu_ctx.light_info() == {"area_lights": 0, "samples": 0, "ran_area": 0, "area_bytes": 0}
    want, wst = gpu_ctx.render(t.camera, 3, precision="f64")
    wrays, wrst = gpu_ctx.trace_rays(rays, 3, precision="f64")
    assert gpu_ctx.light_info()["ran_area"] == 0
    gpu_ctx.upload(t)
    assert gpu_ctx.instance_info()["instances"] == 3 and gpu_ctx.smooth_info()["smooth_triangles"] == 3 * 576
    assert gpu_ctx.texture_info()["textured_triangles"] == 3 * 576 and gpu_ctx.light_info()["samples"] == 9
    img, st = gpu_ctx.render(t.camera, 3, precision="f64")
    got, rst = gpu_ctx.trace_rays(rays, 3, precision="f64")
    print(f"tori: frame max |diff| {_err(img, want):.3g}, rays {_err(got, wrays):.3g}")
    assert _err(img, want) <= TOL and _counts(st) == _counts(wst)
    assert _err(got, wrays) <= TOL and _counts(rst) == _counts(wrst)
    assert gpu_ctx.light_info()["ran_area"] == 1 and gpu_ctx.texture_info()["ran_textured"] == 1


# ------------------------------------------------------------------ 2: a 1 x 1 light
def test_a_one_by_one_light_is_the_point_light_at_its_centre(gpu_ctx, oracle):
    lit, point = AW.one_by_one()
    want, rst = oracle.render(point, point.camera, 0)
    gpu_ctx.upload(lit)
    img, st = gpu_ctx.render(lit.camera, 0, precision="f64")
    print(f"1 x 1: max |err| {_err(img, want):.3g}")
    assert _err(img, want) <= TOL and _counts(st) == _counts(rst)


# ------------------------------------------------------------------ 3, 4: hashed jitter
def _expected(rtc, oracle, tables, rays, ray_ids, remaining):
    """Per ray: the oracle's depth-0 colour of that ray in the world whose lights are the point lights plus
    that ray's own samples (area_light_reference.position) at intensity / N."""
    ray_ids = np.asarray(ray_ids, dtype=np.uint64)
    rows = [(tuple(lt.position), tuple(lt.intensity)) for lt in tables.lights]
    samples = []
    for a, al in enumerate(tables.area_lights):
        n = al.usteps * al.vsteps
        for k in range(n):
            samples.append(ref.position(al, a, ray_ids, remaining, k))
            rows.append(((0.0, 0.0, 0.0), tuple(np.float64(v) / np.float64(n) for v in al.intensity)))
    lights = (rtc.LightDesc * len(rows))()
    for d, (p, i) in zip(lights, rows):
        d.position[:], d.intensity[:] = p, i
    world = dataclasses.replace(tables, lights=lights, area_lights=None)
    first = len(tables.lights)
    out = np.zeros((len(rays), 3))
    shadow = 0
    for r in range(len(rays)):
        for s, pos in enumerate(samples):
            lights[first + s].position[:] = pos[r].tolist()
        c, st = oracle.color_at(world, rays[r:r + 1], 0)
        out[r] = c[0]
        shadow += st["shadow"]
    return out, shadow


def test_hashed_jitter_of_primary_hits_is_the_oracle_under_each_rays_own_samples(gpu_ctx, rtc, oracle):
    """An opaque world.  512 batch rays (ray_id = the index in the batch) and a 32 x 16 frame (ray_id =
    y * W + x, the camera rays formed as tests/test_gpu_trace_rays.py forms them).  `remaining` is the
    primary ray's: 0 at depth 0, 3 at depth 3 -- where the oracle's colour at depth 0 is still the
    reference, since in this world a depth-3 render is the depth-0 render bit for bit (no child is ever
    made, as the counters show)."""
    from test_gpu_trace_rays import camera_rays
    t = AW.opaque(jitter=True, size=AW.SMALL)
    gpu_ctx.upload(t)
    rays = AW.seeded_rays(512, 5)
    want, shadow = _expected(rtc, oracle, t, rays, np.arange(512), 0)
    got, st = gpu_ctx.trace_rays(rays, 0, precision="f64")
    print(f"hashed batch: max |err| {_err(got, want):.3g}")
    assert _err(got, want) <= TOL and st["shadow"] == shadow and st["shaded"] > 250
    got, st = gpu_ctx.color_at(rays, 0, precision="f64")
    assert _err(got, want) <= TOL and st["shadow"] == shadow
    cam = t.camera
    crays = camera_rays(cam)
    ids = np.arange(cam.width * cam.height)
    for depth in (0, 3):
        want, shadow = _expected(rtc, oracle, t, crays, ids, depth)
        img, st = gpu_ctx.render(cam, depth, precision="f64")
        print(f"hashed frame depth {depth}: max |err| {_err(img.reshape(-1, 3), want):.3g}")
        assert _err(img.reshape(-1, 3), want) <= TOL and st["shadow"] == shadow
        assert st["reflect"] == 0 and st["refract"] == 0
    # the oracle at depth 3 is the oracle at depth 0 in this world (under the unjittered lights, which it can render)
    flat = AW.unjittered(t).expanded()
    a, sa = oracle.render(flat, cam, 0)
    b, sb = oracle.render(flat, cam, 3)
    assert a.tobytes() == b.tobytes() and _counts(sa) == _counts(sb) and sb["reflect"] == 0 and sb["refract"] == 0
    # the jitter moves the penumbra: the frame differs from the unjittered one
    gpu_ctx.upload(AW.unjittered(t))
    plain, _ = gpu_ctx.render(cam, 0, precision="f64")
    assert float((np.abs(plain - img).max(axis=2) > 1e-3).mean()) > 0.05


def test_a_reflected_ray_hashes_its_own_remaining_and_its_primary_rays_id(gpu_ctx, rtc, oracle):
    """256 rays onto a mirror plane at y = 0 at depth 1: the primary ray's colour under the jitter of
    remaining = 1 plus reflectiveness x the reflected ray's colour under the jitter of remaining = 0 with the
    same ray_id; the reflected ray runs from p + n EPSILON along reflect(d, n)."""
    t = AW.mirror_plane()
    rays = AW.plane_rays(256)
    o, d = rays[:, :3], rays[:, 3:]
    tt = -o[:, 1] / d[:, 1]
    p = o + d * tt[:, None]
    n = np.array([0.0, 1.0, 0.0])
    over = p + n * EPSILON
    refl = d - n * (2.0 * (d @ n))[:, None]
    ids = np.arange(256)
    first, _ = _expected(rtc, oracle, t, rays, ids, 1)
    second, _ = _expected(rtc, oracle, t, np.ascontiguousarray(np.concatenate([over, refl], axis=1)), ids, 0)
    reflectiveness = t.materials[0].reflectiveness
    assert reflectiveness == 0.6
    want = first + reflectiveness * second
    gpu_ctx.upload(t)
    got, ht, shape, st = gpu_ctx.trace_rays(rays, 1, precision="f64", hits=True)
    assert (shape == 0).all() and st["reflect"] == 256  # every ray meets the plane first
    print(f"remaining: max |err| {_err(got, want):.3g}; reflected rays that hit: {int((np.abs(second).max(axis=1) > 0).sum())}")
    assert (np.abs(second).max(axis=1) > 0).sum() > 20
    assert _err(got, want) <= TOL
    # with remaining = 1 for the reflected ray too the expectation is another one
    wrong, _ = _expected(rtc, oracle, t, np.ascontiguousarray(np.concatenate([over, refl], axis=1)), ids, 1)
    assert _err(first + reflectiveness * wrong, want) > 1e-4
    got, _ = gpu_ctx.color_at(rays, 1, precision="f64")  # the pool kernel: fixed-point sums of 2^-48
    assert _err(got, want) <= TOL


# ------------------------------------------------------------------ 5: consistency, bit for bit
def _assembled(rtc, ctx, cam, depth, precision, shards=2):
    shard_of, strip_row = rtc.shard_row_map(cam.height, shards)
    strips = [ctx.render(cam, depth, precision=precision, shard=(s, shards))[0] for s in range(shards)]
    return np.stack([strips[shard_of[y]][strip_row[y]] for y in range(cam.height)])


def _own_camera_rays(rtc, ctx, cam, precision):
    """The frame kernel's own camera rays: RT_FLAG_NO_TRACE stores each pixel's direction."""
    dirs, _ = ctx.render(cam, 0, precision=precision, flags=rtc.RT_FLAG_NO_TRACE)
    dtype = np.float32 if precision == "f32" else np.float64
    origin = np.array(cam.origin[:], dtype=np.float64).astype(dtype)
    d = dirs.reshape(-1, 3).astype(dtype)
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(origin, d.shape), d], axis=1).astype(np.float64))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_hashed_frames_shards_and_ray_batches_agree_bit_for_bit(gpu_ctx, rtc, precision):
    t = AW.opaque(jitter=True)
    cam = t.camera
    gpu_ctx.upload(t)
    frame, st = gpu_ctx.render(cam, 2, precision=precision)
    assert np.array_equal(_assembled(rtc, gpu_ctx, cam, 2, precision), frame)
    rays = _own_camera_rays(rtc, gpu_ctx, cam, precision)
    got, rst = gpu_ctx.trace_rays(rays, 2, precision=precision)
    assert np.array_equal(got.reshape(frame.shape).astype(frame.dtype), frame)
    assert _counts(rst) == _counts(st)
    m = AW.mirror(jitter=True)  # the pool kernel's shards
    gpu_ctx.upload(m)
    frame, _ = gpu_ctx.render(cam, 3, precision=precision)
    assert np.array_equal(_assembled(rtc, gpu_ctx, cam, 3, precision), frame)


def _f64_results(ctx, tables, depth, rays, flags=0):
    img, st = ctx.render(tables.camera, depth, precision="f64", flags=flags)
    got, rst = ctx.trace_rays(rays, depth, precision="f64", flags=flags)
    return img, _counts(st), got, _counts(rst)


@pytest.mark.parametrize("key", ["opaque", "mirror"])
def test_skips_the_light_cull_and_a_second_run_change_no_bit(rtc, monkeypatch, key):
    t = {"opaque": AW.opaque, "mirror": AW.mirror}[key](jitter=True)
    depth = 0 if key == "opaque" else 3
    rays = AW.seeded_rays(2048, 8)
    with rtc.Context(0) as c:
        c.upload(t)
        want = _f64_results(c, t, depth, rays)
        again = _f64_results(c, t, depth, rays)
        skips = _f64_results(c, t, depth, rays, rtc.RT_FLAG_NO_SKIPS)
    monkeypatch.setenv("RTC_DEBUG", "area_cull=0")
    with rtc.Context(0) as c:
        c.upload(t)
        no_cull = _f64_results(c, t, depth, rays)
    monkeypatch.delenv("RTC_DEBUG")
    for what, other in (("a second run", again), ("RT_FLAG_NO_SKIPS", skips), ("area_cull=0", no_cull)):
        assert np.array_equal(other[0], want[0]) and np.array_equal(other[2], want[2]), what
        assert other[1] == want[1] and other[3] == want[3], what


# ------------------------------------------------------------------ 6: f32
def f32_parity(ctx):
    """{world: (area upload's share, expansion's share)} of f32 frame pixels within 2/255 of the f64 device
    frame of the same upload, 64 x 32."""
    out = {}
    for key, depth in (("opaque", 0), ("mirror", 4)):
        t = _world(key)
        shares = []
        for tables in (t, t.expanded()):
            ctx.upload(tables)
            f64, _ = ctx.render(t.camera, depth, precision="f64")
            f32, _ = ctx.render(t.camera, depth, precision="f32")
            shares.append(M.share_within(f32.astype(np.float64), f64))
        out[key] = tuple(shares)
    return out


def test_f32_reaches_the_share_its_expansion_reaches(gpu_ctx):
    """The yardstick is the expansion's own f32 against its f64 on the same world, less one pixel of the
    64 x 32 frame (0.0005): shadow-edge decisions flip alike in both."""
    shares = f32_parity(gpu_ctx)
    for key, (area, expansion) in shares.items():
        print(f"{key}: area upload {area:.6f}, expansion {expansion:.6f} ({round(area * 2048)} and {round(expansion * 2048)} of 2048)")
    for key, (area, expansion) in shares.items():
        assert area >= expansion - F32A.MARGIN, (key, area, expansion)
        assert area >= F32A.FLOORS[key], (key, area, F32A.FLOORS[key])


def test_f32_floors_are_the_recorded_expansion_shares_less_the_margin():
    rec = json.load(open(os.path.join(ROOT, "profiles", "area_light_parity.json")))
    for key, floor in F32A.FLOORS.items():
        assert floor == pytest.approx(rec["worlds"][key]["expansion"] - F32A.MARGIN, abs=1e-6), key


# ------------------------------------------------------------------ 7: brightness
def test_an_area_light_counts_as_a_point_light_of_its_intensity(gpu_ctx, rtc):
    cam = AW.eye(AW.SMALL)
    refused = None
    for intensity in (1e3, 1e6, 1e9, 1e12, 1e15):
        gpu_ctx.upload(AW.bright(intensity, area=False))
        try:
            gpu_ctx.render(cam, 4, precision="f32")
        except rtc.RenderError as e:
            refused = (intensity, str(e))
            break
    assert refused is not None, "no intensity up to 1e15 is refused for the point light"
    gpu_ctx.upload(AW.bright(refused[0]))
    with pytest.raises(rtc.RenderError) as e:
        gpu_ctx.render(cam, 4, precision="f32")
    assert str(e.value) == refused[1]
    gpu_ctx.upload(AW.bright(1.0))
    img, st = gpu_ctx.render(cam, 4, precision="f32")
    assert np.isfinite(img).all() and img.max() > 0.1 and st["shadow"] == 16 * st["shaded"]


# ------------------------------------------------------------------ 8: status
def test_status_says_the_area_build_ran(rtc):
    t = _world("opaque")
    with rtc.Context(0) as c:
        c.set_jit(rtc.RT_JIT_SYNC)
        c.upload(t)
        assert c.light_info() == {"area_lights": 2, "samples": 20, "ran_area": 0, "area_bytes": 352}
        c.render(t.camera, 0, precision="f32")
        js = c.jit_status()
        assert not js["used"] and "the world has area lights" in js["log"] and js["compile_ms"] == 0.0, js
        assert c.light_info()["ran_area"] == 1
        c.trace_rays(AW.seeded_rays(256, 1), 0, precision="f32")
        assert c.light_info()["ran_area"] == 1
        c.set_jit(rtc.RT_JIT_OFF)
        c.upload(t.expanded())  # a plain upload: point lights only
        assert c.light_info() == {"area_lights": 0, "samples": 0, "ran_area": 0, "area_bytes": 0}
        c.render(t.camera, 0, precision="f32")
        assert c.light_info()["ran_area"] == 0
        c.upload(t)
        c.render(t.camera, 0, precision="f64")
        assert c.light_info()["ran_area"] == 1
    with rtc.Context.multi([0]) as g:  # a group of one rank carries the records
        g.upload(t)
        assert g.light_info()["samples"] == 20
        img, st = g.render(t.camera, 0, precision="f64")
    with rtc.Context(0) as c:
        c.upload(t)
        want, wst = c.render(t.camera, 0, precision="f64")
    assert np.array_equal(img, want) and _counts(st) == _counts(wst)


# ------------------------------------------------------------------ 9: one context, every build of the kernels
WALK = ("plain", "instanced", "smooth", "textured", "area", "instanced", "area", "plain", "textured", "plain")
# world -> (ran_smooth, ran_textured, ran_area) after a launch (an area world holds the texture tables)
RAN = {"plain": (0, 0, 0), "instanced": (0, 0, 0), "smooth": (1, 0, 0), "textured": (0, 1, 0), "area": (0, 1, 1)}
_walk_cache = {}


def _walk_worlds(rtc):
    """Small worlds, one per path of an upload, with their depths; frames of 80 x 60 and 64 x 32 (no per-scene
    build starts below 64K pixels).  Each with the fresh context's frames, counters and ray batch, f32 and f64."""
    if _walk_cache:
        return _walk_cache["worlds"], _walk_cache["rays"], _walk_cache["fresh"]
    import smooth_worlds as S
    import texture_worlds as X
    worlds = {"plain": (S.box_world(rtc, smooth=False), 4), "instanced": (S.box_instances(rtc, smooth=False), 4),
              "smooth": (S.box_world(rtc), 4), "textured": (X.box_world(rtc, X.SIX, "bilinear"), 4),
              "area": (AW.mirror(), 4)}
    assert not worlds["plain"][0].instanced and worlds["instanced"][0].instanced and worlds["smooth"][0].smoothed
    assert worlds["textured"][0].textured and worlds["area"][0].lit
    rays = M.random_rays(256, 31)
    fresh = {}
    for name, (t, depth) in worlds.items():
        with rtc.Context(0) as c:
            c.upload(t)
            fresh[name] = _walk_results(c, t, depth, rays)
            assert _ran(c) == RAN[name], (name, _ran(c))
    _walk_cache.update(worlds=worlds, rays=rays, fresh=fresh)
    return worlds, rays, fresh


def _ran(ctx):
    return (ctx.smooth_info()["ran_smooth"], ctx.texture_info()["ran_textured"], ctx.light_info()["ran_area"])


def _walk_results(ctx, tables, depth, rays):
    out = []
    for precision in ("f32", "f64"):
        img, st = ctx.render(tables.camera, depth, precision=precision)
        got, rst = ctx.trace_rays(rays, depth, precision=precision)
        out.append((img.tobytes(), _counts(st), got.tobytes(), _counts(rst)))
    return out


@pytest.mark.parametrize("devices", [None, [0], [0, 1]], ids=["single", "group of one", "group of two"])
def test_one_context_walks_every_build_and_back(rtc, devices):
    """plain -> instanced -> smooth -> textured -> area -> instanced -> area -> plain -> textured -> plain on one
    context: after every upload the frames, the counters and a batch of 256 rays are the fresh context's bit for
    bit, in f32 and f64, and ran_smooth, ran_textured and ran_area say which kernels ran.  On a group of two the
    other rank takes its kernels from the header."""
    if devices and len(devices) > rtc.device_count():
        pytest.skip("fewer than two devices are visible")
    worlds, rays, fresh = _walk_worlds(rtc)
    with (rtc.Context.multi(devices) if devices else rtc.Context(0)) as c:
        for step, name in enumerate(WALK):
            t, depth = worlds[name]
            c.upload(t)
            got = _walk_results(c, t, depth, rays)
            for precision, g, w in zip(("f32", "f64"), got, fresh[name]):
                assert g[0] == w[0], (step, name, precision, "frame")
                assert g[1] == w[1], (step, name, precision, "frame counters")
                assert g[2] == w[2], (step, name, precision, "rays")
                assert g[3] == w[3], (step, name, precision, "ray counters")
            assert _ran(c) == RAN[name], (step, name, _ran(c))


# ------------------------------------------------------------------ the CLI
def test_cli_area_light(rtc, tmp_path):
    import ctypes as C
    import subprocess

    from rtc_amd import world as W
    from test_cli import CLI, SCENE
    yaml = tmp_path / "scene.yaml"
    yaml.write_text(SCENE)
    out = tmp_path / "out.png"
    r = subprocess.run([CLI, str(yaml), str(out), "--area-light", "-2,5,-3:2,0,0:0,0.5,2:4x3:0.5,0.5,0.4:jitter=9",
                        "--area-light", "1,4,-2:1,0,0:0,0,1:2x2", "--precision", "f64", "--width", "80", "--height", "60"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    scene = rtc.load_scene(str(yaml))
    cam = rtc.camera_resize(scene.camera, 80, 60)
    tables = AW.with_area(scene, [W.AreaLight((-2, 5, -3), (2, 0, 0), (0, 0.5, 2), 4, 3, (0.5, 0.5, 0.4), True, 9),
                                  W.AreaLight((1, 4, -2), (1, 0, 0), (0, 0, 1), 2, 2)])
    with rtc.Context(0) as c:
        c.upload(tables)
        assert c.light_info()["samples"] == 16
        want, _ = c.render(cam, 6, precision="f64", out_format="u8")
        c.upload(scene)
        plain, _ = c.render(cam, 6, precision="f64", out_format="u8")
    ref = tmp_path / "ref.png"
    assert rtc._lib.rt_image_write(str(ref).encode(), want.ctypes.data_as(C.c_void_p), 80, 60) == rtc.RT_OK
    assert out.read_bytes() == ref.read_bytes() and not np.array_equal(want, plain)
