"""Mesh instances on the GPU: worlds uploaded with
rt_scene_upload_instanced (tests/instance_worlds.py) against the flat world
they mean, tables.expanded(): rendered by the f64 oracle, or uploaded through
rt_scene_upload on the same kind of context.

  1. f64 frames within 1e-9 of the oracle's frame of the expansion, counters equal;
  2. worlds with value-equal triangles: those instances are uploaded expanded;
  3. every entry point returns the expansion's bytes, counters and hit indices;
  4. no per-scene build for an instanced world; n_instances = 0 is rt_scene_upload;
  5. instance tables reused on one context;
  6. a group context of one rank;
  7. the CLI's --instance.

Frames are 80 x 60 (mesh_worlds.FRAME).
"""
import numpy as np
import pytest

import instance_worlds as I
import mesh_worlds as M

pytestmark = pytest.mark.gpu

ABS64 = 1e-9  # the project's f64 bar
COUNTERS = ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned", "refract_evals", "schlick_evals")


def _counts(st):
    return {k: st[k] for k in COUNTERS}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint8 else a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def worlds(rtc, tmp_path_factory):
    """Every world: (instanced tables, the expansion, depth, the oracle's frame of the expansion and its counters)."""
    import pyoracle
    tmp = tmp_path_factory.mktemp("instances")
    out = {}
    for key in I.WORLDS + list(I.VALUE_EQUAL):
        tables, depth = I.build_world(rtc, tmp, key)
        flat = tables.expanded()
        ref, rst = pyoracle.render(flat, flat.camera, depth, threads=8)
        ref.setflags(write=False)
        out[key] = (tables, flat, depth, ref, rst)
    return out


def _against_oracle(ctx, key, tables, depth, ref, rst):
    img, st = ctx.render(tables.camera, depth, precision="f64")
    err = np.abs(img - ref).max(axis=2)
    err = np.where(np.isfinite(err), err, np.inf)
    y, x = np.unravel_index(int(err.argmax()), err.shape)
    print(f"{key}: {ctx.instance_info()}, f64 max |err| {err[y, x]:.3g}")
    assert err[y, x] < ABS64, f"{int((err >= ABS64).sum())} px differ, worst ({x}, {y})"
    assert _counts(st) == _counts(rst)
    return st


# ------------------------------------------------------------ 1: f64 frames against the oracle
@pytest.mark.parametrize("key", I.WORLDS)
def test_f64_frame_matches_oracle_of_the_expansion(gpu_ctx, worlds, key):
    tables, flat, depth, ref, rst = worlds[key]
    gpu_ctx.upload(tables)
    info = gpu_ctx.instance_info()
    assert info["instances"] == len(tables.instances) and info["meshes"] == len(tables.meshes), info
    assert info["expanded"] == 0, "no world of this test may pass by falling back to plain records"
    assert info["local_records"] == sum(len(m) for m in tables.meshes)
    assert info["instanced_bytes"] > 0 and info["expansion_bytes"] > 0
    st = _against_oracle(gpu_ctx, key, tables, depth, ref, rst)
    if key == "nested_glass":
        assert st["refract"] > 0 and st["reflect"] > 0  # the pool kernel and the containers walk ran
    if key == "beside_plain":
        tree = gpu_ctx.tree_info()  # the plain run keeps its own tree
        assert tree["nodes"] > 0 and tree["records_in_tree"] == 512, tree


def test_of_equal_t_the_lower_world_index_wins(gpu_ctx, worlds):
    tables, flat, depth, _, _ = worlds["coincident"]
    gpu_ctx.upload(tables)
    rays = np.ascontiguousarray(_camera_rays(tables.camera))
    _, t, shape, _ = gpu_ctx.trace_rays(rays, 0, precision="f64", hits=True)
    on_mesh = shape >= 2
    assert on_mesh.sum() > 200 and (shape[on_mesh] < 2 + 576).all(), "the second instance (higher indices) never wins"


def _camera_rays(cam):
    """The camera's own rays (camera.rs ray_for_pixel in f64), (W * H, 6)."""
    inv = np.array(cam.inverse[:]).reshape(4, 4)
    xs, ys = np.meshgrid(np.arange(cam.width), np.arange(cam.height))
    wx = cam.half_width - (xs + 0.5) * cam.pixel_size
    wy = cam.half_height - (ys + 0.5) * cam.pixel_size
    p = np.stack([wx, wy, -np.ones_like(wx), np.ones_like(wx)], axis=-1).reshape(-1, 4)
    pixel = (p @ inv.T)[:, :3]
    origin = (np.array([0.0, 0.0, 0.0, 1.0]) @ inv.T)[:3]
    d = pixel - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(origin, d.shape), d], axis=1))


# ------------------------------------------------------------ 2: value-equal worlds
@pytest.mark.parametrize("key", list(I.VALUE_EQUAL))
def test_value_equal_instances_are_uploaded_expanded(gpu_ctx, worlds, key):
    tables, flat, depth, ref, rst = worlds[key]
    gpu_ctx.upload(tables)
    info = gpu_ctx.instance_info()
    assert info["expanded"] == I.VALUE_EQUAL[key] and info["instances"] == 2, info
    st = _against_oracle(gpu_ctx, key, tables, depth, ref, rst)
    assert st["refract"] > 0


# ------------------------------------------------------------ 3: bit identity with the expansion
def _all_results(ctx, rtc, tables, depth, rays, flags=0):
    cam = tables.camera
    out = {}
    for precision in ("f32", "f64"):
        out[f"render {precision}"] = ctx.render(cam, depth, precision=precision, flags=flags)
        out[f"shard {precision}"] = ctx.render(cam, depth, precision=precision, shard=(1, 2), flags=flags)
        out[f"supersampled {precision}"] = ctx.render_supersampled(cam, 2, depth, precision=precision, flags=flags)
        rgb, t, shape, st = ctx.trace_rays(rays, depth, precision=precision, hits=True, flags=flags)
        out[f"trace_rays {precision}"] = (np.concatenate([rgb, t[:, None]], axis=1), st)
        out[f"hit shapes {precision}"] = (shape.astype(np.float64), st)
        if not flags:  # (rt_color_at takes no flags; in a world with secondary rays it takes unit directions only)
            unit = rays.copy()
            unit[:, 3:] /= np.linalg.norm(unit[:, 3:], axis=1, keepdims=True)
            out[f"color_at {precision}"] = ctx.color_at(unit, depth, precision=precision)
    out["render u8"] = ctx.render(cam, depth, precision="f32", out_format="u8", flags=flags)
    return out


@pytest.mark.parametrize("knob", [None, "cull=0", "tri_tree=0"])
@pytest.mark.parametrize("key", ["three_tori", "nested_glass", "repeated", "beside_plain"])
def test_every_entry_point_returns_the_expansions_bytes(rtc, worlds, monkeypatch, key, knob):
    tables, flat, depth, _, _ = worlds[key]
    rays = M.random_rays(2048, 4321)
    if knob:
        monkeypatch.setenv("RTC_DEBUG", knob)
    with rtc.Context(0) as c:
        for flags in (0, rtc.RT_FLAG_NO_SKIPS):
            c.upload(tables)
            assert c.instance_info()["instances"] == len(tables.instances)
            got = _all_results(c, rtc, tables, depth, rays, flags)
            c.upload(flat)
            assert c.instance_info()["instances"] == 0
            want = _all_results(c, rtc, flat, depth, rays, flags)
            for what, (a, sa) in got.items():
                b, sb = want[what]
                diff = np.argwhere(_bits(a) != _bits(b))
                assert len(diff) == 0, f"{knob} flags {flags} {what}: {len(diff)} values differ, first at {tuple(diff[0])}"
                assert _counts(sa) == _counts(sb), f"{knob} flags {flags} {what}"
            hit = got["hit shapes f64"][0]
            assert (hit >= 2).sum() > 50, "rays must reach the instances"


# ------------------------------------------------------------ 4: per-scene builds
def test_an_instanced_world_takes_no_per_scene_build(rtc, worlds):
    tables, flat, depth, _, _ = worlds["small"]
    with rtc.Context(0) as c:
        c.set_jit(rtc.RT_JIT_SYNC)
        c.upload(tables)
        c.render(tables.camera, depth, precision="f32")
        js = c.jit_status()
        assert not js["used"] and "mesh instances" in js["log"], js
        assert js["compile_ms"] == 0.0


def test_no_instances_is_rt_scene_upload_itself(rtc):
    tables = I.world([], [])
    assert not tables.instanced
    with rtc.Context(0) as a, rtc.Context(0) as b:
        for c in (a, b):
            c.set_jit(rtc.RT_JIT_SYNC)
        a.upload(tables)
        rc = rtc._lib.rt_scene_upload_instanced(b._h, *tables.instanced_args())
        assert rc == rtc.RT_OK, rtc._lib.rt_last_error()
        assert all(v == 0 for v in b.instance_info().values())
        for precision in ("f32", "f64"):
            x, sx = a.render(tables.camera, 3, precision=precision)
            y, sy = b.render(tables.camera, 3, precision=precision)
            assert np.array_equal(_bits(x), _bits(y)) and _counts(sx) == _counts(sy)
        a.render(tables.camera, 3, precision="f32")
        b.render(tables.camera, 3, precision="f32")
        # per-scene builds still apply to it
        assert a.jit_status()["used"] and b.jit_status()["used"], (a.jit_status(), b.jit_status())


# ------------------------------------------------------------ 5: table reuse on one context
def test_tables_are_reused_across_uploads(rtc, worlds, tmp_path):
    from rtc_amd import world as W
    big = M.world(W.mesh(M.load(rtc, tmp_path, "ico3"), transform=W.translation(0, 0.35, 0), bake=True))
    tables, flat, depth, _, _ = worlds["three_tori"]
    other, _, other_depth, _, _ = worlds["nested_glass"]

    def fresh(t, d):
        with rtc.Context(0) as c:
            c.upload(t)
            return [c.render(t.camera, d, precision=p) for p in ("f32", "f64")]

    want = {"big": fresh(big, 3), "tori": fresh(tables, depth), "glass": fresh(other, other_depth)}
    with rtc.Context(0) as c:
        for name, t, d in (("big", big, 3), ("tori", tables, depth), ("glass", other, other_depth), ("big", big, 3),
                           ("tori", tables, depth)):
            c.upload(t)
            for (a, sa), p in zip(want[name], ("f32", "f64")):
                b, sb = c.render(t.camera, d, precision=p)
                assert np.array_equal(_bits(a), _bits(b)) and _counts(sa) == _counts(sb), (name, p)


# ------------------------------------------------------------ 6: a group context of one rank
def test_group_of_one_rank_carries_the_instances(gpu_ctx, rtc, worlds):
    tables, flat, depth, _, _ = worlds["three_tori"]
    gpu_ctx.upload(tables)
    want = gpu_ctx.instance_info()
    with rtc.Context.multi([0]) as g:
        g.upload(tables)
        info = g.instance_info()
        assert {k: v for k, v in info.items() if k != "build_ms"} == {k: v for k, v in want.items() if k != "build_ms"}
        for precision in ("f32", "f64"):
            a, sa = gpu_ctx.render(tables.camera, depth, precision=precision)
            b, sb = g.render(tables.camera, depth, precision=precision)
            assert np.array_equal(_bits(a), _bits(b)) and _counts(sa) == _counts(sb), precision


# ------------------------------------------------------------ 7: the CLI's --instance
def test_cli_instance_places_copies_of_one_mesh(rtc, tmp_path):
    """`rtc scene.yaml out.png --instance FILE:tx,ty,tz[:s]` renders the PNG of the same scene with the copies
    written out as triangles (rt_mesh_triangles with the placement, bake = 0) after its shapes."""
    import ctypes as C
    import subprocess
    from test_cli import CLI, SCENE
    from rtc_amd import world as W
    yaml = tmp_path / "scene.yaml"
    yaml.write_text(SCENE)
    obj = tmp_path / "ico.obj"
    obj.write_text(M.obj_text(*M.icosphere(2)))
    octa = tmp_path / "octa.obj"
    octa.write_text(I.OCTA)
    places = [(obj, (-1.6, 1.1, 1.0), 0.6), (octa, (0.4, 1.6, 1.5), 1.0), (obj, (0.5, 0.4, -0.5), 0.25)]
    args = []
    for path, t, s in places:
        args += ["--instance", f"{path}:{t[0]!r},{t[1]!r},{t[2]!r}" + ("" if s == 1.0 else f":{s!r}")]
    out = tmp_path / "out.png"
    common = ["--precision", "f64", "--width", "80", "--height", "60"]
    r = subprocess.run([CLI, str(yaml), str(out)] + common + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("320 triangles") == 1 and r.stdout.count("8 triangles") == 1, "each file is loaded once"
    # the same world written out: the scene's shapes, then every copy's triangles on one default material
    scene = rtc.load_scene(str(yaml))
    n, nm = len(scene.shapes), len(scene.materials)
    copies = [rtc.load_obj(str(path)).shape_descs(
        [v for row in W.mat_mul(W.translation(*t), W.scaling(s, s, s)) for v in row], False, nm) for path, t, s in places]
    shapes = (rtc.ShapeDesc * (n + sum(len(c) for c in copies)))()
    C.memmove(shapes, scene.shapes, n * C.sizeof(rtc.ShapeDesc))
    at = n
    for c in copies:
        C.memmove(C.byref(shapes, at * C.sizeof(rtc.ShapeDesc)), c, len(c) * C.sizeof(rtc.ShapeDesc))
        at += len(c)
    mats = (rtc.MaterialDesc * (nm + 1))()
    C.memmove(mats, scene.materials, nm * C.sizeof(rtc.MaterialDesc))
    mats[nm] = W.World([], [W.sphere()]).tables().materials[0]  # Material::default as the tables hold it
    cam = rtc.camera_resize(scene.camera, 80, 60)
    with rtc.Context(0) as c:
        c.upload(rtc.SceneTables(shapes, mats, scene.patterns, scene.lights, cam))
        want, _ = c.render(cam, 6, precision="f64", out_format="u8")
        bare = rtc.SceneTables(scene.shapes, scene.materials, scene.patterns, scene.lights, cam)
        c.upload(bare)
        without, _ = c.render(cam, 6, precision="f64", out_format="u8")
    assert (want != without).any(axis=2).mean() > 0.02, "the copies must be in the picture"
    ref = tmp_path / "ref.png"
    assert rtc._lib.rt_image_write(str(ref).encode(), want.ctypes.data_as(C.c_void_p), 80, 60) == rtc.RT_OK
    assert out.read_bytes() == ref.read_bytes()
    for bad in ("ico.obj", f"{obj}:1,2", f"{obj}:1,2,3:x"):
        assert subprocess.run([CLI, str(yaml), str(out), "--instance", bad], capture_output=True).returncode == 2
    r = subprocess.run([CLI, str(yaml), str(out), "--instance", f"{tmp_path / 'none.obj'}:0,0,0"], capture_output=True,
                       text=True)
    assert r.returncode == 1 and "none.obj" in r.stderr
