"""Mesh worlds on the GPU: OBJ meshes (tests/mesh_worlds.py) loaded through
rtc_amd.load_obj and world.mesh, rendered by kernels that walk the triangle
hierarchy, against the f64 oracle, which tests every triangle
by brute force.

  1. f64 frames within 1e-9 of oracle.render, every counter equal;
  2. the hierarchy, the cull and the skips change no bit and no counter;
  3. 2048 incoherent rays against oracle.color_at;
  4. dyadic rays through the height field's edges and vertices;
  5. f32 frames and rays against the oracle (floors from the measured minima);
  6. a group context of one rank.

Frames are 80 x 60 (partial tiles); no frame reaches the size at which a
per-scene build would start.
"""
import json
import os

import numpy as np
import pytest

import mesh_worlds as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

ABS64 = 1e-9
COUNTERS = ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned", "refract_evals", "schlick_evals")
# Share of pixels (of rays) whose f32 colour is within 2/255 of the oracle's: the minima of the measuring run
# (profiles/mesh_parity.json, written by scripts/mesh_parity.py on the GPU) less 0.005, DESIGN.md §3.7's rule.
PARITY = json.load(open(os.path.join(ROOT, "profiles", "mesh_parity.json")))
F32_FRAME_FLOOR = PARITY["frames_min"] - 0.005
F32_RAYS_FLOOR = PARITY["rays_min"] - 0.005


def _counts(st):
    return {k: st[k] for k in COUNTERS}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


WORLDS = M.WORLDS


@pytest.fixture(scope="module")
def worlds(rtc, tmp_path_factory):
    """Every world with its oracle frame and counters, computed once."""
    import pyoracle
    tmp = tmp_path_factory.mktemp("meshes")
    out = {}
    for key in WORLDS:
        tables, depth = M.build_world(rtc, tmp, key)
        ref, rst = pyoracle.render(tables, tables.camera, depth, threads=8)
        ref.setflags(write=False)
        out[key] = (tables, depth, ref, rst)
    return out


def _has_tree(ctx, records):
    info = ctx.tree_info()
    assert info["nodes"] > 0 and info["leaves"] > 0 and info["depth"] >= 3, info
    assert info["records_in_tree"] == records and info["records_outside"] == 0, info
    return info


# ------------------------------------------------------------ 1: parity with the oracle
@pytest.mark.parametrize("key", WORLDS)
def test_f64_frame_matches_oracle(gpu_ctx, worlds, key):
    tables, depth, ref, rst = worlds[key]
    gpu_ctx.upload(tables)
    info = _has_tree(gpu_ctx, len(tables.shapes) - 2)
    img, st = gpu_ctx.render(tables.camera, depth, precision="f64")
    err = np.abs(img - ref).max(axis=2)
    err = np.where(np.isfinite(err), err, np.inf)
    y, x = np.unravel_index(int(err.argmax()), err.shape)
    print(f"{key}: {len(tables.shapes)} shapes, tree {info}, f64 max |err| {err[y, x]:.3g}")
    assert err[y, x] < ABS64, f"{int((err >= ABS64).sum())} px differ, worst ({x}, {y})"
    assert _counts(st) == _counts(rst)
    if key in ("glass", "doubled"):
        assert st["refract"] > 0 and st["reflect"] > 0  # the pool kernel and the walk ran


def test_of_equal_t_the_lower_world_index_wins(gpu_ctx, worlds):
    tables, depth, ref, _ = worlds["doubled"]
    gpu_ctx.upload(tables)
    rays = np.array([[0.0, 0.1, -4.0, 0.0, 0.0, 1.0]])
    _, t, shape, _ = gpu_ctx.trace_rays(rays, 0, precision="f64", hits=True)
    assert 2 <= shape[0] < 2 + 320, "of two value-equal faces at one t the first in world order is the hit"
    tables, depth, ref, _ = worlds["coincident"]
    gpu_ctx.upload(tables)
    cam = tables.camera
    _, t, shape, _ = gpu_ctx.trace_rays(_camera_rays(cam), 0, precision="f64", hits=True)
    on_mesh = shape >= 2
    assert on_mesh.sum() > 200 and (shape[on_mesh] < 2 + 576).all(), "the coincident copy (higher index) never wins"


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


# ------------------------------------------------------------ 2: acceleration only
def _all_results(ctx, rtc, tables, depth, precision, rays, flags=0):
    cam = tables.camera
    out = {}
    out["render"] = ctx.render(cam, depth, precision=precision, flags=flags)
    out["supersampled"] = ctx.render_supersampled(cam, 2, depth, precision=precision, flags=flags)
    rgb, t, shape, st = ctx.trace_rays(rays, depth, precision=precision, hits=True, flags=flags)
    out["trace_rays"] = (np.concatenate([rgb, t[:, None], shape[:, None].astype(np.float64)], axis=1), st)
    if not flags:  # (rt_color_at takes no flags)
        out["color_at"] = ctx.color_at(rays, depth, precision=precision)
    return out


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("key", ["field", "glass", "doubled"])
def test_tree_cull_and_skips_change_nothing(gpu_ctx, rtc, worlds, monkeypatch, key, precision):
    tables, depth, _, _ = worlds[key]
    rays = np.ascontiguousarray(_camera_rays(tables.camera)[::3])
    gpu_ctx.upload(tables)
    _has_tree(gpu_ctx, len(tables.shapes) - 2)
    base = _all_results(gpu_ctx, rtc, tables, depth, precision, rays)
    variants = {"RT_FLAG_NO_SKIPS": _all_results(gpu_ctx, rtc, tables, depth, precision, rays, rtc.RT_FLAG_NO_SKIPS)}
    for knob in ("tri_tree=0", "cull=0"):
        monkeypatch.setenv("RTC_DEBUG", knob)
        with rtc.Context(0) as c:
            c.upload(tables)
            assert all(v == 0 for v in c.tree_info().values()), (knob, c.tree_info())
            variants[knob] = _all_results(c, rtc, tables, depth, precision, rays)
        monkeypatch.delenv("RTC_DEBUG")
    for name, got in variants.items():
        for what, (a, sa) in got.items():
            b, sb = base[what]
            diff = np.argwhere(_bits(a) != _bits(b))
            assert len(diff) == 0, f"{name} {what}: {len(diff)} values differ, first at {tuple(diff[0])}"
            assert _counts(sa) == _counts(sb), f"{name} {what}"


def test_a_tree_world_takes_no_per_scene_build(rtc, worlds):
    tables, depth, _, _ = worlds["ico2"]
    with rtc.Context(0) as c:
        c.set_jit(rtc.RT_JIT_SYNC)
        c.upload(tables)
        a, sa = c.render(tables.camera, depth, precision="f32")
        js = c.jit_status()
        assert not js["used"] and "triangle hierarchy" in js["log"], js
        assert js["compile_ms"] == 0.0


def test_small_triangle_worlds_keep_the_flat_loop(gpu_ctx, rtc, tmp_path):
    """Fewer bounded triangles than kTriTreeMin: no tree, and the frame is the oracle's."""
    import pyoracle
    from rtc_amd import world as W
    mesh = rtc.load_obj(M.obj_text(*M.height_field(2)))  # 8 triangles
    tables = M.world(W.mesh(mesh, transform=W.scaling(0.5, 1, 0.5)))
    gpu_ctx.upload(tables)
    assert all(v == 0 for v in gpu_ctx.tree_info().values())
    img, st = gpu_ctx.render(tables.camera, 2, precision="f64")
    ref, rst = pyoracle.render(tables, tables.camera, 2, threads=8)
    assert np.abs(img - ref).max() < ABS64 and _counts(st) == _counts(rst)


# ------------------------------------------------------------ 3: incoherent rays
def _incoherent(gpu_ctx, oracle, worlds, key):
    tables, depth, _, _ = worlds[key]
    rays = M.random_rays(2048, 1234)
    ref, rst = oracle.color_at(tables, rays, depth)
    gpu_ctx.upload(tables)
    _has_tree(gpu_ctx, len(tables.shapes) - 2)
    got, st = gpu_ctx.trace_rays(rays, depth, precision="f64")
    assert _counts(st) == _counts(rst)
    return tables, depth, rays, ref, got


@pytest.mark.parametrize("key", ["ico3", "torus", "field"])
def test_incoherent_rays(gpu_ctx, oracle, worlds, key):
    """2048 seeded rays from a box around the mesh, directions uniform on the sphere, |d| from U(0.5, 1.25), in
    the opaque mesh worlds: f64 within 1e-9 of oracle.color_at, counters equal."""
    tables, depth, rays, ref, got = _incoherent(gpu_ctx, oracle, worlds, key)
    err = np.abs(got - ref).max(axis=1)
    err = np.where(np.isfinite(err), err, np.inf)
    k = int(err.argmax())
    print(f"{key}: f64 max |err| {err[k]:.3g}, max |oracle| {np.abs(ref).max():.3g}")
    assert err[k] < ABS64, f"{int((err >= ABS64).sum())} rays differ; worst {rays[k]} got {got[k]} oracle {ref[k]}"
    if key == "ico3":
        got32, _ = gpu_ctx.trace_rays(rays, depth, precision="f32")
        share = M.share_within(got32, ref)
        print(f"{key}: f32 rays within 2/255 of the oracle: {share:.4f} (floor {F32_RAYS_FLOOR:.4f})")
        assert share >= F32_RAYS_FLOOR


def test_incoherent_rays_through_glass(gpu_ctx, oracle, worlds):
    """The same rays in the glass world.  A direction that is not a unit vector makes the reference's refraction
    grow a colour without bound (tests/test_gpu_trace_rays.py: 6.6e23 for these lengths); here the largest is
    7.3e7, where neighbouring f64 values lie 1.5e-8 apart, so an absolute 1e-9 would ask for equal bits (measured:
    1 ray of 2048 one ulp off, 1.49e-8).  The bound is that file's: 1e-9 of max(1, |oracle|inf), which is the
    absolute 1e-9 for every colour up to 1."""
    tables, depth, rays, ref, got = _incoherent(gpu_ctx, oracle, worlds, "glass")
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))
    k = int(err.argmax())
    print(f"glass: f64 max relative err {err[k]:.3g}, max |oracle| {np.abs(ref).max():.3g}")
    assert err[k] <= ABS64, f"ray {rays[k]} got {got[k]} oracle {ref[k]}"
    got32, _ = gpu_ctx.trace_rays(rays, depth, precision="f32")
    share = M.share_within(got32, ref)
    print(f"glass: f32 rays within 2/255 of the oracle: {share:.4f} (floor {F32_RAYS_FLOOR:.4f})")
    assert share >= F32_RAYS_FLOOR


# ------------------------------------------------------------ 4: edges and vertices
def test_edges_and_vertices_of_the_height_field(gpu_ctx, rtc, oracle):
    """Vertical rays from origins on the 1/8 grid: they pass through the field's vertices (1/4 grid), its cell
    edges and its cells' diagonals, where the reference's strict v > 0 and u + v < 1 make some of them miss the
    field altogether.  Every quantity a decision hangs on is dyadic and the determinant is +-1/16, so f32 decides
    as f64 does.  The oracle has no hit query: each triangle shows an exact colour of its own (ambient 1, no
    diffuse, no specular, depth 0), which names the oracle's hit; t is then exact dyadic arithmetic."""
    from rtc_amd import world as W
    verts, faces = M.height_field(16)
    mesh = rtc.load_obj(M.obj_text(verts, faces))
    shapes = []
    for k, d in enumerate(W.mesh(mesh)):
        d.material = W.Material(color=((k % 32 + 1) / 64.0, (k // 32 + 1) / 64.0, 0.5), ambient=1.0, diffuse=0.0,
                                specular=0.0)
        shapes.append(d)
    floor = W.plane(W.Material(color=(1.0, 1.0, 1.0), ambient=1.0, diffuse=0.0, specular=0.0),
                    transform=W.translation(0, -2, 0))
    tables = W.World([W.Light((0.0, 9.0, 0.0), (1.0, 1.0, 1.0))], [floor] + shapes).tables()
    g = np.arange(-17, 18) / 8.0  # one step beyond the field on every side
    xs, zs = np.meshgrid(g, g)
    n = xs.size
    rays = np.zeros((n, 6))
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 4] = xs.ravel(), 4.0, zs.ravel(), -1.0
    ref, _ = oracle.color_at(tables, rays, 0)
    on_floor = (ref == 1.0).all(axis=1)
    want = np.where(on_floor, 0, 1 + (np.rint(ref[:, 0] * 64) - 1 + 32 * (np.rint(ref[:, 1] * 64) - 1))).astype(np.int32)
    assert (ref[~on_floor, 2] == 0.5).all() and (want[~on_floor] >= 1).all() and (want <= 512).all()
    inside = (np.abs(rays[:, 0]) < 2) & (np.abs(rays[:, 2]) < 2)
    fell_through = int((on_floor & inside).sum())
    assert fell_through > 0 and (~on_floor).sum() > 500, "the rays must both hit the field and slip through its seams"
    # exact t: the hit triangle's plane over (x, z), or the floor
    want_t = np.full(n, 6.0)
    for k in np.flatnonzero(~on_floor):
        a, b, c = verts[faces[want[k] - 1]]
        e1, e2 = b - a, c - a
        det = e1[0] * e2[2] - e1[2] * e2[0]
        px, pz = rays[k, 0] - a[0], rays[k, 2] - a[2]
        u, v = (px * e2[2] - pz * e2[0]) / det, (pz * e1[0] - px * e1[2]) / det
        want_t[k] = 4.0 - (a[1] + u * e1[1] + v * e2[1])
    gpu_ctx.upload(tables)
    _has_tree(gpu_ctx, 512)
    _, t64, s64, _ = gpu_ctx.trace_rays(rays, 0, precision="f64", hits=True)
    print(f"{n} rays: {int((~on_floor).sum())} hit the field, {fell_through} inside its outline fell through a seam")
    assert np.array_equal(s64, want), f"{int((s64 != want).sum())} rays hit another shape than the oracle's"
    assert np.array_equal(t64, want_t)
    _, t32, s32, _ = gpu_ctx.trace_rays(rays, 0, precision="f32", hits=True)
    assert np.array_equal(s32, want), f"{int((s32 != want).sum())} f32 rays decide unlike f64"
    assert np.array_equal(t32.astype(np.float64), want_t)


# ------------------------------------------------------------ 5: f32 against the oracle
@pytest.mark.parametrize("key", WORLDS)
def test_f32_frame_against_oracle(gpu_ctx, worlds, key):
    tables, depth, ref, rst = worlds[key]
    gpu_ctx.upload(tables)
    img, st = gpu_ctx.render(tables.camera, depth, precision="f32")
    share = M.share_within(img.astype(np.float64), ref)
    print(f"{key}: f32 pixels within 2/255 of the oracle: {share:.4f} (floor {F32_FRAME_FLOOR:.4f})")
    assert share >= F32_FRAME_FLOOR
    assert st["primary"] == rst["primary"]


# ------------------------------------------------------------ 6: a group context of one rank
def test_group_of_one_rank_carries_the_tree(gpu_ctx, rtc, worlds):
    tables, depth, _, _ = worlds["glass"]
    gpu_ctx.upload(tables)
    want_info = gpu_ctx.tree_info()
    with rtc.Context.multi([0]) as g:
        g.upload(tables)
        info = g.tree_info()
        assert info["nodes"] == want_info["nodes"] > 0 and info["depth"] == want_info["depth"]
        assert info["records_in_tree"] == 320
        for precision in ("f32", "f64"):
            a, sa = gpu_ctx.render(tables.camera, depth, precision=precision)
            b, sb = g.render(tables.camera, depth, precision=precision)
            assert np.array_equal(_bits(a), _bits(b)) and _counts(sa) == _counts(sb), precision


# ------------------------------------------------------------ the CLI's --obj
def test_cli_obj_appends_the_meshes(rtc, oracle, tmp_path):
    """`rtc scene.yaml out.ppm --obj a.obj --obj b.obj`: the YAML world's shapes, then each mesh's triangles
    with Material::default and no transformation, as the oracle renders that world."""
    import ctypes as C
    import subprocess
    from test_cli import CLI, SCENE, read_ppm
    yaml = tmp_path / "scene.yaml"
    yaml.write_text(SCENE)
    verts, faces = M.icosphere(2)
    paths = []
    for k, shift in enumerate(((-1.6, 1.1, 1.0), (0.4, 1.6, 1.5))):
        p = tmp_path / f"mesh{k}.obj"
        p.write_text(M.obj_text(verts * 0.6 + np.array(shift), faces))
        paths.append(str(p))
    out = tmp_path / "out.ppm"
    r = subprocess.run([CLI, str(yaml), str(out), "--precision", "f64", "--width", "80", "--height", "60",
                        "--ppm-binary", "--obj", paths[0], "--obj", paths[1]], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("320 triangles, 3 lines ignored") == 2
    scene = rtc.load_scene(str(yaml))
    n, extra = len(scene.shapes), [rtc.load_obj(p).shape_descs(material=len(scene.materials)) for p in paths]
    shapes = (rtc.ShapeDesc * (n + 640))()
    C.memmove(shapes, scene.shapes, n * C.sizeof(rtc.ShapeDesc))
    for k, d in enumerate(extra):
        C.memmove(C.byref(shapes, (n + 320 * k) * C.sizeof(rtc.ShapeDesc)), d, 320 * C.sizeof(rtc.ShapeDesc))
    mats = (rtc.MaterialDesc * (len(scene.materials) + 1))()
    C.memmove(mats, scene.materials, len(scene.materials) * C.sizeof(rtc.MaterialDesc))
    from rtc_amd import world as W
    default = W.World([], [W.sphere()]).tables().materials[0]  # Material::default as the tables hold it
    mats[len(scene.materials)] = default
    tables = rtc.SceneTables(shapes, mats, scene.patterns, scene.lights, rtc.camera_resize(scene.camera, 80, 60))
    ref, _ = oracle.render(tables, tables.camera, 6, threads=8)
    d = np.abs(read_ppm(out, b"P6").astype(int) - oracle.quantize(ref).astype(int))
    bare, _ = oracle.render(scene, tables.camera, 6, threads=8)
    assert np.abs(ref - bare).max() > 0.05, "the meshes must be in the picture"
    assert d.max() <= 1 and (d == 0).mean() >= 0.999
    assert subprocess.run([CLI, str(yaml), str(out), "--obj"], capture_output=True).returncode == 2
    r = subprocess.run([CLI, str(yaml), str(out), "--obj", str(tmp_path / "none.obj")], capture_output=True, text=True)
    assert r.returncode == 1 and "none.obj" in r.stderr
