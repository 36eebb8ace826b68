"""Smooth triangles on the GPU (worlds in tests/smooth_worlds.py).

There is no oracle for the interpolated normal, so the f64 kernels are held to
tests/smooth_reference.py (a numpy restatement of rtc.h's definition) where
the normals matter, and to the oracle's frame of the FLAT world where they
cannot: geometry, counters, and a box whose vertex normals are its faces' own.

  5. interpolation: f64 frames and ray batches equal the reference within 1e-9;
  6. geometry untouched: hits bit-identical to the flat upload, counters the oracle's;
  7. degenerate normals are flat shading through every entry point;
  8. invariance: knobs, RT_FLAG_NO_SKIPS, the expansion, baking, a group, table reuse;
  9. identity classes on the device;
 10. f32 against the f64 device frame;
 11. small shapes where the kernel can still go wrong;
 12. the CLI's --smooth.

Frames are 80 x 60 (smooth_worlds.FRAME).
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import mesh_worlds as M
import smooth_reference as R
import smooth_worlds as S
from test_supersample_cpu import box_mean

pytestmark = pytest.mark.gpu

ABS64 = 1e-9  # the project's f64 bar
COUNTERS = ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned", "refract_evals", "schlick_evals")

# f32 against the f64 device frame of the same upload (test 10): share of pixels / of random rays whose
# colour is within 2/255 in every channel.  Floors by DESIGN.md §3.7's rule, the minimum observed on the
# MI355X less 0.005 (profiles/smooth_parity.json holds the observations):
#                    observed minimum          floor
#   frame pixels     4799 / 4800 = 0.999792    0.994792
#   random rays      4093 / 4096 = 0.999268    0.994268
F32_TOL = 2.0 / 255.0
F32_FLOOR_PIXELS = 4799.0 / 4800.0 - 0.005
F32_FLOOR_RAYS = 4093.0 / 4096.0 - 0.005


def _counts(st):
    return {k: st[k] for k in COUNTERS}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint8 else a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def ico(rtc):
    """The icosphere alone: smooth and flat tables, the frame's rays, the reference's frame and margin."""
    smooth, flat = S.ico_alone(rtc), S.ico_alone(rtc, smooth=False)
    rays = S.camera_rays(smooth.camera)
    rgb, hit, margin = R.trace(smooth, rays)
    rgb.setflags(write=False)
    return {"smooth": smooth, "flat": flat, "rays": rays, "rgb": rgb, "hit": hit, "margin": margin}


def _oracle(tables, depth, cam=None):
    import pyoracle
    ref, st = pyoracle.render(tables, cam or tables.camera, depth, threads=8)
    ref.setflags(write=False)
    return ref, st


def _assert_within(img, ref, what, bar=ABS64):
    err = np.abs(img - ref).max(axis=-1)
    err = np.where(np.isfinite(err), err, np.inf)
    worst = np.unravel_index(int(err.argmax()), err.shape)
    print(f"{what}: max |err| {err[worst]:.3g}")
    assert err[worst] < bar, f"{what}: {int((err >= bar).sum())} values differ, worst at {worst}: {err[worst]}"


# ------------------------------------------------------------ 5: interpolation
def test_f64_frame_and_rays_equal_the_reference(gpu_ctx, rtc, ico):
    assert ico["margin"].min() > ABS64, "a decision of the reference sits on the fence: move the camera"
    assert (ico["hit"]["shape"] >= 0).mean() > 0.4
    gpu_ctx.upload(ico["smooth"])
    info = gpu_ctx.smooth_info()
    assert info["smooth_triangles"] == 320 and info["normal_bytes"] == 320 * 9 * (4 + 8), info
    w, h = S.FRAME
    img, st = gpu_ctx.render(ico["smooth"].camera, 5, precision="f64")
    assert gpu_ctx.smooth_info()["ran_smooth"] == 1
    _assert_within(img.reshape(-1, 3), ico["rgb"], "render")
    assert st["primary"] == w * h and st["shaded"] == int((ico["hit"]["shape"] >= 0).sum()) == st["shadow"]
    rgb, t, shape, st = gpu_ctx.trace_rays(ico["rays"], 5, precision="f64", hits=True)
    _assert_within(rgb, ico["rgb"], "trace_rays")
    assert np.array_equal(shape, ico["hit"]["shape"]) and np.abs(t - ico["hit"]["t"])[shape >= 0].max() < 1e-12
    # the same faces flat: facets the smooth frame does not show
    gpu_ctx.upload(ico["flat"])
    assert all(v == 0 for v in gpu_ctx.smooth_info().values())
    flat, _ = gpu_ctx.render(ico["flat"].camera, 5, precision="f64")
    assert np.abs(flat - img).max() > 0.05
    rgb_flat, _, _ = R.trace(ico["flat"], ico["rays"])
    _assert_within(flat.reshape(-1, 3), rgb_flat, "flat render against the reference")


def test_pool_kernel_equals_the_reference(gpu_ctx, rtc, ico):
    tables = S.ico_alone(rtc, extra=[S.glass_behind_the_camera()])
    assert tables.has_secondary() and len(tables.shapes) == 321
    gpu_ctx.upload(tables)
    img, st = gpu_ctx.render(tables.camera, 5, precision="f64")
    _assert_within(img.reshape(-1, 3), ico["rgb"], "pool render")
    assert st["reflect"] == 0 and st["refract"] == 0  # no ray met the sphere
    rgb, _ = gpu_ctx.trace_rays(ico["rays"], 5, precision="f64")
    _assert_within(rgb, ico["rgb"], "pool trace_rays")


def test_the_books_known_answer(gpu_ctx, rtc):
    from rtc_amd import world as W
    p, n, ray, u, v, want = R.known_answer()
    white = W.Material(color=(1.0, 1.0, 1.0), ambient=0.0, diffuse=1.0, specular=0.0)
    light = (-3.0, 4.0, -5.0)  # on the side the interpolated normal leans to
    tables = W.World([W.Light(light)], [W.smooth_triangle(*p, *n, white)]).tables()
    ref, hit, _ = R.trace(tables, np.array([ray]))
    assert abs(hit["u"][0] - u) < 1e-12 and abs(hit["v"][0] - v) < 1e-12
    gpu_ctx.upload(tables)
    for precision, bar in (("f64", ABS64), ("f32", 1e-5)):
        rgb, t, shape, _ = gpu_ctx.trace_rays(np.array([ray]), 0, precision=precision, hits=True)
        assert shape[0] == 0 and abs(t[0] - 2.0) < 1e-6
        _assert_within(rgb, ref, f"known answer {precision}", bar)
    # (the book's normal lies in the triangle's plane and the triangle shadows itself: black.)  With every
    # vertex normal leaning towards the eye the colour is the cosine of the interpolated normal with the light
    lean = tuple((x, y, z - 1.0) for x, y, z in n)
    leaning = W.World([W.Light(light)], [W.smooth_triangle(*p, *lean, white)]).tables()
    ref, _, _ = R.trace(leaning, np.array([ray]))
    normal = np.array([-0.2, 0.3, -1.0]) / np.sqrt(0.04 + 0.09 + 1.0)
    ld = np.array(light) - (np.array([-0.2, 0.3, 0.0]) + normal * R.EPSILON)
    cosine = float(np.dot(ld / np.linalg.norm(ld), normal))
    assert cosine > 0.5 and abs(ref[0, 0] - cosine) < 1e-12
    gpu_ctx.upload(leaning)
    for precision, bar in (("f64", ABS64), ("f32", 1e-5)):
        rgb, _ = gpu_ctx.trace_rays(np.array([ray]), 0, precision=precision)
        _assert_within(rgb, ref, f"leaning normals {precision}", bar)
    gpu_ctx.upload(tables)
    with pytest.raises(rtc.RenderError, match="smooth triangle's normal depends on the hit's u and v"):
        gpu_ctx.debug_normal(0, [[-0.2, 0.3, 0.0]])
    (ts,) = gpu_ctx.debug_intersect(0, [ray])  # as for the flat triangle
    assert len(ts) == 1 and abs(ts[0] - 2.0) < 1e-12


# ------------------------------------------------------------ 6: geometry untouched
def test_hits_are_the_flat_uploads_and_counters_the_oracles(gpu_ctx, rtc):
    smooth, flat = S.ico_over_plane(rtc), S.ico_over_plane(rtc, smooth=False)
    assert len(smooth.shapes) == 321
    rays = M.random_rays(2048, 97)
    got = {}
    for name, tables in (("smooth", smooth), ("flat", flat)):
        gpu_ctx.upload(tables)
        tree = gpu_ctx.tree_info()
        assert tree["nodes"] > 0 and tree["records_in_tree"] == 320, tree
        for precision in ("f32", "f64"):
            _, t, shape, _ = gpu_ctx.trace_rays(rays, 3, precision=precision, hits=True)
            got[name, precision] = (t, shape)
        got[name, "frame"] = gpu_ctx.render(tables.camera, 3, precision="f64")
    for precision in ("f32", "f64"):
        (ts, ss), (tf, sf) = got["smooth", precision], got["flat", precision]
        assert np.array_equal(ss, sf) and np.array_equal(_bits(ts), _bits(tf)), precision
        assert (ss >= 1).sum() > 100
    _, rst = _oracle(flat, 3)
    assert _counts(got["smooth", "frame"][1]) == _counts(rst) == _counts(got["flat", "frame"][1])
    assert np.abs(got["smooth", "frame"][0] - got["flat", "frame"][0]).max() > 0.05


# ------------------------------------------------------------ 7: degenerate normals are flat shading
@pytest.fixture(scope="module")
def box(rtc):
    smooth, flat = S.box_world(rtc), S.box_world(rtc, smooth=False)
    ref, rst = _oracle(flat, 4)
    return {"smooth": smooth, "flat": flat, "ref": ref, "rst": rst}


def _rel_within(img, ref, what):
    _assert_within(img / np.maximum(1.0, np.abs(ref)), ref / np.maximum(1.0, np.abs(ref)), what)


def test_degenerate_normals_shade_as_the_flat_box(gpu_ctx, rtc, box):
    import pyoracle
    tables, flat, ref, rst = box["smooth"], box["flat"], box["ref"], box["rst"]
    cam = tables.camera
    gpu_ctx.upload(tables)
    assert gpu_ctx.smooth_info()["smooth_triangles"] == 12
    img, st = gpu_ctx.render(cam, 4, precision="f64")
    _rel_within(img, ref, "frame")
    assert _counts(st) == _counts(rst) and st["refract"] > 0 and st["reflect"] > 0
    # n x n samples per pixel
    cn = rtc.camera_resize(cam, 2 * cam.width, 2 * cam.height)
    ref2, rst2 = _oracle(flat, 4, cn)
    ss, st = gpu_ctx.render_supersampled(cam, 2, 4, precision="f64")
    _rel_within(ss, box_mean(ref2, 2), "supersampled")
    assert _counts(st) == _counts(rst2)
    # shard 1 of 2
    strip, _ = gpu_ctx.render(cam, 4, precision="f64", shard=(1, 2))
    shard, row = rtc.shard_row_map(cam.height, 2)
    for y in np.nonzero(shard == 1)[0]:
        _rel_within(strip[row[y]], ref[y], f"shard row {y}")
    # color_at on the frame's rays (unit directions)
    rays = S.camera_rays(cam)
    rgb, st = gpu_ctx.color_at(rays, 4, precision="f64")
    want, wst = pyoracle.color_at(flat, rays, 4)
    _rel_within(rgb, want, "color_at")
    assert _counts(st) == _counts(wst)
    # u8 within one level
    u8, _ = gpu_ctx.render(cam, 4, precision="f64", out_format="u8")
    assert np.abs(u8.astype(int) - pyoracle.quantize(ref).astype(int)).max() <= 1


def test_degenerate_normals_under_instances(gpu_ctx, rtc):
    tables = S.box_instances(rtc)
    flat = S.box_instances(rtc, smooth=False).expanded()
    ref, rst = _oracle(flat, 4)
    gpu_ctx.upload(tables)
    info, sm = gpu_ctx.instance_info(), gpu_ctx.smooth_info()
    assert info["instances"] == 2 and info["expanded"] == 0 and info["local_records"] == 12, info
    assert sm["smooth_triangles"] == 24 and sm["normal_bytes"] == 12 * 9 * 12, sm
    img, st = gpu_ctx.render(tables.camera, 4, precision="f64")
    _rel_within(img, ref, "instanced frame")
    assert _counts(st) == _counts(rst) and st["refract"] > 0


# ------------------------------------------------------------ 8: invariance
def _results(ctx, tables, depth, rays, flags=0):
    cam, out = tables.camera, {}
    for precision in ("f32", "f64"):
        out[f"render {precision}"] = ctx.render(cam, depth, precision=precision, flags=flags)
        out[f"supersampled {precision}"] = ctx.render_supersampled(cam, 2, depth, precision=precision, flags=flags)
        rgb, t, shape, st = ctx.trace_rays(rays, depth, precision=precision, hits=True, flags=flags)
        out[f"trace_rays {precision}"] = (np.concatenate([rgb, t[:, None]], axis=1), st)
        out[f"hit shapes {precision}"] = (shape.astype(np.float64), st)
    return out


def _same(got, want, what):
    for key, (a, sa) in got.items():
        b, sb = want[key]
        diff = np.argwhere(_bits(a) != _bits(b))
        assert len(diff) == 0, f"{what} {key}: {len(diff)} values differ, first at {tuple(diff[0])}"
        assert _counts(sa) == _counts(sb), f"{what} {key}"


WORLD8 = {"ico": lambda rtc: (S.ico_over_plane(rtc), 3), "ico glass": lambda rtc: (S.ico_over_plane(rtc, material=M.glass()), 4),
          "tori": lambda rtc: (S.torus_instances(rtc), 3)}


@pytest.mark.parametrize("key", list(WORLD8))
def test_knobs_skips_and_the_expansion_change_no_bit(rtc, monkeypatch, key):
    tables, depth = WORLD8[key](rtc)
    rays = M.random_rays(2048, 4321)
    with rtc.Context(0) as c:
        c.upload(tables)
        assert c.smooth_info()["smooth_triangles"] == (320 if key != "tori" else 3 * 576)
        want = _results(c, tables, depth, rays)
        assert (want["hit shapes f64"][0] >= 1).sum() > 50
        c.set_jit(rtc.RT_JIT_SYNC)  # a world with a smooth triangle takes no per-scene build
        c.render(tables.camera, depth, precision="f32")
        js = c.jit_status()
        assert not js["used"] and "smooth triangles" in js["log"] and js["compile_ms"] == 0.0, js
        _same(_results(c, tables, depth, rays, rtc.RT_FLAG_NO_SKIPS), want, "RT_FLAG_NO_SKIPS")
        # the expansion (rt_instances_expand / rt_smooth_expand) on the same context
        flat = tables.expanded()
        if flat is not tables:
            assert c.instance_info()["expanded"] == 0 and c.instance_info()["instances"] == 3
            c.upload(flat)
            assert c.instance_info()["instances"] == 0 and c.smooth_info()["smooth_triangles"] == 3 * 576
            _same(_results(c, flat, depth, rays), want, "the expansion")
    for knob in ("tri_tree=0", "cull=0"):
        monkeypatch.setenv("RTC_DEBUG", knob)
        with rtc.Context(0) as c:
            c.upload(tables)
            _same(_results(c, tables, depth, rays), want, knob)
    monkeypatch.delenv("RTC_DEBUG")
    with rtc.Context.multi([0]) as g:  # a group of one rank carries the normal tables
        g.upload(tables)
        assert g.smooth_info()["smooth_triangles"] == (320 if key != "tori" else 3 * 576)
        for precision in ("f32", "f64"):
            a, sa = g.render(tables.camera, depth, precision=precision)
            b, sb = want[f"render {precision}"]
            assert np.array_equal(_bits(a), _bits(b)) and _counts(sa) == _counts(sb), precision


def test_baked_and_unbaked_agree(gpu_ctx, rtc):
    from rtc_amd import world as W
    verts, faces = M.torus(24, 12)
    ring = np.stack([verts[:, 0], np.zeros(len(verts)), verts[:, 2]], axis=1)
    ring /= np.linalg.norm(ring, axis=1)[:, None]
    mesh = S.load(rtc, verts, faces, (verts - ring) / 0.4)
    T = W.mat_mul(W.rotation_y(0.7), W.shearing(0.3, 0.0, 0.0, 0.2, 0.0, 0.0))
    frames = []
    for bake in (False, True):
        shapes = W.mesh(mesh, S.opaque(), transform=T, bake=bake, smooth=True)
        tables = W.World([S.eye_light()], shapes).tables(S.camera())
        gpu_ctx.upload(tables)
        frames.append(gpu_ctx.render(tables.camera, 3, precision="f64")[0])
    assert frames[0].max() > 0.3
    _assert_within(frames[1], frames[0], "baked against unbaked")


def test_tables_are_reused_flat_smooth_flat(rtc):
    flat, smooth = S.ico_over_plane(rtc, smooth=False), S.ico_over_plane(rtc)

    def fresh(t):
        with rtc.Context(0) as c:
            c.upload(t)
            return [c.render(t.camera, 3, precision=p) for p in ("f32", "f64")]

    want = {"flat": fresh(flat), "smooth": fresh(smooth)}
    with rtc.Context(0) as c:
        for name, t in (("flat", flat), ("smooth", smooth), ("flat", flat), ("smooth", smooth)):
            c.upload(t)
            assert c.smooth_info()["smooth_triangles"] == (320 if name == "smooth" else 0)
            for (a, sa), p in zip(want[name], ("f32", "f64")):
                b, sb = c.render(t.camera, 3, precision=p)
                assert np.array_equal(_bits(a), _bits(b)) and _counts(sa) == _counts(sb), (name, p)
            assert c.smooth_info()["ran_smooth"] == (1 if name == "smooth" else 0)


def test_no_smooth_entry_is_the_instanced_upload_itself(rtc):
    tables = S.flat_of(rtc, S.torus_instances(rtc))
    with rtc.Context(0) as a, rtc.Context(0) as b:
        a.upload(tables)
        assert rtc._lib.rt_scene_upload_smooth(b._h, *tables.smooth_args()) == rtc.RT_OK, rtc._lib.rt_last_error()
        assert all(v == 0 for v in b.smooth_info().values())
        ia, ib = a.instance_info(), b.instance_info()
        assert {k: v for k, v in ia.items() if k != "build_ms"} == {k: v for k, v in ib.items() if k != "build_ms"}
        for precision in ("f32", "f64"):
            x, sx = a.render(tables.camera, 3, precision=precision)
            y, sy = b.render(tables.camera, 3, precision=precision)
            assert np.array_equal(_bits(x), _bits(y)) and _counts(sx) == _counts(sy)


# ------------------------------------------------------------ 9: identity on the device
def test_value_equal_smooth_boxes_are_one_class_and_a_differing_normal_makes_two(gpu_ctx, rtc):
    from rtc_amd import world as W
    # two coincident glass boxes equal in every field: the kDup walk, as the oracle's doubled flat box
    doubled = S.box_world(rtc, copies=2)
    ref, rst = _oracle(S.box_world(rtc, smooth=False, copies=2), 4)
    gpu_ctx.upload(doubled)
    img, st = gpu_ctx.render(doubled.camera, 4, precision="f64")
    _rel_within(img, ref, "value-equal pair")
    assert _counts(st) == _counts(rst)
    # every triangle of the second copy differs from its twin in one normal component: two shapes each, as
    # the oracle's pair of flat boxes that differ by value in the second copy's colour (the first copy wins
    # every tie, so neither the second's colour nor its normals are ever shaded)
    _, _, normals, _ = S.box(True)
    other = normals + 1e-3 * np.roll(normals, 1, axis=1)
    pair = S.box_world(rtc, copies=2, normals_of_second=other)
    glass2 = M.glass()
    glass2.color = (0.1, 0.2, 0.31)
    ref2, rst2 = _oracle(S.box_world(rtc, smooth=False, copies=2, material_of_second=glass2), 4)
    assert np.abs(ref2 - ref).max() > 0.01, "one class and two must not look alike"
    gpu_ctx.upload(pair)
    img2, st2 = gpu_ctx.render(pair.camera, 4, precision="f64")
    _rel_within(img2, ref2, "pair differing in one normal")
    assert _counts(st2) == _counts(rst2)
    # a smooth and a flat twin are two shapes as well
    verts, faces, nn, fnorm = S.box(True)
    place = W.mat_mul(W.translation(0.1, 0.0, 0.3), W.mat_mul(W.rotation_y(0.5), W.scaling(0.8, 0.9, 0.7)))
    mesh = S.load(rtc, verts, faces, nn, fnorm)
    shapes_flat = W.mesh(mesh, M.glass(), transform=place)
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    plane = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                    transform=W.translation(0, -1.3, 0))
    both = W.World(lights, [plane] + W.mesh(mesh, M.glass(), transform=place, smooth=True) + shapes_flat).tables(S.camera())
    gpu_ctx.upload(both)
    img3, st3 = gpu_ctx.render(both.camera, 4, precision="f64")
    _rel_within(img3, ref2, "smooth and flat twin")
    assert _counts(st3) == _counts(rst2)


# ------------------------------------------------------------ 10: f32 against the f64 device frame
def f32_parity(ctx, rtc):
    """{world: (share of frame pixels, share of random rays)} of f32 within 2/255 of the f64 device results."""
    out = {}
    worlds = {"ico alone": (S.ico_alone(rtc), 5)}
    worlds.update({k: f(rtc) for k, f in WORLD8.items()})
    rays = M.random_rays(4096, 2718)
    for name, (tables, depth) in worlds.items():
        ctx.upload(tables)
        f64, _ = ctx.render(tables.camera, depth, precision="f64")
        f32, _ = ctx.render(tables.camera, depth, precision="f32")
        r64, _ = ctx.trace_rays(rays, depth, precision="f64")
        r32, _ = ctx.trace_rays(rays, depth, precision="f32")
        out[name] = (M.share_within(f32.astype(np.float64), f64, F32_TOL), M.share_within(r32, r64, F32_TOL))
    return out


def test_f32_stays_within_two_levels_of_the_f64_frame(gpu_ctx, rtc):
    shares = f32_parity(gpu_ctx, rtc)
    for name, (pixels, rays) in shares.items():
        print(f"{name}: pixels {pixels:.4f} rays {rays:.4f}")
    for name, (pixels, rays) in shares.items():
        assert pixels >= F32_FLOOR_PIXELS, (name, pixels)
        assert rays >= F32_FLOOR_RAYS, (name, rays)


# ------------------------------------------------------------ 11: small shapes
def _small_world(rtc, shapes, eye=((0.2, 0.4, -4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))):
    from rtc_amd import world as W
    return W.World([W.Light((-2.0, 3.0, -5.0), (0.9, 0.9, 0.9))], shapes).tables(S.camera(eye=eye))


def _against_reference(ctx, tables, what, rays=None):
    rays = S.camera_rays(tables.camera) if rays is None else rays
    ref, hit, margin = R.trace(tables, rays)
    assert margin.min() > ABS64, (what, margin.min())
    ctx.upload(tables)
    rgb, t, shape, _ = ctx.trace_rays(rays, 2, precision="f64", hits=True)
    _assert_within(rgb, ref, what)
    assert np.array_equal(shape, hit["shape"])
    if rays.shape[0] == tables.camera.width * tables.camera.height:
        img, _ = ctx.render(tables.camera, 2, precision="f64")
        _assert_within(img.reshape(-1, 3), ref, what + " frame")
    return ref, hit


def test_one_and_eight_triangles_and_a_mixed_leaf(gpu_ctx, rtc):
    from rtc_amd import world as W
    mat = S.opaque()
    p, n = ((0.0, 1.2, 0.1), (-1.3, -0.9, 0.0), (1.1, -0.8, -0.2)), ((0.1, 1.0, -1.0), (-1.0, -0.2, -1.0), (1.0, 0.0, -0.8))
    one = rtc.load_obj(S.obj_text(np.array(p), np.array([[0, 1, 2]]), np.array(n)), normals=True)
    ref, hit = _against_reference(gpu_ctx, _small_world(rtc, W.mesh(one, mat, smooth=True)), "one triangle")
    assert (hit["shape"] == 0).sum() > 300
    verts, faces, normals = S.icosphere(0)  # 20 triangles; the first 8 make one leaf
    eight = rtc.load_obj(S.obj_text(verts, faces[:8], normals, faces[:8]), normals=True)
    _against_reference(gpu_ctx, _small_world(rtc, W.mesh(eight, mat, smooth=True)), "eight triangles")
    # flat and smooth triangles in one leaf, and as instances of one mesh
    text = S.obj_text(verts, faces[:8], normals, faces[:8]).splitlines()
    rows = [i for i, line in enumerate(text) if line.startswith("f ")]
    for i in rows[::2]:
        text[i] = "f " + " ".join(w.split("//")[0] for w in text[i].split()[1:])
    mixed = rtc.load_obj("\n".join(text) + "\n", normals=True)
    assert mixed.n_smooth == 4
    tables = _small_world(rtc, W.mesh(mixed, mat, smooth=True))
    _against_reference(gpu_ctx, tables, "mixed leaf")
    inst = W.World([W.Light((-2.0, 3.0, -5.0), (0.9, 0.9, 0.9))], [],
                    [W.instance(mixed, mat, transform=W.translation(-0.6, 0.0, 0.0), smooth=True),
                     W.instance(mixed, mat, transform=W.mat_mul(W.translation(0.9, 0.1, 0.4), W.rotation_z(0.8)), smooth=True)]
                    ).tables(S.camera(eye=((0.2, 0.4, -4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))))
    flat = inst.expanded()
    ref, hit, margin = R.trace(flat, S.camera_rays(inst.camera))
    assert margin.min() > ABS64 and len(flat.smooth) == 8
    gpu_ctx.upload(inst)
    assert gpu_ctx.instance_info()["expanded"] == 0
    img, _ = gpu_ctx.render(inst.camera, 2, precision="f64")
    _assert_within(img.reshape(-1, 3), ref, "mixed leaf under two instances")


def test_hit_from_behind_and_a_normal_opposing_the_face(gpu_ctx, rtc):
    from rtc_amd import world as W
    mat = W.Material(color=(0.9, 0.5, 0.2), specular=0.3)
    p = ((0.0, 1.2, 0.0), (-1.3, -0.9, 0.0), (1.1, -0.8, 0.0))
    toward = ((0.1, 0.2, -1.0), (-0.3, 0.0, -1.0), (0.2, -0.1, -0.9))  # normals on the camera's side
    away = tuple(tuple(-c for c in v) for v in toward)                  # the same, opposing: the flip decides
    frames = {}
    for name, n in (("toward", toward), ("away", away)):
        tables = _small_world(rtc, [W.smooth_triangle(*p, *n, mat)])
        ref, _ = _against_reference(gpu_ctx, tables, f"normals {name}")
        frames[name] = ref
    # n . eye < 0 flips the shading normal: both triangles shade alike
    assert np.abs(frames["toward"] - frames["away"]).max() < 1e-12 and frames["toward"].max() > 0.3
    # seen from behind (the camera beyond the triangle): the flip again, by the shading normal
    behind = _small_world(rtc, [W.smooth_triangle(*p, *toward, mat)], eye=((0.3, 0.2, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    _against_reference(gpu_ctx, behind, "from behind")
    # a vertex normal opposing the face normal on one corner only: the interpolated normal turns over inside
    # the triangle, and the flip follows it pixel by pixel
    twisted = ((0.0, 0.0, -1.0), (0.0, 0.0, 1.5), (0.1, 0.0, -1.0))
    tables = _small_world(rtc, [W.smooth_triangle(*p, *twisted, mat)])
    _against_reference(gpu_ctx, tables, "twisted")


def test_rays_through_vertices_and_along_edges_of_the_dyadic_field(gpu_ctx, rtc):
    from rtc_amd import world as W
    verts, faces, normals = S.height_field()
    smooth = _small_world(rtc, W.mesh(S.load(rtc, verts, faces, normals), S.opaque(), smooth=True))
    flat = S.flat_of(rtc, smooth)
    # straight down through every vertex, and through the midpoints of the cells' edges (dyadic: exact)
    xs = np.arange(-2.0, 2.0 + 1e-9, 0.125)
    gx, gz = np.meshgrid(xs, xs)
    down = np.stack([gx.ravel(), np.full(gx.size, 3.0), gz.ravel(), np.zeros(gx.size), -np.ones(gx.size), np.zeros(gx.size)], axis=1)
    # along the edges: in the plane z = const of a row of vertices, grazing at dyadic heights
    along = np.stack([np.full(33, -3.0), np.linspace(0.0, 0.5, 33), np.repeat(xs[::8], 7)[:33], np.ones(33), np.zeros(33),
                      np.zeros(33)], axis=1)
    rays = np.ascontiguousarray(np.concatenate([down, along]))
    got = {}
    for name, tables in (("smooth", smooth), ("flat", flat)):
        gpu_ctx.upload(tables)
        for precision in ("f32", "f64"):
            _, t, shape, _ = gpu_ctx.trace_rays(rays, 1, precision=precision, hits=True)
            got[name, precision] = (t, shape)
    for precision in ("f32", "f64"):
        (ts, ss), (tf, sf) = got["smooth", precision], got["flat", precision]
        assert np.array_equal(ss, sf) and np.array_equal(_bits(ts), _bits(tf)), precision
    hits = got["smooth", "f64"][1][:len(down)] >= 0
    assert 0.2 < hits.mean() < 0.9, "rays through vertices and edges must both hit and miss"
    assert (got["smooth", "f64"][1][len(down):] >= 0).any()


# ------------------------------------------------------------ 12: the CLI
def test_cli_smooth(rtc, tmp_path):
    from test_cli import CLI, SCENE
    from rtc_amd import world as W
    yaml = tmp_path / "scene.yaml"
    yaml.write_text(SCENE)
    verts, faces, normals = S.icosphere(2)
    obj = tmp_path / "ico.obj"
    obj.write_text(S.obj_text(verts * 0.8 + np.array([0.0, 1.0, 0.0]), faces, normals))
    common = ["--precision", "f64", "--width", "80", "--height", "60"]
    outs, ignored = {}, {}
    for name, extra in (("smooth", ["--smooth"]), ("flat", [])):
        out = tmp_path / f"{name}.png"
        r = subprocess.run([CLI, str(yaml), str(out), "--obj", str(obj)] + common + extra, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        assert ("320 smooth triangles" in r.stdout) == (name == "smooth")
        ignored[name] = int(re.search(r"(\d+) lines ignored", r.stdout).group(1))
        outs[name] = out.read_bytes()
    assert ignored["flat"] - ignored["smooth"] == len(normals) == 162  # the vn lines
    assert outs["smooth"] != outs["flat"]
    scene = rtc.load_scene(str(yaml))
    cam = rtc.camera_resize(scene.camera, 80, 60)
    n, nm = len(scene.shapes), len(scene.materials)
    mesh = rtc.load_obj(str(obj), normals=True)
    for name, smooth in (("smooth", True), ("flat", False)):
        tri = mesh.shape_descs(None, False, nm)
        shapes = (rtc.ShapeDesc * (n + len(tri)))()
        C.memmove(shapes, scene.shapes, n * C.sizeof(rtc.ShapeDesc))
        C.memmove(C.byref(shapes, n * C.sizeof(rtc.ShapeDesc)), tri, len(tri) * C.sizeof(rtc.ShapeDesc))
        mats = (rtc.MaterialDesc * (nm + 1))()
        C.memmove(mats, scene.materials, nm * C.sizeof(rtc.MaterialDesc))
        mats[nm] = W.World([], [W.sphere()]).tables().materials[0]  # Material::default as the tables hold it
        tables = rtc.SceneTables(shapes, mats, scene.patterns, scene.lights, cam,
                                 smooth=mesh.smooth_descs(first=n) if smooth else None)
        with rtc.Context(0) as c:
            c.upload(tables)
            want, _ = c.render(cam, 6, precision="f64", out_format="u8")
        ref = tmp_path / f"ref_{name}.png"
        assert rtc._lib.rt_image_write(str(ref).encode(), want.ctypes.data_as(C.c_void_p), 80, 60) == rtc.RT_OK
        assert outs[name] == ref.read_bytes(), name
    # the same through world.mesh(smooth=True) on the scene's own tables: byte for byte
    inst_out = tmp_path / "inst.png"
    r = subprocess.run([CLI, str(yaml), str(inst_out), "--instance", f"{obj}:0,0,0", "--smooth"] + common,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "320 smooth triangles" in r.stdout, r.stderr
    assert inst_out.read_bytes() == outs["smooth"], "an instance at the identity is the --obj world"
