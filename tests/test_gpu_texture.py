"""Image textures on the GPU (worlds in tests/texture_worlds.py).

The reference has no textures.  The f64 kernels are held to the oracle where the
definition coincides with one of its patterns (a 2 x 1 texture is a stripe under
the nearest filter and a gradient under the bilinear one; a texture of one
colour is a material colour), and to tests/texture_reference.py (a numpy
restatement of rtc.h's definition) for interpolated coordinates.

  1. oracle ties: stripe, gradient, uniform colour, through every entry point;
  2. interpolated coordinates against the numpy reference;
  3. geometry untouched: hits bit-identical to the untextured upload;
  4. invariance: knobs, RT_FLAG_NO_SKIPS, the expansion, a group, table reuse;
  5. small shapes where the kernel can still go wrong;
  6. f32 against the f64 device frame;
  7. the CLI's --texture.

Frames are 80 x 60 (texture_worlds.FRAME).
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import mesh_worlds as M
import smooth_worlds as S
import texture_reference as T
import texture_worlds as X
from test_supersample_cpu import box_mean

pytestmark = pytest.mark.gpu

ABS64 = 1e-9  # the project's f64 bar
COUNTERS = ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned", "refract_evals", "schlick_evals")
GEOMETRY = tuple(c for c in COUNTERS if c != "lit_patterned")

# f32 against the f64 device frame of the same upload (test 6): share of pixels / of random rays whose colour
# is within 2/255 in every channel.  Floors by DESIGN.md §3.7's rule, the minimum observed on the MI355X less
# 0.005 (profiles/texture_parity.json holds the observations):
#                    observed minimum          floor
#   frame pixels     4799 / 4800 = 0.999792    0.994792   (the glass icosphere; 4800 / 4800 elsewhere)
#   random rays      4093 / 4096 = 0.999268    0.994268   (the glass icosphere; 4095, 4095 and 4094 elsewhere)
F32_TOL = 2.0 / 255.0
F32_MIN_PIXELS, F32_MIN_RAYS = 4799, 4093
F32_FLOOR_PIXELS = F32_MIN_PIXELS / 4800.0 - 0.005
F32_FLOOR_RAYS = F32_MIN_RAYS / 4096.0 - 0.005

A, B = (200, 40, 90), (30, 220, 140)
TWO = np.array([[A, B]], dtype=np.uint8)  # 2 x 1


def _counts(st, keys=COUNTERS):
    return {k: st[k] for k in keys}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint8 else a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


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


def _rel_within(img, ref, what):
    _assert_within(img / np.maximum(1.0, np.abs(ref)), ref / np.maximum(1.0, np.abs(ref)), what)


def _every_entry_point(ctx, rtc, tables, oracle_tables, depth, what, counters=COUNTERS):
    """render, render_supersampled(2), shard 1 of 2, trace_rays, color_at and u8 of `tables` on the device against
    the oracle's `oracle_tables`: 1e-9 on every value, the counters equal."""
    import pyoracle
    cam = tables.camera
    ref, rst = _oracle(oracle_tables, depth)
    ctx.upload(tables)
    img, st = ctx.render(cam, depth, precision="f64")
    assert ctx.texture_info()["ran_textured"] == 1
    _rel_within(img, ref, f"{what}: frame")
    assert _counts(st, counters) == _counts(rst, counters), what
    cn = rtc.camera_resize(cam, 2 * cam.width, 2 * cam.height)
    ref2, rst2 = _oracle(oracle_tables, depth, cn)
    ss, st2 = ctx.render_supersampled(cam, 2, depth, precision="f64")
    _rel_within(ss, box_mean(ref2, 2), f"{what}: supersampled")
    assert _counts(st2, counters) == _counts(rst2, counters), what
    strip, _ = ctx.render(cam, depth, precision="f64", shard=(1, 2))
    shard, row = rtc.shard_row_map(cam.height, 2)
    rows = np.nonzero(shard == 1)[0]
    _rel_within(strip[row[rows]], ref[rows], f"{what}: shard 1 of 2")
    rays = S.camera_rays(cam)
    want, wst = pyoracle.color_at(oracle_tables, rays, depth)
    rgb, st3 = ctx.color_at(rays, depth, precision="f64")
    _rel_within(rgb, want, f"{what}: color_at")
    assert _counts(st3, counters) == _counts(wst, counters), what
    rgb, st4 = ctx.trace_rays(rays, depth, precision="f64")
    _rel_within(rgb, want, f"{what}: trace_rays")
    assert _counts(st4, counters) == _counts(wst, counters), what
    u8, _ = ctx.render(cam, depth, precision="f64", out_format="u8")
    assert np.abs(u8.astype(int) - pyoracle.quantize(ref).astype(int)).max() <= 1, what
    return st


# ------------------------------------------------------------ 1: oracle ties
def _tie_world(pattern, kinds):
    """A plane, a sphere and a cube over it under two lights, all with `pattern` (a callable: a fresh one
    per shape); the cube is glass where `kinds` says so."""
    from rtc_amd import world as W
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    shapes = []
    if "plane" in kinds:
        shapes.append(W.plane(W.Material(pattern=pattern(), specular=0.0), transform=W.translation(0, -1.3, 0)))
    if "sphere" in kinds:
        shapes.append(W.sphere(W.Material(pattern=pattern(), specular=0.4, shininess=50.0),
                               transform=W.mat_mul(W.translation(-0.9, -0.1, 0.3), W.rotation_z(0.4))))
    glass = M.glass() if "glass" in kinds else W.Material(specular=0.3)
    glass.pattern = pattern()
    shapes.append(W.cube(glass, transform=W.mat_mul(W.translation(0.9, -0.3, 0.2),
                                                    W.mat_mul(W.rotation_y(0.6), W.scaling(0.6, 0.7, 0.5)))))
    return W.World(lights, shapes).tables(S.camera())


def test_a_two_texel_texture_with_the_nearest_filter_is_the_oracles_stripes(gpu_ctx, rtc):
    from rtc_amd import world as W
    a, b = tuple(c / 255.0 for c in A), tuple(c / 255.0 for c in B)
    textured = _tie_world(lambda: W.image_pattern(TWO, "nearest"), ("plane", "sphere", "glass"))
    stripes = _tie_world(lambda: W.stripe_pattern(a, b).set_transformation(W.scaling(0.5, 1.0, 1.0)), ("plane", "sphere", "glass"))
    assert len(textured.textures) == 1 and textured.uvs is None
    st = _every_entry_point(gpu_ctx, rtc, textured, stripes, 4, "stripes")
    assert st["refract"] > 0 and st["reflect"] > 0 and st["lit_patterned"] > 1000
    info = gpu_ctx.texture_info()
    assert info["textures"] == 1 and info["textured_triangles"] == 0 and info["uv_bytes"] == 0
    assert info["texel_bytes"] == 2 * 4 + 16, info


def test_a_two_texel_texture_with_the_bilinear_filter_is_the_oracles_gradient(gpu_ctx, rtc):
    from rtc_amd import world as W
    a, b = tuple(c / 255.0 for c in A), tuple(c / 255.0 for c in B)
    inv = [[0.49, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]  # x in [-1, 1] -> 0.5 + 0.49 x

    def with_inverse(p):
        p.transformation_inverse = [row[:] for row in inv]
        return p
    textured = _tie_world(lambda: with_inverse(W.image_pattern(TWO, "bilinear")), ("sphere",))
    gradient = _tie_world(lambda: with_inverse(W.gradient_pattern(a, b)), ("sphere",))
    _every_entry_point(gpu_ctx, rtc, textured, gradient, 4, "gradient")


@pytest.mark.parametrize("size", [(1, 1), (1, 2), (3, 2)])
def test_a_texture_of_one_colour_is_the_oracles_material_colour(gpu_ctx, rtc, size):
    from rtc_amd import world as W
    rgb = (200, 120, 40)
    image = X.uniform(*size, rgb)
    colour = tuple(c / 255.0 for c in rgb)
    verts, faces = M.icosphere(1)
    rng = np.random.default_rng(11)
    tc = rng.uniform(-1.5, 2.5, size=(len(verts), 2))  # arbitrary coordinates, wrapped ones among them
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                    transform=W.translation(0, -1.3, 0))
    places = [W.translation(-1.0, 0.0, 0.2),
              W.mat_mul(W.translation(1.0, 0.2, 0.4), W.mat_mul(W.rotation_y(0.7), W.shearing(0.3, 0.0, 0.0, 0.2, 0.0, 0.0)))]
    half = W.scaling(0.7, 0.7, 0.7)
    geometry = ("primary", "shadow", "reflect", "refract", "shaded", "refract_evals", "schlick_evals")
    for filt in ("nearest", "bilinear"):
        for smooth in (False, True):  # with smooth normals too: one triangle test serves both
            mesh = X.load(rtc, verts, faces, tc, normals=verts.copy() if smooth else None)
            plain = rtc.load_obj(S.obj_text(verts, faces, verts.copy() if smooth else None), normals=smooth)
            mat = lambda textured: W.Material(color=(1.0, 1.0, 1.0) if textured else colour, specular=0.4, shininess=40.0,
                                              pattern=W.image_pattern(image, filt) if textured else None)
            # as plain triangles, and as two instances (translation; rotation x shear)
            one = W.World(lights, [floor] + W.mesh(mesh, mat(True), transform=half, textured=True, smooth=smooth)).tables(S.camera())
            one_ref = W.World(lights, [floor] + W.mesh(plain, mat(False), transform=half, smooth=smooth)).tables(S.camera())
            two = W.World(lights, [floor], [W.instance(mesh, mat(True), transform=W.mat_mul(p, half), textured=True, smooth=smooth)
                                            for p in places]).tables(S.camera())
            two_ref = W.World(lights, [floor], [W.instance(plain, mat(False), transform=W.mat_mul(p, half), smooth=smooth)
                                                for p in places]).tables(S.camera())
            for name, tables, ref_tables in (("triangles", one, one_ref), ("instances", two, two_ref)):
                if smooth:  # the oracle has no smooth triangles: the untextured device frame is the yardstick
                    gpu_ctx.upload(ref_tables)
                    ref, rst = gpu_ctx.render(ref_tables.camera, 3, precision="f64")
                else:
                    ref, rst = _oracle(ref_tables.expanded(), 3)
                gpu_ctx.upload(tables)
                if name == "instances":
                    assert gpu_ctx.instance_info()["expanded"] == 0
                assert gpu_ctx.texture_info()["textured_triangles"] == (80 if name == "triangles" else 160)
                img, st = gpu_ctx.render(tables.camera, 3, precision="f64")
                _rel_within(img, ref, f"{size} {filt} smooth={smooth} {name}")
                assert _counts(st, geometry) == _counts(rst, geometry)
                assert st["lit_patterned"] > rst["lit_patterned"] > 0


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_a_uniform_texture_on_a_smooth_box_whose_normals_are_its_faces_own_is_the_oracles_flat_box(gpu_ctx, rtc, filt):
    rgb = (200, 120, 40)
    colour = tuple(c / 255.0 for c in rgb)
    textured = X.box_world(rtc, X.uniform(3, 2, rgb), filt, smooth=True)
    ref, rst = _oracle(X.box_world(rtc, None, filt, textured=False, color=colour), 4)
    gpu_ctx.upload(textured)
    assert gpu_ctx.smooth_info()["smooth_triangles"] == 12 and gpu_ctx.texture_info()["textured_triangles"] == 12
    img, st = gpu_ctx.render(textured.camera, 4, precision="f64")
    _rel_within(img, ref, f"smooth textured box {filt}")
    assert _counts(st, GEOMETRY) == _counts(rst, GEOMETRY) and st["refract"] > 0
    assert st["lit_patterned"] > rst["lit_patterned"] > 0


# ------------------------------------------------------------ 2: interpolated coordinates
@pytest.fixture(scope="module")
def ico(rtc):
    """The textured icosphere alone, per texture and filter: tables, the frame's rays, the reference."""
    out = {}
    for tex_name, image in (("six", X.SIX), ("5x7", X.colors(5, 7))):
        for filt in ("nearest", "bilinear"):
            tables = X.ico_alone(rtc, image, filt)
            rays = S.camera_rays(tables.camera)
            rgb, hit, margin = T.trace(tables, rays)
            rgb.setflags(write=False)
            out[tex_name, filt] = {"tables": tables, "rays": rays, "rgb": rgb, "hit": hit, "margin": margin, "image": image}
    return out


@pytest.mark.parametrize("tex_name", ["six", "5x7"])
@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_f64_frame_and_rays_equal_the_reference(gpu_ctx, rtc, ico, tex_name, filt):
    w = ico[tex_name, filt]
    assert w["margin"].min() > ABS64, "a decision of the reference sits on the fence: move the camera"
    assert (w["hit"]["shape"] >= 0).mean() > 0.4
    tables = w["tables"]
    gpu_ctx.upload(tables)
    info = gpu_ctx.texture_info()
    th, tw = w["image"].shape[:2]
    assert info["textured_triangles"] == 320 and info["uv_bytes"] == 320 * 6 * (4 + 8) and info["textures"] == 1
    assert info["texel_bytes"] == tw * th * 4 + 16, info
    img, st = gpu_ctx.render(tables.camera, 5, precision="f64")  # the direct kernel: no secondary rays
    assert gpu_ctx.texture_info()["ran_textured"] == 1
    _assert_within(img.reshape(-1, 3), w["rgb"], "render")
    hits = int((w["hit"]["shape"] >= 0).sum())
    assert st["primary"] == 80 * 60 and st["shaded"] == hits == st["shadow"] and st["lit_patterned"] > 0
    rgb, t, shape, _ = gpu_ctx.trace_rays(w["rays"], 5, precision="f64", hits=True)
    _assert_within(rgb, w["rgb"], "trace_rays")
    assert np.array_equal(shape, w["hit"]["shape"])
    # with a glass sphere out of every path: the pool kernel
    pool = X.ico_alone(rtc, w["image"], filt, extra=[S.glass_behind_the_camera()])
    assert pool.has_secondary()
    gpu_ctx.upload(pool)
    img, st = gpu_ctx.render(pool.camera, 5, precision="f64")
    _assert_within(img.reshape(-1, 3), w["rgb"], "pool render")
    assert st["reflect"] == 0 and st["refract"] == 0
    rgb, _ = gpu_ctx.trace_rays(w["rays"], 5, precision="f64")
    _assert_within(rgb, w["rgb"], "pool trace_rays")
    # the coordinates of two vertices exchanged: another picture
    swapped = X.ico_alone(rtc, w["image"], filt, swap=True)
    gpu_ctx.upload(swapped)
    other, _ = gpu_ctx.render(swapped.camera, 5, precision="f64")
    assert np.abs(other.reshape(-1, 3) - w["rgb"]).max() > 0.05


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_coordinates_equal_to_x_and_z_are_the_planar_map(gpu_ctx, rtc, filt):
    image = X.colors(5, 7)
    frames = {}
    for mapped in (True, False):
        tables = X.quad(rtc, image, filt, mapped=mapped)
        rays = S.camera_rays(tables.camera)
        ref, hit, margin = T.trace(tables, rays)
        assert margin.min() > ABS64 and (hit["shape"] >= 0).mean() > 0.2, margin.min()  # (the quad fills 28 % of the frame)
        gpu_ctx.upload(tables)
        assert gpu_ctx.texture_info()["textured_triangles"] == (2 if mapped else 0)
        img, _ = gpu_ctx.render(tables.camera, 2, precision="f64")
        _assert_within(img.reshape(-1, 3), ref, f"quad mapped={mapped}")
        frames[mapped] = img
    # (x, z) interpolated across the quad and wrapped, against (x, z) of the over point through the planar map
    _assert_within(frames[True], frames[False], "interpolated against planar")
    assert frames[True].std() > 0.05


# ------------------------------------------------------------ 3: geometry untouched
def test_hits_are_the_untextured_uploads_and_counters_the_oracles(gpu_ctx, rtc):
    textured = X.ico_over_plane(rtc, X.SIX, "bilinear")
    plain = X.ico_over_plane(rtc, X.SIX, "bilinear", textured=False)
    assert len(textured.shapes) == 321 and plain.uvs is None and not plain.textured
    rays = M.random_rays(2048, 97)
    got = {}
    for name, tables in (("textured", textured), ("plain", plain)):
        gpu_ctx.upload(tables)
        tree = gpu_ctx.tree_info()
        assert tree["nodes"] > 0 and tree["records_in_tree"] == 320, tree
        for precision in ("f32", "f64"):
            _, t, shape, _ = gpu_ctx.trace_rays(rays, 3, precision=precision, hits=True)
            got[name, precision] = (t, shape)
        got[name, "frame"] = gpu_ctx.render(tables.camera, 3, precision="f64")
    for precision in ("f32", "f64"):
        (ts, ss), (tp, sp) = got["textured", precision], got["plain", precision]
        assert np.array_equal(ss, sp) and np.array_equal(_bits(ts), _bits(tp)), precision
        assert (ss >= 1).sum() > 100
    _, rst = _oracle(plain, 3)
    assert _counts(got["plain", "frame"][1]) == _counts(rst)
    assert _counts(got["textured", "frame"][1], GEOMETRY) == _counts(rst, GEOMETRY)
    assert got["textured", "frame"][1]["lit_patterned"] > rst["lit_patterned"]
    assert np.abs(got["textured", "frame"][0] - got["plain", "frame"][0]).max() > 0.05


# ------------------------------------------------------------ 4: invariance
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


WORLD4 = {"ico": lambda rtc: (X.ico_over_plane(rtc, X.colors(5, 7), "bilinear"), 3),
          "ico glass": lambda rtc: (X.ico_over_plane(rtc, X.SIX, "nearest", material=M.glass()), 4),
          "tori": lambda rtc: (X.torus_instances(rtc, X.colors(5, 7), "bilinear"), 3)}


@pytest.mark.parametrize("key", list(WORLD4))
def test_knobs_skips_and_the_expansion_change_no_bit(rtc, monkeypatch, key):
    tables, depth = WORLD4[key](rtc)
    n_textured = 320 if key != "tori" else 3 * 576
    rays = M.random_rays(2048, 4321)
    with rtc.Context(0) as c:
        c.upload(tables)
        assert c.texture_info()["textured_triangles"] == n_textured
        want = _results(c, tables, depth, rays)
        assert (want["hit shapes f64"][0] >= 1).sum() > 50
        c.set_jit(rtc.RT_JIT_SYNC)  # a world with textures takes no per-scene build
        c.render(tables.camera, depth, precision="f32")
        js = c.jit_status()
        assert not js["used"] and "the world has textures" in js["log"] and js["compile_ms"] == 0.0, js
        _same(_results(c, tables, depth, rays, rtc.RT_FLAG_NO_SKIPS), want, "RT_FLAG_NO_SKIPS")
        # rt_instances_expand + rt_uv_expand on the same context (a world without instances is its own expansion)
        flat = tables.expanded()
        if flat is not tables:
            assert c.instance_info()["expanded"] == 0 and c.instance_info()["instances"] == 3
            c.upload(flat)
            assert c.instance_info()["instances"] == 0 and c.texture_info()["textured_triangles"] == n_textured
            _same(_results(c, flat, depth, rays), want, "the expansion")
    for knob in ("tri_tree=0", "cull=0"):
        monkeypatch.setenv("RTC_DEBUG", knob)
        with rtc.Context(0) as c:
            c.upload(tables)
            _same(_results(c, tables, depth, rays), want, knob)
    monkeypatch.delenv("RTC_DEBUG")
    with rtc.Context.multi([0]) as g:  # a group of one rank carries the coordinate tables and the texels
        g.upload(tables)
        assert g.texture_info()["textured_triangles"] == n_textured
        _same(_results(g, tables, depth, rays), want, "a group of one rank")


def test_tables_are_reused_textured_plain_textured(rtc):
    plain = X.ico_over_plane(rtc, X.SIX, "nearest", textured=False)
    textured = X.ico_over_plane(rtc, X.SIX, "nearest")

    def fresh(t):
        with rtc.Context(0) as c:
            c.upload(t)
            return [c.render(t.camera, 3, precision=p) for p in ("f32", "f64")]

    want = {"plain": fresh(plain), "textured": fresh(textured)}
    with rtc.Context(0) as c:
        for name, t in (("textured", textured), ("plain", plain), ("textured", textured), ("plain", plain)):
            c.upload(t)
            info = c.texture_info()
            assert info["textured_triangles"] == (320 if name == "textured" else 0)
            if name == "plain":
                assert all(v == 0 for v in info.values()), info
            for (a, sa), p in zip(want[name], ("f32", "f64")):
                b, sb = c.render(t.camera, 3, precision=p)
                assert np.array_equal(_bits(a), _bits(b)) and _counts(sa) == _counts(sb), (name, p)
            assert c.texture_info()["ran_textured"] == (1 if name == "textured" else 0)


def test_no_texture_is_the_smooth_upload_itself(rtc):
    tables = S.torus_instances(rtc)
    with rtc.Context(0) as a, rtc.Context(0) as b:
        a.upload(tables)
        assert rtc._lib.rt_scene_upload_textured(b._h, *tables.textured_args()) == rtc.RT_OK, rtc._lib.rt_last_error()
        assert all(v == 0 for v in b.texture_info().values()) and a.smooth_info() == b.smooth_info()
        for precision in ("f32", "f64"):
            x, sx = a.render(tables.camera, 3, precision=precision)
            y, sy = b.render(tables.camera, 3, precision=precision)
            assert np.array_equal(_bits(x), _bits(y)) and _counts(sx) == _counts(sy)


# ------------------------------------------------------------ 5: small shapes
def _small_world(rtc, shapes, instances=(), eye=((0.2, 0.4, -4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))):
    from rtc_amd import world as W
    return W.World([W.Light((-2.0, 3.0, -5.0), (0.9, 0.9, 0.9))], list(shapes), list(instances)).tables(S.camera(eye=eye))


def _against_reference(ctx, tables, what):
    flat = tables.expanded()
    rays = S.camera_rays(tables.camera)
    ref, hit, margin = T.trace(flat, rays)
    assert margin.min() > ABS64, (what, margin.min())
    ctx.upload(tables)
    rgb, t, shape, _ = ctx.trace_rays(rays, 2, precision="f64", hits=True)
    _assert_within(rgb, ref, what)
    assert np.array_equal(shape, hit["shape"])
    img, _ = ctx.render(tables.camera, 2, precision="f64")
    _assert_within(img.reshape(-1, 3), ref, what + " frame")
    return ref, hit


P3 = ((0.0, 1.2, 0.1), (-1.3, -0.9, 0.0), (1.1, -0.8, -0.2))


@pytest.mark.parametrize("size", [(1, 1), (1, 6), (6, 1)])
@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_degenerate_texture_sizes(gpu_ctx, rtc, size, filt):
    from rtc_amd import world as W
    image = X.colors(*size, seed=size[0] + 2 * size[1])
    tri = W.textured_triangle(*P3, (0.03, 0.07), (0.93, 0.11), (0.41, 0.97), X.textured_material(image, filt))
    ref, hit = _against_reference(gpu_ctx, _small_world(rtc, [tri]), f"{size} {filt}")
    assert (hit["shape"] == 0).sum() > 300
    if size != (1, 1):
        assert len(np.unique(np.round(ref[hit["shape"] == 0], 6), axis=0)) > 3


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_two_textures_of_different_sizes_and_coordinates_at_and_beyond_the_unit_square(gpu_ctx, rtc, filt):
    from rtc_amd import world as W
    big, small = X.colors(5, 7), X.SIX
    left = tuple((x - 1.4, y, z) for x, y, z in P3)
    right = tuple((x + 1.4, y, z + 0.2) for x, y, z in P3)
    shapes = [
        W.textured_triangle(*left, (0.0, 0.0), (1.0, 0.0), (0.0, 1.0), X.textured_material(big, filt)),     # exactly 0 and 1
        W.textured_triangle(*P3, (-1.3, -0.4), (2.2, 0.3), (0.6, 1.9), X.textured_material(small, filt)),   # wrapped, negative
        W.textured_triangle(*right, (1.0, 1.0), (0.0, 1.0), (1.0, 0.0), X.textured_material(small, filt)),
    ]
    tables = _small_world(rtc, shapes, eye=((0.2, 0.4, -5.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    assert len(tables.textures) == 2 and [p.sub_a for p in tables.patterns] == [0, 1, 1]
    ref, hit = _against_reference(gpu_ctx, tables, f"two textures {filt}")
    assert all((hit["shape"] == k).sum() > 100 for k in range(3))
    info = gpu_ctx.texture_info()
    assert info["textures"] == 2 and info["texel_bytes"] == (35 + 6) * 4 + 2 * 16 and info["uv_bytes"] == 3 * 6 * 12


def test_one_and_eight_triangles_a_mixed_leaf_and_a_smooth_textured_triangle(gpu_ctx, rtc):
    from rtc_amd import world as W
    image = X.colors(5, 7)
    mat = X.textured_material(image, "bilinear")
    verts, faces = M.icosphere(0)  # 20 triangles; the first 8 make one leaf
    tc = X.ico_coords(verts)
    one = X.load(rtc, np.array(P3), np.array([[0, 1, 2]]), np.array([(0.1, 0.2), (0.8, 0.1), (0.5, 0.9)]))
    _against_reference(gpu_ctx, _small_world(rtc, W.mesh(one, mat, textured=True)), "one triangle")
    eight = X.load(rtc, verts, faces[:8], tc)
    _against_reference(gpu_ctx, _small_world(rtc, W.mesh(eight, mat, textured=True)), "eight triangles")
    # triangles with and without coordinates in one leaf (the others take the planar map), and under two instances
    ft = [tuple(f) if i % 2 else None for i, f in enumerate(faces[:8].tolist())]
    mixed = X.load(rtc, verts, faces[:8], tc, face_texcoords=ft)
    assert mixed.n_textured == 4
    _against_reference(gpu_ctx, _small_world(rtc, W.mesh(mixed, mat, textured=True)), "mixed leaf")
    inst = _small_world(rtc, [], [W.instance(mixed, mat, transform=W.translation(-0.6, 0.0, 0.0), textured=True),
                                  W.instance(mixed, mat, transform=W.mat_mul(W.translation(0.9, 0.1, 0.4), W.rotation_z(0.8)),
                                             textured=True)])
    assert len(inst.expanded().uvs) == 8
    _against_reference(gpu_ctx, inst, "mixed leaf under two instances")
    assert gpu_ctx.instance_info()["expanded"] == 0 and gpu_ctx.texture_info()["textured_triangles"] == 8
    # seen from behind
    behind = _small_world(rtc, W.mesh(one, mat, textured=True), eye=((0.3, 0.2, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    _against_reference(gpu_ctx, behind, "from behind")
    # smooth and textured at once, alone and beside a triangle that is only smooth and one that is only textured
    n = ((0.1, 1.0, -1.0), (-1.0, -0.2, -1.0), (1.0, 0.0, -0.8))
    both = W.textured_triangle(*P3, (0.1, 0.2), (0.8, 0.1), (0.5, 0.9), mat)
    both.normals = n
    up = tuple((x, y + 2.3, z) for x, y, z in P3)
    only_smooth = W.smooth_triangle(*up, *n, mat)  # no coordinates: the planar map
    down = tuple((x, y - 2.3, z) for x, y, z in P3)
    only_uv = W.textured_triangle(*down, (0.1, 0.2), (0.8, 0.1), (0.5, 0.9), mat)
    tables = _small_world(rtc, [both, only_smooth, only_uv], eye=((0.2, 0.4, -7.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    _, hit = _against_reference(gpu_ctx, tables, "smooth and textured")
    assert all((hit["shape"] == k).sum() > 50 for k in range(3))
    assert gpu_ctx.smooth_info()["smooth_triangles"] == 2 and gpu_ctx.texture_info()["textured_triangles"] == 2


def test_value_equal_textured_boxes_are_one_class_and_a_differing_coordinate_makes_two(gpu_ctx, rtc):
    rgb = (90, 200, 160)
    image = X.uniform(3, 2, rgb)
    colour = tuple(c / 255.0 for c in rgb)
    # two coincident glass boxes equal in every field, coordinates included: the kDup walk, as the oracle's
    # doubled box of that colour
    doubled = X.box_world(rtc, image, "bilinear", copies=2)
    ref, rst = _oracle(X.box_world(rtc, image, "bilinear", copies=2, textured=False, color=colour), 4)
    gpu_ctx.upload(doubled)
    assert gpu_ctx.texture_info()["textured_triangles"] == 24
    img, st = gpu_ctx.render(doubled.camera, 4, precision="f64")
    _rel_within(img, ref, "value-equal pair")
    assert _counts(st, GEOMETRY) == _counts(rst, GEOMETRY) and st["refract"] > 0
    # the second copy's pattern names a texture of its own with the same picture, and the patterns name the two
    # textures in descending order: still one class (textures compare by content, whatever their indices)
    twin = X.box_world(rtc, image, "bilinear", copies=2, image_of_second=image.copy())
    assert len(twin.textures) == 2 and [p.sub_a for p in twin.patterns if p.kind == 6] == [0, 1]
    twin.textures.reverse()
    for p in twin.patterns:
        if p.kind == 6:
            p.sub_a = 1 - p.sub_a
    gpu_ctx.upload(twin)
    assert gpu_ctx.texture_info()["textures"] == 2
    img, st = gpu_ctx.render(twin.camera, 4, precision="f64")
    _rel_within(img, ref, "value-equal pair over two equal textures")
    assert _counts(st, GEOMETRY) == _counts(rst, GEOMETRY)
    # one coordinate of every triangle of the second copy differs: two shapes each, as the oracle's pair of
    # boxes that differ by value (the first copy wins every tie, so the second's colour is never shaded)
    verts = S.box(True)[0]
    base = np.stack([0.5 + 0.25 * verts[:, 0] + 0.125 * verts[:, 2], 0.5 + 0.25 * verts[:, 1]], axis=1)
    pair = X.box_world(rtc, image, "bilinear", copies=2, coords_of_second=base + np.array([1e-3, 0.0]))
    two = X.box_world(rtc, image, "bilinear", copies=2, textured=False, color=colour)
    for s in two.shapes[13:]:
        two.materials[s.material].color[:] = [0.1, 0.2, 0.31]
    ref2, rst2 = _oracle(two, 4)
    assert np.abs(ref2 - ref).max() > 0.01, "one class and two must not look alike"
    gpu_ctx.upload(pair)
    img2, st2 = gpu_ctx.render(pair.camera, 4, precision="f64")
    _rel_within(img2, ref2, "pair differing in one coordinate")
    assert _counts(st2, GEOMETRY) == _counts(rst2, GEOMETRY)


# ------------------------------------------------------------ 6: f32 against the f64 device frame
def f32_parity(ctx, rtc):
    """{world: (share of frame pixels, share of random rays)} of f32 within 2/255 of the f64 device results."""
    out = {}
    worlds = {"ico bilinear": (X.ico_over_plane(rtc, X.colors(5, 7), "bilinear"), 3),
              "ico nearest": (X.ico_over_plane(rtc, X.colors(5, 7), "nearest"), 3),
              "ico glass": (X.ico_over_plane(rtc, X.SIX, "bilinear", material=M.glass()), 4),
              "tori": (X.torus_instances(rtc, X.colors(5, 7), "bilinear"), 3)}
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
        print(f"{name}: pixels {pixels:.6f} ({round(pixels * 4800)} / 4800) rays {rays:.6f} ({round(rays * 4096)} / 4096)")
    for name, (pixels, rays) in shares.items():
        assert pixels >= F32_FLOOR_PIXELS, (name, pixels)
        assert rays >= F32_FLOOR_RAYS, (name, rays)


# ------------------------------------------------------------ 7: the CLI
@pytest.mark.parametrize("filt", ["bilinear", "nearest"])
def test_cli_texture(rtc, tmp_path, filt):
    from test_cli import CLI, SCENE
    from rtc_amd import world as W
    yaml = tmp_path / "scene.yaml"
    yaml.write_text(SCENE)
    quad = X.QUAD * 0.8 + np.array([0.0, 0.6, 0.0])
    obj = tmp_path / "quad.obj"
    obj.write_text(X.obj_text(quad, np.array([(0, 1, 2), (0, 2, 3)]), np.array([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)])))
    image = X.colors(5, 7)
    tex = tmp_path / "t.ppm"
    rtc.write_image(str(tex), image, "ppm")
    out = tmp_path / "out.png"
    r = subprocess.run([CLI, str(yaml), str(out), "--obj", str(obj), "--texture", str(tex), "--precision", "f64", "--width",
                        "80", "--height", "60"] + (["--texture-filter", filt] if filt != "bilinear" else []),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "5 x 7 texels" in r.stdout and "2 triangles with texture coordinates" in r.stdout, r.stdout
    scene = rtc.load_scene(str(yaml))
    cam = rtc.camera_resize(scene.camera, 80, 60)
    n, nm, npat = len(scene.shapes), len(scene.materials), len(scene.patterns)
    mesh = rtc.load_obj(str(obj), texcoords=True)
    tri = mesh.shape_descs(None, False, nm)
    shapes = (rtc.ShapeDesc * (n + len(tri)))()
    C.memmove(shapes, scene.shapes, n * C.sizeof(rtc.ShapeDesc))
    C.memmove(C.byref(shapes, n * C.sizeof(rtc.ShapeDesc)), tri, len(tri) * C.sizeof(rtc.ShapeDesc))
    mats = (rtc.MaterialDesc * (nm + 1))()
    C.memmove(mats, scene.materials, nm * C.sizeof(rtc.MaterialDesc))
    mats[nm] = W.World([], [W.sphere()]).tables().materials[0]  # Material::default as the tables hold it
    mats[nm].pattern = npat
    pats = (rtc.PatternDesc * (npat + 1))()
    C.memmove(pats, scene.patterns, npat * C.sizeof(rtc.PatternDesc))
    pats[npat] = W.World([], [W.sphere(W.Material(pattern=W.image_pattern(image, filt)))]).tables().patterns[0]
    tables = rtc.SceneTables(shapes, mats, pats, scene.lights, cam, uvs=mesh.uv_descs(first=n),
                             textures=[rtc.read_image(str(tex))])
    with rtc.Context(0) as c:
        c.upload(tables)
        assert c.texture_info()["textured_triangles"] == 2
        want, _ = c.render(cam, 6, precision="f64", out_format="u8")
    ref = tmp_path / "ref.png"
    assert rtc._lib.rt_image_write(str(ref).encode(), want.ctypes.data_as(C.c_void_p), 80, 60) == rtc.RT_OK
    assert out.read_bytes() == ref.read_bytes()
    plain = tmp_path / "plain.png"
    r = subprocess.run([CLI, str(yaml), str(plain), "--obj", str(obj), "--precision", "f64", "--width", "80", "--height", "60"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and plain.read_bytes() != out.read_bytes()
