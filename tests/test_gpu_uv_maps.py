"""Texture maps on the GPU (worlds in tests/uv_map_worlds.py, the conditions of the references
in tests/test_uv_maps_cpu.py).

  1. designed rays: 2048 rays aimed at known points of a unit sphere, cylinder and cube; the f64 colour is the
     restatement's sample(map(p)) within 1e-9, under both filters, with and without a turned pattern;
  2. the oracle on whole frames: a 2 x 1 texture under the nearest filter is the oracle's stripes under each
     map, through every entry point, opaque (the direct kernel), behind glass (the pool kernel) and under an
     area light;
  3. one-colour textures are the oracle's material colour under every map and filter on every shape kind;
  4. bit identity: the planar map named, knobs and skips, a group of one rank, table reuse, textured triangles;
  5. f32 against the f64 device results.

Frames are 64 x 48, ray batches 2048 rays.
"""
import numpy as np
import pytest

import lens_reference as LR
import mesh_worlds as M
import smooth_worlds as S
import uv_map_reference as U
import uv_map_worlds as X
from test_supersample_cpu import box_mean

pytestmark = pytest.mark.gpu

ABS64 = 1e-9  # the project's f64 bar
MARGIN = 1e-6
COUNTERS = ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned", "refract_evals", "schlick_evals")
GEOMETRY = tuple(c for c in COUNTERS if c != "lit_patterned")

# f32 against the f64 device results of the same upload (test 5): the share of 3072 frame pixels / of 2048
# designed rays whose colour is within 2/255 in every channel.  Floors by DESIGN.md §3.7's rule, the minimum
# observed on the MI355X less 0.005 (profiles/uv_map_parity.json holds the observations):
#                    observed minimum          floor
#   frame pixels     3072 / 3072 = 1.000000    0.995000   (the globe, the cylinder and the cube map alike)
#   designed rays    2048 / 2048 = 1.000000    0.995000   (all three, in each of three runs)
F32_TOL = 2.0 / 255.0
F32_MIN_PIXELS, F32_MIN_RAYS = 3072, 2048
F32_FLOOR_PIXELS = F32_MIN_PIXELS / 3072.0 - 0.005
F32_FLOOR_RAYS = F32_MIN_RAYS / 2048.0 - 0.005


def _counts(st, keys=COUNTERS):
    return {k: st[k] for k in keys}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint8 else a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _within(img, ref, what, mask=None):
    err = np.abs(img - ref).max(axis=-1)
    err = np.where(np.isfinite(err), err, np.inf)
    if mask is not None:
        err = np.where(mask, err, 0.0)
    worst = np.unravel_index(int(err.argmax()), err.shape)
    print(f"{what}: max |err| {err[worst]:.3g}")
    assert err[worst] < ABS64, f"{what}: {int((err >= ABS64).sum())} values differ, worst at {worst}: {err[worst]}"


def _rel_within(img, ref, what):
    scale = np.maximum(1.0, np.abs(ref))
    _within(img / scale, ref / scale, what)


# ------------------------------------------------------------ 1: designed rays
@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
@pytest.mark.parametrize("shape,map_name,turned", X.DESIGNED)
def test_designed_rays_show_the_restatements_colours(gpu_ctx, rtc, shape, map_name, turned, filt):
    transform = X.turned() if turned else None
    rays, want, margin = X.designed_reference(shape, map_name, filt, transform)
    sound = margin >= MARGIN
    assert sound.mean() >= 0.99
    tables = X.designed(shape, map_name, filt, transform)
    assert tables.mapped and len(tables.maps) == 1 and len(tables.textures) == (6 if map_name == "cube" else 1)
    gpu_ctx.upload(tables)
    info = gpu_ctx.map_info()
    assert info["mapped_patterns"] == 1 and info["cube_maps"] == (1 if map_name == "cube" else 0), info
    rgb, t, hit, st = gpu_ctx.trace_rays(rays, 2, precision="f64", hits=True)
    assert gpu_ctx.map_info()["ran_mapped"] == 1 and gpu_ctx.texture_info()["ran_textured"] == 1
    assert (hit == 0).all() and st["shaded"] == X.N_RAYS and st["lit_patterned"] > 0
    assert np.abs(t - np.linalg.norm(rays[:, :3], axis=1) * 0.5).max() < 1e-12  # the hit is the point aimed at
    _within(rgb, want, f"{shape} {map_name} {filt} turned={turned}", sound)
    # the rays left out are few, and they too show a colour of the texture (nothing reads out of bounds)
    assert np.isfinite(rgb).all() and rgb.min() >= 0.0 and rgb.max() <= 1.0


# ------------------------------------------------------------ 2: the oracle on whole frames
def _oracle_frames(oracle, rtc, tables, depth):
    cam = tables.camera
    w, h = X.FRAME
    cn = rtc.camera_resize(cam, 2 * w, 2 * h)
    t = tables.expanded()
    out = {"frame": oracle.render(t, cam, depth, threads=8), "fine": oracle.render(t, cn, depth, threads=8),
           "lens": LR.lens_frame(oracle, t, cn, w, h, 2, X.LENS[0], X.LENS[1], False, 0, depth)}
    rays = S.camera_rays(cam)
    out["rays"] = oracle.color_at(t, rays, depth)
    return out, rays


@pytest.mark.parametrize("shape,glass,area", [(s, g, False) for s in X.SHAPES for g in (False, True)] + [("sphere", False, True)])
def test_a_two_texel_texture_is_the_oracles_stripes_under_each_map(gpu_ctx, rtc, oracle, shape, glass, area):
    """render, render_supersampled(2), render_lens, shard 1 of 2, trace_rays, color_at and u8 of the mapped world
    against the oracle's world of stripes: every pixel within 1e-9, all eight counters equal.  (No hit of these
    frames lies within 1e-6 of a plane where the two differ: tests/test_uv_maps_cpu.py.)"""
    depth = 4
    what = f"{shape} glass={glass} area={area}"
    mapped, stripes = X.tie(shape, True, glass, area), X.tie(shape, False, glass, area)
    assert mapped.mapped and mapped.lit == area and mapped.has_secondary() == glass
    want, rays = _oracle_frames(oracle, rtc, stripes, depth)
    cam = mapped.camera
    gpu_ctx.upload(mapped)
    info = gpu_ctx.map_info()
    assert info["mapped_patterns"] == 1 and info["cube_maps"] == (1 if shape == "cube" else 0)
    img, st = gpu_ctx.render(cam, depth, precision="f64")
    assert gpu_ctx.map_info()["ran_mapped"] == 1 and gpu_ctx.light_info()["ran_area"] == (1 if area else 0)
    ref, rst = want["frame"]
    _rel_within(img, ref, f"{what}: frame")
    assert _counts(st) == _counts(rst), what
    assert (st["refract"] > 0 and st["reflect"] > 0) == glass and st["lit_patterned"] > 800
    ss, st2 = gpu_ctx.render_supersampled(cam, 2, depth, precision="f64")
    _rel_within(ss, box_mean(want["fine"][0], 2), f"{what}: supersampled")
    assert _counts(st2) == _counts(want["fine"][1]), what
    lens, st3 = gpu_ctx.render_lens(cam, 2, rtc.Lens(X.LENS[0], X.LENS[1], False, 0), depth, precision="f64")
    _rel_within(lens, want["lens"][0], f"{what}: lens")
    assert _counts(st3) == _counts(want["lens"][1]), what
    assert np.abs(lens - ss).mean() > 1e-5  # the lens is there
    strip, _ = gpu_ctx.render(cam, depth, precision="f64", shard=(1, 2))
    shard, row = rtc.shard_row_map(cam.height, 2)
    rows = np.nonzero(shard == 1)[0]
    _rel_within(strip[row[rows]], ref[rows], f"{what}: shard 1 of 2")
    rgb, st4 = gpu_ctx.trace_rays(rays, depth, precision="f64")
    _rel_within(rgb, want["rays"][0], f"{what}: trace_rays")
    assert _counts(st4) == _counts(want["rays"][1]), what
    rgb, st5 = gpu_ctx.color_at(rays, depth, precision="f64")
    _rel_within(rgb, want["rays"][0], f"{what}: color_at")
    assert _counts(st5) == _counts(want["rays"][1]), what
    u8, _ = gpu_ctx.render(cam, depth, precision="f64", out_format="u8")
    assert np.abs(u8.astype(int) - oracle.quantize(ref).astype(int)).max() <= 1, what
    # both stripes show on the shape
    assert ref.std() > 0.05


# ------------------------------------------------------------ 3: one-colour textures
def _kinds_world(pattern, colour):
    """One shape of every kind over a plane, all with `pattern()` (or the material colour when None)."""
    from rtc_amd import world as W

    def mat(**kw):
        return W.Material(color=(1.0, 1.0, 1.0) if pattern else colour, pattern=pattern() if pattern else None,
                          specular=0.4, shininess=50.0, **kw)
    shapes = [W.plane(mat(), transform=W.translation(0.0, -1.4, 0.0)),
              W.sphere(mat(), transform=W.mat_mul(W.translation(-1.6, 0.0, 0.4), W.scaling(0.6, 0.6, 0.6))),
              W.cube(mat(), transform=W.mat_mul(W.translation(1.5, -0.2, 0.6), W.mat_mul(W.rotation_y(0.5), W.scaling(0.5, 0.5, 0.5)))),
              W.cylinder(-0.7, 0.8, True, mat(), transform=W.mat_mul(W.translation(0.0, -0.3, 0.9), W.scaling(0.5, 1.0, 0.5))),
              W.cone(-0.9, 0.0, True, mat(), transform=W.mat_mul(W.translation(-0.6, 0.3, -0.9), W.scaling(0.5, 0.9, 0.5))),
              W.triangle((0.4, -1.0, -1.2), (1.4, -1.0, -0.8), (0.8, 0.2, -1.0), mat()),
              W.sphere(mat(reflectiveness=0.3, transparency=0.5, refractive_index=1.4),
                       transform=W.mat_mul(W.translation(0.5, 1.0, -1.5), W.scaling(0.35, 0.35, 0.35)))]
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    return W.World(lights, shapes).tables(X.camera())


@pytest.fixture(scope="module")
def one_colour_reference(oracle):
    rgb = (200, 120, 40)
    ref, rst = oracle.render(_kinds_world(None, tuple(c / 255.0 for c in rgb)), None, 4, threads=8)
    ref.setflags(write=False)
    return rgb, ref, rst


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
@pytest.mark.parametrize("map_name", ["planar", "spherical", "cylindrical", "cube"])
def test_a_texture_of_one_colour_is_the_oracles_material_colour(gpu_ctx, one_colour_reference, map_name, filt):
    rgb, ref, rst = one_colour_reference
    sizes = [(1, 1), (3, 2), (2, 5), (1, 1), (4, 1), (1, 3)]
    images = [X.uniform(w, h, rgb) for w, h in sizes]
    tables = _kinds_world(lambda: X.mapped_pattern(map_name, filt, images if map_name == "cube" else images[1], X.turned()), None)
    assert tables.mapped == (map_name != "planar")
    gpu_ctx.upload(tables)
    img, st = gpu_ctx.render(tables.camera, 4, precision="f64")
    _rel_within(img, ref, f"one colour {map_name} {filt}")
    assert _counts(st, GEOMETRY) == _counts(rst, GEOMETRY) and st["refract"] > 0
    assert st["lit_patterned"] > rst["lit_patterned"] == 0
    assert gpu_ctx.map_info()["ran_mapped"] == (1 if map_name != "planar" else 0)


# ------------------------------------------------------------ 4: bit identity
def _results(ctx, tables, depth, rays, flags=0):
    cam, out = tables.camera, {}
    for precision in ("f32", "f64"):
        out[f"render {precision}"] = ctx.render(cam, depth, precision=precision, flags=flags)
        out[f"supersampled {precision}"] = ctx.render_supersampled(cam, 2, depth, precision=precision, flags=flags)
        rgb, t, shape, st = ctx.trace_rays(rays, depth, precision=precision, hits=True, flags=flags)
        out[f"trace_rays {precision}"] = (np.concatenate([rgb, t[:, None]], axis=1), st)
    return out


def _same(got, want, what):
    for key, (a, sa) in got.items():
        b, sb = want[key]
        diff = np.argwhere(_bits(a) != _bits(b))
        assert len(diff) == 0, f"{what} {key}: {len(diff)} values differ, first at {tuple(diff[0])}"
        assert _counts(sa) == _counts(sb), f"{what} {key}"


def _all_maps_world(glass=True):
    """A sphere, a cylinder and a cube, each under its own map with 5 x 7 textures and a turned pattern, over a
    planar-textured floor, with a glass sphere in front."""
    from rtc_amd import world as W
    shapes = [W.plane(W.Material(pattern=X.mapped_pattern("planar", "bilinear"), specular=0.0), transform=W.translation(0.0, -1.4, 0.0)),
              W.sphere(W.Material(pattern=X.mapped_pattern("spherical", "bilinear", transform=X.turned())),
                       transform=W.mat_mul(W.translation(-1.5, 0.0, 0.5), W.scaling(0.7, 0.7, 0.7))),
              W.cylinder(-0.8, 0.8, True, W.Material(pattern=X.mapped_pattern("cylindrical", "nearest")),
                         transform=W.mat_mul(W.translation(0.0, -0.2, 1.0), W.scaling(0.6, 1.0, 0.6))),
              W.cube(W.Material(pattern=X.mapped_pattern("cube", "bilinear", transform=W.scaling(1.2, 0.9, 1.1))),
                     transform=W.mat_mul(W.translation(1.5, -0.2, 0.4), W.mat_mul(W.rotation_y(0.6), W.scaling(0.6, 0.6, 0.6))))]
    if glass:
        shapes.append(W.sphere(M.glass(), transform=W.mat_mul(W.translation(0.4, 0.6, -2.0), W.scaling(0.5, 0.5, 0.5))))
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    return W.World(lights, shapes).tables(X.camera())


def test_the_planar_map_named_is_the_unmapped_upload(rtc):
    unmapped = _all_maps_world()
    unmapped.maps = None  # every image pattern planar, through rt_scene_upload_textured
    named = _all_maps_world()
    for k, m in enumerate(named.maps):  # every image pattern named, with the planar map
        m.map = rtc.TEXTURE_MAPS["planar"]
        m.faces[:] = [-1] * 6
    assert len(named.maps) == 3 and not unmapped.mapped and named.mapped
    rays = M.random_rays(X.N_RAYS, 4321)
    with rtc.Context(0) as a, rtc.Context(0) as b:
        a.upload(unmapped)
        b.upload(named)
        assert all(v == 0 for v in a.map_info().values()) and all(v == 0 for v in b.map_info().values())
        want = _results(a, unmapped, 4, rays)
        _same(_results(b, named, 4, rays), want, "RT_MAP_PLANAR named")
        assert b.map_info()["ran_mapped"] == 0 and b.texture_info()["ran_textured"] == 1
        assert want["render f64"][1]["refract"] > 0
        # and the maps change the picture
        b.upload(_all_maps_world())
        other, _ = b.render(named.camera, 4, precision="f64")
        assert np.abs(other - want["render f64"][0]).max() > 0.05 and b.map_info()["mapped_patterns"] == 3


def test_knobs_skips_and_a_group_of_one_rank_change_no_bit(rtc, monkeypatch):
    tables = _all_maps_world()
    rays = M.random_rays(X.N_RAYS, 4321)
    with rtc.Context(0) as c:
        c.upload(tables)
        assert c.map_info() == {"mapped_patterns": 3, "cube_maps": 1, "ran_mapped": 0}
        want = _results(c, tables, 4, rays)
        assert c.map_info()["ran_mapped"] == 1
        c.set_jit(rtc.RT_JIT_SYNC)  # a world with textures takes no per-scene build
        c.render(tables.camera, 4, precision="f32")
        js = c.jit_status()
        assert not js["used"] and "the world has textures" in js["log"], js
        _same(_results(c, tables, 4, rays, rtc.RT_FLAG_NO_SKIPS), want, "RT_FLAG_NO_SKIPS")
    monkeypatch.setenv("RTC_DEBUG", "cull=0")
    with rtc.Context(0) as c:
        c.upload(tables)
        _same(_results(c, tables, 4, rays), want, "cull=0")
    monkeypatch.delenv("RTC_DEBUG")
    with rtc.Context.multi([0]) as g:  # a group of one rank carries the longer texture table
        g.upload(tables)
        assert g.map_info()["mapped_patterns"] == 3 and g.map_info()["cube_maps"] == 1
        _same(_results(g, tables, 4, rays), want, "a group of one rank")
        assert g.map_info()["ran_mapped"] == 1


def test_tables_are_reused_mapped_plain_mapped(rtc):
    from rtc_amd import world as W
    mapped = _all_maps_world()
    plain = W.World([W.Light((-5.0, 6.0, -5.0), (0.9, 0.9, 0.9))],
                    [W.sphere(), W.plane(W.Material(pattern=W.checker_pattern((1, 1, 1), (0, 0, 0))), transform=W.translation(0, -1, 0))]
                    ).tables(X.camera())

    def fresh(t):
        with rtc.Context(0) as c:
            c.upload(t)
            return [c.render(t.camera, 3, precision=p) for p in ("f32", "f64")]

    want = {"plain": fresh(plain), "mapped": fresh(mapped)}
    with rtc.Context(0) as c:
        for name, t in (("mapped", mapped), ("plain", plain), ("mapped", mapped), ("plain", plain)):
            c.upload(t)
            if name == "plain":
                assert all(v == 0 for v in c.map_info().values()), c.map_info()
            for (a, sa), p in zip(want[name], ("f32", "f64")):
                b, sb = c.render(t.camera, 3, precision=p)
                assert np.array_equal(_bits(a), _bits(b)) and _counts(sa) == _counts(sb), (name, p)
            assert c.map_info()["ran_mapped"] == (1 if name == "mapped" else 0)
            assert c.map_info()["mapped_patterns"] == (3 if name == "mapped" else 0)


def test_a_textured_triangle_ignores_its_patterns_map(gpu_ctx, rtc):
    """Triangles with texture coordinates under a spherical-mapped and under a cube-mapped pattern sample the
    pattern's own texture at their coordinates: the same upload unmapped, bit for bit."""
    from rtc_amd import world as W
    image = X.face_images()[1]
    p3 = ((0.0, 1.2, 0.1), (-1.3, -0.9, 0.0), (1.1, -0.8, -0.2))
    frames = {}
    for name in ("spherical", "cube", "planar"):
        def pattern():
            return X.mapped_pattern(name, "bilinear", transform=X.turned())
        tris = [W.textured_triangle(*p3, (0.03, 0.07), (0.93, 0.11), (0.41, 0.97), W.Material(pattern=pattern())),
                W.textured_triangle(*[(x + 1.2, y, z + 0.5) for x, y, z in p3], (-0.4, 0.2), (1.6, 0.1), (0.5, 1.3), W.Material(pattern=pattern()))]
        tables = W.World([W.Light((-2.0, 3.0, -5.0), (0.9, 0.9, 0.9))], tris).tables(X.camera())
        assert tables.mapped == (name != "planar") and len(tables.uvs) == 2
        gpu_ctx.upload(tables)
        frames[name] = [gpu_ctx.render(tables.camera, 2, precision=p)[0] for p in ("f32", "f64")]
        assert gpu_ctx.map_info()["ran_mapped"] == (1 if name != "planar" else 0)
    for name in ("spherical", "cube"):
        for a, b in zip(frames[name], frames["planar"]):
            assert np.array_equal(_bits(a), _bits(b)), name
    assert frames["planar"][1].std() > 0.05


# ------------------------------------------------------------ 5: f32 against the f64 device results
def f32_parity(ctx):
    """{world: (share of frame pixels, share of the designed rays)} of f32 within 2/255 of the f64 device results:
    the globe, the cylinder and the cube map, 5 x 7 textures under the bilinear filter, turned patterns."""
    out = {}
    for shape in X.SHAPES:
        map_name = X.NATURAL[shape]
        from rtc_amd import world as W
        mat = W.Material(pattern=X.mapped_pattern(map_name, "bilinear", transform=X.turned()), specular=0.3)
        floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                        transform=W.translation(0.0, -1.6, 0.0))
        lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
        tables = W.World(lights, [floor, X.unit_shape(shape, mat)]).tables(X.camera())
        rays, _ = U.designed_rays(shape, X.N_RAYS, X.SEED)
        ctx.upload(tables)
        f64, _ = ctx.render(tables.camera, 3, precision="f64")
        f32, _ = ctx.render(tables.camera, 3, precision="f32")
        r64, _ = ctx.trace_rays(rays, 3, precision="f64")
        r32, _ = ctx.trace_rays(rays, 3, precision="f32")
        out[shape] = (M.share_within(f32.astype(np.float64), f64, F32_TOL), M.share_within(r32, r64, F32_TOL))
    return out


def test_f32_stays_within_two_levels_of_the_f64_results(gpu_ctx):
    shares = f32_parity(gpu_ctx)
    for name, (pixels, rays) in shares.items():
        print(f"{name}: pixels {pixels:.6f} ({round(pixels * 3072)} / 3072) rays {rays:.6f} ({round(rays * 2048)} / 2048)")
    for name, (pixels, rays) in shares.items():
        assert pixels >= F32_FLOOR_PIXELS, (name, pixels)
        assert rays >= F32_FLOOR_RAYS, (name, rays)


# ------------------------------------------------------------ 6: the CLI
@pytest.mark.parametrize("mode", ["spherical", "cylindrical", "cube"])
def test_cli_texture_map_and_cube_map(rtc, tmp_path, mode):
    """--obj (a file without vt lines) with --texture --texture-map, or with --cube-map, writes Context.render's
    image of the same tables byte for byte, and another image than the planar map's."""
    import ctypes as C
    import subprocess
    from test_cli import CLI, SCENE
    from rtc_amd import world as W
    yaml = tmp_path / "scene.yaml"
    yaml.write_text(SCENE)
    verts, faces = M.icosphere(1)
    obj = tmp_path / "ico.obj"
    obj.write_text(S.obj_text(verts * 0.9 + np.array([0.0, 0.9, 0.0]), faces, None))
    images = X.face_images()
    files = []
    for f, image in enumerate(images):
        files.append(tmp_path / f"face{f}.ppm")
        rtc.write_image(str(files[-1]), image, "ppm")
    out = tmp_path / "out.png"
    switches = ["--cube-map", ",".join(str(f) for f in files)] if mode == "cube" else ["--texture", str(files[1]), "--texture-map", mode]
    common = [CLI, str(yaml), None, "--obj", str(obj), "--precision", "f64", "--width", "64", "--height", "48", "--texture-filter", "nearest"]
    r = subprocess.run(common[:2] + [str(out)] + common[3:] + switches, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("5 x 7 texels") == (6 if mode == "cube" else 1), r.stdout
    scene = rtc.load_scene(str(yaml))
    cam = rtc.camera_resize(scene.camera, 64, 48)
    n, nm, npat = len(scene.shapes), len(scene.materials), len(scene.patterns)
    tri = rtc.load_obj(str(obj)).shape_descs(None, False, nm)
    shapes = (rtc.ShapeDesc * (n + len(tri)))()
    C.memmove(shapes, scene.shapes, n * C.sizeof(rtc.ShapeDesc))
    C.memmove(C.byref(shapes, n * C.sizeof(rtc.ShapeDesc)), tri, len(tri) * C.sizeof(rtc.ShapeDesc))
    mats = (rtc.MaterialDesc * (nm + 1))()
    C.memmove(mats, scene.materials, nm * C.sizeof(rtc.MaterialDesc))
    mats[nm] = W.World([], [W.sphere()]).tables().materials[0]  # Material::default as the tables hold it
    mats[nm].pattern = npat
    pats = (rtc.PatternDesc * (npat + 1))()
    C.memmove(pats, scene.patterns, npat * C.sizeof(rtc.PatternDesc))
    pats[npat] = W.World([], [W.sphere(W.Material(pattern=W.image_pattern(images[1], "nearest")))]).tables().patterns[0]
    entry = rtc.UVMapDesc(npat, rtc.TEXTURE_MAPS[mode])
    entry.faces[:] = [0, 1, 2, 3, 4, 5] if mode == "cube" else [-1] * 6
    if mode == "cube":
        pats[npat].sub_a = 1  # (the front face's texture)
    tables = rtc.SceneTables(shapes, mats, pats, scene.lights, cam, maps=(rtc.UVMapDesc * 1)(entry),
                             textures=[rtc.read_image(str(f)) for f in (files if mode == "cube" else files[1:2])])
    with rtc.Context(0) as c:
        c.upload(tables)
        assert c.map_info()["mapped_patterns"] == 1 and c.map_info()["cube_maps"] == (1 if mode == "cube" else 0)
        want, _ = c.render(cam, 6, precision="f64", out_format="u8")
        assert c.map_info()["ran_mapped"] == 1
    ref = tmp_path / "ref.png"
    assert rtc._lib.rt_image_write(str(ref).encode(), want.ctypes.data_as(C.c_void_p), 64, 48) == rtc.RT_OK
    assert out.read_bytes() == ref.read_bytes()
    planar = tmp_path / "planar.png"
    r = subprocess.run(common[:2] + [str(planar)] + common[3:] + ["--texture", str(files[1])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and planar.read_bytes() != out.read_bytes(), r.stderr
