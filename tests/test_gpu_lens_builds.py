"""Lens frames (rt_render_lens) of instanced, smooth and textured worlds on the GPU.

rtc_ss_frames.inc compiles once more per build with lens_ray in camera_ray's place; in the instanced and the
textured build shade_ray walks the triangle hierarchy and the instance table behind it and interpolates
vertex normals and texture coordinates at the hit.  tests/test_gpu_lens.py holds the plain build's lens
kernels to the oracle; here the other two builds' are held to independent references:

  a. instanced worlds, f64: the oracle's ordered mean over the lens rays in the expansion's world;
  b. smooth worlds, f64: tests/smooth_reference.py over the lens rays;
  c. textured worlds, f64: tests/texture_reference.py over the lens rays, and the oracle where a texture
     means one of its patterns (2 x 1 nearest: stripes; 2 x 1 bilinear: a gradient; one colour: the colour);
  d. bit identity with the expansion and under the switches (no LDS world, RT_FLAG_NO_SKIPS, no triangle
     tree), shards, u8, aperture 0: what reaches the f32, `global` and `dup` kernels;
  e. f32 against the references of a-c;
  f. the CLI.

The cases and their references live in tests/test_lens_builds_cpu.py, which also checks without a GPU that
the numpy references leave out at most 0.001 of the pixels (a pixel is compared only if every one of its
rays keeps every decision further than 1e-9 from its threshold) and that the lens visibly changes them.
Every f64 comparison prints its largest error (about 1e-14 is expected).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import f32_tolerance
import f32_tolerance_lens
import mesh_worlds as M
import smooth_worlds as S
import test_lens_builds_cpu as K
import texture_worlds as X
from test_gpu_kernel_ids import global_ctx  # noqa: F401  (the fixture: a context without the LDS world)
from test_supersample_cpu import near_boundary

pytestmark = pytest.mark.gpu

ABS64 = K.ABS64
COUNTERS = ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned", "refract_evals", "schlick_evals")
# (a texture is a pattern: a textured world counts more lit_patterned than the untextured world of its colours)
GEOMETRY = tuple(c for c in COUNTERS if c != "lit_patterned")
SEED = K.SEED
RGB = (200, 120, 40)
COLOUR = tuple(c / 255.0 for c in RGB)
A2, B2 = (200, 40, 90), (30, 220, 140)
TWO = np.array([[A2, B2]], dtype=np.uint8)  # 2 x 1


def _counts(st, keys=COUNTERS):
    return {k: st[k] for k in keys}


def _lens(rtc, lens, jitter):
    return rtc.Lens(lens[0], lens[1], jitter, SEED)


def _within(img, ref, what, mask=None):
    err = np.abs(img - ref).max(axis=-1)
    err = np.where(np.isfinite(err), err, np.inf)
    if mask is not None:
        err = np.where(mask, err, 0.0)
    worst = np.unravel_index(int(err.argmax()), err.shape)
    print(f"{what}: max |err| {err[worst]:.3g}")
    assert err[worst] < ABS64, f"{what}: {int((err >= ABS64).sum())} pixels differ, worst at {worst}: {err[worst]}"


def _visible(ctx, cam, n, depth, img, what):
    pin, _ = ctx.render_supersampled(cam, n, depth, precision="f64")
    change = float(np.abs(img - pin).mean())
    assert change > K.VISIBLE, f"{what}: the lens changes the frame by {change} only"


@pytest.fixture(scope="module")
def notree_ctx(rtc):
    """A context that builds no triangle hierarchy (RTC_DEBUG=tri_tree=0, read when a context is created)."""
    before = os.environ.get("RTC_DEBUG")
    os.environ["RTC_DEBUG"] = "tri_tree=0" if not before else before + ",tri_tree=0"
    try:
        ctx = rtc.Context(0)
    finally:
        if before is None:
            del os.environ["RTC_DEBUG"]
        else:
            os.environ["RTC_DEBUG"] = before
    yield ctx
    ctx.close()


# ------------------------------------------------------------------ a. instanced, f64 against the oracle
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("w,h,n", K.SHAPES)
@pytest.mark.parametrize("key", K.INSTANCED)
def test_instanced_f64_matches_the_oracle_on_the_expansion(gpu_ctx, rtc, key, w, h, n, jitter):
    tables, _, depth = K.instanced_world(key)
    gpu_ctx.upload(tables)
    info = gpu_ctx.instance_info()
    assert info["instances"] == len(tables.instances) and info["expanded"] == 0, info  # no fallback to plain records
    if key == "beside_plain":
        assert gpu_ctx.tree_info()["records_in_tree"] == 512
    cam = rtc.camera_resize(tables.camera, w, h)
    img, st = gpu_ctx.render_lens(cam, n, _lens(rtc, K.INSTANCED_LENS, jitter), depth, precision="f64")
    ref, rst = K.instanced_lens_frame(key, w, h, n, jitter)
    assert img.shape == (h, w, 3)
    _within(img, ref, f"instanced {key} {w}x{h} n={n} jitter {jitter}")
    assert _counts(st) == _counts(rst) and st["primary"] == n * n * w * h
    if key in ("nested_glass", "small"):
        assert st["refract"] > 0 and st["reflect"] > 0  # the pool kernel
    _visible(gpu_ctx, cam, n, depth, img, key)


# ------------------------------------------------------------------ b, c. against the numpy references
def _against_numpy(ctx, rtc, kind, key, w, h, n, jitter, lens):
    ref, sound, counts = K.numpy_lens_frame(kind, key, w, h, n, jitter)
    left_out = 1.0 - float(sound.mean())
    print(f"{kind} {key} {w}x{h} n={n} jitter {jitter}: {left_out:.6f} of pixels left out")
    assert left_out <= K.LEFT_OUT
    world = K.smooth_world if kind == "smooth" else K.textured_world
    for pool in (False, True):
        tables, flat = world(key, pool)
        ctx.upload(tables)
        if tables.instanced:
            assert ctx.instance_info()["expanded"] == 0 and ctx.instance_info()["instances"] == 2
        if kind == "smooth" or key.startswith("smooth"):
            assert ctx.smooth_info()["smooth_triangles"] == len(flat.smooth)
        if kind == "textured":
            assert ctx.texture_info()["textured_triangles"] == len(flat.uvs) == 320
        cam = rtc.camera_resize(tables.camera, w, h)
        img, st = ctx.render_lens(cam, n, _lens(rtc, lens, jitter), 5, precision="f64")
        if kind == "smooth" or key.startswith("smooth"):
            assert ctx.smooth_info()["ran_smooth"] == 1
        if kind == "textured":
            assert ctx.texture_info()["ran_textured"] == 1
        _within(img, ref, f"{kind} {key} {'pool' if pool else 'direct'}", sound)
        assert st["primary"] == counts["primary"] == n * n * w * h and st["reflect"] == 0 and st["refract"] == 0
        if sound.all():  # (a ray on the fence may hit or miss)
            assert st["shaded"] == counts["shaded"] and st["shadow"] == counts["shadow"]
        _visible(ctx, cam, n, 5, img, key)


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("w,h,n", K.NUMPY_SHAPES)
@pytest.mark.parametrize("key", K.SMOOTH)
def test_smooth_f64_matches_the_numpy_reference(gpu_ctx, rtc, key, w, h, n, jitter):
    _against_numpy(gpu_ctx, rtc, "smooth", key, w, h, n, jitter, K.SMOOTH_LENS)


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("key", K.TEXTURED)
def test_textured_f64_matches_the_numpy_reference(gpu_ctx, rtc, key, jitter):
    for w, h, n in K.NUMPY_SHAPES[:1] if key != K.TEXTURED[-1] else K.NUMPY_SHAPES:
        _against_numpy(gpu_ctx, rtc, "textured", key, w, h, n, jitter, K.TEXTURED_LENS)


# ------------------------------------------------------------------ c. oracle anchors
def _stripes(textured):
    from rtc_amd import world as W
    from test_gpu_texture import _tie_world
    a, b = tuple(c / 255.0 for c in A2), tuple(c / 255.0 for c in B2)
    kinds = ("plane", "sphere", "glass")
    if textured:
        return _tie_world(lambda: W.image_pattern(TWO, "nearest"), kinds)
    return _tie_world(lambda: W.stripe_pattern(a, b).set_transformation(W.scaling(0.5, 1.0, 1.0)), kinds)


def _gradient(textured):
    from rtc_amd import world as W
    from test_gpu_texture import _tie_world
    a, b = tuple(c / 255.0 for c in A2), tuple(c / 255.0 for c in B2)
    inv = [[0.49, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]

    def with_inverse(p):
        p.transformation_inverse = [row[:] for row in inv]
        return p
    if textured:
        return _tie_world(lambda: with_inverse(W.image_pattern(TWO, "bilinear")), ("sphere", "glass"))
    return _tie_world(lambda: with_inverse(W.gradient_pattern(a, b)), ("sphere", "glass"))


def _pair_coords():
    verts = S.box(True)[0]
    return np.stack([0.5 + 0.25 * verts[:, 0] + 0.125 * verts[:, 2], 0.5 + 0.25 * verts[:, 1]], axis=1) + np.array([1e-3, 0.0])


def _box(rtc, filt, textured, copies=1, two_classes=False, smooth=False):
    """texture_worlds.box_world's glass box under a texture of one colour, or (textured=False) the world the
    oracle renders: glass of that colour.  copies = 2: a value-equal pair (one identity class per triangle);
    two_classes: the second copy differs in one texture coordinate, which for the oracle is a second box that
    differs by value (the first copy wins every tie, so the second's colour is never shaded)."""
    if textured:
        return X.box_world(rtc, X.uniform(3, 2, RGB), filt, copies=copies, smooth=smooth,
                           coords_of_second=_pair_coords() if two_classes else None)
    flat = X.box_world(rtc, None, filt, copies=copies, textured=False, color=COLOUR)
    if two_classes:
        for s in flat.shapes[13:]:
            flat.materials[s.material].color[:] = [0.1, 0.2, 0.31]
    return flat


ANCHORS = {
    "stripes": (_stripes, COUNTERS),
    "gradient": (_gradient, COUNTERS),
    "one colour nearest": (lambda t: _box(_rtc(), "nearest", t), GEOMETRY),
    "one colour bilinear": (lambda t: _box(_rtc(), "bilinear", t), GEOMETRY),
    "one colour smooth": (lambda t: _box(_rtc(), "bilinear", t, smooth=t), GEOMETRY),
    "one class": (lambda t: _box(_rtc(), "bilinear", t, copies=2), GEOMETRY),
    "two classes": (lambda t: _box(_rtc(), "bilinear", t, copies=2, two_classes=True), GEOMETRY),
}
ANCHOR_SHAPES = {"stripes": K.SHAPES, "one class": K.SHAPES}
_rtc = K._rtc


@pytest.fixture(scope="module")
def anchors():
    """name -> (the textured tables, the oracle's equivalent world as a cached callable), built once."""
    import functools
    out = {}
    for name, (build, _) in ANCHORS.items():
        plain = build(False)
        out[name] = (build(True), functools.partial(lambda t: t, plain))
    return out


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("name", list(ANCHORS))
def test_textured_pool_frames_match_the_oracles_equivalent_world(gpu_ctx, rtc, anchors, name, jitter):
    tables, plain_of = anchors[name]
    keys = ANCHORS[name][1]
    assert tables.textured and tables.has_secondary() and not plain_of().textured
    gpu_ctx.upload(tables)
    if name in ("one class", "two classes"):
        assert gpu_ctx.texture_info()["textured_triangles"] == 24
    for w, h, n in ANCHOR_SHAPES.get(name, K.SHAPES[:1]):
        cam = rtc.camera_resize(tables.camera, w, h)
        img, st = gpu_ctx.render_lens(cam, n, _lens(rtc, K.TEXTURED_LENS, jitter), 4, precision="f64")
        assert gpu_ctx.texture_info()["ran_textured"] == 1
        ref, rst = K.oracle_lens_frame(plain_of, w, h, n, jitter, K.TEXTURED_LENS, 4)
        _within(img, ref, f"{name} {w}x{h} n={n} jitter {jitter}")
        assert _counts(st, keys) == _counts(rst, keys) and st["refract"] > 0 and st["reflect"] > 0
        assert st["lit_patterned"] > 0
        _visible(gpu_ctx, cam, n, 4, img, name)
    if name == "two classes":  # one class and two must not look alike
        one, _ = K.oracle_lens_frame(anchors["one class"][1], *K.SHAPES[0], jitter, K.TEXTURED_LENS, 4)
        assert np.abs(one - ref).max() > 0.01


# ------------------------------------------------------------------ d. bit identity
def _identity_world(rtc, key):
    """(tables, depth, lens, twin, how the twin compares): twin is the expansion (its upload goes through
    another build, or through the same one without instances: equal bytes), or None."""
    if key in ("three_tori", "nested_glass", "repeated", "beside_plain"):
        # (repeated: a mesh with a value-equal pair of faces; that instance goes up expanded, and the world is dup)
        tables, flat, depth = K.instanced_world(key)
        return tables, depth, K.INSTANCED_LENS, flat
    if key == "smooth tori":
        tables = S.torus_instances(rtc)
        return tables, 3, K.SMOOTH_LENS, tables.expanded()
    if key == "smooth glass boxes":
        tables = S.box_instances(rtc)
        return tables, 4, K.SMOOTH_LENS, tables.expanded()
    if key == "textured tori":
        tables = X.torus_instances(rtc, K.IMAGE, "bilinear")
        return tables, 3, K.TEXTURED_LENS, tables.expanded()
    if key == "textured glass ico":
        return X.ico_over_plane(rtc, X.SIX, "nearest", material=M.glass()), 4, K.TEXTURED_LENS, None
    if key == "textured pair":
        return _box(rtc, "bilinear", True, copies=2), 4, K.TEXTURED_LENS, None
    if key == "textured pair, two classes":
        return _box(rtc, "bilinear", True, copies=2, two_classes=True), 4, K.TEXTURED_LENS, None
    raise KeyError(key)


IDENTITY = ("three_tori", "nested_glass", "repeated", "beside_plain", "smooth tori", "smooth glass boxes",
            "textured tori", "textured glass ico", "textured pair", "textured pair, two classes")


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("key", IDENTITY)
def test_switches_and_the_expansion_change_no_bit(gpu_ctx, global_ctx, notree_ctx, rtc, key, precision):  # noqa: F811
    tables, depth, lens, twin = _identity_world(rtc, key)
    w, h, n = K.SHAPES[0]
    cam = rtc.camera_resize(tables.camera, w, h)

    def frames(ctx, t, flags=0):
        ctx.upload(t)
        return [ctx.render_lens(cam, n, _lens(rtc, lens, jitter), depth, precision=precision, flags=flags)
                for jitter in (False, True)]

    want = frames(gpu_ctx, tables)
    info = gpu_ctx.instance_info()
    if tables.instanced:
        assert info["instances"] == len(tables.instances) and info["expanded"] == (1 if key == "repeated" else 0), info
    assert all(np.isfinite(img).all() and img.std() > 0.01 for img, _ in want)
    assert want[0][0].tobytes() != want[1][0].tobytes()
    others = {"no LDS world": frames(global_ctx, tables), "RT_FLAG_NO_SKIPS": frames(gpu_ctx, tables, rtc.RT_FLAG_NO_SKIPS),
              "no triangle tree": frames(notree_ctx, tables)}
    if twin is not None:
        others["the expansion"] = frames(gpu_ctx, twin)
        assert gpu_ctx.instance_info()["instances"] == 0
        others["the expansion, no LDS world"] = frames(global_ctx, twin)
    for what, got in others.items():
        for (a, sa), (b, sb), jitter in zip(got, want, (False, True)):
            diff = np.argwhere(a != b)
            assert len(diff) == 0, f"{key} {what} jitter {jitter}: {len(diff)} values differ, first at {tuple(diff[0])}"
            assert _counts(sa) == _counts(sb), f"{key} {what} jitter {jitter}"


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("name", ["one colour bilinear", "one colour smooth", "one class"])
def test_a_one_colour_texture_is_its_untextured_twin(gpu_ctx, rtc, anchors, name, jitter):
    """Both uploads on the device: the textured build's frame against the frame of the world whose material
    has the texture's colour (the plain build, or the instanced one for smooth normals)."""
    tables, plain_of = anchors[name]
    twin = plain_of() if name != "one colour smooth" else X.without_textures(rtc, _box(rtc, "bilinear", True, smooth=True))
    if name == "one colour smooth":
        for m in twin.materials:
            if m.transparency != 0.0:
                m.color[:] = COLOUR
    w, h, n = K.SHAPES[0]
    cam = rtc.camera_resize(tables.camera, w, h)
    lens = _lens(rtc, K.TEXTURED_LENS, jitter)
    gpu_ctx.upload(tables)
    a, sa = gpu_ctx.render_lens(cam, n, lens, 4, precision="f64")
    gpu_ctx.upload(twin)
    assert gpu_ctx.texture_info()["ran_textured"] == 0
    b, sb = gpu_ctx.render_lens(cam, n, lens, 4, precision="f64")
    _within(a, b, f"{name} against its untextured twin, jitter {jitter}")
    assert _counts(sa, GEOMETRY) == _counts(sb, GEOMETRY) and sa["refract"] > 0


def _shard_u8_zero_world(rtc, anchors, which):
    if which == "instanced":
        tables, _, depth = K.instanced_world("nested_glass")
        return tables, depth, K.INSTANCED_LENS, lambda w, h, n, jitter: K.instanced_lens_frame("nested_glass", w, h, n, jitter)
    tables, plain_of = anchors["stripes"]
    return tables, 4, K.TEXTURED_LENS, lambda w, h, n, jitter: K.oracle_lens_frame(plain_of, w, h, n, jitter, K.TEXTURED_LENS, 4)


@pytest.mark.parametrize("precision,out_format", [("f32", "real"), ("f64", "real"), ("f32", "u8"), ("f64", "u8")])
@pytest.mark.parametrize("which", ["instanced", "textured"])
def test_shards_assemble_and_aperture_zero_is_render_supersampled(gpu_ctx, rtc, anchors, which, precision, out_format):
    tables, depth, lens, _ = _shard_u8_zero_world(rtc, anchors, which)
    w, h, n = K.SHAPES[0]
    cam = rtc.camera_resize(tables.camera, w, h)
    gpu_ctx.upload(tables)
    hashed = _lens(rtc, lens, True)
    whole, st = gpu_ctx.render_lens(cam, n, hashed, depth, precision=precision, out_format=out_format)
    shard_of, row_of = rtc.shard_row_map(h, 3)
    strips, primary = [], 0
    for s in range(3):
        strip, sst = gpu_ctx.render_lens(cam, n, hashed, depth, precision=precision, out_format=out_format, shard=(s, 3))
        strips.append(strip)
        primary += sst["primary"]
    got = np.stack([strips[shard_of[y]][row_of[y]] for y in range(h)])
    assert got.tobytes() == whole.tobytes() and primary == st["primary"] == n * n * w * h
    for jitter in (False, True):
        zero = rtc.Lens(0.0, lens[1], jitter, 3)
        a, sa = gpu_ctx.render_supersampled(cam, n, depth, precision=precision, out_format=out_format)
        b, sb = gpu_ctx.render_lens(cam, n, zero, depth, precision=precision, out_format=out_format)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes() and _counts(sa) == _counts(sb)
        assert a.tobytes() != whole.tobytes()


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("which", ["instanced", "textured"])
def test_u8_is_quantized_once_after_the_mean(gpu_ctx, rtc, oracle, anchors, which, jitter):
    tables, depth, lens, reference = _shard_u8_zero_world(rtc, anchors, which)
    gpu_ctx.upload(tables)
    for w, h, n in K.SHAPES:
        img, _ = gpu_ctx.render_lens(rtc.camera_resize(tables.camera, w, h), n, _lens(rtc, lens, jitter), depth,
                                     precision="f64", out_format="u8")
        ref, _ = reference(w, h, n, jitter)
        exempt = near_boundary(ref, ABS64)
        assert exempt.mean() <= 0.001
        assert img.dtype == np.uint8 and np.array_equal(img[~exempt], oracle.quantize(ref)[~exempt])


# ------------------------------------------------------------------ e. f32 against the f64 references
F32_SHAPE = (160, 100, 2)
F32_WORLDS = ("instanced three_tori", "instanced nested_glass", "smooth direct", "smooth pool", "textured direct",
              "textured pool")


def _f32_case(name, jitter):
    """(tables, depth, lens, the reference's frame, the reference's ray counts) of a world of F32_WORLDS."""
    w, h, n = F32_SHAPE
    kind, which = name.split()
    if kind == "instanced":
        tables, _, depth = K.instanced_world(which)
        ref, rst = K.instanced_lens_frame(which, w, h, n, jitter)
        return tables, depth, K.INSTANCED_LENS, ref, {k: rst[k] for k in ("primary", "shadow", "reflect", "refract")}
    key = "ico" if kind == "smooth" else K.TEXTURED[-1]
    tables, _ = (K.smooth_world if kind == "smooth" else K.textured_world)(key, which == "pool")
    ref, sound, counts = K.numpy_lens_frame(kind, key, w, h, n, jitter)
    assert 1.0 - float(sound.mean()) <= K.LEFT_OUT
    return tables, 5, K.SMOOTH_LENS, ref, {"primary": counts["primary"], "shadow": counts["shadow"], "reflect": 0, "refract": 0}


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("name", F32_WORLDS)
def test_f32_share_within_two_levels_of_the_reference(gpu_ctx, rtc, oracle, name, jitter):
    w, h, n = F32_SHAPE
    tables, depth, lens, ref, rst = _f32_case(name, jitter)
    gpu_ctx.upload(tables)
    img, st = gpu_ctx.render_lens(rtc.camera_resize(tables.camera, w, h), n, _lens(rtc, lens, jitter), depth, precision="f32")
    d = np.abs(oracle.quantize(img.astype(np.float64)).astype(int) - oracle.quantize(ref).astype(int)).max(axis=2)
    share = float((d <= 2).mean())
    print(f"f32 parity: {name!r} jitter {jitter}: share {share:.9f} counters "
          + " ".join(f"{k} {st[k]}/{rst[k]}" for k in rst))
    for k, want in rst.items():
        assert abs(st[k] - want) <= max(3, f32_tolerance.KIND * want), (name, k, st[k], want)
    assert st["primary"] == rst["primary"] == n * n * w * h
    observed = f32_tolerance_lens.SHARE_OBSERVED[name, jitter]
    assert share >= observed - 0.005, (share, observed)


# ------------------------------------------------------------------ f. the CLI
def _scene_with_mesh(rtc, scene, cam, tri, image=None, filt="bilinear", uvs=None, smooth=None):
    """The scene's tables with the mesh's triangles after its shapes on one default material (with the image as
    its pattern), as the CLI's --obj builds them."""
    from rtc_amd import world as W
    n, nm, npat = len(scene.shapes), len(scene.materials), len(scene.patterns)
    shapes = (rtc.ShapeDesc * (n + len(tri)))()
    C.memmove(shapes, scene.shapes, n * C.sizeof(rtc.ShapeDesc))
    C.memmove(C.byref(shapes, n * C.sizeof(rtc.ShapeDesc)), tri, len(tri) * C.sizeof(rtc.ShapeDesc))
    mats = (rtc.MaterialDesc * (nm + 1))()
    C.memmove(mats, scene.materials, nm * C.sizeof(rtc.MaterialDesc))
    mats[nm] = W.World([], [W.sphere()]).tables().materials[0]  # Material::default as the tables hold it
    pats = scene.patterns
    if image is not None:
        mats[nm].pattern = npat
        pats = (rtc.PatternDesc * (npat + 1))()
        C.memmove(pats, scene.patterns, npat * C.sizeof(rtc.PatternDesc))
        pats[npat] = W.World([], [W.sphere(W.Material(pattern=W.image_pattern(image, filt)))]).tables().patterns[0]
    return rtc.SceneTables(shapes, mats, pats, scene.lights, cam, smooth=smooth, uvs=uvs,
                           textures=None if image is None else [image])


@pytest.mark.parametrize("jitter", [(), ("--lens-jitter=9",)])
def test_cli_instances_through_a_lens(tmp_path, rtc, gpu_ctx, jitter):
    from test_cli import CLI, SCENE, read_ppm
    from rtc_amd import world as W
    yaml = tmp_path / "scene.yaml"
    yaml.write_text(SCENE)
    obj = tmp_path / "ico.obj"
    obj.write_text(M.obj_text(*M.icosphere(1)))
    places = [((-1.6, 1.1, 1.0), 0.6), ((0.5, 0.9, -0.5), 0.4)]
    args = []
    for t, s in places:
        args += ["--instance", f"{obj}:{t[0]!r},{t[1]!r},{t[2]!r}:{s!r}"]
    out = tmp_path / "out.ppm"
    r = subprocess.run([CLI, str(yaml), str(out), "--width", "70", "--height", "22", "--samples", "2", "--aperture", "0.2",
                        "--focus", "5.5", *jitter, *args, "--ppm-binary", "-q"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    scene = rtc.load_scene(str(yaml))
    cam = rtc.camera_resize(scene.camera, 70, 22)
    mesh = rtc.load_obj(str(obj))
    nm = len(scene.materials)
    mats = (rtc.MaterialDesc * (nm + 1))()
    C.memmove(mats, scene.materials, nm * C.sizeof(rtc.MaterialDesc))
    mats[nm] = W.World([], [W.sphere()]).tables().materials[0]
    local = mesh.shape_descs(None, False, 0)
    inst = (rtc.InstanceDesc * len(places))()
    for d, (t, s) in zip(inst, places):
        d.mesh, d.material = 0, nm
        forward = [s, 0.0, 0.0, t[0], 0.0, s, 0.0, t[1], 0.0, 0.0, s, t[2], 0.0, 0.0, 0.0, 1.0]  # translation x scaling
        d.inverse[:] = rtc.matrix_inverse(forward).ravel().tolist()
    tables = rtc.SceneTables(scene.shapes, mats, scene.patterns, scene.lights, cam, meshes=[local], instances=inst)
    lens = rtc.Lens(0.2, 5.5, bool(jitter), 9 if jitter else 0)
    gpu_ctx.upload(tables)
    assert gpu_ctx.instance_info()["instances"] == 2 and gpu_ctx.instance_info()["expanded"] == 0
    want, _ = gpu_ctx.render_lens(cam, 2, lens, 6, precision="f32", out_format="u8")
    assert np.array_equal(read_ppm(out, b"P6"), want)
    pin, _ = gpu_ctx.render_supersampled(cam, 2, 6, precision="f32", out_format="u8")
    assert not np.array_equal(want, pin)
    gpu_ctx.upload(scene)
    bare, _ = gpu_ctx.render_lens(cam, 2, lens, 6, precision="f32", out_format="u8")
    assert (want != bare).any(axis=2).mean() > 0.02, "the copies must be in the picture"


@pytest.mark.parametrize("jitter", [(), ("--lens-jitter=9",)])
def test_cli_a_smooth_textured_mesh_through_a_lens(tmp_path, rtc, gpu_ctx, jitter):
    from test_cli import CLI, SCENE, read_ppm
    yaml = tmp_path / "scene.yaml"
    yaml.write_text(SCENE)
    verts, faces = M.icosphere(1)
    obj = tmp_path / "ico.obj"
    obj.write_text(X.obj_text(verts * 0.8 + np.array([0.0, 1.0, 0.0]), faces, X.ico_coords(verts), normals=verts.copy()))
    tex = tmp_path / "t.ppm"
    rtc.write_image(str(tex), K.IMAGE, "ppm")
    out = tmp_path / "out.ppm"
    r = subprocess.run([CLI, str(yaml), str(out), "--width", "70", "--height", "22", "--samples", "2", "--aperture", "0.2",
                        "--focus", "5.5", *jitter, "--obj", str(obj), "--smooth", "--texture", str(tex), "--precision", "f64",
                        "--ppm-binary"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "80 smooth triangles" in r.stdout and "80 triangles with texture coordinates" in r.stdout, r.stdout
    scene = rtc.load_scene(str(yaml))
    cam = rtc.camera_resize(scene.camera, 70, 22)
    mesh = rtc.load_obj(str(obj), normals=True, texcoords=True)
    n = len(scene.shapes)
    tables = _scene_with_mesh(rtc, scene, cam, mesh.shape_descs(None, False, len(scene.materials)), rtc.read_image(str(tex)),
                              "bilinear", mesh.uv_descs(first=n), mesh.smooth_descs(first=n))
    lens = rtc.Lens(0.2, 5.5, bool(jitter), 9 if jitter else 0)
    gpu_ctx.upload(tables)
    assert gpu_ctx.smooth_info()["smooth_triangles"] == 80 and gpu_ctx.texture_info()["textured_triangles"] == 80
    want, _ = gpu_ctx.render_lens(cam, 2, lens, 6, precision="f64", out_format="u8")
    assert gpu_ctx.texture_info()["ran_textured"] == 1
    assert np.array_equal(read_ppm(out, b"P6"), want)
    pin, _ = gpu_ctx.render_supersampled(cam, 2, 6, precision="f64", out_format="u8")
    assert not np.array_equal(want, pin)
