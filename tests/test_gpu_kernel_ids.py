"""The kernel identities no other test reaches (kernel_id.hpp; rtc_kernels.hip kernel_of).

DESIGN.md 3.15 lists which test reaches which kernel of which build.  The large worlds of the mesh,
instance and texture tests run most kernels that read the world from global memory (`lds = false`), but
none ran the plain build's lens kernels that way or its lens pool kernels with value-equal shapes (dup),
and of the area build none ran any `lds = false` kernel, any dup kernel, the f32 supersampled kernels or
most lens kernels.  RTC_DEBUG=lds_world=0, read when a context is created, plans every launch without the
LDS world.  Here a context made under it and the session's default context each render a 32 x 8 canvas (two
wave blocks each way) of every family (frame, supersampled, lens, ray batch), direct and pool, with and
without a value-equal pair, f32 and f64, for the plain and the area build, and the two contexts' frames of
the same call must be equal bit for bit: the two instantiations differ in the address space their table
loads go through and in nothing a value depends on (per-pixel and per-lane sums in one order, the pool's
fixed-point sums in any), and the default context's frames are the ones the other tests hold against the
oracle.  The instanced and the textured build get a world with a value-equal pair each (dup: pool, supersampled,
lens and rays, from LDS and from global memory), held to the oracle here; their lens kernels without dup are
tests/test_gpu_lens_builds.py's.  Last, what a pool world of spheres and planes reaches only without the LDS
world: the per-scene pool builds of every family with the world in global memory, and the `sp` build's
`global` pair.  DESIGN.md 3.15 says what stays unreached (a per-scene direct build with the LDS world) and why.
"""
import numpy as np
import pytest

import area_light_worlds as worlds

SIZE = (32, 8)
GRID = 2


def tables(area, mirror, dup):
    from rtc_amd import world as W
    point, lit = worlds.lights()
    shapes = worlds.shapes(mirror)
    if dup:
        shapes.append(shapes[1])  # the ball once more: one identity class of two
    return W.World(point, shapes, area_lights=lit if area else []).tables(worlds.eye(SIZE))


@pytest.fixture(scope="module")
def global_ctx(rtc):
    """A context whose launches stage no world in LDS."""
    import os
    before = os.environ.get("RTC_DEBUG")
    os.environ["RTC_DEBUG"] = "lds_world=0" if not before else before + ",lds_world=0"
    try:
        ctx = rtc.Context(0)
    finally:
        if before is None:
            del os.environ["RTC_DEBUG"]
        else:
            os.environ["RTC_DEBUG"] = before
    yield ctx
    ctx.close()


def frames(rtc, ctx, scene, precision, depth):
    """Every family's frame of `scene`: the frame, the supersampled and the lens frame, a ray batch."""
    cam = scene.camera
    ctx.upload(scene)
    out = {"frame": ctx.render(cam, depth, precision)[0],
           "supersampled": ctx.render_supersampled(cam, GRID, depth, precision)[0],
           "lens": ctx.render_lens(cam, GRID, rtc.Lens(0.15, 6.0), depth, precision)[0],
           "lens hashed": ctx.render_lens(cam, GRID, rtc.Lens(0.15, 6.0, True, 5), depth, precision)[0]}
    out["rays"] = ctx.trace_rays(worlds.seeded_rays(256, 3), depth, precision)[0]  # (a numpy batch travels as f64)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("dup", [False, True], ids=["distinct", "dup"])
@pytest.mark.parametrize("mirror", [False, True], ids=["direct", "pool"])
@pytest.mark.parametrize("area", [False, True], ids=["plain", "area"])
def test_frames_without_the_lds_world_equal_the_frames_with_it(rtc, gpu_ctx, global_ctx, area, mirror, dup, precision):
    scene = tables(area, mirror, dup)
    depth = 4 if mirror else 0
    want = frames(rtc, gpu_ctx, scene, precision, depth)
    got = frames(rtc, global_ctx, scene, precision, depth)
    assert gpu_ctx.light_info()["ran_area"] == global_ctx.light_info()["ran_area"] == int(area)
    for name, frame in want.items():
        assert frame.shape == got[name].shape and np.isfinite(frame).all(), name
        assert frame.std() > 0.01, name  # (a picture, not a blank canvas)
        assert np.array_equal(frame, got[name]), (name, float(np.abs(frame - got[name]).max()))


# ------------------------------------------------------------------ the instanced and the textured build
RGB = (90, 200, 160)
COLOUR = tuple(c / 255.0 for c in RGB)


def _on_the_small_canvas(rtc, scene):
    import dataclasses
    return dataclasses.replace(scene, camera=rtc.camera_resize(scene.camera, *SIZE))


def _textured_pair(rtc, textured, two_classes):
    """texture_worlds.box_world's two coincident glass boxes under a texture of one colour: one identity class
    per triangle, or (two_classes) two, the second copy differing in one texture coordinate.  textured=False:
    the world the oracle renders, glass of the texture's colour (the first copy wins every tie, so a second
    copy that differs by value is never shaded: any other colour serves)."""
    import smooth_worlds as S
    import texture_worlds as X
    if textured:
        verts = S.box(True)[0]
        base = np.stack([0.5 + 0.25 * verts[:, 0] + 0.125 * verts[:, 2], 0.5 + 0.25 * verts[:, 1]], axis=1)
        return X.box_world(rtc, X.uniform(3, 2, RGB), "bilinear", copies=2,
                           coords_of_second=base + np.array([1e-3, 0.0]) if two_classes else None)
    flat = X.box_world(rtc, None, "bilinear", copies=2, textured=False, color=COLOUR)
    if two_classes:
        for s in flat.shapes[13:]:
            flat.materials[s.material].color[:] = [0.1, 0.2, 0.31]
    return flat


def _build_world(rtc, tmp_path, key):
    """(the tables on the 32 x 8 canvas, depth, the oracle's world of the same picture)."""
    import instance_worlds as I
    if key == "repeated":  # an instance walked, and one whose mesh repeats a face: uploaded expanded, dup
        scene, depth = I.build_world(rtc, tmp_path, key)
        return _on_the_small_canvas(rtc, scene), depth, _on_the_small_canvas(rtc, scene.expanded())
    two = key == "textured pair, two classes"
    return (_on_the_small_canvas(rtc, _textured_pair(rtc, True, two)), 4,
            _on_the_small_canvas(rtc, _textured_pair(rtc, False, two)))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("key", ["repeated", "textured pair", "textured pair, two classes"])
def test_dup_worlds_of_the_other_builds_without_the_lds_world(rtc, gpu_ctx, global_ctx, tmp_path, key, precision):
    """A value-equal pair in the instanced and in the textured build, every family: pool, supersampled, lens
    and rays with `dup`, from LDS and from global memory.  Each world's f64 frame is the oracle's."""
    import pyoracle
    scene, depth, plain = _build_world(rtc, tmp_path, key)
    want = frames(rtc, gpu_ctx, scene, precision, depth)
    if key == "repeated":
        info = gpu_ctx.instance_info()
        assert info["instances"] == 2 and info["expanded"] == 1, info
    else:
        assert gpu_ctx.texture_info()["textured_triangles"] == 24 and gpu_ctx.texture_info()["ran_textured"] == 1
    got = frames(rtc, global_ctx, scene, precision, depth)
    for name, frame in want.items():
        assert frame.shape == got[name].shape and np.isfinite(frame).all(), name
        assert frame.std() > 0.01, name
        assert np.array_equal(frame, got[name]), (name, float(np.abs(frame - got[name]).max()))
    if precision == "f64":
        ref, rst = pyoracle.render(plain, plain.camera, depth)
        err = float(np.abs(want["frame"] - ref).max())
        print(f"{key}: f64 frame against the oracle, max |err| {err:.3g}")
        assert err < 1e-9
        if key != "repeated":
            other, _ = pyoracle.render(_build_world(rtc, tmp_path, "textured pair" if "two" in key else
                                                    "textured pair, two classes")[2], plain.camera, depth)
            assert np.abs(other - ref).max() > 0.01, "one class and two must not look alike"


# ------------------------------------------------------------------ per-scene builds and `sp` without the LDS world
RT_FLAG_NO_SKIPS = 64


def _pool_scene(rtc):
    from conftest import scene_fixture
    scene = scene_fixture("reflect_refract")  # spheres and planes only, reflective and transparent
    assert all(s.kind in (0, 1) for s in scene.shapes) and scene.has_secondary()
    return scene, rtc.camera_resize(scene.camera, 70, 22)


def _families(rtc, ctx, cam, flags=0):
    lens = rtc.Lens(0.25, 5.0, True, 1)
    return {"frame": ctx.render(cam, 6, "f32", flags=flags)[0],
            "supersampled": ctx.render_supersampled(cam, GRID, 6, "f32", flags=flags)[0],
            "lens": ctx.render_lens(cam, GRID, lens, 6, "f32", flags=flags)[0]}


@pytest.mark.gpu
def test_per_scene_pool_builds_without_the_lds_world(rtc, gpu_ctx, global_ctx):
    """RT_JIT_SYNC on the context without the LDS world: the per-scene pool kernels of every family are built
    with the world in global memory, and return the generic kernels' bytes."""
    scene, cam = _pool_scene(rtc)
    gpu_ctx.upload(scene)
    want = _families(rtc, gpu_ctx, cam)
    global_ctx.upload(scene)
    try:
        global_ctx.set_jit(0)
        generic = _families(rtc, global_ctx, cam)
        assert not global_ctx.jit_status()["used"]
        global_ctx.set_jit(1)
        built, unskipped = {}, {}
        for name, call in (("frame", lambda f: global_ctx.render(cam, 6, "f32", flags=f)[0]),
                           ("supersampled", lambda f: global_ctx.render_supersampled(cam, GRID, 6, "f32", flags=f)[0]),
                           ("lens", lambda f: global_ctx.render_lens(cam, GRID, rtc.Lens(0.25, 5.0, True, 1), 6, "f32",
                                                                     flags=f)[0])):
            built[name] = call(0)
            status = global_ctx.jit_status()
            assert status["used"], (name, status["log"][:2000])
            unskipped[name] = call(RT_FLAG_NO_SKIPS)
            assert global_ctx.jit_status()["used"], name
    finally:
        global_ctx.set_jit(2)
    for name, frame in want.items():
        assert frame.std() > 0.01, name
        assert np.array_equal(frame, generic[name]), name
        assert np.array_equal(frame, built[name]), name
        assert np.array_equal(frame, unskipped[name]), name


@pytest.mark.gpu
def test_the_spheres_and_planes_build_without_the_lds_world(rtc, gpu_ctx, global_ctx):
    """An f32 frame of a pool world of spheres and planes takes the `sp` build; without the LDS world, its
    `global` kernel pair."""
    scene, cam = _pool_scene(rtc)
    gpu_ctx.upload(scene)
    want, sw = gpu_ctx.render(cam, 6, "f32")
    assert not gpu_ctx.jit_status()["used"]
    global_ctx.upload(scene)
    try:
        global_ctx.set_jit(0)
        got, sg = global_ctx.render(cam, 6, "f32")
        assert not global_ctx.jit_status()["used"]
    finally:
        global_ctx.set_jit(2)
    assert want.std() > 0.01 and np.array_equal(want, got)
    assert sw["reflect"] == sg["reflect"] > 0 and sw["refract"] == sg["refract"] > 0
