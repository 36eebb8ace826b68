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
oracle.  The kernels of the instanced and textured builds that stay unreached are named in DESIGN.md 3.15.
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
