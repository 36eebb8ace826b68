"""A context whose buffers grow after they have been used renders what a fresh one renders.

The host layer keeps its device memory in buffers that grow on demand
(csrc/device_memory.hpp DeviceBuffer::reserve: free, then allocate, contents
dropped).  One long-lived context is carried through launches that make each
of them grow after an earlier launch has already used it; every frame and its
ray counters must equal, bit for bit, those of the same calls on a context
created for that step alone.

The world is smoke()'s scene (__graft_entry__.py): a reflective floor and a
glass sphere, so frames at depth > 0 run the pool kernel.  Tiles are 64x4
pixels and every frame here is below the per-scene build's 256 tiles.  Which
step grows what (rtc_host.cpp launch / plan_tile_order / rt_render):

  1. 64x8, depth 1 (2 tiles, 2 workgroups): first allocation of the scratch
     frame, the pinned counters, tile cost + order (2 tiles) and the cold
     order (3 words).
  2. 192x64, depth 1, twice (48 tiles): scratch, tile cost + order and the cold
     order grow; the second launch builds the heaviest-first order from the
     costs the first one recorded in the regrown buffers.
  3. 64x8, depth 16: the pool bound (256 + 16 x 256 rays) exceeds its LDS part,
     so the spill buffer is allocated, for 2 workgroups.
  4. 192x64, depth 16: the spill buffer grows to 48 workgroups' regions.
  5. 64x8, depth 16 and depth 1: every buffer is larger than the launch needs
     (the spill block count comes from the buffer's capacity).
  6. RT_FLAG_STAMPS at 64x8, then at 192x64 (depth 1): the stamps (two per
     workgroup) and the item log (64 items per tile) are allocated, then grow.

test_larger_world_on_the_same_context replaces the world tables and the
lights of both precisions with larger ones.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("primary", "shadow", "reflect", "refract", "shaded", "lit_patterned", "refract_evals", "schlick_evals")

# (width, height, depth, flags, launches)
STEPS = [
    (64, 8, 1, 0, 1),
    (192, 64, 1, 0, 2),
    (64, 8, 16, 0, 1),
    (192, 64, 16, 0, 1),
    (64, 8, 16, 0, 1),
    (64, 8, 1, 0, 1),
    (64, 8, 1, "stamps", 1),
    (192, 64, 1, "stamps", 1),
]


@pytest.fixture(scope="module")
def smoke_scene(rtc):
    import importlib.util
    import os

    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("graft_entry_for_regrow", os.path.join(ROOT, "__graft_entry__.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    return rtc.load_scene_text(entry._SMOKE_SCENE)


def _frames(ctx, cam, depth, flags, launches, precision):
    return [ctx.render(cam, depth, precision=precision, flags=flags) for _ in range(launches)]


def _same(got, want, what):
    for i, ((img, st), (ref, ref_st)) in enumerate(zip(got, want)):
        assert img.dtype == ref.dtype and img.shape == ref.shape, (what, i)
        assert np.array_equal(img.view(np.uint8), ref.view(np.uint8)), (what, i, float(np.abs(img - ref).max()))
        assert {k: st[k] for k in COUNTERS} == {k: ref_st[k] for k in COUNTERS}, (what, i)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_regrown_buffers_render_like_a_fresh_context(rtc, smoke_scene, precision):
    assert rtc.device_count() >= 1
    assert rtc.RT_MAX_SUPPORTED_DEPTH == 16
    with rtc.Context(0) as long_lived:
        long_lived.upload(smoke_scene)
        for n, (w, h, depth, flags, launches) in enumerate(STEPS):
            cam = rtc.camera_resize(smoke_scene.camera, w, h)
            f = rtc.RT_FLAG_STAMPS if flags == "stamps" else 0
            got = _frames(long_lived, cam, depth, f, launches, precision)
            with rtc.Context(0) as fresh:
                fresh.upload(smoke_scene)
                want = _frames(fresh, cam, depth, f, launches, precision)
            assert got[0][1]["primary"] == w * h
            assert depth == 0 or got[0][1]["reflect"] > 0  # the pool kernel ran
            _same(got, want, (precision, n, w, h, depth, flags))


def _larger_world(W):
    glass = W.Material(color=(0.1, 0.1, 0.3), diffuse=0.4, reflectiveness=0.9, transparency=0.9, refractive_index=1.5)
    floor = W.Material(pattern=W.checker_pattern((0.35, 0.35, 0.35), (0.65, 0.65, 0.65)), specular=0.0,
                       reflectiveness=0.4)
    shapes = [W.plane(floor), W.sphere(glass, W.translation(0.6, 1.0, -0.6))]
    for i in range(6):
        m = W.Material(color=(0.2 + 0.1 * i, 0.5, 0.9 - 0.1 * i), reflectiveness=0.1 * (i % 3))
        t = W.mat_mul(W.translation(-2.5 + i, 0.5, 1.5), W.scaling(0.5, 0.5, 0.5))
        shapes.append(W.cube(m, t) if i % 2 else W.sphere(m, t))
    shapes.append(W.cylinder(0, 1, True, W.Material(color=(0.9, 0.8, 0.1)), W.translation(-1.5, 0, -0.5)))
    lights = [W.Light((-4.9, 4.9, -1.0), (0.6, 0.6, 0.6)), W.Light((3.0, 6.0, -4.0), (0.3, 0.3, 0.3)),
              W.Light((0.0, 3.0, -6.0), (0.2, 0.2, 0.2))]
    return W.World(lights, shapes)


def test_larger_world_on_the_same_context(rtc, smoke_scene):
    from rtc_amd import world as W
    cam = rtc.camera_resize(smoke_scene.camera, 192, 64)
    tables = _larger_world(W).tables(cam)
    assert tables.counts[0] > smoke_scene.counts[0] and tables.counts[3] > smoke_scene.counts[3]
    with rtc.Context(0) as ctx, rtc.Context(0) as fresh:
        ctx.upload(smoke_scene)
        for precision in ("f32", "f64"):
            ctx.render(cam, 4, precision=precision)  # the small world's tables are in use
        ctx.upload(tables)
        fresh.upload(tables)
        for precision in ("f32", "f64"):
            _same([ctx.render(cam, 4, precision=precision)], [fresh.render(cam, 4, precision=precision)],
                  ("larger world", precision))
        ctx.upload(smoke_scene)  # and back: tables larger than the world needs
        with rtc.Context(0) as fresh_small:
            fresh_small.upload(smoke_scene)
            for precision in ("f32", "f64"):
                _same([ctx.render(cam, 4, precision=precision)], [fresh_small.render(cam, 4, precision=precision)],
                      ("small world again", precision))
