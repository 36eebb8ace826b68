"""The cases of tests/test_gpu_lens_builds.py and their CPU-side conditions: no GPU.

Lens frames of smooth and textured worlds have no oracle: their reference is the numpy restatement of the
triangle's semantics (tests/smooth_reference.py, tests/texture_reference.py) over the lens rays of
tests/lens_reference.py.  A pixel is compared only if every one of its n^2 rays keeps every decision (an edge,
a texel, a wrap) further than the f64 bar from its threshold.  Here, on the references alone:

* the share of pixels left out is at most 0.001 in every case the GPU tests run;
* the lens visibly changes the reference's frame (a mean difference above 0.002 from the same frame through a
  pinhole), for the oracle's frames of the instanced worlds too.
"""
import functools

import numpy as np
import pytest

import instance_worlds as I
import lens_reference as LR
import smooth_reference as R
import smooth_worlds as S
import texture_reference as T
import texture_worlds as X

ABS64 = 1e-9        # the project's f64 bar, and the margin below which a reference's decision sits on the fence
LEFT_OUT = 0.001    # the largest share of pixels a case may leave out
VISIBLE = 0.002     # mean |lens frame - pinhole frame| (tests/test_gpu_lens.py test_the_lens_changes_the_frame)
SEED = S.LENS_SEED
SHAPES = [(70, 22, 2), (70, 22, 3), (130, 10, 4)]  # ragged against the 64 x 4 tile and the 16 x 4 wave block
NUMPY_SHAPES = SHAPES[:2]

# instanced worlds (tests/instance_worlds.py): the eye is 4.5 from what it looks at; a focal plane in front of
# every mesh leaves the whole frame out of focus
INSTANCED = ("three_tori", "nested_glass", "small", "beside_plain")
INSTANCED_LENS = (0.25, 3.0)
SMOOTH = ("ico", "instances")
SMOOTH_LENS = (S.LENS_APERTURE, S.LENS_FOCUS)
# textured icospheres: flat or smooth, nearest or bilinear, coordinates inside the unit square or wrapped
TEXTURED = tuple(f"{shade}-{filt}-{span}" for shade in ("flat", "smooth") for filt in ("nearest", "bilinear")
                 for span in ("inside", "wrap"))
TEXTURED_LENS = SMOOTH_LENS
IMAGE = X.colors(5, 7)


@functools.lru_cache(maxsize=None)
def _rtc():
    import rtc_amd
    return rtc_amd


@functools.lru_cache(maxsize=None)
def instanced_world(key):
    """(tables, the expansion, depth) of a world of tests/instance_worlds.py."""
    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory(prefix="lens_builds_") as tmp:  # (the meshes are read back at once)
        tables, depth = I.build_world(_rtc(), pathlib.Path(tmp), key)
    return tables, tables.expanded(), depth


@functools.lru_cache(maxsize=None)
def smooth_world(key, pool=False):
    """(the tables to upload, the triangles-only expansion the reference traces).  pool: with a glass sphere
    behind the camera that no ray meets, so that the upload takes the pool kernel and means the same frame."""
    rtc = _rtc()
    build = S.ico_alone if key == "ico" else S.ico_instances
    plain = build(rtc)
    return (build(rtc, extra=[S.glass_behind_the_camera()]) if pool else plain), plain.expanded()


@functools.lru_cache(maxsize=None)
def textured_world(key, pool=False):
    rtc = _rtc()
    shade, filt, span = key.split("-")
    kw = dict(wrap=span == "wrap", smooth=shade == "smooth")
    plain = X.ico_alone(rtc, IMAGE, filt, **kw)
    return (X.ico_alone(rtc, IMAGE, filt, extra=[S.glass_behind_the_camera()], **kw) if pool else plain), plain


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def numpy_lens_frame(kind, key, w, h, n, jitter, aperture=None):
    """(frame, sound pixels, counts) of the numpy reference's lens frame of a smooth or textured world, once
    per case; read-only.  aperture 0: the same frame through a pinhole."""
    rtc = _rtc()
    (_, tables), trace, lens = (smooth_world(key), R.trace, SMOOTH_LENS) if kind == "smooth" else \
                               (textured_world(key), T.trace, TEXTURED_LENS)
    cn = rtc.camera_resize(tables.camera, n * w, n * h)
    a = lens[0] if aperture is None else aperture
    frame, sound, counts = LR.traced_lens_frame(trace, tables, cn, w, h, n, a, lens[1], jitter, SEED, ABS64)
    _frozen(frame, sound)
    return frame, sound, counts


@functools.lru_cache(maxsize=None)
def oracle_lens_frame(tables_of, w, h, n, jitter, lens, depth, aperture=None):
    """(frame, stats) of the oracle's lens frame of tables_of() (a cached, argument-free callable), once per
    case; read-only."""
    import pyoracle
    rtc = _rtc()
    tables = tables_of()
    cn = rtc.camera_resize(tables.camera, n * w, n * h)
    a = lens[0] if aperture is None else aperture
    frame, st = LR.lens_frame(pyoracle, tables, cn, w, h, n, a, lens[1], jitter, SEED, depth)
    _frozen(frame)
    return frame, st


@functools.lru_cache(maxsize=None)
def _expansion_of(key):
    return functools.partial(lambda k: instanced_world(k)[1], key)


def instanced_lens_frame(key, w, h, n, jitter, aperture=None):
    return oracle_lens_frame(_expansion_of(key), w, h, n, jitter, INSTANCED_LENS, instanced_world(key)[2], aperture)


# ------------------------------------------------------------------ the conditions
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("w,h,n", NUMPY_SHAPES)
@pytest.mark.parametrize("key", SMOOTH)
def test_smooth_references_leave_out_at_most_a_thousandth(key, w, h, n, jitter):
    frame, sound, counts = numpy_lens_frame("smooth", key, w, h, n, jitter)
    left_out = 1.0 - float(sound.mean())
    print(f"smooth {key} {w}x{h} n={n} jitter {jitter}: {left_out:.6f} of pixels left out")
    assert left_out <= LEFT_OUT
    assert counts["shaded"] > 0.2 * counts["primary"]


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("key", TEXTURED)
def test_textured_references_leave_out_at_most_a_thousandth(key, jitter):
    for w, h, n in NUMPY_SHAPES[:1] if key != TEXTURED[-1] else NUMPY_SHAPES:
        frame, sound, counts = numpy_lens_frame("textured", key, w, h, n, jitter)
        left_out = 1.0 - float(sound.mean())
        print(f"textured {key} {w}x{h} n={n} jitter {jitter}: {left_out:.6f} of pixels left out")
        assert left_out <= LEFT_OUT
        assert counts["shaded"] > 0.2 * counts["primary"]


@pytest.mark.parametrize("jitter", [False, True])
def test_the_lens_visibly_changes_every_references_frame(jitter):
    w, h, n = NUMPY_SHAPES[0]
    for kind, keys in (("smooth", SMOOTH), ("textured", (TEXTURED[0], TEXTURED[-1]))):
        for key in keys:
            lens, _, _ = numpy_lens_frame(kind, key, w, h, n, jitter)
            pin, _, _ = numpy_lens_frame(kind, key, w, h, n, False, 0.0)
            change = float(np.abs(lens - pin).mean())
            print(f"{kind} {key}: mean |lens - pinhole| {change:.4f}")
            assert change > VISIBLE, (kind, key)
    for key in INSTANCED:
        lens, _ = instanced_lens_frame(key, w, h, n, jitter)
        pin, _ = instanced_lens_frame(key, w, h, n, False, 0.0)
        change = float(np.abs(lens - pin).mean())
        print(f"instanced {key}: mean |lens - pinhole| {change:.4f}")
        assert change > VISIBLE, key


def test_the_instanced_u8_cases_stay_clear_of_rounding_boundaries():
    from test_supersample_cpu import near_boundary
    for w, h, n in SHAPES:
        for jitter in (False, True):
            ref, _ = instanced_lens_frame("nested_glass", w, h, n, jitter)
            assert near_boundary(ref, ABS64).mean() <= 0.001, (w, h, n, jitter)


def test_a_glass_sphere_behind_the_camera_is_out_of_every_lens_ray():
    """The pool variants of the smooth and textured worlds mean the frame of the world without the sphere: no
    lens ray, primary or shadow, may meet it.  Its bounding sphere against every ray of the widest case."""
    rtc = _rtc()
    for tables in (smooth_world("ico", True)[0], smooth_world("instances", True)[0], textured_world(TEXTURED[0], True)[0]):
        assert tables.has_secondary()
        ball = [s for s in tables.shapes if s.kind != 5]
        assert len(ball) == 1
        fwd = np.linalg.inv(np.array(list(ball[0].inverse)).reshape(4, 4))
        centre, radius = fwd[:3, 3], float(np.abs(fwd[:3, :3]).sum(axis=1).max())
        w, h, n = NUMPY_SHAPES[1]
        cn = rtc.camera_resize(tables.camera, n * w, n * h)
        rays = LR.lens_rays(cn, w, h, n, SMOOTH_LENS[0], SMOOTH_LENS[1], True, SEED).reshape(-1, 6)
        along = ((centre - rays[:, :3]) * rays[:, 3:]).sum(axis=1)
        assert along.max() < -radius, "the sphere lies behind every lens ray's origin"
        # a shadow ray runs from a point of the meshes (within 1.5 of the origin) to the light beside the eye
        light = np.array(list(tables.lights[0].position))
        assert np.linalg.norm(centre - light) > np.linalg.norm(light) + 1.5 + radius
