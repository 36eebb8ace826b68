"""Texture maps without a GPU: the numpy restatement against the book's tables, the margins of
the designed rays, the three worlds whose image pattern is the oracle's stripes (restatement and oracle), the
frames' distance from the planes where the two differ, the refusals of rt_scene_upload_mapped with a null
context, the Python tables, the identity rule as a stand-alone program under the host sanitizers where g++ has
them, and the CLI's switches.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lens_reference as LR
import uv_map_reference as U
import uv_map_worlds as X
from test_texture_cpu import _sanitize_flags

HERE = os.path.dirname(os.path.abspath(__file__))
LEFT_OUT = 0.01     # at most 1 % of a batch may sit within MARGIN of a decision
MARGIN = 1e-6


# ------------------------------------------------------------------ 1: the book's tables
def test_spherical_map_gives_the_books_table():
    for p, (u, v) in U.BOOK_SPHERICAL:
        gu, gv, _, _ = U.map_uv(U.SPHERICAL, [p])
        assert abs(gu[0] - u) <= 1e-15 and abs(gv[0] - v) <= 1e-15, (p, gu[0], gv[0])


def test_cylindrical_map_gives_the_books_table():
    for p, (u, v) in U.BOOK_CYLINDRICAL:
        gu, gv, _, _ = U.map_uv(U.CYLINDRICAL, [p])
        assert abs(gu[0] - u) <= 1e-15 and abs(gv[0] - v) <= 1e-15, (p, gu[0], gv[0])


def test_cube_faces_and_coordinates_give_the_books_tables():
    for p, face in U.BOOK_FACES:
        assert U.cube_face([p])[0][0] == face, (p, U.FACE_NAMES[face])
    for face, p, (u, v) in U.BOOK_CUBE:
        gu, gv, gf, _ = U.map_uv(U.CUBE, [p])
        assert gf[0] == face and gu[0] == u and gv[0] == v, (U.FACE_NAMES[face], p, gu[0], gv[0])


def test_the_clamp_keeps_the_poles_and_the_margins_name_the_decisions():
    # a rounded r below |y|: c = y / r beyond 1 would make acos NaN
    y = np.nextafter(1.0, 2.0)
    u, v, _, _ = U.map_uv(U.SPHERICAL, [(0.0, y * 3e-200, 0.0), (0.0, -1e-200, 0.0)])
    assert np.isfinite(v).all() and v[0] == 1.0 and v[1] == 0.0
    # the seam, a face tie, a floor jump: margins near 0 there, large elsewhere
    assert U.map_uv(U.SPHERICAL, [(1e-9, 0.3, -1.0)])[3][0] < 1e-9 and U.map_uv(U.SPHERICAL, [(1.0, 0.3, 0.0)])[3][0] == 0.25
    assert U.map_uv(U.CYLINDRICAL, [(1.0, 2.0 + 1e-9, 0.0)])[3][0] < 2e-9
    assert U.map_uv(U.CUBE, [(1.0, 1.0 - 1e-9, 0.2)])[3][0] < 2e-9 and U.map_uv(U.CUBE, [(1.0, 0.5, 0.2)])[3][0] == 0.5
    assert abs(U.map_uv(U.CUBE, [(3.0 + 1e-9, 0.5, 5.0)])[3][0] - 1e-9) < 1e-12  # front: m(x + 1) jumps at x = 3
    # the nearest filter's thresholds come in through colour()
    img = X.colors(5, 7, 1)
    assert U.colour(U.PLANAR, img, 0, [(0.125 + 1e-9, 0.0, 0.3)])[1][0] < 1e-8
    assert U.colour(U.SPHERICAL, X.ONE_A, 1, [(1.0, 0.3, 0.0)])[1][0] == 0.25  # (bilinear: the map's margin alone)


# ------------------------------------------------------------------ 2: the designed rays
@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
@pytest.mark.parametrize("shape,map_name,turned", X.DESIGNED)
def test_designed_rays_leave_out_at_most_one_percent(shape, map_name, filt, turned):
    rays, rgb, margin = X.designed_reference(shape, map_name, filt, X.turned() if turned else None)
    left_out = float((margin < MARGIN).mean())
    print(f"{shape} {map_name} {filt} turned={turned}: {left_out:.5f} left out, {len(np.unique(np.round(rgb, 6), axis=0))} colours")
    assert len(rays) == X.N_RAYS and left_out <= LEFT_OUT
    assert len(np.unique(np.round(rgb, 6), axis=0)) > (10 if filt == "nearest" else 200)  # (a 5 x 7 texture: 35 texels)
    if map_name == "cube":
        _, over = U.designed_rays(shape, X.N_RAYS, X.SEED)
        from rtc_amd import world as W
        pp = U.mul_point(W.inverse(X.turned()) if turned else np.eye(4), over)
        assert set(U.cube_face(pp)[0].tolist()) == set(range(6))  # every face is met


def test_designed_rays_hit_where_they_are_aimed(oracle):
    """The oracle, on the designed world with a material colour, shades every ray (ambient 1: that colour)."""
    from rtc_amd import world as W
    for shape in X.SHAPES:
        rays, _ = U.designed_rays(shape, X.N_RAYS, X.SEED)
        mat = W.Material(color=(0.25, 0.5, 0.75), ambient=1.0, diffuse=0.0, specular=0.0)
        tables = W.World([W.Light((-4.0, 6.0, -5.0), (1.0, 1.0, 1.0))], [X.unit_shape(shape, mat)]).tables(X.camera())
        rgb, st = oracle.color_at(tables, rays, 2)
        assert st["shaded"] == X.N_RAYS and np.abs(rgb - np.array([0.25, 0.5, 0.75])).max() < 1e-15, shape


# ------------------------------------------------------------------ 3: the oracle's stripes
@pytest.mark.parametrize("shape", X.SHAPES)
def test_the_tie_textures_are_the_oracles_stripes(oracle, shape):
    """The restatement's colours of the mapped pattern equal the oracle's stripe_pattern(a, b) at every designed
    over point farther than 1e-6 from the planes x = 0 and x = +-1 (the cube's left and right faces lie 8e-8
    beyond x = +-1 by the over point's offset, on the side the 1 x 1 textures take)."""
    from rtc_amd import world as W
    rays, over = U.designed_rays(shape, X.N_RAYS, X.SEED)
    mat = W.Material(ambient=1.0, diffuse=0.0, specular=0.0, pattern=X.tie_pattern(shape, False))
    tables = W.World([W.Light((-4.0, 6.0, -5.0), (1.0, 1.0, 1.0))], [X.unit_shape(shape, mat)]).tables(X.camera())
    want, _ = oracle.color_at(tables, rays, 2)
    mapped = X.tie_pattern(shape, True)
    images = mapped.faces if shape == "cube" else mapped.image
    got, _ = U.colour(X.KIND[X.NATURAL[shape]], images, 0, over)
    x = over[:, 0]
    near = np.abs(x) < MARGIN
    if shape != "cube":
        near |= np.abs(np.abs(x) - 1.0) < MARGIN
    assert near.mean() <= LEFT_OUT and np.abs(got - want)[~near].max() < 1e-15
    assert {tuple(c) for c in np.round(got * 255).astype(int).tolist()} == {X.A, X.B}
    if shape == "cube":
        face = U.cube_face(over)[0]
        assert (got[face == U.LEFT] == np.array(X.A1)).all() and (got[face == U.RIGHT] == np.array(X.B1)).all()
        assert (face == U.LEFT).sum() > 200 and (face == U.RIGHT).sum() > 200


def tie_frames(oracle, rtc, tables, depth):
    """The oracle's frame, its 2 x 2 supersampled frame's samples, and its lens frame of `tables`."""
    cam = tables.camera
    w, h = X.FRAME
    cn = rtc.camera_resize(cam, 2 * w, 2 * h)
    t = tables.expanded()
    frame, st = oracle.render(t, cam, depth, threads=8)
    fine, st2 = oracle.render(t, cn, depth, threads=8)
    lens, st3 = LR.lens_frame(oracle, t, cn, w, h, 2, X.LENS[0], X.LENS[1], False, 0, depth)
    return {"frame": (frame, st), "fine": (fine, st2), "lens": (lens, st3)}


@pytest.mark.parametrize("shape,glass,area", [(s, g, False) for s in X.SHAPES for g in (False, True)] + [("sphere", False, True)])
def test_no_ray_of_the_tie_frames_lands_within_1e_6_of_the_planes(oracle, rtc, shape, glass, area):
    """The stripes moved by +-1e-6 give the same frames, supersampled samples and lens frames, to the bit: no hit,
    primary or secondary, lies within 1e-6 of a plane where the image pattern and the stripes differ.  For the
    cube the probe is the stripes twice as wide, whose edge is x = 0 alone: its left and right faces lie 8e-8
    beyond x = +-1 on purpose."""
    depth = 4
    probe = shape == "cube"
    got = [tie_frames(oracle, rtc, X.tie(shape, False, glass, area, shift, probe), depth) for shift in (0.0, 1e-6, -1e-6)]
    for key in got[0]:
        for other in got[1:]:
            assert np.array_equal(got[0][key][0], other[key][0]) and got[0][key][1] == other[key][1], (shape, key)
    frame, st = got[0]["frame"]
    assert st["lit_patterned"] > 800 and (st["refract"] > 0) == glass
    # both colours show: the frame has pixels near a x light and near b x light
    assert frame.std() > 0.05


# ------------------------------------------------------------------ 4: refusals, forwarding
def _mapped_world(rtc):
    from rtc_amd import world as W
    shapes = [W.sphere(W.Material(pattern=X.mapped_pattern("spherical", "nearest"))),
              W.cube(W.Material(pattern=X.mapped_pattern("cube", "bilinear"))),
              W.plane(W.Material(pattern=W.checker_pattern((1, 1, 1), (0, 0, 0))))]
    return W.World([W.Light((0.0, 5.0, -5.0), (1.0, 1.0, 1.0))], shapes).tables(X.camera())


def test_upload_refusals_have_their_own_messages_with_a_null_context(rtc):
    lib = rtc._lib

    def refusal(edit=None, null_list=False, count=None):
        t = _mapped_world(rtc)
        if edit:
            edit(t.maps)
        args = list(t.mapped_args())
        if null_list:
            args[-2] = None
        if count is not None:
            args[-1] = count
        rc = lib.rt_scene_upload_mapped(None, *args)
        return rc, lib.rt_last_error().decode()

    def setter(k, **kw):
        def edit(maps):
            for name, value in kw.items():
                if name.startswith("face"):
                    maps[k].faces[int(name[4:])] = value
                else:
                    setattr(maps[k], name, value)
        return edit

    t = _mapped_world(rtc)
    assert [(m.pattern, m.map) for m in t.maps] == [(0, 1), (1, 3)] and [p.kind for p in t.patterns] == [6, 6, 3]
    assert len(t.textures) == 6 and list(t.maps[1].faces) == [1, 0, 2, 3, 4, 5]  # (the spherical pattern shows the front face's image)
    cases = [
        (dict(null_list=True), "rt_scene_upload_mapped: null map list with nonzero count"),
        (dict(edit=setter(1, pattern=3)), "map 1: pattern index out of range"),
        (dict(edit=setter(0, pattern=2)), "map 0: the pattern is not an image pattern"),
        (dict(edit=setter(1, pattern=0, map=1, face0=-1, face1=-1, face2=-1, face3=-1, face4=-1, face5=-1)), "map 1: pattern named twice"),
        (dict(edit=setter(0, map=4)), "map 0: unknown map"),
        (dict(edit=setter(1, face5=6)), "map 1: face texture index out of range"),
        (dict(edit=setter(1, face2=-1)), "map 1: face texture index out of range"),
        (dict(edit=setter(0, face3=0)), "map 0: a face other than -1 for a map that is no cube map"),
    ]
    for kw, text in cases:
        rc, msg = refusal(**kw)
        assert rc == rtc.RT_ERR_INVALID and msg == text, (kw, msg)
    # a well-formed world passes every check and then meets the null context
    assert refusal() == (rtc.RT_ERR_INVALID, "null context")
    # an earlier list's defect is reported first: the map list is the last one checked
    def both(maps):
        maps[0].map = 9
    t = _mapped_world(rtc)
    both(t.maps)
    t.patterns[0].reserved = 2
    assert lib.rt_scene_upload_mapped(None, *t.mapped_args()) == rtc.RT_ERR_INVALID
    assert lib.rt_last_error().decode() == "pattern 0: unknown texture filter"
    # reserved = 2 and sub_b = 0 stay refused (tests/test_texture_cpu.py pins them for the older entry points)
    t = _mapped_world(rtc)
    t.patterns[1].sub_b = 0
    assert lib.rt_scene_upload_mapped(None, *t.mapped_args()) == rtc.RT_ERR_INVALID
    assert lib.rt_last_error().decode() == "pattern 1: an image pattern's sub_b must be -1"


def test_without_a_map_entry_it_is_rt_scene_upload_lit(rtc):
    """n_maps = 0: the list pointer is not looked at, and the refusals and their order are rt_scene_upload_lit's."""
    lib = rtc._lib
    t = _mapped_world(rtc)
    args = list(t.mapped_args())
    args[-1] = 0
    assert lib.rt_scene_upload_mapped(None, *args) == rtc.RT_ERR_INVALID and lib.rt_last_error().decode() == "null context"
    args[-2] = None
    assert lib.rt_scene_upload_mapped(None, *args) == rtc.RT_ERR_INVALID and lib.rt_last_error().decode() == "null context"
    t.patterns[0].sub_a = 6
    texts = []
    for fn, a in ((lib.rt_scene_upload_lit, t.lit_args()), (lib.rt_scene_upload_mapped, args)):
        assert fn(None, *a) == rtc.RT_ERR_INVALID
        texts.append(lib.rt_last_error().decode())
    assert texts[0] == texts[1] == "pattern 0: texture index out of range"
    # the older entry point does not know the list, and Context.upload picks the new one only for a map entry
    plain = _mapped_world(rtc)
    plain.maps = None
    assert not plain.mapped and plain.textured and _mapped_world(rtc).mapped


# ------------------------------------------------------------------ 5: the Python tables
def test_tables_hold_the_maps_as_the_header_lays_them_out(rtc, tmp_path):
    assert C.sizeof(rtc.UVMapDesc) == 32 and C.sizeof(rtc.MapInfo) == 16
    assert (rtc.UVMapDesc.pattern.offset, rtc.UVMapDesc.map.offset, rtc.UVMapDesc.faces.offset) == (0, 4, 8)
    t = _mapped_world(rtc)
    assert isinstance(t.maps, C.Array) and len(t.maps) == 2
    want = np.array([0, 1, -1, -1, -1, -1, -1, -1, 1, 3, 1, 0, 2, 3, 4, 5], dtype=np.int32).tobytes()
    assert bytes(t.maps) == want
    assert rtc.TEXTURE_MAPS == {"planar": 0, "spherical": 1, "cylindrical": 2, "cube": 3}
    # the header's own numbers, through a compiled probe
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtc.h"\nint main(void) { printf("%zu %zu %zu %zu %d %d %d %d\\n", '
                     "sizeof(rt_uv_map_desc), offsetof(rt_uv_map_desc, map), offsetof(rt_uv_map_desc, faces), sizeof(rt_map_info), "
                     "RT_MAP_PLANAR, RT_MAP_SPHERICAL, RT_MAP_CYLINDRICAL, RT_MAP_CUBE); return 0; }\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(os.path.dirname(HERE), "include"), "-o", str(exe), str(probe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["32", "4", "8", "16", "0", "1", "2", "3"]
    # a planar image pattern makes no entry; image_pattern refuses what it does not know
    from rtc_amd import world as W
    flat = W.World([], [W.sphere(W.Material(pattern=W.image_pattern(X.ONE_A, map="planar")))]).tables()
    assert flat.maps is None and not flat.mapped and flat.textured
    with pytest.raises(ValueError):
        W.image_pattern(X.ONE_A, map="cube")
    with pytest.raises(ValueError):
        W.cube_map_pattern(X.ONE_A, X.ONE_A, X.ONE_A, X.ONE_A, X.ONE_A, np.zeros((2, 2), np.uint8))
    # two patterns over one array share the texture; the expansion keeps the maps
    assert t.expanded().maps is t.maps


# ------------------------------------------------------------------ 6: identity and brightness
def test_identity_rule_stand_alone(tmp_path):
    exe = tmp_path / "uv_map_identity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *_sanitize_flags(tmp_path), "-o",
                    str(exe), os.path.join(HERE, "uv_map_identity.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "ok", out.stdout + out.stderr
    assert "refusals: 14 cases" in lines and "cube maps: by their faces' pictures" in lines


# ------------------------------------------------------------------ 7: the CLI
def _cli(rtc):
    return os.path.join(os.path.dirname(rtc.lib_path()), "rtc")


def test_cli_knows_the_switches(rtc):
    r = subprocess.run([_cli(rtc)], capture_output=True, text=True)
    assert r.returncode != 0
    assert "[--texture-map planar|spherical|cylindrical] [--cube-map L,F,R,B,U,D]" in r.stderr
    assert "--texture-map planar|spherical|cylindrical maps a face without texture coordinates" in r.stderr
    assert "--cube-map L,F,R,B,U,D takes six image files in place of --texture" in r.stderr


def test_cli_refusals(rtc, tmp_path):
    from test_cli import SCENE
    yaml = tmp_path / "scene.yaml"
    yaml.write_text(SCENE)
    obj = tmp_path / "t.obj"
    obj.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    tex = tmp_path / "t.ppm"
    rtc.write_image(str(tex), X.colors(3, 2, 1), "ppm")
    out = tmp_path / "out.png"
    six = ",".join([str(tex)] * 6)

    def run(*args):
        r = subprocess.run([_cli(rtc), str(yaml), str(out), *args], capture_output=True, text=True)
        assert not out.exists()
        return r.returncode, r.stderr

    assert run("--texture-map", "conical", "--obj", str(obj), "--texture", str(tex))[0] == 2
    assert run("--texture-map")[0] == 2
    rc, err = run("--texture-map", "spherical", "--obj", str(obj))
    assert rc == 2 and "--texture-map needs --texture" in err
    rc, err = run("--cube-map", six)
    assert rc == 2 and "--cube-map needs a mesh to show on: give --obj or --instance" in err
    rc, err = run("--cube-map", ",".join([str(tex)] * 5), "--obj", str(obj))
    assert rc == 2 and "--cube-map takes six image files: L,F,R,B,U,D" in err
    rc, err = run("--cube-map", six + ",", "--obj", str(obj))
    assert rc == 2 and "--cube-map takes six image files" in err
    rc, err = run("--cube-map", six, "--texture", str(tex), "--obj", str(obj))
    assert rc == 2 and "--cube-map takes the place of --texture" in err
    rc, err = run("--cube-map", six, "--texture-map", "spherical", "--obj", str(obj))
    assert rc == 2 and "--texture-map applies to --texture's pattern" in err
    rc, err = run("--cube-map", ",".join([str(tex)] * 5 + [str(tmp_path / "missing.ppm")]), "--obj", str(obj))
    assert rc == 1 and "missing.ppm" in err
