"""Smooth triangles on the host (no GPU): the OBJ parser with normals, the numpy
reference against the book's known answer, rt_smooth_expand, the struct
layouts, the refusals of rt_scene_upload_smooth with a null context, the world
builder, and the identity rule (tests/smooth_identity.cpp, stand-alone, under
the host sanitizers where g++ has them).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import smooth_reference as R
import smooth_worlds as S
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))

PARSER_TEXT = """# four vertices, four normals, one of each kind of face
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0.5 1.5 0
vt 0.5 0.5
vn 0 0 1
vn 0.25 0 1
f 1//1 2//2 3//-1
vn 0 0.5 2
vn -3 0 0
f 1/1/1 2/1/2 3/1/3 4/1/4 5/1/-4
f 1//1 2 3//3
g tail
f -5//-1 -4//-2 -3//-3
"""


def _sanitize_flags(tmp_path):
    """-fsanitize=address,undefined where this g++ links them (a stand-alone program: no preload)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++", *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0
    return flags if ok else []


# ------------------------------------------------------------------ 1: parser
def test_parser_reads_normals_under_the_flag(rtc):
    m = rtc.load_obj(PARSER_TEXT, normals=True)
    assert m.ignored_lines == 3  # the comment, vt, g: vn is no longer among them
    assert np.array_equal(m.normals, [[0, 0, 1], [0.25, 0, 1], [0, 0.5, 2], [-3, 0, 0]])
    # f i//k with a negative index (2 normals read so far), the fan of five (1, k, k + 1) with i/j/k and -4,
    # a face with one vertex lacking a normal (flat), and negative indices after all four normals
    no = rtc.RT_NO_NORMAL
    assert m.triangles.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 1, 2], [0, 1, 2]]
    assert m.triangle_normals.tolist() == [[0, 1, 1], [0, 1, 2], [0, 2, 3], [0, 3, 0], [no, no, no], [3, 2, 1]]
    assert m.n_smooth == 5
    sm = m.smooth_descs()
    assert [d.index for d in sm] == [0, 1, 2, 3, 5] and all(d.list == rtc.RT_SMOOTH_SHAPES for d in sm)
    assert list(sm[3].normal_1) == [0, 0, 1] and list(sm[3].normal_2) == [-3, 0, 0] and list(sm[3].normal_3) == [0, 0, 1]
    # the same text through the old entry point: today's view, vn counted as ignored, no normals
    old = rtc.load_obj(PARSER_TEXT)
    assert old.ignored_lines == 7 and old.n_smooth == 0 and old.normals.shape == (0, 3)
    assert old.triangle_normals.shape == (0, 3) and np.array_equal(old.triangles, m.triangles)
    assert np.array_equal(old.vertices, m.vertices)
    # CRLF
    crlf = rtc.load_obj(PARSER_TEXT.replace("\n", "\r\n"), normals=True)
    assert np.array_equal(crlf.triangle_normals, m.triangle_normals) and np.array_equal(crlf.normals, m.normals)
    assert crlf.ignored_lines == 3


def test_parser_from_a_file_and_flags(rtc, tmp_path):
    path = tmp_path / "m.obj"
    path.write_text(PARSER_TEXT)
    m = rtc.load_obj(str(path), normals=True)
    assert m.n_smooth == 5
    h = C.c_void_p()
    lib = rtc._lib
    assert lib.rt_mesh_load_obj_ex(None, None, 1, C.byref(h)) == rtc.RT_ERR_INVALID
    assert lib.rt_mesh_load_obj_ex(b"x", b"v 0 0 0\n", 1, C.byref(h)) == rtc.RT_ERR_INVALID
    assert lib.rt_mesh_load_obj_ex(None, b"v 0 0 0\n", 2, C.byref(h)) == rtc.RT_ERR_INVALID
    assert b"unknown flag" in lib.rt_last_error()


@pytest.mark.parametrize("line,text", [
    ("vn 1 2", "line 4: a normal needs three components"),
    ("vn 1 two 3", "line 4: 'two' is not a number in a normal"),
    ("f 1//1 2//x 3//1", "line 4: '2//x' is not a normal index"),
    ("f 1//1 2//2 3//1", "line 4: normal index 2 out of range (1 normals so far)"),
    ("f 1//1 2//0 3//1", "line 4: normal index 0 out of range (1 normals so far)"),
    ("f 1//1 2//-2 3//1", "line 4: normal index -2 out of range (1 normals so far)"),
])
def test_parser_errors_carry_the_line_number(rtc, line, text):
    head = "v 0 0 0\nv 1 0 0\nvn 0 0 1\n"
    with pytest.raises(rtc.RenderError) as e:
        rtc.load_obj(head + line + "\nv 0 1 0\nvn 1 0 0\n", normals=True)
    assert e.value.code == rtc.RT_ERR_IO and text in str(e.value), str(e.value)
    rtc.load_obj(head + "v 0 1 0\n" + ("f 1 2 3\n" if line.startswith("f") else line + "\n"))  # the old entry point skips vn


def test_parser_stand_alone_under_the_host_sanitizers(tmp_path):
    exe, obj = tmp_path / "parser", tmp_path / "m.obj"
    obj.write_text(PARSER_TEXT)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *_sanitize_flags(tmp_path), "-o",
                    str(exe), os.path.join(HERE, "smooth_parser_main.cpp")], check=True)
    out = subprocess.run([str(exe), str(obj)], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", out.stdout + out.stderr
    assert "flags 0: 5 vertices 6 triangles 7 ignored 0 normals 0 smooth" in lines
    assert "flags 1: 5 vertices 6 triangles 3 ignored 4 normals 5 smooth" in lines
    # baked by scaling(2, 4, 0.5): (T^-1)^T n = n / scale per axis, not normalized
    assert "  bake 0 list 7 index 3 n1 0 0 1 n3 0 0 1" in lines
    assert "  bake 1 list 7 index 2 n1 0 0 2 n3 -1.5 0 0" in lines
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nvn 0 1\n")
    out = subprocess.run([str(exe), str(bad)], capture_output=True, text=True)
    assert out.returncode == 0 and "flags 1: error -7: OBJ: line 2: a normal needs three components" in out.stdout


# --------------------------------------------------- 2: the reference itself
def test_reference_gives_the_books_known_answer(rtc):
    from rtc_amd import world as W
    p, n, ray, u, v, want = R.known_answer()
    white = W.Material(color=(1.0, 1.0, 1.0), ambient=0.0, diffuse=1.0, specular=0.0)
    light = (-3.0, 4.0, -5.0)  # on the side the interpolated normal leans to
    tables = W.World([W.Light(light)], [W.smooth_triangle(*p, *n, white)]).tables()
    rgb, hit, margin = R.trace(tables, np.array([ray]))
    assert hit["shape"][0] == 0 and abs(hit["t"][0] - 2.0) < 1e-12
    assert abs(hit["u"][0] - u) < 1e-12 and abs(hit["v"][0] - v) < 1e-12
    tri = R.Triangles(tables)
    ln = (tri.n2[0] * hit["u"][0] + tri.n3[0] * hit["v"][0]) + tri.n1[0] * ((1.0 - hit["u"][0]) - hit["v"][0])
    got = R.normalized(R.mul_normal(tri.inv[0], ln))
    assert np.abs(got - want).max() < 1e-12 and np.abs(got - np.array([-0.5547, 0.83205, 0.0])).max() < 1e-5
    # the book's normal lies in the triangle's plane, so the over point does too and the triangle shadows
    # itself: black.  Leaning every vertex normal towards the eye by (0, 0, -1), the colour of the white,
    # diffuse-only material is the cosine between the normal and the light's direction
    assert rgb[0, 0] == 0.0 and margin[0] > 0.2
    lean = tuple((x, y, z - 1.0) for x, y, z in n)
    tables = W.World([W.Light(light)], [W.smooth_triangle(*p, *lean, white)]).tables()
    rgb, hit, _ = R.trace(tables, np.array([ray]))
    normal = np.array([-0.2, 0.3, -1.0]) / np.sqrt(0.04 + 0.09 + 1.0)
    ld = np.array(light) - (np.array([-0.2, 0.3, 0.0]) + normal * R.EPSILON)
    cosine = float(np.dot(ld / np.linalg.norm(ld), normal))
    assert cosine > 0.5 and abs(rgb[0, 0] - cosine) < 1e-12


def test_reference_fma_is_a_fused_multiply_add():
    rng = np.random.default_rng(7)
    a, b = rng.normal(size=2000), rng.normal(size=2000)
    c = -(a * b)  # the case a plain a * b + c gets wrong: the rounding error of the product
    from fractions import Fraction
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(R.fma(a, b, c), want) and (want != 0).mean() > 0.9
    c = rng.normal(size=2000) * 1e-3
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.abs(R.fma(a, b, c) - want).max() <= np.spacing(np.abs(want)).max()


# ------------------------------------------- 3: expansion, layouts, refusals
def test_struct_layouts_match_the_headers(rtc):
    for header, name, cls in (("rtc.h", "rt_smooth_desc", rtc.SmoothDesc), ("rtc.h", "rt_smooth_info", rtc.SmoothInfo),
                              ("rtc_scene.h", "rt_mesh_normals_view", rtc.MeshNormalsView)):
        hdr = open(os.path.join(ROOT, "include", header)).read()
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in [d for d in body.split(";") if d.strip()]:
            names = decl.split(",")
            fields += [re.sub(r"\[\d+\]", "", names[0].split()[-1].lstrip("*"))]
            fields += [re.sub(r"\[\d+\]", "", n.strip().lstrip("*")) for n in names[1:]]
        assert fields == [n for n, _ in cls._fields_], name
    assert C.sizeof(rtc.SmoothDesc) == 80 and rtc.SmoothDesc.normal_1.offset == 8 and rtc.SmoothDesc.normal_3.offset == 56
    assert C.sizeof(rtc.SmoothInfo) == 16 and rtc.SmoothInfo.normal_bytes.offset == 8
    assert C.sizeof(rtc.MeshNormalsView) == 24 and rtc.MeshNormalsView.triangle_normals.offset == 16
    hdr = open(os.path.join(ROOT, "include", "rtc.h")).read() + open(os.path.join(ROOT, "include", "rtc_scene.h")).read()
    assert "#define RT_SMOOTH_SHAPES 0xFFFFFFFFu" in hdr and "#define RT_OBJ_NORMALS 1u" in hdr
    assert "#define RT_NO_NORMAL 0xFFFFFFFFu" in hdr and "#define RT_ABI_VERSION 3\n" in hdr
    for sym in ("rt_scene_upload_smooth", "rt_smooth_expand", "rt_scene_smooth_info", "rt_mesh_load_obj_ex",
                "rt_mesh_normals_get", "rt_mesh_smooth_normals"):
        assert sym in rtc.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, hdr)


def _raw(descs):
    return bytes(memoryview(descs).cast("B"))


def test_smooth_expand_is_the_concatenation_rule(rtc):
    from rtc_amd import world as W
    ico = S.load(rtc, *S.icosphere(1))  # 80 triangles, all smooth
    verts, faces, normals, fnorm = S.box(False)
    box = rtc.load_obj(S.obj_text(verts, faces, normals, fnorm).replace("f 1//1 3//3 4//4", "f 1//1 3 4//4")
                       .replace("f 1//1 4//4 3//3", "f 1//1 4 3//3"), normals=True)
    assert box.n_smooth == 11  # one face left flat
    p1, p2, p3 = (0, 1, 0), (-1, 0, 0), (1, 0, 0)
    world = W.World([], [W.sphere(), W.smooth_triangle(p1, p2, p3, p1, p2, p3), W.triangle(p1, p2, p3)],
                    [W.instance(ico, transform=W.translation(1, 2, 3), smooth=True),
                     W.instance(box, transform=W.scaling(2, 2, 2), smooth=True),
                     W.instance(ico, transform=W.rotation_y(0.3)),  # the same file placed flat: another mesh
                     W.instance(ico, transform=W.rotation_x(0.3), smooth=True)])
    t = world.tables()
    assert len(t.meshes) == 3 and [i.mesh for i in t.instances] == [0, 1, 2, 0]
    assert len(t.smooth) == 80 + 11 + 1
    flat = t.expanded()
    assert len(flat.shapes) == 3 + 80 + 12 + 80 + 80 and len(flat.smooth) == 1 + 80 + 11 + 80
    idx = [e.index for e in flat.smooth]
    assert idx == sorted(idx) and all(e.list == rtc.RT_SMOOTH_SHAPES for e in flat.smooth)
    flat_face = int(np.nonzero(box.triangle_normals[:, 0] == rtc.RT_NO_NORMAL)[0][0])
    want = [1] + list(range(3, 83)) + [83 + j for j in range(12) if j != flat_face] + list(range(175, 255))
    assert idx == want
    # instance k's triangle j carries the mesh's local normals, whatever the placement
    local = ico.smooth_descs()
    for j in (0, 17, 79):
        for base in (3, 175):
            e = flat.smooth[idx.index(base + j)]
            assert _raw(e)[8:] == _raw(local[j])[8:]
    # a plain world's expansion is itself
    plain = W.World([], [W.smooth_triangle(p1, p2, p3, p1, p2, p3)]).tables()
    assert plain.expanded() is plain


def test_upload_refusals_have_their_own_messages_with_a_null_context(rtc):
    from rtc_amd import world as W
    p1, p2, p3 = (0, 1, 0), (-1, 0, 0), (1, 0, 0)
    ico = S.load(rtc, *S.icosphere(0))  # 20 triangles
    base = W.World([W.Light((0, 0, -5))], [W.sphere(), W.smooth_triangle(p1, p2, p3, p1, p2, p3)],
                   [W.instance(ico, smooth=True)])

    def refusal(edit, null_list=False):
        t = base.tables()
        edit(t.smooth)
        args = list(t.smooth_args())
        if null_list:
            args[6] = None
        rc = rtc._lib.rt_scene_upload_smooth(None, *args)
        return rc, rtc._lib.rt_last_error().decode()

    def setter(k, **kw):
        def edit(sm):
            for name, value in kw.items():
                if name.startswith("normal"):
                    getattr(sm[k], name)[1] = value
                else:
                    setattr(sm[k], name, value)
        return edit

    cases = [
        (setter(0, list=1), "smooth entry 0: list index out of range"),
        (setter(20, index=2), "smooth entry 20: triangle index out of range"),
        (setter(3, index=20), "smooth entry 3: triangle index out of range"),
        (setter(20, index=0), "smooth entry 20: the named record is not a triangle"),
        (setter(5, index=4), "smooth entry 5: the same triangle is named twice"),
        (setter(7, normal_2=float("nan")), "smooth entry 7: a normal component is not finite"),
        (setter(20, normal_3=float("inf")), "smooth entry 20: a normal component is not finite"),
    ]
    seen = set()
    for edit, text in cases:
        rc, msg = refusal(edit)
        assert rc == rtc.RT_ERR_INVALID and msg == text, (msg, text)
        seen.add(re.sub(r"\d+", "N", msg))
    rc, msg = refusal(lambda sm: None, null_list=True)
    assert rc == rtc.RT_ERR_INVALID and msg == "rt_scene_upload_smooth: null smooth list with nonzero count"
    seen.add(msg)
    assert len(seen) == 6  # each refusal its own text
    # a well-formed list passes the checks and then meets the null context, as the instanced upload does
    rc, msg = refusal(lambda sm: None)
    assert rc == rtc.RT_ERR_INVALID and msg == "null context"
    # the instanced lists' own refusals still come first
    t = base.tables()
    t.instances[0].mesh = 5
    assert rtc._lib.rt_scene_upload_smooth(None, *t.smooth_args()) == rtc.RT_ERR_INVALID
    assert rtc._lib.rt_last_error().decode() == "instance 0: mesh index out of range"
    # rt_smooth_expand refuses the same lists
    t = base.tables()
    t.smooth[0].list = 9
    n = C.c_uint32(0)
    assert rtc._lib.rt_smooth_expand(*t.smooth_args()[:8], None, C.byref(n)) == rtc.RT_ERR_INVALID
    assert rtc._lib.rt_last_error().decode() == "smooth entry 0: list index out of range"


def test_world_mesh_smooth_is_smooth_triangle_per_face(rtc):
    from rtc_amd import world as W
    verts, faces, normals = S.icosphere(1)
    mesh = S.load(rtc, verts, faces, normals)
    mat = S.opaque()
    by_mesh = W.World([S.eye_light()], [W.sphere()] + W.mesh(mesh, mat, smooth=True)).tables()
    by_face = W.World([S.eye_light()], [W.sphere()] + [
        W.smooth_triangle(*(tuple(verts[i]) for i in f), *(tuple(normals[i]) for i in f), mat) for f in faces.tolist()
    ]).tables()
    assert _raw(by_mesh.shapes) == _raw(by_face.shapes) and _raw(by_mesh.smooth) == _raw(by_face.smooth)
    assert _raw(by_mesh.materials) == _raw(by_face.materials) and len(by_mesh.smooth) == 80
    assert [e.index for e in by_mesh.smooth] == list(range(1, 81))
    # faces without normals stay flat, and smooth=False names none
    assert W.World([], W.mesh(mesh, mat)).tables().smooth is None
    flat = rtc.load_obj(S.obj_text(verts, faces))
    assert W.World([], W.mesh(flat, mat, smooth=True)).tables().smooth is None
    # baked: the normals go through (T^-1)^T, unnormalized; the picture is the unbaked one up to rounding
    T = W.mat_mul(W.rotation_y(0.7), W.shearing(0.3, 0.0, 0.0, 0.2, 0.0, 0.0))
    baked = W.mesh(mesh, mat, transform=T, bake=True, smooth=True)
    inv = np.array(W.inverse(T))[:3, :3]
    for j in (0, 33, 79):
        for c in range(3):
            assert np.allclose(baked[j].normals[c], inv.T @ normals[faces[j][c]], rtol=0, atol=1e-15)


# ----------------------------------------------------------------- 4: identity
def test_identity_rule_stand_alone(tmp_path):
    exe = tmp_path / "smooth_identity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *_sanitize_flags(tmp_path), "-o",
                    str(exe), os.path.join(HERE, "smooth_identity.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "ok", out.stdout + out.stderr


def test_cli_knows_the_switch(rtc):
    cli = os.path.join(os.path.dirname(rtc.lib_path()), "rtc")
    r = subprocess.run([cli], capture_output=True, text=True)
    assert r.returncode != 0 and "[--smooth]" in r.stderr and "--smooth makes --obj and --instance" in r.stderr
