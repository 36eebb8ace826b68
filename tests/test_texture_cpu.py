"""Image textures without a GPU: the OBJ parser's vt lines, the
image reader, the struct layouts and refusals of rt_scene_upload_textured with a
null context, rt_uv_expand, the world builder, the numpy reference against the
book's known answers, and the identity rule and the file readers as stand-alone
programs under the host sanitizers where g++ has them.
"""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import texture_reference as T
import texture_worlds as X
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))

PARSER_TEXT = """# five vertices, texture coordinates with two and three components, one of each kind of face
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0.5 1.5 0
vn 0 0 1
vt 0 0
vt 1 0 0.5
f 1/1 2/2 3/-1
vt 1 1
vt 0.25 0.75 0
f 1/1/1 2/2/1 3/3/1 4/4/1 5/-4/1
f 1//1 2//1 3//1
f 1/1 2 3/3
g tail
f -5/-1 -4/-2 -3/-3
"""


def _sanitize_flags(tmp_path):
    """-fsanitize=address,undefined where this g++ links them (a stand-alone program: no preload)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++", *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0
    return flags if ok else []


@pytest.fixture(scope="module")
def io_program(tmp_path_factory):
    """tests/texture_io_main.cpp: the parser and the image reader with their own main."""
    tmp = tmp_path_factory.mktemp("texture_io")
    exe = tmp / "texture_io"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *_sanitize_flags(tmp), "-o", str(exe),
                    os.path.join(HERE, "texture_io_main.cpp"), "-lz"], check=True)
    return str(exe)


# ------------------------------------------------------------------ 1: parser
def test_parser_reads_texture_coordinates_under_the_flag(rtc):
    m = rtc.load_obj(PARSER_TEXT, texcoords=True)
    assert m.ignored_lines == 3  # the comment, vn, g: vt is no longer among them
    assert np.array_equal(m.texcoords, [[0, 0], [1, 0], [1, 1], [0.25, 0.75]])  # the third component is dropped
    no = rtc.RT_NO_TEXCOORD
    # f i/j with a negative index (2 read so far), the fan of five with i/j/k and -4, i//k (no coordinates),
    # a face with one vertex lacking a coordinate (none), negative indices after all four
    assert m.triangles.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 1, 2], [0, 1, 2], [0, 1, 2]]
    assert m.triangle_texcoords.tolist() == [[0, 1, 1], [0, 1, 2], [0, 2, 3], [0, 3, 0], [no] * 3, [no] * 3, [3, 2, 1]]
    assert m.n_textured == 5 and m.n_smooth == 0 and m.normals.shape == (0, 3)
    uv = m.uv_descs()
    assert [d.index for d in uv] == [0, 1, 2, 3, 6] and all(d.list == rtc.RT_SMOOTH_SHAPES for d in uv)
    assert list(uv[3].uv_1) == [0, 0] and list(uv[3].uv_2) == [0.25, 0.75] and list(uv[3].uv_3) == [0, 0]
    assert [d.index for d in m.uv_descs(list_index=2, first=10)] == [10, 11, 12, 13, 16]
    # both flags together: the normals of the i/j/k and i//k faces too
    both = rtc.load_obj(PARSER_TEXT, texcoords=True, normals=True)
    assert both.ignored_lines == 2 and both.n_smooth == 4 and both.n_textured == 5
    assert np.array_equal(both.triangle_texcoords, m.triangle_texcoords)
    # CRLF
    crlf = rtc.load_obj(PARSER_TEXT.replace("\n", "\r\n"), texcoords=True)
    assert np.array_equal(crlf.triangle_texcoords, m.triangle_texcoords) and np.array_equal(crlf.texcoords, m.texcoords)
    assert crlf.ignored_lines == 3


def test_the_older_entry_points_give_todays_counts(rtc, tmp_path):
    lib = rtc._lib
    old = rtc.load_obj(PARSER_TEXT)
    assert old.ignored_lines == 7 and old.n_textured == 0 and old.texcoords.shape == (0, 2)  # comment, vn, 4 vt, g
    assert old.triangle_texcoords.shape == (0, 3) and len(old.triangles) == 7
    with_normals = rtc.load_obj(PARSER_TEXT, normals=True)
    assert with_normals.ignored_lines == 6 and with_normals.n_smooth == 4 and with_normals.n_textured == 0
    for flags, ignored in ((0, 7), (1, 6)):
        h = C.c_void_p()
        assert lib.rt_mesh_load_obj_ex(None, PARSER_TEXT.encode(), flags, C.byref(h)) == rtc.RT_OK
        v = rtc.MeshTexcoordsView()
        assert lib.rt_mesh_texcoords_get(h, C.byref(v)) == rtc.RT_OK
        assert (v.n_texcoords, v.n_textured, bool(v.texcoords), bool(v.triangle_texcoords)) == (0, 0, False, False)
        mv = rtc.MeshView()
        assert lib.rt_mesh_view_get(h, C.byref(mv)) == rtc.RT_OK and mv.ignored_lines == ignored
        lib.rt_mesh_free(h)
    path = tmp_path / "m.obj"
    path.write_text(PARSER_TEXT)
    assert rtc.load_obj(str(path), texcoords=True).n_textured == 5
    # flag 2 stays the unknown flag; so is everything above 4 | 1
    h = C.c_void_p()
    for flags in (2, 3, 6, 8):
        assert lib.rt_mesh_load_obj_ex(None, b"v 0 0 0\n", flags, C.byref(h)) == rtc.RT_ERR_INVALID
        assert b"unknown flag" in lib.rt_last_error()


@pytest.mark.parametrize("line,text", [
    ("vt 1", "line 4: a texture coordinate needs two components"),
    ("vt 1 two", "line 4: 'two' is not a number in a texture coordinate"),
    ("vt 1 2 x", "line 4: 'x' is not a number in a texture coordinate"),
    ("f 1/1 2/x 3/1", "line 4: '2/x' is not a texture index"),
    ("f 1/1 2/2/1 3/1", "line 4: texture index 2 out of range (1 texture coordinates so far)"),
    ("f 1/1 2/0 3/1", "line 4: texture index 0 out of range (1 texture coordinates so far)"),
    ("f 1/1 2/-2 3/1", "line 4: texture index -2 out of range (1 texture coordinates so far)"),
])
def test_parser_errors_carry_the_line_number(rtc, line, text):
    head = "v 0 0 0\nv 1 0 0\nvt 0 0\n"
    with pytest.raises(rtc.RenderError) as e:
        rtc.load_obj(head + line + "\nv 0 1 0\nvt 1 0\n", texcoords=True)
    assert e.value.code == rtc.RT_ERR_IO and text in str(e.value), str(e.value)
    rtc.load_obj(head + "v 0 1 0\n" + ("f 1 2 3\n" if line.startswith("f") else line + "\n"))  # without the flag: skipped


def test_parser_stand_alone_under_the_host_sanitizers(io_program, tmp_path):
    obj = tmp_path / "m.obj"
    obj.write_text(PARSER_TEXT)
    out = subprocess.run([io_program, "obj", str(obj)], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", out.stdout + out.stderr
    assert "flags 0: 5 vertices 7 triangles 7 ignored 0 normals 0 smooth 0 texcoords 0 textured" in lines
    assert "flags 1: 5 vertices 7 triangles 6 ignored 1 normals 4 smooth 0 texcoords 0 textured" in lines
    assert "flags 4: 5 vertices 7 triangles 3 ignored 0 normals 0 smooth 4 texcoords 5 textured" in lines
    assert "flags 5: 5 vertices 7 triangles 2 ignored 1 normals 4 smooth 4 texcoords 5 textured" in lines
    assert "  list 7 index 3 t1 0 0 t2 0.25 0.75 t3 0 0" in lines
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nvt 0\n")
    out = subprocess.run([io_program, "obj", str(bad)], capture_output=True, text=True)
    assert out.returncode == 0 and "flags 4: error -7: OBJ: line 2: a texture coordinate needs two components" in out.stdout
    assert "flags 0: 1 vertices 0 triangles 1 ignored" in out.stdout


# ------------------------------------------------------------ 2: image reader
def _png(rows, width, channels, filters, chunks=()):
    """A PNG of 8-bit `channels`-channel `rows` (lists of bytes) whose row y is written with filter type
    filters[y % len(filters)], put together with zlib here."""
    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))

    def paeth(a, b, c):
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        return a if pa <= pb and pa <= pc else (b if pb <= pc else c)
    raw, prev = bytearray(), [0] * (width * channels)
    for y, row in enumerate(rows):
        f = filters[y % len(filters)]
        raw.append(f)
        for i, x in enumerate(row):
            a = row[i - channels] if i >= channels else 0
            b = prev[i]
            c = prev[i - channels] if i >= channels else 0
            pred = (0, a, b, (a + b) // 2, paeth(a, b, c))[f]
            raw.append((x - pred) & 0xFF)
        prev = list(row)
    ihdr = struct.pack(">IIBBBBB", width, len(rows), 8, 2 if channels == 3 else 6, 0, 0, 0)
    body = b"".join(chunk(k, d) for k, d in chunks)
    z = zlib.compress(bytes(raw))
    half = len(z) // 2  # two IDAT chunks: the reader joins them
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + body + chunk(b"IDAT", z[:half]) + chunk(b"IDAT", z[half:]) +
            chunk(b"IEND", b""))


def test_written_images_read_back_unchanged(rtc, tmp_path):
    for shape in ((7, 5), (1, 1), (1, 9), (6, 1)):
        img = X.colors(shape[1], shape[0], seed=shape[0])
        for fmt, name in (("png", "a.png"), ("ppm", "a.ppm"), ("ppm-binary", "b.ppm")):
            path = tmp_path / name
            rtc.write_image(str(path), img, fmt)
            back = rtc.read_image(str(path))
            assert back.dtype == np.uint8 and np.array_equal(back, img), (shape, fmt)


def test_ppm_with_comments_maxval_and_long_lines(rtc, tmp_path):
    p = tmp_path / "c.ppm"
    p.write_text("P3\n# a comment\n2 1\n# another\n15\n15 0 7 # trailing\n0 8 15\n")
    assert rtc.read_image(str(p)).tolist() == [[[255, 0, 119], [0, 136, 255]]]  # round(v * 255 / 15)
    p.write_text("P3 3 1 255 " + " ".join(str(v) for v in range(9)))  # everything on one line
    assert rtc.read_image(str(p)).reshape(-1).tolist() == list(range(9))
    p.write_text("P3\n1 3\n255\n1\n2\n3\n4\n5\n6\n7\n8\n9\n")  # one sample a line
    assert rtc.read_image(str(p)).reshape(-1).tolist() == list(range(1, 10))
    p.write_bytes(b"P6\n1 2\n65535\n" + struct.pack(">6H", 65535, 0, 32768, 257, 128, 65534))  # two bytes a sample
    assert rtc.read_image(str(p)).reshape(-1).tolist() == [255, 0, 128, 1, 0, 255]
    book = tmp_path / "book.ppm"
    book.write_text(T.BOOK_PPM)
    img = rtc.read_image(str(book))
    assert img.shape == (10, 10, 3) and img[0, 9].tolist() == [230] * 3 and img[9, 0].tolist() == [230] * 3


def test_png_rgba_and_every_filter_type(rtc, tmp_path):
    rng = np.random.default_rng(3)
    for channels in (3, 4):
        pix = rng.integers(0, 256, size=(10, 6, channels), dtype=np.uint8)
        p = tmp_path / f"f{channels}.png"
        p.write_bytes(_png([row.reshape(-1).tolist() for row in pix], 6, channels, (0, 1, 2, 3, 4),
                           chunks=[(b"tEXt", b"Comment\0an ancillary chunk")]))
        assert np.array_equal(rtc.read_image(str(p)), pix[..., :3]), channels  # alpha dropped
    for f in range(5):  # each filter type alone, first row included
        pix = rng.integers(0, 256, size=(3, 4, 3), dtype=np.uint8)
        p = tmp_path / f"only{f}.png"
        p.write_bytes(_png([row.reshape(-1).tolist() for row in pix], 4, 3, (f,)))
        assert np.array_equal(rtc.read_image(str(p)), pix), f


def test_malformed_images_are_refused_with_their_own_texts(rtc, tmp_path, io_program):
    good = _png([[1, 2, 3, 4, 5, 6]], 2, 3, (0,))

    def ihdr(depth=8, kind=2, comp=0, filt=0, lace=0, w=2, h=1):
        data = struct.pack(">IIBBBBB", w, h, depth, kind, comp, filt, lace)
        return good[:12] + b"IHDR" + data + struct.pack(">I", zlib.crc32(b"IHDR" + data)) + good[33:]
    crit = good[:33] + struct.pack(">I", 1) + b"ABCD" + b"x" + struct.pack(">I", zlib.crc32(b"ABCDx")) + good[33:]
    cases = {
        "nothing.bin": (b"GIF89a", "neither a PPM (P3, P6) nor a PNG file"),
        "cut.png": (good[:-20], "PNG: truncated"),
        "crc.png": (good[:40] + bytes([good[40] ^ 1]) + good[41:], "PNG: chunk checksum mismatch"),
        "first.png": (good[:8] + good[33:], "PNG: the first chunk is not IHDR"),
        "depth.png": (ihdr(depth=16), "PNG: only 8 bits per channel are read"),
        "grey.png": (ihdr(kind=0), "PNG: only RGB and RGBA colour types are read"),
        "palette.png": (ihdr(kind=3), "PNG: only RGB and RGBA colour types are read"),
        "lace.png": (ihdr(lace=1), "PNG: interlaced images are not read"),
        "method.png": (ihdr(comp=1), "PNG: unknown compression or filter method"),
        "size.png": (ihdr(w=3), "PNG: the image data do not inflate to width x height pixels"),
        "zero.png": (ihdr(w=0), "PNG: bad width or height"),
        "critical.png": (crit, "PNG: unknown critical chunk ABCD"),
        "p3short.ppm": (b"P3\n2 1\n255\n1 2 3 4 5\n", "PPM: truncated pixel data"),
        "p6short.ppm": (b"P6\n2 1\n255\n12345", "PPM: truncated pixel data"),
        "p3word.ppm": (b"P3\n1 1\n255\n1 x 3\n", "PPM: 'x' is not a sample in 0..255"),
        "p3big.ppm": (b"P3\n1 1\n15\n1 16 3\n", "PPM: '16' is not a sample in 0..15"),
        "p6big.ppm": (b"P6\n1 1\n15\n\x01\x10\x03", "PPM: a sample exceeds maxval"),
        "maxval.ppm": (b"P3\n1 1\n65536\n1 2 3\n", "PPM: maxval must be in 1..65535"),
        "maxval0.ppm": (b"P3\n1 1\n0\n0 0 0\n", "PPM: maxval must be in 1..65535"),
        "width.ppm": (b"P3\n0 1\n255\n", "PPM: bad width or height"),
        "head.ppm": (b"P6\n1 1\n255", "PPM: no whitespace after maxval"),
    }
    # a row whose filter type byte is 5
    raw = zlib.compress(bytes([5, 1, 2, 3]))
    bad_row = good[:33] + struct.pack(">I", len(raw)) + b"IDAT" + raw + struct.pack(">I", zlib.crc32(b"IDAT" + raw)) + good[-12:]
    cases["rowfilter.png"] = (ihdr(w=1)[:33] + bad_row[33:], "PNG: unknown filter type in a row")
    seen = set()
    for name, (data, text) in cases.items():
        path = tmp_path / name
        path.write_bytes(data)
        with pytest.raises(rtc.RenderError) as e:
            rtc.read_image(str(path))
        assert e.value.code == rtc.RT_ERR_IO and text in str(e.value), (name, str(e.value))
        seen.add(text)
        out = subprocess.run([io_program, "image", str(path)], capture_output=True, text=True)  # under the sanitizers
        assert out.returncode == 0 and "error -7" in out.stdout and text in out.stdout, (name, out.stdout + out.stderr)
    assert len(seen) == 19
    with pytest.raises(rtc.RenderError, match="cannot open"):
        rtc.read_image(str(tmp_path / "missing.png"))
    # and a good file of each format through the stand-alone reader
    (tmp_path / "good.png").write_bytes(_png([[1, 2, 3, 9, 4, 5, 6, 9], [7, 8, 9, 0, 10, 11, 12, 0]], 2, 4, (4, 3)))
    out = subprocess.run([io_program, "image", str(tmp_path / "good.png")], capture_output=True, text=True)
    assert out.stdout.splitlines() == ["2 x 2: 1 2 3 4 5 6 7 8 9 10 11 12", "ok"], out.stdout + out.stderr
    (tmp_path / "good.ppm").write_text("P3\n# c\n2 1 # d\n3\n0 1 2 3 2 1")
    out = subprocess.run([io_program, "image", str(tmp_path / "good.ppm")], capture_output=True, text=True)
    assert out.stdout.splitlines() == ["2 x 1: 0 85 170 255 170 85", "ok"], out.stdout + out.stderr


# ------------------------------------------------------------------ 3: ABI
def test_struct_layouts_match_the_headers_and_a_compiled_probe(rtc, tmp_path):
    structs = (("rtc.h", "rt_uv_desc", rtc.UVDesc), ("rtc.h", "rt_texture_desc", rtc.TextureDesc),
               ("rtc.h", "rt_texture_info", rtc.TextureInfo), ("rtc_scene.h", "rt_mesh_texcoords_view", rtc.MeshTexcoordsView))
    probe = ['#include <cstddef>\n#include <cstdio>\n#include "rtc_scene.h"\nint main() {']
    for header, name, cls in structs:
        hdr = open(os.path.join(ROOT, "include", header)).read()
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in [d for d in body.split(";") if d.strip()]:
            names = decl.split(",")
            fields += [re.sub(r"\[\d+\]", "", names[0].split()[-1].lstrip("*"))]
            fields += [re.sub(r"\[\d+\]", "", n.strip().lstrip("*")) for n in names[1:]]
        assert fields == [n for n, _ in cls._fields_], name
        probe.append(f'std::printf("{name} %zu", sizeof({name}));')
        probe += [f'std::printf(" %zu", offsetof({name}, {f}));' for f in fields]
        probe.append('std::printf("\\n");')
    probe.append("return 0; }")
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text("\n".join(probe))
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for (header, name, cls), line in zip(structs, lines):
        want = [name, str(C.sizeof(cls))] + [str(getattr(cls, f).offset) for f, _ in cls._fields_]
        assert line.split() == want, (line, want)
    assert C.sizeof(rtc.UVDesc) == 56 and rtc.UVDesc.uv_1.offset == 8 and rtc.UVDesc.uv_3.offset == 40
    hdr = open(os.path.join(ROOT, "include", "rtc.h")).read() + open(os.path.join(ROOT, "include", "rtc_scene.h")).read()
    assert "RT_PATTERN_IMAGE = 6" in hdr and "#define RT_OBJ_TEXCOORDS 4u" in hdr and "#define RT_ABI_VERSION 3\n" in hdr
    assert rtc.PATTERN_KINDS["image"] == 6 and rtc.RT_OBJ_TEXCOORDS == 4 and rtc.TEXTURE_FILTERS == {"nearest": 0, "bilinear": 1}
    for sym in ("rt_scene_upload_textured", "rt_uv_expand", "rt_scene_texture_info", "rt_mesh_texcoords_get", "rt_mesh_uvs",
                "rt_image_read"):
        assert sym in rtc.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, hdr)
    assert "rt_image_free" in rtc.EXPORTED_SYMBOLS and re.search(r"\bvoid rt_image_free\(", hdr)


def _raw(descs):
    return bytes(memoryview(descs).cast("B"))


def _base_world(rtc):
    from rtc_amd import world as W
    verts, faces = X.M.icosphere(0)  # 20 triangles
    ico = X.load(rtc, verts, faces, X.ico_coords(verts))
    p1, p2, p3 = (0, 1, 0), (-1, 0, 0), (1, 0, 0)
    mat = X.textured_material(X.SIX, "bilinear")
    other = W.Material(pattern=W.image_pattern(X.colors(5, 7), "nearest"))
    return W.World([W.Light((0, 0, -5))], [W.sphere(other), W.textured_triangle(p1, p2, p3, (0, 0), (1, 0), (0, 1), mat)],
                   [W.instance(ico, mat, textured=True)]), ico


def test_uv_expand_is_the_concatenation_rule(rtc):
    from rtc_amd import world as W
    verts, faces = X.M.icosphere(1)  # 80 triangles
    ico = X.load(rtc, verts, faces, X.ico_coords(verts))
    bverts, bfaces, _, _ = X.S.box(True)
    ft = [tuple(f) for f in bfaces.tolist()]
    ft[4] = None  # one face without coordinates
    box = X.load(rtc, bverts, bfaces, bverts[:, :2], face_texcoords=ft)
    assert ico.n_textured == 80 and box.n_textured == 11
    p1, p2, p3 = (0, 1, 0), (-1, 0, 0), (1, 0, 0)
    world = W.World([], [W.sphere(), W.textured_triangle(p1, p2, p3, (0, 0), (1, 0), (0.5, 1)), W.triangle(p1, p2, p3)],
                    [W.instance(ico, transform=W.translation(1, 2, 3), textured=True),
                     W.instance(box, transform=W.scaling(2, 2, 2), textured=True),
                     W.instance(ico, transform=W.rotation_y(0.3)),  # the same file without coordinates: another mesh
                     W.instance(ico, transform=W.rotation_x(0.3), textured=True)])
    t = world.tables()
    assert len(t.meshes) == 3 and [i.mesh for i in t.instances] == [0, 1, 2, 0] and len(t.uvs) == 80 + 11 + 1
    flat = t.expanded()
    assert len(flat.shapes) == 3 + 80 + 12 + 80 + 80 and len(flat.uvs) == 1 + 80 + 11 + 80
    idx = [e.index for e in flat.uvs]
    want = [1] + list(range(3, 83)) + [83 + j for j in range(12) if j != 4] + list(range(175, 255))
    assert idx == want and all(e.list == rtc.RT_SMOOTH_SHAPES for e in flat.uvs)
    local = ico.uv_descs()
    for j in (0, 17, 79):  # instance k's triangle j carries the mesh's coordinates, whatever the placement
        for base in (3, 175):
            assert _raw(flat.uvs[idx.index(base + j)])[8:] == _raw(local[j])[8:]
    n = C.c_uint32(0)  # out = NULL counts
    assert rtc._lib.rt_uv_expand(*t.instanced_args()[:6], t.uvs, len(t.uvs), None, C.byref(n)) == rtc.RT_OK
    assert n.value == 172
    plain = W.World([], [W.textured_triangle(p1, p2, p3, (0, 0), (1, 0), (0.5, 1))]).tables()
    assert plain.expanded() is plain and plain.textured


def test_upload_refusals_have_their_own_messages_with_a_null_context(rtc):
    base, _ = _base_world(rtc)

    def refusal(edit, null=None):
        t = base.tables()
        keep = edit(t)
        args = list(t.textured_args())
        if keep is not None:
            args[10] = keep
        if null is not None:
            args[null] = None
        rc = rtc._lib.rt_scene_upload_textured(None, *args)
        return rc, rtc._lib.rt_last_error().decode()

    def uv(k, **kw):
        def edit(t):
            for name, value in kw.items():
                if name.startswith("uv_"):
                    getattr(t.uvs[k], name)[1] = value
                else:
                    setattr(t.uvs[k], name, value)
        return edit

    def pattern(k, **kw):
        def edit(t):
            for name, value in kw.items():
                setattr(t.patterns[k], name, value)
        return edit

    def texture(k, **kw):
        def edit(t):
            td = t.texture_descs()
            for name, value in kw.items():
                setattr(td[k], name, value)
            return td
        return edit

    def complex_over_image(t):
        t.patterns[1].kind, t.patterns[1].sub_a, t.patterns[1].sub_b, t.patterns[1].reserved = 4, 0, 0, 0

    t0 = base.tables()
    assert [p.kind for p in t0.patterns] == [6, 6] and len(t0.textures) == 2 and len(t0.uvs) == 21
    cases = [
        (uv(0, list=1), "uv entry 0: list index out of range"),
        (uv(20, index=2), "uv entry 20: triangle index out of range"),
        (uv(3, index=20), "uv entry 3: triangle index out of range"),
        (uv(20, index=0), "uv entry 20: the named record is not a triangle"),
        (uv(5, index=4), "uv entry 5: the same triangle is named twice"),
        (uv(7, uv_2=float("nan")), "uv entry 7: a texture coordinate is not finite"),
        (uv(20, uv_3=float("inf")), "uv entry 20: a texture coordinate is not finite"),
        (texture(1, rgb=None), "texture 1: null pixels"),
        (texture(0, width=0), "texture 0: zero width or height"),
        (texture(1, height=0), "texture 1: zero width or height"),
        (texture(1, width=1 << 20, height=257), "texture 1: more than 2^28 texels"),
        (pattern(0, sub_a=2), "pattern 0: texture index out of range"),
        (pattern(1, sub_a=-1), "pattern 1: texture index out of range"),
        (pattern(1, sub_b=0), "pattern 1: an image pattern's sub_b must be -1"),
        (pattern(0, reserved=2), "pattern 0: unknown texture filter"),
        (pattern(0, kind=7), "pattern 0: unknown kind"),
        (complex_over_image, "pattern 1: an image pattern cannot be a sub-pattern"),
    ]
    seen = set()
    for edit, text in cases:
        rc, msg = refusal(edit)
        assert rc == rtc.RT_ERR_INVALID and msg == text, (msg, text)
        seen.add(re.sub(r"\d+", "N", msg))
    rc, msg = refusal(lambda t: None, null=8)
    assert rc == rtc.RT_ERR_INVALID and msg == "rt_scene_upload_textured: null uv list with nonzero count"
    seen.add(msg)
    rc, msg = refusal(lambda t: None, null=10)
    assert rc == rtc.RT_ERR_INVALID and msg == "rt_scene_upload_textured: null texture list with nonzero count"
    seen.add(msg)
    assert len(seen) == 15  # each refusal its own text
    rc, msg = refusal(lambda t: None)  # a well-formed world passes the checks and then meets the null context
    assert rc == rtc.RT_ERR_INVALID and msg == "null context"
    # the older lists' refusals still come first, and rt_uv_expand refuses the same coordinate lists
    t = base.tables()
    t.instances[0].mesh = 5
    assert rtc._lib.rt_scene_upload_textured(None, *t.textured_args()) == rtc.RT_ERR_INVALID
    assert rtc._lib.rt_last_error().decode() == "instance 0: mesh index out of range"
    t = base.tables()
    t.uvs[0].list = 9
    n = C.c_uint32(0)
    assert rtc._lib.rt_uv_expand(*t.instanced_args()[:6], t.uvs, len(t.uvs), None, C.byref(n)) == rtc.RT_ERR_INVALID
    assert rtc._lib.rt_last_error().decode() == "uv entry 0: list index out of range"


def test_of_two_defects_the_earlier_check_is_the_one_reported(rtc):
    """The order of the refusals is part of the contract (rtc.h: "checked before the context is looked at").
    Every entry point gets tables with two defects from different steps of its order, and a null context:
      rt_scene_upload            the context, then the base tables;
      _instanced, _smooth        base tables, mesh/instance lists, smooth list, then the context;
      _textured                  texture list, base tables, mesh/instance lists, smooth list, uv list, context;
      _lit                       area list, then as _textured, then the light total, then the context;
    an empty newest list is the previous entry point."""
    base, _ = _base_world(rtc)
    lib = rtc._lib
    SHAPE, INSTANCE = "shape 0: unknown kind", "instance 0: mesh index out of range"
    SMOOTH, UV = "smooth entry 0: list index out of range", "uv entry 0: list index out of range"
    TEXTURE, AREA = "texture 0: zero width or height", "area light 0: a step count of 0"

    def call(entry, *defects, images=True):
        t = base.tables()
        if not images:  # the older entry points do not know pattern kind 6
            for p in t.patterns:
                p.kind = 0
        a = list(t.textured_args()) + [(rtc.AreaLightDesc * 1)(), 1]
        a[18][0].usteps = a[18][0].vsteps = 1  # one valid light of one sample (rt_scene_upload_lit only)
        for d in defects:
            if d == "shape":
                t.shapes[0].kind = 99
            elif d == "instance":
                t.instances[0].mesh = 5
            elif d == "smooth":
                a[6], a[7] = (rtc.SmoothDesc * 1)(), 1
                a[6][0].list = 9
            elif d == "uv":
                t.uvs[0].list = 9
            elif d == "texture":
                a[10][0].width = 0
            elif d == "area":
                a[18][0].usteps = 0
            elif d == "total":  # 2^31 - 1 point lights and one sample (the checks never read the lights)
                a[17] = 0x7FFFFFFF
            elif d == "no area":
                a[19] = 0
            elif d == "no smooth":
                a[6], a[7] = None, 0
        args = {"upload": a[0:2] + a[12:18], "instanced": a[0:6] + a[12:18], "smooth": a[0:8] + a[12:18],
                "textured": a[0:18], "lit": a[0:18] + a[18:20]}[entry]
        assert getattr(lib, "rt_scene_upload" + ("" if entry == "upload" else "_" + entry))(None, *args) == rtc.RT_ERR_INVALID
        return lib.rt_last_error().decode()

    assert call("upload", "shape", images=False) == "null context"
    assert call("upload", "shape") == "null context"
    for entry in ("instanced", "smooth"):
        assert call(entry, "shape", "instance", images=False) == SHAPE
        assert call(entry, "instance", images=False) == INSTANCE  # (... and the null context)
        assert call(entry, images=False) == "null context"
        assert call(entry, "instance") == "pattern 0: unknown kind"
    assert call("smooth", "instance", "smooth", images=False) == INSTANCE
    assert call("smooth", "smooth", images=False) == SMOOTH
    assert call("smooth", "no smooth", "instance", images=False) == INSTANCE  # rt_scene_upload_instanced itself
    assert call("textured", "texture", "shape") == TEXTURE
    assert call("textured", "shape", "instance") == SHAPE
    assert call("textured", "instance", "smooth") == INSTANCE
    assert call("textured", "smooth", "uv") == SMOOTH
    assert call("textured", "uv") == UV
    assert call("textured") == "null context"
    assert call("lit", "area", "texture") == AREA
    assert call("lit", "area", "uv") == AREA
    assert call("lit", "texture", "shape") == TEXTURE
    assert call("lit", "shape", "instance") == SHAPE
    assert call("lit", "smooth", "uv") == SMOOTH
    assert call("lit", "uv", "total") == UV
    assert call("lit", "total") == "table too large"
    assert call("lit") == "null context"
    assert call("lit", "no area", "texture", "shape") == TEXTURE  # rt_scene_upload_textured itself
    assert call("lit", "no area", "uv") == UV
    assert call("lit", "no area") == "null context"


def test_the_older_entry_points_do_not_know_pattern_kind_6(rtc):
    base, _ = _base_world(rtc)
    t = base.tables()
    lib = rtc._lib
    for rc in (lib.rt_scene_upload(None, *t.args()), lib.rt_scene_upload_instanced(None, *t.instanced_args()),
               lib.rt_scene_upload_smooth(None, *t.smooth_args())):
        assert rc == rtc.RT_ERR_INVALID and lib.rt_last_error().decode() == "pattern 0: unknown kind"


def test_world_builder_shares_textures_and_names_coordinates(rtc):
    from rtc_amd import world as W
    base, ico = _base_world(rtc)
    t = base.tables()
    assert t.textured and [p.sub_a for p in t.patterns] == [0, 1] and [p.sub_b for p in t.patterns] == [-1, -1]
    # (the instances' materials are flattened first: the icosphere's bilinear pattern, then the sphere's)
    assert [p.reserved for p in t.patterns] == [1, 0]
    assert np.array_equal(t.textures[0], X.SIX) and t.textures[1].shape == (7, 5, 3)
    assert [(e.list, e.index) for e in t.uvs][:2] == [(0, 0), (0, 1)] and (t.uvs[20].list, t.uvs[20].index) == (0xFFFFFFFF, 1)
    assert list(t.uvs[20].uv_2) == [1.0, 0.0]
    # two patterns over one array object share a texture; mesh(textured=True) is textured_triangle per face
    verts, faces = X.M.icosphere(0)
    tc = X.ico_coords(verts)
    mat = X.textured_material(X.SIX, "nearest")
    by_mesh = W.World([], W.mesh(ico, mat, textured=True)).tables()
    by_face = W.World([], [W.textured_triangle(*(tuple(verts[i]) for i in f), *(tuple(tc[i]) for i in f), mat)
                           for f in faces.tolist()]).tables()
    assert _raw(by_mesh.shapes) == _raw(by_face.shapes) and _raw(by_mesh.uvs) == _raw(by_face.uvs) and len(by_mesh.uvs) == 20
    assert len(by_mesh.textures) == 1 and len(by_mesh.patterns) == 1
    assert W.World([], W.mesh(ico, mat)).tables().uvs is None
    with pytest.raises(ValueError):
        W.image_pattern(np.zeros((2, 2), dtype=np.uint8))
    with pytest.raises(KeyError):
        W.image_pattern(X.SIX, "trilinear")


# ------------------------------------------------------ 4: the reference itself
def test_reference_gives_the_books_known_answers(rtc, tmp_path):
    book = tmp_path / "book.ppm"
    book.write_text(T.BOOK_PPM)
    img = rtc.read_image(str(book))
    # the book's colours are k / 10; the texture holds bytes, round(k * 25.5) / 255: within half a level
    for (u, v), grey in T.BOOK_UV_ANSWERS:
        got = T.uv_pattern_at(img, u, v)
        assert np.abs(got - grey).max() <= 0.5 / 255 and got[0] == got[1] == got[2], ((u, v), got)
    for point, (u, v) in T.BOOK_PLANAR:
        pu, pv = T.planar_map(np.array(point))
        assert (float(pu), float(pv)) == (u, v), point


def test_reference_sampling_rules():
    img = X.SIX  # 3 x 2
    tex = img.astype(np.float64) / 255.0
    # nearest: round half away from zero on x = 2 u and y = 1 - v; exactly 1 stays 1
    for (u, v), (yy, xx) in (((0.0, 1.0), (0, 0)), ((0.24, 1.0), (0, 0)), ((0.25, 1.0), (0, 1)), ((0.75, 0.0), (1, 2)),
                             ((1.0, 0.5), (1, 2)), ((1.0, 0.51), (0, 2)), ((0.5, 0.5), (1, 1))):
        assert np.array_equal(T.uv_pattern_at(img, u, v), tex[yy, xx]), (u, v)
    # bilinear: the formula in its order, and the corners are the texels
    got = T.uv_pattern_at(img, 0.3, 0.75, T.BILINEAR)
    fx, fy = 0.3 * 2.0 - 0.0, 0.25
    want = (tex[0, 0] * (1 - fx) + tex[0, 1] * fx) * (1 - fy) + (tex[1, 0] * (1 - fx) + tex[1, 1] * fx) * fy
    assert np.array_equal(got, want)
    assert np.array_equal(T.uv_pattern_at(img, 1.0, 0.0, T.BILINEAR), tex[1, 2])
    assert np.array_equal(T.uv_pattern_at(img, 0.0, 1.0, T.BILINEAR), tex[0, 0])
    # wrapping: inside [0, 1] as is (1 stays 1), outside c - floor(c); the margin is the distance to the change
    c, m = T.wrap(np.array([0.0, 1.0, 0.25, 1.25, -0.25, 2.0, -1e-12]))
    assert c[:6].tolist() == [0.0, 1.0, 0.25, 0.25, 0.75, 0.0] and abs(c[6] - 1.0) < 1e-11
    assert m[:5].tolist() == [0.0, 0.0, 0.25, 0.25, 0.25] and m[6] < 1e-11
    # the nearest filter's margin: the distance of the fractions from 0.5
    _, m = T.sample(img, T.NEAREST, np.array([0.3]), np.array([0.6]))
    assert abs(m[0] - 0.1) < 1e-12
    _, m = T.sample(X.uniform(1, 1), T.NEAREST, np.array([0.3]), np.array([0.6]))
    assert np.isinf(m[0])


def test_reference_without_textures_is_the_smooth_reference(rtc):
    import smooth_reference as R
    tables = X.S.ico_alone(rtc)
    rays = X.S.camera_rays(tables.camera)[::7]
    a, ha, ma = R.trace(tables, rays)
    b, hb, mb = T.trace(tables, rays)
    assert np.array_equal(a, b) and np.array_equal(ha["shape"], hb["shape"]) and np.array_equal(ma, mb)


# ----------------------------------------------------------------- 5: identity
def test_identity_rule_stand_alone(tmp_path):
    exe = tmp_path / "texture_identity"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *_sanitize_flags(tmp_path), "-o",
                    str(exe), os.path.join(HERE, "texture_identity.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "ok", out.stdout + out.stderr
    assert "refusals: 16 cases" in lines and "expansion: 6 entries" in lines
    assert "renumbering: independent of the patterns' order" in lines


def test_a_header_that_claims_more_than_the_file_holds_is_refused_before_anything_is_allocated(rtc, tmp_path, io_program):
    import time
    cases = {"big.ppm": (b"P6\n16384 16384\n255\n123", "PPM: truncated pixel data"),
             "big3.ppm": (b"P3\n16384 16384\n255\n1 2 3", "PPM: truncated pixel data")}
    ihdr = struct.pack(">IIBBBBB", 16384, 16384, 8, 2, 0, 0, 0)
    z = zlib.compress(bytes(40))

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))
    cases["big.png"] = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", z) + chunk(b"IEND", b""),
                        "PNG: the image data do not inflate to width x height pixels")
    for name, (data, text) in cases.items():
        path = tmp_path / name
        path.write_bytes(data)
        took = []
        for _ in range(3):
            t0 = time.perf_counter()
            with pytest.raises(rtc.RenderError, match=re.escape(text)):
                rtc.read_image(str(path))
            took.append(time.perf_counter() - t0)
        # (805 MB would take a few hundred ms to allocate and clear; the refusal reads 20 to 80 bytes)
        assert min(took) < 0.05, (name, took)
        out = subprocess.run([io_program, "image", str(path)], capture_output=True, text=True)
        assert out.returncode == 0 and text in out.stdout, out.stdout + out.stderr


def test_cli_refuses_a_texture_without_a_mesh(rtc, tmp_path):
    from test_cli import SCENE
    cli = os.path.join(os.path.dirname(rtc.lib_path()), "rtc")
    yaml = tmp_path / "scene.yaml"
    yaml.write_text(SCENE)
    r = subprocess.run([cli, str(yaml), str(tmp_path / "out.png"), "--texture", str(tmp_path / "missing.ppm")],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--texture needs a mesh to show on: give --obj or --instance" in r.stderr
    assert not (tmp_path / "out.png").exists()


def test_cli_knows_the_switches(rtc):
    cli = os.path.join(os.path.dirname(rtc.lib_path()), "rtc")
    r = subprocess.run([cli], capture_output=True, text=True)
    assert r.returncode != 0 and "[--texture IMAGE.ppm|png] [--texture-filter nearest|bilinear]" in r.stderr
    assert "--texture IMAGE.ppm|png gives the --obj and --instance meshes' material" in r.stderr
