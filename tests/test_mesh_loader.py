"""OBJ meshes on the host (rtc_scene.h rt_mesh_*; CPU only): the parser's
subset and its errors, rt_mesh_triangles against world.triangle bit for bit,
and a mesh world in the oracle."""
import ctypes as C

import numpy as np
import pytest

import mesh_worlds as M

RT_ERR_IO = -7


def _bits(desc_array):
    return bytes(memoryview(desc_array).cast("B"))


def test_fan_triangulation_indices_and_ignored_lines(rtc):
    text = "\n".join([
        "# a pentagon and a triangle",        # ignored
        "mtllib none.mtl",                    # ignored
        "v 0 0 0", "v 1 0 0", "v 1.5 1 0", "v 0.5 2 0.25", "v -0.5 1 0",
        "vn 0 0 1",                           # ignored
        "vt 0.5 0.5",                         # ignored
        "g first",                            # ignored
        "f 1 2 3 4 5",                        # fan: (1,2,3) (1,3,4) (1,4,5)
        "",                                   # ignored
        "v 2 2 2e0",
        "usemtl shiny",                       # ignored
        "s 1",                                # ignored
        "f -1 -6/1/1 3//1",                   # relative to the 6 vertices so far: (6, 1, 3)
        "f 2/7 4/8 6/9",
        "o tail",                             # ignored
    ]) + "\n"
    mesh = rtc.load_obj(text)
    assert mesh.vertices.shape == (6, 3) and mesh.vertices[3].tolist() == [0.5, 2.0, 0.25]
    assert mesh.vertices[5].tolist() == [2.0, 2.0, 2.0]
    assert mesh.triangles.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4], [5, 0, 2], [1, 3, 5]]
    assert mesh.triangles.dtype == np.uint32
    assert mesh.ignored_lines == 9


def test_crlf_and_file(rtc, tmp_path):
    verts, faces = M.height_field(2)
    unix = rtc.load_obj(M.obj_text(verts, faces))
    path = tmp_path / "crlf.obj"
    path.write_bytes(M.obj_text(verts, faces, newline="\r\n").encode())
    dos = rtc.load_obj(str(path))
    assert np.array_equal(dos.vertices, verts) and np.array_equal(dos.triangles, faces)
    assert np.array_equal(unix.vertices, dos.vertices) and np.array_equal(unix.triangles, dos.triangles)
    assert unix.ignored_lines == dos.ignored_lines == 3


@pytest.mark.parametrize("text, line, what", [
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", 4, "out of range"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 0\n", 4, "out of range"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\n# c\nf -4 1 2\n", 5, "out of range"),
    ("v 0 0 0\nv 1 zero 0\n", 2, "not a number"),
    ("v 0 0 0\nv 1 0\n", 2, "three coordinates"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n", 4, "three vertices"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\n\nf 1 x 3\n", 5, "not a vertex index"),
    ("v 0 0 0\r\nv 1 0 0\r\nv 0 1 0\r\nf 1 2 /3\r\n", 4, "not a vertex index"),
    # an index may only name a vertex read before the face
    ("v 0 0 0\nv 1 0 0\nf 1 2 3\nv 0 1 0\n", 3, "out of range"),
])
def test_errors_name_the_line(rtc, text, line, what):
    with pytest.raises(rtc.RenderError) as e:
        rtc.load_obj(text)
    assert e.value.code == RT_ERR_IO
    assert f"line {line}:" in str(e.value) and what in str(e.value), str(e.value)


def test_missing_file(rtc, tmp_path):
    with pytest.raises(rtc.RenderError) as e:
        rtc.load_obj(str(tmp_path / "nope.obj"))
    assert e.value.code == RT_ERR_IO and "nope.obj" in str(e.value)


def test_null_arguments(rtc):
    from conftest import PKG
    import os
    lib = C.CDLL(os.path.join(PKG, "rtc_amd", "_lib", "librtc.so"))
    assert lib.rt_mesh_load_obj(None, None) == -1
    assert lib.rt_mesh_load_obj_text(None, None) == -1
    assert lib.rt_mesh_view_get(None, None) == -1
    assert lib.rt_mesh_triangles(None, None, 0, 0, None) == -1
    lib.rt_mesh_free(None)


def _sheared():
    from rtc_amd import world as W
    return W.mat_mul(W.translation(0.3, -0.2, 0.7),
                     W.mat_mul(W.rotation_y(0.6), W.shearing(0.25, 0.0, -0.5, 0.125, 0.0, 0.75)))


@pytest.mark.parametrize("name", ["ico2", "torus", "field"])
def test_triangles_equal_world_triangle_bit_for_bit(rtc, tmp_path, name):
    """rt_mesh_triangles is Triangle::new per face: the descriptors of world.mesh equal those of world.triangle
    on the same vertices, byte for byte; unbaked with a transform they carry its inverse, baked the transformed
    vertices (Matrix * Point in the reference's order) and the identity."""
    from rtc_amd import world as W
    mesh = M.load(rtc, tmp_path, name)
    light = [W.Light((0.0, 5.0, 0.0))]
    by_mesh = W.World(light, W.mesh(mesh)).tables()
    by_tri = W.World(light, M.same_world_by_triangle(mesh)).tables()
    assert len(by_mesh.shapes) == M.TRIANGLES[name]
    assert _bits(by_mesh.shapes) == _bits(by_tri.shapes)
    assert _bits(by_mesh.materials) == _bits(by_tri.materials)

    t = _sheared()
    unbaked = W.World(light, W.mesh(mesh, transform=t)).tables()
    want = W.World(light, [s.set_transformation(t) for s in M.same_world_by_triangle(mesh)]).tables()
    assert _bits(unbaked.shapes) == _bits(want.shapes)

    def mul_point(m, p):  # matrix.rs Mul<Point>: a left fold from 0.0 over (x, y, z, 1)
        out = []
        for r in range(3):
            acc = 0.0
            for c, v in enumerate((p[0], p[1], p[2], 1.0)):
                acc = acc + m[r][c] * v
            out.append(acc)
        return tuple(out)
    v = mesh.vertices
    moved = [W.triangle(mul_point(t, v[a]), mul_point(t, v[b]), mul_point(t, v[c]))
             for a, b, c in mesh.triangles.tolist()]
    baked = W.World(light, W.mesh(mesh, transform=t, bake=True)).tables()
    assert _bits(baked.shapes) == _bits(W.World(light, moved).tables().shapes)
    assert [baked.shapes[0].inverse[i] for i in range(16)] == [1.0 if i % 5 == 0 else 0.0 for i in range(16)]


def test_degenerate_face_is_kept(rtc):
    mesh = rtc.load_obj("v 0 0 0\nv 1 1 1\nv 2 2 2\nv 0 1 0\nf 1 2 3\nf 1 2 4\n")
    d = mesh.shape_descs()
    assert len(d) == 2
    assert all(np.isnan(d[0].normal[q]) for q in range(3)) and all(np.isfinite(d[1].normal[q]) for q in range(3))


def test_oracle_renders_the_obj_icosphere_like_world_triangle(rtc, oracle, tmp_path):
    from rtc_amd import world as W
    mesh = M.load(rtc, tmp_path, "ico2")
    mat = W.Material(color=(0.2, 0.7, 0.4), specular=0.4)
    a = M.world(W.mesh(mesh, mat))
    b = M.world(M.same_world_by_triangle(mesh, mat))
    assert len(a.shapes) == 322
    img_a, st_a = oracle.render(a, a.camera, 2, threads=8)
    img_b, st_b = oracle.render(b, b.camera, 2, threads=8)
    assert np.array_equal(img_a.view(np.uint64), img_b.view(np.uint64)) and st_a == st_b
    # the sphere of triangles is in the picture: the centre pixel differs from the floor-only world's
    bare, _ = oracle.render(M.world([]), a.camera, 2, threads=8)
    assert np.abs(img_a - bare).max() > 0.05
