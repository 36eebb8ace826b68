"""Mesh instances on the host (rtc.h rt_instances_expand and the refusals of
rt_scene_upload_instanced; no GPU): the expansion is the concatenation of
rt_mesh_triangles(..., bake = 0) outputs bit for bit, the ctypes mirrors have
the header's layouts, every malformed list is refused with its own message,
and world.instance means what world.mesh appends.
"""
import ctypes as C
import os
import re

import instance_worlds as I
import mesh_worlds as M
from conftest import ROOT


def _raw(descs):
    return bytes(memoryview(descs).cast("B"))


def _flat(t):
    return [v for row in t for v in row]


def _placements():
    from rtc_amd import world as W
    return [W.translation(1.0, -2.0, 0.5),
            I.chain(W.rotation_y(0.7), W.shearing(0.3, 0.0, 0.0, 0.2, 0.0, 0.0)),
            I.chain(W.translation(0.2, 0.1, 0.0), W.scaling(-0.5, 2.0, 1.25))]


def test_expansion_is_the_concatenation_of_mesh_triangles(rtc, tmp_path):
    from rtc_amd import world as W
    torus, ico = M.load(rtc, tmp_path, "torus"), M.load(rtc, tmp_path, "ico2")
    places = _placements()
    plan = [(torus, 0, places[0], 3), (ico, 1, places[1], 4), (torus, 0, places[2], 5), (ico, 1, None, 6)]
    meshes = [torus.shape_descs(), ico.shape_descs()]
    inst = (rtc.InstanceDesc * len(plan))()
    want = b""
    plain = W.World([], [W.sphere(), W.plane()]).tables().shapes
    want += _raw(plain)
    for k, (mesh, m, place, material) in enumerate(plan):
        inst[k].mesh, inst[k].material = m, material
        inv = W.IDENTITY if place is None else W.inverse(place)
        inst[k].inverse[:] = _flat(inv)
        want += _raw(mesh.shape_descs(None if place is None else _flat(place), False, material))
    tables = rtc.SceneTables(plain, (rtc.MaterialDesc * 7)(), (rtc.PatternDesc * 0)(), (rtc.LightDesc * 0)(),
                             rtc.CameraDesc(), meshes=meshes, instances=inst)
    flat = tables.expanded()
    assert len(flat.shapes) == 2 + 576 + 320 + 576 + 320
    assert _raw(flat.shapes) == want, "rt_instances_expand differs from rt_mesh_triangles(..., bake = 0)"


def test_struct_layouts_match_the_header(rtc):
    hdr = open(os.path.join(ROOT, "include", "rtc.h")).read()
    for name, cls in (("rt_mesh_desc", rtc.MeshDesc), ("rt_instance_desc", rtc.InstanceDesc),
                      ("rt_instance_info", rtc.InstanceInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.sub(r"\[\d+\]", "", f.split()[-1].lstrip("*")) for f in body.split(";") if f.strip()]
        assert fields == [n for n, _ in cls._fields_], name
    assert C.sizeof(rtc.MeshDesc) == 16 and rtc.MeshDesc.n_triangles.offset == 8
    assert C.sizeof(rtc.InstanceDesc) == 136 and rtc.InstanceDesc.inverse.offset == 8
    assert C.sizeof(rtc.InstanceInfo) == 48 and rtc.InstanceInfo.instanced_bytes.offset == 24
    assert rtc.InstanceInfo.build_ms.offset == 40
    for sym in ("rt_scene_upload_instanced", "rt_instances_expand", "rt_scene_instance_info"):
        assert sym in rtc.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, hdr)


def _expand_rc(rtc, shapes, meshes, inst):
    tables = rtc.SceneTables(shapes, (rtc.MaterialDesc * 1)(), (rtc.PatternDesc * 0)(), (rtc.LightDesc * 0)(),
                             rtc.CameraDesc(), meshes=meshes, instances=inst)
    md = tables.mesh_descs()
    out = (rtc.ShapeDesc * (1 << 12))()
    rc = rtc._lib.rt_instances_expand(shapes, len(shapes), md, len(md), inst, len(inst), out)
    return rc, rtc._lib.rt_last_error().decode()


def _one_instance(rtc, mesh=0, material=0):
    inst = (rtc.InstanceDesc * 1)()
    inst[0].mesh, inst[0].material = mesh, material
    inst[0].inverse[:] = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
    return inst


def test_every_refusal_has_its_own_message(rtc):
    none = (rtc.ShapeDesc * 0)()
    octa = rtc.load_obj(I.OCTA)
    good = octa.shape_descs()
    assert _expand_rc(rtc, none, [good], _one_instance(rtc))[0] == rtc.RT_OK
    seen = set()

    def refused(meshes, inst, word):
        rc, why = _expand_rc(rtc, none, meshes, inst)
        assert rc == rtc.RT_ERR_INVALID and word in why, (rc, why)
        assert why not in seen
        seen.add(why)

    not_triangle = octa.shape_descs()
    not_triangle[3].kind = rtc.SHAPE_KINDS["sphere"]
    refused([not_triangle], _one_instance(rtc), "not a triangle")
    moved = octa.shape_descs([1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1])
    refused([moved], _one_instance(rtc), "not the identity")
    refused([(rtc.ShapeDesc * 0)()], _one_instance(rtc), "empty mesh")
    refused([good], _one_instance(rtc, mesh=1), "mesh index out of range")
    field = rtc.load_obj(M.obj_text(*M.height_field(16))).shape_descs()  # 512 triangles
    many = (rtc.InstanceDesc * (1 << 15))()  # 2^15 instances of it: 2^24 shapes
    md = rtc.SceneTables(none, (rtc.MaterialDesc * 1)(), (rtc.PatternDesc * 0)(), (rtc.LightDesc * 0)(),
                         rtc.CameraDesc(), meshes=[field], instances=many).mesh_descs()
    rc = rtc._lib.rt_instances_expand(none, 0, md, 1, many, len(many), None)
    why = rtc._lib.rt_last_error().decode()
    assert rc == rtc.RT_ERR_INVALID and "2^24" in why and why not in seen
    seen.add(why)
    # one fewer fits (the check comes before the output is touched: a null output is then the complaint)
    rc = rtc._lib.rt_instances_expand(none, 0, md, 1, many, len(many) - 1, None)
    assert rc == rtc.RT_ERR_INVALID and "null output" in rtc._lib.rt_last_error().decode()
    # the material index is the upload's to check (the expansion takes no material table); the lists are
    # checked before the context is looked at, so no device is needed
    bad = _one_instance(rtc, material=1)
    mats = (rtc.MaterialDesc * 1)()
    mats[0].pattern = -1
    t = rtc.SceneTables(none, mats, (rtc.PatternDesc * 0)(), (rtc.LightDesc * 0)(), rtc.CameraDesc(), meshes=[good],
                        instances=bad)
    rc = rtc._lib.rt_scene_upload_instanced(None, *t.instanced_args())
    why = rtc._lib.rt_last_error().decode()
    assert rc == rtc.RT_ERR_INVALID and "material index out of range" in why and why not in seen
    t.instances[0].material = 0
    rc = rtc._lib.rt_scene_upload_instanced(None, *t.instanced_args())
    assert rc == rtc.RT_ERR_INVALID and "null context" in rtc._lib.rt_last_error().decode()


def test_world_instance_means_what_world_mesh_appends(rtc, tmp_path):
    from rtc_amd import world as W
    torus, ico = M.load(rtc, tmp_path, "torus"), M.load(rtc, tmp_path, "ico2")
    a, b = W.Material(color=(0.2, 0.4, 0.6)), M.glass()
    places = _placements()
    base = [W.plane(), W.sphere(a, W.translation(0, 1, 0))]
    inst = W.World([], base, [W.instance(torus, a, places[0]), W.instance(ico, b, places[1]),
                              W.instance(torus, b, places[2]), W.instance(ico, a)]).tables()
    assert inst.instanced and len(inst.meshes) == 2 and [i.mesh for i in inst.instances] == [0, 1, 0, 1]
    want = W.World([], base + W.mesh(torus, a, places[0]) + W.mesh(ico, b, places[1]) + W.mesh(torus, b, places[2])
                   + W.mesh(ico, a)).tables()
    got = inst.expanded()
    assert len(got.shapes) == len(want.shapes) == 2 + 2 * 576 + 2 * 320
    skip = rtc.ShapeDesc.material.offset, rtc.ShapeDesc.material.offset + 4  # the material index: compared by value
    for i, (x, y) in enumerate(zip(got.shapes, want.shapes)):
        bx, by = bytes(x), bytes(y)
        assert bx[:skip[0]] + bx[skip[1]:] == by[:skip[0]] + by[skip[1]:], i
        assert bytes(got.materials[x.material]) == bytes(want.materials[y.material]), i
    plain = W.World([], base).tables()
    assert not plain.instanced and plain.expanded() is plain
