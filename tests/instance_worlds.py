"""Instanced worlds for the instance tests: meshes of tests/mesh_worlds.py and
two hand-written ones, placed with world.instance over mesh_worlds.world's
plane, sphere and two lights.  Every world is (tables, depth); the flat world
it means is tables.expanded().
"""
import mesh_worlds as M

# one triangle, and an octahedron (8 triangles), written by hand
ONE = "v -0.75 0 0.25\nv 0.75 0 0\nv 0 1.25 -0.25\nf 1 2 3\n"
OCTA = ("v 1 0 0\nv -1 0 0\nv 0 1 0\nv 0 -1 0\nv 0 0 1\nv 0 0 -1\n"
        "f 1 3 5\nf 3 2 5\nf 2 4 5\nf 4 1 5\nf 3 1 6\nf 2 3 6\nf 4 2 6\nf 1 4 6\n")
OCTA_REPEATED = OCTA + "f 1 3 5\n"  # its first face twice: 9 triangles, two of them value-equal

WORLDS = ["three_tori", "nested_glass", "coincident", "small", "beside_plain"]
VALUE_EQUAL = {"twins": 2, "repeated": 1}  # world -> instances uploaded expanded


def world(plain, instances):
    """mesh_worlds.world's floor, ball and lights, then `plain` shapes; `instances` follow them in world order."""
    from rtc_amd import world as W
    floor = W.plane(W.Material(pattern=W.checker_pattern((0.8, 0.8, 0.8), (0.3, 0.3, 0.35)), specular=0.0),
                    transform=W.translation(0, -1.3, 0))
    ball = W.sphere(W.Material(color=(0.9, 0.3, 0.2)), transform=W.mat_mul(W.translation(1.9, -0.7, 0.6),
                                                                         W.scaling(0.6, 0.6, 0.6)))
    lights = [W.Light((-5.0, 6.0, -5.0), (0.7, 0.7, 0.7)), W.Light((4.0, 5.0, -2.0), (0.4, 0.4, 0.35))]
    return W.World(lights, [floor, ball] + list(plain), list(instances)).tables(M.camera())


def other_glass():
    from rtc_amd import world as W
    return W.Material(color=(0.3, 0.1, 0.1), diffuse=0.2, ambient=0.05, specular=0.6, shininess=200.0,
                      reflectiveness=0.2, transparency=0.9, refractive_index=1.2)


def chain(*ms):
    from rtc_amd import world as W
    out = ms[0]
    for m in ms[1:]:
        out = W.mat_mul(out, m)
    return out


def build_world(rtc, tmp_path, key):
    from rtc_amd import world as W
    get = lambda name: M.load(rtc, tmp_path, name)  # noqa: E731
    opaque = W.Material(color=(0.25, 0.6, 0.85), specular=0.5, shininess=60.0)
    yellow = W.Material(color=(0.9, 0.8, 0.1), diffuse=0.7, specular=0.1)
    if key == "three_tori":  # opaque: the direct kernel; a translation, rotation x shear, a mirrored non-uniform scale
        t = get("torus")
        return world([], [
            W.instance(t, opaque, W.translation(-1.2, 0.2, 0.4)),
            W.instance(t, yellow, chain(W.translation(0.9, 0.5, 1.0), W.rotation_y(0.7),
                                        W.shearing(0.3, 0.0, 0.0, 0.2, 0.0, 0.0), W.scaling(0.7, 0.7, 0.7))),
            W.instance(t, opaque, chain(W.translation(0.2, -0.6, -0.9), W.scaling(-0.5, 0.8, 0.35)))]), 3
    if key == "nested_glass":  # the pool kernel; the containers walk nests across instances
        s = get("ico2")
        return world([], [W.instance(s, M.glass(), W.translation(0, 0.35, 0)),
                          W.instance(s, other_glass(), chain(W.translation(0, 0.35, 0), W.scaling(0.5, 0.5, 0.5)))]), 4
    if key == "coincident":  # one inverse, two materials: equal t everywhere, the lower world index wins
        t, place = get("torus"), chain(W.translation(0, 0.2, 0), W.rotation_x(0.5))
        return world([], [W.instance(t, opaque, place), W.instance(t, yellow, place)]), 3
    if key == "small":  # meshes of 1 and of 8 triangles
        one, octa = rtc.load_obj(ONE), rtc.load_obj(OCTA)
        return world([], [W.instance(one, yellow, W.translation(-1.4, -0.4, 0.3)),
                          W.instance(octa, opaque, chain(W.translation(0.3, 0.1, 0.2), W.rotation_z(0.4))),
                          W.instance(octa, M.glass(), chain(W.translation(-0.5, 0.3, -1.6), W.scaling(0.4, 0.6, 0.4))),
                          W.instance(one, opaque, chain(W.translation(1.0, 0.6, 1.5), W.rotation_y(2.0)))]), 4
    if key == "beside_plain":  # 512 plain mesh triangles (a tree over the plain run) and an instance
        return world(W.mesh(get("field"), opaque, transform=W.translation(0, -0.9, 0.5), bake=True),
                     [W.instance(get("ico2"), yellow, chain(W.translation(-0.3, 0.6, 0.2), W.scaling(0.8, 0.6, 0.8)))]), 3
    if key == "twins":  # two glass instances equal in inverse and material: every triangle has a value-equal partner
        s, g = get("ico2"), M.glass()
        return world([], [W.instance(s, g, W.translation(0, 0.35, 0)), W.instance(s, g, W.translation(0, 0.35, 0))]), 4
    if key == "repeated":  # a mesh with a repeated face (expanded) next to an instance of a sound mesh (walked)
        return world([], [W.instance(rtc.load_obj(OCTA), other_glass(), W.translation(1.0, 0.2, -0.8)),
                          W.instance(rtc.load_obj(OCTA_REPEATED), M.glass(), chain(W.translation(-0.6, 0.3, 0.2),
                                                                                 W.rotation_y(0.3)))]), 4
    raise KeyError(key)
