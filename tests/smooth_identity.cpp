// CPU checks of the host side of smooth triangles (csrc/instances.hpp
// validate_side / side_index / expand_side over SmoothSide, decide_expanded and
// csrc/shape_identity.hpp with normals), compiled stand-alone by
// tests/test_smooth_cpu.py, with the address and undefined-behaviour sanitizers
// where the compiler has them.  Prints one line per check and "ok".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../ray-tracer-challenge-rs_amd/csrc/instances.hpp"
#include "../ray-tracer-challenge-rs_amd/csrc/rtc_internal.hpp"

using namespace rtc;

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            ++g_failed;                                   \
        }                                                 \
    } while (0)

static rt_shape_desc triangle(double x, double y) {
    rt_shape_desc d;
    std::memset(&d, 0, sizeof d);
    d.kind = RT_SHAPE_TRIANGLE;
    for (int i = 0; i < 16; ++i) d.inverse[i] = i % 5 == 0 ? 1.0 : 0.0;
    d.vertex_1[0] = x, d.vertex_1[1] = y;
    d.edge_1[0] = 1.0;
    d.edge_2[1] = 1.0;
    d.normal[2] = -1.0;
    return d;
}
static std::vector<rt_shape_desc> strip(int n, double y = 0.0) {
    std::vector<rt_shape_desc> out;
    for (int i = 0; i < n; ++i) out.push_back(triangle(2.0 * i, y));
    return out;
}
static rt_smooth_desc smooth(uint32_t list, uint32_t index, double tilt = 0.25) {
    rt_smooth_desc d;
    std::memset(&d, 0, sizeof d);
    d.list = list;
    d.index = index;
    d.normal_1[2] = d.normal_2[2] = d.normal_3[2] = -1.0;
    d.normal_1[0] = -tilt, d.normal_2[0] = tilt, d.normal_3[1] = tilt + index;
    return d;
}
static rt_instance_desc place(uint32_t mesh, int32_t material, double tx) {
    rt_instance_desc d;
    std::memset(&d, 0, sizeof d);
    d.mesh = mesh;
    d.material = material;
    for (int i = 0; i < 16; ++i) d.inverse[i] = i % 5 == 0 ? 1.0 : 0.0;
    d.inverse[3] = -tx;
    return d;
}

int main() {
    std::vector<rt_material_desc> mats(3);
    std::memset(mats.data(), 0, mats.size() * sizeof mats[0]);
    for (auto& m : mats) m.pattern = -1;
    mats[1].ambient = 0.5;  // 0 and 2 are value-equal, 1 differs

    // ---- 1: the refusals, each with its own text
    {
        const std::vector<rt_shape_desc> shapes = strip(3), a = strip(4, 5.0);
        rt_shape_desc sphere = shapes[0];
        sphere.kind = RT_SHAPE_SPHERE;
        const std::vector<rt_shape_desc> mixed = {shapes[0], sphere};
        const rt_mesh_desc meshes[1] = {{a.data(), (uint32_t)a.size(), 0}};
        auto why = [&](const std::vector<rt_shape_desc>& s, std::vector<rt_smooth_desc> list) {
            return inst::validate_side<inst::SmoothSide>(s.data(), (uint32_t)s.size(), meshes, 1, list.data(), (uint32_t)list.size());
        };
        CHECK(why(shapes, {smooth(RT_SMOOTH_SHAPES, 2), smooth(0, 3)}).empty(), "a well-formed list passes");
        CHECK(inst::validate_side<inst::SmoothSide>(shapes.data(), 3, meshes, 1, nullptr, 2).find("null smooth list") != std::string::npos,
              "null list");
        CHECK(why(shapes, {smooth(1, 0)}).find("list index out of range") != std::string::npos, "list index");
        CHECK(why(shapes, {smooth(RT_SMOOTH_SHAPES, 3)}).find("triangle index out of range") != std::string::npos, "index");
        CHECK(why(shapes, {smooth(0, 4)}).find("triangle index out of range") != std::string::npos, "mesh index");
        CHECK(why(mixed, {smooth(RT_SMOOTH_SHAPES, 1)}).find("not a triangle") != std::string::npos, "no triangle");
        CHECK(why(shapes, {smooth(0, 1), smooth(RT_SMOOTH_SHAPES, 1), smooth(0, 1)}).find("named twice") != std::string::npos,
              "twice");
        rt_smooth_desc bad = smooth(0, 0);
        bad.normal_3[2] = NAN;
        CHECK(why(shapes, {bad}).find("not finite") != std::string::npos, "NaN component");
        bad.normal_3[2] = INFINITY;
        CHECK(why(shapes, {bad}).find("not finite") != std::string::npos, "infinite component");
        std::printf("refusals: 9 cases\n");
    }

    // ---- 2: the expansion's list is the concatenation rule, ascending
    {
        const std::vector<rt_shape_desc> shapes = strip(3), a = strip(4, 5.0), b = strip(2, 9.0);
        const rt_mesh_desc meshes[2] = {{a.data(), 4, 0}, {b.data(), 2, 0}};
        const std::vector<rt_instance_desc> in = {place(0, 0, 1.0), place(1, 0, 2.0), place(0, 1, 3.0)};
        const std::vector<rt_smooth_desc> list = {smooth(0, 3), smooth(RT_SMOOTH_SHAPES, 1), smooth(0, 0), smooth(1, 1)};
        const uint32_t n = inst::expand_side<inst::SmoothSide>(3, meshes, 2, in.data(), 3, list.data(), 4, nullptr);
        std::vector<rt_smooth_desc> out(n);
        inst::expand_side<inst::SmoothSide>(3, meshes, 2, in.data(), 3, list.data(), 4, out.data());
        const uint32_t want_index[6] = {1, 3 + 0, 3 + 3, 7 + 1, 9 + 0, 9 + 3};
        const int from[6] = {1, 2, 0, 3, 2, 0};
        CHECK(n == 6, "1 plain + 2 + 1 + 2 entries, got %u", n);
        for (uint32_t i = 0; i < n && i < 6; ++i)
            CHECK(out[i].list == RT_SMOOTH_SHAPES && out[i].index == want_index[i] &&
                      std::memcmp(out[i].normal_1, list[from[i]].normal_1, 9 * sizeof(double)) == 0,
                  "entry %u: world index %u", i, out[i].index);
        std::printf("expansion: %u entries\n", n);
    }

    // ---- 3: identity classes with normals
    {
        // world: t0 smooth, t1 = t0's twin (equal in all fields), t2 = coincident but one component differs,
        // t3 = the flat twin, t4 = another flat twin (equal to t3)
        std::vector<rt_shape_desc> s(5, triangle(0.0, 0.0));
        rt_smooth_desc n0 = smooth(RT_SMOOTH_SHAPES, 0), n1 = smooth(RT_SMOOTH_SHAPES, 1), n2 = smooth(RT_SMOOTH_SHAPES, 2);
        std::memcpy(n1.normal_1, n0.normal_1, 9 * sizeof(double));
        std::memcpy(n2.normal_1, n0.normal_1, 9 * sizeof(double));
        n2.normal_2[1] += 1e-9;
        const std::vector<rt_smooth_desc> list = {n0, n1, n2};
        const inst::SideIndex si = inst::side_index<inst::SmoothSide>(5, nullptr, 0, list.data(), 3);
        std::vector<uint32_t> cls;
        const uint32_t dups = ident::shape_classes(s.data(), 5, mats.data(), nullptr, cls, si.of_plain());
        CHECK(cls == (std::vector<uint32_t>{0, 0, 2, 3, 3}) && dups == 2, "classes %u %u %u %u %u", cls[0], cls[1], cls[2],
              cls[3], cls[4]);
        // -0 and +0 compare equal and hash alike
        rt_smooth_desc z = n0;
        z.index = 1;
        z.normal_1[1] = -0.0;
        const std::vector<rt_smooth_desc> lz = {n0, z};
        const inst::SideIndex sz = inst::side_index<inst::SmoothSide>(5, nullptr, 0, lz.data(), 2);
        ident::shape_classes(s.data(), 2, mats.data(), nullptr, cls, sz.of_plain());
        CHECK(cls[1] == 0, "-0 == +0");
        // without a normal table the old answer: all five one class
        ident::shape_classes(s.data(), 5, mats.data(), nullptr, cls);
        CHECK(cls == (std::vector<uint32_t>{0, 0, 0, 0, 0}), "flat classes unchanged");
        std::printf("classes: 3 cases\n");
    }

    // ---- 4: the instance decisions are the expansion's identity classes
    {
        const std::vector<rt_shape_desc> a = strip(4, 5.0);
        std::vector<rt_shape_desc> b = strip(4, 5.0);  // the same faces as a
        const rt_mesh_desc meshes[3] = {{a.data(), 4, 0}, {b.data(), 4, 0}, {a.data(), 4, 0}};
        // mesh 0 smooth on faces 0 and 2; mesh 1 the same normals but for one component of face 2, and face 0 flat;
        // mesh 2 flat
        rt_smooth_desc m1f2 = smooth(1, 2);
        std::memcpy(m1f2.normal_1, smooth(0, 2).normal_1, 9 * sizeof(double));
        m1f2.normal_1[1] = 0.5;
        const std::vector<rt_smooth_desc> list = {smooth(0, 0), smooth(0, 2), m1f2};
        const inst::SideIndex si = inst::side_index<inst::SmoothSide>(0, meshes, 3, list.data(), 3);
        auto decide = [&](const std::vector<rt_shape_desc>& shapes, const std::vector<rt_instance_desc>& in,
                          const std::vector<rt_smooth_desc>& l) {
            const inst::SideIndex x = inst::side_index<inst::SmoothSide>((uint32_t)shapes.size(), meshes, 3, l.data(), (uint32_t)l.size());
            return inst::decide_expanded(shapes.data(), (uint32_t)shapes.size(), meshes, 3, in.data(), (uint32_t)in.size(),
                                         mats.data(), nullptr, &x);
        };
        auto is = [](const std::vector<char>& got, std::vector<char> want) { return got == want; };
        CHECK(is(decide({}, {place(0, 0, 1.0), place(0, 2, 1.0), place(0, 0, 2.0)}, list), {1, 1, 0}),
              "two instances of one smooth mesh with equal inverse and material are partners");
        // meshes 0 and 1 share the flat faces 1 and 3
        CHECK(is(decide({}, {place(0, 0, 1.0), place(1, 0, 1.0)}, list), {1, 1}), "a common flat face: partners");
        // only faces 0 and 2: mesh 0 smooth, mesh 2 flat, so meshes made of those faces share nothing
        const std::vector<rt_shape_desc> two = {a[0], a[2]};
        const rt_mesh_desc pair[3] = {{two.data(), 2, 0}, {two.data(), 2, 0}, {two.data(), 2, 0}};
        auto decide2 = [&](const std::vector<rt_shape_desc>& shapes, const std::vector<rt_instance_desc>& in,
                           const std::vector<rt_smooth_desc>& l) {
            const inst::SideIndex x = inst::side_index<inst::SmoothSide>((uint32_t)shapes.size(), pair, 3, l.data(), (uint32_t)l.size());
            return inst::decide_expanded(shapes.data(), (uint32_t)shapes.size(), pair, 3, in.data(), (uint32_t)in.size(),
                                         mats.data(), nullptr, &x);
        };
        rt_smooth_desc q1 = smooth(1, 1);
        std::memcpy(q1.normal_1, smooth(0, 1).normal_1, 9 * sizeof(double));
        q1.normal_3[0] = 0.125;  // mesh 1's face 1 differs from mesh 0's in one component
        rt_smooth_desc q0 = smooth(1, 0);
        q0.normal_1[0] = 7.0;
        const std::vector<rt_smooth_desc> l2 = {smooth(0, 0), smooth(0, 1), q0, q1};
        CHECK(is(decide2({}, {place(0, 0, 1.0), place(1, 0, 1.0)}, l2), {0, 0}),
              "coincident faces that differ in one normal component: no partners");
        CHECK(is(decide2({}, {place(0, 0, 1.0), place(2, 0, 1.0)}, l2), {0, 0}), "a smooth and a flat twin: no partners");
        // a plain triangle: equal to the virtual one only with the same normals
        rt_shape_desc plain = two[1];
        const rt_instance_desc at = place(0, 0, 1.0);
        std::memcpy(plain.inverse, at.inverse, sizeof plain.inverse);
        std::vector<rt_smooth_desc> l3 = l2;
        CHECK(is(decide2({plain}, {at}, l3), {0}), "a flat plain triangle against a smooth virtual one: none");
        rt_smooth_desc ps = smooth(RT_SMOOTH_SHAPES, 0);
        std::memcpy(ps.normal_1, smooth(0, 1).normal_1, 9 * sizeof(double));
        l3.push_back(ps);
        CHECK(is(decide2({plain}, {at}, l3), {1}), "a smooth plain triangle with the same normals: partner");
        l3.back().normal_2[2] = 3.0;
        CHECK(is(decide2({plain}, {at}, l3), {0}), "... with one other component: none");

        // agreement with shape_identity's classes of the expansion
        const std::vector<rt_instance_desc> in = {place(0, 0, 1.0), place(1, 0, 1.0), place(2, 2, 1.0), place(0, 1, 1.0),
                                                  place(1, 0, 2.0)};
        const std::vector<uint32_t> bases = inst::world_bases(0, pair, in.data(), (uint32_t)in.size());
        std::vector<rt_shape_desc> flat(bases.back());
        inst::expand(nullptr, 0, pair, in.data(), (uint32_t)in.size(), flat.data());
        const uint32_t n = inst::expand_side<inst::SmoothSide>(0, pair, 3, in.data(), (uint32_t)in.size(), l2.data(), (uint32_t)l2.size(), nullptr);
        std::vector<rt_smooth_desc> fl(n);
        inst::expand_side<inst::SmoothSide>(0, pair, 3, in.data(), (uint32_t)in.size(), l2.data(), (uint32_t)l2.size(), fl.data());
        const inst::SideIndex fx = inst::side_index<inst::SmoothSide>((uint32_t)flat.size(), nullptr, 0, fl.data(), n);
        std::vector<uint32_t> cls;
        ident::shape_classes(flat.data(), (uint32_t)flat.size(), mats.data(), nullptr, cls, fx.of_plain());
        std::vector<char> want(in.size(), 0);
        for (uint32_t i = 0; i < flat.size(); ++i)
            if (cls[i] != i)
                for (uint32_t w : {i, cls[i]})
                    want[instance_of_world([&](int k) { return (int)bases[k]; }, (int)in.size(), (int)w)] = 1;
        CHECK(is(decide2({}, in, l2), want) && is(want, {0, 0, 0, 0, 0}), "the decisions are the expansion's classes (none equal)");
        const std::vector<rt_instance_desc> in2 = {place(0, 0, 1.0), place(2, 2, 1.0), place(0, 2, 1.0), place(2, 0, 1.0)};
        CHECK(is(decide2({}, in2, l2), {1, 1, 1, 1}), "smooth with smooth, flat with flat");
        (void)si;
        std::printf("instance decisions: 9 cases\n");
    }

    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
