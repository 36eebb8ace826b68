// CPU checks of the host side of mesh instances (csrc/instances.hpp and the
// per-hit lookup of csrc/rtc_internal.hpp), compiled stand-alone by
// tests/test_instances_index.py.  Prints one line per check and "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
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

static rt_shape_desc triangle(const double a[3], const double b[3], const double c[3]) {
    rt_shape_desc d;
    std::memset(&d, 0, sizeof d);
    d.kind = RT_SHAPE_TRIANGLE;
    for (int i = 0; i < 16; ++i) d.inverse[i] = i % 5 == 0 ? 1.0 : 0.0;
    for (int q = 0; q < 3; ++q) {
        d.vertex_1[q] = a[q];
        d.edge_1[q] = b[q] - a[q];
        d.edge_2[q] = c[q] - a[q];
    }
    d.normal[1] = 1.0;
    return d;
}

// a height field of nx x nz cells, two triangles each
static std::vector<rt_shape_desc> field(int nx, int nz, double lift = 0.0) {
    std::vector<rt_shape_desc> out;
    auto h = [&](int i, int j) { return lift + 0.125 * ((3 * i + 5 * j) % 4); };
    for (int j = 0; j < nz; ++j)
        for (int i = 0; i < nx; ++i) {
            const double a[3] = {i * 0.25, h(i, j), j * 0.25}, b[3] = {(i + 1) * 0.25, h(i + 1, j), j * 0.25};
            const double c[3] = {i * 0.25, h(i, j + 1), (j + 1) * 0.25};
            const double e[3] = {(i + 1) * 0.25, h(i + 1, j + 1), (j + 1) * 0.25};
            out.push_back(triangle(a, c, b));
            out.push_back(triangle(b, c, e));
        }
    return out;
}

static rt_instance_desc place(uint32_t mesh, int32_t material, const hm::M4& forward) {
    rt_instance_desc d;
    std::memset(&d, 0, sizeof d);
    d.mesh = mesh;
    d.material = material;
    const hm::M4 inv = hm::inverse(forward);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) d.inverse[4 * i + j] = inv.m[i][j];
    return d;
}

static hm::M4 rotation_shear() {  // rotation_y(0.7) * shearing(0.3, 0, 0, 0.2, 0, 0), moved
    hm::M4 r = hm::identity(), s = hm::identity(), t = hm::identity();
    r.m[0][0] = std::cos(0.7), r.m[0][2] = std::sin(0.7), r.m[2][0] = -std::sin(0.7), r.m[2][2] = std::cos(0.7);
    s.m[0][1] = 0.3, s.m[1][2] = 0.2;
    t.m[0][3] = 3.0, t.m[1][3] = -1.0, t.m[2][3] = 40.0;
    return hm::mul(t, hm::mul(r, s));
}
static hm::M4 mirrored_scale() {  // scaling(-0.5, 7, 0.02), moved
    hm::M4 m = hm::identity();
    m.m[0][0] = -0.5, m.m[1][1] = 7.0, m.m[2][2] = 0.02;
    m.m[0][3] = -20.0, m.m[1][3] = 0.5, m.m[2][3] = 2.0;
    return m;
}

// ---- 1: world index <-> (instance, local)
static void check_index_maps() {
    const std::vector<rt_shape_desc> a = field(4, 4), b = field(1, 1), c = field(3, 5);
    const rt_mesh_desc meshes[3] = {{a.data(), (uint32_t)a.size(), 0}, {b.data(), (uint32_t)b.size(), 0},
                                    {c.data(), (uint32_t)c.size(), 0}};
    std::vector<rt_instance_desc> inst;
    const uint32_t which[] = {0, 1, 1, 2, 0, 1, 2, 2, 0};
    for (uint32_t m : which) inst.push_back(place(m, 0, hm::identity()));
    const uint32_t ns = 7, n = (uint32_t)inst.size();
    const std::vector<uint32_t> bases = inst::world_bases(ns, meshes, inst.data(), n);
    CHECK(bases[0] == ns, "the first instance starts after the shapes");
    auto base = [&](int i) { return (int)bases[i]; };
    uint32_t w = ns;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t nt = meshes[inst[k].mesh].n_triangles;
        CHECK(bases[k] == w, "base of instance %u", k);
        for (uint32_t j = 0; j < nt; ++j, ++w) {  // every triangle, the first and the last of each instance among them
            const int got = instance_of_world(base, (int)n, (int)w);
            CHECK(got == (int)k && w - bases[got] == j, "world %u -> instance %d local %u, want %u %u", w, got,
                  w - bases[got], k, j);
        }
    }
    CHECK(bases[n] == w, "the world's size");
    CHECK(instance_of_world(base, 1, (int)ns) == 0 && instance_of_world(base, 1, (int)ns + 31) == 0, "one instance");
    // the expansion has the same indices: entry w is triangle j of instance k, under k's inverse and material
    std::vector<rt_shape_desc> shapes(ns, a[0]), flat(w);
    for (uint32_t k = 0; k < n; ++k) inst[k].material = (int32_t)(10 + k);
    inst::expand(shapes.data(), ns, meshes, inst.data(), n, flat.data());
    for (uint32_t k = 0; k < n; ++k) {
        const rt_mesh_desc& m = meshes[inst[k].mesh];
        for (uint32_t j : {0u, m.n_triangles - 1}) {
            const rt_shape_desc& d = flat[bases[k] + j];
            CHECK(d.material == (int32_t)(10 + k) && inst::geometry_eq(d, m.triangles[j]) &&
                      std::memcmp(d.inverse, inst[k].inverse, sizeof d.inverse) == 0,
                  "expansion entry of instance %u local %u", k, j);
        }
    }
    std::printf("index maps: %u instances, %u world indices\n", n, w);
}

// ---- 2, 3: a mesh's plan
template <typename R>
static bool holds(const tri::Ball& outer, const tri::Ball& inner) {  // as the kernel holds them: centre and r^2 in R
    R o[4], i[4];
    tri::cast_ball<R>(outer, o);
    tri::cast_ball<R>(inner, i);
    const double dx = (double)i[0] - o[0], dy = (double)i[1] - o[1], dz = (double)i[2] - o[2];
    return std::sqrt(dx * dx + dy * dy + dz * dz) + std::sqrt((double)i[3]) <= std::sqrt((double)o[3]);
}

static void check_mesh_plan(const char* name, std::vector<rt_shape_desc> tris, uint32_t unbounded) {
    for (uint32_t u = 0; u < unbounded; ++u) tris[3 * u + 1].vertex_1[0] = INFINITY;  // no finite ball: the flat run
    const rt_mesh_desc mesh = {tris.data(), (uint32_t)tris.size(), 0};
    const inst::MeshPlan p = inst::plan_mesh(mesh, true);
    const uint32_t n = mesh.n_triangles;
    CHECK(p.order.size() == n && p.pos.size() == n && p.in_tree == n - unbounded, "%s: sizes", name);
    std::vector<char> seen(n, 0);
    for (uint32_t at = 0; at < n; ++at) {
        CHECK(p.order[at] < n && !seen[p.order[at]], "%s: position %u repeats a record", name, at);
        seen[p.order[at]] = 1;
        CHECK(p.pos[p.order[at]] == at, "%s: local-to-position table at %u", name, at);
        CHECK((at < p.in_tree) == (p.balls[p.order[at]].r >= 0.0), "%s: bounded records come first", name);
    }
    // the table against the tree's order: leaf runs cover [0, in_tree) in order, and a record's position is its leaf's
    uint32_t next = 0;
    for (size_t i = 0; i < p.tree.nodes.size(); ++i) {
        const tri::Node& nd = p.tree.nodes[i];
        if (!nd.count) continue;
        CHECK((uint32_t)nd.first == next, "%s: leaf %zu starts at %d, want %u", name, i, nd.first, next);
        next += nd.count;
    }
    CHECK(next == p.in_tree, "%s: leaves cover the bounded records", name);
    // every node's ball holds the balls of the records below it, in f64 and f32
    for (size_t i = 0; i < p.tree.nodes.size(); ++i) {
        const tri::Node& nd = p.tree.nodes[i];
        for (size_t j = i; j < (size_t)nd.skip; ++j) {
            const tri::Node& leaf = p.tree.nodes[j];
            for (int32_t at = leaf.first; at < leaf.first + leaf.count; ++at) {
                const tri::Ball& b = p.balls[p.order[at]];
                CHECK(holds<double>(nd.ball, b), "%s: node %zu misses record %d (f64)", name, i, at);
                CHECK(holds<float>(nd.ball, b), "%s: node %zu misses record %d (f32)", name, i, at);
            }
        }
    }
    const inst::MeshPlan flat = inst::plan_mesh(mesh, false);
    CHECK(flat.tree.nodes.empty() && flat.in_tree == 0 && flat.order.size() == n, "%s: no cull, no tree", name);
    std::printf("%s: %u records, %zu nodes, depth %u, %u in the flat run\n", name, n, p.tree.nodes.size(), p.tree.depth,
                n - p.in_tree);
}

// ---- 4: the instance's world ball
template <typename R>
static void check_instance_ball(const char* name, const hm::M4& forward) {
    const std::vector<rt_shape_desc> tris = field(6, 5, 0.5);
    const rt_mesh_desc mesh = {tris.data(), (uint32_t)tris.size(), 0};
    const inst::MeshPlan p = inst::plan_mesh(mesh, true);
    const tri::Ball root = p.tree.nodes[0].ball;
    const rt_instance_desc d = place(0, 0, forward);
    tri::Ball wb;
    CHECK(inst::instance_ball(root, d.inverse, &wb), "%s: a ball", name);
    R c[4];
    tri::cast_ball<R>(wb, c);
    std::mt19937_64 rng(11);
    std::normal_distribution<double> g;
    double worst = 0.0;
    for (int s = 0; s < 20000; ++s) {  // points of the root ball's surface, through the forward matrix
        double v[3] = {g(rng), g(rng), g(rng)};
        const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        double q[3], img[3];
        for (int k = 0; k < 3; ++k) q[k] = root.c[k] + root.r * v[k] / len;
        hm::mul_point(forward, q, img);
        const double dx = img[0] - c[0], dy = img[1] - c[1], dz = img[2] - c[2];
        worst = std::max(worst, (dx * dx + dy * dy + dz * dz) / (double)c[3]);
    }
    CHECK(worst <= 1.0, "%s: a point of the root ball's image lies outside the instance ball (%g)", name, worst);
    hm::M4 singular = forward;
    for (int j = 0; j < 4; ++j) singular.m[1][j] = 0.0;
    rt_instance_desc bad = d;
    for (int i = 0; i < 16; ++i) bad.inverse[i] = singular.m[i / 4][i % 4];
    CHECK(!inst::instance_ball(root, bad.inverse, &wb), "%s: a singular matrix has no ball", name);
    std::printf("%s (%s): |image - c|^2 / r^2 at most %.4f\n", name, sizeof(R) == 4 ? "f32" : "f64", worst);
}

// ---- 5: identity decisions
static void check_identity() {
    std::vector<rt_material_desc> mats(3);
    std::memset(mats.data(), 0, mats.size() * sizeof mats[0]);
    for (auto& m : mats) m.pattern = -1;
    mats[1].ambient = 0.5;  // 0 and 2 are value-equal, 1 differs
    const std::vector<rt_shape_desc> a = field(3, 3), b = field(2, 2, 9.0);
    std::vector<rt_shape_desc> rep = field(2, 2, 5.0);
    rep.push_back(rep[3]);  // a repeated face
    const rt_mesh_desc meshes[3] = {{a.data(), (uint32_t)a.size(), 0}, {b.data(), (uint32_t)b.size(), 0},
                                    {rep.data(), (uint32_t)rep.size(), 0}};
    const hm::M4 t1 = rotation_shear(), t2 = mirrored_scale();
    auto decide = [&](const std::vector<rt_shape_desc>& shapes, const std::vector<rt_instance_desc>& in) {
        return inst::decide_expanded(shapes.data(), (uint32_t)shapes.size(), meshes, 3, in.data(), (uint32_t)in.size(),
                                     mats.data(), nullptr);
    };
    auto is = [](const std::vector<char>& got, std::vector<char> want) { return got == want; };
    CHECK(is(decide({}, {place(0, 0, t1), place(0, 2, t1), place(0, 0, t2)}), {1, 1, 0}),
          "equal inverse, value-equal materials: partners");
    CHECK(is(decide({}, {place(0, 0, t1), place(0, 1, t1)}), {0, 0}), "equal inverse, different materials: none");
    CHECK(is(decide({}, {place(0, 0, t1), place(1, 0, t1)}), {0, 0}), "equal inverse and material, no common face: none");
    CHECK(is(decide({}, {place(2, 0, t1), place(0, 0, t2)}), {1, 0}), "a repeated face: its instances only");
    rt_shape_desc plain = a[5];
    const rt_instance_desc at = place(0, 2, t1);
    std::memcpy(plain.inverse, at.inverse, sizeof plain.inverse);
    plain.material = 0;
    CHECK(is(decide({plain}, {place(1, 0, t1), at, place(0, 0, t2)}), {0, 1, 0}), "a plain triangle equal to a virtual one");
    plain.material = 1;
    CHECK(is(decide({plain}, {at}), {0}), "... of another material: none");
    plain.material = 0;
    plain.vertex_1[1] += 1.0;
    CHECK(is(decide({plain}, {at}), {0}), "... of other geometry: none");
    rt_instance_desc nan = place(0, 0, t1);
    nan.inverse[3] = NAN;
    CHECK(is(decide({}, {nan, nan}), {0, 0}), "an inverse with a NaN equals nothing");
    // the decisions are shape_identity's: classes of the expansion say the same
    const std::vector<rt_instance_desc> in = {place(0, 0, t1), place(1, 0, t1), place(0, 2, t1), place(2, 1, t2)};
    const std::vector<uint32_t> bases = inst::world_bases(0, meshes, in.data(), (uint32_t)in.size());
    std::vector<rt_shape_desc> flat(bases.back());
    inst::expand(nullptr, 0, meshes, in.data(), (uint32_t)in.size(), flat.data());
    std::vector<uint32_t> cls;
    ident::shape_classes(flat.data(), (uint32_t)flat.size(), mats.data(), nullptr, cls);
    std::vector<char> want(in.size(), 0);
    for (uint32_t i = 0; i < flat.size(); ++i)
        if (cls[i] != i)
            for (uint32_t w : {i, cls[i]})
                want[instance_of_world([&](int k) { return (int)bases[k]; }, (int)in.size(), (int)w)] = 1;
    CHECK(is(decide({}, in), want) && is(want, {1, 0, 1, 1}), "the decisions are the expansion's identity classes");
    std::printf("identity: 9 cases\n");
}

int main() {
    check_index_maps();
    check_mesh_plan("field 16x16", field(16, 16), 0);
    check_mesh_plan("field 5x3, 2 unbounded", field(5, 3), 2);
    check_mesh_plan("one triangle", field(1, 1), 0);
    check_instance_ball<double>("rotation x shear", rotation_shear());
    check_instance_ball<float>("rotation x shear", rotation_shear());
    check_instance_ball<double>("mirrored non-uniform scale", mirrored_scale());
    check_instance_ball<float>("mirrored non-uniform scale", mirrored_scale());
    check_identity();
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
