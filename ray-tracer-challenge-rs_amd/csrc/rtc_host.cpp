// rtc_host.cpp — the C-ABI of include/rtc.h: context, world flattening and
// upload, launch of the gfx950 kernels, counters.
//
// Boundary it replaces: Camera::render / render_parallel
// (camera.rs:79-112) borrow `&World` and return an owned Canvas; here the
// caller hands the World as POD tables once (rt_scene_upload) and gets the
// canvas written into its own buffer per frame (rt_render / rt_render_device).
// There is no CPU fallback: without a HIP device every call that computes
// fails with RT_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rtc.h"
#include "flop_model.hpp"
#include "host_math.hpp"
#include "debug_knobs.hpp"
#include "launch_terms.hpp"
#include "cull_tables.hpp"
#include "kernel_id.hpp"
#include "primary_rect.hpp"
#include "rtc_context.hpp"
#include "rtc_internal.hpp"
#include "shape_identity.hpp"
#include "tri_tree.hpp"
#include "instances.hpp"

namespace rtc {

// The two entry points every build of the tracer kernels (rtc_kernels.hip, RTC_VARIANT) defines in its own
// namespace: the launch of the kernel a KernelId names (`extra`: a ray batch's RayBatchArg, a lens frame's
// LensParams<R>, else unread) and its occupancy.  A build answers hipErrorInvalidValue for a kernel it does not hold.
#define RTC_KERNEL_LAUNCHERS                                                                                  \
    template <typename R>                                                                                     \
    hipError_t launch_kernel(KernelId id, const LaunchParams<R>& P, const void* extra, uint32_t grid, size_t dyn_lds, \
                             hipStream_t stream);                                                             \
    template <typename R>                                                                                     \
    hipError_t kernel_occupancy(KernelId id, size_t dyn_lds, int* blocks_per_cu);
RTC_KERNEL_LAUNCHERS                          // rtc_kernels*.o: the plain build
namespace instanced { RTC_KERNEL_LAUNCHERS }  // rtc_kernels_inst*.o: with the instance level, for worlds with mesh instances
namespace textured { RTC_KERNEL_LAUNCHERS }   // rtc_kernels_tex*.o: the instance build plus the texture code
namespace area { RTC_KERNEL_LAUNCHERS }       // rtc_kernels_area*.o: the texture build plus the area lights' sample loop
namespace mapped { RTC_KERNEL_LAUNCHERS }     // rtc_kernels_map*.o: the area build plus the texture maps of an image pattern
namespace moving { RTC_KERNEL_LAUNCHERS }     // rtc_kernels_motion*.o: the map build plus a time per ray and the shutter frame kernels; `extra` is a MotionLaunch
namespace sp { RTC_KERNEL_LAUNCHERS }         // rtc_kernels_sp.o: the f32 frame pool kernel for worlds of spheres and planes only
#undef RTC_KERNEL_LAUNCHERS
constexpr uint32_t kKindsSp = (1u << RT_SHAPE_SPHERE) | (1u << RT_SHAPE_PLANE);

// The launchers of each build, by KernelBuild: the one place that maps a world's stored build
// (rt_context::kernel_build) to kernels.
template <typename R>
struct Launchers {
    decltype(&launch_kernel<R>) launch_kernel;
    decltype(&kernel_occupancy<R>) kernel_occupancy;
};
template <typename R>
constexpr Launchers<R> kLaunchers[] = {{launch_kernel<R>, kernel_occupancy<R>},
                                       {instanced::launch_kernel<R>, instanced::kernel_occupancy<R>},
                                       {textured::launch_kernel<R>, textured::kernel_occupancy<R>},
                                       {area::launch_kernel<R>, area::kernel_occupancy<R>},
                                       {mapped::launch_kernel<R>, mapped::kernel_occupancy<R>},
                                       {moving::launch_kernel<R>, moving::kernel_occupancy<R>}};
template <typename R>
const Launchers<R>& launchers(const rt_context* ctx) {
    return kLaunchers<R>[(uint32_t)ctx->kernel_build];
}

hipError_t launch_order_tiles(uint32_t* cost, uint32_t* order, uint32_t n, uint32_t* n_items, float split_per_cost,
                              uint32_t max_split_log2, float urgent_per_cost, uint32_t graded, uint32_t min_split_log2,
                              hipStream_t stream);
template <typename R>
hipError_t launch_debug_shape(const ShapeRec<R>* shapes, int slot, int kind, uint32_t mode, uint32_t world_space,
                              const double* in, uint32_t n, double* out, hipStream_t stream);

namespace {
thread_local std::string g_error;
}

int set_error(int code, const std::string& msg) {
    g_error = msg;
    return code;
}

// World-space bounding sphere of a shape's intersection set, for the
// kernels' wave-level cull (wave_may_hit).  Acceleration only: a shape is
// skipped for a wave only when no lane's ray can meet this sphere at t >= 0,
// so it is padded well beyond the f32/f64 rounding of the local-space tests.
// Returns radius -1 for unbounded shapes (planes, open-ended cylinders,
// every cone) and for transforms whose forward matrix is not finite.
// Cones: a ray parallel to the side (|a| < EPSILON, |b| > EPSILON) gets the
// single root -c / 2b with no y-range test (cone.rs:97-99), anywhere on the
// infinite double cone, so no ball around the finite cone bounds a cone's
// entries (a random world's grazing ray found it: tests/test_gpu_random_worlds.py).
void bounding_sphere(const rt_shape_desc& d, double out[4]) {
    out[0] = out[1] = out[2] = 0.0;
    out[3] = -1.0;
    double c[3] = {0.0, 0.0, 0.0}, r = 0.0;
    const double lo = d.minimum, hi = d.maximum;
    switch (d.kind) {
        case RT_SHAPE_SPHERE: r = 1.0; break;
        case RT_SHAPE_CUBE: r = std::sqrt(3.0); break;
        case RT_SHAPE_CYLINDER: {
            if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi)) return;
            const double half = 0.5 * (hi - lo);
            c[1] = 0.5 * (lo + hi);
            r = std::sqrt(1.0 + half * half);
            break;
        }
        case RT_SHAPE_TRIANGLE: {
            double p[3][3];
            for (int q = 0; q < 3; ++q) {
                p[0][q] = d.vertex_1[q];
                p[1][q] = d.vertex_1[q] + d.edge_1[q];
                p[2][q] = d.vertex_1[q] + d.edge_2[q];
            }
            for (int q = 0; q < 3; ++q) c[q] = (p[0][q] + p[1][q] + p[2][q]) / 3.0;
            for (auto& v : p)
                r = std::max(r, std::sqrt((v[0] - c[0]) * (v[0] - c[0]) + (v[1] - c[1]) * (v[1] - c[1]) +
                                          (v[2] - c[2]) * (v[2] - c[2])));
            break;
        }
        default: return;  // plane, cone
    }
    hm::M4 inv;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) inv.m[i][j] = d.inverse[4 * i + j];
    const hm::M4 f = hm::inverse(inv);
    // spectral norm of the linear part <= sqrt(max abs row sum of F^T F)
    double ftf[3][3] = {}, sigma2 = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) ftf[i][j] += f.m[k][i] * f.m[k][j];
    for (auto& row : ftf) sigma2 = std::max(sigma2, std::fabs(row[0]) + std::fabs(row[1]) + std::fabs(row[2]));
    double wc[3];
    for (int i = 0; i < 3; ++i) wc[i] = f.m[i][0] * c[0] + f.m[i][1] * c[1] + f.m[i][2] * c[2] + f.m[i][3];
    const double wr = r * std::sqrt(sigma2);
    const double scale = std::fabs(wc[0]) + std::fabs(wc[1]) + std::fabs(wc[2]) + wr;
    const double pad = 1e-3 * wr + 1e-4 * scale + 1e-4;
    if (!std::isfinite(wc[0]) || !std::isfinite(wc[1]) || !std::isfinite(wc[2]) || !std::isfinite(wr) ||
        wr + pad > 1e18)
        return;
    for (int i = 0; i < 3; ++i) out[i] = wc[i];
    out[3] = wr + pad;
}

// A sphere whose transformation is a similarity (rotation, uniform scale,
// translation): its world centre and radius^2, for the f32 kernels' roots in
// world space (rtc_internal.hpp kShapeSimilar, rtc_kernels.hip sphere_world).
// The linear part L of the forward transformation must satisfy
// L^T L = s^2 I to 1e-9 of s^2, far below the f32 rounding the kernels work
// at; shadow_puppets.yaml's backdrop (scaled 0.01 in z) keeps the
// object-space test.
bool similar_sphere(const rt_shape_desc& d, double centre[3], double* r2) {
    if (d.kind != RT_SHAPE_SPHERE) return false;
    hm::M4 inv;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) inv.m[i][j] = d.inverse[4 * i + j];
    if (inv.m[3][0] != 0.0 || inv.m[3][1] != 0.0 || inv.m[3][2] != 0.0 || inv.m[3][3] != 1.0) return false;
    const hm::M4 f = hm::inverse(inv);
    double g[3][3] = {};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) g[i][j] += f.m[k][i] * f.m[k][j];
    const double s2 = (g[0][0] + g[1][1] + g[2][2]) / 3.0;
    if (!(s2 > 0.0) || !std::isfinite(s2)) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (!(std::fabs(g[i][j] - (i == j ? s2 : 0.0)) <= 1e-9 * s2)) return false;
    for (int i = 0; i < 3; ++i) {
        centre[i] = f.m[i][3];
        if (!std::isfinite(centre[i])) return false;
    }
    *r2 = s2;
    return true;
}

// A cube whose transformation has a diagonal linear part (rtc_internal.hpp
// kShapeAxisAligned): per axis the world coordinates of its object -1 and +1
// faces, the world |d| below which the axis counts as parallel (EPSILON over
// the axis's scale: the object direction is s d) and the scale's sign, for
// the f32 kernels' world-space slab test.  Off-diagonal terms within 1e-12 of
// the diagonal's size count as zero (far below f32 rounding).
bool axis_aligned_cube(const rt_shape_desc& d, double face_lo[3], double face_hi[3], double eps[3], double sgn[3]) {
    if (d.kind != RT_SHAPE_CUBE) return false;
    const double* m = d.inverse;  // rows of the inverse (row-major 4x4)
    if (m[12] != 0.0 || m[13] != 0.0 || m[14] != 0.0 || m[15] != 1.0) return false;
    double dmax = 0.0;
    for (int i = 0; i < 3; ++i) dmax = std::max(dmax, std::fabs(m[4 * i + i]));
    if (!(dmax > 0.0) || !std::isfinite(dmax)) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (i != j && !(std::fabs(m[4 * i + j]) <= 1e-12 * dmax)) return false;
    for (int i = 0; i < 3; ++i) {
        const double sc = m[4 * i + i], t = m[4 * i + 3];
        if (sc == 0.0 || !std::isfinite(sc) || !std::isfinite(t)) return false;
        face_lo[i] = (-1.0 - t) / sc;
        face_hi[i] = (1.0 - t) / sc;
        eps[i] = 0.00000008 / std::fabs(sc);  // consts.rs EPSILON
        sgn[i] = sc > 0.0 ? 1.0 : -1.0;
    }
    return true;
}

// Device table order: by kind, then by identity class (the world index of
// the class's first shape), then by world index.  Without value-equal shapes
// this is world order within each kind.  The tie rule never depends on the
// table order (the kernels carry world indices), so the order only groups
// each class's members for the containers walk.
std::vector<uint32_t> table_order(const rt_shape_desc* shapes, uint32_t ns, const std::vector<uint32_t>& cls) {
    std::vector<uint32_t> order(ns);
    for (uint32_t i = 0; i < ns; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (shapes[a].kind != shapes[b].kind) return shapes[a].kind < shapes[b].kind;
        return cls[a] < cls[b];
    });
    return order;
}

// The triangle hierarchy of a world (tri_tree.hpp): the bounded triangles of
// `order` (table_order's; a record is bounded when bounding_sphere gives a
// radius and RTC_DEBUG=cull=0 is not set) are moved to the front of the
// triangle run in the tree's leaf order, the unbounded ones follow in their
// old order.  Classes stay adjacent (the tree never divides one, and members
// of a class are bounded alike), so build_world's class ends still hold.
// No tree (an empty plan, `order` untouched) below kTriTreeMin bounded
// triangles, under RTC_DEBUG=tri_tree=0, and (build_scene) for worlds small
// enough for the per-scene builds' records.
struct TrianglePlan {
    tri::Tree tree;
    uint32_t in_tree = 0;  // records of the triangle run reached through leaves (they come first)
    double build_ms = 0.0;
};
TrianglePlan plan_triangles(const rt_context::Knobs& knobs, const rt_shape_desc* shapes, std::vector<uint32_t>& order,
                            const std::vector<uint32_t>& cls, ident::Normals velocity = nullptr) {
    TrianglePlan plan;
    if (!knobs.tri_tree || !knobs.cull) return plan;
    const auto t0 = std::chrono::steady_clock::now();
    size_t first = 0;
    while (first < order.size() && shapes[order[first]].kind != RT_SHAPE_TRIANGLE) ++first;
    std::vector<uint32_t> bounded, unbounded, bcls;
    std::vector<tri::Ball> balls;
    for (size_t j = first; j < order.size(); ++j) {
        double bs[4];
        bounding_sphere(shapes[order[j]], bs);
        // (a moving triangle stays outside the tree, a static world-space structure: it goes to the flat run)
        if (bs[3] >= 0.0 && !ident::normals_of(velocity, order[j])) {
            bounded.push_back(order[j]);
            bcls.push_back(cls[order[j]]);
            balls.push_back({{bs[0], bs[1], bs[2]}, bs[3]});
        } else {
            unbounded.push_back(order[j]);
        }
    }
    if (bounded.size() < (knobs.tri_min ? knobs.tri_min : tri::kTriTreeMin)) return plan;
    plan.tree = tri::build(balls.data(), bcls.data(), (uint32_t)bounded.size(),
                           knobs.tri_leaf ? knobs.tri_leaf : tri::kTriLeaf);
    plan.in_tree = (uint32_t)bounded.size();
    size_t at = first;
    for (uint32_t from : plan.tree.order) order[at++] = bounded[from];
    for (uint32_t i : unbounded) order[at++] = i;
    plan.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return plan;
}

// World indices of a shape list that is not the whole world (an instanced
// world's plain records: the shapes, then the triangles of the instances
// uploaded expanded, whose world indices are the expansion's).  Default: the
// list is the world, shape i is world index i.
struct WorldIndices {
    const uint32_t* index = nullptr;  // world index of list entry i; null: i
    uint32_t n_plain = 0;             // with `index`: entries [0, n_plain) are the world's first shapes (world_slot's reach)
    std::vector<int32_t>* slot_of = nullptr;  // out: slot | kind << 24 of list entry i
    ident::Normals normals = nullptr;  // vertex normals of list entry i, null for a flat shape (null: none is smooth)
    ident::Normals uvs = nullptr;      // texture coordinates of list entry i (six doubles), null for a shape without
    ident::Normals velocity = nullptr;  // the velocity of list entry i (three doubles), null for a static shape (null: none moves)
    uint32_t of(uint32_t i) const { return index ? index[i] : i; }
    uint32_t plain(uint32_t ns) const { return index ? n_plain : ns; }
};

// What both precisions' plain tables of one upload share (build_plain_tables).
struct PlainPlan {
    std::vector<uint32_t> cls;    // value-identity classes (shape_identity.hpp)
    std::vector<uint32_t> order;  // table_order's, the tree's triangles moved to the front of their run
    TrianglePlan triangles;
};
// The plain tables of `wl` (its shapes, materials, patterns and lights) in R on the device.
template <typename R>
int build_world(rt_context* ctx, DeviceWorld<R>& w, const WorldLists& wl, const PlainPlan& pp, const WorldIndices& wi) {
    const rt_shape_desc* shapes = wl.shapes;
    const rt_material_desc* mats = wl.materials;
    const rt_pattern_desc* pats = wl.patterns;
    const rt_light_desc* lights = wl.lights;
    const uint32_t ns = wl.n_shapes, nm = wl.n_materials, np = wl.n_patterns, nl = wl.n_lights;
    const std::vector<uint32_t>& cls = pp.cls;
    const std::vector<uint32_t>& order = pp.order;
    const TrianglePlan& plan = pp.triangles;
    std::vector<ShapeRec<R>> sh;
    std::vector<int32_t> begin(kNumKinds + 1, 0);
    size_t next = 0;
    for (int k = 0; k < kNumKinds; ++k) {
        begin[k] = (int32_t)sh.size();
        for (; next < order.size() && shapes[order[next]].kind == k; ++next) {
            const uint32_t i = order[next];
            const rt_shape_desc& d = shapes[i];
            ShapeRec<R> r{};
            for (int q = 0; q < 12; ++q) r.inv[q] = (R)d.inverse[q];
            double bs[4];
            bounding_sphere(d, bs);
            for (int q = 0; q < 3; ++q) r.bound[q] = (R)bs[q];
            // the device keeps r^2; unbounded is +inf for spheres and cubes
            // (their test has no branch), -1 for the other kinds (wave_may_hit)
            const bool branchless = d.kind == RT_SHAPE_SPHERE || d.kind == RT_SHAPE_CUBE;
            r.bound[3] = ctx->knobs.cull && bs[3] >= 0.0 ? (R)(bs[3] * bs[3])
                                                   : (branchless ? std::numeric_limits<R>::infinity() : (R)-1);
            r.ymin = (R)d.minimum;
            r.ymax = (R)d.maximum;
            for (int q = 0; q < 3; ++q) {
                r.tri[q] = (R)d.vertex_1[q];
                r.tri[3 + q] = (R)d.edge_1[q];
                r.tri[6 + q] = (R)d.edge_2[q];
                r.tri[9 + q] = (R)d.normal[q];
            }
            double centre[3], r2 = 0.0;
            const bool similar = similar_sphere(d, centre, &r2);
            if (similar) {
                for (int q = 0; q < 3; ++q) r.tri[q] = (R)centre[q];
                r.tri[3] = (R)r2;
            }
            double flo[3], fhi[3], feps[3], fsgn[3];
            const bool aligned = axis_aligned_cube(d, flo, fhi, feps, fsgn);
            if (aligned)
                for (int q = 0; q < 3; ++q) {
                    r.tri[q] = (R)flo[q];
                    r.tri[3 + q] = (R)fhi[q];
                    r.tri[6 + q] = (R)feps[q];
                    r.tri[9 + q] = (R)fsgn[q];
                }
            r.world_index = (int32_t)wi.of(i);
            r.material = d.material;
            const bool class_end = next + 1 >= order.size() || cls[order[next + 1]] != cls[i];
            r.flags = (d.closed ? kShapeClosed : 0) | (class_end ? kShapeClassEnd : 0) | (similar ? kShapeSimilar : 0) | (aligned ? kShapeAxisAligned : 0) |
                      (ident::normals_of(wi.normals, i) ? kShapeSmooth : 0) | (ident::normals_of(wi.uvs, i) ? kShapeUV : 0) |
                      (ident::normals_of(wi.velocity, i) ? kShapeMoving : 0) | (int32_t)(wi.of(cls[i]) << kShapeClassShift);
            r.casts_shadow = mats[d.material].casts_shadow ? 1 : 0;
            sh.push_back(r);
        }
    }
    begin[kNumKinds] = (int32_t)sh.size();
    // the shape velocity table of a moving world (rtc_internal.hpp MotionArg), by slot, each component rounded once to R
    std::vector<R> vel;
    if (wi.velocity) {
        vel.assign(4 * std::max<size_t>(sh.size(), 1), (R)0);
        for (size_t j = 0; j < order.size(); ++j)
            if (const double* v = wi.velocity[order[j]])
                for (int q = 0; q < 3; ++q) vel[4 * j + q] = (R)v[q];
    }
    // world order -> (slot | kind << 24), padded to whole 16-byte words
    std::vector<int32_t> ws((sh.size() + 3) / 4 * 4, -1);
    for (int k = 0; k < kNumKinds; ++k)
        for (int32_t j = begin[k]; j < begin[k + 1]; ++j)
            if ((uint32_t)sh[j].world_index < wi.plain(ns)) ws[sh[j].world_index] = j | (k << 24);
    if (wi.slot_of) {  // the records of instances uploaded expanded: table positions by input index
        wi.slot_of->assign(ns, -1);
        for (size_t at = 0, j = 0; at < order.size(); ++at, ++j) (*wi.slot_of)[order[at]] = (int32_t)j | (shapes[order[at]].kind << 24);
    }
    std::vector<MaterialRec<R>> mt(nm);
    bool any_secondary = false;
    for (uint32_t i = 0; i < nm; ++i) {
        const rt_material_desc& d = mats[i];
        MaterialRec<R>& m = mt[i];
        for (int q = 0; q < 3; ++q) m.color[q] = (R)d.color[q];
        m.ambient = (R)d.ambient;
        m.diffuse = (R)d.diffuse;
        m.specular = (R)d.specular;
        m.shininess = (R)d.shininess;
        m.reflectiveness = (R)d.reflectiveness;
        m.transparency = (R)d.transparency;
        m.refractive_index = (R)d.refractive_index;
        m.pattern = d.pattern;
        m.casts_shadow = d.casts_shadow;
        if (d.reflectiveness != 0.0 || d.transparency != 0.0) any_secondary = true;
    }
    std::vector<PatternRec<R>> pt(np);
    for (uint32_t i = 0; i < np; ++i) {
        const rt_pattern_desc& d = pats[i];
        PatternRec<R>& p = pt[i];
        for (int q = 0; q < 3; ++q) {
            p.color_a[q] = (R)d.color_a[q];
            p.color_b[q] = (R)d.color_b[q];
        }
        for (int q = 0; q < 12; ++q) p.inv[q] = (R)d.inverse[q];
        p.kind = d.kind;
        p.sub_a = d.sub_a;
        // (an image pattern: its texture and its filter, and its map from the bits the upload put above the filter)
        p.sub_b = d.kind == RT_PATTERN_IMAGE ? (d.reserved & 0xFF) : d.sub_b;
        p.pad = d.kind == RT_PATTERN_IMAGE ? (d.reserved >> 8) : 0;
    }
    std::vector<LightRec<R>> lt(nl);
    for (uint32_t i = 0; i < nl; ++i)
        for (int q = 0; q < 3; ++q) {
            lt[i].position[q] = (R)lights[i].position[q];
            lt[i].intensity[q] = (R)lights[i].intensity[q];
        }
    int rc;
    // shapes, materials, patterns and world_slot in one allocation, in the LDS layout
    const size_t image_bytes = world_lds_bytes<R>(sh.size(), nm, np);
    std::vector<unsigned char> img(image_bytes);
    size_t at = 0;
    auto put = [&](const void* src, size_t n) {
        if (n) std::memcpy(img.data() + at, src, n);
        at += n;
    };
    put(sh.data(), sh.size() * sizeof(ShapeRec<R>));
    put(mt.data(), mt.size() * sizeof(MaterialRec<R>));
    put(pt.data(), pt.size() * sizeof(PatternRec<R>));
    put(ws.data(), ws.size() * sizeof(int32_t));
    // Copies run on the context's stream, never the null stream: HIP creates a
    // hardware queue for the null stream at its first use, ~8 ms that a one-shot
    // render would pay.
    if ((rc = w.allocate(sh.size(), nm, np, nl))) return rc;
    // the triangle hierarchy in R, its leaves' runs as slots of the shape table
    std::vector<TriNode<R>> nodes(plan.tree.nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) {
        const tri::Node& n = plan.tree.nodes[i];
        tri::cast_ball<R>(n.ball, nodes[i].ball);
        nodes[i].skip = n.skip;
        nodes[i].first = n.count ? begin[RT_SHAPE_TRIANGLE] + n.first : 0;
        nodes[i].count = n.count;
    }
    if ((rc = w.allocate_tree(nodes.size(), begin[RT_SHAPE_TRIANGLE] + (int32_t)plan.in_tree))) return rc;
    if (!nodes.empty() && (rc = hip_status(hipMemcpyAsync(w.tri_nodes.get(), nodes.data(), nodes.size() * sizeof(nodes[0]),
                                                          hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync"))) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    if (image_bytes && (rc = hip_status(hipMemcpyAsync(w.image.get(), img.data(), image_bytes, hipMemcpyHostToDevice,
                                                       ctx->stream), "hipMemcpyAsync"))) {
        (void)hipStreamSynchronize(ctx->stream);  // the node copy may still read `nodes`
        return rc;
    }
    if (!vel.empty()) {
        if ((rc = w.shape_vel.reserve(vel.size()))) {
            (void)hipStreamSynchronize(ctx->stream);
            return rc;
        }
        if ((rc = hip_status(hipMemcpyAsync(w.shape_vel.get(), vel.data(), vel.size() * sizeof(R), hipMemcpyHostToDevice,
                                            ctx->stream), "hipMemcpyAsync"))) {
            (void)hipStreamSynchronize(ctx->stream);
            return rc;
        }
    }
    if (nl && (rc = hip_status(hipMemcpyAsync(w.lights.get(), lt.data(), nl * sizeof(LightRec<R>),
                                              hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync"))) {
        (void)hipStreamSynchronize(ctx->stream);  // the image copy may still read `img`
        return rc;
    }
    RT_HIP(hipStreamSynchronize(ctx->stream));  // (img and lt are host temporaries)
    if constexpr (sizeof(R) == 4) {  // the per-scene build's tables (capture_jit_table), from the host copies
        ctx->jit.shapes = sh;
        ctx->jit.lights = lt;
        ctx->jit.materials = mt;
        ctx->jit.pattern_recs = pt;
    }
    ctx->world_slot.assign(ws.begin(), ws.begin() + wi.plain(ns));
    for (int k = 0; k <= kNumKinds; ++k) w.scene.kind_begin[k] = begin[k];
    w.scene.any_secondary = any_secondary ? 1 : 0;
    return RT_OK;
}

// rt_scene_upload_lit's list; empty: valid.  Each refusal has a text of its own (rtc.h).
static std::string validate_area(const rt_area_light_desc* area, uint32_t n_area) {
    if (n_area && !area) return "rt_scene_upload_lit: null area light list with nonzero count";
    for (uint32_t a = 0; a < n_area; ++a) {
        const rt_area_light_desc& d = area[a];
        const std::string who = "area light " + std::to_string(a);
        if (d.usteps == 0 || d.vsteps == 0) return who + ": a step count of 0";
        if (d.usteps > RT_LIGHT_MAX_STEPS || d.vsteps > RT_LIGHT_MAX_STEPS)
            return who + ": a step count above RT_LIGHT_MAX_STEPS";
        if (d.jitter != RT_JITTER_NONE && d.jitter != RT_JITTER_HASHED) return who + ": unknown jitter mode";
        for (int q = 0; q < 3; ++q)
            if (!std::isfinite(d.corner[q]) || !std::isfinite(d.full_uvec[q]) || !std::isfinite(d.full_vvec[q]) ||
                !std::isfinite(d.intensity[q]))
                return who + ": a component that is not finite";
    }
    return std::string();
}

// rt_scene_upload_moving's list against the validated shape, mesh and instance lists; empty: valid.  Each
// refusal has a text of its own (rtc.h "Motion blur"), in the order written there.
static std::string validate_motion(const WorldLists& wl) {
    if (wl.n_motion && !wl.motion) return "rt_scene_upload_moving: null motion list with nonzero count";
    uint64_t world = wl.n_shapes;  // the expansion's shapes: the top-level ones, then every instance's triangles
    for (uint32_t k = 0; k < wl.n_instances; ++k) world += wl.meshes[wl.instances[k].mesh].n_triangles;
    std::vector<char> shape_named(wl.n_shapes, 0), inst_named(wl.n_instances, 0);
    for (uint32_t m = 0; m < wl.n_motion; ++m) {
        const rt_motion_desc& d = wl.motion[m];
        const std::string who = "motion " + std::to_string(m);
        if (d.target != RT_MOVE_SHAPE && d.target != RT_MOVE_INSTANCE) return who + ": unknown target";
        const bool shape = d.target == RT_MOVE_SHAPE;
        if (shape ? d.index >= world : d.index >= wl.n_instances) return who + ": index out of range";
        if (!shape || d.index < wl.n_shapes) {
            char& named = shape ? shape_named[d.index] : inst_named[d.index];
            if (named) return who + ": target named twice";
            named = 1;
        }
        for (int q = 0; q < 3; ++q)
            if (!std::isfinite(d.velocity[q])) return who + ": a velocity component that is not finite";
        if (shape && d.index >= wl.n_shapes)
            return who + ": the shape belongs to a mesh run (a triangle of an instance's mesh does not move alone: move the instance)";
    }
    return std::string();
}

// The base tables of `wl`: shapes, materials, patterns, lights.
static int validate_base(const WorldLists& wl) {
    const rt_shape_desc* shapes = wl.shapes;
    const rt_material_desc* mats = wl.materials;
    const rt_pattern_desc* pats = wl.patterns;
    const uint32_t ns = wl.n_shapes, nm = wl.n_materials, np = wl.n_patterns, nl = wl.n_lights;
    // (an image pattern exists for rt_scene_upload_textured and _lit only, checked against their texture count)
    const int64_t n_textures = wl.image_patterns ? (int64_t)wl.n_textures : -1;
    if ((ns && !shapes) || (nm && !mats) || (np && !pats) || (nl && !wl.lights))
        return set_error(RT_ERR_INVALID, "rt_scene_upload: null table with nonzero count");
    for (uint32_t i = 0; i < ns; ++i) {
        if (shapes[i].kind < 0 || shapes[i].kind >= kNumKinds)
            return set_error(RT_ERR_INVALID, "shape " + std::to_string(i) + ": unknown kind");
        if (shapes[i].material < 0 || (uint32_t)shapes[i].material >= nm)
            return set_error(RT_ERR_INVALID, "shape " + std::to_string(i) + ": material index out of range");
    }
    for (uint32_t i = 0; i < nm; ++i)
        if (mats[i].pattern >= 0 && (uint32_t)mats[i].pattern >= np)
            return set_error(RT_ERR_INVALID, "material " + std::to_string(i) + ": pattern index out of range");
    for (uint32_t i = 0; i < np; ++i) {
        if (pats[i].kind < 0 || pats[i].kind > (n_textures >= 0 ? RT_PATTERN_IMAGE : RT_PATTERN_TEST))
            return set_error(RT_ERR_INVALID, "pattern " + std::to_string(i) + ": unknown kind");
        if (pats[i].kind == RT_PATTERN_COMPLEX &&
            (pats[i].sub_a < 0 || pats[i].sub_b < 0 || (uint32_t)pats[i].sub_a >= np || (uint32_t)pats[i].sub_b >= np))
            return set_error(RT_ERR_INVALID, "pattern " + std::to_string(i) + ": bad sub-pattern index");
        if (n_textures >= 0 && pats[i].kind == RT_PATTERN_COMPLEX &&
            (pats[pats[i].sub_a].kind == RT_PATTERN_IMAGE || pats[pats[i].sub_b].kind == RT_PATTERN_IMAGE))
            return set_error(RT_ERR_INVALID, "pattern " + std::to_string(i) + ": an image pattern cannot be a sub-pattern");
        if (pats[i].kind == RT_PATTERN_IMAGE) {
            if (pats[i].sub_a < 0 || (int64_t)pats[i].sub_a >= n_textures)
                return set_error(RT_ERR_INVALID, "pattern " + std::to_string(i) + ": texture index out of range");
            if (pats[i].sub_b != -1)
                return set_error(RT_ERR_INVALID, "pattern " + std::to_string(i) + ": an image pattern's sub_b must be -1");
            if (pats[i].reserved != RT_FILTER_NEAREST && pats[i].reserved != RT_FILTER_BILINEAR)
                return set_error(RT_ERR_INVALID, "pattern " + std::to_string(i) + ": unknown texture filter");
        }
    }
    if (ns > 0xFFFFFF || nl > 0x7fffffff) return set_error(RT_ERR_INVALID, "table too large");
    return RT_OK;
}

int validate_scene(const WorldLists& wl) {
    std::string why = validate_area(wl.area, wl.n_area);
    // (the texture list before the base tables: the patterns are checked against it)
    if (why.empty() && wl.image_patterns) why = inst::validate_textures(wl.textures, wl.n_textures);
    if (!why.empty()) return set_error(RT_ERR_INVALID, why);
    if (int rc = validate_base(wl)) return rc;
    why = inst::validate(wl.shapes, wl.n_shapes, wl.meshes, wl.n_meshes, wl.instances, wl.n_instances, wl.n_materials);
    if (why.empty())
        why = inst::validate_side<inst::SmoothSide>(wl.shapes, wl.n_shapes, wl.meshes, wl.n_meshes, wl.smooth, wl.n_smooth);
    if (why.empty()) why = inst::validate_side<inst::UVSide>(wl.shapes, wl.n_shapes, wl.meshes, wl.n_meshes, wl.uvs, wl.n_uvs);
    uint64_t total = wl.n_lights;  // the expansion's lights: the point lights and every area light's samples
    for (uint32_t a = 0; why.empty() && a < wl.n_area; ++a) total += wl.area[a].usteps * wl.area[a].vsteps;
    if (why.empty() && total > 0x7fffffffull) why = "table too large";
    if (why.empty()) why = inst::validate_maps(wl.maps, wl.n_maps, wl.patterns, wl.n_patterns, wl.n_textures);
    if (why.empty()) why = validate_motion(wl);
    return why.empty() ? RT_OK : set_error(RT_ERR_INVALID, why);
}

uint32_t tile_rows_for(uint32_t height, uint32_t shards, uint32_t shard) {
    return shard_tile_rows(height, shards, shard);
}

// LIFO bound of a workgroup's ray pool (rays).  Block-lockstep generations
// pop at most `batch` rays from the top and push at most two children per
// ray, one level deeper, so the pool never holds more than
// kBlock + depth x batch.  A child past the bound would be dropped and
// flagged (RT_ERR_POOL), never written out of bounds.
uint32_t pool_capacity(uint32_t depth, uint32_t batch) {
    return (uint32_t)kBlock + depth * batch;
}

// Dynamic LDS of the pool (after the world tables): the item slots'
// accumulators, then `lcap` LIFO slots (a multiple of 8 keeps every array
// 16-byte aligned).
template <typename R>
size_t pool_lds_bytes(uint32_t lcap) {
    return (size_t)kTileSlots * 3 * kBlock * sizeof(PoolAcc<R>) + (size_t)lcap * (7 * sizeof(R) + sizeof(PoolMeta));
}

// Bound on any pixel of the pool kernel: a shaded hit adds at most
// bright_hit, its children carry at most bright_w of its weight.
double pixel_bound(double bright_hit, double bright_w, uint32_t depth) {
    double tree = 0.0, w = 1.0;
    for (uint32_t g = 0; g <= depth; ++g, w *= bright_w) tree += w;
    return bright_hit * tree;
}

// The pool kernel's fixed-point sums hold pixels up to 2^30 x 2^-acc_log2
// (f32: int32, acc_log2 >= kAccLog2Min) or 2^15 (f64: int64 multiples of
// 2^-48): a world that may exceed that (a TestPattern on an unbounded
// surface, or huge light intensities) is refused rather than wrapped.
int check_pixel_range(const rt_context* ctx, uint32_t depth, bool f32) {
    const double b = pixel_bound(ctx->bright_hit, ctx->bright_w, depth);
    const double lim = f32 ? std::ldexp(1.0, 30 - (int)kAccLog2Min) : std::ldexp(1.0, 14);
    if (!(b < lim))
        return set_error(RT_ERR_INVALID, "pixel colours of this world are unbounded for the ray pool's fixed-point sums "
                                         "(bound " + std::to_string(b) + " >= " + std::to_string(lim) +
                                         "; a TestPattern on an unbounded surface?)");
    return RT_OK;
}

// Scale of the f32 pool kernel's int32 pixel sums (rtc_internal.hpp
// PoolAcc): the largest 2^s with the world's brightest possible pixel below
// 2^30 / 2^s.  A shaded hit adds at most bright_hit (per light, the
// intensity times the material's colour x (ambient + diffuse) + specular,
// material.rs:83-114) and a hit's children carry at most bright_w of its
// weight (reflectiveness + transparency, world.rs:54-66: Schlick's R and
// 1 - R are in [0, 1]), so a pixel is below bright_hit x sum_{g<=depth} bright_w^g.
// A supersampled pixel (trace_pool_ss) is the sum of n^2 such trees, each
// seeded at weight 1/n^2: the weights sum to 1 (in R, n^2 x R(1)/R(n^2) <= 1
// up to one rounding, far inside the factor of 2 between the bound and 2^30),
// so its bound is the same, and so are this scale and check_pixel_range's
// verdict, whatever the grid.
uint32_t acc_shift_f32(double bright_hit, double bright_w, uint32_t depth) {
    const double bound = std::max(pixel_bound(bright_hit, bright_w, depth), 1e-30);
    const int s = 30 - (int)std::ceil(std::log2(bound));
    return (uint32_t)std::min<int>(kAccLog2Max, std::max<int>(kAccLog2Min, s));
}

constexpr size_t kLdsPerCu = 160 * 1024;
// Static LDS of the tracer kernels (the pool kernel's per-wave LIFO tops and
// item tables and the counter flush: 400 B) plus headroom; the code-object
// metadata (tests/test_isa_budget.py) checks the real value.
constexpr size_t kStaticLds = 512;

struct LaunchShape {
    int per_cu;  // workgroups per CU the launch is planned for
    KernelId id;  // the kernel the launch is planned for
    uint32_t world_lds;  // world tables staged in LDS (bytes, 0 = none)
    uint32_t sched;
    uint32_t grid;
    size_t lds;
    uint32_t cap, lcap, batch;  // pool: LIFO bound, its LDS-resident part, pop batch
    uint32_t grid_tiles;        // the launch's tiles (the grid's upper bound)
};

// Workgroups per CU at `lds` dynamic bytes: the occupancy API's register/wave
// limit `api`, capped by the LDS limit from static + dynamic bytes (512-byte
// granules).
int cap_by_lds(int api, size_t lds) {
    const size_t per_block = (kStaticLds + lds + 511) / 512 * 512;
    return std::min(api, (int)(kLdsPerCu / per_block));
}

// Cached occupancy (workgroups per CU) of kernel `id` of the world's build at
// a given dynamic LDS size (cap_by_lds); an upload that changes the build
// clears the cache (set_kernel_build).
template <typename R>
int blocks_per_cu(rt_context* ctx, KernelId id, size_t lds, int* per_cu) {
    const int slot = id.occupancy_slot(sizeof(R) == 8);
    if (ctx->occ_lds[slot] == lds && ctx->occ_blocks[slot] > 0) {
        *per_cu = ctx->occ_blocks[slot];
        return RT_OK;
    }
    int api = 0;
    RT_HIP(launchers<R>(ctx).kernel_occupancy(id, lds, &api));
    *per_cu = cap_by_lds(api, lds);
    ctx->occ_lds[slot] = lds;
    ctx->occ_blocks[slot] = *per_cu;
    return RT_OK;
}

// LDS-resident part of the ray pool: as many slots as keep a pool kernel at
// the workgroups/CU its registers allow, `occ(lds, &blocks)` being its
// occupancy at a given dynamic LDS size; the rest of the bound spills to
// global memory.  *best: that workgroup count.
template <typename R, typename Occ>
int pool_lds_plan(rt_context* ctx, uint32_t world_lds, uint32_t cap, Occ&& occ, uint32_t* lcap, int* best_out) {
    constexpr uint32_t kMinRays = kBlock;
    int best = 0, rc;
    if ((rc = occ(world_lds + pool_lds_bytes<R>(kMinRays), &best))) return rc;
    if (best < 1) best = 1;
    const size_t rec = 7 * sizeof(R) + sizeof(PoolMeta);
    const size_t budget = (size_t)kLdsPerCu / (size_t)best;
    const size_t fixed = kStaticLds + world_lds + pool_lds_bytes<R>(0) + 511;
    uint32_t n = budget > fixed ? (uint32_t)((budget - fixed) / rec) : kMinRays;
    // one workgroup's LDS must also stay within the launch limit
    const size_t room = ctx->lds_per_block > fixed ? ctx->lds_per_block - fixed : 0;
    n = std::min<uint32_t>(n, (uint32_t)(room / rec));
    n = std::min<uint32_t>(cap, std::max<uint32_t>(kMinRays, n & ~7u));
    for (;;) {  // granule rounding: step down until `best` workgroups fit
        int got = 0;
        if ((rc = occ(world_lds + pool_lds_bytes<R>(n), &got))) return rc;
        if (got >= best || n <= kMinRays) break;
        n = std::max<uint32_t>(kMinRays, n - 8);
    }
    *lcap = n;
    if (best_out) *best_out = best;
    return RT_OK;
}

// ... for the static pool kernel `id` (6 workgroups/CU for f32 at <= 80 VGPRs).
// RTC_DEBUG=pool_lds_rays=N overrides (A/B).
template <typename R>
int pool_lds_rays(rt_context* ctx, KernelId id, uint32_t world_lds, uint32_t cap, uint32_t* lcap) {
    if (ctx->knobs.pool_lds_rays > 0) {
        *lcap = std::min<uint32_t>(cap, std::max<uint32_t>(kBlock, ctx->knobs.pool_lds_rays & ~7u));
        return RT_OK;
    }
    return pool_lds_plan<R>(ctx, world_lds, cap, [&](size_t lds, int* b) { return blocks_per_cu<R>(ctx, id, lds, b); },
                            lcap, nullptr);
}

// LDS world of a per-scene kernel that takes the shape records from its
// instruction stream (rtc_kernels.hip kJitRecords: worlds of <= 255 shapes):
// the materials and patterns only.
template <typename R>
size_t jit_world_lds_bytes(const DevScene<R>& sc) {
    return (size_t)sc.n_materials * sizeof(MaterialRec<R>) + (size_t)sc.n_patterns * sizeof(PatternRec<R>);
}
#ifndef RTC_JIT_NO_RECORDS  // (A/B builds: -DRTC_JIT_NO_RECORDS keeps the whole world in LDS)
constexpr int32_t kJitRecordsMaxShapes = 255;
#else
constexpr int32_t kJitRecordsMaxShapes = -1;
#endif

// A per-scene pool kernel built for more waves/SIMD than the static one
// (rtc_jit.cpp jit_function): the pool's LDS share re-planned for the
// workgroups per CU its registers allow, as pool_lds_rays does for the
// static kernel, and the resident grid with it.
template <typename R>
int plan_pool_for(rt_context* ctx, hipFunction_t fn, LaunchShape& ls) {
    auto blocks = [&](size_t lds, int* per_cu) -> int {  // (blocks_per_cu's rule, for this function)
        int api = 0;
        RT_HIP(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&api, fn, kBlock, lds));
        *per_cu = cap_by_lds(api, lds);
        return RT_OK;
    };
    uint32_t n = 0;
    int best = 0, got = 0, rc;
    if ((rc = pool_lds_plan<R>(ctx, ls.world_lds, ls.cap, blocks, &n, &best))) return rc;
    if ((rc = blocks(ls.world_lds + pool_lds_bytes<R>(n), &got))) return rc;
    if (got <= ls.per_cu) return RT_OK;  // no more workgroups than planned: keep the plan
    ls.lcap = n;
    ls.lds = ls.world_lds + pool_lds_bytes<R>(n);
    ls.per_cu = got;
    const uint64_t resident = (uint64_t)got * (uint64_t)ctx->cu_count;
    ls.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(ls.grid_tiles, resident));
    return RT_OK;
}

// id: the launch's family and dup; pool and lds are decided here, and ls.id
// is the kernel planned for.  samples: the grid of a supersampled or lens
// launch (its pool bound), 0 for a plain one.  jit_records: the plan of a
// per-scene kernel that holds the shape records as constants.
template <typename R>
int plan_launch(rt_context* ctx, const DevScene<R>& sc, uint32_t depth, uint32_t n_tiles, KernelId id, uint32_t samples,
                bool jit_records, LaunchShape& ls) {
    const bool pool = id.pool = sc.any_secondary && depth > 0;
    const size_t wb = jit_records ? std::max<size_t>(16, jit_world_lds_bytes(sc))
                                  : world_lds_bytes<R>(sc.kind_begin[kNumKinds], sc.n_materials, sc.n_patterns);
    // (a per-scene direct kernel takes its materials from constants too and
    // stages no world at all: rtc_kernels.hip kJitConstMaterials)
    ls.world_lds = (ctx->knobs.lds_world && wb <= kMaxWorldLds && !(jit_records && !pool)) ? (uint32_t)wb : 0;
    id.lds = ls.world_lds != 0;
    ls.id = id;
    ls.lds = ls.world_lds;
    ls.cap = ls.lcap = ls.batch = 0;
    ls.sched = pool ? kSchedDynamic : ctx->knobs.sched_direct;
    int rc;
    if (pool) {
        // (the pool kernel takes its items from the per-XCD queues only)
        ls.batch = kPoolBatch;
        ls.cap = samples ? pool_capacity_ss(depth, ls.batch, samples) : pool_capacity(depth, ls.batch);
        if ((rc = pool_lds_rays<R>(ctx, id, ls.world_lds, ls.cap, &ls.lcap))) return rc;
        ls.lds += pool_lds_bytes<R>(ls.lcap);
    }
    int per_cu = 0;
    if ((rc = blocks_per_cu<R>(ctx, id, ls.lds, &per_cu))) return rc;
    if (per_cu < 1) per_cu = 1;
    ls.per_cu = per_cu;
    const uint64_t resident = (uint64_t)per_cu * (uint64_t)ctx->cu_count;
    // The f32 direct kernel's static schedule runs 2.5x the resident grid: the
    // dispatcher starts the surplus workgroups as resident ones finish, which
    // evens out the last round.  Same-box sweep, three_sphere / shadow_puppets
    // 1080p (8160 tiles, 2048 resident at 8 waves/SIMD): 2048 34.4 / 42.0 us,
    // 3072 32.6 / 40.1, 4096 33.1 / 40.3, 5120 32.3 / 38.8, 6144 32.9 / 38.8,
    // 8160 (one tile each) 34.1 / 39.8; three_sphere 4K 115.6 -> 107.0 us.
    // The f64 kernel (3 waves/SIMD) measured 3.7% slower that way.
    const bool oversub = !pool && ls.sched == kSchedStatic && sizeof(R) == 4;
    const uint64_t grid_cap = oversub ? std::max<uint64_t>(1, resident * ctx->knobs.direct_oversub10 / 10) : resident;
    ls.grid = ls.sched != kSchedGrid ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_tiles, grid_cap)) : n_tiles;
    ls.grid_tiles = n_tiles;
    return RT_OK;
}

// Same frame as the last pool launch?  (scene upload, canvas, shard, depth,
// precision, grid, camera; ray batches of rt_color_at are never
// cost-ordered)  Then hand its tiles out heaviest-first by the costs earlier
// launches recorded; every launch records its costs.  A frame's tile costs
// hardly change from one launch to the next, so the order is built
// (order_tiles) on launches 2 .. 1 + order_max_builds of a signature and then
// reused: order_tiles ran before every launch, 8 us per 1080p frame and 23 us
// per 4K frame of stream time ahead of the tracer.  A moved camera (the same
// frame otherwise) is ordered by the costs the previous camera's launch
// recorded: neighbouring frames of a camera path have similar tile costs.
// reflect_refract 1080p panning 0.1 degree per frame: 0.545 ms per frame in
// raster order, 0.528 reusing the first camera's order, 0.450 rebuilding
// from the previous frame's costs (scripts/camera_path.py), against 0.422
// for a repeated camera; metal, whose 0.1 ms frames gain little from any
// order, pays the 10 us sort (0.101 -> 0.107 ms).
// A supersampled launch keeps an order and costs of its own (`to` =
// ctx->order_ss, the sample grid in the signature): its tiles cost n^2
// samples each, and it neither reuses nor overwrites what the plain launches
// of the same camera recorded.  So does a lens launch (ctx->order_lens, the
// lens in the signature beside the camera).
template <typename R>
int plan_tile_order(rt_context* ctx, rt_context::TileOrder& to, LaunchParams<R>& P, const rt_camera_desc* cam,
                    uint32_t depth, uint32_t grid, hipStream_t stream, const rt_lens_desc* lens = nullptr,
                    const rt_shutter_desc* shutter = nullptr) {
    if (P.n_tiles > kItemTileMask + 1) return RT_OK;  // items carry 20 tile bits: raster order
    uint64_t h = 1469598103934665603ull;  // FNV-1a
    auto mix = [&h](const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    };
    const uint64_t fields[] = {ctx->scene_gen, P.n_tiles, P.width, P.height, P.shard_index, P.shard_count,
                               depth, sizeof(R), grid, P.ss_grid};
    mix(fields, sizeof(fields));
    const uint64_t geometry = h;
    if (cam) mix(cam, sizeof(*cam));
    if (lens) mix(lens, sizeof(*lens));
    if (shutter) mix(shutter, sizeof(*shutter));
    bool grew_cost = false, grew_order = false;
    int rc = to.d_cost.reserve(P.n_tiles, &grew_cost);
    // up to 2^kMaxSplitLog2 items per tile, then the item count
    if (!rc) rc = to.d_order.reserve(((size_t)P.n_tiles << kMaxSplitLog2) + 1, &grew_order);
    if (rc || grew_cost || grew_order) to.valid = to.built = false;
    if (rc) return rc;
    if (grew_cost || grew_order)  // (the kernel records a tile's cost as the maximum over its parts)
        RT_HIP(hipMemsetAsync(to.d_cost.get(), 0, to.d_cost.capacity() * sizeof(uint32_t), stream));
    const bool same = to.valid && to.sig == h;
    const bool moved = !same && to.valid && to.geometry == geometry;
    if (!same) to.builds = 0;
    if (!to.valid || to.geometry != geometry) to.built = false;
    uint32_t* n_items = to.d_order.get() + to.d_order.capacity() - 1;
    if ((same || moved) && to.builds < kOrderBuilds) {
        const float split = ctx->knobs.split_factor > 0 ? (float)(ctx->knobs.split_factor / grid) : 0.0f;
        const float urgent = ctx->knobs.urgent_factor > 0 ? (float)(ctx->knobs.urgent_factor / grid) : 0.0f;
        RT_HIP(launch_order_tiles(to.d_cost.get(), to.d_order.get(), P.n_tiles, n_items, split, ctx->knobs.split_max,
                                  urgent, 1u, 0u, stream));
        ++to.builds;
        to.built = true;
    }
    if (to.built) {  // built from this frame's costs, or from the previous camera's frame
        P.tile_order = to.d_order.get();
        P.item_count = n_items;
    } else if (P.shard_count == 1) {
        // No costs yet: tiles nearest the image centre first.  The order
        // depends on the canvas only, so it is built and uploaded once per
        // canvas size into its own buffer (order_tiles reuses d_order).
        if (!to.d_cold.get() || to.cold_w != P.width || to.cold_h != P.height) {
            const uint32_t n = P.n_tiles, tx = P.tiles_x;
            std::vector<std::pair<uint64_t, uint32_t>> key(n);
            const int64_t cx = (int64_t)P.width, cy = (int64_t)P.height;  // doubled centre
            for (uint32_t t = 0; t < n; ++t) {
                const int64_t x = 2 * (int64_t)((t % tx) * RT_TILE_W) + RT_TILE_W - cx;
                const int64_t y = 2 * (int64_t)((t / tx) * RT_TILE_H) + RT_TILE_H - cy;
                key[t] = {(uint64_t)(x * x + y * y), t};
            }
            std::sort(key.begin(), key.end());
            std::vector<uint32_t> v(n + 1);
            for (uint32_t i = 0; i < n; ++i) v[i] = key[i].second;
            v[n] = n;
            to.cold_w = to.cold_h = 0;  // (nothing valid until the copy below is done)
            if ((rc = to.d_cold.reserve(v.size()))) return rc;
            // (the launch's stream, not the null stream; v is a host temporary)
            RT_HIP(hipMemcpyAsync(to.d_cold.get(), v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                  stream));
            RT_HIP(hipStreamSynchronize(stream));
            to.cold_w = P.width;
            to.cold_h = P.height;
        }
        P.tile_order = to.d_cold.get();
        P.item_count = to.d_cold.get() + P.n_tiles;
    }
    P.tile_cost = to.d_cost.get();
    to.sig = h;
    to.geometry = geometry;
    to.valid = true;
    return RT_OK;
}

int order_after_last(rt_context* ctx, hipStream_t stream) {
    if (ctx->launched && stream != ctx->last_stream) {
        RT_HIP(hipEventRecord(ctx->ev_order, ctx->last_stream));
        RT_HIP(hipStreamWaitEvent(stream, ctx->ev_order, 0));
    }
    ctx->last_stream = stream;
    ctx->launched = true;
    return RT_OK;
}

// One tracer launch: a frame or shard strip of `cam` (launch_frame), or a batch of rays (rt_color_at).
struct LaunchRequest {
    const rt_camera_desc* cam = nullptr;  // a frame, or ...
    const double* d_rays = nullptr;       // ... n_rays rays of 6 doubles on the device
    uint64_t n_rays = 0;
    uint32_t depth = 0, out_format = RT_OUT_REAL;
    uint32_t shard_index = 0, shard_count = 1;
    void* out_device = nullptr;
    hipStream_t stream = nullptr;
    uint32_t flags = 0;
    bool image_rows = false;
    uint32_t samples = 0;  // a supersampled frame's grid (cam = the sample camera, out_w x out_h the output), 0 = plain
    uint32_t out_w = 0, out_h = 0;
    const rt_lens_desc* lens = nullptr;  // with samples (a grid of 1 too): a lens frame (rt_render_lens*), aperture > 0
    // with samples (a grid of 1 too), of a moving world: a shutter frame (rt_render_shutter*), with or without a lens
    const rt_shutter_desc* shutter = nullptr;
};

// Host restatement of the kernels' transforms (rtc_kernels.hip xform_point): the f64 left fold, the f32 fused chain.
inline void lens_xform_point(const double* m, const double p[3], double out[3]) {
    for (int r = 0; r < 3; ++r)
        out[r] = (((0.0 + m[4 * r] * p[0]) + m[4 * r + 1] * p[1]) + m[4 * r + 2] * p[2]) + m[4 * r + 3];
}
inline void lens_xform_point(const float* m, const float p[3], float out[3]) {
    for (int r = 0; r < 3; ++r)
        out[r] = std::fmaf(m[4 * r + 2], p[2], std::fmaf(m[4 * r + 1], p[1], std::fmaf(m[4 * r], p[0], m[4 * r + 3])));
}

// The lens point of cell position (fu, fv) = (ci + ju, cj + jv) (rtc.h "Thin-lens
// camera": square to disc, camera-space L, origin = inverse * L), in the
// kernels' own operations (rtc_kernels.hip lens_ray's hashed branch; this file
// is compiled with -ffp-contract=off).
template <typename R>
void lens_point(const R* inv, R aperture, R inv_n, R fu, R fv, LensPoint<R>& out) {
    const R a = (R)2 * (fu * inv_n) - (R)1, b = (R)2 * (fv * inv_n) - (R)1;
    const R ex = a * std::sqrt((R)1 - (b * b) * (R)0.5), ey = b * std::sqrt((R)1 - (a * a) * (R)0.5);
    out.lx = aperture * ex;
    out.ly = aperture * ey;
    const R l[3] = {out.lx, out.ly, (R)0};
    lens_xform_point(inv, l, out.origin);
}

// The launch's lens: under RT_JITTER_NONE the n^2 lens points, one per sample
// (cell centres), which the kernels read instead of working them out per lane.
template <typename R>
void set_lens_params(const LaunchParams<R>& P, const rt_lens_desc& lens, uint32_t n, LensParams<R>& o) {
    o.aperture = (R)lens.aperture;
    o.focal = (R)lens.focal_distance;
    o.inv_n = (R)1 / (R)n;
    o.jitter = lens.jitter;
    o.lk = hash_mix(lens.seed ^ kLensKey);
    if (lens.jitter != RT_JITTER_NONE) return;
    for (uint32_t j = 0; j < n; ++j)
        for (uint32_t i = 0; i < n; ++i)
            lens_point<R>(P.cam.inv, o.aperture, o.inv_n, (R)i + (R)0.5, (R)j + (R)0.5, o.points[j * n + i]);
}

// The launch's shutter (rtc.h "The shutter"): open and span = close - open formed in f64, each rounded once to R.
template <typename R>
void set_shutter_params(const rt_shutter_desc& sh, uint32_t n, ShutterParams<R>& o) {
    o.open = (R)sh.open;
    o.span = (R)(sh.close - sh.open);
    o.inv_n2 = (R)1 / (R)(n * n);
    o.jitter = sh.jitter;
    o.tk = hash_mix(sh.seed ^ kShutterKey);
}

// The velocity tables of a moving world as its kernels take them (rtc_internal.hpp MotionArg).
template <typename R>
MotionArg motion_arg(const DeviceWorld<R>& w) {
    return {w.shape_vel.get(), w.inst_counts.instances ? w.inst_vel.get() : nullptr};
}

// Step 1 of a launch (frames and ray batches alike): the launch's view of the
// world, its tables, triangle hierarchy, mesh instances (none: no world index
// reaches inst_world_begin), side tables, textures and area lights.
template <typename R>
void set_world_params(const rt_context* ctx, const DeviceWorld<R>& w, LaunchParams<R>& P) {
    P.scene = w.scene;
    P.tri_nodes = w.n_tri_nodes ? w.tri_nodes.get() : nullptr;
    P.n_tri_nodes = w.n_tri_nodes;
    P.tri_flat_begin = w.tri_flat_begin;
    const InstanceCounts& c = w.inst_counts;
    P.n_instances = c.instances;
    P.inst_world_begin = c.instances ? c.world_begin : std::numeric_limits<int32_t>::max();
    P.inst = c.instances ? w.inst.get() : nullptr;
    P.inst_shapes = w.inst_shapes.get();
    P.inst_nodes = w.inst_nodes.get();
    P.inst_pos = w.inst_pos.get();
    P.smooth_plain = w.smooth.plain();
    P.smooth_inst = w.smooth.inst();
    P.uv_plain = w.uv.plain();
    P.uv_inst = w.uv.inst();
    P.texels = w.texels;
    P.textures = w.tex_table;
    P.area = w.n_area ? w.area.get() : nullptr;
    P.n_area = w.n_area;
    P.area_samples = w.area_samples;
    P.area_cull = ctx->knobs.area_cull ? 1u : 0u;  // (RTC_DEBUG=area_cull=0 clears it)
}

// Step 2: what the launch renders, a camera's canvas (with the lens of a lens
// frame) or a ray batch, and where its output and counters go.
template <typename R>
void set_target_params(rt_context* ctx, const LaunchRequest& q, LaunchParams<R>& P, ShutterArg<R>& frame_arg) {
    LensParams<R>& lens_params = frame_arg.lens;
    P.image_rows = q.image_rows ? 1u : 0u;
    if (const rt_camera_desc* cam = q.cam) {
        for (int i = 0; i < 12; ++i) P.cam.inv[i] = (R)cam->inverse[i];
        for (int i = 0; i < 3; ++i) P.cam.origin[i] = (R)cam->origin[i];
        P.cam.half_width = (R)cam->half_width;
        P.cam.half_height = (R)cam->half_height;
        P.cam.pixel_size = (R)cam->pixel_size;
        // (a supersampled frame: the canvas and its tiles are the output's)
        P.ss_grid = q.samples;
        if (q.lens) set_lens_params(P, *q.lens, q.samples, lens_params);
        if (q.shutter) set_shutter_params(*q.shutter, q.samples, frame_arg.shutter);  // (no lens: aperture 0, the pinhole's rays)
        P.width = q.samples ? q.out_w : cam->width;
        P.height = q.samples ? q.out_h : cam->height;
        P.tiles_x = (P.width + RT_TILE_W - 1) / RT_TILE_W;
        P.tile_rows = tile_rows_for(P.height, q.shard_count, q.shard_index);
        P.n_tiles = P.tiles_x * P.tile_rows;
        P.tiles_x_magic = div_magic(P.tiles_x, P.n_tiles);
    } else {
        P.rays = q.d_rays;
        P.n_rays = q.n_rays;
        P.n_tiles = (uint32_t)((q.n_rays + kBlock - 1) / kBlock);
    }
    P.out = q.out_device;
    P.out_format = q.out_format;
    P.shard_index = q.shard_index;
    P.shard_count = q.shard_count;
    P.max_depth = q.depth;
    P.tile_counter = ctx->d_tile_counter.get();
    P.counters = ctx->d_counters.get();
    P.error_flag = ctx->d_error.get();
    if (q.flags & RT_FLAG_GENERATIONS) P.gen_counts = ctx->d_gen_counts.get();
}

// The kernel a frame launch runs and its plan.
struct KernelChoice {
    LaunchShape ls;               // ls.id: the kernel's identity
    hipFunction_t jit = nullptr;  // the per-scene build of ls.id, or null: the generic kernel of the world's build ...
    bool sp = false;              // ... or of the spheres-and-planes build
};

// Step 3: the generic kernel's plan, then the per-scene build of the same
// kernel where the launch may take one and it has landed, else the
// spheres-and-planes build where the world allows it.
template <typename R>
int choose_kernel(rt_context* ctx, const DeviceWorld<R>& w, const LaunchRequest& q, uint32_t n_tiles, KernelChoice& k) {
    int rc;
    LaunchShape& ls = k.ls;
    KernelId id;
    id.family = q.shutter ? KernelFamily::shutter
                : q.lens  ? KernelFamily::lens
                : q.samples ? KernelFamily::supersampled
                            : KernelFamily::frame;
    // value-equal shapes (rt_scene_upload's identity classes) take the pool
    // kernel whose containers walk aggregates per class
    id.dup = ctx->duplicate_shapes > 0;
    if ((rc = plan_launch<R>(ctx, w.scene, q.depth, n_tiles, id, q.samples, false, ls))) return rc;
    // large f32 frames run the per-scene build of the same kernel (rtc_jit.cpp);
    // a direct one takes the shape records and materials from its instruction
    // stream and is planned with no LDS world (pool builds keep the LDS world:
    // rtc_jit.cpp make_request)
    if constexpr (sizeof(R) == 4) {
        // (the per-scene pool kernel keeps the stamps and item log: a stamped
        // launch times the kernel a warm renderer runs; the direct one has none)
        const uint32_t generic_only =
            RT_FLAG_NO_SHADE | RT_FLAG_NO_TRACE | RT_FLAG_GENERATIONS | (ls.id.pool ? 0u : RT_FLAG_STAMPS);
        // (a world with a triangle hierarchy runs the generic kernels, which walk it)
        const bool instanced = walked_instances(w), smooth = has_smooth(w);
        const bool tree = w.n_tri_nodes > 0 || instanced || smooth || has_textures(w) || w.moving;
        if (tree && ctx->jit.mode != RT_JIT_OFF && ctx->jit.log.empty())
            ctx->jit.log = w.moving ? "no per-scene build: the world has moving shapes, whose displaced points the generic kernels form"
                           : has_area(w) ? "no per-scene build: the world has area lights, which the generic kernels sample"
                           : has_textures(w) ? "no per-scene build: the world has textures, which the generic kernels sample"
                           : smooth ? "no per-scene build: the world has smooth triangles, whose normals the generic kernels interpolate"
                           : instanced
                               ? "no per-scene build: the world has mesh instances, which the generic kernels walk"
                               : "no per-scene build: the world has a triangle hierarchy, which the generic kernels walk";
        const bool want = q.cam && !id.dup && !tree && !(q.flags & generic_only) &&
                          (ctx->jit.mode == RT_JIT_SYNC || (ctx->jit.mode >= RT_JIT_AUTO && n_tiles >= kJitMinTiles));
        if (want) {
            ++ctx->jit.frames;
            LaunchShape lj = ls;
            if (ctx->knobs.lds_world && !ls.id.pool && w.scene.kind_begin[kNumKinds] <= kJitRecordsMaxShapes &&
                (rc = plan_launch<R>(ctx, w.scene, q.depth, n_tiles, id, q.samples, true, lj)))
                return rc;
            int waves = 0;
            if ((rc = jit_function(ctx, lj.id, lj.lds, lj.per_cu, &k.jit, (q.flags & RT_FLAG_NO_SKIPS) != 0, &waves)))
                return rc;
            if (k.jit && waves > 0 && (rc = plan_pool_for<R>(ctx, k.jit, lj))) return rc;
            if (k.jit) ls = lj;
        }
    }
    // Worlds of spheres and planes only run the pool kernel built without the
    // other kinds' loops (rtc_kernels_sp.o; same pixels).  Same-box A/B:
    // reflect_refract -2.8%, refraction -6.7%.  The direct kernel measured
    // slower that way (three_sphere +2.5%), so it keeps every kind.  Both pool
    // builds are capped at the same waves/SIMD and use the same LDS, so the
    // occupancy planned above holds.  RTC_DEBUG=kind_variants=0 disables.
    uint32_t kinds = 0;
    for (int kind = 0; kind < kNumKinds; ++kind)
        if (w.scene.kind_begin[kind + 1] > w.scene.kind_begin[kind]) kinds |= 1u << kind;
    // (supersampled launches: the all-kinds build only)
    k.sp = sizeof(R) == 4 && !k.jit && ls.id.family == KernelFamily::frame && ls.id.pool && !id.dup &&
           ctx->knobs.kind_variants && (kinds & ~kKindsSp) == 0 &&
           ctx->kernel_build == KernelBuild::plain;  // (the other builds' worlds hold triangles)
    return RT_OK;
}

// Step 4: the pool's spill regions, one per workgroup of the grid.
template <typename R>
int reserve_spill(rt_context* ctx, const LaunchShape& ls, LaunchParams<R>& P) {
    if (ls.cap <= ls.lcap) return RT_OK;
    const size_t per_block = (size_t)8 * (ls.cap - ls.lcap) * sizeof(R);
    if (int rc = ctx->d_spill.reserve((size_t)ls.grid * per_block)) return rc;
    P.spill = ctx->d_spill.get();
    P.spill_blocks = (uint32_t)(ctx->d_spill.capacity() / per_block);  // (of a buffer an earlier launch may have sized)
    return RT_OK;
}

// The tile order a family's launches keep (plan_tile_order).
inline rt_context::TileOrder& tile_order_of(rt_context* ctx, KernelFamily family) {
    return family == KernelFamily::shutter        ? ctx->order_shutter
           : family == KernelFamily::lens         ? ctx->order_lens
           : family == KernelFamily::supersampled ? ctx->order_ss
                                                  : ctx->order;
}

// Step 5 (pool launches only: the direct kernel reads no queue heads): the
// launch's set of queue heads and its tile order.
// Dynamic launches start from zeroed queue heads with no memset in
// between: two sets alternate, both zeroed at context creation, and each
// launch zeroes the other set for the next one (trace_pool; the
// previous user of that set is complete by stream order).
// The set flips only once the launch is enqueued (launch): a launch that fails
// before that leaves its set unused and still zero for the next one.
template <typename R>
int set_queue_heads(rt_context* ctx, const LaunchRequest& q, const LaunchShape& ls, LaunchParams<R>& P) {
    const size_t set = (size_t)kTileQueues * kQueueStride;
    P.tile_counter = ctx->d_tile_counter.get() + (ctx->head_set ? set : 0);
    P.next_tile_counter = ctx->d_tile_counter.get() + (ctx->head_set ? 0 : set);
    if (!ctx->knobs.tile_order || !q.cam) return RT_OK;  // frames only: a ray batch's content is not in the signature
    return plan_tile_order<R>(ctx, tile_order_of(ctx, ls.id.family), P, q.cam, q.depth, ls.grid, q.stream, q.lens, q.shutter);
}

// Step 6 (RT_FLAG_STAMPS): the workgroups' stamps and a pool launch's item log, reserved behind the tile order.
template <typename R>
int reserve_stamps(rt_context* ctx, const LaunchShape& ls, hipStream_t stream, LaunchParams<R>& P) {
    int rc;
    if ((rc = ctx->d_stamps.reserve((size_t)2 * ls.grid))) return rc;
    P.stamps = ctx->d_stamps.get();
    ctx->stamp_count = ls.grid;
    if (ls.id.pool) {  // every item of the launch: up to 2^kMaxSplitLog2 per tile
        const size_t items = (size_t)P.n_tiles << kMaxSplitLog2;
        if ((rc = ctx->d_item_log.reserve(1 + 3 * items))) return rc;
        RT_HIP(hipMemsetAsync(ctx->d_item_log.get(), 0, sizeof(uint64_t), stream));
        P.item_log = ctx->d_item_log.get();
    }
    return RT_OK;
}

// The launches that read the launch terms and the cull tables: camera frames
// of the per-scene f32 direct kernel, not supersampled (those take no primary
// cull: the tables stay zero), of a world of at most kPrimaryRectSlots slots
// whose records the per-scene tables hold.
inline bool reads_launch_tables(const rt_context* ctx, const DeviceWorld<float>& w, const LaunchRequest& q,
                                const KernelChoice& k) {
    const size_t ns = ctx->jit.shapes.size();
    return k.jit && k.ls.id.family == KernelFamily::frame && !k.ls.id.pool && q.cam && ns <= (size_t)kPrimaryRectSlots &&
           (int)ns == w.scene.kind_begin[kNumKinds];
}

// Step 7: the per-scene direct kernel's launch terms (launch_terms.hpp): what
// its shape tests form from the origin alone, from the same f32 records, for
// any canvas (a few dozen f32 operations per slot); and, for a canvas within
// them, its cull tables (cull_tables.hpp).
inline void fill_launch_tables(const rt_context* ctx, const DeviceWorld<float>& w, LaunchParams<float>& P) {
    const std::vector<ShapeRec<float>>& shapes = ctx->jit.shapes;
    launch_terms(shapes.data(), w.scene.kind_begin, (int)shapes.size(), P.cam.origin, P.terms);
    if (!cull_tables_hold(P.width, P.height)) return;
    // (the shadow bits speak of the lights the kernel holds as constants: none unless those are the world's)
    const std::vector<LightRec<float>>& lights = ctx->jit.lights;
    const int n_lights = (int)lights.size() == w.scene.n_lights ? (int)lights.size() : 0;
    fill_cull_tables(P.cam, P.width, P.height, shapes.data(), shapes.size(), w.scene.kind_begin, lights.data(), n_lights,
                     P.terms, P.cull_cols, P.cull_rows);
}

// Step 8: the launch itself, of the per-scene function or of the generic
// kernel of the world's build (or of the spheres-and-planes build).
template <typename R>
int dispatch(rt_context* ctx, const DeviceWorld<R>& w, const KernelChoice& k, const LaunchParams<R>& P,
             const ShutterArg<R>& frame_arg, hipStream_t stream) {
    const LensParams<R>& lens_params = frame_arg.lens;
    const LaunchShape& ls = k.ls;
    if (k.jit) {
        const ShapeRec<R>* sh = P.scene.shapes;
        const MaterialRec<R>* mt = P.scene.materials;
        const PatternRec<R>* pt = P.scene.patterns;
        const LightRec<R>* lt = P.scene.lights;
        void* args[] = {const_cast<LaunchParams<R>*>(&P), &sh, &mt, &pt, &lt,
                        const_cast<LensParams<R>*>(&lens_params)};  // (the last: read by the lens kernels only)
        (void)hipGetLastError();
        RT_HIP(hipModuleLaunchKernel(k.jit, ls.grid, 1, 1, kBlock, 1, 1, (unsigned)ls.lds, stream, args, nullptr));
        return RT_OK;
    }
    auto launch_kernel = launchers<R>(ctx).launch_kernel;
    if constexpr (sizeof(R) == 4)
        if (k.sp) launch_kernel = sp::launch_kernel<R>;
    // (the lens is the frame argument's first member: the lens kernels read it there, the shutter kernels the whole;
    // the motion build takes the velocity tables in front of it)
    const MotionLaunch ml{motion_arg(w), &frame_arg};
    const void* extra = ctx->kernel_build == KernelBuild::moving ? static_cast<const void*>(&ml) : &frame_arg;
    if (hipError_t e = launch_kernel(ls.id, P, extra, ls.grid, ls.lds, stream); e != hipSuccess)
        return set_error(RT_ERR_HIP, std::string("launch of the ") + ls.id.describe() + " kernel (grid " +
                                         std::to_string(ls.grid) + ", dynamic LDS " + std::to_string(ls.lds) +
                                         " B, pool " + std::to_string(ls.lcap) + "/" + std::to_string(ls.cap) +
                                         " rays in LDS): " + hipGetErrorString(e));
    return RT_OK;
}

template <typename R>
int launch(rt_context* ctx, DeviceWorld<R>& w, const LaunchRequest& q) {
    int rc;
    LaunchParams<R> P{};
    ShutterArg<R> frame_arg{};  // a lens or shutter launch's last kernel argument: the lens, then the shutter
    set_world_params(ctx, w, P);
    set_target_params(ctx, q, P, frame_arg);
    if (P.n_tiles == 0) return RT_OK;
    if ((rc = order_after_last(ctx, q.stream))) return rc;
    KernelChoice k;
    if ((rc = choose_kernel(ctx, w, q, P.n_tiles, k))) return rc;
    const LaunchShape& ls = k.ls;
    ctx->jit.used = k.jit != nullptr;
    P.pool_capacity = ls.cap;
    P.pool_lds_capacity = ls.lcap;
    P.pop_batch = ls.batch;
    if (ls.id.pool && (rc = check_pixel_range(ctx, q.depth, sizeof(R) == 4))) return rc;
    P.acc_log2 = acc_shift_f32(ctx->bright_hit, ctx->bright_w, q.depth);
    if ((rc = reserve_spill(ctx, ls, P))) return rc;
    P.persistent = ls.sched;
    P.flags = q.flags;
    P.world_lds = ls.world_lds;
    if (ls.id.pool && (rc = set_queue_heads(ctx, q, ls, P))) return rc;
    if ((q.flags & RT_FLAG_STAMPS) && (rc = reserve_stamps(ctx, ls, q.stream, P))) return rc;
    if (q.flags & RT_FLAG_FAIL_LAUNCH) return set_error(RT_ERR_HIP, "launch refused (RT_FLAG_FAIL_LAUNCH)");
    if constexpr (sizeof(R) == 4)
        if (reads_launch_tables(ctx, w, q, k)) fill_launch_tables(ctx, w, P);
    if ((rc = dispatch(ctx, w, k, P, frame_arg, q.stream))) return rc;
    if (ls.id.pool) ctx->head_set ^= 1;  // (the queue heads' set: see set_queue_heads)
    ctx->smooth_info.ran_smooth = !k.jit && has_smooth(w) ? 1u : 0u;
    ctx->texture_info.ran_textured = !k.jit && has_textures(w) ? 1u : 0u;
    ctx->map_info.ran_mapped = ctx->texture_info.ran_textured && ctx->kernel_build == KernelBuild::mapped ? 1u : 0u;
    ctx->light_info.ran_area = !k.jit && has_area(w) ? 1u : 0u;
    ctx->motion_info.ran_motion = ls.id.family == KernelFamily::shutter ? 1u : 0u;
    return RT_OK;
}

// A ray batch's launch: the world in LDS as for the other kernels, no pool
// (cap = the per-lane LIFO's entries, none of them in LDS), a resident grid
// striding over the batch's chunks of kBlock rays.
template <typename R>
int plan_rays(rt_context* ctx, const DevScene<R>& sc, uint32_t depth, uint32_t n_chunks, KernelId id, LaunchShape& ls) {
    const size_t wb = world_lds_bytes<R>(sc.kind_begin[kNumKinds], sc.n_materials, sc.n_patterns);
    ls.world_lds = (ctx->knobs.lds_world && wb <= kMaxWorldLds) ? (uint32_t)wb : 0;
    id.lds = ls.world_lds != 0;
    ls.id = id;
    ls.lds = ls.world_lds;
    ls.cap = ray_stack_entries(depth);
    ls.lcap = ls.batch = 0;
    ls.sched = kSchedStatic;
    int per_cu = 0, rc;
    if ((rc = blocks_per_cu<R>(ctx, id, ls.lds, &per_cu))) return rc;
    ls.per_cu = std::max(per_cu, 1);
    const uint64_t resident = (uint64_t)ls.per_cu * (uint64_t)ctx->cu_count;
    ls.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_chunks, resident));
    ls.grid_tiles = n_chunks;
    return RT_OK;
}

// One ray batch (rt_trace_rays*): n rays of R at d_rays -> RGB of R at d_rgb
// and, if d_hits, the primary hits, on `stream`.  No range check of the
// world and none of the directions: trace_rays sums per lane in plain R.
template <typename R>
int launch_rays(rt_context* ctx, DeviceWorld<R>& w, const void* d_rays, const void* d_times, uint64_t n,
                const rt_ray_options* o, void* d_rgb, void* d_hits, hipStream_t stream) {
    int rc;
    LaunchParams<R> P{};
    set_world_params(ctx, w, P);
    P.n_rays = n;
    P.n_tiles = (uint32_t)((n + kBlock - 1) / kBlock);
    P.max_depth = o->max_depth;
    P.flags = o->flags;
    P.counters = ctx->d_counters.get();
    P.error_flag = ctx->d_error.get();
    if (o->flags & RT_FLAG_GENERATIONS) P.gen_counts = ctx->d_gen_counts.get();
    if ((rc = order_after_last(ctx, stream))) return rc;
    LaunchShape ls;
    KernelId id;
    id.family = KernelFamily::rays;
    id.dup = ctx->duplicate_shapes > 0;
    if ((rc = plan_rays<R>(ctx, w.scene, o->max_depth, P.n_tiles, id, ls))) return rc;
    P.pool_capacity = ls.cap;
    P.persistent = ls.sched;
    P.world_lds = ls.world_lds;
    if (ls.cap) {
        // the lanes' LIFOs share the pool's spill buffer: launches are ordered
        // (order_after_last), so it has one user at a time
        const size_t per_block = ray_stack_word(1, ls.cap, 0, 0) * sizeof(R);
        if ((rc = ctx->d_spill.reserve((size_t)ls.grid * per_block))) return rc;
        P.spill = ctx->d_spill.get();
        P.spill_blocks = (uint32_t)std::min<size_t>(ctx->d_spill.capacity() / per_block, 0xFFFFFFFFu);
    }
    ctx->jit.used = false;
    if (o->flags & RT_FLAG_FAIL_LAUNCH) return set_error(RT_ERR_HIP, "launch refused (RT_FLAG_FAIL_LAUNCH)");
    // (a static world has no mover for a time to displace: its batch runs as it always did, whatever the times)
    const RayBatchTimedArg batch{{d_rays, d_rgb, d_hits}, d_times};
    const MotionLaunch ml{motion_arg(w), &batch};
    const void* extra = ctx->kernel_build == KernelBuild::moving ? static_cast<const void*>(&ml) : &batch.batch;
    if (hipError_t e = launchers<R>(ctx).launch_kernel(ls.id, P, extra, ls.grid, ls.lds, stream); e != hipSuccess)
        return set_error(RT_ERR_HIP, std::string("launch of the ") + ls.id.describe() + " kernel (grid " +
                                         std::to_string(ls.grid) + ", dynamic LDS " + std::to_string(ls.lds) + " B, " +
                                         std::to_string(ls.cap) + " stack entries per lane): " + hipGetErrorString(e));
    ctx->smooth_info.ran_smooth = has_smooth(w) ? 1u : 0u;
    ctx->texture_info.ran_textured = has_textures(w) ? 1u : 0u;
    ctx->map_info.ran_mapped = ctx->texture_info.ran_textured && ctx->kernel_build == KernelBuild::mapped ? 1u : 0u;
    ctx->light_info.ran_area = has_area(w) ? 1u : 0u;
    ctx->motion_info.ran_motion = d_times && w.moving ? 1u : 0u;
    return RT_OK;
}

int check_ray_options(const rt_ray_options* o) {
    if (!o) return set_error(RT_ERR_INVALID, "null options");
    if (o->precision > RT_PRECISION_F64) return set_error(RT_ERR_INVALID, "unknown precision");
    if (o->max_depth > RT_MAX_SUPPORTED_DEPTH) return set_error(RT_ERR_INVALID, "max_depth above RT_MAX_SUPPORTED_DEPTH");
    constexpr uint32_t kRayFlags = RT_FLAG_NO_COUNTERS | RT_FLAG_FAIL_LAUNCH | RT_FLAG_GENERATIONS | RT_FLAG_NO_SKIPS;
    if (o->flags & ~kRayFlags) return set_error(RT_ERR_INVALID, "flag not supported by ray batches");
    return RT_OK;
}

int launch_rays_precision(rt_context* ctx, const void* d_rays, const void* d_times, uint64_t n, const rt_ray_options* o,
                          void* d_rgb, void* d_hits, hipStream_t stream) {
    return o->precision == RT_PRECISION_F32
               ? launch_rays<float>(ctx, ctx->w32, d_rays, d_times, n, o, d_rgb, d_hits, stream)
               : launch_rays<double>(ctx, ctx->w64, d_rays, d_times, n, o, d_rgb, d_hits, stream);
}

InitTrace::InitTrace(const char* what) : what_(what), on_(debug_knob("trace_init", nullptr)) {
    t0_ = t_ = std::chrono::steady_clock::now();
}
void InitTrace::step(const char* name) {
    if (!on_) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[rtc init] %s: %s %.3f ms (%.3f ms total)\n", what_, name,
                 std::chrono::duration<double, std::milli>(now - t_).count(),
                 std::chrono::duration<double, std::milli>(now - t0_).count());
    t_ = now;
}

int check_ready(rt_context* ctx) {
    if (!ctx) return set_error(RT_ERR_INVALID, "null context");
    if (!ctx->have_scene) return set_error(RT_ERR_NO_SCENE, "render before rt_scene_upload");
    return RT_OK;
}

int check_options(const rt_render_options* o) {
    if (!o) return set_error(RT_ERR_INVALID, "null options");
    if (o->precision > RT_PRECISION_F64) return set_error(RT_ERR_INVALID, "unknown precision");
    if (o->out_format > RT_OUT_U8) return set_error(RT_ERR_INVALID, "unknown output format");
    if (o->max_depth > RT_MAX_SUPPORTED_DEPTH) return set_error(RT_ERR_INVALID, "max_depth above RT_MAX_SUPPORTED_DEPTH");
    if (o->shard_count == 0 || o->shard_index >= o->shard_count) return set_error(RT_ERR_INVALID, "bad shard");
    return RT_OK;
}

void sum_counter_shards(const unsigned long long* shards, unsigned long long out[kNumCounters]) {
    for (int i = 0; i < kNumCounters; ++i) out[i] = 0;
    for (int s = 0; s < kCounterShards; ++s)
        for (int i = 0; i < kNumCounters; ++i) out[i] += shards[(size_t)s * kNumCounters + i];
}

int read_counters(rt_context* ctx, unsigned long long out[kNumCounters]) {
    std::vector<unsigned long long> shards((size_t)kCounterShards * kNumCounters);
    RT_HIP(hipMemcpy(shards.data(), ctx->d_counters.get(), shards.size() * sizeof(unsigned long long),
                     hipMemcpyDeviceToHost));
    sum_counter_shards(shards.data(), out);
    return RT_OK;
}

void fill_stats(rt_context* ctx, const unsigned long long before[kNumCounters],
                const unsigned long long after[kNumCounters], float ms, rt_stats* s) {
    uint64_t d[kNumCounters];
    for (int i = 0; i < kNumCounters; ++i) d[i] = after[i] - before[i];
    s->primary = d[0];
    s->shadow = d[1];
    s->reflect = d[2];
    s->refract = d[3];
    s->shaded = d[4];
    s->lit_patterned = d[5];
    s->refract_evals = d[6];
    s->schlick_evals = d[7];
    s->kernel_ms = ms;
    s->algorithmic_flops = algorithmic_flops(ctx->flops, *s);
    s->gather_ms = 0.0;
    s->frame_ms = ms;
    s->n_shards = 1;
    s->reserved = 0;
}

// Device scratch -> the caller's host buffer, enqueued on ctx->stream after
// the render.  A pageable hipMemcpyAsync runs at the PCIe rate here (the
// runtime pipelines its own pinned staging): measured on MI355X for a 1080p
// f32 frame (24.9 MB) into a canvas kept across frames, 0.52 ms per whole
// rt_render call; a pinned staging buffer copied out by 4 host threads as
// each of 8 DMA chunks landed took 0.71 ms (scripts/host_frame_probe.py).
// A canvas allocated per call pays its page faults on top (~0.3 ms at 1080p).
int copy_to_host(rt_context* ctx, void* out, size_t bytes) {
    RT_HIP(hipMemcpyAsync(out, ctx->d_scratch.get(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    return RT_OK;
}

int check_pool_error(rt_context* ctx) {
    int32_t err = 0;
    RT_HIP(hipMemcpyAsync(&err, ctx->d_error.get(), sizeof(err), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    if (err) {
        RT_HIP(hipMemsetAsync(ctx->d_error.get(), 0, sizeof(int32_t), ctx->stream));
        return set_error(RT_ERR_POOL, device_error_text(err));
    }
    return RT_OK;
}

}  // namespace rtc

using namespace rtc;

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

const char* rt_last_error(void) { return rtc::g_error.c_str(); }

int rt_device_count(int* count) {
    if (!count) return set_error(RT_ERR_INVALID, "null count");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return RT_OK;
}

int rt_context_create(int device_ordinal, rt_context** out) { return create_device_context(device_ordinal, out); }

int rt_context_destroy(rt_context* ctx) {
    if (!ctx) return RT_OK;
    for (rt_context* p : ctx->group.peers) destroy_device_context(p);
    destroy_device_context(ctx);
    return RT_OK;
}

}  // extern "C"

namespace rtc {

// A/B and diagnostic switches (debug_knobs.hpp: RTC_DEBUG=key=value,...)
rt_context::Knobs read_knobs() {
    rt_context::Knobs k;
    std::string v;
    // direct-kernel tile scheduling: "grid" (one workgroup per tile, the
    // hardware dispatcher balances) or "static" (resident grid, fixed stride)
    if (debug_knob("sched_direct", &v)) {
        if (v == "grid") k.sched_direct = kSchedGrid;
        else if (v == "static") k.sched_direct = kSchedStatic;
    }
    if (debug_knob("lds_world", &v)) k.lds_world = v != "0";
    if (debug_knob("cull", &v)) k.cull = v != "0";
    if (debug_knob("tri_tree", &v)) k.tri_tree = v != "0";
    if (debug_knob("area_cull", &v)) k.area_cull = v != "0";
    if (debug_knob("tri_min", &v)) k.tri_min = (uint32_t)std::max(0, std::atoi(v.c_str()));
    if (debug_knob("tri_leaf", &v)) k.tri_leaf = (uint32_t)std::max(0, std::atoi(v.c_str()));
    if (debug_knob("kind_variants", &v)) k.kind_variants = v != "0";
    if (debug_knob("pool_lds_rays", &v)) k.pool_lds_rays = (uint32_t)std::atoi(v.c_str());
    if (debug_knob("tile_order", &v)) k.tile_order = v != "0";
    if (debug_knob("split", &v)) k.split_factor = std::atof(v.c_str());
    if (debug_knob("split_max", &v))
        k.split_max = (uint32_t)std::min<int>((int)kMaxSplitLog2, std::max(0, std::atoi(v.c_str())));
    if (debug_knob("urgent", &v)) k.urgent_factor = std::atof(v.c_str());
    if (debug_knob("direct_oversub", &v)) k.direct_oversub10 = (uint32_t)std::max(1, std::atoi(v.c_str()));
    return k;
}

int create_device_context(int device_ordinal, rt_context** out) {
    if (!out) return set_error(RT_ERR_INVALID, "null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return set_error(RT_ERR_NO_DEVICE, "no HIP device available (the render path has no CPU fallback)");
    if (device_ordinal < 0 || device_ordinal >= n) return set_error(RT_ERR_INVALID, "device ordinal out of range");
    // RTC_DEBUG=trace_init=1: milliseconds of each step of context creation on
    // stderr (the one-shot render's breakdown)
    InitTrace tr("context");
    auto ctx = std::make_unique<rt_context>();
    ctx->device = device_ordinal;
    RT_HIP(hipSetDevice(device_ordinal));
    tr.step("hipSetDevice");
    // two attributes instead of hipGetDeviceProperties (which fills every
    // field of the struct); the gfx target for the per-scene builds is read
    // when the first build needs it (device_arch, rtc_jit.cpp)
    int cus = 0, lds = 0;
    RT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_ordinal));
    RT_HIP(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device_ordinal));
    tr.step("hipDeviceGetAttribute x2");
    ctx->cu_count = cus;
    ctx->lds_per_block = (size_t)lds;  // launch limit of static + dynamic LDS
    ctx->knobs = read_knobs();
    // RTC_JIT: the per-scene build mode (rt_context_set_jit's values), a user setting
    if (const char* e = std::getenv("RTC_JIT"))
        ctx->jit.mode = (e[0] >= '0' && e[0] <= '3' && !e[1]) ? e[0] - '0' : RT_JIT_AUTO;
    int rc;
    if ((rc = ctx->stream.create(hipStreamNonBlocking))) return rc;
    tr.step("hipStreamCreate");
    if ((rc = ctx->ev_start.create()) || (rc = ctx->ev_stop.create()) ||
        (rc = ctx->ev_order.create(hipEventDisableTiming)))
        return rc;
    tr.step("hipEventCreate x3");
    const size_t heads = 2 * (size_t)kTileQueues * kQueueStride;  // two sets
    if ((rc = ctx->d_tile_counter.reserve(heads))) return rc;
    tr.step("hipMalloc");
    // (on the context's stream: the null stream's queue would cost ~8 ms more)
    RT_HIP(hipMemsetAsync(ctx->d_tile_counter.get(), 0, heads * sizeof(unsigned long long), ctx->stream));
    tr.step("hipMemsetAsync (first)");
    const size_t n_counters = (size_t)kCounterShards * kNumCounters, n_gen = 2 * (size_t)kGenSlots;
    if ((rc = ctx->d_counters.reserve(n_counters)) || (rc = ctx->d_error.reserve(1)) ||
        (rc = ctx->d_gen_counts.reserve(n_gen)))
        return rc;
    RT_HIP(hipMemsetAsync(ctx->d_counters.get(), 0, n_counters * sizeof(unsigned long long), ctx->stream));
    RT_HIP(hipMemsetAsync(ctx->d_error.get(), 0, sizeof(int32_t), ctx->stream));
    RT_HIP(hipMemsetAsync(ctx->d_gen_counts.get(), 0, n_gen * sizeof(unsigned long long), ctx->stream));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    tr.step("hipMalloc+hipMemsetAsync x3, sync");
    *out = ctx.release();
    return RT_OK;
}

void destroy_device_context(rt_context* ctx) { delete ctx; }

}  // namespace rtc

rt_context::~rt_context() {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();  // launches on caller streams too
    for (auto& c : canvases) {
        if (c.second.owned) (void)hipFree(c.first);
        else (void)hipIpcCloseMemHandle(c.first);
    }
    if (group.comm) (void)ncclCommDestroy(group.comm);
}

// Every rt_scene_upload* entry point after it has filled `in`: the lists are checked before the context is
// looked at (rtc.h), except that a group's rank 0 checks its own (group_scene_upload) -- unless image patterns
// are known, which are rewritten here and so are checked here on every rank.
static int upload_world(rt_context* ctx, const WorldLists& in) {
    const bool group = ctx && ctx->group.comm;
    if (!group || in.image_patterns)
        if (int rc = validate_scene(in)) return rc;
    if (!ctx) return set_error(RT_ERR_INVALID, "null context");
    WorldLists wl = in;
    // (a velocity of zero in every component, +0 or -0, is no motion: that shape is static)
    std::vector<rt_motion_desc> movers;
    for (uint32_t m = 0; m < in.n_motion && in.motion; ++m)
        if (in.motion[m].velocity[0] != 0.0 || in.motion[m].velocity[1] != 0.0 || in.motion[m].velocity[2] != 0.0)
            movers.push_back(in.motion[m]);
    wl.motion = movers.data();
    wl.n_motion = (uint32_t)movers.size();
    if (group && wl.n_motion && ctx->group.n_ranks > 1)
        return set_error(RT_ERR_INVALID, "a moving world is uploaded to one device: a group of " +
                                             std::to_string(ctx->group.n_ranks) + " ranks shares no velocity tables");
    // (patterns compare by their textures' contents: a copy with every image pattern's texture renumbered)
    std::vector<rt_pattern_desc> cp;
    std::vector<int32_t> records;  // (a cube map's faces: more records of the device texture table)
    if (wl.image_patterns) {
        cp.assign(wl.patterns, wl.patterns + wl.n_patterns);
        inst::canonical_image_patterns(cp.data(), wl.n_patterns, wl.textures, wl.n_textures, wl.maps, wl.n_maps, &records);
        wl.patterns = cp.data();
        wl.tex_records = records.data();
        wl.n_tex_records = (uint32_t)records.size();
    }
    if (group) return group_scene_upload(ctx, wl);
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipDeviceSynchronize());  // launches on caller streams may still read the old tables
    return build_scene(ctx, wl);
}

// rt_smooth_expand and rt_uv_expand: the side list of the expansion.
template <typename Side>
static int expand_side_list(const WorldLists& wl, const typename Side::Desc* list, uint32_t n_list,
                            typename Side::Desc* out, uint32_t* n_out) {
    // (materials are the upload's to check: any index passes here)
    std::string why = inst::validate(wl.shapes, wl.n_shapes, wl.meshes, wl.n_meshes, wl.instances, wl.n_instances, 0x7FFFFFFFu);
    if (why.empty()) why = inst::validate_side<Side>(wl.shapes, wl.n_shapes, wl.meshes, wl.n_meshes, list, n_list);
    if (!why.empty()) return set_error(RT_ERR_INVALID, why);
    const uint32_t n = inst::expand_side<Side>(wl.n_shapes, wl.meshes, wl.n_meshes, wl.instances, wl.n_instances, list, n_list, out);
    if (n_out) *n_out = n;
    return RT_OK;
}

extern "C" {

int rt_scene_upload(rt_context* ctx, const rt_shape_desc* shapes, uint32_t ns, const rt_material_desc* mats,
                    uint32_t nm, const rt_pattern_desc* pats, uint32_t np, const rt_light_desc* lights,
                    uint32_t nl) {
    if (!ctx) return set_error(RT_ERR_INVALID, "null context");  // (this entry point looks at the context first)
    return upload_world(ctx, WorldLists{shapes, ns, mats, nm, pats, np, lights, nl});
}

int rt_scene_upload_instanced(rt_context* ctx, const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes,
                              uint32_t n_meshes, const rt_instance_desc* instances, uint32_t n_inst,
                              const rt_material_desc* mats, uint32_t nm, const rt_pattern_desc* pats, uint32_t np,
                              const rt_light_desc* lights, uint32_t nl) {
    return upload_world(ctx, WorldLists{shapes, ns, mats, nm, pats, np, lights, nl, meshes, n_meshes, instances, n_inst});
}

int rt_scene_upload_smooth(rt_context* ctx, const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes,
                           uint32_t n_meshes, const rt_instance_desc* instances, uint32_t n_inst,
                           const rt_smooth_desc* smooth, uint32_t n_smooth, const rt_material_desc* mats, uint32_t nm,
                           const rt_pattern_desc* pats, uint32_t np, const rt_light_desc* lights, uint32_t nl) {
    return upload_world(ctx, WorldLists{shapes, ns, mats, nm, pats, np, lights, nl, meshes, n_meshes, instances, n_inst,
                                        smooth, n_smooth});
}

int rt_scene_upload_textured(rt_context* ctx, const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes,
                             uint32_t n_meshes, const rt_instance_desc* instances, uint32_t n_inst,
                             const rt_smooth_desc* smooth, uint32_t n_smooth, const rt_uv_desc* uvs, uint32_t n_uvs,
                             const rt_texture_desc* textures, uint32_t n_textures, const rt_material_desc* mats,
                             uint32_t nm, const rt_pattern_desc* pats, uint32_t np, const rt_light_desc* lights,
                             uint32_t nl) {
    return upload_world(ctx, WorldLists{shapes, ns, mats, nm, pats, np, lights, nl, meshes, n_meshes, instances, n_inst,
                                        smooth, n_smooth, uvs, n_uvs, textures, n_textures, nullptr, 0, true});
}

int rt_scene_upload_lit(rt_context* ctx, const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes,
                        uint32_t n_meshes, const rt_instance_desc* instances, uint32_t n_inst,
                        const rt_smooth_desc* smooth, uint32_t n_smooth, const rt_uv_desc* uvs, uint32_t n_uvs,
                        const rt_texture_desc* textures, uint32_t n_textures, const rt_material_desc* mats, uint32_t nm,
                        const rt_pattern_desc* pats, uint32_t np, const rt_light_desc* lights, uint32_t nl,
                        const rt_area_light_desc* area, uint32_t n_area) {
    return upload_world(ctx, WorldLists{shapes, ns, mats, nm, pats, np, lights, nl, meshes, n_meshes, instances, n_inst,
                                        smooth, n_smooth, uvs, n_uvs, textures, n_textures, area, n_area, true});
}

int rt_scene_upload_mapped(rt_context* ctx, const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes,
                           uint32_t n_meshes, const rt_instance_desc* instances, uint32_t n_inst,
                           const rt_smooth_desc* smooth, uint32_t n_smooth, const rt_uv_desc* uvs, uint32_t n_uvs,
                           const rt_texture_desc* textures, uint32_t n_textures, const rt_material_desc* mats, uint32_t nm,
                           const rt_pattern_desc* pats, uint32_t np, const rt_light_desc* lights, uint32_t nl,
                           const rt_area_light_desc* area, uint32_t n_area, const rt_uv_map_desc* maps, uint32_t n_maps) {
    WorldLists wl{shapes, ns, mats, nm, pats, np, lights, nl, meshes, n_meshes, instances, n_inst,
                  smooth, n_smooth, uvs, n_uvs, textures, n_textures, area, n_area, true};
    wl.maps = maps;
    wl.n_maps = n_maps;
    return upload_world(ctx, wl);
}

int rt_scene_upload_moving(rt_context* ctx, const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes,
                           uint32_t n_meshes, const rt_instance_desc* instances, uint32_t n_inst,
                           const rt_smooth_desc* smooth, uint32_t n_smooth, const rt_uv_desc* uvs, uint32_t n_uvs,
                           const rt_texture_desc* textures, uint32_t n_textures, const rt_material_desc* mats, uint32_t nm,
                           const rt_pattern_desc* pats, uint32_t np, const rt_light_desc* lights, uint32_t nl,
                           const rt_area_light_desc* area, uint32_t n_area, const rt_uv_map_desc* maps, uint32_t n_maps,
                           const rt_motion_desc* motion, uint32_t n_motion) {
    WorldLists wl{shapes, ns, mats, nm, pats, np, lights, nl, meshes, n_meshes, instances, n_inst,
                  smooth, n_smooth, uvs, n_uvs, textures, n_textures, area, n_area, true};
    wl.maps = maps;
    wl.n_maps = n_maps;
    wl.motion = motion;
    wl.n_motion = n_motion;
    return upload_world(ctx, wl);
}

int rt_scene_motion_info(rt_context* ctx, rt_motion_info* out) {
    if (!ctx || !out) return set_error(RT_ERR_INVALID, "null argument");
    *out = ctx->have_scene ? ctx->motion_info : rt_motion_info{};
    return RT_OK;
}

int rt_motion_displace(const rt_shape_desc* shapes, uint32_t ns, const rt_instance_desc* instances, uint32_t n_inst,
                       const rt_motion_desc* motion, uint32_t n_motion, double tau, rt_shape_desc* out_shapes,
                       rt_instance_desc* out_instances) {
    if ((ns && (!shapes || !out_shapes)) || (n_inst && (!instances || !out_instances)) || (n_motion && !motion))
        return set_error(RT_ERR_INVALID, "rt_motion_displace: null list with nonzero count");
    if (!std::isfinite(tau)) return set_error(RT_ERR_INVALID, "rt_motion_displace: a time that is not finite");
    for (uint32_t m = 0; m < n_motion; ++m) {
        if (motion[m].target != RT_MOVE_SHAPE && motion[m].target != RT_MOVE_INSTANCE)
            return set_error(RT_ERR_INVALID, "motion " + std::to_string(m) + ": unknown target");
        if (motion[m].index >= (motion[m].target == RT_MOVE_SHAPE ? ns : n_inst))
            return set_error(RT_ERR_INVALID, "motion " + std::to_string(m) + ": index out of range");
    }
    for (uint32_t i = 0; i < ns; ++i)
        if (out_shapes + i != shapes + i) out_shapes[i] = shapes[i];
    for (uint32_t k = 0; k < n_inst; ++k)
        if (out_instances + k != instances + k) out_instances[k] = instances[k];
    for (uint32_t m = 0; m < n_motion; ++m) {
        const rt_motion_desc& d = motion[m];
        // (a static target, and every target at tau = 0, keeps the input's inverse bit for bit)
        if ((d.velocity[0] == 0.0 && d.velocity[1] == 0.0 && d.velocity[2] == 0.0) || tau == 0.0) continue;
        double* inv = d.target == RT_MOVE_SHAPE ? out_shapes[d.index].inverse : out_instances[d.index].inverse;
        // inverse * translation(-v tau) as matrix.rs multiplies: each element the left fold over the row and the
        // column; only the translation's last column differs from the identity's
        const double t[3] = {-(d.velocity[0] * tau), -(d.velocity[1] * tau), -(d.velocity[2] * tau)};
        hm::M4 a, b = hm::identity();
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) a.m[r][c] = inv[4 * r + c];
        for (int r = 0; r < 3; ++r) b.m[r][3] = t[r];
        const hm::M4 p = hm::mul(a, b);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) inv[4 * r + c] = p.m[r][c];
    }
    return RT_OK;
}

int rt_smooth_expand(const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes, uint32_t n_meshes,
                     const rt_instance_desc* instances, uint32_t n_inst, const rt_smooth_desc* smooth, uint32_t n_smooth,
                     rt_smooth_desc* out, uint32_t* n_out) {
    const WorldLists wl{.shapes = shapes, .n_shapes = ns, .meshes = meshes, .n_meshes = n_meshes, .instances = instances,
                        .n_instances = n_inst};
    return expand_side_list<inst::SmoothSide>(wl, smooth, n_smooth, out, n_out);
}

int rt_uv_expand(const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes, uint32_t n_meshes,
                 const rt_instance_desc* instances, uint32_t n_inst, const rt_uv_desc* uvs, uint32_t n_uvs,
                 rt_uv_desc* out, uint32_t* n_out) {
    const WorldLists wl{.shapes = shapes, .n_shapes = ns, .meshes = meshes, .n_meshes = n_meshes, .instances = instances,
                        .n_instances = n_inst};
    return expand_side_list<inst::UVSide>(wl, uvs, n_uvs, out, n_out);
}

int rt_scene_texture_info(rt_context* ctx, rt_texture_info* out) {
    if (!ctx || !out) return set_error(RT_ERR_INVALID, "null argument");
    *out = ctx->have_scene ? ctx->texture_info : rt_texture_info{};
    return RT_OK;
}

int rt_scene_map_info(rt_context* ctx, rt_map_info* out) {
    if (!ctx || !out) return set_error(RT_ERR_INVALID, "null argument");
    *out = ctx->have_scene ? ctx->map_info : rt_map_info{};
    return RT_OK;
}

static uint32_t area_mix(uint32_t x) {  // rtc.h "Hashed jitter"
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// Sample k of a valid light, in f64 (the kernels' arithmetic in R = double).
static void area_sample(const rt_area_light_desc& d, uint32_t area_index, uint32_t ray_id, uint32_t remaining, uint32_t k,
                        double pos[3]) {
    const uint32_t i = k % d.usteps, j = k / d.usteps;
    double ju = 0.5, jv = 0.5;
    if (d.jitter == RT_JITTER_HASHED) {
        const uint32_t key = area_mix(area_mix(area_mix(d.seed ^ ray_id) ^ remaining) ^ ((area_index << 8) | k));
        ju = (double)(key >> 8) * 0x1p-24;
        jv = (double)(area_mix(key ^ 0x9E3779B9u) >> 8) * 0x1p-24;
    }
    const double fu = (double)i + ju, fv = (double)j + jv;
    for (int q = 0; q < 3; ++q) {
        const double u = d.full_uvec[q] / (double)d.usteps, v = d.full_vvec[q] / (double)d.vsteps;
        pos[q] = (d.corner[q] + u * fu) + v * fv;
    }
}

int rt_area_light_sample(const rt_area_light_desc* desc, uint32_t area_index, uint32_t ray_id, uint32_t remaining,
                         uint32_t k, double pos[3]) {
    if (!desc || !pos) return set_error(RT_ERR_INVALID, "null argument");
    const std::string why = validate_area(desc, 1);
    if (!why.empty()) return set_error(RT_ERR_INVALID, why);
    if (k >= desc->usteps * desc->vsteps) return set_error(RT_ERR_INVALID, "rt_area_light_sample: sample index out of range");
    area_sample(*desc, area_index, ray_id, remaining, k, pos);
    return RT_OK;
}

int rt_lights_expand(const rt_light_desc* lights, uint32_t nl, const rt_area_light_desc* area, uint32_t n_area,
                     rt_light_desc* out, uint32_t* n_out) {
    if (nl && !lights) return set_error(RT_ERR_INVALID, "rt_lights_expand: null light list with nonzero count");
    const std::string why = validate_area(area, n_area);
    if (!why.empty()) return set_error(RT_ERR_INVALID, why);
    uint64_t n = nl;
    for (uint32_t a = 0; a < n_area; ++a) {
        if (area[a].jitter == RT_JITTER_HASHED)
            return set_error(RT_ERR_INVALID, "area light " + std::to_string(a) +
                                                 ": a hashed light has no expansion (its samples depend on the ray)");
        n += area[a].usteps * area[a].vsteps;
    }
    if (n > 0x7fffffffull) return set_error(RT_ERR_INVALID, "table too large");
    if (out) {
        for (uint32_t l = 0; l < nl; ++l) out[l] = lights[l];
        uint32_t at = nl;
        for (uint32_t a = 0; a < n_area; ++a) {
            const uint32_t N = area[a].usteps * area[a].vsteps;
            for (uint32_t k = 0; k < N; ++k, ++at) {
                area_sample(area[a], a, 0, 0, k, out[at].position);
                for (int q = 0; q < 3; ++q) out[at].intensity[q] = area[a].intensity[q] / (double)N;
            }
        }
    }
    if (n_out) *n_out = (uint32_t)n;
    return RT_OK;
}

int rt_scene_light_info(rt_context* ctx, rt_light_info* out) {
    if (!ctx || !out) return set_error(RT_ERR_INVALID, "null argument");
    *out = ctx->have_scene ? ctx->light_info : rt_light_info{};
    return RT_OK;
}

int rt_scene_smooth_info(rt_context* ctx, rt_smooth_info* out) {
    if (!ctx || !out) return set_error(RT_ERR_INVALID, "null argument");
    *out = ctx->have_scene ? ctx->smooth_info : rt_smooth_info{};
    return RT_OK;
}

int rt_instances_expand(const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes, uint32_t n_meshes,
                        const rt_instance_desc* instances, uint32_t n_inst, rt_shape_desc* out) {
    // (materials are the upload's to check: any index passes here)
    const std::string why = inst::validate(shapes, ns, meshes, n_meshes, instances, n_inst, 0x7FFFFFFFu);
    if (!why.empty()) return set_error(RT_ERR_INVALID, why);
    if (!out && (ns || n_inst)) return set_error(RT_ERR_INVALID, "rt_instances_expand: null output");
    inst::expand(shapes, ns, meshes, instances, n_inst, out);
    return RT_OK;
}

int rt_scene_instance_info(rt_context* ctx, rt_instance_info* out) {
    if (!ctx || !out) return set_error(RT_ERR_INVALID, "null argument");
    *out = ctx->have_scene ? ctx->instance_info : rt_instance_info{};
    return RT_OK;
}

}  // extern "C"

namespace rtc {

// Largest |coordinate| of a point of the shape's surface in object space
// (+inf for an unbounded surface): the reach of a TestPattern on it.
double object_extent(const rt_shape_desc& d) {
    const double inf = std::numeric_limits<double>::infinity();
    switch (d.kind) {
        case RT_SHAPE_SPHERE:
        case RT_SHAPE_CUBE: return 1.0;
        case RT_SHAPE_CYLINDER:
            return std::isfinite(d.minimum) && std::isfinite(d.maximum)
                       ? std::max({1.0, std::fabs(d.minimum), std::fabs(d.maximum)})
                       : inf;
        case RT_SHAPE_CONE:
            return std::isfinite(d.minimum) && std::isfinite(d.maximum)
                       ? std::max(std::fabs(d.minimum), std::fabs(d.maximum))
                       : inf;
        case RT_SHAPE_TRIANGLE: {
            double e = 0.0;
            for (int k = 0; k < 3; ++k)
                e = std::max({e, std::fabs(d.vertex_1[k]), std::fabs(d.vertex_1[k] + d.edge_1[k]),
                              std::fabs(d.vertex_1[k] + d.edge_2[k])});
            return e;
        }
        default: return inf;  // plane
    }
}

// The brightness bound of acc_shift_f32 for these tables: the largest
// colour a material can show (its colour, the colours of every pattern its
// pattern reaches, and for a TestPattern, pattern.rs:55-58, the pattern-space
// point itself: bounded by the surface's object-space extent through the
// material's pattern transform, +inf on an unbounded surface), times the
// lights' intensities and the Phong coefficients.  An area light counts as a
// point light of its intensity: its samples' weights sum to 1.
static void scene_brightness(const WorldLists& wl, double* bright_hit, double* bright_w) {
    const rt_shape_desc* shapes = wl.shapes;
    const rt_material_desc* mats = wl.materials;
    const rt_pattern_desc* pats = wl.patterns;
    const uint32_t ns = wl.n_shapes, nm = wl.n_materials, np = wl.n_patterns;
    // per material: the colours its pattern chain may return, and whether a
    // TestPattern is among them
    std::vector<double> col(nm, 0.0);
    std::vector<char> test(nm, 0);
    for (uint32_t i = 0; i < nm; ++i) {
        for (int c = 0; c < 3; ++c) col[i] = std::max(col[i], std::fabs(mats[i].color[c]));
        std::vector<int32_t> todo;
        std::vector<char> seen(np, 0);
        if (mats[i].pattern >= 0 && (uint32_t)mats[i].pattern < np) todo.push_back(mats[i].pattern);
        while (!todo.empty()) {
            const int32_t q = todo.back();
            todo.pop_back();
            if (q < 0 || (uint32_t)q >= np || seen[q]) continue;
            seen[q] = 1;
            const rt_pattern_desc& pd = pats[q];
            if (pd.kind == RT_PATTERN_TEST) test[i] = 1;
            else if (pd.kind == RT_PATTERN_COMPLEX) todo.insert(todo.end(), {pd.sub_a, pd.sub_b});
            else
                for (int c = 0; c < 3; ++c) col[i] = std::max({col[i], std::fabs(pd.color_a[c]), std::fabs(pd.color_b[c])});
        }
    }
    for (uint32_t s = 0; s < ns; ++s) {  // a TestPattern's colour: the pattern-space point
        const int32_t m = shapes[s].material;
        if (m < 0 || (uint32_t)m >= nm || !test[m]) continue;
        const double ext = object_extent(shapes[s]) * (1.0 + 1e-3) + 1e-3;  // (over_point: a hair off the surface)
        const double* inv = pats[mats[m].pattern].inverse;  // (a complex pattern's subs use its transform)
        for (int r = 0; r < 3; ++r) {
            const double v = (std::fabs(inv[4 * r]) + std::fabs(inv[4 * r + 1]) + std::fabs(inv[4 * r + 2])) * ext +
                             std::fabs(inv[4 * r + 3]);
            col[m] = std::max(col[m], std::isnan(v) ? std::numeric_limits<double>::infinity() : v);
        }
    }
    // Children's weight: a reflective and transparent material mixes them as
    // r·R + t·(1 − R) (world.rs:59-63), at most max(r, t) while Schlick's R
    // stays in [0, 1] -- true when every refractive index is positive (r0 of
    // computed_hit.rs:62 in [0, 1), cos in [0, 1]; TIR gives R = 1); the
    // margin covers cos a rounding past 1 on an unrenormalised refracted
    // direction (world.rs:150).  Otherwise the children add: |r| + |t|.
    bool ri_positive = true;
    for (uint32_t i = 0; i < nm; ++i) ri_positive = ri_positive && mats[i].refractive_index > 0.0;
    double per_light = 0.0, w = 0.0;
    for (uint32_t i = 0; i < nm; ++i) {
        const rt_material_desc& m = mats[i];
        per_light = std::max(per_light, col[i] * (std::fabs(m.ambient) + std::fabs(m.diffuse)) + std::fabs(m.specular));
        const bool mixed = ri_positive && m.reflectiveness > 0.0 && m.transparency > 0.0;
        w = std::max(w, mixed ? std::max(m.reflectiveness, m.transparency) * (1.0 + 1e-6)
                              : std::fabs(m.reflectiveness) + std::fabs(m.transparency));
    }
    double area_intensity = 0.0;
    for (uint32_t a = 0; a < wl.n_area; ++a) {
        double in = 0.0;
        for (int q = 0; q < 3; ++q) in = std::max(in, std::fabs(wl.area[a].intensity[q]));
        area_intensity += in;
    }
    double hit = area_intensity * per_light;
    for (uint32_t l = 0; l < wl.n_lights; ++l) {
        double in = 0.0;
        for (int k = 0; k < 3; ++k) in = std::max(in, std::fabs(wl.lights[l].intensity[k]));
        hit += in * per_light;
    }
    *bright_hit = std::isfinite(hit) ? hit : std::numeric_limits<double>::infinity();
    *bright_w = std::isfinite(w) ? w : std::numeric_limits<double>::infinity();
}

namespace {
// The plain tables of `wl` (shapes, materials, patterns, lights; its other
// lists are the caller's to upload), the shapes with the world indices `wi`;
// generic_only: the world also has instances the generic kernels walk, so no
// per-scene build will run and the plain triangle run gets its tree at any
// world size.
int build_plain_tables(rt_context* ctx, const WorldLists& wl, const WorldIndices& wi, bool generic_only) {
    int rc;
    const rt_shape_desc* shapes = wl.shapes;
    const uint32_t ns = wl.n_shapes;
    PlainPlan pp;
    ctx->duplicate_shapes = ident::shape_classes(shapes, ns, wl.materials, wl.patterns, pp.cls, wi.normals, wi.uvs, wi.velocity);
    pp.order = table_order(shapes, ns, pp.cls);
    // A world the per-scene builds take whole (their records: up to
    // kJitRecordsMaxShapes shapes) keeps the flat triangle run and with it
    // its per-scene kernels, which measured faster for f32 frames up to that
    // size than the generic kernels with a tree (a tree inside
    // per-scene builds is future work).  RTC_DEBUG=tri_min=N overrides.
    const bool per_scene_world = (int64_t)ns <= (int64_t)kJitRecordsMaxShapes && !ctx->knobs.tri_min && !generic_only;
    if (!per_scene_world) pp.triangles = plan_triangles(ctx->knobs, shapes, pp.order, pp.cls, wi.velocity);
    const TrianglePlan& plan = pp.triangles;
    ctx->tree_info = rt_tree_info{};
    if (!plan.tree.nodes.empty()) {
        uint32_t triangles = 0;
        for (uint32_t i = 0; i < ns; ++i) triangles += shapes[i].kind == RT_SHAPE_TRIANGLE;
        ctx->tree_info = {(uint32_t)plan.tree.nodes.size(), plan.tree.leaves, plan.tree.depth, plan.in_tree,
                          triangles - plan.in_tree, 0u, plan.build_ms};
    }
    if ((rc = build_world<float>(ctx, ctx->w32, wl, pp, wi)) || (rc = capture_jit_table(ctx)) ||
        (rc = build_world<double>(ctx, ctx->w64, wl, pp, wi)))
        return rc;
    ctx->flops = FlopScene{};
    for (uint32_t i = 0; i < ns; ++i) {
        const rt_shape_desc& d = shapes[i];
        ctx->flops.per_ray += shape_test_flops(d.kind, d.closed != 0);
    }
    ctx->flops.n_lights = wl.n_lights;
    scene_brightness(wl, &ctx->bright_hit, &ctx->bright_w);
    ++ctx->scene_gen;  // invalidates the recorded tile costs
    return RT_OK;
}

// One per-triangle side list of an upload (inst::SmoothSide, inst::UVSide) as the build holds it.
struct SideList {
    inst::SideIndex index;            // by plain shape and by mesh triangle
    std::vector<const double*> list;  // by entry of the plain list: the triangle's reals, or null
    uint32_t triangles = 0;           // triangles of the expansion the list names
};

// The instance tables of one precision (rtc_internal.hpp InstRec), from the
// plans of the meshes in use and the per-instance decisions.
struct InstancePlan {
    std::vector<inst::MeshPlan> meshes;             // by mesh; empty for a mesh no walked instance uses
    std::vector<uint32_t> rec_begin, node_begin, pos_begin;  // by mesh
    std::vector<uint32_t> bases;                    // inst::world_bases
    std::vector<char> expanded;                     // by instance
    std::vector<uint32_t> expanded_pos;             // by instance: its run of the position table (expanded ones)
    std::vector<int32_t> slot_of;                   // build_world's, by entry of the plain list
    std::vector<uint32_t> list_begin;               // by instance: its first entry of the plain list (expanded ones)
    InstanceCounts counts;
    SideList normals, uvs;                          // the smooth list and the uv list
    std::vector<const double*> velocity;            // by instance: its velocity, null for a static one (empty: none moves)
};

// A side list of `wl` in the build's terms, before the expanded instances' entries are appended to `list`.
template <typename Side>
SideList side_list(const WorldLists& wl, const typename Side::Desc* descs, uint32_t n_descs) {
    SideList s;
    s.index = inst::side_index<Side>(wl.n_shapes, wl.meshes, wl.n_meshes, descs, n_descs);
    s.list.assign(wl.n_shapes, nullptr);
    for (uint32_t i = 0; i < (uint32_t)s.index.plain.size(); ++i) s.list[i] = s.index.plain[i];
    s.triangles = (uint32_t)std::count_if(s.list.begin(), s.list.end(), [](const double* p) { return p != nullptr; });
    for (uint32_t k = 0; k < wl.n_instances; ++k) s.triangles += s.index.named_in_mesh(wl.instances[k].mesh);
    return s;
}

template <typename R>
int upload_instances(rt_context* ctx, DeviceWorld<R>& w, const InstancePlan& ip, const WorldLists& wl) {
    const rt_mesh_desc* meshes = wl.meshes;
    const uint32_t n_inst = wl.n_instances;
    int rc;
    if ((rc = w.allocate_instances(ip.counts))) return rc;
    std::vector<ShapeRec<R>> recs(ip.counts.records);
    std::vector<TriNode<R>> nodes(ip.counts.nodes);
    std::vector<int32_t> pos(ip.counts.pos, 0);
    for (size_t m = 0; m < ip.meshes.size(); ++m) {
        const inst::MeshPlan& mp = ip.meshes[m];
        if (mp.order.empty()) continue;
        for (uint32_t at = 0; at < mp.order.size(); ++at) {
            const uint32_t j = mp.order[at];
            const rt_shape_desc& d = meshes[m].triangles[j];
            ShapeRec<R> r{};
            for (int q = 0; q < 12; ++q) r.inv[q] = (R)d.inverse[q];
            const tri::Ball& b = mp.balls[j];
            for (int q = 0; q < 3; ++q) r.bound[q] = (R)b.c[q];
            r.bound[3] = b.r >= 0.0 ? (R)(b.r * b.r) : (R)-1;
            r.ymin = (R)d.minimum;
            r.ymax = (R)d.maximum;
            for (int q = 0; q < 3; ++q) {
                r.tri[q] = (R)d.vertex_1[q];
                r.tri[3 + q] = (R)d.edge_1[q];
                r.tri[6 + q] = (R)d.edge_2[q];
                r.tri[9 + q] = (R)d.normal[q];
            }
            r.world_index = (int32_t)j;  // the local index: for_instances adds the instance's base
            r.flags = kShapeClassEnd | (ident::normals_of(ip.normals.index.of_mesh((uint32_t)m), j) ? kShapeSmooth : 0) |
                      (ident::normals_of(ip.uvs.index.of_mesh((uint32_t)m), j) ? kShapeUV : 0);
            recs[ip.rec_begin[m] + at] = r;
            pos[ip.pos_begin[m] + j] = (int32_t)(ip.rec_begin[m] + at);
        }
        for (size_t i = 0; i < mp.tree.nodes.size(); ++i) {
            const tri::Node& n = mp.tree.nodes[i];
            TriNode<R>& out = nodes[ip.node_begin[m] + i];
            tri::cast_ball<R>(n.ball, out.ball);
            out.skip = n.skip;
            out.first = n.count ? n.first : 0;  // from the mesh's first record (InstRec::rec_begin)
            out.count = n.count;
        }
    }
    std::vector<InstRec<R>> ir(n_inst);
    for (uint32_t k = 0; k < n_inst; ++k) {
        const rt_instance_desc& d = wl.instances[k];
        const uint32_t m = d.mesh;
        InstRec<R>& r = ir[k];
        r = InstRec<R>{};
        for (int q = 0; q < 12; ++q) r.inv[q] = (R)d.inverse[q];
        r.ball[3] = (R)-1;
        r.world_base = (int32_t)ip.bases[k];
        r.casts_shadow = wl.materials[d.material].casts_shadow ? 1 : 0;
        r.material = d.material;
        r.n_triangles = (int32_t)meshes[m].n_triangles;
        r.moving = !ip.velocity.empty() && ip.velocity[k] ? 1 : 0;
        if (ip.expanded[k]) {
            r.expanded = 1;
            r.pos_begin = (int32_t)ip.expanded_pos[k];
            for (uint32_t j = 0; j < meshes[m].n_triangles; ++j) pos[r.pos_begin + j] = ip.slot_of[ip.list_begin[k] + j];
            continue;
        }
        const inst::MeshPlan& mp = ip.meshes[m];
        r.node_begin = (int32_t)ip.node_begin[m];
        r.n_nodes = (int32_t)mp.tree.nodes.size();
        r.rec_begin = (int32_t)ip.rec_begin[m];
        r.rec_flat = r.rec_begin + (int32_t)mp.in_tree;
        r.rec_end = r.rec_begin + (int32_t)mp.order.size();
        r.pos_begin = (int32_t)ip.pos_begin[m];
        tri::Ball wb;
        // (a mesh with records outside its tree has no ball: every wave tests those)
        if (!mp.tree.nodes.empty() && mp.in_tree == mp.order.size() &&
            inst::instance_ball(mp.tree.nodes[0].ball, d.inverse, &wb))
            tri::cast_ball<R>(wb, r.ball);
    }
    auto put = [&](void* dst, const void* src, size_t bytes) -> int {
        return bytes ? hip_status(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync")
                     : RT_OK;
    };
    // the instance velocity table of a moving world (rtc_internal.hpp MotionArg), each component rounded once to R
    std::vector<R> vel;
    if (!ip.velocity.empty()) {
        vel.assign(4 * (size_t)n_inst, (R)0);
        for (uint32_t k = 0; k < n_inst; ++k)
            if (ip.velocity[k])
                for (int q = 0; q < 3; ++q) vel[4 * (size_t)k + q] = (R)ip.velocity[k][q];
        if ((rc = w.inst_vel.reserve(vel.size()))) return rc;
    }
    rc = put(w.inst.get(), ir.data(), ir.size() * sizeof(ir[0]));
    if (!rc) rc = put(w.inst_vel.get(), vel.data(), vel.size() * sizeof(R));
    if (!rc) rc = put(w.inst_shapes.get(), recs.data(), recs.size() * sizeof(recs[0]));
    if (!rc) rc = put(w.inst_nodes.get(), nodes.data(), nodes.size() * sizeof(nodes[0]));
    if (!rc) rc = put(w.inst_pos.get(), pos.data(), pos.size() * sizeof(pos[0]));
    const int rs = hip_status(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");  // (host temporaries)
    return rc ? rc : rs;
}

// A side table of one precision (rtc_internal.hpp kShapeSmooth, kShapeUV): an
// entry per record of the triangle run when a plain record is named (side.list:
// by entry of the plain list, ip.slot_of: build_world's), and an entry per
// local record of the walked meshes when one of those is.  An entry of a
// record the list does not name is zero and never read.
template <typename Side, typename R>
int upload_side(rt_context* ctx, const DeviceWorld<R>& w, SideTable<R, Side::kReals>& table, const InstancePlan& ip,
                const SideList& side) {
    constexpr int kReals = Side::kReals;
    const int32_t tri0 = w.scene.kind_begin[RT_SHAPE_TRIANGLE], tri1 = w.scene.kind_begin[RT_SHAPE_TRIANGLE + 1];
    SmoothCounts c;
    if (std::any_of(side.list.begin(), side.list.end(), [](const double* p) { return p != nullptr; }))
        c.plain = (uint32_t)(tri1 - tri0);
    for (size_t m = 0; m < ip.meshes.size(); ++m)
        if (!ip.meshes[m].order.empty() && side.index.named_in_mesh((uint32_t)m)) c.inst = ip.counts.records;
    if (int rc = table.allocate(c)) return rc;
    std::vector<R> host(((size_t)c.plain + c.inst) * kReals, (R)0);
    if (c.plain)
        for (size_t i = 0; i < side.list.size(); ++i)
            if (side.list[i]) {
                const int32_t slot = ip.slot_of[i] & 0xFFFFFF;
                if (slot < tri0 || slot >= tri1) return set_error(RT_ERR_INVALID, Side::kOutsideRun);
                for (int q = 0; q < kReals; ++q) host[(size_t)(slot - tri0) * kReals + q] = (R)side.list[i][q];
            }
    if (c.inst)
        for (size_t m = 0; m < ip.meshes.size(); ++m) {
            const inst::MeshPlan& mp = ip.meshes[m];
            const ident::Normals N = side.index.of_mesh((uint32_t)m);
            for (uint32_t at = 0; N && at < mp.order.size(); ++at)
                if (const double* n = N[mp.order[at]])
                    for (int q = 0; q < kReals; ++q) host[((size_t)c.plain + ip.rec_begin[m] + at) * kReals + q] = (R)n[q];
        }
    if (host.empty()) return RT_OK;
    const int rc = hip_status(hipMemcpyAsync(table.reals.get(), host.data(), host.size() * sizeof(R), hipMemcpyHostToDevice,
                                             ctx->stream), "hipMemcpyAsync");
    const int rs = hip_status(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");  // (host temporary)
    return rc ? rc : rs;
}
static_assert(inst::SmoothSide::kReals == kSmoothReals && inst::UVSide::kReals == kUVReals, "the device tables' entry sizes");

// The texels of every texture, one packed dword each (R | G << 8 | B << 16), and the per-texture table; a
// world without a texture still gets a one-entry table, whose address marks the world as textured.
int upload_textures(rt_context* ctx, const WorldLists& wl) {
    const rt_texture_desc* textures = wl.textures;
    const uint32_t n_textures = wl.n_textures;
    std::vector<TexRec> table(std::max<uint32_t>(n_textures, 1u), TexRec{0, 1, 1});
    uint64_t total = 0;
    for (uint32_t t = 0; t < n_textures; ++t) {
        table[t] = TexRec{total, textures[t].width, textures[t].height};
        total += (uint64_t)textures[t].width * textures[t].height;
    }
    // (cube maps: each one's own texture and its six faces as consecutive records, a copy of the texture's each)
    for (uint32_t r = 0; r < wl.n_tex_records; ++r) table.push_back(table[wl.tex_records[r]]);
    int rc;
    if ((rc = ctx->texels.reserve(std::max<uint64_t>(total, 1))) || (rc = ctx->tex_table.reserve(table.size()))) return rc;
    std::vector<uint32_t> host(std::max<uint64_t>(total, 1), 0u);
    for (uint32_t t = 0; t < n_textures; ++t) {
        const uint8_t* src = textures[t].rgb;
        uint32_t* dst = host.data() + table[t].offset;
        const size_t n = (size_t)textures[t].width * textures[t].height;
        for (size_t i = 0; i < n; ++i) dst[i] = (uint32_t)src[3 * i] | (uint32_t)src[3 * i + 1] << 8 | (uint32_t)src[3 * i + 2] << 16;
    }
    rc = hip_status(hipMemcpyAsync(ctx->texels.get(), host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                   ctx->stream), "hipMemcpyAsync");
    if (!rc)
        rc = hip_status(hipMemcpyAsync(ctx->tex_table.get(), table.data(), table.size() * sizeof(TexRec),
                                       hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
    const int rs = hip_status(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");  // (host temporaries)
    if (rc || rs) return rc ? rc : rs;
    ctx->tex_counts = TextureCounts{(uint32_t)table.size(), 1u, total};  // (the table's records: a group sizes its copies by them)
    ctx->w32.texels = ctx->w64.texels = ctx->texels.get();
    ctx->w32.tex_table = ctx->w64.tex_table = ctx->tex_table.get();
    return RT_OK;
}

// The area light records of one precision (rtc_internal.hpp AreaLightRec): the cell edges are the full edges
// divided by the step counts in f64 (rtc.h "Sample positions"), then everything is rounded once to R.
template <typename R>
int upload_area(rt_context* ctx, DeviceWorld<R>& w, const WorldLists& wl) {
    uint32_t samples = 0;
    std::vector<AreaLightRec<R>> host(wl.n_area);
    for (uint32_t a = 0; a < wl.n_area; ++a) {
        const rt_area_light_desc& d = wl.area[a];
        AreaLightRec<R>& r = host[a];
        for (int q = 0; q < 3; ++q) {
            r.corner[q] = (R)d.corner[q];
            r.uvec[q] = (R)(d.full_uvec[q] / (double)d.usteps);
            r.vvec[q] = (R)(d.full_vvec[q] / (double)d.vsteps);
            r.intensity[q] = (R)d.intensity[q];
        }
        r.usteps = d.usteps;
        r.vsteps = d.vsteps;
        r.jitter = d.jitter;
        r.seed = d.seed;
        samples += d.usteps * d.vsteps;
    }
    if (int rc = w.allocate_area(wl.n_area, samples)) return rc;
    if (!wl.n_area) return RT_OK;
    const int rc = hip_status(hipMemcpyAsync(w.area.get(), host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice,
                                             ctx->stream), "hipMemcpyAsync");
    const int rs = hip_status(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");  // (host temporary)
    return rc ? rc : rs;
}

// The context holds no instance, smooth triangle, texture or area light from here on (the buffers keep
// their room): a build fills in what its world has.
void clear_lists(rt_context* ctx) {
    ctx->instance_info = rt_instance_info{};
    ctx->smooth_info = rt_smooth_info{};
    ctx->texture_info = rt_texture_info{};
    ctx->light_info = rt_light_info{};
    ctx->map_info = rt_map_info{};
    ctx->motion_info = rt_motion_info{};
    ctx->smooth_shape.clear();
    ctx->tex_counts = TextureCounts{};
    auto clear = [](auto& w) {
        w.inst_counts = InstanceCounts{};
        w.smooth.counts = w.uv.counts = SmoothCounts{};
        w.texels = nullptr;
        w.tex_table = nullptr;
        w.n_area = w.area_samples = 0;
        w.moving = false;
    };
    clear(ctx->w32);
    clear(ctx->w64);
}

// The general path of build_scene: the plain list (the shapes, then the triangles of the instances uploaded
// expanded), the tables of the meshes the kernels walk, the side tables, and for a `textured` world the
// texture tables and the area lights.  *plain_only: every instance has a value-equal partner and the world
// has nothing else, so the plain list, the expansion, was uploaded as rt_scene_upload would (per-scene
// builds included) and nothing more.
int build_general(rt_context* ctx, const WorldLists& wl, bool textured, bool* plain_only) {
    int rc;
    const rt_mesh_desc* meshes = wl.meshes;
    const rt_instance_desc* instances = wl.instances;
    const uint32_t ns = wl.n_shapes, n_meshes = wl.n_meshes, n_inst = wl.n_instances;
    const auto t0 = std::chrono::steady_clock::now();
    InstancePlan ip;
    ip.normals = side_list<inst::SmoothSide>(wl, wl.smooth, wl.n_smooth);
    ip.uvs = side_list<inst::UVSide>(wl, wl.uvs, wl.n_uvs);
    ip.expanded = inst::decide_expanded(wl.shapes, ns, meshes, n_meshes, instances, n_inst, wl.materials, wl.patterns,
                                        wl.n_smooth ? &ip.normals.index : nullptr);
    ip.bases = inst::world_bases(ns, meshes, instances, n_inst);
    // the movers (rt_scene_upload_moving): the velocity of each top-level shape and of each instance, null for a static one
    std::vector<const double*> shape_velocity(wl.n_motion ? ns : 0, nullptr), inst_velocity(wl.n_motion ? n_inst : 0, nullptr);
    for (uint32_t m = 0; m < wl.n_motion; ++m)
        (wl.motion[m].target == RT_MOVE_SHAPE ? shape_velocity : inst_velocity)[wl.motion[m].index] = wl.motion[m].velocity;
    std::vector<const double*> velocity = shape_velocity;  // by entry of the plain list
    std::vector<rt_shape_desc> list(wl.shapes, wl.shapes + ns);
    std::vector<uint32_t> index(ns);
    for (uint32_t i = 0; i < ns; ++i) index[i] = i;
    ip.list_begin.assign(n_inst, 0);
    ip.expanded_pos.assign(n_inst, 0);
    uint32_t n_expanded = 0, walked_triangles = 0;
    std::vector<char> walked(n_meshes, 0);
    for (uint32_t k = 0; k < n_inst; ++k) {
        const rt_mesh_desc& mesh = meshes[instances[k].mesh];
        if (!ip.expanded[k]) {
            walked[instances[k].mesh] = 1;
            walked_triangles += mesh.n_triangles;
            continue;
        }
        ++n_expanded;
        ip.list_begin[k] = (uint32_t)list.size();
        list.resize(list.size() + mesh.n_triangles);
        inst::expand_instance(mesh, instances[k], list.data() + ip.list_begin[k]);
        for (uint32_t j = 0; j < mesh.n_triangles; ++j) {
            index.push_back(ip.bases[k] + j);
            ip.normals.list.push_back(ident::normals_of(ip.normals.index.of_mesh(instances[k].mesh), j));
            ip.uvs.list.push_back(ident::normals_of(ip.uvs.index.of_mesh(instances[k].mesh), j));
            if (wl.n_motion) velocity.push_back(inst_velocity[k]);  // (an expanded instance's records carry its velocity)
        }
    }
    WorldLists plain = wl;  // (build_plain_tables reads the base tables alone)
    plain.shapes = list.data();
    plain.n_shapes = (uint32_t)list.size();
    *plain_only = n_expanded == n_inst && !wl.n_smooth && !textured && !wl.n_motion;
    if (*plain_only) {
        if ((rc = build_plain_tables(ctx, plain, WorldIndices{}, false))) return rc;
        ctx->instance_info.meshes = n_meshes;
        ctx->instance_info.instances = ctx->instance_info.expanded = n_inst;
        ctx->instance_info.build_ms =
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return RT_OK;
    }
    // the meshes the kernels walk: records, nodes and local-to-position tables, once each
    ip.meshes.resize(n_meshes);
    ip.rec_begin.assign(n_meshes, 0);
    ip.node_begin.assign(n_meshes, 0);
    ip.pos_begin.assign(n_meshes, 0);
    for (uint32_t m = 0; m < n_meshes; ++m) {
        if (!walked[m]) continue;
        ip.meshes[m] = inst::plan_mesh(meshes[m], ctx->knobs.cull, ctx->knobs.tri_tree, ctx->knobs.tri_leaf ? ctx->knobs.tri_leaf : tri::kTriLeaf);
        ip.rec_begin[m] = ip.counts.records;
        ip.node_begin[m] = ip.counts.nodes;
        ip.pos_begin[m] = ip.counts.pos;
        ip.counts.records += meshes[m].n_triangles;
        ip.counts.nodes += (uint32_t)ip.meshes[m].tree.nodes.size();
        ip.counts.pos += meshes[m].n_triangles;
    }
    for (uint32_t k = 0; k < n_inst; ++k)
        if (ip.expanded[k]) {
            ip.expanded_pos[k] = ip.counts.pos;
            ip.counts.pos += meshes[instances[k].mesh].n_triangles;
        }
    ip.counts.instances = n_inst;
    ip.counts.world_begin = (int32_t)ns;
    const double plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    WorldIndices wi;
    wi.index = index.data();
    wi.n_plain = ns;
    wi.slot_of = &ip.slot_of;
    wi.normals = wl.n_smooth ? ip.normals.list.data() : nullptr;
    wi.uvs = wl.n_uvs ? ip.uvs.list.data() : nullptr;
    wi.velocity = wl.n_motion ? velocity.data() : nullptr;
    if ((rc = build_plain_tables(ctx, plain, wi, true))) return rc;
    if (wl.n_motion) {
        ip.velocity = inst_velocity;
        ctx->w32.moving = ctx->w64.moving = true;
        ctx->motion_info.moving_shapes = (uint32_t)std::count_if(shape_velocity.begin(), shape_velocity.end(), [](const double* v) { return v != nullptr; });
        ctx->motion_info.moving_instances = wl.n_motion - ctx->motion_info.moving_shapes;
        // (four reals an entry in both precisions: one per slot of the shape table, one per instance)
        ctx->motion_info.motion_bytes =
            ((uint64_t)std::max<size_t>(list.size(), 1) + n_inst) * 4 * (sizeof(float) + sizeof(double));
    }
    if (textured) {
        if ((rc = upload_side<inst::UVSide>(ctx, ctx->w32, ctx->w32.uv, ip, ip.uvs)) ||
            (rc = upload_side<inst::UVSide>(ctx, ctx->w64, ctx->w64.uv, ip, ip.uvs)) || (rc = upload_textures(ctx, wl)))
            return rc;
        ctx->texture_info.textured_triangles = ip.uvs.triangles;
        ctx->texture_info.textures = wl.n_textures;
        ctx->texture_info.uv_bytes = ctx->w32.uv.bytes() + ctx->w64.uv.bytes();
        ctx->texture_info.texel_bytes = ctx->tex_counts.texels * sizeof(uint32_t) + (uint64_t)wl.n_textures * sizeof(TexRec);
        for (uint32_t k = 0; k < wl.n_maps; ++k) {
            ctx->map_info.mapped_patterns += wl.maps[k].map != RT_MAP_PLANAR;
            ctx->map_info.cube_maps += wl.maps[k].map == RT_MAP_CUBE;
        }
    }
    if ((rc = upload_instances<float>(ctx, ctx->w32, ip, wl)) || (rc = upload_instances<double>(ctx, ctx->w64, ip, wl)) ||
        (rc = upload_side<inst::SmoothSide>(ctx, ctx->w32, ctx->w32.smooth, ip, ip.normals)) ||
        (rc = upload_side<inst::SmoothSide>(ctx, ctx->w64, ctx->w64.smooth, ip, ip.normals)))
        return rc;
    ctx->smooth_info.smooth_triangles = ip.normals.triangles;
    ctx->smooth_info.normal_bytes = ctx->w32.smooth.bytes() + ctx->w64.smooth.bytes();
    ctx->smooth_shape.assign(wl.n_smooth ? ns : 0, 0);
    for (uint32_t i = 0; i < (uint32_t)ip.normals.index.plain.size(); ++i) ctx->smooth_shape[i] = ip.normals.index.plain[i] != nullptr;
    // what the expansion's other tables would have come to: the triangle tests
    // of the flop model, and the brightness bound (a TestPattern's reach is
    // the object-space extent of the mesh, whatever the placement)
    ctx->flops.per_ray += (double)walked_triangles * shape_test_flops(RT_SHAPE_TRIANGLE, false);
    {
        std::vector<double> extent(n_meshes, 0.0);
        for (uint32_t m = 0; m < n_meshes; ++m)
            if (walked[m])
                for (uint32_t j = 0; j < meshes[m].n_triangles; ++j)
                    extent[m] = std::max(extent[m], object_extent(meshes[m].triangles[j]));
        std::vector<rt_shape_desc> reach = list;
        for (uint32_t k = 0; k < n_inst; ++k)
            if (!ip.expanded[k]) {
                rt_shape_desc d{};
                d.kind = RT_SHAPE_TRIANGLE;
                d.material = instances[k].material;
                for (int q = 0; q < 3; ++q) d.vertex_1[q] = extent[instances[k].mesh];
                reach.push_back(d);
            }
        plain.shapes = reach.data();
        plain.n_shapes = (uint32_t)reach.size();
        scene_brightness(plain, &ctx->bright_hit, &ctx->bright_w);
    }
    if (wl.n_area) {
        if ((rc = upload_area<float>(ctx, ctx->w32, wl)) || (rc = upload_area<double>(ctx, ctx->w64, wl))) return rc;
        ctx->light_info.area_lights = wl.n_area;
        ctx->light_info.samples = ctx->w32.area_samples;
        ctx->light_info.area_bytes = (uint64_t)wl.n_area * (sizeof(AreaLightRec<float>) + sizeof(AreaLightRec<double>));
        ctx->flops.n_lights += ctx->w32.area_samples;  // the expansion's light count
    }
    rt_instance_info& info = ctx->instance_info;
    info.meshes = n_meshes;
    info.instances = n_inst;
    info.expanded = n_expanded;
    info.top_depth = 0;
    info.local_records = ip.counts.records;
    info.local_nodes = ip.counts.nodes;
    info.instanced_bytes =
        (uint64_t)ip.counts.records * (sizeof(ShapeRec<float>) + sizeof(ShapeRec<double>)) +
        (uint64_t)ip.counts.nodes * (sizeof(TriNode<float>) + sizeof(TriNode<double>)) +
        (uint64_t)n_inst * (sizeof(InstRec<float>) + sizeof(InstRec<double>)) + (uint64_t)ip.counts.pos * 2 * sizeof(int32_t);
    // (a tree over n records of leaves of kTriLeaf has about n / 4 nodes; the expansion also takes a world_slot word per shape)
    info.expansion_bytes = (uint64_t)walked_triangles * (sizeof(ShapeRec<float>) + sizeof(ShapeRec<double>) + 2 * sizeof(int32_t)) +
                           (uint64_t)(walked_triangles / 4) * (sizeof(TriNode<float>) + sizeof(TriNode<double>));
    info.build_ms = plan_ms;
    return RT_OK;
}
}  // namespace

void set_kernel_build(rt_context* ctx, KernelBuild build) {
    if (build != ctx->kernel_build) std::fill(std::begin(ctx->occ_blocks), std::end(ctx->occ_blocks), 0);  // other kernels now
    ctx->kernel_build = build;
}

// Which path an upload takes, and which build of the kernels its world runs, is decided here, by what the
// validated lists hold:
//   a nonzero velocity                        the general path, the motion build (with whatever else the world holds);
//   else a map other than the planar one      the general path, the map build (with the texture and area tables);
//   else an area light                        the general path, the area build (with the texture tables);
//   else a coordinate entry or image pattern  the general path, the texture build (no other world uploads textures);
//   else a smooth entry                       the general path, the instance build;
//   else instances                            the general path and the instance build, unless every instance has a
//                                             value-equal partner: then the plain path with the expansion;
//   else                                      the plain path (per-scene builds allowed), the plain build.
int build_scene(rt_context* ctx, const WorldLists& wl) {
    ctx->have_scene = false;
    clear_lists(ctx);
    bool images = false;
    for (uint32_t i = 0; i < wl.n_patterns; ++i) images = images || wl.patterns[i].kind == RT_PATTERN_IMAGE;
    const bool textured = wl.n_area || wl.n_uvs || images;
    bool plain_only = !wl.n_instances && !wl.n_smooth && !textured && !wl.n_motion;
    if (int rc = plain_only ? build_plain_tables(ctx, wl, WorldIndices{}, false) : build_general(ctx, wl, textured, &plain_only))
        return rc;
    set_kernel_build(ctx, wl.n_motion ? KernelBuild::moving
                          : ctx->map_info.mapped_patterns ? KernelBuild::mapped
                          : wl.n_area ? KernelBuild::area
                          : textured ? KernelBuild::textured
                          : plain_only ? KernelBuild::plain
                                       : KernelBuild::instanced);
    ctx->have_scene = true;
    return RT_OK;
}

int fetch_jit_tables(rt_context* ctx) {
    const DevScene<float>& sc = ctx->w32.scene;
    ctx->jit.shapes.assign(sc.kind_begin[kNumKinds], ShapeRec<float>{});
    ctx->jit.lights.assign(sc.n_lights, LightRec<float>{});
    ctx->jit.materials.assign(sc.n_materials, MaterialRec<float>{});
    ctx->jit.pattern_recs.assign(sc.n_patterns, PatternRec<float>{});
    auto get = [&](auto& v, const void* src) -> hipError_t {
        return v.empty() ? hipSuccess
                         : hipMemcpyAsync(v.data(), src, v.size() * sizeof(v[0]), hipMemcpyDeviceToHost, ctx->stream);
    };
    RT_HIP(get(ctx->jit.shapes, ctx->w32.shapes));
    RT_HIP(get(ctx->jit.lights, ctx->w32.lights.get()));
    RT_HIP(get(ctx->jit.materials, ctx->w32.materials));
    RT_HIP(get(ctx->jit.pattern_recs, ctx->w32.patterns));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int capture_jit_table(rt_context* ctx) {
    // (jit.shapes, lights, materials, pattern_recs: build_world<float>'s host tables)
    rt_context::Jit& j = ctx->jit;
    for (int k = 0; k <= kNumKinds; ++k) j.begin[k] = ctx->w32.scene.kind_begin[k];
    const std::vector<MaterialRec<float>>& mats = j.materials;
    j.patterns = std::any_of(mats.begin(), mats.end(), [](const MaterialRec<float>& m) { return m.pattern >= 0; });
    j.transparent =
        std::any_of(mats.begin(), mats.end(), [](const MaterialRec<float>& m) { return m.transparency != 0.0f; });
    j.pattern_kinds = 0;
    for (const PatternRec<float>& q : j.pattern_recs)  // every kind a pattern_color walk can meet (complex sub-patterns included)
        j.pattern_kinds |= 1u << std::min<uint32_t>((uint32_t)q.kind, RT_PATTERN_TEST);
    j.reset();
    return RT_OK;
}

// A launch for whichever precision's world the request asks for.
int launch_precision(rt_context* ctx, uint32_t precision, const LaunchRequest& q) {
    return precision == RT_PRECISION_F32 ? launch<float>(ctx, ctx->w32, q) : launch<double>(ctx, ctx->w64, q);
}

int launch_frame(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, uint32_t shard_index,
                 uint32_t shard_count, void* out_device, hipStream_t s, bool image_rows) {
    RT_HIP(hipSetDevice(ctx->device));
    return launch_precision(ctx, o->precision,
                            {.cam = cam, .depth = o->max_depth, .out_format = o->out_format, .shard_index = shard_index,
                             .shard_count = shard_count, .out_device = out_device, .stream = s, .flags = o->flags,
                             .image_rows = image_rows});
}

// ------------------------------------------------------------ peer canvas
unsigned long long* canvas_flags(void* canvas, uint64_t image_bytes) {
    return reinterpret_cast<unsigned long long*>(static_cast<unsigned char*>(canvas) + canvas_flag_offset(image_bytes));
}

unsigned long long timeout_ticks(double timeout_ms) {  // s_memrealtime runs at 100 MHz
    return timeout_ms < 0 ? ~0ull : (unsigned long long)(timeout_ms * 1e5);
}

// After a canvas's flags (n_flags ready flags + the release flag): a trailer
// {image bytes, n_flags}, so rt_canvas_open can check the caller's sizes
// against the creator's instead of placing its flags at a wrong offset.
size_t canvas_flag_bytes(uint32_t n_flags) { return ((size_t)n_flags + 1 + 2) * sizeof(unsigned long long); }

// The canvas is fine-grained device memory: other GPUs store pixels and
// flags into it over xGMI while the owner's canvas_wait polls the flags, and
// the owner then copies the image out.  In coarse-grained memory the owner's
// L2 may keep a line (a flag it polled, pixels it copied out last frame) that
// a peer's store to HBM never updates, and a system-scope acquire does not
// invalidate such lines; fine-grained lines are the ones its acquire
// (canvas_wait) invalidates and its kernels' releases write back.
int canvas_create(rt_context* ctx, uint64_t bytes, uint32_t n_flags, void** canvas) {
    RT_HIP(hipSetDevice(ctx->device));
    const size_t flag_bytes = canvas_flag_bytes(n_flags);
    void* p = nullptr;
    RT_HIP(hipExtMallocWithFlags(&p, canvas_flag_offset(bytes) + flag_bytes, hipDeviceMallocFinegrained));
    std::vector<unsigned long long> tail((size_t)n_flags + 3, 0ull);
    tail[n_flags + 1] = bytes;
    tail[n_flags + 2] = n_flags;
    if (hipError_t e = hipMemcpy(canvas_flags(p, bytes), tail.data(), flag_bytes, hipMemcpyHostToDevice);
        e != hipSuccess) {
        (void)hipFree(p);
        return set_error(RT_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    }
    ctx->canvases[p] = {bytes, n_flags, true};
    *canvas = p;
    return RT_OK;
}

int canvas_close(rt_context* ctx, void* canvas) {
    auto it = ctx->canvases.find(canvas);
    if (it == ctx->canvases.end()) return set_error(RT_ERR_INVALID, "not a canvas of this context");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipDeviceSynchronize());
    const bool owned = it->second.owned;
    ctx->canvases.erase(it);
    if (owned) RT_HIP(hipFree(canvas));
    else RT_HIP(hipIpcCloseMemHandle(canvas));
    return RT_OK;
}

}  // namespace rtc

extern "C" {

int rt_canvas_create(rt_context* ctx, uint64_t bytes, uint32_t n_flags, void** canvas,
                     uint8_t handle[RT_IPC_HANDLE_BYTES]) {
    static_assert(sizeof(hipIpcMemHandle_t) == RT_IPC_HANDLE_BYTES, "RT_IPC_HANDLE_BYTES must match hipIpcMemHandle_t");
    if (!ctx || !canvas || n_flags == 0 || bytes == 0) return set_error(RT_ERR_INVALID, "rt_canvas_create: bad arguments");
    int rc = canvas_create(ctx, bytes, n_flags, canvas);
    if (rc || !handle) return rc;
    hipIpcMemHandle_t h;
    if (hipError_t e = hipIpcGetMemHandle(&h, *canvas); e != hipSuccess) {
        (void)canvas_close(ctx, *canvas);
        *canvas = nullptr;
        return set_error(RT_ERR_HIP, std::string("hipIpcGetMemHandle: ") + hipGetErrorString(e));
    }
    std::memcpy(handle, &h, sizeof h);
    return RT_OK;
}

int rt_canvas_open(rt_context* ctx, const uint8_t handle[RT_IPC_HANDLE_BYTES], uint64_t bytes, uint32_t n_flags,
                   void** canvas) {
    if (!ctx || !handle || !canvas || n_flags == 0 || bytes == 0)
        return set_error(RT_ERR_INVALID, "rt_canvas_open: bad arguments");
    RT_HIP(hipSetDevice(ctx->device));
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle, sizeof h);
    void* p = nullptr;
    RT_HIP(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
    // the creator's sizes, from the canvas's trailer (inside the mapped range only)
    hipDeviceptr_t base = nullptr;
    size_t range = 0;
    const size_t need = canvas_flag_offset(bytes) + canvas_flag_bytes(n_flags);
    unsigned long long tail[2] = {0, 0};
    const bool fits = hipMemGetAddressRange(&base, &range, (hipDeviceptr_t)p) == hipSuccess &&
                      static_cast<char*>(p) + need <= static_cast<char*>(base) + range;
    if (!fits || hipMemcpy(tail, canvas_flags(p, bytes) + n_flags + 1, sizeof tail, hipMemcpyDeviceToHost) != hipSuccess ||
        tail[0] != bytes || tail[1] != n_flags) {
        (void)hipIpcCloseMemHandle(p);
        return set_error(RT_ERR_INVALID, "rt_canvas_open: bytes / n_flags differ from the creator's (" +
                                             std::to_string(tail[0]) + " / " + std::to_string(tail[1]) + ")");
    }
    ctx->canvases[p] = {bytes, n_flags, false};
    *canvas = p;
    return RT_OK;
}

int rt_canvas_close(rt_context* ctx, void* canvas) {
    if (!ctx || !canvas) return set_error(RT_ERR_INVALID, "rt_canvas_close: bad arguments");
    return canvas_close(ctx, canvas);
}

int rt_render_to_canvas(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, void* canvas,
                        uint64_t seq, double timeout_ms, void* hip_stream) {
    int rc = check_ready(ctx);
    if (rc) return rc;
    if ((rc = check_options(o))) return rc;
    if (ctx->group.comm) return set_error(RT_ERR_INVALID, "rt_render_to_canvas takes a single-GPU context");
    auto it = ctx->canvases.find(canvas);
    if (!cam || it == ctx->canvases.end()) return set_error(RT_ERR_INVALID, "null camera or unknown canvas");
    const rt_context::Canvas& c = it->second;
    if ((uint64_t)cam->width * cam->height * pixel_bytes(o) > c.bytes || o->shard_index >= c.n_flags || seq == 0)
        return set_error(RT_ERR_INVALID, "rt_render_to_canvas: canvas too small, shard without a flag, or seq 0");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    RT_HIP(hipSetDevice(ctx->device));
    unsigned long long* flags = canvas_flags(canvas, c.bytes);
    // the owner has released the previous frame (its readers are done)
    if (seq > 1) RT_HIP(launch_canvas_wait(flags + c.n_flags, 1, seq - 1, timeout_ticks(timeout_ms), ctx->d_error.get(), s));
    if (cam->width && cam->height &&
        (rc = launch_frame(ctx, cam, o, o->shard_index, o->shard_count, canvas, s, true)))
        return rc;
    RT_HIP(launch_canvas_signal(flags + o->shard_index, seq, s));
    return RT_OK;
}

int rt_canvas_wait(rt_context* ctx, void* canvas, uint64_t seq, double timeout_ms, void* hip_stream) {
    if (!ctx) return set_error(RT_ERR_INVALID, "null context");
    auto it = ctx->canvases.find(canvas);
    if (it == ctx->canvases.end()) return set_error(RT_ERR_INVALID, "unknown canvas");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(launch_canvas_wait(canvas_flags(canvas, it->second.bytes), it->second.n_flags, seq, timeout_ticks(timeout_ms),
                              ctx->d_error.get(), static_cast<hipStream_t>(hip_stream)));
    return RT_OK;
}

int rt_canvas_read(rt_context* ctx, void* canvas, void* out_host, uint64_t bytes) {
    if (!ctx || !out_host) return set_error(RT_ERR_INVALID, "null argument");
    auto it = ctx->canvases.find(canvas);
    if (it == ctx->canvases.end() || bytes > it->second.bytes) return set_error(RT_ERR_INVALID, "unknown canvas or size");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipDeviceSynchronize());
    RT_HIP(hipMemcpy(out_host, canvas, bytes, hipMemcpyDeviceToHost));
    return check_pool_error(ctx);
}

int rt_canvas_release(rt_context* ctx, void* canvas, uint64_t seq, void* hip_stream) {
    if (!ctx) return set_error(RT_ERR_INVALID, "null context");
    auto it = ctx->canvases.find(canvas);
    if (it == ctx->canvases.end()) return set_error(RT_ERR_INVALID, "unknown canvas");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(launch_canvas_signal(canvas_flags(canvas, it->second.bytes) + it->second.n_flags, seq,
                                static_cast<hipStream_t>(hip_stream)));
    return RT_OK;
}

int rt_shard_rows(uint32_t height, uint32_t shard_count, uint32_t* rows) {
    if (!rows || shard_count == 0) return set_error(RT_ERR_INVALID, "bad arguments");
    *rows = tile_rows_for(height, shard_count, 0) * RT_TILE_H;
    return RT_OK;
}

int rt_shard_row_map(uint32_t height, uint32_t shard_count, uint32_t* shard_of_row, uint32_t* strip_row_of_row) {
    if (shard_count == 0 || (height && (!shard_of_row || !strip_row_of_row)))
        return set_error(RT_ERR_INVALID, "bad arguments");
    for (uint32_t y = 0; y < height; ++y) shard_of_image_row(y, shard_count, &shard_of_row[y], &strip_row_of_row[y]);
    return RT_OK;
}

int rt_render_device(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, void* out_device,
                     void* hip_stream) {
    int rc = check_ready(ctx);
    if (rc) return rc;
    if ((rc = check_options(o))) return rc;
    if (!cam || (!out_device && !(ctx->group.comm && ctx->group.rank != 0)))  // a group's other ranks write no image
        return set_error(RT_ERR_INVALID, "null camera or output");
    if (cam->width == 0 || cam->height == 0) return RT_OK;  // empty canvas (canvas.rs:27-35)
    hipStream_t s = static_cast<hipStream_t>(hip_stream);  // NULL = HIP's default stream
    if (ctx->group.comm) return group_render_device(ctx, cam, o, out_device, s);
    return launch_frame(ctx, cam, o, o->shard_index, o->shard_count, out_device, s);
}

}  // extern "C"

namespace {

// rt_camera_resize(cam, w, h), rtc_scene.h
rt_camera_desc camera_resized(const rt_camera_desc& c, uint32_t w, uint32_t h) {
    rt_camera_desc r = c;
    const hm::CameraSize z = hm::camera_size(w, h, c.field_of_view);
    r.width = w;
    r.height = h;
    r.half_width = z.half_width;
    r.half_height = z.half_height;
    r.pixel_size = z.pixel_size;
    return r;
}

// What a supersampled call may ask for (rtc.h), checked before any work; the
// sample camera Cn of `cam` into *cn.
int check_supersampled(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, uint32_t samples,
                       rt_camera_desc* cn) {
    int rc = check_ready(ctx);
    if (rc) return rc;
    if ((rc = check_options(o))) return rc;
    if (!cam) return set_error(RT_ERR_INVALID, "null camera");
    if (samples < 1 || samples > RT_MAX_SAMPLE_GRID)
        return set_error(RT_ERR_INVALID, "sample grid " + std::to_string(samples) + " outside 1.." +
                                             std::to_string(RT_MAX_SAMPLE_GRID));
    if ((uint64_t)samples * cam->width > 0xFFFFFFFFull || (uint64_t)samples * cam->height > 0xFFFFFFFFull)
        return set_error(RT_ERR_INVALID, "sample grid " + std::to_string(samples) + " x the canvas is beyond 2^32 - 1 "
                                         "sample columns or rows (the grid's range is 1.." +
                                             std::to_string(RT_MAX_SAMPLE_GRID) + ")");
    if (o->flags & ~(RT_FLAG_NO_SKIPS | RT_FLAG_NO_COUNTERS | RT_FLAG_FAIL_LAUNCH))
        return set_error(RT_ERR_INVALID, "supersampled frames take RT_FLAG_NO_SKIPS, RT_FLAG_NO_COUNTERS and "
                                         "RT_FLAG_FAIL_LAUNCH only (the diagnostic launches are rt_render's)");
    if (ctx->group.comm && ctx->group.n_ranks > 1)
        return set_error(RT_ERR_INVALID, "supersampled frames are not split across a group of " +
                                             std::to_string(ctx->group.n_ranks) +
                                             " ranks: render shards per context (shard_index, shard_count)");
    *cn = camera_resized(*cam, samples * cam->width, samples * cam->height);
    // The sample camera keeps the output camera's half extents bit for bit
    // (n W / n H and W / H round to the same f64; tests/test_supersample_cpu.py):
    // the premise of "a pixel is the mean of Cn's pixels".  A size where it
    // failed would be refused here.
    const rt_camera_desc c1 = camera_resized(*cam, cam->width, cam->height);
    if (cam->width && cam->height && (c1.half_width != cn->half_width || c1.half_height != cn->half_height))
        return set_error(RT_ERR_INVALID, "sample grid " + std::to_string(samples) +
                                             ": the sample camera's half extents differ from the output camera's");
    return RT_OK;
}

// What a lens is (rtc.h "Thin-lens camera"), checked before the context is looked at.
int check_lens(const rt_lens_desc* lens) {
    if (!lens) return set_error(RT_ERR_INVALID, "null lens");
    if (!(lens->aperture >= 0.0) || !std::isfinite(lens->aperture))
        return set_error(RT_ERR_INVALID, "lens aperture below 0 or not finite");
    if (!(lens->focal_distance > 0.0) || !std::isfinite(lens->focal_distance))
        return set_error(RT_ERR_INVALID, "lens focal distance not above 0 or not finite");
    if (lens->jitter != RT_JITTER_NONE && lens->jitter != RT_JITTER_HASHED)
        return set_error(RT_ERR_INVALID, "lens jitter " + std::to_string(lens->jitter) +
                                             " is neither RT_JITTER_NONE nor RT_JITTER_HASHED");
    return RT_OK;
}

// One supersampled frame (or shard strip) of output camera `cam`, sample
// camera `cn`, into `out_device` on `s`.  A grid of 1 is the plain frame.
// lens: the same frame through a lens of positive aperture (null: none); a
// grid of 1 is then one lens ray per pixel.
int launch_frame_ss(rt_context* ctx, const rt_camera_desc* cam, const rt_camera_desc* cn, const rt_render_options* o,
                    uint32_t samples, void* out_device, hipStream_t s, const rt_lens_desc* lens = nullptr,
                    const rt_shutter_desc* shutter = nullptr) {
    if (samples == 1 && !lens && !shutter) return launch_frame(ctx, cam, o, o->shard_index, o->shard_count, out_device, s);
    RT_HIP(hipSetDevice(ctx->device));
    return launch_precision(ctx, o->precision,
                            {.cam = cn, .depth = o->max_depth, .out_format = o->out_format,
                             .shard_index = o->shard_index, .shard_count = o->shard_count, .out_device = out_device,
                             .stream = s, .flags = o->flags, .samples = samples, .out_w = cam->width,
                             .out_h = cam->height, .lens = lens, .shutter = shutter});
}

// rt_render's frame into a host buffer; samples != 0: rt_render_supersampled's
// (cn = the sample camera), with a lens rt_render_lens's.
int render_to_host(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, void* out_host,
                   rt_stats* stats, uint32_t samples, const rt_camera_desc* cn, const rt_lens_desc* lens = nullptr,
                   const rt_shutter_desc* shutter = nullptr) {
    int rc;
    if (!out_host) return set_error(RT_ERR_INVALID, "null output");
    RT_HIP(hipSetDevice(ctx->device));
    const uint32_t rows = tile_rows_for(cam->height, o->shard_count, o->shard_index) * RT_TILE_H;
    const uint32_t valid_rows = o->shard_count == 1 ? cam->height : rows;
    const size_t bytes = (size_t)rows * cam->width * pixel_bytes(o);
    const size_t out_bytes = (size_t)valid_rows * cam->width * pixel_bytes(o);
    if (bytes == 0) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return RT_OK;
    }
    InitTrace tr("rt_render");
    if ((rc = ctx->d_scratch.reserve(bytes))) return rc;
    tr.step("scratch");
    // (before and after: kCounterShards x kNumCounters each; the error flag in the 64 bytes behind them)
    if ((rc = ctx->h_counters.reserve(2 * (size_t)kCounterShards * kNumCounters + 8))) return rc;
    tr.step("pinned counters");
    hipStream_t s = ctx->stream;
    // counters before and after, and the error flag, come back in pinned
    // memory on the stream: one host sync for the whole frame
    if ((rc = order_after_last(ctx, s))) return rc;
    const size_t cbytes = (size_t)kCounterShards * kNumCounters * sizeof(unsigned long long);
    unsigned long long* h_before = ctx->h_counters.get();
    unsigned long long* h_after = h_before + (size_t)kCounterShards * kNumCounters;
    int32_t* h_err = reinterpret_cast<int32_t*>(h_after + (size_t)kCounterShards * kNumCounters);
    RT_HIP(hipMemcpyAsync(h_before, ctx->d_counters.get(), cbytes, hipMemcpyDeviceToHost, s));
    if (o->shard_count > 1) RT_HIP(hipMemsetAsync(ctx->d_scratch.get(), 0, bytes, s));  // strip rows past the canvas
    RT_HIP(hipEventRecord(ctx->ev_start, s));
    tr.step("enqueue before launch");
    if ((rc = samples ? launch_frame_ss(ctx, cam, cn, o, samples, ctx->d_scratch.get(), s, lens, shutter)
                      : launch_frame(ctx, cam, o, o->shard_index, o->shard_count, ctx->d_scratch.get(), s)))
        return rc;
    tr.step("launch");
    RT_HIP(hipEventRecord(ctx->ev_stop, s));
    RT_HIP(hipMemcpyAsync(h_after, ctx->d_counters.get(), cbytes, hipMemcpyDeviceToHost, s));
    RT_HIP(hipMemcpyAsync(h_err, ctx->d_error.get(), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if ((rc = copy_to_host(ctx, out_host, out_bytes))) return rc;
    tr.step("enqueue copies");
    RT_HIP(hipStreamSynchronize(s));
    tr.step("synchronize (kernel + copies)");
    float ms = 0.f;
    RT_HIP(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
    if (*h_err) {
        RT_HIP(hipMemsetAsync(ctx->d_error.get(), 0, sizeof(int32_t), s));
        RT_HIP(hipStreamSynchronize(s));
        return set_error(RT_ERR_POOL, device_error_text(*h_err));
    }
    if (stats) {
        unsigned long long before[kNumCounters], after[kNumCounters];
        sum_counter_shards(h_before, before);
        sum_counter_shards(h_after, after);
        fill_stats(ctx, before, after, ms, stats);
    }
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_render(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, void* out_host,
              rt_stats* stats) {
    int rc = check_ready(ctx);
    if (rc) return rc;
    if ((rc = check_options(o))) return rc;
    if (!cam) return set_error(RT_ERR_INVALID, "null camera");
    if (ctx->group.comm) return group_render(ctx, cam, o, out_host, stats);
    return render_to_host(ctx, cam, o, out_host, stats, 0, nullptr);
}

int rt_render_supersampled(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, uint32_t samples,
                           void* out_host, rt_stats* stats) {
    rt_camera_desc cn;
    if (int rc = check_supersampled(ctx, cam, o, samples, &cn)) return rc;
    return render_to_host(ctx, cam, o, out_host, stats, samples, &cn);
}

int rt_render_supersampled_device(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o,
                                  uint32_t samples, void* out_device, void* hip_stream) {
    rt_camera_desc cn;
    if (int rc = check_supersampled(ctx, cam, o, samples, &cn)) return rc;
    if (!out_device) return set_error(RT_ERR_INVALID, "null camera or output");
    if (cam->width == 0 || cam->height == 0) return RT_OK;  // empty canvas, as rt_render_device
    return launch_frame_ss(ctx, cam, &cn, o, samples, out_device, static_cast<hipStream_t>(hip_stream));
}

int rt_render_lens(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, uint32_t samples,
                   const rt_lens_desc* lens, void* out_host, rt_stats* stats) {
    if (int rc = check_lens(lens)) return rc;
    rt_camera_desc cn;
    if (int rc = check_supersampled(ctx, cam, o, samples, &cn)) return rc;
    // (aperture 0: every lens point is the pinhole, and the frame is the supersampled one)
    return render_to_host(ctx, cam, o, out_host, stats, samples, &cn, lens->aperture == 0.0 ? nullptr : lens);
}

int rt_render_lens_device(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, uint32_t samples,
                          const rt_lens_desc* lens, void* out_device, void* hip_stream) {
    if (int rc = check_lens(lens)) return rc;
    rt_camera_desc cn;
    if (int rc = check_supersampled(ctx, cam, o, samples, &cn)) return rc;
    if (!out_device) return set_error(RT_ERR_INVALID, "null camera or output");
    if (cam->width == 0 || cam->height == 0) return RT_OK;  // empty canvas, as rt_render_device
    return launch_frame_ss(ctx, cam, &cn, o, samples, out_device, static_cast<hipStream_t>(hip_stream),
                           lens->aperture == 0.0 ? nullptr : lens);
}

}  // extern "C"

namespace {
// What a shutter is (rtc.h "The shutter"), checked before the context is looked at.
int check_shutter(const rt_shutter_desc* sh) {
    if (!sh) return set_error(RT_ERR_INVALID, "null shutter");
    if (!std::isfinite(sh->open) || !std::isfinite(sh->close))
        return set_error(RT_ERR_INVALID, "shutter bound that is not finite");
    if (sh->open > sh->close) return set_error(RT_ERR_INVALID, "shutter opens after it closes (open > close)");
    if (sh->jitter != RT_JITTER_NONE && sh->jitter != RT_JITTER_HASHED)
        return set_error(RT_ERR_INVALID, "shutter jitter " + std::to_string(sh->jitter) +
                                             " is neither RT_JITTER_NONE nor RT_JITTER_HASHED");
    return RT_OK;
}
}  // namespace

extern "C" {

int rt_render_shutter(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, uint32_t samples,
                      const rt_lens_desc* lens, const rt_shutter_desc* shutter, void* out_host, rt_stats* stats) {
    if (int rc = check_shutter(shutter)) return rc;
    if (lens)
        if (int rc = check_lens(lens)) return rc;
    rt_camera_desc cn;
    if (int rc = check_supersampled(ctx, cam, o, samples, &cn)) return rc;
    // (aperture 0: the pinhole's sample rays; a world without movers: the lens frame, or the supersampled one)
    if (lens && lens->aperture == 0.0) lens = nullptr;
    return render_to_host(ctx, cam, o, out_host, stats, samples, &cn, lens, ctx->w32.moving ? shutter : nullptr);
}

int rt_render_shutter_device(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, uint32_t samples,
                             const rt_lens_desc* lens, const rt_shutter_desc* shutter, void* out_device, void* hip_stream) {
    if (int rc = check_shutter(shutter)) return rc;
    if (lens)
        if (int rc = check_lens(lens)) return rc;
    rt_camera_desc cn;
    if (int rc = check_supersampled(ctx, cam, o, samples, &cn)) return rc;
    if (!out_device) return set_error(RT_ERR_INVALID, "null camera or output");
    if (cam->width == 0 || cam->height == 0) return RT_OK;  // empty canvas, as rt_render_device
    if (lens && lens->aperture == 0.0) lens = nullptr;
    return launch_frame_ss(ctx, cam, &cn, o, samples, out_device, static_cast<hipStream_t>(hip_stream), lens,
                           ctx->w32.moving ? shutter : nullptr);
}

int rt_shutter_time(const rt_camera_desc* cam, uint32_t n, const rt_shutter_desc* shutter, uint32_t x, uint32_t y,
                    uint32_t i, uint32_t j, double* tau) {
    if (int rc = check_shutter(shutter)) return rc;
    if (!cam || !tau) return set_error(RT_ERR_INVALID, "null argument");
    if (n < 1 || n > RT_MAX_SAMPLE_GRID || (uint64_t)n * cam->width > 0xFFFFFFFFull ||
        (uint64_t)n * cam->height > 0xFFFFFFFFull)
        return set_error(RT_ERR_INVALID, "sample grid " + std::to_string(n) + " outside 1.." +
                                             std::to_string(RT_MAX_SAMPLE_GRID));
    if (x >= cam->width || y >= cam->height || i >= n || j >= n)
        return set_error(RT_ERR_INVALID, "rt_shutter_time: pixel or sample out of range");
    ShutterParams<double> sp;  // the kernels' arithmetic in R = double (rtc_internal.hpp shutter_time)
    set_shutter_params(*shutter, n, sp);
    *tau = shutter_time(sp, n, cam->width, x, y, i, j);
    return RT_OK;
}

int rt_lens_ray(const rt_camera_desc* cam, uint32_t n, const rt_lens_desc* lens, uint32_t x, uint32_t y, uint32_t i,
                uint32_t j, double ray[6]) {
    if (int rc = check_lens(lens)) return rc;
    if (!cam || !ray) return set_error(RT_ERR_INVALID, "null argument");
    if (n < 1 || n > RT_MAX_SAMPLE_GRID || (uint64_t)n * cam->width > 0xFFFFFFFFull ||
        (uint64_t)n * cam->height > 0xFFFFFFFFull)
        return set_error(RT_ERR_INVALID, "sample grid " + std::to_string(n) + " outside 1.." +
                                             std::to_string(RT_MAX_SAMPLE_GRID));
    if (x >= cam->width || y >= cam->height || i >= n || j >= n)
        return set_error(RT_ERR_INVALID, "rt_lens_ray: pixel or sample out of range");
    // The kernels' arithmetic in R = double (rtc_kernels.hip lens_ray).
    const rt_camera_desc cn = camera_resized(*cam, n * cam->width, n * cam->height);
    const uint32_t px = n * x + i, py = n * y + j;
    const double ox = ((double)px + 0.5) * cn.pixel_size, oy = ((double)py + 0.5) * cn.pixel_size;
    const double wx = cn.half_width - ox, wy = cn.half_height - oy;
    const double f = lens->focal_distance;
    double fu = (double)i + 0.5, fv = (double)j + 0.5;
    if (lens->jitter == RT_JITTER_HASHED)
        lens_hashed_cell<double>(hash_mix(lens->seed ^ kLensKey), py * (n * cam->width) + px, y * cam->width + x, n, i,
                                 j, fu, fv);
    LensPoint<double> lp;
    lens_point<double>(cn.inverse, lens->aperture, 1.0 / (double)n, fu, fv, lp);
    const double focal[3] = {wx * f, wy * f, -f};
    double target[3];
    lens_xform_point(cn.inverse, focal, target);
    const double d[3] = {target[0] - lp.origin[0], target[1] - lp.origin[1], target[2] - lp.origin[2]};
    const double m = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (int q = 0; q < 3; ++q) {
        ray[q] = lp.origin[q];
        ray[3 + q] = d[q] / m;
    }
    return RT_OK;
}

int rt_color_at(rt_context* ctx, const double* rays, uint64_t n, uint32_t depth, uint32_t precision, double* out,
                rt_stats* stats) {
    int rc = check_ready(ctx);
    if (rc) return rc;
    if (!rays || !out) return set_error(RT_ERR_INVALID, "null rays or output");
    if (precision > RT_PRECISION_F64) return set_error(RT_ERR_INVALID, "unknown precision");
    if (depth > RT_MAX_SUPPORTED_DEPTH) return set_error(RT_ERR_INVALID, "max_depth above RT_MAX_SUPPORTED_DEPTH");
    if (n == 0) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return RT_OK;
    }
    // Worlds with secondary rays run the pool kernel, whose fixed-point pixel
    // sums are sized for unit directions (check_pixel_range): with |d| != 1
    // the specular term grows as |d|^shininess (material.rs:100-109, eye =
    // -d) past any fixed range.  The camera's rays are unit (camera.rs:66),
    // so only a caller's own rays can be refused here.
    if ((ctx->w32.scene.any_secondary || ctx->w64.scene.any_secondary) && depth > 0) {
        for (uint64_t i = 0; i < n; ++i) {
            const double* d = rays + 6 * i + 3;
            const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
            if (!(std::fabs(dd - 1.0) <= 1e-6))
                return set_error(RT_ERR_INVALID, "rt_color_at: ray " + std::to_string(i) + " has |d|^2 = " +
                                                     std::to_string(dd) +
                                                     "; in a world with reflective or transparent materials "
                                                     "directions must be unit length (within 1e-6)");
        }
    }
    RT_HIP(hipSetDevice(ctx->device));
    const size_t in_bytes = n * 6 * sizeof(double), out_bytes = n * 3 * element_bytes(RT_OUT_REAL, precision);
    if ((rc = ctx->d_scratch.reserve(in_bytes + out_bytes))) return rc;
    double* d_rays = reinterpret_cast<double*>(ctx->d_scratch.get());
    void* d_out = ctx->d_scratch.get() + in_bytes;
    RT_HIP(hipMemcpy(d_rays, rays, in_bytes, hipMemcpyHostToDevice));
    unsigned long long before[kNumCounters], after[kNumCounters];
    if ((rc = read_counters(ctx, before))) return rc;
    RT_HIP(hipEventRecord(ctx->ev_start, ctx->stream));
    if ((rc = launch_precision(ctx, precision,
                               {.d_rays = d_rays, .n_rays = n, .depth = depth, .out_device = d_out, .stream = ctx->stream})))
        return rc;
    RT_HIP(hipEventRecord(ctx->ev_stop, ctx->stream));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    RT_HIP(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
    if (precision == RT_PRECISION_F32) {
        std::vector<float> tmp(n * 3);
        RT_HIP(hipMemcpy(tmp.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n * 3; ++i) out[i] = tmp[i];
    } else {
        RT_HIP(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
    }
    if ((rc = check_pool_error(ctx))) return rc;
    if (stats) {
        if ((rc = read_counters(ctx, after))) return rc;
        fill_stats(ctx, before, after, ms, stats);
    }
    return RT_OK;
}

int rt_trace_rays_device(rt_context* ctx, const void* rays_device, uint64_t n_rays, const rt_ray_options* o,
                         void* out_rgb_device, void* out_hit_device, void* hip_stream) {
    return rt_trace_rays_timed_device(ctx, rays_device, nullptr, n_rays, o, out_rgb_device, out_hit_device, hip_stream);
}

int rt_trace_rays_timed_device(rt_context* ctx, const void* rays_device, const void* times_device, uint64_t n_rays,
                               const rt_ray_options* o, void* out_rgb_device, void* out_hit_device, void* hip_stream) {
    if (!ctx) return set_error(RT_ERR_INVALID, "null context");
    if (!rays_device || !out_rgb_device) return set_error(RT_ERR_INVALID, "null rays or output");
    int rc = check_ray_options(o);
    if (rc) return rc;
    if (n_rays > kMaxRayBatch) return set_error(RT_ERR_INVALID, "more than 2^31 rays in one batch");
    if ((rc = check_ready(ctx))) return rc;
    if (n_rays == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    return launch_rays_precision(ctx, rays_device, times_device, n_rays, o, out_rgb_device, out_hit_device,
                                 static_cast<hipStream_t>(hip_stream));
}

int rt_trace_rays(rt_context* ctx, const double* rays, uint64_t n, const rt_ray_options* o, double* out,
                  void* out_hit_f64, rt_stats* stats) {
    return rt_trace_rays_timed(ctx, rays, nullptr, n, o, out, static_cast<rt_ray_hit_f64*>(out_hit_f64), stats);
}

int rt_trace_rays_timed(rt_context* ctx, const double* rays, const double* times, uint64_t n, const rt_ray_options* o,
                        double* out, rt_ray_hit_f64* out_hit, rt_stats* stats) {
    if (!ctx) return set_error(RT_ERR_INVALID, "null context");
    if (!rays || !out) return set_error(RT_ERR_INVALID, "null rays or output");
    int rc = check_ray_options(o);
    if (rc) return rc;
    if (n > kMaxRayBatch) return set_error(RT_ERR_INVALID, "more than 2^31 rays in one batch");
    if ((rc = check_ready(ctx))) return rc;
    if (n == 0) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return RT_OK;
    }
    RT_HIP(hipSetDevice(ctx->device));
    // staging in the kernel's own real type: [rays][rgb][hits][times], each 16-byte aligned
    const bool f32 = o->precision == RT_PRECISION_F32;
    const size_t real = f32 ? sizeof(float) : sizeof(double);
    auto align16 = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t in_bytes = n * 6 * real, rgb_bytes = n * 3 * real;
    const size_t hit_bytes = out_hit ? n * (f32 ? sizeof(rt_ray_hit_f32) : sizeof(rt_ray_hit_f64)) : 0;
    const size_t rgb_at = align16(in_bytes), hit_at = rgb_at + align16(rgb_bytes);
    const size_t times_at = hit_at + align16(hit_bytes), times_bytes = times ? n * real : 0;
    if ((rc = ctx->d_scratch.reserve(times_at + times_bytes))) return rc;
    unsigned char* d_rays = ctx->d_scratch.get();
    unsigned char* d_rgb = d_rays + rgb_at;
    unsigned char* d_hit = out_hit ? d_rays + hit_at : nullptr;
    unsigned char* d_times = times ? d_rays + times_at : nullptr;
    if (times && f32) {
        std::vector<float> tmp(n);
        for (uint64_t i = 0; i < n; ++i) tmp[i] = (float)times[i];
        RT_HIP(hipMemcpy(d_times, tmp.data(), times_bytes, hipMemcpyHostToDevice));
    } else if (times) {
        RT_HIP(hipMemcpy(d_times, times, times_bytes, hipMemcpyHostToDevice));
    }
    if (f32) {
        std::vector<float> tmp(n * 6);
        for (uint64_t i = 0; i < n * 6; ++i) tmp[i] = (float)rays[i];
        RT_HIP(hipMemcpy(d_rays, tmp.data(), in_bytes, hipMemcpyHostToDevice));
    } else {
        RT_HIP(hipMemcpy(d_rays, rays, in_bytes, hipMemcpyHostToDevice));
    }
    unsigned long long before[kNumCounters], after[kNumCounters];
    if ((rc = read_counters(ctx, before))) return rc;
    RT_HIP(hipEventRecord(ctx->ev_start, ctx->stream));
    if ((rc = launch_rays_precision(ctx, d_rays, d_times, n, o, d_rgb, d_hit, ctx->stream))) return rc;
    RT_HIP(hipEventRecord(ctx->ev_stop, ctx->stream));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    RT_HIP(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
    if (f32) {
        std::vector<float> tmp(n * 3);
        RT_HIP(hipMemcpy(tmp.data(), d_rgb, rgb_bytes, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n * 3; ++i) out[i] = tmp[i];
        if (out_hit) {
            std::vector<rt_ray_hit_f32> h(n);
            RT_HIP(hipMemcpy(h.data(), d_hit, hit_bytes, hipMemcpyDeviceToHost));
            for (uint64_t i = 0; i < n; ++i) out_hit[i] = {h[i].t, h[i].shape, 0};
        }
    } else {
        RT_HIP(hipMemcpy(out, d_rgb, rgb_bytes, hipMemcpyDeviceToHost));
        if (out_hit) RT_HIP(hipMemcpy(out_hit, d_hit, hit_bytes, hipMemcpyDeviceToHost));
    }
    if ((rc = check_pool_error(ctx))) return rc;
    if (stats) {
        if ((rc = read_counters(ctx, after))) return rc;
        fill_stats(ctx, before, after, ms, stats);
    }
    return RT_OK;
}

namespace {
// rt_debug_intersect / rt_debug_normal: one launch of the KAT harness kernel
int debug_shape(rt_context* ctx, uint32_t shape, uint32_t mode, const double* in, size_t in_stride, uint64_t n,
                uint32_t precision, uint32_t world_space, double* out, size_t out_stride) {
    int rc = check_ready(ctx);
    if (rc) return rc;
    if (!in || !out) return set_error(RT_ERR_INVALID, "null input or output");
    if (precision > RT_PRECISION_F64) return set_error(RT_ERR_INVALID, "unknown precision");
    if (shape >= ctx->world_slot.size()) return set_error(RT_ERR_INVALID, "shape index out of range");
    if (mode == 1 && shape < ctx->smooth_shape.size() && ctx->smooth_shape[shape])
        return set_error(RT_ERR_INVALID, "rt_debug_normal: a smooth triangle's normal depends on the hit's u and v, "
                                         "which a point does not give");
    if (n == 0) return RT_OK;
    if (n > 0xFFFFFFFFull) return set_error(RT_ERR_INVALID, "too many rays");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t in_bytes = n * in_stride * sizeof(double), out_bytes = n * out_stride * sizeof(double);
    if ((rc = ctx->d_scratch.reserve(in_bytes + out_bytes))) return rc;
    double* d_in = reinterpret_cast<double*>(ctx->d_scratch.get());
    double* d_out = d_in + n * in_stride;
    RT_HIP(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    const int32_t ws = ctx->world_slot[shape];
    const int slot = ws & 0xFFFFFF, kind = ws >> 24;
    if ((rc = order_after_last(ctx, ctx->stream))) return rc;
    hipError_t e = precision == RT_PRECISION_F32
                       ? launch_debug_shape<float>(ctx->w32.shapes, slot, kind, mode, world_space, d_in, (uint32_t)n,
                                                   d_out, ctx->stream)
                       : launch_debug_shape<double>(ctx->w64.shapes, slot, kind, mode, world_space, d_in, (uint32_t)n,
                                                    d_out, ctx->stream);
    if (e != hipSuccess) return set_error(RT_ERR_HIP, std::string("debug_shape launch: ") + hipGetErrorString(e));
    RT_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}
}  // namespace

int rt_debug_intersect(rt_context* ctx, uint32_t shape, const double* rays, uint64_t n, uint32_t precision,
                       uint32_t world_space, double* out) {
    return debug_shape(ctx, shape, 0, rays, 6, n, precision, world_space, out, 1 + RT_DEBUG_MAX_ENTRIES);
}

int rt_debug_normal(rt_context* ctx, uint32_t shape, const double* points, uint64_t n, uint32_t precision,
                    uint32_t world_space, double* out) {
    return debug_shape(ctx, shape, 1, points, 3, n, precision, world_space, out, 3);
}

int rt_context_set_frames_in_flight(rt_context* ctx, uint32_t frames) {
    if (!ctx || frames < 1) return set_error(RT_ERR_INVALID, "bad arguments");
    // (an A/B setting of RTC_DEBUG wins over the hint)
    std::string v;
    const bool grid_knob = debug_knob("direct_oversub", &v), split_knob = debug_knob("split", &v);
    for (rt_context* m : members(ctx)) {
        if (!grid_knob) m->knobs.direct_oversub10 = frames > 1 ? 15u : 25u;
        // pool kernels: with the next frame filling a launch's tail, tiles
        // split only above 1.5x the mean workgroup load (a 4K shard of 8 with
        // two in flight, round 6: cover 0.104 -> 0.094 ms per frame, table
        // 0.115 -> 0.113; a frame alone keeps 1.0x)
        const double split = frames > 1 ? 1.5 : 1.0;
        if (!split_knob && m->knobs.split_factor != split) {
            m->knobs.split_factor = split;
            m->order.valid = m->order_ss.valid = m->order_lens.valid = m->order_shutter.valid = false;  // the next launches rebuild the tile order with it
        }
    }
    return RT_OK;
}

int rt_context_set_jit(rt_context* ctx, int mode) {
    if (!ctx || mode < RT_JIT_OFF || mode > RT_JIT_EAGER) return set_error(RT_ERR_INVALID, "bad arguments");
    for (rt_context* m : members(ctx)) m->jit.mode = mode;
    return RT_OK;
}

int rt_jit_status(rt_context* ctx, int* used_last_launch, double* compile_ms, char* log, size_t log_len) {
    if (!ctx) return set_error(RT_ERR_INVALID, "null context");
    if (used_last_launch) *used_last_launch = ctx->jit.used ? 1 : 0;
    if (compile_ms) *compile_ms = ctx->jit.compile_ms;
    if (log && log_len) {
        std::strncpy(log, ctx->jit.log.c_str(), log_len - 1);
        log[log_len - 1] = '\0';
    }
    return RT_OK;
}

int rt_scene_tree_info(rt_context* ctx, rt_tree_info* out) {
    if (!ctx || !out) return set_error(RT_ERR_INVALID, "null argument");
    *out = ctx->have_scene ? ctx->tree_info : rt_tree_info{};
    return RT_OK;
}

int rt_jit_wait(rt_context* ctx, double timeout_ms, int* pending) {
    if (!ctx) return set_error(RT_ERR_INVALID, "null context");
    // one deadline for the whole group: each member waits for what is left of it
    const auto t0 = std::chrono::steady_clock::now();
    auto remaining = [&] {
        if (timeout_ms < 0) return timeout_ms;
        const double spent = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return std::max(0.0, timeout_ms - spent);
    };
    int total = 0, left = 0;
    for (rt_context* c : members(ctx)) {
        jit_wait(c, remaining(), &left);
        total += left;
    }
    if (pending) *pending = total;
    return RT_OK;
}

int rt_debug_stamps(rt_context* ctx, uint64_t* out, uint32_t max_wg, uint32_t* n) {
    if (!ctx || !n) return set_error(RT_ERR_INVALID, "null argument");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipDeviceSynchronize());
    *n = ctx->stamp_count;
    const uint32_t copy = std::min(max_wg, ctx->stamp_count);
    if (out && copy)
        RT_HIP(hipMemcpy(out, ctx->d_stamps.get(), 2 * sizeof(uint64_t) * copy, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_item_log(rt_context* ctx, uint64_t* out, uint32_t max_items, uint32_t* n) {
    if (!ctx || !n) return set_error(RT_ERR_INVALID, "null argument");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipDeviceSynchronize());
    uint64_t count = 0;
    const unsigned long long* log = ctx->d_item_log.get();  // a count, then 3 words per item
    if (log) RT_HIP(hipMemcpy(&count, log, sizeof count, hipMemcpyDeviceToHost));
    *n = (uint32_t)std::min<uint64_t>(count, log ? (ctx->d_item_log.capacity() - 1) / 3 : 0);
    const uint32_t copy = std::min(max_items, *n);
    if (out && copy)
        RT_HIP(hipMemcpy(out, log + 1, 3 * sizeof(uint64_t) * copy, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_tile_costs(rt_context* ctx, uint32_t* out, uint32_t max_tiles, uint32_t* n) {
    if (!ctx || !n) return set_error(RT_ERR_INVALID, "null argument");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipDeviceSynchronize());
    *n = ctx->order.valid ? (uint32_t)ctx->order.d_cost.capacity() : 0;
    const uint32_t copy = std::min(max_tiles, *n);
    if (out && copy) RT_HIP(hipMemcpy(out, ctx->order.d_cost.get(), copy * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_read_counters(rt_context* ctx, rt_stats* totals) {
    if (!ctx || !totals) return set_error(RT_ERR_INVALID, "null argument");
    if (!ctx->group.peers.empty()) return group_read_counters(ctx, totals);
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipDeviceSynchronize());
    unsigned long long zero[kNumCounters] = {}, now[kNumCounters];
    int rc = read_counters(ctx, now);
    if (rc) return rc;
    fill_stats(ctx, zero, now, 0.f, totals);
    return check_pool_error(ctx);
}

int rt_read_generation_counts(rt_context* ctx, rt_generation_counts* out) {
    if (!ctx || !out) return set_error(RT_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    for (rt_context* m : members(ctx)) {
        unsigned long long buf[2 * kGenSlots];
        RT_HIP(hipSetDevice(m->device));
        RT_HIP(hipDeviceSynchronize());
        RT_HIP(hipMemcpy(buf, m->d_gen_counts.get(), sizeof buf, hipMemcpyDeviceToHost));
        for (int i = 0; i < kGenSlots; ++i) {
            out->traced[i] += buf[i];
            out->shaded[i] += buf[kGenSlots + i];
        }
    }
    RT_HIP(hipSetDevice(ctx->device));
    return RT_OK;
}

int rt_assemble_shards(rt_context* ctx, const void* gathered, uint32_t width, uint32_t height, uint32_t shards,
                       uint32_t bpp, void* image, void* hip_stream) {
    if (!ctx || !gathered || !image || shards == 0 || bpp == 0) return set_error(RT_ERR_INVALID, "bad arguments");
    RT_HIP(hipSetDevice(ctx->device));
    uint32_t rows = 0;
    rt_shard_rows(height, shards, &rows);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);  // NULL = HIP's default stream
    RT_HIP(launch_assemble(gathered, image, width, height, shards, rows, bpp, s));
    return RT_OK;
}

}  // extern "C"
