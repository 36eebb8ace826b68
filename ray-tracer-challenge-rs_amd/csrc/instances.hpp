// instances.hpp — the host side of mesh instances (rtc.h
// rt_scene_upload_instanced; header only: rtc_host.cpp, tests/instances.cpp).
//
// An instanced world MEANS its expansion, shapes ++ E(0) ++ E(1) ++ ... with
// E(k) the triangles of mesh instances[k].mesh under instances[k]'s inverse
// and material (expand() is that definition in code).  What is here:
//   validate()      the refusals of rtc.h, each with its own text;
//   plan_mesh()     a mesh's local balls, its hierarchy (tri_tree.hpp), the
//                   record order the tree leaves it in and the table from
//                   local index to record position;
//   instance_ball() the world ball of a placed mesh;
//   decide_expanded() which instances have a value-equal partner and are
//                   uploaded as plain records (the containers walk identifies
//                   shapes by value: shape_identity.hpp);
//   world_bases()   the world index of each instance's first triangle;
//   validate_side(), side_index(), expand_side()
//                   the per-triangle side lists (vertex normals, texture
//                   coordinates): one implementation, two uses.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/rtc.h"
#include "host_math.hpp"
#include "shape_identity.hpp"
#include "tri_tree.hpp"

namespace rtc {
namespace inst {

// world_slot keeps 24 bits of slot (rtc_internal.hpp DevScene::world_slot)
constexpr uint64_t kMaxWorldShapes = 1ull << 24;

inline bool identity_inverse(const double m[16]) {
    for (int i = 0; i < 16; ++i)
        if (!(m[i] == (i % 5 == 0 ? 1.0 : 0.0))) return false;
    return true;
}

// Empty when the lists are well formed, else the reason (RT_ERR_INVALID).
inline std::string validate(const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes, uint32_t n_meshes,
                            const rt_instance_desc* instances, uint32_t n_inst, uint32_t n_materials) {
    if ((ns && !shapes) || (n_meshes && !meshes) || (n_inst && !instances))
        return "rt_scene_upload_instanced: null table with nonzero count";
    for (uint32_t m = 0; m < n_meshes; ++m) {
        if (meshes[m].n_triangles == 0 || !meshes[m].triangles) return "mesh " + std::to_string(m) + ": empty mesh";
        for (uint32_t j = 0; j < meshes[m].n_triangles; ++j) {
            const rt_shape_desc& d = meshes[m].triangles[j];
            if (d.kind != RT_SHAPE_TRIANGLE)
                return "mesh " + std::to_string(m) + " record " + std::to_string(j) + ": not a triangle";
            if (!identity_inverse(d.inverse))
                return "mesh " + std::to_string(m) + " record " + std::to_string(j) + ": inverse is not the identity";
        }
    }
    uint64_t total = ns;
    for (uint32_t k = 0; k < n_inst; ++k) {
        if (instances[k].mesh >= n_meshes) return "instance " + std::to_string(k) + ": mesh index out of range";
        if (instances[k].material < 0 || (uint32_t)instances[k].material >= n_materials)
            return "instance " + std::to_string(k) + ": material index out of range";
        total += meshes[instances[k].mesh].n_triangles;
        if (total >= kMaxWorldShapes) return "instanced world: the expansion has 2^24 shapes or more";
    }
    return "";
}

// World index of each instance's triangle 0; bases[n_inst] = the world's size.
inline std::vector<uint32_t> world_bases(uint32_t ns, const rt_mesh_desc* meshes, const rt_instance_desc* instances,
                                         uint32_t n_inst) {
    std::vector<uint32_t> b(n_inst + 1);
    uint32_t at = ns;
    for (uint32_t k = 0; k < n_inst; ++k) {
        b[k] = at;
        at += meshes[instances[k].mesh].n_triangles;
    }
    b[n_inst] = at;
    return b;
}

// E(k) into out[0 .. n_triangles): the mesh's records with the instance's inverse and material.
inline void expand_instance(const rt_mesh_desc& mesh, const rt_instance_desc& in, rt_shape_desc* out) {
    for (uint32_t j = 0; j < mesh.n_triangles; ++j) {
        out[j] = mesh.triangles[j];
        std::memcpy(out[j].inverse, in.inverse, sizeof in.inverse);
        out[j].material = in.material;
    }
}
inline void expand(const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes, const rt_instance_desc* instances,
                   uint32_t n_inst, rt_shape_desc* out) {
    for (uint32_t i = 0; i < ns; ++i) out[i] = shapes[i];
    rt_shape_desc* at = out + ns;
    for (uint32_t k = 0; k < n_inst; ++k) {
        expand_instance(meshes[instances[k].mesh], instances[k], at);
        at += meshes[instances[k].mesh].n_triangles;
    }
}

// The ball rtc_host.cpp bounding_sphere gives a triangle record whose inverse
// is the identity (the forward matrix is the identity too: stretch 1, the
// centre unmoved); false for one without a finite ball.
inline bool local_ball(const rt_shape_desc& d, tri::Ball* out) {
    double p[3][3], c[3], r = 0.0;
    for (int q = 0; q < 3; ++q) {
        p[0][q] = d.vertex_1[q];
        p[1][q] = d.vertex_1[q] + d.edge_1[q];
        p[2][q] = d.vertex_1[q] + d.edge_2[q];
    }
    for (int q = 0; q < 3; ++q) c[q] = (p[0][q] + p[1][q] + p[2][q]) / 3.0;
    for (auto& v : p)
        r = std::max(r, std::sqrt((v[0] - c[0]) * (v[0] - c[0]) + (v[1] - c[1]) * (v[1] - c[1]) +
                                  (v[2] - c[2]) * (v[2] - c[2])));
    const double pr = tri::padded_radius(c, r);
    if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2]) || !std::isfinite(pr) || pr > 1e18)
        return false;
    *out = {{c[0], c[1], c[2]}, pr};
    return true;
}

// One mesh as the device holds it: the records with a ball first, in the
// leaf order of the tree over them, the others after them in mesh order (a
// flat run every wave that reaches an instance tests).
struct MeshPlan {
    tri::Tree tree;                // leaves' runs are positions
    std::vector<uint32_t> order;   // position -> local index
    std::vector<uint32_t> pos;     // local index -> position
    std::vector<tri::Ball> balls;  // by local index; r < 0: none
    uint32_t in_tree = 0;          // positions [0, in_tree) are reached through leaves
};
// cull = false (RTC_DEBUG=cull=0): no balls, no tree, every record in the flat run.
// tree = false (RTC_DEBUG=tri_tree=0): the balls, and every record in the flat run.
inline MeshPlan plan_mesh(const rt_mesh_desc& mesh, bool cull, bool tree = true, uint32_t leaf_max = tri::kTriLeaf) {
    MeshPlan p;
    const uint32_t n = mesh.n_triangles;
    p.balls.assign(n, tri::Ball{{0.0, 0.0, 0.0}, -1.0});
    std::vector<uint32_t> bounded, unbounded;
    std::vector<tri::Ball> bb;
    for (uint32_t j = 0; j < n; ++j) {
        tri::Ball b;
        const bool have = cull && local_ball(mesh.triangles[j], &b);
        if (have) p.balls[j] = b;
        if (have && tree) {
            bounded.push_back(j);
            bb.push_back(b);
        } else {
            unbounded.push_back(j);
        }
    }
    // (every record a class of its own: an instanced mesh has no repeated face, decide_expanded)
    p.tree = tri::build(bb.data(), bounded.data(), (uint32_t)bounded.size(), leaf_max);
    p.in_tree = (uint32_t)bounded.size();
    p.order.reserve(n);
    for (uint32_t from : p.tree.order) p.order.push_back(bounded[from]);
    for (uint32_t j : unbounded) p.order.push_back(j);
    p.pos.assign(n, 0);
    for (uint32_t at = 0; at < n; ++at) p.pos[p.order[at]] = at;
    return p;
}

// The world ball of a mesh (its root ball, local space) under an instance:
// the centre's image, the radius times an upper bound of the linear part's
// largest stretch (sqrt of the largest absolute row sum of F^T F, as
// bounding_sphere), padded by bounding_sphere's rule.  false: no ball (a
// singular or non-finite forward matrix).
inline bool instance_ball(const tri::Ball& root, const double inverse[16], tri::Ball* out) {
    hm::M4 inv;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) inv.m[i][j] = inverse[4 * i + j];
    const hm::M4 f = hm::inverse(inv);
    double ftf[3][3] = {}, sigma2 = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) ftf[i][j] += f.m[k][i] * f.m[k][j];
    for (auto& row : ftf) sigma2 = std::max(sigma2, std::fabs(row[0]) + std::fabs(row[1]) + std::fabs(row[2]));
    double wc[3];
    for (int i = 0; i < 3; ++i)
        wc[i] = f.m[i][0] * root.c[0] + f.m[i][1] * root.c[1] + f.m[i][2] * root.c[2] + f.m[i][3];
    const double wr = root.r * std::sqrt(sigma2);
    const double pr = tri::padded_radius(wc, wr);
    if (!std::isfinite(wc[0]) || !std::isfinite(wc[1]) || !std::isfinite(wc[2]) || !std::isfinite(wr) ||
        !std::isfinite(sigma2) || !(pr <= 1e18))
        return false;
    *out = {{wc[0], wc[1], wc[2]}, pr};
    return true;
}

// ---- identity ---------------------------------------------------------------
// Two triangles of the expansion are value-equal (shape_identity.hpp shape_eq)
// only when their inverses are equal, their materials value-equal and their
// local geometry equal.  So: holders of an (inverse, material), the instances
// and the plain triangles, are bucketed by the inverse's hash; two holders of
// one bucket with equal inverse and material are partners when their geometry
// meets: two instances of one mesh always, of two meshes when the meshes share
// a face, an instance and a plain triangle when the mesh has that face.  A
// mesh with a repeated face makes every instance of it its own partner.  (An
// inverse that holds a NaN equals nothing, itself included.)
// (nx, ny: the triangles' nine vertex normals, null for a flat one: smooth
// triangles are equal when those are too, a smooth and a flat one never)
inline bool geometry_eq(const rt_shape_desc& x, const rt_shape_desc& y, const double* nx = nullptr,
                        const double* ny = nullptr) {
    return ident::reals_eq(x.vertex_1, y.vertex_1, 3) && ident::reals_eq(x.edge_1, y.edge_1, 3) &&
           ident::reals_eq(x.edge_2, y.edge_2, 3) && ident::reals_eq(x.normal, y.normal, 3) &&
           ident::normals_eq(nx, ny);
}
inline uint64_t local_hash(const rt_shape_desc& s) {  // consistent with geometry_eq (-0 and +0 alike; normals not hashed)
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](double v) {
        if (v == 0.0) v = 0.0;
        uint64_t b;
        std::memcpy(&b, &v, sizeof b);
        h = (h ^ b) * 1099511628211ull;
        h ^= h >> 29;
    };
    for (double v : s.vertex_1) mix(v);
    for (double v : s.edge_1) mix(v);
    for (double v : s.edge_2) mix(v);
    return h;
}
inline uint64_t inverse_hash(const double m[16]) {
    uint64_t h = 1469598103934665603ull;
    for (int i = 0; i < 16; ++i) {
        double v = m[i];
        if (v == 0.0) v = 0.0;
        uint64_t b;
        std::memcpy(&b, &v, sizeof b);
        h = (h ^ b) * 1099511628211ull;
        h ^= h >> 29;
    }
    return h;
}
// A mesh's faces by hash, sorted: (hash, local index)
using FaceIndex = std::vector<std::pair<uint64_t, uint32_t>>;
inline FaceIndex face_index(const rt_mesh_desc& mesh) {
    FaceIndex f(mesh.n_triangles);
    for (uint32_t j = 0; j < mesh.n_triangles; ++j) f[j] = {local_hash(mesh.triangles[j]), j};
    std::sort(f.begin(), f.end());
    return f;
}
// (na, nb, tn: the vertex normals of the meshes' triangles by local index and of `t`: ident::Normals)
inline bool repeated_face(const rt_mesh_desc& mesh, const FaceIndex& f, ident::Normals na = nullptr) {
    for (size_t a = 0; a < f.size(); ++a)
        for (size_t b = a + 1; b < f.size() && f[b].first == f[a].first; ++b)
            if (geometry_eq(mesh.triangles[f[a].second], mesh.triangles[f[b].second], ident::normals_of(na, f[a].second),
                            ident::normals_of(na, f[b].second)))
                return true;
    return false;
}
inline bool has_face(const rt_mesh_desc& mesh, const FaceIndex& f, const rt_shape_desc& t, ident::Normals na = nullptr,
                     const double* tn = nullptr) {
    const uint64_t h = local_hash(t);
    for (auto it = std::lower_bound(f.begin(), f.end(), std::make_pair(h, 0u)); it != f.end() && it->first == h; ++it)
        if (geometry_eq(mesh.triangles[it->second], t, ident::normals_of(na, it->second), tn)) return true;
    return false;
}
inline bool share_face(const rt_mesh_desc& a, const FaceIndex& fa, const rt_mesh_desc& b, const FaceIndex& fb,
                       ident::Normals na = nullptr, ident::Normals nb = nullptr) {
    size_t i = 0, j = 0;
    while (i < fa.size() && j < fb.size()) {
        if (fa[i].first < fb[j].first) ++i;
        else if (fb[j].first < fa[i].first) ++j;
        else {
            const uint64_t h = fa[i].first;
            size_t ie = i, je = j;
            while (ie < fa.size() && fa[ie].first == h) ++ie;
            while (je < fb.size() && fb[je].first == h) ++je;
            for (size_t x = i; x < ie; ++x)
                for (size_t y = j; y < je; ++y)
                    if (geometry_eq(a.triangles[fa[x].second], b.triangles[fb[y].second],
                                    ident::normals_of(na, fa[x].second), ident::normals_of(nb, fb[y].second)))
                        return true;
            i = ie;
            j = je;
        }
    }
    return false;
}

// ---- per-triangle side lists (rtc.h rt_scene_upload_smooth, rt_scene_upload_textured) ----
// Vertex normals and texture coordinates are both lists of entries that name a
// triangle (a plain shape, or a mesh's local record) and give it a run of
// reals.  What differs is here; the code below is written once for both.
struct SmoothSide {  // rt_scene_upload_smooth's list: nine normal components an entry
    using Desc = rt_smooth_desc;
    static constexpr int kReals = 9;
    static constexpr const char* kEntry = "smooth entry ";
    static constexpr const char* kNullList = "rt_scene_upload_smooth: null smooth list with nonzero count";
    static constexpr const char* kNotFinite = ": a normal component is not finite";
    static constexpr const char* kOutsideRun = "smooth triangle outside the triangle run";
    static const double* reals(const Desc& d) { return d.normal_1; }
    static double* reals(Desc& d) { return d.normal_1; }
};
static_assert(sizeof(rt_smooth_desc) == 80 && offsetof(rt_smooth_desc, normal_1) == 8 &&
                  offsetof(rt_smooth_desc, normal_3) == 8 + 6 * sizeof(double),
              "the nine normal components are contiguous");
struct UVSide {  // rt_scene_upload_textured's coordinate list: six components an entry
    using Desc = rt_uv_desc;
    static constexpr int kReals = 6;
    static constexpr const char* kEntry = "uv entry ";
    static constexpr const char* kNullList = "rt_scene_upload_textured: null uv list with nonzero count";
    static constexpr const char* kNotFinite = ": a texture coordinate is not finite";
    static constexpr const char* kOutsideRun = "textured triangle outside the triangle run";
    static const double* reals(const Desc& d) { return d.uv_1; }
    static double* reals(Desc& d) { return d.uv_1; }
};
static_assert(sizeof(rt_uv_desc) == 56 && offsetof(rt_uv_desc, uv_1) == 8 &&
                  offsetof(rt_uv_desc, uv_3) == 8 + 4 * sizeof(double),
              "the six coordinate components are contiguous");

// Empty when the list is well formed against validated instanced lists, else
// the reason (RT_ERR_INVALID), each with its own text.
template <typename Side>
inline std::string validate_side(const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes, uint32_t n_meshes,
                                 const typename Side::Desc* list, uint32_t n_list) {
    if (n_list && !list) return Side::kNullList;
    std::vector<std::vector<char>> seen(n_meshes + 1);  // [n_meshes]: the plain shapes
    for (uint32_t k = 0; k < n_list; ++k) {
        const typename Side::Desc& d = list[k];
        const std::string who = Side::kEntry + std::to_string(k);
        if (d.list != RT_SMOOTH_SHAPES && d.list >= n_meshes) return who + ": list index out of range";
        const bool plain = d.list == RT_SMOOTH_SHAPES;
        const uint32_t n = plain ? ns : meshes[d.list].n_triangles;
        if (d.index >= n) return who + ": triangle index out of range";
        const rt_shape_desc& t = plain ? shapes[d.index] : meshes[d.list].triangles[d.index];
        if (t.kind != RT_SHAPE_TRIANGLE) return who + ": the named record is not a triangle";
        std::vector<char>& s = seen[plain ? n_meshes : d.list];
        if (s.empty()) s.assign(n, 0);
        if (s[d.index]) return who + ": the same triangle is named twice";
        s[d.index] = 1;
        for (int q = 0; q < Side::kReals; ++q)
            if (!std::isfinite(Side::reals(d)[q])) return who + Side::kNotFinite;
    }
    return "";
}

// The reals of a validated side list by triangle: per plain shape and per mesh
// triangle the entry's reals, or null for a triangle the list does not name.
struct SideIndex {
    std::vector<const double*> plain;              // by shape; empty: none is named
    std::vector<std::vector<const double*>> mesh;  // by mesh, by local index; empty: none of the mesh's is
    ident::Normals of_plain() const { return plain.empty() ? nullptr : plain.data(); }
    ident::Normals of_mesh(uint32_t m) const { return mesh[m].empty() ? nullptr : mesh[m].data(); }
    uint32_t named_in_mesh(uint32_t m) const {
        return (uint32_t)std::count_if(mesh[m].begin(), mesh[m].end(), [](const double* p) { return p != nullptr; });
    }
};
template <typename Side>
inline SideIndex side_index(uint32_t ns, const rt_mesh_desc* meshes, uint32_t n_meshes, const typename Side::Desc* list,
                            uint32_t n_list) {
    SideIndex si;
    si.mesh.resize(n_meshes);
    for (uint32_t k = 0; k < n_list; ++k) {
        const typename Side::Desc& d = list[k];
        std::vector<const double*>& v = d.list == RT_SMOOTH_SHAPES ? si.plain : si.mesh[d.list];
        if (v.empty()) v.assign(d.list == RT_SMOOTH_SHAPES ? ns : meshes[d.list].n_triangles, nullptr);
        v[d.index] = Side::reals(d);
    }
    return si;
}
// The side list of the expansion (expand()): the plain entries, then per
// instance its mesh's entries at the instance's world indices, every entry with
// RT_SMOOTH_SHAPES, in ascending world index (the reals do not transform).
// Returns the count; out may be null.
template <typename Side>
inline uint32_t expand_side(uint32_t ns, const rt_mesh_desc* meshes, uint32_t n_meshes, const rt_instance_desc* instances,
                            uint32_t n_inst, const typename Side::Desc* list, uint32_t n_list, typename Side::Desc* out) {
    const SideIndex si = side_index<Side>(ns, meshes, n_meshes, list, n_list);
    uint32_t at = 0;
    auto put = [&](uint32_t world, const double* reals) {
        if (out) {
            out[at].list = RT_SMOOTH_SHAPES;
            out[at].index = world;
            std::memcpy(Side::reals(out[at]), reals, Side::kReals * sizeof(double));
        }
        ++at;
    };
    for (uint32_t i = 0; i < (uint32_t)si.plain.size(); ++i)
        if (si.plain[i]) put(i, si.plain[i]);
    uint32_t base = ns;
    for (uint32_t k = 0; k < n_inst; ++k) {
        const uint32_t m = instances[k].mesh;
        for (uint32_t j = 0; j < (uint32_t)si.mesh[m].size(); ++j)
            if (si.mesh[m][j]) put(base + j, si.mesh[m][j]);
        base += meshes[m].n_triangles;
    }
    return at;
}

// ---- image textures (rtc.h rt_scene_upload_textured) --------------------------
// Empty when the texture list is well formed, else the reason (RT_ERR_INVALID).
inline std::string validate_textures(const rt_texture_desc* textures, uint32_t n_textures) {
    if (n_textures && !textures) return "rt_scene_upload_textured: null texture list with nonzero count";
    for (uint32_t k = 0; k < n_textures; ++k) {
        const rt_texture_desc& t = textures[k];
        const std::string who = "texture " + std::to_string(k);
        if (!t.rgb) return who + ": null pixels";
        if (!t.width || !t.height) return who + ": zero width or height";
        if ((uint64_t)t.width * t.height > (uint64_t)RT_TEXTURE_MAX_TEXELS) return who + ": more than 2^28 texels";
    }
    return "";
}
// Do two textures hold the same picture (width, height, bytes)?
inline bool texture_eq(const rt_texture_desc& a, const rt_texture_desc& b) {
    return a.width == b.width && a.height == b.height &&
           (a.rgb == b.rgb || std::memcmp(a.rgb, b.rgb, (size_t)a.width * a.height * 3) == 0);
}
// Image patterns compare by their textures' contents (shape_identity.hpp pattern_eq) and bound the brightness by
// their largest channel (scene_brightness).  Rewrites validated patterns in place: an image pattern's sub_a
// becomes the smallest index of a texture with the same picture, whichever patterns name which textures and in
// what order, and its color_a and color_b (ignored otherwise) the largest channel / 255.
//
// Texture maps (rtc.h rt_scene_upload_mapped; `maps` validated by validate_maps): a pattern with a map other
// than the planar one gets it into bits 8 and up of `reserved`, beside the filter, so pattern_eq compares it.
// A cube map's sub_a becomes n_textures + kCubeRecords * s, where s numbers the distinct tuples (renumbered
// sub_a, six renumbered faces) in the order the patterns meet them, and `records` (cleared first) receives
// each tuple's kCubeRecords texture indices: the device texture table's records after the textures' own
// (rtc_internal.hpp TexRec).  Equal sub_a then means equal pictures on every face, and the brightness bound
// is the largest channel over the seven.
constexpr uint32_t kCubeRecords = 7;  // the pattern's own texture (a textured triangle samples it), then the faces
inline void canonical_image_patterns(rt_pattern_desc* pats, uint32_t np, const rt_texture_desc* textures,
                                     uint32_t n_textures, const rt_uv_map_desc* maps = nullptr, uint32_t n_maps = 0,
                                     std::vector<int32_t>* records = nullptr) {
    std::vector<int32_t> first(n_textures, -1);
    std::vector<double> top(n_textures, 0.0);
    auto renumber = [&](uint32_t t) {
        if (first[t] < 0) {
            first[t] = (int32_t)t;
            for (uint32_t e = 0; e < t; ++e)  // (every earlier texture, named by a pattern or not)
                if (texture_eq(textures[e], textures[t])) {
                    first[t] = (int32_t)e;
                    break;
                }
            const size_t n = (size_t)textures[t].width * textures[t].height * 3;
            top[t] = (double)*std::max_element(textures[t].rgb, textures[t].rgb + n) / 255.0;
        }
        return first[t];
    };
    std::vector<const rt_uv_map_desc*> map_of(n_maps ? np : 0, nullptr);
    for (uint32_t k = 0; k < n_maps; ++k) map_of[maps[k].pattern] = &maps[k];
    if (records) records->clear();
    std::vector<int32_t> sets;  // kCubeRecords indices a distinct tuple
    for (uint32_t i = 0; i < np; ++i) {
        rt_pattern_desc& p = pats[i];
        if (p.kind != RT_PATTERN_IMAGE) continue;
        const uint32_t t = (uint32_t)p.sub_a;
        p.sub_a = renumber(t);
        double bound = top[t];
        const rt_uv_map_desc* const m = n_maps ? map_of[i] : nullptr;
        if (m && m->map != RT_MAP_PLANAR) p.reserved |= (int32_t)(m->map << 8);
        if (m && m->map == RT_MAP_CUBE) {
            int32_t tuple[kCubeRecords] = {p.sub_a};
            for (int f = 0; f < 6; ++f) {
                tuple[1 + f] = renumber((uint32_t)m->faces[f]);
                bound = std::max(bound, top[(uint32_t)m->faces[f]]);
            }
            size_t s = 0;
            while (s < sets.size() && !std::equal(tuple, tuple + kCubeRecords, sets.begin() + s)) s += kCubeRecords;
            if (s == sets.size()) sets.insert(sets.end(), tuple, tuple + kCubeRecords);
            p.sub_a = (int32_t)(n_textures + s);
        }
        for (int q = 0; q < 3; ++q) p.color_a[q] = p.color_b[q] = bound;
    }
    if (records) *records = sets;
}

// rt_scene_upload_mapped's list against the validated patterns and the texture count; empty: valid.
inline std::string validate_maps(const rt_uv_map_desc* maps, uint32_t n_maps, const rt_pattern_desc* pats, uint32_t np,
                                 uint32_t n_textures) {
    if (n_maps && !maps) return "rt_scene_upload_mapped: null map list with nonzero count";
    std::vector<char> named(np, 0);
    for (uint32_t k = 0; k < n_maps; ++k) {
        const rt_uv_map_desc& m = maps[k];
        const std::string who = "map " + std::to_string(k);
        if (m.pattern >= np) return who + ": pattern index out of range";
        if (pats[m.pattern].kind != RT_PATTERN_IMAGE) return who + ": the pattern is not an image pattern";
        if (named[m.pattern]) return who + ": pattern named twice";
        named[m.pattern] = 1;
        if (m.map > RT_MAP_CUBE) return who + ": unknown map";
        for (int f = 0; f < 6; ++f) {
            if (m.map == RT_MAP_CUBE && (m.faces[f] < 0 || (uint32_t)m.faces[f] >= n_textures))
                return who + ": face texture index out of range";
            if (m.map != RT_MAP_CUBE && m.faces[f] != -1) return who + ": a face other than -1 for a map that is no cube map";
        }
    }
    return "";
}

// expanded[k] = 1: instance k has a triangle value-equal to another triangle
// of the expansion and is uploaded as plain records.  si: the world's smooth
// triangles (null: none), whose normals are part of a triangle's value.
// Texture coordinates are left out of the faces' comparison here: two faces
// equal but for their coordinates make their instances partners, which are
// then uploaded as plain records, where shape_classes does compare the
// coordinates.  The decision errs towards expanding, never towards a wrong
// identity class.
inline std::vector<char> decide_expanded(const rt_shape_desc* shapes, uint32_t ns, const rt_mesh_desc* meshes,
                                         uint32_t n_meshes, const rt_instance_desc* instances, uint32_t n_inst,
                                         const rt_material_desc* mats, const rt_pattern_desc* pats,
                                         const SideIndex* si = nullptr) {
    auto mesh_normals = [&](uint32_t m) { return si ? si->of_mesh(m) : nullptr; };
    const ident::Normals plain_normals = si ? si->of_plain() : nullptr;
    std::vector<char> expanded(n_inst, 0);
    if (!n_inst) return expanded;
    std::vector<FaceIndex> faces(n_meshes);
    std::vector<char> used(n_meshes, 0), repeated(n_meshes, 0);
    for (uint32_t k = 0; k < n_inst; ++k) used[instances[k].mesh] = 1;
    for (uint32_t m = 0; m < n_meshes; ++m)
        if (used[m]) {
            faces[m] = face_index(meshes[m]);
            repeated[m] = repeated_face(meshes[m], faces[m], mesh_normals(m));
        }
    struct Holder {
        const double* inverse;
        int32_t material;
        int64_t instance;  // or -1: plain triangle `shape`
        uint32_t shape;
    };
    std::unordered_map<uint64_t, std::vector<Holder>> buckets;
    for (uint32_t k = 0; k < n_inst; ++k)
        buckets[inverse_hash(instances[k].inverse)].push_back({instances[k].inverse, instances[k].material, k, 0u});
    for (uint32_t i = 0; i < ns; ++i)
        if (shapes[i].kind == RT_SHAPE_TRIANGLE) {
            auto it = buckets.find(inverse_hash(shapes[i].inverse));
            if (it != buckets.end()) it->second.push_back({shapes[i].inverse, shapes[i].material, -1, i});
        }
    for (auto& kv : buckets) {
        const std::vector<Holder>& hs = kv.second;
        for (size_t a = 0; a < hs.size(); ++a) {
            if (hs[a].instance < 0) continue;  // (instances come first in a bucket)
            const uint32_t ka = (uint32_t)hs[a].instance, ma = instances[ka].mesh;
            if (!ident::reals_eq(hs[a].inverse, hs[a].inverse, 16)) continue;  // a NaN: equal to nothing
            if (repeated[ma]) expanded[ka] = 1;
            for (size_t b = a + 1; b < hs.size(); ++b) {
                if (hs[b].instance >= 0 && expanded[ka] && expanded[(uint32_t)hs[b].instance]) continue;
                if (hs[b].instance < 0 && expanded[ka]) continue;
                if (!ident::reals_eq(hs[a].inverse, hs[b].inverse, 16) ||
                    !ident::material_eq(mats, pats, hs[a].material, hs[b].material))
                    continue;
                if (hs[b].instance >= 0) {
                    const uint32_t kb = (uint32_t)hs[b].instance, mb = instances[kb].mesh;
                    if (ma == mb ||
                        share_face(meshes[ma], faces[ma], meshes[mb], faces[mb], mesh_normals(ma), mesh_normals(mb)))
                        expanded[ka] = expanded[kb] = 1;
                } else if (has_face(meshes[ma], faces[ma], shapes[hs[b].shape], mesh_normals(ma),
                                    ident::normals_of(plain_normals, hs[b].shape))) {
                    expanded[ka] = 1;
                }
            }
        }
    }
    return expanded;
}

}  // namespace inst
}  // namespace rtc
