// mesh_loader.cpp — triangle meshes from Wavefront OBJ text (rtc_scene.h
// rt_mesh_*): the book's subset (vertices and fan-triangulated faces), and the
// faces as the reference's Triangle::new (triangle.rs:21-35) in f64 with the
// reference's operation order.  Pure host code.
#include <cerrno>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/rtc_scene.h"
#include "rtc_internal.hpp"

struct rt_mesh {
    std::vector<double> vertices;     // x, y, z per vertex
    std::vector<uint32_t> triangles;  // three 0-based vertex indices per triangle
    uint32_t ignored_lines = 0;
    // RT_OBJ_NORMALS loads (rt_mesh_load_obj_ex); empty otherwise
    std::vector<double> normals;             // x, y, z per vn line, as written
    std::vector<uint32_t> triangle_normals;  // three 0-based normal indices per triangle, RT_NO_NORMAL x 3: a flat face
    uint32_t n_smooth = 0;
    bool with_normals = false;
    // RT_OBJ_TEXCOORDS loads; empty otherwise
    std::vector<double> texcoords;             // u, v per vt line (a third component is read and dropped)
    std::vector<uint32_t> triangle_texcoords;  // three 0-based vt indices per triangle, RT_NO_TEXCOORD x 3: none
    uint32_t n_textured = 0;
    bool with_texcoords = false;
};

namespace rtc {
namespace {

struct ObjError {
    std::string what;
};

std::vector<std::string> split_words(const std::string& line) {
    std::vector<std::string> words;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && (line[i] == ' ' || line[i] == '\t')) ++i;
        size_t j = i;
        while (j < line.size() && line[j] != ' ' && line[j] != '\t') ++j;
        if (j > i) words.push_back(line.substr(i, j - i));
        i = j;
    }
    return words;
}

double parse_real(const std::string& w, size_t line_no) {
    char* end = nullptr;
    errno = 0;
    const double v = std::strtod(w.c_str(), &end);
    if (w.empty() || end != w.c_str() + w.size())
        throw ObjError{"line " + std::to_string(line_no) + ": '" + w + "' is not a number"};
    return v;
}

// the vertex index of a face word (i, i/j, i//k, i/j/k), 0-based
uint32_t parse_index(const std::string& w, size_t n_vertices, size_t line_no) {
    const std::string head = w.substr(0, w.find('/'));
    char* end = nullptr;
    errno = 0;
    const long long i = std::strtoll(head.c_str(), &end, 10);
    if (head.empty() || end != head.c_str() + head.size() || errno == ERANGE)
        throw ObjError{"line " + std::to_string(line_no) + ": '" + w + "' is not a vertex index"};
    const long long at = i > 0 ? i - 1 : (long long)n_vertices + i;  // negative: back from the vertices so far
    if (i == 0 || at < 0 || at >= (long long)n_vertices)
        throw ObjError{"line " + std::to_string(line_no) + ": vertex index " + std::to_string(i) + " out of range (" +
                       std::to_string(n_vertices) + " vertices so far)"};
    return (uint32_t)at;
}

// the normal index of a face word (i//k, i/j/k), 0-based; RT_NO_NORMAL for a word without one
uint32_t parse_normal_index(const std::string& w, size_t n_normals, size_t line_no) {
    const size_t s1 = w.find('/');
    if (s1 == std::string::npos) return RT_NO_NORMAL;
    const size_t s2 = w.find('/', s1 + 1);
    if (s2 == std::string::npos) return RT_NO_NORMAL;
    const std::string tail = w.substr(s2 + 1);
    if (tail.empty()) return RT_NO_NORMAL;
    char* end = nullptr;
    errno = 0;
    const long long i = std::strtoll(tail.c_str(), &end, 10);
    if (end != tail.c_str() + tail.size() || errno == ERANGE)
        throw ObjError{"line " + std::to_string(line_no) + ": '" + w + "' is not a normal index"};
    const long long at = i > 0 ? i - 1 : (long long)n_normals + i;  // negative: back from the normals so far
    if (i == 0 || at < 0 || at >= (long long)n_normals)
        throw ObjError{"line " + std::to_string(line_no) + ": normal index " + std::to_string(i) + " out of range (" +
                       std::to_string(n_normals) + " normals so far)"};
    return (uint32_t)at;
}

// the texture index of a face word (i/j, i/j/k), 0-based; RT_NO_TEXCOORD for a word without one (i, i//k)
uint32_t parse_texcoord_index(const std::string& w, size_t n_texcoords, size_t line_no) {
    const size_t s1 = w.find('/');
    if (s1 == std::string::npos) return RT_NO_TEXCOORD;
    const size_t s2 = w.find('/', s1 + 1);
    const std::string mid = w.substr(s1 + 1, s2 == std::string::npos ? std::string::npos : s2 - s1 - 1);
    if (mid.empty()) return RT_NO_TEXCOORD;
    char* end = nullptr;
    errno = 0;
    const long long i = std::strtoll(mid.c_str(), &end, 10);
    if (end != mid.c_str() + mid.size() || errno == ERANGE)
        throw ObjError{"line " + std::to_string(line_no) + ": '" + w + "' is not a texture index"};
    const long long at = i > 0 ? i - 1 : (long long)n_texcoords + i;  // negative: back from the vt lines so far
    if (i == 0 || at < 0 || at >= (long long)n_texcoords)
        throw ObjError{"line " + std::to_string(line_no) + ": texture index " + std::to_string(i) + " out of range (" +
                       std::to_string(n_texcoords) + " texture coordinates so far)"};
    return (uint32_t)at;
}

void parse_obj(const std::string& text, rt_mesh& m, uint32_t flags = 0) {
    const bool with_normals = (flags & RT_OBJ_NORMALS) != 0;
    const bool with_texcoords = (flags & RT_OBJ_TEXCOORDS) != 0;
    m.with_normals = with_normals;
    m.with_texcoords = with_texcoords;
    size_t pos = 0, line_no = 0;
    while (pos < text.size()) {
        size_t eol = text.find('\n', pos);
        if (eol == std::string::npos) eol = text.size();
        std::string line = text.substr(pos, eol - pos);
        pos = eol + 1;
        ++line_no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        const std::vector<std::string> w = split_words(line);
        if (!w.empty() && w[0] == "v") {
            if (w.size() < 4) throw ObjError{"line " + std::to_string(line_no) + ": a vertex needs three coordinates"};
            for (int q = 1; q <= 3; ++q) m.vertices.push_back(parse_real(w[q], line_no));
        } else if (!w.empty() && w[0] == "f") {
            if (w.size() < 4) throw ObjError{"line " + std::to_string(line_no) + ": a face needs three vertices"};
            std::vector<uint32_t> idx, nidx, tidx;
            bool smooth = with_normals, mapped = with_texcoords;
            for (size_t q = 1; q < w.size(); ++q) {
                idx.push_back(parse_index(w[q], m.vertices.size() / 3, line_no));
                if (with_normals) {
                    nidx.push_back(parse_normal_index(w[q], m.normals.size() / 3, line_no));
                    smooth = smooth && nidx.back() != RT_NO_NORMAL;  // every vertex names one, or the face is flat
                }
                if (with_texcoords) {
                    tidx.push_back(parse_texcoord_index(w[q], m.texcoords.size() / 2, line_no));
                    mapped = mapped && tidx.back() != RT_NO_TEXCOORD;  // every vertex names one, or the face has none
                }
            }
            for (size_t k = 1; k + 1 < idx.size(); ++k) {  // the fan (1, k, k + 1)
                m.triangles.push_back(idx[0]);
                m.triangles.push_back(idx[k]);
                m.triangles.push_back(idx[k + 1]);
                if (with_normals) {
                    m.triangle_normals.push_back(smooth ? nidx[0] : RT_NO_NORMAL);
                    m.triangle_normals.push_back(smooth ? nidx[k] : RT_NO_NORMAL);
                    m.triangle_normals.push_back(smooth ? nidx[k + 1] : RT_NO_NORMAL);
                    m.n_smooth += smooth ? 1u : 0u;
                }
                if (with_texcoords) {
                    m.triangle_texcoords.push_back(mapped ? tidx[0] : RT_NO_TEXCOORD);
                    m.triangle_texcoords.push_back(mapped ? tidx[k] : RT_NO_TEXCOORD);
                    m.triangle_texcoords.push_back(mapped ? tidx[k + 1] : RT_NO_TEXCOORD);
                    m.n_textured += mapped ? 1u : 0u;
                }
            }
        } else if (with_normals && !w.empty() && w[0] == "vn") {
            if (w.size() < 4) throw ObjError{"line " + std::to_string(line_no) + ": a normal needs three components"};
            for (int q = 1; q <= 3; ++q) {
                char* end = nullptr;
                const double v = std::strtod(w[q].c_str(), &end);
                if (w[q].empty() || end != w[q].c_str() + w[q].size())
                    throw ObjError{"line " + std::to_string(line_no) + ": '" + w[q] + "' is not a number in a normal"};
                m.normals.push_back(v);
            }
        } else if (with_texcoords && !w.empty() && w[0] == "vt") {
            if (w.size() < 3)
                throw ObjError{"line " + std::to_string(line_no) + ": a texture coordinate needs two components"};
            for (size_t q = 1; q < w.size() && q <= 3; ++q) {  // u v [w]: the third is checked and dropped
                char* end = nullptr;
                const double v = std::strtod(w[q].c_str(), &end);
                if (w[q].empty() || end != w[q].c_str() + w[q].size())
                    throw ObjError{"line " + std::to_string(line_no) + ": '" + w[q] +
                                   "' is not a number in a texture coordinate"};
                if (q <= 2) m.texcoords.push_back(v);
            }
        } else {
            ++m.ignored_lines;
        }
    }
}

int load(const std::string& text, rt_mesh** out, uint32_t flags = 0) {
    try {
        auto m = std::make_unique<rt_mesh>();
        parse_obj(text, *m, flags);
        *out = m.release();
        return RT_OK;
    } catch (const ObjError& e) {
        return set_error(RT_ERR_IO, "OBJ: " + e.what);
    } catch (const std::exception& e) {
        return set_error(RT_ERR_IO, std::string("OBJ: ") + e.what());
    }
}

int load_file(const char* path, rt_mesh** out, uint32_t flags) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return set_error(RT_ERR_IO, std::string("cannot open ") + path + ": " + std::strerror(errno));
    std::stringstream ss;
    ss << f.rdbuf();
    if (f.bad()) return set_error(RT_ERR_IO, std::string("cannot read ") + path);
    return load(ss.str(), out, flags);
}

// Matrix<4> * Point (matrix.rs:332-346): per row a left fold from 0.0 over
// (x, y, z, 1), no FMA
void mul_point(const double* t, const double p[3], double out[3]) {
    const double v[4] = {p[0], p[1], p[2], 1.0};
    for (int r = 0; r < 3; ++r) {
        double acc = 0.0;
        for (int c = 0; c < 4; ++c) acc = acc + t[4 * r + c] * v[c];
        out[r] = acc;
    }
}

}  // namespace
}  // namespace rtc

extern "C" {

int rt_mesh_load_obj_text(const char* text, rt_mesh** out) {
    if (!text || !out) return rtc::set_error(RT_ERR_INVALID, "rt_mesh_load_obj_text: null argument");
    return rtc::load(text, out);
}

int rt_mesh_load_obj(const char* path, rt_mesh** out) {
    if (!path || !out) return rtc::set_error(RT_ERR_INVALID, "rt_mesh_load_obj: null argument");
    return rtc::load_file(path, out, 0);
}

int rt_mesh_load_obj_ex(const char* path, const char* text, uint32_t flags, rt_mesh** out) {
    if (!out || (path == nullptr) == (text == nullptr))
        return rtc::set_error(RT_ERR_INVALID, "rt_mesh_load_obj_ex: give a path or a text (one of the two) and an output");
    if (flags & ~(RT_OBJ_NORMALS | RT_OBJ_TEXCOORDS))
        return rtc::set_error(RT_ERR_INVALID, "rt_mesh_load_obj_ex: unknown flag");
    return text ? rtc::load(text, out, flags) : rtc::load_file(path, out, flags);
}

int rt_mesh_normals_get(const rt_mesh* m, rt_mesh_normals_view* v) {
    if (!m || !v) return rtc::set_error(RT_ERR_INVALID, "rt_mesh_normals_get: null argument");
    *v = rt_mesh_normals_view{};
    if (!m->with_normals) return RT_OK;
    v->normals = m->normals.data();
    v->n_normals = (uint32_t)(m->normals.size() / 3);
    v->n_smooth = m->n_smooth;
    v->triangle_normals = m->triangle_normals.data();
    return RT_OK;
}

int rt_mesh_texcoords_get(const rt_mesh* m, rt_mesh_texcoords_view* v) {
    if (!m || !v) return rtc::set_error(RT_ERR_INVALID, "rt_mesh_texcoords_get: null argument");
    *v = rt_mesh_texcoords_view{};
    if (!m->with_texcoords) return RT_OK;
    v->texcoords = m->texcoords.data();
    v->n_texcoords = (uint32_t)(m->texcoords.size() / 2);
    v->n_textured = m->n_textured;
    v->triangle_texcoords = m->triangle_texcoords.data();
    return RT_OK;
}

int rt_mesh_uvs(const rt_mesh* m, rt_uv_desc* out, uint32_t list, uint32_t* n_out) {
    if (!m) return rtc::set_error(RT_ERR_INVALID, "rt_mesh_uvs: null argument");
    if (n_out) *n_out = m->n_textured;
    if (!out || !m->n_textured) return RT_OK;
    uint32_t at = 0;
    const size_t n = m->triangle_texcoords.size() / 3;
    for (size_t t = 0; t < n; ++t) {
        const uint32_t* k = &m->triangle_texcoords[3 * t];
        if (k[0] == RT_NO_TEXCOORD) continue;
        rt_uv_desc& d = out[at++];
        std::memset(&d, 0, sizeof d);
        d.list = list;
        d.index = (uint32_t)t;
        double* dst[3] = {d.uv_1, d.uv_2, d.uv_3};
        for (int c = 0; c < 3; ++c)
            for (int q = 0; q < 2; ++q) dst[c][q] = m->texcoords[2 * (size_t)k[c] + q];
    }
    return RT_OK;
}

int rt_mesh_smooth_normals(const rt_mesh* m, const double* transform, int bake, rt_smooth_desc* out, uint32_t list,
                           uint32_t* n_out) {
    if (!m) return rtc::set_error(RT_ERR_INVALID, "rt_mesh_smooth_normals: null argument");
    if (n_out) *n_out = m->n_smooth;
    if (!out || !m->n_smooth) return RT_OK;
    double inv[16];
    const bool baked = transform && bake;
    if (baked)
        if (const int rc = rt_matrix_inverse(transform, inv)) return rc;
    uint32_t at = 0;
    const size_t n = m->triangle_normals.size() / 3;
    for (size_t t = 0; t < n; ++t) {
        const uint32_t* k = &m->triangle_normals[3 * t];
        if (k[0] == RT_NO_NORMAL) continue;
        rt_smooth_desc& d = out[at++];
        std::memset(&d, 0, sizeof d);
        d.list = list;
        d.index = (uint32_t)t;
        double* dst[3] = {d.normal_1, d.normal_2, d.normal_3};
        for (int c = 0; c < 3; ++c) {
            const double* src = &m->normals[3 * (size_t)k[c]];
            // baked: transpose(inverse) * n, a left fold per row like Matrix<4> * Vector (matrix.rs:348-362), no FMA
            for (int r = 0; r < 3; ++r)
                dst[c][r] = baked ? ((0.0 + inv[r] * src[0]) + inv[4 + r] * src[1]) + inv[8 + r] * src[2] : src[r];
        }
    }
    return RT_OK;
}

int rt_mesh_view_get(const rt_mesh* m, rt_mesh_view* v) {
    if (!m || !v) return rtc::set_error(RT_ERR_INVALID, "rt_mesh_view_get: null argument");
    v->vertices = m->vertices.data();
    v->n_vertices = (uint32_t)(m->vertices.size() / 3);
    v->triangles = m->triangles.data();
    v->n_triangles = (uint32_t)(m->triangles.size() / 3);
    v->ignored_lines = m->ignored_lines;
    return RT_OK;
}

void rt_mesh_free(rt_mesh* m) { delete m; }

int rt_mesh_triangles(const rt_mesh* m, const double* transform, int bake, int32_t material, rt_shape_desc* out) {
    if (!m || (!out && !m->triangles.empty())) return rtc::set_error(RT_ERR_INVALID, "rt_mesh_triangles: null argument");
    double inv[16];
    for (int i = 0; i < 16; ++i) inv[i] = i % 5 == 0 ? 1.0 : 0.0;
    if (transform && !bake) {
        const int rc = rt_matrix_inverse(transform, inv);
        if (rc) return rc;
    }
    const size_t n = m->triangles.size() / 3;
    for (size_t t = 0; t < n; ++t) {
        double p[3][3];
        for (int k = 0; k < 3; ++k) {
            const double* v = &m->vertices[3 * (size_t)m->triangles[3 * t + k]];
            if (transform && bake) rtc::mul_point(transform, v, p[k]);
            else std::memcpy(p[k], v, sizeof p[k]);
        }
        rt_shape_desc& d = out[t];
        std::memset(&d, 0, sizeof d);
        d.kind = RT_SHAPE_TRIANGLE;
        d.material = material;
        std::memcpy(d.inverse, inv, sizeof inv);
        d.minimum = -DBL_MAX;
        d.maximum = DBL_MAX;
        double* e1 = d.edge_1;
        double* e2 = d.edge_2;
        for (int q = 0; q < 3; ++q) {
            d.vertex_1[q] = p[0][q];
            e1[q] = p[1][q] - p[0][q];
            e2[q] = p[2][q] - p[0][q];
        }
        // edge_2.cross(&edge_1) (vector.rs:97-103: mul_add), then normalized()
        // (vector.rs:84-91: plain squares and sums, one division per axis)
        const double c[3] = {std::fma(e2[1], e1[2], -e2[2] * e1[1]), std::fma(e2[2], e1[0], -e2[0] * e1[2]),
                             std::fma(e2[0], e1[1], -e2[1] * e1[0])};
        const double mag = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        for (int q = 0; q < 3; ++q) d.normal[q] = c[q] / mag;
    }
    return RT_OK;
}

}  // extern "C"
