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

void parse_obj(const std::string& text, rt_mesh& m) {
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
            std::vector<uint32_t> idx;
            for (size_t q = 1; q < w.size(); ++q) idx.push_back(parse_index(w[q], m.vertices.size() / 3, line_no));
            for (size_t k = 1; k + 1 < idx.size(); ++k) {  // the fan (1, k, k + 1)
                m.triangles.push_back(idx[0]);
                m.triangles.push_back(idx[k]);
                m.triangles.push_back(idx[k + 1]);
            }
        } else {
            ++m.ignored_lines;
        }
    }
}

int load(const std::string& text, rt_mesh** out) {
    try {
        auto m = std::make_unique<rt_mesh>();
        parse_obj(text, *m);
        *out = m.release();
        return RT_OK;
    } catch (const ObjError& e) {
        return set_error(RT_ERR_IO, "OBJ: " + e.what);
    } catch (const std::exception& e) {
        return set_error(RT_ERR_IO, std::string("OBJ: ") + e.what());
    }
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
    std::ifstream f(path, std::ios::binary);
    if (!f) return rtc::set_error(RT_ERR_IO, std::string("cannot open ") + path + ": " + std::strerror(errno));
    std::stringstream ss;
    ss << f.rdbuf();
    if (f.bad()) return rtc::set_error(RT_ERR_IO, std::string("cannot read ") + path);
    return rtc::load(ss.str(), out);
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
