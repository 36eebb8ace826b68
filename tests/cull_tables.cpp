// Host check of the direct kernel's cull tables (csrc/cull_tables.hpp
// fill_cull_tables), compiled stand-alone by tests/test_cull_tables.py and, with
// the address and undefined-behaviour sanitizers, by
// tests/test_cull_tables_sanitizers.py.
//
// fill_cull_tables builds the tables a launch uploads from toggles and one
// running XOR.  Here every entry is stated a second time by its definition
// (rtc_internal.hpp, "Primary cull" and "Shadow cull"), entry by entry and with
// no toggles, from the same rectangle functions (primary_rect.hpp), and every
// word of both tables is compared:
//   - bit s of cols[i]: slot s's rectangle is empty or its columns miss
//     [16 i, 16 i + 15]; rows likewise with 4; a plane's slot by plane_rect;
//   - a pair bit (light, plane, caster) likewise by shadow_rect;
//   - a plane's bit as its own caster: every column iff shadow_self_clear;
//   - a plane's near bit: the block columns and rows that lie wholly inside the
//     intersection of the lights' shadow_near spans, the ragged last block
//     ending with the canvas;
//   - no shadow bit at all where ShadowLayout does not fit;
//   - zero at and beyond ceil(width / 16) and ceil(height / 4).
// Canvases of one block, exactly one block, ragged by a pixel each way, several
// blocks and the tables' limit; worlds from three_sphere's shape to eight
// slots; then NaN, infinite, denormal and huge values in a caster's bound and
// a light; then lights near the end of their reach over the plane, whose near
// spans shrink to parts of one block.  Prints one line per check and "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../ray-tracer-challenge-rs_amd/csrc/cull_tables.hpp"
#include "../ray-tracer-challenge-rs_amd/csrc/launch_terms.hpp"

using namespace rtc;

static int g_failed = 0;
#define CHECK(cond, ...)                                       \
    do {                                                       \
        if (!(cond)) {                                         \
            if (g_failed < 20) {                               \
                std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                      \
                std::printf("\n");                             \
            }                                                  \
            ++g_failed;                                        \
        }                                                      \
    } while (0)

// a small deterministic generator (xorshift)
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}
static float uni(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() >> 8) / 16777216.0f; }

// (the odd values of tests/plane_rects.cpp)
static float odd_value() {
    static const float kOdd[] = {0.0f, -0.0f, 1.0f, -1.0f, 1e-45f, -1e-45f, 1e-38f, 1e-20f, -1e-20f, 1e20f, -1e20f, 3e38f,
                                 std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                                 std::numeric_limits<float>::quiet_NaN(), 8e-8f, 1e-7f, -1e-7f};
    return kOdd[rnd() % (sizeof kOdd / sizeof kOdd[0])];
}

static CameraRec<float> level_camera(float fov_half, uint32_t width, uint32_t height, float ex, float ey, float ez) {
    // a camera at (ex, ey, ez) looking along +z: camera x = -world x, camera z = -world z
    CameraRec<float> c;
    std::memset(&c, 0, sizeof c);
    c.inv[0] = -1.0f, c.inv[5] = 1.0f, c.inv[10] = -1.0f;
    c.inv[3] = ex, c.inv[7] = ey, c.inv[11] = ez;
    c.origin[0] = ex, c.origin[1] = ey, c.origin[2] = ez;
    const float aspect = (float)width / (float)height;
    c.half_width = aspect >= 1.0f ? fov_half : fov_half * aspect;
    c.half_height = aspect >= 1.0f ? fov_half / aspect : fov_half;
    c.pixel_size = c.half_width * 2.0f / (float)width;
    return c;
}

// A world as the per-scene tables hold it: f32 records by kind, f32 lights.
struct World {
    const char* name;
    std::vector<ShapeRec<float>> shapes;
    int32_t kind_begin[kNumKinds + 1];
    std::vector<LightRec<float>> lights;
};
static ShapeRec<float> record() {
    ShapeRec<float> r;
    std::memset(&r, 0, sizeof r);
    r.inv[0] = r.inv[5] = r.inv[10] = 1.0f;
    r.casts_shadow = 1;
    return r;
}
// a bounded slot (a sphere, a cube): only its ball goes into the tables
static ShapeRec<float> ball(float x, float y, float z, float r) {
    ShapeRec<float> s = record();
    s.bound[0] = x, s.bound[1] = y, s.bound[2] = z, s.bound[3] = r * r;
    return s;
}
// the plane n . x = h: row 1 of the inverse is {n, -h}; unbounded
static ShapeRec<float> plane(float nx, float ny, float nz, float h) {
    ShapeRec<float> s = record();
    s.inv[4] = nx, s.inv[5] = ny, s.inv[6] = nz, s.inv[7] = -h;
    s.bound[3] = -1.0f;
    return s;
}
static LightRec<float> light(float x, float y, float z) {
    LightRec<float> l;
    std::memset(&l, 0, sizeof l);
    l.position[0] = x, l.position[1] = y, l.position[2] = z;
    l.intensity[0] = l.intensity[1] = l.intensity[2] = 1.0f;
    return l;
}
// spheres, then planes, then cubes: the table's order by kind
static World world(const char* name, std::vector<ShapeRec<float>> spheres, std::vector<ShapeRec<float>> planes,
                   std::vector<ShapeRec<float>> cubes, std::vector<LightRec<float>> lights) {
    World w;
    w.name = name;
    w.lights = lights;
    int32_t at = 0;
    for (int k = 0; k <= kNumKinds; ++k) {
        w.kind_begin[k] = at;
        const std::vector<ShapeRec<float>>* run = k == RT_SHAPE_SPHERE ? &spheres : k == RT_SHAPE_PLANE ? &planes : k == RT_SHAPE_CUBE ? &cubes : nullptr;
        if (run) {
            w.shapes.insert(w.shapes.end(), run->begin(), run->end());
            at += (int32_t)run->size();
        }
    }
    return w;
}

static bool empty_rect(const uint32_t r[4]) { return r[0] > r[2] || r[1] > r[3]; }
// the rectangle is empty or its span on `axis` (0: columns, 1: rows) misses pixels [lo, hi]
static bool misses(const uint32_t r[4], int axis, uint32_t lo, uint32_t hi) {
    return empty_rect(r) || r[axis + 2] < lo || r[axis] > hi;
}

struct Tables {
    uint32_t cols[kCullCols], rows[kCullRows];
};
// near spans the restatement met that hold pixels but no whole block and straddle no block edge
// (fill_cull_tables' b1 < b0 case), and ones that end in the ragged last block
static int g_inside_one_block = 0, g_ragged_end = 0;

// Every entry by its definition.
static void restate(const CameraRec<float>& cam, uint32_t w, uint32_t h, const World& wd, const LaunchTerms& terms, Tables& t) {
    std::memset(&t, 0, sizeof t);
    const int ns = (int)wd.shapes.size();
    const uint32_t nc = (w + kCullCellW - 1) / kCullCellW, nr = (h + kCullCellH - 1) / kCullCellH;
    // set bit b where rectangle r misses the block column or the block row
    auto by_rect = [&](const uint32_t r[4], int b) {
        for (uint32_t i = 0; i < nc; ++i)
            if (misses(r, 0, kCullCellW * i, kCullCellW * i + kCullCellW - 1)) t.cols[i] |= 1u << b;
        for (uint32_t j = 0; j < nr; ++j)
            if (misses(r, 1, kCullCellH * j, kCullCellH * j + kCullCellH - 1)) t.rows[j] |= 1u << b;
    };
    for (int s = 0; s < ns; ++s) {
        uint32_t r[4];
        primary_rect(cam, w, h, wd.shapes[s].bound, r);
        by_rect(r, s);
    }
    const int p0 = wd.kind_begin[RT_SHAPE_PLANE], np = wd.kind_begin[RT_SHAPE_PLANE + 1] - p0;
    if (np > 0) {
        PlaneView view;
        PlaneLine lines[kPrimaryRectSlots];
        plane_view(cam, w, h, view);
        for (int p = 0; p < np; ++p) plane_line(view, wd.shapes[p0 + p].inv + 4, terms.head[1 + p], lines[p]);
        for (int p = 0; p < np; ++p) {
            uint32_t r[4];
            plane_rect(view, lines, np, p, r);
            by_rect(r, p0 + p);
        }
    }
    const int nl = (int)wd.lights.size();
    const ShadowLayout lay(wd.kind_begin, nl);
    if (!lay.fits()) return;
    for (int p = p0; p < p0 + np; ++p) {
        const float* row = wd.shapes[p].inv + 4;
        const float n[3] = {row[0], row[1], row[2]}, hp = -row[3];
        uint32_t lo[2] = {0, 0}, hi[2] = {w - 1, h - 1};  // the intersection of the lights' spans, per axis
        for (int l = 0; l < nl; ++l) {
            const float* lp = wd.lights[l].position;
            uint32_t span[4];
            shadow_near(cam, w, h, n, hp, lp, span);
            for (int a = 0; a < 2; ++a) {
                if (span[a] > lo[a]) lo[a] = span[a];
                if (span[a + 2] < hi[a]) hi[a] = span[a + 2];
            }
            for (int c = 0; c < ns; ++c) {
                if (c == p) {
                    if (shadow_self_clear(cam, n, hp, lp))
                        for (uint32_t i = 0; i < nc; ++i) t.cols[i] |= 1u << lay.pair_bit(l, p, c);
                    continue;
                }
                if (lay.is_plane(c)) continue;  // another plane: no bit
                uint32_t r[4];
                shadow_rect(cam, w, h, n, hp, lp, wd.shapes[c].bound, r);
                by_rect(r, lay.pair_bit(l, p, c));
            }
        }
        const uint32_t nb = 1u << lay.near_bit(p);
        const uint32_t cell[2] = {kCullCellW, kCullCellH}, pixels[2] = {w, h};
        for (int a = 0; a < 2; ++a) {
            if (lo[a] > hi[a]) continue;
            g_inside_one_block += (hi[a] + 1) / cell[a] < (lo[a] + cell[a] - 1) / cell[a];
            g_ragged_end += hi[a] == pixels[a] - 1 && pixels[a] % cell[a] != 0;
        }
        for (uint32_t i = 0; i < nc; ++i) {
            const uint32_t first = kCullCellW * i, last = first + kCullCellW - 1 < w - 1 ? first + kCullCellW - 1 : w - 1;
            if (lo[0] <= hi[0] && lo[0] <= first && last <= hi[0]) t.cols[i] |= nb;
        }
        for (uint32_t j = 0; j < nr; ++j) {
            const uint32_t first = kCullCellH * j, last = first + kCullCellH - 1 < h - 1 ? first + kCullCellH - 1 : h - 1;
            if (lo[1] <= hi[1] && lo[1] <= first && last <= hi[1]) t.rows[j] |= nb;
        }
    }
}

struct BitCounts {
    uint32_t primary = 0, shadow = 0;  // entries x bits set below and from kShadowBit0
};

// The function a launch calls against the restatement, every word; twice, for the same answer.
static BitCounts compare(const CameraRec<float>& cam, uint32_t w, uint32_t h, const World& wd, Tables& got) {
    LaunchTerms terms;
    launch_terms(wd.shapes.data(), wd.kind_begin, (int)wd.shapes.size(), cam.origin, terms);
    static Tables want, again;
    std::memset(&got, 0, sizeof got);
    std::memset(&again, 0, sizeof again);
    fill_cull_tables(cam, w, h, wd.shapes.data(), wd.shapes.size(), wd.kind_begin, wd.lights.data(), (int)wd.lights.size(), terms,
                     got.cols, got.rows);
    fill_cull_tables(cam, w, h, wd.shapes.data(), wd.shapes.size(), wd.kind_begin, wd.lights.data(), (int)wd.lights.size(), terms,
                     again.cols, again.rows);
    CHECK(std::memcmp(&got, &again, sizeof got) == 0, "%s %ux%u: two calls, two answers", wd.name, w, h);
    restate(cam, w, h, wd, terms, want);
    BitCounts n;
    const uint32_t low = (1u << kShadowBit0) - 1;
    for (uint32_t i = 0; i < kCullCols; ++i) {
        CHECK(got.cols[i] == want.cols[i], "%s %ux%u: cols[%u] = %08x, by definition %08x", wd.name, w, h, i, got.cols[i], want.cols[i]);
        n.primary += (uint32_t)__builtin_popcount(got.cols[i] & low), n.shadow += (uint32_t)__builtin_popcount(got.cols[i] & ~low);
    }
    for (uint32_t j = 0; j < kCullRows; ++j) {
        CHECK(got.rows[j] == want.rows[j], "%s %ux%u: rows[%u] = %08x, by definition %08x", wd.name, w, h, j, got.rows[j], want.rows[j]);
        n.primary += (uint32_t)__builtin_popcount(got.rows[j] & low), n.shadow += (uint32_t)__builtin_popcount(got.rows[j] & ~low);
    }
    const uint32_t nc = (w + kCullCellW - 1) / kCullCellW, nr = (h + kCullCellH - 1) / kCullCellH;
    for (uint32_t i = nc; i < kCullCols; ++i) CHECK(got.cols[i] == 0, "%s %ux%u: cols[%u] beyond the canvas is %08x", wd.name, w, h, i, got.cols[i]);
    for (uint32_t j = nr; j < kCullRows; ++j) CHECK(got.rows[j] == 0, "%s %ux%u: rows[%u] beyond the canvas is %08x", wd.name, w, h, j, got.rows[j]);
    return n;
}

int main() {
    static const uint32_t kCanvases[][2] = {{1, 1}, {16, 4}, {17, 5}, {64, 48}, {100, 37}, {2048, 2048}};
    static_assert(cull_tables_hold(2048, 2048) && !cull_tables_hold(2049, 2048) && !cull_tables_hold(2048, 2049));
    // the eye of every world: (0, 1.5, -5), looking along +z
    const float ex = 0.0f, ey = 1.5f, ez = -5.0f;
    std::vector<World> worlds;
    // three_sphere's shape: a floor, three spheres, one light
    worlds.push_back(world("three_sphere", {ball(-0.5f, 1, 0.5f, 1), ball(1.5f, 0.5f, -0.5f, 0.5f), ball(-1.5f, 0.33f, -0.75f, 0.33f)},
                           {plane(0, 1, 0, 0)}, {}, {light(-10, 10, -10)}));
    // six slots whose shadow bits fit: 2 + 2 * 5 = 12
    worlds.push_back(world("two planes, four casters",
                           {ball(-2, 1, 1, 1), ball(0, 0.5f, 0, 0.5f), ball(2, 0.7f, 2, 0.7f)}, {plane(0, 1, 0, 0), plane(0, 0, 1, 6)},
                           {ball(1, 0.3f, -2, 0.5f)}, {light(-4, 8, -6)}));
    worlds.push_back(world("one plane, three casters, two lights", {ball(-1, 1, 0, 1), ball(1.5f, 0.4f, -1, 0.4f)}, {plane(0, 1, 0, 0)},
                           {ball(0, 0.5f, 3, 0.9f)}, {light(-10, 10, -10), light(6, 4, -3)}));
    // 3 + 2 * 3 * 4 = 27 > 24: no shadow bits
    worlds.push_back(world("three planes, three casters, two lights", {ball(-1, 1, 0, 1), ball(1.5f, 0.4f, -1, 0.4f), ball(0, 2.5f, 2, 0.5f)},
                           {plane(0, 1, 0, 0), plane(0, 0, 1, 6), plane(1, 0, 0, -5)}, {}, {light(-3, 6, -6), light(3, 5, -2)}));
    // beyond kShadowRectSlots: the primary and plane bits only
    worlds.push_back(world("eight slots",
                           {ball(-3, 0.5f, 0, 0.5f), ball(-2, 0.5f, 1, 0.5f), ball(-1, 0.5f, 2, 0.5f), ball(0, 0.5f, 3, 0.5f), ball(1, 0.5f, 2, 0.5f)},
                           {plane(0, 1, 0, 0), plane(0, 0, 1, 8)}, {ball(2, 0.5f, 1, 0.8f)}, {light(-10, 10, -10)}));
    worlds.push_back(world("no plane", {ball(-0.5f, 1, 0.5f, 1), ball(1.5f, 0.5f, -0.5f, 0.5f), ball(0, 3, 4, 0.25f)}, {}, {}, {light(-10, 10, -10)}));
    worlds.push_back(world("a sphere behind the eye", {ball(0, 1.5f, -9, 1), ball(1, 0.5f, 0, 0.5f)}, {plane(0, 1, 0, 0)}, {}, {light(-10, 10, -10)}));
    worlds.push_back(world("a sphere over the whole canvas", {ball(0, 1.5f, 0, 4), ball(1, 0.5f, -2, 0.25f)}, {plane(0, 1, 0, 0)}, {}, {light(-10, 10, -10)}));
    worlds.push_back(world("lights on both sides of the plane", {ball(-1, 1, 0, 1), ball(1.5f, 0.4f, -1, 0.4f)}, {plane(0, 1, 0, 0)}, {},
                           {light(-5, 6, -4), light(2, -3, 1)}));

    static Tables t;
    for (const World& wd : worlds) {
        const int ns = (int)wd.shapes.size();
        const ShadowLayout lay(wd.kind_begin, (int)wd.lights.size());
        BitCounts total;
        for (const auto& cv : kCanvases) {
            const uint32_t w = cv[0], h = cv[1];
            const CameraRec<float> cam = level_camera(0.5f, w, h, ex, ey, ez);
            const BitCounts n = compare(cam, w, h, wd, t);
            total.primary += n.primary, total.shadow += n.shadow;
            const uint32_t nc = (w + kCullCellW - 1) / kCullCellW, nr = (h + kCullCellH - 1) / kCullCellH;
            if (!lay.fits()) CHECK(n.shadow == 0, "%s %ux%u: shadow bits where the layout does not fit", wd.name, w, h);
            if (!std::strcmp(wd.name, "a sphere behind the eye"))  // slot 0: empty rectangle, every entry
                for (uint32_t i = 0; i < nc + nr; ++i) CHECK((i < nc ? t.cols[i] : t.rows[i - nc]) & 1u, "%s %ux%u: entry %u lacks bit 0", wd.name, w, h, i);
            if (!std::strcmp(wd.name, "a sphere over the whole canvas"))  // slot 0: the whole canvas, no entry
                for (uint32_t i = 0; i < nc + nr; ++i) CHECK(!((i < nc ? t.cols[i] : t.rows[i - nc]) & 1u), "%s %ux%u: entry %u has bit 0", wd.name, w, h, i);
        }
        // (a small ball on a 2048 x 2048 canvas misses most block columns: the tables are not all zero)
        CHECK(total.primary > 0, "%s: no primary bit on any canvas", wd.name);
        if (lay.fits()) CHECK(total.shadow > 0, "%s: no shadow bit on any canvas", wd.name);
        std::printf("%s: %d slots, layout %s, %u primary and %u shadow bits over the canvases\n", wd.name, ns, lay.fits() ? "fits" : "does not fit",
                    total.primary, total.shadow);
    }
    // odd values in a caster's bound and in a light, and now and then in the plane's row and the camera
    int runs = 0;
    for (int it = 0; it < 3000; ++it) {
        World wd = worlds[it % 3];
        const uint32_t w = 1 + rnd() % (it % 100 == 0 ? 2048 : 200), h = 1 + rnd() % (it % 100 == 0 ? 2048 : 120);
        CameraRec<float> cam = level_camera(uni(0.1f, 1.2f), w, h, uni(-3, 3), uni(0.2f, 4), uni(-8, -2));
        const int casters = wd.kind_begin[RT_SHAPE_PLANE];
        for (int k = 0; k < 2; ++k) wd.shapes[rnd() % casters].bound[rnd() % 4] = odd_value();
        wd.lights[rnd() % wd.lights.size()].position[rnd() % 3] = odd_value();
        if (it % 5 == 0) wd.shapes[wd.kind_begin[RT_SHAPE_PLANE]].inv[4 + rnd() % 4] = odd_value();
        if (it % 7 == 0) (rnd() % 2 ? cam.origin[rnd() % 3] : cam.inv[rnd() % 12]) = odd_value();
        wd.name = "odd values";
        compare(cam, w, h, wd, t);
        ++runs;
    }
    std::printf("%d runs with odd values\n", runs);
    // lights near the end of their reach over the plane: narrow near spans, down to parts of one block
    g_inside_one_block = g_ragged_end = 0;
    for (int it = 0; it < 2000; ++it) {
        World wd = worlds[it % 3];
        const uint32_t w = 1 + rnd() % 120, h = 1 + rnd() % 60;
        const CameraRec<float> cam = level_camera(uni(0.2f, 1.2f), w, h, uni(-3, 3), uni(0.5f, 30), uni(-8, -2));
        for (LightRec<float>& l : wd.lights) l.position[0] = uni(-40, 40), l.position[1] = uni(60, 89), l.position[2] = uni(-10, 80);
        wd.name = "narrow spans";
        compare(cam, w, h, wd, t);
    }
    std::printf("narrow spans: %d inside one block, %d ending in a ragged last block\n", g_inside_one_block, g_ragged_end);
    CHECK(g_inside_one_block > 0 && g_ragged_end > 0, "the narrow spans never met the one-block case or the ragged end");
    std::printf("%d failed checks\n", g_failed);
    if (g_failed) return 1;
    std::printf("ok\n");
    return 0;
}
