// Host check of the direct kernel's plane rectangles (csrc/primary_rect.hpp
// plane_view, plane_line, plane_rect), compiled stand-alone by
// tests/test_plane_rects_sanitizers.py with the address and
// undefined-behaviour sanitizers where the compiler has them.
//
// The function a launch runs, on the edge inputs of tests/test_plane_rects.py
// (parallel, nearly parallel and coincident planes, an eye on and next to a
// plane, sheared and unevenly scaled rows) and on the ones only a program can
// feed it: NaN, infinite, zero, denormal and huge rows, heights and cameras,
// singular camera matrices, canvases of one pixel and of 2048 x 2048, eight
// planes at once.  Every answer must be a rectangle of the canvas or the empty
// rectangle {~0, ~0, 0, 0}, the same when asked again, and the whole canvas
// where the inputs admit no cull; a room seen from inside must split as the
// geometry says.  Prints one line per check and "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../ray-tracer-challenge-rs_amd/csrc/launch_terms.hpp"
#include "../ray-tracer-challenge-rs_amd/csrc/primary_rect.hpp"

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

static float height_of(const float row[4], const float o[3]) {
    return launch_kfma(row[2], o[2], launch_kfma(row[1], o[1], launch_kfma(row[0], o[0], row[3])));
}

// every rectangle of the set; returns how many are smaller than the canvas
static int rects_of(const CameraRec<float>& cam, uint32_t w, uint32_t h, const float (*rows)[4], int n, uint32_t out[][4],
                    const char* what) {
    PlaneView view;
    PlaneLine lines[kPrimaryRectSlots];
    plane_view(cam, w, h, view);
    for (int p = 0; p < n; ++p) plane_line(view, rows[p], height_of(rows[p], cam.origin), lines[p]);
    int culled = 0;
    for (int q = 0; q < n; ++q) {
        uint32_t again[4];
        plane_rect(view, lines, n, q, out[q]);
        plane_rect(view, lines, n, q, again);
        CHECK(std::memcmp(out[q], again, sizeof again) == 0, "%s: plane %d: two calls, two answers", what, q);
        const uint32_t* r = out[q];
        const bool empty = r[0] == ~0u && r[1] == ~0u && r[2] == 0 && r[3] == 0;
        CHECK(empty || (r[0] <= r[2] && r[1] <= r[3] && r[2] <= w - 1 && r[3] <= h - 1), "%s: plane %d: {%u, %u, %u, %u} on %u x %u",
              what, q, r[0], r[1], r[2], r[3], w, h);
        culled += empty || r[0] != 0 || r[1] != 0 || r[2] != w - 1 || r[3] != h - 1;
    }
    return culled;
}

static bool is_full(const uint32_t r[4], uint32_t w, uint32_t h) { return r[0] == 0 && r[1] == 0 && r[2] == w - 1 && r[3] == h - 1; }

int main() {
    uint32_t r[kPrimaryRectSlots][4];

    // a room seen from inside: a floor at y = 0, walls at x = -5 and x = +5, the eye at (0, 1, -5)
    {
        const uint32_t w = 640, h = 360;
        const CameraRec<float> cam = level_camera(0.6f, w, h, 0.0f, 1.0f, -5.0f);
        const float rows[3][4] = {{0, 1, 0, 0}, {1, 0, 0, 5}, {-1, 0, 0, 5}};
        const int culled = rects_of(cam, w, h, rows, 3, r, "room");
        CHECK(culled == 3, "room: %d of 3 rectangles cull", culled);
        CHECK(r[0][1] > h / 2 - 4 && r[0][3] == h - 1 && r[0][0] == 0 && r[0][2] == w - 1, "room: the floor lies below the horizon");
        // (pixel 0 looks along wx = +half_width, world x < 0: the wall at x = -5 is the left one)
        CHECK(r[1][0] == 0 && r[1][2] < w / 2 + 4 && r[2][0] > w / 2 - 4 && r[2][2] == w - 1, "room: the walls split at the centre");
        std::printf("room: floor from row %u, walls {%u..%u} and {%u..%u}\n", r[0][1], r[1][0], r[1][2], r[2][0], r[2][2]);
    }
    // pairs that no margin separates: coincident, the same plane from the other side, the eye on a plane
    {
        const uint32_t w = 333, h = 201;
        const CameraRec<float> cam = level_camera(0.5f, w, h, 0.3f, 1.5f, -4.0f);
        const float same[2][4] = {{0, 1, 0, 0}, {0, 1, 0, 0}};
        rects_of(cam, w, h, same, 2, r, "coincident");
        CHECK(r[0][1] == r[1][1] && r[0][1] > 0 && r[0][3] == h - 1, "coincident: both keep the half below the horizon");
        const float flip[2][4] = {{0, 1, 0, 0}, {0, -2, 0, 0}};
        rects_of(cam, w, h, flip, 2, r, "flipped");
        CHECK(r[0][1] == r[1][1] && r[0][3] == h - 1 && r[1][3] == h - 1, "flipped: both keep the half below the horizon");
        const float on[2][4] = {{0, 1, 0, -1.5f}, {0, 0, 1, -6}};  // the eye in the first plane; a wall ahead
        rects_of(cam, w, h, on, 2, r, "eye on a plane");
        CHECK(is_full(r[0], w, h) && is_full(r[1], w, h), "eye on a plane: no cull for the pair");
        const float near_[2][4] = {{0, 1, 0, -1.4999999f}, {0, 0, 1, -6}};  // 1e-7 below the eye
        rects_of(cam, w, h, near_, 2, r, "eye next to a plane");
        const float par[2][4] = {{0, 1, 0, 0}, {0, 1, 0, 2}};  // floors at y = 0 and y = -2
        rects_of(cam, w, h, par, 2, r, "parallel");
        // (at the horizon itself both entries run off to infinity and no margin parts them)
        CHECK(r[1][3] - r[1][1] <= 6 && r[1][1] + 8 > r[0][1] && !is_full(r[0], w, h), "parallel: the lower floor keeps a band at the horizon");
        std::printf("pairs: ok\n");
    }
    // a plane behind the camera, a single pixel, the largest canvas of the tables
    {
        const CameraRec<float> cam = level_camera(0.4f, 64, 48, 0, 0, 0);
        const float behind[1][4] = {{0, 0, 1, 3}};  // z = -3
        rects_of(cam, 64, 48, behind, 1, r, "behind");
        CHECK(r[0][0] == ~0u, "behind: empty");
        const CameraRec<float> one = level_camera(0.4f, 1, 1, 0, 1, 0);
        const float floor_[2][4] = {{0, 1, 0, 0}, {0, 0, 1, -3}};
        rects_of(one, 1, 1, floor_, 2, r, "one pixel");
        const CameraRec<float> big = level_camera(1.2f, 2048, 2048, 0, 1, 0);
        rects_of(big, 2048, 2048, floor_, 2, r, "2048 x 2048");
        std::printf("canvases: ok\n");
    }
    // random and odd inputs: up to eight planes, odd values in rows, cameras and sizes
    int sets = 0, culled = 0;
    for (int it = 0; it < 20000; ++it) {
        const uint32_t w = 1 + rnd() % (it % 50 == 0 ? 2048 : 400), h = 1 + rnd() % (it % 50 == 0 ? 2048 : 300);
        CameraRec<float> cam = level_camera(uni(0.1f, 1.5f), w, h, uni(-8, 8), uni(-8, 8), uni(-8, 8));
        for (int i = 0; i < 12; ++i)
            if (i % 4 != 3) cam.inv[i] = uni(-1.5f, 1.5f);
        const int odd = it % 4;  // 0: plain; 1: odd rows; 2: an odd camera; 3: both
        if (odd & 2) {
            for (int k = 0; k < 3; ++k) {
                const uint32_t at = rnd() % 18;
                if (at < 12) cam.inv[at] = odd_value();
                else if (at < 15) cam.origin[at - 12] = odd_value();
                else (at == 15 ? cam.half_width : at == 16 ? cam.half_height : cam.pixel_size) = odd_value();
            }
            if (rnd() % 4 == 0)
                for (int i = 0; i < 4; ++i) cam.inv[8 + i] = cam.inv[i];  // singular
        }
        const int n = 1 + (int)(rnd() % kPrimaryRectSlots);
        float rows[kPrimaryRectSlots][4];
        for (int p = 0; p < n; ++p) {
            const float scale = std::pow(10.0f, uni(-3, 3));
            for (int k = 0; k < 3; ++k) rows[p][k] = uni(-1, 1) * scale;
            rows[p][3] = uni(-10, 10) * scale;
            if (p > 0 && rnd() % 4 == 0) {  // parallel to, nearly parallel to or the same as the one before
                std::memcpy(rows[p], rows[p - 1], sizeof rows[p]);
                const uint32_t how = rnd() % 3;
                if (how == 0) rows[p][3] += uni(-3, 3) * scale;
                if (how == 1) rows[p][rnd() % 3] *= 1.0f + uni(-1e-4f, 1e-4f);
            }
            if (rnd() % 8 == 0)  // through the eye, to f32's last bit or so
                rows[p][3] = -(rows[p][0] * cam.origin[0] + rows[p][1] * cam.origin[1] + rows[p][2] * cam.origin[2]);
            if (odd & 1)
                for (int k = 0; k < 2; ++k) rows[p][rnd() % 4] = odd_value();
        }
        culled += rects_of(cam, w, h, rows, n, r, "random") > 0;
        ++sets;
    }
    std::printf("%d random sets, %d with a cull\n", sets, culled);
    CHECK(culled > sets / 10, "the random sets hardly ever cull");
    std::printf("%d failed checks\n", g_failed);
    if (g_failed) return 1;
    std::printf("ok\n");
    return 0;
}
