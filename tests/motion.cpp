// CPU checks of the host side of motion (csrc/shape_identity.hpp with
// velocities, csrc/rtc_internal.hpp shutter_time), compiled stand-alone by
// tests/test_motion_cpu.py.  Prints one line per check and "ok".
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ray-tracer-challenge-rs_amd/csrc/rtc_internal.hpp"
#include "../ray-tracer-challenge-rs_amd/csrc/shape_identity.hpp"

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

static rt_shape_desc sphere_at(double x) {
    rt_shape_desc d;
    std::memset(&d, 0, sizeof d);
    d.kind = RT_SHAPE_SPHERE;
    for (int i = 0; i < 16; ++i) d.inverse[i] = i % 5 == 0 ? 1.0 : 0.0;
    d.inverse[3] = -x;
    return d;
}

int main() {
    // ---- 1: value identity with velocities
    {
        rt_material_desc mat;
        std::memset(&mat, 0, sizeof mat);
        mat.pattern = -1;
        // shapes 0..4 are one value; 5 is elsewhere
        std::vector<rt_shape_desc> s = {sphere_at(1), sphere_at(1), sphere_at(1), sphere_at(1), sphere_at(1), sphere_at(2)};
        const double va[3] = {1.0, 0.0, 0.0}, vb[3] = {1.0, 0.0, 0.0}, vc[3] = {1.0, 0.0, 1e-300}, vz[3] = {0.0, -0.0, 0.0};
        std::vector<uint32_t> cls;
        CHECK(ident::shape_classes(s.data(), 6, &mat, nullptr, cls) == 4, "without velocities: five of one class");
        // 0 static, 1 and 2 with equal velocities (two arrays of equal values), 3 another velocity, 4 static, 5 moving
        const double* vel[6] = {nullptr, va, vb, vc, nullptr, va};
        const uint32_t dups = ident::shape_classes(s.data(), 6, &mat, nullptr, cls, nullptr, nullptr, vel);
        std::printf("classes with velocities: %u %u %u %u %u %u (%u duplicates)\n", cls[0], cls[1], cls[2], cls[3], cls[4], cls[5], dups);
        CHECK(dups == 2, "two shapes equal an earlier one");
        CHECK(cls[0] == 0 && cls[4] == 0, "the static ones stay one class");
        CHECK(cls[1] == 1 && cls[2] == 1, "equal velocities, equal shapes: one class");
        CHECK(cls[3] == 3, "a velocity that differs in its last bit: a class of its own");
        CHECK(cls[5] == 5, "another transformation: a class of its own whatever the velocity");
        CHECK(!ident::velocity_eq(nullptr, va) && ident::velocity_eq(nullptr, nullptr) && ident::velocity_eq(va, vb),
              "a static shape equals no mover");
        // (a zero velocity never reaches the classes: the upload drops it; as values +0 and -0 are equal)
        const double pz[3] = {0.0, 0.0, 0.0};
        CHECK(ident::velocity_eq(vz, pz), "-0 == +0 as f64 values");
    }
    // ---- 2: the shutter's time, both precisions, against the formula written out
    {
        for (uint32_t n = 1; n <= 4; ++n) {
            ShutterParams<double> sp{0.25, 1.5, 1.0 / (double)(n * n), RT_JITTER_NONE, 0u};
            ShutterParams<float> sf{0.25f, 1.5f, 1.0f / (float)(n * n), RT_JITTER_NONE, 0u};
            for (uint32_t j = 0; j < n; ++j)
                for (uint32_t i = 0; i < n; ++i) {
                    const double u = ((double)(j * n + i) + 0.5) * (1.0 / (double)(n * n));
                    const double su = 1.5 * u;
                    CHECK(shutter_time(sp, n, 7, 3, 2, i, j) == 0.25 + su, "cell centres, n = %u", n);
                    CHECK(std::fabs((double)shutter_time(sf, n, 7, 3, 2, i, j) - (0.25 + su)) < 1e-6, "f32 cell centres, n = %u", n);
                }
            // hashed: every cell of a pixel is taken once, and the time lies in its cell
            sp.jitter = RT_JITTER_HASHED;
            sp.tk = hash_mix(77u ^ kShutterKey);
            std::vector<int> seen(n * n, 0);
            for (uint32_t j = 0; j < n; ++j)
                for (uint32_t i = 0; i < n; ++i) {
                    const double tau = shutter_time(sp, n, 7, 5, 4, i, j);
                    const double u = (tau - 0.25) / 1.5;
                    CHECK(u >= 0.0 && u < 1.0, "hashed time inside the shutter");
                    const int cell = (int)std::floor(u * n * n + 1e-9);
                    if (cell >= 0 && cell < (int)(n * n)) ++seen[cell];
                }
            for (uint32_t c = 0; c < n * n; ++c) CHECK(seen[c] == 1, "hashed, n = %u: cell %u taken %d times", n, c, seen[c]);
        }
        std::printf("shutter times: cell centres exact, hashed cells a permutation, n = 1..4\n");
    }
    // ---- 3: the records' layouts the motion build relies on
    {
        CHECK(sizeof(MotionArg) == 16 && sizeof(RayBatchTimedArg) == 32, "argument sizes");
        constexpr size_t lens_f = offsetof(ShutterArg<float>, lens), lens_d = offsetof(ShutterArg<double>, lens);
        CHECK(lens_f == 0 && lens_d == 0, "the lens leads the frame argument");
        CHECK((kShapeMoving & (kShapeClosed | kShapeClassEnd | kShapeSimilar | kShapeAxisAligned | kShapeSmooth | kShapeUV)) == 0 &&
                  kShapeMoving < (1 << kShapeClassShift),
              "kShapeMoving is a flag bit of its own below the class");
        constexpr size_t moving_at = offsetof(InstRec<float>, moving);
        CHECK(moving_at + 4 == sizeof(InstRec<float>), "InstRec::moving takes the old pad word");
    }
    std::printf(g_failed ? "%d checks failed\n" : "ok\n", g_failed);
    return g_failed ? 1 : 0;
}
