// CPU check of the per-scene direct kernel's launch terms
// (csrc/launch_terms.hpp launch_terms, rtc_internal.hpp LaunchTerms), compiled
// stand-alone by tests/test_launch_terms_cpu.py with contraction off, and with
// the address and undefined-behaviour sanitizers where the compiler has them.
//
// The host's terms must be the bits the kernel's lanes compute, so the
// kernel's expressions (rtc_kernels.hip xform_point with kfma's dropped zero
// terms, Real<float>::surface_offset) are stated here a second time, lane-wise
// and in the kernel's operand order, and compared bit for bit over random
// records and origins: zero and negative-zero matrix entries, origins on an
// axis, tiny and huge ones.  The function must also write every field (the
// same bytes into a zeroed and into a dirtied table) and give the same table
// when called again.  Prints one line per check and "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

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

static uint32_t bits(float v) {
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

// a small deterministic generator (xorshift)
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() >> 8) * (1.0f / 16777216.0f); }
// a matrix entry or coordinate: often an exact zero of either sign, 1 or -1, else any magnitude
static float entry(float scale) {
    switch (rnd() % 8) {
        case 0: return 0.0f;
        case 1: return -0.0f;
        case 2: return 1.0f;
        case 3: return -1.0f;
        case 4: return uniform(-1e-6f, 1e-6f) * scale;
        case 5: return uniform(-1e4f, 1e4f) * scale;
        default: return uniform(-3.0f, 3.0f) * scale;
    }
}

// ---- the kernel's expressions, per lane (rtc_kernels.hip)
struct V {
    float x, y, z;
};
// kfma: a per-scene build drops a term whose matrix entry is a zero
static float k_fma(float m, float x, float acc) {
    if (m == 0.0f) return acc;
    return fmaf(m, x, acc);
}
static V k_xform_point(const float* m, V p) {
    return {k_fma(m[2], p.z, k_fma(m[1], p.y, k_fma(m[0], p.x, m[3]))),
            k_fma(m[6], p.z, k_fma(m[5], p.y, k_fma(m[4], p.x, m[7]))),
            k_fma(m[10], p.z, k_fma(m[9], p.y, k_fma(m[8], p.x, m[11])))};
}
static float k_surface_scale_flat(V p, V o) {  // surface_offset's mo
    const float mp = fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fmaxf(fabsf(p.z), 1.0f));
    return fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), mp));
}

static void check_world(int n_spheres, int n_planes, int n_cubes, int round) {
    const int n = n_spheres + n_planes + n_cubes;
    int32_t kb[kNumKinds + 1];
    for (int k = 0; k <= kNumKinds; ++k)
        kb[k] = k <= RT_SHAPE_SPHERE ? 0 : k <= RT_SHAPE_PLANE ? n_spheres : k <= RT_SHAPE_CUBE ? n_spheres + n_planes : n;
    std::vector<ShapeRec<float>> sh((size_t)n);
    for (ShapeRec<float>& r : sh) {
        std::memset(&r, 0, sizeof r);
        for (float& m : r.inv) m = entry(1.0f);
        for (int i = 0; i < 3; ++i) r.bound[i] = entry(4.0f);
        r.bound[3] = rnd() % 6 == 0 ? HUGE_VALF : rnd() % 6 == 0 ? -1.0f : uniform(0.0f, 30.0f);
        for (float& t : r.tri) t = entry(4.0f);
        r.flags = rnd() % 2 ? kShapeSimilar : 0;
    }
    const V o = {entry(5.0f), entry(5.0f), entry(5.0f)};
    const float origin[3] = {o.x, o.y, o.z};
    LaunchTerms a, b;
    std::memset(&a, 0, sizeof a);
    std::memset(&b, 0xA5, sizeof b);
    launch_terms(sh.data(), kb, n, origin, a);
    launch_terms(sh.data(), kb, n, origin, b);
    CHECK(std::memcmp(&a, &b, sizeof a) == 0, "round %d: a field is left unwritten", round);
    launch_terms(sh.data(), kb, n, origin, b);
    CHECK(std::memcmp(&a, &b, sizeof a) == 0, "round %d: a second call differs", round);
    int planes = 0;
    for (int s = 0; s < n && s < kPrimaryRectSlots; ++s) {
        const bool plane = s >= n_spheres && s < n_spheres + n_planes;
        if (!plane) continue;
        const V want = k_xform_point(sh[(size_t)s].inv, o);  // closest_hit's lo; a plane's test reads lo.y
        const float got = a.head[1 + s - n_spheres];
        CHECK(bits(got) == bits(want.y), "round %d slot %d: the plane's height: %a != %a", round, s, got, want.y);
        ++planes;
    }
    for (int i = 1 + planes; i < kPrimaryRectSlots + 4; ++i)
        CHECK(bits(a.head[i]) == 0, "round %d: head[%d] past the planes is not zero", round, i);
    // the offset scale of a flat kind's hit at any point p
    for (int i = 0; i < 16; ++i) {
        const V p = {entry(10.0f), entry(10.0f), entry(10.0f)};
        const float mp = fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fmaxf(fabsf(p.z), 1.0f));
        const float with_terms = fmaxf(fmaxf(fabsf(a.head[0]), fabsf(a.head[0])), fmaxf(fabsf(a.head[0]), mp));
        CHECK(bits(with_terms) == bits(k_surface_scale_flat(p, o)), "round %d: the offset scale", round);
    }
}

int main() {
    int rounds = 0;
    for (int i = 0; i < 4000; ++i, ++rounds) {
        const int total = 1 + (int)(rnd() % 10);  // (past the cap too: the first kPrimaryRectSlots slots are written)
        const int ns = (int)(rnd() % (uint32_t)(total + 1)), np = (int)(rnd() % (uint32_t)(total - ns + 1));
        check_world(ns, np, total - ns - np, i);
    }
    // the eye in a plane, and a mirrored plane: heights of +0 and -0
    {
        ShapeRec<float> r[2];
        std::memset(r, 0, sizeof r);
        r[0].inv[0] = r[0].inv[5] = r[0].inv[10] = 1.0f;
        r[1].inv[0] = r[1].inv[10] = 1.0f, r[1].inv[5] = -1.0f, r[1].inv[7] = -0.0f;
        int32_t kb[kNumKinds + 1];
        for (int k = 0; k <= kNumKinds; ++k) kb[k] = k <= RT_SHAPE_PLANE ? 0 : 2;
        const float origin[3] = {0.0f, 0.0f, -5.0f};
        LaunchTerms t;
        launch_terms(r, kb, 2, origin, t);
        CHECK(bits(t.head[1]) == bits(0.0f), "the eye in the plane: %a", t.head[1]);
        CHECK(bits(t.head[2]) == bits(-0.0f), "the mirrored plane: %a", t.head[2]);
        CHECK(bits(t.head[0]) == bits(5.0f), "origin_max %a", t.head[0]);
    }
    std::printf("%d worlds, %d failed checks\n", rounds, g_failed);
    if (g_failed) return 1;
    std::printf("ok\n");
    return 0;
}
