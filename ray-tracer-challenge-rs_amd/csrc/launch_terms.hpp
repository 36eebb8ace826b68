// launch_terms.hpp — the launch terms of the per-scene f32 direct kernel
// (rtc_internal.hpp LaunchTerms, rtc_kernels.hip closest_hit and
// prepare_hit_const): what the kernel's tests form from a primary ray's
// origin alone, worked out once per launch on the host.
//
// The values must be the device's bits, so only IEEE f32 operations are
// used, each in the kernel's own operand order: fmaf where the kernel fuses
// (kfma), and max, which is exact.  The translation unit that includes this
// is built with contraction off, like the kernels (-ffp-contract=off).  No
// reciprocal and no root goes in: the hardware's are not correctly rounded.
// tests/launch_terms.cpp states the kernel's expressions a second time and
// compares bit for bit.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "rtc_internal.hpp"

namespace rtc {

// kfma of the per-scene build (rtc_kernels.hip): the record's matrix entries
// are compile-time constants there, and a zero entry's term is dropped.
inline float launch_kfma(float m, float x, float acc) { return m == 0.0f ? acc : std::fmaf(m, x, acc); }

// The terms of a world of `n` slots (n <= kPrimaryRectSlots; kind_begin as
// DevScene's) for rays from `origin`.  Every field of `out` is written.
inline void launch_terms(const ShapeRec<float>* shapes, const int32_t* kind_begin, int n, const float origin[3],
                         LaunchTerms& out) {
    std::memset(&out, 0, sizeof out);
    // surface_offset's max over the origin (max is exact, its order free)
    out.head[0] = std::fmax(std::fmax(std::fabs(origin[0]), std::fabs(origin[1])), std::fabs(origin[2]));
    const int p0 = kind_begin[RT_SHAPE_PLANE], p1 = kind_begin[RT_SHAPE_PLANE + 1];
    for (int s = p0; s < p1 && s < n && s < kPrimaryRectSlots; ++s) {
        // lo.y of xform_point(inv, origin): a left fold from the translation
        const float* m = shapes[s].inv;
        out.head[1 + s - p0] = launch_kfma(m[6], origin[2], launch_kfma(m[5], origin[1], launch_kfma(m[4], origin[0], m[7])));
    }
}

}  // namespace rtc
