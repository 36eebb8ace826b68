// primary_rect.hpp — the screen rectangle of a shape's bounding ball for one
// camera (host, f64): the per-launch primary cull of the per-scene f32 direct
// kernel (rtc_internal.hpp LaunchParams::primary_rect, rtc_kernels.hip
// closest_hit).  Acceleration only: the rectangle must hold every pixel whose
// primary ray passes the kernel's per-lane ball test (wave_ball_may_hit), so a
// wave whose pixel block misses it may pass the shape by.
//
// Every primary ray starts at the camera's origin, so the test is a question
// about pixels.  Pixel (x, y) looks along M v, v = (wx, wy, -1) with
// wx = half_width - (x + 0.5) pixel_size (camera_ray) and M the linear part
// of the camera's inverse transformation.  M need not be a rotation
// (view_transform's rows are unit only for an `up` at right angles to the
// view), so the ball is taken to the rays, not the rays to the ball: with
// oc = centre - origin, q = M^T oc, G = M^T M and k = |oc|^2 - R^2 > 0 (the
// eye outside the ball), the line along M v passes within R of the centre iff
//     (q . v)^2 - k v^T G v >= 0,
// a quadric cone v^T A v >= 0, A = q q^T - k G.  On the canvas plane
// h = (wx, wy, 1) it is the conic h^T C h >= 0, C = D A D, D = diag(1, 1, -1),
// an ellipse iff its leading 2 x 2 minor is positive: the ball then lies
// wholly on one side of the eye plane, in front (the centre's camera z < 0)
// or behind.  The ellipse's extent in wx ends at the two vertical tangents,
// lines l = (1, 0, -c) with l^T adj(C) l = 0:
//     c = (C*_02 +- sqrt(C*_02^2 - C*_00 C*_22)) / C*_22,   C* = adj(C),
// and likewise in wy with index 1.  (For M = I, centre (a_x, a_y, -b):
// c = (a b +- R sqrt(a^2 + b^2 - R^2)) / (b^2 - R^2), the tangents from the
// eye to a circle.)  The slopes map to pixels by inverting wx above, and the
// rectangle is widened by one pixel on each side.
//
// What the kernel tests is not the ball itself but
//     (|oc|^2 kKeep - r^2) |d|^2 <= (oc . d)^2   (front: oc . d >= 0 or inside)
// in f32, kKeep = 1 - 1e-5: a ball of r^2 + 1e-5 |oc|^2, plus rounding of a
// few ulp of |oc|^2 |d|^2.  R^2 here is r^2 + 2e-5 |oc|^2 (the second 1e-5 is
// ~80 times that rounding), R is then grown by the f32 rounding of oc itself.
// The f32 rounding of the ray (direction to ~1e-7, wx to ~1e-7 half_width)
// stays far below the one-pixel margin (canvases up to tens of thousands of
// pixels a side).
//
// The inputs are the f32 values the kernel reads (CameraRec<float>, the
// record's bound), so both sides speak of the same ball and the same camera.
// Full canvas (no cull) when the eye is inside the ball or the ball reaches
// the eye plane, when r^2 is not a finite number >= 0 (unbounded shapes,
// RTC_DEBUG=cull=0) and when M is singular or anything is not finite.  A ball
// wholly behind the eye plane meets no primary ray: an empty rectangle.
#pragma once

#include <cmath>
#include <cstdint>

#include "rtc_internal.hpp"

namespace rtc {

// {x0, y0, x1, y1}, inclusive; empty (x0 > x1, y0 > y1) as {~0, ~0, 0, 0}.  width, height >= 1.
inline void primary_rect(const CameraRec<float>& cam, uint32_t width, uint32_t height, const float bound[4],
                         uint32_t rect[4]) {
    auto full = [&] {
        rect[0] = rect[1] = 0;
        rect[2] = width - 1;
        rect[3] = height - 1;
    };
    auto empty = [&] {
        rect[0] = rect[1] = ~0u;
        rect[2] = rect[3] = 0;
    };
    full();
    const double r2 = bound[3];
    if (!(r2 >= 0.0) || !std::isfinite(r2)) return;
    double m[3][3], g[3][3] = {};  // camera -> world: d_world = M v
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m[i][j] = cam.inv[4 * i + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) g[i][j] += m[k][i] * m[k][j];
    double oc[3], q[3] = {}, oo = 0.0, mag = 0.0;
    for (int i = 0; i < 3; ++i) {
        oc[i] = (double)bound[i] - (double)cam.origin[i];
        oo += oc[i] * oc[i];
        mag += std::fabs((double)bound[i]) + std::fabs((double)cam.origin[i]);
    }
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) q[i] += m[k][i] * oc[k];
    // the kernel forms oc in f32: each component within an ulp of the larger
    // operand, so its |oc| is within `slip` of this one
    const double slip = 2.4e-7 * mag;
    const double R = (std::sqrt(r2 + 2e-5 * oo) + slip) * (1.0 + 1e-5);  // the kernel's ball
    const double k = oo - R * R;
    if (!(k > 1e-6 * oo) || !std::isfinite(k)) return;  // the eye in or on the ball
    // camera z of the centre, up to the positive factor det(M)^2: (M^-1 oc)_z det(M) = row 2 of adj(M) . oc
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    const double cz = ((m[1][0] * m[2][1] - m[1][1] * m[2][0]) * oc[0] - (m[0][0] * m[2][1] - m[0][1] * m[2][0]) * oc[1] +
                       (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * oc[2]) * det;
    if (!std::isfinite(cz) || !std::isfinite(det) || det == 0.0) return;
    // C = D (q q^T - k G) D and its adjugate (both symmetric)
    double c[3][3], ad[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[i][j] = (q[i] * q[j] - k * g[i][j]) * ((i == 2) != (j == 2) ? -1.0 : 1.0);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            ad[i][j] = c[i1][j1] * c[i2][j2] - c[i1][j2] * c[i2][j1];  // cofactor (symmetric: no transpose)
        }
    // an ellipse, by a margin that keeps the adjugate's cancellation harmless
    if (!(ad[2][2] > 1e-6 * (std::fabs(c[0][0] * c[1][1]) + c[0][1] * c[0][1]))) return;
    if (cz > 0.0) return empty();  // wholly behind the eye plane
    const double hw = cam.half_width, hh = cam.half_height, ps = cam.pixel_size;
    if (!(ps > 0.0) || !std::isfinite(hw) || !std::isfinite(hh)) return;
    // pixels [lo, hi] of one axis: half = half_width or half_height, n = pixels
    auto extent = [&](int ax, double half, uint32_t n, uint32_t& lo, uint32_t& hi) {
        const double disc = ad[ax][2] * ad[ax][2] - ad[ax][ax] * ad[2][2];
        if (!(disc >= 0.0)) return true;  // (not a real ellipse, or NaN: keep the full extent)
        const double root = std::sqrt(disc);
        const double w_min = (ad[ax][2] - root) / ad[2][2], w_max = (ad[ax][2] + root) / ad[2][2];
        // w = half - (p + 0.5) ps: the larger slope is the smaller pixel
        const double p_lo = std::floor((half - w_max) / ps - 0.5) - 1.0;
        const double p_hi = std::ceil((half - w_min) / ps - 0.5) + 1.0;
        if (!(p_lo == p_lo) || !(p_hi == p_hi)) return true;  // NaN: keep the full extent
        if (p_hi < 0.0 || p_lo > (double)(n - 1)) return false;
        lo = (uint32_t)(p_lo < 0.0 ? 0.0 : p_lo);
        hi = (uint32_t)(p_hi > (double)(n - 1) ? (double)(n - 1) : p_hi);
        return true;
    };
    if (!extent(0, hw, width, rect[0], rect[2]) || !extent(1, hh, height, rect[1], rect[3])) empty();
}

}  // namespace rtc
