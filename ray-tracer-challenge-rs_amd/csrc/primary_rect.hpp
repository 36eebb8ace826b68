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

// The conic's extent on the canvas, shared by the primary cull and the shadow
// cull below (shadow_rect): the pixels whose camera vector v = (wx, wy, -1)
// satisfies (q . v)^2 - k v^T G v >= 0 for q = m^T oc, G = m^T m and
// k = |oc|^2 - R^2, i.e. whose line along m v passes within R of oc.  Returns
// kConicFull (rect untouched) where no ellipse bounds them (the origin in or
// on the ball, a conic that is no ellipse, anything not finite), kConicOff
// when the ellipse lies off the canvas, else kConicRect with `rect` the
// ellipse's pixel rectangle widened by one pixel on each side.
enum ConicExtent { kConicFull, kConicOff, kConicRect };
struct ConicForm {
    double ad[3][3];  // adj(C), C = D (q q^T - k G) D
};
// the conic of (m, oc, R): false = kConicFull
inline bool conic_form(const double m[3][3], const double oc[3], double R, ConicForm& f) {
    double g[3][3] = {}, q[3] = {}, oo = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) g[i][j] += m[k][i] * m[k][j];
    for (int i = 0; i < 3; ++i) oo += oc[i] * oc[i];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) q[i] += m[k][i] * oc[k];
    const double k = oo - R * R;
    if (!(k > 1e-6 * oo) || !std::isfinite(k)) return false;  // the origin in or on the ball
    // C = D (q q^T - k G) D and its adjugate (both symmetric)
    double c[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[i][j] = (q[i] * q[j] - k * g[i][j]) * ((i == 2) != (j == 2) ? -1.0 : 1.0);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            f.ad[i][j] = c[i1][j1] * c[i2][j2] - c[i1][j2] * c[i2][j1];  // cofactor (symmetric: no transpose)
        }
    // an ellipse, by a margin that keeps the adjugate's cancellation harmless
    return f.ad[2][2] > 1e-6 * (std::fabs(c[0][0] * c[1][1]) + c[0][1] * c[0][1]);
}
inline ConicExtent conic_extent(const ConicForm& f, double hw, double hh, double ps, uint32_t width, uint32_t height,
                                uint32_t rect[4]) {
    if (!(ps > 0.0) || !std::isfinite(hw) || !std::isfinite(hh)) return kConicFull;
    const auto& ad = f.ad;
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
    uint32_t r[4] = {0, 0, width - 1, height - 1};
    if (!extent(0, hw, width, r[0], r[2]) || !extent(1, hh, height, r[1], r[3])) return kConicOff;
    for (int i = 0; i < 4; ++i) rect[i] = r[i];
    return kConicRect;
}

inline void rect_full(uint32_t width, uint32_t height, uint32_t rect[4]) {
    rect[0] = rect[1] = 0;
    rect[2] = width - 1;
    rect[3] = height - 1;
}
inline void rect_empty(uint32_t rect[4]) {
    rect[0] = rect[1] = ~0u;
    rect[2] = rect[3] = 0;
}

// {x0, y0, x1, y1}, inclusive; empty (x0 > x1, y0 > y1) as {~0, ~0, 0, 0}.  width, height >= 1.
inline void primary_rect(const CameraRec<float>& cam, uint32_t width, uint32_t height, const float bound[4],
                         uint32_t rect[4]) {
    rect_full(width, height, rect);
    const double r2 = bound[3];
    if (!(r2 >= 0.0) || !std::isfinite(r2)) return;
    double m[3][3];  // camera -> world: d_world = M v
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m[i][j] = cam.inv[4 * i + j];
    double oc[3], oo = 0.0, mag = 0.0;
    for (int i = 0; i < 3; ++i) {
        oc[i] = (double)bound[i] - (double)cam.origin[i];
        oo += oc[i] * oc[i];
        mag += std::fabs((double)bound[i]) + std::fabs((double)cam.origin[i]);
    }
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
    ConicForm f;
    if (!conic_form(m, oc, R, f)) return;
    if (cz > 0.0) return rect_empty(rect);  // wholly behind the eye plane
    if (conic_extent(f, cam.half_width, cam.half_height, cam.pixel_size, width, height, rect) == kConicOff) rect_empty(rect);
}

// The shadow cull of the same kernel (rtc_kernels.hip any_hit, the instances
// of shade_hit_const for a wave whose hits all lie on one plane): which pixel
// blocks can a caster's bounding ball shadow on a plane n . x = h, for a light
// at l?  The primary ray of pixel v = (wx, wy, -1) meets the plane at
// x = o + t M v, t = (h - n.o) / (n . M v), so
//     x - l = A v / (n . M v),   A = (o - l)(n^T M) + (h - n.o) M:
// as seen from the light the hit lies along A v, and "the line from the light
// through the hit passes within R of the caster's centre c" is the conic above
// with A in place of M and cl = c - l in place of oc.  It is a double cone:
// n . M v changes sign across the plane's horizon on the canvas, so no side
// is dropped (pixels beyond the horizon hit nothing and cost nothing).
//
// What the kernel tests is one of two forms, with tl = l - over, tt = |tl|^2,
// d the unit vector from the over-point to the light and oc = c - over:
//     light side:  (|cl|^2 kKeep - r^2) tt <= (cl . tl)^2,  cl . tl <= 0
//     first form:  (|oc|^2 kKeep - r^2) |d|^2 <= (oc . d)^2,  front
// Both bound the distance D of c from the line through the light and the
// over-point: D^2 <= r^2 + 1e-5 |cl|^2 and D^2 <= r^2 + 1e-5 |oc|^2, plus
// rounding of ~12 ulp of the products.  The second grows with the distance
// s = |x - l| of the hit (|oc| <= |cl| + s): far enough away every ray
// passes it, whatever the caster (s > 316 |cl|), so no rectangle short of a
// band along the plane's horizon holds its pixels.  A wave takes that form
// only when one of its lanes has tt > kLightCullFar^2 = 100^2, so the cull is
// split by the distance from the light:
//   - shadow_rect speaks for hits within S0 = kShadowReach = 99 of the light,
//     whose waves take the light-side form: R^2 = r^2 + 2e-5 |cl|^2, as
//     primary_rect's (the second 1e-5 is ~80 times the rounding);
//   - shadow_near gives the pixel columns and rows of the canvas whose every
//     hit on the plane lies within S0 (1 - 2e-3) of the light.  The launch
//     lets a block take the rectangles' bits only inside those (one bit per
//     plane, rtc_internal.hpp ShadowLayout::near_bit), so a wave with a hit
//     beyond S0, the only kind that can take the first form, runs the
//     per-lane tests as before.
//
// R is then grown as the angle sin(theta) = R / |cl| seen from the light:
//   - the f32 rounding of cl (slip, as in primary_rect);
//   - the over-point: it lies off the plane point x by the offset, at most
//     3e-5 max(1, |p|inf, |o|inf) (a plane takes 1.9e-6 of that maximum, the
//     other kinds 3e-5 max(1, |p|inf)), and p itself is rounded to an ulp.
//     With |p|inf <= |l|inf + s and s >= d that moves the hit, seen from the
//     light, by an angle of at most 3e-5 ((1 + |l|inf + |o|inf) / d + 1);
//   - t = -y_o / y_d carries the relative rounding of y_d = n . d, about
//     2e-7 t / e for an eye at height e over the plane, which slides the hit
//     along its ray by 2e-7 t^2 / e: seen from the light, at s >= max(d,
//     t - |o - l|), an angle of at most 2e-7 / e times the larger of
//     (|o - l| + d)^2 / d and (S0 + |o - l|)^2 / S0, taken five times.
// The sum is taken four times over.  The ray's own rounding (1e-7 of the
// direction) stays far below the one-pixel margin, as for primary rays.
//
// The whole canvas (no cull): r^2 negative or not finite, the light in or
// next to the ball, a shadow that reaches the horizon (no ellipse), the eye
// or the light on the plane (by 1e-4 and 1e-3 of the scene's scale), the
// light farther than 0.9 S0 from the plane, a singular A, anything not finite.
constexpr double kShadowReach = 99.0;  // < any_hit's kLightCullFar = 100
struct ShadowFrame {
    double a[3][3];  // A above
    double mv[3];    // n^T M, signed so that mv . v > 0 where the primary ray meets the plane
    double o[3], l[3];
    double eye, d;   // heights of the eye and the light over the plane (> 0; they may lie on opposite sides)
    double s0;       // the reach of the cull from the light
    double hw, hh, ps;
};
// false: no cull for this plane and light
inline bool shadow_frame(const CameraRec<float>& cam, const float n[3], float h, const float light[3], ShadowFrame& s) {
    double m[3][3], nn = 0.0, no = 0.0, nl = 0.0, omax = 0.0, lmax = 0.0;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) m[i][j] = cam.inv[4 * i + j];
        s.o[i] = cam.origin[i];
        s.l[i] = light[i];
        nn += (double)n[i] * n[i];
        no += (double)n[i] * s.o[i];
        nl += (double)n[i] * s.l[i];
        omax = std::fmax(omax, std::fabs(s.o[i]));
        lmax = std::fmax(lmax, std::fabs(s.l[i]));
    }
    nn = std::sqrt(nn);
    if (!(nn > 0.0) || !std::isfinite(nn)) return false;
    const double e = (double)h - no;  // (h - n.o), the numerator of t
    s.eye = std::fabs(e) / nn;
    s.d = std::fabs((double)h - nl) / nn;
    const double scale = 1.0 + omax + lmax + std::fabs((double)h) / nn;
    if (!(s.eye > 1e-4 * scale) || !(s.d > 1e-3 * scale) || !std::isfinite(s.eye) || !std::isfinite(s.d)) return false;
    s.s0 = kShadowReach;
    if (!(s.d < 0.9 * s.s0)) return false;
    const double sgn = e > 0.0 ? 1.0 : -1.0;
    double frob = 0.0;
    for (int j = 0; j < 3; ++j) {
        double t = 0.0;
        for (int k = 0; k < 3; ++k) t += (double)n[k] * m[k][j];
        s.mv[j] = sgn * t;
        for (int i = 0; i < 3; ++i) {
            s.a[i][j] = (s.o[i] - s.l[i]) * t + e * m[i][j];
            frob += s.a[i][j] * s.a[i][j];
        }
    }
    const auto& a = s.a;
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                       a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    if (!std::isfinite(det) || !std::isfinite(frob) || !(std::fabs(det) > 1e-9 * frob * std::sqrt(frob))) return false;
    s.hw = cam.half_width, s.hh = cam.half_height, s.ps = cam.pixel_size;
    return s.ps > 0.0 && std::isfinite(s.hw) && std::isfinite(s.hh) && std::isfinite(s.ps);
}

// The inclusive rectangle that holds every pixel whose f32 primary ray meets
// the plane (n, h) at t > 0 within the reach of the light and whose shadow
// ray to `light` passes either form of any_hit's cull of the ball `bound`.
// Inputs as the kernel reads them (the plane: row 1 of the record's inverse,
// n = inv[4..6], h = -inv[7]).  Empty as primary_rect's.
inline void shadow_rect(const CameraRec<float>& cam, uint32_t width, uint32_t height, const float n[3], float h,
                        const float light[3], const float bound[4], uint32_t rect[4]) {
    rect_full(width, height, rect);
    const double r2 = bound[3];
    if (!(r2 >= 0.0) || !std::isfinite(r2)) return;
    ShadowFrame s;
    if (!shadow_frame(cam, n, h, light, s)) return;
    double cl[3], cc = 0.0, mag = 0.0, ol = 0.0, omax = 0.0, lmax = 0.0;
    for (int i = 0; i < 3; ++i) {
        cl[i] = (double)bound[i] - s.l[i];
        cc += cl[i] * cl[i];
        mag += std::fabs((double)bound[i]) + std::fabs(s.l[i]);
        ol += (s.o[i] - s.l[i]) * (s.o[i] - s.l[i]);
        omax = std::fmax(omax, std::fabs(s.o[i]));
        lmax = std::fmax(lmax, std::fabs(s.l[i]));
    }
    const double lc = std::sqrt(cc), eye_l = std::sqrt(ol);
    const double R0 = std::sqrt(r2 + 2e-5 * cc) + 2.4e-7 * mag;
    const double slide = std::fmax((eye_l + s.d) * (eye_l + s.d) / s.d, (s.s0 + eye_l) * (s.s0 + eye_l) / s.s0);
    const double turn = 3e-5 * ((1.0 + lmax + omax) / s.d + 1.0) + 1e-6 * slide / s.eye;
    const double sine = (R0 / lc + 4.0 * turn) * (1.0 + 1e-5);
    if (!(sine < 0.999) || !std::isfinite(sine)) return;  // the light in or next to the ball
    ConicForm f;
    if (!conic_form(s.a, cl, lc * sine, f)) return;
    if (conic_extent(f, s.hw, s.hh, s.ps, width, height, rect) == kConicOff) rect_empty(rect);
}

// The pixel columns [span[0], span[2]] and rows [span[1], span[3]] of the
// canvas, inclusive, in which every pixel that meets the plane at all meets it
// within S0 (1 - 2e-3) of the light: the hits within S form a disc of the
// plane, the canvas maps onto the plane projectively (where mv . v > 0), so
// the pixels in question form a convex set K of the canvas, a band of rows
// lies in K when its four corners do, and along one canvas edge K is an
// interval: where S (mv . v) >= |A v|, a quadratic in the pixel coordinate.
// The edges are taken one pixel outside the canvas and the interval is drawn
// in by one pixel.  An axis with no such band is empty (lo > hi: ~0, 0).
inline void shadow_near(const CameraRec<float>& cam, uint32_t width, uint32_t height, const float n[3], float h,
                        const float light[3], uint32_t span[4]) {
    span[0] = span[1] = ~0u;
    span[2] = span[3] = 0;
    ShadowFrame s;
    if (!shadow_frame(cam, n, h, light, s)) return;
    const double S = s.s0 * (1.0 - 2e-3);
    auto near_at = [&](double px, double py) {
        const double v[3] = {s.hw - (px + 0.5) * s.ps, s.hh - (py + 0.5) * s.ps, -1.0};
        double f = 0.0, gg = 0.0;
        for (int i = 0; i < 3; ++i) {
            f += s.mv[i] * v[i];
            const double g = s.a[i][0] * v[0] + s.a[i][1] * v[1] + s.a[i][2] * v[2];
            gg += g * g;
        }
        return f > 0.0 && S * S * f * f >= gg;
    };
    // the pixels u of the line (px, py) + u (dx, dy), as reals, that lie in K: false = none
    auto line_span = [&](double px, double py, double dx, double dy, double& lo, double& hi) {
        const double v0[3] = {s.hw - (px + 0.5) * s.ps, s.hh - (py + 0.5) * s.ps, -1.0}, dv[3] = {-dx * s.ps, -dy * s.ps, 0.0};
        double f0 = 0.0, f1 = 0.0, qa = 0.0, qb = 0.0, qc = 0.0;
        for (int i = 0; i < 3; ++i) {
            f0 += s.mv[i] * v0[i];
            f1 += s.mv[i] * dv[i];
            const double g0 = s.a[i][0] * v0[0] + s.a[i][1] * v0[1] + s.a[i][2] * v0[2];
            const double g1 = s.a[i][0] * dv[0] + s.a[i][1] * dv[1] + s.a[i][2] * dv[2];
            qa -= g1 * g1;
            qb -= g0 * g1;
            qc -= g0 * g0;
        }
        qa += S * S * f1 * f1, qb += S * S * f0 * f1, qc += S * S * f0 * f0;  // Q(u) = qa u^2 + 2 qb u + qc >= 0
        const double disc = qb * qb - qa * qc;
        if (!std::isfinite(disc) || !(disc > 0.0) || qa == 0.0) return false;  // (a band that grazes K, or none: no cull)
        const double root = std::sqrt(disc);
        const double u1 = (-qb - root) / qa, u2 = (-qb + root) / qa;  // qa < 0: u2 < u1
        if (qa < 0.0) {  // between the roots, on the side of the plane the rays meet
            lo = u2, hi = u1;
            return f0 + f1 * 0.5 * (lo + hi) > 0.0;
        }
        // beyond one root, the one on the side where mv . v grows
        if (f1 > 0.0) lo = u2, hi = HUGE_VAL;
        else if (f1 < 0.0) lo = -HUGE_VAL, hi = u1;
        else return false;
        return true;
    };
    auto axis = [&](bool rows, uint32_t n_pix, uint32_t n_other, uint32_t& lo, uint32_t& hi) {
        double lo_a, hi_a, lo_b, hi_b;
        const double e0 = -1.0, e1 = (double)n_other;  // the two edges, a pixel outside
        if (rows ? !line_span(e0, 0.0, 0.0, 1.0, lo_a, hi_a) || !line_span(e1, 0.0, 0.0, 1.0, lo_b, hi_b)
                 : !line_span(0.0, e0, 1.0, 0.0, lo_a, hi_a) || !line_span(0.0, e1, 1.0, 0.0, lo_b, hi_b))
            return;
        const double a = std::fmax(std::fmax(lo_a, lo_b), -1.0), b = std::fmin(std::fmin(hi_a, hi_b), (double)n_pix);
        if (!(a <= b)) return;
        // (the corners once more, directly: rounding of the roots must not let a far corner in)
        const double ai = std::ceil(a), bi = std::floor(b);
        if (!(ai <= bi)) return;
        if (rows ? !near_at(e0, ai) || !near_at(e1, ai) || !near_at(e0, bi) || !near_at(e1, bi)
                 : !near_at(ai, e0) || !near_at(ai, e1) || !near_at(bi, e0) || !near_at(bi, e1))
            return;
        if (ai + 1.0 > bi - 1.0) return;
        lo = (uint32_t)(ai + 1.0);
        hi = (uint32_t)(bi - 1.0);
    };
    axis(false, width, height, span[0], span[2]);
    axis(true, height, width, span[1], span[3]);
}

// The plane as its own caster: with the eye and the light on one side of it,
// by a margin that dwarfs f32 rounding, the over-point of a hit seen from the
// eye lies on the light's side too and the segment to the light never crosses
// the plane: the kernel's side test (any_hit: object y of the over-point and
// of the light of one sign, |y_over| <= 1e4 |y_light|) skips it for every
// lane.  y_over is the offset, at most 1.9e-6 |n| max(1, |p|inf, |o|inf) plus
// a few ulp, with |p|inf <= |o|inf + t and t <= eye / 8e-8 (the plane's entry
// is taken for |y_d| >= 8e-8 only): asked to stay below 1e3 |y_light|.  (On
// opposite sides the light lies behind the surface, l . n < 0, and no shadow
// ray is traced at all: nothing to cull.)
inline bool shadow_self_clear(const CameraRec<float>& cam, const float n[3], float h, const float light[3]) {
    double nn = 0.0, no = 0.0, nl = 0.0, omax = 0.0, lmax = 0.0;
    for (int i = 0; i < 3; ++i) {
        nn += (double)n[i] * n[i];
        no += (double)n[i] * cam.origin[i];
        nl += (double)n[i] * light[i];
        omax = std::fmax(omax, std::fabs((double)cam.origin[i]));
        lmax = std::fmax(lmax, std::fabs((double)light[i]));
    }
    nn = std::sqrt(nn);
    if (!(nn > 0.0) || !std::isfinite(nn)) return false;
    const double ye = (no - (double)h) / nn, yl = (nl - (double)h) / nn;  // signed heights
    const double scale = 1.0 + omax + lmax + std::fabs((double)h) / nn;
    if (!std::isfinite(ye) || !std::isfinite(yl) || !(ye * yl > 0.0)) return false;
    if (!(std::fabs(ye) > 1e-3 * scale) || !(std::fabs(yl) > 1e-3 * scale)) return false;
    const double over_max = 3e-6 * (1.0 + omax + std::fabs(ye) * nn / 8e-8);  // (t in object units of y)
    return over_max <= 1e3 * std::fabs(yl);
}

// The primary cull of a plane (rtc_kernels.hip closest_hit, RTC_PLANE_RECTS):
// the rectangle outside which plane q cannot be the nearest entry of a primary
// ray, because its own entry lies behind the origin or because another
// plane's entry in front is nearer.  Both questions are linear in the pixel.
//
// Pixel (x, y) looks along D = M v, v = (wx, wy, -1) as above, affine in
// (x, y).  The kernel tests plane i (row 1 of its record's inverse: n_i, and
// the launch term h_i = n_i . o + inv[7], the origin's object-space height)
// with
//     ld = n_i . d,  d = D / |D|;   valid: |ld| >= 8e-8;   t_i = rcp(ld) (-h_i),
// an entry in front iff it is valid and t_i >= 0.  With s_i = -h_i,
// g_i = |n_i| / |s_i| and
//     u_i(x, y) = (n_i . D) / s_i        (affine in the pixel),
// 1 / t_i = u_i / |D| =: w_i, so the entry is in front iff u_i > 0 and, where
// both are, t_p < t_q iff u_p > u_q: half-planes of the canvas.
//
// What the kernel evaluates, in f32 (eta = 2^-24 a rounding):
//   - wx = half_width - (x + 0.5) pixel_size: two roundings of values up to
//     2 half_width, |dwx| <= 3 eta half_width; likewise wy;
//   - D_k, three fused terms: three roundings of partial sums bounded by
//     S_k = |M_k0| half_width + |M_k1| half_height + |M_k2|, plus dwx and dwy
//     carried through: |dD_k| <= 6 eta S_k, |dD| <= 6 eta |S|;
//   - d = D rsq(|D|^2): the sum of squares to 3 eta, v_rsq_f32 to an ulp
//     (2 eta) and half the sum's error, the product one more: the direction
//     turns by at most 2 |dD| / |D| and its length is off by 5 eta;
//   - ld, three fused terms: 3 eta |n_i| |d|;
// so the cosine c_i = n_i . D / (|n_i| |D|) reaches the kernel as ld / |n_i|
// within
//     eps = 2 eta (6 |S| / Dmin + 5),   Dmin = 1 / |M^-1|_F <= |D|  (|v| >= 1),
// and t_i = rcp(ld) s_i adds v_rcp_f32's ulp and the product's rounding,
// 4 eta of t_i: |1 / t_i - w_i| <= 4 eta |w_i| + 1.001 eps g_i.  Every margin
// below is 100 times that bound:
//   - plane i counts as behind the origin only where c_i sign(s_i) < -tau_i,
//     and as in front and valid only where it is > tau_i,
//     tau_i = 100 eps + 1e-6 / |n_i| (the second for the validity test);
//   - p counts as nearer than q only where
//         w_p (1 - kappa) - w_q (1 + kappa) > 100.1 eps (g_p + g_q) + 1.001 tau_q g_q,
//     kappa = 400 eta.  The last term covers a q whose true entry lies just
//     behind the origin (w_q in [-tau_q g_q, 0)) and which the kernel may see
//     just in front of it: there w_p (1 - kappa) alone exceeds 100 times the
//     bound.  Elsewhere the two entries differ by 99 times the bound, some 400
//     ulp of t, so neither the reciprocal's nor the root's last bit reorders
//     them.
// The inequalities are taken in u = w |D| with the right sides times
// Dmax >= |D| (|D| is convex in the pixel: the largest of the corners).
//
// Against one p, the pixels where q may still be the nearest plane are
//     A_q and (p possibly not in front)  or  A_q and (p not clearly nearer),
// A_q = the canvas where q is possibly in front: two convex polygons, the
// canvas cut by two half-planes each.  The rectangle is the bounding box of
// their union, intersected over p (plane_rect below intersects the polygons
// themselves where it can), rounded outward and widened by a pixel.
// Coincident and nearly coincident planes, ties that the world index would
// break and an eye on or next to a plane never separate by the margin: no
// cull for that pair.  A plane whose numbers leave the range where f32 keeps
// t normal (|n|, |h| / |n| outside 1e-15 .. 1e15, anything not finite) is not
// culled and culls nothing; a singular or non-finite camera culls nothing.
struct PlaneView {
    bool ok = false;
    double m[3][3];      // camera -> world
    double hw, hh, ps;   // as the kernel reads them
    double eps, dmax;
    uint32_t width, height;
};
inline void plane_view(const CameraRec<float>& cam, uint32_t width, uint32_t height, PlaneView& v) {
    v.ok = false;
    v.width = width, v.height = height;
    v.hw = cam.half_width, v.hh = cam.half_height, v.ps = cam.pixel_size;
    auto& m = v.m;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m[i][j] = cam.inv[4 * i + j];
    if (!(v.ps > 0.0) || !std::isfinite(v.hw) || !std::isfinite(v.hh) || !std::isfinite(v.ps)) return;
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    double adj2 = 0.0, s2 = 0.0;  // |adj(M)|_F^2, |S|^2
    for (int i = 0; i < 3; ++i) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        for (int j = 0; j < 3; ++j) {
            const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            const double c = m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
            adj2 += c * c;
        }
        const double s = std::fabs(m[i][0]) * (std::fabs(v.hw) + v.ps) + std::fabs(m[i][1]) * (std::fabs(v.hh) + v.ps) +
                         std::fabs(m[i][2]);
        s2 += s * s;
    }
    if (!std::isfinite(det) || !std::isfinite(adj2) || !std::isfinite(s2) || !(std::fabs(det) > 1e-12 * std::sqrt(adj2) * std::sqrt(s2)))
        return;
    const double dmin = std::fabs(det) / std::sqrt(adj2);
    v.dmax = 0.0;
    for (int c = 0; c < 4; ++c) {  // the corners, a pixel outside the canvas
        const double wx = v.hw - ((c & 1 ? (double)width : -1.0) + 0.5) * v.ps, wy = v.hh - ((c & 2 ? (double)height : -1.0) + 0.5) * v.ps;
        double dd = 0.0;
        for (int i = 0; i < 3; ++i) {
            const double d = m[i][0] * wx + m[i][1] * wy - m[i][2];
            dd += d * d;
        }
        v.dmax = std::fmax(v.dmax, std::sqrt(dd));
    }
    constexpr double eta = 1.0 / 16777216.0;
    v.eps = 2.0 * eta * (6.0 * std::sqrt(s2) / dmin + 5.0);
    v.ok = std::isfinite(v.eps) && std::isfinite(v.dmax) && v.eps < 1e-3 && v.dmax > 0.0;
}
// u_i = a x + b y + c over the pixels, and its margins (already times Dmax)
struct PlaneLine {
    bool ok = false;
    double a, b, c;
    double side;  // tau_i g_i Dmax
    double gap;   // 100.1 eps g_i Dmax
};
// row = {n, inv[7]}: row 1 of the record's inverse; h = the launch term (launch_terms.hpp)
inline void plane_line(const PlaneView& v, const float row[4], float h, PlaneLine& l) {
    l.ok = false;
    if (!v.ok) return;
    const double n[3] = {row[0], row[1], row[2]}, s = -(double)h;
    const double nn = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), sa = std::fabs(s);
    if (!std::isfinite(nn) || !std::isfinite(sa) || !(nn > 1e-15) || !(nn < 1e15) || !(sa > 1e-15 * nn) || !(sa < 1e15 * nn)) return;
    double nm[3];
    for (int j = 0; j < 3; ++j) nm[j] = (n[0] * v.m[0][j] + n[1] * v.m[1][j] + n[2] * v.m[2][j]) / s;
    l.a = -nm[0] * v.ps;
    l.b = -nm[1] * v.ps;
    l.c = nm[0] * (v.hw - 0.5 * v.ps) + nm[1] * (v.hh - 0.5 * v.ps) - nm[2];
    const double g = nn / sa;
    l.side = (100.0 * v.eps + 1e-6 / nn) * g * v.dmax;
    l.gap = 100.1 * v.eps * g * v.dmax;
    // (finite, and far from where the clipping's products could overflow)
    l.ok = std::fabs(l.a) < 1e100 && std::fabs(l.b) < 1e100 && std::fabs(l.c) < 1e100 && l.side < 1e100 && l.gap < 1e100;
}
struct PlanePoly {
    static constexpr int kMax = 16;  // the canvas's four corners and one more per cut (at most 1 + 7 cuts)
    int n = 0;
    double x[kMax], y[kMax];
    // keep a x + b y + c >= 0 (a convex polygon gains at most one corner)
    void clip(double a, double b, double c) {
        double ox[kMax], oy[kMax], f[kMax];
        for (int i = 0; i < n; ++i) f[i] = a * x[i] + b * y[i] + c;
        int k = 0;
        for (int i = 0; i < n && k + 2 <= kMax; ++i) {
            const int j = i + 1 == n ? 0 : i + 1;
            if (f[i] >= 0.0) ox[k] = x[i], oy[k] = y[i], ++k;
            if ((f[i] >= 0.0) != (f[j] >= 0.0)) {
                const double t = f[i] / (f[i] - f[j]);
                ox[k] = x[i] + t * (x[j] - x[i]), oy[k] = y[i] + t * (y[j] - y[i]), ++k;
            }
        }
        n = k;
        for (int i = 0; i < k; ++i) x[i] = ox[i], y[i] = oy[i];
    }
    void extend(double box[4]) const {  // {x0, y0, x1, y1}
        for (int i = 0; i < n; ++i) {
            box[0] = std::fmin(box[0], x[i]), box[1] = std::fmin(box[1], y[i]);
            box[2] = std::fmax(box[2], x[i]), box[3] = std::fmax(box[3], y[i]);
        }
    }
};
// The rectangle of plane q among `n` planes (lines[i] of plane i, n <= kPrimaryRectSlots); as primary_rect's.
// Where p is in front on all of what is left of A_q (the usual case: a room's
// walls and floor), the pixels where q may win form one convex polygon, and
// the cuts of the planes p accumulate in it; a p that may lie behind the eye
// somewhere in it bounds the rectangle by the box of its two polygons instead.
inline void plane_rect(const PlaneView& v, const PlaneLine* lines, int n, int q, uint32_t rect[4]) {
    rect_full(v.width, v.height, rect);
    if (!v.ok || q < 0 || q >= n || n > kPrimaryRectSlots || !lines[q].ok) return;
    const PlaneLine& lq = lines[q];
    constexpr double kappa = 400.0 / 16777216.0;
    PlanePoly aq;  // the canvas (a pixel outside it) where q is possibly in front
    aq.n = 4;
    aq.x[0] = aq.x[3] = -1.0, aq.x[1] = aq.x[2] = (double)v.width;
    aq.y[0] = aq.y[1] = -1.0, aq.y[2] = aq.y[3] = (double)v.height;
    aq.clip(lq.a, lq.b, lq.c + lq.side);
    double box[4] = {-HUGE_VAL, -HUGE_VAL, HUGE_VAL, HUGE_VAL};
    for (int p = 0; p < n && aq.n; ++p) {
        if (p == q || !lines[p].ok) continue;
        const PlaneLine& lp = lines[p];
        PlanePoly behind = aq;
        behind.clip(-lp.a, -lp.b, lp.side - lp.c);  // p possibly not in front
        const double rhs = lp.gap + lq.gap + 1.001 * lq.side;
        const double la = lq.a * (1.0 + kappa) - lp.a * (1.0 - kappa), lb = lq.b * (1.0 + kappa) - lp.b * (1.0 - kappa),
                     lc = rhs + lq.c * (1.0 + kappa) - lp.c * (1.0 - kappa);  // >= 0: p not clearly nearer
        if (behind.n == 0) {
            aq.clip(la, lb, lc);
            continue;
        }
        PlanePoly level = aq;
        level.clip(la, lb, lc);
        double bp[4] = {HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
        behind.extend(bp);
        level.extend(bp);
        box[0] = std::fmax(box[0], bp[0]), box[1] = std::fmax(box[1], bp[1]);
        box[2] = std::fmin(box[2], bp[2]), box[3] = std::fmin(box[3], bp[3]);
    }
    double bq[4] = {HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    aq.extend(bq);
    box[0] = std::fmax(box[0], bq[0]), box[1] = std::fmax(box[1], bq[1]);
    box[2] = std::fmin(box[2], bq[2]), box[3] = std::fmin(box[3], bq[3]);
    if (!(box[0] == box[0]) || !(box[1] == box[1]) || !(box[2] == box[2]) || !(box[3] == box[3])) return;  // NaN: no cull
    const double x0 = std::floor(box[0]) - 1.0, y0 = std::floor(box[1]) - 1.0, x1 = std::ceil(box[2]) + 1.0, y1 = std::ceil(box[3]) + 1.0;
    const double xm = (double)(v.width - 1), ym = (double)(v.height - 1);
    if (!(x0 <= x1) || !(y0 <= y1) || x1 < 0.0 || y1 < 0.0 || x0 > xm || y0 > ym) return rect_empty(rect);
    rect[0] = (uint32_t)(x0 < 0.0 ? 0.0 : x0), rect[1] = (uint32_t)(y0 < 0.0 ? 0.0 : y0);
    rect[2] = (uint32_t)(x1 > xm ? xm : x1), rect[3] = (uint32_t)(y1 > ym ? ym : y1);
}
}  // namespace rtc
