// cull_tables.hpp — the per-scene f32 direct kernel's cull tables for one
// launch (host only): the rectangles of primary_rect.hpp as miss bits per
// block column and block row (rtc_internal.hpp LaunchParams::cull_cols,
// cull_rows, ShadowLayout).  What rtc_host.cpp's launch uploads, as a function
// of plain records, so tests/cull_tables.cpp can state every word a second
// time, by definition, and compare.
#pragma once

#include <cstddef>
#include <cstdint>

#include "primary_rect.hpp"
#include "rtc_internal.hpp"

namespace rtc {

// The canvases the tables span.
constexpr bool cull_tables_hold(uint32_t width, uint32_t height) {
    return width <= kCullCols * kCullCellW && height <= kCullRows * kCullCellH;
}

// The per-scene direct kernel's primary cull: each slot's screen
// rectangle for this camera (primary_rect.hpp), from the f32 bounds
// the kernel's own ball test reads, as miss bits per block column and
// block row (rtc_internal.hpp), and above them the shadow cull's bits
// for waves that hit one plane (shadow_rect).  Recomputed every launch
// (the camera is the call's argument): a conic per slot and per
// (light, plane, caster), well under a microsecond for a small world.
//
// `shapes`: the n_shapes <= kPrimaryRectSlots f32 records of the whole world,
// by kind (kind_begin as DevScene's); `lights`: the n_lights f32 lights the
// kernel holds as constants (0: no shadow bits); `terms`: the launch terms of
// the same camera (launch_terms.hpp: the planes' heights).  The canvas must
// lie within the tables (cull_tables_hold).  Writes the entries of the
// canvas's block columns and block rows, cols[0 .. ceil(width / 16)) and
// rows[0 .. ceil(height / 4)); the entries behind them are left as they are
// (a launch's are zero).
inline void fill_cull_tables(const CameraRec<float>& cam, uint32_t width, uint32_t height, const ShapeRec<float>* shapes,
                             size_t n_shapes, const int32_t* kind_begin, const LightRec<float>* lights, int n_lights,
                             const LaunchTerms& terms, uint32_t cols[kCullCols], uint32_t rows[kCullRows]) {
    const size_t ns = n_shapes;
    const uint32_t nc = (width + kCullCellW - 1) / kCullCellW, nr = (height + kCullCellH - 1) / kCullCellH;
    // Each bit changes at a few edges only, so the tables are built
    // from toggles: flip_*[i] holds the bits that change value between
    // entry i - 1 and entry i, and one running XOR fills the entries.
    uint32_t flip_cols[kCullCols + 1] = {}, flip_rows[kCullRows + 1] = {};
    // bit `b` set outside the rectangle's block columns and block rows
    auto outside = [&](const uint32_t r[4], uint32_t b) {
        const bool none = r[0] > r[2] || r[1] > r[3];  // empty: every block misses
        const uint32_t c0 = none ? nc : r[0] / kCullCellW, c1 = none ? nc : r[2] / kCullCellW + 1;
        const uint32_t r0 = none ? nr : r[1] / kCullCellH, r1 = none ? nr : r[3] / kCullCellH + 1;
        flip_cols[0] ^= b, flip_cols[c0] ^= b, flip_cols[c1] ^= b;
        flip_rows[0] ^= b, flip_rows[r0] ^= b, flip_rows[r1] ^= b;
    };
    for (size_t s = 0; s < ns; ++s) {
        uint32_t r[4];
        primary_rect(cam, width, height, shapes[s].bound, r);
        outside(r, 1u << s);
    }
    // A plane's bit: the blocks where its entry lies behind the eye or
    // another plane's is nearer (plane_rect), from the records' rows
    // and the heights the kernel reads (`terms`).
    const int p0 = kind_begin[RT_SHAPE_PLANE], np = kind_begin[RT_SHAPE_PLANE + 1] - p0;
    if (np > 0) {
        PlaneView pv;
        PlaneLine pl[kPrimaryRectSlots];
        plane_view(cam, width, height, pv);
        for (int p = 0; p < np; ++p) plane_line(pv, shapes[p0 + p].inv + 4, terms.head[1 + p], pl[p]);
        for (int p = 0; p < np; ++p) {
            uint32_t r[4];
            plane_rect(pv, pl, np, p, r);
            outside(r, 1u << (p0 + p));
        }
    }
    // The shadow cull's bits (rtc_internal.hpp ShadowLayout), from the
    // f32 records and lights the per-scene kernel holds as constants.
    const ShadowLayout lay(kind_begin, n_lights);
    if (lay.fits()) {
        for (int p = lay.plane0; p < lay.plane0 + lay.planes; ++p) {
            const ShapeRec<float>& pl = shapes[p];
            const float n[3] = {pl.inv[4], pl.inv[5], pl.inv[6]}, h = -pl.inv[7];  // object y = n . x - h
            uint32_t near[4] = {0, 0, width - 1, height - 1};  // the columns and rows within every light's reach
            for (int l = 0; l < lay.lights; ++l) {
                const float* lp = lights[l].position;
                uint32_t sp[4];
                shadow_near(cam, width, height, n, h, lp, sp);
                for (int a = 0; a < 2; ++a) {
                    near[a] = sp[a] > near[a] ? sp[a] : near[a];
                    near[a + 2] = sp[a + 2] < near[a + 2] ? sp[a + 2] : near[a + 2];
                }
                for (size_t c = 0; c < ns; ++c) {
                    const int bit = lay.pair_bit(l, p, (int)c);
                    if (bit < 0) continue;
                    if ((int)c == p) {  // the plane itself: every block or none
                        if (shadow_self_clear(cam, n, h, lp)) flip_cols[0] ^= 1u << bit;
                        continue;
                    }
                    uint32_t r[4];
                    shadow_rect(cam, width, height, n, h, lp, shapes[c].bound, r);
                    outside(r, 1u << bit);
                }
            }
            // whole blocks inside the span (the canvas's last, ragged block ends with the canvas)
            auto blocks = [](uint32_t lo, uint32_t hi, uint32_t cell, uint32_t pixels, uint32_t& b0, uint32_t& b1) {
                b0 = b1 = 0;
                if (lo > hi) return;
                b0 = (lo + cell - 1) / cell;
                b1 = hi + 1 >= pixels ? (pixels + cell - 1) / cell : (hi + 1) / cell;
                if (b1 < b0) b1 = b0;
            };
            const uint32_t nb = 1u << lay.near_bit(p);
            uint32_t b0, b1;
            blocks(near[0], near[2], kCullCellW, width, b0, b1);
            flip_cols[b0] ^= nb, flip_cols[b1] ^= nb;
            blocks(near[1], near[3], kCullCellH, height, b0, b1);
            flip_rows[b0] ^= nb, flip_rows[b1] ^= nb;
        }
    }
    uint32_t acc = 0;
    for (uint32_t i = 0; i < nc; ++i) cols[i] = acc ^= flip_cols[i];
    acc = 0;
    for (uint32_t j = 0; j < nr; ++j) rows[j] = acc ^= flip_rows[j];
}

}  // namespace rtc
