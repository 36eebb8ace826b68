// tri_tree.hpp — a bounding-ball hierarchy over a world's triangle records
// (host build, header only; rtc_host.cpp build_scene, tests/tri_tree.cpp).
//
// The kernels' triangle step visits every record of the triangle run
// (rtc_kernels.hip for_kind), one ball test per record and wave.  A mesh of N
// triangles makes that N tests per closest_hit, per light in any_hit and per
// containers walk.  The tree groups the bounded records (rtc_host.cpp
// bounding_sphere gives them a padded ball) under nested balls, so a wave
// passes a whole subtree by on one test (rtc_kernels.hip for_triangles).
//
// Layout: nodes in depth-first preorder.  A node is a ball, a skip link (the
// index of the first node after its subtree) and, for a leaf, a run of
// records [first, first + count) of the reordered triangle run; an inner
// node's count is 0.  The walk needs no stack: at node i, a miss goes to
// skip, a hit runs the node's records (none for an inner node) and goes to
// i + 1, its first child.
//
// Units: value-equal triangles form one identity class (shape_identity.hpp)
// whose records are adjacent in the table, and the containers walk settles a
// class at its last record (kShapeClassEnd), so a class is never divided: the
// build partitions classes, not records, and a class of more than kTriLeaf
// records makes one larger leaf.  Members of a class have equal geometry and
// transformation, hence equal balls.
//
// Split: the median of the units' ball centres along the longest axis of
// their bounding box, ties by table position (deterministic); nth_element
// per level, O(n log n) over the build.
//
// Balls: a node's centre is the middle of the box around its members' balls
// and its radius the largest |c - c_i| + r_i over them, so it holds every
// member's (already padded) ball exactly, in f64.  It is then padded by
// bounding_sphere's rule (1e-3 of the radius, 1e-4 of |c|_1 + r, and 1e-4):
// the cast of the centre to f32 moves it by at most 2^-24 |c| per axis and
// the cast of r^2 changes r by 2^-25 r, both far inside the pad, so the node
// ball as the kernel holds it still contains every member's ball as the
// kernel holds that, and a ray that meets a member's ball meets every
// ancestor's.  The kernels test nodes with the same wave_ball_may_hit as
// records (conservative for rays that meet the ball), so a subtree is passed
// by only when no lane's ray meets any ball inside it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace rtc {
namespace tri {

// Fewest bounded triangle records for which a world gets a tree (worlds of
// more shapes than the per-scene builds' records hold: rtc_host.cpp
// build_scene), and the most records of a leaf (classes aside).  DESIGN.md 3.9
// has the sweep.
constexpr uint32_t kTriTreeMin = 64;
constexpr uint32_t kTriLeaf = 8;

struct Ball {
    double c[3];
    double r;  // padded radius (not squared)
};

struct Node {
    Ball ball;
    int32_t skip;   // first node after this node's subtree
    int32_t first;  // leaf: first record, as a position in `order`
    int32_t count;  // leaf: records; inner node: 0
};

struct Tree {
    std::vector<Node> nodes;      // preorder
    std::vector<uint32_t> order;  // position in leaf order -> input index
    uint32_t leaves = 0, depth = 0;
};

// bounding_sphere's padding (rtc_host.cpp), for a ball around other balls
inline double padded_radius(const double c[3], double r) {
    const double scale = std::fabs(c[0]) + std::fabs(c[1]) + std::fabs(c[2]) + r;
    return r + (1e-3 * r + 1e-4 * scale + 1e-4);
}

// The kernel's view of a ball: centre and r^2 in R.
template <typename R>
inline void cast_ball(const Ball& b, R out[4]) {
    for (int q = 0; q < 3; ++q) out[q] = (R)b.c[q];
    out[3] = (R)(b.r * b.r);
}

// balls[i], cls[i]: the ball and identity class of record i of the bounded
// triangle run, in table order (members of a class adjacent).
inline Tree build(const Ball* balls, const uint32_t* cls, uint32_t n, uint32_t leaf_max = kTriLeaf) {
    Tree t;
    if (n == 0) return t;
    struct Unit {
        uint32_t first, count;  // records [first, first + count) of the input
    };
    std::vector<Unit> units;
    for (uint32_t i = 0; i < n; ++i) {
        if (i && cls[i] == cls[i - 1]) ++units.back().count;
        else units.push_back({i, 1u});
    }
    t.order.reserve(n);
    t.nodes.reserve(2 * units.size());
    struct Frame {
        uint32_t lo, hi, depth;
    };
    // Preorder without recursion: a node is emitted when its range of units
    // is popped, left child before right.  An inner node's skip link is the
    // index of the node that follows its subtree, known only once the
    // subtree is out: `open` holds the inner nodes still being filled, the
    // innermost last, and a range that starts at or past an open node's end
    // closes it.
    std::vector<Frame> stack{{0u, (uint32_t)units.size(), 1u}};
    struct Open {
        int32_t node;
        uint32_t hi;  // the subtree ends when a range starting at hi (or nothing) comes next
    };
    std::vector<Open> open;
    while (!stack.empty()) {
        const Frame f = stack.back();
        stack.pop_back();
        while (!open.empty() && open.back().hi <= f.lo) {
            t.nodes[open.back().node].skip = (int32_t)t.nodes.size();
            open.pop_back();
        }
        // the ball around the range's members
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        uint32_t records = 0;
        for (uint32_t u = f.lo; u < f.hi; ++u) {
            const Ball& b = balls[units[u].first];
            records += units[u].count;
            for (int q = 0; q < 3; ++q) {
                lo[q] = std::min(lo[q], b.c[q] - b.r);
                hi[q] = std::max(hi[q], b.c[q] + b.r);
                clo[q] = std::min(clo[q], b.c[q]);
                chi[q] = std::max(chi[q], b.c[q]);
            }
        }
        Node nd{};
        for (int q = 0; q < 3; ++q) nd.ball.c[q] = 0.5 * (lo[q] + hi[q]);
        double r = 0.0;
        for (uint32_t u = f.lo; u < f.hi; ++u) {
            const Ball& b = balls[units[u].first];
            const double dx = b.c[0] - nd.ball.c[0], dy = b.c[1] - nd.ball.c[1], dz = b.c[2] - nd.ball.c[2];
            r = std::max(r, std::sqrt(dx * dx + dy * dy + dz * dz) + b.r);
        }
        // (the distance's own rounding, a few ulp of r, is inside the pad too)
        nd.ball.r = padded_radius(nd.ball.c, r);
        t.depth = std::max(t.depth, f.depth);
        const int32_t self = (int32_t)t.nodes.size();
        if (records <= leaf_max || f.hi - f.lo == 1) {
            nd.first = (int32_t)t.order.size();
            nd.count = (int32_t)records;
            for (uint32_t u = f.lo; u < f.hi; ++u)
                for (uint32_t k = 0; k < units[u].count; ++k) t.order.push_back(units[u].first + k);
            nd.skip = self + 1;
            t.nodes.push_back(nd);
            ++t.leaves;
            continue;
        }
        int axis = 0;
        for (int q = 1; q < 3; ++q)
            if (chi[q] - clo[q] > chi[axis] - clo[axis]) axis = q;
        const uint32_t mid = f.lo + (f.hi - f.lo) / 2;
        std::nth_element(units.begin() + f.lo, units.begin() + mid, units.begin() + f.hi,
                         [&](const Unit& a, const Unit& b) {
                             const double ca = balls[a.first].c[axis], cb = balls[b.first].c[axis];
                             return ca < cb || (ca == cb && a.first < b.first);
                         });
        t.nodes.push_back(nd);
        open.push_back({self, f.hi});
        stack.push_back({mid, f.hi, f.depth + 1});  // popped second: the right child follows the left subtree
        stack.push_back({f.lo, mid, f.depth + 1});
    }
    for (const Open& o : open) t.nodes[o.node].skip = (int32_t)t.nodes.size();
    return t;
}

}  // namespace tri
}  // namespace rtc
