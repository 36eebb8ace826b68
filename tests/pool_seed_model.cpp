// Host model of the supersampled pool kernel's seeding rule (rtc_kernels.hip
// trace_pool_ss) against its capacity rule (rtc_internal.hpp
// pool_capacity_ss).  The pool is a LIFO of rays, each with its `remaining`;
// a generation pops min(size, batch) rays off the top and pushes every popped
// ray's children at remaining - 1 (none at remaining 0); the seeds of the
// next sample, `pixels` rays at remaining = depth, enter only when the pool
// has drained.  For grids 1..RT_MAX_SAMPLE_GRID and depths 0..16:
//  * two children everywhere, a full tile (256 pixels): the peak equals the
//    rule (it is tight) from depth 1 on, and is the seeds alone at depth 0;
//  * two children everywhere, ragged tiles and split parts (fewer pixels),
//    and random trees (0..2 children, mixed within a generation): the peak
//    never exceeds the rule.
// Prints "peak <grid> <depth> <peak> <rule>" per full-tile case, then "ok".
// tests/test_supersample_cpu.py runs it.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "../ray-tracer-challenge-rs_amd/csrc/rtc_internal.hpp"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

// The LIFO as runs of equal `remaining` (bottom first): {remaining, rays}.
using Runs = std::vector<std::pair<uint32_t, uint64_t>>;

void push(Runs& st, uint32_t rem, uint64_t n) {
    if (!n) return;
    if (!st.empty() && st.back().first == rem) st.back().second += n;
    else st.push_back({rem, n});
}

// children(rng) in 0..2 for a chunk of popped rays; null rng = always two.
uint64_t walk(uint32_t grid, uint32_t depth, uint32_t pixels, uint32_t batch, Rng* rng, uint64_t* seeded) {
    Runs st;
    uint64_t size = 0, peak = 0;
    *seeded = 0;
    for (uint32_t sample = 0; sample < grid * grid; ++sample) {
        if (size != 0) return ~0ull;  // the rule: seeds enter a drained pool only
        push(st, depth, pixels);
        size += pixels;
        *seeded += pixels;
        peak = std::max(peak, size);
        while (size) {
            uint64_t take = std::min<uint64_t>(size, batch);
            size -= take;
            Runs popped;
            while (take) {
                auto& top = st.back();
                const uint64_t n = std::min(top.second, take);
                popped.push_back({top.first, n});
                top.second -= n;
                take -= n;
                if (!top.second) st.pop_back();
            }
            for (const auto& [rem, n] : popped) {
                if (rem == 0) continue;
                uint64_t left = n;
                while (left) {  // chunks of one child count each (all of it without an rng)
                    const uint64_t c = rng ? std::min<uint64_t>(left, 1 + rng->next() % 64) : left;
                    const uint32_t kids = rng ? rng->next() % 3 : 2;
                    push(st, rem - 1, kids * c);
                    size += kids * c;
                    left -= c;
                }
            }
            peak = std::max(peak, size);
        }
    }
    return peak;
}

}  // namespace

int main() {
    const uint32_t batch = rtc::kPoolBatch, full = rtc::kBlock;
    for (uint32_t grid = 1; grid <= RT_MAX_SAMPLE_GRID; ++grid)
        for (uint32_t depth = 0; depth <= RT_MAX_SUPPORTED_DEPTH; ++depth) {
            const uint64_t rule = rtc::pool_capacity_ss(depth, batch, grid);
            uint64_t seeded = 0;
            const uint64_t peak = walk(grid, depth, full, batch, nullptr, &seeded);
            std::printf("peak %u %u %llu %llu\n", grid, depth, (unsigned long long)peak, (unsigned long long)rule);
            if (seeded != (uint64_t)grid * grid * full) return 1;
            if (peak != (depth ? rule : full)) return 2;  // tight
            for (uint32_t pixels : {1u, 4u, 37u, 64u, 128u, 255u}) {
                if (walk(grid, depth, pixels, batch, nullptr, &seeded) > rule) return 3;
                Rng rng{depth * 977u + grid * 31u + pixels};
                if (walk(grid, depth, pixels, batch, &rng, &seeded) > rule) return 4;
            }
            Rng rng{depth * 131u + grid};
            for (int rep = 0; rep < 8; ++rep)
                if (walk(grid, depth, full, batch, &rng, &seeded) > rule) return 5;
        }
    std::printf("ok\n");
    return 0;
}
