// rtc_internal.hpp — records shared by the host launcher (rtc_host.cpp) and
// the gfx950 kernels (rtc_kernels.hip).
//
// HBM layout of a flattened world (SURVEY.md §7 "SoA per-type shape tables"):
// the reference's Vec<Box<dyn Shape>> (world.rs:11) becomes ONE array of
// fixed-size ShapeRec sorted by kind (spheres, planes, cubes, cylinders,
// cones, triangles), with `kind_begin[k]..kind_begin[k+1]` delimiting the
// per-type loops.  Every lane of a wave walks the same records in the same
// order, so the shape loads are wave-uniform scalar (s_load) loads that hit
// the scalar cache; `world_index` restores the reference's world order for
// the stable-sort tie rule.  Materials, patterns and
// lights are small side tables.  Everything is cast once from the caller's
// f64 tables to the kernel's real type R (f32 or f64).
#pragma once

#include <cstdint>
#ifndef __HIPCC_RTC__
#include <string>
#endif

#include "../../include/rtc.h"

#if defined(__HIP__)
#define RTC_HD __host__ __device__
#else
#define RTC_HD
#endif

namespace rtc {

#ifndef __HIPCC_RTC__
int set_error(int code, const std::string& msg);  // rtc_host.cpp (thread-local)
#endif

// Row-block shards: tile row k of the image (RT_TILE_H rows)
// belongs to shard k % shards, which renders its tile rows in order into a
// contiguous strip.  One definition for the kernels' pixel mapping, the
// de-interleave kernel and the host (rt_shard_row_map, tested on CPU).
RTC_HD inline uint32_t shard_tile_rows(uint32_t height, uint32_t shards, uint32_t shard) {
    const uint32_t trows = (height + RT_TILE_H - 1) / RT_TILE_H;
    return trows > shard ? (trows - shard + shards - 1) / shards : 0;
}
// first image row of tile row `tile_row` of shard `shard`'s strip
RTC_HD inline uint32_t shard_tile_image_row(uint32_t tile_row, uint32_t shards, uint32_t shard) {
    return (tile_row * shards + shard) * RT_TILE_H;
}
// image row of row `strip_row` of shard `shard`'s strip
RTC_HD inline uint32_t shard_image_row(uint32_t strip_row, uint32_t shards, uint32_t shard) {
    return shard_tile_image_row(strip_row / RT_TILE_H, shards, shard) + strip_row % RT_TILE_H;
}
// shard and strip row of image row y (the inverse)
RTC_HD inline void shard_of_image_row(uint32_t y, uint32_t shards, uint32_t* shard, uint32_t* strip_row) {
    const uint32_t trow = y / RT_TILE_H;
    *shard = trow % shards;
    *strip_row = (trow / shards) * RT_TILE_H + y % RT_TILE_H;
}

constexpr int kBlock = 256;        // threads per workgroup = 4 waves of 64
constexpr int kWaves = kBlock / 64;  // waves per workgroup
// The pool kernel's shape (rtc_kernels.hip trace_pool): block-lockstep
// generations of up to kBlock rays over one tile's pixel accumulators.
constexpr int kTileSlots = 1;
constexpr uint32_t kPoolBatch = kBlock;  // rays a generation pops
constexpr int kTilePixels = RT_TILE_W * RT_TILE_H;  // one tile per workgroup pass
static_assert(kTilePixels == kBlock, "one pixel per thread per tile");
constexpr int kNumKinds = 6;
constexpr int kNumCounters = 8;    // order of rt_stats' first eight fields
constexpr int kGenSlots = RT_MAX_SUPPORTED_DEPTH + 1;  // rt_generation_counts, by `remaining`
// Event counters are sharded: workgroup b adds into shard b % kCounterShards
// (same-address global atomics from every workgroup cost ~66 us per 1080p
// frame on MI355X; sharded they are noise).  The host sums the shards.
constexpr int kCounterShards = 256;
// Tile queues: one atomic head saturates at ~88 dequeues/us on MI355X
// (MI355X_MICROARCH.md, price list row "dequeue"), i.e. ~93 us for the 8160
// tiles of a 1920x1080 frame.  Tile t lives in queue t % 8 and workgroup b
// pulls from queue b % 8 (blocks b and b+8 share an XCD under round-robin
// dispatch; placement only affects speed).
constexpr int kTileQueues = 8;
// Queue heads sit kQueueStride u64 apart (256 B): adjacent heads shared one
// cache line, so every XCD's dequeues serialized on it (~17 us per 1792
// dequeues on MI355X).
constexpr int kQueueStride = 32;
// Work items of a cost-ordered pool launch: one part of a tile split 4 to 64
// ways (order_tiles).  item = tile | part << 20 | log2(parts) << 26 |
// priority << 29; part p of a tile split 2^l ways seeds the pixels of
// threads t with t >> (8 - l) == p (waves, half-waves, wave rows, half rows
// and quarter rows of a wave's 16 x 4 block).  Cost-ordered launches need n_tiles <= 2^20
// (plan_tile_order; larger frames keep raster order).
// An item of priority p > 0 (the costliest, order_tiles) runs its waves at
// s_setprio(p).
constexpr uint32_t kItemTileMask = 0xFFFFFu;
constexpr uint32_t kItemPartShift = 20, kItemSplitShift = 26, kItemPartMask = 63u, kItemSplitMask = 7u;
constexpr uint32_t kItemPrioShift = 29;  // (bit 31 stays clear: no item equals kNoItem)
constexpr uint32_t kMaxSplitLog2 = 6;  // up to 64 items per tile (4 pixels each)
// order_tiles runs on launches 2 .. 1 + kOrderBuilds of a frame signature,
// then the order is reused (rtc_host.cpp plan_tile_order).
constexpr int kOrderBuilds = 8;
constexpr uint32_t kNoItem = 0xFFFFFFFFu;  // next_tile: the launch's items are all taken

// A work item, decoded.  Only launches that hand items out through a tile
// order (LaunchParams::tile_order set: cost-ordered or centre-out, which
// plan_tile_order allows for n_tiles <= 2^20 only) carry the packed fields;
// a raster launch's item is the plain tile index, whatever the launch's size
// (an rt_color_at batch reaches 2^24 tiles).  Decoding a raster item >= 2^20
// as packed would mask its tile and read stray part/split/priority bits.
struct WorkItem {
    uint32_t tile, part, split_log2, prio;
};
RTC_HD inline WorkItem decode_item(uint32_t item, bool packed) {
    if (!packed) return {item, 0u, 0u, 0u};
    return {item & kItemTileMask, (item >> kItemPartShift) & kItemPartMask, (item >> kItemSplitShift) & kItemSplitMask,
            (item >> kItemPrioShift) & 3u};
}
RTC_HD inline uint32_t encode_item(uint32_t tile, uint32_t part, uint32_t split_log2, uint32_t prio) {
    return tile | part << kItemPartShift | split_log2 << kItemSplitShift | prio << kItemPrioShift;
}
// Part p of a tile split 2^l ways seeds the threads t of the tile's
// workgroup with t >> (8 - l) == p (halves, wave pairs, waves, half-waves,
// wave rows); l = 0 seeds all 256.
RTC_HD inline bool item_seeds(uint32_t tid, const WorkItem& w) { return (tid >> (8u - w.split_log2)) == w.part; }

// Spilled pool entries: workgroup b of a pool launch owns records
// [b * spill_cap, (b + 1) * spill_cap) of LaunchParams::spill, 8 words each;
// slot s >= lds_cap of its LIFO is record s - lds_cap.
RTC_HD inline uint64_t spill_word(uint32_t block, uint32_t spill_cap, uint32_t slot, uint32_t lds_cap) {
    return ((uint64_t)block * spill_cap + (slot - lds_cap)) * 8u;
}

// LIFO bound (rays) of a workgroup's pool in a supersampled launch
// (rtc_kernels.hip trace_pool_ss).  Seeding rule: the seeds of sample s + 1
// (at most kBlock rays, each at remaining = depth) enter only when the pool
// has drained, i.e. holds no ray of sample s.  So at every moment the pool
// holds rays of one sample only, and what one sample can pile up is what a
// plain frame's single seeding can.  A generation pops min(size, batch) rays
// off the top and pushes at most two children per popped ray, each at its
// parent's remaining - 1, none from remaining 0.  Call the rays one
// generation pushed a segment (the seeds are the first).  Children lie above
// every ray that stayed and have less remaining than any of them (the popped
// rays were on top of those), so from the bottom up the segments' largest
// remaining strictly falls from `depth`: at most depth + 1 segments.  A
// segment is born with at most 2 x batch rays; a later segment exists only
// after a full batch was popped off it (a pop that reaches below a segment
// removes it), so every segment but the top one holds at most `batch`, and
// the seeds' at most kBlock - batch.  Size <= (kBlock - batch) + (depth - 1)
// x batch + 2 x batch = kBlock + depth x batch, whatever the grid: the bound
// of a plain frame (rtc_host.cpp pool_capacity; batch = kPoolBatch = kBlock).
// tests/pool_seed_model.cpp walks the rule for grids 1..RT_MAX_SAMPLE_GRID
// and depths 0..16 with two children everywhere against this function.
RTC_HD inline uint32_t pool_capacity_ss(uint32_t depth, uint32_t batch, uint32_t grid) {
    (void)grid;  // a drained pool forgets the samples before
    return (uint32_t)kBlock + depth * batch;
}

// Ray batches (rtc_kernels.hip trace_rays): one ray tree per lane, walked
// depth first with a private LIFO of pending rays.  The lane holds the ray it
// is shading in registers; shading pushes its children (at most two, each at
// remaining - 1, none at remaining 0) and the lane then pops its next ray.
// Entries the LIFO must hold for a tree of `max_depth`: by induction on the
// walk, when the lane shades a ray at remaining r the LIFO holds at most one
// pending sibling per ancestor, max_depth - r entries (the other sibling is
// the ancestor's popped child on the path to this ray), and pushing two
// children makes max_depth - r + 2.  Only rays at r >= 1 push, so the peak is
// at r = 1: max_depth + 1 entries, reached by a path that spawns two children
// at every level; a tree of depth 0 pushes nothing.
// (Both children are stored and one is popped straight back: keeping it in
// registers would save one entry and cost a second live ray through
// shade_ray.)  tests/test_trace_rays_cpu.py models the walk against this.
RTC_HD inline uint32_t ray_stack_entries(uint32_t max_depth) { return max_depth ? max_depth + 1u : 0u; }
// Lane `tid` of workgroup `block` keeps entry e of its LIFO at this word (of
// the launch's real type) of the stack buffer: 8 words per entry {o, d,
// weight, remaining}, the 256 lanes of an entry adjacent, so a wave's push or
// pop is one contiguous 2 KB (f32) run.
RTC_HD inline uint64_t ray_stack_word(uint32_t block, uint32_t entries, uint32_t e, uint32_t tid) {
    return (((uint64_t)block * entries + e) * 256u + tid) * 8u;
}
// Rays of one rt_trace_rays* call: chunks of 256 indexed in 32 bits with room
// for the grid stride, element offsets in 64.
constexpr uint64_t kMaxRayBatch = 1ull << 31;

// RTC_BOUNDS_CHECK builds (debug variant, scripts/build_variant.sh): the pool
// kernel checks every computed index against its buffer before the access,
// skips a bad access and raises one of these bits of LaunchParams::error_flag
// (the host reports them as RT_ERR_POOL with the bit's name).
constexpr int32_t kErrPoolOverflow = 1;  // a child beyond the LIFO bound (no debug build needed)
constexpr int32_t kErrPoolSpin = 2;      // a pool lock's spin bound ran out (scripts/patches/pool_free_and_diag.patch only)
constexpr int32_t kErrBoundsSlot = 4;    // pool slot outside [0, cap)
constexpr int32_t kErrBoundsSpill = 8;   // spill record outside the launch's spill buffer
constexpr int32_t kErrBoundsTile = 16;   // work item's tile >= n_tiles
constexpr int32_t kErrBoundsOut = 32;    // output element outside the canvas or strip
constexpr int32_t kErrPeerTimeout = 64;  // rt_canvas_wait: a shard's flag did not arrive in time
constexpr int32_t kErrBitsAll[] = {kErrPoolOverflow, kErrPoolSpin, kErrBoundsSlot, kErrBoundsSpill,
                                   kErrBoundsTile, kErrBoundsOut, kErrPeerTimeout};
#ifndef __HIPCC_RTC__
// The kernels' error word as rt_last_error text (RT_ERR_POOL), one distinct
// phrase per bit (tests/index_math.cpp checks that every kErr* bit has one).
inline std::string device_error_text(int32_t err) {
    std::string m;
    auto add = [&](int32_t bit, const char* what) {
        if (err & bit) m += (m.empty() ? "" : "; ") + std::string(what);
    };
    add(kErrPoolOverflow, "device ray pool overflow: a child beyond the LIFO bound");
    add(kErrPoolSpin, "device ray pool: a lock's spin bound ran out (a starved wave, not an overflow)");
    add(kErrBoundsSlot, "bounds check: pool slot outside the LIFO bound");
    add(kErrBoundsSpill, "bounds check: spill region outside the spill buffer");
    add(kErrBoundsTile, "bounds check: work item tile outside the launch");
    add(kErrBoundsOut, "bounds check: output index outside the canvas");
    add(kErrPeerTimeout, "peer canvas: a shard's flag (or the owner's release) did not arrive within the timeout");
    const int32_t unknown = err & ~(kErrPoolOverflow | kErrPoolSpin | kErrBoundsSlot | kErrBoundsSpill |
                                    kErrBoundsTile | kErrBoundsOut | kErrPeerTimeout);
    if (unknown) m += (m.empty() ? "" : "; ") + std::string("device error bits ") + std::to_string(unknown);
    return m;
}
#endif

// Peer canvas (rt_canvas_create): the W x H image and, after it at this
// alignment, one u64 completion flag per shard.
constexpr uint64_t kCanvasFlagAlign = 256;
// t / d for every t < n as one multiply-high by m = ceil(2^32 / d): with
// m d = 2^32 + e, 0 <= e < d, t m / 2^32 = t/d + t e / (d 2^32), and the
// second term stays below 1/d (so below the gap to the next integer) while
// n d < 2^32.  Returns 0 where that does not hold (divide instead).  The
// tracer kernels take the tile row of tile t this way (LaunchParams::
// tiles_x_magic): one s_mul_hi_u32 instead of a ~25-instruction division.
RTC_HD inline uint32_t div_magic(uint32_t d, uint32_t n) {
    if (d < 2 || (uint64_t)n * d >= (1ull << 32)) return 0;
    return (uint32_t)(((1ull << 32) + d - 1) / d);
}
RTC_HD inline uint32_t div_by(uint32_t t, uint32_t d, uint32_t magic) {
    return magic ? (uint32_t)(((uint64_t)t * magic) >> 32) : t / d;
}

RTC_HD inline uint64_t canvas_flag_offset(uint64_t image_bytes) {
    return (image_bytes + kCanvasFlagAlign - 1) / kCanvasFlagAlign * kCanvasFlagAlign;
}
// Tile scheduling modes (the direct kernel: RTC_DEBUG=sched_direct=grid|static; the pool kernel: dynamic)
constexpr uint32_t kSchedGrid = 0;     // one workgroup per tile; the dispatcher balances
constexpr uint32_t kSchedDynamic = 1;  // resident grid, per-XCD atomic tile queues
constexpr uint32_t kSchedStatic = 2;   // resident grid, tiles b, b+G, ... (no atomics)
// World tables up to this size are staged into LDS for the per-lane gathers
// (~120 f32 shapes); larger worlds gather from global memory (L2-resident).
constexpr size_t kMaxWorldLds = 16 * 1024;

// Fixed-point pixel accumulator of the pool kernel: contributions are summed
// as int64 multiples of 2^-48 so the per-pixel sum is independent of the
// (nondeterministic) order in which waves add to it.
constexpr double kAccScale = 281474976710656.0;  // 2^48
constexpr double kAccInvScale = 1.0 / 281474976710656.0;
// The f32 pool kernel sums in int32 multiples of 2^-acc_log2 instead: half
// the LDS (3 KB of a workgroup's ~26 KB, given to the ray pool), and the
// scale is the largest that keeps the world's brightest possible pixel below
// 2^30 (acc_shift_f32), e.g. 2^-22 for reflect_refract: 2.4e-7 per
// contribution against an f32 ulp of 1.2e-7 at 1.0.
template <bool B, typename T, typename F>
struct Choose {
    using type = T;
};
template <typename T, typename F>
struct Choose<false, T, F> {
    using type = F;
};
#ifndef RTC_ACC_I64  // (A/B builds: -DRTC_ACC_I64 keeps the f32 sums in int64 too)
template <typename R>
using PoolAcc = typename Choose<sizeof(R) == 4, int32_t, long long>::type;
#else
template <typename R>
using PoolAcc = long long;
#endif
constexpr uint32_t kAccLog2Min = 8, kAccLog2Max = 28;
// A pool entry's meta word (pixel | remaining << 8: 13 bits; the pixel is the
// lane of the workgroup's tile, 0..255) as stored in the LDS part of the
// pool; spilled entries keep 32 bits in their record.
#ifndef RTC_POOL_META32  // (A/B builds: -DRTC_POOL_META32 keeps 32-bit entries)
using PoolMeta = uint16_t;
#else
using PoolMeta = uint32_t;
#endif
static_assert(RT_MAX_SUPPORTED_DEPTH < 32, "remaining must fit the pool meta's 8 high bits");

// ShapeRec::flags.  Value-equal shapes (shape_identity.hpp) form one identity
// class; its members are adjacent within their kind's run of the table, the
// last one carries kShapeClassEnd, and every member carries the class id (the
// world index of its first member), so the containers walk can toggle one
// entry per class as the reference does (intersection.rs:47).  A world with
// no value-equal shapes has one class per shape, each its own world index.
constexpr int32_t kShapeClosed = 1;    // cylinder/cone `closed`
constexpr int32_t kShapeClassEnd = 2;  // last member of its identity class
// A sphere whose transformation is a similarity (rotation, uniform scale,
// translation: rtc_host.cpp similar_sphere): tri[0..2] holds its world
// centre and tri[3] its radius^2, and the f32 kernels find its roots in world
// space (rtc_kernels.hip sphere_world).
constexpr int32_t kShapeSimilar = 4;
// A cube whose transformation has a diagonal linear part (scale and
// translation only: rtc_host.cpp axis_aligned_cube): tri[0..2] holds the
// world coordinates of its object -1 faces, tri[3..5] of its +1 faces,
// tri[6..8] the world |d| below which an axis counts as parallel (EPSILON
// over the axis's scale) and tri[9..11] the scale's signs, and the f32
// kernels run its slab test in world space (rtc_kernels.hip cube_world).
constexpr int32_t kShapeAxisAligned = 8;
// A smooth triangle (rtc.h rt_scene_upload_smooth): its three vertex normals
// are entry `slot - kind_begin[RT_SHAPE_TRIANGLE]` of LaunchParams::
// smooth_plain (a record of the shape table) or entry `position` of
// smooth_inst (a mesh's local record at that position of inst_shapes), nine
// reals each.  Only the instance build's prepare_hit reads the bit.
constexpr int32_t kShapeSmooth = 16;
constexpr int kSmoothReals = 9;  // n1, n2, n3
// A triangle with texture coordinates (rtc.h rt_scene_upload_textured): its
// t1, t2, t3 are entry `slot - kind_begin[RT_SHAPE_TRIANGLE]` of LaunchParams::
// uv_plain or entry `position` of uv_inst, six reals each, laid out like the
// normal tables.  Only the texture build's prepare_hit reads the bit.
constexpr int32_t kShapeUV = 32;
constexpr int kUVReals = 6;  // t1, t2, t3
// A moving shape (rtc.h rt_scene_upload_moving): its velocity is entry `slot`
// of the launch's shape velocity table (MotionArg::shape_vel).  A moving mesh
// instance carries the same fact in InstRec::moving and its velocity at entry
// `instance` of MotionArg::inst_vel; the virtual records for_instances hands
// out carry the bit and the velocity itself in `bound[0..2]`, their cull being
// done.  Only the motion build (RTC_MOTION) reads the bit; a static shape in a
// moving world pays its wave-uniform test and nothing more.
constexpr int32_t kShapeMoving = 64;
// One texture of the upload: its first texel in LaunchParams::texels (one
// packed dword per texel, R | G << 8 | B << 16, row 0 at the top) and its size.
struct alignas(16) TexRec {
    uint64_t offset;
    uint32_t width, height;
};
static_assert(sizeof(TexRec) == 16);
constexpr int kShapeClassShift = 8;

template <typename R>
struct alignas(16) ShapeRec {
    R inv[12];     // rows 0..2 of transformation_inverse (row 3 is never read:
                   // Mul<Point>/Mul<Vector> produce 3 rows, matrix.rs:332-362)
    R bound[4];    // world bounding sphere (center, radius^2) for the wave cull; < 0 = unbounded
    // Right after inv/bound so one scalar-load burst at the top of a shape
    // iteration covers everything a sphere/plane/cube test reads (a later
    // world_index load cost a second s_waitcnt per iteration).
    int32_t world_index;
    int32_t casts_shadow;  // material.casts_shadow, hoisted for the any-hit loop
    int32_t material;
    int32_t flags;  // kShapeClosed | kShapeClassEnd | identity class << kShapeClassShift
    R ymin, ymax;  // cylinder/cone min/max (cylinder.rs:12-14)
    R tri[12];     // triangle vertex_1, edge_1, edge_2, normal (triangle.rs:12-17);
                   // a kShapeSimilar sphere: world centre, radius^2;
                   // a kShapeAxisAligned cube: its world slabs
};

template <typename R>
struct alignas(16) MaterialRec {
    R color[3];
    R ambient, diffuse, specular, shininess;
    R reflectiveness, transparency, refractive_index;
    int32_t pattern;       // -1 = None
    int32_t casts_shadow;
};

template <typename R>
struct alignas(16) PatternRec {
    R color_a[3];
    R color_b[3];
    R inv[12];
    int32_t kind;
    int32_t sub_a, sub_b;
    int32_t pad;
};

// LDS image of the world: [shapes][materials][patterns][world_slot], every
// record a multiple of 16 bytes so each section stays 16-byte aligned.
template <typename R>
constexpr size_t world_lds_bytes(size_t ns, size_t nm, size_t np) {
    return ns * sizeof(ShapeRec<R>) + nm * sizeof(MaterialRec<R>) + np * sizeof(PatternRec<R>) +
           (ns + 3) / 4 * 16;
}
static_assert(sizeof(ShapeRec<float>) % 16 == 0 && sizeof(ShapeRec<double>) % 16 == 0);
static_assert(sizeof(MaterialRec<float>) % 16 == 0 && sizeof(MaterialRec<double>) % 16 == 0);
static_assert(sizeof(PatternRec<float>) % 16 == 0 && sizeof(PatternRec<double>) % 16 == 0);

template <typename R>
struct alignas(16) LightRec {
    R position[3];
    R intensity[3];
};

// An area light (rtc.h rt_scene_upload_lit): a parallelogram of usteps x vsteps
// cells, each sampled once per shaded hit; uvec and vvec are the cell edges
// (the full edges divided by the step counts on the host, then rounded to R).
// Read wave-uniformly by the area build's shade_ray; no other kernel loads it.
template <typename R>
struct alignas(16) AreaLightRec {
    R corner[3];
    R uvec[3];
    R vvec[3];
    R intensity[3];
    uint32_t usteps, vsteps, jitter, seed;
};
static_assert(sizeof(AreaLightRec<float>) == 64 && sizeof(AreaLightRec<double>) == 112);

template <typename R>
struct CameraRec {
    R inv[12];
    R origin[3];
    R half_width, half_height, pixel_size;
};

// A node of the triangle hierarchy (tri_tree.hpp; rtc_kernels.hip
// for_triangles): nodes in depth-first preorder, `skip` the first node after
// this node's subtree, a leaf's records [first, first + count) of the shape
// table (an inner node's count is 0).
template <typename R>
struct alignas(16) TriNode {
    R ball[4];  // padded bounding ball of the subtree: centre, radius^2
    int32_t skip, first, count, pad;
};
static_assert(sizeof(TriNode<float>) == 32 && sizeof(TriNode<double>) == 48);

// A placed copy of a mesh (rt_scene_upload_instanced): the world is the flat
// list `shapes ++ E(0) ++ E(1) ...`, E(k) the mesh's triangles under instance
// k's inverse and material, and the kernels walk it without writing it out.
// The mesh's triangles sit once in a table of local records (identity
// inverse; ShapeRec::world_index holds the triangle's index in the mesh,
// ShapeRec::bound its padded local ball) under a local hierarchy of TriNode
// whose leaf runs count from the mesh's first record.  An instance uploaded
// expanded (it has a value-equal partner: rtc_host.cpp) keeps its record for
// the hit's lookup only: its triangles are plain records of the shape table.
template <typename R>
struct alignas(16) InstRec {
    R inv[12];   // rows 0..2 of the instance's inverse
    R ball[4];   // world ball of the whole mesh under this instance (centre, r^2); r^2 < 0: none
    int32_t world_base;    // world index of the mesh's triangle 0 under this instance
    int32_t casts_shadow;  // of `material`
    int32_t material;
    int32_t n_triangles;
    int32_t node_begin, n_nodes;  // the mesh's nodes in the instance node table
    int32_t rec_begin;            // the mesh's first local record; leaves' runs count from here
    int32_t rec_flat;             // the mesh's records outside its tree: [rec_flat, rec_end)
    int32_t rec_end;
    int32_t pos_begin;  // local index j -> inst_pos[pos_begin + j]: the local record (or, expanded: slot | kind << 24)
    int32_t expanded;   // 1: uploaded as plain records, the walk passes it by
    int32_t moving;     // 1: the instance has a velocity (kShapeMoving); zero in every world without motion
};
static_assert(sizeof(InstRec<float>) % 16 == 0 && sizeof(InstRec<double>) % 16 == 0);

// The instance a world index belongs to: the last one whose base is <= w
// (bases ascend).  One definition for the kernels' per-hit lookup and the
// host (tests/instances.cpp).  n >= 1 and w >= base(0).
template <typename Base>
RTC_HD inline int instance_of_world(Base&& base, int n, int w) {
    int lo = 0, hi = n;  // base(lo) <= w < base(hi) (base(n) = +inf)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (base(mid) <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <typename R>
struct DevScene {
    const ShapeRec<R>* shapes;
    const MaterialRec<R>* materials;
    const PatternRec<R>* patterns;
    const LightRec<R>* lights;
    const int32_t* world_slot;  // world order -> slot | kind << 24 (rounded up to 4 entries)
    // Per-lane gathers (the hit's shape, its material and pattern) go through
    // these: LDS copies staged at kernel start when the tables fit
    // (LaunchParams::world_lds), else the global tables above.
    const ShapeRec<R>* lshapes;
    const MaterialRec<R>* lmats;
    const PatternRec<R>* lpats;
    const int32_t* lworld_slot;
    int32_t kind_begin[kNumKinds + 1];
    int32_t n_materials, n_patterns;
    int32_t n_lights;
    int32_t any_secondary;  // some material has reflectiveness or transparency != 0
    int32_t no_skips;       // RT_FLAG_NO_SKIPS launch (the generic kernels; per-scene builds: RTC_NO_SKIPS)
};

// Primary cull of the per-scene f32 direct kernel (rtc_kernels.hip
// closest_hit): each launch of a camera frame works out, per shape slot, the
// screen rectangle outside which no primary ray can pass the slot's wave cull
// (primary_rect.hpp), and hands it over as two bit tables over the kernel's
// wave blocks (kCullCellW x kCullCellH pixels): bit s of cull_cols[i] is set
// when slot s's rectangle misses pixel columns [16 i, 16 i + 15], bit s of
// cull_rows[j] when it misses rows [4 j, 4 j + 3].  A wave passes slot s by
// when either bit of its block is set: two scalar loads and an OR per wave
// and tile, whatever the number of slots (a compare of the block against each
// rectangle cost ~14 SALU per slot and ate the gain: the scalar unit is as
// busy as the vector units in this kernel).  A plane's slot
// has a bit too: its rectangle (primary_rect.hpp plane_rect) holds every pixel
// where the plane's entry can be the nearest of the planes' entries in front
// of the eye; outside it the entry lies behind the eye or another plane's is
// nearer, and the wave passes the plane's test by.  All zero (no
// cull) for every other launch, for worlds of more than kPrimaryRectSlots
// slots (the same small-world limit as RTC_JIT_NORMAL_MAX) and for canvases
// beyond the tables.
constexpr int kPrimaryRectSlots = 8;
constexpr uint32_t kCullCellW = 16, kCullCellH = 4;
constexpr uint32_t kCullCols = 128, kCullRows = 512;  // canvases up to 2048 x 2048

// Shadow cull of the same kernel (rtc_kernels.hip any_hit under
// shade_hit_const, primary_rect.hpp shadow_rect): bits 8..31 of the same
// words.  A wave whose hits all lie on plane p asks, per light l and caster c,
// whether its block lies outside the screen rectangle in which c's ball can
// shadow p from l; the plane as its own caster has a bit too (set in every
// column when the eye and the light share a side of it).  The rectangles speak
// only for hits within reach of the light (shadow_near), so each plane has one
// more bit, set where a block column or row holds no hit beyond it; the pair
// bits count only under it.  One mapping for the host (scene.kind_begin) and
// the kernel (jit::kBegin); a world whose bits do not fit takes none, and
// every launch the primary cull leaves at zero leaves these at zero too.
constexpr int kShadowRectSlots = 6;  // the wave-uniform hit's cap (rtc_kernels.hip kUniformHitSlots)
constexpr int kShadowBit0 = kPrimaryRectSlots, kShadowBits = 32 - kPrimaryRectSlots;
struct ShadowLayout {
    int planes, casters, lights, plane0;  // casters: the slots that are no planes
    constexpr ShadowLayout(const int32_t* kb, int n_lights)
        : planes(kb[RT_SHAPE_PLANE + 1] - kb[RT_SHAPE_PLANE]), casters(kb[kNumKinds] - planes), lights(n_lights),
          plane0(kb[RT_SHAPE_PLANE]) {}
    constexpr bool fits() const {
        return planes > 0 && lights > 0 && planes + casters <= kShadowRectSlots &&
               planes + lights * planes * (casters + 1) <= kShadowBits;
    }
    constexpr bool is_plane(int slot) const { return slot >= plane0 && slot < plane0 + planes; }
    // the bit under which plane `slot`'s pair bits count
    constexpr int near_bit(int slot) const { return kShadowBit0 + (slot - plane0); }
    // caster `c` on plane `slot` from `light`; -1: no bit (another plane)
    constexpr int pair_bit(int light, int slot, int c) const {
        if (is_plane(c) && c != slot) return -1;
        const int rank = c == slot ? casters : (c < plane0 ? c : c - planes);
        return kShadowBit0 + planes + (light * planes + (slot - plane0)) * (casters + 1) + rank;
    }
};

// Launch terms of the same kernel (launch_terms.hpp, rtc_kernels.hip
// closest_hit and prepare_hit_const): every primary ray of a frame starts at
// the camera's origin, so what a test forms from the origin alone is one
// value per launch.  The host works the values out in the kernel's own f32
// operations (sub, mul, fma, max: the device's bits) and a wave reads them
// with its block's cull words, one scalar load per tile:
//   [0]     max(|o.x|, |o.y|, |o.z|), the origin's part of the flat kinds' offset scale
//   [1 + p] plane p of the plane run: lo.y of xform_point(inv, origin), all its test reads
// (nearly every tile tests some plane, so every tile loads them all; the terms
// of the other kinds' tests were measured too and left out).
// Filled for the launches the kernel reads them in (camera frames of the
// per-scene f32 direct kernel, worlds of at most kPrimaryRectSlots slots).
struct alignas(16) LaunchTerms {
    float head[kPrimaryRectSlots + 4];
};

// The thin lens of a lens frame (rtc.h "Thin-lens camera"),
// in the kernel's real type.  `lk` = mix(seed ^ 0x4C454E53), hashed once on
// the host.  Under RT_JITTER_NONE the lens point of sample (i, j) is the same
// for every pixel, so the host works all n^2 of them out in the kernel's own
// operations (lens_points) and the kernels read entry j * n + i with scalar
// loads: a sample trip is a pinhole frame from a shifted origin.  Under
// RT_JITTER_HASHED the table is unread and each lane works out its own.
// The lens kernels (trace_direct_lens, trace_pool_lens) take it as one more
// argument behind the four table pointers: LaunchParams, which every shipped
// kernel takes, stays as it is, to the byte.
constexpr uint32_t kLensKey = 0x4C454E53u;
template <typename R>
struct LensPoint {
    R origin[3];  // inverse * (lx, ly, 0): the ray's origin in world space
    R lx, ly;     // the lens point in camera space
};
template <typename R>
struct LensParams {
    R aperture, focal, inv_n;
    uint32_t jitter, lk;
    LensPoint<R> points[RT_MAX_SAMPLE_GRID * RT_MAX_SAMPLE_GRID];
};

// A caller's ray batch (rt_trace_rays*) as the host hands it to a launch: the
// ray-batch kernel's (trace_rays) argument behind the four table pointers,
// laid out as the kernel's own RayBatch<R> (rtc_kernels.hip, which checks it).
struct RayBatchArg {
    const void* rays;  // n_rays x {o, d} of R
    void* rgb;         // n_rays x 3 of R
    void* hits;        // n_rays x rt_ray_hit_f32 / rt_ray_hit_f64, or null
};

// The jitter hash of rtc.h ("Hashed jitter"), uint32_t wraparound.
RTC_HD inline uint32_t hash_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// Lens cell (ci, cj) and position (ju, jv) in it of sample (i, j) of pixel
// (x, y) under RT_JITTER_HASHED: `ray_id` the sample's pixel index in the
// sample camera, `pixel_id` = y * W + x in whole-image coordinates.  One
// definition for the kernels and rt_lens_ray.
template <typename R>
RTC_HD inline void lens_hashed_cell(uint32_t lk, uint32_t ray_id, uint32_t pixel_id, uint32_t n, uint32_t i, uint32_t j,
                                    R& fu, R& fv) {
    const uint32_t key = hash_mix(lk ^ ray_id);
    const R ju = (R)(key >> 8) * (R)0x1p-24;
    const R jv = (R)(hash_mix(key ^ 0x9E3779B9u) >> 8) * (R)0x1p-24;
    const uint32_t n2 = n * n;
    const uint32_t r = hash_mix(lk ^ hash_mix(pixel_id)) % n2;
    const uint32_t k = (j * n + i + r) % n2;
    const uint32_t cj = k / n, ci = k - cj * n;
    fu = (R)ci + ju;
    fv = (R)cj + jv;
}

// Motion (rtc.h "Motion blur"; the motion build only, RTC_MOTION).
// The velocity tables of a moving world, four reals an entry (x, y, z, 0), each
// rounded once to R: one entry per slot of the shape table, one per instance.
// Every kernel of the motion build takes them as one more argument behind the
// four table pointers, in front of the family's own (MotionLaunch below):
// LaunchParams stays as it is.
struct MotionArg {
    const void* shape_vel;  // kind_begin[kNumKinds] x 4 of R; a static shape's entry is zero and never read
    const void* inst_vel;   // n_instances x 4 of R, or null
};
// What the host hands the motion build's launch_kernel as `extra`: the tables
// and the family's own argument (a RayBatchTimedArg, a LensParams<R>, a
// ShutterArg<R>, or null).
struct MotionLaunch {
    MotionArg motion;
    const void* extra;
};
// A timed ray batch (rt_trace_rays_timed*): the batch and a time per ray in R, null = every time 0.
struct RayBatchTimedArg {
    RayBatchArg batch;
    const void* times;
};
// The shutter of a shutter frame in the kernel's real type: `open` and
// `span` = close - open formed in f64 and rounded once, inv_n2 = R(1) / R(n^2),
// `tk` = mix(seed ^ 0x54494D45) hashed once on the host.
constexpr uint32_t kShutterKey = 0x54494D45u;
template <typename R>
struct ShutterParams {
    R open, span, inv_n2;
    uint32_t jitter, tk;
};
// A shutter frame's argument: the lens (aperture 0: the pinhole's sample rays, camera_ray's arithmetic) and the shutter.
template <typename R>
struct ShutterArg {
    LensParams<R> lens;
    ShutterParams<R> shutter;
};
// The time of sample (i, j) of pixel (x, y), y the whole-image row, W the
// image's width, n the grid.  One definition for the kernels and
// rt_shutter_time (R = double).
template <typename R>
RTC_HD inline R shutter_time(const ShutterParams<R>& S, uint32_t n, uint32_t W, uint32_t x, uint32_t y, uint32_t i,
                             uint32_t j) {
    const uint32_t n2 = n * n;
    uint32_t c = j * n + i;
    R jt = (R)0.5;
    if (S.jitter == RT_JITTER_HASHED) {
        const uint32_t ray_id = (n * y + j) * (n * W) + n * x + i;
        const uint32_t key = hash_mix(S.tk ^ ray_id);
        jt = (R)(key >> 8) * (R)0x1p-24;
        const uint32_t r = hash_mix(S.tk ^ hash_mix(y * W + x)) % n2;
        c = (c + r) % n2;
    }
    const R u = ((R)c + jt) * S.inv_n2;
    const R su = S.span * u;  // multiply, then add
    return S.open + su;
}

// One launch of the tracer.
template <typename R>
struct LaunchParams {
    DevScene<R> scene;
    CameraRec<R> cam;
    const double* rays;      // color_at mode: n_rays x {o, d} (f64), else null
    uint64_t n_rays;
    void* out;               // row-major RGB of R (RT_OUT_REAL) or u8 (RT_OUT_U8)
    uint32_t out_format;
    uint32_t width, height;  // canvas
    uint32_t tiles_x;        // tiles per row
    uint32_t tile_rows;      // tile rows of THIS shard's strip
    uint32_t image_rows;     // 1: store pixels at their image rows of a whole W x H canvas (peer canvas),
                             // 0: at their strip rows (the shard's own strip)
    uint32_t shard_index, shard_count;
    uint32_t n_tiles;        // tiles_x * tile_rows (or ray chunks in color_at mode)
    uint32_t max_depth;      // `remaining` of the primary ray
    uint32_t pool_capacity;  // pool kernel: LIFO bound (rays) per workgroup
    uint32_t pool_lds_capacity;  // of which held in LDS; the rest in `spill`
    uint32_t pop_batch;      // pool kernel: rays a wave traces per iteration (<= 64)
    uint32_t acc_log2;       // f32 pool kernel: pixel sums in int32 multiples of 2^-acc_log2
    uint32_t persistent;     // kSched*: tile scheduling of this launch
    uint32_t flags;          // RT_FLAG_* diagnostic ablations
    uint32_t world_lds;      // bytes of world tables staged at the start of dynamic LDS (0 = none)
    void* spill;                 // pool overflow: grid x 8 x (pool_capacity - pool_lds_capacity) words
    uint32_t spill_blocks;       // workgroups the spill buffer holds regions for (RTC_BOUNDS_CHECK)
    uint32_t tiles_x_magic;      // div_magic(tiles_x, n_tiles): tile row = div_by(t, tiles_x, magic)
    unsigned long long* stamps;  // RT_FLAG_STAMPS: 2 x grid s_memrealtime values
    unsigned long long* item_log;  // RT_FLAG_STAMPS pool launches: [0] count, then 3 x u64 per item
    unsigned long long* tile_counter;  // kTileQueues queue heads, kQueueStride apart (zero at launch)
    unsigned long long* next_tile_counter;  // the heads of the next dynamic launch, zeroed by this one
    const uint32_t* tile_order;        // queue position -> work item (heaviest first), null = raster order
    const uint32_t* item_count;        // items in tile_order (>= n_tiles: split tiles), null = n_tiles
    uint32_t* tile_cost;               // pool kernel: per-tile duration (10 ns ticks), null = not recorded
    unsigned long long* counters;      // kCounterShards x kNumCounters cumulative u64
    unsigned long long* gen_counts;    // RT_FLAG_GENERATIONS: traced[kGenSlots], shaded[kGenSlots]; else null
    int32_t* error_flag;               // set nonzero on pool overflow
    uint32_t cull_cols[kCullCols];     // primary cull: slots whose rectangle misses a block column ...
    uint32_t cull_rows[kCullRows];     // ... or a block row (above); zero = none.  Bits 8..31: ShadowLayout's
    // Supersampled frames (trace_direct_ss, trace_pool_ss; 0 for every other
    // launch): n x n samples per pixel.  `cam` is then the sample camera (the
    // output camera resized to n x width by n x height) while width, height
    // and the tiles stay those of the output.  Last, so that no field the
    // shipped kernels load moves.
    uint32_t ss_grid;
    // The triangle hierarchy of the world (null / 0 for a world without one;
    // never read by per-scene builds).  The triangle step reads these from
    // the kernel arguments where it runs (rtc_kernels.hip for_triangles), so
    // they take no room in DevScene, which the kernels hold in registers.
    uint32_t n_tri_nodes;
    const TriNode<R>* tri_nodes;  // null: no tree, every triangle record is visited
    uint32_t tri_flat_begin;      // triangle records from this slot on are outside the tree (unbounded ones)
    // Mesh instances (null / 0 for a world without them; read where the
    // triangle step and the hit's lookup run, like the tree's fields above).
    uint32_t n_instances;
    int32_t inst_world_begin;          // world indices from here on are instances' triangles (n_shapes)
    const InstRec<R>* inst;            // by ascending world_base
    const ShapeRec<R>* inst_shapes;    // every mesh's local records
    const TriNode<R>* inst_nodes;      // every mesh's hierarchy
    const int32_t* inst_pos;           // InstRec::pos_begin
    // Smooth triangles (rt_scene_upload_smooth; null for every other world):
    // the vertex normals of the triangle run and of the meshes' local records,
    // dense and parallel to them (kShapeSmooth; a flat triangle's entry is
    // never read).  Read per lane, once per shaded hit on a smooth triangle,
    // by the instance build's prepare_hit; no other kernel loads them.
    const R* smooth_plain;
    const R* smooth_inst;
    // Image textures (rt_scene_upload_textured; null for every other world):
    // the coordinate tables, laid out like the normal tables (kShapeUV), the
    // texels of every texture in one allocation and the per-texture table.  A
    // PatternRec of kind RT_PATTERN_IMAGE holds its texture in sub_a and its
    // filter in sub_b.  `textures` is non-null exactly when the world has an
    // image pattern or a coordinate entry (such a world runs the texture build,
    // rtc::textured::launch_kernel); read by that build's prepare_hit only.
    const R* uv_plain;
    const R* uv_inst;
    const uint32_t* texels;
    const TexRec* textures;
    // Area lights (rt_scene_upload_lit; null / 0 for every other world): the
    // records in list order and the sum of their sample counts (what the event
    // counters add to n_lights per shaded hit).  A world with one runs the area
    // build (rtc::area::launch_kernel); read by that build's shade_ray only.
    const AreaLightRec<R>* area;
    uint32_t n_area;
    uint32_t area_samples;
    uint32_t area_cull;  // 1: the light-level caster cull runs (rtc_kernels.hip area_pass_mask); RTC_DEBUG=area_cull=0 clears it
    // The per-scene f32 direct kernel's launch terms (above); zero for every
    // other launch.  Appended, like the fields before it.
    LaunchTerms terms;
};
// (the kernels take LaunchParams by value with four table pointers behind it: one 4 KB kernarg segment)
static_assert(sizeof(LaunchParams<float>) + 4 * sizeof(void*) <= 4096 && sizeof(LaunchParams<double>) + 4 * sizeof(void*) <= 4096);
// (the lens kernels: LensParams behind the pointers, at this offset of the same segment)
template <typename R>
constexpr size_t kLensArgOffset = sizeof(LaunchParams<R>) + 4 * sizeof(void*);
static_assert(kLensArgOffset<float> % alignof(LensParams<float>) == 0 && kLensArgOffset<double> % alignof(LensParams<double>) == 0);
static_assert(kLensArgOffset<float> + sizeof(LensParams<float>) <= 4096 && kLensArgOffset<double> + sizeof(LensParams<double>) <= 4096);

}  // namespace rtc
