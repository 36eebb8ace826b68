// rtc_ss_frames.inc — the bodies of the supersampled frame kernels, included
// twice by rtc_kernels.hip (inside namespace rtc): once as trace_direct_ss /
// trace_pool_ss (RTC_SS_LENS 0: rt_render_supersampled*, DESIGN.md §3.8) and
// once as trace_direct_lens / trace_pool_lens (RTC_SS_LENS 1: rt_render_lens*,
// §3.14; the lens is one more kernel argument).  The includer defines RTC_SS_DIRECT, RTC_SS_POOL (the kernels'
// names) and RTC_SS_LENS.  Two kernels of one text, not two instantiations of
// one template: the supersampled kernels keep their names and, instruction for
// instruction, the code they had before there was a lens (a body shared
// through an inlined function template compiled them differently).

// RTC_SS_LENS (trace_direct_lens): the same frame through a thin lens
// (rt_render_lens*, DESIGN.md §3.14): sample (i, j) is lens_ray's ray.  Nothing
// else changes: shade_ray runs with NoBlock and no launch terms here, so
// nothing downstream assumes that the primary rays share an origin.
// RTC_SS_SHUTTER (with RTC_SS_LENS; the motion build's trace_direct_shutter and
// trace_pool_shutter, rt_render_shutter*, DESIGN.md §3.17): the argument is a
// ShutterArg, the lens and the shutter; the sample also has a time
// (shutter_time), and a lens of aperture 0 (wave-uniform) takes camera_ray.
#ifndef RTC_SS_SHUTTER
#define RTC_SS_SHUTTER 0
#endif
template <typename R, bool kLds>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(sizeof(R) == 4 ? RTC_DIRECT_SS_WAVES : 1))) void RTC_SS_DIRECT(
#if RTC_SS_SHUTTER
    LaunchParams<R> P, RTC_WORLD_PARAMS(R), ShutterArg<R> sa) {
#elif RTC_SS_LENS
    LaunchParams<R> P, RTC_WORLD_PARAMS(R), LensParams<R> lens) {
#else
    LaunchParams<R> P, RTC_WORLD_PARAMS(R)) {
#endif
    extern __shared__ __align__(16) unsigned char smem[];
    (void)scene_view<R, kLds>(P, shapes, materials, patterns, lights, smem, true);
    Counts k = {};
    const uint32_t tid = threadIdx.x;
    for (uint32_t t = blockIdx.x;; t += gridDim.x) {  // (tiles as in trace_direct)
        const LaunchParams<R>& P = kernarg_params<R>();
        const DevScene<R> sc = scene_view<R, kLds>(P, shapes, materials, patterns, lights, smem);
        if (t >= P.n_tiles) break;
        uint32_t x, y;
        uint64_t out_idx;
        const bool valid = tile_pixel(P, t, tid, x, y, out_idx);
        const uint32_t n = __builtin_amdgcn_readfirstlane(P.ss_grid);
        V3<R> c = {(R)0, (R)0, (R)0};
        for (uint32_t j = 0; j < n; ++j) {
            for (uint32_t i = 0; i < n; ++i) {
                Shaded<R> sh;
                bool hit = false;
                if (valid) {
                    V3<R> o, d;
#if RTC_SS_SHUTTER
                    if (kernarg_lens<R>().aperture == (R)0) camera_ray(P.cam, n * x + i, n * y + j, o, d);
                    else lens_ray(P, kernarg_lens<R>(), n, x, y, i, j, o, d);
                    sh.tau = shutter_time(kernarg_shutter<R>(), n, P.width, x, y, i, j);
#elif RTC_SS_LENS
                    lens_ray(P, kernarg_lens<R>(), n, x, y, i, j, o, d);  // (re-read where it is used, as P is)
#else
                    camera_ray(P.cam, n * x + i, n * y + j, o, d);
#endif
#if RTC_AREA_LIGHTS
                    sh.ray_id = (n * y + j) * (n * P.width) + n * x + i;
                    if (shade_ray<R, false>(sc, o, d, P.max_depth, sh)) {
#else
                    if (shade_ray<R, false>(sc, o, d, 0, sh)) {
#endif
                        hit = true;
                        c = {c.x + sh.surface.x, c.y + sh.surface.y, c.z + sh.surface.z};
                    }
                }
                count_events(k, valid, hit, sh, sc.n_lights);
            }
        }
        const R inv = (R)1 / (R)(n * n);
        if (valid) store_pixel(P, out_idx, V3<R>{c.x * inv, c.y * inv, c.z * inv});
    }
    if (!(P.flags & RT_FLAG_NO_COUNTERS)) flush_counts(k, P.counters);
}

// trace_pool_ss: trace_pool with n^2 seedings per item.  The item loop, the
// accumulators, generations, split parts, priorities and cost stamps are
// trace_pool's; a sample is one more batch of the item's pixels, seeded at
// weight R(1) / R(n^2) and remaining = max_depth into the same fixed-point
// sums, which are order-independent, so the frame stays bit-deterministic.
// The weights of a pixel's samples sum to 1: the brightness bound behind
// acc_log2 and check_pixel_range is that of a plain frame.
// Seeding rule: sample s + 1 is seeded when the pool has drained.  The pool
// then never holds rays of two samples, and its bound is the plain frame's
// (rtc_internal.hpp pool_capacity_ss, with the proof).  The price is the
// thin generations at the end of each sample's tree instead of the item's.
// A tile's recorded cost is its whole n^2-sample duration.
// RTC_SS_LENS (trace_pool_lens): the seeds are lens_ray's rays, made at the
// seeding, where the lane knows x, y, i, j; the pool's entries and meta are
// unchanged.
template <typename R, bool kLds, bool kDup>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(sizeof(R) == 4 ? RTC_POOL_WAVES : 1))) void RTC_SS_POOL(
#if RTC_SS_SHUTTER
    LaunchParams<R> P, RTC_WORLD_PARAMS(R), ShutterArg<R> sa) {
#elif RTC_SS_LENS
    LaunchParams<R> P, RTC_WORLD_PARAMS(R), LensParams<R> lens) {
#else
    LaunchParams<R> P, RTC_WORLD_PARAMS(R)) {
#endif
    extern __shared__ __align__(16) unsigned char smem_all[];
    const DevScene<R> sc = scene_view<R, kLds>(P, shapes, materials, patterns, lights, smem_all, true);
    unsigned char* smem = smem_all + (kLds ? P.world_lds : 0);
    __shared__ unsigned int s_tile[2];
    __shared__ int s_top[2];
    const uint32_t cap = P.pool_capacity;
    const uint32_t lcap = P.pool_lds_capacity, gcap = cap - lcap;
    Pool<R> pl;
    pl.acc = reinterpret_cast<PoolAcc<R>*>(smem);
    pl.lds = reinterpret_cast<R*>(smem + 3 * kBlock * sizeof(PoolAcc<R>));
    const float acc_scale = __builtin_ldexpf(1.0f, (int)P.acc_log2);
    pl.lds_cap = (int)lcap;
    pl.spill = reinterpret_cast<R*>(P.spill) + spill_word(blockIdx.x, gcap, lcap, lcap);
    pl.spill_cap = (int)gcap;
#ifdef RTC_BOUNDS_CHECK
    pl.err = P.error_flag;
    if (!in_bounds(gcap == 0 || blockIdx.x < P.spill_blocks, P.error_flag, kErrBoundsSpill)) pl.spill_cap = 0;
#endif

    Counts k = {};
    const uint32_t tid = threadIdx.x;
    // (the queue heads alternate between dynamic launches as in trace_pool)
    if (P.persistent == kSchedDynamic && blockIdx.x == 0 && tid < (uint32_t)kTileQueues)
        P.next_tile_counter[tid * kQueueStride] = 0ull;
    uint32_t probe = 0;
    const uint32_t n_items = P.item_count && tid == 0 ? *P.item_count : P.n_tiles;
    const uint32_t n = __builtin_amdgcn_readfirstlane(P.ss_grid), n2 = n * n;
    const R seed_w = (R)1 / (R)n2;
    unsigned long long tile_start = 0;  // thread 0: s_memrealtime at the tile's start
    for (uint32_t it = 0;; ++it) {
        if (tid == 0) {
            s_tile[it & 1] = next_tile(P, it, probe, n_items);
            s_top[0] = 0;
            tile_start = __builtin_amdgcn_s_memrealtime();
        }
        for (int c = 0; c < 3; ++c) pl.acc[c * kBlock + tid] = 0;
        __syncthreads();
        const uint32_t item = __builtin_amdgcn_readfirstlane(s_tile[it & 1]);
        if (item == kNoItem) break;
        const WorkItem wi = decode_item(item, P.tile_order != nullptr);
        const uint32_t t = wi.tile, split = wi.split_log2;
#ifdef RTC_BOUNDS_CHECK
        if (!in_bounds(t < P.n_tiles, P.error_flag, kErrBoundsTile)) continue;  // (every thread: uniform)
#endif
        const uint32_t prio = wi.prio;
        if (prio) set_wave_prio(prio);
        // This thread's pixel, if it is on the canvas and in this item's part
        // of the tile (all of it unless split).  Worked out from the thread
        // index at each seeding and at the store: the opaque copy keeps the
        // compiler from hoisting the pixel, its sample coordinates and their
        // conversions above the generations, where they would be held in
        // VGPRs through every tree (reflect_refract's per-scene build: 56
        // B/lane of scratch held, 44 this way).
        // The generic build is the other way round: worked out once per item
        // and held it takes 36-56 B/lane, recomputed 92-112 (with or without
        // the opaque copy), so it keeps trace_pool's way.
#ifdef RTC_JIT
        auto pixel = [&](uint32_t& x, uint32_t& y, uint64_t& out_idx) {
            uint32_t lane = tid;
            asm volatile("" : "+v"(lane));
            return tile_pixel(P, t, lane, x, y, out_idx) && item_seeds(lane, wi);
        };
#else
        uint32_t x, y;
        uint64_t out_idx;
        const bool valid = tile_pixel(P, t, tid, x, y, out_idx) && item_seeds(tid, wi);
#endif
        // One sample after the other, j outer and i inner: its seeds enter a
        // drained pool (s_top[0] = 0: set with the item, and below once the
        // sample before has run out), then its generations run as trace_pool's.
        for (uint32_t sample = 0; sample < n2; ++sample) {
            if (sample) {
                // (the generations end on s_top[gen & 1] == 0; s_top[0] may hold
                // an older size.  Every thread has read the top it left on.)
                if (tid == 0) s_top[0] = 0;
                __syncthreads();
            }
            {
                const uint32_t j = sample / n, i = sample - j * n;
#ifdef RTC_JIT
                uint32_t x, y;
                uint64_t out_idx;
                const bool valid = pixel(x, y, out_idx);
#endif
                V3<R> o, d;
#if RTC_SS_SHUTTER
                if (valid) {
                    if (sa.lens.aperture == (R)0) camera_ray(P.cam, n * x + i, n * y + j, o, d);
                    else lens_ray(P, sa.lens, n, x, y, i, j, o, d);
                }
#elif RTC_SS_LENS
                if (valid) lens_ray(P, lens, n, x, y, i, j, o, d);
#else
                if (valid) camera_ray(P.cam, n * x + i, n * y + j, o, d);
#endif
                k.c[0] += wave_count(valid);
                const int slot = wave_reserve(valid, &s_top[0]);
                if (valid) pool_put(pl, slot, o, d, seed_w, tid | (P.max_depth << 8));
            }
            __syncthreads();
            for (uint32_t gen = 0;; ++gen) {
                const int cur = gen & 1;
                const int size = s_top[cur];
                if (size == 0) break;
                const int kpop = size < (int)P.pop_batch ? size : (int)P.pop_batch;
                const int bottom = size - kpop;
                const bool active = (int)tid < kpop;
                V3<R> ro, rd;
                R rw = (R)0;
                uint32_t meta = 0;
                if (active) pool_get(pl, bottom + (int)tid, ro, rd, rw, meta);
                if (tid == 0) s_top[cur ^ 1] = bottom;
                __syncthreads();  // every lane holds its ray; the next top is set
                Shaded<R> sh;
                bool hit = false;
                const uint32_t pix = meta & 0xFFu;
                const uint32_t child_meta = pix | (((meta >> 8) - 1u) << 8);
                auto push = [&](V3<R> co, V3<R> cd, R cw) {
                    const int slot = wave_reserve(true, &s_top[cur ^ 1]);
                    if (slot < (int)cap) pool_put(pl, slot, co, cd, rw * cw, child_meta);
                    else atomicOr(P.error_flag, kErrPoolOverflow);
                };
#if RTC_AREA_LIGHTS
                // (one sample's rays at a time in the pool: the sample is the loop's, the pixel the entry's)
                sh.ray_id = sample_ray_id(P, t, pix, n, sample - (sample / n) * n, sample / n);
#endif
#if RTC_SS_SHUTTER
                {  // the entry's time from its pixel and the loop's sample, where its ray_id is: the pool's entries stay as they are
                    uint32_t sx, sy;
                    uint64_t so;
                    (void)tile_pixel(P, t, pix, sx, sy, so);
                    sh.tau = shutter_time(kernarg_shutter<R>(), n, P.width, sx, sy, sample - (sample / n) * n, sample / n);
                }
#endif
                if (active) hit = shade_ray<R, true, kDup>(sc, ro, rd, meta >> 8, sh, push);
                count_events(k, false, hit, sh, sc.n_lights);
                if (hit) {
                    acc_add(pl.acc, pix, sh.surface.x * rw, acc_scale);
                    acc_add(pl.acc + kBlock, pix, sh.surface.y * rw, acc_scale);
                    acc_add(pl.acc + 2 * kBlock, pix, sh.surface.z * rw, acc_scale);
                }
                __syncthreads();  // pushes complete before the next pop
                if (s_top[cur ^ 1] > (int)cap) {  // overflowed: drop the pool (error already flagged)
                    __syncthreads();
                    if (tid == 0) s_top[cur ^ 1] = 0;
                    __syncthreads();
                }
            }
        }
        const double inv = sizeof(PoolAcc<R>) == 4 ? __builtin_ldexp(1.0, -(int)P.acc_log2) : kAccInvScale;
        const V3<R> c = {(R)((double)pl.acc[tid] * inv), (R)((double)pl.acc[kBlock + tid] * inv),
                         (R)((double)pl.acc[2 * kBlock + tid] * inv)};
#ifdef RTC_JIT
        uint32_t x, y;
        uint64_t out_idx;
        const bool valid = pixel(x, y, out_idx);
#endif
        bool store = valid;
#ifdef RTC_BOUNDS_CHECK
        store &= in_bounds(!valid || out_idx < (uint64_t)(P.image_rows ? P.height : P.tile_rows * RT_TILE_H) * P.width,
                           P.error_flag, kErrBoundsOut);
#endif
        if (store) store_pixel(P, out_idx, c);
        if (prio) __builtin_amdgcn_s_setprio(0);
        __syncthreads();  // accumulators are re-zeroed for the next tile
        if (tid == 0 && P.tile_cost) {  // (as trace_pool: a split tile's slowest part times the parts)
            const uint32_t c = (uint32_t)min(__builtin_amdgcn_s_memrealtime() - tile_start, 0x0FFFFFFFull);
            if (split) atomicMax(&P.tile_cost[t], c << split);
            else P.tile_cost[t] = c;
        }
    }
    if (!(P.flags & RT_FLAG_NO_COUNTERS)) flush_counts(k, P.counters);
}
