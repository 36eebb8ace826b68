// rtc_context.hpp — the per-device state behind an rt_context handle and the
// host-side internals shared by the single-device entry points
// (rtc_host.cpp) and the multi-GPU group (rtc_group.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rtc.h"
#include "device_memory.hpp"
#include "flop_model.hpp"
#include "kernel_id.hpp"
#include "rtc_internal.hpp"

namespace rtc {

// World tables cast to R and laid out per kind (rtc_internal.hpp).
// The shape, material and pattern tables and world_slot sit in ONE
// allocation in the kernels' LDS layout ([shapes][materials][patterns]
// [world_slot], world_lds_bytes), so a workgroup stages the world into LDS
// with one contiguous copy (scene_view).
// Sizes of a world's instance tables (the same for both precisions; a group's header carries them).
struct InstanceCounts {
    uint32_t instances = 0, records = 0, nodes = 0, pos = 0;
    int32_t world_begin = 0;  // world indices from here on are instances' triangles
};

// Entries of a world's per-triangle side table (the smooth triangles' normals,
// the texture coordinates): one per record of the triangle run and one per
// local record of the meshes, or zero where that part holds no such triangle
// (rtc_internal.hpp kShapeSmooth, kShapeUV).
struct SmoothCounts {
    uint32_t plain = 0, inst = 0;
};

// A side table of one precision, kReals reals an entry: the plain part's
// entries, then the meshes', outside the LDS image.
template <typename R, int kReals>
struct SideTable {
    DeviceBuffer<R> reals;
    SmoothCounts counts{};  // zeros: the world has no such triangle
    // Room for the entries of `c`.
    int allocate(const SmoothCounts& c) {
        if (int rc = reals.reserve(((size_t)c.plain + c.inst) * kReals)) return rc;
        counts = c;
        return RT_OK;
    }
    size_t bytes() const { return ((size_t)counts.plain + counts.inst) * kReals * sizeof(R); }
    const R* plain() const { return counts.plain ? reals.get() : nullptr; }
    const R* inst() const { return counts.inst ? reals.get() + (size_t)counts.plain * kReals : nullptr; }
};

// Which build of the tracer kernels a world runs (rtc_host.cpp kLaunchers): every
// build holds the code of the ones before it.  Stored in rt_context::kernel_build
// by set_kernel_build and nowhere re-derived.
enum class KernelBuild : uint32_t {
    plain,      // rtc::launch_kernel: worlds of shapes alone
    instanced,  // rtc::instanced::*: the instance level and the smooth triangle's normal (rtc_kernels.hip prepare_hit)
    textured,   // rtc::textured::*: ... plus the texture code, for an image pattern or a coordinate entry
    area,       // rtc::area::*: ... plus the area lights' sample loop
    mapped,     // rtc::mapped::*: ... plus the spherical, cylindrical and cube maps of an image pattern
    moving,     // rtc::moving::*: ... plus a time per ray, the displaced point of a mover and the shutter frame kernels
};

// Texel storage of a world (rt_scene_upload_textured): the texture count and the texels of all of them; a
// group's header carries them.  `on`: the world has an image pattern or a coordinate entry (it runs the
// texture code even where it holds no texture).
struct TextureCounts {
    uint32_t textures = 0, on = 0;
    uint64_t texels = 0;
};

template <typename R>
struct DeviceWorld {
    DeviceBuffer<unsigned char> image;  // the allocation holding the four tables
    ShapeRec<R>* shapes = nullptr;
    MaterialRec<R>* materials = nullptr;
    PatternRec<R>* patterns = nullptr;
    DeviceBuffer<LightRec<R>> lights;
    DeviceBuffer<TriNode<R>> tri_nodes;  // the triangle hierarchy (tri_tree.hpp), outside the LDS image
    uint32_t n_tri_nodes = 0;            // 0: the world has no tree
    uint32_t tri_flat_begin = 0;         // first triangle slot outside the tree
    int32_t* world_slot = nullptr;
    // Mesh instances (rt_scene_upload_instanced; rtc_internal.hpp InstRec): outside the LDS image like the tree
    DeviceBuffer<InstRec<R>> inst;
    DeviceBuffer<ShapeRec<R>> inst_shapes;  // every mesh's local records
    DeviceBuffer<TriNode<R>> inst_nodes;    // every mesh's hierarchy
    DeviceBuffer<int32_t> inst_pos;         // local index -> record (InstRec::pos_begin)
    InstanceCounts inst_counts{};           // zeros: a world without instances
    SideTable<R, kSmoothReals> smooth;  // smooth triangles (rt_scene_upload_smooth): the vertex normals
    // Texture coordinates (rt_scene_upload_textured); the texels and the per-texture table are the context's
    // (rt_context::texels), one copy for both precisions
    SideTable<R, kUVReals> uv;
    const uint32_t* texels = nullptr;
    const TexRec* tex_table = nullptr;      // non-null: the world runs the texture code
    // Area lights (rt_scene_upload_lit; rtc_internal.hpp AreaLightRec), outside the LDS image
    // Motion (rt_scene_upload_moving; rtc_internal.hpp MotionArg): the velocity tables, four reals an entry,
    // one entry per slot of the shape table and one per instance; outside the LDS image
    DeviceBuffer<R> shape_vel, inst_vel;
    bool moving = false;                    // the world has a mover: it runs the motion build
    DeviceBuffer<AreaLightRec<R>> area;
    uint32_t n_area = 0;                    // 0: a world without area lights
    uint32_t area_samples = 0;              // the sum of their sample counts
    DevScene<R> scene{};
    // Point the tables into `image` for ns shapes, nm materials, np patterns.
    void carve(size_t ns, size_t nm, size_t np) {
        unsigned char* b = image.get();
        shapes = reinterpret_cast<ShapeRec<R>*>(b);
        materials = reinterpret_cast<MaterialRec<R>*>(b + ns * sizeof(ShapeRec<R>));
        patterns = reinterpret_cast<PatternRec<R>*>(b + ns * sizeof(ShapeRec<R>) + nm * sizeof(MaterialRec<R>));
        world_slot = reinterpret_cast<int32_t*>(b + ns * sizeof(ShapeRec<R>) + nm * sizeof(MaterialRec<R>) +
                                                np * sizeof(PatternRec<R>));
    }
    // Room for the tables of ns shapes, nm materials and np patterns (an empty
    // world still gets a buffer) and for nl lights; what the buffers held is
    // gone if they grew.  Points the tables and the scene's view at them.
    int allocate(size_t ns, size_t nm, size_t np, size_t nl) {
        int rc;
        if ((rc = image.reserve(std::max<size_t>(world_lds_bytes<R>(ns, nm, np), 16))) || (rc = lights.reserve(nl)))
            return rc;
        carve(ns, nm, np);
        scene.shapes = shapes;
        scene.materials = materials;
        scene.patterns = patterns;
        scene.lights = nl ? lights.get() : nullptr;
        scene.world_slot = world_slot;
        scene.n_materials = (int32_t)nm;
        scene.n_patterns = (int32_t)np;
        scene.n_lights = (int32_t)nl;
        return RT_OK;
    }
    // Room for n nodes of the triangle hierarchy, flat run from record `flat_begin`; n = 0: no tree.
    int allocate_tree(size_t n, int32_t flat_begin) {
        if (int rc = tri_nodes.reserve(n)) return rc;
        n_tri_nodes = (uint32_t)n;
        tri_flat_begin = n ? (uint32_t)flat_begin : 0u;
        return RT_OK;
    }
    // Room for the instance tables of `c`; all zero: the world has no instances.
    int allocate_instances(const InstanceCounts& c) {
        int rc;
        if ((rc = inst.reserve(c.instances)) || (rc = inst_shapes.reserve(c.records)) ||
            (rc = inst_nodes.reserve(c.nodes)) || (rc = inst_pos.reserve(c.pos)))
            return rc;
        inst_counts = c;
        return RT_OK;
    }
    // Room for n area lights of `samples` samples in all; n = 0: the world has none.
    int allocate_area(uint32_t n, uint32_t samples) {
        if (int rc = area.reserve(n)) return rc;
        n_area = n;
        area_samples = n ? samples : 0u;
        return RT_OK;
    }
};

// Does the world hold instances the kernels walk?  (A world whose instances
// were all uploaded expanded is a plain world and holds none.)
template <typename R>
inline bool walked_instances(const DeviceWorld<R>& w) {
    return w.inst_counts.instances > 0;
}
// Does the world hold the texture tables (an image pattern, a triangle with texture coordinates or an area
// light: rt_scene_upload_textured, rt_scene_upload_lit)?
template <typename R>
inline bool has_textures(const DeviceWorld<R>& w) {
    return w.tex_table != nullptr;
}
// Does the world hold an area light (rt_scene_upload_lit)?
template <typename R>
inline bool has_area(const DeviceWorld<R>& w) {
    return w.n_area > 0;
}
// Does the world hold a smooth triangle (rt_scene_upload_smooth)?
template <typename R>
inline bool has_smooth(const DeviceWorld<R>& w) {
    return w.smooth.counts.plain > 0 || w.smooth.counts.inst > 0;
}

struct CodeBuild;  // rtc_jit.cpp: one hipRTC build of a per-scene kernel, possibly in flight

}  // namespace rtc

// One device's render state.  A single-device context is one of these; a
// multi-GPU context (rtc_group.cpp) is the rank-0 member, holding the other
// devices of the process as `group.peers`, each member with its own
// communicator.  Buffers, events and the stream are owning members
// (device_memory.hpp): ~rt_context does what needs an order, they do the rest.
struct rt_context {
    // A/B and diagnostic switches (debug_knobs.hpp: RTC_DEBUG=key=value,...)
    struct Knobs {
        // Defaults from A/B on MI355X (scripts/ab_sched.sh, scripts/stamps2.sh):
        // uniform-cost direct tiles -> static stride; high-variance pool tiles ->
        // per-XCD atomic queues; per-lane stores beat LDS-staged ones (the
        // staging barriers wait for store completion).
        // (RTC_DEBUG=sched_direct=grid|static; the pool kernel always takes the
        // per-XCD queues)
        uint32_t sched_direct = rtc::kSchedStatic;
        // f32 direct kernel's resident-grid multiple, in tenths (RTC_DEBUG=direct_oversub=T)
        uint32_t direct_oversub10 = 25;
        bool lds_world = true;      // RTC_DEBUG=lds_world=0 gathers shade data from global memory
        bool cull = true;  // RTC_DEBUG=cull=0 uploads every shape as unbounded (no wave cull; exactness tests)
        bool tri_tree = true;  // RTC_DEBUG=tri_tree=0 uploads without a triangle hierarchy (flat triangle loop)
        bool area_cull = true;  // RTC_DEBUG=area_cull=0: area lights' samples without the light-level caster cull
        // RTC_DEBUG=tri_min=N,tri_leaf=N: the sweep's values of tri_tree.hpp's kTriTreeMin and kTriLeaf (0 = those)
        uint32_t tri_min = 0, tri_leaf = 0;
        bool kind_variants = true;  // RTC_DEBUG=kind_variants=0: always the all-kinds kernels
        uint32_t pool_lds_rays = 0;  // RTC_DEBUG=pool_lds_rays=N: LDS-resident pool slots (0 = sized for occupancy)
        bool tile_order = true;      // RTC_DEBUG=tile_order=0: raster order always
        // Tiles costing more than split_factor x the mean workgroup load are
        // handed out in parts (order_tiles); RTC_DEBUG=split=0 never splits.  Round-3
        // sweep (per-scene kernels, slowest of 8 shards at 4K / 1-GPU frame):
        // 1.5: cover 0.239 / 1.132 ms, table 0.244 / 1.389; 1.0: 0.217 / 1.142,
        // 0.226 / 1.369; 0.75: 0.206 / 1.128, 0.233 / 1.384; 0.5: 0.205 / 1.128,
        // 0.245 / 1.414; reflect_refract 1080p, slowest of 4: 0.146 / 0.129 /
        // 0.126 / 0.131 with whole frames unchanged (0.385-0.403).
        double split_factor = 1.0;
        // RTC_DEBUG=split_max=L: log2 of the most parts a tile is split into.  Same-box
        // sweep (profiles/ab/r03_split16_sweep.txt, r03_shard_floor.txt), slowest
        // shard ms at 2 / 3 / 4: cover 4K of 8 0.198 / 0.202 / 0.207, of 32
        // 0.130 / 0.096 / 0.115; reflect_refract 1080p of 4 0.127 / 0.128 /
        // 0.121, of 16 0.112 / 0.092 / 0.097; whole frames split nothing.
        uint32_t split_max = 3;
        // Items (tiles or parts) costing more than urgent_factor x the mean
        // workgroup load run at raised wave priority, graded 1/2/3 above 1x/2x/4x
        // that cost (RTC_DEBUG=urgent=F, 0 = none; one level for all measured no better).  Same-box sweep, kernel ms, none / flat 0.25 / flat 0.125 /
        // graded 0.125: reflect_refract 0.367 / 0.310 / 0.306 / 0.310, cylinders
        // 0.124 / 0.117 / 0.117 / 0.117, cover 4K 1.014 / 1.023 / 1.011 / 1.011,
        // table 4K, refraction, metal within 1 %; slowest of 8 shards at 4K: cover
        // 0.215 / 0.201 / 0.215 / 0.201, table 0.229 / 0.266 / 0.230 / 0.231.
        double urgent_factor = 0.125;
    };
    // Heaviest-first tile order for repeated pool launches of the same frame
    // (order_tiles): per-tile costs of the last launch and its signature.
    struct TileOrder {
        rtc::DeviceBuffer<uint32_t> d_cost;   // one per tile
        rtc::DeviceBuffer<uint32_t> d_order;  // up to 2^kMaxSplitLog2 items per tile, then the item count
        uint64_t sig = 0;
        uint64_t geometry = 0;  // sig without the camera
        bool valid = false;
        bool built = false;     // d_order holds an order for `geometry`
        int builds = 0;         // order_tiles runs for the current signature so far
        // First launch of a frame geometry (no recorded costs): tiles handed out
        // centre-out instead of in raster order (full frames; shards keep raster).
        rtc::DeviceBuffer<uint32_t> d_cold;  // centre-out order + item count, for cold_w x cold_h
        uint32_t cold_w = 0, cold_h = 0;
    };
    // Per-scene f32 kernels (rtc_jit.cpp): the f32 shape table of the last
    // upload, the kernels built for it (direct/pool x global/LDS world), and
    // RTC_JIT / rt_context_set_jit = RT_JIT_OFF | RT_JIT_SYNC | RT_JIT_AUTO
    // (default) | RT_JIT_EAGER (rtc.h).
    struct Jit {
        std::vector<rtc::ShapeRec<float>> shapes;
        std::vector<rtc::LightRec<float>> lights;  // per-scene builds unroll the lights as constants
        std::vector<rtc::MaterialRec<float>> materials;  // ... and the direct kernel reads materials as constants
        std::vector<rtc::PatternRec<float>> pattern_recs;  // (pattern kinds present)
        bool patterns = true;                      // some material has a pattern (else pattern code is dropped)
        uint32_t pattern_kinds = ~0u;              // pattern kinds in the world's table (bit per RT_PATTERN_*)
        bool transparent = true;                   // some material is transparent (else no refraction code)
        int32_t begin[rtc::kNumKinds + 1] = {};
        // one entry per build of the world: KernelId::variant (kernel_id.hpp), the kernel's identity x
        // RT_FLAG_NO_SKIPS x (pool) 7 waves/SIMD (rtc_jit.cpp jit_function)
        static constexpr int kVariants = rtc::KernelId::kVariants;
        hipFunction_t fn[kVariants] = {};
        std::shared_ptr<rtc::CodeBuild> build[kVariants];  // the build each variant waits for (host thread)
        bool rejected[kVariants] = {};   // built, but refused for occupancy or scratch (that variant only)
        bool owner[kVariants] = {};      // this context started the build: its time goes into compile_ms
        uint32_t frames = 0;     // large f32 frames of this upload so far (RT_JIT_AUTO starts at the 2nd)
        std::string arch;            // the device's gfx target (gcnArchName), for hipRTC; read lazily (device_arch)
        int mode = 2;
        bool failed = false, used = false;  // failed: the world's build failed (compile or load)
        double compile_ms = 0;  // compile (or disk-cache load) time of this context's per-scene builds
        int cache_hits = 0;     // builds loaded from the on-disk cache
        std::string log;
        // A new upload: no kernel, build or verdict of the previous world is kept.
        void reset() {
            for (int v = 0; v < kVariants; ++v) {
                fn[v] = nullptr;
                build[v].reset();
                rejected[v] = owner[v] = false;
            }
            frames = 0;
            failed = false;
            log.clear();
        }
    };
    // Multi-GPU group (rtc_group.cpp).  A frame is split
    // into n_ranks shards of cyclic RT_TILE_H-row blocks; this member renders
    // shard `rank` into d_strip, RCCL gathers the strips onto rank 0, which
    // de-interleaves them into the image.  Single-device contexts: comm null.
    struct Group {
        ncclComm_t comm = nullptr;
        int n_ranks = 1, rank = 0;
        std::vector<rt_context*> peers;  // rank 0 of a one-process group: the other devices' members
        rtc::DeviceBuffer<int32_t> d_status;  // agree_status's word, allocated with the member so a rank can always join
        rtc::DeviceBuffer<unsigned char> d_strip;     // this member's shard strip
        rtc::DeviceBuffer<unsigned char> d_gathered;  // rank 0: every strip, shard-major
        rtc::Event ev_render0, ev_render1, ev_gather1;  // frame timing
        // RT_GATHER_PEER groups: the shared canvas (rank 0's allocation; mapped or
        // peer-accessed on the others) and the frame sequence number.
        int gather_mode = RT_GATHER_RCCL;
        void* canvas = nullptr;
        uint64_t canvas_bytes = 0, canvas_seq = 0;
    };

    rt_context() = default;
    rt_context(const rt_context&) = delete;
    rt_context& operator=(const rt_context&) = delete;
    // In this order: hipSetDevice, hipDeviceSynchronize (launches on caller
    // streams too), close the canvases, ncclCommDestroy; then the members.
    ~rt_context();

    int device = 0;
    int cu_count = 0;
    size_t lds_per_block = 64 * 1024;
    rtc::KernelBuild kernel_build = rtc::KernelBuild::plain;  // the uploaded world's (set_kernel_build)
    // occupancy cache of kernel_build's kernels, by KernelId::occupancy_slot (kernel_id.hpp): the dynamic LDS
    // size last asked about and the workgroups per CU at it (0: nothing cached)
    size_t occ_lds[rtc::KernelId::kOccupancyEntries] = {};
    int occ_blocks[rtc::KernelId::kOccupancyEntries] = {};
    Knobs knobs;
    rtc::Stream stream;
    rtc::Event ev_start, ev_stop;
    // Stream order across entry points: every launch shares the queue heads,
    // tile costs/order and pool spill.  rt_render_device runs on the caller's
    // stream, rt_render/rt_color_at on `stream`; a launch on a stream other
    // than the previous launch's first makes its stream wait on all work
    // submitted so far to that one (ev_order recorded at the switch).
    rtc::Event ev_order;
    hipStream_t last_stream = nullptr;
    bool launched = false;
    rtc::DeviceBuffer<unsigned long long> d_tile_counter;  // two sets of queue heads (launch: dynamic schedule)
    int head_set = 0;                              // the set the next dynamic launch uses
    rtc::DeviceBuffer<unsigned long long> d_counters;  // kNumCounters cumulative
    rtc::DeviceBuffer<unsigned long long> d_gen_counts;  // RT_FLAG_GENERATIONS: traced, shaded x kGenSlots, cumulative
    rtc::DeviceBuffer<int32_t> d_error;
    // rt_render: counters before/after and the error flag come back pinned,
    // on the stream, so a frame needs one host sync
    rtc::PinnedBuffer<unsigned long long> h_counters;  // 2 x kCounterShards x kNumCounters + the error flag
    bool have_scene = false;
    rtc::DeviceWorld<float> w32;
    rtc::DeviceWorld<double> w64;
    rtc::FlopScene flops;  // per-kind shape counts for the algorithmic FLOP model
    double bright_hit = 1.0, bright_w = 0.0;  // brightness bound of the world (acc_shift_f32)
    uint64_t scene_gen = 0;      // bumped by every rt_scene_upload
    uint32_t duplicate_shapes = 0;  // shapes value-equal to an earlier one (one identity class)
    rt_tree_info tree_info{};       // the triangle hierarchy of the uploaded world (rt_scene_tree_info; zeros = none)
    rt_instance_info instance_info{};  // meshes and instances of the uploaded world (rt_scene_instance_info)
    rt_smooth_info smooth_info{};      // smooth triangles of the uploaded world (rt_scene_smooth_info)
    std::vector<uint8_t> smooth_shape; // by plain shape: a smooth triangle (rt_debug_normal refuses it); empty: none
    // Image textures (rt_scene_upload_textured): the texels of every texture (a packed dword each) and the
    // per-texture table, shared by both precisions' worlds (DeviceWorld::texels, tex_table)
    rtc::DeviceBuffer<uint32_t> texels;
    rtc::DeviceBuffer<rtc::TexRec> tex_table;
    rtc::TextureCounts tex_counts{};
    rt_texture_info texture_info{};    // rt_scene_texture_info
    rt_light_info light_info{};        // area lights of the uploaded world (rt_scene_light_info)
    rt_map_info map_info{};            // texture maps of the uploaded world (rt_scene_map_info)
    rt_motion_info motion_info{};      // movers of the uploaded world (rt_scene_motion_info)
    std::vector<int32_t> world_slot;  // world index -> slot | kind << 24 of the uploaded table
    // ray-pool overflow regions, one per resident workgroup; a ray batch's per-lane LIFOs (launch_rays)
    rtc::DeviceBuffer<unsigned char> d_spill;
    TileOrder order;
    TileOrder order_ss;  // ... of the supersampled launches (rt_render_supersampled*): costs of n^2 samples per tile
    TileOrder order_lens;  // ... of the lens launches (rt_render_lens*): the lens in the signature
    TileOrder order_shutter;  // ... of the shutter launches (rt_render_shutter*): the lens and the shutter in the signature
    Jit jit;
    rtc::DeviceBuffer<unsigned char> d_scratch;  // host-buffer renders / color_at staging
    rtc::DeviceBuffer<unsigned long long> d_stamps;  // RT_FLAG_STAMPS diagnostics: two per workgroup
    uint32_t stamp_count = 0;
    rtc::DeviceBuffer<unsigned long long> d_item_log;  // RT_FLAG_STAMPS pool launches: a count, then item spans
    Group group;
    // Peer canvases this context created or mapped (rt_canvas_*): image
    // bytes and flag count per base pointer.
    struct Canvas {
        uint64_t bytes = 0;
        uint32_t n_flags = 0;
        bool owned = false;  // created here (hipFree) or mapped (hipIpcCloseMemHandle / peer pointer)
    };
    std::map<void*, Canvas> canvases;
};

namespace rtc {

// The context and the other devices' members of a one-process group.
inline std::vector<rt_context*> members(rt_context* ctx) {
    std::vector<rt_context*> m{ctx};
    m.insert(m.end(), ctx->group.peers.begin(), ctx->group.peers.end());
    return m;
}
inline size_t element_bytes(uint32_t out_format, uint32_t precision) {
    return out_format == RT_OUT_U8 ? 1 : (precision == RT_PRECISION_F32 ? 4 : 8);
}
inline size_t pixel_bytes(const rt_render_options* o) { return 3 * element_bytes(o->out_format, o->precision); }

// rtc_host.cpp
// RTC_DEBUG=trace_init=1: per-step milliseconds of context creation, upload and
// the first renders on stderr (the one-shot breakdown).
class InitTrace {
public:
    explicit InitTrace(const char* what);
    void step(const char* name);
private:
    const char* what_;
    bool on_;
    std::chrono::steady_clock::time_point t0_, t_;
};
int create_device_context(int device, rt_context** out);
void destroy_device_context(rt_context* ctx);  // null is fine
int check_ready(rt_context* ctx);
int check_options(const rt_render_options* o);
// kCounterShards x kNumCounters as the kernels keep them -> their sums
void sum_counter_shards(const unsigned long long* shards, unsigned long long out[kNumCounters]);
int read_counters(rt_context* ctx, unsigned long long out[kNumCounters]);
void fill_stats(rt_context* ctx, const unsigned long long before[kNumCounters],
                const unsigned long long after[kNumCounters], float ms, rt_stats* s);
int check_pool_error(rt_context* ctx);
int order_after_last(rt_context* ctx, hipStream_t stream);  // cross-stream launch order (rtc.h)
int copy_to_host(rt_context* ctx, void* out, size_t bytes);  // d_scratch -> caller host buffer, on ctx->stream
uint32_t tile_rows_for(uint32_t height, uint32_t shards, uint32_t shard);
// Every list an upload can carry (rtc.h rt_scene_upload ... rt_scene_upload_lit): an entry point fills the
// ones it takes and leaves the others empty.
struct WorldLists {
    const rt_shape_desc* shapes = nullptr;
    uint32_t n_shapes = 0;
    const rt_material_desc* materials = nullptr;
    uint32_t n_materials = 0;
    const rt_pattern_desc* patterns = nullptr;
    uint32_t n_patterns = 0;
    const rt_light_desc* lights = nullptr;
    uint32_t n_lights = 0;
    const rt_mesh_desc* meshes = nullptr;  // rt_scene_upload_instanced's lists
    uint32_t n_meshes = 0;
    const rt_instance_desc* instances = nullptr;
    uint32_t n_instances = 0;
    const rt_smooth_desc* smooth = nullptr;  // rt_scene_upload_smooth's list
    uint32_t n_smooth = 0;
    const rt_uv_desc* uvs = nullptr;  // rt_scene_upload_textured's lists
    uint32_t n_uvs = 0;
    const rt_texture_desc* textures = nullptr;
    uint32_t n_textures = 0;
    const rt_area_light_desc* area = nullptr;  // rt_scene_upload_lit's list
    uint32_t n_area = 0;
    // the upload came through rt_scene_upload_textured or rt_scene_upload_lit: image patterns are known and
    // checked against `textures` (the older entry points refuse pattern kind 6)
    bool image_patterns = false;
    const rt_uv_map_desc* maps = nullptr;  // rt_scene_upload_mapped's list
    uint32_t n_maps = 0;
    // the device texture table's records after the textures' own (a texture index each: instances.hpp
    // canonical_image_patterns), filled in by the upload once the maps are validated
    const int32_t* tex_records = nullptr;
    uint32_t n_tex_records = 0;
    const rt_motion_desc* motion = nullptr;  // rt_scene_upload_moving's list (the upload drops its zero velocities)
    uint32_t n_motion = 0;
};
// Every refusal of rtc.h for these lists, in the entry points' order: the area list, the texture list, the
// base tables, the mesh and instance lists, the smooth list, the uv list, the lights' total.
int validate_scene(const WorldLists& wl);
// Flatten and upload the validated lists to this device (no sync): the plain tables alone, or with the
// instance, side, texture and area tables, by what the lists hold; then set_kernel_build.
int build_scene(rt_context* ctx, const WorldLists& wl);
// The one place that stores which build of the kernels the context's world runs and that clears the
// occupancy cache (when the build changes): the end of a successful build_scene, and from the header on a
// group's other ranks.
void set_kernel_build(rt_context* ctx, KernelBuild build);
// One frame (or shard strip) of this device into `out_device` on `stream`.
int capture_jit_table(rt_context* ctx);  // the f32 table of the uploaded world, for rtc_jit.cpp
int fetch_jit_tables(rt_context* ctx);   // build_world<float>'s host tables read back (a group's other ranks)
int launch_frame(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, uint32_t shard_index,
                 uint32_t shard_count, void* out_device, hipStream_t stream, bool image_rows = false);
// Peer canvas internals (rtc_host.cpp): flags of a canvas, and the kernels.
unsigned long long* canvas_flags(void* canvas, uint64_t image_bytes);  // n_flags ready flags, then release
int canvas_create(rt_context* ctx, uint64_t bytes, uint32_t n_flags, void** canvas);
int canvas_close(rt_context* ctx, void* canvas);
hipError_t launch_canvas_signal(unsigned long long* flag, unsigned long long seq, hipStream_t stream);
hipError_t launch_canvas_wait(const unsigned long long* flags, uint32_t n, unsigned long long seq,
                              unsigned long long timeout_ticks, int32_t* err, hipStream_t stream);
unsigned long long timeout_ticks(double timeout_ms);
// rtc_jit.cpp: the per-scene kernel of this context's world for a launch of
// `static_blocks` workgroups per CU, or null (use the generic kernel)
constexpr uint32_t kJitMinTiles = 256;  // 64K pixels
// *pool_waves: the waves/SIMD the returned pool kernel was built for (7, or
// 0 = the static build's), so the caller can plan its LDS for them.
// id: the kernel the launch was planned for.  A supersampled kernel
// (trace_direct_ss / trace_pool_ss) is a build of its own that only worlds
// rendered supersampled ask for; its pool build is made at the static
// occupancy alone.  A lens kernel (trace_direct_lens / trace_pool_lens) likewise.
int jit_function(rt_context* ctx, KernelId id, size_t dyn_lds, int static_blocks, hipFunction_t* fn, bool no_skips,
                 int* pool_waves);
int jit_wait(rt_context* ctx, double timeout_ms, int* pending);
const std::string& device_arch(rt_context* ctx);  // rtc_jit.cpp: the device's gfx target, read once

// rtc_group.cpp: the same entry points on a multi-GPU context
int group_scene_upload(rt_context* ctx, const WorldLists& wl);
int group_render_device(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, void* out_device,
                        hipStream_t stream);
int group_render(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, void* out_host,
                 rt_stats* stats);
int group_read_counters(rt_context* ctx, rt_stats* totals);
hipError_t launch_assemble(const void* gathered, void* image, uint32_t width, uint32_t height, uint32_t shards,
                           uint32_t strip_rows, uint32_t bpp, hipStream_t stream);

#define RT_HIP(call)                                        \
    do {                                                    \
        if (int rc_ = hip_status((call), #call)) return rc_; \
    } while (0)

}  // namespace rtc
