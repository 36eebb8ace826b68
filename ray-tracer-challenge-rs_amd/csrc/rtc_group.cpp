// rtc_group.cpp — multi-GPU contexts behind the C-ABI (include/rtc.h).
//
// The north star tiles one image across the GPUs of a node: "RCCL broadcast
// of the scene + gather of framebuffer strips over xGMI" (SURVEY.md §8b, §8e).
// The reference's contract is that the library owns the parallelism and the
// caller just calls render_parallel (camera.rs:97-112), so the split lives
// here, not in the caller:
//
//   rt_scene_upload*  rank 0 flattens the World (rtc_host.cpp build_scene)
//                     and ncclBroadcasts a header plus the four device
//                     buffers (per precision: the table image, the lights)
//                     (f32 and f64 records) to every other GPU.
//   rt_render[_device] every member renders its shard — cyclic RT_TILE_H-row
//                     blocks (rank r takes tile rows r, r+G, ...), which
//                     spreads the cost of expensive rows (cover's reflective
//                     cubes) — into a contiguous strip; ncclGather brings the
//                     strips to rank 0 (equal counts: every strip is padded
//                     to rt_shard_rows rows); rank 0 de-interleaves them
//                     into the image (assemble_shards).
//
// Members: rank 0 of a one-process group (rt_context_create_multi) is the
// context handed to the caller and holds the other devices' members in
// `peers`; RCCL calls for all of them go in one ncclGroupStart/End.  In the
// one-process-per-GPU form (rt_context_create_rank) each process holds just
// its own member and the same code runs with one local member.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rtc.h"
#include "rtc_context.hpp"

namespace rtc {
namespace {

#define RT_NCCL(call)                                                                                      \
    do {                                                                                                   \
        ncclResult_t r_ = (call);                                                                          \
        if (r_ != ncclSuccess) return set_error(RT_ERR_COMM, std::string(#call) + ": " + ncclGetErrorString(r_)); \
    } while (0)

// The flattened world's shape, broadcast ahead of the tables so the other
// ranks can allocate them.
struct SceneHeader {
    int32_t status;  // rank 0's validation/upload result: the others fail with it too
    KernelBuild build;  // the kernels the world runs (rank 0's build_scene chose them)
    uint32_t ns, nm, np, nl;
    uint32_t n_world_slots;  // world indices world_slot answers for (ns, but for an instanced world)
    int32_t kind_begin[kNumKinds + 1];
    int32_t any_secondary;
    uint32_t duplicates;
    double flops_per_ray;
    double bright_hit, bright_w;  // acc_shift_f32's bound
    uint32_t n_tri_nodes;         // the triangle hierarchy (tri_tree.hpp): 0 = none
    int32_t tri_flat_begin;
    rt_tree_info tree_info;
    InstanceCounts inst;  // mesh instances (rt_scene_upload_instanced): zeros = none
    rt_instance_info instance_info;
    SmoothCounts smooth;  // smooth triangles (rt_scene_upload_smooth): zeros = none
    rt_smooth_info smooth_info;
    SmoothCounts uv;      // image textures (rt_scene_upload_textured): zeros = none
    TextureCounts tex;
    rt_texture_info texture_info;
    uint32_t n_area, area_samples;  // area lights (rt_scene_upload_lit): zeros = none
    rt_light_info light_info;
    rt_map_info map_info;  // texture maps (rt_scene_upload_mapped): zeros = none
};

// (device pointer, bytes) of every table of a member's world, in one order
// on every rank.
template <typename R>
void world_buffers(DeviceWorld<R>& w, const SceneHeader& h, std::vector<std::pair<void*, size_t>>& out) {
    out.push_back({w.image.get(), world_lds_bytes<R>(h.ns, h.nm, h.np)});  // shapes, materials, patterns, world_slot
    out.push_back({w.lights.get(), h.nl * sizeof(LightRec<R>)});
    out.push_back({w.tri_nodes.get(), h.n_tri_nodes * sizeof(TriNode<R>)});
    out.push_back({w.inst.get(), h.inst.instances * sizeof(InstRec<R>)});
    out.push_back({w.inst_shapes.get(), h.inst.records * sizeof(ShapeRec<R>)});
    out.push_back({w.inst_nodes.get(), h.inst.nodes * sizeof(TriNode<R>)});
    out.push_back({w.inst_pos.get(), h.inst.pos * sizeof(int32_t)});
    out.push_back({w.smooth.reals.get(), w.smooth.bytes()});  // (allocated for the header's counts)
    out.push_back({w.uv.reals.get(), w.uv.bytes()});
    out.push_back({w.area.get(), (size_t)h.n_area * sizeof(AreaLightRec<R>)});
}

// Rank 0's `value` to every member of every rank, over RCCL (collective):
// got[i] is what ms[i] received.
template <typename T>
int broadcast_value(const std::vector<rt_context*>& ms, const T& value, std::vector<T>& got) {
    std::vector<DeviceBuffer<T>> d(ms.size());
    for (size_t i = 0; i < ms.size(); ++i) {
        RT_HIP(hipSetDevice(ms[i]->device));
        if (int rc = d[i].reserve(1)) return rc;
        if (ms[i]->group.rank == 0) RT_HIP(hipMemcpy(d[i].get(), &value, sizeof(T), hipMemcpyHostToDevice));
    }
    RT_NCCL(ncclGroupStart());
    for (size_t i = 0; i < ms.size(); ++i)
        RT_NCCL(ncclBroadcast(d[i].get(), d[i].get(), sizeof(T), ncclUint8, 0, ms[i]->group.comm, ms[i]->stream));
    RT_NCCL(ncclGroupEnd());
    got.resize(ms.size());
    for (size_t i = 0; i < ms.size(); ++i) {
        RT_HIP(hipSetDevice(ms[i]->device));
        RT_HIP(hipStreamSynchronize(ms[i]->stream));
        RT_HIP(hipMemcpy(&got[i], d[i].get(), sizeof(T), hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

int init_member(rt_context* m, ncclComm_t comm, int n_ranks, int rank) {
    rt_context::Group& g = m->group;
    g.comm = comm;  // (the member owns it from here on: ~rt_context)
    g.n_ranks = n_ranks;
    g.rank = rank;
    RT_HIP(hipSetDevice(m->device));
    int rc;
    if ((rc = g.ev_render0.create()) || (rc = g.ev_render1.create()) || (rc = g.ev_gather1.create())) return rc;
    return g.d_status.reserve(1);
}

// The shards of one frame: every local member renders its strip on its
// stream (rank 0's on `root_stream`), RCCL gathers the strips onto rank 0,
// rank 0 de-interleaves them into `image` (rank 0's device).  With `timed`,
// events bracket each member's render and rank 0's gather + assemble.
int render_shards_peer(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, void* image,
                       hipStream_t root_stream, bool timed);

int render_shards(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, void* image,
                  hipStream_t root_stream, bool timed) {
    if (ctx->group.gather_mode == RT_GATHER_PEER) return render_shards_peer(ctx, cam, o, image, root_stream, timed);
    const std::vector<rt_context*> ms = members(ctx);
    const uint32_t G = (uint32_t)ctx->group.n_ranks;
    const uint32_t rows = tile_rows_for(cam->height, G, 0) * RT_TILE_H;  // shard 0 has the most rows
    const size_t strip = (size_t)rows * cam->width * pixel_bytes(o);
    int rc;
    auto stream_of = [&](rt_context* m) { return m->group.rank == 0 ? root_stream : m->stream; };
    for (rt_context* m : ms) {
        RT_HIP(hipSetDevice(m->device));
        rt_context::Group& g = m->group;
        if ((rc = g.rank ? g.d_strip.reserve(strip) : g.d_gathered.reserve(strip * G))) return rc;
    }
    // Rank 0 renders its strip straight into its slot of the gather buffer
    // (slot 0), and gathers in place: RCCL then copies only the other ranks'.
    auto strip_of = [&](rt_context* m) { return m->group.rank ? m->group.d_strip.get() : m->group.d_gathered.get(); };
    for (rt_context* m : ms) {
        hipStream_t s = stream_of(m);
        RT_HIP(hipSetDevice(m->device));
        if (timed) RT_HIP(hipEventRecord(m->group.ev_render0, s));
        if ((rc = launch_frame(m, cam, o, (uint32_t)m->group.rank, G, strip_of(m), s))) return rc;
        if (timed) RT_HIP(hipEventRecord(m->group.ev_render1, s));
    }
    RT_NCCL(ncclGroupStart());
    for (rt_context* m : ms)
        RT_NCCL(ncclGather(strip_of(m), m->group.rank ? nullptr : m->group.d_gathered.get(), strip, ncclUint8, 0,
                           m->group.comm, stream_of(m)));
    RT_NCCL(ncclGroupEnd());
    for (rt_context* m : ms) {
        if (m->group.rank != 0) continue;
        RT_HIP(hipSetDevice(m->device));
        RT_HIP(launch_assemble(m->group.d_gathered.get(), image, cam->width, cam->height, G, rows, (uint32_t)pixel_bytes(o),
                               root_stream));
        if (timed) RT_HIP(hipEventRecord(m->group.ev_gather1, root_stream));
    }
    return RT_OK;
}

// RT_GATHER_PEER: the group's canvas on rank 0, big enough for `bytes` of
// image (every rank asks for the same size: collective).  One process per
// GPU: rank 0 creates it and RCCL-broadcasts its IPC handle, the others map
// it.  One process with several GPUs: the other members write through peer
// access to rank 0's pointer.
int ensure_group_canvas(rt_context* ctx, uint64_t bytes) {
    const std::vector<rt_context*> ms = members(ctx);
    if (ctx->group.canvas && ctx->group.canvas_bytes >= bytes) return RT_OK;
    const uint32_t G = (uint32_t)ctx->group.n_ranks;
    const bool remote = (int)ms.size() < ctx->group.n_ranks;  // ranks in other processes
    int rc;
    for (rt_context* m : ms) {  // drop the old canvas (rank 0's allocation, a mapping, or a peer pointer)
        if (m->group.canvas && m->canvases.count(m->group.canvas) && (rc = canvas_close(m, m->group.canvas))) return rc;
        m->group.canvas = nullptr;
        m->group.canvas_bytes = 0;
        m->group.canvas_seq = 0;  // a new canvas's flags start at 0: its first frame is seq 1 on every rank
    }
    void* root = nullptr;
    for (rt_context* m : ms)
        if (m->group.rank == 0) {
            if ((rc = canvas_create(m, bytes, G, &root))) return rc;
            m->group.canvas = root;
            m->group.canvas_bytes = bytes;
        }
    if (remote) {  // the IPC handle from rank 0 to every rank, over RCCL
        hipIpcMemHandle_t h{};
        if (root) {
            RT_HIP(hipSetDevice(ctx->device));
            RT_HIP(hipIpcGetMemHandle(&h, root));
        }
        std::vector<hipIpcMemHandle_t> got;
        if ((rc = broadcast_value(ms, h, got))) return rc;
        for (size_t i = 0; i < ms.size(); ++i) {
            if (ms[i]->group.rank == 0) continue;
            RT_HIP(hipSetDevice(ms[i]->device));
            void* p = nullptr;
            RT_HIP(hipIpcOpenMemHandle(&p, got[i], hipIpcMemLazyEnablePeerAccess));
            ms[i]->canvases[p] = {bytes, G, false};
            ms[i]->group.canvas = p;
            ms[i]->group.canvas_bytes = bytes;
        }
    } else {  // every rank in this process: peer access to rank 0's device
        for (rt_context* m : ms) {
            if (m->group.rank == 0) continue;
            RT_HIP(hipSetDevice(m->device));
            if (m->device != ctx->device) {
                hipError_t e = hipDeviceEnablePeerAccess(ctx->device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                    return set_error(RT_ERR_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
                (void)hipGetLastError();
            }
            m->group.canvas = root;
            m->group.canvas_bytes = bytes;
        }
    }
    return RT_OK;
}

// RT_GATHER_PEER frame: each member waits until rank 0 has released the
// previous frame, renders its shard at image rows into the canvas and raises
// its flag; rank 0 waits for every flag, copies the image out and releases
// the frame.  No strip, no gather, no de-interleave.
constexpr double kPeerTimeoutMs = 10000.0;
int render_shards_peer(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, void* image,
                       hipStream_t root_stream, bool timed) {
    const std::vector<rt_context*> ms = members(ctx);
    const uint32_t G = (uint32_t)ctx->group.n_ranks;
    const uint64_t bytes = (uint64_t)cam->width * cam->height * pixel_bytes(o);
    int rc;
    if ((rc = ensure_group_canvas(ctx, bytes))) return rc;
    auto stream_of = [&](rt_context* m) { return m->group.rank == 0 ? root_stream : m->stream; };
    for (rt_context* m : ms) {
        hipStream_t s = stream_of(m);
        RT_HIP(hipSetDevice(m->device));
        const uint64_t seq = ++m->group.canvas_seq;  // every rank renders the same frames: the same number
        unsigned long long* flags = canvas_flags(m->group.canvas, m->group.canvas_bytes);
        if (seq > 1) RT_HIP(launch_canvas_wait(flags + G, 1, seq - 1, timeout_ticks(kPeerTimeoutMs), m->d_error.get(), s));
        if (timed) RT_HIP(hipEventRecord(m->group.ev_render0, s));
        if ((rc = launch_frame(m, cam, o, (uint32_t)m->group.rank, G, m->group.canvas, s, true))) return rc;
        if (timed) RT_HIP(hipEventRecord(m->group.ev_render1, s));
        RT_HIP(launch_canvas_signal(flags + m->group.rank, seq, s));
    }
    for (rt_context* m : ms) {
        if (m->group.rank != 0) continue;
        RT_HIP(hipSetDevice(m->device));
        unsigned long long* flags = canvas_flags(m->group.canvas, m->group.canvas_bytes);
        RT_HIP(launch_canvas_wait(flags, G, m->group.canvas_seq, timeout_ticks(kPeerTimeoutMs), m->d_error.get(),
                                  root_stream));
        if (image) RT_HIP(hipMemcpyAsync(image, m->group.canvas, bytes, hipMemcpyDeviceToDevice, root_stream));
        RT_HIP(launch_canvas_signal(flags + G, m->group.canvas_seq, root_stream));
        if (timed) RT_HIP(hipEventRecord(m->group.ev_gather1, root_stream));
    }
    return RT_OK;
}

// One member's ray counts and FLOPs into the group's.
void add_rays(rt_stats& t, const rt_stats& s) {
    t.primary += s.primary;
    t.shadow += s.shadow;
    t.reflect += s.reflect;
    t.refract += s.refract;
    t.shaded += s.shaded;
    t.lit_patterned += s.lit_patterned;
    t.refract_evals += s.refract_evals;
    t.schlick_evals += s.schlick_evals;
    t.algorithmic_flops += s.algorithmic_flops;
}

int check_group_options(rt_context* ctx, const rt_render_options* o) {
    if (o->shard_count != 1 || o->shard_index != 0)
        return set_error(RT_ERR_INVALID, "a multi-GPU context shards frames itself: shard_index/shard_count must be 0/1");
    for (rt_context* m : members(ctx))
        if (!m->have_scene) return set_error(RT_ERR_NO_SCENE, "render before rt_scene_upload");
    return RT_OK;
}

}  // namespace

// The group's agreement on one step's outcome: every member of every rank
// contributes `local` (RT_OK or its error) to a max all-reduce of -status;
// RT_ERR_COMM when another rank failed, RT_OK when none did (a member's own
// failure is returned by its caller).
int agree_status(const std::vector<rt_context*>& ms, int local) {
    // The status words were allocated with the members (init_member), so a
    // rank always takes part in the all-reduce: a member whose word cannot be
    // written still joins (its stale word is overwritten by the max) and
    // reports its own error afterwards, instead of leaving the other ranks
    // blocked in the collective.
    const int32_t mine = local ? -local : 0;
    std::vector<int32_t> got(ms.size(), 0);
    int rc = RT_OK;
    auto word = [&](size_t i) { return ms[i]->group.d_status.get(); };
    for (size_t i = 0; i < ms.size(); ++i) {
        if (hipSetDevice(ms[i]->device) != hipSuccess ||
            hipMemcpyAsync(word(i), &mine, sizeof mine, hipMemcpyHostToDevice, ms[i]->stream) != hipSuccess)
            if (!rc) rc = set_error(RT_ERR_HIP, "status exchange: writing the status word");
    }
    ncclResult_t r = ncclGroupStart();
    for (size_t i = 0; i < ms.size() && r == ncclSuccess; ++i)
        r = ncclAllReduce(word(i), word(i), 1, ncclInt32, ncclMax, ms[i]->group.comm, ms[i]->stream);
    if (r == ncclSuccess) r = ncclGroupEnd();
    for (size_t i = 0; i < ms.size() && r == ncclSuccess; ++i) {
        if (hipSetDevice(ms[i]->device) != hipSuccess || hipStreamSynchronize(ms[i]->stream) != hipSuccess ||
            hipMemcpy(&got[i], word(i), sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
            if (!rc) rc = set_error(RT_ERR_HIP, "status exchange: read back");
    }
    if (r != ncclSuccess) return set_error(RT_ERR_COMM, std::string("status exchange: ") + ncclGetErrorString(r));
    if (rc) return rc;
    for (int32_t g : got)
        if (g && !local) return set_error(RT_ERR_COMM, "another rank of the group failed (status " + std::to_string(-g) + ")");
    return RT_OK;
}

int group_scene_upload(rt_context* ctx, const WorldLists& wl) {
    const std::vector<rt_context*> ms = members(ctx);
    int rc;
    SceneHeader root_h{};
    for (rt_context* m : ms) {  // launches on caller streams may still read the old tables
        RT_HIP(hipSetDevice(m->device));
        RT_HIP(hipDeviceSynchronize());
        m->have_scene = false;
    }
    int root_rc = RT_OK;
    std::string root_err;
    if (ctx->group.rank == 0) {  // only rank 0's tables are used (rtc.h)
        // a failure here still takes part in the header broadcast, so the
        // other ranks return it instead of waiting in the table broadcast
        // (a world whose image patterns are known was checked and then rewritten by upload_world on every rank)
        root_rc = wl.image_patterns ? RT_OK : validate_scene(wl);
        if (!root_rc && hipSetDevice(ctx->device) != hipSuccess) root_rc = set_error(RT_ERR_HIP, "hipSetDevice");
        if (!root_rc) root_rc = build_scene(ctx, wl);
        if (root_rc) root_err = rt_last_error();
        root_h.status = root_rc;
        root_h.build = ctx->kernel_build;
        root_h.n_world_slots = (uint32_t)ctx->world_slot.size();
        root_h.inst = ctx->w32.inst_counts;
        root_h.instance_info = ctx->instance_info;
        root_h.smooth = ctx->w32.smooth.counts;
        root_h.smooth_info = ctx->smooth_info;
        root_h.uv = ctx->w32.uv.counts;
        root_h.tex = ctx->tex_counts;
        root_h.texture_info = ctx->texture_info;
        root_h.n_area = ctx->w32.n_area;
        root_h.area_samples = ctx->w32.area_samples;
        root_h.light_info = ctx->light_info;
        root_h.map_info = ctx->map_info;
        // (the shape table's size: an instanced world's also holds the instances uploaded expanded)
        root_h.ns = root_rc ? wl.n_shapes : (uint32_t)ctx->w32.scene.kind_begin[kNumKinds];
        root_h.nm = wl.n_materials;
        root_h.np = wl.n_patterns;
        root_h.nl = wl.n_lights;
        for (int k = 0; k <= kNumKinds; ++k) root_h.kind_begin[k] = ctx->w32.scene.kind_begin[k];
        root_h.any_secondary = ctx->w32.scene.any_secondary;
        root_h.duplicates = ctx->duplicate_shapes;
        root_h.flops_per_ray = ctx->flops.per_ray;
        root_h.bright_hit = ctx->bright_hit;
        root_h.bright_w = ctx->bright_w;
        root_h.n_tri_nodes = ctx->w32.n_tri_nodes;
        root_h.tri_flat_begin = (int32_t)ctx->w32.tri_flat_begin;
        root_h.tree_info = ctx->tree_info;
    }
    // 1. the header
    std::vector<SceneHeader> hdr;
    if ((rc = broadcast_value(ms, root_h, hdr))) return rc;
    if (root_rc) return set_error(root_rc, root_err);
    for (const SceneHeader& h : hdr)
        if (h.status) return set_error(h.status, "rt_scene_upload failed on rank 0");

    // 2. the tables, broadcast in place from rank 0's device buffers.  Every
    // rank first allocates its copies, then the ranks agree on the outcome
    // (one all-reduce of a status word): a rank whose allocation failed still
    // takes part, so no other rank is left waiting in the table broadcast.
    int local_rc = RT_OK;
    std::string local_err;
    for (size_t i = 0; i < ms.size() && !local_rc; ++i) {
        rt_context* m = ms[i];
        if (hipSetDevice(m->device) != hipSuccess) local_rc = set_error(RT_ERR_HIP, "hipSetDevice");
        else if (m->group.rank != 0) {
            const SceneHeader& h = hdr[i];
            if ((local_rc = m->w32.allocate(h.ns, h.nm, h.np, h.nl)) == RT_OK &&
                (local_rc = m->w64.allocate(h.ns, h.nm, h.np, h.nl)) == RT_OK &&
                (local_rc = m->w32.allocate_tree(h.n_tri_nodes, h.tri_flat_begin)) == RT_OK &&
                (local_rc = m->w64.allocate_tree(h.n_tri_nodes, h.tri_flat_begin)) == RT_OK &&
                (local_rc = m->w32.allocate_instances(h.inst)) == RT_OK &&
                (local_rc = m->w64.allocate_instances(h.inst)) == RT_OK &&
                (local_rc = m->w32.smooth.allocate(h.smooth)) == RT_OK &&
                (local_rc = m->w64.smooth.allocate(h.smooth)) == RT_OK &&
                (local_rc = m->w32.uv.allocate(h.uv)) == RT_OK && (local_rc = m->w64.uv.allocate(h.uv)) == RT_OK &&
                (local_rc = m->w32.allocate_area(h.n_area, h.area_samples)) == RT_OK &&
                (local_rc = m->w64.allocate_area(h.n_area, h.area_samples)) == RT_OK &&
                (local_rc = m->texels.reserve(h.tex.on ? std::max<uint64_t>(h.tex.texels, 1) : 0)) == RT_OK)
                local_rc = m->tex_table.reserve(h.tex.on ? std::max<uint32_t>(h.tex.textures, 1u) : 0);
            // (the texels and the per-texture table: one copy a member, seen by both precisions' worlds)
            m->tex_counts = h.tex;
            m->w32.texels = m->w64.texels = h.tex.on && !local_rc ? m->texels.get() : nullptr;
            m->w32.tex_table = m->w64.tex_table = h.tex.on && !local_rc ? m->tex_table.get() : nullptr;
        }
        if (local_rc) local_err = rt_last_error();
    }
    if ((rc = agree_status(ms, local_rc))) return rc;
    if (local_rc) return set_error(local_rc, local_err);
    RT_NCCL(ncclGroupStart());
    for (size_t i = 0; i < ms.size(); ++i) {
        std::vector<std::pair<void*, size_t>> bufs;
        world_buffers(ms[i]->w32, hdr[i], bufs);
        world_buffers(ms[i]->w64, hdr[i], bufs);
        if (hdr[i].tex.on) {
            bufs.push_back({ms[i]->texels.get(), std::max<uint64_t>(hdr[i].tex.texels, 1) * sizeof(uint32_t)});
            bufs.push_back({ms[i]->tex_table.get(), std::max<uint32_t>(hdr[i].tex.textures, 1u) * sizeof(TexRec)});
        }
        for (auto& b : bufs)
            if (b.second) RT_NCCL(ncclBroadcast(b.first, b.first, b.second, ncclUint8, 0, ms[i]->group.comm, ms[i]->stream));
    }
    RT_NCCL(ncclGroupEnd());
    for (size_t i = 0; i < ms.size(); ++i) {
        rt_context* m = ms[i];
        RT_HIP(hipSetDevice(m->device));
        RT_HIP(hipStreamSynchronize(m->stream));
        if (m->group.rank == 0) continue;
        const SceneHeader& h = hdr[i];
        for (int k = 0; k <= kNumKinds; ++k) m->w32.scene.kind_begin[k] = m->w64.scene.kind_begin[k] = h.kind_begin[k];
        m->w32.scene.any_secondary = m->w64.scene.any_secondary = h.any_secondary;
        m->world_slot.assign(h.n_world_slots, 0);
        if (h.n_world_slots)
            RT_HIP(hipMemcpy(m->world_slot.data(), m->w32.world_slot, h.n_world_slots * sizeof(int32_t),
                             hipMemcpyDeviceToHost));
        if ((rc = fetch_jit_tables(m)) || (rc = capture_jit_table(m))) return rc;
        m->flops = FlopScene{};
        m->flops.per_ray = h.flops_per_ray;
        m->flops.n_lights = h.nl + h.area_samples;
        m->bright_hit = h.bright_hit;
        m->bright_w = h.bright_w;
        m->duplicate_shapes = h.duplicates;
        m->tree_info = h.tree_info;
        m->instance_info = h.instance_info;
        m->smooth_info = h.smooth_info;
        m->texture_info = h.texture_info;
        m->light_info = h.light_info;
        m->map_info = h.map_info;
        set_kernel_build(m, h.build);  // (the header's: this rank built nothing)
        m->have_scene = true;
        ++m->scene_gen;
    }
    return RT_OK;
}

int group_render_device(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, void* out_device,
                        hipStream_t stream) {
    int rc = check_group_options(ctx, o);
    if (rc) return rc;
    return render_shards(ctx, cam, o, out_device, stream, false);
}

int group_render(rt_context* ctx, const rt_camera_desc* cam, const rt_render_options* o, void* out_host,
                 rt_stats* stats) {
    int rc = check_group_options(ctx, o);
    if (rc) return rc;
    if (ctx->group.rank == 0 && !out_host) return set_error(RT_ERR_INVALID, "null output on rank 0");
    const std::vector<rt_context*> ms = members(ctx);
    const size_t bytes = (size_t)cam->width * cam->height * pixel_bytes(o);
    if (bytes == 0) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return RT_OK;
    }
    std::vector<std::vector<unsigned long long>> before(ms.size(), std::vector<unsigned long long>(kNumCounters));
    for (size_t i = 0; i < ms.size(); ++i) {
        RT_HIP(hipSetDevice(ms[i]->device));
        if ((rc = read_counters(ms[i], before[i].data()))) return rc;
    }
    if (ctx->group.rank == 0) {
        RT_HIP(hipSetDevice(ctx->device));
        if ((rc = ctx->d_scratch.reserve(bytes))) return rc;
    }
    void* image = ctx->group.rank == 0 ? ctx->d_scratch.get() : nullptr;
    if ((rc = render_shards(ctx, cam, o, image, ctx->stream, true))) return rc;
    if (ctx->group.rank == 0) {  // enqueued behind the de-interleave on rank 0's stream
        RT_HIP(hipSetDevice(ctx->device));
        if ((rc = copy_to_host(ctx, out_host, bytes))) return rc;
    }
    for (rt_context* m : ms) {
        RT_HIP(hipSetDevice(m->device));
        RT_HIP(hipStreamSynchronize(m->stream));
    }
    rt_stats total{};
    float render_ms = 0.f, gather_ms = 0.f, frame_ms = 0.f;
    for (size_t i = 0; i < ms.size(); ++i) {
        rt_context* m = ms[i];
        RT_HIP(hipSetDevice(m->device));
        if ((rc = check_pool_error(m))) return rc;
        unsigned long long after[kNumCounters];
        if ((rc = read_counters(m, after))) return rc;
        float r = 0.f;
        RT_HIP(hipEventElapsedTime(&r, m->group.ev_render0, m->group.ev_render1));
        render_ms = std::max(render_ms, r);
        if (m->group.rank == 0) {
            RT_HIP(hipEventElapsedTime(&gather_ms, m->group.ev_render1, m->group.ev_gather1));
            RT_HIP(hipEventElapsedTime(&frame_ms, m->group.ev_render0, m->group.ev_gather1));
        }
        rt_stats s{};
        fill_stats(m, before[i].data(), after, r, &s);
        add_rays(total, s);
    }
    if (stats) {
        *stats = total;
        stats->kernel_ms = render_ms;
        stats->gather_ms = gather_ms;
        stats->frame_ms = frame_ms;
        stats->n_shards = (uint32_t)ctx->group.n_ranks;
    }
    return RT_OK;
}

int group_read_counters(rt_context* ctx, rt_stats* totals) {
    rt_stats t{};
    int rc;
    for (rt_context* m : members(ctx)) {
        RT_HIP(hipSetDevice(m->device));
        RT_HIP(hipDeviceSynchronize());
        unsigned long long zero[kNumCounters] = {}, now[kNumCounters];
        if ((rc = read_counters(m, now))) return rc;
        rt_stats s{};
        fill_stats(m, zero, now, 0.f, &s);
        add_rays(t, s);
        if ((rc = check_pool_error(m))) return rc;
    }
    t.n_shards = (uint32_t)ctx->group.n_ranks;
    *totals = t;
    return RT_OK;
}

}  // namespace rtc

using namespace rtc;

extern "C" {

int rt_context_create_multi(const int* devices, int n, rt_context** out) {
    if (!devices || !out || n < 1) return set_error(RT_ERR_INVALID, "rt_context_create_multi: bad arguments");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return set_error(RT_ERR_NO_DEVICE, "no HIP device available (the render path has no CPU fallback)");
    for (int i = 0; i < n; ++i) {
        if (devices[i] < 0 || devices[i] >= count) return set_error(RT_ERR_INVALID, "device ordinal out of range");
        for (int j = 0; j < i; ++j)
            if (devices[j] == devices[i]) return set_error(RT_ERR_INVALID, "a device appears twice");
    }
    std::vector<std::unique_ptr<rt_context>> ms(n);
    for (int i = 0; i < n; ++i) {
        rt_context* m = nullptr;
        if (int rc = create_device_context(devices[i], &m)) return rc;
        ms[i].reset(m);
    }
    std::vector<ncclComm_t> comms(n, nullptr);
    if (ncclResult_t r = ncclCommInitAll(comms.data(), n, devices); r != ncclSuccess)
        return set_error(RT_ERR_COMM, std::string("ncclCommInitAll: ") + ncclGetErrorString(r));
    for (int i = 0; i < n; ++i) ms[i]->group.comm = comms[i];  // owned before any step can fail
    for (int i = 0; i < n; ++i)
        if (int rc = init_member(ms[i].get(), comms[i], n, i)) return rc;
    for (int i = 1; i < n; ++i) ms[0]->group.peers.push_back(ms[i].release());
    *out = ms[0].release();
    return RT_OK;
}

int rt_comm_unique_id(uint8_t id[RT_UNIQUE_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == RT_UNIQUE_ID_BYTES, "RT_UNIQUE_ID_BYTES must match ncclUniqueId");
    if (!id) return set_error(RT_ERR_INVALID, "null id");
    ncclUniqueId u;
    if (ncclResult_t r = ncclGetUniqueId(&u); r != ncclSuccess)
        return set_error(RT_ERR_COMM, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    std::memcpy(id, &u, sizeof(u));
    return RT_OK;
}

int rt_context_create_rank(int device, int n_ranks, int rank, const uint8_t id[RT_UNIQUE_ID_BYTES],
                           rt_context** out) {
    if (!id || !out || n_ranks < 1 || rank < 0 || rank >= n_ranks)
        return set_error(RT_ERR_INVALID, "rt_context_create_rank: bad arguments");
    *out = nullptr;
    rt_context* created = nullptr;
    if (int rc = create_device_context(device, &created)) return rc;
    std::unique_ptr<rt_context> m(created);
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    ncclComm_t comm = nullptr;
    (void)hipSetDevice(device);
    if (ncclResult_t r = ncclCommInitRank(&comm, n_ranks, u, rank); r != ncclSuccess)
        return set_error(RT_ERR_COMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    if (int rc = init_member(m.get(), comm, n_ranks, rank)) return rc;
    *out = m.release();
    return RT_OK;
}

int rt_context_set_gather(rt_context* ctx, int mode) {
    if (!ctx || (mode != RT_GATHER_RCCL && mode != RT_GATHER_PEER)) return set_error(RT_ERR_INVALID, "bad arguments");
    for (rt_context* m : members(ctx)) m->group.gather_mode = mode;
    return RT_OK;
}

int rt_context_group(rt_context* ctx, int* n_ranks, int* rank, int* local_devices) {
    if (!ctx) return set_error(RT_ERR_INVALID, "null context");
    if (n_ranks) *n_ranks = ctx->group.n_ranks;
    if (rank) *rank = ctx->group.rank;
    if (local_devices) *local_devices = 1 + (int)ctx->group.peers.size();
    return RT_OK;
}

}  // extern "C"
