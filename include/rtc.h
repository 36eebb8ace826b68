/*
 * rtc.h — C-ABI of the MI355X-native render path for the Ray Tracer Challenge
 * world model of przemo199/ray-tracer-challenge-rs.
 *
 * This is the drop-in boundary.  It replaces, for one
 * frame, the reference's
 *     Camera::render           ray-tracer/src/composites/camera.rs:79-95
 *     Camera::render_parallel  ray-tracer/src/composites/camera.rs:97-112
 * and, per ray,
 *     World::color_at          ray-tracer/src/composites/world.rs:89-95
 * with a HIP wavefront tracer for gfx950.  The reference's only caller of the
 * render loop is ray-tracer-cli/src/main.rs:18-21; a GPU variant is a third
 * RenderingMode arm there (ray-tracer-cli/src/cli/rendering_mode.rs:3-7).
 *
 * Conventions (mirroring the reference's ownership rules):
 *   - every input is a plain POD array in f64, i.e. exactly the values the
 *     reference holds on the host (Matrix<4> is [[f64;4];4] row-major,
 *     primitives/matrix.rs:8);
 *   - the caller owns every host buffer; the library owns device buffers
 *     except the explicit *_device entry points, which write into a
 *     caller-owned device buffer on a caller-supplied HIP stream;
 *   - return 0 (RT_OK) on success, a negative rt_status on failure;
 *     rt_last_error() gives a thread-local message.  The reference panics
 *     instead (release profile panic=abort, Cargo.toml:16); a host wrapper
 *     mirroring it turns a negative status into a panic/exception;
 *   - one context drives one GPU and is used from one host thread at a time;
 *     its launches are ordered: rt_render / rt_color_at run on the context's
 *     own stream, rt_render_device on the caller's, and a launch on another
 *     stream than the previous launch's waits for everything submitted to
 *     that stream so far.  A stream handed to rt_render_device must stay
 *     valid until the context's next launch on a different stream (or
 *     rt_context_destroy);
 *   - there is NO CPU fallback: without a usable HIP device every entry
 *     point that computes returns RT_ERR_NO_DEVICE.
 */
#ifndef RTC_H
#define RTC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 3

/* Image tile rendered by one workgroup (one wave = one 64-pixel row run, so
 * output stores are contiguous); RT_TILE_H rows are also the row-block unit
 * of shards. */
#define RT_TILE_W 64
#define RT_TILE_H 4

/* World::MAX_REFLECTION_ITERATIONS, ray-tracer/src/composites/world.rs:15 */
#define RT_DEFAULT_MAX_DEPTH 6
/* largest recursion depth the device ray pool is sized for */
#define RT_MAX_SUPPORTED_DEPTH 16

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = -1,      /* bad argument / malformed descriptor       */
    RT_ERR_HIP = -2,          /* a HIP runtime call failed                 */
    RT_ERR_NO_DEVICE = -3,    /* no HIP device / extension not usable      */
    RT_ERR_NO_SCENE = -4,     /* render before rt_scene_upload             */
    RT_ERR_OOM = -5,          /* device allocation failed                  */
    RT_ERR_POOL = -6,         /* device ray pool overflow (never expected) */
    RT_ERR_IO = -7,           /* file / parse error (scene loader)         */
    RT_ERR_COMM = -8          /* RCCL (multi-GPU) call failed              */
} rt_status;

/* Shape kinds: ray-tracer/src/shapes.rs:1-17 */
typedef enum rt_shape_kind {
    RT_SHAPE_SPHERE = 0,   /* shapes/sphere.rs   */
    RT_SHAPE_PLANE = 1,    /* shapes/plane.rs    */
    RT_SHAPE_CUBE = 2,     /* shapes/cube.rs     */
    RT_SHAPE_CYLINDER = 3, /* shapes/cylinder.rs */
    RT_SHAPE_CONE = 4,     /* shapes/cone.rs     */
    RT_SHAPE_TRIANGLE = 5  /* shapes/triangle.rs */
} rt_shape_kind;

/* Pattern kinds: ray-tracer/src/patterns.rs:1-14 (+ test-only TestPattern,
 * patterns/pattern.rs:29-66, which the reference's own world tests use). */
typedef enum rt_pattern_kind {
    RT_PATTERN_STRIPE = 0,   /* patterns/stripe_pattern.rs   */
    RT_PATTERN_GRADIENT = 1, /* patterns/gradient_pattern.rs */
    RT_PATTERN_RING = 2,     /* patterns/ring_pattern.rs     */
    RT_PATTERN_CHECKER = 3,  /* patterns/checker_pattern.rs  */
    RT_PATTERN_COMPLEX = 4,  /* patterns/complex_pattern.rs  */
    RT_PATTERN_TEST = 5,     /* patterns/pattern.rs:29-66    */
    RT_PATTERN_IMAGE = 6     /* an image texture (rt_scene_upload_textured only; no reference) */
} rt_pattern_kind;

typedef enum rt_precision {
    RT_PRECISION_F32 = 0, /* the throughput path (north star: f32)          */
    RT_PRECISION_F64 = 1  /* parity path: same op order / FMA sites as ref  */
} rt_precision;

typedef enum rt_out_format {
    RT_OUT_REAL = 0, /* f32 RGB (precision f32) or f64 RGB (precision f64)  */
    RT_OUT_U8 = 1    /* u8 RGB, round(clamp(c,0,1)*255): canvas.rs:117-123  */
} rt_out_format;

/* One entry of World.shapes (world.rs:9-12).  The shape's inverse transform
 * is what Transform::transformation_inverse() returns (shapes/shape.rs:6-14);
 * the library never inverts, so host and device see the same f64 inverse. */
typedef struct rt_shape_desc {
    int32_t kind;        /* rt_shape_kind                                  */
    int32_t material;    /* index into the material table                  */
    double inverse[16];  /* row-major Matrix<4>                            */
    double minimum;      /* cylinder/cone `min` (cylinder.rs:12, cone.rs:12) */
    double maximum;      /* cylinder/cone `max`                            */
    int32_t closed;      /* cylinder/cone `closed`                         */
    int32_t reserved;
    double vertex_1[3];  /* triangle.rs:12-17 */
    double edge_1[3];
    double edge_2[3];
    double normal[3];
} rt_shape_desc;

/* composites/material.rs:9-20 */
typedef struct rt_material_desc {
    double color[3];
    double ambient;
    double diffuse;
    double specular;
    double shininess;
    double reflectiveness;
    double transparency;
    double refractive_index;
    int32_t casts_shadow;
    int32_t pattern; /* index into the pattern table, -1 = None */
} rt_material_desc;

/* One Arc<dyn Pattern> (patterns/pattern.rs:6-15). */
typedef struct rt_pattern_desc {
    int32_t kind;       /* rt_pattern_kind                                 */
    int32_t sub_a;      /* ComplexPattern pattern_a (index), else -1       */
    int32_t sub_b;      /* ComplexPattern pattern_b (index), else -1       */
    int32_t reserved;
    double color_a[3];
    double color_b[3];
    double inverse[16]; /* pattern transformation_inverse, row-major       */
} rt_pattern_desc;

/* primitives/light.rs:6-10 */
typedef struct rt_light_desc {
    double position[3];
    double intensity[3];
} rt_light_desc;

/* The private state of Camera (camera.rs:10-19) after Camera::new
 * (camera.rs:25-49) and set_transformation (camera.rs:124-127). */
typedef struct rt_camera_desc {
    uint32_t width;
    uint32_t height;
    double field_of_view;
    double half_width;
    double half_height;
    double pixel_size;
    double inverse[16]; /* camera transformation_inverse, row-major */
    double origin[3];   /* inverse * Point::ORIGIN (camera.rs:114-116)  */
} rt_camera_desc;

/* Diagnostic ablation flags (profiling only; outputs are wrong with them). */
#define RT_FLAG_NO_COUNTERS 1u /* skip the per-workgroup counter flush      */
#define RT_FLAG_NO_SHADE 2u    /* closest hit only, colour = normalised t   */
#define RT_FLAG_NO_TRACE 4u    /* camera ray only, colour = direction       */
#define RT_FLAG_STAMPS 8u      /* record per-workgroup start/end timestamps */
#define RT_FLAG_FAIL_LAUNCH 16u /* fail with RT_ERR_HIP after planning, before
                                  * the enqueue (tests the error path)      */
#define RT_FLAG_GENERATIONS 32u /* also count rays per generation (generic
                                  * kernels; rt_read_generation_counts).
                                  * Pixels and rt_stats are unchanged.      */
#define RT_FLAG_NO_SKIPS 64u    /* trace without the skips: the shadow ray's
                                  * (light behind the surface, plane side,
                                  * cube faces, blocked clusters), the cube
                                  * exit path, planes behind every ray of a
                                  * wave and the containers walk's hit-point
                                  * cull: acceleration only, so pixels and
                                  * rt_stats are unchanged (exactness tests;
                                  * per-scene kernels get a build of their
                                  * own)                                    */

typedef struct rt_render_options {
    uint32_t max_depth;    /* `remaining` of the primary ray; 6 = reference */
    uint32_t precision;    /* rt_precision                                  */
    uint32_t out_format;   /* rt_out_format                                 */
    uint32_t shard_index;  /* row-block sharding            */
    uint32_t shard_count;  /* 1 = the whole image                           */
    uint32_t flags;        /* 0; RT_FLAG_* diagnostic ablations (never in  */
                           /* a parity or benchmark result)                */
} rt_render_options;

/* Ray counts in the reference's semantics plus the terms of
 * the algorithmic-FLOP convention. */
typedef struct rt_stats {
    uint64_t primary;        /* camera rays (or rays handed to rt_color_at) */
    uint64_t shadow;         /* L per shaded hit (world.rs:46-52)           */
    uint64_t reflect;        /* spawned reflection rays (world.rs:114-128)  */
    uint64_t refract;        /* spawned refraction rays (world.rs:130-157)  */
    uint64_t shaded;         /* shaded hits (prepare_computations calls)    */
    uint64_t lit_patterned;  /* light evaluations on a patterned material   */
    uint64_t refract_evals;  /* refracted_color past the opaque/depth check */
    uint64_t schlick_evals;  /* schlicks_approximation calls                */
    double kernel_ms;        /* device time of the render launch (multi-GPU: */
                             /* the slowest shard's)                         */
    double algorithmic_flops;/* SURVEY.md §8d convention                    */
    double gather_ms;        /* multi-GPU: RCCL gather of the strips + the   */
                             /* de-interleave on rank 0 (0 on one GPU)       */
    double frame_ms;         /* device time of the whole frame               */
    uint32_t n_shards;       /* GPUs the frame was split over                */
    uint32_t reserved;
} rt_stats;

typedef struct rt_context rt_context;

int rt_abi_version(void);
const char* rt_last_error(void);
int rt_device_count(int* count);

int rt_context_create(int device_ordinal, rt_context** out);
int rt_context_destroy(rt_context* ctx);

/* Multi-GPU contexts (the north star's "image optionally
 * tiled across 8 GPUs of one node via RCCL broadcast of the scene + gather of
 * framebuffer strips over xGMI").  A group context splits every frame into
 * one shard per GPU (cyclic RT_TILE_H-row blocks, rt_shard_rows), gathers the
 * strips onto rank 0 with RCCL and de-interleaves them there;
 * rt_scene_upload flattens the world on rank 0 and RCCL-broadcasts the device
 * tables to every GPU.  The entry points keep their single-GPU meaning:
 * rt_render / rt_render_device deliver the WHOLE image on rank 0 (so
 * options.shard_index/shard_count must be 0/1), rt_color_at runs on rank 0.
 *  - one process driving several GPUs: rt_context_create_multi
 *    (ncclCommInitAll over `devices`);
 *  - one process per GPU: rank 0 makes an id with rt_comm_unique_id, the
 *    caller shares it (any channel), and every rank calls
 *    rt_context_create_rank (ncclCommInitRank).  Every rank then makes the
 *    same calls with the same camera and options (collective semantics);
 *    only rank 0's scene tables and output buffer are used — other ranks may
 *    pass NULL tables with zero counts and a NULL output.  Counters and stats
 *    are the calling process's own shards. */
#define RT_UNIQUE_ID_BYTES 128
int rt_context_create_multi(const int* devices, int n_devices, rt_context** out);
int rt_comm_unique_id(uint8_t id[RT_UNIQUE_ID_BYTES]);
int rt_context_create_rank(int device, int n_ranks, int rank, const uint8_t id[RT_UNIQUE_ID_BYTES],
                           rt_context** out);
/* Shards per frame, this context's rank, and the GPUs this process drives. */
int rt_context_group(rt_context* ctx, int* n_ranks, int* rank, int* local_devices);

/* Flatten + upload a world.  Replaces the World value that Camera::render
 * borrows (camera.rs:79).  Tables are copied; the caller may free them. */
int rt_scene_upload(rt_context* ctx,
                    const rt_shape_desc* shapes, uint32_t n_shapes,
                    const rt_material_desc* materials, uint32_t n_materials,
                    const rt_pattern_desc* patterns, uint32_t n_patterns,
                    const rt_light_desc* lights, uint32_t n_lights);

/* Rows of the strip one shard writes (RT_TILE_H-row blocks, cyclic: tile
 * row k of the image belongs to shard k % shard_count).  Every strip is
 * padded to this height (shard 0's), so gathers use equal counts. */
int rt_shard_rows(uint32_t height, uint32_t shard_count, uint32_t* rows);
/* For each image row y < height: the shard that renders it and its row in
 * that shard's strip (the map rt_assemble_shards inverts).  Host only. */
int rt_shard_row_map(uint32_t height, uint32_t shard_count, uint32_t* shard_of_row, uint32_t* strip_row_of_row);

/* Synchronous render into a caller-owned HOST buffer: Camera::render /
 * render_parallel semantics (camera.rs:79-112).  Output is row-major, y = 0
 * on top (canvas.rs:53-55); 3 channels per pixel of f32/f64/u8. With
 * shard_count > 1 the buffer holds this shard's strip (rt_shard_rows rows). */
int rt_render(rt_context* ctx, const rt_camera_desc* camera,
              const rt_render_options* options, void* out_host,
              rt_stats* stats);

/* Asynchronous render into a caller-owned DEVICE buffer on `hip_stream`
 * (a hipStream_t; NULL = HIP's default stream).  No host sync.  The caller's
 * HIP runtime must be the one librtc is bound to (one runtime per process). */
int rt_render_device(rt_context* ctx, const rt_camera_desc* camera,
                     const rt_render_options* options, void* out_device,
                     void* hip_stream);

/* Batch World::color_at (world.rs:89-95): rays[i] = {ox,oy,oz,dx,dy,dz},
 * out[i] = RGB, both f64 host arrays; `max_depth` = remaining.  In a world
 * with reflective or transparent materials (max_depth > 0) every direction
 * must be unit length within 1e-6, as the camera's are (camera.rs:66), or
 * RT_ERR_INVALID: the ray trees' fixed-point pixel sums are bounded for unit
 * directions, and with eye = -d the specular term grows as |d|^shininess. */
int rt_color_at(rt_context* ctx, const double* rays, uint64_t n_rays,
                uint32_t max_depth, uint32_t precision, double* out_rgb,
                rt_stats* stats);

/* Ray batches: World::color_at (world.rs:89-95) for ANY ray in ANY uploaded
 * world.  rays[i] = {ox,oy,oz,dx,dy,dz}, rgb[i] = its colour.  Each ray's
 * tree is walked by one GPU lane that sums its contributions in a fixed order
 * (refraction subtree before reflection subtree), so there is no unit-length
 * rule for directions and no brightness bound on the world (rt_color_at and
 * rt_render* keep theirs), and results are bit-reproducible.  A zero or
 * non-finite direction yields whatever the reference's arithmetic yields.
 *   options.max_depth  `remaining` of the rays (<= RT_MAX_SUPPORTED_DEPTH);
 *   options.precision  rt_precision: the element type of the device buffers;
 *   options.flags      0, or RT_FLAG_NO_COUNTERS | RT_FLAG_NO_SKIPS |
 *                      RT_FLAG_GENERATIONS | RT_FLAG_FAIL_LAUNCH;
 *   options.reserved   0.
 * Hits (optional): per ray, t of the PRIMARY ray's closest hit and the hit
 * shape's index in the uploaded shape table; a miss is shape = -1 (t = +inf).
 * At most 2^31 rays per call; n_rays = 0 is RT_OK.  Group contexts run the
 * batch on rank 0. */
typedef struct rt_ray_options {
    uint32_t max_depth;
    uint32_t precision;
    uint32_t flags;
    uint32_t reserved;
} rt_ray_options;
typedef struct rt_ray_hit_f32 {
    float t;
    int32_t shape;
} rt_ray_hit_f32;
typedef struct rt_ray_hit_f64 {
    double t;
    int32_t shape;
    int32_t reserved;
} rt_ray_hit_f64;

/* Asynchronous, on `hip_stream` (NULL = HIP's default stream), no host sync,
 * stream-ordered with the context's other launches as rt_render_device is.
 * Caller-owned DEVICE buffers in the precision's own type: n_rays x 6 f32/f64
 * in, n_rays x 3 out, and n_rays x rt_ray_hit_f32/_f64 (8/16-byte aligned) or
 * NULL.  Counters accumulate into rt_read_counters; a device error is
 * reported by the context's next synchronous call. */
int rt_trace_rays_device(rt_context* ctx, const void* rays_device, uint64_t n_rays,
                         const rt_ray_options* options, void* out_rgb_device,
                         void* out_hit_device, void* hip_stream);
/* Synchronous host convenience, like rt_color_at: f64 host arrays in and out
 * for either precision (f32 rounds the rays once on the host and widens the
 * results), out_hit = n_rays x rt_ray_hit_f64 or NULL, plus stats. */
int rt_trace_rays(rt_context* ctx, const double* rays, uint64_t n_rays,
                  const rt_ray_options* options, double* out_rgb, void* out_hit,
                  rt_stats* stats);

/* Supersampled frames: `grid` x `grid` samples per pixel, averaged in the
 * frame kernel.  `camera` is the OUTPUT camera (W x H); the buffer is W x H x
 * 3 in options.out_format (a shard's strip when shard_count > 1), exactly as
 * for rt_render*.  The samples are the pixels of the sample camera Cn =
 * rt_camera_resize(camera, grid W, grid H): sample (i, j) of pixel (x, y) is
 * Cn's ray_for_pixel(grid x + i, grid y + j) (camera.rs:52-68), traced by
 * World::color_at at max_depth, and the pixel is the mean of its grid^2
 * sample colours; u8 output is quantized once, after the mean.  rt_stats
 * counts what a frame of Cn counts (primary = grid^2 W H).  grid = 1 is
 * rt_render* itself: the same bytes and counters.
 * RT_ERR_INVALID for a grid outside 1..RT_MAX_SAMPLE_GRID, for grid W or
 * grid H beyond uint32_t, for flags other than RT_FLAG_NO_SKIPS |
 * RT_FLAG_NO_COUNTERS | RT_FLAG_FAIL_LAUNCH, for a world rt_render* refuses
 * (the samples' weights sum to 1, so the brightness bound is the same) and
 * for a group context of more than one rank (shard the frame yourself with
 * shard_index / shard_count).  Stream order as for rt_render_device. */
#define RT_MAX_SAMPLE_GRID 4
int rt_render_supersampled(rt_context* ctx, const rt_camera_desc* camera,
                           const rt_render_options* options, uint32_t grid,
                           void* out_host, rt_stats* stats);
int rt_render_supersampled_device(rt_context* ctx, const rt_camera_desc* camera,
                                  const rt_render_options* options, uint32_t grid,
                                  void* out_device, void* hip_stream);

/* Diagnostics: the per-workgroup {start, end} s_memrealtime stamps (100 MHz)
 * of the last launch made with RT_FLAG_STAMPS; *n = number of workgroups. */
int rt_debug_stamps(rt_context* ctx, uint64_t* out, uint32_t max_workgroups, uint32_t* n);

/* Diagnostics: per-tile durations (10 ns ticks) the last pool launch
 * recorded for heaviest-first ordering; *n = entries available (tiles of
 * the largest pool launch so far, 0 before any). */
int rt_debug_tile_costs(rt_context* ctx, uint32_t* out, uint32_t max_tiles, uint32_t* n);

/* Diagnostics: the work items of the last pool launch made with
 * RT_FLAG_STAMPS, in the order they were taken: 3 x u64 per item {item |
 * workgroup << 32, start, end} (s_memrealtime, 100 MHz; item encoding in
 * rtc_internal.hpp); *n = number of items logged. */
int rt_debug_item_log(rt_context* ctx, uint64_t* out, uint32_t max_items, uint32_t* n);

/* Known-answer harness: the device's own per-shape code for the shape at
 * world index `shape` of the uploaded world, on caller-given inputs (the
 * reference's per-shape unit tests, e.g. cone.rs:191-252, run on the GPU).
 * rt_debug_intersect: rays[i] = {ox,oy,oz,dx,dy,dz}; world_space = 0 treats
 * them as local rays (Intersect::local_intersect), 1 transforms them by the
 * shape's inverse first (Ray::intersect, ray.rs:45-49).  out[i*5] = entries
 * the reference pushes (<= RT_DEBUG_MAX_ENTRIES), out[i*5+1..] their t in push
 * order.  rt_debug_normal: points[i] = {x,y,z}; world_space = 0 gives
 * local_normal_at (not normalized), 1 gives normal_at (shape.rs:22-27);
 * out[i*3..] = the normal.  Synchronous; host buffers. */
#define RT_DEBUG_MAX_ENTRIES 4
int rt_debug_intersect(rt_context* ctx, uint32_t shape, const double* rays, uint64_t n_rays, uint32_t precision,
                       uint32_t world_space, double* out);
int rt_debug_normal(rt_context* ctx, uint32_t shape, const double* points, uint64_t n_points, uint32_t precision,
                    uint32_t world_space, double* out);

/* Per-scene kernels.  For f32 frames the library compiles (hipRTC), once
 * per uploaded world, the same tracer source with the world's shape table as
 * compile-time constants, and runs it instead of the generic kernel (same
 * pixels, bit for bit).  Modes (rt_context_set_jit; env RTC_JIT=0|1|2|3 at
 * context creation):
 *   RT_JIT_OFF    never;
 *   RT_JIT_SYNC   every f32 frame, the build compiled in line on the first
 *                 one (deterministic: tests);
 *   RT_JIT_AUTO   the default.  Frames of at least 64K pixels; the build runs
 *                 on a host thread, started by the SECOND such frame of an
 *                 uploaded world, and frames render with the generic kernel
 *                 until it is ready.  A one-shot render (Camera::render, the
 *                 CLI) never compiles; repeated renders switch once the
 *                 build lands.  A build already made in this process (or on
 *                 disk) for the same world is used from the first frame;
 *   RT_JIT_EAGER  as AUTO, but the first large frame starts the build.
 * rt_jit_status: whether the last launch ran a per-scene kernel, the compile
 * (or cache-load) milliseconds of the builds this context started, and the
 * last build error (a failed build keeps the generic kernel for that world).
 * rt_jit_wait: block until this context's builds in flight have finished
 * (at most timeout_ms; < 0 = no limit); *pending = builds still running.
 * A context destroyed with a build in flight does not wait for it: the
 * compile runs in a child process (rtc_jitc) and a DETACHED thread of this
 * process waits for it, runs librtc code when it ends, and is never joined.
 * So librtc must not be unloaded (dlclose) while rt_jit_wait reports pending
 * builds; process exit is safe (the orphaned compiler still finishes and
 * fills the disk cache).  Builds are also cached on
 * disk across processes: env RTC_JIT_CACHE = a directory, or 0 for none
 * (default $XDG_CACHE_HOME/rtc_jit, else ~/.cache/rtc_jit). */
enum { RT_JIT_OFF = 0, RT_JIT_SYNC = 1, RT_JIT_AUTO = 2, RT_JIT_EAGER = 3 };
int rt_context_set_jit(rt_context* ctx, int mode);

/* A planning hint: the caller keeps `frames` frames in flight (consecutive
 * frames alternating between that many contexts, each on a stream of its
 * own, so one frame's launch tail overlaps the next frame's start;
 * INTEGRATION.md §2).  1 (the default) plans each launch for its own
 * latency; > 1 plans the f32 direct kernel's grid for throughput (1.5x the
 * resident workgroups instead of 2.5x: round 6, three_sphere 1080p with two
 * in flight 339 -> 355-361 Gray/s, one frame alone 15.5 -> 16.1 us) and
 * splits the pool kernels' heavy tiles only above 1.5x the mean workgroup
 * load instead of 1x (a 4K shard of 8 with two in flight: cover 0.104 ->
 * 0.094 ms).  Pixels and rt_stats are unchanged.  Applies to every member of
 * a group. */
int rt_context_set_frames_in_flight(rt_context* ctx, uint32_t frames);
int rt_jit_status(rt_context* ctx, int* used_last_launch, double* compile_ms, char* log, size_t log_len);
int rt_jit_wait(rt_context* ctx, double timeout_ms, int* pending);

/* The triangle hierarchy of the uploaded world.  A world
 * of more than 255 shapes with at least 64 bounded triangles (a mesh:
 * rtc_scene.h rt_mesh_*) gets a tree of bounding balls over its triangle
 * records at rt_scene_upload, and the generic kernels pass by every subtree
 * whose ball no ray of a wave can meet;
 * pixels and rt_stats are those of the flat loop over every triangle.  Such a
 * world runs the generic kernels only (rt_jit_status says so in its log).
 * rt_scene_tree_info reports the tree: all zeros when the world has none (too
 * few triangles, a world small enough for the per-scene builds' records,
 * RTC_DEBUG=tri_tree=0 or RTC_DEBUG=cull=0 at upload).  On a
 * group context: this process's first member, whose tables came from rank 0. */
typedef struct rt_tree_info {
    uint32_t nodes;            /* inner nodes and leaves */
    uint32_t leaves;
    uint32_t depth;            /* nodes on the longest root-to-leaf path */
    uint32_t records_in_tree;  /* triangle records reached through the leaves */
    uint32_t records_outside;  /* triangle records tested for every wave (unbounded ones) */
    uint32_t reserved;
    double build_ms;           /* host time of the tree build at upload */
} rt_tree_info;
int rt_scene_tree_info(rt_context* ctx, rt_tree_info* out);

/* Mesh instances: one mesh, many placements.  An instanced
 * world is three lists: the plain shapes, meshes (local-space triangles with
 * the identity inverse, as rt_mesh_triangles(mesh, NULL, 0, any) writes them;
 * their `material` is ignored) and instances (mesh, inverse, material).  It
 * MEANS the flat world
 *     shapes ++ E(0) ++ E(1) ++ ...
 * where E(k) is mesh instances[k].mesh's triangles in mesh order, each with
 * inverse = instances[k].inverse and material = instances[k].material: what
 * rt_mesh_triangles(mesh, transform, 0, material) writes when inverse =
 * rt_matrix_inverse(transform).  rt_instances_expand writes that list (host
 * only; `out` holds n_shapes + the sum of the instances' triangle counts).
 * World indices are the expansion's (triangle j of instance k: n_shapes +
 * the triangle counts of instances 0..k-1 + j): tie rule, rt_ray_hit_*::shape.
 * Every entry point returns for an instanced upload what it returns for the
 * expansion uploaded with rt_scene_upload, bytes and rt_stats, while the
 * device holds each mesh's records and bounding-ball hierarchy once and one
 * small record per instance.  An instance with a triangle value-equal to
 * another of the world (shape_identity: equal inverse, material and geometry;
 * in itself, in another instance or among the plain shapes) is uploaded as
 * plain records, and rt_instance_info counts it in `expanded`.  A world with
 * an instance not expanded runs the generic kernels only (rt_jit_status says
 * so); n_instances = 0 is rt_scene_upload itself.
 * RT_ERR_INVALID, each with its own rt_last_error text: a mesh record that is
 * no triangle or whose inverse is not the identity, an empty mesh, a mesh or
 * material index out of range, an expansion of 2^24 shapes or more. */
typedef struct rt_mesh_desc {
    const rt_shape_desc* triangles;
    uint32_t n_triangles;
    uint32_t reserved;
} rt_mesh_desc;
typedef struct rt_instance_desc {
    uint32_t mesh;       /* index into the mesh list     */
    int32_t material;    /* index into the material table */
    double inverse[16];  /* row-major Matrix<4>: the inverse of the placement */
} rt_instance_desc;
int rt_scene_upload_instanced(rt_context* ctx,
                              const rt_shape_desc* shapes, uint32_t n_shapes,
                              const rt_mesh_desc* meshes, uint32_t n_meshes,
                              const rt_instance_desc* instances, uint32_t n_instances,
                              const rt_material_desc* materials, uint32_t n_materials,
                              const rt_pattern_desc* patterns, uint32_t n_patterns,
                              const rt_light_desc* lights, uint32_t n_lights);
int rt_instances_expand(const rt_shape_desc* shapes, uint32_t n_shapes,
                        const rt_mesh_desc* meshes, uint32_t n_meshes,
                        const rt_instance_desc* instances, uint32_t n_instances,
                        rt_shape_desc* out);
/* What the last upload holds of meshes and instances (zeros after
 * rt_scene_upload).  Bytes are device bytes of both precisions' tables. */
typedef struct rt_instance_info {
    uint32_t meshes;
    uint32_t instances;
    uint32_t expanded;          /* instances uploaded as plain records (value-equal partners) */
    uint32_t top_depth;         /* depth of the hierarchy over the instances; 0: a flat loop */
    uint32_t local_records;     /* local triangle records per precision (not expanded meshes') */
    uint32_t local_nodes;       /* nodes of the meshes' hierarchies per precision */
    uint64_t instanced_bytes;   /* local records, nodes, instance records and index tables */
    uint64_t expansion_bytes;   /* records and nodes the not expanded instances' triangles would take as plain shapes */
    double build_ms;            /* host time of the mesh builds and the identity decisions */
} rt_instance_info;
int rt_scene_instance_info(rt_context* ctx, rt_instance_info* out);

/* Smooth triangles (the book's chapter 15): a Triangle plus
 * three vertex normals n1, n2, n3 that belong to p1, p2, p3 in the face's own
 * vertex order, used as given (never normalized on upload).  Intersection is
 * Triangle::local_intersect (triangle.rs:39-56) itself, same t and same
 * decisions; the local normal at a hit is
 *     n2 * u + n3 * v + n1 * (1 - u - v)
 * per component, left to right with plain multiplies and adds, u and v the two
 * barycentric values that test computed; it goes through Shape::normal_at's
 * tail (shape.rs:22-27, normalize(inverse^T * ln)) and everything downstream
 * (the flip by n . eye < 0, reflectv, over_point / under_point, Schlick,
 * refraction) uses that normal.  The pattern-space point, casts_shadow, the
 * bounding ball, the hierarchy and every geometric cull are the flat
 * triangle's.  Value identity (the containers walk): two smooth triangles are
 * equal iff their flat parts and all nine normal components are (== on
 * doubles); a smooth and a flat triangle never are.
 * The normals travel in a sparse side list next to rt_scene_upload_instanced's
 * lists: entry {list, index} names triangle `index` of the plain shapes
 * (list = RT_SMOOTH_SHAPES) or of mesh `list`.  An instanced mesh's smooth
 * triangles keep their local normals under every placement: the expansion of
 * instance k gives triangle j the same three normals with the instance's
 * inverse.  rt_smooth_expand writes the expansion's list (host only): every
 * entry with RT_SMOOTH_SHAPES and the world index of rt_instances_expand's
 * shape, ascending; `out` holds the plain entries plus, per instance, its
 * mesh's entries; *n_out the number written (out may be NULL to count).
 * n_smooth = 0 is rt_scene_upload_instanced itself.  A world with a smooth
 * triangle runs the generic kernels only (rt_jit_status says so in its log),
 * those of the instance build, whatever n_instances is.
 * RT_ERR_INVALID, each with its own rt_last_error text and checked before the
 * context is looked at: a null list with n_smooth > 0, a list index out of
 * range, a triangle index out of range, a named record that is no triangle,
 * the same triangle named twice, a normal component that is not finite. */
#define RT_SMOOTH_SHAPES 0xFFFFFFFFu
typedef struct rt_smooth_desc {   /* 80 bytes */
    uint32_t list;    /* RT_SMOOTH_SHAPES: `index` counts the plain shapes; else an index into the mesh list */
    uint32_t index;   /* the triangle in that list */
    double normal_1[3], normal_2[3], normal_3[3];
} rt_smooth_desc;
int rt_scene_upload_smooth(rt_context* ctx,
                           const rt_shape_desc* shapes, uint32_t n_shapes,
                           const rt_mesh_desc* meshes, uint32_t n_meshes,
                           const rt_instance_desc* instances, uint32_t n_instances,
                           const rt_smooth_desc* smooth, uint32_t n_smooth,
                           const rt_material_desc* materials, uint32_t n_materials,
                           const rt_pattern_desc* patterns, uint32_t n_patterns,
                           const rt_light_desc* lights, uint32_t n_lights);
int rt_smooth_expand(const rt_shape_desc* shapes, uint32_t n_shapes,
                     const rt_mesh_desc* meshes, uint32_t n_meshes,
                     const rt_instance_desc* instances, uint32_t n_instances,
                     const rt_smooth_desc* smooth, uint32_t n_smooth,
                     rt_smooth_desc* out, uint32_t* n_out);
/* The smooth triangles of the last upload (zeros after any other upload):
 * how many the world means (an instance counts its mesh's once per
 * placement), the device bytes of both precisions' normal tables, and whether
 * the last launch ran kernels that hold the smooth code. */
typedef struct rt_smooth_info {
    uint32_t smooth_triangles;
    uint32_t ran_smooth;
    uint64_t normal_bytes;
} rt_smooth_info;
int rt_scene_smooth_info(rt_context* ctx, rt_smooth_info* out);

/* Image textures (the book's bonus chapter "Texture
 * mapping").  The reference has none of it, so this text is the contract.
 *
 * Texture: width x height RGB bytes, row 0 at the top, a host pointer read
 * during the upload only.  Texel (x, y) has colour (R)byte / (R)255 per
 * channel in the kernel's real type R (f64: (double)b / 255.0, an IEEE
 * division).
 *
 * Image pattern: kind RT_PATTERN_IMAGE (6) of rt_pattern_desc, whose layout is
 * untouched: sub_a = index into the upload's texture list, sub_b = -1,
 * reserved = the filter (RT_FILTER_NEAREST 0, RT_FILTER_BILINEAR 1), color_a
 * and color_b ignored, inverse = the pattern transform (planar map only).  It
 * may be a material's pattern, never a sub-pattern of a complex pattern.
 *
 * (u, v) of a hit.  A triangle with texture coordinates t1, t2, t3 (of p1, p2,
 * p3; the rt_uv_desc side list, built like rt_smooth_desc's):
 *     uv = t2 * u_b + t3 * v_b + t1 * (1 - u_b - v_b)
 * per component, left to right, plain multiplies and adds (no fused operation
 * in the f64 path), u_b and v_b the two barycentric values
 * Triangle::local_intersect compared for the accepted hit (the bits the
 * smooth normal uses, from the one triangle test prepare_hit re-runs).  A
 * component outside [0, 1] is wrapped by c - floor(c), one inside is used as
 * is (exactly 1 stays 1).  The pattern's inverse is ignored for such hits, and
 * an instanced mesh's triangles keep their coordinates under every placement.
 * Any other hit (every shape kind, a triangle without coordinates included):
 * the book's planar map of the pattern-space point
 * pp = pattern.inverse * (shape.inverse * over_point), where the other
 * pattern kinds sample: u = pp.x - floor(pp.x), v = pp.z - floor(pp.z).
 *
 * Sampling: x = u * (w - 1), y = (1 - v) * (h - 1) (the book's flip).
 * Nearest: xi = floor(x) + (x - floor(x) >= 0.5 ? 1 : 0), the same for y
 * (round half away from zero, written so both precisions decide alike; not
 * floor(x + 0.5), not round-to-even).  Bilinear: x0 = floor(x),
 * x1 = min(x0 + 1, w - 1), fx = x - x0, the same for y; per channel
 *     (c00 * (1 - fx) + c10 * fx) * (1 - fy) + (c01 * (1 - fx) + c11 * fx) * fy
 * with cXY the texel at (xX, yY), plain operations in that order.
 * The sampled colour replaces the material's colour exactly where a pattern's
 * does, once per hit; t, tie rules, normals, casts_shadow, bounding balls, the
 * tree, the culls and the skips are untouched, and rt_stats.lit_patterned
 * counts an image-patterned hit like any patterned hit.
 *
 * Value identity (the containers walk): two triangles with coordinates are
 * equal iff their other parts and all six coordinate components are (== on
 * doubles); one with and one without never are.  Two image patterns are equal
 * iff their inverse, filter and textures' contents (width, height, bytes) are,
 * whatever the textures' indices.  The brightness bound of an image pattern is
 * its texture's largest channel / 255.
 *
 * rt_scene_upload_textured is rt_scene_upload_smooth's argument list plus the
 * coordinate list and the texture list; with n_uvs = n_textures = 0 it is
 * rt_scene_upload_smooth itself (which, like every older entry point, refuses
 * pattern kind 6 as "unknown kind").  A world with an image pattern or a
 * coordinate entry runs the generic kernels only, those of the texture build
 * (the instance build plus the sampling code; rt_jit_status says so in its log).  rt_uv_expand pairs with
 * rt_instances_expand / rt_smooth_expand (host only; out may be NULL to
 * count).  RT_ERR_INVALID, each with its own rt_last_error text and checked
 * before the context is looked at: a null list with a nonzero count, a list or
 * triangle index out of range, a named record that is no triangle, the same
 * triangle named twice, a coordinate that is not finite; a texture with null
 * pixels, zero width or height, or width * height > 2^28; an image pattern
 * with sub_a out of range, sub_b != -1, a filter other than 0 or 1, or used as
 * a sub-pattern. */
#define RT_FILTER_NEAREST 0
#define RT_FILTER_BILINEAR 1
#define RT_TEXTURE_MAX_TEXELS (1u << 28)
typedef struct rt_texture_desc {
    const uint8_t* rgb;   /* width * height * 3 bytes, row 0 at the top */
    uint32_t width, height;
} rt_texture_desc;
typedef struct rt_uv_desc {   /* 56 bytes */
    uint32_t list;    /* RT_SMOOTH_SHAPES: `index` counts the plain shapes; else an index into the mesh list */
    uint32_t index;   /* the triangle in that list */
    double uv_1[2], uv_2[2], uv_3[2];
} rt_uv_desc;
int rt_scene_upload_textured(rt_context* ctx,
                             const rt_shape_desc* shapes, uint32_t n_shapes,
                             const rt_mesh_desc* meshes, uint32_t n_meshes,
                             const rt_instance_desc* instances, uint32_t n_instances,
                             const rt_smooth_desc* smooth, uint32_t n_smooth,
                             const rt_uv_desc* uvs, uint32_t n_uvs,
                             const rt_texture_desc* textures, uint32_t n_textures,
                             const rt_material_desc* materials, uint32_t n_materials,
                             const rt_pattern_desc* patterns, uint32_t n_patterns,
                             const rt_light_desc* lights, uint32_t n_lights);
int rt_uv_expand(const rt_shape_desc* shapes, uint32_t n_shapes,
                 const rt_mesh_desc* meshes, uint32_t n_meshes,
                 const rt_instance_desc* instances, uint32_t n_instances,
                 const rt_uv_desc* uvs, uint32_t n_uvs,
                 rt_uv_desc* out, uint32_t* n_out);
/* The textures of the last upload (zeros after any other upload): the
 * triangles with coordinates as the world means them (an instance counts its
 * mesh's once per placement), the texture count, the device bytes of both
 * precisions' coordinate tables and of the texel storage (one packed RGBX
 * dword per texel plus the per-texture table), and whether the last launch ran
 * kernels that hold the texture code. */
typedef struct rt_texture_info {
    uint32_t textured_triangles;
    uint32_t textures;
    uint32_t ran_textured;
    uint32_t reserved;
    uint64_t uv_bytes;
    uint64_t texel_bytes;
} rt_texture_info;
int rt_scene_texture_info(rt_context* ctx, rt_texture_info* out);
/* Reads an image into width * height * 3 RGB bytes (row 0 at the top) that
 * rt_image_free releases.  PPM P3 and P6: comments, any maxval <= 65535
 * (samples scaled to bytes as round(v * 255 / maxval)), lines of any length.
 * PNG (through zlib): 8-bit RGB or RGBA, non-interlaced, all five filter
 * types; alpha is dropped.  Anything else is RT_ERR_IO with its own text.
 * rt_image_read(rt_image_write(x)) == x for both formats.  Host only. */
int rt_image_read(const char* path, uint8_t** rgb, uint32_t* width, uint32_t* height);
void rt_image_free(uint8_t* rgb);

/* Area lights (the book's bonus chapter "Soft shadows").  The
 * reference has none of it, so this text is the contract.
 *
 * An area light is a parallelogram: `corner`, the two full edges and a grid
 * of usteps x vsteps cells, one sample per cell.
 *
 * Sample positions.  uvec = full_uvec / usteps and vvec = full_vvec / vsteps:
 * IEEE divisions per component by the count as a double, done once on the
 * host; the kernels read corner, uvec and vvec rounded once to their real
 * type.  Cell (i, j), i < usteps, j < vsteps, has index k = j * usteps + i and
 * the sample, per component,
 *     pos = (corner + uvec * (i + ju)) + vvec * (j + jv)
 * with plain multiplies and adds, left to right, in the kernel's real type.
 * RT_JITTER_NONE: ju = jv = 0.5 (the cell's centre).
 *
 * Lighting.  An area light MEANS its expansion into N = usteps * vsteps point
 * lights at those positions, each of intensity `intensity` / N, and the
 * world's light list means
 *     lights ++ E(area 0) ++ E(area 1) ++ ...
 * in the idiom of rt_instances_expand.  Per area light and hit the kernels
 * compute eff = base * intensity and ambient = eff * m.ambient once, then
 * sum = the samples' diffuse + specular terms in ascending k, where sample k
 * contributes only where light . normal >= 0 and is_shadowed(over_point,
 * pos_k) is false (calculate_lighting's arithmetic with pos_k for the light's
 * position; its specular only where reflect . eye > 0), and
 *     colour = ambient + sum / N.
 * That is the expansion's colour up to rounding.  It departs from the book on
 * purpose: the book multiplies the mean unshadowed lighting by the visible
 * fraction; weighting each sample by its own shadow test is the Monte-Carlo
 * estimator, and the form an expansion can check.
 *
 * Counters are the expansion's, exactly: rt_stats.shadow counts N per area
 * light per shaded hit, lit_patterned N per area light per patterned hit; the
 * pattern or texture colour is evaluated once per hit, as before.
 *
 * The brightness bound of the fixed-point pixel sums counts an area light as
 * a point light of `intensity`: a world rt_render* refuses with a point light
 * is refused with the equal area light.
 *
 * Hashed jitter (RT_JITTER_HASHED) is precision-independent.  With uint32_t
 * wraparound,
 *     mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *     key = mix(mix(mix(seed ^ ray_id) ^ remaining) ^ ((area_index << 8) | k))
 *     ju  = (key >> 8) * 2^-24
 *     jv  = (mix(key ^ 0x9E3779B9) >> 8) * 2^-24
 * both exact in f32 and f64.  `remaining` is that of the ray being shaded,
 * area_index the light's place in the area list.  ray_id: for frames
 * y * W + x in WHOLE-image coordinates (a shard, a canvas render and every
 * rank of a group produce the whole frame's pixels); for supersampled frames
 * the sample's pixel index in the sample camera Cn, (grid y + j)(grid W) +
 * grid x + i; for rt_color_at and rt_trace_rays* the ray's index in the batch
 * modulo 2^32.  A secondary ray keeps its primary ray's ray_id.  Results stay
 * bit-reproducible.
 *
 * rt_scene_upload_lit is rt_scene_upload_textured's argument list plus the
 * area list; with n_area = 0 it is rt_scene_upload_textured itself.  A world
 * with an area light runs the generic kernels only, those of the area build
 * (the texture build plus the sample loop; rt_jit_status says so in its log),
 * whatever else it holds.  rt_lights_expand writes the expansion's light list
 * (host only; `out` holds n_lights + the sum of the sample counts, *n_out the
 * number written, out may be NULL to count); a hashed light, whose samples
 * depend on the ray, is RT_ERR_INVALID there.  rt_area_light_sample gives the
 * f64 position of one sample for either jitter mode (host only).
 * RT_ERR_INVALID, each with its own rt_last_error text and checked before the
 * context is looked at: a null list with a nonzero count, a step count of 0
 * or above RT_LIGHT_MAX_STEPS, a jitter other than 0 or 1, a component that
 * is not finite.  Zero-length edges are allowed (all samples coincide). */
#define RT_LIGHT_MAX_STEPS 16          /* per axis: at most 256 samples */
#define RT_JITTER_NONE   0             /* cell centres */
#define RT_JITTER_HASHED 1             /* per ray, above */
typedef struct rt_area_light_desc {    /* 112 bytes */
    double corner[3], full_uvec[3], full_vvec[3], intensity[3];
    uint32_t usteps, vsteps, jitter, seed;
} rt_area_light_desc;
int rt_scene_upload_lit(rt_context* ctx,
                        const rt_shape_desc* shapes, uint32_t n_shapes,
                        const rt_mesh_desc* meshes, uint32_t n_meshes,
                        const rt_instance_desc* instances, uint32_t n_instances,
                        const rt_smooth_desc* smooth, uint32_t n_smooth,
                        const rt_uv_desc* uvs, uint32_t n_uvs,
                        const rt_texture_desc* textures, uint32_t n_textures,
                        const rt_material_desc* materials, uint32_t n_materials,
                        const rt_pattern_desc* patterns, uint32_t n_patterns,
                        const rt_light_desc* lights, uint32_t n_lights,
                        const rt_area_light_desc* area, uint32_t n_area);
int rt_lights_expand(const rt_light_desc* lights, uint32_t n_lights,
                     const rt_area_light_desc* area, uint32_t n_area,
                     rt_light_desc* out, uint32_t* n_out);
int rt_area_light_sample(const rt_area_light_desc* desc, uint32_t area_index, uint32_t ray_id,
                         uint32_t remaining, uint32_t k, double pos[3]);
/* The area lights of the last upload (zeros after any other upload): how many,
 * the sum of their sample counts, the device bytes of both precisions'
 * records, and whether the last launch ran kernels that hold the sample loop. */
typedef struct rt_light_info {
    uint32_t area_lights;
    uint32_t samples;
    uint32_t ran_area;
    uint32_t reserved;
    uint64_t area_bytes;
} rt_light_info;
int rt_scene_light_info(rt_context* ctx, rt_light_info* out);

/* Texture maps: how a hit without texture coordinates gets
 * its (u, v).  The book's bonus chapter "Texture mapping" is the source; the
 * reference has no textures, so this text is the contract.
 *
 * For a hit without texture coordinates let pp = pattern.inverse *
 * (shape.inverse * over_point), the point the planar map uses.  All arithmetic
 * is in the kernel's real type R: plain multiplies and adds, left to right,
 * the kernel's divisions (IEEE in f64); pi is rounded once to R; atan2, acos
 * and sqrt are the device math library's for R.  An image pattern has one map:
 *   RT_MAP_PLANAR       u = pp.x - floor(pp.x), v = pp.z - floor(pp.z)
 *                       (rt_scene_upload_textured's behaviour, bit for bit)
 *   RT_MAP_SPHERICAL    theta = atan2(pp.x, pp.z)
 *                       r = sqrt((pp.x^2 + pp.y^2) + pp.z^2)
 *                       c = pp.y / r, clamped into [-1, 1] (a rounded r just
 *                           below |y| would make acos NaN at the poles)
 *                       phi = acos(c)
 *                       u = 1 - (theta / (2 pi) + 0.5),  v = 1 - phi / pi
 *   RT_MAP_CYLINDRICAL  u as in the spherical map,  v = pp.y - floor(pp.y)
 *   RT_MAP_CUBE         six textures, in the book's order: left 0, front 1,
 *                       right 2, back 3, up 4, down 5.  With a = max(|x|, |y|,
 *                       |z|) the face is the first true of a == x: right,
 *                       a == -x: left, a == y: up, a == -y: down, a == z:
 *                       front, else back.  With m(c) = c - 2 floor(c / 2):
 *                           front  u = m(x + 1) / 2   v = m(y + 1) / 2
 *                           back   u = m(1 - x) / 2   v = m(y + 1) / 2
 *                           left   u = m(z + 1) / 2   v = m(y + 1) / 2
 *                           right  u = m(1 - z) / 2   v = m(y + 1) / 2
 *                           up     u = m(x + 1) / 2   v = m(1 - z) / 2
 *                           down   u = m(x + 1) / 2   v = m(z + 1) / 2
 * u = 1 stays 1, as for interpolated coordinates.  Sampling (u, v) under
 * either filter, the clamp of texel indices, lit_patterned, t, ties, normals,
 * culls and skips are rt_scene_upload_textured's.  A hit that has texture
 * coordinates ignores the map and the pattern's inverse and samples the
 * pattern's sub_a texture.  The pattern's inverse serves every map.
 *
 * rt_scene_upload_mapped is rt_scene_upload_lit's argument list plus a sparse
 * list of maps; with n_maps = 0 it is rt_scene_upload_lit itself, and an image
 * pattern that no entry names is planar.  A cube map's pattern keeps a valid
 * sub_a (textured triangles sample it); its faces may repeat.  Two image
 * patterns are equal iff, beyond rt_scene_upload_textured's rule, their maps
 * are equal and, for cube maps, the six faces' contents are equal pairwise; a
 * cube map's brightness bound is the largest channel over its six faces.
 * RT_ERR_INVALID, each with its own rt_last_error text and checked before the
 * context is looked at: a null list with a nonzero count, a pattern index out
 * of range, a named pattern that is not RT_PATTERN_IMAGE, a pattern named
 * twice, an unknown map, a face index out of range for a cube map, a face
 * other than -1 for any other map.  Per-scene builds stay refused. */
#define RT_MAP_PLANAR      0
#define RT_MAP_SPHERICAL   1
#define RT_MAP_CYLINDRICAL 2
#define RT_MAP_CUBE        3
#define RT_FACE_LEFT  0
#define RT_FACE_FRONT 1
#define RT_FACE_RIGHT 2
#define RT_FACE_BACK  3
#define RT_FACE_UP    4
#define RT_FACE_DOWN  5
typedef struct rt_uv_map_desc {   /* 32 bytes */
    uint32_t pattern;   /* index of an RT_PATTERN_IMAGE pattern */
    uint32_t map;       /* RT_MAP_* */
    int32_t  faces[6];  /* RT_MAP_CUBE: texture indices left, front, right, back, up, down; else all -1 */
} rt_uv_map_desc;
int rt_scene_upload_mapped(rt_context* ctx,
                           const rt_shape_desc* shapes, uint32_t n_shapes,
                           const rt_mesh_desc* meshes, uint32_t n_meshes,
                           const rt_instance_desc* instances, uint32_t n_instances,
                           const rt_smooth_desc* smooth, uint32_t n_smooth,
                           const rt_uv_desc* uvs, uint32_t n_uvs,
                           const rt_texture_desc* textures, uint32_t n_textures,
                           const rt_material_desc* materials, uint32_t n_materials,
                           const rt_pattern_desc* patterns, uint32_t n_patterns,
                           const rt_light_desc* lights, uint32_t n_lights,
                           const rt_area_light_desc* area, uint32_t n_area,
                           const rt_uv_map_desc* maps, uint32_t n_maps);
/* The maps of the last upload (zeros after any other upload, and after one
 * whose entries are all RT_MAP_PLANAR): patterns with a map other than the
 * planar one, cube maps among them, and whether the last launch ran kernels
 * that hold the map code. */
typedef struct rt_map_info {
    uint32_t mapped_patterns;
    uint32_t cube_maps;
    uint32_t ran_mapped;
    uint32_t reserved;
} rt_map_info;
int rt_scene_map_info(rt_context* ctx, rt_map_info* out);

/* Thin-lens camera: depth of field.  The reference has no
 * lens, so this text is the contract.
 *
 * rt_render_lens* is rt_render_supersampled* with one change: sample (i, j) of
 * pixel (x, y) is a LENS RAY.  Everything else is that call's: `camera` is the
 * output camera C (W x H), Cn = rt_camera_resize(C, grid W, grid H) the sample
 * camera, grid in 1..RT_MAX_SAMPLE_GRID, the same flags, brightness rule,
 * shards and refusal of groups of more than one rank; rt_stats counts the
 * grid W x grid H ray set (primary = grid^2 W H); every sample weighs
 * 1 / grid^2, summed j outer, i inner (plain sums in the direct kernel, the
 * fixed-point sums in the pool kernel); u8 is quantized once, after the mean.
 *
 * The lens ray.  All arithmetic in the kernel's real type R, plain multiplies
 * and adds, no FMA, in the order written.  With n = grid and Cn's fields:
 *     px = n x + i,  py = n y + j
 *     wx = half_width  - (px + 0.5) * pixel_size
 *     wy = half_height - (py + 0.5) * pixel_size        (camera.rs:52-68)
 * Lens cell (ci, cj) and position (ju, jv) in it:
 *     RT_JITTER_NONE:    ci = i, cj = j, ju = jv = 0.5
 *     RT_JITTER_HASHED, with mix of "Hashed jitter" above and uint32_t wraparound:
 *         lk  = mix(seed ^ 0x4C454E53)
 *         key = mix(lk ^ ray_id),  ray_id = (n y + j)(n W) + n x + i
 *         ju  = (key >> 8) * 2^-24,  jv = (mix(key ^ 0x9E3779B9) >> 8) * 2^-24
 *         r   = mix(lk ^ mix(y W + x)) mod n^2          (the cells rotate per pixel)
 *         k'  = (j n + i + r) mod n^2,  ci = k' mod n,  cj = k' div n
 *     y is the WHOLE-image row (shards hash what the whole frame hashes), ray_id
 *     the value supersampled frames give the area lights' hash.
 * Square to disc (no trigonometry: the device and a host restatement agree to
 * the bit), inv_n = R(1) / R(n):
 *     a  = 2 * ((ci + ju) * inv_n) - 1,   b = 2 * ((cj + jv) * inv_n) - 1
 *     ex = a * sqrt(1 - (b * b) * 0.5),   ey = b * sqrt(1 - (a * a) * 0.5)
 * Lens point and focal point in camera space, f = focal_distance:
 *     L = (aperture * ex, aperture * ey, 0),   F = (wx * f, wy * f, -f)
 * The ray: origin = inverse * L and target = inverse * F as points, each row
 * the left fold (((0 + m0 x) + m1 y) + m2 z) + m3 (matrix.rs:332-346);
 * direction = normalized(target - origin) (vector.rs:84-91).  That is the f64
 * kernels' arithmetic to the bit.  The f32 kernels form the direction as
 * M3 * (F - L) with their own fused transforms; their bar is statistical.
 *
 * aperture == 0 IS rt_render_supersampled* (after the checks): the same bytes
 * and counters, as grid = 1 there is rt_render*.  grid = 1 with a positive
 * aperture is one lens point per pixel: accumulate frames over seeds.
 * RT_ERR_INVALID, each with its own rt_last_error text and checked before the
 * context is looked at: a null lens, an aperture below 0 or not finite, a
 * focal distance not above 0 or not finite, a jitter other than 0 or 1; then
 * whatever rt_render_supersampled* refuses, with its text.
 * rt_lens_ray (host only) writes the f64 ray {origin, direction} of sample
 * (i, j) of pixel (x, y), `camera` being the OUTPUT camera, for either jitter
 * mode. */
typedef struct rt_lens_desc {      /* 24 bytes */
    double aperture;               /* lens radius in camera space, >= 0, finite */
    double focal_distance;         /* distance of the focal plane along the view axis, > 0, finite */
    uint32_t jitter;               /* RT_JITTER_NONE | RT_JITTER_HASHED */
    uint32_t seed;
} rt_lens_desc;
int rt_render_lens(rt_context* ctx, const rt_camera_desc* camera,
                   const rt_render_options* options, uint32_t grid,
                   const rt_lens_desc* lens, void* out_host, rt_stats* stats);
int rt_render_lens_device(rt_context* ctx, const rt_camera_desc* camera,
                          const rt_render_options* options, uint32_t grid,
                          const rt_lens_desc* lens, void* out_device, void* hip_stream);
int rt_lens_ray(const rt_camera_desc* camera, uint32_t grid, const rt_lens_desc* lens,
                uint32_t x, uint32_t y, uint32_t i, uint32_t j, double ray[6]);

/* Motion blur: moving shapes and a shutter.  The reference
 * has no motion, so this text is the contract; what it says can be checked
 * against the reference all the same, because a ray of time tau in a moving
 * world is that ray in the static world whose movers are displaced by v tau
 * (rt_motion_displace), which the reference renders.
 *
 * What moves.  A top-level shape or a mesh instance may have a constant
 * velocity v (world units per unit of time): at time tau it is the shape with
 * transformation translation(v tau) * T.  Nothing else moves: no light, not
 * the camera, no triangle inside an rt_mesh_desc run (to move a mesh, place it
 * as an instance).  The top-level triangle hierarchy stays a static,
 * world-space structure: a moving top-level triangle goes to the flat run
 * behind it.
 *
 * rt_scene_upload_moving is rt_scene_upload_mapped with a motion list; with
 * n_motion = 0 it is that call itself.  An entry whose velocity is zero in
 * every component (+0 or -0) is dropped at upload: that shape is static.  Two
 * shapes are value-equal (the containers walk's identity classes) iff they
 * were equal before and their velocities are equal as f64 values.  A moving
 * instance with a value-equal partner is uploaded expanded, as now, and its
 * records carry the velocity.  (Two movers that share a transformation and
 * differ in velocity are two classes at every time, tau = 0 included, where
 * the displaced static world has them value-equal: the one place the two
 * differ.)  A moving world is uploaded to one device: a context of a group of
 * more than one rank refuses it with RT_ERR_INVALID.
 * RT_ERR_INVALID, each with its own rt_last_error text and checked before the
 * context is looked at, after the other lists' own checks, in this order: a null list with a nonzero
 * count, an unknown target, an index out of range, a target named twice, a
 * component that is not finite, a shape that belongs to a mesh run (a shape
 * index from n_shapes on that is still a world index of the expansion names a
 * triangle of an instance's mesh: move the instance instead).
 *
 * The displaced point.  All arithmetic in the kernel's real type R; v is
 * rounded once to R.  For a ray of time tau and a moving shape, every POINT p
 * that the reference multiplies by shape.inverse is replaced, per component, by
 * p.x - v.x * tau: multiply, then subtract, no FMA in the f64 kernels.  The
 * points are the ray origin in Ray::intersect, the world point in normal_at,
 * the point in pattern_at_shape and over_point in the texture maps.  Vectors
 * are untouched.  The hit's t, the hit point o + t d, over_point and
 * under_point are in world space at time tau, as the displaced static world
 * gives them.  A secondary ray (reflection, refraction, shadow) keeps its
 * primary ray's tau.  Counters, ties and the u8 quantization are unchanged.
 *
 * The shutter.  rt_render_shutter* is rt_render_lens* with one change: sample
 * (i, j) of pixel (x, y) also has a time.  A NULL lens or aperture == 0 gives
 * the sample rays of rt_render_supersampled* (camera_ray's arithmetic), else
 * the lens rays.  Grid range, flags, shards (hashes take whole-image
 * coordinates), the refusal of groups of more than one rank, the sample order
 * (j outer, i inner), the weights, the counters, the stream order and the u8
 * rule are rt_render_lens*'s.  The time, with n = grid, mix and ray_id as
 * under "Hashed jitter" and uint32_t wraparound:
 *     RT_JITTER_NONE:    c = j n + i,  jt = 0.5
 *     RT_JITTER_HASHED:  tk  = mix(seed ^ 0x54494D45)
 *                        key = mix(tk ^ ray_id),   ray_id = (n y + j)(n W) + n x + i
 *                        jt  = (key >> 8) * 2^-24
 *                        r   = mix(tk ^ mix(y W + x)) mod n^2
 *                        c   = (j n + i + r) mod n^2
 *     u   = (c + jt) * inv_n2,          inv_n2 = R(1) / R(n^2)
 *     tau = open_R + span_R * u         (multiply, then add)
 * open and span = close - open are formed in f64 on the host and each rounded
 * once to R; y is the whole-image row.  rt_shutter_time (host only) returns
 * the f64 value for either jitter mode, `camera` being the OUTPUT camera.
 * A world without moving shapes makes rt_render_shutter* equal rt_render_lens*
 * after the checks (rt_render_supersampled* when there is no lens): the same
 * bytes and counters.  RT_ERR_INVALID, each with its own text: a null
 * shutter, a bound that is not finite, open > close, a jitter other than 0 or
 * 1; after those whatever rt_render_lens* refuses, with its text.
 *
 * Ray batches.  rt_trace_rays_timed* is rt_trace_rays* with a time per ray,
 * on the device in the precision's own type; times == NULL: every time is 0.
 * out_hit is the primary ray's closest hit at its time.
 *
 * Everything else on a moving world (rt_render*, rt_render_supersampled*,
 * rt_render_lens*, rt_color_at, rt_trace_rays*) sees the world at tau = 0: the
 * static world's colours and counters.  Per-scene builds are refused for a
 * world with a moving shape; rt_jit_status says so in its log.
 *
 * rt_motion_displace (host only) writes the static world at time tau: each
 * moving target's inverse becomes inverse * translation(-v tau), v tau formed
 * per component in f64 and the product as matrix.rs multiplies (each element
 * the left fold ((a0 b0 + a1 b1) + a2 b2) + a3 b3).  out_shapes holds
 * n_shapes entries and out_instances n_instances (either may be NULL when its
 * count is 0; each may alias its input); at tau = 0, and for a zero velocity,
 * the inverse is the input's bit for bit.  This is "the world at time tau" of
 * the tests, and how a still at tau is rendered through the older entry
 * points, per-scene kernels included. */
#define RT_MOVE_SHAPE    0
#define RT_MOVE_INSTANCE 1
typedef struct rt_motion_desc {   /* 32 bytes */
    uint32_t target;              /* RT_MOVE_* */
    uint32_t index;               /* into `shapes` (world order) or `instances` */
    double   velocity[3];
} rt_motion_desc;
int rt_scene_upload_moving(rt_context* ctx,
                           const rt_shape_desc* shapes, uint32_t n_shapes,
                           const rt_mesh_desc* meshes, uint32_t n_meshes,
                           const rt_instance_desc* instances, uint32_t n_instances,
                           const rt_smooth_desc* smooth, uint32_t n_smooth,
                           const rt_uv_desc* uvs, uint32_t n_uvs,
                           const rt_texture_desc* textures, uint32_t n_textures,
                           const rt_material_desc* materials, uint32_t n_materials,
                           const rt_pattern_desc* patterns, uint32_t n_patterns,
                           const rt_light_desc* lights, uint32_t n_lights,
                           const rt_area_light_desc* area, uint32_t n_area,
                           const rt_uv_map_desc* maps, uint32_t n_maps,
                           const rt_motion_desc* motion, uint32_t n_motion);
typedef struct rt_shutter_desc {  /* 24 bytes */
    double   open, close;         /* finite, open <= close */
    uint32_t jitter, seed;        /* RT_JITTER_NONE | RT_JITTER_HASHED */
} rt_shutter_desc;
int rt_render_shutter(rt_context* ctx, const rt_camera_desc* camera,
                      const rt_render_options* options, uint32_t grid,
                      const rt_lens_desc* lens /* may be NULL */, const rt_shutter_desc* shutter,
                      void* out_host, rt_stats* stats);
int rt_render_shutter_device(rt_context* ctx, const rt_camera_desc* camera,
                             const rt_render_options* options, uint32_t grid,
                             const rt_lens_desc* lens, const rt_shutter_desc* shutter,
                             void* out_device, void* hip_stream);
int rt_shutter_time(const rt_camera_desc* camera, uint32_t grid, const rt_shutter_desc* shutter,
                    uint32_t x, uint32_t y, uint32_t i, uint32_t j, double* tau);
int rt_trace_rays_timed(rt_context* ctx, const double* rays, const double* times, uint64_t n_rays,
                        const rt_ray_options* options, double* out_rgb, rt_ray_hit_f64* out_hit,
                        rt_stats* stats);
int rt_trace_rays_timed_device(rt_context* ctx, const void* rays_device, const void* times_device,
                               uint64_t n_rays, const rt_ray_options* options,
                               void* out_rgb_device, void* out_hit_device, void* hip_stream);
int rt_motion_displace(const rt_shape_desc* shapes, uint32_t n_shapes,
                       const rt_instance_desc* instances, uint32_t n_instances,
                       const rt_motion_desc* motion, uint32_t n_motion, double tau,
                       rt_shape_desc* out_shapes, rt_instance_desc* out_instances);
/* The motion of the last upload (zeros after an upload without a nonzero
 * velocity): moving shapes and instances, the bytes of the velocity tables of
 * both precisions, and whether the last launch was a shutter frame or a timed
 * ray batch of kernels that hold the motion code. */
typedef struct rt_motion_info {
    uint32_t moving_shapes;
    uint32_t moving_instances;
    uint32_t ran_motion;
    uint32_t reserved;
    uint64_t motion_bytes;
} rt_motion_info;
int rt_scene_motion_info(rt_context* ctx, rt_motion_info* out);

/* Peer canvas: a frame assembled in place instead of gathered (SURVEY.md
 * §8e; the north star's "gather of framebuffer strips over xGMI" done as the
 * shards' own stores into rank 0's image).  The owner creates a device canvas
 * (an image of `bytes` plus n_flags completion flags and one release flag)
 * and shares its IPC handle; other processes map it with rt_canvas_open.
 * rt_render_to_canvas renders shard options.shard_index of
 * options.shard_count straight into the canvas at its pixels' IMAGE rows,
 * then raises that shard's flag to `seq`; before rendering it waits (on the
 * device) until the owner has released frame seq - 1, so a shard never
 * overwrites a frame still being read.  rt_canvas_wait makes the owner's
 * stream wait until every flag has reached `seq`; rt_canvas_release marks
 * frame `seq` consumed (stream-ordered after its readers).  `seq` starts at 1
 * and grows by one per frame; the flags start at 0.  The waits are bounded:
 * after timeout_ms a wait ends and RT_ERR_POOL ("peer canvas") is reported
 * at the context's next synchronous call.  Asynchronous on `hip_stream`
 * except create / open / close, which synchronize. */
#define RT_IPC_HANDLE_BYTES 64
int rt_canvas_create(rt_context* ctx, uint64_t bytes, uint32_t n_flags, void** canvas,
                     uint8_t handle[RT_IPC_HANDLE_BYTES]);
int rt_canvas_open(rt_context* ctx, const uint8_t handle[RT_IPC_HANDLE_BYTES], uint64_t bytes, uint32_t n_flags,
                   void** canvas);
int rt_canvas_close(rt_context* ctx, void* canvas);
int rt_render_to_canvas(rt_context* ctx, const rt_camera_desc* camera, const rt_render_options* options,
                        void* canvas, uint64_t seq, double timeout_ms, void* hip_stream);
int rt_canvas_wait(rt_context* ctx, void* canvas, uint64_t seq, double timeout_ms, void* hip_stream);
int rt_canvas_release(rt_context* ctx, void* canvas, uint64_t seq, void* hip_stream);
/* The canvas image (its first `bytes`) into a host buffer, after everything
 * submitted to this context's device (synchronous). */
int rt_canvas_read(rt_context* ctx, void* canvas, void* out_host, uint64_t bytes);

/* How a multi-GPU context brings the shards to rank 0: RT_GATHER_RCCL (the
 * default) renders strips and ncclGathers + de-interleaves them;
 * RT_GATHER_PEER renders every shard into one peer canvas on rank 0 (IPC
 * handle broadcast over RCCL once; peer access within one process) and
 * copies the finished image to the caller's buffer.  Collective: every rank
 * sets the same mode. */
enum { RT_GATHER_RCCL = 0, RT_GATHER_PEER = 1 };
int rt_context_set_gather(rt_context* ctx, int mode);

/* Cumulative device counters since context creation (after a sync). */
int rt_read_counters(rt_context* ctx, rt_stats* totals);

/* Rays per generation (the wavefront's size at each bounce), cumulative
 * over this context's launches made with RT_FLAG_GENERATIONS.  Indexed by
 * `remaining` (world.rs:70-86): a primary ray is traced at max_depth and a
 * reflected or refracted child at its parent's remaining - 1
 * (world.rs:114-157), so generation g of a frame rendered at depth D is
 * entry D - g.  traced = radiance rays traced (internal_color_at calls),
 * shaded = hits shaded; each shaded hit casts one shadow ray per light
 * (world.rs:46-52).  Group contexts report the calling process's GPUs. */
typedef struct rt_generation_counts {
    uint64_t traced[RT_MAX_SUPPORTED_DEPTH + 1];
    uint64_t shaded[RT_MAX_SUPPORTED_DEPTH + 1];
} rt_generation_counts;
int rt_read_generation_counts(rt_context* ctx, rt_generation_counts* out);

/* De-interleave gathered shard strips (shard-major, each rt_shard_rows tall)
 * into one row-major image on the device, on `hip_stream`. */
int rt_assemble_shards(rt_context* ctx, const void* gathered_device,
                       uint32_t width, uint32_t height, uint32_t shard_count,
                       uint32_t bytes_per_pixel, void* image_device,
                       void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* RTC_H */
