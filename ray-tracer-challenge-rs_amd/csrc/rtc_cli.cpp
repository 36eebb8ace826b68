// rtc_cli.cpp — command-line driver mirroring ray-tracer-cli/src/main.rs:11-31
// and cli/cli_arguments.rs:4-13: `<SCENE> <OUT> [-r serial|parallel] [-q]`,
// timing of the render call only (main.rs:17-24), then the PNG save
// (main.rs:26, canvas.rs:114-137; OUT ending in anything but .png gets the
// reference's P3 text, canvas.rs:75-97, or a binary P6 with --ppm-binary).
// The reference's rendering modes pick Camera::render or render_parallel;
// here every mode renders on the GPU (the library owns the
// parallelism), so `-r serial|parallel|gpu` are accepted and equivalent.
// Extra flags: --width/--height (same as editing the YAML camera size),
// --depth (World::MAX_REFLECTION_ITERATIONS = 6 by default), --precision
// f32|f64, --device N, --gpus N (split the frame across devices 0..N-1 of a
// multi-GPU context), --samples N (N x N samples per pixel,
// averaged on the device: rt_render_supersampled; 1, the
// default, is the reference's one ray per pixel), --obj FILE (repeatable: the
// triangles of a Wavefront OBJ mesh, rtc_scene.h rt_mesh_*, appended after the
// YAML world's shapes with Material::default and no transformation),
// --instance FILE:tx,ty,tz[:s] (repeatable: a copy of the mesh scaled by s,
// default 1, and moved by (tx, ty, tz), with Material::default, after every
// shape and --obj triangle, in command-line order; each FILE is loaded once and
// the world goes up through rt_scene_upload_instanced),
// --smooth (--obj and --instance read the files' vertex normals and the faces
// that name three are smooth triangles: rt_scene_upload_smooth, DESIGN.md
// §3.11; without it the output is what it was), --texture IMAGE.ppm|png with
// --texture-filter nearest|bilinear (the --obj and --instance meshes' material
// gets an image pattern and their vt lines are read: rt_scene_upload_textured,
// DESIGN.md §3.12), --texture-map planar|spherical|cylindrical (how a face
// without vt coordinates is mapped) and --cube-map L,F,R,B,U,D (six images in
// place of --texture: rt_scene_upload_mapped), --area-light cx,cy,cz:ux,uy,uz:vx,vy,vz:USTEPSxVSTEPS
// [:r,g,b][:jitter[=SEED]] (repeatable: an area light added to the scene's
// lights, rt_scene_upload_lit), --aperture R --focus D
// [--lens-jitter[=SEED]] (a thin lens of radius R focused at distance D, both
// in camera space: rt_render_lens; works with --samples, whose
// N x N samples leave the cells of an N x N grid on the lens disc), --move
// I:vx,vy,vz and --instance ...:v=vx,vy,vz with --shutter open,close[:jitter=SEED]
// (motion blur: rt_scene_upload_moving and rt_render_shutter, DESIGN.md §3.17;
// each sample also has a time in the shutter's interval).  Pixels are
// quantized on the device as canvas.rs:117-123 does.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/rtc.h"
#include "../../include/rtc_scene.h"

static int usage() {
    std::fprintf(stderr,
                 "usage: rtc <SCENE.yaml> <OUT.png|OUT.ppm> [-r serial|parallel|gpu] [-q] [--width W] [--height H]\n"
                 "           [--depth D] [--precision f32|f64] [--device N] [--gpus N] [--ppm-binary] [--timings]\n"
                 "           [--samples N] [--obj MESH.obj]... [--instance MESH.obj:tx,ty,tz[:s][:v=vx,vy,vz]]... [--smooth]\n"
                 "           [--texture IMAGE.ppm|png] [--texture-filter nearest|bilinear]\n"
                 "           [--texture-map planar|spherical|cylindrical] [--cube-map L,F,R,B,U,D]\n"
                 "           [--area-light cx,cy,cz:ux,uy,uz:vx,vy,vz:USTEPSxVSTEPS[:r,g,b][:jitter[=SEED]]]...\n"
                 "           [--aperture R --focus D [--lens-jitter[=SEED]]]\n"
                 "           [--move I:vx,vy,vz]... [--shutter open,close[:jitter=SEED]]\n"
                 "  --obj MESH.obj appends the mesh's triangles (v and f lines; faces fan-triangulated) to the\n"
                 "  scene's shapes, with the default material and no transformation; repeatable.\n"
                 "  --instance MESH.obj:tx,ty,tz[:s] places a copy of the mesh, scaled by s (default 1) and moved by\n"
                 "  (tx, ty, tz), with the default material, after the shapes; repeatable, each file is read once.\n"
                 "  --smooth makes --obj and --instance read the files' vertex normals (vn lines, f i//k and i/j/k):\n"
                 "  a face whose vertices all name a normal is shaded with the interpolated normal.\n"
                 "  --texture IMAGE.ppm|png gives the --obj and --instance meshes' material that image as its pattern\n"
                 "  and reads the files' texture coordinates (vt lines, f i/j and i/j/k); a face without them is\n"
                 "  mapped by its x and z.  --texture-filter nearest|bilinear picks the filter (default bilinear).\n"
                 "  --texture-map planar|spherical|cylindrical maps a face without texture coordinates by its x and z\n"
                 "  (the default), by longitude and latitude around the origin, or by longitude and height.\n"
                 "  --cube-map L,F,R,B,U,D takes six image files in place of --texture, the faces left, front, right,\n"
                 "  back, up and down of the cube |x|, |y|, |z| <= 1; a face with texture coordinates samples F.\n"
                 "  --area-light adds an area light to the scene's lights: the parallelogram from corner c along the\n"
                 "  full edges u and v, USTEPS x VSTEPS samples (1..%d each), intensity r,g,b (default 1,1,1), sampled\n"
                 "  at the cell centres or, with jitter, at hashed positions per ray (seed SEED, default 0); repeatable.\n"
                 "  --samples N renders N x N samples per pixel (1..%d, default 1 = one ray per pixel centre) and\n"
                 "  averages them on the GPU.\n"
                 "  --aperture R --focus D renders through a thin lens of radius R focused at distance D along the\n"
                 "  view axis (depth of field); each of the N x N samples leaves its own point of the lens, the cell\n"
                 "  centres of a grid on the disc or, with --lens-jitter[=SEED], hashed positions per sample.\n"
                 "  --move I:vx,vy,vz gives shape I of the scene (file order, from 0) the constant velocity (vx, vy, vz);\n"
                 "  repeatable.  --instance ...:v=vx,vy,vz gives that copy of the mesh a velocity.  --shutter open,close\n"
                 "  renders motion blur: each of the N x N samples of --samples N (through the lens of --aperture and\n"
                 "  --focus where given) sees every mover where it is at the sample's time between open and close,\n"
                 "  the cell centres of the interval or, with :jitter=SEED, hashed times per sample.\n"
                 "  -r serial|parallel are accepted for the reference's command lines but render on the GPU like\n"
                 "  -r gpu: this build ships no CPU renderer (Camera::render / render_parallel are not in it).\n",
                 RT_LIGHT_MAX_STEPS, RT_MAX_SAMPLE_GRID);
    return 2;
}

// One --area-light argument: cx,cy,cz:ux,uy,uz:vx,vy,vz:USTEPSxVSTEPS[:r,g,b][:jitter[=SEED]]
static bool parse_area_light(const std::string& a, rt_area_light_desc* out) {
    std::vector<std::string> part;
    for (size_t at = 0;;) {
        const size_t c = a.find(':', at);
        part.push_back(a.substr(at, c == std::string::npos ? c : c - at));
        if (c == std::string::npos) break;
        at = c + 1;
    }
    auto triple = [](const std::string& v, double t[3]) {
        char tail = 0;
        return std::sscanf(v.c_str(), "%lf,%lf,%lf%c", &t[0], &t[1], &t[2], &tail) == 3;
    };
    if (part.size() < 4 || part.size() > 6) return false;
    *out = rt_area_light_desc{};
    if (!triple(part[0], out->corner) || !triple(part[1], out->full_uvec) || !triple(part[2], out->full_vvec)) return false;
    char tail = 0;
    if (std::sscanf(part[3].c_str(), "%ux%u%c", &out->usteps, &out->vsteps, &tail) != 2) return false;
    out->intensity[0] = out->intensity[1] = out->intensity[2] = 1.0;
    out->jitter = RT_JITTER_NONE;
    size_t at = 4;
    if (at < part.size() && triple(part[at], out->intensity)) ++at;
    if (at < part.size()) {
        if (part[at] == "jitter") {
            out->jitter = RT_JITTER_HASHED;
        } else if (part[at].rfind("jitter=", 0) == 0) {
            char* end = nullptr;
            const unsigned long seed = std::strtoul(part[at].c_str() + 7, &end, 0);
            if (end == part[at].c_str() + 7 || *end || seed > 0xFFFFFFFFul) return false;
            out->jitter = RT_JITTER_HASHED;
            out->seed = (uint32_t)seed;
        } else {
            return false;
        }
        ++at;
    }
    return at == part.size();
}

// Three finite numbers "x,y,z" and nothing else.
static bool parse_triple(const std::string& v, double t[3]) {
    char tail = 0;
    return std::sscanf(v.c_str(), "%lf,%lf,%lf%c", &t[0], &t[1], &t[2], &tail) == 3 && t[0] - t[0] == 0.0 &&
           t[1] - t[1] == 0.0 && t[2] - t[2] == 0.0;
}

// One --move argument: I:vx,vy,vz
struct Move {
    uint32_t shape;
    double v[3];
};
static bool parse_move(const std::string& a, Move* out) {
    const size_t c = a.find(':');
    if (c == std::string::npos || c == 0) return false;
    char* end = nullptr;
    const std::string index = a.substr(0, c);
    const unsigned long i = std::strtoul(index.c_str(), &end, 10);
    if (index[0] < '0' || index[0] > '9' || *end || i > 0xFFFFFFFFul) return false;
    out->shape = (uint32_t)i;
    return parse_triple(a.substr(c + 1), out->v);
}

// One --shutter argument: open,close[:jitter=SEED]
static bool parse_shutter(const std::string& a, rt_shutter_desc* out) {
    const size_t c = a.find(':');
    const std::string bounds = a.substr(0, c);
    char tail = 0;
    *out = rt_shutter_desc{0.0, 0.0, RT_JITTER_NONE, 0};
    if (std::sscanf(bounds.c_str(), "%lf,%lf%c", &out->open, &out->close, &tail) != 2) return false;
    if (!(out->open - out->open == 0.0) || !(out->close - out->close == 0.0) || out->open > out->close) return false;
    if (c == std::string::npos) return true;
    const std::string j = a.substr(c + 1);
    if (j.rfind("jitter=", 0) != 0) return false;
    char* end = nullptr;
    const unsigned long seed = std::strtoul(j.c_str() + 7, &end, 0);
    if (j[7] < '0' || j[7] > '9' || *end || seed > 0xFFFFFFFFul) return false;
    out->jitter = RT_JITTER_HASHED;
    out->seed = (uint32_t)seed;
    return true;
}

// One --instance argument: FILE:tx,ty,tz[:s][:v=vx,vy,vz]
struct Placement {
    std::string file;
    double t[3], s;
    double v[3];
    bool moving;
};
static bool parse_placement(const std::string& whole, Placement* out) {
    auto triple = [](const std::string& v, double t[3]) {
        char tail = 0;
        return std::sscanf(v.c_str(), "%lf,%lf,%lf%c", &t[0], &t[1], &t[2], &tail) == 3;
    };
    std::string a = whole;
    out->moving = false;
    out->v[0] = out->v[1] = out->v[2] = 0.0;
    const size_t vel = a.rfind(":v=");
    if (vel != std::string::npos) {  // the trailing velocity, then the placement as it always was
        if (!parse_triple(a.substr(vel + 3), out->v)) return false;
        out->moving = true;
        a = a.substr(0, vel);
    }
    const size_t last = a.rfind(':');
    if (last == std::string::npos || last == 0) return false;
    out->s = 1.0;
    if (triple(a.substr(last + 1), out->t)) {
        out->file = a.substr(0, last);
        return true;
    }
    char* end = nullptr;
    out->s = std::strtod(a.c_str() + last + 1, &end);
    const size_t mid = a.rfind(':', last - 1);
    if (end == a.c_str() + last + 1 || *end || mid == std::string::npos || mid == 0) return false;
    out->file = a.substr(0, mid);
    return triple(a.substr(mid + 1, last - mid - 1), out->t);
}

int main(int argc, char** argv) {
    if (argc < 3) return usage();
    // A one-shot process copies one frame back: the HIP runtime's first
    // copy on an SDMA engine costs 8-12 ms of engine set-up, a blit kernel
    // on the compute queue ~2.4 ms for the same 24.9 MB (DESIGN.md §5,
    // scripts/init_probe.cpp).  Read when the runtime starts (the first HIP
    // call, in rt_context_create); a value already in the environment wins.
    setenv("GPU_FORCE_BLIT_COPY_SIZE", "1048576", 0);  // KiB: every copy below 1 GiB

    const char* scene_path = argv[1];
    const char* out_path = argv[2];
    bool quiet = false, ppm_binary = false, timings = false;
    uint32_t width = 0, height = 0, depth = RT_DEFAULT_MAX_DEPTH, precision = RT_PRECISION_F32;
    int device = 0, gpus = 1;
    uint32_t samples = 1;
    rt_lens_desc lens = {0.0, 0.0, RT_JITTER_NONE, 0};
    bool have_aperture = false, have_focus = false, have_lens_jitter = false;
    bool smooth = false;
    const char* texture_path = nullptr;
    int texture_filter = RT_FILTER_BILINEAR;
    uint32_t texture_map = RT_MAP_PLANAR;
    bool have_texture_map = false;
    std::vector<std::string> cube_paths;  // --cube-map: left, front, right, back, up, down
    std::vector<const char*> obj_paths;
    std::vector<Placement> placements;
    std::vector<rt_area_light_desc> area_lights;
    std::vector<Move> moves;
    rt_shutter_desc shutter = {0.0, 0.0, RT_JITTER_NONE, 0};
    bool have_shutter = false;
    for (int i = 3; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : nullptr; };
        if (a == "-q" || a == "--quiet") quiet = true;
        else if (a == "--ppm-binary") ppm_binary = true;
        else if (a == "--timings") timings = true;
        else if (a == "--smooth") smooth = true;
        else if (a == "--texture") { texture_path = next(); if (!texture_path) return usage(); }
        else if (a == "--texture-filter") {
            const char* v = next();
            if (!v || (std::strcmp(v, "nearest") && std::strcmp(v, "bilinear"))) return usage();
            texture_filter = std::strcmp(v, "nearest") == 0 ? RT_FILTER_NEAREST : RT_FILTER_BILINEAR;
        }
        else if (a == "--texture-map") {
            const char* v = next();
            if (!v) return usage();
            if (std::strcmp(v, "planar") == 0) texture_map = RT_MAP_PLANAR;
            else if (std::strcmp(v, "spherical") == 0) texture_map = RT_MAP_SPHERICAL;
            else if (std::strcmp(v, "cylindrical") == 0) texture_map = RT_MAP_CYLINDRICAL;
            else return usage();
            have_texture_map = true;
        }
        else if (a == "--cube-map") {
            const char* v = next();
            if (!v) return usage();
            const std::string list = v;
            cube_paths.clear();
            for (size_t at = 0;;) {
                const size_t c = list.find(',', at);
                cube_paths.push_back(list.substr(at, c == std::string::npos ? c : c - at));
                if (c == std::string::npos) break;
                at = c + 1;
            }
            bool six = cube_paths.size() == 6;
            for (const std::string& f : cube_paths) six = six && !f.empty();
            if (!six) {
                std::fprintf(stderr, "error: --cube-map takes six image files: L,F,R,B,U,D\n");
                return usage();
            }
        }
        else if (a == "-r" || a == "--rendering-mode") {
            const char* v = next();
            if (!v || (std::strcmp(v, "serial") && std::strcmp(v, "parallel") && std::strcmp(v, "gpu"))) return usage();
        }
        else if (a == "--gpus") { const char* v = next(); if (!v || std::atoi(v) < 1) return usage(); gpus = std::atoi(v); }
        else if (a == "--width") { const char* v = next(); if (!v) return usage(); width = (uint32_t)std::atoi(v); }
        else if (a == "--height") { const char* v = next(); if (!v) return usage(); height = (uint32_t)std::atoi(v); }
        else if (a == "--depth") { const char* v = next(); if (!v) return usage(); depth = (uint32_t)std::atoi(v); }
        else if (a == "--samples") {
            const char* v = next();
            char* end = nullptr;
            const long n = v ? std::strtol(v, &end, 10) : 0;
            if (!v || *end || n < 1 || n > RT_MAX_SAMPLE_GRID) {
                std::fprintf(stderr, "error: --samples takes a whole number from 1 to %d\n", RT_MAX_SAMPLE_GRID);
                return usage();
            }
            samples = (uint32_t)n;
        }
        else if (a == "--aperture" || a == "--focus") {
            const char* v = next();
            char* end = nullptr;
            const double d = v ? std::strtod(v, &end) : 0.0;
            const bool aperture = a == "--aperture";
            if (!v || end == v || *end || !(d - d == 0.0) || (aperture ? d < 0.0 : !(d > 0.0))) {
                std::fprintf(stderr, aperture ? "error: --aperture takes a lens radius, a number >= 0\n"
                                              : "error: --focus takes a focal distance, a number > 0\n");
                return usage();
            }
            (aperture ? lens.aperture : lens.focal_distance) = d;
            (aperture ? have_aperture : have_focus) = true;
        }
        else if (a == "--lens-jitter" || a.rfind("--lens-jitter=", 0) == 0) {
            if (a.size() > 13) {
                const char* v = a.c_str() + 14;
                char* end = nullptr;
                const unsigned long seed = std::strtoul(v, &end, 0);
                if (end == v || *end || *v == '-' || seed > 0xFFFFFFFFul) {
                    std::fprintf(stderr, "error: --lens-jitter takes an optional =SEED, a whole number below 2^32\n");
                    return usage();
                }
                lens.seed = (uint32_t)seed;
            }
            lens.jitter = RT_JITTER_HASHED;
            have_lens_jitter = true;
        }
        else if (a == "--obj") { const char* v = next(); if (!v) return usage(); obj_paths.push_back(v); }
        else if (a == "--instance") {
            const char* v = next();
            Placement p;
            if (!v || !parse_placement(v, &p)) {
                std::fprintf(stderr, "error: --instance takes FILE:tx,ty,tz[:s][:v=vx,vy,vz]\n");
                return usage();
            }
            placements.push_back(p);
        }
        else if (a == "--move") {
            const char* v = next();
            Move m;
            if (!v || !parse_move(v, &m)) {
                std::fprintf(stderr, "error: --move takes I:vx,vy,vz, a shape of the scene (file order, from 0) and its velocity\n");
                return usage();
            }
            for (const Move& other : moves)
                if (other.shape == m.shape) {
                    std::fprintf(stderr, "error: --move names shape %u twice\n", m.shape);
                    return usage();
                }
            moves.push_back(m);
        }
        else if (a == "--shutter") {
            const char* v = next();
            if (!v || !parse_shutter(v, &shutter)) {
                std::fprintf(stderr, "error: --shutter takes open,close[:jitter=SEED], two finite times with open <= close\n");
                return usage();
            }
            have_shutter = true;
        }
        else if (a == "--area-light") {
            const char* v = next();
            rt_area_light_desc d;
            if (!v || !parse_area_light(v, &d)) {
                std::fprintf(stderr, "error: --area-light takes cx,cy,cz:ux,uy,uz:vx,vy,vz:USTEPSxVSTEPS[:r,g,b][:jitter[=SEED]]\n");
                return usage();
            }
            area_lights.push_back(d);
        }
        else if (a == "--device") { const char* v = next(); if (!v) return usage(); device = std::atoi(v); }
        else if (a == "--precision") {
            const char* v = next();
            if (!v) return usage();
            precision = std::strcmp(v, "f64") == 0 ? RT_PRECISION_F64 : RT_PRECISION_F32;
        } else return usage();
    }
    if (have_aperture && !have_focus) {
        std::fprintf(stderr, "error: --aperture needs --focus D, the distance of the plane in focus\n");
        return usage();
    }
    if ((have_focus || have_lens_jitter) && !have_aperture) {
        std::fprintf(stderr, "error: --focus and --lens-jitter describe a lens: give --aperture R\n");
        return usage();
    }
    bool movers = !moves.empty();
    for (const Placement& p : placements) movers = movers || p.moving;
    if (movers && !have_shutter) {
        std::fprintf(stderr, "error: --move and --instance ...:v= describe motion: give --shutter open,close\n");
        return usage();
    }
    if (!quiet) std::printf("Rendering image using scene at %s\n", scene_path);
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    const auto t_load = clk::now();
    rt_scene* scene = nullptr;
    if (rt_scene_load_yaml(scene_path, &scene) != RT_OK) {
        std::fprintf(stderr, "error: %s\n", rt_last_error());
        return 1;
    }
    rt_scene_view v;
    rt_scene_view_get(scene, &v);
    // --move: the scene's shapes in file order; --instance ...:v=: the placements in command-line order
    std::vector<rt_motion_desc> motion;
    for (const Move& m : moves) {
        if (m.shape >= v.n_shapes) {
            std::fprintf(stderr, "error: --move names shape %u, the scene has %u shapes\n", m.shape, v.n_shapes);
            return 2;
        }
        motion.push_back({RT_MOVE_SHAPE, m.shape, {m.v[0], m.v[1], m.v[2]}});
    }
    for (size_t k = 0; k < placements.size(); ++k)
        if (placements[k].moving)
            motion.push_back({RT_MOVE_INSTANCE, (uint32_t)k, {placements[k].v[0], placements[k].v[1], placements[k].v[2]}});
    rt_camera_desc cam = v.camera;
    if (width || height) rt_camera_resize(&cam, width ? width : cam.width, height ? height : cam.height);
    // --obj: the scene's tables with each mesh's triangles after its shapes, all on one Material::default
    // (material.rs:157-161) appended to the materials
    std::vector<rt_shape_desc> shapes(v.shapes, v.shapes + v.n_shapes);
    std::vector<rt_material_desc> materials(v.materials, v.materials + v.n_materials);
    // --texture: the image, one more pattern after the scene's, and the meshes' texture coordinates
    std::vector<rt_pattern_desc> patterns(v.patterns, v.patterns + v.n_patterns);
    std::vector<rt_uv_desc> uv_list;
    // (--texture: one texture; --cube-map: six, the pattern's own being the front face's)
    std::vector<rt_texture_desc> textures;
    std::vector<uint8_t*> texture_rgb;
    std::vector<rt_uv_map_desc> maps;
    auto free_textures = [&] {
        for (uint8_t* rgb : texture_rgb) rt_image_free(rgb);
        texture_rgb.clear();
    };
    const bool cube_mapped = !cube_paths.empty();
    if ((texture_path || cube_mapped) && obj_paths.empty() && placements.empty()) {
        std::fprintf(stderr, "error: %s needs a mesh to show on: give --obj or --instance\n", texture_path ? "--texture" : "--cube-map");
        return usage();
    }
    if (texture_path && cube_mapped) {
        std::fprintf(stderr, "error: --cube-map takes the place of --texture: give one of them\n");
        return usage();
    }
    if (have_texture_map && cube_mapped) {
        std::fprintf(stderr, "error: --texture-map applies to --texture's pattern, not to a --cube-map\n");
        return usage();
    }
    if (have_texture_map && !texture_path) {
        std::fprintf(stderr, "error: --texture-map needs --texture\n");
        return usage();
    }
    const bool textured = texture_path != nullptr || cube_mapped;
    if (textured) {
        std::vector<std::string> files = cube_paths;
        if (texture_path) files.assign(1, texture_path);
        for (const std::string& f : files) {
            rt_texture_desc t = {};
            uint8_t* rgb = nullptr;
            if (rt_image_read(f.c_str(), &rgb, &t.width, &t.height) != RT_OK) {
                free_textures();
                std::fprintf(stderr, "error: %s\n", rt_last_error());
                return 1;
            }
            t.rgb = rgb;
            texture_rgb.push_back(rgb);
            textures.push_back(t);
            if (!quiet) std::printf("%s: %u x %u texels\n", f.c_str(), t.width, t.height);
        }
        rt_pattern_desc p = {};
        p.kind = RT_PATTERN_IMAGE;
        p.sub_a = cube_mapped ? RT_FACE_FRONT : 0;
        p.sub_b = -1;
        p.reserved = texture_filter;
        for (int q = 0; q < 4; ++q) p.inverse[5 * q] = 1.0;
        patterns.push_back(p);
        if (cube_mapped) maps.push_back({(uint32_t)patterns.size() - 1, RT_MAP_CUBE, {0, 1, 2, 3, 4, 5}});
        else if (texture_map != RT_MAP_PLANAR) maps.push_back({(uint32_t)patterns.size() - 1, texture_map, {-1, -1, -1, -1, -1, -1}});
    }
    if (!obj_paths.empty() || !placements.empty()) {
        rt_material_desc m = {};
        m.color[0] = m.color[1] = m.color[2] = 1.0;
        m.ambient = 0.1;
        m.diffuse = 0.9;
        m.specular = 0.9;
        m.shininess = 200.0;
        m.refractive_index = 1.0;
        m.casts_shadow = 1;
        m.pattern = textured ? (int32_t)patterns.size() - 1 : -1;
        materials.push_back(m);
    }
    // --smooth: the files' vertex normals, as rt_scene_upload_smooth's side list
    std::vector<rt_smooth_desc> smooth_list;
    const uint32_t obj_flags = (smooth ? RT_OBJ_NORMALS : 0u) | (textured ? RT_OBJ_TEXCOORDS : 0u);
    auto add_uvs = [&](const rt_mesh* mesh, uint32_t list, uint32_t first) {
        uint32_t n = 0;
        if (!textured || rt_mesh_uvs(mesh, nullptr, list, &n) != RT_OK || !n) return n;
        const size_t at = uv_list.size();
        uv_list.resize(at + n);
        rt_mesh_uvs(mesh, uv_list.data() + at, list, &n);
        for (size_t k = at; k < uv_list.size(); ++k) uv_list[k].index += first;
        return n;
    };
    auto add_normals = [&](const rt_mesh* mesh, uint32_t list, uint32_t first) {
        uint32_t n = 0;
        if (!smooth || rt_mesh_smooth_normals(mesh, nullptr, 0, nullptr, list, &n) != RT_OK || !n) return n;
        const size_t at = smooth_list.size();
        smooth_list.resize(at + n);
        rt_mesh_smooth_normals(mesh, nullptr, 0, smooth_list.data() + at, list, &n);
        for (size_t k = at; k < smooth_list.size(); ++k) smooth_list[k].index += first;
        return n;
    };
    for (const char* path : obj_paths) {
        rt_mesh* mesh = nullptr;
        rt_mesh_view mv;
        if (rt_mesh_load_obj_ex(path, nullptr, obj_flags, &mesh) != RT_OK || rt_mesh_view_get(mesh, &mv) != RT_OK) {
            std::fprintf(stderr, "error: %s\n", rt_last_error());
            return 1;
        }
        const size_t at = shapes.size();
        shapes.resize(at + mv.n_triangles);
        if (rt_mesh_triangles(mesh, nullptr, 0, (int32_t)materials.size() - 1, shapes.data() + at) != RT_OK) {
            std::fprintf(stderr, "error: %s\n", rt_last_error());
            return 1;
        }
        const uint32_t n_smooth = add_normals(mesh, RT_SMOOTH_SHAPES, (uint32_t)at);
        if (!quiet)
            std::printf("%s: %u vertices, %u triangles, %u lines ignored\n", path, mv.n_vertices, mv.n_triangles,
                        mv.ignored_lines);
        if (!quiet && smooth) std::printf("%s: %u smooth triangles\n", path, n_smooth);
        const uint32_t n_uv = add_uvs(mesh, RT_SMOOTH_SHAPES, (uint32_t)at);
        if (!quiet && textured) std::printf("%s: %u triangles with texture coordinates\n", path, n_uv);
        rt_mesh_free(mesh);
    }
    // --instance: each file's local triangles once, and one (mesh, inverse, material) per placement
    std::map<std::string, uint32_t> mesh_of;
    std::vector<std::vector<rt_shape_desc>> mesh_triangles;
    std::vector<rt_instance_desc> instances;
    for (const Placement& p : placements) {
        auto found = mesh_of.find(p.file);
        if (found == mesh_of.end()) {
            rt_mesh* mesh = nullptr;
            rt_mesh_view mv;
            if (rt_mesh_load_obj_ex(p.file.c_str(), nullptr, obj_flags, &mesh) != RT_OK ||
                rt_mesh_view_get(mesh, &mv) != RT_OK) {
                std::fprintf(stderr, "error: %s\n", rt_last_error());
                return 1;
            }
            std::vector<rt_shape_desc> tri(mv.n_triangles);
            if (rt_mesh_triangles(mesh, nullptr, 0, 0, tri.data()) != RT_OK) {
                std::fprintf(stderr, "error: %s\n", rt_last_error());
                return 1;
            }
            if (!quiet)
                std::printf("%s: %u vertices, %u triangles, %u lines ignored\n", p.file.c_str(), mv.n_vertices,
                            mv.n_triangles, mv.ignored_lines);
            const uint32_t n_smooth = add_normals(mesh, (uint32_t)mesh_triangles.size(), 0u);
            if (!quiet && smooth) std::printf("%s: %u smooth triangles\n", p.file.c_str(), n_smooth);
            const uint32_t n_uv = add_uvs(mesh, (uint32_t)mesh_triangles.size(), 0u);
            if (!quiet && textured) std::printf("%s: %u triangles with texture coordinates\n", p.file.c_str(), n_uv);
            rt_mesh_free(mesh);
            found = mesh_of.emplace(p.file, (uint32_t)mesh_triangles.size()).first;
            mesh_triangles.push_back(std::move(tri));
        }
        // translation(t) * scaling(s, s, s) (transformations.rs), inverted as Shape::set_transformation does
        const double forward[16] = {p.s, 0, 0, p.t[0], 0, p.s, 0, p.t[1], 0, 0, p.s, p.t[2], 0, 0, 0, 1};
        rt_instance_desc d = {};
        d.mesh = found->second;
        d.material = (int32_t)materials.size() - 1;
        rt_matrix_inverse(forward, d.inverse);
        instances.push_back(d);
    }
    std::vector<rt_mesh_desc> meshes;
    for (const auto& tri : mesh_triangles) meshes.push_back({tri.data(), (uint32_t)tri.size(), 0u});
    const double load_ms = ms_since(t_load);
    const auto t_ctx = clk::now();
    rt_context* ctx = nullptr;
    std::vector<int> devices;
    for (int g = 0; g < gpus; ++g) devices.push_back(device + g);
    const int created = gpus > 1 ? rt_context_create_multi(devices.data(), gpus, &ctx) : rt_context_create(device, &ctx);
    const double ctx_ms = ms_since(t_ctx);
    const auto t_up = clk::now();
    if (created != RT_OK ||
        rt_scene_upload_moving(ctx, shapes.data(), (uint32_t)shapes.size(), meshes.data(), (uint32_t)meshes.size(),
                                 instances.data(), (uint32_t)instances.size(), smooth_list.data(),
                                 (uint32_t)smooth_list.size(), uv_list.data(), (uint32_t)uv_list.size(), textures.data(),
                                 (uint32_t)textures.size(), materials.data(), (uint32_t)materials.size(), patterns.data(),
                                 (uint32_t)patterns.size(), v.lights,
                                 v.n_lights, area_lights.data(),
                                 (uint32_t)area_lights.size(), maps.data(),
                                 (uint32_t)maps.size(), motion.data(),
                                 (uint32_t)motion.size()) != RT_OK) {  // (no motion: rt_scene_upload_mapped; no map: rt_scene_upload_lit; no area light: rt_scene_upload_textured; no texture: rt_scene_upload_smooth; no smooth triangle: rt_scene_upload_instanced; no instances: rt_scene_upload)
        free_textures();
        std::fprintf(stderr, "error: %s\n", rt_last_error());
        return 1;
    }
    free_textures();  // (the upload copied the texels)
    // One frame: the default per-scene policy (RT_JIT_AUTO) starts a hipRTC
    // build only at a world's second large frame, so this render never
    // compiles.
    const double upload_ms = ms_since(t_up);
    rt_render_options o = {depth, precision, RT_OUT_U8, 0, 1, 0};
    std::vector<uint8_t> img((size_t)cam.width * cam.height * 3);
    rt_stats st;
    auto t0 = std::chrono::steady_clock::now();
    if ((have_shutter  ? rt_render_shutter(ctx, &cam, &o, samples, have_aperture ? &lens : nullptr, &shutter, img.data(), &st)
         : have_aperture ? rt_render_lens(ctx, &cam, &o, samples, &lens, img.data(), &st)
         : samples > 1 ? rt_render_supersampled(ctx, &cam, &o, samples, img.data(), &st)
                       : rt_render(ctx, &cam, &o, img.data(), &st)) != RT_OK) {
        std::fprintf(stderr, "error: %s\n", rt_last_error());
        return 1;
    }
    double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (timings)  // one-shot cost by phase: the reference times the render call only
        std::printf("timings: load_ms=%.3f context_ms=%.3f upload_ms=%.3f render_ms=%.3f kernel_ms=%.3f\n", load_ms,
                    ctx_ms, upload_ms, s * 1e3, st.kernel_ms);
    if (!quiet) {
        std::printf("Image rendered in: %.3fs\n", s);
        std::printf("kernel %.3f ms on %u GPU(s)\n", st.kernel_ms, st.n_shards ? st.n_shards : 1u);
        const double rays = (double)(st.primary + st.shadow + st.reflect + st.refract);
        std::printf("rays: primary %llu shadow %llu reflect %llu refract %llu (%.1f Mray/s kernel)\n",
                    (unsigned long long)st.primary, (unsigned long long)st.shadow, (unsigned long long)st.reflect,
                    (unsigned long long)st.refract, rays / (st.kernel_ms * 1e3));
    }
    if (rt_image_write_format(out_path, img.data(), cam.width, cam.height,
                              ppm_binary ? RT_IMAGE_PPM_BINARY : RT_IMAGE_AUTO) != RT_OK) {
        std::fprintf(stderr, "error: %s\n", rt_last_error());
        return 1;
    }
    if (!quiet) std::printf("Image saved at %s\n", out_path);
    rt_context_destroy(ctx);
    rt_scene_free(scene);
    return 0;
}
