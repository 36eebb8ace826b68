/*
 * rtc_scene.h — host-side scene input for the render path (C-ABI).
 *
 * Mirrors the reference's scene construction API so a caller can go from the
 * YAML scene files to the descriptor tables rt_scene_upload() takes:
 *   load_scene_description(path) -> (World, Camera)
 *       ray-tracer-cli/src/scene_loader.rs:361-367   -> rt_scene_load_yaml
 *   Camera::new + set_transformation(view_transform(from, to, up))
 *       scene_loader.rs:255-266, camera.rs:25-49/124-127,
 *       transformations.rs:75-87                      -> rt_camera_make
 *   Matrix<4>::inverse  primitives/matrix.rs:247-258  -> rt_matrix_inverse
 *   Canvas::to_png_file / to_ppm_file  canvas.rs:75-137 -> rt_image_write
 *   Color::clamped + u8 cast  canvas.rs:81, 117-123   -> rt_canvas_quantize
 * All arithmetic is f64 and follows the reference's operation order, so the
 * tables are bit-identical to what the reference holds after loading.
 * Pure host code: none of these functions needs a GPU.
 */
#ifndef RTC_SCENE_H
#define RTC_SCENE_H

#include "rtc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_scene rt_scene;

typedef struct rt_scene_view {
    const rt_shape_desc* shapes;
    uint32_t n_shapes;
    const rt_material_desc* materials;
    uint32_t n_materials;
    const rt_pattern_desc* patterns;
    uint32_t n_patterns;
    const rt_light_desc* lights;
    uint32_t n_lights;
    rt_camera_desc camera;
    /* Shapes equal by value to an earlier shape (shape.rs:34-38).  The
     * reference's containers walk identifies shapes by value
     * (intersection.rs:47); rt_scene_upload gives value-equal shapes one
     * identity class so the device walk does the same. */
    uint32_t duplicate_shapes;
} rt_scene_view;

/* load_scene_description (scene_loader.rs:361-367).  RT_ERR_IO on a parse
 * error, with the reason in rt_last_error(). */
int rt_scene_load_yaml(const char* path, rt_scene** out);
int rt_scene_load_yaml_text(const char* text, rt_scene** out);
int rt_scene_view_get(const rt_scene* scene, rt_scene_view* view);
void rt_scene_free(rt_scene* scene);

/* Triangle meshes from Wavefront OBJ text, the book's subset:
 *   v x y z          a vertex;
 *   f i j k ...      a face of three or more vertices, fan-triangulated as
 *                    (1, k, k+1); indices are 1-based, negative ones count
 *                    back from the vertices read so far, and of i/j/k, i//k
 *                    and i/j only the vertex index i is used.
 * Every other line (vn, vt, g, o, s, usemtl, mtllib, comments, blanks) is
 * skipped and counted in ignored_lines.  LF or CRLF.  RT_ERR_IO, with the
 * line number in rt_last_error(), for a number that does not parse or an
 * index out of range on a v or f line, and for a file that cannot be read.
 * The view's pointers live as long as the mesh. */
typedef struct rt_mesh rt_mesh;

typedef struct rt_mesh_view {
    const double* vertices;     /* n_vertices x 3 */
    uint32_t n_vertices;
    const uint32_t* triangles;  /* n_triangles x 3 vertex indices, 0-based */
    uint32_t n_triangles;
    uint32_t ignored_lines;
} rt_mesh_view;

int rt_mesh_load_obj(const char* path, rt_mesh** out);
int rt_mesh_load_obj_text(const char* text, rt_mesh** out);
int rt_mesh_view_get(const rt_mesh* mesh, rt_mesh_view* view);
void rt_mesh_free(rt_mesh* mesh);

/* The mesh's faces as the reference's Triangle::new(v1, v2, v3)
 * (triangle.rs:21-35): edge_1 = v2 - v1, edge_2 = v3 - v1, normal =
 * normalize(edge_2 x edge_1) with Vector::cross's mul_add and
 * Vector::normalized's plain sums, into out[0 .. n_triangles), each with
 * `material`.  transform: a row-major forward 4x4, NULL = identity.
 *   bake = 0  every triangle gets inverse = rt_matrix_inverse(transform)
 *             (Shape::set_transformation);
 *   bake = 1  the vertices are multiplied by `transform` first (Matrix<4> *
 *             Point, matrix.rs:332-346) and the inverse stays the identity:
 *             another, equally valid world that is cheaper per ray.
 * A degenerate face is kept: its normal is NaN and its determinant zero, as
 * the reference's would be.  Host only. */
int rt_mesh_triangles(const rt_mesh* mesh, const double* transform, int bake, int32_t material, rt_shape_desc* out);

/* OBJ vertex normals (smooth triangles: rtc.h rt_scene_upload_smooth).
 * rt_mesh_load_obj_ex reads a file (`path`) or a text (`text`); exactly one of
 * the two is given.  flags = 0 is rt_mesh_load_obj / rt_mesh_load_obj_text.
 * Under RT_OBJ_NORMALS:
 *   vn x y z         a normal, kept as written (not normalized) and not
 *                    counted in ignored_lines;
 *   f i/j/k, i//k    the third index names the vertex's normal: 1-based,
 *                    negative ones count back from the normals read so far.
 * A face is smooth iff every one of its vertices names a normal, otherwise the
 * whole face is flat; the fan (1, k, k+1) carries each vertex's normal with
 * it.  RT_ERR_IO with the line number, each with its own text: a vn with fewer
 * than three numbers, a vn with something that is not a number, a normal
 * index that is no integer, a normal index out of range (or naming a normal
 * not yet read). */
#define RT_OBJ_NORMALS 1u
#define RT_NO_NORMAL 0xFFFFFFFFu
int rt_mesh_load_obj_ex(const char* path, const char* text, uint32_t flags, rt_mesh** out);

typedef struct rt_mesh_normals_view {
    const double* normals;            /* n_normals x 3 */
    uint32_t n_normals;
    uint32_t n_smooth;                /* triangles with three normals */
    const uint32_t* triangle_normals; /* n_triangles x 3, 0-based; RT_NO_NORMAL (0xFFFFFFFF) x 3 for a flat face */
} rt_mesh_normals_view;
/* all zero for a mesh loaded without RT_OBJ_NORMALS */
int rt_mesh_normals_get(const rt_mesh* mesh, rt_mesh_normals_view* view);

/* One rt_smooth_desc per smooth triangle of the mesh, in triangle order, with
 * `list` as given (RT_SMOOTH_SHAPES or a mesh index) and index = the
 * triangle's index in the mesh: the list that pairs with
 * rt_mesh_triangles(mesh, transform, bake, ...) written at the head of that
 * list (a caller that appends the triangles after other shapes adds their
 * count to every index).  bake = 0 writes the file's normals (the triangles' inverse
 * carries the transformation); bake = 1 writes (T^-1)^T n, not normalized:
 * normals map linearly, so the baked world is the same picture up to rounding,
 * as rt_mesh_triangles says of its vertices.  out may be NULL to count;
 * *n_out = the mesh's n_smooth.  Host only. */
int rt_mesh_smooth_normals(const rt_mesh* mesh, const double* transform, int bake, rt_smooth_desc* out,
                           uint32_t list, uint32_t* n_out);

/* OBJ texture coordinates (image textures: rtc.h rt_scene_upload_textured).
 * Under RT_OBJ_TEXCOORDS, which combines with RT_OBJ_NORMALS, rt_mesh_load_obj_ex
 * also reads
 *   vt u v [w]       a texture coordinate (u, v), kept as written (w is checked
 *                    to be a number and dropped) and not counted in
 *                    ignored_lines;
 *   f i/j, i/j/k     the second index names the vertex's coordinate: 1-based,
 *                    negative ones count back from the vt lines read so far.
 * A face has coordinates iff every one of its vertices names one (i and i//k
 * name none); the fan (1, k, k+1) carries each vertex's coordinate with it.
 * RT_ERR_IO with the line number, each with its own text: a vt with fewer than
 * two numbers, a vt with something that is not a number, a texture index that
 * is no integer, a texture index out of range.  Without the flag nothing
 * changes: vt lines are counted in ignored_lines.  The flag is 4, not 2:
 * flags = 2 was the first unknown flag when RT_OBJ_NORMALS came, callers and
 * tests were told it is refused, and it stays refused. */
#define RT_OBJ_TEXCOORDS 4u
#define RT_NO_TEXCOORD 0xFFFFFFFFu
typedef struct rt_mesh_texcoords_view {
    const double* texcoords;            /* n_texcoords x 2 */
    uint32_t n_texcoords;
    uint32_t n_textured;                /* triangles with three coordinates */
    const uint32_t* triangle_texcoords; /* n_triangles x 3, 0-based; RT_NO_TEXCOORD x 3 for a face without */
} rt_mesh_texcoords_view;
/* all zero for a mesh loaded without RT_OBJ_TEXCOORDS */
int rt_mesh_texcoords_get(const rt_mesh* mesh, rt_mesh_texcoords_view* view);
/* One rt_uv_desc per triangle with coordinates, in triangle order, with `list`
 * as given and index = the triangle's index in the mesh, like
 * rt_mesh_smooth_normals.  Coordinates do not transform, so there is no bake.
 * out may be NULL to count; *n_out = the mesh's n_textured.  Host only. */
int rt_mesh_uvs(const rt_mesh* mesh, rt_uv_desc* out, uint32_t list, uint32_t* n_out);

/* Camera::new(width, height, fov) + set_transformation(view_transform(...)) */
int rt_camera_make(uint32_t width, uint32_t height, double field_of_view,
                   const double from[3], const double to[3], const double up[3],
                   rt_camera_desc* out);

/* Re-run Camera::new for a new canvas size, keeping fov and transform —
 * equivalent to editing the YAML camera width/height. */
int rt_camera_resize(rt_camera_desc* camera, uint32_t width, uint32_t height);

/* Camera::set_transformation (camera.rs:124-127): store the inverse of the
 * row-major `transform` and update the origin (camera.rs:114-116). */
int rt_camera_set_transform(rt_camera_desc* camera, const double transform[16]);

/* The inclusive pixel rectangle {x0, y0, x1, y1} of `camera`'s canvas that
 * holds every pixel whose f32 primary ray can pass the kernels' wave cull of
 * a bounding ball `bound` = {centre, radius^2} as the f32 shape table holds
 * it: what a frame's launch hands the per-scene direct kernel for each shape
 * (its primary cull).  The whole canvas where no cull applies (the eye in or
 * beside the ball, radius^2 negative or not finite, a camera transformation
 * that is no similarity); x0 > x1 for a ball behind the camera.  Host only. */
int rt_camera_bound_rect(const rt_camera_desc* camera, const float bound[4], uint32_t rect[4]);

/* The shadow cull of the same kernel, for a wave whose hits all lie on the
 * plane n . x = h (`plane` = {n, h} in f32: row 1 of the plane record's
 * inverse, h negated), a light at `light` and a caster's bounding ball
 * `bound`: the inclusive rectangle {x0, y0, x1, y1} that holds every pixel
 * whose f32 primary ray meets the plane at t > 0, within reach of the light
 * (99, below the distance at which the kernels' shadow cull changes form),
 * and whose shadow ray from the f32 over-point passes the kernels' ball cull
 * of the caster.  The whole canvas where no cull applies; x0 > x1 when
 * the shadow falls off the canvas.  Host only. */
int rt_camera_shadow_rect(const rt_camera_desc* camera, const float plane[4], const float light[3],
                          const float bound[4], uint32_t rect[4]);

/* The pixel columns [span[0], span[2]] and rows [span[1], span[3]] of the
 * canvas in which every primary ray that meets the plane at all meets it
 * within that reach of the light; lo > hi = none.  A frame's launch lets a
 * 16 x 4 pixel block take rt_camera_shadow_rect's answer only when the block
 * lies in those columns or in those rows.  Host only. */
int rt_camera_shadow_near(const rt_camera_desc* camera, const float plane[4], const float light[3], uint32_t span[4]);

/* The primary cull of the same kernel for planes: `planes` holds row 1 of
 * each plane record's f32 inverse, four floats a plane ({n, d}: object
 * y = n . x + d), `n_planes` of them (1 to 8).  The inclusive rectangle
 * {x0, y0, x1, y1} holds every pixel at which plane `q`'s entry can be the
 * nearest of those planes' entries in front of the eye, as the f32 kernel
 * evaluates them; outside it the entry lies behind the eye or another
 * plane's is nearer by a margin no rounding of the kernel's crosses.  The
 * whole canvas where no cull applies; x0 > x1 where the plane is never the
 * nearest.  What a frame's launch works out per plane slot.  Host only. */
int rt_camera_plane_rect(const rt_camera_desc* camera, const float* planes, uint32_t n_planes, uint32_t q,
                         uint32_t rect[4]);

/* Matrix<4>::inverse, row-major 16 doubles. */
int rt_matrix_inverse(const double m[16], double out[16]);

/* Canvas::to_png_file / to_ppm_file (canvas.rs:75-137) for an 8-bit frame
 * (rt_render with RT_OUT_U8, row-major RGB, y = 0 at the top): a path ending
 * in ".png" (any case) gets an RGB8 PNG (filter None, best deflate, as the
 * reference writes), anything else the reference's P3 text byte for byte
 * (canvas.rs:75-97: 5 pixels per line across row boundaries, channels
 * right-aligned to width 3, no trailing newline).  The parent directories
 * are created first (canvas.rs:99-105).  RT_ERR_IO on a write failure.
 * Host only. */
int rt_image_write(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height);

enum {
    RT_IMAGE_AUTO = 0,        /* by extension, as rt_image_write */
    RT_IMAGE_PNG = 1,         /* Canvas::to_png_file */
    RT_IMAGE_PPM = 2,         /* Canvas::to_ppm_file: P3 text, the reference's bytes */
    RT_IMAGE_PPM_BINARY = 3   /* P6 (not in the reference): the same pixels in 1/4 of the bytes */
};
int rt_image_write_format(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height, int format);

/* The canvas's 8-bit quantization on the host (canvas.rs:81, 117-123):
 * round(clamp(c, 0, 1) * 255), half away from zero, NaN -> 0, for f64
 * canvases (the kernels quantize RT_OUT_U8 frames themselves). */
int rt_canvas_quantize(const double* rgb, uint64_t n_channels, uint8_t* out);

#ifdef __cplusplus
}
#endif

#endif /* RTC_SCENE_H */
