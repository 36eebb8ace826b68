"""rtc_amd — MI355X-native render path for the Ray Tracer Challenge world model
of przemo199/ray-tracer-challenge-rs.

Python view of the C-ABI in include/rtc.h / include/rtc_scene.h (librtc.so,
built from ray-tracer-challenge-rs_amd/csrc).  It mirrors the reference's
render API:

    load_scene_description(path)   ray-tracer-cli/src/scene_loader.rs:361-367
    Camera.render / render_parallel ray-tracer/src/composites/camera.rs:79-112
                                   -> Context.render (the GPU arm)
    World.color_at                 ray-tracer/src/composites/world.rs:89-95
                                   -> Context.color_at (batched)

There is no CPU fallback: importing works without a GPU (for the scene
loader and ABI checks), but every call that renders raises RenderError with
RT_ERR_NO_DEVICE when no HIP device is usable, and the module refuses to load
at all when librtc.so is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

__all__ = [
    "RenderError", "lib_path", "abi_version", "device_count", "matrix_inverse", "camera_make",
    "camera_resize", "camera_set_transform", "camera_bound_rect", "camera_plane_rect", "load_scene", "load_scene_text", "SceneTables", "Context", "shard_rows",
    "load_obj", "Mesh", "SmoothDesc", "RT_SMOOTH_SHAPES", "RT_OBJ_NORMALS", "RT_NO_NORMAL",
    "AreaLightDesc", "RT_LIGHT_MAX_STEPS", "RT_JITTER_NONE", "RT_JITTER_HASHED", "area_light_sample",
    "LensDesc", "Lens", "lens_ray",
    "UVMapDesc", "TEXTURE_MAPS", "UVDesc", "TextureDesc", "RT_OBJ_TEXCOORDS", "RT_NO_TEXCOORD", "TEXTURE_FILTERS", "read_image",
    "RT_DEFAULT_MAX_DEPTH", "RT_TILE_H", "RT_TILE_W",
]

RT_ABI_VERSION = 3  # rtc.h; rt_abi_version() must agree (checked at load)
RT_TILE_W = 64
RT_TILE_H = 4
RT_DEFAULT_MAX_DEPTH = 6  # World::MAX_REFLECTION_ITERATIONS, world.rs:15
RT_MAX_SUPPORTED_DEPTH = 16
RT_MAX_SAMPLE_GRID = 4  # rt_render_supersampled*: grid x grid samples per pixel

RT_OK = 0
RT_ERR_INVALID, RT_ERR_HIP, RT_ERR_NO_DEVICE, RT_ERR_NO_SCENE = -1, -2, -3, -4
RT_ERR_OOM, RT_ERR_POOL, RT_ERR_IO, RT_ERR_COMM = -5, -6, -7, -8
STATUS = {0: "RT_OK", -1: "RT_ERR_INVALID", -2: "RT_ERR_HIP", -3: "RT_ERR_NO_DEVICE", -4: "RT_ERR_NO_SCENE",
          -5: "RT_ERR_OOM", -6: "RT_ERR_POOL", -7: "RT_ERR_IO", -8: "RT_ERR_COMM"}
RT_UNIQUE_ID_BYTES = 128
RT_IPC_HANDLE_BYTES = 64
RT_GATHER_RCCL, RT_GATHER_PEER = 0, 1
RT_SMOOTH_SHAPES = 0xFFFFFFFF  # rt_smooth_desc.list: `index` counts the plain shapes
RT_OBJ_NORMALS = 1             # rt_mesh_load_obj_ex: read vn lines and the faces' normal indices
RT_NO_NORMAL = 0xFFFFFFFF      # rt_mesh_normals_view.triangle_normals of a flat face
RT_OBJ_TEXCOORDS = 4           # rt_mesh_load_obj_ex: read vt lines and the faces' texture indices
RT_NO_TEXCOORD = 0xFFFFFFFF    # rt_mesh_texcoords_view.triangle_texcoords of a face without coordinates
TEXTURE_FILTERS = {"nearest": 0, "bilinear": 1}  # rt_pattern_desc.reserved of an image pattern
TEXTURE_MAPS = {"planar": 0, "spherical": 1, "cylindrical": 2, "cube": 3}  # rt_uv_map_desc.map
RT_LIGHT_MAX_STEPS = 16                 # rt_area_light_desc: steps per axis
RT_JITTER_NONE, RT_JITTER_HASHED = 0, 1  # rt_area_light_desc.jitter

SHAPE_KINDS = {"sphere": 0, "plane": 1, "cube": 2, "cylinder": 3, "cone": 4, "triangle": 5}
PATTERN_KINDS = {"stripe": 0, "gradient": 1, "ring": 2, "checker": 3, "complex": 4, "test": 5, "image": 6}
PRECISIONS = {"f32": 0, "f64": 1}
# rt_render_options.flags: diagnostic ablations (rtc.h); never in a parity or bench result
RT_FLAG_NO_COUNTERS, RT_FLAG_NO_SHADE, RT_FLAG_NO_TRACE, RT_FLAG_STAMPS, RT_FLAG_FAIL_LAUNCH = 1, 2, 4, 8, 16
RT_FLAG_GENERATIONS = 32  # count rays per generation (rt_read_generation_counts); pixels unchanged
RT_FLAG_NO_SKIPS = 64  # no shadow-ray skips or cube exit path (acceleration only: pixels and counters unchanged)
RT_JIT_OFF, RT_JIT_SYNC, RT_JIT_AUTO, RT_JIT_EAGER = 0, 1, 2, 3
OUT_FORMATS = {"real": 0, "u8": 1}


class RenderError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{STATUS.get(code, code)}: {message}")
        self.code = code


# ----------------------------------------------------------------- structs
class ShapeDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("material", C.c_int32), ("inverse", C.c_double * 16),
                ("minimum", C.c_double), ("maximum", C.c_double), ("closed", C.c_int32),
                ("reserved", C.c_int32), ("vertex_1", C.c_double * 3), ("edge_1", C.c_double * 3),
                ("edge_2", C.c_double * 3), ("normal", C.c_double * 3)]


class MaterialDesc(C.Structure):
    _fields_ = [("color", C.c_double * 3), ("ambient", C.c_double), ("diffuse", C.c_double),
                ("specular", C.c_double), ("shininess", C.c_double), ("reflectiveness", C.c_double),
                ("transparency", C.c_double), ("refractive_index", C.c_double), ("casts_shadow", C.c_int32),
                ("pattern", C.c_int32)]


class PatternDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("sub_a", C.c_int32), ("sub_b", C.c_int32), ("reserved", C.c_int32),
                ("color_a", C.c_double * 3), ("color_b", C.c_double * 3), ("inverse", C.c_double * 16)]


class LightDesc(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("intensity", C.c_double * 3)]


class CameraDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("field_of_view", C.c_double),
                ("half_width", C.c_double), ("half_height", C.c_double), ("pixel_size", C.c_double),
                ("inverse", C.c_double * 16), ("origin", C.c_double * 3)]

    def copy(self) -> "CameraDesc":
        c = CameraDesc()
        C.pointer(c)[0] = self
        return c


class RenderOptions(C.Structure):
    _fields_ = [("max_depth", C.c_uint32), ("precision", C.c_uint32), ("out_format", C.c_uint32),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32), ("flags", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("primary", C.c_uint64), ("shadow", C.c_uint64), ("reflect", C.c_uint64),
                ("refract", C.c_uint64), ("shaded", C.c_uint64), ("lit_patterned", C.c_uint64),
                ("refract_evals", C.c_uint64), ("schlick_evals", C.c_uint64), ("kernel_ms", C.c_double),
                ("algorithmic_flops", C.c_double), ("gather_ms", C.c_double), ("frame_ms", C.c_double),
                ("n_shards", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["rays"] = self.primary + self.shadow + self.reflect + self.refract
        return d


class RayOptions(C.Structure):
    _fields_ = [("max_depth", C.c_uint32), ("precision", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


# rt_ray_hit_f64 / rt_ray_hit_f32 as numpy records
RAY_HIT_F64 = np.dtype([("t", np.float64), ("shape", np.int32), ("reserved", np.int32)])
RAY_HIT_F32 = np.dtype([("t", np.float32), ("shape", np.int32)])


class GenerationCounts(C.Structure):
    _fields_ = [("traced", C.c_uint64 * (RT_MAX_SUPPORTED_DEPTH + 1)),
                ("shaded", C.c_uint64 * (RT_MAX_SUPPORTED_DEPTH + 1))]


class SceneView(C.Structure):
    _fields_ = [("shapes", C.POINTER(ShapeDesc)), ("n_shapes", C.c_uint32),
                ("materials", C.POINTER(MaterialDesc)), ("n_materials", C.c_uint32),
                ("patterns", C.POINTER(PatternDesc)), ("n_patterns", C.c_uint32),
                ("lights", C.POINTER(LightDesc)), ("n_lights", C.c_uint32),
                ("camera", CameraDesc), ("duplicate_shapes", C.c_uint32)]


class MeshView(C.Structure):
    _fields_ = [("vertices", C.POINTER(C.c_double)), ("n_vertices", C.c_uint32),
                ("triangles", C.POINTER(C.c_uint32)), ("n_triangles", C.c_uint32), ("ignored_lines", C.c_uint32)]


class TreeInfo(C.Structure):
    _fields_ = [("nodes", C.c_uint32), ("leaves", C.c_uint32), ("depth", C.c_uint32),
                ("records_in_tree", C.c_uint32), ("records_outside", C.c_uint32), ("reserved", C.c_uint32),
                ("build_ms", C.c_double)]


class MeshDesc(C.Structure):
    _fields_ = [("triangles", C.POINTER(ShapeDesc)), ("n_triangles", C.c_uint32), ("reserved", C.c_uint32)]


class InstanceDesc(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("material", C.c_int32), ("inverse", C.c_double * 16)]


class InstanceInfo(C.Structure):
    _fields_ = [("meshes", C.c_uint32), ("instances", C.c_uint32), ("expanded", C.c_uint32),
                ("top_depth", C.c_uint32), ("local_records", C.c_uint32), ("local_nodes", C.c_uint32),
                ("instanced_bytes", C.c_uint64), ("expansion_bytes", C.c_uint64), ("build_ms", C.c_double)]


class SmoothDesc(C.Structure):
    _fields_ = [("list", C.c_uint32), ("index", C.c_uint32), ("normal_1", C.c_double * 3),
                ("normal_2", C.c_double * 3), ("normal_3", C.c_double * 3)]


class SmoothInfo(C.Structure):
    _fields_ = [("smooth_triangles", C.c_uint32), ("ran_smooth", C.c_uint32), ("normal_bytes", C.c_uint64)]


class UVDesc(C.Structure):
    _fields_ = [("list", C.c_uint32), ("index", C.c_uint32), ("uv_1", C.c_double * 2), ("uv_2", C.c_double * 2),
                ("uv_3", C.c_double * 2)]


class TextureDesc(C.Structure):
    _fields_ = [("rgb", C.POINTER(C.c_uint8)), ("width", C.c_uint32), ("height", C.c_uint32)]


class TextureInfo(C.Structure):
    _fields_ = [("textured_triangles", C.c_uint32), ("textures", C.c_uint32), ("ran_textured", C.c_uint32),
                ("reserved", C.c_uint32), ("uv_bytes", C.c_uint64), ("texel_bytes", C.c_uint64)]


class AreaLightDesc(C.Structure):
    _fields_ = [("corner", C.c_double * 3), ("full_uvec", C.c_double * 3), ("full_vvec", C.c_double * 3),
                ("intensity", C.c_double * 3), ("usteps", C.c_uint32), ("vsteps", C.c_uint32),
                ("jitter", C.c_uint32), ("seed", C.c_uint32)]


class LensDesc(C.Structure):
    _fields_ = [("aperture", C.c_double), ("focal_distance", C.c_double), ("jitter", C.c_uint32), ("seed", C.c_uint32)]


class LightInfo(C.Structure):
    _fields_ = [("area_lights", C.c_uint32), ("samples", C.c_uint32), ("ran_area", C.c_uint32),
                ("reserved", C.c_uint32), ("area_bytes", C.c_uint64)]


class UVMapDesc(C.Structure):
    _fields_ = [("pattern", C.c_uint32), ("map", C.c_uint32), ("faces", C.c_int32 * 6)]


class MapInfo(C.Structure):
    _fields_ = [("mapped_patterns", C.c_uint32), ("cube_maps", C.c_uint32), ("ran_mapped", C.c_uint32),
                ("reserved", C.c_uint32)]


class MotionDesc(C.Structure):
    _fields_ = [("target", C.c_uint32), ("index", C.c_uint32), ("velocity", C.c_double * 3)]


class ShutterDesc(C.Structure):
    _fields_ = [("open", C.c_double), ("close", C.c_double), ("jitter", C.c_uint32), ("seed", C.c_uint32)]


class MotionInfo(C.Structure):
    _fields_ = [("moving_shapes", C.c_uint32), ("moving_instances", C.c_uint32), ("ran_motion", C.c_uint32),
                ("reserved", C.c_uint32), ("motion_bytes", C.c_uint64)]


RT_MOVE_SHAPE, RT_MOVE_INSTANCE = 0, 1


class MeshTexcoordsView(C.Structure):
    _fields_ = [("texcoords", C.POINTER(C.c_double)), ("n_texcoords", C.c_uint32), ("n_textured", C.c_uint32),
                ("triangle_texcoords", C.POINTER(C.c_uint32))]


class MeshNormalsView(C.Structure):
    _fields_ = [("normals", C.POINTER(C.c_double)), ("n_normals", C.c_uint32), ("n_smooth", C.c_uint32),
                ("triangle_normals", C.POINTER(C.c_uint32))]


# --------------------------------------------------------------- library
_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path() -> str:
    # RTC_LIBRARY: an alternative in-tree build of the same ABI (A/B of build
    # variants, scripts/ab_builds.sh); never a different implementation.
    return os.environ.get("RTC_LIBRARY") or os.path.join(_HERE, "_lib", "librtc.so")


def _load() -> C.CDLL:
    path = lib_path()
    # torch-ROCm bundles its own HIP runtime with the same soname
    # (libamdhip64.so.7) as /opt/rocm's.  Load it first so librtc binds to the
    # SAME runtime: torch streams, events and allocations are then valid
    # handles for the C-ABI (one HIP runtime per process).
    # Kernel arguments in device memory: each wave's first s_load of its
    # arguments then hits HBM/L2 instead of crossing PCIe (measured ~2 us per
    # 1080p frame on MI355X).  Must be set before the HIP runtime starts.
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
    # RTC_NO_TORCH=1: a torch-free host (bench.py's one-shot child, timing
    # what a Rust caller of the C-ABI pays: the HIP runtime starts in
    # rt_context_create); librtc then binds /opt/rocm's runtime on its own.
    if os.environ.get("RTC_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(path):
        raise ImportError(f"rtc_amd: {path} is missing — build it with `python -c 'import __graft_entry__ as g; "
                          f"g.build()'` (hipcc --offload-arch=gfx950)")
    lib = C.CDLL(path)
    P = C.POINTER
    sig = {
        "rt_abi_version": (C.c_int, []),
        "rt_last_error": (C.c_char_p, []),
        "rt_device_count": (C.c_int, [P(C.c_int)]),
        "rt_context_create": (C.c_int, [C.c_int, P(C.c_void_p)]),
        "rt_context_destroy": (C.c_int, [C.c_void_p]),
        "rt_scene_upload": (C.c_int, [C.c_void_p, P(ShapeDesc), C.c_uint32, P(MaterialDesc), C.c_uint32,
                                      P(PatternDesc), C.c_uint32, P(LightDesc), C.c_uint32]),
        "rt_shard_rows": (C.c_int, [C.c_uint32, C.c_uint32, P(C.c_uint32)]),
        "rt_render": (C.c_int, [C.c_void_p, P(CameraDesc), P(RenderOptions), C.c_void_p, P(Stats)]),
        "rt_render_device": (C.c_int, [C.c_void_p, P(CameraDesc), P(RenderOptions), C.c_void_p, C.c_void_p]),
        "rt_render_supersampled": (C.c_int, [C.c_void_p, P(CameraDesc), P(RenderOptions), C.c_uint32, C.c_void_p,
                                             P(Stats)]),
        "rt_render_supersampled_device": (C.c_int, [C.c_void_p, P(CameraDesc), P(RenderOptions), C.c_uint32,
                                                    C.c_void_p, C.c_void_p]),
        "rt_color_at": (C.c_int, [C.c_void_p, P(C.c_double), C.c_uint64, C.c_uint32, C.c_uint32, P(C.c_double),
                                  P(Stats)]),
        "rt_trace_rays_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, P(RayOptions), C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
        "rt_trace_rays": (C.c_int, [C.c_void_p, P(C.c_double), C.c_uint64, P(RayOptions), P(C.c_double), C.c_void_p,
                                    P(Stats)]),
        "rt_read_counters": (C.c_int, [C.c_void_p, P(Stats)]),
        "rt_read_generation_counts": (C.c_int, [C.c_void_p, P(GenerationCounts)]),
        "rt_debug_stamps": (C.c_int, [C.c_void_p, P(C.c_uint64), C.c_uint32, P(C.c_uint32)]),
        "rt_debug_tile_costs": (C.c_int, [C.c_void_p, P(C.c_uint32), C.c_uint32, P(C.c_uint32)]),
        "rt_debug_item_log": (C.c_int, [C.c_void_p, P(C.c_uint64), C.c_uint32, P(C.c_uint32)]),
        "rt_assemble_shards": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p]),
        "rt_scene_load_yaml": (C.c_int, [C.c_char_p, P(C.c_void_p)]),
        "rt_scene_load_yaml_text": (C.c_int, [C.c_char_p, P(C.c_void_p)]),
        "rt_scene_view_get": (C.c_int, [C.c_void_p, P(SceneView)]),
        "rt_scene_free": (None, [C.c_void_p]),
        "rt_mesh_load_obj": (C.c_int, [C.c_char_p, P(C.c_void_p)]),
        "rt_mesh_load_obj_text": (C.c_int, [C.c_char_p, P(C.c_void_p)]),
        "rt_mesh_view_get": (C.c_int, [C.c_void_p, P(MeshView)]),
        "rt_mesh_free": (None, [C.c_void_p]),
        "rt_mesh_triangles": (C.c_int, [C.c_void_p, P(C.c_double), C.c_int, C.c_int32, P(ShapeDesc)]),
        "rt_scene_tree_info": (C.c_int, [C.c_void_p, P(TreeInfo)]),
        "rt_scene_upload_instanced": (C.c_int, [C.c_void_p, P(ShapeDesc), C.c_uint32, P(MeshDesc), C.c_uint32,
                                                P(InstanceDesc), C.c_uint32, P(MaterialDesc), C.c_uint32,
                                                P(PatternDesc), C.c_uint32, P(LightDesc), C.c_uint32]),
        "rt_instances_expand": (C.c_int, [P(ShapeDesc), C.c_uint32, P(MeshDesc), C.c_uint32, P(InstanceDesc),
                                          C.c_uint32, P(ShapeDesc)]),
        "rt_scene_instance_info": (C.c_int, [C.c_void_p, P(InstanceInfo)]),
        "rt_scene_upload_smooth": (C.c_int, [C.c_void_p, P(ShapeDesc), C.c_uint32, P(MeshDesc), C.c_uint32,
                                             P(InstanceDesc), C.c_uint32, P(SmoothDesc), C.c_uint32,
                                             P(MaterialDesc), C.c_uint32, P(PatternDesc), C.c_uint32, P(LightDesc),
                                             C.c_uint32]),
        "rt_smooth_expand": (C.c_int, [P(ShapeDesc), C.c_uint32, P(MeshDesc), C.c_uint32, P(InstanceDesc), C.c_uint32,
                                       P(SmoothDesc), C.c_uint32, P(SmoothDesc), P(C.c_uint32)]),
        "rt_scene_smooth_info": (C.c_int, [C.c_void_p, P(SmoothInfo)]),
        "rt_mesh_load_obj_ex": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint32, P(C.c_void_p)]),
        "rt_mesh_normals_get": (C.c_int, [C.c_void_p, P(MeshNormalsView)]),
        "rt_mesh_smooth_normals": (C.c_int, [C.c_void_p, P(C.c_double), C.c_int, P(SmoothDesc), C.c_uint32,
                                             P(C.c_uint32)]),
        "rt_scene_upload_textured": (C.c_int, [C.c_void_p, P(ShapeDesc), C.c_uint32, P(MeshDesc), C.c_uint32,
                                               P(InstanceDesc), C.c_uint32, P(SmoothDesc), C.c_uint32, P(UVDesc),
                                               C.c_uint32, P(TextureDesc), C.c_uint32, P(MaterialDesc), C.c_uint32,
                                               P(PatternDesc), C.c_uint32, P(LightDesc), C.c_uint32]),
        "rt_uv_expand": (C.c_int, [P(ShapeDesc), C.c_uint32, P(MeshDesc), C.c_uint32, P(InstanceDesc), C.c_uint32,
                                   P(UVDesc), C.c_uint32, P(UVDesc), P(C.c_uint32)]),
        "rt_scene_texture_info": (C.c_int, [C.c_void_p, P(TextureInfo)]),
        "rt_scene_upload_lit": (C.c_int, [C.c_void_p, P(ShapeDesc), C.c_uint32, P(MeshDesc), C.c_uint32,
                                          P(InstanceDesc), C.c_uint32, P(SmoothDesc), C.c_uint32, P(UVDesc),
                                          C.c_uint32, P(TextureDesc), C.c_uint32, P(MaterialDesc), C.c_uint32,
                                          P(PatternDesc), C.c_uint32, P(LightDesc), C.c_uint32, P(AreaLightDesc),
                                          C.c_uint32]),
        "rt_scene_upload_mapped": (C.c_int, [C.c_void_p, P(ShapeDesc), C.c_uint32, P(MeshDesc), C.c_uint32,
                                             P(InstanceDesc), C.c_uint32, P(SmoothDesc), C.c_uint32, P(UVDesc),
                                             C.c_uint32, P(TextureDesc), C.c_uint32, P(MaterialDesc), C.c_uint32,
                                             P(PatternDesc), C.c_uint32, P(LightDesc), C.c_uint32, P(AreaLightDesc),
                                             C.c_uint32, P(UVMapDesc), C.c_uint32]),
        "rt_scene_map_info": (C.c_int, [C.c_void_p, P(MapInfo)]),
        "rt_scene_upload_moving": (C.c_int, [C.c_void_p, P(ShapeDesc), C.c_uint32, P(MeshDesc), C.c_uint32,
                                             P(InstanceDesc), C.c_uint32, P(SmoothDesc), C.c_uint32, P(UVDesc),
                                             C.c_uint32, P(TextureDesc), C.c_uint32, P(MaterialDesc), C.c_uint32,
                                             P(PatternDesc), C.c_uint32, P(LightDesc), C.c_uint32, P(AreaLightDesc),
                                             C.c_uint32, P(UVMapDesc), C.c_uint32, P(MotionDesc), C.c_uint32]),
        "rt_scene_motion_info": (C.c_int, [C.c_void_p, P(MotionInfo)]),
        "rt_motion_displace": (C.c_int, [P(ShapeDesc), C.c_uint32, P(InstanceDesc), C.c_uint32, P(MotionDesc),
                                         C.c_uint32, C.c_double, P(ShapeDesc), P(InstanceDesc)]),
        "rt_render_shutter": (C.c_int, [C.c_void_p, P(CameraDesc), P(RenderOptions), C.c_uint32, P(LensDesc),
                                        P(ShutterDesc), C.c_void_p, P(Stats)]),
        "rt_render_shutter_device": (C.c_int, [C.c_void_p, P(CameraDesc), P(RenderOptions), C.c_uint32, P(LensDesc),
                                               P(ShutterDesc), C.c_void_p, C.c_void_p]),
        "rt_shutter_time": (C.c_int, [P(CameraDesc), C.c_uint32, P(ShutterDesc), C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_uint32, P(C.c_double)]),
        "rt_trace_rays_timed": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double), C.c_uint64, P(RayOptions),
                                          P(C.c_double), C.c_void_p, P(Stats)]),
        "rt_trace_rays_timed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, P(RayOptions),
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
        "rt_lights_expand": (C.c_int, [P(LightDesc), C.c_uint32, P(AreaLightDesc), C.c_uint32, P(LightDesc),
                                       P(C.c_uint32)]),
        "rt_render_lens": (C.c_int, [C.c_void_p, P(CameraDesc), P(RenderOptions), C.c_uint32, P(LensDesc), C.c_void_p,
                                     P(Stats)]),
        "rt_render_lens_device": (C.c_int, [C.c_void_p, P(CameraDesc), P(RenderOptions), C.c_uint32, P(LensDesc),
                                            C.c_void_p, C.c_void_p]),
        "rt_lens_ray": (C.c_int, [P(CameraDesc), C.c_uint32, P(LensDesc), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                  P(C.c_double)]),
        "rt_area_light_sample": (C.c_int, [P(AreaLightDesc), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                           P(C.c_double)]),
        "rt_scene_light_info": (C.c_int, [C.c_void_p, P(LightInfo)]),
        "rt_mesh_texcoords_get": (C.c_int, [C.c_void_p, P(MeshTexcoordsView)]),
        "rt_mesh_uvs": (C.c_int, [C.c_void_p, P(UVDesc), C.c_uint32, P(C.c_uint32)]),
        "rt_image_read": (C.c_int, [C.c_char_p, P(P(C.c_uint8)), P(C.c_uint32), P(C.c_uint32)]),
        "rt_image_free": (None, [P(C.c_uint8)]),
        "rt_image_write": (C.c_int, [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]),
        "rt_image_write_format": (C.c_int, [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]),
        "rt_canvas_quantize": (C.c_int, [P(C.c_double), C.c_uint64, P(C.c_uint8)]),
        "rt_camera_make": (C.c_int, [C.c_uint32, C.c_uint32, C.c_double, P(C.c_double), P(C.c_double),
                                     P(C.c_double), P(CameraDesc)]),
        "rt_camera_resize": (C.c_int, [P(CameraDesc), C.c_uint32, C.c_uint32]),
        "rt_camera_bound_rect": (C.c_int, [P(CameraDesc), P(C.c_float), P(C.c_uint32)]),
        "rt_camera_shadow_rect": (C.c_int, [P(CameraDesc), P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_uint32)]),
        "rt_camera_shadow_near": (C.c_int, [P(CameraDesc), P(C.c_float), P(C.c_float), P(C.c_uint32)]),
        "rt_camera_plane_rect": (C.c_int, [P(CameraDesc), P(C.c_float), C.c_uint32, C.c_uint32, P(C.c_uint32)]),
        "rt_matrix_inverse": (C.c_int, [P(C.c_double), P(C.c_double)]),
        "rt_camera_set_transform": (C.c_int, [P(CameraDesc), P(C.c_double)]),
        "rt_shard_row_map": (C.c_int, [C.c_uint32, C.c_uint32, P(C.c_uint32), P(C.c_uint32)]),
        "rt_context_create_multi": (C.c_int, [P(C.c_int), C.c_int, P(C.c_void_p)]),
        "rt_comm_unique_id": (C.c_int, [P(C.c_uint8)]),
        "rt_context_create_rank": (C.c_int, [C.c_int, C.c_int, C.c_int, P(C.c_uint8), P(C.c_void_p)]),
        "rt_context_group": (C.c_int, [C.c_void_p, P(C.c_int), P(C.c_int), P(C.c_int)]),
        "rt_context_set_jit": (C.c_int, [C.c_void_p, C.c_int]),
        "rt_context_set_frames_in_flight": (C.c_int, [C.c_void_p, C.c_uint32]),
        "rt_jit_status": (C.c_int, [C.c_void_p, P(C.c_int), P(C.c_double), C.c_char_p, C.c_size_t]),
        "rt_jit_wait": (C.c_int, [C.c_void_p, C.c_double, P(C.c_int)]),
        "rt_canvas_create": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, P(C.c_void_p), P(C.c_uint8)]),
        "rt_canvas_open": (C.c_int, [C.c_void_p, P(C.c_uint8), C.c_uint64, C.c_uint32, P(C.c_void_p)]),
        "rt_canvas_close": (C.c_int, [C.c_void_p, C.c_void_p]),
        "rt_render_to_canvas": (C.c_int, [C.c_void_p, P(CameraDesc), P(RenderOptions), C.c_void_p, C.c_uint64,
                                          C.c_double, C.c_void_p]),
        "rt_canvas_wait": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_void_p]),
        "rt_canvas_release": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
        "rt_canvas_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
        "rt_context_set_gather": (C.c_int, [C.c_void_p, C.c_int]),
        "rt_debug_intersect": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_double), C.c_uint64, C.c_uint32, C.c_uint32,
                                         P(C.c_double)]),
        "rt_debug_normal": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_double), C.c_uint64, C.c_uint32, C.c_uint32,
                                      P(C.c_double)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.rt_abi_version() != RT_ABI_VERSION:
        raise ImportError(f"rtc_amd: {path} has ABI {lib.rt_abi_version()}, this module expects {RT_ABI_VERSION}")
    return lib


_lib = _load()

# Every symbol include/rtc.h and include/rtc_scene.h declare (checked by tests).
EXPORTED_SYMBOLS = (
    "rt_abi_version", "rt_last_error", "rt_device_count", "rt_context_create", "rt_context_destroy",
    "rt_scene_upload", "rt_shard_rows", "rt_render", "rt_render_device", "rt_color_at", "rt_read_counters",
    "rt_trace_rays", "rt_trace_rays_device", "rt_render_supersampled", "rt_render_supersampled_device",
    "rt_read_generation_counts",
    "rt_debug_stamps", "rt_debug_tile_costs", "rt_debug_item_log", "rt_debug_intersect", "rt_debug_normal", "rt_camera_set_transform",
    "rt_shard_row_map", "rt_context_create_multi", "rt_comm_unique_id", "rt_context_create_rank", "rt_context_group",
    "rt_context_set_jit", "rt_context_set_frames_in_flight", "rt_jit_status", "rt_jit_wait", "rt_canvas_create", "rt_canvas_open", "rt_canvas_close",
    "rt_render_to_canvas", "rt_canvas_wait", "rt_canvas_release", "rt_canvas_read", "rt_context_set_gather",
    "rt_assemble_shards", "rt_scene_load_yaml", "rt_scene_load_yaml_text", "rt_scene_view_get", "rt_scene_free",
    "rt_camera_make", "rt_camera_resize", "rt_camera_bound_rect", "rt_camera_shadow_rect", "rt_camera_shadow_near",
    "rt_camera_plane_rect", "rt_matrix_inverse", "rt_image_write", "rt_image_write_format",
    "rt_canvas_quantize",
    "rt_mesh_load_obj", "rt_mesh_load_obj_text", "rt_mesh_view_get", "rt_mesh_free", "rt_mesh_triangles",
    "rt_scene_tree_info",
    "rt_scene_upload_instanced", "rt_instances_expand", "rt_scene_instance_info",
    "rt_scene_upload_smooth", "rt_smooth_expand", "rt_scene_smooth_info",
    "rt_mesh_load_obj_ex", "rt_mesh_normals_get", "rt_mesh_smooth_normals",
    "rt_scene_upload_textured", "rt_uv_expand", "rt_scene_texture_info", "rt_mesh_texcoords_get", "rt_mesh_uvs",
    "rt_image_read", "rt_image_free",
    "rt_scene_upload_lit", "rt_lights_expand", "rt_area_light_sample", "rt_scene_light_info",
    "rt_render_lens", "rt_render_lens_device", "rt_lens_ray",
    "rt_scene_upload_mapped", "rt_scene_map_info",
    "rt_scene_upload_moving", "rt_scene_motion_info", "rt_motion_displace", "rt_render_shutter",
    "rt_render_shutter_device", "rt_shutter_time", "rt_trace_rays_timed", "rt_trace_rays_timed_device",
)


def _check(rc: int) -> None:
    if rc != RT_OK:
        raise RenderError(rc, _lib.rt_last_error().decode(errors="replace"))


def abi_version() -> int:
    return _lib.rt_abi_version()


def device_count() -> int:
    n = C.c_int(0)
    _check(_lib.rt_device_count(C.byref(n)))
    return n.value


def matrix_inverse(m) -> np.ndarray:
    """Matrix<4>::inverse (matrix.rs:247-258) on 16 row-major f64."""
    a = (C.c_double * 16)(*np.asarray(m, dtype=np.float64).reshape(16))
    out = (C.c_double * 16)()
    _check(_lib.rt_matrix_inverse(a, out))
    return np.array(out[:], dtype=np.float64).reshape(4, 4)


def camera_make(width: int, height: int, fov: float, frm, to, up) -> CameraDesc:
    """Camera::new + set_transformation(view_transform(from, to, up))."""
    cam = CameraDesc()
    v = lambda x: (C.c_double * 3)(*[float(t) for t in x])  # noqa: E731
    _check(_lib.rt_camera_make(width, height, float(fov), v(frm), v(to), v(up), C.byref(cam)))
    return cam


def camera_set_transform(cam: CameraDesc, transform) -> CameraDesc:
    """Camera::set_transformation (camera.rs:124-127) on a copy: inverse + origin."""
    c = cam.copy()
    t = (C.c_double * 16)(*np.asarray(transform, dtype=np.float64).reshape(16))
    _check(_lib.rt_camera_set_transform(C.byref(c), t))
    return c


def camera_resize(cam: CameraDesc, width: int, height: int) -> CameraDesc:
    """Camera::new for another canvas size, same fov/transform (= editing YAML width/height)."""
    c = cam.copy()
    _check(_lib.rt_camera_resize(C.byref(c), width, height))
    return c


def camera_bound_rect(cam: CameraDesc, bound) -> tuple:
    """(x0, y0, x1, y1), inclusive: the pixels of `cam` whose primary rays can pass the wave cull of the
    bounding ball `bound` = (centre, radius^2) in f32; x0 > x1 = none (rt_camera_bound_rect)."""
    b = (C.c_float * 4)(*np.asarray(bound, dtype=np.float32).reshape(4))
    r = (C.c_uint32 * 4)()
    _check(_lib.rt_camera_bound_rect(C.byref(cam), b, r))
    return tuple(r[:])


def _f32s(values, n):
    return (C.c_float * n)(*np.asarray(values, dtype=np.float32).reshape(n))


def camera_shadow_rect(cam: CameraDesc, plane, light, bound) -> tuple:
    """(x0, y0, x1, y1), inclusive: the pixels of `cam` that meet the plane `plane` = (n, h), n . x = h, within
    reach of `light` and whose shadow rays can pass the wave cull of the caster's ball `bound` = (centre,
    radius^2), all in f32; x0 > x1 = none (rt_camera_shadow_rect)."""
    r = (C.c_uint32 * 4)()
    _check(_lib.rt_camera_shadow_rect(C.byref(cam), _f32s(plane, 4), _f32s(light, 3), _f32s(bound, 4), r))
    return tuple(r[:])


def camera_shadow_near(cam: CameraDesc, plane, light) -> tuple:
    """(x0, y0, x1, y1): the columns x0..x1 and the rows y0..y1 of `cam` whose every hit on `plane` lies within
    reach of `light`; lo > hi = none (rt_camera_shadow_near)."""
    r = (C.c_uint32 * 4)()
    _check(_lib.rt_camera_shadow_near(C.byref(cam), _f32s(plane, 4), _f32s(light, 3), r))
    return tuple(r[:])


def camera_plane_rect(cam: CameraDesc, planes, q: int) -> tuple:
    """(x0, y0, x1, y1), inclusive: the pixels of `cam` at which plane `q` of `planes` (row 1 of each record's f32
    inverse, shape (n, 4)) can be the nearest plane in front of the eye; x0 > x1 = none (rt_camera_plane_rect)."""
    rows = np.ascontiguousarray(planes, dtype=np.float32).reshape(-1, 4)
    r = (C.c_uint32 * 4)()
    _check(_lib.rt_camera_plane_rect(C.byref(cam), _f32s(rows, rows.size), rows.shape[0], int(q), r))
    return tuple(r[:])


IMAGE_FORMATS = {"auto": 0, "png": 1, "ppm": 2, "ppm-binary": 3}


def write_image(path, image: np.ndarray, fmt: str = "auto") -> None:
    """Canvas::to_png_file / to_ppm_file (canvas.rs:75-137) of an 8-bit (H, W, 3) frame
    (render(..., out_format="u8")): PNG when `path` ends in .png, the reference's P3
    text otherwise; fmt "ppm-binary" writes P6 instead (an opt-in, not the reference's)."""
    img = np.ascontiguousarray(image)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("write_image takes a uint8 array of shape (H, W, 3)")
    _check(_lib.rt_image_write_format(os.fsencode(path), img.ctypes.data if img.size else None, img.shape[1],
                                      img.shape[0], IMAGE_FORMATS[fmt]))


def read_image(path) -> np.ndarray:
    """rt_image_read: a PPM (P3, P6) or PNG (8-bit RGB / RGBA, alpha dropped) file as a uint8 array of shape
    (H, W, 3), row 0 at the top: what world.image_pattern takes."""
    rgb, w, h = C.POINTER(C.c_uint8)(), C.c_uint32(0), C.c_uint32(0)
    _check(_lib.rt_image_read(os.fsencode(path), C.byref(rgb), C.byref(w), C.byref(h)))
    try:
        return np.ctypeslib.as_array(rgb, (h.value, w.value, 3)).copy()
    finally:
        _lib.rt_image_free(rgb)


def Lens(aperture: float, focal_distance: float, jitter: bool = False, seed: int = 0) -> "LensDesc":
    """A thin lens (rtc.h rt_lens_desc): its radius and the focal plane's distance along the view axis, both in
    camera space; jitter False = cell centres (RT_JITTER_NONE), True = hashed per sample with `seed`."""
    return LensDesc(float(aperture), float(focal_distance), RT_JITTER_HASHED if jitter else RT_JITTER_NONE,
                    int(seed) & 0xFFFFFFFF)


def lens_ray(camera: "CameraDesc", grid: int, lens: "LensDesc", x: int, y: int, i: int, j: int) -> np.ndarray:
    """rt_lens_ray: the f64 ray (origin, direction) of sample (i, j) of pixel (x, y) of a lens frame of the
    output camera `camera`, for either jitter mode."""
    ray = (C.c_double * 6)()
    _check(_lib.rt_lens_ray(C.byref(camera), grid, C.byref(lens), x, y, i, j, ray))
    return np.array(ray[:], dtype=np.float64)


def Shutter(open: float, close: float, jitter: bool = False, seed: int = 0) -> "ShutterDesc":
    """A shutter (rtc.h rt_shutter_desc): the interval of time a frame's samples spread over; jitter False =
    cell centres (RT_JITTER_NONE), True = hashed per sample with `seed`."""
    return ShutterDesc(float(open), float(close), RT_JITTER_HASHED if jitter else RT_JITTER_NONE,
                       int(seed) & 0xFFFFFFFF)


def shutter_time(camera: "CameraDesc", grid: int, shutter: "ShutterDesc", x: int, y: int, i: int, j: int) -> float:
    """rt_shutter_time: the f64 time of sample (i, j) of pixel (x, y) of a shutter frame of the output camera
    `camera`, for either jitter mode."""
    tau = C.c_double(0.0)
    _check(_lib.rt_shutter_time(C.byref(camera), grid, None if shutter is None else C.byref(shutter), x, y, i, j,
                                C.byref(tau)))
    return tau.value


def area_light_sample(desc: "AreaLightDesc", area_index: int, ray_id: int, remaining: int, k: int) -> np.ndarray:
    """rt_area_light_sample: the f64 position of sample k of an area light, for either jitter mode."""
    pos = (C.c_double * 3)()
    _check(_lib.rt_area_light_sample(C.byref(desc), area_index, ray_id, remaining, k, pos))
    return np.array(pos[:], dtype=np.float64)


def canvas_quantize(image: np.ndarray) -> np.ndarray:
    """canvas.rs:81, 117-123 on the host: round(clamp(c, 0, 1) * 255) as u8 of an f64 canvas."""
    src = np.ascontiguousarray(image, dtype=np.float64)
    out = np.zeros(src.shape, dtype=np.uint8)
    _check(_lib.rt_canvas_quantize(src.ctypes.data_as(C.POINTER(C.c_double)), src.size,
                                   out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


def shard_rows(height: int, shard_count: int) -> int:
    r = C.c_uint32(0)
    _check(_lib.rt_shard_rows(height, shard_count, C.byref(r)))
    return r.value


def shard_row_map(height: int, shard_count: int):
    """(shard, strip row) of every image row (rtc.h rt_shard_row_map; host only)."""
    shard = np.zeros(height, dtype=np.uint32)
    row = np.zeros(height, dtype=np.uint32)
    _check(_lib.rt_shard_row_map(height, shard_count, shard.ctypes.data_as(C.POINTER(C.c_uint32)),
                                 row.ctypes.data_as(C.POINTER(C.c_uint32))))
    return shard, row


def comm_unique_id() -> bytes:
    """RCCL unique id for rt_context_create_rank (rank 0 makes it, the caller shares it)."""
    buf = (C.c_uint8 * RT_UNIQUE_ID_BYTES)()
    _check(_lib.rt_comm_unique_id(buf))
    return bytes(buf)


@dataclass
class SceneTables:
    """Flattened world: the POD tables rt_scene_upload takes, plus the camera."""
    shapes: C.Array
    materials: C.Array
    patterns: C.Array
    lights: C.Array
    camera: CameraDesc
    duplicate_shapes: int = 0
    # Mesh instances (rtc.h rt_scene_upload_instanced): each mesh an array of ShapeDesc (local triangles,
    # identity inverse) and an array of InstanceDesc; None / empty = a plain world.
    meshes: list | None = None
    instances: C.Array | None = None
    # Smooth triangles (rtc.h rt_scene_upload_smooth): an array of SmoothDesc naming triangles of `shapes`
    # (list = RT_SMOOTH_SHAPES) or of a mesh, with their three vertex normals; None / empty = none.
    smooth: C.Array | None = None
    # Image textures (rtc.h rt_scene_upload_textured): an array of UVDesc naming triangles like `smooth` with
    # their three texture coordinates, and the textures image patterns index (pattern.sub_a): uint8 arrays
    # of shape (H, W, 3); None / empty = none.
    uvs: C.Array | None = None
    textures: list | None = None
    # Area lights (rtc.h rt_scene_upload_lit): an array of AreaLightDesc; None / empty = none.
    area_lights: C.Array | None = None
    # Texture maps (rtc.h rt_scene_upload_mapped): an array of UVMapDesc naming image patterns with their map
    # and a cube map's six textures; None / empty = every image pattern is planar.
    maps: C.Array | None = None
    # Motion (rtc.h rt_scene_upload_moving): an array of MotionDesc naming shapes of `shapes` (RT_MOVE_SHAPE)
    # or instances (RT_MOVE_INSTANCE) with their velocities; None / empty = nothing moves.
    motion: C.Array | None = None

    @property
    def moving(self) -> bool:
        return self.motion is not None and len(self.motion) > 0

    def moving_args(self):
        """rt_scene_upload_moving's arguments after the context: mapped_args() with the motion list at the end."""
        mo = self.motion if self.motion is not None else (MotionDesc * 0)()
        return self.mapped_args() + (mo, len(mo))

    def at_time(self, tau: float) -> "SceneTables":
        """The static world at time tau (rt_motion_displace): every moving shape's and instance's inverse
        becomes inverse * translation(-v tau); the other tables are shared and the result has no motion list.
        A world without one: itself."""
        if not self.moving:
            return self
        inst = self.instances if self.instances is not None else (InstanceDesc * 0)()
        shapes = (ShapeDesc * len(self.shapes))()
        out_inst = (InstanceDesc * len(inst))()
        _check(_lib.rt_motion_displace(self.shapes, len(self.shapes), inst, len(inst), self.motion, len(self.motion),
                                       float(tau), shapes, out_inst))
        return SceneTables(shapes, self.materials, self.patterns, self.lights, self.camera, self.duplicate_shapes,
                           meshes=self.meshes, instances=out_inst if len(inst) else self.instances,
                           smooth=self.smooth, uvs=self.uvs, textures=self.textures, area_lights=self.area_lights,
                           maps=self.maps)

    @property
    def mapped(self) -> bool:
        return self.maps is not None and len(self.maps) > 0

    def mapped_args(self):
        """rt_scene_upload_mapped's arguments after the context: lit_args() with the map list at the end."""
        mp = self.maps if self.maps is not None else (UVMapDesc * 0)()
        return self.lit_args() + (mp, len(mp))

    @property
    def lit(self) -> bool:
        return self.area_lights is not None and len(self.area_lights) > 0

    def lit_args(self):
        """rt_scene_upload_lit's arguments after the context: textured_args() with the area list at the end."""
        al = self.area_lights if self.area_lights is not None else (AreaLightDesc * 0)()
        return self.textured_args() + (al, len(al))

    def expanded_lights(self):
        """The light list the world means (rt_lights_expand): the point lights, then every area light's
        samples as point lights of intensity / N.  A hashed light has no expansion (RenderError)."""
        if not self.lit:
            return self.lights
        n = C.c_uint32(0)
        a = (self.lights, len(self.lights), self.area_lights, len(self.area_lights))
        _check(_lib.rt_lights_expand(*a, None, C.byref(n)))
        out = (LightDesc * n.value)()
        _check(_lib.rt_lights_expand(*a, out, C.byref(n)))
        return out

    @property
    def textured(self) -> bool:
        return (self.uvs is not None and len(self.uvs) > 0) or bool(self.textures) or \
            any(p.kind == PATTERN_KINDS["image"] for p in self.patterns)

    def texture_descs(self):
        """The TextureDesc array over `textures` (it borrows their memory: keep the tables alive)."""
        tex = [np.ascontiguousarray(t, dtype=np.uint8) for t in (self.textures or [])]
        arr = (TextureDesc * len(tex))()
        for i, t in enumerate(tex):
            if t.ndim != 3 or t.shape[2] != 3:
                raise ValueError("a texture is a uint8 array of shape (H, W, 3)")
            arr[i].rgb = t.ctypes.data_as(C.POINTER(C.c_uint8))
            arr[i].width, arr[i].height = t.shape[1], t.shape[0]
        arr._keep = tex
        return arr

    def textured_args(self):
        """rt_scene_upload_textured's arguments after the context: smooth_args() with the coordinate list
        and the texture list after the smooth list."""
        a = self.smooth_args()
        uv = self.uvs if self.uvs is not None else (UVDesc * 0)()
        td = self.texture_descs()
        return a[:8] + (uv, len(uv), td, len(td)) + a[8:]

    @property
    def instanced(self) -> bool:
        return self.instances is not None and len(self.instances) > 0

    @property
    def smoothed(self) -> bool:
        return self.smooth is not None and len(self.smooth) > 0

    def smooth_args(self):
        """rt_scene_upload_smooth's arguments after the context: instanced_args() with the smooth list
        after the instances."""
        a = self.instanced_args()
        sm = self.smooth if self.smooth is not None else (SmoothDesc * 0)()
        return a[:6] + (sm, len(sm)) + a[6:]

    def mesh_descs(self):
        """The MeshDesc array over `meshes` (it borrows their memory: keep the tables alive)."""
        meshes = self.meshes or []
        arr = (MeshDesc * len(meshes))()
        for i, m in enumerate(meshes):
            arr[i].triangles = C.cast(m, C.POINTER(ShapeDesc))
            arr[i].n_triangles = len(m)
        return arr

    def instanced_args(self):
        """(shapes, n, meshes, n, instances, n, materials, n, patterns, n, lights, n) for C calls."""
        inst = self.instances if self.instances is not None else (InstanceDesc * 0)()
        md = self.mesh_descs()
        return (self.shapes, len(self.shapes), md, len(md), inst, len(inst), self.materials, len(self.materials),
                self.patterns, len(self.patterns), self.lights, len(self.lights))

    def expanded(self) -> "SceneTables":
        """The flat world an instanced one means (rt_instances_expand): the shapes, then every instance's
        triangles with its inverse and material; the other tables are shared.  A plain world: itself.
        A smooth list is expanded with it (rt_smooth_expand): every entry then names a world index.
        Area lights are expanded too (rt_lights_expand): the result holds point lights only."""
        if not self.instanced:
            if not self.lit:
                return self
            return SceneTables(self.shapes, self.materials, self.patterns, self.expanded_lights(), self.camera,
                               self.duplicate_shapes, smooth=self.smooth, uvs=self.uvs, textures=self.textures,
                               maps=self.maps)
        md, inst = self.mesh_descs(), self.instances
        total = len(self.shapes) + sum(len(self.meshes[i.mesh]) for i in inst if i.mesh < len(self.meshes))
        out = (ShapeDesc * total)()
        _check(_lib.rt_instances_expand(self.shapes, len(self.shapes), md, len(md), inst, len(inst), out))
        smooth = None
        if self.smoothed:
            n = C.c_uint32(0)
            a = self.smooth_args()[:8]
            _check(_lib.rt_smooth_expand(*a, None, C.byref(n)))
            smooth = (SmoothDesc * n.value)()
            _check(_lib.rt_smooth_expand(*a, smooth, C.byref(n)))
        uvs = None
        if self.uvs is not None and len(self.uvs):
            n = C.c_uint32(0)
            a = self.instanced_args()[:6] + (self.uvs, len(self.uvs))
            _check(_lib.rt_uv_expand(*a, None, C.byref(n)))
            uvs = (UVDesc * n.value)()
            _check(_lib.rt_uv_expand(*a, uvs, C.byref(n)))
        return SceneTables(out, self.materials, self.patterns, self.expanded_lights(), self.camera, smooth=smooth,
                           uvs=uvs, textures=self.textures, maps=self.maps)

    @property
    def counts(self):
        return len(self.shapes), len(self.materials), len(self.patterns), len(self.lights)

    def args(self):
        """(shapes, n, materials, n, patterns, n, lights, n) for C calls."""
        return (self.shapes, len(self.shapes), self.materials, len(self.materials), self.patterns,
                len(self.patterns), self.lights, len(self.lights))

    def has_secondary(self) -> bool:
        return any(m.reflectiveness != 0.0 or m.transparency != 0.0 for m in self.materials)


def _tables_from_view(v: SceneView) -> SceneTables:
    def copy(ptr, n, typ):
        arr = (typ * n)()
        if n:
            C.memmove(arr, ptr, n * C.sizeof(typ))
        return arr
    return SceneTables(copy(v.shapes, v.n_shapes, ShapeDesc), copy(v.materials, v.n_materials, MaterialDesc),
                       copy(v.patterns, v.n_patterns, PatternDesc), copy(v.lights, v.n_lights, LightDesc),
                       v.camera.copy(), v.duplicate_shapes)


def _load_with(fn, arg: bytes) -> SceneTables:
    h = C.c_void_p()
    _check(fn(arg, C.byref(h)))
    try:
        v = SceneView()
        _check(_lib.rt_scene_view_get(h, C.byref(v)))
        return _tables_from_view(v)
    finally:
        _lib.rt_scene_free(h)


def load_scene(path: str) -> SceneTables:
    """load_scene_description (scene_loader.rs:361-367): YAML file -> tables + camera."""
    return _load_with(_lib.rt_scene_load_yaml, os.fsencode(path))


def load_scene_text(text: str) -> SceneTables:
    return _load_with(_lib.rt_scene_load_yaml_text, text.encode())


class Mesh:
    """A triangle mesh read from OBJ text (rtc_scene.h rt_mesh_*): vertices (n, 3) f64, triangles (m, 3)
    uint32 (0-based) and the number of lines the loader skipped.  world.mesh() makes Shapes of it."""

    def __init__(self, handle: C.c_void_p):
        self._h = handle
        v = MeshView()
        _check(_lib.rt_mesh_view_get(self._h, C.byref(v)))
        self.vertices = np.ctypeslib.as_array(v.vertices, (v.n_vertices, 3)).copy() if v.n_vertices else \
            np.zeros((0, 3), dtype=np.float64)
        self.triangles = np.ctypeslib.as_array(v.triangles, (v.n_triangles, 3)).copy() if v.n_triangles else \
            np.zeros((0, 3), dtype=np.uint32)
        self.ignored_lines = int(v.ignored_lines)
        # load_obj(..., normals=True): the vn lines (k, 3) f64, per triangle its three 0-based normal
        # indices (RT_NO_NORMAL x 3 for a flat face) and the number of smooth triangles; else empty / 0
        nv = MeshNormalsView()
        _check(_lib.rt_mesh_normals_get(self._h, C.byref(nv)))
        self.normals = np.ctypeslib.as_array(nv.normals, (nv.n_normals, 3)).copy() if nv.n_normals else \
            np.zeros((0, 3), dtype=np.float64)
        self.triangle_normals = np.ctypeslib.as_array(nv.triangle_normals, (v.n_triangles, 3)).copy() \
            if nv.triangle_normals and v.n_triangles else np.zeros((0, 3), dtype=np.uint32)
        self.n_smooth = int(nv.n_smooth)
        # load_obj(..., texcoords=True): the vt lines (k, 2) f64 (u, v), per triangle its three 0-based
        # indices (RT_NO_TEXCOORD x 3 for a face without) and the number of triangles with coordinates
        tv = MeshTexcoordsView()
        _check(_lib.rt_mesh_texcoords_get(self._h, C.byref(tv)))
        self.texcoords = np.ctypeslib.as_array(tv.texcoords, (tv.n_texcoords, 2)).copy() if tv.n_texcoords else \
            np.zeros((0, 2), dtype=np.float64)
        self.triangle_texcoords = np.ctypeslib.as_array(tv.triangle_texcoords, (v.n_triangles, 3)).copy() \
            if tv.triangle_texcoords and v.n_triangles else np.zeros((0, 3), dtype=np.uint32)
        self.n_textured = int(tv.n_textured)

    def uv_descs(self, list_index: int = RT_SMOOTH_SHAPES, first: int = 0):
        """rt_mesh_uvs: one UVDesc per triangle with texture coordinates, pairing with shape_descs(); `first`
        is added to every index.  Coordinates do not transform: there is no bake."""
        out = (UVDesc * self.n_textured)()
        n = C.c_uint32(0)
        _check(_lib.rt_mesh_uvs(self._h, out if self.n_textured else None, int(list_index), C.byref(n)))
        for d in out:
            d.index += first
        return out

    def smooth_descs(self, transform=None, bake: bool = False, list_index: int = RT_SMOOTH_SHAPES, first: int = 0):
        """rt_mesh_smooth_normals: one SmoothDesc per smooth triangle, pairing with shape_descs(transform,
        bake); `first` is added to every index (the triangles' position in their list)."""
        out = (SmoothDesc * self.n_smooth)()
        t = None if transform is None else (C.c_double * 16)(*np.asarray(transform, dtype=np.float64).reshape(16))
        n = C.c_uint32(0)
        _check(_lib.rt_mesh_smooth_normals(self._h, t, int(bool(bake)), out if self.n_smooth else None,
                                           int(list_index), C.byref(n)))
        for d in out:
            d.index += first
        return out

    def shape_descs(self, transform=None, bake: bool = False, material: int = 0):
        """rt_mesh_triangles: the faces as an array of ShapeDesc (Triangle::new per face)."""
        out = (ShapeDesc * len(self.triangles))()
        t = None if transform is None else (C.c_double * 16)(*np.asarray(transform, dtype=np.float64).reshape(16))
        _check(_lib.rt_mesh_triangles(self._h, t, int(bool(bake)), int(material), out))
        return out

    def __del__(self):
        try:
            if self._h:
                _lib.rt_mesh_free(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


def load_obj(path_or_text, normals: bool = False, texcoords: bool = False) -> Mesh:
    """An OBJ file (a path: str without a newline, bytes or os.PathLike) or OBJ text (a str holding a
    newline) -> Mesh.  Raises RenderError(RT_ERR_IO) with the line number for a bad v or f line.
    normals=True also reads the vn lines and the faces' normal indices (Mesh.normals, triangle_normals,
    n_smooth; rtc_scene.h rt_mesh_load_obj_ex); texcoords=True the vt lines and the faces' texture indices
    (Mesh.texcoords, triangle_texcoords, n_textured)."""
    h = C.c_void_p()
    flags = (RT_OBJ_NORMALS if normals else 0) | (RT_OBJ_TEXCOORDS if texcoords else 0)
    if flags:
        if isinstance(path_or_text, str) and "\n" in path_or_text:
            _check(_lib.rt_mesh_load_obj_ex(None, path_or_text.encode(), flags, C.byref(h)))
        else:
            _check(_lib.rt_mesh_load_obj_ex(os.fsencode(path_or_text), None, flags, C.byref(h)))
    elif isinstance(path_or_text, str) and "\n" in path_or_text:
        _check(_lib.rt_mesh_load_obj_text(path_or_text.encode(), C.byref(h)))
    else:
        _check(_lib.rt_mesh_load_obj(os.fsencode(path_or_text), C.byref(h)))
    return Mesh(h)


def _ray_batch_kind(rays, precision, device):
    """("torch" | "numpy", "f32" | "f64") of a ray batch for Context.trace_rays, or ValueError."""
    if precision is not None and precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)} or None")
    if isinstance(rays, np.ndarray):
        kind, names = "numpy", {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}
        contiguous = rays.flags.c_contiguous
    else:
        import sys
        torch = sys.modules.get("torch")  # (a tensor cannot exist unless torch is loaded)
        if torch is None or not isinstance(rays, torch.Tensor):
            raise ValueError("rays must be a numpy array or a torch tensor of shape (n, 6)")
        kind, names = "torch", {torch.float32: "f32", torch.float64: "f64"}
        contiguous = rays.is_contiguous()
        if not rays.is_cuda or rays.device.index != device:
            raise ValueError(f"rays are on {rays.device}, the context drives cuda:{device}")
    if rays.ndim != 2 or rays.shape[1] != 6:
        raise ValueError(f"rays must have shape (n, 6), not {tuple(rays.shape)}")
    if rays.dtype not in names:
        raise ValueError(f"rays must be float32 or float64, not {rays.dtype}")
    if not contiguous:
        raise ValueError("rays must be C-contiguous")
    if kind == "numpy":  # host rays travel as f64 either way (rt_trace_rays): `precision` may choose the kernel
        return kind, precision or names[rays.dtype]
    if precision is not None and precision != names[rays.dtype]:
        raise ValueError(f"precision {precision} does not match the tensor's dtype {rays.dtype}")
    return kind, names[rays.dtype]


class Context:
    """One GPU.  Mirrors the borrow in Camera::render(&self, world: &World)."""

    def __init__(self, device: int = 0, _handle: C.c_void_p | None = None):
        h = _handle
        if h is None:
            h = C.c_void_p()
            _check(_lib.rt_context_create(device, C.byref(h)))
        self._h = h
        self.device = device
        self.scene: SceneTables | None = None

    @classmethod
    def multi(cls, devices) -> "Context":
        """One process, several GPUs (rt_context_create_multi: ncclCommInitAll).  Frames are split in
        row-block shards across the devices and gathered onto devices[0]."""
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _check(_lib.rt_context_create_multi(arr, len(devices), C.byref(h)))
        return cls(devices[0], h)

    @classmethod
    def rank(cls, device: int, n_ranks: int, rank: int, unique_id: bytes) -> "Context":
        """One process per GPU (rt_context_create_rank: ncclCommInitRank); every rank then makes the same
        calls; rank 0's scene and output are the ones used."""
        buf = (C.c_uint8 * RT_UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        h = C.c_void_p()
        _check(_lib.rt_context_create_rank(device, n_ranks, rank, buf, C.byref(h)))
        return cls(device, h)

    def group(self):
        """(shards per frame, this context's rank, GPUs driven by this process)."""
        n, r, loc = C.c_int(), C.c_int(), C.c_int()
        _check(_lib.rt_context_group(self._h, C.byref(n), C.byref(r), C.byref(loc)))
        return n.value, r.value, loc.value

    def close(self) -> None:
        if self._h:
            _lib.rt_context_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_frames_in_flight(self, frames: int) -> None:
        """Planning hint (rtc.h rt_context_set_frames_in_flight): the caller keeps `frames` frames in
        flight on as many contexts; > 1 plans the direct kernel for throughput.  Pixels unchanged."""
        _check(_lib.rt_context_set_frames_in_flight(self._h, frames))

    def set_jit(self, mode: int) -> None:
        """Per-scene kernels (rtc.h rt_context_set_jit): 0 never, 1 every f32 frame (built in line),
        2 frames of >= 64K pixels, built on a host thread from the 2nd such frame (the default),
        3 the same from the 1st."""
        _check(_lib.rt_context_set_jit(self._h, mode))

    def jit_wait(self, timeout_ms: float = -1.0) -> int:
        """Wait for this context's per-scene builds in flight; returns how many are still running."""
        n = C.c_int(0)
        _check(_lib.rt_jit_wait(self._h, float(timeout_ms), C.byref(n)))
        return n.value

    def jit_status(self) -> dict:
        """Whether the last launch ran a per-scene kernel, compile ms so far, last build error."""
        used, ms, log = C.c_int(), C.c_double(), C.create_string_buffer(4096)
        _check(_lib.rt_jit_status(self._h, C.byref(used), C.byref(ms), log, len(log)))
        return {"used": bool(used.value), "compile_ms": ms.value, "log": log.value.decode(errors="replace")}

    def tree_info(self) -> dict:
        """The uploaded world's triangle hierarchy (rtc.h rt_scene_tree_info): nodes, leaves, depth, records in
        and outside the tree and the host build's ms; all zero when the world has none."""
        t = TreeInfo()
        _check(_lib.rt_scene_tree_info(self._h, C.byref(t)))
        return {name: getattr(t, name) for name, _ in t._fields_ if name != "reserved"}

    def instance_info(self) -> dict:
        """The uploaded world's meshes and instances (rtc.h rt_scene_instance_info): counts, the instances
        uploaded expanded, local records and nodes, device bytes against the expansion's, build ms."""
        t = InstanceInfo()
        _check(_lib.rt_scene_instance_info(self._h, C.byref(t)))
        return {name: getattr(t, name) for name, _ in t._fields_}

    def smooth_info(self) -> dict:
        """The uploaded world's smooth triangles (rtc.h rt_scene_smooth_info): how many, the device bytes of
        the normal tables, whether the last launch ran the kernels that interpolate them."""
        t = SmoothInfo()
        _check(_lib.rt_scene_smooth_info(self._h, C.byref(t)))
        return {name: getattr(t, name) for name, _ in t._fields_}

    def texture_info(self) -> dict:
        """The uploaded world's textures (rtc.h rt_scene_texture_info): triangles with coordinates, textures,
        the device bytes of the coordinate tables and the texels, whether the last launch ran the texture code."""
        t = TextureInfo()
        _check(_lib.rt_scene_texture_info(self._h, C.byref(t)))
        return {name: getattr(t, name) for name, _ in t._fields_ if name != "reserved"}

    def light_info(self) -> dict:
        """The uploaded world's area lights (rtc.h rt_scene_light_info): how many, their samples in all, the
        device bytes of their records, whether the last launch ran the kernels that hold the sample loop."""
        t = LightInfo()
        _check(_lib.rt_scene_light_info(self._h, C.byref(t)))
        return {name: getattr(t, name) for name, _ in t._fields_ if name != "reserved"}

    def map_info(self) -> dict:
        """The uploaded world's texture maps (rtc.h rt_scene_map_info): patterns with a map other than the
        planar one, cube maps among them, whether the last launch ran the kernels that hold the map code."""
        t = MapInfo()
        _check(_lib.rt_scene_map_info(self._h, C.byref(t)))
        return {name: getattr(t, name) for name, _ in t._fields_ if name != "reserved"}

    def motion_info(self) -> dict:
        """The uploaded world's motion (rtc.h rt_scene_motion_info): moving shapes and instances, the device
        bytes of the velocity tables, whether the last launch was a shutter frame or a timed ray batch."""
        t = MotionInfo()
        _check(_lib.rt_scene_motion_info(self._h, C.byref(t)))
        return {name: getattr(t, name) for name, _ in t._fields_ if name != "reserved"}

    def upload(self, scene: SceneTables | None) -> None:
        """rt_scene_upload_moving for tables with a motion list; else rt_scene_upload, rt_scene_upload_instanced for tables with instances, rt_scene_upload_smooth for
        tables with smooth triangles, rt_scene_upload_textured for tables with texture coordinates or
        textures, rt_scene_upload_lit for tables with area lights, or rt_scene_upload_mapped for tables with
        a texture map entry; on a non-zero rank of a group, None
        (the scene comes from rank 0)."""
        if scene is None:
            _check(_lib.rt_scene_upload(self._h, None, 0, None, 0, None, 0, None, 0))
        elif scene.moving:
            _check(_lib.rt_scene_upload_moving(self._h, *scene.moving_args()))
        elif scene.mapped:
            _check(_lib.rt_scene_upload_mapped(self._h, *scene.mapped_args()))
        elif scene.lit:
            _check(_lib.rt_scene_upload_lit(self._h, *scene.lit_args()))
        elif scene.textured:
            _check(_lib.rt_scene_upload_textured(self._h, *scene.textured_args()))
        elif scene.smoothed:
            _check(_lib.rt_scene_upload_smooth(self._h, *scene.smooth_args()))
        elif scene.instanced:
            _check(_lib.rt_scene_upload_instanced(self._h, *scene.instanced_args()))
        else:
            _check(_lib.rt_scene_upload(self._h, *scene.args()))
        self.scene = scene

    @staticmethod
    def options(depth=RT_DEFAULT_MAX_DEPTH, precision="f32", out_format="real", shard=(0, 1),
                flags: int = 0) -> RenderOptions:
        return RenderOptions(depth, PRECISIONS[precision], OUT_FORMATS[out_format], shard[0], shard[1], flags)

    def render(self, camera: CameraDesc, depth: int = RT_DEFAULT_MAX_DEPTH, precision: str = "f32",
               out_format: str = "real", shard=(0, 1), out: np.ndarray | None = None, flags: int = 0):
        """Render one frame (or one shard's strip) into a host array (H, W, 3); returns (image, stats).
        `out` reuses a caller's array of that shape and dtype (a canvas kept across frames)."""
        opts = self.options(depth, precision, out_format, shard, flags)
        rows = camera.height if shard[1] == 1 else shard_rows(camera.height, shard[1])
        dtype = np.uint8 if out_format == "u8" else (np.float32 if precision == "f32" else np.float64)
        if out is not None:
            if out.shape != (rows, camera.width, 3) or out.dtype != dtype or not out.flags.c_contiguous:
                raise ValueError(f"out must be a C-contiguous {dtype.__name__} array of shape {(rows, camera.width, 3)}")
            img = out
        else:
            img = np.zeros((rows, camera.width, 3), dtype=dtype)
        st = Stats()
        _check(_lib.rt_render(self._h, C.byref(camera), C.byref(opts), img.ctypes.data_as(C.c_void_p),
                              C.byref(st)))
        return img, st.as_dict()

    def render_stats(self, camera: CameraDesc, depth: int = RT_DEFAULT_MAX_DEPTH, precision: str = "f32",
                     out_format: str = "real", out=None):
        """rt_render into `out` (a host array of the frame, or None on a group's non-zero ranks): stats only."""
        opts = self.options(depth, precision, out_format)
        st = Stats()
        ptr = None if out is None else out.ctypes.data_as(C.c_void_p)
        _check(_lib.rt_render(self._h, C.byref(camera), C.byref(opts), ptr, C.byref(st)))
        return st.as_dict()

    def render_device(self, camera: CameraDesc, out_ptr: int, stream_ptr: int | None = None,
                      depth: int = RT_DEFAULT_MAX_DEPTH, precision: str = "f32", out_format: str = "real",
                      shard=(0, 1), flags: int = 0) -> None:
        """Asynchronous render into a device buffer (e.g. a torch tensor's data_ptr()) on a HIP stream
        (stream_ptr None/0 = HIP's default stream, which is torch's default stream)."""
        opts = self.options(depth, precision, out_format, shard, flags)
        _check(_lib.rt_render_device(self._h, C.byref(camera), C.byref(opts), C.c_void_p(out_ptr or 0),
                                     C.c_void_p(stream_ptr or 0)))

    def render_supersampled(self, camera: CameraDesc, grid: int, depth: int = RT_DEFAULT_MAX_DEPTH,
                            precision: str = "f32", out_format: str = "real", shard=(0, 1),
                            out: np.ndarray | None = None, flags: int = 0):
        """render() with grid x grid samples per pixel, averaged in the frame kernel (rtc.h
        rt_render_supersampled): `camera` is the output camera, the samples are the pixels of
        camera_resize(camera, grid * W, grid * H), the stats count that frame's rays.  grid 1 is render()."""
        opts = self.options(depth, precision, out_format, shard, flags)
        rows = camera.height if shard[1] == 1 else shard_rows(camera.height, shard[1])
        dtype = np.uint8 if out_format == "u8" else (np.float32 if precision == "f32" else np.float64)
        if out is not None:
            if out.shape != (rows, camera.width, 3) or out.dtype != dtype or not out.flags.c_contiguous:
                raise ValueError(f"out must be a C-contiguous {dtype.__name__} array of shape {(rows, camera.width, 3)}")
            img = out
        else:
            img = np.zeros((rows, camera.width, 3), dtype=dtype)
        st = Stats()
        _check(_lib.rt_render_supersampled(self._h, C.byref(camera), C.byref(opts), grid,
                                           img.ctypes.data_as(C.c_void_p), C.byref(st)))
        return img, st.as_dict()

    def render_supersampled_device(self, camera: CameraDesc, grid: int, out_ptr: int, stream_ptr: int | None = None,
                                   depth: int = RT_DEFAULT_MAX_DEPTH, precision: str = "f32",
                                   out_format: str = "real", shard=(0, 1), flags: int = 0) -> None:
        """render_device() with grid x grid samples per pixel (rtc.h rt_render_supersampled_device): the
        W x H x 3 buffer of the output camera, asynchronous on the stream."""
        opts = self.options(depth, precision, out_format, shard, flags)
        _check(_lib.rt_render_supersampled_device(self._h, C.byref(camera), C.byref(opts), grid,
                                                  C.c_void_p(out_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def render_lens(self, camera: CameraDesc, grid: int, lens: "LensDesc", depth: int = RT_DEFAULT_MAX_DEPTH,
                    precision: str = "f32", out_format: str = "real", shard=(0, 1),
                    out: np.ndarray | None = None, flags: int = 0):
        """render_supersampled() through a thin lens (rtc.h rt_render_lens): sample (i, j) of a pixel leaves its
        point of the lens disc and passes through the pinhole ray's point on the focal plane.  An aperture of 0
        is render_supersampled(); grid 1 is one lens point per pixel (accumulate frames over seeds)."""
        opts = self.options(depth, precision, out_format, shard, flags)
        rows = camera.height if shard[1] == 1 else shard_rows(camera.height, shard[1])
        dtype = np.uint8 if out_format == "u8" else (np.float32 if precision == "f32" else np.float64)
        if out is not None:
            if out.shape != (rows, camera.width, 3) or out.dtype != dtype or not out.flags.c_contiguous:
                raise ValueError(f"out must be a C-contiguous {dtype.__name__} array of shape {(rows, camera.width, 3)}")
            img = out
        else:
            img = np.zeros((rows, camera.width, 3), dtype=dtype)
        st = Stats()
        _check(_lib.rt_render_lens(self._h, C.byref(camera), C.byref(opts), grid,
                                   None if lens is None else C.byref(lens), img.ctypes.data_as(C.c_void_p),
                                   C.byref(st)))
        return img, st.as_dict()

    def render_lens_device(self, camera: CameraDesc, grid: int, lens: "LensDesc", out_ptr: int,
                           stream_ptr: int | None = None, depth: int = RT_DEFAULT_MAX_DEPTH, precision: str = "f32",
                           out_format: str = "real", shard=(0, 1), flags: int = 0) -> None:
        """render_supersampled_device() through a thin lens (rtc.h rt_render_lens_device): the W x H x 3 buffer
        of the output camera, asynchronous on the stream."""
        opts = self.options(depth, precision, out_format, shard, flags)
        _check(_lib.rt_render_lens_device(self._h, C.byref(camera), C.byref(opts), grid,
                                          None if lens is None else C.byref(lens), C.c_void_p(out_ptr or 0),
                                          C.c_void_p(stream_ptr or 0)))

    def render_shutter(self, camera: CameraDesc, grid: int, shutter: "ShutterDesc", lens: "LensDesc | None" = None,
                       depth: int = RT_DEFAULT_MAX_DEPTH, precision: str = "f32", out_format: str = "real",
                       shard=(0, 1), out: np.ndarray | None = None, flags: int = 0):
        """render_lens() with a time per sample (rtc.h rt_render_shutter): sample (i, j) of a pixel sees every
        moving shape where it is at the sample's time in [shutter.open, shutter.close].  lens None (or an
        aperture of 0) takes render_supersampled()'s sample rays.  In a world without movers it is
        render_lens() / render_supersampled()."""
        opts = self.options(depth, precision, out_format, shard, flags)
        rows = camera.height if shard[1] == 1 else shard_rows(camera.height, shard[1])
        dtype = np.uint8 if out_format == "u8" else (np.float32 if precision == "f32" else np.float64)
        if out is not None:
            if out.shape != (rows, camera.width, 3) or out.dtype != dtype or not out.flags.c_contiguous:
                raise ValueError(f"out must be a C-contiguous {dtype.__name__} array of shape {(rows, camera.width, 3)}")
            img = out
        else:
            img = np.zeros((rows, camera.width, 3), dtype=dtype)
        st = Stats()
        _check(_lib.rt_render_shutter(self._h, C.byref(camera), C.byref(opts), grid,
                                      None if lens is None else C.byref(lens),
                                      None if shutter is None else C.byref(shutter),
                                      img.ctypes.data_as(C.c_void_p), C.byref(st)))
        return img, st.as_dict()

    def render_shutter_device(self, camera: CameraDesc, grid: int, shutter: "ShutterDesc", out_ptr: int,
                              lens: "LensDesc | None" = None, stream_ptr: int | None = None,
                              depth: int = RT_DEFAULT_MAX_DEPTH, precision: str = "f32", out_format: str = "real",
                              shard=(0, 1), flags: int = 0) -> None:
        """render_lens_device() with a time per sample (rtc.h rt_render_shutter_device): the W x H x 3 buffer of
        the output camera, asynchronous on the stream."""
        opts = self.options(depth, precision, out_format, shard, flags)
        _check(_lib.rt_render_shutter_device(self._h, C.byref(camera), C.byref(opts), grid,
                                             None if lens is None else C.byref(lens),
                                             None if shutter is None else C.byref(shutter),
                                             C.c_void_p(out_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def color_at(self, rays, depth: int = RT_DEFAULT_MAX_DEPTH, precision: str = "f32"):
        """Batched World::color_at: rays (n, 6) = origin, direction -> colours (n, 3) f64.  In a world with
        reflective or transparent materials the directions must be unit length (rtc.h rt_color_at)."""
        r = np.ascontiguousarray(np.asarray(rays, dtype=np.float64).reshape(-1, 6))
        out = np.zeros((r.shape[0], 3), dtype=np.float64)
        st = Stats()
        _check(_lib.rt_color_at(self._h, r.ctypes.data_as(C.POINTER(C.c_double)), r.shape[0], depth,
                                PRECISIONS[precision], out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)))
        return out, st.as_dict()

    def trace_rays(self, rays, depth: int = RT_DEFAULT_MAX_DEPTH, precision: str | None = None, hits: bool = False,
                   flags: int = 0, times=None):
        """World::color_at for any rays in any uploaded world (rtc.h rt_trace_rays*): no unit-length rule, no
        brightness bound.  rays (n, 6) = origin, direction, float32 or float64, C-contiguous; the dtype is the
        precision (a tensor's must agree with `precision` if given; a numpy batch travels as f64 and
        `precision` may pick the f32 kernel for it).
          - a torch tensor on this context's device: rt_trace_rays_device on torch's current stream, no sync,
            no host copy; returns colours (n, 3), with hits=True (colours, t (n,), shape (n,) int32);
          - a numpy array: rt_trace_rays; returns (colours f64, stats), with hits=True (colours, t, shape, stats).
        shape is the primary hit's index in the uploaded shape table, -1 on a miss (t = inf).
        times: a time per ray (rtc.h rt_trace_rays_timed*), shape (n,), of the rays' own kind (a tensor of their
        dtype on their device, or a numpy array); None = every ray at time 0.
        Raises ValueError for anything else before the library is called."""
        kind, prec = _ray_batch_kind(rays, precision, self.device)
        if times is not None:
            if kind == "numpy":
                times = np.ascontiguousarray(times, dtype=np.float64)
            elif type(times) is not type(rays) or times.dtype != rays.dtype or times.device != rays.device or \
                    not times.is_contiguous():
                raise ValueError("times must be a contiguous tensor of the rays' dtype on their device")
            if times.ndim != 1 or times.shape[0] != rays.shape[0]:
                raise ValueError(f"times must have shape ({int(rays.shape[0])},), not {tuple(times.shape)}")
        opts = RayOptions(int(depth), PRECISIONS[prec], int(flags), 0)
        n = int(rays.shape[0])
        if kind == "torch":
            import torch
            rgb = torch.empty((n, 3), dtype=rays.dtype, device=rays.device)
            # rt_ray_hit_f32 = {f32, i32}, rt_ray_hit_f64 = {f64, i32, i32}: n x 2 words of the real's size
            rec = torch.empty((n, 2), dtype=torch.int32 if prec == "f32" else torch.int64,
                              device=rays.device) if hits else None
            if n:
                stream = torch.cuda.current_stream(rays.device).cuda_stream
                _check(_lib.rt_trace_rays_timed_device(self._h, C.c_void_p(rays.data_ptr()),
                                                 None if times is None else C.c_void_p(times.data_ptr()), n,
                                                 C.byref(opts), C.c_void_p(rgb.data_ptr()),
                                                 C.c_void_p(rec.data_ptr()) if hits else None, C.c_void_p(stream or 0)))
            if not hits:
                return rgb
            t = rec[:, 0].view(rays.dtype).contiguous()
            shape = (rec[:, 1] if prec == "f32" else rec.view(torch.int32).reshape(n, 4)[:, 2]).contiguous()
            return rgb, t, shape
        r = np.ascontiguousarray(rays, dtype=np.float64)
        out = np.zeros((n, 3), dtype=np.float64)
        rec = np.zeros(n, dtype=RAY_HIT_F64) if hits else None
        st = Stats()
        _check(_lib.rt_trace_rays_timed(self._h, r.ctypes.data_as(C.POINTER(C.c_double)),
                                  None if times is None else times.ctypes.data_as(C.POINTER(C.c_double)), n,
                                  C.byref(opts), out.ctypes.data_as(C.POINTER(C.c_double)),
                                  rec.ctypes.data_as(C.c_void_p) if hits else None, C.byref(st)))
        if not hits:
            return out, st.as_dict()
        return out, rec["t"].copy(), rec["shape"].copy(), st.as_dict()

    def debug_stamps(self) -> np.ndarray:
        """(workgroups, 2) s_memrealtime {start, end} of the last RT_FLAG_STAMPS launch (100 MHz ticks)."""
        n = C.c_uint32(0)
        _check(_lib.rt_debug_stamps(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 2), dtype=np.uint64)
        _check(_lib.rt_debug_stamps(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), n.value, C.byref(n)))
        return out

    def debug_item_log(self) -> np.ndarray:
        """Items of the last RT_FLAG_STAMPS pool launch: rows {item | wg << 32, start, end}."""
        n = C.c_uint32()
        _check(_lib.rt_debug_item_log(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3), dtype=np.uint64)
        _check(_lib.rt_debug_item_log(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), n.value, C.byref(n)))
        return out

    def debug_tile_costs(self) -> np.ndarray:
        """Per-tile durations (10 ns ticks) recorded by the last pool launch."""
        n = C.c_uint32(0)
        _check(_lib.rt_debug_tile_costs(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        _check(_lib.rt_debug_tile_costs(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n)))
        return out

    def debug_intersect(self, shape: int, rays, precision: str = "f64", world_space: bool = False):
        """The device's per-shape intersect on (n, 6) rays: list of t tuples (push order) per ray."""
        r = np.ascontiguousarray(np.asarray(rays, dtype=np.float64).reshape(-1, 6))
        out = np.zeros((r.shape[0], 5), dtype=np.float64)
        _check(_lib.rt_debug_intersect(self._h, shape, r.ctypes.data_as(C.POINTER(C.c_double)), r.shape[0],
                                       PRECISIONS[precision], int(world_space),
                                       out.ctypes.data_as(C.POINTER(C.c_double))))
        return [tuple(row[1:1 + int(row[0])]) for row in out]

    def debug_normal(self, shape: int, points, precision: str = "f64", world_space: bool = False) -> np.ndarray:
        """The device's local_normal_at (world_space=False) or normal_at on (n, 3) points."""
        p = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        out = np.zeros_like(p)
        _check(_lib.rt_debug_normal(self._h, shape, p.ctypes.data_as(C.POINTER(C.c_double)), p.shape[0],
                                    PRECISIONS[precision], int(world_space), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def set_gather(self, mode: int) -> None:
        """Multi-GPU contexts: RT_GATHER_RCCL (strips + ncclGather + de-interleave) or RT_GATHER_PEER (every
        shard stores into one canvas on rank 0; rtc.h).  Collective."""
        _check(_lib.rt_context_set_gather(self._h, mode))

    # ------------------------------------------------ peer canvas (rtc.h)
    def canvas_create(self, nbytes: int, n_flags: int, ipc: bool = True):
        """(device pointer, IPC handle bytes or None) of a new canvas of `nbytes` + n_flags shard flags."""
        p = C.c_void_p()
        h = (C.c_uint8 * RT_IPC_HANDLE_BYTES)()
        _check(_lib.rt_canvas_create(self._h, nbytes, n_flags, C.byref(p), h if ipc else None))
        return p.value, (bytes(h) if ipc else None)

    def canvas_open(self, handle: bytes, nbytes: int, n_flags: int) -> int:
        """Map another process's canvas (its rt_canvas_create handle); returns the device pointer."""
        h = (C.c_uint8 * RT_IPC_HANDLE_BYTES).from_buffer_copy(handle)
        p = C.c_void_p()
        _check(_lib.rt_canvas_open(self._h, h, nbytes, n_flags, C.byref(p)))
        return p.value

    def canvas_close(self, canvas: int) -> None:
        _check(_lib.rt_canvas_close(self._h, C.c_void_p(canvas)))

    def render_to_canvas(self, camera: CameraDesc, canvas: int, seq: int, depth: int = RT_DEFAULT_MAX_DEPTH,
                         precision: str = "f32", out_format: str = "real", shard=(0, 1), stream_ptr: int | None = None,
                         timeout_ms: float = 10000.0) -> None:
        opts = self.options(depth, precision, out_format, shard)
        _check(_lib.rt_render_to_canvas(self._h, C.byref(camera), C.byref(opts), C.c_void_p(canvas), seq,
                                        float(timeout_ms), C.c_void_p(stream_ptr or 0)))

    def canvas_wait(self, canvas: int, seq: int, timeout_ms: float = 10000.0, stream_ptr: int | None = None) -> None:
        _check(_lib.rt_canvas_wait(self._h, C.c_void_p(canvas), seq, float(timeout_ms), C.c_void_p(stream_ptr or 0)))

    def canvas_release(self, canvas: int, seq: int, stream_ptr: int | None = None) -> None:
        _check(_lib.rt_canvas_release(self._h, C.c_void_p(canvas), seq, C.c_void_p(stream_ptr or 0)))

    def canvas_read(self, canvas: int, shape, dtype=np.uint8) -> np.ndarray:
        """The canvas image as a host array of `shape` (synchronous; raises on a peer-canvas timeout)."""
        out = np.zeros(shape, dtype=dtype)
        _check(_lib.rt_canvas_read(self._h, C.c_void_p(canvas), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def counters(self) -> dict:
        st = Stats()
        _check(_lib.rt_read_counters(self._h, C.byref(st)))
        return st.as_dict()

    def generation_counts(self):
        """(traced, shaded) per `remaining` 0..16, cumulative over RT_FLAG_GENERATIONS launches (rtc.h)."""
        g = GenerationCounts()
        _check(_lib.rt_read_generation_counts(self._h, C.byref(g)))
        return np.array(g.traced[:], dtype=np.uint64), np.array(g.shaded[:], dtype=np.uint64)

    def render_generations(self, camera: CameraDesc, depth: int = RT_DEFAULT_MAX_DEPTH, precision: str = "f32"):
        """One diagnostic frame with RT_FLAG_GENERATIONS: (image, stats, per-generation dict).  Generation g
        (0 = camera rays) is `remaining` depth - g; shadow rays are L per shaded hit (world.rs:46-52)."""
        t0, s0 = self.generation_counts()
        opts = self.options(depth, precision, "real", (0, 1), RT_FLAG_GENERATIONS)
        dtype = np.float32 if precision == "f32" else np.float64
        img = np.zeros((camera.height, camera.width, 3), dtype=dtype)
        st = Stats()
        _check(_lib.rt_render(self._h, C.byref(camera), C.byref(opts), img.ctypes.data_as(C.c_void_p), C.byref(st)))
        t1, s1 = self.generation_counts()
        traced, shaded = (t1 - t0)[::-1][-(depth + 1):], (s1 - s0)[::-1][-(depth + 1):]
        return img, st.as_dict(), {"traced": [int(v) for v in traced], "shaded": [int(v) for v in shaded]}

    def assemble_shards(self, gathered_ptr: int, width: int, height: int, shards: int, bytes_per_pixel: int,
                        image_ptr: int, stream_ptr: int | None = None) -> None:
        _check(_lib.rt_assemble_shards(self._h, C.c_void_p(gathered_ptr), width, height, shards, bytes_per_pixel,
                                       C.c_void_p(image_ptr), C.c_void_p(stream_ptr or 0)))
