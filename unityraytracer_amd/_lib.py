"""ctypes binding of libunityraytracer_amd.so (include/urt.h).

The shared library is the product: hand-written HIP kernels + the C ABI.  It is built in-tree by
`unityraytracer_amd.build.build_library()` (hipcc, gfx950).  There is no fallback of any kind: if the
library is missing this module raises, and if no GPU is usable `Context()` raises."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("URT_LIB_PATH") or os.path.join(_HERE, "libunityraytracer_amd.so")   # override: A/B builds in experiments

URT_OK = 0
ERROR_NAMES = {1: "INVALID_ARGUMENT", 2: "INVALID_HANDLE", 3: "NO_DEVICE", 4: "HIP", 5: "UNBOUND", 6: "LAYOUT", 7: "OUT_OF_MEMORY", 8: "SCENE", 9: "WATCHDOG"}

# every symbol include/urt.h declares (tests check that the .so exports each of them)
ABI_SYMBOLS = [
    "urt_abi_version", "urt_device_count", "urt_context_create", "urt_context_destroy", "urt_last_error", "urt_context_set_stream",
    "urt_synchronize", "urt_flush", "urt_buffer_create", "urt_buffer_set_data", "urt_buffer_set_data_range", "urt_buffer_set_data_device", "urt_buffer_get_data_range", "urt_buffer_copy", "urt_skin_vertices", "urt_buffer_bounds", "urt_normals_plan_create", "urt_normals_plan_info", "urt_normals_plan_release", "urt_compute_normals", "urt_morph_plan_create", "urt_morph_plan_info", "urt_morph_plan_release", "urt_morph_vertices", "urt_mesh_leaf_bounds_device", "urt_sphere_leaf_bounds_device", "urt_build_object_bvh_device", "urt_buffer_get_info", "urt_buffer_release", "urt_texture_create",
    "urt_texture_create_external", "urt_texture_set_pixels", "urt_texture_get_pixels", "urt_texture_get_info", "urt_texture_read_begin", "urt_texture_read_end", "urt_texture_read_begin_format", "urt_texture_read_end_format", "urt_texture_release",
    "urt_shader_set_buffer", "urt_shader_set_texture", "urt_shader_set_matrix", "urt_shader_set_vector", "urt_shader_set_float",
    "urt_shader_set_int", "urt_shader_dispatch", "urt_shader_dispatch_rows", "urt_blit_add", "urt_blit", "urt_texture_pack_rows",
    "urt_texture_unpack_rows", "urt_texture_unpack_rows_on", "urt_texture_pack_rows_rgb", "urt_texture_unpack_rows_rgb", "urt_ray_query", "urt_ray_query_device", "urt_radiance_query", "urt_radiance_query_device", "urt_render_aov", "urt_denoise", "urt_reproject", "urt_reproject_objects", "urt_reproject_deformed", "urt_blit_add_history", "urt_upsample", "urt_auto_exposure", "urt_tonemap", "urt_depth_of_field", "urt_motion_blur", "urt_bloom", "urt_select_pixels", "urt_blend_samples", "urt_resample_below", "urt_set_option", "urt_get_counters", "urt_reset_counters", "urt_debug_build_blas", "urt_debug_get_blas", "urt_debug_blas_cache_stats",
    "urt_debug_scene_info", "urt_debug_launch_info", "urt_debug_read_scene_blas", "urt_debug_read_scene_qnodes", "urt_debug_read_scene_cones", "urt_debug_read_tile_entry", "urt_debug_serve_stats", "urt_debug_refit_stats", "urt_debug_deform_stats", "urt_debug_scene_cost", "urt_debug_scene_vertex_spans", "urt_debug_prepare_stats", "urt_debug_buffer_state", "urt_debug_live_resources", "urt_debug_build_walk_table", "urt_debug_build_normals_plan", "urt_debug_build_morph_plan", "urt_host_compute_normals", "urt_host_mesh_leaf_bounds", "urt_host_sphere_leaf_bounds", "urt_host_object_bvh_length",
    "urt_host_build_object_bvh", "urt_host_build_object_bvh_pairing", "urt_host_mesh_motion", "urt_host_sphere_motion", "urt_host_last_error", "urt_host_load_hdr", "urt_host_write_pfm", "urt_host_write_png", "urt_host_encode_srgb8", "urt_host_srgb8_first_floats",
    "urt_host_resize_rgba", "urt_host_io_last_error", "urt_host_log", "urt_host_log_scene_counts", "urt_host_log_tree_report", "urt_host_dump_bvh", "urt_host_dump_normals",
    "urt_host_debug_last_error",
    "urt_group_create", "urt_group_destroy", "urt_group_size", "urt_group_context", "urt_group_last_error", "urt_group_buffer_create",
    "urt_group_buffer_set_data", "urt_group_buffer_set_data_range", "urt_group_buffer_release", "urt_group_texture_create", "urt_group_texture_set_pixels",
    "urt_group_texture_get_pixels", "urt_group_texture_release", "urt_group_shader_set_buffer", "urt_group_shader_set_texture",
    "urt_group_shader_set_matrix", "urt_group_shader_set_vector", "urt_group_shader_set_float", "urt_group_shader_set_int",
    "urt_group_set_option", "urt_group_shader_dispatch", "urt_group_blit_add", "urt_group_blit", "urt_group_gather", "urt_group_flush",
    "urt_group_synchronize", "urt_group_get_counters", "urt_group_reset_counters",
]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rays", "tlas_nodes", "blas_nodes", "tri_tests", "sphere_tests", "hit_tri", "hit_sphere",
                                          "hit_ground", "hit_sky", "pixels", "dispatches")] + [("trace_ms", C.c_float), ("watchdog_trips", C.c_uint32), ("launches", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Ray(C.Structure):
    """urt_Ray (include/urt_types.h), 32 B."""
    _pack_ = 1
    _fields_ = [("origin", C.c_float * 3), ("t_max", C.c_float), ("direction", C.c_float * 3), ("reserved", C.c_int32)]


class RayHit(C.Structure):
    """urt_RayHit (include/urt_types.h), 48 B."""
    _pack_ = 1
    _fields_ = [("distance", C.c_float), ("position", C.c_float * 3), ("normal", C.c_float * 3), ("kind", C.c_int32),
                ("object", C.c_int32), ("primitive", C.c_int32), ("u", C.c_float), ("v", C.c_float)]


class PathRay(C.Structure):
    """urt_PathRay (include/urt_types.h), 48 B."""
    _pack_ = 1
    _fields_ = [("origin", C.c_float * 3), ("seed", C.c_float), ("direction", C.c_float * 3), ("reserved0", C.c_int32),
                ("px", C.c_float), ("py", C.c_float), ("reserved1", C.c_int32 * 2)]


class PathPixel(C.Structure):
    """urt_PathPixel (include/urt_types.h), 8 B."""
    _pack_ = 1
    _fields_ = [("x", C.c_int32), ("y", C.c_int32)]


URT_STRIDE_PATHRAY, URT_STRIDE_PATHPIXEL = 48, 8
URT_QUERY_CLOSEST, URT_QUERY_ANY = 0, 1
URT_RADIANCE_RAYS, URT_RADIANCE_PIXELS = 0, 1
RADIANCE_MAX_SAMPLES, RADIANCE_MAX_BOUNCES = 4096, 64            # include/urt.h: samples 1..4096, bounces 0..64
URT_AOV_PIXEL_CENTER, URT_AOV_FRAME_RAY = 0, 1


class DenoiseParams(C.Structure):
    """urt_DenoiseParams (include/urt.h), 16 B."""
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


# what urt_denoise uses for params == NULL (include/urt.h URT_DENOISE_DEFAULT_*)
DENOISE_DEFAULTS = {"iterations": 5, "sigma_color": 8.0, "sigma_normal": 0.5, "sigma_depth": 0.1}


class ReprojectParams(C.Structure):
    """urt_ReprojectParams (include/urt.h), 80 B."""
    _fields_ = [("prev_world_to_clip", C.c_float * 16), ("max_history", C.c_float), ("normal_threshold", C.c_float),
                ("plane_threshold", C.c_float), ("flags", C.c_int32)]


class ReprojectImages(C.Structure):
    """urt_ReprojectImages (include/urt.h), 11 texture handles, 88 B; motion 0 = not wanted."""
    _fields_ = [(n, C.c_uint64) for n in ("prev_color", "prev_count", "prev_hit", "prev_normal", "prev_id", "hit", "normal", "id", "color",
                                          "count", "motion")]


class ObjectMotion(C.Structure):
    """urt_ObjectMotion (include/urt_types.h), 48 B: current world -> previous world, three columns of the linear part, then the translation."""
    _fields_ = [("a", C.c_float * 12)]


class ReprojectMotion(C.Structure):
    """urt_ReprojectMotion (include/urt.h), 24 B: the two motion-table buffer handles (0 = not moved) of urt_reproject_objects."""
    _fields_ = [("mesh_motion", C.c_uint64), ("sphere_motion", C.c_uint64), ("moved_max_history", C.c_float), ("flags", C.c_int32)]


class ReprojectDeform(C.Structure):
    """urt_ReprojectDeform (include/urt.h), 40 B: the four buffer handles of urt_reproject_deformed and the per-vertex path's normal threshold."""
    _fields_ = [("prev_vertices", C.c_uint64), ("indices", C.c_uint64), ("prev_mesh_objects", C.c_uint64), ("deformed", C.c_uint64),
                ("normal_threshold", C.c_float), ("flags", C.c_int32)]


class SkinBuffers(C.Structure):
    """urt_SkinBuffers (include/urt.h), 40 B: the five input buffer handles of urt_skin_vertices (rest_normals 0 = positions only)."""
    _fields_ = [(n, C.c_uint64) for n in ("rest_vertices", "rest_normals", "bone_indices", "bone_weights", "bones")]


class NormalsPlanInfo(C.Structure):
    """urt_NormalsPlanInfo (include/urt.h), 32 B: what urt_normals_plan_info reports of a normals plan."""
    _fields_ = [(n, C.c_int32) for n in ("first", "count", "n_lists", "n_triangles", "n_entries", "max_valence")] + [("device_bytes", C.c_uint64)]


class MorphDelta(C.Structure):
    """urt_MorphDelta (include/urt.h), 32 B: one target's delta of one vertex (absolute vertex number) at weight 1."""
    _fields_ = [("vertex", C.c_int32), ("target", C.c_int32), ("dp", C.c_float * 3), ("dn", C.c_float * 3)]


MORPH_DELTA_DT = [("vertex", "<i4"), ("target", "<i4"), ("dp", "<f4", (3,)), ("dn", "<f4", (3,))]      # the same 32 bytes as a numpy dtype
MORPH_NORMALIZE = 1                                         # URT_MORPH_NORMALIZE
MORPH_MAX_TARGETS = 4096


class MorphPlanInfo(C.Structure):
    """urt_MorphPlanInfo (include/urt.h), 32 B: what urt_morph_plan_info reports of a morph plan."""
    _fields_ = [(n, C.c_int32) for n in ("first", "count", "n_targets", "n_entries", "max_valence", "n_touched")] + [("device_bytes", C.c_uint64)]


# the object-level BVH on the device (include/urt.h URT_OBJECT_BVH_DEVICE_MAX, URT_MESH_LEAF_BLOCKS): the most leaves urt_build_object_bvh_device
# takes, and the per-MeshObject workgroup cap of urt_mesh_leaf_bounds_device (a MeshObject of more than 256 * MESH_LEAF_BLOCKS index slots is strided over)
OBJECT_BVH_DEVICE_MAX = 1024
MESH_LEAF_BLOCKS = 256


class UpsampleParams(C.Structure):
    """urt_UpsampleParams (include/urt.h), 16 B."""
    _fields_ = [("normal_threshold", C.c_float), ("plane_threshold", C.c_float), ("count_scale", C.c_float), ("flags", C.c_int32)]


class UpsampleImages(C.Structure):
    """urt_UpsampleImages (include/urt.h), 11 texture handles, 88 B; low_count, albedo and count 0 = not given."""
    _fields_ = [(n, C.c_uint64) for n in ("low_color", "low_count", "low_hit", "low_normal", "low_id", "hit", "normal", "id", "albedo", "color",
                                          "count")]


# flags of urt_UpsampleParams and the values params == NULL stands for (include/urt.h URT_UPSAMPLE_*, URT_UPSAMPLE_DEFAULT_*)
URT_UPSAMPLE_WIDE_FALLBACK, URT_UPSAMPLE_SKY_FROM_ALBEDO = 1, 2
UPSAMPLE_DEFAULTS = {"normal_threshold": 0.9, "plane_threshold": 0.02, "count_scale": 1.0, "flags": URT_UPSAMPLE_WIDE_FALLBACK}


class ExposureState(C.Structure):
    """urt_ExposureState (include/urt.h), 1040 B, in device memory: all zero = fresh."""
    _fields_ = [("exposure", C.c_float), ("target", C.c_float), ("counted", C.c_uint32), ("skipped", C.c_uint32), ("hist", C.c_uint32 * 256)]


class ExposureParams(C.Structure):
    """urt_ExposureParams (include/urt.h), 24 B."""
    _fields_ = [("key", C.c_float), ("min_exposure", C.c_float), ("max_exposure", C.c_float), ("rate", C.c_float),
                ("low_permille", C.c_int32), ("high_permille", C.c_int32)]


class TonemapParams(C.Structure):
    """urt_TonemapParams (include/urt.h), 16 B."""
    _fields_ = [("exposure", C.c_float), ("white", C.c_float), ("op", C.c_int32), ("flags", C.c_int32)]


# operators of urt_TonemapParams and the values params == NULL stands for (include/urt.h URT_TONEMAP_*, URT_EXPOSURE_DEFAULT_*,
# URT_TONEMAP_DEFAULT_*)
URT_TONEMAP_LINEAR, URT_TONEMAP_REINHARD, URT_TONEMAP_ACES = 0, 1, 2
EXPOSURE_DEFAULTS = {"key": 0.18, "min_exposure": 1.0 / 64.0, "max_exposure": 64.0, "rate": 1.0, "low_permille": 100, "high_permille": 950}
TONEMAP_DEFAULTS = {"exposure": 1.0, "white": 4.0, "op": URT_TONEMAP_ACES, "flags": 0}


class DofParams(C.Structure):
    """urt_DofParams (include/urt.h), 16 B."""
    _fields_ = [("focus_distance", C.c_float), ("scale", C.c_float), ("max_radius", C.c_float), ("flags", C.c_int32)]


# the flag and the limit of urt_DofParams and the values params == NULL stands for (include/urt.h URT_DOF_FLAG_COC, URT_DOF_MAX_RADIUS,
# URT_DOF_DEFAULT_*)
URT_DOF_FLAG_COC = 1
URT_DOF_MAX_RADIUS = 16.0
DOF_DEFAULTS = {"focus_distance": 10.0, "scale": 8.0, "max_radius": 8.0, "flags": 0}


class MotionBlurParams(C.Structure):
    """urt_MotionBlurParams (include/urt.h), 16 B."""
    _fields_ = [("shutter", C.c_float), ("max_radius", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


# the flag and the limit of urt_MotionBlurParams and the values params == NULL stands for (include/urt.h URT_MOTION_BLUR_FLAG_VELOCITY,
# URT_MOTION_BLUR_MAX_RADIUS, URT_MOTION_BLUR_DEFAULT_*)
URT_MOTION_BLUR_FLAG_VELOCITY = 1
URT_MOTION_BLUR_MAX_RADIUS = 16.0
MOTION_BLUR_DEFAULTS = {"shutter": 0.5, "max_radius": 16.0, "flags": 0}


class BloomParams(C.Structure):
    """urt_BloomParams (include/urt.h), 28 B."""
    _fields_ = [("threshold", C.c_float), ("soft_knee", C.c_float), ("clamp", C.c_float), ("scatter", C.c_float), ("intensity", C.c_float),
                ("levels", C.c_int32), ("flags", C.c_int32)]


# the flag of urt_BloomParams and the values params == NULL stands for (include/urt.h URT_BLOOM_FLAG_ONLY, URT_BLOOM_DEFAULT_*)
URT_BLOOM_FLAG_ONLY = 1
BLOOM_DEFAULTS = {"threshold": 1.0, "soft_knee": 0.5, "clamp": 65504.0, "scatter": 0.7, "intensity": 0.2, "levels": 6, "flags": 0}


# the starting values a host passes to urt_reproject / urt_blit_add_history (include/urt.h URT_REPROJECT_DEFAULT_*)
REPROJECT_DEFAULTS = {"max_history": 64.0, "normal_threshold": 0.9, "plane_threshold": 0.02}
# normal_threshold of urt_ReprojectDeform (include/urt.h URT_REPROJECT_DEFAULT_DEFORM_NORMAL_THRESHOLD)
REPROJECT_DEFORM_NORMAL_THRESHOLD = 0.3


class LaunchInfo(C.Structure):
    """urt_launch_info (include/urt.h): the last trace launch of a context."""
    _fields_ = [("kernel", C.c_char * 96)] + [(n, C.c_int) for n in (
        "kernel_mode", "front_mode", "count_stats", "n_blocks", "block_threads", "lds_bytes", "waves_per_cu", "n_frames", "frame_group",
        "xcd_run", "tile_order", "top_nodes", "tlas_stack", "blas_stack", "lds_tables", "slab_frames", "slab_frames_max",
        "slab_out_of_memory", "experiment", "blas_builder", "trace_stream", "slab_base", "overlapped", "overlapped_launches", "cones", "handout", "tile_entry", "tile_entry_k")]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["kernel"] = self.kernel.decode()
        return d


class UrtError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"URT_ERR_{ERROR_NAMES.get(code, code)}: {message}")
        self.code = code


_lib = None


def load():
    """Load the shared library, declaring every prototype.  Raises ImportError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the HIP path.")
    lib = C.CDLL(LIB_PATH)
    lib.urt_abi_version.argtypes, lib.urt_abi_version.restype = [], C.c_int
    if lib.urt_abi_version() < 0 and os.environ.get("URT_ALLOW_EXPERIMENT") != "1":
        # an A/B, probe or diagnostic BUILD (csrc/experiments.h: -DURT_STAMPS, -DURT_PROBE_NOSTORE, ...): never the product.  Only the
        # measurement scripts under scripts/ opt in; tests, bench.py and the smoke must not run on one by accident (URT_LIB_PATH).
        raise ImportError(f"{LIB_PATH} is an experiment build (urt_abi_version() = {lib.urt_abi_version()}): refused. "
                          "Set URT_ALLOW_EXPERIMENT=1 to load it on purpose (scripts/ only).")
    vp, i, f, u64 = C.c_void_p, C.c_int, C.c_float, C.c_uint64
    pi, pf = C.POINTER(C.c_int), C.POINTER(C.c_float)
    protos = {
        "urt_abi_version": ([], i),
        "urt_device_count": ([pi], i),
        "urt_context_create": ([i, C.POINTER(vp)], i),
        "urt_context_destroy": ([vp], i),
        "urt_last_error": ([vp], C.c_char_p),
        "urt_context_set_stream": ([vp, vp], i),
        "urt_synchronize": ([vp], i),
        "urt_flush": ([vp], i),
        "urt_buffer_create": ([vp, i, i, C.POINTER(u64)], i),
        "urt_buffer_set_data": ([vp, u64, vp, i], i),
        "urt_buffer_set_data_range": ([vp, u64, i, vp, i], i),
        "urt_buffer_set_data_device": ([vp, u64, i, vp, i], i),
        "urt_buffer_get_data_range": ([vp, u64, i, vp, i], i),
        "urt_buffer_copy": ([vp, u64, i, u64, i, i], i),
        "urt_skin_vertices": ([vp, C.POINTER(SkinBuffers), i, i, u64, u64], i),
        "urt_buffer_bounds": ([vp, u64, i, i, vp, pi], i),
        "urt_debug_buffer_state": ([vp, u64, vp], i),
        "urt_normals_plan_create": ([vp, u64, u64, i, i, C.POINTER(u64)], i),
        "urt_normals_plan_info": ([vp, u64, C.POINTER(NormalsPlanInfo)], i),
        "urt_normals_plan_release": ([vp, u64], i),
        "urt_compute_normals": ([vp, u64, u64], i),
        "urt_debug_build_normals_plan": ([vp, i, vp, i, i, i, vp, vp, i, vp, i, vp], i),
        "urt_morph_plan_create": ([vp, vp, i, i, i, i, C.POINTER(u64)], i),
        "urt_morph_plan_info": ([vp, u64, C.POINTER(MorphPlanInfo)], i),
        "urt_morph_plan_release": ([vp, u64], i),
        "urt_morph_vertices": ([vp, u64, u64, u64, u64, u64, u64, i], i),
        "urt_debug_build_morph_plan": ([vp, i, i, i, i, vp, vp, vp], i),
        "urt_mesh_leaf_bounds_device": ([vp, u64, u64, u64, u64], i),
        "urt_sphere_leaf_bounds_device": ([vp, u64, u64], i),
        "urt_build_object_bvh_device": ([vp, u64, u64], i),
        "urt_buffer_get_info": ([vp, u64, pi, pi], i),
        "urt_buffer_release": ([vp, u64], i),
        "urt_texture_create": ([vp, i, i, C.POINTER(u64)], i),
        "urt_texture_create_external": ([vp, i, i, vp, C.POINTER(u64)], i),
        "urt_texture_set_pixels": ([vp, u64, vp], i),
        "urt_texture_get_pixels": ([vp, u64, vp], i),
        "urt_texture_get_info": ([vp, u64, pi, pi, C.POINTER(vp)], i),
        "urt_texture_read_begin": ([vp, u64, C.POINTER(u64)], i),
        "urt_texture_read_end": ([vp, u64, C.POINTER(C.POINTER(C.c_float))], i),
        "urt_texture_read_begin_format": ([vp, u64, i, C.POINTER(u64)], i),
        "urt_texture_read_end_format": ([vp, u64, C.POINTER(vp), C.POINTER(C.c_size_t)], i),
        "urt_texture_release": ([vp, u64], i),
        "urt_shader_set_buffer": ([vp, i, C.c_char_p, u64], i),
        "urt_shader_set_texture": ([vp, i, C.c_char_p, u64], i),
        "urt_shader_set_matrix": ([vp, C.c_char_p, vp], i),
        "urt_shader_set_vector": ([vp, C.c_char_p, vp], i),
        "urt_shader_set_float": ([vp, C.c_char_p, f], i),
        "urt_shader_set_int": ([vp, C.c_char_p, i], i),
        "urt_shader_dispatch": ([vp, i, i, i, i], i),
        "urt_shader_dispatch_rows": ([vp, i, i, i, i, i, i], i),
        "urt_blit_add": ([vp, u64, u64, f], i),
        "urt_blit": ([vp, u64, u64], i),
        "urt_texture_pack_rows": ([vp, u64, i, i, vp, C.POINTER(u64)], i),
        "urt_texture_unpack_rows": ([vp, u64, i, i, vp], i),
        "urt_texture_unpack_rows_on": ([vp, u64, i, i, vp, vp], i),
        "urt_texture_pack_rows_rgb": ([vp, u64, i, i, vp, C.POINTER(u64)], i),
        "urt_texture_unpack_rows_rgb": ([vp, u64, i, i, vp, f, vp], i),
        "urt_ray_query": ([vp, vp, i, vp, i], i),
        "urt_ray_query_device": ([vp, vp, i, vp, i], i),
        "urt_radiance_query": ([vp, vp, i, i, i, vp, i], i),
        "urt_radiance_query_device": ([vp, vp, i, i, i, vp, i], i),
        "urt_render_aov": ([vp, u64, u64, u64, u64, i], i),
        "urt_denoise": ([vp, u64, u64, u64, u64, u64, C.POINTER(DenoiseParams)], i),
        "urt_reproject": ([vp, C.POINTER(ReprojectImages), C.POINTER(ReprojectParams)], i),
        "urt_reproject_objects": ([vp, C.POINTER(ReprojectImages), C.POINTER(ReprojectParams), C.POINTER(ReprojectMotion)], i),
        "urt_reproject_deformed": ([vp, C.POINTER(ReprojectImages), C.POINTER(ReprojectParams), C.POINTER(ReprojectMotion),
                                    C.POINTER(ReprojectDeform)], i),
        "urt_blit_add_history": ([vp, u64, u64, u64, f], i),
        "urt_upsample": ([vp, C.POINTER(UpsampleImages), C.POINTER(UpsampleParams)], i),
        "urt_auto_exposure": ([vp, u64, u64, C.POINTER(ExposureParams), vp], i),
        "urt_tonemap": ([vp, u64, u64, C.POINTER(TonemapParams), vp], i),
        "urt_depth_of_field": ([vp, u64, u64, u64, C.POINTER(DofParams)], i),
        "urt_motion_blur": ([vp, u64, u64, u64, u64, C.POINTER(MotionBlurParams)], i),
        "urt_bloom": ([vp, u64, u64, C.POINTER(BloomParams), vp], i),
        "urt_select_pixels": ([vp, u64, f, vp, i, pi], i),
        "urt_blend_samples": ([vp, vp, vp, i, f, u64, u64, f], i),
        "urt_resample_below": ([vp, u64, u64, f, i, i, f, f, pi], i),
        "urt_set_option": ([vp, C.c_char_p, i], i),
        "urt_get_counters": ([vp, C.POINTER(Counters)], i),
        "urt_reset_counters": ([vp], i),
        "urt_debug_build_blas": ([vp, i, vp, i, vp, i, pi, pi, pi], i),
        "urt_debug_get_blas": ([vp, vp, vp, vp], i),
        "urt_debug_blas_cache_stats": ([vp, vp, vp], i),
        "urt_debug_scene_info": ([vp, pi, pi, pi, pf], i),
        "urt_debug_launch_info": ([vp, C.POINTER(LaunchInfo)], i),
        "urt_debug_serve_stats": ([vp, vp], i),
        "urt_debug_refit_stats": ([vp, vp, vp], i),
        "urt_debug_deform_stats": ([vp, vp], i),
        "urt_debug_scene_cost": ([vp, vp, i], i),
        "urt_debug_scene_vertex_spans": ([vp, vp, vp, i], i),
        "urt_debug_prepare_stats": ([vp, vp], i),
        "urt_debug_live_resources": ([vp], i),
        "urt_debug_build_walk_table": ([vp, i, i, vp, vp, vp, i, pi], i),
        "urt_host_dump_normals": ([C.c_char_p, vp, i, vp, i, vp, i, vp, i, pi], i),
        "urt_debug_read_scene_blas": ([vp, vp, vp, vp], i),
        "urt_debug_read_scene_qnodes": ([vp, vp, pi, pi], i),
        "urt_debug_read_scene_cones": ([vp, vp, vp, pi], i),
        "urt_debug_read_tile_entry": ([vp, vp, u64, pi, pi, pi, vp], i),
        "urt_host_compute_normals": ([vp, i, vp, i, vp], i),
        "urt_host_mesh_leaf_bounds": ([vp, i, vp, i, vp, i, i, vp], i),
        "urt_host_sphere_leaf_bounds": ([vp, i, i, vp], i),
        "urt_host_object_bvh_length": ([i], i),
        "urt_host_build_object_bvh": ([vp, i, vp, i], i),
        "urt_host_build_object_bvh_pairing": ([vp, i, vp, i], i),
        "urt_host_mesh_motion": ([vp, vp, i, vp], i),
        "urt_host_sphere_motion": ([vp, vp, i, vp], i),
        "urt_host_last_error": ([], C.c_char_p),
        "urt_host_load_hdr": ([C.c_char_p, pi, pi, vp, C.c_size_t], i),
        "urt_host_write_pfm": ([C.c_char_p, vp, i, i], i),
        "urt_host_write_png": ([C.c_char_p, vp, i, i], i),
        "urt_host_encode_srgb8": ([vp, C.c_size_t, vp], i),
        "urt_host_srgb8_first_floats": ([vp], i),
        "urt_host_resize_rgba": ([vp, i, i, vp, i, i], i),
        "urt_host_io_last_error": ([], C.c_char_p),
        "urt_host_log": ([C.c_char_p, i, i, C.c_char_p], i),
        "urt_host_log_scene_counts": ([C.c_char_p, i, i, i, i, i, i], i),
        "urt_host_log_tree_report": ([C.c_char_p, i, i, i, i, i, i, i], i),
        "urt_host_dump_bvh": ([C.c_char_p, vp, i, i, vp, vp, pi], i),
        "urt_host_debug_last_error": ([], C.c_char_p),
        "urt_group_create": ([pi, i, C.POINTER(vp)], i),
        "urt_group_destroy": ([vp], i),
        "urt_group_size": ([vp], i),
        "urt_group_context": ([vp, i], vp),
        "urt_group_last_error": ([vp], C.c_char_p),
        "urt_group_buffer_create": ([vp, i, i, C.POINTER(u64)], i),
        "urt_group_buffer_set_data": ([vp, u64, vp, i], i),
        "urt_group_buffer_set_data_range": ([vp, u64, i, vp, i], i),
        "urt_group_buffer_release": ([vp, u64], i),
        "urt_group_texture_create": ([vp, i, i, C.POINTER(u64)], i),
        "urt_group_texture_set_pixels": ([vp, u64, vp], i),
        "urt_group_texture_get_pixels": ([vp, u64, vp], i),
        "urt_group_texture_release": ([vp, u64], i),
        "urt_group_shader_set_buffer": ([vp, i, C.c_char_p, u64], i),
        "urt_group_shader_set_texture": ([vp, i, C.c_char_p, u64], i),
        "urt_group_shader_set_matrix": ([vp, C.c_char_p, vp], i),
        "urt_group_shader_set_vector": ([vp, C.c_char_p, vp], i),
        "urt_group_shader_set_float": ([vp, C.c_char_p, f], i),
        "urt_group_shader_set_int": ([vp, C.c_char_p, i], i),
        "urt_group_set_option": ([vp, C.c_char_p, i], i),
        "urt_group_shader_dispatch": ([vp, i, i, i, i], i),
        "urt_group_blit_add": ([vp, u64, u64, f], i),
        "urt_group_blit": ([vp, u64, u64], i),
        "urt_group_gather": ([vp, u64, u64], i),
        "urt_group_flush": ([vp], i),
        "urt_group_synchronize": ([vp], i),
        "urt_group_get_counters": ([vp, C.POINTER(Counters)], i),
        "urt_group_reset_counters": ([vp], i),
    }
    assert sorted(protos) == sorted(ABI_SYMBOLS)
    for name, (args, res) in protos.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if os.environ.get("URT_LIB_PATH"):     # an older build under A/B (scripts/sweep.py --libs): it simply lacks the newer entry points
                continue
            raise
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib
