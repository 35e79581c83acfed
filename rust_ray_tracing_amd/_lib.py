"""ctypes binding of libmipt.so (include/mipt.h) -- the C ABI is the product boundary.

The library is built in-tree by ``__graft_entry__.build()`` (``make -C rust_ray_tracing_amd/csrc``).
There is no fallback: if the shared object is missing, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIPT_LIB") or os.path.join(_HERE, "libmipt.so")   # MIPT_LIB: A/B a kernel variant

# ---- numpy views of the reference PODs (reference src/scene.rs:87-146, src/bvh.rs:164-171) ----
VERTEX = np.dtype([("position", "<f4", 3), ("tex_coord_x", "<f4"), ("normal", "<f4", 3), ("tex_coord_y", "<f4")])
TRIANGLE = np.dtype([("vertices", VERTEX, 3), ("material_id", "<u4"), ("_pad", "u1", 12)])
NODE = np.dtype([("bounds_min", "<f4", 3), ("first_tri_or_child", "<u4"), ("bounds_max", "<f4", 3), ("num_tris", "<u4")])
MATERIAL = np.dtype([
    ("base_color", "<f4", 3), ("transmission", "<f4"), ("specular_tint", "<f4", 3), ("ior", "<f4"),
    ("emission", "<f4", 3), ("roughness", "<f4"), ("metallic", "<f4"), ("transparency", "<f4"),
    ("base_color_tex_id", "<u4"), ("transparency_tex_id", "<u4"), ("roughness_tex_id", "<u4"),
    ("metallic_tex_id", "<u4"), ("emission_tex_id", "<u4"), ("normal_tex_id", "<u4")])
CAMERA = np.dtype([("look_at", "<f4", (4, 4)), ("position", "<f4", 3), ("_pad", "<f4")])
assert VERTEX.itemsize == 32 and TRIANGLE.itemsize == 112 and NODE.itemsize == 32
assert MATERIAL.itemsize == 80 and CAMERA.itemsize == 80

NO_TEXTURE = 0xFFFFFFFF

SEED_PIXEL_STREAM, SEED_PER_SAMPLE = 0, 1
TRAVERSAL_REFERENCE, TRAVERSAL_CULLED = 0, 1
SHADING_CPU, SHADING_WGPU = 0, 1
FLAG_COUNT, FLAG_PACKED, FLAG_SUM, FLAG_ACCUM, FLAG_TOUCHED = 1, 2, 4, 8, 16
CULL_MARGIN_SAFE = 0.0078125  # MIPT_CULL_MARGIN_SAFE

OK, ERR_INVALID_ARG, ERR_HIP, ERR_SCENE_LIMIT, ERR_BVH, ERR_IO, ERR_STACK, ERR_RCCL = 0, -1, -2, -3, -4, -5, -6, -7
MULTI_TILES, MULTI_SAMPLES = 0, 1
UPDATE_REFIT, UPDATE_REBUILD = 0, 1


class MiptTexture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgba8", C.c_void_p)]


class MiptSceneDesc(C.Structure):
    _fields_ = [("tris", C.c_void_p), ("n_tris", C.c_uint32),
                ("nodes", C.c_void_p), ("n_nodes", C.c_uint32),
                ("materials", C.c_void_p), ("n_materials", C.c_uint32),
                ("textures", C.POINTER(MiptTexture)), ("n_textures", C.c_uint32)]


class MiptOptions(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("samples", C.c_uint32),
                ("max_ray_depth", C.c_uint32), ("seed_mode", C.c_uint32), ("traversal", C.c_uint32),
                ("flags", C.c_uint32), ("tile_rank", C.c_uint32), ("tile_world", C.c_uint32),
                ("sample_begin", C.c_uint32), ("cull_margin", C.c_float), ("shading", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class MiptStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("rays", C.c_uint64), ("inner_steps", C.c_uint64),
                ("tri_tests", C.c_uint64), ("hits", C.c_uint64), ("texel_fetches", C.c_uint64),
                ("stack_overflows", C.c_uint64), ("tex_clamped", C.c_uint64), ("max_stack", C.c_uint64),
                ("pixels", C.c_uint64), ("diag", C.c_uint64 * 11), ("touched_lines", C.c_uint64 * 2)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("diag", "touched_lines")}
        d["diag"] = list(self.diag)
        d["touched_lines"] = list(self.touched_lines)
        return d


class MiptSceneInfo(C.Structure):
    _fields_ = [("n_tris", C.c_uint32), ("n_nodes", C.c_uint32), ("n_pair_records", C.c_uint32), ("max_leaf", C.c_uint32),
                ("geometry_bytes", C.c_uint64), ("built_on_device", C.c_uint32), ("replica_of_device", C.c_uint32),
                ("upload_ms", C.c_double), ("build_ms", C.c_double), ("layout_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MiptUpdateInfo(C.Structure):
    _fields_ = [("upload_ms", C.c_double), ("build_ms", C.c_double), ("layout_ms", C.c_double), ("total_ms", C.c_double),
                ("n_tris", C.c_uint32), ("n_nodes", C.c_uint32), ("n_pair_records", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


# ---- ray queries (include/mipt.h "ray queries") ----
RAY = np.dtype([("origin", "<f4", 3), ("t_max", "<f4"), ("direction", "<f4", 3), ("reserved", "<u4")])   # MiptRay
HIT = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4")])                               # MiptHit
assert RAY.itemsize == 32 and HIT.itemsize == 16
HIT_NONE, HIT_FRONT_FACE, HIT_TRI_MASK = 0xFFFFFFFF, 0x80000000, 0x01FFFFFF
QUERY_MAX_RAYS = 1 << 31


class MiptQueryOptions(C.Structure):
    _fields_ = [("traversal", C.c_uint32), ("cull_margin", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 5)]


# ---- radiance queries (include/mipt.h "radiance queries"): MiptRay's last word is the ray's seed ----
class MiptRadianceOptions(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("max_ray_depth", C.c_uint32), ("traversal", C.c_uint32), ("cull_margin", C.c_float),
                ("shading", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 10)]


assert C.sizeof(MiptRadianceOptions) == 64


# ---- baking (include/mipt.h "baking"): a MiptHit with a seed in its t word is a surface point ----
SURFACE_POINT = np.dtype([("seed", "<u4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4")])                     # MiptSurfacePoint
assert SURFACE_POINT.itemsize == 16


class MiptBakeTexelOptions(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class MiptBakeTexelInfo(C.Structure):
    _fields_ = [("covered_texels", C.c_uint64), ("degenerate_tris", C.c_uint32), ("kernel_ms", C.c_float), ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class MiptBakeOptions(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("max_ray_depth", C.c_uint32), ("traversal", C.c_uint32), ("cull_margin", C.c_float),
                ("shading", C.c_uint32), ("flags", C.c_uint32), ("first_sample", C.c_uint32), ("sample_stride", C.c_uint32),
                ("reserved", C.c_uint32 * 8)]


assert C.sizeof(MiptBakeOptions) == 64 and C.sizeof(MiptBakeTexelOptions) == 32 and C.sizeof(MiptBakeTexelInfo) == 32

BAKE_SURFACE_UNIT_NORMALS = 1


class MiptBakeSurfaceOptions(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32 * 7)]


# ---- lightmap finishing (include/mipt.h "lightmap finishing") ----
LIGHTMAP_MAX_RADIUS = 64


class MiptLightmapFilterOptions(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("sigma_color", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_plane", C.c_float), ("sigma_distance", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 8)]


class MiptLightmapFilterBuffers(C.Structure):
    _fields_ = [("radiance", C.c_void_p), ("points", C.c_void_p), ("position", C.c_void_p), ("normal", C.c_void_p), ("out", C.c_void_p),
                ("reserved", C.c_void_p * 3)]


class MiptLightmapDilateOptions(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("radius", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class MiptLightmapDilateBuffers(C.Structure):
    _fields_ = [("radiance", C.c_void_p), ("points", C.c_void_p), ("out", C.c_void_p), ("level", C.c_void_p), ("reserved", C.c_void_p * 4)]


assert C.sizeof(MiptBakeSurfaceOptions) == 32 and C.sizeof(MiptLightmapFilterOptions) == 64 and C.sizeof(MiptLightmapFilterBuffers) == 64
assert C.sizeof(MiptLightmapDilateOptions) == 32 and C.sizeof(MiptLightmapDilateBuffers) == 64


# ---- irradiance probes (include/mipt.h "irradiance probes") ----
PROBE = np.dtype([("position", "<f4", 3), ("seed", "<u4")])                                                   # MiptProbe
assert PROBE.itemsize == 16
PROBE_CLAMP = 1
PROBE_SH_WORDS = 27


class MiptProbeBakeOptions(C.Structure):
    _fields_ = list(MiptBakeOptions._fields_)


class MiptProbeGrid(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("dims", C.c_uint32 * 3), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 6)]


class MiptProbeIrradianceBuffers(C.Structure):
    _fields_ = [("sh", C.c_void_p), ("valid", C.c_void_p), ("position", C.c_void_p), ("normal", C.c_void_p), ("irradiance", C.c_void_p),
                ("reserved", C.c_void_p * 3)]


assert C.sizeof(MiptProbeBakeOptions) == 64 and C.sizeof(MiptProbeGrid) == 64 and C.sizeof(MiptProbeIrradianceBuffers) == 64


# ---- first-hit feature buffers (include/mipt.h "first-hit feature buffers") ----
FEATURES = (("depth", 1, np.float32), ("prim", 1, np.uint32), ("material", 1, np.uint32), ("position", 3, np.float32),
            ("uv", 2, np.float32), ("normal", 3, np.float32), ("albedo", 3, np.float32), ("emission", 3, np.float32))   # name, values per pixel, type


class MiptFeatureBuffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _, _ in FEATURES] + [("reserved", C.c_void_p * 4)]


assert C.sizeof(MiptFeatureBuffers) == 96


# ---- previous positions (include/mipt.h "previous positions") ----
class MiptMotionBuffers(C.Structure):
    _fields_ = [("prev_tris", C.c_void_p), ("n_prev_tris", C.c_uint32), ("reserved0", C.c_uint32), ("prev_position", C.c_void_p),
                ("reserved", C.c_void_p * 5)]


assert C.sizeof(MiptMotionBuffers) == 64


# ---- a-trous denoiser (include/mipt.h "a-trous denoiser") ----
class MiptDenoiseOptions(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("n_views", C.c_uint32), ("iterations", C.c_uint32),
                ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 8)]


class MiptDenoiseBuffers(C.Structure):
    _fields_ = [("hdr", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("albedo", C.c_void_p), ("out", C.c_void_p),
                ("reserved", C.c_void_p * 3)]


assert C.sizeof(MiptDenoiseOptions) == 64 and C.sizeof(MiptDenoiseBuffers) == 64


# ---- temporal accumulation (include/mipt.h "temporal accumulation") ----
class MiptTemporalOptions(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("n_views", C.c_uint32), ("flags", C.c_uint32),
                ("alpha_min", C.c_float), ("max_history", C.c_float), ("normal_tol", C.c_float), ("depth_tol", C.c_float),
                ("reserved", C.c_uint32 * 8)]


class MiptTemporalBuffers(C.Structure):
    _fields_ = [("hdr", C.c_void_p), ("position", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("material", C.c_void_p),
                ("albedo", C.c_void_p), ("history_in", C.c_void_p), ("history_out", C.c_void_p), ("out", C.c_void_p),
                ("length", C.c_void_p), ("variance", C.c_void_p), ("reserved", C.c_void_p * 5)]


assert C.sizeof(MiptTemporalOptions) == 64 and C.sizeof(MiptTemporalBuffers) == 128


# ---- variance-guided a-trous filter (include/mipt.h "variance-guided a-trous filter") ----
class MiptVarianceOptions(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("n_views", C.c_uint32), ("iterations", C.c_uint32),
                ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("short_history", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class MiptVarianceBuffers(C.Structure):
    _fields_ = [("hdr", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("albedo", C.c_void_p), ("variance", C.c_void_p),
                ("length", C.c_void_p), ("out", C.c_void_p), ("variance_out", C.c_void_p), ("reserved", C.c_void_p * 8)]


assert C.sizeof(MiptVarianceOptions) == 64 and C.sizeof(MiptVarianceBuffers) == 128


# ---- guided upsampling (include/mipt.h "guided upsampling") ----
class MiptUpsampleOptions(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("n_views", C.c_uint32), ("scale", C.c_uint32),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 9)]


class MiptUpsampleBuffers(C.Structure):
    _fields_ = [("lo_hdr", C.c_void_p), ("lo_normal", C.c_void_p), ("lo_depth", C.c_void_p), ("lo_albedo", C.c_void_p),
                ("lo_material", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("albedo", C.c_void_p),
                ("material", C.c_void_p), ("out", C.c_void_p), ("weight", C.c_void_p), ("reserved", C.c_void_p * 5)]


assert C.sizeof(MiptUpsampleOptions) == 64 and C.sizeof(MiptUpsampleBuffers) == 128

# ---- adaptive sampling (include/mipt.h "adaptive sampling") ----
class MiptSampleMapOptions(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("n_views", C.c_uint32), ("flags", C.c_uint32),
                ("min_samples", C.c_uint32), ("max_samples", C.c_uint32), ("budget", C.c_float), ("reserved", C.c_uint32 * 9)]


class MiptSampleMapBuffers(C.Structure):
    _fields_ = [("variance", C.c_void_p), ("hdr", C.c_void_p), ("albedo", C.c_void_p), ("counts", C.c_void_p), ("reserved", C.c_void_p * 4)]


class MiptSampleMapFillOptions(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("n_views", C.c_uint32), ("flags", C.c_uint32),
                ("min_samples", C.c_uint32), ("max_samples", C.c_uint32), ("budget", C.c_float), ("rounds", C.c_uint32),
                ("reserved", C.c_uint32 * 8)]


assert C.sizeof(MiptSampleMapOptions) == 64 and C.sizeof(MiptSampleMapBuffers) == 64 and C.sizeof(MiptSampleMapFillOptions) == 64

MESH_PART = np.dtype([("first_tri", "<u4"), ("n_tris", "<u4"), ("material_id", "<u4"), ("reserved", "<u4")])   # MiptMeshPart
assert MESH_PART.itemsize == 16


class MiptMeshDesc(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("n_positions", C.c_uint32),
                ("normals", C.c_void_p), ("n_normals", C.c_uint32),
                ("tex_coords", C.c_void_p), ("n_tex_coords", C.c_uint32),
                ("indices", C.c_void_p), ("n_indices", C.c_uint32),
                ("normal_indices", C.c_void_p), ("tex_coord_indices", C.c_void_p),
                ("parts", C.c_void_p), ("n_parts", C.c_uint32),
                ("transforms", C.c_void_p)]


class MiptMeshInfo(C.Structure):
    _fields_ = [("n_positions", C.c_uint32), ("n_normals", C.c_uint32), ("n_tex_coords", C.c_uint32), ("n_indices", C.c_uint32),
                ("n_tris", C.c_uint32), ("n_parts", C.c_uint32), ("has_transforms", C.c_uint32), ("index_streams", C.c_uint32),
                ("array_bytes", C.c_uint64), ("expanded_bytes", C.c_uint64), ("hbm_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MiptMultiStats(C.Structure):
    _fields_ = [("total", MiptStats), ("collective_ms", C.c_double), ("wall_ms", C.c_double),
                ("device_kernel_ms", C.c_double * 8), ("n_devices", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        d = self.total.as_dict()
        d.update(collective_ms=self.collective_ms, wall_ms=self.wall_ms, n_devices=self.n_devices,
                 device_kernel_ms=list(self.device_kernel_ms)[: self.n_devices])
        return d


# every symbol include/mipt.h declares (tests/test_abi.py checks the list against the header)
EXPORTS = [
    "mipt_scene_create", "mipt_scene_destroy", "mipt_render", "mipt_render_device",
    "mipt_packed_pixels", "mipt_unpack_tiles", "mipt_tonemap_device", "mipt_postprocess_device", "mipt_bvh_build", "mipt_bvh_build_device",
    "mipt_camera_from_pose", "mipt_material_default", "mipt_last_error", "mipt_abi_version",
    "mipt_device_count", "mipt_obj_load", "mipt_obj_free", "mipt_obj_get",
    "mipt_texture_load", "mipt_texture_free", "mipt_image_save_png",
    "mipt_multi_create", "mipt_multi_destroy", "mipt_multi_device_count", "mipt_render_multi",
    "mipt_render_multi_device", "mipt_multi_root_device", "mipt_multi_device_stats",
    "mipt_scene_create_from_triangles", "mipt_scene_get_bvh", "mipt_scene_info", "mipt_multi_create_from_triangles", "mipt_multi_scene", "mipt_obj_load_triangles",
    "mipt_scene_update_triangles", "mipt_scene_update_triangles_device", "mipt_multi_update_triangles",
    "mipt_render_batch", "mipt_render_batch_device",
    "mipt_query_closest", "mipt_query_closest_device", "mipt_query_occluded", "mipt_query_occluded_device",
    "mipt_render_features", "mipt_render_features_device",
    "mipt_denoise_workspace_bytes", "mipt_denoise", "mipt_denoise_device",
    "mipt_temporal_history_bytes", "mipt_temporal", "mipt_temporal_device",
    "mipt_denoise_variance_workspace_bytes", "mipt_denoise_variance", "mipt_denoise_variance_device",
    "mipt_upsample_workspace_bytes", "mipt_upsample", "mipt_upsample_device",
    "mipt_mesh_expand", "mipt_scene_create_from_mesh", "mipt_scene_set_transforms", "mipt_scene_update_mesh_device", "mipt_scene_mesh_info",
    "mipt_render_motion", "mipt_render_motion_device", "mipt_scene_track_motion",
    "mipt_render_adaptive", "mipt_render_adaptive_device", "mipt_sample_map_workspace_bytes", "mipt_sample_map", "mipt_sample_map_device",
    "mipt_temporal_counts", "mipt_temporal_counts_device",
    "mipt_sample_map_fill_workspace_bytes", "mipt_sample_map_fill", "mipt_sample_map_fill_device",
    "mipt_query_radiance", "mipt_query_radiance_device",
    "mipt_bake_texels", "mipt_bake_texels_device", "mipt_bake_gather", "mipt_bake_gather_device",
    "mipt_bake_surface", "mipt_bake_surface_device",
    "mipt_lightmap_filter_workspace_bytes", "mipt_lightmap_filter", "mipt_lightmap_filter_device",
    "mipt_lightmap_dilate_workspace_bytes", "mipt_lightmap_dilate", "mipt_lightmap_dilate_device",
    "mipt_probe_bake", "mipt_probe_bake_device", "mipt_probe_irradiance", "mipt_probe_irradiance_device",
]

_lib = None


def load() -> C.CDLL:
    """Load libmipt.so once.  torch (if importable) is imported first so that libmipt binds to
    the HIP runtime torch already loaded (same SONAME libamdhip64.so.7): device pointers of torch
    tensors are then valid in our launches."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C rust_ray_tracing_amd/csrc). "
                          "There is no CPU fallback for the MI355X backend.")
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing only
        pass
    _lib = _bind(C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL))
    return _lib


def _bind(lib: C.CDLL) -> C.CDLL:
    """argtypes / restype of every include/mipt.h entry point on a loaded library (the product or a build variant of it)."""
    vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    lib.mipt_scene_create.argtypes = [C.POINTER(MiptSceneDesc), C.c_int, C.POINTER(vp)]
    lib.mipt_scene_create.restype = C.c_int
    lib.mipt_scene_destroy.argtypes = [vp]
    lib.mipt_scene_destroy.restype = None
    lib.mipt_render.argtypes = [vp, vp, C.POINTER(MiptOptions), vp, vp, C.POINTER(MiptStats)]
    lib.mipt_render.restype = C.c_int
    lib.mipt_render_device.argtypes = [vp, vp, C.POINTER(MiptOptions), vp, vp, vp, C.POINTER(MiptStats)]
    lib.mipt_render_device.restype = C.c_int
    lib.mipt_render_batch.argtypes = [vp, vp, u32, C.POINTER(MiptOptions), vp, vp, C.POINTER(MiptStats)]
    lib.mipt_render_batch.restype = C.c_int
    lib.mipt_render_batch_device.argtypes = [vp, vp, u32, C.POINTER(MiptOptions), vp, vp, vp, C.POINTER(MiptStats)]
    lib.mipt_render_batch_device.restype = C.c_int
    lib.mipt_packed_pixels.argtypes = [u32, u32, u32]
    lib.mipt_packed_pixels.restype = u64
    lib.mipt_unpack_tiles.argtypes = [vp, u32, u32, u32, vp, vp]
    lib.mipt_unpack_tiles.restype = C.c_int
    lib.mipt_tonemap_device.argtypes = [vp, u64, f32, vp, vp]
    lib.mipt_tonemap_device.restype = C.c_int
    lib.mipt_postprocess_device.argtypes = [vp, u64, f32, vp, vp]
    lib.mipt_postprocess_device.restype = C.c_int
    lib.mipt_bvh_build.argtypes = [vp, u32, vp, u32, C.POINTER(u32), u32]
    lib.mipt_bvh_build.restype = C.c_int
    lib.mipt_bvh_build_device.argtypes = [vp, u32, vp, u32, C.POINTER(u32), C.c_int, C.POINTER(C.c_double)]
    lib.mipt_bvh_build_device.restype = C.c_int
    lib.mipt_camera_from_pose.argtypes = [C.POINTER(f32 * 3), f32, f32, vp]
    lib.mipt_camera_from_pose.restype = C.c_int
    lib.mipt_material_default.argtypes = [vp]
    lib.mipt_material_default.restype = None
    lib.mipt_last_error.argtypes = []
    lib.mipt_last_error.restype = C.c_char_p
    lib.mipt_abi_version.argtypes = []
    lib.mipt_abi_version.restype = C.c_int
    lib.mipt_device_count.argtypes = []
    lib.mipt_device_count.restype = C.c_int
    lib.mipt_obj_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.mipt_obj_load.restype = C.c_int
    lib.mipt_obj_load_triangles.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.mipt_obj_load_triangles.restype = C.c_int
    lib.mipt_obj_free.argtypes = [vp]
    lib.mipt_obj_free.restype = None
    lib.mipt_obj_get.argtypes = [vp, C.POINTER(MiptSceneDesc), C.POINTER(C.POINTER(C.c_char_p))]
    lib.mipt_obj_get.restype = C.c_int
    lib.mipt_texture_load.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(MiptTexture), C.POINTER(u32)]
    lib.mipt_texture_load.restype = C.c_int
    lib.mipt_texture_free.argtypes = [vp]
    lib.mipt_texture_free.restype = None
    lib.mipt_image_save_png.argtypes = [C.c_char_p, u32, u32, u32, vp]
    lib.mipt_image_save_png.restype = C.c_int
    lib.mipt_multi_create.argtypes = [C.POINTER(MiptSceneDesc), vp, C.c_int, C.POINTER(vp)]
    lib.mipt_multi_create.restype = C.c_int
    lib.mipt_multi_destroy.argtypes = [vp]
    lib.mipt_multi_destroy.restype = None
    lib.mipt_multi_device_count.argtypes = [vp]
    lib.mipt_multi_device_count.restype = C.c_int
    lib.mipt_render_multi.argtypes = [vp, vp, C.POINTER(MiptOptions), u32, vp, vp, C.POINTER(MiptMultiStats)]
    lib.mipt_render_multi.restype = C.c_int
    lib.mipt_render_multi_device.argtypes = [vp, vp, C.POINTER(MiptOptions), u32, vp, vp, C.POINTER(MiptMultiStats)]
    lib.mipt_render_multi_device.restype = C.c_int
    lib.mipt_multi_root_device.argtypes = [vp]
    lib.mipt_multi_root_device.restype = C.c_int
    lib.mipt_multi_device_stats.argtypes = [vp, C.c_int, C.POINTER(MiptStats)]
    lib.mipt_multi_device_stats.restype = C.c_int
    lib.mipt_scene_create_from_triangles.argtypes = [C.POINTER(MiptSceneDesc), C.c_int, C.POINTER(vp)]
    lib.mipt_scene_create_from_triangles.restype = C.c_int
    lib.mipt_scene_get_bvh.argtypes = [vp, vp, u32, C.POINTER(u32), vp]
    lib.mipt_scene_get_bvh.restype = C.c_int
    lib.mipt_scene_info.argtypes = [vp, C.POINTER(MiptSceneInfo)]
    lib.mipt_scene_info.restype = C.c_int
    lib.mipt_multi_create_from_triangles.argtypes = [C.POINTER(MiptSceneDesc), vp, C.c_int, C.POINTER(vp)]
    lib.mipt_multi_create_from_triangles.restype = C.c_int
    lib.mipt_multi_scene.argtypes = [vp, C.c_int]
    lib.mipt_multi_scene.restype = vp
    lib.mipt_scene_update_triangles.argtypes = [vp, vp, u32, u32, C.POINTER(MiptUpdateInfo)]
    lib.mipt_scene_update_triangles.restype = C.c_int
    lib.mipt_scene_update_triangles_device.argtypes = [vp, vp, u32, u32, vp, C.POINTER(MiptUpdateInfo)]
    lib.mipt_scene_update_triangles_device.restype = C.c_int
    lib.mipt_multi_update_triangles.argtypes = [vp, vp, u32, u32, C.POINTER(MiptUpdateInfo)]
    lib.mipt_multi_update_triangles.restype = C.c_int
    lib.mipt_mesh_expand.argtypes = [C.POINTER(MiptMeshDesc), vp, u32, C.POINTER(u32)]
    lib.mipt_mesh_expand.restype = C.c_int
    lib.mipt_scene_create_from_mesh.argtypes = [C.POINTER(MiptSceneDesc), C.POINTER(MiptMeshDesc), C.c_int, C.POINTER(vp)]
    lib.mipt_scene_create_from_mesh.restype = C.c_int
    lib.mipt_scene_set_transforms.argtypes = [vp, vp, u32, u32, C.POINTER(MiptUpdateInfo)]
    lib.mipt_scene_set_transforms.restype = C.c_int
    lib.mipt_scene_update_mesh_device.argtypes = [vp, vp, vp, vp, u32, vp, C.POINTER(MiptUpdateInfo)]
    lib.mipt_scene_update_mesh_device.restype = C.c_int
    lib.mipt_scene_mesh_info.argtypes = [vp, C.POINTER(MiptMeshInfo)]
    lib.mipt_scene_mesh_info.restype = C.c_int
    qo = C.POINTER(MiptQueryOptions)
    lib.mipt_query_closest.argtypes = [vp, vp, u64, qo, vp, C.POINTER(MiptStats)]
    lib.mipt_query_closest.restype = C.c_int
    lib.mipt_query_closest_device.argtypes = [vp, vp, u64, qo, vp, vp, C.POINTER(MiptStats)]
    lib.mipt_query_closest_device.restype = C.c_int
    lib.mipt_query_occluded.argtypes = [vp, vp, u64, qo, vp, C.POINTER(MiptStats)]
    lib.mipt_query_occluded.restype = C.c_int
    lib.mipt_query_occluded_device.argtypes = [vp, vp, u64, qo, vp, vp, C.POINTER(MiptStats)]
    lib.mipt_query_occluded_device.restype = C.c_int
    ro = C.POINTER(MiptRadianceOptions)
    lib.mipt_query_radiance.argtypes = [vp, vp, u64, ro, vp, C.POINTER(MiptStats)]
    lib.mipt_query_radiance.restype = C.c_int
    lib.mipt_query_radiance_device.argtypes = [vp, vp, u64, ro, vp, vp, C.POINTER(MiptStats)]
    lib.mipt_query_radiance_device.restype = C.c_int
    bt, bi, bo = C.POINTER(MiptBakeTexelOptions), C.POINTER(MiptBakeTexelInfo), C.POINTER(MiptBakeOptions)
    lib.mipt_bake_texels.argtypes = [vp, u32, u32, bt, vp, bi]
    lib.mipt_bake_texels.restype = C.c_int
    lib.mipt_bake_texels_device.argtypes = [vp, u32, u32, bt, vp, vp, bi]
    lib.mipt_bake_texels_device.restype = C.c_int
    lib.mipt_bake_gather.argtypes = [vp, vp, u64, bo, vp, C.POINTER(MiptStats)]
    lib.mipt_bake_gather.restype = C.c_int
    lib.mipt_bake_gather_device.argtypes = [vp, vp, u64, bo, vp, vp, C.POINTER(MiptStats)]
    lib.mipt_bake_gather_device.restype = C.c_int
    bs = C.POINTER(MiptBakeSurfaceOptions)
    lib.mipt_bake_surface.argtypes = [vp, vp, u64, bs, vp, vp]
    lib.mipt_bake_surface.restype = C.c_int
    lib.mipt_bake_surface_device.argtypes = [vp, vp, u64, bs, vp, vp, vp]
    lib.mipt_bake_surface_device.restype = C.c_int
    lfo, lfb = C.POINTER(MiptLightmapFilterOptions), C.POINTER(MiptLightmapFilterBuffers)
    lib.mipt_lightmap_filter_workspace_bytes.argtypes = [u32, u32]
    lib.mipt_lightmap_filter_workspace_bytes.restype = u64
    lib.mipt_lightmap_filter.argtypes = [lfo, lfb, C.c_int]
    lib.mipt_lightmap_filter.restype = C.c_int
    lib.mipt_lightmap_filter_device.argtypes = [lfo, lfb, vp, u64, vp]
    lib.mipt_lightmap_filter_device.restype = C.c_int
    ldo, ldb = C.POINTER(MiptLightmapDilateOptions), C.POINTER(MiptLightmapDilateBuffers)
    lib.mipt_lightmap_dilate_workspace_bytes.argtypes = [u32, u32]
    lib.mipt_lightmap_dilate_workspace_bytes.restype = u64
    lib.mipt_lightmap_dilate.argtypes = [ldo, ldb, C.c_int]
    lib.mipt_lightmap_dilate.restype = C.c_int
    lib.mipt_lightmap_dilate_device.argtypes = [ldo, ldb, vp, u64, vp]
    lib.mipt_lightmap_dilate_device.restype = C.c_int
    pbo, pg, pib = C.POINTER(MiptProbeBakeOptions), C.POINTER(MiptProbeGrid), C.POINTER(MiptProbeIrradianceBuffers)
    lib.mipt_probe_bake.argtypes = [vp, vp, u64, pbo, vp, C.POINTER(MiptStats)]
    lib.mipt_probe_bake.restype = C.c_int
    lib.mipt_probe_bake_device.argtypes = [vp, vp, u64, pbo, vp, vp, C.POINTER(MiptStats)]
    lib.mipt_probe_bake_device.restype = C.c_int
    lib.mipt_probe_irradiance.argtypes = [pg, u64, pib, C.c_int]
    lib.mipt_probe_irradiance.restype = C.c_int
    lib.mipt_probe_irradiance_device.argtypes = [pg, u64, pib, vp]
    lib.mipt_probe_irradiance_device.restype = C.c_int
    fb = C.POINTER(MiptFeatureBuffers)
    lib.mipt_render_features.argtypes = [vp, vp, u32, C.POINTER(MiptOptions), fb, C.POINTER(MiptStats)]
    lib.mipt_render_features.restype = C.c_int
    lib.mipt_render_features_device.argtypes = [vp, vp, u32, C.POINTER(MiptOptions), fb, vp, C.POINTER(MiptStats)]
    lib.mipt_render_features_device.restype = C.c_int
    mb = C.POINTER(MiptMotionBuffers)
    lib.mipt_render_motion.argtypes = [vp, vp, u32, C.POINTER(MiptOptions), mb, C.POINTER(MiptStats)]
    lib.mipt_render_motion.restype = C.c_int
    lib.mipt_render_motion_device.argtypes = [vp, vp, u32, C.POINTER(MiptOptions), mb, vp, C.POINTER(MiptStats)]
    lib.mipt_render_motion_device.restype = C.c_int
    lib.mipt_scene_track_motion.argtypes = [vp, u32]
    lib.mipt_scene_track_motion.restype = C.c_int
    do, db = C.POINTER(MiptDenoiseOptions), C.POINTER(MiptDenoiseBuffers)
    lib.mipt_denoise_workspace_bytes.argtypes = [u32, u32, u32]
    lib.mipt_denoise_workspace_bytes.restype = u64
    lib.mipt_denoise.argtypes = [do, db, C.c_int]
    lib.mipt_denoise.restype = C.c_int
    lib.mipt_denoise_device.argtypes = [do, db, vp, u64, vp]
    lib.mipt_denoise_device.restype = C.c_int
    to, tb = C.POINTER(MiptTemporalOptions), C.POINTER(MiptTemporalBuffers)
    lib.mipt_temporal_history_bytes.argtypes = [u32, u32, u32]
    lib.mipt_temporal_history_bytes.restype = u64
    lib.mipt_temporal.argtypes = [to, vp, tb, C.c_int]
    lib.mipt_temporal.restype = C.c_int
    lib.mipt_temporal_device.argtypes = [to, vp, tb, vp]
    lib.mipt_temporal_device.restype = C.c_int
    lib.mipt_temporal_counts.argtypes = [to, vp, tb, vp, u32, C.c_int]
    lib.mipt_temporal_counts.restype = C.c_int
    lib.mipt_temporal_counts_device.argtypes = [to, vp, tb, vp, u32, vp]
    lib.mipt_temporal_counts_device.restype = C.c_int
    vo, vb = C.POINTER(MiptVarianceOptions), C.POINTER(MiptVarianceBuffers)
    lib.mipt_denoise_variance_workspace_bytes.argtypes = [u32, u32, u32]
    lib.mipt_denoise_variance_workspace_bytes.restype = u64
    lib.mipt_denoise_variance.argtypes = [vo, vb, C.c_int]
    lib.mipt_denoise_variance.restype = C.c_int
    lib.mipt_denoise_variance_device.argtypes = [vo, vb, vp, u64, vp]
    lib.mipt_denoise_variance_device.restype = C.c_int
    uo, ub = C.POINTER(MiptUpsampleOptions), C.POINTER(MiptUpsampleBuffers)
    lib.mipt_upsample_workspace_bytes.argtypes = [u32, u32, u32, u32]
    lib.mipt_upsample_workspace_bytes.restype = u64
    lib.mipt_upsample.argtypes = [uo, ub, C.c_int]
    lib.mipt_upsample.restype = C.c_int
    lib.mipt_upsample_device.argtypes = [uo, ub, vp, u64, vp]
    lib.mipt_upsample_device.restype = C.c_int
    lib.mipt_render_adaptive.argtypes = [vp, vp, u32, C.POINTER(MiptOptions), vp, vp, vp, C.POINTER(MiptStats)]
    lib.mipt_render_adaptive.restype = C.c_int
    lib.mipt_render_adaptive_device.argtypes = [vp, vp, u32, C.POINTER(MiptOptions), vp, vp, vp, vp, C.POINTER(MiptStats)]
    lib.mipt_render_adaptive_device.restype = C.c_int
    so, sb = C.POINTER(MiptSampleMapOptions), C.POINTER(MiptSampleMapBuffers)
    lib.mipt_sample_map_workspace_bytes.argtypes = [u32, u32, u32]
    lib.mipt_sample_map_workspace_bytes.restype = u64
    lib.mipt_sample_map.argtypes = [so, sb, C.c_int]
    lib.mipt_sample_map.restype = C.c_int
    lib.mipt_sample_map_device.argtypes = [so, sb, vp, vp]
    lib.mipt_sample_map_device.restype = C.c_int
    fo = C.POINTER(MiptSampleMapFillOptions)
    lib.mipt_sample_map_fill_workspace_bytes.argtypes = [u32, u32, u32, u32]
    lib.mipt_sample_map_fill_workspace_bytes.restype = u64
    lib.mipt_sample_map_fill.argtypes = [fo, sb, C.c_int]
    lib.mipt_sample_map_fill.restype = C.c_int
    lib.mipt_sample_map_fill_device.argtypes = [fo, sb, vp, vp]
    lib.mipt_sample_map_fill_device.restype = C.c_int
    return lib


MULTITEST_LIB_PATH = os.path.join(_HERE, "libmipt_multitest.so")
_multitest = None


def load_multitest() -> C.CDLL:
    """libmipt_multitest.so: the product's objects with mipt_multi.cpp compiled against the RCCL TEST DOUBLE of
    tests/cpp/rccl_double/ (N logical ranks on one device).  Test infrastructure: lets the n > 1 code of mipt_render_multi run on
    the one-GPU box.  Same C ABI (+ rccl_double_inject); its own error string and device state."""
    global _multitest
    if _multitest is not None:
        return _multitest
    load()
    if not os.path.exists(MULTITEST_LIB_PATH):
        raise ImportError(f"{MULTITEST_LIB_PATH} is missing: run __graft_entry__.build()")
    lib = _bind(C.CDLL(MULTITEST_LIB_PATH))
    lib.rccl_double_inject.argtypes = [C.c_int, C.c_int]
    lib.rccl_double_inject.restype = C.c_longlong
    _multitest = lib
    return lib


DIAG_LIB_PATH = os.path.join(_HERE, "libmipt_diag.so")
DIAG_EXPORTS = ["mipt_debug_eval", "mipt_debug_eval_range", "mipt_debug_wgsl", "mipt_debug_texel", "mipt_debug_divide", "mipt_debug_popcount", "mipt_debug_tile_order", "mipt_diag_scene_tile_order", "mipt_debug_hot_select", "mipt_diag_scene_hot_pixels", "mipt_diag_scene_list", "mipt_diag_scene_hot_bits", "mipt_diag_scene_cost_atomics", "mipt_diag_last_error",
                "mipt_internal_pair_order", "mipt_internal_pair_order_top", "mipt_internal_tri_slots",
                "mipt_diag_scene_sizes", "mipt_diag_scene_tables", "mipt_diag_scene_read", "mipt_diag_scene_hash", "mipt_diag_write_obj", "mipt_diag_host_layout", "mipt_diag_hash_words"]
_diag = None


def load_diag() -> C.CDLL:
    """libmipt_diag.so (include/mipt_diag.h): the device-arithmetic probe the GPU known-answer tests use and the
    re-exported layout functions (pair-record order, triangle slots).  Test infrastructure; the product library exports none of it."""
    global _diag
    if _diag is not None:
        return _diag
    load()
    if not os.path.exists(DIAG_LIB_PATH):
        raise ImportError(f"{DIAG_LIB_PATH} is missing: run __graft_entry__.build()")
    lib = C.CDLL(DIAG_LIB_PATH)
    vp = C.c_void_p
    lib.mipt_debug_eval.argtypes = [C.c_int, vp, vp, C.c_uint64, vp]
    lib.mipt_debug_eval.restype = C.c_int
    lib.mipt_debug_eval_range.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_float, vp]
    lib.mipt_debug_eval_range.restype = C.c_int
    lib.mipt_debug_wgsl.argtypes = [C.c_int, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, vp]
    lib.mipt_debug_wgsl.restype = C.c_int
    lib.mipt_debug_texel.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.POINTER(C.c_uint64)]
    lib.mipt_debug_texel.restype = C.c_int
    lib.mipt_debug_divide.argtypes = [vp, C.c_uint64, C.c_float, vp]
    lib.mipt_debug_divide.restype = C.c_int
    lib.mipt_debug_popcount.argtypes = [vp, C.c_uint64, vp, vp]
    lib.mipt_debug_popcount.restype = C.c_int
    lib.mipt_debug_tile_order.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    lib.mipt_debug_tile_order.restype = C.c_int
    lib.mipt_diag_scene_tile_order.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(C.c_uint32 * 3)]
    lib.mipt_diag_scene_tile_order.restype = C.c_int
    lib.mipt_debug_hot_select.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
    lib.mipt_debug_hot_select.restype = C.c_int
    lib.mipt_diag_scene_hot_pixels.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.POINTER(C.c_uint32 * 3)]
    lib.mipt_diag_scene_hot_pixels.restype = C.c_int
    lib.mipt_diag_scene_list.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32 * 2)]
    lib.mipt_diag_scene_list.restype = C.c_int
    lib.mipt_diag_scene_hot_bits.argtypes = [vp, vp, C.c_uint32]
    lib.mipt_diag_scene_hot_bits.restype = C.c_int
    lib.mipt_diag_scene_cost_atomics.argtypes = [vp, C.c_int]
    lib.mipt_diag_scene_cost_atomics.restype = C.c_int
    lib.mipt_diag_last_error.argtypes = []
    lib.mipt_diag_last_error.restype = C.c_char_p
    u32p = C.POINTER(C.c_uint32)
    lib.mipt_internal_pair_order.argtypes = [vp, C.c_uint32, vp, C.c_uint32, u32p]
    lib.mipt_internal_pair_order.restype = C.c_int
    lib.mipt_internal_pair_order_top.argtypes = []
    lib.mipt_internal_pair_order_top.restype = C.c_uint32
    lib.mipt_internal_tri_slots.argtypes = [vp, C.c_uint32, C.c_uint32, vp, u32p]
    lib.mipt_internal_tri_slots.restype = C.c_int
    lib.mipt_diag_scene_sizes.argtypes = [vp, C.POINTER(C.c_uint64 * 2)]
    lib.mipt_diag_scene_sizes.restype = C.c_int
    lib.mipt_diag_scene_tables.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    lib.mipt_diag_scene_tables.restype = C.c_int
    lib.mipt_diag_scene_read.argtypes = [vp, C.c_int, vp, C.c_uint64]
    lib.mipt_diag_scene_read.restype = C.c_int
    lib.mipt_diag_scene_hash.argtypes = [vp, C.POINTER(C.c_uint64 * 2)]
    lib.mipt_diag_scene_hash.restype = C.c_int
    lib.mipt_diag_write_obj.argtypes = [C.c_char_p, vp, C.c_uint64, C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32]
    lib.mipt_diag_write_obj.restype = C.c_int
    lib.mipt_diag_host_layout.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64 * 2), C.POINTER(C.c_uint32 * 4)]
    lib.mipt_diag_host_layout.restype = C.c_int
    lib.mipt_diag_hash_words.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.mipt_diag_hash_words.restype = C.c_int
    _diag = lib
    return lib


class MiptError(RuntimeError):
    def __init__(self, code: int, where: str):
        self.code = code
        msg = load().mipt_last_error()
        super().__init__(f"{where} failed with status {code}: {msg.decode() if msg else ''}")


def check(code: int, where: str) -> None:
    if code != 0:
        raise MiptError(code, where)


def ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)
