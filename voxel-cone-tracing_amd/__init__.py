"""Thin ctypes binding of libvct_amd.so (the C ABI in include/vct.h).

The directory name carries a hyphen, so import it through `vctpkg.load()` (repo root) or
importlib; the module registers itself as `voxel_cone_tracing_amd`.  There is no Python or CPU
implementation of any kernel here: if the HIP library is missing, import fails.
"""
import ctypes as C
import os

import numpy as np

try:
    # torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's): whichever is loaded
    # first serves the whole process, and torch breaks on the other one.  Load torch's first so
    # that torch tensors, streams and this library share one HIP runtime.
    import torch  # noqa: F401
except ImportError:  # pure ctypes use without torch is fine
    pass

_HERE = os.path.dirname(os.path.abspath(__file__))
# VCT_AMD_LIB: path of an alternative build of the same library (A/B experiments only)
LIB_PATH = os.environ.get("VCT_AMD_LIB") or os.path.join(_HERE, "libvct_amd.so")

GB_PLANES = 23
GB_LINEAR, GB_TILED = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1
VOX_CONSERVATIVE_AVG, VOX_REFERENCE = 0, 1
ABI_VERSION = 8
# lighting components (include/vct.h: the reference's Show* switches) and per-component outputs
SHOW_DIFFUSE, SHOW_INDIRECT_DIFFUSE, SHOW_SPECULAR, SHOW_INDIRECT_SPECULAR, SHOW_AMBIENT_OCCLUSION = 1, 2, 4, 8, 16
SHOW_ALL = 31
AOV_INDIRECT_DIFFUSE, AOV_INDIRECT_SPECULAR, AOV_DIRECT = 1, 2, 4
# sources of the voxel view (Context.render_voxels)
VOXVIEW_CURRENT, VOXVIEW_RADIANCE, VOXVIEW_ALBEDO, VOXVIEW_NORMAL = 0, 1, 2, 3
# point queries (Context.gather_points / cone_points)
QUERY_SORT_CELLS = 1
POINT_QUERY_MAX = 1 << 26
APERTURE_DIFFUSE, APERTURE_SPECULAR = 0, 1
# per-material gloss (Context.set_gloss_classes)
GLOSS_CLASSES_MAX = 8
# G-buffer import (Context.import_gbuffer): input formats and flags of include/vct.h "G-buffer import"
IMPORT_POSITION_F32X3, IMPORT_POSITION_F32X4, IMPORT_DEPTH_F32 = 0, 1, 2
IMPORT_NORMAL_F32X3, IMPORT_NORMAL_F16X4, IMPORT_NORMAL_OCT_SNORM16X2 = 0, 1, 2
IMPORT_COLOR_UNORM8X4, IMPORT_COLOR_F16X4, IMPORT_COLOR_F32X4 = 0, 1, 2
IMPORT_FLIP_Y, IMPORT_DEPTH_ZERO_TO_ONE, IMPORT_OPAQUE = 1, 2, 4


def APERTURE_GLOSS(k):
    """aperture of cone_points that marches with gloss class k's step table (include/vct.h VCT_APERTURE_GLOSS)"""
    return 2 + int(k)


# every symbol include/vct.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "vct_default_config", "vct_create", "vct_destroy", "vct_last_error", "vct_get_config",
    "vct_set_camera_position", "vct_set_light_direction", "vct_set_ambient_factor",
    "vct_set_cone_apertures", "vct_set_trace_variant", "vct_trace_resident_strided", "vct_comm_set_interleaved",
    "vct_selftest_interleaved", "vct_upload_triangles", "vct_upload_shadow_map", "vct_voxelize",
    "vct_inject_light", "vct_build_mips", "vct_upload_volume_rgba8", "vct_upload_chain_rgba8",
    "vct_download_chain_rgba8", "vct_chain_texels", "vct_trace", "vct_trace_slab",
    "vct_trace_resident", "vct_synchronize", "vct_download_steps", "vct_download_cones",
    "vct_last_step_count", "vct_last_trace_ms", "vct_get_stream", "vct_get_frame_device",
    "vct_selftest_const_divide", "vct_selftest_area_divide", "vct_set_frame_target", "vct_bounce",
    "vct_download_voxel_attributes", "vct_download_aniso_rgba8", "vct_upload_mesh_attributes", "vct_render_shadow_map",
    "vct_download_shadow_map", "vct_render_gbuffer", "vct_download_gbuffer", "vct_trace_current", "vct_trace_resident_rows",
    "vct_last_trace_stats", "vct_download_frame", "vct_render_gbuffer_rows",
    "vct_slab_partition", "vct_comm_get_unique_id", "vct_comm_init", "vct_comm_destroy", "vct_comm_slab",
    "vct_frame_step", "vct_comm_sync", "vct_comm_frame", "vct_comm_download_frame",
    "vct_upload_mesh_uvs", "vct_upload_textures", "vct_gi_pass",
    "vct_comm_set_timeout_ms", "vct_last_row_steps", "vct_slab_partition_weighted", "vct_comm_set_slab_rows",
    "vct_get_stage_counts", "vct_comm_info", "vct_comm_last_gather_ms", "vct_set_footprint_records",
    "vct_set_frames_in_flight", "vct_get_frames_in_flight", "vct_select_frame_slot", "vct_selftest_texel_buffer",
    "vct_set_trace_timing", "vct_set_lighting_components", "vct_get_lighting_components", "vct_set_aov_outputs",
    "vct_download_aov", "vct_get_aov_device", "vct_set_diffuse_rate", "vct_get_diffuse_rate", "vct_last_diffuse_rate_ms",
    "vct_render_voxels", "vct_last_voxel_view_ms",
    "vct_gather_points", "vct_cone_points", "vct_last_point_query", "vct_last_point_query_ms",
    "vct_upload_emission", "vct_set_pixel_emission", "vct_download_pixel_emission",
    "vct_set_gloss_classes", "vct_get_gloss_classes", "vct_upload_material_gloss", "vct_set_pixel_gloss",
    "vct_download_pixel_gloss",
    "vct_set_sky", "vct_get_sky",
    "vct_import_gbuffer", "vct_import_gbuffer_rows", "vct_last_gbuffer_import_ms",
    "vct_set_lights", "vct_get_lights", "vct_download_pixel_lights", "vct_last_lights_ms",
    "vct_set_dynamic_mesh", "vct_update_dynamic_positions", "vct_get_dynamic", "vct_download_dynamic_voxels",
    "vct_last_dynamic_ms", "vct_set_dynamic_draw", "vct_get_dynamic_draw",
    "vct_set_dynamic_bounce", "vct_get_dynamic_bounce", "vct_set_dynamic_emission", "vct_get_dynamic_emission",
    "vct_set_dynamic_parts", "vct_get_dynamic_parts", "vct_update_dynamic_transforms", "vct_download_dynamic_positions",
    "vct_last_dynamic_transform_ms", "vct_set_dynamic_skin", "vct_get_dynamic_skin",
    "vct_set_dynamic_normals", "vct_update_dynamic_normals", "vct_get_dynamic_normals", "vct_download_dynamic_frames",
]


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("device", C.c_int32), ("voxel_dim", C.c_int32),
        ("grid_world_size", C.c_float), ("width", C.c_int32), ("height", C.c_int32),
        ("shadow_map_size", C.c_int32), ("model_scale", C.c_float),
        ("ambient_factor", C.c_float), ("shininess", C.c_float), ("max_distance", C.c_float),
        ("max_alpha", C.c_float), ("tan_diffuse", C.c_float), ("tan_specular", C.c_float),
        ("wrap_repeat", C.c_int32), ("debug_outputs", C.c_int32), ("trace_variant", C.c_int32),
        ("voxel_attributes", C.c_int32), ("anisotropic_mips", C.c_int32), ("texture_mipmaps", C.c_int32),
    ]


class GlossClass(C.Structure):
    _fields_ = [("tan_specular", C.c_float), ("shininess", C.c_float)]


LIGHTS_MAX = 64
LIGHT_SPOT = 1
DYNAMIC_DRAW_SHADOW, DYNAMIC_DRAW_GBUFFER = 1, 2      # vct_set_dynamic_draw
DYNAMIC_PARTS_MAX = 1 << 16                           # VCT_DYNAMIC_PARTS_MAX (vct_set_dynamic_parts)
DYNAMIC_BONES_MAX = 1 << 16                           # VCT_DYNAMIC_BONES_MAX (vct_set_dynamic_skin)


class Light(C.Structure):
    """vct_light of include/vct.h (56 B)"""
    _fields_ = [("position", C.c_float * 3), ("radius", C.c_float), ("color", C.c_float * 3), ("source_radius", C.c_float),
                ("direction", C.c_float * 3), ("cos_outer", C.c_float), ("cos_inner", C.c_float), ("flags", C.c_uint32)]


def point_light(position, color, radius, source_radius):
    """A point light as Context.set_lights takes it."""
    return dict(position=tuple(position), color=tuple(color), radius=radius, source_radius=source_radius)


def spot_light(position, color, radius, source_radius, direction, cos_inner, cos_outer):
    """A spot light: axis `direction` (any length), cosines of the inner / outer half angle."""
    return dict(position=tuple(position), color=tuple(color), radius=radius, source_radius=source_radius,
                direction=tuple(direction), cos_inner=cos_inner, cos_outer=cos_outer, flags=LIGHT_SPOT)


class GBuffer(C.Structure):
    _fields_ = [("planes", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("layout", C.c_int32), ("location", C.c_int32)]


class GBufferImport(C.Structure):
    """vct_gbuffer_import of include/vct.h"""
    _fields_ = [("position", C.c_void_p), ("normal", C.c_void_p), ("shading_normal", C.c_void_p),
                ("albedo", C.c_void_p), ("specular", C.c_void_p), ("shadow", C.c_void_p), ("material", C.c_void_p),
                ("position_format", C.c_int32), ("normal_format", C.c_int32), ("albedo_format", C.c_int32),
                ("specular_format", C.c_int32), ("location", C.c_int32), ("flags", C.c_uint32),
                ("inv_view_proj", C.c_float * 16), ("depth_clear", C.c_float), ("normal_scale", C.c_float),
                ("specular_constant", C.c_float * 3)]


class VctError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make lib` (hipcc --offload-arch=gfx950). "
        "There is no CPU fallback for the voxel-cone-tracing path.")

_lib = C.CDLL(LIB_PATH)
_lib.vct_last_error.restype = C.c_char_p
_lib.vct_last_error.argtypes = [C.c_void_p]
_lib.vct_chain_texels.restype = C.c_size_t
_lib.vct_chain_texels.argtypes = [C.c_int32]
_lib.vct_destroy.restype = None
_lib.vct_destroy.argtypes = [C.c_void_p]
_lib.vct_create.argtypes = [C.c_void_p, C.c_void_p]
for _n in ("vct_set_camera_position", "vct_set_light_direction", "vct_upload_volume_rgba8",
           "vct_upload_chain_rgba8", "vct_download_chain_rgba8", "vct_download_aniso_rgba8", "vct_download_steps",
           "vct_download_cones", "vct_last_step_count", "vct_last_trace_ms", "vct_last_trace_stats", "vct_get_stream",
           "vct_get_config"):
    getattr(_lib, _n).argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_ambient_factor.argtypes = [C.c_void_p, C.c_float]
_lib.vct_set_cone_apertures.argtypes = [C.c_void_p, C.c_float, C.c_float]
_lib.vct_set_trace_variant.argtypes = [C.c_void_p, C.c_int32]
_lib.vct_trace_resident_strided.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
_lib.vct_comm_set_interleaved.argtypes = [C.c_void_p, C.c_int32]
_lib.vct_selftest_interleaved.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
_lib.vct_upload_triangles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                      C.c_int32]
_lib.vct_upload_shadow_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
_lib.vct_voxelize.argtypes = [C.c_void_p, C.c_int32]
_lib.vct_download_voxel_attributes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_upload_mesh_attributes.argtypes = [C.c_void_p] * 5
for _n in ("vct_render_shadow_map", "vct_download_shadow_map", "vct_render_gbuffer", "vct_download_gbuffer",
           "vct_download_frame"):
    getattr(_lib, _n).argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_trace_current.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
_lib.vct_trace_resident_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
_lib.vct_gi_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
_lib.vct_gi_pass.restype = C.c_int
for _n in ("vct_inject_light", "vct_build_mips", "vct_trace_resident", "vct_synchronize", "vct_bounce"):
    getattr(_lib, _n).argtypes = [C.c_void_p]
_lib.vct_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
_lib.vct_trace_slab.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
_lib.vct_get_frame_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_set_frame_target.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_selftest_const_divide.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
_lib.vct_selftest_area_divide.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
_lib.vct_render_gbuffer_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
_lib.vct_slab_partition.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_comm_get_unique_id.argtypes = [C.c_void_p]
_lib.vct_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
_lib.vct_comm_slab.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_comm_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_comm_download_frame.argtypes = [C.c_void_p, C.c_void_p]
for _n in ("vct_comm_destroy", "vct_frame_step", "vct_comm_sync"):
    getattr(_lib, _n).argtypes = [C.c_void_p]
COMM_ID_BYTES = 128
_lib.vct_get_stage_counts.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_comm_set_timeout_ms.argtypes = [C.c_void_p, C.c_int32]
_lib.vct_set_footprint_records.argtypes = [C.c_void_p, C.c_int32]
_lib.vct_comm_info.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_comm_last_gather_ms.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_last_row_steps.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
_lib.vct_slab_partition_weighted.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
_lib.vct_comm_set_slab_rows.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_upload_mesh_uvs.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_frames_in_flight.argtypes = [C.c_void_p, C.c_int32]
_lib.vct_get_frames_in_flight.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_select_frame_slot.argtypes = [C.c_void_p, C.c_int32]
_lib.vct_set_trace_timing.argtypes = [C.c_void_p, C.c_int32]
_lib.vct_selftest_texel_buffer.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_lighting_components.argtypes = [C.c_void_p, C.c_uint32]
_lib.vct_get_lighting_components.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_aov_outputs.argtypes = [C.c_void_p, C.c_uint32]
_lib.vct_download_aov.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
_lib.vct_get_aov_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
_lib.vct_set_diffuse_rate.argtypes = [C.c_void_p, C.c_int32]
_lib.vct_get_diffuse_rate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_last_diffuse_rate_ms.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_render_voxels.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
_lib.vct_last_voxel_view_ms.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_gather_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
_lib.vct_cone_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32]
_lib.vct_last_point_query.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_last_point_query_ms.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_upload_emission.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_pixel_emission.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
_lib.vct_download_pixel_emission.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_gloss_classes.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
_lib.vct_get_gloss_classes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_upload_material_gloss.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_pixel_gloss.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
_lib.vct_download_pixel_gloss.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_sky.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_get_sky.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_import_gbuffer.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_import_gbuffer_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
_lib.vct_last_gbuffer_import_ms.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
_lib.vct_get_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_download_pixel_lights.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_last_lights_ms.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_dynamic_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
_lib.vct_update_dynamic_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
_lib.vct_get_dynamic.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_download_dynamic_voxels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_last_dynamic_ms.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_dynamic_draw.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
_lib.vct_get_dynamic_draw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_set_dynamic_bounce.argtypes = [C.c_void_p, C.c_int32]
_lib.vct_get_dynamic_bounce.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_dynamic_emission.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_get_dynamic_emission.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_set_dynamic_parts.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
_lib.vct_get_dynamic_parts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_update_dynamic_transforms.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
_lib.vct_download_dynamic_positions.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_last_dynamic_transform_ms.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_set_dynamic_skin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
_lib.vct_get_dynamic_skin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_set_dynamic_normals.argtypes = [C.c_void_p, C.c_void_p]
_lib.vct_update_dynamic_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
_lib.vct_get_dynamic_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_download_dynamic_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.vct_upload_textures.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]


def lib():
    return _lib


def default_config(**kw):
    cfg = Config()
    _lib.vct_default_config(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def slab_partition(height, world, rank):
    """(tile_row0, tile_row1, rows_per_rank) of rank's slab: equal padded slabs of ceil(tile_rows / world)."""
    r0, r1, per = C.c_int32(), C.c_int32(), C.c_int32()
    if _lib.vct_slab_partition(height, world, rank, C.byref(r0), C.byref(r1), C.byref(per)) != 0:
        raise VctError("vct_slab_partition: bad arguments")
    return r0.value, r1.value, per.value


def slab_partition_weighted(row_cost, world):
    """Tile-row boundaries [world + 1] of `world` contiguous slabs of near-equal cost (row_cost: per tile row)."""
    cost = np.ascontiguousarray(row_cost, np.uint64)
    starts = np.zeros(world + 1, np.int32)
    if _lib.vct_slab_partition_weighted(_ptr(cost), cost.shape[0], world, _ptr(starts)) != 0:
        raise VctError("vct_slab_partition_weighted: bad arguments")
    return starts


def comm_unique_id():
    """ncclGetUniqueId as 128 bytes (rank 0 creates it, every rank passes it to Context.comm_init)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    rc = _lib.vct_comm_get_unique_id(buf)
    if rc != 0:
        raise VctError(f"vct_comm_get_unique_id failed ({rc}): {_lib.vct_last_error(None).decode()}")
    return bytes(buf)


def chain_texels(V):
    return _lib.vct_chain_texels(V)


def _plane_elems(cfg, layout, nplanes):
    """Elements of `nplanes` per-pixel planes of the frame in a layout: linear [nplanes, h*w] or tiled [tiles, nplanes, 64]."""
    if layout == GB_LINEAR:
        return nplanes * cfg.width * cfg.height
    return ((cfg.width + 7) // 8) * ((cfg.height + 7) // 8) * nplanes * 64


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    return a.ctypes.data_as(C.c_void_p)


def _dynamic_normals_array(self, who, nrm):
    """nrm as float32 [ntri, 3, 3] (or [ntri, 9]) of the attached mesh, checked before any pointer is handed over"""
    nrm = np.ascontiguousarray(nrm, np.float32)
    ntri = getattr(self, "_dyn_ntri", 0)
    shaped = (nrm.ndim == 3 and nrm.shape[1:] == (3, 3)) or (nrm.ndim == 2 and nrm.shape[1] == 9)
    if not shaped or (ntri and nrm.shape[0] != ntri):          # (no mesh attached: the library refuses)
        raise VctError(f"{who}: normals of shape {tuple(nrm.shape)}, the attached dynamic mesh has {ntri} triangles: "
                       f"[{ntri}, 3, 3] is expected")
    return nrm


class Context:
    """One context per GPU; mirrors the call order of the reference's orchestrator
    (ctor -> init: voxelize, inject, mips -> Render per frame; VCT.h:57-190)."""

    def __init__(self, cfg=None, **kw):
        cfg = cfg or default_config(**kw)
        self._h = C.c_void_p()
        rc = _lib.vct_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            raise VctError(f"vct_create failed ({rc}): {_lib.vct_last_error(None).decode()}")
        self.cfg = Config()
        _lib.vct_get_config(self._h, C.byref(self.cfg))

    def current_config(self):
        """The configuration as the setters have left it (`cfg` is the one the context was created with)."""
        cfg = Config()
        self._ck(_lib.vct_get_config(self._h, C.byref(cfg)), "vct_get_config")
        return cfg

    def close(self):
        if self._h:
            _lib.vct_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc, what):
        if rc != 0:
            raise VctError(f"{what} failed ({rc}): {_lib.vct_last_error(self._h).decode()}")

    # --- uniforms
    def set_camera_position(self, pos):
        a = np.ascontiguousarray(pos, np.float32)
        self._ck(_lib.vct_set_camera_position(self._h, _ptr(a)), "vct_set_camera_position")

    def set_light_direction(self, d):
        a = np.ascontiguousarray(d, np.float32)
        self._ck(_lib.vct_set_light_direction(self._h, _ptr(a)), "vct_set_light_direction")

    def set_ambient_factor(self, a):
        self._ck(_lib.vct_set_ambient_factor(self._h, float(a)), "vct_set_ambient_factor")

    def set_cone_apertures(self, td, ts):
        self._ck(_lib.vct_set_cone_apertures(self._h, float(td), float(ts)), "vct_set_cone_apertures")

    def set_footprint_records(self, on=True):
        """One 32-byte footprint record per texel of the levels >= 1 (include/vct.h): for HBM-bound volumes."""
        self._ck(_lib.vct_set_footprint_records(self._h, int(bool(on))), "vct_set_footprint_records")

    def set_trace_variant(self, variant):
        self._ck(_lib.vct_set_trace_variant(self._h, int(variant)), "vct_set_trace_variant")

    def set_lighting_components(self, mask):
        """SHOW_* bits of the composite (the reference's Show* switches; default SHOW_ALL): from the next trace on."""
        self._ck(_lib.vct_set_lighting_components(self._h, int(mask)), "vct_set_lighting_components")

    def lighting_components(self):
        v = C.c_uint32()
        self._ck(_lib.vct_get_lighting_components(self._h, C.byref(v)), "vct_get_lighting_components")
        return v.value

    def set_aov_outputs(self, which):
        """AOV_* bits: per-component RGBA16F frames beside the frame, for every frame slot (0 frees them)."""
        self._ck(_lib.vct_set_aov_outputs(self._h, int(which)), "vct_set_aov_outputs")

    def download_aov(self, bit):
        """One per-component output (one AOV_* bit) of the selected slot: uint16 [h, w, 4] (fp16 bits)."""
        out = np.zeros((self.cfg.height, self.cfg.width, 4), np.uint16)
        self._ck(_lib.vct_download_aov(self._h, int(bit), _ptr(out)), "vct_download_aov")
        return out

    def aov_device(self, bit):
        """(device pointer, bytes) of one per-component output of the selected slot (zero-copy consumers)."""
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(_lib.vct_get_aov_device(self._h, int(bit), C.byref(p), C.byref(n)), "vct_get_aov_device")
        return p.value, n.value

    def set_diffuse_rate(self, rate):
        """1 (default): every pixel marches its six diffuse cones; 2: one pixel per 2x2 quad does and the others take a
        depth- and normal-aware mean of the nearest four (include/vct.h).  From the next whole-frame trace on."""
        self._ck(_lib.vct_set_diffuse_rate(self._h, int(rate)), "vct_set_diffuse_rate")

    def diffuse_rate(self):
        """(rate, pixels whose diffuse cones the last trace marched: anchors + fill pixels; 0 at rate 1).  Waits."""
        r, n = C.c_int32(), C.c_uint64()
        self._ck(_lib.vct_get_diffuse_rate(self._h, C.byref(r), C.byref(n)), "vct_get_diffuse_rate")
        return r.value, n.value

    def last_diffuse_rate_ms(self):
        """Device ms of the last rate-2 pass's launches: (coarse march, resolve, fill march, specular trace + composite)."""
        v = (C.c_float * 4)()
        self._ck(_lib.vct_last_diffuse_rate_ms(self._h, v), "vct_last_diffuse_rate_ms")
        return tuple(float(x) for x in v)

    # --- scene / volume
    def upload_triangles(self, pos, material, albedo):
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
        material = np.ascontiguousarray(material, np.int32)
        albedo = np.ascontiguousarray(albedo, np.float32).reshape(-1, 4)
        self._ck(_lib.vct_upload_triangles(self._h, _ptr(pos), _ptr(material), pos.shape[0],
                                           _ptr(albedo), albedo.shape[0]), "vct_upload_triangles")
        self._nmat = albedo.shape[0]            # what upload_emission checks its table against (the C side reads nmat rows)

    def upload_emission(self, emission):
        """Material emission [nmat, 3] (fp32 RGB, finite, >= 0) of the uploaded mesh; None or an all-zero table detaches.
        Shows in the chain after the next voxelize + inject_light (+ build_mips), in the frame after the next G-buffer pass."""
        if emission is None:
            self._ck(_lib.vct_upload_emission(self._h, None), "vct_upload_emission")
            return
        emission = np.ascontiguousarray(emission, np.float32).reshape(-1, 3)
        nmat = getattr(self, "_nmat", None)
        if nmat is not None and emission.shape[0] != nmat:
            raise VctError(f"upload_emission: {emission.shape[0]} rows, the uploaded mesh has {nmat} materials")
        self._ck(_lib.vct_upload_emission(self._h, _ptr(emission)), "vct_upload_emission")

    def set_pixel_emission(self, planes, layout=GB_LINEAR):
        """Pixel-emission planes of the selected frame slot: a float32 array (linear [3, h*w] or tiled [tiles, 3, 64]) or
        an int device pointer; None detaches.  Every following trace adds them to the frame's rgb."""
        if planes is None:
            self._ck(_lib.vct_set_pixel_emission(self._h, None, GB_LINEAR, MEM_HOST), "vct_set_pixel_emission")
            return
        if isinstance(planes, int):
            self._ck(_lib.vct_set_pixel_emission(self._h, _ptr(planes), layout, MEM_DEVICE), "vct_set_pixel_emission")
            return
        planes = np.ascontiguousarray(planes, np.float32)
        want = _plane_elems(self.cfg, layout, 3)
        if planes.size != want:
            raise VctError(f"set_pixel_emission: {planes.size} floats, this layout of the frame has {want}")
        self._ck(_lib.vct_set_pixel_emission(self._h, _ptr(planes), layout, MEM_HOST), "vct_set_pixel_emission")

    def download_pixel_emission(self):
        """The selected slot's pixel-emission planes, float32 [3, h*w] (linear)."""
        out = np.zeros((3, self.cfg.width * self.cfg.height), np.float32)
        self._ck(_lib.vct_download_pixel_emission(self._h, _ptr(out)), "vct_download_pixel_emission")
        return out

    # --- per-material gloss (include/vct.h "per-material gloss")
    def set_gloss_classes(self, classes):
        """Gloss classes [(tan_specular, shininess), ...], 1 .. 8 of them; None or an empty list detaches.  Every frame
        slot gets a zeroed pixel-gloss plane: class 0 everywhere until a G-buffer pass or set_pixel_gloss writes it."""
        if classes is None or len(classes) == 0:
            self._ck(_lib.vct_set_gloss_classes(self._h, None, 0), "vct_set_gloss_classes")
            return
        a = np.ascontiguousarray(classes, np.float32).reshape(-1, 2)
        self._ck(_lib.vct_set_gloss_classes(self._h, _ptr(a), a.shape[0]), "vct_set_gloss_classes")

    def get_gloss_classes(self):
        """(classes float32 [n, 2], march steps int32 [n]) of the attached table; n = 0: none attached."""
        out, n, steps = np.zeros((GLOSS_CLASSES_MAX, 2), np.float32), C.c_int32(), np.zeros(GLOSS_CLASSES_MAX, np.int32)
        self._ck(_lib.vct_get_gloss_classes(self._h, _ptr(out), C.byref(n), _ptr(steps)), "vct_get_gloss_classes")
        return out[:n.value].copy(), steps[:n.value].copy()

    def upload_material_gloss(self, mat_class):
        """Gloss class per material of the uploaded mesh, uint8 [nmat]; None detaches.  The G-buffer passes then write the
        selected slot's pixel-gloss plane."""
        if mat_class is None:
            self._ck(_lib.vct_upload_material_gloss(self._h, None), "vct_upload_material_gloss")
            return
        m = np.ascontiguousarray(mat_class)
        if m.dtype != np.uint8:
            if m.size and (m.min() < 0 or m.max() > 255):
                raise VctError("upload_material_gloss: classes are bytes (0 .. 255)")
            m = m.astype(np.uint8)
        m = m.reshape(-1)
        nmat = getattr(self, "_nmat", None)
        if nmat is not None and m.shape[0] != nmat:
            raise VctError(f"upload_material_gloss: {m.shape[0]} entries, the uploaded mesh has {nmat} materials")
        self._ck(_lib.vct_upload_material_gloss(self._h, _ptr(m)), "vct_upload_material_gloss")

    def set_pixel_gloss(self, classes, layout=GB_LINEAR):
        """Pixel-gloss plane of the selected frame slot: a uint8 array (linear [h*w] or tiled [tiles, 64]) or an int device
        pointer; None zeroes the plane.  Needs gloss classes attached."""
        if classes is None:
            self._ck(_lib.vct_set_pixel_gloss(self._h, None, GB_LINEAR, MEM_HOST), "vct_set_pixel_gloss")
            return
        if isinstance(classes, int):
            self._ck(_lib.vct_set_pixel_gloss(self._h, _ptr(classes), layout, MEM_DEVICE), "vct_set_pixel_gloss")
            return
        classes = np.ascontiguousarray(classes, np.uint8)
        want = _plane_elems(self.cfg, layout, 1)
        if classes.size != want:
            raise VctError(f"set_pixel_gloss: {classes.size} bytes, this layout of the frame has {want}")
        self._ck(_lib.vct_set_pixel_gloss(self._h, _ptr(classes), layout, MEM_HOST), "vct_set_pixel_gloss")

    def download_pixel_gloss(self):
        """The selected slot's pixel-gloss plane, uint8 [h*w] (linear), bytes as stored (unclamped)."""
        out = np.zeros(self.cfg.width * self.cfg.height, np.uint8)
        self._ck(_lib.vct_download_pixel_gloss(self._h, _ptr(out)), "vct_download_pixel_gloss")
        return out

    # --- sky light (include/vct.h "sky light")
    def set_sky(self, sh):
        """The context's sky: float32 [9, 3] real spherical-harmonic coefficients (orthonormal basis, world axes, index
        l(l+1)+m) per colour channel.  None detaches, and so does a table of zeros; a NaN or infinite value is refused and
        the sky in force stays."""
        if sh is None:
            self._ck(_lib.vct_set_sky(self._h, None), "vct_set_sky")
            return
        a = np.ascontiguousarray(sh, np.float32)
        if a.shape != (9, 3):
            raise VctError(f"set_sky: shape {a.shape}, a sky is float32 [9, 3]")
        self._ck(_lib.vct_set_sky(self._h, _ptr(a)), "vct_set_sky")

    def sky(self):
        """(sh float32 [9, 3], poly float32 [9, 3], attached bool): the coefficients as given, their folded polynomial form
        (what the kernels read), and whether a sky is attached (zeros and False when none is)."""
        sh, poly, on = np.zeros((9, 3), np.float32), np.zeros((9, 3), np.float32), C.c_int32()
        self._ck(_lib.vct_get_sky(self._h, _ptr(sh), _ptr(poly), C.byref(on)), "vct_get_sky")
        return sh, poly, bool(on.value)

    # --- G-buffer import (include/vct.h "G-buffer import")
    @staticmethod
    def _import_format(what, a, npix, given):
        """The format of one input: as given, or inferred from a numpy array's dtype and element count."""
        if given is not None:
            return int(given)
        if a is None:
            return 0
        if isinstance(a, int):
            raise VctError(f"import_gbuffer: {what} is a device pointer: name its format")
        per = a.size / npix
        table = {"position": {("float32", 3): IMPORT_POSITION_F32X3, ("float32", 4): IMPORT_POSITION_F32X4,
                              ("float32", 1): IMPORT_DEPTH_F32},
                 "normal": {("float32", 3): IMPORT_NORMAL_F32X3, ("float16", 4): IMPORT_NORMAL_F16X4,
                            ("int16", 2): IMPORT_NORMAL_OCT_SNORM16X2},
                 "colour": {("uint8", 4): IMPORT_COLOR_UNORM8X4, ("float16", 4): IMPORT_COLOR_F16X4,
                            ("float32", 4): IMPORT_COLOR_F32X4}}[what if what in ("position", "normal") else "colour"]
        fmt = table.get((a.dtype.name, per))
        if fmt is None:
            raise VctError(f"import_gbuffer: {what} is {a.dtype.name} x {per:g} per pixel, which is none of its formats")
        return fmt

    def import_gbuffer(self, position, normal, albedo, shading_normal=None, specular=None, shadow=None, material=None,
                       position_format=None, normal_format=None, albedo_format=None, specular_format=None, flags=0,
                       inv_view_proj=None, depth_clear=1.0, normal_scale=1.0, specular_constant=(0.0, 0.0, 0.0), rows=None):
        """A renderer's buffers into the selected slot's resident G-buffer; trace_current() / trace_resident() follow.
        Every input is a numpy array (host memory) or an int device pointer, all of one kind: position float32 [h*w, 3],
        [h*w, 4] or depth [h*w]; normal (and shading_normal) float32 x 3, float16 x 4 or octahedral int16 x 2; albedo and
        specular uint8, float16 or float32 x 4; shadow float32 [h*w]; material uint16 [h*w].  Formats are inferred from
        numpy inputs and must be named (IMPORT_*) for device pointers.  flags: IMPORT_FLIP_Y | IMPORT_DEPTH_ZERO_TO_ONE |
        IMPORT_OPAQUE.  inv_view_proj: column-major float32[16], depth inputs only.  rows = (tile_row0, tile_row1): only
        those tile rows are written.  Device inputs are queued on the slot's stream; host inputs return when written."""
        npix = self.cfg.width * self.cfg.height
        named = dict(position=position, normal=normal, shading_normal=shading_normal, albedo=albedo, specular=specular,
                     shadow=shadow, material=material)
        given = {k: v for k, v in named.items() if v is not None}
        kinds = {isinstance(v, int) for v in given.values()}
        if len(kinds) > 1:
            raise VctError("import_gbuffer: every input lives where `location` says: all numpy arrays or all device pointers")
        device = kinds == {True}
        if not device:
            fixed = dict(shadow=np.float32, material=np.uint16)
            for k, v in given.items():
                v = np.ascontiguousarray(v, fixed.get(k))
                if k in fixed and v.size != npix:
                    raise VctError(f"import_gbuffer: {k} has {v.size} elements, the frame has {npix} pixels")
                given[k] = v
        d = GBufferImport()
        d.position_format = self._import_format("position", given.get("position"), npix, position_format)
        d.normal_format = self._import_format("normal", given.get("normal"), npix, normal_format)
        if not device and "shading_normal" in given and \
                self._import_format("normal", given["shading_normal"], npix, normal_format) != d.normal_format:
            raise VctError("import_gbuffer: shading_normal has normal's format")
        d.albedo_format = self._import_format("albedo", given.get("albedo"), npix, albedo_format)
        d.specular_format = self._import_format("specular", given.get("specular"), npix, specular_format)
        for k in named:
            v = given.get(k)
            setattr(d, k, None if v is None else (v if device else v.ctypes.data))
        d.location = MEM_DEVICE if device else MEM_HOST
        d.flags = int(flags)
        if inv_view_proj is not None:
            d.inv_view_proj[:] = [float(x) for x in np.asarray(inv_view_proj, np.float32).reshape(16)]
        d.depth_clear, d.normal_scale = float(depth_clear), float(normal_scale)
        d.specular_constant[:] = [float(x) for x in specular_constant]
        if rows is None:
            self._ck(_lib.vct_import_gbuffer(self._h, C.byref(d)), "vct_import_gbuffer")
        else:
            self._ck(_lib.vct_import_gbuffer_rows(self._h, C.byref(d), int(rows[0]), int(rows[1])), "vct_import_gbuffer_rows")

    def last_gbuffer_import_ms(self):
        """Device ms of the kernel of the selected slot's last G-buffer import (trace timing must have been on)."""
        v = C.c_float()
        self._ck(_lib.vct_last_gbuffer_import_ms(self._h, C.byref(v)), "vct_last_gbuffer_import_ms")
        return v.value

    # --- local lights (include/vct.h "local lights")
    @staticmethod
    def _light(d):
        """One vct_light from a Light or a dict of its fields (point_light / spot_light build such dicts)."""
        if isinstance(d, Light):
            return d
        l = Light()
        for k in ("position", "color", "direction"):
            v = [float(x) for x in d.get(k, (0.0, 0.0, 0.0))]
            if len(v) != 3:
                raise VctError(f"set_lights: {k} has three components")
            getattr(l, k)[:] = v
        l.radius, l.source_radius = float(d["radius"]), float(d["source_radius"])
        l.cos_outer, l.cos_inner = float(d.get("cos_outer", 0.0)), float(d.get("cos_inner", 0.0))
        l.flags = int(d.get("flags", 0))
        return l

    def set_lights(self, lights):
        """The context's point and spot lights: a sequence of at most LIGHTS_MAX Light structures or dicts of their fields
        (point_light(), spot_light()).  None or an empty sequence detaches.  The voxel chain takes them with the next
        voxelize + inject_light (+ build_mips), the frame with the next composite launch.  Needs voxel_attributes = 1."""
        if lights is None or len(lights) == 0:
            self._ck(_lib.vct_set_lights(self._h, None, 0), "vct_set_lights")
            return
        if len(lights) > LIGHTS_MAX:
            raise VctError(f"set_lights: {len(lights)} lights, a context takes at most {LIGHTS_MAX}")
        arr = (Light * len(lights))(*[self._light(d) for d in lights])
        self._ck(_lib.vct_set_lights(self._h, C.cast(arr, C.c_void_p), len(lights)), "vct_set_lights")

    def lights(self):
        """The attached lights as a list of Light structures (empty: none attached)."""
        out, n = (Light * LIGHTS_MAX)(), C.c_int32()
        self._ck(_lib.vct_get_lights(self._h, C.cast(out, C.c_void_p), C.byref(n)), "vct_get_lights")
        return [out[i] for i in range(n.value)]

    def download_pixel_lights(self):
        """The selected slot's lit planes (pixel emission + the local lights' direct terms) as its last composite launch
        left them, float32 [3, h*w] (linear)."""
        out = np.zeros((3, self.cfg.width * self.cfg.height), np.float32)
        self._ck(_lib.vct_download_pixel_lights(self._h, _ptr(out)), "vct_download_pixel_lights")
        return out

    def last_lights_ms(self):
        """(voxel kernel of the last inject_light, pixel kernel of the selected slot's last composite launch), device ms;
        trace timing must have been on for both."""
        v = (C.c_float * 2)()
        self._ck(_lib.vct_last_lights_ms(self._h, v), "vct_last_lights_ms")
        return v[0], v[1]

    # --- dynamic mesh (include/vct.h "dynamic mesh")
    def set_dynamic_mesh(self, pos, material=None, albedo=None, max_bricks=0):
        """Attaches the dynamic mesh: positions [ntri, 9] (model space), a material index per triangle and a flat albedo
        table [nmat, 4]; pos None detaches.  max_bricks 0: twice the bricks these positions touch, at least 64.  Every
        following voxelize + inject_light (or gi_pass) voxelizes it and merges it into level 0: it wins per voxel."""
        if pos is None:
            self._ck(_lib.vct_set_dynamic_mesh(self._h, None, None, 0, None, 0, 0), "vct_set_dynamic_mesh")
            self._dyn_ntri = self._dyn_nmat = self._dyn_nparts = self._dyn_nbones = 0
            return
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
        material = np.ascontiguousarray(material, np.int32).reshape(-1)
        albedo = np.ascontiguousarray(albedo, np.float32).reshape(-1, 4)
        if material.shape[0] != pos.shape[0]:
            raise VctError(f"set_dynamic_mesh: {material.shape[0]} material indices for {pos.shape[0]} triangles")
        self._ck(_lib.vct_set_dynamic_mesh(self._h, _ptr(pos), _ptr(material), pos.shape[0], _ptr(albedo), albedo.shape[0],
                                           int(max_bricks)), "vct_set_dynamic_mesh")
        self._dyn_ntri = pos.shape[0]
        self._dyn_nmat = albedo.shape[0]
        self._dyn_nparts = 0         # the parts went with the previous mesh
        self._dyn_nbones = 0         # ... and so did the skin

    def update_dynamic_positions(self, pos):
        """New positions of the attached dynamic mesh's triangles: a float32 array [ntri, 9] or an int device pointer to
        as many floats.  Asynchronous on the selected slot's stream; the next voxelize uses them."""
        if isinstance(pos, int):
            self._ck(_lib.vct_update_dynamic_positions(self._h, _ptr(pos), MEM_DEVICE), "vct_update_dynamic_positions")
            return
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
        ntri = getattr(self, "_dyn_ntri", 0)
        if ntri and pos.shape[0] != ntri:
            raise VctError(f"update_dynamic_positions: {pos.shape[0]} triangles, the attached mesh has {ntri}")
        self._dyn_pos = pos          # stays alive until the stream has passed the copy
        self._ck(_lib.vct_update_dynamic_positions(self._h, _ptr(pos), MEM_HOST), "vct_update_dynamic_positions")

    def dynamic_info(self):
        """ntri, nmat, max_bricks and, of the last resolved pass: bricks needed / used, fragments, triangles skipped by the
        vertex contract, and whether the layer was left out for capacity.  Waits for the stream."""
        v = (C.c_int32 * 8)()
        self._ck(_lib.vct_get_dynamic(self._h, v), "vct_get_dynamic")
        keys = ("ntri", "nmat", "max_bricks", "bricks_needed", "bricks_used", "fragments", "skipped", "left_out")
        return dict(zip(keys, (int(x) for x in v)))

    def download_dynamic_voxels(self):
        """(radiance, albedo, normal) uint8 [V, V, V, 4]: the dynamic layer of the last resolved pass alone, zero elsewhere
        (albedo and normal None without voxel_attributes)."""
        V = self.cfg.voxel_dim
        rad = np.zeros((V, V, V, 4), np.uint8)
        alb = nrm = None
        if self.cfg.voxel_attributes:
            alb, nrm = np.zeros((V, V, V, 4), np.uint8), np.zeros((V, V, V, 4), np.uint8)
        self._ck(_lib.vct_download_dynamic_voxels(self._h, _ptr(rad), _ptr(alb), _ptr(nrm)), "vct_download_dynamic_voxels")
        return rad, alb, nrm

    def last_dynamic_ms(self):
        """(dynamic kernels of the last voxelize, merge of the last inject_light), device ms; trace timing must have been on."""
        v = (C.c_float * 2)()
        self._ck(_lib.vct_last_dynamic_ms(self._h, v), "vct_last_dynamic_ms")
        return v[0], v[1]

    def set_dynamic_draw(self, flags, specular=None):
        """Draws the dynamic mesh in the raster stages: DYNAMIC_DRAW_SHADOW (render_shadow_map) | DYNAMIC_DRAW_GBUFFER
        (render_gbuffer), with the specular colour `specular` (None: 0, 0, 0) for every dynamic triangle.  Context state:
        it outlives the mesh and does nothing while none is attached."""
        sp = None if specular is None else np.ascontiguousarray(specular, np.float32).reshape(3)
        self._ck(_lib.vct_set_dynamic_draw(self._h, int(flags), _ptr(sp)), "vct_set_dynamic_draw")

    def dynamic_draw(self):
        """(flags, specular [3]) as set by set_dynamic_draw."""
        flags, sp = C.c_int32(0), (C.c_float * 3)()
        self._ck(_lib.vct_get_dynamic_draw(self._h, C.byref(flags), sp), "vct_get_dynamic_draw")
        return int(flags.value), np.array(list(sp), np.float32)

    def set_dynamic_bounce(self, on):
        """bounce() with a dynamic mesh attached: off (the default) it is refused, on it runs over the merged chain and
        shades the voxels the dynamic layer occupies with the layer's albedo and normal.  Context state: it outlives the
        mesh and does nothing while none is attached."""
        self._ck(_lib.vct_set_dynamic_bounce(self._h, int(on)), "vct_set_dynamic_bounce")

    @property
    def dynamic_bounce(self):
        """The switch as set by set_dynamic_bounce."""
        on = C.c_int32(0)
        self._ck(_lib.vct_get_dynamic_bounce(self._h, C.byref(on)), "vct_get_dynamic_bounce")
        return bool(on.value)

    def set_dynamic_emission(self, emission):
        """Material emission [nmat, 3] (fp32 RGB, finite, >= 0) of the ATTACHED dynamic mesh; None or an all-zero table
        detaches.  The mesh drops it on attach, replace and detach.  Shows in the chain from the next voxelize +
        inject_light on, and -- with DYNAMIC_DRAW_GBUFFER -- in the pixel-emission planes of the next G-buffer pass."""
        if emission is None:
            self._ck(_lib.vct_set_dynamic_emission(self._h, None), "vct_set_dynamic_emission")
            return
        emission = np.ascontiguousarray(emission, np.float32)
        nmat = getattr(self, "_dyn_nmat", 0)
        if emission.ndim != 2 or emission.shape[1] != 3 or (nmat and emission.shape[0] != nmat):
            raise VctError(f"set_dynamic_emission: a table of shape {tuple(emission.shape)}, the attached dynamic mesh has "
                           f"{nmat} materials: [{nmat}, 3] is expected")
        self._ck(_lib.vct_set_dynamic_emission(self._h, _ptr(emission)), "vct_set_dynamic_emission")

    def dynamic_emission(self):
        """The dynamic mesh's emission table as set, float32 [nmat, 3], or None while none is attached."""
        n = C.c_int32(0)
        self._ck(_lib.vct_get_dynamic_emission(self._h, None, C.byref(n)), "vct_get_dynamic_emission")
        if not n.value:
            return None
        out = np.zeros((n.value, 3), np.float32)
        self._ck(_lib.vct_get_dynamic_emission(self._h, _ptr(out), C.byref(n)), "vct_get_dynamic_emission")
        return out

    def set_dynamic_parts(self, part, nparts=None):
        """Splits the ATTACHED dynamic mesh into rigid parts: `part` is an int32 index per triangle in 0 .. nparts-1
        (nparts None: the largest index + 1); the layer's current positions become the rest positions that
        update_dynamic_transforms moves.  None detaches.  The mesh drops its parts on attach, replace and detach."""
        if part is None:
            self._ck(_lib.vct_set_dynamic_parts(self._h, None, 0), "vct_set_dynamic_parts")
            self._dyn_nparts = 0
            return
        part = np.ascontiguousarray(part, np.int32)
        ntri = getattr(self, "_dyn_ntri", 0)
        if part.ndim != 1 or (ntri and part.shape[0] != ntri):
            raise VctError(f"set_dynamic_parts: part indices of shape {tuple(part.shape)}, the attached dynamic mesh has "
                           f"{ntri} triangles: [{ntri}] is expected")
        if nparts is None:
            nparts = int(part.max()) + 1 if part.size else 0
        self._ck(_lib.vct_set_dynamic_parts(self._h, _ptr(part), int(nparts)), "vct_set_dynamic_parts")
        self._dyn_nparts = int(nparts)

    def dynamic_parts(self):
        """(nparts, part int32 [ntri]) as set by set_dynamic_parts, or None while no parts are attached."""
        n = C.c_int32(0)
        self._ck(_lib.vct_get_dynamic_parts(self._h, C.byref(n), None), "vct_get_dynamic_parts")
        if not n.value:
            return None
        part = np.zeros(self.dynamic_info()["ntri"], np.int32)
        self._ck(_lib.vct_get_dynamic_parts(self._h, C.byref(n), _ptr(part)), "vct_get_dynamic_parts")
        return int(n.value), part

    def set_dynamic_skin(self, bones, weights, nbones=None):
        """Skins the ATTACHED dynamic mesh: `bones` int32 and `weights` float32, both [ntri, 3, 4] (or [ntri, 12]) -- four
        bone indices in 0 .. nbones-1 and four weights per triangle corner (nbones None: the largest index + 1).  The
        layer's current positions become the rest positions; update_dynamic_transforms then takes one 3 x 4 matrix per
        bone.  Weights are used as given (not normalised), all four terms always: point unused slots at a bone in use.
        bones None detaches.  The mesh drops its skin on attach, replace and detach; parts and a skin exclude each other."""
        if bones is None:
            self._ck(_lib.vct_set_dynamic_skin(self._h, None, None, 0), "vct_set_dynamic_skin")
            self._dyn_nbones = 0
            return
        bones = np.ascontiguousarray(bones, np.int32)
        weights = np.ascontiguousarray(weights, np.float32)
        ntri = getattr(self, "_dyn_ntri", 0)
        for name, a in (("bone indices", bones), ("weights", weights)):
            if not ((a.ndim == 3 and a.shape[1:] == (3, 4)) or (a.ndim == 2 and a.shape[1] == 12)) or (ntri and a.shape[0] != ntri):
                raise VctError(f"set_dynamic_skin: {name} of shape {tuple(a.shape)}, the attached dynamic mesh has "
                               f"{ntri} triangles: [{ntri}, 3, 4] is expected")
        if bones.shape[0] != weights.shape[0]:
            raise VctError(f"set_dynamic_skin: bone indices for {bones.shape[0]} triangles, weights for {weights.shape[0]}")
        if nbones is None:
            nbones = int(bones.max()) + 1 if bones.size else 0
        self._ck(_lib.vct_set_dynamic_skin(self._h, _ptr(bones), _ptr(weights), int(nbones)), "vct_set_dynamic_skin")
        self._dyn_nbones = int(nbones)

    def dynamic_skin(self):
        """(nbones, bones int32 [ntri, 3, 4], weights float32 [ntri, 3, 4]) as set by set_dynamic_skin, or None while no
        skin is attached."""
        n = C.c_int32(0)
        self._ck(_lib.vct_get_dynamic_skin(self._h, C.byref(n), None, None), "vct_get_dynamic_skin")
        if not n.value:
            return None
        ntri = self.dynamic_info()["ntri"]
        bones, weights = np.zeros((ntri, 3, 4), np.int32), np.zeros((ntri, 3, 4), np.float32)
        self._ck(_lib.vct_get_dynamic_skin(self._h, C.byref(n), _ptr(bones), _ptr(weights)), "vct_get_dynamic_skin")
        return int(n.value), bones, weights

    def update_dynamic_transforms(self, m):
        """One 3 x 4 model matrix per part of the attached dynamic mesh, rows first: a float32 array [nparts, 12] or
        [nparts, 3, 4], or an int device pointer to as many floats.  The layer's positions become rest x matrix, on the
        device; asynchronous on the selected slot's stream; the next voxelize uses them.  With a skin attached
        (set_dynamic_skin) the same call takes one matrix per bone, [nbones, 12] or [nbones, 3, 4]."""
        if isinstance(m, int):
            self._ck(_lib.vct_update_dynamic_transforms(self._h, _ptr(m), MEM_DEVICE), "vct_update_dynamic_transforms")
            return
        m = np.ascontiguousarray(m, np.float32)
        # a skin's bone count is always known here; a parts count of 0 is unknown to the binding: the library decides
        n, owner, noun = getattr(self, "_dyn_nbones", 0), "skin", "bones"
        if not n:
            n, owner, noun = getattr(self, "_dyn_nparts", 0), "mesh", "parts"
        if not ((m.ndim == 2 and m.shape[1] == 12) or (m.ndim == 3 and m.shape[1:] == (3, 4))) or (n and m.shape[0] != n):
            raise VctError(f"update_dynamic_transforms: matrices of shape {tuple(m.shape)}, the attached {owner} has {n} "
                           f"{noun}: [{n}, 12] or [{n}, 3, 4] is expected")
        self._dyn_m = m              # stays alive until the stream has passed the copy
        self._ck(_lib.vct_update_dynamic_transforms(self._h, _ptr(m), MEM_HOST), "vct_update_dynamic_transforms")

    def download_dynamic_positions(self):
        """The dynamic layer's current positions, float32 [ntri, 9]: those of the last update_dynamic_positions or
        update_dynamic_transforms.  Waits for the stream."""
        ntri = self.dynamic_info()["ntri"]
        if not ntri:
            raise VctError("download_dynamic_positions: no dynamic mesh attached")
        pos = np.zeros((ntri, 9), np.float32)
        self._ck(_lib.vct_download_dynamic_positions(self._h, _ptr(pos)), "vct_download_dynamic_positions")
        return pos

    def set_dynamic_normals(self, nrm):
        """Corner normals of the ATTACHED dynamic mesh, float32 [ntri, 3, 3] (or [ntri, 9]): the drawn mesh then shades
        smooth -- a frame per corner in place of the face frame.  In the space of the rest positions while parts or a skin
        are attached (moved by the cofactor matrix on the device), used as given while none is.  Any value is accepted: a
        corner whose normal is not usable (NaN, zero, 90 degrees or more from its face) takes the face frame.  None
        detaches.  The mesh drops its normals on attach, replace and detach; a mover attached or detached leaves them."""
        if nrm is None:
            self._ck(_lib.vct_set_dynamic_normals(self._h, None), "vct_set_dynamic_normals")
            return
        nrm = _dynamic_normals_array(self, "set_dynamic_normals", nrm)
        self._ck(_lib.vct_set_dynamic_normals(self._h, _ptr(nrm)), "vct_set_dynamic_normals")

    def update_dynamic_normals(self, nrm):
        """New corner normals of a deforming mesh: a float32 array [ntri, 3, 3] (or [ntri, 9]) or an int device pointer to
        as many floats.  Asynchronous on the selected slot's stream, ordered like update_dynamic_positions."""
        if isinstance(nrm, int):
            self._ck(_lib.vct_update_dynamic_normals(self._h, _ptr(nrm), MEM_DEVICE), "vct_update_dynamic_normals")
            return
        nrm = _dynamic_normals_array(self, "update_dynamic_normals", nrm)
        self._dyn_nrm = nrm          # stays alive until the stream has passed the copy
        self._ck(_lib.vct_update_dynamic_normals(self._h, _ptr(nrm), MEM_HOST), "vct_update_dynamic_normals")

    def dynamic_normals(self):
        """The corner normals as last given, float32 [ntri, 3, 3], or None while none are attached."""
        on = C.c_int32(0)
        self._ck(_lib.vct_get_dynamic_normals(self._h, C.byref(on), None), "vct_get_dynamic_normals")
        if not on.value:
            return None
        nrm = np.zeros((self.dynamic_info()["ntri"], 3, 3), np.float32)
        self._ck(_lib.vct_get_dynamic_normals(self._h, C.byref(on), _ptr(nrm)), "vct_get_dynamic_normals")
        return nrm

    def download_dynamic_frames(self):
        """(normal, tangent, bitangent) float32 [ntri, 9] each: the drawn mesh's frames as the shade kernel will read them
        -- the face frames, or the corner frames of set_dynamic_normals.  Needs a draw flag on.  Waits for the stream."""
        ntri = getattr(self, "_dyn_ntri", 0)
        if not ntri:
            raise VctError("download_dynamic_frames: no dynamic mesh attached")
        out = [np.zeros((ntri, 9), np.float32) for _ in range(3)]
        self._ck(_lib.vct_download_dynamic_frames(self._h, _ptr(out[0]), _ptr(out[1]), _ptr(out[2])), "vct_download_dynamic_frames")
        return tuple(out)

    def last_dynamic_transform_ms(self):
        """Device ms of the last update_dynamic_transforms' kernel; trace timing must have been on."""
        v = C.c_float(0.0)
        self._ck(_lib.vct_last_dynamic_transform_ms(self._h, C.byref(v)), "vct_last_dynamic_transform_ms")
        return float(v.value)

    def upload_shadow_map(self, depth, light_vp_rowmajor):
        if depth is None:
            self._ck(_lib.vct_upload_shadow_map(self._h, None, 0, None), "vct_upload_shadow_map")
            return
        depth = np.ascontiguousarray(depth, np.float32)
        m = np.ascontiguousarray(np.asarray(light_vp_rowmajor, np.float32).T)   # -> column-major
        self._ck(_lib.vct_upload_shadow_map(self._h, _ptr(depth), depth.shape[0], _ptr(m)),
                 "vct_upload_shadow_map")

    def voxelize(self, mode=VOX_CONSERVATIVE_AVG):
        self._ck(_lib.vct_voxelize(self._h, mode), "vct_voxelize")

    def inject_light(self):
        self._ck(_lib.vct_inject_light(self._h), "vct_inject_light")

    def build_mips(self):
        self._ck(_lib.vct_build_mips(self._h), "vct_build_mips")

    # --- raster input stages on the GPU
    def upload_mesh_attributes(self, normal, tangent, bitangent, specular):
        arrs = [np.ascontiguousarray(a, np.float32) for a in (normal, tangent, bitangent, specular)]
        self._ck(_lib.vct_upload_mesh_attributes(self._h, *(_ptr(a) for a in arrs)),
                 "vct_upload_mesh_attributes")

    def upload_mesh_uvs(self, uv):
        uv = np.ascontiguousarray(uv, np.float32)
        self._ck(_lib.vct_upload_mesh_uvs(self._h, _ptr(uv)), "vct_upload_mesh_uvs")

    def upload_textures(self, textures, mat_tex):
        """textures: list of uint8 [h, w, 4] (row 0 at v = 0); mat_tex: int32 [nmat, 3] diffuse / specular /
        height texture index or -1.  An empty list detaches the textures."""
        texs = [np.ascontiguousarray(t, np.uint8) for t in textures]
        n = len(texs)
        ptrs = (C.c_void_p * max(n, 1))(*[t.ctypes.data for t in texs])
        w = np.array([t.shape[1] for t in texs], np.int32)
        h = np.array([t.shape[0] for t in texs], np.int32)
        mt = np.ascontiguousarray(mat_tex, np.int32)
        self._ck(_lib.vct_upload_textures(self._h, ptrs, _ptr(w), _ptr(h), n, _ptr(mt)), "vct_upload_textures")

    def upload_scene(self, scene):
        """Everything of a voxel_cone_tracing_amd.scene.Scene: triangles, frames, texture coordinates, maps."""
        self.upload_triangles(scene.pos, scene.material, scene.albedo)
        self.upload_mesh_attributes(*scene.frames(), scene.specular)
        if scene.textures:
            self.upload_mesh_uvs(scene.uv)
            self.upload_textures(scene.textures, scene.mat_tex)
        if getattr(scene, "emission", None) is not None and np.any(scene.emission):
            self.upload_emission(scene.emission)       # Ke of the MTL file (an all-zero table would only detach)

    def render_shadow_map(self, light_vp_colmajor):
        m = np.ascontiguousarray(light_vp_colmajor, np.float32).reshape(16)
        self._ck(_lib.vct_render_shadow_map(self._h, _ptr(m)), "vct_render_shadow_map")

    def download_shadow_map(self):
        S = self.cfg.shadow_map_size
        out = np.zeros((S, S), np.float32)
        self._ck(_lib.vct_download_shadow_map(self._h, _ptr(out)), "vct_download_shadow_map")
        return out

    def render_gbuffer(self, view_proj_colmajor):
        m = np.ascontiguousarray(view_proj_colmajor, np.float32).reshape(16)
        self._ck(_lib.vct_render_gbuffer(self._h, _ptr(m)), "vct_render_gbuffer")

    def gi_pass(self, light_vp_colmajor, view_proj_colmajor, mode=VOX_CONSERVATIVE_AVG):
        """Shadow map -> {voxelize, inject, mips} beside {G-buffer raster} -> trace, one call (include/vct.h)."""
        lv = np.ascontiguousarray(light_vp_colmajor, np.float32).reshape(16)
        m = np.ascontiguousarray(view_proj_colmajor, np.float32).reshape(16)
        self._ck(_lib.vct_gi_pass(self._h, _ptr(lv), _ptr(m), mode), "vct_gi_pass")

    def render_gbuffer_rows(self, view_proj_colmajor, row0, row1):
        m = np.ascontiguousarray(view_proj_colmajor, np.float32).reshape(16)
        self._ck(_lib.vct_render_gbuffer_rows(self._h, _ptr(m), row0, row1), "vct_render_gbuffer_rows")

    # --- multi-GPU slabs + one RCCL gather per frame
    def comm_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._ck(_lib.vct_comm_init(self._h, buf, rank, world), "vct_comm_init")

    def comm_destroy(self):
        self._ck(_lib.vct_comm_destroy(self._h), "vct_comm_destroy")

    def comm_slab(self):
        r0, r1 = C.c_int32(), C.c_int32()
        self._ck(_lib.vct_comm_slab(self._h, C.byref(r0), C.byref(r1)), "vct_comm_slab")
        return r0.value, r1.value

    def comm_info(self):
        """What RCCL says about the communicator: dict(nranks, rank, device, rccl_version)."""
        v = (C.c_int32 * 4)()
        self._ck(_lib.vct_comm_info(self._h, v), "vct_comm_info")
        return dict(nranks=v[0], rank=v[1], device=v[2], rccl_version=v[3])

    def comm_last_gather_ms(self):
        v = C.c_float()
        self._ck(_lib.vct_comm_last_gather_ms(self._h, C.byref(v)), "vct_comm_last_gather_ms")
        return v.value

    def comm_set_timeout_ms(self, ms):
        self._ck(_lib.vct_comm_set_timeout_ms(self._h, int(ms)), "vct_comm_set_timeout_ms")

    def comm_set_slab_rows(self, starts):
        """Collective: load-aware slab boundaries [world + 1] in tile rows (None: the equal partition)."""
        a = None if starts is None else np.ascontiguousarray(starts, np.int32)
        self._ck(_lib.vct_comm_set_slab_rows(self._h, _ptr(a)), "vct_comm_set_slab_rows")

    def comm_set_interleaved(self, on=True):
        """Collective: tile row r belongs to rank r % world (every rank needs the whole G-buffer resident)."""
        self._ck(_lib.vct_comm_set_interleaved(self._h, 1 if on else 0), "vct_comm_set_interleaved")

    def selftest_interleaved(self, world):
        """Pixels that differ between the de-interleaved frame of `world` emulated ranks and the frame of one launch."""
        bad = C.c_uint64(0)
        self._ck(_lib.vct_selftest_interleaved(self._h, int(world), C.byref(bad)), "vct_selftest_interleaved")
        return bad.value

    def trace_gbuffer_strided(self, row0, row1, stride):
        """Asynchronous trace of every stride-th tile row of [row0, row1) of the resident G-buffer."""
        self._ck(_lib.vct_trace_resident_strided(self._h, row0, row1, stride), "vct_trace_resident_strided")

    def last_row_steps(self):
        """Executed cone steps per 8-pixel tile row of the last screen trace (uint64 [ceil(height / 8)])."""
        n = (self.cfg.height + 7) // 8
        out = np.zeros(n, np.uint64)
        self._ck(_lib.vct_last_row_steps(self._h, _ptr(out), n), "vct_last_row_steps")
        return out

    def frame_step(self):
        self._ck(_lib.vct_frame_step(self._h), "vct_frame_step")

    def comm_sync(self):
        self._ck(_lib.vct_comm_sync(self._h), "vct_comm_sync")

    def comm_download_frame(self):
        out = np.zeros((self.cfg.height, self.cfg.width, 4), np.uint16)
        self._ck(_lib.vct_comm_download_frame(self._h, _ptr(out)), "vct_comm_download_frame")
        return out

    def download_gbuffer(self):
        out = np.zeros((GB_PLANES, self.cfg.width * self.cfg.height), np.float32)
        self._ck(_lib.vct_download_gbuffer(self._h, _ptr(out)), "vct_download_gbuffer")
        return out

    def trace_gbuffer_rows(self, row0, row1):
        """Asynchronous trace of tile rows [row0, row1) of the resident G-buffer."""
        self._ck(_lib.vct_trace_resident_rows(self._h, row0, row1), "vct_trace_resident_rows")

    def trace_current(self):
        out = np.zeros((self.cfg.height, self.cfg.width, 4), np.uint16)
        self._ck(_lib.vct_trace_current(self._h, _ptr(out), MEM_HOST), "vct_trace_current")
        return out

    def bounce(self):
        self._ck(_lib.vct_bounce(self._h), "vct_bounce")

    def voxel_attributes(self):
        V = self.cfg.voxel_dim
        alb = np.zeros((V, V, V, 4), np.uint8)
        nrm = np.zeros((V, V, V, 4), np.uint8)
        self._ck(_lib.vct_download_voxel_attributes(self._h, _ptr(alb), _ptr(nrm)),
                 "vct_download_voxel_attributes")
        return alb, nrm

    def upload_volume(self, l0):
        l0 = np.ascontiguousarray(l0, np.uint8)
        assert l0.size == self.cfg.voxel_dim ** 3 * 4
        self._ck(_lib.vct_upload_volume_rgba8(self._h, _ptr(l0)), "vct_upload_volume_rgba8")

    def upload_chain(self, chain):
        chain = np.ascontiguousarray(chain, np.uint8)
        assert chain.size == chain_texels(self.cfg.voxel_dim) * 4
        self._ck(_lib.vct_upload_chain_rgba8(self._h, _ptr(chain)), "vct_upload_chain_rgba8")

    def download_aniso(self):
        V = self.cfg.voxel_dim
        out = np.zeros((6, chain_texels(V) - V ** 3, 4), np.uint8)
        self._ck(_lib.vct_download_aniso_rgba8(self._h, _ptr(out)), "vct_download_aniso_rgba8")
        return out

    def download_chain(self):
        out = np.zeros((chain_texels(self.cfg.voxel_dim), 4), np.uint8)
        self._ck(_lib.vct_download_chain_rgba8(self._h, _ptr(out)), "vct_download_chain_rgba8")
        return out

    # --- trace
    def _gb(self, planes, layout, location):
        gb = GBuffer()
        gb.planes = planes if isinstance(planes, int) else planes.ctypes.data
        gb.width, gb.height = self.cfg.width, self.cfg.height
        gb.layout, gb.location = layout, location
        return gb

    def trace(self, planes, rows=None, layout=GB_LINEAR, out_device_ptr=None):
        """planes: float32 [23, h*w] numpy (host) or an int device pointer (location=device).
        Returns the RGBA16F frame as uint16 [h, w, 4] (host) unless out_device_ptr is given."""
        location = MEM_DEVICE if isinstance(planes, int) else MEM_HOST
        if location == MEM_HOST:
            planes = np.ascontiguousarray(planes, np.float32)
        gb = self._gb(planes, layout, location)
        h, w = self.cfg.height, self.cfg.width
        if out_device_ptr is not None:
            out, optr, oloc = None, C.c_void_p(out_device_ptr), MEM_DEVICE
        else:
            out = np.zeros((h, w, 4), np.uint16)
            optr, oloc = _ptr(out), MEM_HOST
        if rows is None:
            self._ck(_lib.vct_trace(self._h, C.byref(gb), optr, oloc), "vct_trace")
        else:
            self._ck(_lib.vct_trace_slab(self._h, C.byref(gb), rows[0], rows[1], optr, oloc),
                     "vct_trace_slab")
        return out

    def download_frame(self):
        out = np.zeros((self.cfg.height, self.cfg.width, 4), np.uint16)
        self._ck(_lib.vct_download_frame(self._h, _ptr(out)), "vct_download_frame")
        return out

    def render_voxels(self, inv_view_proj, source=VOXVIEW_CURRENT, level=0):
        """Voxel view (include/vct.h): ray-march `level` of a chain (VOXVIEW_CURRENT / _RADIANCE) or a voxel attribute
        (VOXVIEW_ALBEDO / _NORMAL) into the selected slot's frame.  inv_view_proj: column-major float32[16], e.g.
        scene.invert_matrix(scene.camera_view_proj(cam, w, h)).  Asynchronous; download_frame() returns the view."""
        m = np.ascontiguousarray(inv_view_proj, np.float32).reshape(16)
        self._ck(_lib.vct_render_voxels(self._h, _ptr(m), int(source), int(level)), "vct_render_voxels")

    def last_voxel_view_ms(self):
        """Device ms of the walk kernel of the selected slot's last voxel view (trace timing must have been on)."""
        v = C.c_float()
        self._ck(_lib.vct_last_voxel_view_ms(self._h, C.byref(v)), "vct_last_voxel_view_ms")
        return v.value

    # --- point queries (include/vct.h): gathers and single cones at caller-given points
    def gather_points(self, points, want_cones=False, want_steps=False, sort=False, n=None, out_device_ptr=None,
                      cones_device_ptr=None, steps_device_ptr=None):
        """The six-cone diffuse gather at caller-given points.  points: float32 [n, 12] numpy = position, normal (model-scaled,
        as G-buffer planes 3-5), tangent, bitangent per point; returns the gather float32 [n, 4], or a tuple (gather[, cones
        [n, 6, 4]][, steps uint8 [n, 6]]) with want_cones / want_steps.  sort: QUERY_SORT_CELLS (same results; for lists
        that are not in spatial order).  Device form, for torch tensors: points = an int device pointer, n = the point
        count, out_device_ptr (and optionally cones_device_ptr / steps_device_ptr) = device pointers of the outputs; the
        work is queued on the slot's stream and None is returned (synchronize())."""
        flags = QUERY_SORT_CELLS if sort else 0
        if isinstance(points, int):
            if n is None or out_device_ptr is None:
                raise VctError("gather_points: a device pointer needs n and out_device_ptr")
            self._ck(_lib.vct_gather_points(self._h, _ptr(points), int(n), MEM_DEVICE, _ptr(out_device_ptr), _ptr(cones_device_ptr),
                                            _ptr(steps_device_ptr), flags), "vct_gather_points")
            return None
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 12)
        n = pts.shape[0]
        out = np.zeros((n, 4), np.float32)
        cones = np.zeros((n, 6, 4), np.float32) if want_cones else None
        steps = np.zeros((n, 6), np.uint8) if want_steps else None
        self._ck(_lib.vct_gather_points(self._h, _ptr(pts), n, MEM_HOST, _ptr(out), _ptr(cones), _ptr(steps), flags),
                 "vct_gather_points")
        res = (out,) + ((cones,) if want_cones else ()) + ((steps,) if want_steps else ())
        return res[0] if len(res) == 1 else res

    def cone_points(self, points, aperture=APERTURE_DIFFUSE, want_steps=False, sort=False, n=None, out_device_ptr=None,
                    steps_device_ptr=None):
        """One cone per point.  points: float32 [n, 9] = position, normal, direction (used as given: normalise it yourself);
        aperture: APERTURE_DIFFUSE / APERTURE_SPECULAR (set_cone_apertures) or APERTURE_GLOSS(k) (set_gloss_classes).  Returns float32 [n, 4] (and steps uint8 [n]
        with want_steps).  Device form as gather_points."""
        flags = QUERY_SORT_CELLS if sort else 0
        if isinstance(points, int):
            if n is None or out_device_ptr is None:
                raise VctError("cone_points: a device pointer needs n and out_device_ptr")
            self._ck(_lib.vct_cone_points(self._h, _ptr(points), int(n), MEM_DEVICE, int(aperture), _ptr(out_device_ptr),
                                          _ptr(steps_device_ptr), flags), "vct_cone_points")
            return None
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 9)
        n = pts.shape[0]
        out = np.zeros((n, 4), np.float32)
        steps = np.zeros(n, np.uint8) if want_steps else None
        self._ck(_lib.vct_cone_points(self._h, _ptr(pts), n, MEM_HOST, int(aperture), _ptr(out), _ptr(steps), flags),
                 "vct_cone_points")
        return (out, steps) if want_steps else out

    def last_point_query(self):
        """(points, executed steps, kind: 0 gather / 1 cone, 1 if marched in sorted order) of the slot's last query.  Waits."""
        v = (C.c_uint64 * 4)()
        self._ck(_lib.vct_last_point_query(self._h, v), "vct_last_point_query")
        return tuple(int(x) for x in v)

    def last_point_query_ms(self):
        """Device ms of the march kernel of the slot's last point query (trace timing must have been on)."""
        v = C.c_float()
        self._ck(_lib.vct_last_point_query_ms(self._h, C.byref(v)), "vct_last_point_query_ms")
        return v.value

    def set_frame_target(self, dev_ptr):
        """Kernel output goes to caller-owned HBM (full-frame addressing); None restores the default."""
        self._ck(_lib.vct_set_frame_target(self._h, C.c_void_p(dev_ptr) if dev_ptr else None),
                 "vct_set_frame_target")

    def trace_resident(self):
        self._ck(_lib.vct_trace_resident(self._h), "vct_trace_resident")

    def synchronize(self):
        self._ck(_lib.vct_synchronize(self._h), "vct_synchronize")

    def selftest_texel_buffer(self):
        """Channel values (of 4096) that the typed-buffer texel load converts differently from (float)c / 255.0f: 0 expected."""
        v = C.c_uint64()
        self._ck(_lib.vct_selftest_texel_buffer(self._h, C.byref(v)), "vct_selftest_texel_buffer")
        return v.value

    def set_frames_in_flight(self, n):
        """2: a second frame slot (stream, G-buffer, frame) so that frame k + 1 starts while frame k drains; 1: default."""
        self._ck(_lib.vct_set_frames_in_flight(self._h, n), "vct_set_frames_in_flight")

    def frames_in_flight(self):
        """(frames in flight, selected slot)"""
        n, s = C.c_int32(), C.c_int32()
        self._ck(_lib.vct_get_frames_in_flight(self._h, C.byref(n), C.byref(s), None), "vct_get_frames_in_flight")
        return n.value, s.value

    def frame_slot_streams_overlap(self):
        """True when the second slot's stream was seen to run beside the first (include/vct.h)."""
        v = C.c_int32()
        self._ck(_lib.vct_get_frames_in_flight(self._h, None, None, C.byref(v)), "vct_get_frames_in_flight")
        return bool(v.value)

    def select_frame_slot(self, slot):
        """Every later call works on this slot's G-buffer / frame / stream (call with k & 1 before frame k)."""
        self._ck(_lib.vct_select_frame_slot(self._h, slot), "vct_select_frame_slot")

    def steps(self):
        out = np.zeros((self.cfg.height * self.cfg.width, 7), np.uint8)
        self._ck(_lib.vct_download_steps(self._h, _ptr(out)), "vct_download_steps")
        return out

    def cones(self):
        out = np.zeros((self.cfg.height * self.cfg.width, 7, 4), np.float32)
        self._ck(_lib.vct_download_cones(self._h, _ptr(out)), "vct_download_cones")
        return out

    def last_step_count(self):
        v = C.c_uint64()
        self._ck(_lib.vct_last_step_count(self._h, C.byref(v)), "vct_last_step_count")
        return v.value

    def last_trace_stats(self):
        """Instrumented builds (-DVCT_STATS=1) only: dict of wave-level march counters."""
        v = (C.c_uint64 * 32)()
        self._ck(_lib.vct_last_trace_stats(self._h, v), "vct_last_trace_stats")
        keys = ("wave_steps", "lane_steps", "coop_zero", "coop_hit", "fallback", "fallback_lanes", "fallback_fits",
                "greedy_blocks", "greedy_le2", "greedy_le3", "greedy_le4", "quads_live", "quads_fit333", "quads_same",
                "quadrants_live", "quadrants_fit444")
        # block reuse: per kind of wave and level of the step (include/vct.h)
        keys += tuple(f"reuse_{c}_{wave}_{level}" for wave in ("diffuse", "specular") for level in ("first", "second")
                      for c in ("candidates", "hits", "hits_zero", "equal_anchor"))
        return dict(zip(keys, (int(x) for x in v)))

    def stage_counts(self):
        v = (C.c_uint64 * 8)()
        self._ck(_lib.vct_get_stage_counts(self._h, v), "vct_get_stage_counts")
        d = dict(zip(("triangles", "vox_candidates", "march_division", "accumulator_bricks", "touched_bricks",
                      "comm_reserved_cus", "raster_form", "vox_items"), (int(x) for x in v)))
        # word [2]: the division form in bits 0-7; a screen trace's texel-resource form above (1 per level, 2 per wave)
        d["texel_resource"] = d["march_division"] >> 8
        d["march_division"] &= 0xff
        return d

    def set_trace_timing(self, on=True):
        """Bracket march launches with the timing events last_trace_ms() reads (default on; ~7 us per launch: include/vct.h)."""
        self._ck(_lib.vct_set_trace_timing(self._h, int(bool(on))), "vct_set_trace_timing")

    def last_trace_ms(self):
        v = C.c_float()
        self._ck(_lib.vct_last_trace_ms(self._h, C.byref(v)), "vct_last_trace_ms")
        return v.value

    def selftest_const_divide(self, d):
        v = C.c_uint64()
        self._ck(_lib.vct_selftest_const_divide(self._h, float(d), C.byref(v)), "vct_selftest_const_divide")
        return v.value

    def selftest_area_divide(self, seed, count):
        v = C.c_uint64()
        self._ck(_lib.vct_selftest_area_divide(self._h, int(seed), int(count), C.byref(v)), "vct_selftest_area_divide")
        return v.value

    def stream(self):
        v = C.c_void_p()
        self._ck(_lib.vct_get_stream(self._h, C.byref(v)), "vct_get_stream")
        return v.value

    def frame_device(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(_lib.vct_get_frame_device(self._h, C.byref(p), C.byref(n)), "vct_get_frame_device")
        return p.value, n.value


def half_to_float(u16):
    return np.asarray(u16, np.uint16).view(np.float16).astype(np.float32)
