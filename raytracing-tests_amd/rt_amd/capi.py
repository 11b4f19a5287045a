"""ctypes binding of librt_hip.so (include/rt_hip.h + include/rt_hip_debug.h + include/rt_scene.h).

This is the Python side of the drop-in boundary: a thin mirror of the C ABI with numpy
arrays in and out.  It loads the in-tree HIP library and fails loudly if it is missing --
there is no CPU fallback anywhere in the product path.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RT_HIP_LIB: an alternative build of the same library (diagnostic variants, tools/ only)
LIB_PATH = os.environ.get("RT_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "librt_hip.so")

RT_OK, RT_E_ARG, RT_E_HIP, RT_E_NODEVICE, RT_E_UNSUPPORTED = 0, -1, -2, -3, -4

RT_STAGE_IOW01, RT_STAGE_IOW03, RT_STAGE_INW01, RT_STAGE_INW04 = 1, 3, 11, 14
RT_STAGE_IOW02 = 2
RT_IOW_CUBOID, RT_IOW_ELLIPSOID = 1, 2
RT_INW_ELLIPSOID, RT_INW_CUBOID = 1, 2

ABI_VERSION = 5  # RT_ABI_VERSION, include/rt_hip.h

PRESET_IOW03_REF3 = 1
PRESET_IOW03_FINAL = 2
PRESET_INW01_GRID = 3
PRESET_INW01_RANDOM = 4
PRESET_INW04_REFSET = 5
PRESET_INW04_CORNELL = 6


class RtCamera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("dir", C.c_float * 3), ("fov_y_rad", C.c_float),
                ("aperture", C.c_float), ("focus_dist", C.c_float)]


class RtParams(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("spp", C.c_int), ("max_bounces", C.c_int),
                ("tile_x0", C.c_int), ("tile_y0", C.c_int), ("tile_w", C.c_int), ("tile_h", C.c_int),
                ("show_normal", C.c_int), ("device", C.c_int)]


class RtStats(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("node_visits", C.c_uint64), ("prim_tests", C.c_uint64),
                ("shadow_queries", C.c_uint64), ("stack_drops", C.c_uint64), ("nan_drops", C.c_uint64),
                ("ms", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class RtGeomDesc(C.Structure):
    _fields_ = [("type", C.c_int), ("position", C.c_float * 3), ("last_position", C.c_float * 3),
                ("rotation_deg", C.c_float * 3), ("scale", C.c_float * 3), ("color", C.c_float * 3),
                ("refractivity", C.c_float), ("reflectivity", C.c_float), ("refractive_index", C.c_float),
                ("scat_refract", C.c_float), ("scat_reflect", C.c_float), ("emissive", C.c_int),
                ("texture_index", C.c_int)]


class RtCamDesc(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("pitch_deg", C.c_float), ("yaw_deg", C.c_float),
                ("fov_y_deg", C.c_float), ("aperture", C.c_float), ("focus_dist", C.c_float)]


class RtTexture(C.Structure):
    _fields_ = [("texels", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("channels", C.c_int)]


class RtOptions(C.Structure):
    """rt_options (include/rt_hip.h): the exact strategy switches of the render path."""
    _fields_ = [("size", C.c_uint32)] + [(n, C.c_int) for n in (
        "inw_wide_walk", "inw_order", "inw_beams", "inw_ri_grid", "inw_lds_nodes", "inw_fused_cull",
        "inw_claim_order", "inw_ring_pm", "inw_ring_sm", "inw_stackless", "inw_device_build", "inw_claim_xcd",
        "inw_qnodes", "inw_time_bins", "inw_walk_bins", "inw_beam_bins", "inw_sphere_records", "inw_compact_nodes",
        "iow_spec", "iow_linear", "iow_narrow", "iow_lds_bvh", "iow_leaf_batch", "iow_coop_max", "iow_chunks_lpt",
        "rounds_seq", "rounds_spec", "park_min",
        "spec_iters", "spec_probe", "spec_heavy", "spec_rounds", "spec_tail_rounds", "spec_tail_budget", "spec_scan",
        "spec_chain", "spec_alt", "spec_alt_cap", "spec_alt_seg", "spec_alt_every", "spec_spread", "spec_prior_from",
        "spec_sort", "spec_solo", "spec_validate")] + [("spec_max_gb", C.c_double), ("inw_sky_blocks", C.c_int),
                                                    ("inw_beam_prune", C.c_int)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class RtPathInfo(C.Structure):
    """rt_path_info (include/rt_hip_debug.h): what a scene's last render ran."""
    _fields_ = [("kernel", C.c_char * 64), ("launches", C.c_int), ("order", C.c_int), ("order_forced", C.c_int),
                ("wide_walk", C.c_int), ("beams", C.c_int), ("ri_grid", C.c_int), ("fused_cull", C.c_int),
                ("lds_nodes", C.c_int), ("claim_order", C.c_int), ("ring_entries", C.c_int), ("iow_bvh", C.c_int),
                ("ring_lds", C.c_int), ("stackless", C.c_int), ("lbvh_lds_nodes", C.c_int),
                ("qnodes", C.c_int), ("global_stack", C.c_int), ("walk_stack", C.c_int), ("ref_walks", C.c_uint64),
                ("time_bins", C.c_int), ("beam_bins", C.c_int), ("sphere_records", C.c_int),
                ("beam_prune", C.c_int)]

    ORDERS = {0: None, 1: "pixel-major", 2: "sample-major", 3: "per-pixel", 4: "sample-parallel", 5: "sequential"}

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["kernel"] = self.kernel.decode()
        d["order"] = self.ORDERS.get(self.order, self.order)
        return d


_FP = C.POINTER(C.c_float)
_IP = C.POINTER(C.c_int)
_U32P = C.POINTER(C.c_uint32)
_U64P = C.POINTER(C.c_uint64)

# name -> (restype, argtypes); every symbol include/*.h declares
SIGNATURES = {
    "rt_abi_version": (C.c_int, []),
    "rt_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_int, _IP]),
    "rt_render_iow01": (C.c_int, [C.POINTER(RtCamera), _FP, C.POINTER(RtParams), _FP, C.POINTER(RtStats)]),
    "rt_render_iow03": (C.c_int, [_FP, _FP, C.c_uint32, C.POINTER(RtCamera), C.POINTER(RtParams), _FP,
                                  C.POINTER(RtStats)]),
    "rt_render_iow00": (C.c_int, [C.POINTER(RtParams), _FP]),
    "rt_pack_iow02": (C.c_int, [C.c_void_p, C.c_uint32, _FP, _FP]),
    "rt_render_iow02": (C.c_int, [_FP, _FP, C.c_uint32, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_int, C.c_int,
                                  _FP, C.POINTER(RtStats)]),
    "rt_render_inw_mf": (C.c_int, [_FP, C.c_uint32, _FP, C.POINTER(RtCamera), _FP, C.c_int, C.POINTER(RtParams), _FP,
                                   _FP, C.POINTER(RtStats)]),
    "rt_render_inw": (C.c_int, [_FP, C.c_uint32, C.c_int, _FP, _FP, C.c_uint32, C.POINTER(RtCamera),
                                C.POINTER(RtParams), _FP, _FP, C.POINTER(RtStats)]),
    "rt_render_inw_tex": (C.c_int, [_FP, C.c_uint32, C.c_int, _FP, _FP, C.c_uint32, C.POINTER(RtTexture), C.c_int,
                                    C.POINTER(RtCamera), C.POINTER(RtParams), _FP, _FP, C.POINTER(RtStats)]),
    "rt_noise_texture": (C.c_int, [C.c_int, C.c_int, C.c_int, _FP, C.c_int, C.c_float, C.c_float, C.c_float,
                                   C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "rt_noise_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "rt_noise_texture_async": (C.c_int, [C.c_int, C.c_int, C.c_int, _FP, C.c_int, C.c_float, C.c_float, C.c_float,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rt_texture_remap": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                   C.POINTER(C.c_double)]),
    "rt_remap_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "rt_texture_remap_async": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    "rt_lbvh_build": (C.c_int, [_FP, C.c_uint32, _FP]),
    "rt_lbvh_workspace_bytes": (C.c_size_t, [C.c_uint32]),
    "rt_lbvh_build_async": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rt_lbvh_build_gpu": (C.c_int, [_FP, C.c_uint32, _FP, C.c_int, C.POINTER(C.c_double)]),
    "rt_dev_scene_iow03": (C.c_void_p, [_FP, _FP, C.c_uint32, C.c_int, C.c_int]),
    "rt_dev_scene_inw": (C.c_void_p, [_FP, C.c_uint32, C.c_int, _FP, _FP, C.c_uint32, C.c_int, C.c_int]),
    "rt_dev_scene_inw_tex": (C.c_void_p, [_FP, C.c_uint32, C.c_int, _FP, _FP, C.c_uint32, C.POINTER(RtTexture),
                                          C.c_int, C.c_int, C.c_int]),
    "rt_dev_scene_free": (None, [C.c_void_p]),
    "rt_render_tiles_async": (C.c_int, [C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_void_p,
                                        C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_image_async": (C.c_int, [C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_scene_preset": (C.c_int, [C.c_int, C.c_uint32, C.c_int, C.POINTER(RtGeomDesc), C.c_int,
                                  C.POINTER(RtCamDesc), C.POINTER(RtParams)]),
    "rt_camera_from_desc": (C.c_int, [C.POINTER(RtCamDesc), C.c_int, C.POINTER(RtCamera)]),
    "rt_pack_iow03": (C.c_int, [C.POINTER(RtGeomDesc), C.c_uint32, _FP, _FP]),
    "rt_pack_inw": (C.c_int, [C.POINTER(RtGeomDesc), C.c_uint32, C.c_int, _FP, _FP, _FP, _U32P]),
    "rt_sample_tables": (C.c_int, [C.c_int, _FP, _FP, _IP]),
    "rt_tile_spiral": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _IP, C.c_int]),
    "rt_render_spiral_async": (C.c_int, [C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_display_rgba8_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    "rt_debug_counters": (C.c_int, [C.c_void_p]),
    "rt_debug_pixel_rays": (C.c_int, [C.c_void_p]),
    "rt_debug_rounds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "rt_debug_spec_hist": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_debug_launches": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "rt_debug_chunks": (C.c_int, [C.c_void_p]),
    "rt_debug_spec_times": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rt_debug_time_kernels": (C.c_int, [C.c_int]),
    "rt_debug_check_fastmath": (C.c_int, [C.c_int, _U64P, _U32P]),
    "rt_debug_kernel_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "rt_debug_spec_pixels": (C.c_int, [C.c_void_p, _U32P, C.c_uint32]),
    "rt_debug_spec_list_hist": (C.c_int, [C.c_void_p, _U64P]),
    "rt_debug_spec_list_stale": (C.c_int, [C.c_void_p, _U64P]),
    "rt_debug_spec_dump": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_inw_host_build": (C.c_int, [_FP, C.c_uint32, _U32P, C.POINTER(C.c_double)]),
    "rt_iow_host_build": (C.c_int, [_FP, _FP, C.c_uint32, _U32P, C.POINTER(C.c_double)]),
    "rt_options_default": (None, [C.POINTER(RtOptions)]),
    "rt_options_set": (C.c_int, [C.POINTER(RtOptions)]),
    "rt_options_get": (C.c_int, [C.POINTER(RtOptions)]),
    "rt_dev_scene_set_options": (C.c_int, [C.c_void_p, C.POINTER(RtOptions)]),
    "rt_dev_scene_inw_update": (C.c_int, [C.c_void_p, _FP, C.c_uint32, _FP, _FP, _FP, C.c_uint32,
                                          C.POINTER(C.c_double)]),
    "rt_dev_scene_inw_update_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                 C.c_int, C.c_void_p, C.POINTER(C.c_double)]),
    "rt_inw_swept_boxes_async": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_dev_scene_iow03_update": (C.c_int, [C.c_void_p, _FP, _FP, C.c_uint32, C.c_int, C.POINTER(C.c_double)]),
    "rt_dev_scene_iow03_update_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p,
                                                   C.POINTER(C.c_double)]),
    "rt_debug_iow_prepare_host": (C.c_int, [_FP, _FP, C.c_uint32, _FP, _FP, _FP]),
    "rt_debug_iow_records": (C.c_int, [C.c_void_p, _FP, _FP, _FP]),
    "rt_debug_update_iow_kernel": (C.c_int, [C.c_int, _IP]),
    "rt_debug_iow_info": (C.c_int, [C.c_void_p, _U32P]),
    "rt_debug_iow_dump": (C.c_int, [C.c_void_p, _U32P, _FP, _FP]),
    "rt_debug_path": (C.c_int, [C.c_void_p, C.POINTER(RtPathInfo)]),
    "rt_debug_sky_blocks": (C.c_int, [C.c_void_p, _U32P]),
    "rt_debug_beam_lists": (C.c_int, [C.c_void_p, _U64P, _U32P, _FP, _U64P, C.c_uint32]),
    "rt_beam_keep_host": (C.c_int, [_FP, _FP, C.c_float, C.c_float, C.c_float, C.c_float, _FP, _FP, C.c_uint32,
                                    C.c_uint32, C.c_int, _IP]),
    "rt_debug_wide_info": (C.c_int, [C.c_void_p, _U32P, _U32P]),
    "rt_debug_query_fused": (C.c_int, [C.c_void_p]),
    "rt_tile_deal": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _IP, C.c_int]),
    "rt_group_create": (C.c_void_p, [_IP, C.c_int]),
    "rt_debug_build_level_cap": (C.c_int, [C.c_int]),
    "rt_debug_time_bins": (C.c_int, [_FP, _FP, C.c_uint32, C.c_uint32, _FP, C.c_uint32, _U32P]),
    "rt_debug_bin_boxes": (C.c_int, [_FP, C.c_uint32, C.c_uint32, C.c_uint32, _FP]),
    "rt_debug_sphere_records": (C.c_int, [_FP, C.c_uint32, C.c_int, _FP]),
    "rt_debug_inw_stick_out": (C.c_int, [_FP, C.c_uint32, _FP, _FP, C.POINTER(C.c_double)]),
    "rt_debug_walk_dump": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, _U64P]),
    "rt_debug_inw_host_dump": (C.c_int, [_FP, C.c_uint32, _U32P, _FP, _FP, _U32P, _U32P, _U32P, _FP, _IP]),
    "rt_debug_iow_host_dump": (C.c_int, [_FP, _FP, C.c_uint32, _U32P, _FP, _FP]),
    "rt_group_free": (None, [C.c_void_p]),
    "rt_trace_rays_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "rt_trace_inw": (C.c_int, [_FP, C.c_uint32, C.c_int, _FP, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_int,
                               C.POINTER(RtStats)]),
    "rt_debug_trace_kernel": (C.c_int, [C.c_int, C.c_int, _IP]),
    "rt_trace_iow_rays_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "rt_trace_iow03": (C.c_int, [_FP, _FP, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_int,
                                 C.POINTER(RtStats)]),
    "rt_debug_trace_iow_kernel": (C.c_int, [C.c_int, C.c_int, _IP]),
    "rt_path_rays_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "rt_path_inw": (C.c_int, [_FP, C.c_uint32, C.c_int, _FP, _FP, C.c_uint32, C.POINTER(RtTexture), C.c_int, C.c_int,
                              C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.POINTER(RtStats)]),
    "rt_debug_paths_kernel": (C.c_int, [C.c_int, C.c_int, _IP]),
    "rt_debug_paths_max_blocks": (C.c_int, [C.c_int]),
    "rt_path_iow_rays_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "rt_path_iow03": (C.c_int, [_FP, _FP, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int,
                                C.c_void_p, C.c_int, C.POINTER(RtStats)]),
    "rt_debug_path_iow_kernel": (C.c_int, [C.c_int, _IP]),
    "rt_debug_path_iow_max_blocks": (C.c_int, [C.c_int]),
    "rt_camera_rays_async": (C.c_int, [C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_void_p, C.c_uint32,
                                       C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_pixel_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_uint32]),
    "rt_pixel_query_async": (C.c_int, [C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_void_p, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rt_pixels_inw": (C.c_int, [_FP, C.c_uint32, C.c_int, _FP, _FP, C.c_uint32, C.POINTER(RtTexture), C.c_int,
                                C.POINTER(RtCamera), C.POINTER(RtParams), C.c_void_p, C.c_uint32, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int, C.POINTER(RtStats)]),
    "rt_pixels_iow03": (C.c_int, [_FP, _FP, C.c_uint32, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_void_p,
                                  C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(RtStats)]),
    "rt_debug_pixels_kernel": (C.c_int, [C.c_int, _IP]),
    "rt_render_pass_async": (C.c_int, [C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_passes_inw": (C.c_int, [_FP, C.c_uint32, C.c_int, _FP, _FP, C.c_uint32, C.POINTER(RtTexture), C.c_int,
                                       C.POINTER(RtCamera), C.POINTER(RtParams), _U32P, C.c_int, _FP, _FP,
                                       C.c_void_p, C.c_int, C.POINTER(RtStats)]),
    "rt_render_passes_iow03": (C.c_int, [_FP, _FP, C.c_uint32, C.POINTER(RtCamera), C.POINTER(RtParams), _U32P,
                                         C.c_int, _FP, C.c_void_p, C.c_int, C.POINTER(RtStats)]),
    "rt_debug_pass_kernel": (C.c_int, [C.c_int, _IP]),
    "rt_debug_update_kernel": (C.c_int, [C.c_int, _IP]),
    "rt_debug_pass_max_blocks": (C.c_int, [C.c_int]),
    "rt_render_pass_pixels_async": (C.c_int, [C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_void_p,
                                              C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "rt_pass_select_async": (C.c_int, [C.c_void_p, C.POINTER(RtParams), C.c_void_p, C.c_void_p, C.c_float, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_adaptive_inw": (C.c_int, [_FP, C.c_uint32, C.c_int, _FP, _FP, C.c_uint32, C.POINTER(RtTexture), C.c_int,
                                         C.POINTER(RtCamera), C.POINTER(RtParams), C.c_uint32, C.c_float, C.c_uint32,
                                         C.c_uint32, _FP, _FP, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int, C.POINTER(RtStats)]),
    "rt_render_adaptive_iow03": (C.c_int, [_FP, _FP, C.c_uint32, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_uint32,
                                           C.c_float, C.c_uint32, C.c_uint32, _FP, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, C.POINTER(RtStats)]),
    "rt_debug_adaptive_chunk": (C.c_int, [C.c_int]),
    "rt_render_multi_async": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_inw_multi": (C.c_int, [_FP, C.c_uint32, C.c_int, _FP, _FP, C.c_uint32, C.POINTER(RtCamera),
                                      C.POINTER(RtParams), _IP, C.c_int, C.c_int, _FP, _FP, C.POINTER(RtStats)]),
    "rt_render_pass_tiles_async": (C.c_int, [C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_void_p,
                                             C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_render_pass_multi_async": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtParams),
                                             C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "rt_render_passes_inw_multi": (C.c_int, [_FP, C.c_uint32, C.c_int, _FP, _FP, C.c_uint32, C.POINTER(RtCamera),
                                             C.POINTER(RtParams), _IP, C.c_int, C.c_int, _U32P, C.c_int, _FP, _FP,
                                             C.POINTER(RtStats)]),
    "rt_render_pass_slots_async": (C.c_int, [C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtParams), C.c_void_p,
                                             C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_pass_select_tiles_async": (C.c_int, [C.c_void_p, C.POINTER(RtParams), C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "rt_render_adaptive_multi_async": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtParams),
                                                 C.c_int, C.c_int, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_group_adaptive_active": (C.c_int, [C.c_void_p, _U32P]),
    "rt_render_adaptive_inw_multi": (C.c_int, [_FP, C.c_uint32, C.c_int, _FP, _FP, C.c_uint32, C.POINTER(RtCamera),
                                               C.POINTER(RtParams), _IP, C.c_int, C.c_int, C.c_uint32, C.c_float,
                                               C.c_uint32, C.c_uint32, _FP, _FP, C.c_void_p, C.c_void_p,
                                               C.POINTER(RtStats)]),
}

_lib = None


def load(path: str = LIB_PATH) -> C.CDLL:
    """Load librt_hip.so.  Raises (never falls back) if the HIP library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f"librt_hip.so not built at {path}: run __graft_entry__.build() "
                           "(there is no CPU fallback for the render path)")
    # torch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  Loading torch first makes
    # the dynamic linker resolve our NEEDED libamdhip64.so.7 to that same runtime, so device
    # pointers, streams and RCCL from torch and our kernels share one HIP runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def fptr(a: np.ndarray | None):
    if a is None:
        return None
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(_FP)


def check(rc: int, what: str) -> None:
    if rc != RT_OK:
        raise RuntimeError(f"{what} failed with status {rc}")


# ---------------------------------------------------------------------------- options
def default_options() -> RtOptions:
    o = RtOptions()
    load().rt_options_default(C.byref(o))
    return o


def get_options() -> RtOptions:
    o = RtOptions()
    check(load().rt_options_get(C.byref(o)), "rt_options_get")
    return o


def set_options(o: RtOptions) -> None:
    check(load().rt_options_set(C.byref(o)), "rt_options_set")


class options:
    """Context manager: the library-wide rt_options with some fields changed, e.g.
    `with R.options(inw_order=2, inw_ring_sm=64): R.render(sc)`; restores the previous ones."""

    def __init__(self, **fields):
        self.fields = fields

    def __enter__(self) -> RtOptions:
        self.prev = get_options()
        o = RtOptions.from_buffer_copy(self.prev)
        for k, v in self.fields.items():
            if k not in dict(RtOptions._fields_):
                raise KeyError(f"unknown rt_options field {k!r}")
            setattr(o, k, v)
        set_options(o)
        return o

    def __exit__(self, *exc) -> None:
        set_options(self.prev)


def debug_path(scene_handle) -> dict:
    """rt_debug_path of a device scene: the kernel and exact shortcuts of its last render."""
    p = RtPathInfo()
    check(load().rt_debug_path(scene_handle, C.byref(p)), "rt_debug_path")
    return p.as_dict()


def debug_sky_blocks(scene_handle) -> tuple:
    """rt_debug_sky_blocks of a device scene's last render: (blocks flagged, of them rendered by
    k_inw_sky, blocks of the frame)."""
    out = (C.c_uint32 * 3)()
    check(load().rt_debug_sky_blocks(scene_handle, out), "rt_debug_sky_blocks")
    return tuple(out)


# ----------------------------------------------------------------------------- scenes
@dataclass
class Scene:
    """A packed scene in the reference's record layouts (what the GL textures held)."""
    stage: int
    desc: object            # ctypes array of RtGeomDesc
    n: int
    camera: RtCamera
    params: RtParams
    types: np.ndarray | None = None    # IOW-03
    records: np.ndarray | None = None  # IOW-03 (N,24)
    geom: np.ndarray | None = None     # INW (N,28)
    aabbs: np.ndarray | None = None    # INW (N,6)
    nodes: np.ndarray | None = None    # INW (2N-1,8)
    lights: np.ndarray | None = None   # INW-04 (L,7)
    n_lights: int = 0
    textures: list | None = None       # INW-04 u_MaterialTextures: (H, W, 3|4) uint8 images

    @property
    def layout(self) -> int:
        return 4 if self.stage == RT_STAGE_INW04 else 1


PRESET_STAGE = {PRESET_IOW03_REF3: RT_STAGE_IOW03, PRESET_IOW03_FINAL: RT_STAGE_IOW03,
                 PRESET_INW01_GRID: RT_STAGE_INW01, PRESET_INW01_RANDOM: RT_STAGE_INW01,
                 PRESET_INW04_REFSET: RT_STAGE_INW04, PRESET_INW04_CORNELL: RT_STAGE_INW04}


def preset_desc(preset: int, seed: int = 0, n_hint: int = 0):
    lib = load()
    n = lib.rt_scene_preset(preset, seed, n_hint, None, 0, None, None)
    if n < 0:
        raise RuntimeError(f"unknown preset {preset}")
    arr = (RtGeomDesc * max(n, 1))()
    cam, par = RtCamDesc(), RtParams()
    check(lib.rt_scene_preset(preset, seed, n_hint, arr, n, C.byref(cam), C.byref(par)) - n, "rt_scene_preset")
    return arr, n, cam, par


def camera_from_desc(cd: RtCamDesc, stage: int) -> RtCamera:
    cam = RtCamera()
    check(load().rt_camera_from_desc(C.byref(cd), stage, C.byref(cam)), "rt_camera_from_desc")
    return cam


def pack(desc, n: int, stage: int, build_lbvh: bool = True) -> dict:
    lib = load()
    out: dict = {}
    if stage == RT_STAGE_IOW03:
        types = np.zeros(n, np.float32)
        rec = np.zeros((n, 24), np.float32)
        check(lib.rt_pack_iow03(desc, n, fptr(types), fptr(rec)), "rt_pack_iow03")
        out.update(types=types, records=rec)
    else:
        layout = 4 if stage == RT_STAGE_INW04 else 1
        geom = np.zeros((n, 28), np.float32)
        aabbs = np.zeros((n, 6), np.float32)
        lights = np.zeros((max(n, 1), 7), np.float32)
        nl = C.c_uint32(0)
        check(lib.rt_pack_inw(desc, n, layout, fptr(geom), fptr(aabbs), fptr(lights), C.byref(nl)), "rt_pack_inw")
        out.update(geom=geom, aabbs=aabbs, lights=lights[: nl.value].copy(), n_lights=nl.value)
        if build_lbvh:
            out["nodes"] = lbvh_build(aabbs)
    return out


def make_scene(preset: int, seed: int = 0, n_hint: int = 0, **param_overrides) -> Scene:
    stage = PRESET_STAGE[preset]
    arr, n, cd, par = preset_desc(preset, seed, n_hint)
    for k, v in param_overrides.items():
        setattr(par, k, v)
    cam = camera_from_desc(cd, stage)
    sc = Scene(stage=stage, desc=arr, n=n, camera=cam, params=par)
    for k, v in pack(arr, n, stage).items():
        setattr(sc, k, v)
    return sc


def texture_array(textures):
    """rt_texture[] for a list of (H, W, 3|4) uint8 images (row 0 first); returns (array, keep-alive)."""
    keep = [np.ascontiguousarray(t, np.uint8) for t in textures]
    arr = (RtTexture * max(1, len(keep)))()
    for i, t in enumerate(keep):
        assert t.ndim == 3 and t.shape[2] in (3, 4), t.shape
        arr[i] = RtTexture(t.ctypes.data, t.shape[1], t.shape[0], t.shape[2])
    return arr, keep


NOISE_SIMPLEX, NOISE_FBM, NOISE_TURBULENCE = 0, 1, 2
MAP_MERCATOR, MAP_CUBIC = 0, 1


def noise_texture(width=600, height=100, kind=NOISE_SIMPLEX, gradient=((0, 0, 0), (1, 1, 1)), freq=0.01,
                  lac=2.0, gain=0.5, octaves=5, device: int = -1):
    """GPU Helper::Noise::MakeTexture<glm::vec3> (rt_noise_texture): (height, width, 3) uint8, ms."""
    g = np.ascontiguousarray(np.asarray(gradient, np.float32).reshape(-1, 3))
    out = np.zeros((height, width, 3), np.uint8)
    ms = C.c_double(0.0)
    check(load().rt_noise_texture(width, height, kind, fptr(g) if len(g) else None, len(g), freq, lac, gain,
                                  octaves, out.ctypes.data, device, C.byref(ms)), "rt_noise_texture")
    return out, ms.value


def texture_remap(img, load_as, map_to, device: int = -1):
    """GPU re-projection of LoadFromDiskToGPU(loc, loadAs, mapTo) (rt_texture_remap): image, ms."""
    img = np.ascontiguousarray(img, np.uint8)
    out = np.zeros_like(img)
    ms = C.c_double(0.0)
    check(load().rt_texture_remap(img.ctypes.data, img.shape[1], img.shape[0], img.shape[2], load_as, map_to,
                                  out.ctypes.data, device, C.byref(ms)), "rt_texture_remap")
    return out, ms.value


def tile_spiral(width: int, height: int, tile_w: int = 100, tile_h: int = 100) -> np.ndarray:
    """Progressive tile order of Adding_Materials::OnUpdate (rt_tile_spiral): (n, 4) int32 rows
    (tx, ty, dispatch_w, dispatch_h)."""
    lib = load()
    n = lib.rt_tile_spiral(width, height, tile_w, tile_h, None, 0)
    check(min(n, 0), "rt_tile_spiral")
    out = np.zeros((max(n, 1), 4), np.int32)
    lib.rt_tile_spiral(width, height, tile_w, tile_h, out.ctypes.data_as(_IP), n)
    return out[:n]


def tile_deal(width: int, height: int, tile: int, n_dev: int) -> list:
    """rt_tile_deal: the multi-GPU deal order of the frame's tiles, [(tx, ty), ...]; entry k goes to
    device k % n_dev."""
    lib = load()
    n = lib.rt_tile_deal(width, height, tile, n_dev, None, 0)
    check(min(n, 0), "rt_tile_deal")
    out = np.zeros((max(n, 1), 2), np.int32)
    lib.rt_tile_deal(width, height, tile, n_dev, out.ctypes.data_as(_IP), n)
    return [tuple(int(v) for v in row) for row in out[:n]]


def render_inw_multi(sc: "Scene", devices, params: RtParams | None = None, tile: int = 16):
    """rt_render_inw_multi: the INW frame tile-partitioned over `devices` with the RCCL gather to
    devices[0]; returns (rgba, depth, stats) like render()."""
    p = params or sc.params
    devs = (C.c_int * len(devices))(*devices)
    rgba = np.zeros((p.height, p.width, 4), np.float32)
    depth = np.zeros((p.height, p.width), np.float32)
    st = RtStats()
    lights = sc.lights if sc.lights is not None and len(sc.lights) else None
    check(load().rt_render_inw_multi(fptr(sc.geom), sc.n, sc.layout, fptr(sc.nodes), fptr(lights), sc.n_lights,
                                     C.byref(sc.camera), C.byref(p), devs, len(devices), tile, fptr(rgba), fptr(depth),
                                     C.byref(st)), "rt_render_inw_multi")
    return rgba, depth, st.as_dict()


def lbvh_build_gpu(aabbs, device: int = -1):
    """GPU LBVH (rt_lbvh_build_gpu): same (2N-1) x 8 node buffer as lbvh_build; returns (nodes, ms)."""
    aabbs = np.ascontiguousarray(aabbs, np.float32)
    n = aabbs.shape[0]
    nodes = np.zeros((2 * n - 1, 8), np.float32)
    ms = C.c_double(0.0)
    check(load().rt_lbvh_build_gpu(fptr(aabbs), n, fptr(nodes), device, C.byref(ms)), "rt_lbvh_build_gpu")
    return nodes, ms.value


def inw_host_build(nodes: np.ndarray, n: int) -> dict:
    """rt_inw_host_build: the INW device scene's host-built structures (sizes) and host time."""
    info = (C.c_uint32 * 8)()
    ms = C.c_double(0.0)
    check(load().rt_inw_host_build(fptr(np.ascontiguousarray(nodes, np.float32)), n, info, C.byref(ms)),
          "rt_inw_host_build")
    keys = ("wide_nodes", "dfs_high", "wide_depth", "ri_grid", "ri_cells", "ri_ids")
    return {**dict(zip(keys, list(info)[:6])), "ms": ms.value}


def iow_host_build(types: np.ndarray, records: np.ndarray, n: int) -> dict:
    """rt_iow_host_build: the IOW-03 culling BVH's size (0: linear loop) and host time."""
    info = (C.c_uint32 * 4)()
    ms = C.c_double(0.0)
    check(load().rt_iow_host_build(fptr(types), fptr(records), n, info, C.byref(ms)), "rt_iow_host_build")
    return {"wide_nodes": info[0], "ms": ms.value}


def inw_host_dump(nodes: np.ndarray, n: int) -> dict | None:
    """rt_debug_inw_host_dump: everything inw_wide_build and ri_grid_build make of an LBVH node buffer
    (None: not walkable).  wnodes (N, 40) float32 with the links as int bits; the ri_* entries are None
    when the grid was dropped (ri_grid = 0)."""
    lib = load()
    nodes = np.ascontiguousarray(nodes, np.float32)
    info = (C.c_uint32 * 8)()
    check(lib.rt_debug_inw_host_dump(fptr(nodes), n, info, None, None, None, None, None, None, None),
          "rt_debug_inw_host_dump")
    nw, high, depth, ok, cells, nids, wb = list(info)[:7]
    if not nw:
        return None
    wn = np.zeros((nw, 40), np.float32)
    leaf = np.zeros((n, 8), np.float32)
    rank = np.zeros((2, n), np.uint32)
    rc = np.zeros(cells + 1, np.uint32)
    ri = np.zeros(max(1, nids), np.uint32)
    frame = np.zeros(9, np.float32)
    dim = np.zeros(3, np.int32)
    check(lib.rt_debug_inw_host_dump(fptr(nodes), n, info, fptr(wn), fptr(leaf), rank.ctypes.data_as(_U32P),
                                     rc.ctypes.data_as(_U32P), ri.ctypes.data_as(_U32P), fptr(frame),
                                     dim.ctypes.data_as(_IP)), "rt_debug_inw_host_dump")
    out = {"wnodes": wn, "n_wtree0": nw, "wbins": 1, "wbin_stride": 0, "leafbox": leaf, "rank": rank,
           "dfs_high": high, "depth": depth, "wbound": np.array([wb], np.uint32).view(np.float32)[0], "ri_grid": ok,
           "ri_cells": None, "ri_ids": None, "ri_lo": None, "ri_hi": None, "ri_inv": None, "ri_dim": None}
    if ok:
        out.update(ri_cells=rc, ri_ids=ri[:nids], ri_lo=frame[0:3], ri_hi=frame[3:6], ri_inv=frame[6:9], ri_dim=dim)
    return out


def iow_host_dump(types: np.ndarray, records: np.ndarray, n: int) -> dict | None:
    """rt_debug_iow_host_dump: the IOW-03 culling BVH (wide (N, 32) float32, links as int bits in
    columns 24..27) and the per-object boxes obox (n, 6) (lo xyz, hi xyz), unpacked from the kernels'
    layout.  None: no BVH (the linear loop)."""
    lib = load()
    types = np.ascontiguousarray(types, np.float32)
    records = np.ascontiguousarray(records, np.float32)
    info = (C.c_uint32 * 4)()
    check(lib.rt_debug_iow_host_dump(fptr(types), fptr(records), n, info, None, None), "rt_debug_iow_host_dump")
    if not info[0]:
        return None
    wide = np.zeros((info[0], 32), np.float32)
    raw = np.zeros(6 * n, np.float32)
    check(lib.rt_debug_iow_host_dump(fptr(types), fptr(records), n, info, fptr(wide), fptr(raw)),
          "rt_debug_iow_host_dump")
    obox = np.concatenate([raw[:4 * n].reshape(n, 4), raw[4 * n:].reshape(n, 2)], axis=1)
    return {"wide": wide, "obox": obox}


RT_UPDATE_HOST_BUILD, RT_UPDATE_DEVICE_BUILD = 1, 2
RT_UPDATE_BINS, RT_UPDATE_NO_BINS = 4, 8


def update_iow03(handle, types: np.ndarray, records: np.ndarray, flags: int = 0) -> list:
    """rt_dev_scene_iow03_update: the next edit of the IOW-03 device scene `handle` (new types (n) and
    records (n, 24)); flags 0, RT_UPDATE_HOST_BUILD or RT_UPDATE_DEVICE_BUILD.  Returns timing_ms: host
    ms of [records, boxes and culling BVH, upload of host-built structures, the whole call]."""
    types = np.ascontiguousarray(types, np.float32)
    records = np.ascontiguousarray(records, np.float32)
    tm = (C.c_double * 4)()
    check(load().rt_dev_scene_iow03_update(handle, fptr(types), fptr(records), len(types), int(flags), tm),
          "rt_dev_scene_iow03_update")
    return list(tm)


IOW_INFO_KEYS = ("objects", "wide_nodes", "wide_depth", "built", "lds", "updates")


def iow_info(handle) -> dict:
    """rt_debug_iow_info of an IOW-03 device scene: objects, wide_nodes (0: linear loop), wide_depth, built
    (0 host, 1 device, 2 host after the level cap, 3 host because of a non-finite box), lds (the
    LDS-staged kernel instances apply), updates (successful updates so far)."""
    info = (C.c_uint32 * 8)()
    check(load().rt_debug_iow_info(handle, info), "rt_debug_iow_info")
    return dict(zip(IOW_INFO_KEYS, (int(x) for x in info)))


def iow_dump(handle) -> dict | None:
    """rt_debug_iow_dump: the culling BVH and object boxes of an IOW-03 device scene as its kernels read
    them, in iow_host_dump's keys (wide (N, 32), obox (n, 6)).  None: no BVH (the linear loop)."""
    lib = load()
    info = (C.c_uint32 * 4)()
    check(lib.rt_debug_iow_dump(handle, info, None, None), "rt_debug_iow_dump")
    if not info[0]:
        return None
    n = iow_info(handle)["objects"]
    wide = np.zeros((info[0], 32), np.float32)
    raw = np.zeros(6 * n, np.float32)
    check(lib.rt_debug_iow_dump(handle, info, fptr(wide), fptr(raw)), "rt_debug_iow_dump")
    obox = np.concatenate([raw[:4 * n].reshape(n, 4), raw[4 * n:].reshape(n, 2)], axis=1)
    return {"wide": wide, "obox": obox}


RT_WALK_WNODES, RT_WALK_CNODES, RT_WALK_QNODES, RT_WALK_LEAFBOX, RT_WALK_LBVH = 0, 1, 2, 3, 4
RT_WALK_RI_CELLS, RT_WALK_RI_IDS, RT_WALK_RI_FRAME, RT_WALK_WBOUND = 5, 6, 7, 8
RT_WALK_HOT, RT_WALK_COLD, RT_WALK_SPH = 9, 10, 11


def walk_dump(scene, what: int, dtype=np.float32):
    """rt_debug_walk_dump: one structure of an INW device scene (a handle from rt_dev_scene_inw*) as a
    flat array of `dtype`, and the hook's info list."""
    lib = load()
    info = (C.c_uint64 * 8)()
    check(lib.rt_debug_walk_dump(scene, what, None, 0, info), "rt_debug_walk_dump")
    out = np.zeros(int(info[0]) // np.dtype(dtype).itemsize, dtype)
    if info[0]:
        check(lib.rt_debug_walk_dump(scene, what, out.ctypes.data, out.nbytes, info), "rt_debug_walk_dump")
    return out, [int(x) for x in info]


def walk_dump_all(scene) -> dict:
    """Every structure rt_debug_walk_dump and rt_debug_wide_info read back, in inw_host_dump's keys plus
    cnodes (N, 28), qnodes (N, 4 * float4 per node), lbvh (2n-1, 8), n and build (where it was built), and the
    records the kernels see: hot (n, 28), cold (n, 8), sph (n, 12) or None (not every object is a sphere)."""
    lib = load()
    wi = (C.c_uint32 * 8)()
    check(lib.rt_debug_wide_info(scene, wi, None), "rt_debug_wide_info")
    n = int(wi[6])
    rank = np.zeros((2, n), np.uint32)
    check(lib.rt_debug_wide_info(scene, wi, rank.ctypes.data_as(_U32P)), "rt_debug_wide_info")
    wn, iw = walk_dump(scene, RT_WALK_WNODES)
    cn, _ = walk_dump(scene, RT_WALK_CNODES)
    qn, iq = walk_dump(scene, RT_WALK_QNODES)
    leaf, _ = walk_dump(scene, RT_WALK_LEAFBOX)
    lbvh, _ = walk_dump(scene, RT_WALK_LBVH)
    cells, ic = walk_dump(scene, RT_WALK_RI_CELLS, np.uint32)
    ids, _ = walk_dump(scene, RT_WALK_RI_IDS, np.uint32)
    frame, _ = walk_dump(scene, RT_WALK_RI_FRAME)
    wb, _ = walk_dump(scene, RT_WALK_WBOUND)
    hot, ih = walk_dump(scene, RT_WALK_HOT)
    cold, icd = walk_dump(scene, RT_WALK_COLD)
    sph, isp = walk_dump(scene, RT_WALK_SPH)
    ok = int(ic[2])
    return {"n": n, "build": int(wi[7]), "wnodes": wn.reshape(-1, 40), "n_wtree0": iw[2], "wbins": iw[3],
            "wbin_stride": iw[4], "depth": iw[5], "cnodes": cn.reshape(-1, 28),
            "qnodes": qn.reshape(-1, 4 * max(1, iq[2])), "leafbox": leaf.reshape(-1, 8), "lbvh": lbvh.reshape(-1, 8),
            "rank": rank, "dfs_high": int(wi[1]), "wbound": wb[0] if len(wb) else None, "ri_grid": ok,
            "ri_cells": cells if ok else None, "ri_ids": ids if ok else None,
            "ri_lo": frame[0:3] if ok else None, "ri_hi": frame[3:6] if ok else None,
            "ri_inv": frame[6:9] if ok else None, "ri_dim": frame[9:12].view(np.int32) if ok else None,
            "wide_info": [int(x) for x in wi], "hot": hot.reshape(-1, max(1, ih[2])),
            "cold": cold.reshape(-1, max(1, icd[2])), "sph": sph.reshape(-1, max(1, isp[2])) if isp[0] else None}


def inw_stick_out(geom: np.ndarray, nodes: np.ndarray | None = None, aabbs: np.ndarray | None = None) -> float:
    """rt_debug_inw_stick_out: the most an object sticks out of its leaf box (of `nodes`, or of aabbs), as a
    multiple of the margin up to which a scene takes the wide walk."""
    geom = np.ascontiguousarray(geom, np.float32)
    nodes = None if nodes is None else np.ascontiguousarray(nodes, np.float32)
    aabbs = None if aabbs is None else np.ascontiguousarray(aabbs, np.float32)
    out = C.c_double(0.0)
    check(load().rt_debug_inw_stick_out(fptr(geom), len(geom), fptr(nodes), fptr(aabbs), C.byref(out)),
          "rt_debug_inw_stick_out")
    return out.value


def lbvh_build(aabbs: np.ndarray) -> np.ndarray:
    aabbs = np.ascontiguousarray(aabbs, np.float32)
    n = aabbs.shape[0]
    nodes = np.zeros((2 * n - 1, 8), np.float32)
    check(load().rt_lbvh_build(fptr(aabbs), n, fptr(nodes)), "rt_lbvh_build")
    return nodes


def sample_tables(spp: int):
    sf = np.zeros((spp, 2), np.float32)
    fib = np.zeros((spp, 3), np.float32)
    ring = np.zeros((spp, 2), np.int32)
    check(load().rt_sample_tables(spp, fptr(sf), fptr(fib), ring.ctypes.data_as(_IP)), "rt_sample_tables")
    return sf, fib, ring


# ---------------------------------------------------------------------------- render
def render(sc: Scene, params: RtParams | None = None, sphere=None):
    """Blocking GPU render of a packed scene; returns (rgba (H,W,4), depth or None, stats dict)."""
    lib = load()
    p = params or sc.params
    rgba = np.zeros((p.height, p.width, 4), np.float32)
    st = RtStats()
    depth = None
    if sc.stage == RT_STAGE_IOW01:
        sph = np.asarray(sphere, np.float32)
        rc = lib.rt_render_iow01(C.byref(sc.camera), fptr(sph), C.byref(p), fptr(rgba), C.byref(st))
    elif sc.stage == RT_STAGE_IOW03:
        rc = lib.rt_render_iow03(fptr(sc.types), fptr(sc.records), sc.n, C.byref(sc.camera), C.byref(p),
                                 fptr(rgba), C.byref(st))
    else:
        depth = np.zeros((p.height, p.width), np.float32)
        lights = sc.lights if sc.lights is not None and len(sc.lights) else None
        tex = getattr(sc, "textures", None) or []
        if tex:
            arr, keep = texture_array(tex)
            rc = lib.rt_render_inw_tex(fptr(sc.geom), sc.n, sc.layout, fptr(sc.nodes), fptr(lights), sc.n_lights,
                                       arr, len(tex), C.byref(sc.camera), C.byref(p), fptr(rgba), fptr(depth),
                                       C.byref(st))
        else:
            rc = lib.rt_render_inw(fptr(sc.geom), sc.n, sc.layout, fptr(sc.nodes), fptr(lights), sc.n_lights,
                                   C.byref(sc.camera), C.byref(p), fptr(rgba), fptr(depth), C.byref(st))
    check(rc, "render")
    return rgba, depth, st.as_dict()


# ----------------------------------------------------------------------- ray queries
# rt_ray / rt_hit (include/rt_hip.h), 32 bytes each
RAY_DTYPE = np.dtype([("o", np.float32, 3), ("tmax", np.float32), ("d", np.float32, 3), ("ratio", np.float32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("id", np.int32), ("n", np.float32, 3), ("extra", np.float32),
                      ("pad", np.uint32, 2)])
RT_TRACE_INVERT, RT_TRACE_ANY = 1, 2


def trace(sc: Scene, rays: np.ndarray, flags: int = 0, device: int = -1):
    """rt_trace_inw: blocking closest-hit queries of `rays` (RAY_DTYPE) on a packed INW scene;
    returns (hits (HIT_DTYPE), stats dict)."""
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    hits = np.zeros(rays.shape, HIT_DTYPE)
    st = RtStats()
    check(load().rt_trace_inw(fptr(sc.geom), sc.n, sc.layout, fptr(sc.nodes), rays.ctypes.data, rays.size, int(flags),
                              hits.ctypes.data, device, C.byref(st)), "rt_trace_inw")
    return hits, st.as_dict()


def trace_kernel_info(any_hit: bool = False, fused: bool = True) -> dict:
    """rt_debug_trace_kernel: the query kernel's registers, scratch, LDS and resident blocks per CU."""
    info = (C.c_int * 4)()
    check(load().rt_debug_trace_kernel(int(any_hit), int(fused), info), "rt_debug_trace_kernel")
    return dict(zip(("vgprs", "scratch_bytes", "lds_bytes", "blocks_per_cu"), list(info)))


def trace_iow(sc: Scene, rays: np.ndarray, flags: int = 0, device: int = -1):
    """rt_trace_iow03: blocking closest-hit queries of `rays` (RAY_DTYPE) on a packed IOW-03 scene;
    returns (hits (HIT_DTYPE), stats dict)."""
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    hits = np.zeros(rays.shape, HIT_DTYPE)
    st = RtStats()
    check(load().rt_trace_iow03(fptr(sc.types), fptr(sc.records), sc.n, rays.ctypes.data, rays.size, int(flags),
                                hits.ctypes.data, device, C.byref(st)), "rt_trace_iow03")
    return hits, st.as_dict()


def trace_iow_kernel_info(any_hit: bool = False, lds: bool = True) -> dict:
    """rt_debug_trace_iow_kernel: the IOW-03 query kernel's registers, scratch, LDS and resident blocks per CU."""
    info = (C.c_int * 4)()
    check(load().rt_debug_trace_iow_kernel(int(any_hit), int(lds), info), "rt_debug_trace_iow_kernel")
    return dict(zip(("vgprs", "scratch_bytes", "lds_bytes", "blocks_per_cu"), list(info)))


# --------------------------------------------------------------------- path queries
# rt_path_ray / rt_path_out (include/rt_hip.h), 32 bytes each
PATH_RAY_DTYPE = np.dtype([("o", np.float32, 3), ("sample", np.uint32), ("d", np.float32, 3), ("pad", np.uint32)])
PATH_OUT_DTYPE = np.dtype([("rgb", np.float32, 3), ("depth", np.float32), ("segments", np.uint32),
                           ("drops", np.uint32), ("nans", np.uint32), ("status", np.uint32)])


def paths(sc: Scene, rays: np.ndarray, max_bounces: int, flags: int = 0, device: int = -1):
    """rt_path_inw: blocking path (radiance) queries of `rays` (PATH_RAY_DTYPE) on a packed INW scene
    with its lights and textures; the sample tables are sc.params.spp long.  Returns (out
    (PATH_OUT_DTYPE), stats dict)."""
    rays = np.ascontiguousarray(rays, PATH_RAY_DTYPE)
    out = np.zeros(rays.shape, PATH_OUT_DTYPE)
    st = RtStats()
    lights = sc.lights if sc.lights is not None and len(sc.lights) else None
    tex = getattr(sc, "textures", None) or []
    arr, keep = texture_array(tex)
    check(load().rt_path_inw(fptr(sc.geom), sc.n, sc.layout, fptr(sc.nodes), fptr(lights), sc.n_lights,
                             arr if tex else None, len(tex), int(sc.params.spp), int(max_bounces), rays.ctypes.data,
                             rays.size, int(flags), out.ctypes.data, device, C.byref(st)), "rt_path_inw")
    del keep
    return out, st.as_dict()


def paths_kernel_info(lights: bool = False, fused: bool = True) -> dict:
    """rt_debug_paths_kernel: the path-query kernel's registers, scratch, LDS and resident blocks per CU."""
    info = (C.c_int * 4)()
    check(load().rt_debug_paths_kernel(int(lights), int(fused), info), "rt_debug_paths_kernel")
    return dict(zip(("vgprs", "scratch_bytes", "lds_bytes", "blocks_per_cu"), list(info)))


# rt_path_iow_ray / rt_path_iow_out (include/rt_hip.h), 48 bytes each
PATH_IOW_RAY_DTYPE = np.dtype([("o", np.float32, 3), ("sample", np.uint32), ("d", np.float32, 3), ("pad", np.uint32),
                               ("ri_in", np.float32, 4)])
PATH_IOW_OUT_DTYPE = np.dtype([("rgb", np.float32, 3), ("stale", np.uint32), ("segments", np.uint32),
                               ("drops", np.uint32), ("nans", np.uint32), ("status", np.uint32),
                               ("ri_out", np.float32, 4)])


def path_iow(sc: Scene, rays: np.ndarray, max_bounces: int, chain: int = 1, spp: int | None = None,
             device: int = -1):
    """rt_path_iow03: blocking path (radiance) queries of `rays` (PATH_IOW_RAY_DTYPE) on a packed IOW-03
    scene, in chains of `chain`; the scatter table is spp (default sc.params.spp) long.  Returns (out
    (PATH_IOW_OUT_DTYPE), stats dict)."""
    rays = np.ascontiguousarray(rays, PATH_IOW_RAY_DTYPE)
    out = np.zeros(rays.shape, PATH_IOW_OUT_DTYPE)
    st = RtStats()
    check(load().rt_path_iow03(fptr(sc.types), fptr(sc.records), sc.n, int(sc.params.spp if spp is None else spp),
                               int(max_bounces), rays.ctypes.data, rays.size, int(chain), 0, out.ctypes.data, device,
                               C.byref(st)), "rt_path_iow03")
    return out, st.as_dict()


def path_iow_kernel_info(lds: bool = True) -> dict:
    """rt_debug_path_iow_kernel: the IOW-03 path-query kernel's registers, scratch, LDS and resident blocks per CU."""
    info = (C.c_int * 4)()
    check(load().rt_debug_path_iow_kernel(int(lds), info), "rt_debug_path_iow_kernel")
    return dict(zip(("vgprs", "scratch_bytes", "lds_bytes", "blocks_per_cu"), list(info)))


# -------------------------------------------------------------------- pixel queries
# rt_pixel / rt_pixel_out (include/rt_hip.h), 8 and 32 bytes
PIXEL_DTYPE = np.dtype([("x", np.int32), ("y", np.int32)])
PIXEL_OUT_DTYPE = np.dtype([("rgba", np.float32, 4), ("depth", np.float32), ("segments", np.uint32),
                            ("drops", np.uint32), ("nans", np.uint32)])


def as_pixels(pixels) -> np.ndarray:
    """PIXEL_DTYPE records from such records or from (n, 2) integer (x, y) pairs."""
    a = np.asarray(pixels)
    if a.dtype != PIXEL_DTYPE:
        xy = np.ascontiguousarray(a, np.int32).reshape(-1, 2)
        a = np.zeros(len(xy), PIXEL_DTYPE)
        a["x"], a["y"] = xy[:, 0], xy[:, 1]
    return np.ascontiguousarray(a.reshape(-1))


def dev_scene(sc: Scene, spp: int | None = None, device: int = -1):
    """A device scene (rt_dev_scene_iow03 / rt_dev_scene_inw_tex) of a packed scene with its lights and
    textures; free it with load().rt_dev_scene_free."""
    lib = load()
    spp = int(sc.params.spp if spp is None else spp)
    if sc.stage == RT_STAGE_IOW03:
        s = lib.rt_dev_scene_iow03(fptr(sc.types), fptr(sc.records), sc.n, spp, device)
    else:
        lights = sc.lights if sc.lights is not None and len(sc.lights) else None
        tex = getattr(sc, "textures", None) or []
        arr, keep = texture_array(tex)
        s = lib.rt_dev_scene_inw_tex(fptr(sc.geom), sc.n, sc.layout, fptr(sc.nodes), fptr(lights), sc.n_lights,
                                     arr if tex else None, len(tex), spp, device)
        del keep
    if not s:
        raise RuntimeError("device scene creation failed")
    return s


def camera_rays(sc: Scene, pixels, s0: int = 0, ns: int | None = None, params: RtParams | None = None):
    """rt_camera_rays_async through torch device buffers on the current stream: the camera rays of samples
    [s0, s0 + ns) (default: to spp) of `pixels` ((n, 2) (x, y) pairs or PIXEL_DTYPE) of the frame
    (sc.camera, params), pixel-major.  Returns PATH_RAY_DTYPE records (INW) or PATH_IOW_RAY_DTYPE (IOW-03)."""
    import torch
    lib = load()
    p = params or sc.params
    px = as_pixels(pixels)
    ns = int(p.spp - s0 if ns is None else ns)
    dtype = PATH_IOW_RAY_DTYPE if sc.stage == RT_STAGE_IOW03 else PATH_RAY_DTYPE
    n = len(px) * ns
    s = dev_scene(sc, p.spp)
    try:
        dev = torch.device("cuda")
        d_px = torch.from_numpy(np.frombuffer(px.tobytes() + bytes(8), np.uint8).copy()).to(dev)
        d_rays = torch.zeros(max(n, 1) * dtype.itemsize, dtype=torch.uint8, device=dev)
        check(lib.rt_camera_rays_async(s, C.byref(sc.camera), C.byref(p), d_px.data_ptr(), len(px), int(s0), ns,
                                       d_rays.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "rt_camera_rays_async")
        torch.cuda.synchronize()
        return d_rays.cpu().numpy()[: n * dtype.itemsize].view(dtype)
    finally:
        lib.rt_dev_scene_free(s)


def pixels(sc: Scene, pixels, want_rays: bool = False, want_samples: bool = False, params: RtParams | None = None,
           device: int = -1) -> dict:
    """rt_pixels_inw / rt_pixels_iow03: the blocking pixel query of `pixels` ((n, 2) (x, y) pairs or
    PIXEL_DTYPE) of the frame (sc.camera, params).  Returns {"pixels": PIXEL_OUT_DTYPE records, "stats":
    dict, and when asked for "rays" / "samples": (n, spp) path-query records / answers}."""
    lib = load()
    p = params or sc.params
    px = as_pixels(pixels)
    iow = sc.stage == RT_STAGE_IOW03
    n = len(px)
    out = np.zeros(n, PIXEL_OUT_DTYPE)
    rays = np.zeros((n, p.spp), PATH_IOW_RAY_DTYPE if iow else PATH_RAY_DTYPE) if want_rays else None
    samples = np.zeros((n, p.spp), PATH_IOW_OUT_DTYPE if iow else PATH_OUT_DTYPE) if want_samples else None
    st = RtStats()
    tail = (C.byref(sc.camera), C.byref(p), px.ctypes.data if n else None, n,
            rays.ctypes.data if want_rays else None, samples.ctypes.data if want_samples else None,
            out.ctypes.data if n else None, device, C.byref(st))
    if iow:
        check(lib.rt_pixels_iow03(fptr(sc.types), fptr(sc.records), sc.n, *tail), "rt_pixels_iow03")
    else:
        lights = sc.lights if sc.lights is not None and len(sc.lights) else None
        tex = getattr(sc, "textures", None) or []
        arr, keep = texture_array(tex)
        check(lib.rt_pixels_inw(fptr(sc.geom), sc.n, sc.layout, fptr(sc.nodes), fptr(lights), sc.n_lights,
                                arr if tex else None, len(tex), *tail), "rt_pixels_inw")
        del keep
    res = {"pixels": out, "stats": st.as_dict()}
    if want_rays:
        res["rays"] = rays
    if want_samples:
        res["samples"] = samples
    return res


PIXELS_KERNELS = ("k_camera_rays INW", "k_camera_rays IOW-03", "k_pixel_fold INW", "k_pixel_fold IOW-03")


def pixels_kernel_info(which: int) -> dict:
    """rt_debug_pixels_kernel: registers, scratch, LDS and resident blocks per CU of PIXELS_KERNELS[which]."""
    info = (C.c_int * 4)()
    check(load().rt_debug_pixels_kernel(int(which), info), "rt_debug_pixels_kernel")
    return dict(zip(("vgprs", "scratch_bytes", "lds_bytes", "blocks_per_cu"), list(info)))


# ------------------------------------------------------------- progressive passes
# rt_pass_state (include/rt_hip.h), 32 bytes
PASS_STATE_DTYPE = np.dtype([("acc", np.float32, 3), ("depth", np.float32), ("ri", np.float32, 4)])


def render_passes(sc: Scene, cuts, want_state: bool = False, params: RtParams | None = None, rgba=None, depth=None,
                  state=None, device: int = -1) -> dict:
    """rt_render_passes_inw / rt_render_passes_iow03: the blocking progressive passes of the frame
    (sc.camera, params): pass i renders samples [cuts[i - 1], cuts[i]) of the rectangle params.tile_*.
    Returns {"rgba": (n_cuts, H, W, 4), "depth": (n_cuts, H, W) or None on IOW-03, "stats": dict, and
    with want_state "state": (H, W) PASS_STATE_DTYPE after the last pass}.  rgba, depth and state: arrays
    of those shapes to start from (pixels outside the rectangle keep their bytes); default zeros."""
    lib = load()
    p = params or sc.params
    iow = sc.stage == RT_STAGE_IOW03
    cuts = np.ascontiguousarray(cuts, np.uint32).reshape(-1)
    n, H, W = len(cuts), p.height, p.width
    rgba = np.zeros((n, H, W, 4), np.float32) if rgba is None else np.ascontiguousarray(rgba, np.float32)
    assert rgba.shape == (n, H, W, 4)
    if iow:
        depth = None
    else:
        depth = np.zeros((n, H, W), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32)
        assert depth.shape == (n, H, W)
    if want_state:
        state = np.zeros((H, W), PASS_STATE_DTYPE) if state is None else np.ascontiguousarray(state, PASS_STATE_DTYPE)
        assert state.shape == (H, W)
    st = RtStats()
    tail = (state.ctypes.data if want_state else None, device, C.byref(st))
    if iow:
        check(lib.rt_render_passes_iow03(fptr(sc.types), fptr(sc.records), sc.n, C.byref(sc.camera), C.byref(p),
                                         cuts.ctypes.data_as(_U32P), n, fptr(rgba), *tail), "rt_render_passes_iow03")
    else:
        lights = sc.lights if sc.lights is not None and len(sc.lights) else None
        tex = getattr(sc, "textures", None) or []
        arr, keep = texture_array(tex)
        check(lib.rt_render_passes_inw(fptr(sc.geom), sc.n, sc.layout, fptr(sc.nodes), fptr(lights), sc.n_lights,
                                       arr if tex else None, len(tex), C.byref(sc.camera), C.byref(p),
                                       cuts.ctypes.data_as(_U32P), n, fptr(rgba), fptr(depth), *tail),
              "rt_render_passes_inw")
        del keep
    res = {"rgba": rgba, "depth": depth, "stats": st.as_dict()}
    if want_state:
        res["state"] = state
    return res


PASS_KERNELS = ("k_pass_rays (INW)", "k_pass_fold (INW)", "k_iow_pass LDS nodes", "k_iow_pass global nodes")


# rt_debug_pass_kernel's `which` of the tile-list instances (rt_render_pass_tiles_async)
PASS_TILE_KERNELS = {16: "k_pass_rays tile list (INW)", 17: "k_pass_fold tile list (INW)",
                     18: "k_iow_pass tile list, LDS nodes", 19: "k_iow_pass tile list, global nodes"}


def pass_kernel_info(which: int) -> dict:
    """rt_debug_pass_kernel: registers, scratch, LDS and resident blocks per CU of PASS_KERNELS[which]
    (which = 0..3), ADAPTIVE_KERNELS[which] (8..14), PASS_TILE_KERNELS[which] (16..19) or
    ADAPTIVE_TILE_KERNELS[which] (24..28, 30)."""
    info = (C.c_int * 4)()
    check(load().rt_debug_pass_kernel(int(which), info), "rt_debug_pass_kernel")
    return dict(zip(("vgprs", "scratch_bytes", "lds_bytes", "blocks_per_cu"), list(info)))


# ------------------------------------------------------------- adaptive sample passes
# rt_pass_aux (include/rt_hip.h), 16 bytes; rt_pixel, 8 bytes
PASS_AUX_DTYPE = np.dtype([("even", np.float32, 3), ("count", np.uint32)])
PIXEL_DTYPE = np.dtype([("x", np.int32), ("y", np.int32)])
# rt_debug_pass_kernel's `which` of the adaptive-pass kernels
ADAPTIVE_KERNELS = {8: "k_adapt_rays (INW)", 9: "k_adapt_fold (INW)", 10: "k_iow_adapt LDS nodes",
                    11: "k_iow_adapt global nodes", 12: "k_select_count", 13: "k_select_scan", 14: "k_select_scatter"}


# ... and of their tile-list instances (rt_render_pass_slots_async, rt_pass_select_tiles_async): + 16; the scan
# serves both forms
ADAPTIVE_TILE_KERNELS = {24: "k_adapt_rays tile list (INW)", 25: "k_adapt_fold tile list (INW)",
                         26: "k_iow_adapt tile list, LDS nodes", 27: "k_iow_adapt tile list, global nodes",
                         28: "k_select_count tile list", 30: "k_select_scatter tile list"}
SLOT_NONE = 0xFFFFFFFF  # RT_SLOT_NONE: the padding of a slot list


def _dptr(t):
    """A device pointer: None, an integer, or anything with data_ptr() (a torch tensor)."""
    return t.data_ptr() if hasattr(t, "data_ptr") else t


def update_inw_device(handle, d_geom, n: int, d_aabbs, d_lights=None, n_lights: int = 0, flags: int = 0,
                      stream=None) -> list:
    """rt_dev_scene_inw_update_device: the next frame's geometry of the INW device scene `handle` from
    device buffers (pointers or torch tensors): d_geom n * 28 records, d_aabbs n * 6 boxes, d_lights the
    layout-4 lights; flags 0, RT_UPDATE_BINS or RT_UPDATE_NO_BINS.  Returns timing_ms: host ms of [records
    and decisions, LBVH, swept tree + RI grid + derived nodes, time-bin trees]."""
    tm = (C.c_double * 4)()
    check(load().rt_dev_scene_inw_update_device(handle, _dptr(d_geom), int(n), _dptr(d_aabbs), _dptr(d_lights),
                                                int(n_lights), int(flags), stream, tm),
          "rt_dev_scene_inw_update_device")
    return list(tm)


def inw_swept_boxes(d_geom, n: int, d_out, stream=None) -> None:
    """rt_inw_swept_boxes_async: per record of d_geom (n * 28, device) a box that holds the object over
    the shutter interval into d_out (n * 6, device); pointers or torch tensors."""
    check(load().rt_inw_swept_boxes_async(_dptr(d_geom), int(n), _dptr(d_out), stream), "rt_inw_swept_boxes_async")


UPDATE_KERNELS = ("k_inw_prepare", "k_bin_boxes", "k_swept_boxes", "k_bin_place")


def update_kernel_info(which: int) -> dict:
    """rt_debug_update_kernel: registers, scratch, LDS and resident blocks per CU of UPDATE_KERNELS[which]."""
    info = (C.c_int * 4)()
    check(load().rt_debug_update_kernel(int(which), info), "rt_debug_update_kernel")
    return dict(zip(("vgprs", "scratch_bytes", "lds_bytes", "blocks_per_cu"), list(info)))


def update_iow03_device(handle, d_types, d_records, n: int, flags: int = 0, stream=None) -> list:
    """rt_dev_scene_iow03_update_device: the next edit of the IOW-03 device scene `handle` from device
    buffers (pointers or torch tensors): d_types n floats, d_records n * 24; flags 0, RT_UPDATE_HOST_BUILD
    or RT_UPDATE_DEVICE_BUILD.  Returns timing_ms: host ms of [records and priors, boxes and culling BVH,
    copy-back + upload of host-built structures, the whole call]."""
    tm = (C.c_double * 4)()
    check(load().rt_dev_scene_iow03_update_device(handle, _dptr(d_types), _dptr(d_records), int(n), int(flags), stream,
                                                  tm), "rt_dev_scene_iow03_update_device")
    return list(tm)


IOW_HOT_FLOATS, IOW_COLD_FLOATS = 20, 8


def iow_prepare_host(types: np.ndarray, records: np.ndarray) -> dict:
    """rt_debug_iow_prepare_host: the host packer's hot (n, 20) and cold (n, 8) records and the RI priors
    (10 floats: ri_prior, alt_vals[8], n_alt_vals) of IOW-03 types (n) and records (n, 24).  No device."""
    types = np.ascontiguousarray(types, np.float32)
    records = np.ascontiguousarray(records, np.float32)
    n = len(types)
    hot, cold = np.zeros((n, IOW_HOT_FLOATS), np.float32), np.zeros((n, IOW_COLD_FLOATS), np.float32)
    priors = np.zeros(10, np.float32)
    check(load().rt_debug_iow_prepare_host(fptr(types), fptr(records), n, fptr(hot), fptr(cold), fptr(priors)),
          "rt_debug_iow_prepare_host")
    return {"hot": hot, "cold": cold, "priors": priors}


def iow_records(handle) -> dict:
    """rt_debug_iow_records: the current hot records, cold records and priors of an IOW-03 device scene, in
    iow_prepare_host's keys."""
    n = iow_info(handle)["objects"]
    hot, cold = np.zeros((n, IOW_HOT_FLOATS), np.float32), np.zeros((n, IOW_COLD_FLOATS), np.float32)
    priors = np.zeros(10, np.float32)
    check(load().rt_debug_iow_records(handle, fptr(hot), fptr(cold), fptr(priors)), "rt_debug_iow_records")
    return {"hot": hot, "cold": cold, "priors": priors}


UPDATE_IOW_KERNELS = ("k_iow_prepare float4 loads", "k_iow_prepare scalar loads", "k_iow_mode", "k_iow_priors")


def update_iow_kernel_info(which: int) -> dict:
    """rt_debug_update_iow_kernel: registers, scratch, LDS and resident blocks per CU of UPDATE_IOW_KERNELS[which]."""
    info = (C.c_int * 4)()
    check(load().rt_debug_update_iow_kernel(int(which), info), "rt_debug_update_iow_kernel")
    return dict(zip(("vgprs", "scratch_bytes", "lds_bytes", "blocks_per_cu"), list(info)))


def pass_pixels(handle, camera: RtCamera, params: RtParams, d_pixels, n_pixels: int, ns: int, d_state, d_aux,
                d_rgba=None, d_depth=None, d_counters=None, stream=None) -> int:
    """rt_render_pass_pixels_async on device buffers (pointers or torch tensors); returns the status."""
    return load().rt_render_pass_pixels_async(handle, C.byref(camera), C.byref(params), _dptr(d_pixels), n_pixels, ns,
                                              _dptr(d_state), _dptr(d_aux), _dptr(d_rgba), _dptr(d_depth),
                                              _dptr(d_counters), stream)


def render_pass_tiles(handle, camera: RtCamera, params: RtParams, d_tiles, n_tiles: int, tile_size: int, s0: int,
                      ns: int, d_state, d_out=None, d_depth=None, d_counters=None, stream=None) -> int:
    """rt_render_pass_tiles_async on device buffers (pointers or torch tensors); returns the status."""
    return load().rt_render_pass_tiles_async(handle, C.byref(camera), C.byref(params), _dptr(d_tiles), n_tiles,
                                             tile_size, s0, ns, _dptr(d_state), _dptr(d_out), _dptr(d_depth),
                                             _dptr(d_counters), stream)


def render_passes_multi(sc: Scene, devices, cuts, tile: int = 16, rgba=None, depth=None) -> dict:
    """rt_render_passes_inw_multi: the blocking progressive passes of the INW frame (sc.camera, sc.params) on
    the device group `devices`.  Returns {"rgba": (n_cuts, H, W, 4), "depth": (n_cuts, H, W), "stats": dict};
    rgba and depth: arrays of those shapes to start from, default zeros."""
    p = sc.params
    cuts = np.ascontiguousarray(cuts, np.uint32).reshape(-1)
    n, H, W = len(cuts), p.height, p.width
    rgba = np.zeros((n, H, W, 4), np.float32) if rgba is None else np.ascontiguousarray(rgba, np.float32)
    depth = np.zeros((n, H, W), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32)
    assert rgba.shape == (n, H, W, 4) and depth.shape == (n, H, W)
    devs = (C.c_int * len(devices))(*devices)
    lights = sc.lights if sc.lights is not None and len(sc.lights) else None
    st = RtStats()
    check(load().rt_render_passes_inw_multi(fptr(sc.geom), sc.n, sc.layout, fptr(sc.nodes), fptr(lights), sc.n_lights,
                                            C.byref(sc.camera), C.byref(p), devs, len(devices), tile,
                                            cuts.ctypes.data_as(_U32P), n, fptr(rgba), fptr(depth), C.byref(st)),
          "rt_render_passes_inw_multi")
    return {"rgba": rgba, "depth": depth, "stats": st.as_dict()}


def pass_select(handle, params: RtParams, d_state, d_aux, tol: float, min_samples: int, d_list, d_n_active,
                d_err=None, stream=None) -> int:
    """rt_pass_select_async on device buffers (pointers or torch tensors); returns the status."""
    return load().rt_pass_select_async(handle, C.byref(params), _dptr(d_state), _dptr(d_aux), float(tol),
                                       int(min_samples), _dptr(d_list), _dptr(d_n_active), _dptr(d_err), stream)


def pass_slots(handle, camera: RtCamera, params: RtParams, d_tiles, n_tiles: int, tile_size: int, d_slots,
               n_slots: int, ns: int, d_state, d_aux, d_out=None, d_depth=None, d_counters=None, stream=None) -> int:
    """rt_render_pass_slots_async on device buffers (pointers or torch tensors); returns the status."""
    return load().rt_render_pass_slots_async(handle, C.byref(camera), C.byref(params), _dptr(d_tiles), n_tiles,
                                             tile_size, _dptr(d_slots), n_slots, ns, _dptr(d_state), _dptr(d_aux),
                                             _dptr(d_out), _dptr(d_depth), _dptr(d_counters), stream)


def pass_select_tiles(handle, params: RtParams, d_tiles, n_tiles: int, tile_size: int, d_state, d_aux, tol: float,
                      min_samples: int, d_slots, d_n_active, d_err=None, stream=None) -> int:
    """rt_pass_select_tiles_async on device buffers (pointers or torch tensors); returns the status."""
    return load().rt_pass_select_tiles_async(handle, C.byref(params), _dptr(d_tiles), n_tiles, tile_size,
                                             _dptr(d_state), _dptr(d_aux), float(tol), int(min_samples),
                                             _dptr(d_slots), _dptr(d_n_active), _dptr(d_err), stream)


def render_adaptive_multi_round(group, scenes, camera: RtCamera, params: RtParams, tile: int, first: bool, ns: int,
                                tol: float, min_samples: int, d_rgba=None, d_depth=None, d_count=None,
                                d_counters=None, stream=None) -> int:
    """rt_render_adaptive_multi_async: one adaptive round of the group (scenes: a ctypes array of one device
    scene per group device; the buffers are device-0 pointers or torch tensors); returns the status."""
    return load().rt_render_adaptive_multi_async(group, scenes, C.byref(camera), C.byref(params), tile,
                                                 1 if first else 0, ns, float(tol), int(min_samples), _dptr(d_rgba),
                                                 _dptr(d_depth), _dptr(d_count), _dptr(d_counters), stream)


def group_adaptive_active(group) -> int:
    """rt_group_adaptive_active: the active slots the group's last adaptive round left (waits for the counts)."""
    n = C.c_uint32(0)
    check(load().rt_group_adaptive_active(group, C.byref(n)), "rt_group_adaptive_active")
    return int(n.value)


def render_adaptive_multi(sc: Scene, devices, batch: int, tol: float, min_samples: int = 2,
                          max_rounds: int | None = None, tile: int = 16, rgba=None, depth=None) -> dict:
    """rt_render_adaptive_inw_multi: the blocking adaptive loop of the INW frame (sc.camera, sc.params) on the
    device group `devices`.  Returns {"rgba": (H, W, 4), "depth": (H, W), "count": (H, W) uint32, "rounds":
    int, "stats": dict}; rgba and depth: arrays of those shapes to start from, default zeros."""
    p = sc.params
    H, W = p.height, p.width
    rgba = np.zeros((H, W, 4), np.float32) if rgba is None else np.ascontiguousarray(rgba, np.float32)
    depth = np.zeros((H, W), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32)
    assert rgba.shape == (H, W, 4) and depth.shape == (H, W)
    count = np.zeros((H, W), np.uint32)
    rounds = C.c_uint32(0)
    devs = (C.c_int * len(devices))(*devices)
    lights = sc.lights if sc.lights is not None and len(sc.lights) else None
    st = RtStats()
    check(load().rt_render_adaptive_inw_multi(fptr(sc.geom), sc.n, sc.layout, fptr(sc.nodes), fptr(lights), sc.n_lights,
                                              C.byref(sc.camera), C.byref(p), devs, len(devices), tile, int(batch),
                                              float(tol), int(min_samples), int(max_rounds or 0), fptr(rgba),
                                              fptr(depth), count.ctypes.data, C.addressof(rounds), C.byref(st)),
          "rt_render_adaptive_inw_multi")
    return {"rgba": rgba, "depth": depth, "count": count, "rounds": int(rounds.value), "stats": st.as_dict()}


def render_adaptive(sc: Scene, batch: int, tol: float, min_samples: int = 2, max_rounds: int | None = None,
                    params: RtParams | None = None, rgba=None, depth=None, state=None, device: int = -1) -> dict:
    """rt_render_adaptive_inw / rt_render_adaptive_iow03: the blocking adaptive loop on the frame (sc.camera,
    params) -- rounds of one listed pass of `batch` samples and one select, while pixels are active and
    rounds remain (max_rounds None: no limit).  Returns {"rgba": (H, W, 4), "depth": (H, W) or None on
    IOW-03, "count": (H, W) uint32, "err": (H, W) (+inf where no select ran), "state": (H, W)
    PASS_STATE_DTYPE, "aux": (H, W) PASS_AUX_DTYPE, "rounds": int, "stats": dict}.  rgba, depth and state:
    arrays of those shapes to start from (pixels outside the rectangle keep their bytes); default zeros."""
    lib = load()
    p = params or sc.params
    iow = sc.stage == RT_STAGE_IOW03
    H, W = p.height, p.width
    rgba = np.zeros((H, W, 4), np.float32) if rgba is None else np.ascontiguousarray(rgba, np.float32)
    assert rgba.shape == (H, W, 4)
    if iow:
        depth = None
    else:
        depth = np.zeros((H, W), np.float32) if depth is None else np.ascontiguousarray(depth, np.float32)
        assert depth.shape == (H, W)
    state = np.zeros((H, W), PASS_STATE_DTYPE) if state is None else np.ascontiguousarray(state, PASS_STATE_DTYPE)
    assert state.shape == (H, W)
    count = np.zeros((H, W), np.uint32)
    err = np.full((H, W), np.inf, np.float32)
    aux = np.zeros((H, W), PASS_AUX_DTYPE)
    rounds = C.c_uint32(0)
    st = RtStats()
    mid = (int(batch), float(tol), int(min_samples), int(max_rounds or 0), fptr(rgba))
    tail = (count.ctypes.data, err.ctypes.data, state.ctypes.data, aux.ctypes.data, C.addressof(rounds), device,
            C.byref(st))
    if iow:
        check(lib.rt_render_adaptive_iow03(fptr(sc.types), fptr(sc.records), sc.n, C.byref(sc.camera), C.byref(p),
                                           *mid, *tail), "rt_render_adaptive_iow03")
    else:
        lights = sc.lights if sc.lights is not None and len(sc.lights) else None
        tex = getattr(sc, "textures", None) or []
        arr, keep = texture_array(tex)
        check(lib.rt_render_adaptive_inw(fptr(sc.geom), sc.n, sc.layout, fptr(sc.nodes), fptr(lights), sc.n_lights,
                                         arr if tex else None, len(tex), C.byref(sc.camera), C.byref(p), *mid,
                                         fptr(depth), *tail), "rt_render_adaptive_inw")
        del keep
    return {"rgba": rgba, "depth": depth, "count": count, "err": err, "state": state, "aux": aux,
            "rounds": int(rounds.value), "stats": st.as_dict()}


def render_iow01(camera: RtCamera, sphere, params: RtParams):
    sc = Scene(stage=RT_STAGE_IOW01, desc=None, n=0, camera=camera, params=params)
    rgba, _, st = render(sc, params, sphere=sphere)
    return rgba, st


def render_iow00(params: RtParams) -> np.ndarray:
    """IOW-00 (In-One-Weekend/base.cpp:7-28): the UV gradient of the base stage."""
    rgba = np.zeros((params.height, params.width, 4), np.float32)
    check(load().rt_render_iow00(C.byref(params), fptr(rgba)), "rt_render_iow00")
    return rgba


def pack_iow02(desc, n: int) -> tuple[np.ndarray, np.ndarray]:
    """Groups::Geometry::FillBuffer (groups.h:45-64): types[N], records[N, 18]."""
    types = np.zeros(n, np.float32)
    rec = np.zeros((n, 18), np.float32)
    check(load().rt_pack_iow02(desc, n, fptr(types), fptr(rec)), "rt_pack_iow02")
    return types, rec


def render_iow02(types, records, camera: RtCamera, params: RtParams, cull_front: int = 0, cull_back: int = 1):
    """IOW-02 groups stage (02_Groups/computeShaderSrc.glsl); defaults cull the back side
    (groups.h:91-92)."""
    types = np.ascontiguousarray(types, np.float32)
    records = np.ascontiguousarray(records, np.float32).reshape(-1, 18)
    rgba = np.zeros((params.height, params.width, 4), np.float32)
    st = RtStats()
    check(load().rt_render_iow02(fptr(types), fptr(records), len(types), C.byref(camera), C.byref(params),
                                 int(cull_front), int(cull_back), fptr(rgba), C.byref(st)), "rt_render_iow02")
    return rgba, st.as_dict()


def render_inw_mf(sc: "Scene", focus, params: RtParams | None = None):
    """INW-01 with the shader's MULTIFOCUS branch (01_BVH...glsl:388-404, 505-549), focus distances
    `focus` (1..9)."""
    p = params or sc.params
    f = np.ascontiguousarray(focus, np.float32)
    rgba = np.zeros((p.height, p.width, 4), np.float32)
    depth = np.zeros((p.height, p.width), np.float32)
    st = RtStats()
    check(load().rt_render_inw_mf(fptr(sc.geom), sc.n, fptr(sc.nodes), C.byref(sc.camera), fptr(f), len(f),
                                  C.byref(p), fptr(rgba), fptr(depth), C.byref(st)), "rt_render_inw_mf")
    return rgba, depth, st.as_dict()


def iow01_defaults(width: int = 400, height: int = 225) -> tuple[RtCamera, np.ndarray, RtParams]:
    """IOW-01 stage defaults (Sphere.h:26,34-37): camera (0,1,10), pitch 0 / yaw -90, focus 1,
    sphere (0,3,-1) r 3, ShowNormal = true."""
    cd = RtCamDesc()
    cd.position[:] = (0.0, 1.0, 10.0)
    cd.pitch_deg, cd.yaw_deg, cd.fov_y_deg, cd.aperture, cd.focus_dist = 0.0, -90.0, 0.0, 0.0, 1.0
    cam = camera_from_desc(cd, RT_STAGE_IOW01)
    p = RtParams()
    p.width, p.height, p.spp, p.max_bounces, p.show_normal, p.device = width, height, 1, 1, 1, -1
    return cam, np.array([0.0, 3.0, -1.0, 3.0], np.float32), p
