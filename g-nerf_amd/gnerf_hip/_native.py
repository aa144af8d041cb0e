"""The native library itself: where it is, its C ABI (signatures and structs), loading it, and what every wrapper needs to hand a
tensor to it.  ALL mutable state of the package lives in this module (_lib, _ext, _workspaces, _split_overflow, _device_geometry,
_filter_tap_cache, _decoder_packs, _decoder_seen): the sibling modules read it as `_native._ext` and never import those names, which would freeze a copy."""

import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# GNERF_HIP_LIB points tools/ablate.py at a timing-only variant build; everything else uses the in-tree library.
LIB_PATH = os.environ.get('GNERF_HIP_LIB') or os.path.join(_HERE, 'libgnerf_hip.so')

_lib = None

F32, F16, F64 = 0, 1, 2
_DTYPE_CODE = {torch.float32: F32, torch.float16: F16, torch.float64: F64}

MAX_SAMPLES = 256
DEBUG_SLOTS = 8
ABI_VERSION = 15
# decoder arithmetic of the fused renderer (GNERF_MLP_* in include/gnerf_hip.h)
MLP_MODES = {'auto': 0, 'f16x3': 1, 'f32': 2}

_c_p = ctypes.c_void_p
_c_i = ctypes.c_int
_c_i64 = ctypes.c_int64
_c_f = ctypes.c_float


class RenderParams(ctypes.Structure):
    """struct gnerf_render_params (include/gnerf_hip.h)."""
    _fields_ = [
        ('planes_nhwc', _c_p), ('n_items', ctypes.c_int32), ('plane_h', ctypes.c_int32), ('plane_w', ctypes.c_int32),
        ('ray_origins', _c_p), ('ray_dirs', _c_p), ('rays_per_item', ctypes.c_int32), ('image_width', ctypes.c_int32),
        ('w1', _c_p), ('b1', _c_p), ('w2', _c_p), ('b2', _c_p),
        ('depth_resolution', ctypes.c_int32), ('depth_resolution_importance', ctypes.c_int32),
        ('ray_start', _c_f), ('ray_end', _c_f),
        ('ray_start_per_ray', _c_p), ('ray_end_per_ray', _c_p),
        ('box_warp', _c_f), ('white_back', ctypes.c_int32), ('disparity_space_sampling', ctypes.c_int32),
        ('noise_coarse', _c_p), ('noise_fine', _c_p),
        ('out_rgb', _c_p), ('out_depth', _c_p), ('out_wsum', _c_p),
        ('workspace', _c_p), ('debug', _c_p),
        ('planes_absmax', _c_p), ('mlp_mode', ctypes.c_int32), ('planes_interleaved', ctypes.c_int32),
        ('planes_shared', ctypes.c_int32), ('depth_clamp_per_item', ctypes.c_int32),
        ('cam2world', _c_p), ('intrinsics', _c_p), ('rng_mode', ctypes.c_int32), ('rng_per_item', ctypes.c_int32),
        ('rng_seed', ctypes.c_uint64), ('rng_offset_coarse', ctypes.c_uint64), ('rng_offset_fine', ctypes.c_uint64),
        ('rng_offset_item_stride', ctypes.c_uint64), ('rng_threads_coarse', ctypes.c_uint32), ('rng_threads_fine', ctypes.c_uint32),
        ('sigma_noise_coarse', _c_p), ('sigma_noise_fine', _c_p),
    ]


class RenderGrads(ctypes.Structure):
    """struct gnerf_render_grads (include/gnerf_hip.h)."""
    _fields_ = [
        ('grad_rgb', _c_p), ('grad_depth', _c_p), ('grad_wsum', _c_p),
        ('grad_planes_nhwc', _c_p),
        ('grad_w1', _c_p), ('grad_b1', _c_p), ('grad_w2', _c_p), ('grad_b2', _c_p),
        ('scatter_stage', _c_p),
    ]


# name -> (restype, argtypes); must list every function include/gnerf_hip.h declares (tests check this).
SIGNATURES = {
    'gnerf_abi_version': (_c_i, []),
    'gnerf_last_error': (ctypes.c_char_p, []),
    'gnerf_build_info': (ctypes.c_char_p, []),
    'gnerf_clock_sample': (_c_i, [_c_p, ctypes.c_double, _c_p]),
    'gnerf_bias_act': (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i64, _c_i, _c_i64, _c_i, _c_i, _c_f, _c_f, _c_f, _c_p]),
    'gnerf_upfirdn2d': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, ctypes.POINTER(_c_i64), _c_i, _c_i, ctypes.POINTER(_c_i64),
                               _c_i, _c_i, ctypes.POINTER(_c_i64), _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_f, _c_p]),
    'gnerf_filtered_lrelu_act': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, ctypes.POINTER(_c_i64), _c_i, _c_i, _c_i, _c_i,
                                        _c_f, _c_f, _c_f, _c_i, _c_p]),
    'gnerf_filtered_lrelu': (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, ctypes.POINTER(_c_i64),
                                    _c_i, _c_i, ctypes.POINTER(_c_i64), _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i,
                                    _c_i, _c_i, _c_i, _c_i, _c_i, _c_f, _c_f, _c_f, _c_i, _c_p]),
    'gnerf_grid_sample_2d': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, ctypes.POINTER(_c_i64), _c_i, _c_i, _c_p]),
    'gnerf_grid_sample_2d_backward': (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, ctypes.POINTER(_c_i64), _c_i, _c_i, _c_p]),
    'gnerf_planes_to_nhwc': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p]),
    'gnerf_planes_to_nhwc_stats': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p, _c_p, _c_p]),
    'gnerf_planes_absmax': (_c_i, [_c_p, _c_i64, _c_p, _c_p]),
    'gnerf_planes_from_nhwc': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p]),
    'gnerf_make_rays': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_p, _c_p, _c_p]),
    'gnerf_torch_rand_plan': (_c_i, [_c_i64, _c_i, _c_i, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]),
    'gnerf_torch_rand': (_c_i, [_c_p, _c_i64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, _c_p]),
    'gnerf_to_uint8_nhwc': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p]),
    'gnerf_render_workspace_bytes': (ctypes.c_size_t, []),
    'gnerf_render_forward': (_c_i, [ctypes.POINTER(RenderParams), _c_p]),
    'gnerf_render_backward': (_c_i, [ctypes.POINTER(RenderParams), ctypes.POINTER(RenderGrads), _c_p]),
    'gnerf_render_backward_rays': (_c_i, [ctypes.POINTER(RenderParams), ctypes.POINTER(RenderGrads), _c_p, _c_p, _c_p]),
    'gnerf_render_scatter_rows': (_c_i, [ctypes.POINTER(RenderParams), _c_p, _c_p, _c_p]),
    'gnerf_render_decoder_pack_bytes': (ctypes.c_size_t, []),
    'gnerf_render_pack_decoder': (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_render_forward_packed': (_c_i, [ctypes.POINTER(RenderParams), _c_p, _c_p]),
    'gnerf_render_backward_stage_bytes': (ctypes.c_size_t, [ctypes.POINTER(RenderParams)]),
    'gnerf_render_backward_exchange_bytes': (ctypes.c_size_t, [ctypes.POINTER(RenderParams)]),
    'gnerf_query_points': (_c_i, [_c_p, _c_i, _c_i, _c_i, _c_p, _c_i, _c_f, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_p]),
    'gnerf_query_points_backward': (_c_i, [_c_p, _c_i, _c_i, _c_i, _c_p, _c_i, _c_f, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p,
                                           _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_p]),
    'gnerf_query_points_grad': (_c_i, [_c_p, _c_i, _c_i, _c_i, _c_p, _c_i, _c_f, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_p]),
    'gnerf_project_points_to_level': (_c_i, [_c_p, _c_i, _c_i, _c_i, _c_p, _c_i, _c_f, _c_p, _c_p, _c_p, _c_p, _c_f, ctypes.POINTER(_c_f), _c_i, _c_f, _c_f,
                                             _c_p, _c_p, _c_p, _c_p, _c_i, _c_p]),
    'gnerf_modulate_weights':(_c_i, [_c_p, _c_p, _c_p, _c_i, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_p]),
    'gnerf_normalise_styles': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_p]),
    'gnerf_scale_channels': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p]),
    'gnerf_modconv_epilogue': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p, _c_p, _c_i, _c_i, _c_p, _c_i, _c_f, _c_f, _c_f, _c_p]),
    'gnerf_conv3x3_epilogue_nhwc': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_p, _c_p, _c_i, _c_p, _c_f, _c_f, _c_f, _c_p, _c_p]),
    'gnerf_conv_transpose3x3_s2_nhwc': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_p]),
    'gnerf_conv3x3_epilogue_torgb_nhwc': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p, _c_p, _c_i, _c_p, _c_f, _c_f, _c_f, _c_p, _c_p, _c_f, _c_p, _c_p]),
    'gnerf_split_f16x3_nhwc': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p, _c_p]),
    'gnerf_make_rays_and_draws': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_p, _c_p, _c_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint32,
                                         _c_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, _c_p]),
    'gnerf_conv3x3_f32x3_epilogue_nhwc': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_p, _c_p, _c_p, _c_f, _c_f, _c_f, _c_p, _c_p]),
    'gnerf_conv_transpose3x3_s2_f32x3_nhwc': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_p]),
    'gnerf_upsample2x_add_nhwc': (_c_i, [_c_p, _c_p, ctypes.POINTER(_c_f), _c_i, _c_f, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p, _c_p]),
    'gnerf_scale_channels_nhwc': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p]),
    'gnerf_modconv_epilogue_nhwc': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p, _c_p, _c_i, _c_i, _c_p, _c_i, _c_f, _c_f, _c_f, _c_p, _c_p]),
    'gnerf_torgb_nhwc': (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_f, _c_p]),
    'gnerf_torgb_nhwc_accumulate': (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_f, _c_p]),
    'gnerf_blur4_epilogue_nhwc': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_f, _c_p, _c_p, _c_i, _c_f, _c_f, _c_f, _c_p, _c_p]),
    'gnerf_marching_cubes_workspace_bytes': (_c_i, [_c_i, _c_i, _c_i, ctypes.POINTER(ctypes.c_size_t)]),
    'gnerf_marching_cubes_count': (_c_i, [_c_p, _c_i, _c_i, _c_i, _c_f, _c_p, _c_p, _c_p]),
    'gnerf_marching_cubes_emit': (_c_i, [_c_p, _c_i, _c_i, _c_i, _c_f, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_ssim_workspace_bytes': (_c_i, [_c_i, _c_i, _c_i, _c_i, _c_i, ctypes.POINTER(ctypes.c_size_t)]),
    'gnerf_ssim_forward': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), ctypes.POINTER(_c_f), _c_i,
                                  _c_f, _c_f, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_ssim_backward': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), ctypes.POINTER(_c_f), _c_i,
                                   _c_f, _c_f, _c_p, _c_p, _c_p, ctypes.POINTER(_c_i64), _c_p, ctypes.POINTER(_c_i64), _c_p]),
    'gnerf_modconv_backward_workspace_bytes': (_c_i, [_c_i, _c_i, _c_i, _c_i, _c_i, ctypes.POINTER(ctypes.c_size_t)]),
    'gnerf_scale_channels_backward': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_scale_channels_backward_nhwc': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_modconv_epilogue_backward': (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_f, _c_f, _c_f, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_modconv_epilogue_backward_nhwc': (_c_i, [_c_p, _c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_f, _c_f, _c_f, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_resize_aa_forward': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), _c_i,
                                       ctypes.c_double, ctypes.c_double, _c_p]),
    'gnerf_resize_aa_backward': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, _c_i, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), _c_i,
                                        ctypes.c_double, ctypes.c_double, _c_p]),
    'gnerf_raster_workspace_bytes': (_c_i, [_c_i, _c_i, _c_i, _c_i, _c_i, ctypes.POINTER(ctypes.c_size_t)]),
    'gnerf_raster_visibility': (_c_i, [_c_p, _c_i, _c_p, _c_i, _c_p, _c_p, _c_i, _c_i, _c_i, _c_f, _c_i, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_raster_resolve': (_c_i, [_c_p, _c_p, _c_i, _c_p, _c_i, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p, _c_p, _c_p, ctypes.POINTER(_c_f),
                                    _c_p, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_mesh_bake_colors': (_c_i, [_c_p, _c_i, _c_p, _c_p, _c_i, _c_p, _c_i, _c_i, _c_p, _c_i, _c_i, _c_p, _c_p, _c_f, _c_f, _c_i, _c_f, _c_i, _c_p,
                                      _c_p, _c_p, _c_p, _c_p]),
    'gnerf_mesh_atlas_layout': (_c_i, [_c_i, _c_i, ctypes.POINTER(_c_i), ctypes.POINTER(_c_i), ctypes.POINTER(_c_i)]),
    'gnerf_mesh_bake_texture': (_c_i, [_c_p, _c_i, _c_p, _c_i, _c_i, _c_p, _c_p, _c_i, _c_p, _c_i, _c_i, _c_p, _c_i, _c_i, _c_p, _c_p, _c_f, _c_f, _c_i, _c_f, _c_i,
                                       _c_p, ctypes.POINTER(ctypes.c_ubyte), _c_p, _c_p, _c_p, _c_p]),
    'gnerf_raster_resolve_textured': (_c_i, [_c_p, _c_p, _c_i, _c_p, _c_i, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p, _c_i, ctypes.POINTER(ctypes.c_ubyte), _c_p, _c_p]),
    'gnerf_mesh_workspace_bytes': (_c_i, [_c_i, _c_i, ctypes.POINTER(ctypes.c_size_t)]),
    'gnerf_mesh_components': (_c_i, [_c_p, _c_i, _c_i, _c_p, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_mesh_compact_count': (_c_i, [_c_p, _c_i, _c_i, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_mesh_compact_emit': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_mesh_smooth': (_c_i, [_c_p, _c_i, _c_p, _c_i, _c_i, _c_f, _c_f, _c_i, _c_p, _c_p, _c_p]),
    'gnerf_mesh_simplify_workspace_bytes': (_c_i, [_c_i, _c_i, ctypes.POINTER(ctypes.c_size_t)]),
    'gnerf_mesh_simplify_count': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_f, ctypes.POINTER(_c_f), _c_p, _c_p, _c_p]),
    'gnerf_mesh_simplify_emit': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_f, ctypes.POINTER(_c_f), _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_mesh_flip_guard': (_c_i, [_c_p, _c_p, _c_p, _c_i, _c_i, _c_i, _c_p, _c_p, _c_p, _c_p]),
    'gnerf_query_lattice': (_c_i, [_c_p, _c_i, _c_i, _c_p, _c_i, _c_i, ctypes.c_double, _c_f, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i, _c_p]),
    'gnerf_band_workspace_bytes': (_c_i, [_c_i, _c_i, ctypes.POINTER(ctypes.c_size_t)]),
    'gnerf_band_seed': (_c_i, [_c_p, _c_i, _c_i, _c_f, ctypes.POINTER(_c_i), _c_p, _c_p, _c_p, _c_p]),
    'gnerf_band_points_count': (_c_i, [_c_p, _c_i, _c_i, _c_p, _c_p, _c_p]),
    'gnerf_band_points_emit': (_c_i, [_c_p, _c_i, _c_i, _c_p, _c_p, _c_i64, _c_p]),
    'gnerf_band_grow': (_c_i, [_c_p, _c_i, _c_i, _c_f, ctypes.POINTER(_c_i), _c_p, _c_p, _c_p, _c_p]),
    'gnerf_band_fill': (_c_i, [_c_p, _c_i, _c_i, ctypes.POINTER(_c_i), _c_p, _c_p]),
    'gnerf_band_mesh_workspace_bytes': (_c_i, [_c_i, _c_i, _c_i64, ctypes.POINTER(ctypes.c_size_t)]),
    'gnerf_band_mesh_count': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_f, ctypes.POINTER(_c_i), ctypes.POINTER(_c_i), ctypes.POINTER(_c_i), _c_i64, _c_p, _c_p, _c_p]),
    'gnerf_band_mesh_emit': (_c_i, [_c_p, _c_p, _c_i, _c_i, _c_f, ctypes.POINTER(_c_i), ctypes.POINTER(_c_i), ctypes.POINTER(_c_i), _c_i64, _c_p, _c_p, _c_p, _c_p]),
}
# exports added WITHOUT a new ABI version: a library of the same version built before them (a variant build behind GNERF_HIP_LIB) loads, and
# what needs them asks modconv_backward_available() / render_ray_grad_available() / decoder_pack_available() / resize_aa_available() /
# raster_available() / mesh_clean_available() / mesh_simplify_available() / project_to_level_available() / mesh_flip_guard_available() /
# scatter_plane_rows_available() / texture_available() / query_lattice_available() / band_available()
OPTIONAL_SYMBOLS = frozenset(n for n in SIGNATURES if n.startswith(('gnerf_project_points_to_level', 'gnerf_modconv_backward_','gnerf_scale_channels_backward', 'gnerf_modconv_epilogue_backward',
                                                                    'gnerf_render_backward_rays', 'gnerf_render_scatter_rows', 'gnerf_render_decoder_pack_bytes',
                                                                    'gnerf_render_pack_decoder', 'gnerf_render_forward_packed', 'gnerf_resize_aa_', 'gnerf_raster_', 'gnerf_mesh_', 'gnerf_query_lattice', 'gnerf_band_')))


def profiled(name):
    """Decorator: the call runs inside torch.autograd.profiler.record_function(name) WHILE a profiler is collecting (Kineto,
    or emit_nvtx -> roctx ranges that rocprofv3 --marker-trace shows), and as a plain call otherwise -- a record_function entered with
    no profiler attached still costs microseconds of host time per call, which an orbit frame of ~190 launches cannot afford.
    The reference opens the same ranges with misc.profiled_function (misc.py:102-107; conv2d_resample.py:47, bias_act.py:92, ...)."""
    import functools

    def deco(fn):
        @functools.wraps(fn)
        def wrapper(*args, **kwargs):
            if torch.autograd._profiler_enabled():
                with torch.autograd.profiler.record_function(name):
                    return fn(*args, **kwargs)
            return fn(*args, **kwargs)
        return wrapper
    return deco


def load():
    """Load the library once.  Raises RuntimeError (never falls back) if it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(f'{LIB_PATH} is missing: build it with g-nerf_amd/csrc/build.sh '
                           f'(or python -c "import __graft_entry__ as g; g.build()"). There is no fallback path.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None) if name in OPTIONAL_SYMBOLS else getattr(lib, name)
        if fn is None:
            continue
        fn.restype = res
        fn.argtypes = args
    if lib.gnerf_abi_version() != ABI_VERSION:
        raise RuntimeError(f'libgnerf_hip.so ABI version {lib.gnerf_abi_version()} != {ABI_VERSION}: rebuild it (g-nerf_amd/csrc/build.sh)')
    _lib = lib
    return lib


def is_available():
    return os.path.isfile(LIB_PATH)


# The thin PyTorch-ROCm C++ extension over the same C ABI (csrc/torch_binding.cpp -> gnerf_torch_ext.so): pybind entry points
# with the reference plugins' exact signatures (bias_act.cpp:36, upfirdn2d.cpp:20, filtered_lrelu.cpp:20,217) plus
# render_forward.  It is the default binding of the public ops (custom_ops.get_plugin) because a call costs ~3 us of host
# time instead of ~11 through ctypes; GNERF_HIP_BINDING=ctypes forces the ctypes route, which stays complete and is what
# everything falls back to when the extension has not been built.  Either way the kernels are libgnerf_hip.so's.
EXT_PATH = os.path.join(_HERE, 'gnerf_torch_ext.so')
_ext = None


def ext():
    """The extension module, or None (not built, or GNERF_HIP_BINDING=ctypes).  GNERF_HIP_BINDING=ext makes absence an error."""
    global _ext
    if _ext is None:
        want = os.environ.get('GNERF_HIP_BINDING', '')
        if want == 'ctypes' or os.environ.get('GNERF_HIP_LIB'):          # variant builds of the library are ctypes-only
            _ext = False
        elif not os.path.isfile(EXT_PATH):
            if want == 'ext':
                raise RuntimeError(f'{EXT_PATH} is missing: build it with g-nerf_amd/csrc/build.sh')
            _ext = False
        else:
            load()
            import importlib.util
            spec = importlib.util.spec_from_file_location('gnerf_torch_ext', EXT_PATH)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            # abi_version() is the header version compiled INTO the extension (its struct layouts); load() has already held the
            # library to ABI_VERSION, and library_abi_version() is what the extension's own link resolved to
            if mod.abi_version() != ABI_VERSION or mod.library_abi_version() != ABI_VERSION:
                raise RuntimeError(f'gnerf_torch_ext.so was built against ABI {mod.abi_version()} (library it links: '
                                   f'{mod.library_abi_version()}) != {ABI_VERSION}: rebuild (csrc/build.sh)')
            _ext = mod
    return _ext or None


E_UNSUPPORTED = -3      # GNERF_E_UNSUPPORTED (include/gnerf_hip.h)


class NativeError(RuntimeError):
    """A call into the library returned an error; `code` is the C ABI's return value (GNERF_E_*)."""

    def __init__(self, message, code):
        super().__init__(message)
        self.code = int(code)


def _check(code, what):
    if code != 0:
        msg = load().gnerf_last_error().decode('utf-8', 'replace')
        raise NativeError(f'{what} failed ({code}): {msg}', code)


# The three helpers below sit on every call; written for low host overhead (the public ops are called ~45 times per
# generator forward): raw stream handle without building a Stream object, plain ints for pointers (argtypes are
# c_void_p), and no device context switch when the tensor already lives on the current device.
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream(t):
    if _raw_stream is not None:
        return _raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


class _NoSwitch:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on_device(device):
    """Context that makes `device` current for the launch; free when it already is."""
    if device.index is None or device.index == torch.cuda.current_device():
        return _NO_SWITCH
    return torch.cuda.device(device)


def _launch(name, t, *args):
    """Call the export `name` with `args` and t's current stream as its last argument, on t's device; raises NativeError on failure."""
    with _on_device(t.device):
        code = getattr(load(), name)(*args, _stream(t))
    _check(code, name)


def _strides(t):
    return (ctypes.c_int64 * t.ndim)(*t.stride())


def _clamp_arg(clamp):
    """The ABI's clamp argument: negative means none."""
    return float(-1 if clamp is None else clamp)


def _act_code(act, what='gnerf_hip'):
    """The ABI's activation code of the two activations the fused epilogues take."""
    if act not in ('linear', 'lrelu'):
        raise RuntimeError(f'{what}: act must be linear or lrelu')
    return 3 if act == 'lrelu' else 1


def _is_dense(t):
    """Non-overlapping and dense in SOME dimension order (what ATen's is_non_overlapping_and_dense checks)."""
    if t.is_contiguous():
        return True
    expected = 1
    for stride, size in sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1):
        if stride != expected:
            return False
        expected *= size
    return True


def _same_layout(a, b):
    """has_same_layout of the reference's bias_act.cpp:18-29: strides are compared only where the size is >= 2 (a size-1
    dimension's stride is arbitrary, e.g. after .contiguous() on [N,C,1,1])."""
    return all(sa == sb for sz, sa, sb in zip(a.shape, a.stride(), b.stride()) if sz >= 2)


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and t.device.type != 'cuda':
            raise RuntimeError('gnerf_hip: tensor is not on a GPU device')



def is_channels_last(x):
    """True for a 4-D tensor whose MEMORY is [N,H,W,C] with C > 1 (and not also NCHW-contiguous)."""
    return x.ndim == 4 and x.shape[1] > 1 and x.stride(1) == 1 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()


def _activation_layout(x, what):
    """'nchw' or 'nhwc' for a dense float16/float32 4-D activation tensor; anything else raises."""
    if x.ndim != 4 or x.dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f'{what}: x must be a 4-D float16/float32 tensor')
    if x.is_contiguous():
        return 'nchw'
    if is_channels_last(x):
        return 'nhwc'
    raise RuntimeError(f'{what}: x must be contiguous (NCHW) or channels_last')


_workspaces = {}                   # (device index, stream) -> the render workspace
_split_overflow = {}               # device -> conv3x3.split_overflow_flag
_device_geometry = {}              # device index -> planes.torch_rand_geometry's (CUs, threads per CU)
_filter_tap_cache = {}             # planes._filter_taps
_decoder_packs = {}                # render._decoder_pack's cache: key -> (pack, decoder tensors), least recently used first
_decoder_seen = {}                 # ... and the keys it has seen once: key -> decoder tensors, oldest first
_EMPTY = torch.empty([0])        # "absent tensor" for the C++ binding, as the reference's _null_tensor (bias_act.py:38)


def _workspace(device):
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None:
        ws = torch.zeros([max(int(load().gnerf_render_workspace_bytes()), 16)], dtype=torch.uint8, device=device)     # zeroed once; calls leave it zeroed
        _workspaces[key] = ws
    return ws


def clock_under_load(run, microseconds=3000.0, device=None):
    """MHz the shader clock holds while `run()` (which enqueues work on the current stream for at least `microseconds`) executes: a
    one-wave sampler on a side stream (gnerf_clock_sample) reads the shader-cycle counter against the 100 MHz reference meanwhile."""
    dev = device if device is not None else torch.device('cuda', torch.cuda.current_device())
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    run()                                                   # the load is already running when the sampler starts (it does not wait for it)
    with _on_device(dev):
        _check(load().gnerf_clock_sample(out.data_ptr(), float(microseconds), ctypes.c_void_p(side.cuda_stream)), 'gnerf_clock_sample')
    run()
    torch.cuda.synchronize(dev)
    cyc, ticks = [int(v) for v in out.tolist()]
    return 100.0 * cyc / ticks if ticks else None
