"""ctypes binding of libgnerf_hip.so (C ABI in include/gnerf_hip.h).

This package is the only place that touches the native library.  PyTorch is used for what it is
good at here -- device memory, the current HIP stream, dtypes -- and nothing else: every
function below hands raw device pointers to a hand-written gfx950 kernel.

There is NO fallback: if the library is missing or a call fails, a RuntimeError is raised (a failed native call: NativeError, which
carries the C ABI's return code).

One module per native family, along the lines of csrc/: _native (the library, its ABI, loading, what every wrapper shares, and ALL
mutable state), plugins, planes, modconv, conv3x3, render, mesh, ssim, resize, raster.  Everything public is re-exported here.
"""

import ctypes  # noqa: F401  (ctypes, os and torch have always been attributes of the package)
import os  # noqa: F401

import torch  # noqa: F401

from . import _native, conv3x3, mesh, modconv, planes, plugins, raster, render, resize, ssim  # noqa: F401
from ._native import (ABI_VERSION, DEBUG_SLOTS, E_UNSUPPORTED, EXT_PATH, F16, F32, F64, LIB_PATH, MAX_SAMPLES, MLP_MODES, OPTIONAL_SYMBOLS, SIGNATURES,  # noqa: F401
                      NativeError, RenderGrads, RenderParams, clock_under_load, ext, is_available, is_channels_last, load, profiled,
                      _activation_layout, _check, _stream, _workspace, _workspaces)
from .plugins import bias_act, filtered_lrelu, filtered_lrelu_act_, grid_sample_2d, grid_sample_2d_backward, grid_sample_supported, upfirdn2d  # noqa: F401
from .planes import (TorchPhiloxPlan, commit_philox_plan, make_rays, make_rays_and_draws, planes_absmax, planes_from_nhwc, planes_to_nhwc,  # noqa: F401
                     to_uint8_nhwc, torch_philox_plan, torch_rand, torch_rand_geometry, upsample2x_add_nhwc)
from .modconv import (TORGB_CHANNELS, blur_epilogue_channels_last, modconv_backward_available, modconv_epilogue, modconv_epilogue_backward,  # noqa: F401
                      modulate_weights, normalise_styles, scale_channels, scale_channels_backward, torgb_channels_last, torgb_weights)
from .conv3x3 import (conv3x3_epilogue, conv3x3_epilogue_supported, conv3x3_epilogue_torgb, conv3x3_epilogue_torgb_supported,  # noqa: F401
                      conv3x3_f32x3_epilogue, conv3x3_f32x3_supported, conv_transpose3x3_s2, conv_transpose3x3_s2_f32x3,
                      conv_transpose3x3_s2_f32x3_supported, conv_transpose3x3_s2_supported, pack_conv3x3_weights, pack_conv3x3_weights_f32x3,
                      pack_conv_transpose3x3_weights, pack_conv_transpose3x3_weights_f32x3, split_f16x3, split_overflow_flag)
from .render import (decoder_pack_available, last_mlp_choice, pack_decoder, planes_layout, query_points, query_points_backward, query_points_grad, render_backward,  # noqa: F401
                     render_forward, render_generated_supported, render_ray_grad_available, render_ray_grad_refusal, render_ray_grad_supported, _render_params,
                     project_points_to_level, project_to_level_available, _project_points_to_level_ctypes,
                     scatter_plane_rows, scatter_plane_rows_available,
                     query_lattice, query_lattice_available, _query_lattice_ctypes)
from .mesh import (MESH_SMOOTH_MAX_FACES, marching_cubes, mesh_clean_available, mesh_compact, mesh_components, mesh_smooth, mesh_workspace_bytes,  # noqa: F401
                   mesh_simplify, mesh_simplify_available, mesh_simplify_count, mesh_simplify_workspace_bytes,
                   mesh_flip_guard, mesh_flip_guard_available, _mesh_flip_guard_ctypes,
                   _marching_cubes_ctypes, _mesh_compact_ctypes, _mesh_components_ctypes, _mesh_simplify_ctypes, _mesh_smooth_ctypes)
from .mesh import (BAND_BRICKS, BandVolume, band_available, band_fill, band_grow, band_points_count, band_points_emit, band_seed,  # noqa: F401
                   band_workspace_bytes, band_marching_cubes, band_mesh_available, band_mesh_workspace_bytes)
from .ssim import SSIM_MAX_WIN, ssim_backward, ssim_forward  # noqa: F401
from .resize import (RESIZE_MAX_TAPS, RESIZE_MODES, resize_aa_available, resize_aa_backward, resize_aa_forward, resize_aa_refusal,  # noqa: F401
                     resize_aa_supported)
from .raster import (RASTER_CULL, RASTER_MAX_SIZE, RASTER_OUTPUTS, RASTER_SHADING, RASTER_SMALL_PIXELS, raster_available, raster_workspace_bytes, rasterize,  # noqa: F401
                     resolve, shading_vector, _rasterize_ctypes, _resolve_ctypes)
from .raster import BAKE_MAX_GUARD, BAKE_MAX_POWER, BAKE_OUTPUTS, BAKE_RULES, bake_available, bake_colors, _bake_colors_ctypes  # noqa: F401
from .raster import (ATLAS_MAX_PATCH, ATLAS_MAX_SIZE, ATLAS_MIN_PATCH, TEXTURE_OUTPUTS, atlas_layout, bake_texture, resolve_textured, texture_available,  # noqa: F401
                     _bake_texture_ctypes, _resolve_textured_ctypes)
