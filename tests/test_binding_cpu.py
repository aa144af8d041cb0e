"""The gnerf_hip package after its split into modules: every name callers used is still an attribute of the package, a failed native
call raises NativeError with the C ABI's return code, and the small argument helpers encode what the ABI expects."""

import pytest

import gnerf_hip
from gnerf_hip import _native

# dir(gnerf_hip) without underscore names, as it was while the binding was one module; release_workspaces (a no-op without a caller) left
PUBLIC_NAMES = [
    'ABI_VERSION', 'DEBUG_SLOTS', 'EXT_PATH', 'E_UNSUPPORTED', 'F16', 'F32', 'F64', 'LIB_PATH', 'MAX_SAMPLES', 'MLP_MODES', 'OPTIONAL_SYMBOLS',
    'RenderGrads', 'RenderParams', 'SIGNATURES', 'SSIM_MAX_WIN', 'TORGB_CHANNELS', 'TorchPhiloxPlan', 'bias_act', 'blur_epilogue_channels_last',
    'clock_under_load', 'commit_philox_plan', 'conv3x3_epilogue', 'conv3x3_epilogue_supported', 'conv3x3_epilogue_torgb',
    'conv3x3_epilogue_torgb_supported', 'conv3x3_f32x3_epilogue', 'conv3x3_f32x3_supported', 'conv_transpose3x3_s2', 'conv_transpose3x3_s2_f32x3',
    'conv_transpose3x3_s2_f32x3_supported', 'conv_transpose3x3_s2_supported', 'ctypes', 'ext', 'filtered_lrelu', 'filtered_lrelu_act_',
    'grid_sample_2d', 'grid_sample_2d_backward', 'grid_sample_supported', 'is_available', 'is_channels_last', 'last_mlp_choice', 'load', 'make_rays',
    'make_rays_and_draws', 'marching_cubes', 'modconv_backward_available', 'modconv_epilogue', 'modconv_epilogue_backward', 'modulate_weights',
    'normalise_styles', 'os', 'pack_conv3x3_weights', 'pack_conv3x3_weights_f32x3', 'pack_conv_transpose3x3_weights',
    'pack_conv_transpose3x3_weights_f32x3', 'planes_absmax', 'planes_from_nhwc', 'planes_layout', 'planes_to_nhwc', 'profiled', 'query_points',
    'query_points_backward', 'render_backward', 'render_forward', 'render_generated_supported', 'scale_channels', 'scale_channels_backward',
    'split_f16x3', 'split_overflow_flag', 'ssim_backward', 'ssim_forward', 'to_uint8_nhwc', 'torch', 'torch_philox_plan', 'torch_rand',
    'torch_rand_geometry', 'torgb_channels_last', 'torgb_weights', 'upfirdn2d', 'upsample2x_add_nhwc']
PRIVATE_NAMES = ['_render_params', '_workspace', '_workspaces', '_check', '_stream', '_activation_layout', '_marching_cubes_ctypes']


def test_package_keeps_its_names():
    assert PUBLIC_NAMES == sorted(PUBLIC_NAMES)
    missing = [n for n in PUBLIC_NAMES + PRIVATE_NAMES + ['NativeError'] if not hasattr(gnerf_hip, n)]
    assert not missing, missing
    assert not hasattr(gnerf_hip, 'release_workspaces')
    assert gnerf_hip._workspaces is _native._workspaces          # the package hands out the state, it holds no copy of its own


def test_failed_call_raises_native_error_with_the_code(monkeypatch):
    class Lib:
        @staticmethod
        def gnerf_last_error():
            return b'msg'
    assert issubclass(gnerf_hip.NativeError, RuntimeError)
    monkeypatch.setattr(_native, '_lib', Lib())
    _native._check(0, 'x')
    with pytest.raises(gnerf_hip.NativeError) as info:
        _native._check(-3, 'x')
    assert info.value.code == -3 == gnerf_hip.E_UNSUPPORTED
    assert str(info.value) == 'x failed (-3): msg'


def test_argument_helpers():
    assert _native._clamp_arg(None) == -1.0 and isinstance(_native._clamp_arg(None), float)
    assert _native._clamp_arg(256) == 256.0
    assert _native._act_code('lrelu') == 3 and _native._act_code('linear') == 1
    with pytest.raises(RuntimeError, match='act must be linear or lrelu'):
        _native._act_code('relu')
    with pytest.raises(RuntimeError, match='^modconv_epilogue: act must be linear or lrelu$'):
        _native._act_code('relu', 'modconv_epilogue')
