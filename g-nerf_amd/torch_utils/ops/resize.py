"""Antialiased resize: interpolate_aa(x, ...) = F.interpolate(x, ..., align_corners=False, antialias=True) for mode 'bilinear' / 'bicubic'
(what superresolution.py:290-293 and training_loop.py's ssim_resize call).

Definition (ATen's, per axis; include/gnerf_hip.h states it in full): scale = in / out, or 1 / scale_factor when a scale factor was given and
is not recomputed; a triangle (bilinear) or Keys cubic (bicubic) filter, stretched by the scale when it is above 1, over the input pixels
within its support around scale * (i + 0.5), normalised to sum 1; y = W_y x W_x^T.

Routing: CPU tensors take the PyTorch op; GPU tensors take the gfx950 kernel (csrc/resize.hip) through a
torch.autograd.Function -- except the calls the kernel does not cover (a band over its limit: scale above 32 (bilinear) / 16 (bicubic) or
below 1/32; a dtype other than float16 / float32; an input that is not 4-D), which take the PyTorch op with one RuntimeWarning per reason and
process.  GNERF_RESIZE_AA=0 sends everything to the PyTorch op.
The operator is linear: the Function's backward is the same Function with the transposed flag flipped, so it is differentiable to any order.
"""

import functools
import math
import os
import warnings

import torch
import torch.nn.functional as F


def output_size_and_scales(in_size, size=None, scale_factor=None, recompute_scale_factor=None):
    """F.interpolate's rules for a 2-D resize: -> ((out_h, out_w), (scale_h, scale_w)), a scale being the in / out ratio the resampling is
    to use (1 / scale_factor), or None where it is the ratio of the sizes."""
    dim = len(in_size)
    if size is not None and scale_factor is not None:
        raise ValueError('only one of size or scale_factor should be defined')
    if size is not None:
        if recompute_scale_factor:
            raise ValueError('recompute_scale_factor is not meaningful with an explicit size.')
        if isinstance(size, (list, tuple)):
            if len(size) != dim:
                raise ValueError(f'Input and output must have the same number of spatial dimensions, but got input with spatial dimensions of '
                                 f'{list(in_size)} and output size of {size}.')
            return tuple(int(s) for s in size), (None,) * dim
        return (int(size),) * dim, (None,) * dim
    if scale_factor is None:
        raise ValueError('either size or scale_factor should be defined')
    if isinstance(scale_factor, (list, tuple)):
        if len(scale_factor) != dim:
            raise ValueError(f'Input and scale_factor must have the same number of spatial dimensions, but got input with spatial dimensions of '
                             f'{list(in_size)} and scale_factor of shape {scale_factor}.')
        factors = [float(s) for s in scale_factor]
    else:
        factors = [float(scale_factor)] * dim
    out = tuple(int(math.floor(float(s) * f)) for s, f in zip(in_size, factors))
    if recompute_scale_factor:
        return out, (None,) * dim
    return out, tuple(1.0 / f for f in factors)


class _ResizeAAKernel(torch.autograd.Function):
    """W_y x W_x^T (transposed: W_y^T x W_x) on the gfx950 kernel.  Nothing is saved: the operator does not depend on x."""

    @staticmethod
    def forward(ctx, x, in_size, out_size, mode, scales, transposed):
        import gnerf_hip
        ctx.consts = (in_size, out_size, mode, scales, transposed)
        if transposed:
            return gnerf_hip.resize_aa_backward(x, in_size, mode, scales)
        return gnerf_hip.resize_aa_forward(x, out_size, mode, scales)

    @staticmethod
    def backward(ctx, g):
        in_size, out_size, mode, scales, transposed = ctx.consts
        return _ResizeAAKernel.apply(g, in_size, out_size, mode, scales, not transposed), None, None, None, None, None


_warned_fallbacks = set()


def _warn_gpu_fallback(reason):
    if reason not in _warned_fallbacks:
        _warned_fallbacks.add(reason)
        warnings.warn(f'interpolate_aa: GPU tensor, but {reason}: running the PyTorch op, not the HIP kernel', RuntimeWarning, stacklevel=3)


@functools.lru_cache(maxsize=256)
def _plan(shape, dtype, size, scale_factor, mode, recompute_scale_factor):
    """What a call on a GPU tensor comes to (a pure function of its arguments, so it is worked out once per distinct call):
    -> (out_size, scales, why the kernel does not cover it -- one string per REASON, not per shape -- or None)."""
    import gnerf_hip
    if len(shape) != 4:
        return None, None, 'the input is not 4-D'
    out_size, scales = output_size_and_scales(shape[2:], size, scale_factor, recompute_scale_factor)
    if 0 in shape or min(out_size) < 1:
        return out_size, scales, ''                                   # the PyTorch op's own error, no warning
    if dtype not in (torch.float32, torch.float16):
        return out_size, scales, f'the dtype is {dtype} (the kernel takes float16 and float32)'
    if not gnerf_hip.resize_aa_supported(shape, out_size, mode, scales):
        return out_size, scales, "the resampling band is over the kernel's limit (65 taps per output, 65 outputs per input) or a tensor has 2^31 elements"
    return out_size, scales, None


def kernel_enabled():
    return os.environ.get('GNERF_RESIZE_AA', '1') != '0'


def _on_gpu(x):
    return x.device.type == 'cuda'


def interpolate_aa(x, size=None, scale_factor=None, mode='bilinear', recompute_scale_factor=None):
    """F.interpolate(x, size, scale_factor, mode, align_corners=False, recompute_scale_factor, antialias=True), by this project's routing rule."""
    if mode not in ('bilinear', 'bicubic'):
        raise ValueError(f"interpolate_aa: mode must be 'bilinear' or 'bicubic' (the antialiased modes), got {mode!r}")

    def torch_op():
        return F.interpolate(x, size=size, scale_factor=scale_factor, mode=mode, align_corners=False, recompute_scale_factor=recompute_scale_factor,
                             antialias=True)
    if not _on_gpu(x) or not kernel_enabled():
        return torch_op()
    out_size, scales, reason = _plan(tuple(x.shape), x.dtype, tuple(size) if isinstance(size, list) else size,
                                     tuple(scale_factor) if isinstance(scale_factor, list) else scale_factor, mode, recompute_scale_factor)
    if reason is not None:
        if reason:
            _warn_gpu_fallback(reason)
        return torch_op()
    return _ResizeAAKernel.apply(x, tuple(x.shape[2:]), out_size, mode, scales, False)
