"""The antialiased resize, forward and transposed (csrc/resize.hip)."""

import math

import torch

from . import _native
from ._native import _DTYPE_CODE, _check, _launch, _on_device, _ptr, _require_cuda, _strides, is_channels_last, load, profiled


RESIZE_MAX_TAPS = 65
RESIZE_MODES = {'bilinear': 0, 'bicubic': 1}


def resize_aa_available():
    """False for a library of this ABI version built before the resize exports (a variant build behind GNERF_HIP_LIB)."""
    return hasattr(load(), 'gnerf_resize_aa_forward')


def _axis_refusal(name, size_in, size_out, scale, mode):
    scale = float(scale) if scale is not None and scale > 0 else size_in / size_out
    half = 2.0 if mode == 'bicubic' else 1.0
    support = half * scale if scale >= 1.0 else half
    if not math.isfinite(scale) or min(math.floor(2.0 * support) + 1, size_in) > RESIZE_MAX_TAPS:
        return f'{name} {size_in} -> {size_out} needs more than {RESIZE_MAX_TAPS} taps per output'
    if min(math.floor(2.0 * support / scale) + 1, size_out) > RESIZE_MAX_TAPS:
        return f'{name} {size_in} -> {size_out}: more than {RESIZE_MAX_TAPS} outputs touch one input'
    return None


def resize_aa_refusal(shape, out_size, mode='bilinear', scales=(None, None)):
    """Why gnerf_resize_aa_* returns GNERF_E_UNSUPPORTED for an [N, C, H, W] `shape` resized to `out_size` (the rule of csrc/resize.hip's
    make_axis), or None.  scales: per axis, the scale the kernel is to use (in / out where None or <= 0)."""
    if mode not in RESIZE_MODES:
        return f'mode {mode!r}'
    n, c, h, w = (int(v) for v in shape)
    oh, ow = (int(v) for v in out_size)
    if n * c * h * w >= 2 ** 31 or n * c * oh * ow >= 2 ** 31:
        return 'a tensor of 2^31 elements or more'
    return _axis_refusal('height', h, oh, scales[0], mode) or _axis_refusal('width', w, ow, scales[1], mode)


def resize_aa_supported(shape, out_size, mode='bilinear', scales=(None, None)):
    return resize_aa_refusal(shape, out_size, mode, scales) is None


def _resize(name, x, in_size, out_size, mode, scales, transposed):
    _require_cuda(x)
    if x.ndim != 4:
        raise ValueError(f'{name}: x must be [N, C, H, W], got {tuple(x.shape)}')
    if x.dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f'{name}: the kernel takes float32 and float16 images, not {x.dtype}')
    if mode not in RESIZE_MODES:
        raise ValueError(f'{name}: mode must be bilinear or bicubic, got {mode!r}')
    (in_h, in_w), (out_h, out_w) = (int(v) for v in in_size), (int(v) for v in out_size)
    src, dst = ((out_h, out_w), (in_h, in_w)) if transposed else ((in_h, in_w), (out_h, out_w))
    if tuple(x.shape[2:]) != src:
        raise ValueError(f'{name}: x is {tuple(x.shape[2:])}, expected {src}')
    if x.numel() == 0 or min(dst) < 1:
        raise ValueError(f'{name}: empty image {tuple(x.shape)} -> {dst}')
    sh, sw = (float(s) if s is not None and s > 0 else 0.0 for s in scales)
    x = x.detach()
    e = _native.ext()
    if e is not None:
        with _on_device(x.device):
            y, code = e.resize_aa(x, in_h, in_w, out_h, out_w, RESIZE_MODES[mode], sh, sw, bool(transposed))
        _check(code, f'gnerf_{name}')
        return y
    y = torch.empty([x.shape[0], x.shape[1], *dst], dtype=x.dtype, device=x.device,
                    memory_format=torch.channels_last if is_channels_last(x) else torch.contiguous_format)
    _launch(f'gnerf_{name}', x, _ptr(x), _ptr(y), _DTYPE_CODE[x.dtype], x.shape[0], x.shape[1], in_h, in_w, out_h, out_w, _strides(x), _strides(y),
            RESIZE_MODES[mode], sh, sw)
    return y


@profiled('gnerf_hip::resize_aa_forward')
def resize_aa_forward(x, out_size, mode='bilinear', scales=(None, None)):
    """F.interpolate(x, mode=mode, align_corners=False, antialias=True) of x [N, C, H, W] (CUDA, float32 or float16, any strides) to
    out_size = (out_h, out_w), in x's dtype and memory format.  scales: per axis, 1 / scale_factor where the caller's scale factor is to be
    used as given, else None (in / out).  Definition and guarantees: include/gnerf_hip.h, gnerf_resize_aa_*.  A call the kernel does not
    cover raises NativeError with code E_UNSUPPORTED (resize_aa_supported tells beforehand).  No host synchronisation: capturable in a graph."""
    return _resize('resize_aa_forward', x, x.shape[2:], out_size, mode, scales, False)


@profiled('gnerf_hip::resize_aa_backward')
def resize_aa_backward(dy, in_size, mode='bilinear', scales=(None, None)):
    """The transpose of resize_aa_forward: dy [N, C, out_h, out_w] -> dx [N, C, *in_size], the gradient w.r.t. the forward's input.  `scales`
    are the forward's."""
    return _resize('resize_aa_backward', dy, in_size, dy.shape[2:], mode, scales, True)
