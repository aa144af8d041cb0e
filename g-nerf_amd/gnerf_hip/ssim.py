"""The fused SSIM loss, forward and backward (csrc/ssim.hip)."""

import ctypes

import torch

from . import _native
from ._native import _DTYPE_CODE, _c_f, _check, _launch, _on_device, _ptr, _require_cuda, _strides, load, profiled


SSIM_MAX_WIN = 11


def _ssim_images(x, y, window, what):
    _require_cuda(x, y)
    if x.ndim != 4 or x.shape != y.shape or x.dtype != y.dtype or x.device != y.device:
        raise ValueError(f'{what}: X and Y must be [N, C, H, W] tensors of one shape, dtype and device')
    if x.dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f'{what}: the kernel takes float32 and float16 images, not {x.dtype}')
    window = [float(v) for v in window]
    if len(window) % 2 != 1 or len(window) > SSIM_MAX_WIN:
        raise ValueError(f'{what}: the window must have an odd length of at most {SSIM_MAX_WIN}, got {len(window)}')
    if min(x.shape[2:]) < len(window):
        raise ValueError(f'{what}: a {x.shape[2]} x {x.shape[3]} image is smaller than the window of {len(window)}')
    return window


def _ssim_forward_ctypes(x, y, window, C1, C2):
    n, c, h, w = x.shape
    nbytes = ctypes.c_size_t()
    _check(load().gnerf_ssim_workspace_bytes(n, c, h, w, len(window), ctypes.byref(nbytes)), 'gnerf_ssim_workspace_bytes')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)
    out = torch.empty([2, n, c], dtype=torch.float32, device=x.device)
    _launch('gnerf_ssim_forward', x, _ptr(x), _ptr(y), _DTYPE_CODE[x.dtype], n, c, h, w, _strides(x), _strides(y), (_c_f * len(window))(*window),
            len(window), float(C1), float(C2), _ptr(ws), _ptr(out[0]), _ptr(out[1]))
    return out[0], out[1]


def _ssim_backward_ctypes(x, y, window, C1, C2, g_ssim, g_cs, need_dx, need_dy):
    n, c, h, w = x.shape
    dx = torch.empty_like(x) if need_dx else None
    dy = torch.empty_like(y) if need_dy else None
    _launch('gnerf_ssim_backward', x, _ptr(x), _ptr(y), _DTYPE_CODE[x.dtype], n, c, h, w, _strides(x), _strides(y), (_c_f * len(window))(*window),
            len(window), float(C1), float(C2), _ptr(g_ssim), _ptr(g_cs), _ptr(dx), None if dx is None else _strides(dx),
            _ptr(dy), None if dy is None else _strides(dy))
    return dx, dy


@profiled('gnerf_hip::ssim_forward')
def ssim_forward(x, y, window, C1, C2):
    """Per-channel SSIM and contrast-structure means of X, Y [N, C, H, W] (CUDA, float32 or float16, any strides) under the 1-D `window`
    (a sequence of an odd number <= 11 of floats) -> (ssim [N, C], cs [N, C]) float32.  Definition and guarantees: include/gnerf_hip.h,
    gnerf_ssim_*.  No host synchronisation: capturable in a graph."""
    window = _ssim_images(x, y, window, 'ssim_forward')
    x, y = x.detach(), y.detach()
    e = _native.ext()
    if e is not None:
        with _on_device(x.device):
            return e.ssim_forward(x, y, window, float(C1), float(C2))
    return _ssim_forward_ctypes(x, y, window, C1, C2)


@profiled('gnerf_hip::ssim_backward')
def ssim_backward(x, y, window, C1, C2, g_ssim, g_cs, need_dx=True, need_dy=True):
    """Gradients of sum(g_ssim * ssim + g_cs * cs) of ssim_forward w.r.t. X and Y -> (dX, dY) in X's dtype and layout (None where not
    asked for).  g_ssim / g_cs: [N, C] tensors or None (= zeros; not both)."""
    window = _ssim_images(x, y, window, 'ssim_backward')
    if not (need_dx or need_dy):
        return None, None
    if g_ssim is None and g_cs is None:
        raise ValueError('ssim_backward: g_ssim and g_cs are both None')
    n, c = x.shape[:2]

    def upstream(g):
        if g is None:
            return None
        _require_cuda(g)
        if tuple(g.shape) != (n, c):
            raise ValueError(f'ssim_backward: an upstream gradient of shape {tuple(g.shape)}, expected {(n, c)}')
        return g.detach().to(torch.float32).contiguous()
    g_ssim, g_cs = upstream(g_ssim), upstream(g_cs)
    x, y = x.detach(), y.detach()
    e = _native.ext()
    if e is not None:
        with _on_device(x.device):
            dx, dy = e.ssim_backward(x, y, window, float(C1), float(C2), g_ssim, g_cs, bool(need_dx), bool(need_dy))
        return (dx if need_dx else None), (dy if need_dy else None)
    return _ssim_backward_ctypes(x, y, window, C1, C2, g_ssim, g_cs, need_dx, need_dy)
