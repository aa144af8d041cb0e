"""The reference's four plugins on the ctypes route: bias_act, upfirdn2d, filtered_lrelu and the grid sampler."""

import torch

from ._native import E_UNSUPPORTED, _DTYPE_CODE, _check, _is_dense, _launch, _on_device, _ptr, _require_cuda, _same_layout, _stream, _strides, load, profiled


@profiled('gnerf_hip::bias_act')
def bias_act(x, b, xref, yref, dy, grad, dim, act, alpha, gain, clamp):
    """Same contract as bias_act_plugin.bias_act (reference bias_act.cpp:36): absent tensors are
    empty tensors (numel 0) or None; returns a new tensor laid out like x."""
    def opt(t):
        return None if t is None or t.numel() == 0 else t
    b, xref, yref, dy = opt(b), opt(xref), opt(yref), opt(dy)
    _require_cuda(x, b, xref, yref, dy)
    if x.dtype not in _DTYPE_CODE:
        raise RuntimeError(f'bias_act: unsupported dtype {x.dtype}')
    if not _is_dense(x):
        raise RuntimeError('bias_act: x must be non-overlapping and dense')
    for name, t in (('xref', xref), ('yref', yref), ('dy', dy)):
        if t is not None and (t.shape != x.shape or t.dtype != x.dtype or not _same_layout(t, x)):
            raise RuntimeError(f'bias_act: {name} must have the same shape, dtype and layout as x')
    size_b, step_b = 0, 1
    if b is not None:
        if b.ndim != 1 or b.dtype != x.dtype or not b.is_contiguous():
            raise RuntimeError('bias_act: b must be a contiguous 1-D tensor of the same dtype as x')
        if not 0 <= dim < x.ndim or b.numel() != x.shape[dim]:
            raise RuntimeError('bias_act: b has the wrong number of elements or dim is out of bounds')
        size_b, step_b = b.numel(), x.stride(dim)
    y = torch.empty_like(x)
    _launch('gnerf_bias_act', x, _ptr(x), _ptr(b), _ptr(xref), _ptr(yref), _ptr(dy), _ptr(y), _DTYPE_CODE[x.dtype], x.numel(), size_b, step_b,
            int(grad), int(act), float(alpha), float(gain), float(clamp))
    return y


@profiled('gnerf_hip::upfirdn2d')
def upfirdn2d(x, f, upx, upy, downx, downy, padx0, padx1, pady0, pady1, flip, gain):
    """Same contract as upfirdn2d_plugin.upfirdn2d (reference upfirdn2d.cpp:20): x [N,C,H,W] in NCHW or
    channels_last, f float32 [fh,fw] on x's device; returns y in x's memory format."""
    _require_cuda(x, f)
    if x.ndim != 4 or f.ndim != 2 or f.dtype != torch.float32:
        raise RuntimeError('upfirdn2d: x must be rank 4 and f a rank-2 float32 tensor')
    if x.dtype not in _DTYPE_CODE:
        raise RuntimeError(f'upfirdn2d: unsupported dtype {x.dtype}')
    if x.numel() == 0 or f.numel() == 0:
        raise RuntimeError('upfirdn2d: x and f must not be empty')
    n, c, ih, iw = x.shape
    fh, fw = f.shape
    ow = (iw * upx + padx0 + padx1 - fw + downx) // downx
    oh = (ih * upy + pady0 + pady1 - fh + downy) // downy
    if ow < 1 or oh < 1:
        raise RuntimeError('upfirdn2d: output must be at least 1x1')
    mf = torch.channels_last if (x.stride(1) == 1 and c > 1) else torch.contiguous_format
    y = torch.empty([n, c, oh, ow], dtype=x.dtype, device=x.device, memory_format=mf)
    _launch('gnerf_upfirdn2d', x, _ptr(x), _ptr(f), _ptr(y), _DTYPE_CODE[x.dtype], n, c, ih, iw, _strides(x), fh, fw, _strides(f), oh, ow,
            _strides(y), upx, upy, downx, downy, padx0, pady0, 1 if flip else 0, float(gain))
    return y


@profiled('gnerf_hip::filtered_lrelu_act_')
def filtered_lrelu_act_(x, si, sx, sy, gain, slope, clamp, write_signs):
    """Same contract as filtered_lrelu_plugin.filtered_lrelu_act_ (reference filtered_lrelu.cpp:217):
    in-place on x; returns the sign tensor written (or an empty tensor)."""
    _require_cuda(x)
    if x.ndim != 4 or x.dtype not in _DTYPE_CODE:
        raise RuntimeError('filtered_lrelu_act_: x must be a rank-4 float tensor')
    n, c, h, w = x.shape
    read_signs = si is not None and si.numel() > 0
    so = torch.empty([0], dtype=torch.uint8, device=x.device)
    s_h = s_w = 0
    mode = 0
    s = None
    if read_signs:
        _require_cuda(si)
        if si.dtype != torch.uint8 or si.ndim != 4 or not si.is_contiguous():
            raise RuntimeError('filtered_lrelu_act_: si must be a contiguous rank-4 uint8 tensor')
        s, s_h, s_w, mode = si, si.shape[2], si.shape[3] * 4, 2
    elif write_signs:
        s_w = (w + 15) & ~15
        s_h = h
        so = torch.empty([n, c, s_h, s_w // 4], dtype=torch.uint8, device=x.device)
        s, mode, sx, sy = so, 1, 0, 0
    _launch('gnerf_filtered_lrelu_act', x, _ptr(x), _ptr(s), _DTYPE_CODE[x.dtype], n, c, h, w, _strides(x), s_h, s_w, int(sx), int(sy), float(gain),
            float(slope), float(clamp), mode)
    return so


@profiled('gnerf_hip::filtered_lrelu')
def filtered_lrelu(x, fu, fd, b, si, up, down, px0, px1, py0, py1, sx, sy, gain, slope, clamp, flip_filters, write_signs):
    """Same contract as filtered_lrelu_plugin.filtered_lrelu (reference filtered_lrelu.cpp:20-213): returns
    (y, so, rc); rc = -1 with empty tensors means "no fused kernel for this configuration" and the caller runs the
    generic three-launch route (filtered_lrelu.py:225-231).  Anything else that goes wrong raises."""
    _require_cuda(x)
    if x.ndim != 4 or x.numel() == 0:
        raise RuntimeError('filtered_lrelu: x must be a non-empty rank-4 tensor')
    for f, name in ((fu, 'fu'), (fd, 'fd')):
        _require_cuda(f)
        if f.dtype != torch.float32 or f.ndim not in (1, 2) or f.numel() == 0:
            raise RuntimeError(f'filtered_lrelu: {name} must be a non-empty float32 tensor of rank 1 or 2')
    _require_cuda(b)
    if b.dtype != x.dtype or b.ndim != 1 or b.shape[0] != x.shape[1]:
        raise RuntimeError('filtered_lrelu: b must be a vector with one entry per channel of x, same dtype')
    if up < 1 or down < 1:
        raise RuntimeError('filtered_lrelu: up and down must be at least 1')
    none = (torch.empty([0], device=x.device), torch.empty([0], device=x.device), -1)
    if x.dtype not in (torch.float32, torch.float16):
        return none
    if (fu.ndim == 2 and tuple(fu.shape) != (1, 1)) or (fd.ndim == 2 and tuple(fd.shape) != (1, 1)):
        return none                                            # non-separable filters: generic route
    n, c, xh, xw = x.shape
    fut, fdt = fu.shape[-1] - 1, fd.shape[-1] - 1
    cw, chh = xw * up + (px0 + px1) - fut, xh * up + (py0 + py1) - fut
    if not (cw > fdt and chh > fdt):
        raise RuntimeError('filtered_lrelu: upsampled buffer must be at least the size of downsampling filter')
    yw, yh = (cw - fdt + (down - 1)) // down, (chh - fdt + (down - 1)) // down
    if yw < 1 or yh < 1:
        raise RuntimeError('filtered_lrelu: output must be at least 1x1')
    channels_last = x.stride(1) == 1 and c > 1
    y = torch.empty([n, c, yh, yw], dtype=x.dtype, device=x.device,
                    memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    read_signs = si is not None and si.numel() > 0
    so = torch.empty([0], dtype=torch.uint8, device=x.device)
    s, s_h, s_w, mode = None, 0, 0, 0
    if write_signs:
        s_h = yh * down - (down - 1) + fdt
        s_w = (yw * down - (down - 1) + fdt + 15) & ~15
        so = torch.empty([n, c, s_h, s_w >> 2], dtype=torch.uint8, device=x.device)
        s, mode = so, 1
    elif read_signs:
        _require_cuda(si)
        if si.dtype != torch.uint8 or si.ndim != 4 or not si.is_contiguous() or si.shape[0] != n or si.shape[1] != c:
            raise RuntimeError('filtered_lrelu: signs must be a contiguous uint8 [n, c, h, w/4] tensor matching x')
        s, s_h, s_w, mode = si, si.shape[2], si.shape[3] * 4, 2
    fu_c, fd_c, b_c = fu.contiguous(), fd.contiguous(), b.contiguous()
    with _on_device(x.device):
        code = load().gnerf_filtered_lrelu(_ptr(x), _ptr(fu_c), _ptr(fd_c), _ptr(b_c), _ptr(s), _ptr(y), _DTYPE_CODE[x.dtype],
                                           n, c, xh, xw, _strides(x), yh, yw, _strides(y),
                                           fu.shape[-1], fu.ndim, fd.shape[-1], fd.ndim, int(up), int(down), int(px0), int(py0),
                                           s_h, s_w, int(sx), int(sy), mode, float(gain), float(slope), float(clamp),
                                           1 if flip_filters else 0, _stream(x))
    if code == E_UNSUPPORTED:
        return none
    _check(code, 'gnerf_filtered_lrelu')
    return y, so, 0


def grid_sample_supported(image, grid):
    """True when the native sampler covers this call (GPU tensors, float16/float32 image, 4-D, positive strides)."""
    return (image.is_cuda and grid.is_cuda and image.ndim == 4 and grid.ndim == 4 and grid.shape[-1] == 2 and grid.shape[0] == image.shape[0]
            and image.dtype in (torch.float32, torch.float16) and image.numel() > 0 and grid.numel() > 0
            and image.stride(2) > 0 and image.stride(3) > 0)


@profiled('gnerf_hip::grid_sample_2d')
def grid_sample_2d(image, grid):
    """Bilinear, zero padding, align_corners=False (what grid_sample_gradfix.grid_sample evaluates, grid_sample_gradfix.py:45):
    image [N,C,H,W], grid [N,Ho,Wo,2] -> [N,C,Ho,Wo] in image's dtype."""
    _require_cuda(image, grid)
    n, c, h, w = image.shape
    ho, wo = grid.shape[1], grid.shape[2]
    g = grid.float().contiguous()
    out = torch.empty([n, c, ho, wo], dtype=image.dtype, device=image.device)
    _launch('gnerf_grid_sample_2d', image, _ptr(image), _ptr(g), _ptr(out), _DTYPE_CODE[image.dtype], n, c, h, w, _strides(image), ho, wo)
    return out


@profiled('gnerf_hip::grid_sample_2d_backward')
def grid_sample_2d_backward(grad_out, image, grid, need_image=True, need_grid=True):
    """The adjoint (aten::grid_sampler_2d_backward upstream, grid_sample_gradfix.py:62-77): returns (grad_image, grad_grid), each
    None when not requested; grad_image in image's dtype, grad_grid in grid's."""
    _require_cuda(grad_out, image, grid)
    n, c, h, w = image.shape
    ho, wo = grid.shape[1], grid.shape[2]
    g = grid.float().contiguous()
    go = grad_out.to(image.dtype).contiguous()
    gi = torch.zeros([n, c, h, w], dtype=torch.float32, device=image.device) if need_image else None
    gg = torch.zeros([n, ho, wo, 2], dtype=torch.float32, device=image.device) if need_grid else None
    _launch('gnerf_grid_sample_2d_backward', image, _ptr(go), _ptr(image), _ptr(g), _ptr(gi), _ptr(gg), _DTYPE_CODE[image.dtype], n, c, h, w,
            _strides(image), ho, wo)
    return (None if gi is None else gi.to(image.dtype)), (None if gg is None else gg.to(grid.dtype))
