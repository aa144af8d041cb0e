"""The surroundings of the modulated convolution (csrc/modconv.hip, modconv_backward.hip, torgb.hip, blur.hip): weight modulation, the
per-channel scale, the fused epilogue with its backward, ToRGB and the blur + epilogue pass."""

import ctypes

import torch

from . import _native
from ._native import (OPTIONAL_SYMBOLS, _DTYPE_CODE, _act_code, _activation_layout, _check, _clamp_arg, _launch, _ptr, _require_cuda, _same_layout,
                      is_available, is_channels_last, load, profiled)
from .conv3x3 import _f32_operand


@profiled('gnerf_hip::modulate_weights')
def modulate_weights(weight, styles, demodulate=True, out_dtype=torch.float32, want_weights=True, want_dcoefs=False, transposed=False,
                     channels_last=False):
    """Per-sample modulated (+ demodulated) convolution weights in one launch (networks_stylegan2.py:61-75), with the fp16
    pre-normalisation of :62-64 when out_dtype is float16 and demodulate.  weight [O,I,k,k], styles [N,I] float32.
    Returns (w, dcoefs): w [N,O,I,k,k] in out_dtype (or None), or -- transposed -- [N,I,O,k,k], the form conv_transpose2d takes;
    with channels_last the memory of every sample's 4-D weight is channels_last ([O,k,k,I] / [I,k,k,O]; the returned tensor is
    a strided view with the logical shape above).  dcoefs [N,O] float32 or None."""
    _require_cuda(weight, styles)
    w32, s32 = weight.detach().to(torch.float32).contiguous(), styles.detach().to(torch.float32).contiguous()
    o, i, kh, kw = w32.shape
    n = s32.shape[0]
    if s32.shape != (n, i) or out_dtype not in (torch.float32, torch.float16):
        raise RuntimeError('modulate_weights: styles must be [N, I] and out_dtype float32 or float16')
    out = view = None
    if want_weights:
        a, b = (i, o) if transposed else (o, i)
        if channels_last:
            out = torch.empty([n, a, kh, kw, b], dtype=out_dtype, device=w32.device)
            view = out.permute(0, 1, 4, 2, 3)
        else:
            out = view = torch.empty([n, a, b, kh, kw], dtype=out_dtype, device=w32.device)
    dco = torch.empty([n, o], dtype=torch.float32, device=w32.device) if (want_dcoefs and demodulate) else None
    prenorm = 1 if (out_dtype == torch.float16 and demodulate) else 0
    _launch('gnerf_modulate_weights', w32, _ptr(w32), _ptr(s32), _ptr(out), _DTYPE_CODE[out_dtype], _ptr(dco), n, o, i, kh * kw,
            1 if demodulate else 0, prenorm, (1 if transposed else 0) + (2 if channels_last else 0))
    return view, dco


@profiled('gnerf_hip::normalise_styles')
def normalise_styles(styles):
    """styles [N,I] / max|styles[n]| per row (networks_stylegan2.py:64)."""
    _require_cuda(styles)
    s32 = styles.detach().to(torch.float32).contiguous()
    out = torch.empty_like(s32)
    _launch('gnerf_normalise_styles', s32, _ptr(s32), _ptr(out), s32.shape[0], s32.shape[1])
    return out


@profiled('gnerf_hip::scale_channels')
def scale_channels(x, scale):
    """x [N,C,H,W] (NCHW contiguous or channels_last, float16/32) * scale [N,C] float32, the product formed in x's dtype
    (networks_stylegan2.py:77).  The result has x's memory format."""
    _require_cuda(x, scale)
    layout = _activation_layout(x, 'scale_channels')
    n, c, h, w = x.shape
    s32 = scale.detach().to(torch.float32).contiguous()
    if s32.numel() != n * c:
        raise RuntimeError('scale_channels: scale must have N*C elements')
    y = torch.empty_like(x)
    if layout == 'nhwc':
        _launch('gnerf_scale_channels_nhwc', x, _ptr(x), _ptr(s32), _ptr(y), _DTYPE_CODE[x.dtype], n, h * w, c)
    else:
        _launch('gnerf_scale_channels', x, _ptr(x), _ptr(s32), _ptr(y), _DTYPE_CODE[x.dtype], n * c, h * w)
    return y


@profiled('gnerf_hip::modconv_epilogue')
def modconv_epilogue(x, bias=None, scale=None, noise=None, round_noise=False, act='lrelu', alpha=0.2, gain=1.0, clamp=None, next_scale=None):
    """Everything after the modulated convolution in one pass (networks_stylegan2.py:79-83 / :96-97 then :331-333):
    t = x * scale[n,c] + noise (rounded to x's dtype; skipped when both are None), y = clamp(act(t + bias[c]) * gain).
    x [N,C,H,W] NCHW contiguous or channels_last, float16/32; scale [N,C] float32; noise float32 [H,W] or [N,1,H,W]; bias [C] (any
    float dtype).  next_scale [N,C] (channels_last only): y is additionally multiplied by it in x's dtype -- the next layer's
    `x * styles` folded into this pass.  The result has x's memory format."""
    _require_cuda(x, bias, scale, noise, next_scale)
    layout = _activation_layout(x, 'modconv_epilogue')
    act = _act_code(act, 'modconv_epilogue')
    n, c, h, w = x.shape
    s32 = None if scale is None else scale.detach().to(torch.float32).contiguous()
    nz = None if noise is None else noise.detach().to(torch.float32).contiguous()
    per_item = 0
    if nz is not None:
        if nz.numel() == n * h * w and n > 1:
            per_item = 1
        elif nz.numel() != h * w:
            raise RuntimeError('modconv_epilogue: noise must have H*W or N*H*W elements')
    b = None if bias is None else bias.detach().to(x.dtype).contiguous()
    if (s32 is not None and s32.numel() != n * c) or (b is not None and b.numel() != c):
        raise RuntimeError('modconv_epilogue: scale must have N*C and bias C elements')
    nx = None if next_scale is None else next_scale.detach().to(torch.float32).contiguous()
    if nx is not None and (layout != 'nhwc' or nx.numel() != n * c):
        raise RuntimeError('modconv_epilogue: next_scale needs a channels_last x and N*C elements')
    y = torch.empty_like(x)
    # the two exports differ in how they take the shape (and next_scale exists for channels_last only)
    name, shape, tail = ('gnerf_modconv_epilogue_nhwc', (n, h * w, c), (_ptr(nx),)) if layout == 'nhwc' else ('gnerf_modconv_epilogue', (n * c, h * w, c), ())
    _launch(name, x, _ptr(x), _ptr(y), _DTYPE_CODE[x.dtype], *shape, _ptr(s32), _ptr(nz), per_item, 1 if round_noise else 0, _ptr(b), act,
            float(alpha), float(gain), _clamp_arg(clamp), *tail)
    return y


def modconv_backward_available():
    """True when the loaded library exports the backward kernels of scale_channels / modconv_epilogue (found by symbol, not by version)."""
    if not is_available():
        return False
    lib = load()
    return all(hasattr(lib, name) for name in OPTIONAL_SYMBOLS)


def _modconv_backward_workspace(x, layout):
    n, c, h, w = x.shape
    nbytes = ctypes.c_size_t(0)
    _check(load().gnerf_modconv_backward_workspace_bytes(1 if layout == 'nhwc' else 0, _DTYPE_CODE[x.dtype], n, c, h * w, ctypes.byref(nbytes)),
           'gnerf_modconv_backward_workspace_bytes')
    return torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=x.device)


def _like_activation(g, x, what):
    """The incoming gradient `g` in x's dtype and memory format (autograd hands over whatever the consumer's backward produced)."""
    if g.shape != x.shape or g.dtype != x.dtype or g.device != x.device:
        raise RuntimeError(f'{what}: the gradient must match the activations in shape, dtype and device')
    return g if _same_layout(g, x) else g.contiguous(memory_format=torch.channels_last if is_channels_last(x) else torch.contiguous_format)


@profiled('gnerf_hip::scale_channels_backward')
def scale_channels_backward(dxs, x, scale, need_dx=True, need_dscale=True):
    """Backward of scale_channels(x, scale) for the incoming gradient dxs -> (dx like x, dscale float32 [N, C]); None where not asked for.
    dx = round(dxs * scale) in x's dtype, dscale = sum over the pixels of dxs * x in float32 (fixed order, no atomics)."""
    _require_cuda(dxs, x, scale)
    layout = _activation_layout(x, 'scale_channels_backward')
    dxs = _like_activation(dxs, x, 'scale_channels_backward')
    n, c, h, w = x.shape
    s32 = scale.detach().to(torch.float32).contiguous()
    if s32.numel() != n * c:
        raise RuntimeError('scale_channels_backward: scale must have N*C elements')
    e = _native.ext()
    if e is not None and hasattr(e, 'modconv_backward'):
        return e.modconv_backward(False, dxs, None, x, s32, 1, 0.0, 1.0, -1.0, bool(need_dx), bool(need_dscale), False, 0)[:2]
    dx = torch.empty_like(x) if need_dx else None
    dscale = torch.empty([n, c], dtype=torch.float32, device=x.device) if need_dscale else None
    ws = _modconv_backward_workspace(x, layout) if need_dscale else None
    name, shape = ('gnerf_scale_channels_backward_nhwc', (n, h * w, c)) if layout == 'nhwc' else ('gnerf_scale_channels_backward', (n, c, h * w))
    _launch(name, x, _ptr(dxs), _ptr(x), _ptr(s32), _DTYPE_CODE[x.dtype], *shape, _ptr(dx), _ptr(dscale), _ptr(ws))
    return dx, dscale


@profiled('gnerf_hip::modconv_epilogue_backward')
def modconv_epilogue_backward(dy, y, x, scale=None, act='lrelu', alpha=0.2, gain=1.0, clamp=None, need_dx=True, need_dscale=False, need_dbias=False,
                              need_dnoise=None):
    """Backward of modconv_epilogue for the incoming gradient dy -> (dx like dy, dscale [N,C], dbias [C], dnoise), float32 sums, None where not
    asked for.  y: the forward's result (what the activation and clamp masks are read from; may be None for act='linear' without a clamp);
    x: the forward's input (needed for dscale only, else None); need_dnoise: None, 'plane' ([H,W]) or 'item' ([N,1,H,W]).
    Definition and guarantees: include/gnerf_hip.h, gnerf_modconv_epilogue_backward."""
    _require_cuda(dy, y, x, scale)
    layout = _activation_layout(dy, 'modconv_epilogue_backward')
    act_code = _act_code(act, 'modconv_epilogue_backward')
    if need_dnoise not in (None, 'plane', 'item'):
        raise RuntimeError("modconv_epilogue_backward: need_dnoise must be None, 'plane' or 'item'")
    if y is None and (act == 'lrelu' or clamp is not None):
        raise RuntimeError('modconv_epilogue_backward: the forward output y is needed for lrelu and for a clamp')
    if need_dscale and (x is None or scale is None):
        raise RuntimeError('modconv_epilogue_backward: dscale needs x and scale')
    for t in (y, x):
        if t is not None and (t.shape != dy.shape or t.dtype != dy.dtype or not _same_layout(t, dy)):
            raise RuntimeError('modconv_epilogue_backward: y and x must match dy in shape, dtype and memory format')
    n, c, h, w = dy.shape
    s32 = None if scale is None else scale.detach().to(torch.float32).contiguous()
    if s32 is not None and s32.numel() != n * c:
        raise RuntimeError('modconv_epilogue_backward: scale must have N*C elements')
    dev = dy.device
    e = _native.ext()
    if e is not None and hasattr(e, 'modconv_backward'):
        return e.modconv_backward(True, dy, y, x if need_dscale else None, s32, act_code, float(alpha), float(gain), _clamp_arg(clamp),
                                  bool(need_dx), bool(need_dscale), bool(need_dbias), {None: 0, 'plane': 1, 'item': 2}[need_dnoise])
    dx = torch.empty_like(dy) if need_dx else None
    dscale = torch.empty([n, c], dtype=torch.float32, device=dev) if need_dscale else None
    dbias = torch.empty([c], dtype=torch.float32, device=dev) if need_dbias else None
    dnoise = None if need_dnoise is None else torch.empty([n, 1, h, w] if need_dnoise == 'item' else [h, w], dtype=torch.float32, device=dev)
    ws = _modconv_backward_workspace(dy, layout) if (need_dscale or need_dbias or need_dnoise) else None
    name, shape = ('gnerf_modconv_epilogue_backward_nhwc', (n, h * w, c)) if layout == 'nhwc' else ('gnerf_modconv_epilogue_backward', (n, c, h * w))
    _launch(name, dy, _ptr(dy), _ptr(y), _ptr(x) if need_dscale else None, _ptr(s32), _DTYPE_CODE[dy.dtype], *shape, 1 if need_dnoise == 'item' else 0,
            act_code, float(alpha), float(gain), _clamp_arg(clamp), _ptr(dx), _ptr(dscale), _ptr(dbias), _ptr(dnoise), _ptr(ws))
    return dx, dscale, dbias, dnoise


def torgb_weights(weight, styles):
    """float16 [N, 3, C] = half(weight[o, c] * styles[n, c]): the 1 x 1 weights gnerf_torgb_nhwc forms per workgroup, as conv3x3_epilogue_torgb takes
    them (a constant of (latent, weight): cache it).  weight [3, C(, 1, 1)] float32, styles [N, C] float32 (ToRGB's affine output x its weight gain)."""
    w = weight.detach().to(torch.float32).reshape(1, 3, -1)
    return (w * styles.detach().to(torch.float32)[:, None, :]).to(torch.float16).contiguous()


@profiled('gnerf_hip::blur_epilogue_channels_last')
def blur_epilogue_channels_last(x, f, padding, blur_gain=1.0, bias=None, scale=None, act='lrelu', alpha=0.2, gain=1.0, clamp=None, next_scale=None,
                                flip_filter=False):
    """upfirdn2d(x, f, padding=padding, gain=blur_gain) with a 4x4 filter, then modconv_epilogue (no noise), in one pass over a
    channels_last x [N,C,H,W] (float16 / float32, C filling 16-byte vectors).  padding = [x0, x1, y0, y1].  Bit-identical to the
    two calls.  Returns a channels_last tensor."""
    _require_cuda(x, f, bias, scale, next_scale)
    if not is_channels_last(x) or x.dtype not in (torch.float32, torch.float16):
        raise RuntimeError('blur_epilogue_channels_last: x must be a channels_last float16/float32 tensor')
    act = _act_code(act, 'blur_epilogue_channels_last')
    n, c, h, w = x.shape
    f32 = f.detach().to(torch.float32).contiguous()
    if f32.shape != (4, 4) or c % (16 // x.element_size()) != 0:
        raise RuntimeError('blur_epilogue_channels_last: a 4x4 filter and whole 16-byte channel vectors are required')
    px0, px1, py0, py1 = [int(v) for v in padding]
    oh, ow = h + py0 + py1 - 3, w + px0 + px1 - 3
    if oh < 1 or ow < 1:
        raise RuntimeError('blur_epilogue_channels_last: output must be at least 1x1')
    s32 = _f32_operand(scale, n * c, 'scale', 'blur_epilogue_channels_last')
    nx = _f32_operand(next_scale, n * c, 'next_scale', 'blur_epilogue_channels_last')
    b = None if bias is None else bias.detach().to(x.dtype).contiguous()
    if b is not None and b.numel() != c:
        raise RuntimeError('blur_epilogue_channels_last: scale / next_scale must have N*C and bias C elements')
    if b is not None and b.data_ptr() % 16:          # fetched as vectors like the two above: a view at an odd offset is copied
        b = b.clone()
    y = torch.empty([n, c, oh, ow], dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    _launch('gnerf_blur4_epilogue_nhwc', x, _ptr(x), _ptr(f32), _ptr(y), _DTYPE_CODE[x.dtype], n, c, h, w, oh, ow, px0, py0, 1 if flip_filter else 0,
            float(blur_gain), _ptr(s32), _ptr(b), act, float(alpha), float(gain), _clamp_arg(clamp), _ptr(nx))
    return y


TORGB_CHANNELS = (32, 64, 128, 256, 512)


@profiled('gnerf_hip::torgb_channels_last')
def torgb_channels_last(x, weight, styles, bias=None, clamp=None, accumulate_into=None):
    """ToRGBLayer to three channels on a channels_last float16 x [N,C,H,W] (networks_stylegan2.py:349-367): weight [3,C,1,1] or [3,C]
    float32, styles [N,C] float32 (weight_gain applied), bias [3].  Returns float16 [N,3,H,W], NCHW.  See include/gnerf_hip.h.
    accumulate_into: a contiguous float32 [N,3,H,W] image; the layer's output (rounded to float16) is added to it IN PLACE and the
    image is returned -- the block's `img.add_(y.to(torch.float32))` in the same launch."""
    _require_cuda(x, weight, styles, bias)
    if x.dtype != torch.float16 or not is_channels_last(x) or x.shape[1] not in TORGB_CHANNELS:
        raise RuntimeError('torgb_channels_last: x must be a channels_last float16 tensor with 32, 64, 128, 256 or 512 channels')
    n, c, h, w = x.shape
    w32 = weight.detach().to(torch.float32).reshape(-1).contiguous()
    s32 = styles.detach().to(torch.float32).contiguous()
    if w32.numel() != 3 * c or s32.numel() != n * c:
        raise RuntimeError('torgb_channels_last: weight must be [3,C] and styles [N,C]')
    b = None if bias is None else bias.detach().to(torch.float16).contiguous()
    if accumulate_into is not None:
        img = accumulate_into
        _require_cuda(img)
        if img.dtype != torch.float32 or tuple(img.shape) != (n, 3, h, w) or not img.is_contiguous():
            raise RuntimeError('torgb_channels_last: accumulate_into must be a contiguous float32 [N,3,H,W] tensor')
        _launch('gnerf_torgb_nhwc_accumulate', x, _ptr(x), _ptr(w32), _ptr(s32), _ptr(b), _ptr(img), n, h * w, c,
                _clamp_arg(clamp))
        return img
    y = torch.empty([n, 3, h, w], dtype=torch.float16, device=x.device)
    _launch('gnerf_torgb_nhwc', x, _ptr(x), _ptr(w32), _ptr(s32), _ptr(b), _ptr(y), n, h * w, c, _clamp_arg(clamp))
    return y
