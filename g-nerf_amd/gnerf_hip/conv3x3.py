"""The fused 3x3 convolutions (csrc/conv3x3.hip): weight packing, what the kernels take, the float16 and the fp32-grade ([hi | lo | hi]
split) convolution + epilogue, and the stride-2 transposed convolution."""

import torch

from . import _native
from ._native import _clamp_arg, _launch, _ptr, _require_cuda, is_channels_last, profiled


def _nhwc_memory(x):
    """Is the MEMORY of the 4-D tensor x [N,H,W,C]?  is_channels_last -- or one pixel per image (H = W = 1), whose dense memory is [N,C] in
    either layout and which is_channels_last, made to tell the two layouts apart, counts as NCHW."""
    return is_channels_last(x) or (x.ndim == 4 and x.shape[1] > 1 and x.shape[2] == 1 and x.shape[3] == 1 and x.is_contiguous())


def _operands(x, w, name, w_name, channels='C', c_out=None):
    """Check the two operands every kernel here takes -- x (x3 for the split form) channels_last float16 [N,C,H,W], w contiguous float16
    [9,O,C padded to a multiple of 64], O == c_out when given -- and return (N, C, H, W, O)."""
    n, c, h, wd = x.shape
    o = w.shape[1]
    if not _nhwc_memory(x) or x.dtype != torch.float16 or tuple(w.shape) != (9, c_out or o, -(-c // 64) * 64) or w.dtype != torch.float16 or not w.is_contiguous():
        raise RuntimeError(f"{name}: {'x3' if channels == '3C' else 'x'} must be channels_last float16 [N,{channels},H,W] and {w_name} contiguous float16 "
                           f"[9,{c_out or 'O'},{channels}]")
    return n, c, h, wd, o


def _f32_operand(t, numel, what, name):
    """A per-channel / per-pixel operand as the kernels fetch it: float32, contiguous, `numel` elements, 16-byte aligned (a view at an odd
    offset is copied).  None stays None."""
    if t is None:
        return None
    t = t.detach().to(torch.float32).contiguous()
    if t.numel() != numel:
        raise RuntimeError(f'{name}: {what} must have {numel} elements')
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _pad_input_channels(w9):
    """[9, O, I] -> [9, O, I rounded up to a multiple of 64] with zeros (the kernels read the weights in 64-channel chunks; the activations'
    missing channels are masked to zero by the kernel)."""
    i = w9.shape[2]
    pad = -i % 64
    return (torch.nn.functional.pad(w9, (0, pad)) if pad else w9).contiguous()


def pack_conv3x3_weights(weight, dtype=torch.float16):
    """[O, I, 3, 3] -> the tap-major [9, O, I] form gnerf_conv3x3_epilogue_nhwc reads (w_packed[ky * 3 + kx, o, c] = weight[o, c, ky, kx])."""
    o, i = weight.shape[:2]
    return _pad_input_channels(weight.detach().to(dtype).permute(2, 3, 0, 1).reshape(9, o, i))


def conv3x3_epilogue_supported(x, c_out):
    """Does the fused convolution + epilogue kernel take this activation tensor?  (float16, channels_last, 8 x 32 pixel tiles, input channels
    in multiples of 8 -- the last 64-channel chunk is zero-padded --, output channels in blocks of 128.)"""
    return (x.is_cuda and x.dtype == torch.float16 and x.ndim == 4 and is_channels_last(x) and x.shape[2] % 8 == 0 and x.shape[3] % 32 == 0
            and x.shape[1] % 8 == 0 and c_out % 128 == 0 and x.shape[1] * x.shape[2] * x.shape[3] * 2 < (1 << 31))


@profiled('gnerf_hip::conv3x3_epilogue')
def conv3x3_epilogue(x, w_packed, bias=None, scale=None, noise=None, round_noise=False, alpha=0.2, gain=1.0, clamp=None, next_scale=None):
    """conv2d(x, w, padding=1) followed by modconv_epilogue(act='lrelu') in ONE launch (csrc/conv3x3.hip): x [N,C,H,W] float16
    channels_last, w_packed = pack_conv3x3_weights(w) [9,O,C padded to a multiple of 64] float16; scale / next_scale [N,O] float32, noise float32 [H,W], bias [O].
    Returns a channels_last [N,O,H,W] float16 tensor.  Shapes outside conv3x3_epilogue_supported raise (GNERF_E_UNSUPPORTED)."""
    _require_cuda(x, w_packed, bias, scale, noise, next_scale)
    name = 'conv3x3_epilogue'
    n, c, h, w, o = _operands(x, w_packed, name, 'w_packed')
    s32, nx, nz = _f32_operand(scale, n * o, 'scale', name), _f32_operand(next_scale, n * o, 'next_scale', name), _f32_operand(noise, h * w, 'noise', name)
    b = None if bias is None else bias.detach().to(torch.float16).contiguous()
    if b is not None and b.numel() != o:
        raise RuntimeError('conv3x3_epilogue: bias must have O elements')
    y = torch.empty([n, o, h, w], dtype=torch.float16, device=x.device, memory_format=torch.channels_last)
    _launch('gnerf_conv3x3_epilogue_nhwc', x, _ptr(x), _ptr(w_packed), _ptr(y), n, h, w, c, o, _ptr(s32), _ptr(nz), 1 if round_noise else 0, _ptr(b),
            float(alpha), float(gain), _clamp_arg(clamp), _ptr(nx))
    return y


def conv3x3_epilogue_torgb_supported(x, c_out):
    return conv3x3_epilogue_supported(x, c_out) and c_out == 128


@profiled('gnerf_hip::conv3x3_epilogue_torgb')
def conv3x3_epilogue_torgb(x, w_packed, img, rgb_w, rgb_bias=None, rgb_clamp=None, bias=None, scale=None, noise=None, round_noise=False, alpha=0.2, gain=1.0, clamp=None):
    """img += ToRGB(conv3x3_epilogue(x, ...)) in ONE launch that stores no layer output (csrc/conv3x3.hip, ABI 11): the last layer of a block whose x
    nothing else reads, with the block's ToRGB (rgb_w = torgb_weights(weight, styles) float16 [N,3,128], rgb_bias [3], rgb_clamp) in its epilogue and
    the result added to the running image img float32 [N,3,H,W] (dense NCHW) in place -- conv3x3_epilogue followed by torgb_channels_last(...,
    accumulate_into=img) with the same roundings.  x [N,C,H,W] float16 channels_last, w_packed [9,128,C padded] float16, scale [N,128] float32 (required)."""
    _require_cuda(x, w_packed, img, rgb_w, rgb_bias, bias, scale, noise)
    name = 'conv3x3_epilogue_torgb'
    n, c, h, w, o = _operands(x, w_packed, name, 'w_packed', c_out=128)
    if img.dtype != torch.float32 or tuple(img.shape) != (n, 3, h, w) or not img.is_contiguous():
        raise RuntimeError('conv3x3_epilogue_torgb: img must be a dense float32 [N,3,H,W] tensor')
    if rgb_w.dtype != torch.float16 or tuple(rgb_w.shape) != (n, 3, 128) or not rgb_w.is_contiguous() or scale is None:
        raise RuntimeError('conv3x3_epilogue_torgb: rgb_w must be float16 [N,3,128] (torgb_weights) and a demodulation scale is required')
    s32, nz = _f32_operand(scale, n * o, 'scale', name), _f32_operand(noise, h * w, 'noise', name)
    b = None if bias is None else bias.detach().to(torch.float16).contiguous()
    rb = None if rgb_bias is None else rgb_bias.detach().to(torch.float16).to(torch.float32).contiguous()       # (the stand-alone layer adds its float16 bias)
    if (b is not None and b.numel() != o) or (rb is not None and rb.numel() != 3):
        raise RuntimeError('conv3x3_epilogue_torgb: bias must have 128 elements, rgb_bias 3')
    _launch('gnerf_conv3x3_epilogue_torgb_nhwc', x, _ptr(x), _ptr(w_packed), n, h, w, c, _ptr(s32), _ptr(nz), 1 if round_noise else 0, _ptr(b),
            float(alpha), float(gain), _clamp_arg(clamp), _ptr(rgb_w), _ptr(rb), _clamp_arg(rgb_clamp),
            _ptr(img))
    return img


def _split_weights_f16x3(weight):
    """[O, I, kh, kw] float32 -> [O, 3 I, kh, kw] float32 holding [hi | hi | lo] along the input channels, hi = half(w), lo = half(w - hi): the
    weight operand of the fp32-grade convolution (gnerf_conv3x3_f32x3_epilogue_nhwc), against activations split as [hi | lo | hi]."""
    w = weight.detach().to(torch.float32)
    hi = w.to(torch.float16).to(torch.float32)
    lo = (w - hi).to(torch.float16).to(torch.float32)
    return torch.cat([hi, hi, lo], 1)


def pack_conv3x3_weights_f32x3(weight):
    """pack_conv3x3_weights of the [hi | hi | lo] split of a float32 weight [O, I, 3, 3]: float16 [9, O, 3 I padded to a multiple of 64]."""
    return pack_conv3x3_weights(_split_weights_f16x3(weight))


def pack_conv_transpose3x3_weights_f32x3(weight):
    """pack_conv_transpose3x3_weights of the [hi | hi | lo] split of a float32 weight [O, I, 3, 3] (correlation form)."""
    return pack_conv_transpose3x3_weights(_split_weights_f16x3(weight))


def split_overflow_flag(device):
    """The sticky device int split_f16x3 reports out-of-range activations in (one per device; read it with .item() when a check is wanted)."""
    f = _native._split_overflow.get(device)
    if f is None:
        f = _native._split_overflow[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return f


@profiled('gnerf_hip::split_f16x3')
def split_f16x3(x, scale=None):
    """x float32 channels_last [N, C, H, W] (C % 8 == 0), scale float32 [N, C] or None -> float16 channels_last [N, 3C, H, W] = [hi | lo | hi] of
    x * scale (csrc/conv3x3.hip): the activation operand of conv3x3_f32x3_epilogue / conv_transpose3x3_s2_f32x3."""
    _require_cuda(x, scale)
    n, c, h, w = x.shape
    if x.dtype != torch.float32 or not is_channels_last(x) or c % 8:
        raise RuntimeError('split_f16x3: x must be a channels_last float32 [N,C,H,W] tensor with C % 8 == 0')
    s32 = None if scale is None else scale.detach().to(torch.float32).contiguous()
    if s32 is not None and s32.numel() != n * c:
        raise RuntimeError('split_f16x3: scale must have N * C elements')
    y = torch.empty([n, 3 * c, h, w], dtype=torch.float16, device=x.device, memory_format=torch.channels_last)
    _launch('gnerf_split_f16x3_nhwc', x, _ptr(x), _ptr(s32), _ptr(y), n, h * w, c, _ptr(split_overflow_flag(x.device)))
    return y


def conv3x3_f32x3_supported(x, c_out):
    """Does the fp32-grade convolution take this float32 activation tensor (as its [hi | lo | hi] split)?  channels_last is not required of x:
    the caller converts; 8 x 32 pixel tiles, input channels in eights, output channels in blocks of 128."""
    return (x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and x.shape[2] % 8 == 0 and x.shape[3] % 32 == 0 and x.shape[1] % 8 == 0
            and c_out % 128 == 0 and 3 * x.shape[1] * x.shape[2] * x.shape[3] * 2 < (1 << 31))


def conv_transpose3x3_s2_f32x3_supported(x, c_out):
    return (x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and x.shape[1] % 8 == 0 and c_out % 128 == 0
            and 3 * x.shape[1] * x.shape[2] * x.shape[3] * 2 < (1 << 31))


@profiled('gnerf_hip::conv3x3_f32x3_epilogue')
def conv3x3_f32x3_epilogue(x3, w3_packed, bias=None, scale=None, noise=None, alpha=0.2, gain=1.0, clamp=None, next_scale=None):
    """The fp32-grade form of conv3x3_epilogue: x3 = split_f16x3(x) [N,3C,H,W] float16 channels_last, w3_packed = pack_conv3x3_weights_f32x3(w);
    bias float32 [O]; returns a channels_last float32 [N,O,H,W] tensor (nothing is rounded on the way out)."""
    _require_cuda(x3, w3_packed, bias, scale, noise, next_scale)
    name = 'conv3x3_f32x3_epilogue'
    n, c3, h, w, o = _operands(x3, w3_packed, name, 'w3_packed', '3C')
    s32, nx = _f32_operand(scale, n * o, 'scale', name), _f32_operand(next_scale, n * o, 'next_scale', name)
    nz, b = _f32_operand(noise, h * w, 'noise', name), _f32_operand(bias, o, 'bias', name)
    y = torch.empty([n, o, h, w], dtype=torch.float32, device=x3.device, memory_format=torch.channels_last)
    _launch('gnerf_conv3x3_f32x3_epilogue_nhwc', x3, _ptr(x3), _ptr(w3_packed), _ptr(y), n, h, w, c3, o, _ptr(s32), _ptr(nz), _ptr(b), float(alpha),
            float(gain), _clamp_arg(clamp), _ptr(nx))
    return y


@profiled('gnerf_hip::conv_transpose3x3_s2_f32x3')
def conv_transpose3x3_s2_f32x3(x3, w3_phases):
    """The fp32-grade form of conv_transpose3x3_s2: x3 = split_f16x3(x), w3_phases = pack_conv_transpose3x3_weights_f32x3(w); returns a
    channels_last float32 [N,O,2H+1,2W+1] tensor."""
    _require_cuda(x3, w3_phases)
    n, c3, h, w, o = _operands(x3, w3_phases, 'conv_transpose3x3_s2_f32x3', 'w3_phases', '3C')
    y = torch.empty([n, o, 2 * h + 1, 2 * w + 1], dtype=torch.float32, device=x3.device, memory_format=torch.channels_last)
    _launch('gnerf_conv_transpose3x3_s2_f32x3_nhwc', x3, _ptr(x3), _ptr(w3_phases), _ptr(y), n, h, w, c3, o)
    return y


def pack_conv_transpose3x3_weights(weight, dtype=torch.float16):
    """[O, I, 3, 3] (the correlation-form weight of a x2 layer: conv_transpose2d(x, weight.transpose(0, 1), stride=2)) -> the [9, O, I] form
    gnerf_conv_transpose3x3_s2_nhwc reads: the taps grouped by OUTPUT PHASE (py, px) = (oy & 1, ox & 1) -- phase (0,0): (ky, kx) = (0,0),
    (0,2), (2,0), (2,2); phase (0,1): (0,1), (2,1); phase (1,0): (1,0), (1,2); phase (1,1): (1,1)."""
    order = [(0, 0), (0, 2), (2, 0), (2, 2), (0, 1), (2, 1), (1, 0), (1, 2), (1, 1)]
    w = weight.detach().to(dtype)
    return _pad_input_channels(torch.stack([w[:, :, ky, kx] for ky, kx in order]))


def conv_transpose3x3_s2_supported(x, c_out):
    """Does the phase-decomposed transposed convolution take this activation tensor?  (float16, channels_last, input channels in
    multiples of 8, output channels in blocks of 128; any height and width.)"""
    return (x.is_cuda and x.dtype == torch.float16 and x.ndim == 4 and _nhwc_memory(x) and x.shape[1] % 8 == 0 and c_out % 128 == 0
            and x.shape[1] * x.shape[2] * x.shape[3] * 2 < (1 << 31))


@profiled('gnerf_hip::conv_transpose3x3_s2')
def conv_transpose3x3_s2(x, w_phases):
    """conv_transpose2d(x, w.transpose(0, 1), stride=2) for a 3x3 kernel (csrc/conv3x3.hip, MODE 1): x [N,C,H,W] float16 channels_last,
    w_phases = pack_conv_transpose3x3_weights(w) [9,O,C padded to a multiple of 64] float16.  Returns a channels_last [N,O,2H+1,2W+1] float16 tensor."""
    _require_cuda(x, w_phases)
    n, c, h, w, o = _operands(x, w_phases, 'conv_transpose3x3_s2', 'w_phases')
    y = torch.empty([n, o, 2 * h + 1, 2 * w + 1], dtype=torch.float16, device=x.device, memory_format=torch.channels_last)
    _launch('gnerf_conv_transpose3x3_s2_nhwc', x, _ptr(x), _ptr(w_phases), _ptr(y), n, h, w, c, o)
    return y
