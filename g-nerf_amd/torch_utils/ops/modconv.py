"""The two elementwise passes around the un-fused modulated convolution (networks_stylegan2.py:76-86 and the bias_act of :331-333) as
differentiable ops, so that a TRAINING layer runs on this repo's kernels too:

    scale_channels(x, scale)                 x * scale[n, c]                                   (the input scaling by the styles, :77)
    epilogue(x, scale, noise, bias, ...)     t = x * scale[n, c] + noise                       (demodulation + noise, fma.fma at :79-81)
                                             y = clamp(act(t + bias[c]) * gain)                (bias_act, act linear or lrelu)

On GPU tensors (float16 / float32, NCHW contiguous or channels_last) each is an autograd.Function: the forward is gnerf_hip.scale_channels /
gnerf_hip.modconv_epilogue (the inference kernels, bit for bit), the backward one pass of csrc/modconv.hip's backward kernels plus their small
finishing launches -- float32 sums in a fixed order without atomics, so a backward gives the same bits every time.  The backward is first order
only (once_differentiable): differentiating it again raises PyTorch's "marked with @once_differentiable" error instead of returning a wrong
value.  On CPU tensors (and other dtypes / layouts) the ops are the plain PyTorch-op composition, differentiable to any order.

Gradients flow to x, scale, noise and bias.  What is saved: the epilogue's OUTPUT where the activation or a clamp needs a mask (the tensor the
next layer saves as its input anyway), its input only when scale needs a gradient, and for scale_channels its input when scale needs one.
"""

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable


def _kernel_form(x):
    """True where the kernels take x: a dense float16 / float32 GPU activation tensor, NCHW contiguous or channels_last."""
    if not (x.is_cuda and x.ndim == 4 and x.dtype in (torch.float16, torch.float32)):
        return False
    if not (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)):
        return False
    import gnerf_hip
    if not gnerf_hip.modconv_backward_available():
        raise RuntimeError('torch_utils.ops.modconv: libgnerf_hip.so has no modconv backward kernels: rebuild it (g-nerf_amd/csrc/build.sh)')
    return True


def _memory_format(x):
    return torch.contiguous_format if x.is_contiguous() else torch.channels_last


def _per_channel(v, x):
    return v.to(x.dtype).reshape(x.shape[0], x.shape[1], 1, 1)


def scale_channels_torch(x, scale):
    """The PyTorch-op form of scale_channels."""
    return x * _per_channel(scale, x)


def epilogue_torch(x, scale=None, noise=None, bias=None, act='lrelu', alpha=0.2, gain=1.0, clamp=None):
    """The PyTorch-op form of epilogue: every intermediate in x's dtype, as the reference's fma + bias_act chain materialises them."""
    assert act in ('linear', 'lrelu')
    if scale is not None and noise is not None:
        x = torch.addcmul(noise.to(x.dtype), x, _per_channel(scale, x))
    elif scale is not None:
        x = x * _per_channel(scale, x)
    elif noise is not None:
        x = x + noise.to(x.dtype)
    if bias is not None:
        x = x + bias.to(x.dtype).reshape(1, -1, 1, 1)
    if act == 'lrelu':
        x = F.leaky_relu(x, alpha)
    if gain != 1:
        x = x * gain
    if clamp is not None:
        x = x.clamp(-clamp, clamp)
    return x


class _ScaleChannels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        import gnerf_hip
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, scale if ctx.needs_input_grad[0] or ctx.needs_input_grad[1] else None)
        ctx.memory_format = _memory_format(x)
        return gnerf_hip.scale_channels(x, scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, dxs):
        import gnerf_hip
        x, scale = ctx.saved_tensors
        need_dx, need_ds = ctx.needs_input_grad
        if not (need_dx or need_ds):
            return None, None
        dxs = dxs.contiguous(memory_format=ctx.memory_format)            # (autograd hands over whatever layout the consumer's backward produced)
        dx, dscale = gnerf_hip.scale_channels_backward(dxs, x if x is not None else dxs, scale, need_dx=need_dx, need_dscale=need_ds)
        return dx, (dscale.to(scale.dtype).reshape(scale.shape) if need_ds else None)


class _Epilogue(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, noise, bias, act, alpha, gain, clamp):
        import gnerf_hip
        y = gnerf_hip.modconv_epilogue(x, bias, scale=scale, noise=noise, round_noise=True, act=act, alpha=alpha, gain=gain, clamp=clamp)
        need = ctx.needs_input_grad
        masked = act == 'lrelu' or clamp is not None
        ctx.save_for_backward(y if masked and any(need[:4]) else None, x if need[1] else None, scale if need[0] or need[1] else None)
        ctx.consts = (act, alpha, gain, clamp)
        ctx.memory_format = _memory_format(x)
        ctx.noise_meta = None if noise is None else (noise.shape, noise.dtype, 'item' if noise.numel() != x.shape[2] * x.shape[3] else 'plane')
        ctx.bias_meta = None if bias is None else (bias.shape, bias.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        import gnerf_hip
        y, x, scale = ctx.saved_tensors
        act, alpha, gain, clamp = ctx.consts
        need_dx, need_ds, need_dn, need_db = ctx.needs_input_grad[:4]
        if not (need_dx or need_ds or need_dn or need_db):
            return (None,) * 8
        dy = dy.contiguous(memory_format=ctx.memory_format)
        dx, dscale, dbias, dnoise = gnerf_hip.modconv_epilogue_backward(
            dy, y, x, scale, act=act, alpha=alpha, gain=gain, clamp=clamp, need_dx=need_dx, need_dscale=need_ds, need_dbias=need_db,
            need_dnoise=ctx.noise_meta[2] if need_dn else None)
        if need_ds:
            dscale = dscale.to(scale.dtype).reshape(scale.shape)
        if need_dn:
            dnoise = dnoise.to(ctx.noise_meta[1]).reshape(ctx.noise_meta[0])
        if need_db:
            dbias = dbias.to(ctx.bias_meta[1]).reshape(ctx.bias_meta[0])
        return dx, dscale, dnoise, dbias, None, None, None, None


def scale_channels(x, scale):
    """x [N,C,H,W] * scale [N,C] (or [N,C,1,1]), the product formed in x's dtype; the result has x's memory format."""
    if _kernel_form(x):
        return _ScaleChannels.apply(x, scale)
    return scale_channels_torch(x, scale)


def epilogue(x, scale=None, noise=None, bias=None, act='lrelu', alpha=0.2, gain=1.0, clamp=None):
    """clamp(act(x * scale[n,c] + noise + bias[c]) * gain) with x [N,C,H,W]; scale [N,C]; noise [H,W], [1,1,H,W] or [N,1,H,W]; bias [C]; act
    'linear' or 'lrelu' (slope alpha); every operand optional.  The result has x's dtype and memory format."""
    if act not in ('linear', 'lrelu'):
        raise ValueError("modconv.epilogue: act must be 'linear' or 'lrelu'")
    if _kernel_form(x):
        return _Epilogue.apply(x, scale, noise, bias, act, float(alpha), float(gain), None if clamp is None else float(clamp))
    return epilogue_torch(x, scale, noise, bias, act, alpha, gain, clamp)
