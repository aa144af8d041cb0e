"""SSIM and MS-SSIM with the interface of the pytorch_msssim package (what training_loop.py:30 imports and :341-376 calls):
ssim, ms_ssim, SSIM, MS_SSIM.

Definition (Wang et al. 2004, as that package computes it): a 1-D Gaussian window g (win_size taps, sigma win_sigma, sum 1) applied
separably per channel as a valid correlation; mu = g*X, sigma^2 = g*X^2 - mu^2, sigma12 = g*XY - mu1 mu2;
cs = (2 sigma12 + C2) / (sigma1^2 + sigma2^2 + C2), ssim = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs, C = (K * data_range)^2;
the value per (n, c) is the mean over the map.

Routing: CPU tensors take the PyTorch-op form below; GPU tensors take the gfx950 kernel (csrc/ssim.hip, forward and
backward, through a torch.autograd.Function) with no fallback -- except the calls the kernel does not cover (a window longer than 11 taps,
5-D inputs, a spatial side shorter than the window), which take the PyTorch-op form with one RuntimeWarning per reason and process.
The kernel's gradient is first order only.
"""

import functools
import warnings

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
KERNEL_MAX_WIN = 11


@functools.lru_cache(maxsize=32)
def gaussian_window(win_size=11, win_sigma=1.5, dtype=torch.float64):
    """g[i] ~ exp(-(i - win_size // 2)^2 / (2 sigma^2)), normalised to sum 1 (computed in float64, returned as `dtype`).  Cached: treat
    the result as read-only."""
    coords = torch.arange(win_size, dtype=torch.float64) - win_size // 2
    g = torch.exp(-coords.square() / (2.0 * float(win_sigma) ** 2))
    return (g / g.sum()).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the PyTorch-op form


def _filter_separable(x, win):
    """The window along every spatial dimension of x [N, C, *spatial] in turn (valid correlation, per channel); a dimension shorter than
    the window is left unsmoothed, with a warning, as the package does."""
    conv = F.conv2d if x.ndim == 4 else F.conv3d
    channels, taps = x.shape[1], win.numel()
    for i, size in enumerate(x.shape[2:]):
        if size < taps:
            warnings.warn(f'ssim: no smoothing along dimension {2 + i} of an input of shape {tuple(x.shape)}: shorter than the window of {taps}')
            continue
        shape = [channels, 1] + [1] * (x.ndim - 2)
        shape[2 + i] = taps
        x = conv(x, win.reshape([1, 1] + [-1 if d == i else 1 for d in range(x.ndim - 2)]).expand(shape), groups=channels)
    return x


def ssim_pair_torch(X, Y, win, C1, C2):
    """(ssim [N, C], cs [N, C]) of X, Y [N, C, *spatial] with PyTorch ops; win: 1-D tensor.  Differentiable to any order."""
    win = win.to(device=X.device, dtype=X.dtype)
    mu1, mu2 = _filter_separable(X, win), _filter_separable(Y, win)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sigma1_sq = _filter_separable(X * X, win) - mu1_sq
    sigma2_sq = _filter_separable(Y * Y, win) - mu2_sq
    sigma12 = _filter_separable(X * Y, win) - mu12
    cs_map = (2 * sigma12 + C2) / (sigma1_sq + sigma2_sq + C2)
    ssim_map = (2 * mu12 + C1) / (mu1_sq + mu2_sq + C1) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel form


class _SsimPairKernel(torch.autograd.Function):
    """(ssim [N, C], cs [N, C]) float32 on the gfx950 kernel.  Nothing but the inputs is saved: the backward kernel recomputes the moments."""

    @staticmethod
    def forward(ctx, X, Y, window, C1, C2):
        import gnerf_hip
        ctx.save_for_backward(X, Y)
        ctx.consts = (window, C1, C2)
        ctx.set_materialize_grads(False)                             # an unused output (ssim() drops cs) arrives as None, not as zeros
        return gnerf_hip.ssim_forward(X, Y, window, C1, C2)

    @staticmethod
    def backward(ctx, g_ssim, g_cs):
        # once_differentiable would turn a create_graph backward into a silent non-differentiable result; the check has to see the
        # gradients while they still carry requires_grad, so it sits here and the decorated body below does the work.
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (g_ssim, g_cs, *ctx.saved_tensors)):
            raise RuntimeError('ssim: double backward (create_graph=True) through the fused kernel is not supported: its gradient is first '
                               'order only; ssim_pair_torch is the PyTorch-op form, differentiable to any order')
        return _SsimPairKernel._backward_once(ctx, g_ssim, g_cs)

    @staticmethod
    @once_differentiable
    def _backward_once(ctx, g_ssim, g_cs):
        import gnerf_hip
        if g_ssim is None and g_cs is None:
            return None, None, None, None, None
        X, Y = ctx.saved_tensors
        window, C1, C2 = ctx.consts
        dX, dY = gnerf_hip.ssim_backward(X, Y, window, C1, C2, g_ssim, g_cs, need_dx=ctx.needs_input_grad[0], need_dy=ctx.needs_input_grad[1])
        return dX, dY, None, None, None


_warned_fallbacks = set()


def _warn_gpu_fallback(reason):
    if reason not in _warned_fallbacks:
        _warned_fallbacks.add(reason)
        warnings.warn(f'ssim: GPU tensors, but {reason}: running the PyTorch-op form, not the fused HIP kernel', RuntimeWarning, stacklevel=4)


def _uncovered(X, win):
    """Why the kernel does not cover this call on GPU tensors, or None."""
    if X.ndim == 5:
        return '5-D (3-D image) inputs'
    if win.numel() > KERNEL_MAX_WIN:
        return f'the window has {win.numel()} taps (the kernel takes up to {KERNEL_MAX_WIN})'
    if min(X.shape[2:]) < win.numel():
        return 'a spatial side is shorter than the window'
    return None


def ssim_pair(X, Y, win, C1, C2):
    """(ssim [N, C], cs [N, C]) by this project's routing rule; win: 1-D tensor.  The kernel form returns float32 whatever X's dtype.
    The kernel takes its taps by value from the host: the default window (a cached CPU tensor) or a caller's CPU tensor costs nothing, a
    caller's window that lives on the GPU is read back on every call -- one host synchronisation, which also rules out graph capture."""
    if X.device.type != 'cuda':
        return ssim_pair_torch(X, Y, win, C1, C2)
    reason = _uncovered(X, win)
    if reason is not None:
        _warn_gpu_fallback(reason)
        return ssim_pair_torch(X, Y, win, C1, C2)
    if X.dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f'ssim: no kernel for {X.dtype} images on a GPU (float32 and float16 only); ssim_pair_torch is the PyTorch-op form')
    return _SsimPairKernel.apply(X, Y, tuple(float(v) for v in win.detach().double().cpu().tolist()), float(C1), float(C2))


# ---------------------------------------------------------------------------------------------------------------------
# the package's interface


def _prepare(X, Y, win_size, win_sigma, win, what):
    if X.shape != Y.shape:
        raise ValueError(f'{what}: input images should have the same dimensions, but got {tuple(X.shape)} and {tuple(Y.shape)}')
    for d in range(X.ndim - 1, 1, -1):                               # singleton spatial dimensions go, as in the package
        X, Y = X.squeeze(d), Y.squeeze(d)
    if X.ndim not in (4, 5):
        raise ValueError(f'{what}: input images should be 4-d or 5-d tensors, but got {tuple(X.shape)}')
    if X.dtype != Y.dtype or X.device != Y.device:
        raise ValueError(f'{what}: input images should have the same dtype and device, but got {X.dtype} on {X.device} and {Y.dtype} on {Y.device}')
    if win is not None:
        win = win.reshape(-1) if win.ndim == 1 else win.reshape(-1, win.shape[-1])[0]      # the package repeats one window per channel
        win_size = win.numel()
    if win_size % 2 != 1:
        raise ValueError(f'{what}: window size should be odd, got {win_size}')
    if win is None:
        win = gaussian_window(win_size, win_sigma)
    return X, Y, win


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03), nonnegative_ssim=False):
    """pytorch_msssim.ssim: a scalar (size_average) or [N] (the mean over channels of the per-channel values)."""
    X, Y, win = _prepare(X, Y, win_size, win_sigma, win, 'ssim')
    per_channel, _ = ssim_pair(X, Y, win, (K[0] * data_range) ** 2, (K[1] * data_range) ** 2)
    if nonnegative_ssim:
        per_channel = torch.relu(per_channel)
    return per_channel.mean() if size_average else per_channel.mean(1)


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """pytorch_msssim.ms_ssim: prod_l relu(cs_l)^w_l over the first levels times relu(ssim)^w of the last, 2x average pooling in between."""
    X, Y, win = _prepare(X, Y, win_size, win_sigma, win, 'ms_ssim')
    weights = MS_SSIM_WEIGHTS if weights is None else tuple(float(v) for v in (weights.tolist() if torch.is_tensor(weights) else weights))
    levels = len(weights)
    if not min(X.shape[-2:]) > (win.numel() - 1) * 2 ** (levels - 1):
        raise ValueError(f'ms_ssim: image size should be larger than {(win.numel() - 1) * 2 ** (levels - 1)} due to the {levels - 1} '
                         f'downsamplings, got {tuple(X.shape[-2:])}')
    pool = F.avg_pool2d if X.ndim == 4 else F.avg_pool3d
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    terms = []
    for level in range(levels):
        per_channel, cs = ssim_pair(X, Y, win, C1, C2)
        if level < levels - 1:
            terms.append(torch.relu(cs))
            padding = [s % 2 for s in X.shape[2:]]
            X, Y = pool(X, kernel_size=2, padding=padding), pool(Y, kernel_size=2, padding=padding)
    terms.append(torch.relu(per_channel))
    stacked = torch.stack(terms, dim=0)                              # [levels, N, C]
    value = torch.prod(stacked ** stacked.new_tensor(weights).view(-1, 1, 1), dim=0)
    return value.mean() if size_average else value.mean(1)


class SSIM(torch.nn.Module):
    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2, K=(0.01, 0.03), nonnegative_ssim=False):
        super().__init__()
        self.win_size, self.win_sigma, self.channel, self.spatial_dims = win_size, win_sigma, channel, spatial_dims
        self.size_average, self.data_range, self.K, self.nonnegative_ssim = size_average, data_range, K, nonnegative_ssim

    def forward(self, X, Y):
        # (no `win` buffer as in the package: the window comes from its parameters, cached, so that float64 inputs get float64 taps)
        return ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win_size=self.win_size, win_sigma=self.win_sigma, K=self.K,
                    nonnegative_ssim=self.nonnegative_ssim)


class MS_SSIM(torch.nn.Module):
    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2, weights=None, K=(0.01, 0.03)):
        super().__init__()
        self.win_size, self.win_sigma, self.channel, self.spatial_dims = win_size, win_sigma, channel, spatial_dims
        self.size_average, self.data_range, self.weights, self.K = size_average, data_range, weights, K

    def forward(self, X, Y):
        return ms_ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win_size=self.win_size, win_sigma=self.win_sigma,
                       weights=self.weights, K=self.K)
