"""CPU tests of torch_utils/ops/ssim.py (the PyTorch-op form, the package interface, the pytorch_msssim shim, the --ssim terms of the
training step) against tests/ssim_ref.py, and of the C ABI 15 declarations.  The cases are shared with tests/test_ssim_gpu.py."""

import ctypes
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssim_ref
from torch_utils.ops import ssim as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT = 0.72418548526                                    # (2ab + C1) / (a^2 + b^2 + C1) for a = 0.3, b = 0.7, L = 1


def _smooth(gen, n, size):
    return F.interpolate(torch.rand(n, 3, 16, 16, generator=gen, dtype=torch.float64), size=(size, size), mode='bicubic', align_corners=False).clamp(0, 1)


def cases(full=True):
    """name -> (X, Y float64 [N, 3, H, W], data_range, win_size).  full=False leaves the 512^2 cases out."""
    gen = torch.Generator().manual_seed(20)
    r = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)
    out = {
        'noise_64': (r(2, 3, 64, 64), r(2, 3, 64, 64), 1.0, 11),
        'noise_64_range255': (r(2, 3, 64, 64) * 255, r(2, 3, 64, 64) * 255, 255.0, 11),
        'odd_37x53_win11': (r(2, 3, 37, 53), r(2, 3, 37, 53), 1.0, 11),
        'odd_37x53_win7': (r(2, 3, 37, 53), r(2, 3, 37, 53), 1.0, 7),
        'odd_37x53_win3': (r(2, 3, 37, 53), r(2, 3, 37, 53), 1.0, 3),
        'flat_0.3_0.7': (torch.full((1, 3, 64, 64), 0.3, dtype=torch.float64), torch.full((1, 3, 64, 64), 0.7, dtype=torch.float64), 1.0, 11),
    }
    if full:
        img = _smooth(gen, 2, 512)
        out['image_plus_noise_512'] = (img, (img + 0.1 * torch.randn(2, 3, 512, 512, generator=gen, dtype=torch.float64)).clamp(0, 1), 1.0, 11)
        out['smooth_512'] = (_smooth(gen, 2, 512), _smooth(gen, 2, 512), 1.0, 11)
        out['smooth_512_range255'] = (_smooth(gen, 1, 512) * 255, _smooth(gen, 1, 512) * 255, 255.0, 11)
    return out


def pair_and_grads(X, Y, L, k, form, g_ssim=None, g_cs=None):
    """(ssim, cs, dX, dY) of `form(X, Y, win, C1, C2)` under the upstream weights (default: ones for ssim, none for cs)."""
    X, Y = X.detach().clone().requires_grad_(True), Y.detach().clone().requires_grad_(True)
    s, cs = form(X, Y, S.gaussian_window(k, 1.5), (0.01 * L) ** 2, (0.03 * L) ** 2)
    loss = (s.double() * (1.0 if g_ssim is None else g_ssim.to(s.device).double())).sum()
    if g_cs is not None:
        loss = loss + (cs.double() * g_cs.to(cs.device).double()).sum()
    dX, dY = torch.autograd.grad(loss, [X, Y])
    return s.detach(), cs.detach(), dX, dY


@pytest.mark.parametrize('name', sorted(cases()))
def test_op_form_matches_the_direct_2d_restatement(name):
    """float64: within 1e-12 of ssim_ref.  float32: its error against float64 is printed per case -- the yardstick of the GPU test -- and
    held to 1e-4: sigma^2 = g*X^2 - mu^2 cancels with an absolute error of a few float32 ulps of L^2 (~1e-7 L^2) over a denominator of at
    least C2 = 9e-4 L^2, so a map point is good to ~1e-4 relative at worst and the mean is no worse."""
    X, Y, L, k = cases()[name]
    ref_s, ref_cs = ssim_ref.ssim_pair(X.numpy(), Y.numpy(), L, k)
    s, cs, dX, dY = pair_and_grads(X, Y, L, k, S.ssim_pair_torch)
    assert np.abs(s.numpy() - ref_s).max() < 1e-12 and np.abs(cs.numpy() - ref_cs).max() < 1e-12
    s32, cs32, dX32, dY32 = pair_and_grads(X.float(), Y.float(), L, k, S.ssim_pair_torch)
    ref32 = pair_and_grads(X.float().double(), Y.float().double(), L, k, S.ssim_pair_torch)
    verr = float((s32.double() - ref32[0]).abs().max())
    gerr = float((dY32.double() - ref32[3]).abs().max() / ref32[3].abs().max().clamp_min(1e-300))
    print(f'{name}: float32 value error {verr:.2e}, gradient error / max |grad| {gerr:.2e}')
    assert verr < 1e-4


def test_closed_forms_and_symmetry():
    a, b = torch.full((2, 3, 32, 40), 0.3, dtype=torch.float64), torch.full((2, 3, 32, 40), 0.7, dtype=torch.float64)
    assert abs(float(S.ssim(a, b, data_range=1.0)) - FLAT) < 1e-10
    assert abs((2 * 0.3 * 0.7 + 1e-4) / (0.09 + 0.49 + 1e-4) - FLAT) < 1e-10
    X, Y, L, k = cases(False)['noise_64']
    assert float(S.ssim(X, X, data_range=1.0)) == 1.0
    assert float(S.ssim(X.float(), X.float(), data_range=1.0)) == 1.0
    assert torch.equal(S.ssim(X, Y, data_range=1.0, size_average=False), S.ssim(Y, X, data_range=1.0, size_average=False))


def test_interface_shapes_options_and_errors():
    X, Y, L, k = cases(False)['noise_64']
    assert S.ssim(X, Y, data_range=1.0).shape == () and S.ssim(X, Y, data_range=1.0, size_average=False).shape == (2,)
    per = ssim_ref.ssim_pair(X.numpy(), Y.numpy(), 1.0)[0]
    assert np.abs(S.ssim(X, Y, data_range=1.0, size_average=False).numpy() - per.mean(axis=1)).max() < 1e-12
    assert abs(float(S.SSIM(data_range=1.0)(X, Y)) - per.mean()) < 1e-12
    # anti-correlated images give negative per-channel values: relu comes before the channel mean
    neg = ssim_ref.ssim_pair(X.numpy(), 1 - X.numpy(), 1.0)[0]
    assert (neg < 0).all()
    assert float(S.ssim(X, 1 - X, data_range=1.0)) < 0 and float(S.ssim(X, 1 - X, data_range=1.0, nonnegative_ssim=True)) == 0.0
    mixed = torch.cat([X[:, :1], 1 - X[:, 1:]], 1)
    want = np.maximum(ssim_ref.ssim_pair(X.numpy(), mixed.numpy(), 1.0)[0], 0).mean(axis=1)
    assert np.abs(S.ssim(X, mixed, data_range=1.0, size_average=False, nonnegative_ssim=True).numpy() - want).max() < 1e-12
    # a caller's window, per channel as the package builds it
    win = torch.tensor(ssim_ref.window(7, 1.0)).repeat(3, 1, 1, 1)
    assert abs(float(S.ssim(X, Y, data_range=1.0, win=win)) - ssim_ref.ssim(X.numpy(), Y.numpy(), 1.0, k=7, sigma=1.0)) < 1e-12
    with pytest.raises(ValueError):
        S.ssim(X, Y[:, :, :-1], data_range=1.0)
    with pytest.raises(ValueError):
        S.ssim(X, Y.float(), data_range=1.0)
    with pytest.raises(ValueError):
        S.ssim(X, Y, data_range=1.0, win_size=10)
    with pytest.raises(ValueError):
        S.ssim(X[0], Y[0], data_range=1.0)
    # a side shorter than the window is left unsmoothed (with the package's warning), 5-D inputs are 3-D images
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        v = S.ssim(X[:, :, :8], Y[:, :, :8], data_range=1.0)
    assert w and torch.isfinite(v)
    assert torch.isfinite(S.ssim(X.reshape(1, 3, 2, 64, 64)[:, :, :, :16, :16].repeat(1, 1, 6, 1, 1), Y.reshape(1, 3, 2, 64, 64)[:, :, :, :16, :16].repeat(1, 1, 6, 1, 1), data_range=1.0))


def test_ms_ssim_matches_the_restatement_and_checks_the_size():
    gen = torch.Generator().manual_seed(3)
    X = _smooth(gen, 2, 192)[:, :, :, :177].contiguous()
    Y = (X + 0.05 * torch.randn(X.shape, generator=gen, dtype=torch.float64)).clamp(0, 1)
    want = ssim_ref.ms_ssim(X.numpy(), Y.numpy(), 1.0, size_average=False)
    assert np.abs(S.ms_ssim(X, Y, data_range=1.0, size_average=False).numpy() - want).max() < 1e-12
    assert abs(float(S.MS_SSIM(data_range=1.0)(X, Y)) - want.mean()) < 1e-12
    with pytest.raises(ValueError):
        S.ms_ssim(X[:, :, :160, :160], Y[:, :, :160, :160], data_range=1.0)          # needs > (11 - 1) * 16
    assert torch.isfinite(S.ms_ssim(X[:, :, :161, :161], Y[:, :, :161, :161], data_range=1.0))


def test_gradcheck_of_the_op_form():
    gen = torch.Generator().manual_seed(4)
    X = torch.rand(2, 2, 17, 19, generator=gen, dtype=torch.float64, requires_grad=True)
    Y = torch.rand(2, 2, 17, 19, generator=gen, dtype=torch.float64, requires_grad=True)
    win = S.gaussian_window(11, 1.5)
    assert torch.autograd.gradcheck(lambda a, b: S.ssim_pair_torch(a, b, win, 1e-4, 9e-4), (X, Y), atol=1e-7, rtol=1e-5)


def test_pytorch_msssim_resolves_to_the_shim():
    code = ('import sys; sys.path.insert(0, sys.argv[1]); import pytorch_msssim as P, os; '
            'assert os.path.dirname(os.path.abspath(P.__file__)) == os.path.join(sys.argv[1], "pytorch_msssim"), P.__file__; '
            'from pytorch_msssim import ssim, ms_ssim, SSIM, MS_SSIM; import torch_utils.ops.ssim as S; '
            'assert ssim is S.ssim and ms_ssim is S.ms_ssim and SSIM is S.SSIM and MS_SSIM is S.MS_SSIM; print("ok")')
    out = subprocess.run([sys.executable, '-c', code, os.path.join(ROOT, 'g-nerf_amd')], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', out.stdout + out.stderr


class _TinyG(torch.nn.Module):
    """The generator interface generator_loss uses, at toy size: z -> a 16^2 image, upsampled to the 32^2 `image`."""

    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(8, 3 * 16 * 16)

    def mapping(self, z, c):
        return z

    def synthesis(self, ws, c, neural_rendering_resolution=None, **kw):
        raw = torch.tanh(self.fc(ws)).view(-1, 3, 16, 16)
        return dict(image=F.interpolate(raw, size=(32, 32), mode='bilinear', align_corners=False), image_raw=raw, image_depth=raw[:, :1] + 2.5)


def _tiny_loss(ssim, seed=0):
    import train_step_mi355x as T
    torch.manual_seed(seed)
    G = _TinyG()
    batch = dict(z=torch.randn(4, 8), c=torch.zeros(4, 25), loss_image=torch.rand(4, 3, 32, 32) * 2 - 1, factor=torch.tensor([1.0, 0.5, 1.0, 0.0]))
    D = lambda img, c: img.mean((1, 2, 3))
    kw = {} if ssim is None else dict(ssim=ssim)
    loss, parts, gen = T.generator_loss(G, D, batch, 16, **kw)
    loss.backward()
    return loss.detach(), parts, G.fc.weight.grad.clone()


def test_generator_loss_ssim_terms():
    base, base_parts, base_grad = _tiny_loss(None)
    off, off_parts, off_grad = _tiny_loss(False)
    assert torch.equal(base, off) and torch.equal(base_grad, off_grad) and list(base_parts) == ['l1', 'l1_raw', 'gan'] == list(off_parts)
    assert all(torch.equal(base_parts[k], off_parts[k]) for k in base_parts)
    on, parts, grad = _tiny_loss(True)
    assert set(parts) == {'l1', 'l1_raw', 'ssim', 'ssim_raw', 'gan'}
    assert all(torch.isfinite(v) for v in parts.values()) and torch.isfinite(grad).all()
    assert 0 < float(parts['ssim']) < 2 and 0 < float(parts['ssim_raw']) < 2 and float(on) > float(off)
    assert not torch.equal(grad, off_grad)


def test_abi_15_declarations():
    import gnerf_hip
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    assert int(re.search(r'#define GNERF_ABI_VERSION (\d+)', header).group(1)) == gnerf_hip.ABI_VERSION == 15
    assert int(re.search(r'#define GNERF_SSIM_MAX_WIN (\d+)', header).group(1)) == gnerf_hip.SSIM_MAX_WIN == S.KERNEL_MAX_WIN == 11
    p, i, f, i64p, fp = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_float)
    assert gnerf_hip.SIGNATURES['gnerf_ssim_workspace_bytes'] == (i, [i, i, i, i, i, ctypes.POINTER(ctypes.c_size_t)])
    assert gnerf_hip.SIGNATURES['gnerf_ssim_forward'] == (i, [p, p, i, i, i, i, i, i64p, i64p, fp, i, f, f, p, p, p, p])
    assert gnerf_hip.SIGNATURES['gnerf_ssim_backward'] == (i, [p, p, i, i, i, i, i, i64p, i64p, fp, i, f, f, p, p, p, i64p, p, i64p, p])
    # the argument counts are the header's
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in ('gnerf_ssim_workspace_bytes', 'gnerf_ssim_forward', 'gnerf_ssim_backward'):
        args = re.search(name + r'\s*\((.*?)\)\s*;', header, flags=re.S).group(1)
        assert len(args.split(',')) == len(gnerf_hip.SIGNATURES[name][1]), name


def test_c_entry_points_refuse_bad_shapes_without_a_gpu():
    """The argument checks come before any launch, so they answer on a machine without a GPU: an image smaller than the window, an even
    window, a window longer than 11, null pointers -- an error code and a message, never a crash."""
    import gnerf_hip
    lib = gnerf_hip.load()
    nbytes = ctypes.c_size_t()
    assert lib.gnerf_ssim_workspace_bytes(4, 3, 512, 512, 11, ctypes.byref(nbytes)) == 0 and nbytes.value == 4 * 3 * 16 * 16 * 8
    for h, w, win, word in ((8, 64, 11, b'smaller'), (64, 8, 11, b'smaller'), (64, 64, 10, b'odd'), (64, 64, 13, b'odd'), (64, 64, 0, b'odd')):
        assert lib.gnerf_ssim_workspace_bytes(1, 3, h, w, win, ctypes.byref(nbytes)) == -1
        assert word in lib.gnerf_last_error(), lib.gnerf_last_error()
    assert lib.gnerf_ssim_workspace_bytes(1, 3, 64, 64, 11, None) == -1
    st = (ctypes.c_int64 * 4)(3 * 64 * 64, 64 * 64, 64, 1)
    win = (ctypes.c_float * 11)(*ssim_ref.window())
    assert lib.gnerf_ssim_forward(None, None, 0, 1, 3, 64, 64, st, st, win, 11, 1e-4, 9e-4, None, None, None, None) == -1
    assert b'null' in lib.gnerf_last_error()
    assert lib.gnerf_ssim_backward(None, None, 0, 1, 3, 64, 64, st, st, win, 11, 1e-4, 9e-4, None, None, None, None, None, None, None) == -1
    assert b'null' in lib.gnerf_last_error()
    # CPU tensors never reach the library
    X = torch.rand(1, 3, 32, 32)
    with pytest.raises(RuntimeError):
        gnerf_hip.ssim_forward(X, X, ssim_ref.window(), 1e-4, 9e-4)
    with pytest.raises(RuntimeError):
        gnerf_hip.ssim_backward(X, X, ssim_ref.window(), 1e-4, 9e-4, torch.ones(1, 3), None)


def test_singleton_spatial_dimensions_go_as_in_the_package():
    gen = torch.Generator().manual_seed(21)
    X, Y = torch.rand(1, 3, 40, 40, generator=gen, dtype=torch.float64), torch.rand(1, 3, 40, 40, generator=gen, dtype=torch.float64)
    want = S.ssim(X, Y, data_range=1.0)
    assert torch.equal(S.ssim(X[:, :, None], Y[:, :, None], data_range=1.0), want)            # [N, C, 1, H, W] is a 2-D image
    assert torch.equal(S.ssim(X[..., None], Y[..., None], data_range=1.0), want)
    with pytest.raises(ValueError):                                                             # [N, C, 1, W] is left with one spatial dimension
        S.ssim(X[:, :, :1], Y[:, :, :1], data_range=1.0)
    assert not any(name == 'win' for name, _ in list(S.SSIM().named_buffers()) + list(S.MS_SSIM().named_buffers()))


def test_an_unused_output_reaches_the_backward_as_none(monkeypatch):
    """ssim() drops cs: the autograd function must hand the kernel None for it (the entry's null-pointer path), not a tensor of zeros
    that autograd filled in.  The library calls are replaced by the op form, so this runs without a GPU."""
    import gnerf_hip
    seen = []

    def forward(X, Y, window, C1, C2):
        return S.ssim_pair_torch(X.detach(), Y.detach(), torch.tensor(window, dtype=X.dtype), C1, C2)

    def backward(X, Y, window, C1, C2, g_ssim, g_cs, need_dx=True, need_dy=True):
        seen.append((g_ssim is None, g_cs is None, need_dx, need_dy))
        x, y = X.detach().requires_grad_(True), Y.detach().requires_grad_(True)
        with torch.enable_grad():
            s, cs = S.ssim_pair_torch(x, y, torch.tensor(window, dtype=X.dtype), C1, C2)
            total = sum((g * v).sum() for g, v in ((g_ssim, s), (g_cs, cs)) if g is not None)
        dx, dy = torch.autograd.grad(total, [x, y])
        return (dx if need_dx else None), (dy if need_dy else None)
    monkeypatch.setattr(gnerf_hip, 'ssim_forward', forward)
    monkeypatch.setattr(gnerf_hip, 'ssim_backward', backward)
    gen = torch.Generator().manual_seed(22)
    X, Y = torch.rand(2, 3, 24, 24, generator=gen, dtype=torch.float64), torch.rand(2, 3, 24, 24, generator=gen, dtype=torch.float64)
    window = tuple(S.gaussian_window().tolist())

    def grads(use):
        x, y = X.clone(), Y.clone().requires_grad_(True)
        s, cs = S._SsimPairKernel.apply(x, y, window, 1e-4, 9e-4)
        sum(v.sum() for v, u in ((s, use[0]), (cs, use[1])) if u).backward()
        yr = Y.clone().requires_grad_(True)
        sr, csr = S.ssim_pair_torch(X, yr, S.gaussian_window(), 1e-4, 9e-4)
        sum(v.sum() for v, u in ((sr, use[0]), (csr, use[1])) if u).backward()
        assert (y.grad - yr.grad).abs().max() < 1e-14
    grads((True, False)), grads((False, True)), grads((True, True))
    assert seen == [(False, True, False, True), (True, False, False, True), (False, False, False, True)]
