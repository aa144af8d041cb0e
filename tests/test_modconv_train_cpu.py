"""CPU tests of the differentiable modulated-convolution surroundings (torch_utils/ops/modconv.py) and of what the training route leaves alone.

The yardstick of this file and of tests/test_modconv_train_gpu.py is `epilogue64` / `scale64` below: a float64 restatement of the un-fused
modulated convolution's elementwise steps (networks_stylegan2.py:76-86: `x * styles`, then `fma(x, dcoefs, noise)`) and of bias_act (add the
bias, leaky ReLU or nothing, gain, clamp), differentiated by float64 autograd."""

import ctypes
import os
import re

import pytest
import torch

from torch_utils.ops import modconv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scale64(x, scale):
    return x * scale[:, :, None, None]


def epilogue64(x, scale=None, noise=None, bias=None, act='lrelu', alpha=0.2, gain=1.0, clamp=None):
    """-> (y, pre-activation u), both float64."""
    u = x
    if scale is not None:
        u = u * scale[:, :, None, None]
    if noise is not None:
        u = u + noise
    if bias is not None:
        u = u + bias[None, :, None, None]
    y = torch.where(u > 0, u, u * alpha) if act == 'lrelu' else u
    y = y * gain
    if clamp is not None:
        y = torch.minimum(torch.maximum(y, torch.full_like(y, -clamp)), torch.full_like(y, clamp))
    return y, u


def make_case(shape, dtype, noise_kind, use_scale, use_bias, use_clamp, act, seed=0, gain=1.25):
    """Operands representable in `dtype` (so every form sees the same numbers) -> dict of CPU tensors in `dtype` (scale float32) plus the
    upstream gradient dy and the clamp.  The clamp cuts about 10 % of the elements; x is moved where the float64 pre-activation (or the value
    in front of the clamp) would lie within `margin` of a decision, and the caller asserts that none is left there."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed + 1000 * c + h)
    rnd = lambda *s: torch.randn(*s, generator=g)
    q = lambda t: t.to(dtype).to(torch.float64)
    x = q(rnd(n, c, h, w))
    scale = q(0.5 + torch.rand(n, c, generator=g)) if use_scale else None
    noise = None if noise_kind == 'none' else q(0.5 * (rnd(h, w) if noise_kind == 'plane' else rnd(n, 1, h, w)))
    bias = q(0.3 * rnd(c)) if use_bias else None
    dy = q(rnd(n, c, h, w))
    margin = 2e-2 if dtype == torch.float16 else 1e-4
    y, u = epilogue64(x, scale, noise, bias, act, 0.2, gain, None)
    clamp = None
    if use_clamp:
        clamp = max(round(float(y.abs().flatten().kthvalue(int(0.9 * y.numel())).values) * 8) / 8, 0.125)
    for _ in range(4):                                  # the fixed offset: +0.25 on x wherever a decision is closer than the margin
        y, u = epilogue64(x, scale, noise, bias, act, 0.2, gain, None)
        bad = u.abs() < margin
        if clamp is not None:
            bad |= (y.abs() - clamp).abs() < margin
        if not bad.any():
            break
        x = torch.where(bad, q(x + 0.25), x)
    cast = lambda t, d=dtype: None if t is None else t.to(d)
    return dict(x=cast(x), scale=cast(scale, torch.float32), noise=cast(noise, torch.float32), bias=cast(bias), dy=cast(dy), act=act, alpha=0.2, gain=gain,
                clamp=clamp, margin=margin)


def assert_decisions_clear(case):
    """No float64 pre-activation within the margin of 0, no clamped value within it of +-clamp: a mask flip cannot be blamed on the yardstick."""
    d = lambda t: None if t is None else t.double()
    y, u = epilogue64(d(case['x']), d(case['scale']), d(case['noise']), d(case['bias']), case['act'], case['alpha'], case['gain'], None)
    assert float(u.abs().min()) >= case['margin']
    if case['clamp'] is not None:
        assert float((y.abs() - case['clamp']).abs().min()) >= case['margin']
        cut = float((y.abs() > case['clamp']).double().mean())
        assert 0.03 <= cut <= 0.2, cut


def grads_of(fn, case, dtype=None, device=None, memory_format=torch.contiguous_format):
    """(y, dx, dscale, dnoise, dbias) of fn(x, scale, noise, bias, act=..) for the upstream gradient dy; operands cast to `dtype`
    (None: as they are) on `device`."""
    def leaf(t, keep_dtype=False):
        if t is None:
            return None
        t = t.to(device=device, dtype=None if keep_dtype and dtype != torch.float64 else dtype)
        if t.ndim == 4 and t.shape[1] > 1:
            t = t.contiguous(memory_format=memory_format)
        return t.detach().requires_grad_(True)
    x, scale, noise, bias = leaf(case['x']), leaf(case['scale'], True), leaf(case['noise'], True), leaf(case['bias'])
    y = fn(x, scale, noise, bias, act=case['act'], alpha=case['alpha'], gain=case['gain'], clamp=case['clamp'])
    y = y[0] if isinstance(y, tuple) else y
    ins = [t for t in (x, scale, noise, bias) if t is not None]
    got = iter(torch.autograd.grad(y, ins, case['dy'].to(device=y.device, dtype=y.dtype)))
    return (y.detach(),) + tuple(None if t is None else next(got) for t in (x, scale, noise, bias))


@pytest.mark.parametrize('act', ['lrelu', 'linear'])
@pytest.mark.parametrize('noise_kind', ['none', 'plane', 'item'])
def test_op_forms_equal_float64_restatement(noise_kind, act):
    for use_scale, use_bias, use_clamp in ((True, True, True), (False, False, False), (True, False, True), (False, True, False)):
        case = make_case((2, 5, 7, 9), torch.float32, noise_kind, use_scale, use_bias, use_clamp, act)
        assert_decisions_clear(case)
        ref = grads_of(epilogue64, case, torch.float64)
        got = grads_of(modconv.epilogue, case, torch.float64)
        for a, b in zip(got, ref):
            assert (a is None) == (b is None)
            if a is not None:
                assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12
    x = torch.randn(2, 5, 7, 9, dtype=torch.float64, requires_grad=True)
    s = torch.rand(2, 5, dtype=torch.float64, requires_grad=True)
    assert torch.equal(modconv.scale_channels(x, s), scale64(x, s))


def test_gradcheck_float64():
    case = make_case((2, 3, 4, 5), torch.float32, 'item', True, True, True, 'lrelu')
    assert_decisions_clear(case)
    d = lambda t: t.double().requires_grad_(True)
    x, scale, noise, bias = d(case['x']), d(case['scale']), d(case['noise']), d(case['bias'])
    for act in ('lrelu', 'linear'):
        assert torch.autograd.gradcheck(lambda *a: modconv.epilogue(*a, act=act, gain=case['gain'], clamp=case['clamp']), (x, scale, noise, bias), eps=1e-6)
    assert torch.autograd.gradcheck(modconv.scale_channels, (x, scale))
    # CPU tensors: the PyTorch-op composition, differentiable twice
    gx, = torch.autograd.grad(modconv.scale_channels(x, scale).square().sum(), x, create_graph=True)
    gx.sum().backward()
    assert scale.grad is not None


def test_prototypes_in_header_and_ctypes_table():
    import gnerf_hip
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    assert '#define GNERF_ABI_VERSION 15' in header and gnerf_hip.ABI_VERSION == 15
    i, p, f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    expected = {
        'gnerf_modconv_backward_workspace_bytes': (i, [i, i, i, i, i, ctypes.POINTER(ctypes.c_size_t)]),
        'gnerf_scale_channels_backward': (i, [p, p, p, i, i, i, i, p, p, p, p]),
        'gnerf_scale_channels_backward_nhwc': (i, [p, p, p, i, i, i, i, p, p, p, p]),
        'gnerf_modconv_epilogue_backward': (i, [p, p, p, p, i, i, i, i, i, i, f, f, f, p, p, p, p, p, p]),
        'gnerf_modconv_epilogue_backward_nhwc': (i, [p, p, p, p, i, i, i, i, i, i, f, f, f, p, p, p, p, p, p]),
    }
    for name, sig in expected.items():
        assert gnerf_hip.SIGNATURES[name] == sig, name
        assert name in gnerf_hip.OPTIONAL_SYMBOLS
        args = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header).group(1)
        assert len(args.split(',')) == len(sig[1]), name
    assert gnerf_hip.modconv_backward_available()              # found by symbol in the library build() made
    src = open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'torch_binding.cpp')).read()
    for name in expected:
        assert name in src, f'{name} is not called from torch_binding.cpp'


def test_cpu_routes_unchanged(monkeypatch):
    import gnerf_generator as G
    assert G._MODCONV_TRAIN is True
    torch.manual_seed(0)
    layer, rgb = G.StyledConv(8, 8, 16, 8), G.ToRGB(8, 3, 16)
    x, w = torch.randn(2, 8, 8, 8, requires_grad=True), torch.randn(2, 16)
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            assert layer.route(x, w, 'const', fused=False) == '_reference_unfused' and layer.route(x, w, 'const', fused=True) == '_reference_fused'
            assert rgb.route(x, w, fused=False) == '_reference_unfused' and rgb.route(x, w, fused=True) == '_reference_fused'
    assert hasattr(G.StyledConv, '_train') and hasattr(G.ToRGB, '_train')
    y = layer(x, w, 'const', fused=False)
    y.sum().backward()
    assert x.grad is not None and layer.noise_strength.grad is not None
