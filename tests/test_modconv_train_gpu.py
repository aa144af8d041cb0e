"""GPU tests of the backward kernels of csrc/modconv.hip (through torch_utils/ops/modconv.py) and of the `_train` route of the generator's layers.

Yardstick: the float64 restatement in tests/test_modconv_train_cpu.py (epilogue64 / scale64), differentiated by float64 autograd on the CPU;
for the layers, the layer itself in float64 on the CPU (its `_reference_unfused`).

Tolerance rule (the one of tests/test_ssim_gpu.py): the kernel form's error against float64 may be at most TWICE the error of the same-dtype
composed PyTorch-op form on the same inputs, with a floor of 8 ulp of the result's dtype times the tensor's largest magnitude (the factor and the
floor cover another summation order and the one rounding of the output format).  Both errors are printed.  The op-level inputs are chosen so that
no float64 pre-activation lies within a margin (1e-4 for float32, 2e-2 for float16: far more than the format's rounding of the operands' sum) of
0 or of +-clamp, which is asserted, and the clamp cuts about 10 % of the elements."""

import itertools

import pytest
import torch

from test_modconv_train_cpu import assert_decisions_clear, epilogue64, grads_of, make_case, scale64
from torch_utils.ops import modconv

pytestmark = pytest.mark.gpu

ULPS = 8
EPS = {torch.float32: 2.0 ** -23, torch.float16: 2.0 ** -11, torch.float64: 2.0 ** -52}
# (shape, dtype, memory format): odd sizes and tails; a channel count that fills no power of two of vectors; reductions over several workgroups
COMBOS = {
    'odd_f32_nchw': ((2, 5, 7, 9), torch.float32, torch.contiguous_format),
    'c24_f16_nhwc': ((3, 24, 6, 10), torch.float16, torch.channels_last),
    'big_f32_nchw': ((2, 16, 64, 64), torch.float32, torch.contiguous_format),
    'big_f16_nhwc': ((2, 16, 64, 64), torch.float16, torch.channels_last),
}
NAMES = ('y', 'dx', 'dscale', 'dnoise', 'dbias')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def check(what, got, ref, op, dtype=None):
    """got (kernel form) and op (same-dtype PyTorch-op form) against ref (float64)."""
    dtype = dtype or got.dtype
    ref = ref.double().cpu()
    err = float((got.detach().double().cpu() - ref).abs().max())
    err_op = float((op.detach().double().cpu() - ref).abs().max())
    floor = ULPS * EPS[dtype] * float(ref.abs().max())
    tol = max(2 * err_op, floor)
    print(f'{what}: kernel form {err:.3e}, op form {err_op:.3e}, floor {floor:.3e}, tolerance {tol:.3e}')
    assert got.shape == ref.shape and err <= tol, what


_case_refs = {}


def case_refs(combo, noise_kind, act, flags):
    """The case, its float64 results and the same-dtype op form's (on the CPU), computed once."""
    key = (combo, noise_kind, act, flags)
    if key not in _case_refs:
        shape, dtype, _ = COMBOS[combo]
        case = make_case(shape, dtype, noise_kind, *flags, act)
        assert_decisions_clear(case)
        _case_refs[key] = (case, grads_of(epilogue64, case, torch.float64), grads_of(modconv.epilogue_torch, case))
    return _case_refs[key]


@pytest.mark.parametrize('act', ['lrelu', 'linear'])
@pytest.mark.parametrize('noise_kind', ['none', 'plane', 'item'])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_epilogue_matches_float64(dev, combo, noise_kind, act):
    _, dtype, mf = COMBOS[combo]
    for flags in itertools.product((True, False), repeat=3):          # with and without scale, bias, clamp
        case, ref, op = case_refs(combo, noise_kind, act, flags)
        got = grads_of(modconv.epilogue, case, device=dev, memory_format=mf)
        assert got[0].dtype == dtype and got[1].dtype == dtype and got[1].stride() == got[0].stride()
        assert torch.equal(got[0], _plain_forward(case, dev, mf)), 'the forward is gnerf_hip.modconv_epilogue, bit for bit'
        for name, g, r, o in zip(NAMES, got, ref, op):
            assert (g is None) == (r is None)
            if g is not None:
                check(f'{combo}/{noise_kind}/{act}/scale,bias,clamp={flags} {name}', g, r, o, dtype if name in ('y', 'dx', 'dbias') else torch.float32)


def _plain_forward(case, dev, mf):
    import gnerf_hip
    to = lambda t: None if t is None else t.to(dev)
    return gnerf_hip.modconv_epilogue(case['x'].to(dev).contiguous(memory_format=mf), to(case['bias']), scale=to(case['scale']), noise=to(case['noise']),
                                      round_noise=True, act=case['act'], alpha=case['alpha'], gain=case['gain'], clamp=case['clamp'])


@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_scale_channels_matches_float64(dev, combo):
    shape, dtype, mf = COMBOS[combo]
    case = make_case(shape, dtype, 'none', True, False, False, 'linear', seed=7)

    def run(fn, dt=None, device=None):
        x = case['x'].to(device=device, dtype=dt)
        x = (x.contiguous(memory_format=mf) if device is not None else x).detach().requires_grad_(True)
        s = case['scale'].to(device=device, dtype=torch.float64 if dt == torch.float64 else None).detach().requires_grad_(True)
        y = fn(x, s)
        return (y.detach(),) + torch.autograd.grad(y, (x, s), case['dy'].to(device=device, dtype=y.dtype))
    ref, op, got = run(scale64, torch.float64), run(modconv.scale_channels_torch), run(modconv.scale_channels, device=dev)
    import gnerf_hip
    assert torch.equal(got[0], gnerf_hip.scale_channels(case['x'].to(dev).contiguous(memory_format=mf), case['scale'].to(dev)))
    assert got[1].dtype == dtype and got[1].stride() == got[0].stride() and got[2].dtype == torch.float32
    for name, g, r, o in zip(('y', 'dx', 'dscale'), got, ref, op):
        check(f'{combo} scale_channels {name}', g, r, o, torch.float32 if name == 'dscale' else dtype)


def _leaves(case, dev, mf, needs):
    out = []
    for name, need in zip(('x', 'scale', 'noise', 'bias'), needs):
        t = case[name].to(dev)
        t = t.contiguous(memory_format=mf) if t.ndim == 4 and t.shape[1] > 1 else t
        out.append(t.detach().requires_grad_(need))
    return out


@pytest.mark.parametrize('combo', ['odd_f32_nchw', 'c24_f16_nhwc'])
def test_unneeded_gradients_are_skipped(dev, combo):
    shape, dtype, mf = COMBOS[combo]
    case, ref, op = case_refs(combo, 'plane', 'lrelu', (True, True, True))
    for needs in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True), (False, True, True, False)):
        x, scale, noise, bias = _leaves(case, dev, mf, needs)
        y = modconv.epilogue(x, scale, noise, bias, act='lrelu', alpha=0.2, gain=case['gain'], clamp=case['clamp'])
        y.backward(case['dy'].to(dev))
        for i, (t, need) in enumerate(zip((x, scale, noise, bias), needs)):
            assert (t.grad is not None) == need
            if need:
                check(f'{combo} needs={needs} {NAMES[i + 1]}', t.grad, ref[i + 1], op[i + 1], dtype if i in (0, 3) else torch.float32)
    x, scale = _leaves(case, dev, mf, (False, True, False, False))[:2]
    modconv.scale_channels(x, scale).backward(case['dy'].to(dev))
    assert x.grad is None and scale.grad is not None


def test_ctypes_binding_agrees(dev, monkeypatch):
    import gnerf_hip
    assert gnerf_hip.ext() is not None, 'gnerf_torch_ext.so is not built'
    for combo in ('odd_f32_nchw', 'big_f16_nhwc'):
        _, _, mf = COMBOS[combo]
        case, _, _ = case_refs(combo, 'item', 'lrelu', (True, True, True))
        a = grads_of(modconv.epilogue, case, device=dev, memory_format=mf)
        with monkeypatch.context() as m:
            m.setattr(gnerf_hip._native, 'ext', lambda: None)
            b = grads_of(modconv.epilogue, case, device=dev, memory_format=mf)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize('combo', ['big_f32_nchw', 'big_f16_nhwc'])
def test_backward_is_bit_reproducible_and_batch_independent(dev, combo):
    _, dtype, mf = COMBOS[combo]
    case, _, _ = case_refs(combo, 'plane', 'lrelu', (True, True, True))
    a = grads_of(modconv.epilogue, case, device=dev, memory_format=mf)
    b = grads_of(modconv.epilogue, case, device=dev, memory_format=mf)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    # item 1 alone: its dx and dscale are those it has inside the batch
    one = dict(case, x=case['x'][1:], scale=case['scale'][1:], dy=case['dy'][1:])
    c = grads_of(modconv.epilogue, one, device=dev, memory_format=mf)
    assert torch.equal(c[1], a[1][1:]) and torch.equal(c[2], a[2][1:])
    x, s = case['x'].to(dev).contiguous(memory_format=mf), case['scale'].to(dev)
    dy = case['dy'].to(dev).contiguous(memory_format=mf)
    import gnerf_hip
    full, alone = gnerf_hip.scale_channels_backward(dy, x, s), gnerf_hip.scale_channels_backward(dy[1:], x[1:], s[1:])
    again = gnerf_hip.scale_channels_backward(dy, x, s)
    assert torch.equal(full[0], again[0]) and torch.equal(full[1], again[1])
    assert torch.equal(alone[0], full[0][1:]) and torch.equal(alone[1], full[1][1:])


def test_double_backward_raises(dev):
    case, _, _ = case_refs('odd_f32_nchw', 'plane', 'lrelu', (True, True, True))
    x, scale, noise, bias = _leaves(case, dev, torch.contiguous_format, (True, True, True, True))
    with pytest.raises(RuntimeError, match='once_differentiable'):
        y = modconv.epilogue(x, scale, noise, bias, gain=case['gain'], clamp=case['clamp'])
        gx, = torch.autograd.grad(y.square().sum(), x, create_graph=True)
        gx.square().sum().backward()
    with pytest.raises(RuntimeError, match='once_differentiable'):
        gx, = torch.autograd.grad(modconv.scale_channels(x, scale).square().sum(), x, create_graph=True)
        gx.square().sum().backward()


# ---------------------------------------------------------------------------------------------------------------- the layers

def _layer_grads(layer, x, w, device, dtype, mf, **kw):
    """(y, dx, dw, parameter gradients by name) of sum(layer(x, w) * upstream) with the layer's parameters on `device` (float64: as double)."""
    import copy
    layer = copy.deepcopy(layer).to(device)
    if dtype == torch.float64:
        layer = layer.double()
        if hasattr(layer, 'resample_filter'):
            layer.resample_filter = layer.resample_filter.float()          # (the filter stays float32: upfirdn2d casts it itself)
    xd = x.to(device=device, dtype=dtype).contiguous(memory_format=mf).detach().requires_grad_(True)
    wd = w.to(device=device, dtype=torch.float64 if dtype == torch.float64 else torch.float32).detach().requires_grad_(True)
    route = layer.route(xd, wd, 'const', fused=False) if 'noise_mode' in kw else layer.route(xd, wd, fused=False)
    y = layer(xd, wd, fused=False, **kw)
    g = torch.Generator().manual_seed(5)
    up = torch.randn(y.shape, generator=g).to(device=device, dtype=y.dtype)
    names, params = zip(*layer.named_parameters())
    grads = torch.autograd.grad(y, (xd, wd) + params, up)
    return route, dict(zip(('y', 'x', 'w') + names, (y.detach(),) + grads))


@pytest.mark.parametrize('kind', ['conv', 'conv_up2', 'torgb'])
@pytest.mark.parametrize('fmt', ['f32', 'f16_channels_last'])
def test_layer_trains_on_the_kernels(dev, monkeypatch, kind, fmt):
    import gnerf_generator as G
    dtype, mf = (torch.float32, torch.contiguous_format) if fmt == 'f32' else (torch.float16, torch.channels_last)
    torch.manual_seed(3)
    if kind == 'torgb':
        layer, kw = G.ToRGB(16, 3, 32, conv_clamp=2.0), {}
    else:
        up = 2 if kind == 'conv_up2' else 1
        layer, kw = G.StyledConv(16, 16, 32, 16 * up, up=up, conv_clamp=2.0), dict(noise_mode='const')
        with torch.no_grad():
            layer.noise_strength.fill_(0.3)
    with torch.no_grad():
        layer.bias.normal_(0, 0.3)
    x = torch.randn(2, 16, 16, 16).to(dtype).float()
    w = torch.randn(2, 32)
    _, ref = _layer_grads(layer, x, w, 'cpu', torch.float64, torch.contiguous_format, **kw)
    route, got = _layer_grads(layer, x, w, dev, dtype, mf, **kw)
    assert route == '_train'
    monkeypatch.setattr(G, '_MODCONV_TRAIN', False)                   # what GNERF_MODCONV_TRAIN=0 sets
    route_op, op = _layer_grads(layer, x, w, dev, dtype, mf, **kw)
    assert route_op == '_reference_unfused'
    assert set(got) == set(ref) and got['x'].dtype == dtype
    for name in sorted(ref):
        check(f'{kind}/{fmt} {name}', got[name], ref[name], op[name])
