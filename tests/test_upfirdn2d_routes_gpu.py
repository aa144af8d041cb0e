"""The five kernels behind csrc/upfirdn2d.hip's launch_up, off the diagonal the networks use: every up = 2 phase of the fir4 kernel,
non-symmetric filters in both orientations, several tiles side by side and on top of each other, the any kernel's grid-stride
loop and channels_last index split, filters with exchanged strides -- forward, first- and second-order gradients (the transposed
configuration of torch_utils/ops/upfirdn2d.py) against float64 references, and the kernel each call reaches.

The cases, their expected routes and the references are tests/upfirdn_cases.py's; tests/test_upfirdn2d_cases_cpu.py shows that a
wrong flip, phase or origin moves most outputs of every case beyond the bounds used here."""

import numpy as np
import pytest
import torch

import upfirdn_cases as U
from conftest import has_gpu

pytestmark = pytest.mark.gpu

_DTYPE = {'float32': torch.float32, 'float16': torch.float16, 'float64': torch.float64}
_FLIP_IDS = ['conv', 'flip']


@pytest.fixture(scope='module')
def dev():
    if not has_gpu():
        pytest.fail('GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)')
    import gnerf_hip
    gnerf_hip.load()
    return torch.device('cuda', 0)


def _tensor(a, dtype, dev, layout='nchw'):
    t = torch.from_numpy(a.copy()).to(_DTYPE[dtype]).to(dev)
    return t.contiguous(memory_format=torch.channels_last) if layout == 'nhwc' else t


def _filter(case, dev):
    return torch.from_numpy(U.FILTERS[case.filt].copy()).to(dev)


def _op(case, x, f, flip):
    from torch_utils.ops import upfirdn2d
    return upfirdn2d.upfirdn2d(x, f, **U.kwargs(case, flip))


def _assert_close(got, ref, tol, what):
    """rtol = tol, atol = tol * max(1, max |ref|), as test_upfirdn2d_blur_edge_shapes applies the project's tolerances."""
    got = got.detach().double().cpu().numpy()
    scale = max(1.0, float(np.abs(ref).max()))
    err = np.abs(got - ref)
    print(f'{what}: max error {err.max():.3e}, worst error / bound {(err / (tol * scale + tol * np.abs(ref))).max():.3f}, max |ref| {scale:.3g}')
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * scale, err_msg=str(what))


def _assert_layout(t, layout, what):
    if layout == 'nhwc':
        assert t.is_contiguous(memory_format=torch.channels_last) and t.stride(1) == 1, what
    else:
        assert t.is_contiguous(), what


@pytest.mark.parametrize('flip', U.FLIPS, ids=_FLIP_IDS)
@pytest.mark.parametrize('name,dtype,layout', U.FORWARD_RUNS)
def test_forward_vs_oracle(dev, name, dtype, layout, flip):
    case = U.BY_NAME[name]
    x = _tensor(U.input64(name, dtype), dtype, dev, layout)
    _assert_layout(x, layout, 'input')
    y = _op(case, x, _filter(case, dev), flip)
    ref = U.reference(name, flip, dtype)
    assert y.dtype == _DTYPE[dtype] and tuple(y.shape) == ref.shape
    _assert_layout(y, layout, (name, dtype, layout))
    _assert_close(y, ref, U.TOL[dtype], (name, dtype, layout, flip, U.expected_route(case, dtype, layout)))


_GRAD_RUNS = [(c.name, 'float32') for c in U.FIR4 + U.TILE] + [(c.name, 'float16') for c in U.PHASES]


@pytest.mark.parametrize('flip', U.FLIPS, ids=_FLIP_IDS)
@pytest.mark.parametrize('name,dtype', _GRAD_RUNS)
def test_gradient_vs_float64_autograd(dev, name, dtype, flip):
    """dx of the GPU op (the transposed configuration: up <-> down, filter flipped, all four paddings recomputed) against autograd
    through the PyTorch-op form on float64 CPU tensors; and <op(x), dy> == <x, dx>, which holds whatever the reference says."""
    case = U.BY_NAME[name]
    x = _tensor(U.input64(name, dtype), dtype, dev).requires_grad_(True)
    dy = _tensor(U.cotangent64(name, dtype), dtype, dev)
    y = _op(case, x, _filter(case, dev), flip)
    (dx,) = torch.autograd.grad(y, x, dy)
    assert dx.dtype == x.dtype and dx.shape == x.shape and dx.is_contiguous()
    _assert_close(dx, U.grad_reference(name, flip, dtype), U.TOL[dtype], (name, dtype, flip, 'dx'))
    y64, dy64, x64, dx64 = (t.detach().double() for t in (y, dy, x, dx))
    lhs, rhs = float((y64 * dy64).sum()), float((x64 * dx64).sum())
    bound = U.TOL['float32'] * float(y64.norm()) * float(dy64.norm())
    print(f'{name} {dtype} flip={flip}: <op(x), dy> = {lhs:.9g}, <x, dx> = {rhs:.9g}, difference / bound {abs(lhs - rhs) / bound:.3f}')
    assert abs(lhs - rhs) <= bound, (name, dtype, flip, lhs, rhs, bound)


@pytest.mark.parametrize('flip', U.FLIPS, ids=_FLIP_IDS)
@pytest.mark.parametrize('name', [c.name for c in U.SECOND_ORDER])
def test_second_order_gradient(dev, name, flip):
    """d<dx, w>/d dy with dx built under create_graph: _Resample.backward re-enters _Resample.apply, so the configuration is transposed
    twice and must land back on the forward one (the result is op(w))."""
    case = U.BY_NAME[name]
    dtype = 'float32'
    x = _tensor(U.input64(name, dtype), dtype, dev).requires_grad_(True)
    dy = _tensor(U.cotangent64(name, dtype), dtype, dev).requires_grad_(True)
    w = _tensor(U.weight64(name, dtype), dtype, dev)
    (dx,) = torch.autograd.grad(_op(case, x, _filter(case, dev), flip), x, dy, create_graph=True)
    assert dx.requires_grad
    (g,) = torch.autograd.grad((dx * w).sum(), dy)
    assert g.dtype == dy.dtype and g.shape == dy.shape
    _assert_close(g, U.grad2_reference(name, flip, dtype), U.TOL[dtype], (name, flip, 'd<dx, w>/d dy'))


# one call per route with the filter's strides exchanged
_STRIDED = [('up2_p11', 'float32', 'nchw'), ('down2_0211', 'float16', 'nchw'), ('tile_wide', 'float32', 'nchw'), ('tile_up3_down2', 'float16', 'nchw'),
            ('up2_p10', 'float64', 'nchw'), ('down2_crop', 'float32', 'nhwc'), ('blur', 'float32', 'nchw'), ('blur', 'float16', 'nchw'),
            ('blur', 'float32', 'nhwc'), ('blur', 'float16', 'nhwc')]


def test_strided_cases_cover_every_route():
    assert {U.expected_route(U.BY_NAME[n], d, lay) for n, d, lay in _STRIDED} == set(U.ROUTE_KERNEL)


@pytest.mark.parametrize('flip', U.FLIPS, ids=_FLIP_IDS)
@pytest.mark.parametrize('name,dtype,layout', _STRIDED)
def test_strided_filter_is_bit_identical(dev, name, dtype, layout, flip):
    case = U.BY_NAME[name]
    f = _filter(case, dev)
    fs = U.strided_filter(f)
    assert fs.shape == f.shape and fs.stride() == (1, f.shape[0]) and f.stride() == (f.shape[1], 1) and torch.equal(fs, f)
    x = _tensor(U.input64(name, dtype), dtype, dev, layout)
    assert torch.equal(_op(case, x, fs, flip), _op(case, x, f, flip)), (name, dtype, layout, flip)


def test_routes(dev):
    """Which kernel each kind of call reaches, from the profiler's record of its launches: one representative per expected route of
    tests/upfirdn_cases.py (expected_route), the backward of an up = 2 call, both passes of the separable calls -- and no other upfirdn_
    kernel in the same call.  Names are matched on the function name only, not on template arguments."""
    from torch.profiler import ProfilerActivity, profile
    calls = [('up2_p10', 'float32', 'nchw', 'forward'), ('down2_0211', 'float16', 'nchw', 'forward'), ('up2_p11', 'float32', 'nchw', 'backward'),
             ('tile_sep8_down2', 'float32', 'nchw', 'forward'), ('tile_wide', 'float16', 'nchw', 'forward'),
             ('up2_p00', 'float64', 'nchw', 'forward'), ('up2_p01', 'float32', 'nhwc', 'forward'), ('any_down3', 'float32', 'nchw', 'forward'),
             ('blur', 'float32', 'nchw', 'forward'), ('blur', 'float16', 'nhwc', 'forward')]
    prepared, expected = [], []
    for name, dtype, layout, what in calls:
        case = U.BY_NAME[name]
        x = _tensor(U.input64(name, dtype), dtype, dev, layout)
        f = _filter(case, dev)
        forward = lambda _=None, case=case, x=x, f=f: _op(case, x, f, False)
        if what == 'backward':                      # the transposed configuration of an up = 2 call: a down = 2 call on the same kernel
            x.requires_grad_(True)
            dy = _tensor(U.cotangent64(name, dtype), dtype, dev)
            prepared.append((forward, lambda y, x=x, dy=dy: torch.autograd.grad(y, x, dy)))       # (outside the profile, inside it)
            route = 'fir4'
        else:
            prepared.append((lambda: None, forward))
            route = U.expected_route(case, dtype, layout)
        expected.append([U.ROUTE_KERNEL[route]] * len(U.launches(case)))
    assert {k for ks in expected for k in ks} == set(U.KERNELS)
    assert expected[3] == ['upfirdn_tile_kernel'] * 2 and expected[7] == ['upfirdn_any_kernel'] * 2      # both passes of the separable calls
    for before, run in prepared:                    # warm up
        run(before())
    torch.cuda.synchronize(dev)
    recorded = []
    for before, run in prepared:
        arg = before()
        torch.cuda.synchronize(dev)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            run(arg)
            torch.cuda.synchronize(dev)
        events = sorted((e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'upfirdn_' in e.name),
                        key=lambda e: e.time_range.start)
        seen = []
        for e in events:
            known = [k for k in U.KERNELS if k in e.name]
            assert len(known) == 1, e.name
            seen.append(known[0])
        recorded.append(seen)
    for call, want, got in zip(calls, expected, recorded):
        print(call, '->', got)
    assert recorded == expected, list(zip(calls, expected, recorded))
