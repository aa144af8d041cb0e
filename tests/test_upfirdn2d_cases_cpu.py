"""Conditions on the inputs of tests/test_upfirdn2d_routes_gpu.py (tests/upfirdn_cases.py), so that its comparisons cannot pass
vacuously: the two references agree, a wrong flip / phase / origin moves most outputs far beyond the tolerance, and the cases
cross the tile seams and the grid cap of the kernels they are meant for.  No GPU."""

import numpy as np
import pytest
import torch

import upfirdn_cases as U

_NAMES = [c.name for c in U.CASES]


def _scale(ref):
    return max(1.0, float(np.abs(ref).max()))


def test_filters_are_not_symmetric():
    for name, f in U.FILTERS.items():
        assert f.dtype == np.float32
        flipped = f[::-1, ::-1] if f.ndim == 2 else f[::-1]
        assert np.abs(f - flipped).max() > 0.1, name
    assert U.FILTERS['f44'].shape == (4, 4) and U.FILTERS['f43'].shape == (4, 3)
    assert [U.FILTERS[k].shape for k in ('f5', 'f8', 'f12')] == [(5,), (8,), (12,)]
    s = U.strided_filter(torch.from_numpy(U.FILTERS['f43'].copy()))
    assert tuple(s.shape) == (4, 3) and s.stride() == (1, 4) and torch.equal(s, torch.from_numpy(U.FILTERS['f43'].copy()))


@pytest.mark.parametrize('name', _NAMES)
def test_references_agree(name):
    """The numpy oracle and the PyTorch-op form, both in float64: same shape, equal to 1e-6 of max |ref| (the PyTorch form multiplies
    f * gain in float32: 8.6e-8 measured at worst).  The public op on CPU tensors IS the PyTorch-op form."""
    from torch_utils.ops import upfirdn2d
    case = U.BY_NAME[name]
    f = torch.from_numpy(U.FILTERS[case.filt].copy())
    worst = 0.0
    for flip in U.FLIPS:
        ref = U.reference(name, flip, 'float64')
        x = torch.from_numpy(U.input64(name, 'float64').copy())
        form = upfirdn2d._upfirdn2d_ref(x, f, **U.kwargs(case, flip))
        assert tuple(form.shape) == ref.shape == U._out_shape(case)
        err = float(np.abs(form.numpy() - ref).max()) / float(np.abs(ref).max())
        worst = max(worst, err)
        assert err <= 1e-6, (name, flip, err)
        assert torch.equal(upfirdn2d.upfirdn2d(x, f, impl='cuda', **U.kwargs(case, flip)), form)
    print(f'{name}: oracle vs PyTorch form, max error / max |ref| = {worst:.2e}')


@pytest.mark.parametrize('name', _NAMES)
def test_cases_discriminate(name):
    """The oracle evaluated with the flip toggled, with the x origin moved by one (x0 + 1, x1 - 1) and with the y origin moved by one
    must each differ from the true reference on more than half of the outputs
      * by more than 100 * tol(fp16) = 100 * 6e-3 = 0.6 -- `tol` as the GPU tests name it, in output units.  (Multiplied by max |ref| as
        well, the bound could be met by no random input: outputs are sums of independent terms, near normal with deviation s, max |ref|
        is about 4 s over these 10^4 outputs, and the difference of two such outputs exceeds 0.6 * 4 s on under a tenth of them.)
      * and by more than the whole error the fp16 comparison allows that output, atol + rtol |ref| with the scale: so the wrong kernel
        fails the widest of the GPU bounds on more than half of the outputs, and the narrower fp32 / fp64 bounds with them."""
    case = U.BY_NAME[name]
    tol = U.TOL['float16']
    x0, x1, y0, y1 = case.padding
    for flip in U.FLIPS:
        ref = U.reference(name, flip, 'float64')
        allowed = tol * _scale(ref) + tol * np.abs(ref)
        others = {'flip toggled': U.reference(name, not flip, 'float64'),
                  'x origin + 1': U.reference(name, flip, 'float64', (x0 + 1, x1 - 1, y0, y1)),
                  'y origin + 1': U.reference(name, flip, 'float64', (x0, x1, y0 + 1, y1 - 1))}
        for what, other in others.items():
            assert other.shape == ref.shape, (name, what)
            d = np.abs(other - ref)
            far, beyond = float((d > 100 * tol).mean()), float((d > allowed).mean())
            print(f'{name} flip={flip} {what}: {far:.3f} of the outputs differ by > {100 * tol}, {beyond:.3f} by more than the fp16 bound')
            assert far > 0.5 and beyond > 0.5, (name, flip, what, far, beyond)


def _tiles(out_hw, tile_wh):
    return -(-out_hw[1] // tile_wh[0]), -(-out_hw[0] // tile_wh[1])            # (in x, in y)


def test_cases_cross_seams():
    """Every fir4 / tile case has >= 2 tiles in x and in y in each dtype it runs on those kernels (fp32, fp16), in every launch of the
    call; the two cases listed as wide-only / tall-only cross on their own axis, and between them both axes are covered."""
    assert {c.seams for c in U.TILE if c.seams != 'xy'} == {'x', 'y'}
    assert all(c.seams == 'xy' for c in U.FIR4)
    for case in U.FIR4 + U.TILE:
        for dtype in ('float32', 'float16'):
            assert U.expected_route(case, dtype, 'nchw') == ('tile' if case in U.TILE else 'fir4')
            tile = U.TILE_TILE if case in U.TILE else U.FIR4_TILE[(case.kind[5:], dtype)]
            for out_hw in U.launches(case):
                tx, ty = _tiles(out_hw, tile)
                assert tx >= 2 or 'x' not in case.seams, (case.name, dtype, out_hw, 'enlarge along x')
                assert ty >= 2 or 'y' not in case.seams, (case.name, dtype, out_hw, 'enlarge along y')
    for case in U.FIR4 + U.TILE:
        f = U.FILTERS[case.filt]
        fir4 = f.shape == (4, 4) and U.xy(case.up)[0] == U.xy(case.up)[1] and U.xy(case.down)[0] == U.xy(case.down)[1] \
            and (U.xy(case.up)[0], U.xy(case.down)[0]) in ((2, 1), (1, 2))
        assert fir4 == (case in U.FIR4), case.name
        assert max(f.shape) <= U.TILE_MAX_TAPS and max(U.xy(case.down)) <= 2, case.name
    for case in U.CASES:
        if case.kind == 'any':
            assert max(U.FILTERS[case.filt].shape) > U.TILE_MAX_TAPS or max(U.xy(case.down)) > 2, case.name


def test_up2_phases():
    seen = set()
    for case in U.CASES:
        if case.kind == 'fir4_up2':
            assert (case.padding[0] % 2, case.padding[2] % 2) == case.phase, case.name
            seen.add(case.phase)
    assert seen == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert [c.phase for c in U.PHASES] == [(0, 0), (1, 0), (0, 1), (1, 1)]


def test_grid_stride_cases_exceed_the_grid():
    for name in ('stride_f64', 'stride_f16_nhwc'):
        case = U.BY_NAME[name]
        (oh, ow), = U.launches(case)
        assert case.shape[0] * case.shape[1] * oh * ow > U.ANY_MAX_LANES, name
        assert all(U.expected_route(case, d, lay) == 'any' for d, lay in U.runs(case))
    assert U.runs(U.BY_NAME['stride_f16_nhwc']) == [('float16', 'nhwc')] and U.BY_NAME['stride_f16_nhwc'].shape[1] > 1
