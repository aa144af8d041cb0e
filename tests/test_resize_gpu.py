"""GPU tests of the antialiased resize kernel (csrc/resize.hip through gnerf_hip.resize_aa_forward / _backward and
torch_utils/ops/resize.py), against the float64 restatement of tests/resize_ref.py.

The tolerance is resize_ref.error_bound, per output element: |kernel - restatement| <= gamma * (|W_y| |x| |W_x|^T) + rho with
gamma = (K_y + K_x + 8) * 2^-24 (K: the axis' largest tap count) and rho = 0 for float32 output, 2^-11 |y| + 2^-24 for float16 output;
the backward gets the same bound with the transposed bands.  Test images hold float16-representable values, so float16 and float32 kernels
see exactly the numbers the restatement sees."""

import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_ref as R
from torch_utils.ops import resize as RZ

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2
CHANNELS = (1, 3, 32, 33)            # 32: the 16-byte channel vectors of the hot channels_last tensor; 33: a partial channel tile
LAYOUTS = ('nchw', 'channels_last', 'strided', 'strided_channels_last')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def place(a, layout, dtype, dev):
    """The float64 array `a` [N, C, H, W] as a GPU tensor of `dtype` in `layout`; the strided ones are views into larger tensors (every
    second column, an offset in rows and in channels -- the channels_last view keeps its unit channel stride but loses the 16-byte alignment)."""
    t = torch.from_numpy(a).to(dtype)
    n, c, h, w = t.shape
    if layout == 'nchw':
        return t.to(dev).contiguous()
    if layout == 'channels_last':
        return t.to(dev).contiguous(memory_format=torch.channels_last)
    big = torch.full([n, c + 2, h + 3, 2 * w + 1], float('nan'), dtype=dtype, device=dev)
    if layout == 'strided_channels_last':
        big = big.contiguous(memory_format=torch.channels_last)
    view = big[:, 1:c + 1, 2:h + 2, 1:2 * w + 1:2]
    view.copy_(t.to(dev))
    assert view.shape == t.shape and not view.is_contiguous()
    return view


def check(what, got, ref, bound):
    got = got.detach().double().cpu().numpy()
    assert got.shape == ref.shape, what
    assert np.isfinite(got).all(), what
    ratio = np.abs(got - ref) / np.maximum(bound, 1e-300)
    worst = float(ratio.max())
    print(f'{what}: max error {float(np.abs(got - ref).max()):.3e}, worst error / bound {worst:.3f}')
    assert worst <= 1.0, what


@pytest.mark.parametrize('half', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('mode', ['bilinear', 'bicubic'])
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_kernel_within_the_bound(dev, name, mode, half):
    """Forward and backward of every case, for C in {1, 3, 32, 33} (N = 2) and every layout, within the derived bound."""
    import gnerf_hip
    in_size, out_size, scales = R.case(name)
    Wy, Wx = R.matrices(in_size, out_size, mode, scales)
    dtype = torch.float16 if half else torch.float32
    for c in CHANNELS:
        x, g = R.image(N, c, in_size), R.image(N, c, out_size, seed=7)
        y_ref, dx_ref = R.forward(x, out_size, mode, scales), R.transposed(g, in_size, mode, scales)
        y_bound, dx_bound = R.error_bound(Wy, Wx, x, y_ref, half), R.error_bound(Wy.T, Wx.T, g, dx_ref, half)
        for layout in LAYOUTS:
            tag = f'{name}/{mode}/{"f16" if half else "f32"}/C{c}/{layout}'
            xd, gd = place(x, layout, dtype, dev), place(g, layout, dtype, dev)
            y = gnerf_hip.resize_aa_forward(xd, out_size, mode, scales)
            dx = gnerf_hip.resize_aa_backward(gd, in_size, mode, scales)
            assert y.dtype == dtype and dx.dtype == dtype and y.shape == (N, c, *out_size) and dx.shape == (N, c, *in_size)
            if layout == 'channels_last' and c > 1:
                assert y.is_contiguous(memory_format=torch.channels_last) and dx.is_contiguous(memory_format=torch.channels_last)
            check(tag + ' forward', y, y_ref, y_bound)
            check(tag + ' backward', dx, dx_ref, dx_bound)


def test_hot_shapes_within_the_bound(dev):
    """The three hot tensors at full size (batch 1): more workgroups than one wave of them, 512-pixel coordinates."""
    import gnerf_hip
    for c, in_size, out_size, half, layout in ((32, (64, 64), (128, 128), True, 'channels_last'), (3, (64, 64), (128, 128), False, 'nchw'),
                                               (3, (512, 512), (64, 64), False, 'nchw')):
        Wy, Wx = R.matrices(in_size, out_size)
        x, g = R.image(1, c, in_size), R.image(1, c, out_size, seed=7)
        y_ref, dx_ref = R.forward(x, out_size), R.transposed(g, in_size)
        dtype = torch.float16 if half else torch.float32
        y = gnerf_hip.resize_aa_forward(place(x, layout, dtype, dev), out_size)
        dx = gnerf_hip.resize_aa_backward(place(g, layout, dtype, dev), in_size)
        check(f'hot {in_size}->{out_size} C{c} forward', y, y_ref, R.error_bound(Wy, Wx, x, y_ref, half))
        check(f'hot {in_size}->{out_size} C{c} backward', dx, dx_ref, R.error_bound(Wy.T, Wx.T, g, dx_ref, half))


def test_several_tiles_per_axis():
    """mixed_70x45 needs more than one tile along both axes of both directions whatever the tile: the source caps a tile at kMaxTile."""
    src = open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'resize.hip')).read()
    tile = int(re.search(r'constexpr int kMaxTile = (\d+);', src).group(1))
    in_size, out_size, _ = R.case('mixed_70x45')
    assert min(in_size) > tile and min(out_size) > tile


@pytest.mark.parametrize('mode', ['bilinear', 'bicubic'])
def test_adjoint_identity(dev, mode):
    """<A x, g> = <x, A^T g> for the two kernels in float32, to 1e-5 of the product of the norms.  Each side is off by at most
    gamma || |A| |x| || ||g|| <= gamma || |A| || ||x|| ||g||, so the two differ by at most 2 gamma || |A| ||; with gamma =
    (17 + 17 + 8) * 2^-24 = 2.5e-6 at K <= 17 and || |A| || <= 2 that is 1e-5.  The cases with more taps average more (|| |A| || < 1): the
    test evaluates 2 gamma || |W_y| || || |W_x| || for every case and finds it below 1e-5 before it holds the kernels to 1e-5."""
    import gnerf_hip
    for name in sorted(R.CASES):
        in_size, out_size, scales = R.case(name)
        Wy, Wx = R.matrices(in_size, out_size, mode, scales)
        derived = 2 * (R.taps(Wy) + R.taps(Wx) + 8) * R.U32 * np.linalg.norm(np.abs(Wy), 2) * np.linalg.norm(np.abs(Wx), 2)
        assert derived <= 1e-5, (name, derived)
        x, g = R.image(N, 3, in_size), R.image(N, 3, out_size, seed=7)
        xd, gd = place(x, 'nchw', torch.float32, dev), place(g, 'nchw', torch.float32, dev)
        Ax = gnerf_hip.resize_aa_forward(xd, out_size, mode, scales).double().cpu().numpy()
        ATg = gnerf_hip.resize_aa_backward(gd, in_size, mode, scales).double().cpu().numpy()
        lhs, rhs = float((Ax * g).sum()), float((x * ATg).sum())
        tol = 1e-5 * float(np.linalg.norm(x)) * float(np.linalg.norm(g))
        print(f'{name}/{mode}: <Ax, g> = {lhs:.9e}, <x, ATg> = {rhs:.9e}, difference {abs(lhs - rhs):.3e}, tolerance {tol:.3e}')
        assert abs(lhs - rhs) <= tol, name


@pytest.mark.parametrize('half', [False, True], ids=['f32', 'f16'])
def test_double_backward(dev, half):
    """autograd.grad(create_graph=True), then a second gradient: d <A^T g, v> / dg = A v, the forward operator applied to the cotangent."""
    dtype = torch.float16 if half else torch.float32
    for name, mode in (('up2_5x7', 'bilinear'), ('frac_down_17x13', 'bicubic'), ('scale_factor_20x30', 'bilinear')):
        in_size, size, scale_factor = R.CASES[name]
        _, out_size, scales = R.case(name)
        Wy, Wx = R.matrices(in_size, out_size, mode, scales)
        x = place(R.image(N, 3, in_size), 'nchw', dtype, dev).requires_grad_(True)
        g = place(R.image(N, 3, out_size, seed=7), 'nchw', dtype, dev).requires_grad_(True)
        v = R.image(N, 3, in_size, seed=9)
        y = RZ.interpolate_aa(x, size=size, scale_factor=scale_factor, mode=mode)
        dx, = torch.autograd.grad(y, x, g, create_graph=True)
        assert dx.requires_grad
        dg, = torch.autograd.grad(dx, g, place(v, 'nchw', dtype, dev))
        ref = R.forward(v, out_size, mode, scales)
        check(f'{name}/{mode} double backward', dg, ref, R.error_bound(Wy, Wx, v, ref, half))
        # and the first order pieces it was built from
        y_ref = R.forward(x.detach().double().cpu().numpy(), out_size, mode, scales)
        check(f'{name}/{mode} op forward', y, y_ref, R.error_bound(Wy, Wx, x.detach().double().cpu().numpy(), y_ref, half))
        gn = g.detach().double().cpu().numpy()
        dx_ref = R.transposed(gn, in_size, mode, scales)
        check(f'{name}/{mode} op backward', dx, dx_ref, R.error_bound(Wy.T, Wx.T, gn, dx_ref, half))


def test_r1_style_penalty_runs_through_the_op(dev):
    """R1: the squared gradient of a function of the resized image, differentiated again, against float64 autograd of the PyTorch op."""
    x = place(R.image(N, 3, (17, 13)), 'nchw', torch.float32, dev).requires_grad_(True)
    d1, = torch.autograd.grad(RZ.interpolate_aa(x, size=(5, 7)).square().sum(), x, create_graph=True)
    d1.square().sum().backward()
    xr = x.detach().double().cpu().requires_grad_(True)
    r1, = torch.autograd.grad(F.interpolate(xr, size=(5, 7), mode='bilinear', align_corners=False, antialias=True).square().sum(), xr, create_graph=True)
    r1.square().sum().backward()
    assert float((x.grad.double().cpu() - xr.grad).abs().max()) <= 1e-5 * float(xr.grad.abs().max())


def both(x, g, in_size, out_size, mode='bilinear', scales=(None, None)):
    import gnerf_hip
    return gnerf_hip.resize_aa_forward(x, out_size, mode, scales), gnerf_hip.resize_aa_backward(g, in_size, mode, scales)


@pytest.mark.parametrize('half', [False, True], ids=['f32', 'f16'])
def test_bit_identity(dev, monkeypatch, half):
    """Reruns; the ctypes binding against the extension; NCHW against channels_last; an item alone against the same item in a batch of 3."""
    import gnerf_hip
    dtype = torch.float16 if half else torch.float32
    assert gnerf_hip.ext() is not None, 'gnerf_torch_ext.so is not built'
    for name, mode, c in (('up2_8x8', 'bilinear', 32), ('mixed_70x45', 'bicubic', 3), ('down8_40x24', 'bilinear', 33), ('scale_factor_20x30', 'bicubic', 8)):
        in_size, out_size, scales = R.case(name)
        x, g = R.image(3, c, in_size), R.image(3, c, out_size, seed=7)
        xd, gd = place(x, 'nchw', dtype, dev), place(g, 'nchw', dtype, dev)
        first = both(xd, gd, in_size, out_size, mode, scales)
        again = both(xd, gd, in_size, out_size, mode, scales)
        assert all(torch.equal(a, b) for a, b in zip(first, again)), name
        with monkeypatch.context() as m:
            m.setattr(gnerf_hip._native, 'ext', lambda: None)
            through_ctypes = both(xd, gd, in_size, out_size, mode, scales)
        assert all(torch.equal(a, b) and a.stride() == b.stride() for a, b in zip(first, through_ctypes)), name
        for layout in ('channels_last', 'strided', 'strided_channels_last'):
            other = both(place(x, layout, dtype, dev), place(g, layout, dtype, dev), in_size, out_size, mode, scales)
            assert all(torch.equal(a, b.contiguous()) for a, b in zip(first, other)), (name, layout)
        alone = both(xd[1:2], gd[1:2], in_size, out_size, mode, scales)
        assert all(torch.equal(a[1:2], b) for a, b in zip(first, alone)), name


def test_graph_capture_of_a_first_call_equals_eager(dev):
    """No table, no cache, no attribute to set per shape: a shape the process has never resized is captured, replayed and equals eager."""
    import gnerf_hip
    in_size, out_size = (23, 19), (11, 29)                           # used nowhere else in this module
    xd = place(R.image(N, 8, in_size), 'channels_last', torch.float16, dev)
    gd = place(R.image(N, 8, out_size, seed=7), 'channels_last', torch.float16, dev)
    warm = place(R.image(1, 8, (6, 6)), 'channels_last', torch.float16, dev)
    both(warm, warm, (6, 6), (6, 6))                                 # the library and its code object are loaded; the shape below is new
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = both(xd, gd, in_size, out_size, 'bicubic')
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = both(xd, gd, in_size, out_size, 'bicubic')
    assert all(torch.equal(a, b) for a, b in zip(eager, captured))
    xd.copy_(place(R.image(N, 8, in_size, seed=3), 'channels_last', torch.float16, dev))          # the replay reads the input where it was
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured[0], gnerf_hip.resize_aa_forward(xd, out_size, 'bicubic'))


@pytest.mark.parametrize('binding', ['ext', 'ctypes'])
def test_refusals_and_fallbacks(dev, monkeypatch, binding):
    import gnerf_hip
    if binding == 'ctypes':
        monkeypatch.setattr(gnerf_hip._native, 'ext', lambda: None)
    monkeypatch.setattr(RZ, '_warned_fallbacks', set())
    for in_size, out_size in (((200, 8), (3, 8)), ((8, 3), (8, 200))):
        x, g = torch.rand(1, 2, *in_size, device=dev), torch.rand(1, 2, *out_size, device=dev)
        assert not gnerf_hip.resize_aa_supported(x.shape, out_size)
        for call in (lambda: gnerf_hip.resize_aa_forward(x, out_size), lambda: gnerf_hip.resize_aa_backward(g, in_size)):
            with pytest.raises(gnerf_hip.NativeError) as info:
                call()
            assert info.value.code == gnerf_hip.E_UNSUPPORTED
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            xg = x.clone().requires_grad_(True)
            y = RZ.interpolate_aa(xg, size=out_size)
            y.backward(g)
        assert torch.equal(y.detach(), F.interpolate(x, size=out_size, mode='bilinear', align_corners=False, antialias=True))
        ref = R.transposed(g.double().cpu().numpy(), in_size)
        assert np.abs(xg.grad.double().cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()      # (ATen's float32 kernel: its own accuracy)
    # the band limit itself is covered: scale 32 and 1 / 32 run on the kernel, within the bound
    x = R.image(1, 2, (160, 96))
    y_ref = R.forward(x, (5, 3))
    Wy, Wx = R.matrices((160, 96), (5, 3))
    assert R.taps(Wy) >= 63
    check('scale 32', gnerf_hip.resize_aa_forward(place(x, 'nchw', torch.float32, dev), (5, 3)), y_ref, R.error_bound(Wy, Wx, x, y_ref, False))
    g = R.image(1, 2, (160, 96), seed=7)                             # the backward of (5, 3) -> (160, 96) gathers up to 65 outputs per input
    dx_ref = R.transposed(g, (5, 3))
    Uy, Ux = R.matrices((5, 3), (160, 96))
    assert R.taps(Uy.T) >= 63
    check('scale 1/32 transposed', gnerf_hip.resize_aa_backward(place(g, 'nchw', torch.float32, dev), (5, 3)), dx_ref,
          R.error_bound(Uy.T, Ux.T, g, dx_ref, False))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        for _ in range(2):
            x64 = torch.rand(1, 2, 8, 8, device=dev, dtype=torch.float64)
            y64 = RZ.interpolate_aa(x64, size=(4, 4))
            RZ.interpolate_aa(torch.rand(1, 1, 200, 8, device=dev), size=(3, 8))
    assert y64.dtype == torch.float64 and torch.equal(y64, F.interpolate(x64, size=(4, 4), mode='bilinear', align_corners=False, antialias=True))
    messages = [str(w.message) for w in caught if issubclass(w.category, RuntimeWarning) and 'interpolate_aa' in str(w.message)]
    assert len(messages) == 1 and 'float64' in messages[0], messages  # the band's warning was given above, once


def _probe():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import resize_sr_probe
    finally:
        sys.path.pop(0)
    return resize_sr_probe


def test_superresolution_runs_the_kernel_and_is_no_further_from_float32(dev, tmp_path, monkeypatch):
    """One forward + backward of SuperRes8XDC (default sizes, batch 1) under torch.profiler shows no `_upsample_bilinear2d_aa` op; with
    GNERF_RESIZE_AA=0, in a fresh process, it shows the forward and the backward op.  Both fp16 runs are measured against the float32 form
    of the same module (relative L2, output image and input gradients): the kernel route may be at most twice as far from it as the torch
    route, and the two routes differ from each other by no more than their two distances add up to."""
    P = _probe()
    monkeypatch.delenv('GNERF_RESIZE_AA', raising=False)
    kernel = P.run(False, dev)
    assert kernel['aa_ops'] == [] and 'gnerf_hip::resize_aa_forward' in kernel['kernel_ops'] and 'gnerf_hip::resize_aa_backward' in kernel['kernel_ops']
    env = dict(os.environ, GNERF_RESIZE_AA='0')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'resize_sr_probe.py'), '--out', str(tmp_path / 'torch.pt'), '--fp32-out',
                          str(tmp_path / 'fp32.pt')], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    torch_route, fp32 = torch.load(tmp_path / 'torch.pt'), torch.load(tmp_path / 'fp32.pt')
    assert any(n.endswith('_upsample_bilinear2d_aa') for n in torch_route['aa_ops']), torch_route['aa_ops']
    assert any(n.endswith('_upsample_bilinear2d_aa_backward') for n in torch_route['aa_ops']), torch_route['aa_ops']
    assert torch_route['kernel_ops'] == []
    d = P.distances(kernel, torch_route, fp32)
    print('distances from the float32 form:', d)
    for key in ('out', 'grads'):
        assert d['kernel'][key] <= 2.0 * d['torch'][key], (key, d)
        assert d['kernel_vs_torch'][key] <= (d['kernel'][key] + d['torch'][key]) * (1 + 1e-6), (key, d)
    assert d['torch']['grads'] < 0.05 and d['torch']['out'] < 0.05   # the yardstick is one: the fp16 module is the float32 module to fp16's noise
