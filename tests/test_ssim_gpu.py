"""GPU tests of the fused SSIM kernel (csrc/ssim.hip through gnerf_hip.ssim_forward / ssim_backward and torch_utils/ops/ssim.py).

The tolerance rule of every comparison with float64 here: the kernel's error may be at most TWICE the error of the float32 PyTorch-op form
on the same inputs (computed in the test, on the CPU; the factor covers a different summation order), with a floor of 8 * 2^-23 for values
and 8 * 2^-23 * max |grad| for gradients.  float16 inputs are compared after the same rounding of the inputs (the reference sees the rounded
images); their gradients come back as float16, so each element is additionally allowed half a float16 ulp of the reference value
(2^-11 |g|, and 2^-25 in the subnormal range) -- the rounding of the output format, which no float32 computation has."""

import ctypes
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import ssim_ref
from test_ssim_cpu import cases, pair_and_grads
from torch_utils.ops import ssim as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 8 * 2.0 ** -23


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def upstream(X, scale=1.0):
    g = torch.Generator().manual_seed(X.shape[-1])
    return (torch.rand(X.shape[0], X.shape[1], generator=g) + 0.5) * scale, (torch.rand(X.shape[0], X.shape[1], generator=g) - 0.5) * scale


_refs = {}


def references(name, half):
    """float64 results (values from ssim_ref, gradients from float64 autograd of the op form) and the float32 op form's errors against
    them, for the case's inputs rounded to float32 or float16."""
    key = (name, half)
    if key not in _refs:
        X, Y, L, k = cases()[name]
        X, Y = (X.half(), Y.half()) if half else (X.float(), Y.float())
        gs, gc = upstream(X, 4096.0 if half else 1.0)
        ref_s, ref_cs = ssim_ref.ssim_pair(X.double().numpy(), Y.double().numpy(), L, k)
        r = pair_and_grads(X.double(), Y.double(), L, k, S.ssim_pair_torch, gs, gc)
        assert np.abs(r[0].numpy() - ref_s).max() < 1e-11 and np.abs(r[1].numpy() - ref_cs).max() < 1e-11
        o = pair_and_grads(X.float(), Y.float(), L, k, S.ssim_pair_torch, gs, gc)
        errs = [float((a.double() - b).abs().max()) for a, b in zip(o, r)]
        _refs[key] = (X, Y, L, k, gs, gc, (torch.from_numpy(ref_s), torch.from_numpy(ref_cs), r[2], r[3]), errs)
    return _refs[key]


def check(what, got, ref, err32, half_output=False):
    ref = ref.double()
    got = got.detach().double().cpu()
    scale = float(ref.abs().max()) if ref.ndim == 4 else 1.0
    tol = max(2 * err32, FLOOR * scale)
    diff = (got - ref).abs()
    allowed = torch.full_like(diff, tol)
    if half_output:
        allowed = allowed + ref.abs() * 2.0 ** -11 + 2.0 ** -25
    worst = float((diff / allowed).max())
    print(f'{what}: error {float(diff.max()):.3e}, float32 op form {err32:.3e}, tolerance {tol:.3e} (scale {scale:.3e}), worst error / allowed {worst:.3f}')
    assert worst <= 1.0, what


@pytest.mark.parametrize('binding', ['ext', 'ctypes'])
@pytest.mark.parametrize('half', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('layout', ['nchw', 'channels_last'])
@pytest.mark.parametrize('name', sorted(cases()))
def test_kernel_matches_float64(dev, monkeypatch, name, layout, half, binding):
    import gnerf_hip
    if binding == 'ctypes':
        monkeypatch.setattr(gnerf_hip._native, 'ext', lambda: None)
    else:
        assert gnerf_hip.ext() is not None, 'gnerf_torch_ext.so is not built'
    X, Y, L, k, gs, gc, ref, errs = references(name, half)
    mf = torch.channels_last if layout == 'channels_last' else torch.contiguous_format
    Xd, Yd = X.to(dev).contiguous(memory_format=mf), Y.to(dev).contiguous(memory_format=mf)
    got = pair_and_grads(Xd, Yd, L, k, S.ssim_pair, gs, gc)
    assert got[0].dtype == torch.float32 and got[2].dtype == X.dtype and got[2].stride() == Xd.stride() and got[3].stride() == Yd.stride()
    tag = f'{name}/{layout}/{"f16" if half else "f32"}/{binding}'
    check(tag + ' ssim', got[0], ref[0], errs[0])
    check(tag + ' cs', got[1], ref[1], errs[1])
    check(tag + ' dX', got[2], ref[2], errs[2], half)
    check(tag + ' dY', got[3], ref[3], errs[3], half)


@pytest.mark.parametrize('half', [False, True], ids=['f32', 'f16'])
def test_identical_images(dev, half):
    X = cases(False)['noise_64'][0]
    X = (X.half() if half else X.float()).to(dev)
    s, cs, dX, dY = pair_and_grads(X, X.clone(), 1.0, 11, S.ssim_pair)
    assert float((s - 1).abs().max()) <= FLOOR and float((cs - 1).abs().max()) <= FLOOR
    assert float(dX.abs().max()) <= 1e-9 and float(dY.abs().max()) <= 1e-9


def test_backward_routes(dev):
    """dX only, dY only, g_cs only, g_ssim only and both upstream gradients, against float64 autograd of the op form."""
    import gnerf_hip
    X, Y, L, k, gs, gc, _, _ = references('odd_37x53_win7', False)
    win, C1, C2 = ssim_ref.window(k), (0.01 * L) ** 2, (0.03 * L) ** 2
    Xd, Yd = X.to(dev), Y.to(dev)
    for g1, g2 in ((gs, None), (None, gc), (gs, gc)):
        zero = torch.zeros_like(gs)
        ref = pair_and_grads(X.double(), Y.double(), L, k, S.ssim_pair_torch, zero if g1 is None else g1, g2)
        o32 = pair_and_grads(X, Y, L, k, S.ssim_pair_torch, zero if g1 is None else g1, g2)
        e = [float((a.double() - b).abs().max()) for a, b in zip(o32, ref)]
        up = [None if g is None else g.to(dev) for g in (g1, g2)]
        dX, dY = gnerf_hip.ssim_backward(Xd, Yd, win, C1, C2, *up)
        check('both outputs dX', dX, ref[2], e[2])
        check('both outputs dY', dY, ref[3], e[3])
        only_x = gnerf_hip.ssim_backward(Xd, Yd, win, C1, C2, *up, need_dx=True, need_dy=False)
        only_y = gnerf_hip.ssim_backward(Xd, Yd, win, C1, C2, *up, need_dx=False, need_dy=True)
        assert only_x[1] is None and only_y[0] is None and torch.equal(only_x[0], dX) and torch.equal(only_y[1], dY)
    # through autograd: a gradient for the generated image (Y) alone, as in the training step
    Yg = Yd.clone().requires_grad_(True)
    (1 - S.ssim(Xd, Yg, data_range=L, size_average=False, win_size=k)).sum().backward()
    ref = pair_and_grads(X.double(), Y.double(), L, k, S.ssim_pair_torch, torch.full_like(gs, -1 / 3))
    o32 = pair_and_grads(X, Y, L, k, S.ssim_pair_torch, torch.full_like(gs, -1 / 3))
    check('autograd dY', Yg.grad, ref[3], float((o32[3].double() - ref[3]).abs().max()))
    with pytest.raises(RuntimeError, match='double backward'):
        Yg2 = Yd.clone().requires_grad_(True)
        g, = torch.autograd.grad(S.ssim(Xd, Yg2, data_range=L, win_size=k), Yg2, create_graph=True)
        g.sum().backward()


def test_reproducible_and_independent_of_the_batch(dev):
    import gnerf_hip
    gen = torch.Generator().manual_seed(9)
    for shape in ((4, 3, 512, 512), (4, 3, 64, 64), (4, 2, 45, 70)):
        X, Y = torch.rand(shape, generator=gen).to(dev), torch.rand(shape, generator=gen).to(dev)
        gs, gc = (t.to(dev) for t in upstream(X))
        win = ssim_ref.window()

        def run(x, y, a, b):
            return gnerf_hip.ssim_forward(x, y, win, 1e-4, 9e-4) + gnerf_hip.ssim_backward(x, y, win, 1e-4, 9e-4, a, b)
        first, second = run(X, Y, gs, gc), run(X, Y, gs, gc)
        assert all(torch.equal(a, b) for a, b in zip(first, second))
        for i in range(shape[0]):
            alone = run(X[i:i + 1].clone(), Y[i:i + 1].clone(), gs[i:i + 1].clone(), gc[i:i + 1].clone())
            assert all(torch.equal(a[0], b[i]) for a, b in zip(alone, first)), (shape, i)


def test_ms_ssim_at_512(dev):
    X, Y, L, k = cases()['image_plus_noise_512']
    X, Y = X.float(), Y.float()

    def run(x, y):
        y = y.detach().clone().requires_grad_(True)
        v = S.ms_ssim(x, y, data_range=L, size_average=False)
        v.double().sum().backward()
        return v.detach(), y.grad
    want = ssim_ref.ms_ssim(X.double().numpy(), Y.double().numpy(), L, size_average=False)
    ref = run(X.double(), Y.double())
    assert np.abs(ref[0].numpy() - want).max() < 1e-11
    o32 = run(X, Y)
    got = run(X.to(dev), Y.to(dev))
    check('ms_ssim value', got[0], ref[0], float((o32[0].double() - ref[0]).abs().max()))
    check('ms_ssim dY', got[1], ref[1], float((o32[1].double() - ref[1]).abs().max()))


def test_graph_capture_equals_eager(dev):
    import gnerf_hip
    gen = torch.Generator().manual_seed(11)
    X, Y = torch.rand(4, 3, 64, 64, generator=gen).to(dev), torch.rand(4, 3, 64, 64, generator=gen).to(dev)
    gs, gc = (t.to(dev) for t in upstream(X))
    win = ssim_ref.window()

    def run():
        return gnerf_hip.ssim_forward(X, Y, win, 1e-4, 9e-4) + gnerf_hip.ssim_backward(X, Y, win, 1e-4, 9e-4, gs, gc)
    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, captured))
    X.copy_(torch.rand(4, 3, 64, 64, generator=gen))              # the replay reads the inputs where they were
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(run(), captured))


def test_uncovered_calls_warn_once_and_agree_with_the_cpu_form(dev, monkeypatch):
    import gnerf_hip
    gen = torch.Generator().manual_seed(12)
    r = lambda *s: torch.rand(*s, generator=gen)
    long_win = torch.tensor(ssim_ref.window(13, 2.0), dtype=torch.float32)
    calls = {
        'window': (r(1, 3, 40, 40), r(1, 3, 40, 40), dict(win=long_win)),
        '5-D': (r(1, 2, 12, 16, 16), r(1, 2, 12, 16, 16), {}),
        'short side': (r(1, 3, 8, 40), r(1, 3, 8, 40), {}),
    }
    monkeypatch.setattr(S, '_warned_fallbacks', set())
    monkeypatch.setattr(gnerf_hip, 'ssim_forward', lambda *a, **k: pytest.fail('the kernel was called'))
    for name, (X, Y, kw) in calls.items():
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            want = S.ssim(X, Y, data_range=1.0, **kw)              # CPU tensors: the op form, no RuntimeWarning, no library call
        assert not [x for x in w if issubclass(x.category, RuntimeWarning)], name
        for expect in (1, 0):
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter('always')
                got = S.ssim(X.to(dev), Y.to(dev), data_range=1.0, **kw)
            assert len([x for x in w if issubclass(x.category, RuntimeWarning)]) == expect, (name, expect)
            assert abs(float(got) - float(want)) < 1e-5, name
    with pytest.raises(RuntimeError, match='float32 and float16'):
        S.ssim(torch.rand(1, 3, 32, 32, dtype=torch.float64, device=dev), torch.rand(1, 3, 32, 32, dtype=torch.float64, device=dev), data_range=1.0)


def test_c_entry_refuses_with_a_message(dev):
    import gnerf_hip
    lib = gnerf_hip.load()
    X = torch.rand(1, 3, 8, 64, device=dev)
    out, ws = torch.zeros(2, 3, device=dev), torch.zeros(4096, dtype=torch.uint8, device=dev)
    st = (ctypes.c_int64 * 4)(*X.stride())
    win = (ctypes.c_float * 11)(*ssim_ref.window())
    args = (X.data_ptr(), X.data_ptr(), 0, 1, 3)
    tail = (1e-4, 9e-4, ws.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), None)
    assert lib.gnerf_ssim_forward(*args, 8, 64, st, st, win, 11, *tail) == -1 and b'smaller than the window' in lib.gnerf_last_error()
    assert lib.gnerf_ssim_forward(*args, 8, 64, st, st, win, 4, *tail) == -1 and b'odd' in lib.gnerf_last_error()
    assert lib.gnerf_ssim_backward(*args, 8, 64, st, st, win, 11, 1e-4, 9e-4, out[0].data_ptr(), None, X.data_ptr(), st, None, None, None) == -1
    assert b'smaller than the window' in lib.gnerf_last_error()
    assert lib.gnerf_ssim_backward(*args, 8, 64, st, st, win, 6, 1e-4, 9e-4, out[0].data_ptr(), None, X.data_ptr(), st, None, None, None) == -1
    assert b'odd' in lib.gnerf_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


def test_train_step_with_ssim_end_to_end(dev):
    out = subprocess.run(['timeout', '-k', '10', '600', sys.executable, os.path.join(ROOT, 'g-nerf_amd', 'train_step_mi355x.py'), '--steps', '2', '--warmup', '1',
                          '--ssim'], capture_output=True, text=True, timeout=700, env={**os.environ, 'RANK': '0', 'WORLD_SIZE': '1'})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['ssim_terms'] is True and '(1 - SSIM)' in line['workload']
    for k in ('ssim', 'ssim_raw', 'l1', 'l1_raw', 'gan', 'loss'):
        assert np.isfinite(line['losses'][k]), (k, line['losses'])
    assert 0 < line['losses']['ssim'] < 2 and 0 < line['losses']['ssim_raw'] < 2


def test_generator_gradients_kernel_against_op_form(dev, monkeypatch):
    """The flat vector of G's gradients of generator_loss(ssim=True) under the tolerance rule of this file: the reference is the same step
    with the SSIM terms evaluated by the op form in float64, the yardstick the same step with the float32 op form (on the GPU: the rest of
    the step cannot run elsewhere).  The step runs in float32 (force_fp32): with float16 blocks a last-bit difference in dL/dimage is
    re-rounded to float16 on the way back and says nothing about SSIM.

    How the differences are taken.  Two separate runs of this step do not give the same bits even on one route: MIOpen's convolutions
    differ from call to call, in the forward already.  Measured on an MI355X, SSIM in float64 both times: the images
    differ by 8e-7 and the gradient vectors by 2.4e-5 of a largest entry of 1.18, while the float32 op form's error is 1.9e-6 and the
    floor 1.1e-6, so the difference of two runs' gradient vectors measures the convolution library and not SSIM.  The step is therefore
    run ONCE (on the kernel route), and generator_loss is evaluated again on the same generated images for each route, which gives the
    route's dL/dimage and dL/dimage_raw with nothing else changed.  G's backward is linear in them, so the difference between a route's
    gradient vector and the reference's is G's backward of the difference of those upstream gradients: one pass through the retained
    graph per route, whose own call-to-call noise is relative to that small difference and not to the gradient.  (The difference is
    scaled by a power of two to the size of the upstream gradient on the way in, and back on the way out, so that the backward's float16-split
    convolutions see the operand range of the real step.)"""
    import gen_cases as C
    import train_step_mi355x as T
    G, D = C.build(dev)
    batch = C.batch_on(dev)
    kw = dict(force_fp32=True)
    disc = lambda img, c: D(img, c, **kw)
    params = [p for p in G.parameters()]
    G.train().requires_grad_(True)
    try:
        with C.DI.DetNoise('config5'):
            loss, parts, gen = T.generator_loss(G, disc, batch, 64, ssim=True, **kw)          # the step itself, SSIM on the kernel
        assert torch.isfinite(parts['ssim']) and torch.isfinite(parts['ssim_raw'])
        images = [gen['image'], gen['image_raw']]
        assert all(t.dtype == torch.float32 and t.requires_grad for t in images)

        def flat(grads):
            return torch.cat([g.flatten() for g in grads if g is not None]).double().cpu()
        whole = flat(torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True))
        assert torch.isfinite(whole).all() and float(whole.abs().max()) > 0

        leaves = [t.detach().requires_grad_(True) for t in images]

        class SameImages:                                            # generator_loss on the images of the one run above
            @staticmethod
            def mapping(z, c):
                return None

            @staticmethod
            def synthesis(ws, c, **_):
                return dict(image=leaves[0], image_raw=leaves[1], image_depth=gen['image_depth'].detach())

        def upstream(route):
            monkeypatch.setattr(S, 'ssim_pair', route)
            again = T.generator_loss(SameImages, disc, batch, 64, ssim=True)[0]
            return [g.double() for g in torch.autograd.grad(again, leaves)]

        def in_double(X, Y, win, C1, C2):
            s, cs = S.ssim_pair_torch(X.double(), Y.double(), win, C1, C2)
            return s.float(), cs.float()
        kernel_route = S.ssim_pair
        u_ref, u_32, u_kernel = upstream(in_double), upstream(S.ssim_pair_torch), upstream(kernel_route)
        assert all(torch.equal(a, b) for a, b in zip(u_kernel, upstream(kernel_route)))          # no convolution library in this part

        def gradient_difference(u):
            delta = [a - b for a, b in zip(u, u_ref)]
            size, want = max(float(d.abs().max()) for d in delta), max(float(r.abs().max()) for r in u_ref)
            if size == 0.0:
                return torch.zeros_like(whole), 0.0
            scale = 2.0 ** int(np.floor(np.log2(want / size)))
            out = torch.autograd.grad(images, params, grad_outputs=[(d * scale).float() for d in delta], retain_graph=True, allow_unused=True)
            return flat(out) / scale, size
        d32, up32 = gradient_difference(u_32)
        dk, upk = gradient_difference(u_kernel)
    finally:
        G.requires_grad_(False).eval()
    err32, err = float(d32.abs().max()), float(dk.abs().max())
    tol = max(2 * err32, FLOOR * float(whole.abs().max()))
    print(f'G gradients: kernel error {err:.3e}, float32 op form {err32:.3e}, max |grad| {float(whole.abs().max()):.3e}, tolerance {tol:.3e}; '
          f'upstream (dL/dimage, dL/dimage_raw): kernel error {upk:.3e}, float32 op form {up32:.3e}, max {max(float(r.abs().max()) for r in u_ref):.3e}')
    assert err <= tol
