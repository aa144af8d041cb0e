"""The fused renderer's ray gradient on the GPU (gnerf_render_backward_rays, csrc/render_ray_grad.inl): against autograd through the
float64 oracle, its indexing one ray at a time, bit-reproducibility across requests, runs, layouts and bindings, its refusals,
ImportanceRenderer.fused_ray_grad and gnerf_harness.fit_camera."""

import warnings

import pytest
import torch

import ray_grad_ref as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda', 0)


def _clear_env(monkeypatch):
    for k in ('GNERF_BWD_KERNEL', 'GNERF_BWD_MLP', 'GNERF_BWD_SCATTER'):
        monkeypatch.delenv(k, raising=False)


def _nhwc(ref, dev, interleaved=False):
    import gnerf_hip
    if interleaved:
        N, _, _, H, W = ref.planes.shape
        return ref.planes.permute(0, 3, 4, 1, 2).reshape(N, H, W, 96).contiguous().to(dev)
    return gnerf_hip.planes_to_nhwc(ref.planes.to(dev))


def _backward(ref, dev, nhwc=None, grads=None, **kw):
    """gnerf_hip.render_backward on the case's inputs; grads = (g_rgb, g_depth, g_wsum) replaces the case's upstream gradients."""
    import gnerf_hip
    g_rgb, g_depth, g_wsum = grads if grads is not None else (ref.g_rgb, ref.g_depth, ref.g_wsum)
    kw.setdefault('ray_start', RR.RAY_START)
    kw.setdefault('ray_end', RR.RAY_END)
    return gnerf_hip.render_backward(_nhwc(ref, dev) if nhwc is None else nhwc, ref.N, [t.to(dev) for t in ref.dec], ref.o.to(dev), ref.d.to(dev),
                                     ref.nc.to(dev), ref.nf.to(dev) if ref.F else None, g_rgb.to(dev), g_depth.to(dev), g_wsum.to(dev),
                                     depth_resolution=ref.S, depth_resolution_importance=ref.F, box_warp=ref.box_warp, white_back=ref.white_back,
                                     image_width=ref.cfg['res'], **kw)


def _check_against_oracle(ref, g_o, g_d, what):
    """The project's tolerances for this backward (test_render_backward_vs_oracle): max error <= 2e-3 of the gradient's largest entry and
    l2 error <= 1e-3, for each of the two gradients, over the rays whose samples keep 1e-4 texels from every cell boundary; the others finite."""
    assert ref.left_out <= RR.MAX_LEFT_OUT, (what, ref.left_out)
    for name, got, want in (('grad_origins', g_o, ref.grad_o), ('grad_dirs', g_d, ref.grad_d)):
        got = got.cpu()
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), (what, name)
        a, b = got[ref.keep], want[ref.keep]
        print(f'{ref.name} {what} {name}: max {RR.rel_max(a, b):.3e} l2 {RR.rel_l2(a, b):.3e} (left out {ref.left_out:.3f})')
        assert RR.rel_max(a, b) <= 2e-3, (what, name, RR.rel_max(a, b))
        assert RR.rel_l2(a, b) <= 1e-3, (what, name, RR.rel_l2(a, b))


@pytest.mark.parametrize('case', list(RR.CASES))
def test_ray_gradient_vs_oracle(dev, case, monkeypatch):
    """Joint request (planes, decoder and rays) with the default arithmetic, with exact-fp32 products in both first-pass kernels, and -- for
    the shapes the pipelined kernels take -- with the one-wave-per-ray first pass."""
    ref = RR.reference(case)
    nhwc = _nhwc(ref, dev)
    for mode in (None, 'f32') + (('wave',) if case in RR.PIPELINED else ()):
        _clear_env(monkeypatch)
        if mode == 'f32':
            monkeypatch.setenv('GNERF_BWD_MLP', 'f32')
        elif mode == 'wave':
            monkeypatch.setenv('GNERF_BWD_KERNEL', 'wave')
        g_planes, g_dec, (g_o, g_d) = _backward(ref, dev, nhwc, need_rays=True)
        _check_against_oracle(ref, g_o, g_d, mode or 'default')
        # the other gradients of the same call are the backward's as before
        gp = g_planes.reshape(ref.N, 3, *ref.cfg['hw'], 32).permute(0, 1, 4, 2, 3).cpu()
        assert RR.rel_max(gp, ref.grad_planes) < 2e-3 and RR.rel_l2(gp, ref.grad_planes) < 1e-3, mode
        for a, b in zip(g_dec, ref.grad_dec):
            assert RR.rel_max(a.cpu(), b) < 2e-3 and RR.rel_l2(a.cpu(), b) < 1e-3, mode
    _clear_env(monkeypatch)


def test_one_ray_at_a_time(dev, monkeypatch):
    """Upstream gradients that are zero outside one ray: only that ray's six outputs are non-zero -- exact zeros elsewhere -- and they are
    the oracle's.  First ray, last ray of item 0, first ray of item 1 and last ray of the call, on the ragged-items case (padded ray
    sequence) and with the one-wave-per-ray first pass: a misindexed block is an error of 1, not of 1e-4."""
    ref = RR.reference('ragged_items')
    nhwc = _nhwc(ref, dev)
    R = ref.N * ref.M
    for mode in (None, 'wave'):
        _clear_env(monkeypatch)
        if mode:
            monkeypatch.setenv('GNERF_BWD_KERNEL', mode)
        for ray in (0, ref.M - 1, ref.M, R - 1):
            assert bool(ref.keep.reshape(-1)[ray]), 'pick the case seed so that these rays are compared'
            sel = torch.zeros(R, 1)
            sel[ray] = 1.0
            grads = [(g.reshape(R, -1) * sel).reshape(g.shape) for g in (ref.g_rgb, ref.g_depth, ref.g_wsum)]
            _, _, (g_o, g_d) = _backward(ref, dev, nhwc, grads, need_rays=True)
            want_o, want_d, *_ = ref.oracle(*grads)
            for got, want in ((g_o.cpu().reshape(R, 3), want_o.reshape(R, 3)), (g_d.cpu().reshape(R, 3), want_d.reshape(R, 3))):
                others = torch.ones(R, dtype=torch.bool)
                others[ray] = False
                assert bool((got[others] == 0).all()), (mode, ray)
                assert bool((want[others] == 0).all())
                assert RR.rel_max(got[ray], want[ray]) <= 2e-3, (mode, ray, got[ray], want[ray])
    _clear_env(monkeypatch)


@pytest.mark.parametrize('case', ['ragged_items', 'training_counts', 'wave_route'])
def test_requests_runs_layouts_and_bindings_agree_bit_for_bit(dev, case, monkeypatch):
    import gnerf_hip
    from gnerf_hip import _native
    _clear_env(monkeypatch)
    ref = RR.reference(case)
    nhwc = _nhwc(ref, dev)
    g_planes, g_dec, (g_o, g_d) = _backward(ref, dev, nhwc, need_rays=True)
    # a second run
    g_planes2, g_dec2, (g_o2, g_d2) = _backward(ref, dev, nhwc, need_rays=True)
    assert torch.equal(g_o, g_o2) and torch.equal(g_d, g_d2)
    # the ray-only request (frozen planes and decoder): the rows are staged, the scatter is skipped
    none_p, none_d, (g_o3, g_d3) = _backward(ref, dev, nhwc, need_rays=True, need_planes=False, need_decoder=False)
    assert none_p is None and none_d is None
    assert torch.equal(g_o, g_o3) and torch.equal(g_d, g_d3)
    # ... and with the decoder's gradient but not the planes'
    none_p, g_dec4, (g_o4, g_d4) = _backward(ref, dev, nhwc, need_rays=True, need_planes=False)
    assert none_p is None and torch.equal(g_o, g_o4) and torch.equal(g_d, g_d4)
    # the other gradients do not notice the ray request: planes bit for bit (binned scatter), the decoder's -- summed with float atomics --
    # within the spread test_render_backward_vs_oracle allows between routes
    plain = _backward(ref, dev, nhwc)
    assert len(plain) == 2
    assert torch.equal(plain[0], g_planes)
    for a, b, c in zip(plain[1], g_dec, g_dec4):
        assert RR.rel_max(a, b) < 2e-3 and RR.rel_max(c, b) < 2e-3
    # the interleaved plane layout
    _, _, (g_o5, g_d5) = _backward(ref, dev, _nhwc(ref, dev, interleaved=True), need_rays=True, need_decoder=False)
    assert torch.equal(g_o, g_o5) and torch.equal(g_d, g_d5)
    # the other binding
    assert _native.ext() is not None, 'the default binding is the extension'
    monkeypatch.setattr(_native, '_ext', False)
    assert gnerf_hip.ext() is None
    _, _, (g_o6, g_d6) = _backward(ref, dev, nhwc, need_rays=True)
    assert torch.equal(g_o, g_o6) and torch.equal(g_d, g_d6)


def test_refusals(dev, monkeypatch):
    """What the formula does not cover is GNERF_E_UNSUPPORTED before any launch, through either binding."""
    import gnerf_hip
    _clear_env(monkeypatch)
    ref = RR.reference('no_importance')
    R = ref.N * ref.M
    sigma_noise = (torch.zeros(R, ref.S, device=dev), None)
    for kw in (dict(ray_start=torch.full([R], RR.RAY_START, device=dev), ray_end=torch.full([R], RR.RAY_END, device=dev)),
               dict(staged_scatter=False), dict(sigma_noise=sigma_noise), dict(staged_scatter=False, need_planes=False, need_decoder=False)):
        with pytest.raises(gnerf_hip.NativeError) as info:
            _backward(ref, dev, need_rays=True, **kw)
        assert info.value.code == gnerf_hip.E_UNSUPPORTED, kw
    monkeypatch.setenv('GNERF_BWD_SCATTER', 'direct')
    with pytest.raises(gnerf_hip.NativeError) as info:
        _backward(ref, dev, need_rays=True)
    assert info.value.code == gnerf_hip.E_UNSUPPORTED
    monkeypatch.delenv('GNERF_BWD_SCATTER')
    assert len(_backward(ref, dev, need_rays=True)) == 3                  # (the same call without the obstacle)


# ---------------------------------------------------------------------------- the drop-in class


def _class_scene(dev, case='ragged_everything'):
    import gnerf_harness as H
    ref = RR.reference(case)
    dec = H.TriPlaneDecoder().to(dev)
    with torch.no_grad():                                   # the case's effective weights as the module's raw ones
        fc1, fc2 = dec.net[0], dec.net[2]
        w1, b1, w2, b2 = [t.to(dev) for t in ref.dec]
        fc1.weight.copy_(w1 / fc1.weight_gain); fc1.bias.copy_(b1 / fc1.bias_gain)
        fc2.weight.copy_(w2 / fc2.weight_gain); fc2.bias.copy_(b2 / fc2.bias_gain)
    return ref, dec


def _render_with_draws(r, planes, dec, o, d, opts, ref, dev, monkeypatch):
    """r(...) with the case's two uniform draws in place of torch's (both routes draw coarse then fine; the op form draws the coarse
    one with rand_like)."""
    draws = [ref.nc.to(dev), ref.nf.to(dev)]
    real, real_like = torch.rand, torch.rand_like

    def fake_rand(*a, **k):
        shape = a[0] if isinstance(a[0], (list, tuple, torch.Size)) else a
        return draws.pop(0).reshape(*shape)
    monkeypatch.setattr(torch, 'rand', fake_rand)
    monkeypatch.setattr(torch, 'rand_like', lambda t, **k: draws.pop(0).reshape(t.shape).to(t.dtype))
    try:
        return r(planes, dec, o, d, opts)
    finally:
        monkeypatch.setattr(torch, 'rand', real)
        monkeypatch.setattr(torch, 'rand_like', real_like)


@pytest.mark.parametrize('train_planes', [False, True])
def test_renderer_class_takes_the_fused_route(dev, train_planes, monkeypatch):
    """fused_ray_grad = True: no warning, the graph is _FusedRender's, and the rays' gradients are the PyTorch-op form's -- with frozen
    planes and decoder, and with planes and decoder that need a gradient too."""
    from training.volumetric_rendering import renderer as RM
    _clear_env(monkeypatch)
    ref, dec = _class_scene(dev)
    dec.requires_grad_(train_planes)
    opts = dict(ref.opts, disparity_space_sampling=False)
    g = [t.to(dev) for t in (ref.g_rgb, ref.g_depth, ref.g_wsum)]
    results = {}
    RM._warned_fallbacks.clear()
    for fused in (True, False):
        monkeypatch.setattr(RM.ImportanceRenderer, 'fused_ray_grad', fused)
        r = RM.ImportanceRenderer()
        planes = ref.planes.to(dev).requires_grad_(train_planes)
        o, d = ref.o.to(dev).requires_grad_(True), ref.d.to(dev).requires_grad_(True)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            rgb, depth, wsum = _render_with_draws(r, planes, dec, o, d, opts, ref, dev, monkeypatch)
        said = [str(w.message) for w in rec if issubclass(w.category, RuntimeWarning)]
        if fused:
            assert not said, said
            assert type(rgb.grad_fn).__name__.startswith('_FusedRender'), rgb.grad_fn
        else:
            assert len(said) == 1 and 'rays need a gradient' in said[0] and 'fused_ray_grad is False' in said[0], said
        ((rgb * g[0]).sum() + (depth * g[1]).sum() + (wsum * g[2]).sum()).backward()
        results[fused] = (o.grad.cpu(), d.grad.cpu(), None if planes.grad is None else planes.grad.cpu())
        dec.zero_grad()
    keep = ref.keep
    for a, b in zip(results[True][:2], results[False][:2]):
        assert bool(torch.isfinite(a).all())
        assert RR.rel_max(a[keep], b[keep]) <= 2e-3 and RR.rel_l2(a[keep], b[keep]) <= 1e-3, (RR.rel_max(a[keep], b[keep]), RR.rel_l2(a[keep], b[keep]))
    if train_planes:
        assert RR.rel_max(results[True][2], results[False][2]) <= 2e-3
    # ... and the oracle's
    _check_against_oracle(ref, results[True][0], results[True][1], 'class')


def test_renderer_class_falls_back_and_differentiates_once(dev, monkeypatch):
    from training.volumetric_rendering import renderer as RM
    _clear_env(monkeypatch)
    ref, dec = _class_scene(dev, 'no_importance')
    dec.requires_grad_(False)
    monkeypatch.setattr(RM.ImportanceRenderer, 'fused_ray_grad', True)
    r = RM.ImportanceRenderer()
    planes = ref.planes.to(dev)
    o, d = ref.o.to(dev).requires_grad_(True), ref.d.to(dev).requires_grad_(True)
    RM._warned_fallbacks.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        rgb, _, _ = r(planes, dec, o, d, dict(ref.opts, ray_start='auto', ray_end='auto', disparity_space_sampling=False))
    said = [str(w.message) for w in rec if issubclass(w.category, RuntimeWarning)]
    assert len(said) == 1 and 'rays need a gradient' in said[0] and "'auto'" in said[0] and 'PyTorch-op form' in said[0], said
    assert not type(rgb.grad_fn).__name__.startswith('_FusedRender')
    # a second differentiation of the fused route raises and says what to do
    rgb, _, _ = r(planes, dec, o, d, dict(ref.opts, disparity_space_sampling=False))
    first, = torch.autograd.grad(rgb.sum(), o, create_graph=True)
    with pytest.raises(RuntimeError, match='fused_ray_grad = False'):
        first.sum().backward()


# ---------------------------------------------------------------------------- end to end


def test_fit_camera_gradient_and_descent(dev, monkeypatch):
    """A random-init generator at 16 x 16 rays: the gradient of fit_camera's loss by (yaw, pitch, radius) on the fused route agrees with the
    PyTorch-op form's to 2e-3 of its largest entry, and a handful of steps on the fused route lowers the loss."""
    import gnerf_harness as H
    from gnerf_generator import Generator
    from training.volumetric_rendering import renderer as RM
    _clear_env(monkeypatch)
    torch.manual_seed(3)
    G = Generator().to(dev).eval().requires_grad_(False)
    ws = G.mapping(torch.randn(1, 512, device=dev), H.camera_label(H.lookat_pose(1.57, 1.52, 2.7, dev)))
    res = 16
    with torch.no_grad():
        target = G.synthesis(ws, H.camera_label(H.lookat_pose(1.57, 1.52, 2.7, dev)), neural_rendering_resolution=res, noise_mode='const')['image_raw']
    start = (1.57 + 0.25, 1.52 - 0.12, 2.7 + 0.15)
    grads = {}
    RM._warned_fallbacks.clear()
    for fused in (True, False):
        monkeypatch.setattr(RM.ImportanceRenderer, 'fused_ray_grad', fused)
        torch.manual_seed(17)                                # the same two draws on either route
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            grads[fused] = H.camera_loss_gradient(G, ws, target, *start, resolution=res)
    a, b = grads[True][1], grads[False][1]
    print('fit_camera gradient: fused', a.tolist(), 'ops', b.tolist(), 'loss', grads[True][0], grads[False][0])
    assert float((a - b).abs().max()) <= 2e-3 * float(b.abs().max()), (a, b)
    monkeypatch.setattr(RM.ImportanceRenderer, 'fused_ray_grad', True)
    torch.manual_seed(17)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)       # the fused route: silent
        traj = H.fit_camera(G, ws, target, *start, steps=8, lr=0.02, resolution=res)
    losses = [t['loss'] for t in traj]
    print('fit_camera losses', losses)
    assert min(losses[-3:]) < losses[0]
