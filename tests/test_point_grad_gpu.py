"""GPU tests of gnerf_query_points_grad (csrc/query_grad.inl), the position gradient of the point query: against autograd through the
float64 oracle, across layouts, bindings and reruns; run_model with points that require a gradient; normals and colours at mesh vertices
end to end."""

import warnings

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = pytest.mark.gpu

BOUND = 2e-3          # the bound test_query_points_backward_vs_oracle holds the plane / decoder gradients of the same arithmetic chain to


@pytest.fixture(scope='module')
def dev():
    if not has_gpu():
        pytest.fail('GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)')
    import gnerf_hip
    gnerf_hip.load()
    return torch.device('cuda', 0)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _interleaved(planes):
    N, P, C, H, W = planes.shape
    return planes.permute(0, 3, 4, 1, 2).reshape(N, H, W, P * C).contiguous()


@pytest.fixture(scope='module')
def case(dev):
    """The inputs of test_query_points_backward_vs_oracle (seed 9, N = 2, P = 70: partial last tile, planes 24 x 20, some taps zero-padded)
    and, made once, the float64 oracle's point gradients for the three forms of incoming gradient."""
    import gnerf_hip
    from oracle import render_ref as R
    gen = torch.Generator().manual_seed(9)
    N, P_, hw = 2, 70, (24, 20)
    planes = torch.randn(N, 3, 32, *hw, generator=gen) * 1.5
    dec = R.fold_decoder(torch.randn(64, 32, generator=gen), torch.randn(64, generator=gen) * 0.2,
                         torch.randn(33, 64, generator=gen), torch.randn(33, generator=gen) * 0.2)
    pts = (torch.rand(N, P_, 3, generator=gen) - 0.5) * 1.1
    g_sigma = torch.randn(N, P_, 1, generator=gen)
    g_rgb = torch.randn(N, P_, 32, generator=gen)
    # precondition: no pixel coordinate is within 1e-4 of an integer for either plane extent, so float32 rounding cannot move a point
    # into another cell (where floor's one-sided derivative would differ) -- no point needs to be excluded
    for extent in hw:
        pix = ((2.0 * pts.double() + 1) * extent - 1) / 2
        gap = float((pix - pix.round()).abs().min())
        print(f'extent {extent}: closest pixel coordinate to an integer {gap:.2e}')
        assert gap >= 1e-4

    def oracle(points, box_warp, use_sigma, use_rgb):
        p64 = points.double().requires_grad_(True)
        sig, rgb = R.query_points(planes.double(), [t.double() for t in dec], p64, box_warp)
        loss = (sig * g_sigma[:, :points.shape[1]].double()).sum() * use_sigma + (rgb * g_rgb[:, :points.shape[1]].double()).sum() * use_rgb
        return torch.autograd.grad(loss, p64)[0]

    forms = {'both': (True, True), 'sigma': (True, False), 'rgb': (False, True)}
    ref = {k: oracle(pts, 1.0, *v) for k, v in forms.items()}
    return dict(N=N, planes=planes, nhwc=gnerf_hip.planes_to_nhwc(planes.to(dev)), inter=_interleaved(planes).to(dev), dec=[t.to(dev) for t in dec],
                pts=pts, g_sigma=g_sigma, g_rgb=g_rgb, forms=forms, ref=ref, oracle=oracle)


def _grad(case, dev, form='both', pts=None, box_warp=1.0, layout='nhwc'):
    import gnerf_hip
    pts = case['pts'] if pts is None else pts
    use_sigma, use_rgb = case['forms'][form]
    n = pts.shape[1]
    return gnerf_hip.query_points_grad(case[layout], case['N'], case['dec'], pts.to(dev), box_warp,
                                       case['g_sigma'][:, :n].to(dev) if use_sigma else None, case['g_rgb'][:, :n].to(dev) if use_rgb else None)


@pytest.mark.parametrize('form', ['both', 'sigma', 'rgb'])
def test_point_gradient_vs_oracle(dev, case, form):
    got = _grad(case, dev, form)
    assert got.shape == (2, 70, 3) and got.dtype == torch.float32 and torch.isfinite(got).all()
    err = _rel(got.cpu(), case['ref'][form])
    print(f'{form}: rel {err:.3e}')
    assert err < BOUND


@pytest.mark.parametrize('n_points', [1, 16, 17])
def test_point_gradient_tile_edges(dev, case, n_points):
    pts = case['pts'][:, :n_points].contiguous()
    for form in case['forms']:
        err = _rel(_grad(case, dev, form, pts=pts).cpu(), case['oracle'](pts, 1.0, *case['forms'][form]))
        print(f'P = {n_points}, {form}: rel {err:.3e}')
        assert err < BOUND


def test_point_gradient_box_warp_2(dev, case):
    pts = case['pts'] * 2                                      # the same plane coordinates (exactly), half the gradient
    for form in case['forms']:
        ref = case['oracle'](pts, 2.0, *case['forms'][form])
        assert _rel(ref * 2, case['ref'][form]) < 1e-12
        err = _rel(_grad(case, dev, form, pts=pts, box_warp=2.0).cpu(), ref)
        print(f'box_warp 2, {form}: rel {err:.3e}')
        assert err < BOUND


def test_layouts_bindings_and_reruns_are_bit_identical(dev, case, monkeypatch):
    import gnerf_hip
    from gnerf_hip import _native
    assert gnerf_hip.ext() is not None, 'the pybind extension is built by csrc/build.sh'
    for form in case['forms']:
        first = _grad(case, dev, form)
        assert torch.equal(first, _grad(case, dev, form))                                   # two runs
        assert torch.equal(first, _grad(case, dev, form, layout='inter'))                   # [N,H,W,96] against [3N,H,W,32]
        with monkeypatch.context() as m:
            m.setattr(_native, '_ext', False)                                               # the ctypes route
            assert gnerf_hip.ext() is None
            assert torch.equal(first, _grad(case, dev, form))
            assert torch.equal(first, _grad(case, dev, form, layout='inter'))
    # the output buffer is written, not accumulated into: a call after another one with other gradients gives its own result
    assert not torch.equal(_grad(case, dev, 'sigma'), _grad(case, dev, 'rgb'))


def test_arguments_are_checked(dev, case):
    import gnerf_hip
    with pytest.raises(RuntimeError, match='both None'):
        gnerf_hip.query_points_grad(case['nhwc'], 2, case['dec'], case['pts'].to(dev), 1.0, None, None)
    with pytest.raises(RuntimeError, match='must match'):
        gnerf_hip.query_points_grad(case['nhwc'], 2, case['dec'], case['pts'].to(dev), 1.0, case['g_sigma'][:, :5].to(dev), None)
    lib = gnerf_hip.load()
    rc = lib.gnerf_query_points_grad(case['nhwc'].data_ptr(), 2, 24, 20, case['pts'].to(dev).data_ptr(), 70, 1.0, *[t.data_ptr() for t in case['dec']],
                                     None, None, torch.empty(2, 70, 3, device=dev).data_ptr(), 0, None)
    assert rc == -1 and b'both null' in lib.gnerf_last_error()                                # GNERF_E_ARG


@pytest.mark.parametrize('box_warp', [1.0, 2.0])
def test_far_points_have_exactly_zero_gradient(dev, case, box_warp):
    signs = torch.tensor([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=torch.float32)
    pts = (signs * 2 * box_warp).unsqueeze(0).repeat(2, 3, 1)[:, :19].contiguous()          # |p| = 2 box_warp on every axis: every tap outside
    for form in case['forms']:
        got = _grad(case, dev, form, pts=pts, box_warp=box_warp)
        assert torch.equal(got, torch.zeros_like(got))


# ---------------------------------------------------------------------------------------------------------------- run_model

@pytest.fixture(scope='module')
def model(dev, golden):
    from training.volumetric_rendering.renderer import ImportanceRenderer
    from test_host_cpu import Decoder, options_of
    g = golden('render_s12.npz')
    gen = torch.Generator().manual_seed(4)
    n = g['planes'].shape[0]
    return dict(ren=ImportanceRenderer().to(dev), dec=Decoder(g).to(dev), opts=options_of(g), planes=torch.from_numpy(g['planes']).to(dev),
                pts=(torch.rand(n, 50, 3, generator=gen) - 0.5).to(dev), gs=torch.randn(n, 50, 1, generator=gen).to(dev), gc=torch.randn(n, 50, 32, generator=gen).to(dev))


class _Spy:
    """Records the arguments of a gnerf_hip entry point the renderer calls (looked up on the package at call time), then calls it."""

    def __init__(self, monkeypatch, name):
        import gnerf_hip
        self.calls, real = [], getattr(gnerf_hip, name)

        def spy(*args, **kwargs):
            self.calls.append((args, kwargs))
            return real(*args, **kwargs)
        monkeypatch.setattr(gnerf_hip, name, spy)


def _same_arguments(a, b):
    def same(x, y):
        if isinstance(x, torch.Tensor) or isinstance(y, torch.Tensor):
            return isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
        if isinstance(x, (tuple, list)):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        return x == y
    return same(a[0], b[0]) and a[1].keys() == b[1].keys() and all(same(a[1][k], b[1][k]) for k in a[1])


def _run(model, points_grad, params_grad, fused=True, one_tile=False):
    """Gradients of one run_model call: (points, planes, [decoder parameters]); None where not asked for.  one_tile: one item, 16 points."""
    from training.volumetric_rendering import renderer as Rn
    ren, dec = model['ren'], model['dec']
    dec.requires_grad_(params_grad).zero_grad(set_to_none=True)
    model = {k: (v[:1, :16] if k in ('pts', 'gs', 'gc') else v[:1]) if one_tile and isinstance(v, torch.Tensor) else v for k, v in model.items()}
    planes = model['planes'].clone().requires_grad_(params_grad)
    pts = model['pts'].clone().requires_grad_(points_grad)
    Rn._warned_fallbacks.clear()
    type(ren).fused_point_grad = fused
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            out = ren.run_model(planes, dec, pts, torch.zeros_like(pts), model['opts'])
    finally:
        type(ren).fused_point_grad = True
    fell_back = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    assert type(out['sigma'].grad_fn).__name__.startswith('_FusedQuery') == (fused or not points_grad)
    assert bool(fell_back) == (points_grad and not fused)
    ((out['sigma'] * model['gs']).sum() + (out['rgb'] * model['gc']).sum()).backward()
    dec_grads = [p.grad.clone() for p in dec.parameters()] if params_grad else None
    dec.requires_grad_(False)
    return pts.grad, planes.grad, dec_grads


def test_run_model_with_points_that_need_a_gradient(dev, model, monkeypatch):
    backward_calls = _Spy(monkeypatch, 'query_points_backward').calls
    g_pts, g_planes, g_dec = _run(model, True, True)                             # fused, no warning (asserted in _run)
    assert len(backward_calls) == 1
    r_pts, r_planes, r_dec = _run(model, True, True, fused=False)                # the PyTorch-op route, with its warning
    assert g_pts.shape == model['pts'].shape
    for a, b in [(g_pts, r_pts), (g_planes, r_planes)] + list(zip(g_dec, r_dec)):
        assert _rel(a, b) < 2e-3                                                 # test_run_model_training_on_gpu's tolerance
    # The plane and decoder gradients do not depend on whether the points ask for theirs.  "The same bits" can be asserted of the
    # OUTPUTS only on one 16-point tile: gnerf_query_points_backward sums the decoder gradients of several waves (and plane texels hit
    # twice) with float atomics in the order they arrive, so two identical larger calls differ in their last bits whatever the points
    # do (tests/test_gpu_parity.py holds that kernel to 1e-5 between layouts for the same reason); with one tile every other addend is
    # an exact zero and the sum has one order.  At the full size the check is on the INPUTS: the kernel is called with identical
    # arguments, bit for bit, whether or not the points require a gradient -- and the outputs agree to the reordering's rounding.
    t_pts, t_planes, t_dec = _run(model, True, True, one_tile=True)
    none_pts, d_planes, d_dec = _run(model, False, True, one_tile=True)
    assert none_pts is None and t_pts is not None
    assert torch.equal(d_planes, t_planes) and all(torch.equal(a, b) for a, b in zip(d_dec, t_dec))
    # ... and at the full size to the rounding of a reordered float32 sum of <= 50 addends per item
    del backward_calls[1:]
    none_pts, d_planes, d_dec = _run(model, False, True)
    assert none_pts is None and len(backward_calls) == 2 and _same_arguments(backward_calls[0], backward_calls[1])
    for a, b in [(d_planes, g_planes)] + list(zip(d_dec, g_dec)):
        assert _rel(a, b) < 1e-5
    # only the points (frozen planes and decoder)
    o_pts, o_planes, o_dec = _run(model, True, False)
    assert o_planes is None and o_dec is None and torch.equal(o_pts, g_pts)


def test_double_backward_names_the_switch(dev, model):
    ren = model['ren']
    pts = model['pts'].clone().requires_grad_(True)
    sigma = ren.run_model(model['planes'], model['dec'], pts, torch.zeros_like(pts), model['opts'])['sigma']
    grad, = torch.autograd.grad(sigma.sum(), pts, create_graph=True)
    assert torch.isfinite(grad).all()
    with pytest.raises(RuntimeError, match='fused_point_grad'):
        (grad.norm(dim=-1) - 1).square().mean().backward()                       # an eikonal term


def test_unused_output_takes_the_kernels_without_its_half(dev, model, monkeypatch):
    """A loss on sigma alone hands no dL/drgb to either kernel (None, not zeros): the colour half of the decoder is skipped."""
    grad_calls, backward_calls = _Spy(monkeypatch, 'query_points_grad').calls, _Spy(monkeypatch, 'query_points_backward').calls
    ren = model['ren']
    planes, pts = model['planes'].clone().requires_grad_(True), model['pts'].clone().requires_grad_(True)
    out = ren.run_model(planes, model['dec'], pts, torch.zeros_like(pts), model['opts'])
    (out['sigma'] * model['gs']).sum().backward()
    assert len(grad_calls) == 1 and len(backward_calls) == 1
    assert grad_calls[0][0][6] is None and backward_calls[0][0][6] is None and torch.equal(grad_calls[0][0][5], model['gs'])
    want = _run(model, True, True)                                              # both outputs in the loss, dL/drgb multiplied away
    pts2 = model['pts'].clone().requires_grad_(True)
    out = ren.run_model(model['planes'], model['dec'], pts2, torch.zeros_like(pts2), model['opts'])
    ((out['sigma'] * model['gs']).sum() + (out['rgb'] * 0).sum()).backward()
    assert _rel(pts.grad, pts2.grad) < 1e-6 and _rel(want[0], pts.grad) > 1e-3


def test_double_backward_of_the_plane_gradient_raises_too(dev, model):
    """create_graph=True with only the planes asking: the first-order gradient comes back, a second differentiation raises (it used to
    be taken for a constant when the incoming gradient did not itself require one)."""
    planes = model['planes'].clone().requires_grad_(True)
    pts = model['pts']
    sigma = model['ren'].run_model(planes, model['dec'], pts, torch.zeros_like(pts), model['opts'])['sigma']
    grad, = torch.autograd.grad(sigma.sum(), planes, create_graph=True)
    assert grad.shape == planes.shape and torch.isfinite(grad).all() and grad.requires_grad
    with pytest.raises(RuntimeError, match='fused_point_grad'):
        grad.square().sum().backward()
    plain, = torch.autograd.grad(model['ren'].run_model(planes, model['dec'], pts, torch.zeros_like(pts), model['opts'])['sigma'].sum(), planes)
    assert not plain.requires_grad and _rel(plain, grad.detach()) < 1e-5


def test_rays_that_need_a_gradient_stay_on_pytorch_ops(dev, model, golden, monkeypatch):
    """forward()'s fallback for rays with a gradient shades its points through PyTorch ops, as it always did, not the fused query."""
    calls = [_Spy(monkeypatch, n).calls for n in ('query_points', 'query_points_grad', 'query_points_backward')]
    g = golden('render_s12.npz')
    o = torch.from_numpy(g['ray_origins'])[:, :16].to(dev).requires_grad_(True)
    d = torch.from_numpy(g['ray_dirs'])[:, :16].to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        rgb, depth, wsum = model['ren'](model['planes'], model['dec'], o, d, model['opts'])
    assert not type(rgb.grad_fn).__name__.startswith('_Fused')
    (rgb.sum() + depth.sum()).backward()
    assert torch.isfinite(o.grad).all() and bool((o.grad != 0).any()) and not any(calls)


def test_query_normals_on_gpu(dev, model):
    ren, pts = model['ren'], model['pts']
    import gnerf_hip
    sigma, normals = ren.query_normals(model['planes'], model['dec'], pts, model['opts'])
    nhwc, dec = ren._planes_nhwc(model['planes'])[0], ren._decoder_cache((model['dec'].net[0], model['dec'].net[2]))
    want_sigma = gnerf_hip.query_points(nhwc, len(pts), dec, pts, model['opts']['box_warp'])[0]
    grad = gnerf_hip.query_points_grad(nhwc, len(pts), dec, pts, model['opts']['box_warp'], torch.ones_like(want_sigma), None)
    assert torch.equal(sigma, want_sigma) and not normals.requires_grad
    length = normals.norm(dim=-1)
    assert bool(((length - 1).abs() < 1e-5).all()) and _rel(normals, -grad / grad.norm(dim=-1, keepdim=True)) < 1e-6
    # points outside every plane: the gradient is exactly zero, and the normal is the exact zero vector (no NaN)
    far = torch.full_like(pts[:1], 2 * model['opts']['box_warp'])
    sigma0, normals0 = ren.query_normals(model['planes'][:1], model['dec'], far, model['opts'])
    assert torch.isfinite(sigma0).all() and torch.equal(normals0, torch.zeros_like(normals0))


# ---------------------------------------------------------------------------------------------------------------- end to end

def test_mesh_with_normals_and_colours(dev, tmp_path):
    import gen_videos_mi355x as gv
    import shape_mi355x as S
    from training.volumetric_rendering.renderer import sample_from_planes
    res = 32
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    ws = gv.orbit_latents(G, z, dev)
    vol, planes = gv.extract_density_grid(G, ws, res, return_planes=True)
    assert torch.equal(vol, gv.extract_density_grid(G, ws, res, planes=planes))            # planes= : the backbone is not run again
    level = float(vol.median())
    bare, full = str(tmp_path / 'bare.ply'), str(tmp_path / 'full.ply')
    nv, nf, _ = gv.mesh_density_grid(vol, bare, level)
    assert (nv, nf) == gv.mesh_density_grid(vol, full, level, attrs='all', G=G, planes=planes)[:2] and nf > 100
    assert S.read_ply_attrs(bare) == {}
    verts, faces = S.read_ply(bare)
    v2, f2 = S.read_ply(full)
    assert len(verts) == nv and len(faces) == nf
    assert np.array_equal(verts.view(np.uint32), v2.view(np.uint32)) and np.array_equal(faces, f2)
    attrs = S.read_ply_attrs(full)
    normals, colors = attrs['normals'], attrs['colors']
    assert normals.shape == (nv, 3) and colors.shape == (nv, 3) and colors.dtype == np.uint8
    length = np.linalg.norm(normals.astype(np.float64), axis=1)
    assert np.all((np.abs(length - 1) < 1e-5) | (length == 0))
    # the same attributes from PyTorch ops at the same vertices
    kw = G.rendering_kwargs
    world = gv.lattice_to_world(gv.mesh_to_lattice(torch.from_numpy(verts).to(dev), res), res, kw['box_warp']).unsqueeze(0)
    with torch.enable_grad():
        pts = world.clone().requires_grad_(True)
        out = G.decoder(sample_from_planes(G.renderer.plane_axes.to(dev), planes[:1], pts, padding_mode='zeros', box_warp=kw['box_warp']), None)
        grad, = torch.autograd.grad(out['sigma'].sum(), pts)
    ref_normals = gv.normals_to_mesh_frame(-grad[0] / grad[0].norm(dim=-1, keepdim=True).clamp_min(1e-30), res, kw['box_warp'])
    err = _rel(torch.from_numpy(normals), ref_normals.cpu())
    print(f'{nv} vertices, normals rel {err:.3e}')
    assert err < 2e-3
    ref_colors = ((out['rgb'][0, :, :3].detach() * 0.5 + 0.5) * 255).clamp(0, 255).round()
    assert int((torch.from_numpy(colors).float() - ref_colors.cpu()).abs().max()) <= 1
    for which, keys in (('normals', {'normals'}), ('colors', {'colors'})):
        one = str(tmp_path / f'{which}.ply')
        gv.mesh_density_grid(vol, one, level, attrs=which, G=G, planes=planes)
        got = S.read_ply_attrs(one)
        assert set(got) == keys and np.array_equal(got[which], attrs[which])
