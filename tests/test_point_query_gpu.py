"""GPU tests of the three point-query kernels past one 16-point tile per wave: gnerf_query_points (csrc/render_query.hip, query_kernel),
gnerf_query_points_backward (csrc/query_bwd.inl, query_bwd_kernel) and gnerf_query_points_grad (csrc/query_grad.inl, query_grad_kernel)
against the float64 oracle (oracle/render_ref.py:query_points, autograd for the gradients) on one scene in which every kernel takes at least
two trips of its grid-stride loop, a wave's loop crosses from one item into the next, and the tile whose plane scatter is deferred into
another item's gather is a partial one.  The backward is probed one tile at a time: its outputs are linear in the incoming gradients, so
with every gradient outside one tile zero a lost, doubled or misplaced tile is an error of order 1, not of 1e-4."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, has_gpu

pytestmark = pytest.mark.gpu

BOUND = 2e-3                         # tests/test_point_grad_gpu.py's BOUND = test_query_points_backward_vs_oracle's: of the largest entry
NEAR = 1e-4                          # points this close (in texels) to a texel boundary are left out of the position-gradient comparison

N, P, HW = 3, 16 * 2731 + 5, (24, 20)
TPI = (P + 15) // 16                 # tiles per item: 2732, the last one with 5 live points
N_TILES = N * TPI                    # 8196
#        first trip | first tile of a backward wave's second trip; 16 identical points | item 0's partial last tile, its scatter deferred
#        into item 1 | first tile of item 1 | first tile of a forward workgroup's second trip; 16 points in one texel cell | every tap
#        padded | the call's last tile: partial, flushed after the loop
PROBES = (0, 2048, 2731, 2732, 4096, 6000, 8195)
SAME, CELL, FAR = 2048, 4096, 6000


@pytest.fixture(scope='module')
def dev():
    if not has_gpu():
        pytest.fail('GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)')
    import gnerf_hip
    gnerf_hip.load()
    return torch.device('cuda', 0)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _entrywise_ok(a, b, rtol=5e-3, floor=2e-4):
    """tests/test_gpu_parity.py's: every entry within rtol of its own magnitude, with an absolute floor of `floor` x the largest entry."""
    a, b = a.double(), b.double()
    return bool(((a - b).abs() <= rtol * b.abs() + floor * b.abs().max()).all())


def _interleaved(planes):
    n, p, c, h, w = planes.shape
    return planes.permute(0, 3, 4, 1, 2).reshape(n, h, w, p * c).contiguous()


def _tile(g):
    """Global tile -> (item, slice of its live points)."""
    item, t = divmod(g, TPI)
    return item, slice(16 * t, min(16 * t + 16, P))


def kernel_strides():
    """Tiles between two trips of one wave (backward, position gradient) or workgroup (forward), read from the launch code's own caps."""
    csrc = os.path.join(PKG, 'csrc')
    read = lambda name: open(os.path.join(csrc, name)).read()
    num_cu = int(re.search(r'constexpr int kNumCU = (\d+);', read('common.h')).group(1))
    waves = int(re.search(r'constexpr int kBwdWaves = (\d+);', read('render_bwd_tile.inl')).group(1))
    text = read('render_query.hip')

    def body(name):
        start = text.index(f'extern "C" int gnerf_{name}(')
        return text[start:text.index('\n}\n', start)]
    forward = re.search(r'blocks = int\(tiles < int64_t\(kNumCU\) \* (\d+) \? tiles : int64_t\(kNumCU\) \* (\d+)\);\s*hipLaunchKernelGGL\(query_kernel, dim3\(blocks\), dim3\(64\)',
                        body('query_points'))
    assert forward and forward.group(1) == forward.group(2)
    capped = r'blocks = \(tiles \+ kBwdWaves - 1\) / kBwdWaves;\s*if \(blocks > int64_t\(kNumCU\) \* (\d+)\) blocks = int64_t\(kNumCU\) \* (\d+);'
    backward, grad = re.search(capped, body('query_points_backward')), re.search(capped, body('query_points_grad'))
    assert backward and backward.group(1) == backward.group(2) and grad and grad.group(1) == grad.group(2)
    return dict(forward=num_cu * int(forward.group(1)), backward=num_cu * int(backward.group(1)) * waves, grad=num_cu * int(grad.group(1)) * waves)


def make_scene():
    """CPU only.  test_query_points_backward_vs_oracle's recipe (seed 9, planes 24 x 20, points (rand - 0.5) * 1.1: some taps zero-padded)
    at N = 3, P = 43701, with three tiles overwritten on purpose."""
    from oracle import render_ref as R
    gen = torch.Generator().manual_seed(9)
    planes = torch.randn(N, 3, 32, *HW, generator=gen) * 1.5
    dec = R.fold_decoder(torch.randn(64, 32, generator=gen), torch.randn(64, generator=gen) * 0.2,
                         torch.randn(33, 64, generator=gen), torch.randn(33, generator=gen) * 0.2)
    pts = (torch.rand(N, P, 3, generator=gen) - 0.5) * 1.1
    g_sigma = torch.randn(N, P, 1, generator=gen)
    g_rgb = torch.randn(N, P, 32, generator=gen)
    # 16 identical points: every tap of the tile's scatter collides.  Pixel coordinates 20 p + 9.5 and 24 p + 11.5:
    # x -> 14.24 / 17.188, y -> 3.868, z -> 11.92 / 14.404
    item, sl = _tile(SAME)
    pts[item, sl] = torch.tensor([0.237, -0.318, 0.121])
    # 16 distinct points inside one texel cell of each plane: x -> 6.25 / 7.6, y -> 16.3, z -> 16.25 / 19.6, each +- 0.096 at the most
    item, sl = _tile(CELL)
    pts[item, sl] = torch.tensor([-0.1625, 0.2, 0.3375]) + (torch.rand(16, 3, generator=gen) - 0.5) * 0.008
    # |p| = 2 box_warp on every axis, in all eight octants: every tap is padded
    item, sl = _tile(FAR)
    pts[item, sl] = torch.tensor([[sx, sy, sz] for sx in (-2., 2.) for sy in (-2., 2.) for sz in (-2., 2.)]).repeat(2, 1)
    # the pixel coordinates the three planes read: x as a column and a row, y as a row, z as a row and a column
    p64 = pts.double()
    pix = torch.stack([((2 * p64[..., k] + 1) * HW[e] - 1) / 2 for k, e in ((0, 1), (0, 0), (1, 0), (2, 0), (2, 1))], -1)
    near = ((pix - pix.round()).abs() < NEAR).any(-1)                                  # [N, P]
    extent = torch.tensor([20., 24., 24., 24., 20.])
    return dict(planes=planes, dec=dec, pts=pts, g_sigma=g_sigma, g_rgb=g_rgb, pix=pix, extent=extent, near=near)


def oracle_tiles(scene, tiles):
    """float64 plane and decoder gradients of the points of `tiles` alone, with the scene's incoming gradients: (planes [N,3,32,H,W], [4])."""
    from oracle import render_ref as R
    pl = scene['planes'].double().requires_grad_(True)
    dc = [t.double().requires_grad_(True) for t in scene['dec']]
    loss = 0
    for g in tiles:
        item, sl = _tile(g)
        sig, rgb = R.query_points(pl[item:item + 1], dc, scene['pts'][item:item + 1, sl].double(), 1.0)
        loss = loss + (sig * scene['g_sigma'][item:item + 1, sl].double()).sum() + (rgb * scene['g_rgb'][item:item + 1, sl].double()).sum()
    grads = torch.autograd.grad(loss, [pl] + dc)
    return grads[0], list(grads[1:])


def oracle_dense(scene):
    """float64 outputs of the whole scene and, for dL/dsigma alone and dL/drgb alone, the gradients by planes, decoder and points (the
    gradients are linear in the incoming ones: 'both' is their sum)."""
    from oracle import render_ref as R
    pl = scene['planes'].double().requires_grad_(True)
    dc = [t.double().requires_grad_(True) for t in scene['dec']]
    p64 = scene['pts'].double().requires_grad_(True)
    sig, rgb = R.query_points(pl, dc, p64, 1.0)
    out = dict(out_sigma=sig.detach(), out_rgb=rgb.detach())
    for form, loss in (('sigma', (sig * scene['g_sigma'].double()).sum()), ('rgb', (rgb * scene['g_rgb'].double()).sum())):
        grads = torch.autograd.grad(loss, [pl] + dc + [p64], retain_graph=form == 'sigma')
        out[form] = dict(planes=grads[0], dec=list(grads[1:5]), pts=grads[5])
    s, c = out['sigma'], out['rgb']
    out['both'] = dict(planes=s['planes'] + c['planes'], dec=[a + b for a, b in zip(s['dec'], c['dec'])], pts=s['pts'] + c['pts'])
    return out


@pytest.fixture(scope='module')
def case(dev):
    """The scene, its device copies in both plane layouts, and the float64 oracle's results, made once and left unchanged."""
    import gnerf_hip
    scene = make_scene()
    nhwc = gnerf_hip.planes_to_nhwc(scene['planes'].to(dev))
    ref = oracle_dense(scene)
    probe = {g: oracle_tiles(scene, [g]) for g in PROBES}
    probe['all'] = oracle_tiles(scene, PROBES)
    return dict(scene, nhwc=nhwc, inter=_interleaved(scene['planes']).to(dev), dec_dev=[t.to(dev) for t in scene['dec']],
                pts_dev=scene['pts'].to(dev), gs_dev=scene['g_sigma'].to(dev), gc_dev=scene['g_rgb'].to(dev), ref=ref, probe=probe)


FORMS = {'both': (True, True), 'sigma': (True, False), 'rgb': (False, True)}


def _planes_nchw(grad, layout):
    """A plane gradient in the layout it was asked for -> [N,3,32,H,W] on the CPU."""
    g = grad.cpu()
    if layout == 'inter':
        return g.reshape(N, *HW, 3, 32).permute(0, 3, 4, 1, 2)
    return g.reshape(N, 3, *HW, 32).permute(0, 1, 4, 2, 3)


def _backward(case, gs, gc, layout='nhwc', pts=None, box_warp=1.0, **kw):
    import gnerf_hip
    gp, gd = gnerf_hip.query_points_backward(case[layout], N, case['dec_dev'], case['pts_dev'] if pts is None else pts, box_warp, gs, gc, **kw)
    return None if gp is None else _planes_nchw(gp, layout), None if gd is None else [t.cpu() for t in gd]


def _masked(case, tiles):
    """The scene's incoming gradients on the live points of `tiles`, exact zeros everywhere else."""
    gs, gc = torch.zeros_like(case['g_sigma']), torch.zeros_like(case['g_rgb'])
    for g in tiles:
        item, sl = _tile(g)
        gs[item, sl], gc[item, sl] = case['g_sigma'][item, sl], case['g_rgb'][item, sl]
    dev = case['pts_dev'].device
    return gs.to(dev), gc.to(dev)


# ---------------------------------------------------------------------------------------------------------------- the scene itself

def test_scene_makes_every_kernel_loop():
    """Trips per wave (workgroup for the forward) from the launch code's own caps.  Strides in tiles: forward kNumCU * 16 = 4096 workgroups
    of one wave; backward kNumCU * 2 workgroups of 4 waves = 2048; position gradient kNumCU * 3 workgroups of 4 waves = 3072."""
    strides = kernel_strides()
    print(strides)
    assert N * ((P + 15) // 16) > 2 * max(strides.values()), 'a launch cap grew: the scene no longer makes every wave loop -- enlarge P'
    assert strides == dict(forward=4096, backward=2048, grad=3072), 'a launch cap changed: PROBES name tiles by the trips they fall in'
    assert P % 16 == 5 and _tile(2731) == (0, slice(16 * 2731, P)) and _tile(8195)[0] == 2
    for stride in strides.values():
        assert N_TILES >= 2 * stride                                              # every wave takes at least two trips
        later = TPI - 1 + stride                                                  # the trip after item 0's partial tile, same wave
        assert later < N_TILES and later // TPI != 0                              # ... exists, and lies in another item
    assert SAME == strides['backward'] and CELL == strides['forward']             # first tiles of a second trip


def test_scene_points_and_texel_boundaries():
    """CPU only: the overwritten tiles are what they claim to be, and few points (none in a probe tile) sit on a texel boundary."""
    s = make_scene()
    item, sl = _tile(SAME)
    assert bool((s['pts'][item, sl] == s['pts'][item, sl][0]).all())
    item, sl = _tile(CELL)
    cell = s['pix'][item, sl].floor()
    assert bool((cell == cell[0]).all()) and len(torch.unique(s['pts'][item, sl], dim=0)) == 16
    assert bool(((s['pix'][item, sl] >= 0) & (s['pix'][item, sl] < s['extent'] - 1)).all())       # all four taps inside
    item, sl = _tile(FAR)
    assert bool(((s['pix'][item, sl] < -1) | (s['pix'][item, sl] > 24)).all())
    share = float(s['near'].double().mean())
    print(f'{int(s["near"].sum())} of {N * P} points within {NEAR} of a texel boundary ({share:.3%})')
    assert share < 0.01
    for g in PROBES:
        item, sl = _tile(g)
        assert not bool(s['near'][item, sl].any()), g
    outside = float((s['pts'].abs() > 0.5).any(-1).double().mean())
    assert outside > 0.05                                                              # zero-padded taps are well represented


# ---------------------------------------------------------------------------------------------------------------- forward

def test_forward_all_points(dev, case):
    import gnerf_hip
    sigma, rgb = gnerf_hip.query_points(case['nhwc'], N, case['dec_dev'], case['pts_dev'], 1.0)
    assert sigma.shape == (N, P, 1) and rgb.shape == (N, P, 32)
    ref = case['ref']
    es, ec = (sigma.cpu().double() - ref['out_sigma']).abs(), (rgb.cpu().double() - ref['out_rgb']).abs()
    print(f'sigma: max abs err {float(es.max()):.3e}, max err / (5e-5 + 1e-4 |ref|) {float((es / (5e-5 + 1e-4 * ref["out_sigma"].abs())).max()):.3f}; '
          f'rgb: max abs err {float(ec.max()):.3e}')
    np.testing.assert_allclose(sigma.cpu().numpy(), ref['out_sigma'].numpy(), rtol=1e-4, atol=5e-5)      # test_query_points_vs_oracle's bounds
    np.testing.assert_allclose(rgb.cpu().numpy(), ref['out_rgb'].numpy(), rtol=0, atol=2e-5)
    # densities only, and the interleaved plane layout: the same bits
    only, none = gnerf_hip.query_points(case['nhwc'], N, case['dec_dev'], case['pts_dev'], 1.0, want_rgb=False)
    assert none is None and torch.equal(only, sigma)
    si, ci = gnerf_hip.query_points(case['inter'], N, case['dec_dev'], case['pts_dev'], 1.0)
    assert torch.equal(si, sigma) and torch.equal(ci, rgb)
    assert torch.equal(gnerf_hip.query_points(case['inter'], N, case['dec_dev'], case['pts_dev'], 1.0, want_rgb=False)[0], sigma)
    # the far tile (a later trip, item 2): the decoder's value at zero features -- what the kernel gives for one point on all-zero planes
    zero_s, zero_c = gnerf_hip.query_points(torch.zeros_like(case['nhwc'][:3]), 1, case['dec_dev'], torch.zeros(1, 1, 3, device=dev), 1.0)
    item, sl = _tile(FAR)
    assert torch.equal(sigma[item, sl], zero_s[0].expand(16, 1)) and torch.equal(rgb[item, sl], zero_c[0].expand(16, 32))


def test_forward_box_warp_2_is_bit_identical(dev, case):
    """box_warp = 2 with the points doubled reads the same plane coordinates: the kernel multiplies a point by float(2.0 / box_warp), which
    is exactly 2 and exactly 1 for the two calls, and doubling a float32 only raises its exponent (no coordinate here is near overflow or
    subnormal), so 2 * p and (2 p) * 1 are the same float."""
    import gnerf_hip
    a = gnerf_hip.query_points(case['nhwc'], N, case['dec_dev'], case['pts_dev'], 1.0)
    b = gnerf_hip.query_points(case['nhwc'], N, case['dec_dev'], case['pts_dev'] * 2, 2.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('n_points', [1, 16, 17])
def test_forward_and_backward_tile_edges(dev, case, n_points):
    import gnerf_hip
    from oracle import render_ref as R
    pts, gs, gc = case['pts'][:, :n_points].contiguous(), case['g_sigma'][:, :n_points].contiguous(), case['g_rgb'][:, :n_points].contiguous()
    pl = case['planes'].double().requires_grad_(True)
    dc = [t.double().requires_grad_(True) for t in case['dec']]
    ref_sigma, ref_rgb = R.query_points(pl, dc, pts.double(), 1.0)
    sigma, rgb = gnerf_hip.query_points(case['nhwc'], N, case['dec_dev'], pts.to(dev), 1.0)
    np.testing.assert_allclose(sigma.cpu().numpy(), ref_sigma.detach().numpy(), rtol=1e-4, atol=5e-5)
    np.testing.assert_allclose(rgb.cpu().numpy(), ref_rgb.detach().numpy(), rtol=0, atol=2e-5)
    ref = torch.autograd.grad((ref_sigma * gs.double()).sum() + (ref_rgb * gc.double()).sum(), [pl] + dc)
    gp, gd = _backward(case, gs.to(dev), gc.to(dev), pts=pts.to(dev))
    errs = [_rel(gp, ref[0])] + [_rel(a, b) for a, b in zip(gd, ref[1:])]
    print(f'P = {n_points}: planes, w1, b1, w2, b2 rel ' + ' '.join(f'{e:.3e}' for e in errs))
    assert max(errs) < BOUND
    assert bool((gp[ref[0] == 0] == 0).all())


def test_backward_box_warp_2_is_bit_identical(dev, case):
    """As the forward: the same plane coordinates, so the same taps, weights and decoder; dL/dplanes does not depend on box_warp otherwise.
    One tile per item (P = 16): each item's planes are then written by one wave in program order, and the float sums have one order."""
    pts, gs, gc = case['pts_dev'][:, :16].contiguous(), case['gs_dev'][:, :16].contiguous(), case['gc_dev'][:, :16].contiguous()
    a = _backward(case, gs, gc, pts=pts, need_decoder=False)[0]
    b = _backward(case, gs, gc, pts=pts * 2, box_warp=2.0, need_decoder=False)[0]
    assert bool((a != 0).any()) and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- position gradient

@pytest.mark.parametrize('form', list(FORMS))
def test_point_gradient_all_points(dev, case, form):
    import gnerf_hip
    use_sigma, use_rgb = FORMS[form]
    run = lambda: gnerf_hip.query_points_grad(case['nhwc'], N, case['dec_dev'], case['pts_dev'], 1.0,
                                              case['gs_dev'] if use_sigma else None, case['gc_dev'] if use_rgb else None)
    first = run()
    assert first.shape == (N, P, 3) and bool(torch.isfinite(first).all())
    assert torch.equal(first, run())                                                   # no atomics: the same bits
    got, ref, keep = first.cpu(), case['ref'][form]['pts'], ~case['near']
    err = _rel(got[keep], ref[keep])
    print(f'{form}: rel {err:.3e} over {int(keep.sum())} of {N * P} points')
    assert err < BOUND
    for g in PROBES:                                                                   # ... and of each probe tile's own largest entry
        item, sl = _tile(g)
        if g == FAR:
            assert torch.equal(got[item, sl], torch.zeros(16, 3)) and bool((ref[item, sl] == 0).all())
            continue
        err = _rel(got[item, sl], ref[item, sl])
        print(f'{form}: tile {g}: rel {err:.3e}')
        assert err < BOUND, g


# ---------------------------------------------------------------------------------------------------------------- backward, probes

def _check_probe(got_planes, got_dec, ref_planes, ref_dec, what):
    errs = {}
    if got_planes is not None:
        zero = ref_planes == 0
        stray = int((got_planes[zero] != 0).sum())
        assert stray == 0, f'{what}: {stray} plane-gradient entries are non-zero where the oracle has exact zeros'
        errs['planes'] = _rel(got_planes, ref_planes)
    if got_dec is not None:
        errs.update({k: _rel(a, b) for k, a, b in zip(('w1', 'b1', 'w2', 'b2'), got_dec, ref_dec)})
    print(f'{what}: ' + ' '.join(f'{k} {e:.3e}' for k, e in errs.items()))
    assert max(errs.values()) < BOUND, (what, errs)


@pytest.mark.parametrize('g', PROBES)
def test_backward_one_probe_tile(dev, case, g):
    """Incoming gradients zero except on tile g's live points: the result is that tile's contribution alone, compared with the oracle on
    those <= 16 points at the project's bound taken against the probe's own largest entry.  Exact zeros where the oracle has them: every
    texel of the other items and every texel the tile's taps do not reach."""
    gs, gc = _masked(case, [g])
    gp, gd = _backward(case, gs, gc)
    ref_planes, ref_dec = case['probe'][g]
    item = _tile(g)[0]
    assert bool((ref_planes[[i for i in range(N) if i != item]] == 0).all())
    if g == FAR:
        assert bool((ref_planes == 0).all()) and torch.equal(gp, torch.zeros_like(gp))
        assert bool((ref_dec[0] == 0).all()) and float(ref_dec[2].abs().max()) > 0    # dW1 = dH^T X with X = 0; the rest does not depend on taps
    else:
        assert float(ref_planes[item].abs().max()) > 0
    _check_probe(gp, gd, ref_planes, ref_dec, f'tile {g}')


def test_backward_all_probe_tiles_decoder_only_and_planes_only(dev, case):
    """The seven probe tiles at once: accumulators that survive from trip to trip show in the decoder gradients."""
    gs, gc = _masked(case, PROBES)
    ref_planes, ref_dec = case['probe']['all']
    gp, gd = _backward(case, gs, gc, need_planes=False)
    assert gp is None
    _check_probe(None, gd, ref_planes, ref_dec, 'probes, decoder only')
    gp, gd = _backward(case, gs, gc, need_decoder=False)
    assert gd is None
    _check_probe(gp, None, ref_planes, ref_dec, 'probes, planes only')
    gp, gd = _backward(case, gs, gc)
    _check_probe(gp, gd, ref_planes, ref_dec, 'probes, both')


# ---------------------------------------------------------------------------------------------------------------- backward, dense

@pytest.mark.parametrize('form', list(FORMS))
def test_backward_dense(dev, case, form):
    """The whole scene with random incoming gradients at test_render_backward_vs_oracle's bounds."""
    use_sigma, use_rgb = FORMS[form]
    gp, gd = _backward(case, case['gs_dev'] if use_sigma else None, case['gc_dev'] if use_rgb else None)
    ref = case['ref'][form]
    for name, a, b in [('planes', gp, ref['planes'])] + [(k, x, y) for k, x, y in zip(('w1', 'b1', 'w2', 'b2'), gd, ref['dec'])]:
        if name in ('w2', 'b2'):                                # sigma only: the colour rows get nothing; rgb only: the density row
            rows = slice(0, 1) if form == 'sigma' else slice(1, 33) if form == 'rgb' else slice(0, 33)
            other = torch.ones(33, dtype=torch.bool)
            other[rows] = False
            assert bool((b[other] == 0).all()) and bool((a[other] == 0).all())
        rel, l2, ok = _rel(a, b), _rel_l2(a, b), _entrywise_ok(a, b)
        print(f'{form}: {name}: rel {rel:.3e} l2 {l2:.3e} entrywise {ok}')
        assert rel < 2e-3 and l2 < 1e-3 and ok, (form, name)


def test_backward_dense_interleaved_within_run_to_run_spread(dev, case):
    """The two plane layouts differ only in the order of the float atomics, as two runs of one layout do: the interleaved result is
    allowed 4 times the spread of two runs of the separate layout (each figure of the largest entry of its tensor).
    Measured on an MI355X, spread / interleaved against separate: planes 4.8e-7 / 4.8e-7, w1 8.2e-7 / 9.3e-7, b1 7.6e-7 / 6.7e-7,
    w2 1.0e-6 / 8.3e-7, b2 5.3e-7 / 7.3e-7."""
    names = ('planes', 'w1', 'b1', 'w2', 'b2')
    flat = lambda r: dict(zip(names, [r[0]] + r[1]))
    a, b = flat(_backward(case, case['gs_dev'], case['gc_dev'])), flat(_backward(case, case['gs_dev'], case['gc_dev']))
    c = flat(_backward(case, case['gs_dev'], case['gc_dev'], layout='inter'))
    for k in names:
        spread, err = _rel(b[k], a[k]), _rel(c[k], a[k])
        print(f'{k}: run-to-run spread {spread:.3e}, interleaved against separate {err:.3e}')
        assert err <= 4 * spread, k
    assert _rel(c['planes'], case['ref']['both']['planes']) < 2e-3


# ---------------------------------------------------------------------------------------------------------------- n_points guard

@pytest.mark.parametrize('entry', ['gnerf_query_points', 'gnerf_query_points_backward', 'gnerf_query_points_grad'])
def test_too_many_points_is_refused_before_the_pointers(entry):
    """The kernels index pts[idx * 3 + k] and 16 * t + j in int: n_points above (INT32_MAX - 15) / 3 is GNERF_E_ARG.  Every pointer is
    null, so no launch is possible either way: at the limit itself the same call stops at the null-pointer check."""
    import gnerf_hip
    from gnerf_hip import _native
    lib = gnerf_hip.load()
    limit = (2 ** 31 - 1 - 15) // 3
    assert limit == 715827877
    n_pointers = sum(t is ctypes.c_void_p for t in _native.SIGNATURES[entry][1]) - 3          # planes, points, ..., stream
    call = lambda n: getattr(lib, entry)(None, 3, 24, 20, None, n, 1.0, *[None] * n_pointers, 0, None)
    assert call(limit + 1) == -1                                                              # GNERF_E_ARG
    text = lib.gnerf_last_error()
    assert b'too many points' in text and str(limit + 1).encode() in text and entry[len('gnerf_'):].encode() + b':' in text
    assert call(limit) == -1 and b'too many points' not in lib.gnerf_last_error() and b'null' in lib.gnerf_last_error()
