"""Guided dealing of ray units in the pipelined render kernel (render_pipe.inl, pipe_dealing.h: on demand, with units that shrink from
8 rays to 4, 2 and 1 as an XCD's range runs out -- the default) against on-demand dealing with fixed 8-ray units
(GNERF_PIPE_DEALING=uniform) and against static dealing (GNERF_PIPE_DEALING=static), both read per call.  Which workgroup renders a
ray changes nothing in the ray's arithmetic, so the outputs must agree BIT FOR BIT (tolerance zero); every ray must be rendered
(outputs pre-filled with NaN come back finite); consecutive calls and replays of a captured HIP graph give the same bits and leave
the workspace idle (the per-XCD counters, the clamp's ticket and the depth-range words all zero).

On-demand dealing engages from 8 192 rays (1 024 workgroup slots x 8): the cases are the smallest that reach it, one per
instantiation of the kernel, and one below the threshold that must take the static path whatever the switch says."""

import ctypes
import math

import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.production_path]


@pytest.fixture(scope='module')
def dev():
    if not has_gpu():
        pytest.fail('GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)')
    import gnerf_hip
    gnerf_hip.load()
    return torch.device('cuda', 0)


def _scene(dev, n_items, rays_per_item, res, S, F, plane, seed):
    """planes, decoder, rays (camera rays when res > 0, else rays of random pixels of such cameras) and the two draws."""
    import gnerf_hip
    from oracle import render_ref as R
    g = torch.Generator().manual_seed(seed)
    planes = torch.randn(n_items, 3, 32, plane, plane, generator=g)
    dec = (torch.randn(64, 32, generator=g) / math.sqrt(32), torch.zeros(64), torch.randn(33, 64, generator=g) / math.sqrt(64), torch.zeros(33))
    c2w = torch.cat([R.lookat_pose(3.14 / 2 + 0.2 * i, 3.14 / 2 - 0.1 * i, 2.7) for i in range(n_items)])
    intr = torch.tensor([[4.2647, 0, 0.5], [0, 4.2647, 0.5], [0, 0, 1]]).repeat(n_items, 1, 1)
    if res > 0:
        o, d = R.make_rays(c2w, intr, res)
    else:
        o, d = R.make_rays(c2w, intr, 128)
        pick = torch.stack([torch.randperm(128 * 128, generator=g)[:rays_per_item] for _ in range(n_items)])
        o, d = torch.gather(o, 1, pick[..., None].expand(-1, -1, 3)), torch.gather(d, 1, pick[..., None].expand(-1, -1, 3))
    nc, nf = torch.rand(n_items * rays_per_item, S, generator=g), torch.rand(n_items * rays_per_item, F, generator=g)
    nhwc, amax = gnerf_hip.planes_to_nhwc(planes.to(dev), with_absmax=True)
    return dict(planes=planes, nhwc=nhwc, amax=amax, dec=tuple(t.to(dev) for t in dec), o=o.to(dev).contiguous(), d=d.to(dev).contiguous(),
                nc=nc.to(dev), nf=nf.to(dev), n=n_items, m=rays_per_item, res=res, S=S, F=F, c2w=c2w.to(dev), intr=intr.to(dev))


def _plan(sc):
    """the in-kernel draws follow the device generator: same state for every call compared (made on the host, outside any capture)"""
    import gnerf_hip
    torch.manual_seed(1234)
    return gnerf_hip.torch_philox_plan(sc['nhwc'].device, sc['n'], sc['m'], sc['S'], sc['F'])


def _render(sc, out, generated=False, plan=None):
    """gnerf_render_forward (the ctypes binding) into the caller's pre-filled output tensors, on the current stream."""
    import gnerf_hip
    dev = sc['nhwc'].device
    if generated:
        rays, extra = (None, None, None, None), ((sc['c2w'], sc['intr'], sc['res']), plan if plan is not None else _plan(sc))
    else:
        rays, extra = (sc['o'], sc['d'], sc['nc'], sc['nf']), (None, None)
    p, keep, m = gnerf_hip._render_params(sc['nhwc'], sc['n'], sc['dec'], *rays, sc['S'], sc['F'], 2.25, 3.3, 1.0, False, False, sc['res'],
                                          'render_forward', sc['amax'], 'auto', False, False, *extra)
    assert m == sc['m']
    p.out_rgb, p.out_depth, p.out_wsum = (t.data_ptr() for t in out)
    p.workspace, p.debug = gnerf_hip._workspace(dev).data_ptr(), None
    gnerf_hip._check(gnerf_hip.load().gnerf_render_forward(ctypes.byref(p), gnerf_hip._stream(sc['nhwc'])), 'gnerf_render_forward')
    return keep


def _outputs(sc):
    dev = sc['nhwc'].device
    return tuple(torch.full([sc['n'], sc['m'], c], float('nan'), device=dev) for c in (32, 1, 1))


def _assert_idle_words(w):
    """the depth range, the clamp's ticket, the per-item depth ranges and the eight dealing counters (the last 8 lines of 32 words) are zero"""
    assert int(w[0]) == 0 and int(w[1]) == 0 and int(w[3]) == 0
    assert not bool(w[16:16 + 2 * 4096].any())
    assert not bool(w[len(w) - 8 * 32:].any()), w[len(w) - 8 * 32:].reshape(8, 32)[:, 0].tolist()


def _assert_idle(dev):
    import gnerf_hip
    torch.cuda.synchronize()
    _assert_idle_words(gnerf_hip._workspace(dev).view(torch.int32).cpu())


NAMES = ('rgb', 'depth', 'weights_sum')

# name -> (items, rays per item, image width (0: no tile order), coarse, fine, plane side, in-kernel rays and draws)
CASES = {
    'ragged_1_item': (1, 10007, 0, 48, 48, 64, False),      # FULL instantiation; XCD ranges of 1 250 / 1 251 rays: the 1- and 2-ray levels with their extra units
    'ragged_3_items': (3, 4099, 0, 40, 32, 64, False),      # general instantiation, workgroups straddling items; all three shrinking levels
    'pipe2': (4, 64 * 64, 64, 96, 96, 64, False),           # pipe<2>: 96 workgroups per XCD, every level full
    'generated': (1, 96 * 96, 96, 48, 48, 64, True),        # in-kernel rays and draws (GEN): a unit's rays made per shortened unit
    'small': (1, 64 * 64, 64, 48, 48, 64, False),           # below the threshold: static dealing whatever the switch says
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_guided_dealing_equals_uniform_and_static_dealing_bit_for_bit(dev, case, monkeypatch):
    n, m, res, S, F, plane, generated = CASES[case]
    sc = _scene(dev, n, m, res, S, F, plane, seed=7)
    _assert_idle(dev)
    monkeypatch.delenv('GNERF_PIPE_DEALING', raising=False)
    first = _outputs(sc)
    _render(sc, first, generated)
    _assert_idle(dev)                                       # counters back at zero inside the call
    for name, t in zip(NAMES, first):
        assert bool(torch.isfinite(t).all()), f'{case}: {name}: rays left unrendered: {int((~torch.isfinite(t)).sum())} values'
    second = _outputs(sc)
    _render(sc, second, generated)                          # a second call finds the counters where a first call does
    _assert_idle(dev)
    others = {}
    for mode in ('uniform', 'static'):
        monkeypatch.setenv('GNERF_PIPE_DEALING', mode)
        others[mode] = _outputs(sc)
        _render(sc, others[mode], generated)
        _assert_idle(dev)
    for i, name in enumerate(NAMES):
        assert torch.equal(first[i], second[i]), f'{case}: {name} differs between two guided calls in {int((first[i] != second[i]).sum())} values'
        for mode in ('uniform', 'static'):
            assert bool(torch.isfinite(others[mode][i]).all())
            assert torch.equal(first[i], others[mode][i]), f'{case}: {name} differs between guided and {mode} dealing in {int((first[i] != others[mode][i]).sum())} values'


@pytest.mark.parametrize('case', sorted(CASES))
def test_two_calls_then_three_graph_replays_give_the_same_bits_and_an_idle_workspace(dev, case, monkeypatch):
    """The counters' reset is part of the captured sequence (clamp_depth_kernel's last block), nothing on the host."""
    import gnerf_hip
    n, m, res, S, F, plane, generated = CASES[case]
    monkeypatch.delenv('GNERF_PIPE_DEALING', raising=False)
    sc = _scene(dev, n, m, res, S, F, plane, seed=11)
    eager = _outputs(sc)
    _render(sc, eager, generated)
    again = _outputs(sc)
    _render(sc, again, generated)
    _assert_idle(dev)
    for name, a, b in zip(NAMES, eager, again):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), f'{case}: {name} differs between two consecutive calls'
    plan = _plan(sc) if generated else None                 # (seed and offsets are plain launch arguments: the captured call replays them)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = _outputs(sc)
    with torch.cuda.stream(side):
        keep = _render(sc, out, generated, plan)            # (this stream's workspace is made here, outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        keep = _render(sc, out, generated, plan)
    for replay in range(3):
        for t in out:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(NAMES, eager, out):
            assert torch.equal(a, b), f'{case}: {name} of replay {replay} differs from the eager call in {int((a != b).sum())} values'
        _assert_idle_words(gnerf_hip._workspaces[(dev.index, side.cuda_stream)].view(torch.int32).cpu())
    del keep


def test_views_of_one_item_equal_separate_calls_bit_for_bit(dev, monkeypatch):
    """Three views of one object in one launch (planes_shared, per-item depth clamp; the C++ binding where it is built): 3 x 4 099 rays are
    dealt on demand with guided units and workgroups straddle the views; each view alone is a launch below the threshold."""
    import gnerf_hip
    monkeypatch.delenv('GNERF_PIPE_DEALING', raising=False)
    n, m, S, F = 3, 4099, 48, 48
    sc = _scene(dev, n, m, 0, S, F, 64, seed=13)
    nhwc, amax = gnerf_hip.planes_to_nhwc(sc['planes'][:1].to(dev), with_absmax=True)
    opts = dict(depth_resolution=S, depth_resolution_importance=F, ray_start=2.25, ray_end=3.3, box_warp=1.0, planes_absmax=amax)
    nc, nf = sc['nc'].view(n, m, S), sc['nf'].view(n, m, F)
    together = gnerf_hip.render_forward(nhwc, n, sc['dec'], sc['o'], sc['d'], sc['nc'], sc['nf'], planes_shared=True, depth_clamp_per_item=True, **opts)
    _assert_idle(dev)
    for i in range(n):
        alone = gnerf_hip.render_forward(nhwc, 1, sc['dec'], sc['o'][i:i + 1].contiguous(), sc['d'][i:i + 1].contiguous(), nc[i].contiguous(), nf[i].contiguous(), **opts)
        _assert_idle(dev)
        for name, a, b in zip(NAMES, together, alone):
            assert bool(torch.isfinite(a[i]).all())
            assert torch.equal(a[i:i + 1], b), f'view {i}: {name} differs from the view rendered alone in {int((a[i:i + 1] != b).sum())} values'
