"""On-demand dealing of ray units in the pipelined render kernel (render_pipe.inl, pipe_dealing.h) against the static dealing it
replaces (GNERF_PIPE_DEALING=static, read per call).  Which workgroup renders a ray changes nothing in the ray's arithmetic, so the
outputs must agree BIT FOR BIT; every ray must be rendered (outputs pre-filled with NaN come back finite); and the per-XCD counters
must be back at zero behind every call -- consecutive calls and replays of a captured HIP graph give the same bits, and the workspace
reads idle."""

import ctypes

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
    import math
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
    return dict(nhwc=nhwc, amax=amax, dec=tuple(t.to(dev) for t in dec), o=o.to(dev).contiguous(), d=d.to(dev).contiguous(), nc=nc.to(dev), nf=nf.to(dev),
                n=n_items, m=rays_per_item, res=res, S=S, F=F, c2w=c2w.to(dev), intr=intr.to(dev))


def _render(sc, out, generated=False):
    """gnerf_render_forward into the caller's (pre-filled) output tensors, on the current stream."""
    import gnerf_hip
    dev = sc['nhwc'].device
    if generated:
        torch.manual_seed(1234)             # the in-kernel draws follow the device generator: same state for every call compared
        rays, extra = (None, None, None, None), (( sc['c2w'], sc['intr'], sc['res']), gnerf_hip.torch_philox_plan(dev, sc['n'], sc['m'], sc['S'], sc['F']))
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


def _workspace_words(dev):
    import gnerf_hip
    torch.cuda.synchronize()
    return gnerf_hip._workspace(dev).view(torch.int32).cpu()


def _assert_idle(dev):
    """the depth range, the clamp's ticket and the eight dealing counters (the last 8 lines of 32 words) are zero"""
    w = _workspace_words(dev)
    assert int(w[0]) == 0 and int(w[1]) == 0 and int(w[3]) == 0
    assert not bool(w[16:16 + 2 * 4096].any())
    assert not bool(w[len(w) - 8 * 32:].any()), w[len(w) - 8 * 32:].reshape(8, 32)[:, 0].tolist()


# name -> (items, rays per item, image width (0: no tile order), coarse, fine, plane side, in-kernel rays and draws)
CASES = {
    'config2': (4, 128 * 128, 128, 48, 48, 256, False),                # pipe<1>, FULL instantiation, 1024 workgroups, 8 units each
    'config2_generated': (4, 128 * 128, 128, 48, 48, 256, True),       # the instantiation that makes its rays (a unit at a time) and draws
    'ragged_1_item': (1, 10007, 0, 48, 48, 64, False),                 # rays per item not a multiple of 8 or 16; short last units
    'ragged_3_items': (3, 4099, 0, 40, 32, 64, False),                 # ... over items, general instantiation (sample counts below the slots')
    'pipe2': (4, 64 * 64, 64, 96, 96, 64, False),                      # pipe<2>: 768 workgroups
    'small_static': (1, 64 * 64, 64, 48, 48, 64, False),               # fewer than 8 rays per workgroup slot: static dealing either way
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_on_demand_dealing_equals_static_dealing_bit_for_bit(dev, case, monkeypatch):
    n, m, res, S, F, plane, generated = CASES[case]
    sc = _scene(dev, n, m, res, S, F, plane, seed=7)
    _assert_idle(dev)
    monkeypatch.delenv('GNERF_PIPE_DEALING', raising=False)
    first = _outputs(sc)
    _render(sc, first, generated)
    _assert_idle(dev)                                       # counters back at zero inside the call
    for t in first:
        assert bool(torch.isfinite(t).all()), f'{case}: rays left unrendered: {int((~torch.isfinite(t)).sum())} values'
    second = _outputs(sc)
    _render(sc, second, generated)                          # a second call finds the counters where a first call does
    _assert_idle(dev)
    monkeypatch.setenv('GNERF_PIPE_DEALING', 'static')
    static = _outputs(sc)
    _render(sc, static, generated)
    _assert_idle(dev)
    for name, a, b, c in zip(('rgb', 'depth', 'weights_sum'), first, second, static):
        assert bool(torch.isfinite(c).all())
        assert torch.equal(a, c), f'{case}: {name} differs between on-demand and static dealing in {int((a != c).sum())} values'
        assert torch.equal(a, b), f'{case}: {name} differs between two on-demand calls'


@pytest.mark.parametrize('case', ['config2', 'ragged_3_items'])
def test_graph_replays_leave_the_counters_at_zero(dev, case, monkeypatch):
    """The reset is part of the captured sequence (clamp_depth_kernel's last block), nothing on the host: three replays, same bits."""
    import gnerf_hip
    n, m, res, S, F, plane, generated = CASES[case]
    monkeypatch.delenv('GNERF_PIPE_DEALING', raising=False)
    sc = _scene(dev, n, m, res, S, F, plane, seed=11)
    eager = _outputs(sc)
    _render(sc, eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = _outputs(sc)
    with torch.cuda.stream(side):
        keep = _render(sc, out)                             # (this stream's workspace is made here, outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        keep = _render(sc, out)
    for replay in range(3):
        for t in out:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(('rgb', 'depth', 'weights_sum'), eager, out):
            assert torch.equal(a, b), f'{case}: {name} of replay {replay} differs from the eager call in {int((a != b).sum())} values'
        ws = gnerf_hip._workspaces[(dev.index, side.cuda_stream)].view(torch.int32).cpu()
        assert int(ws[0]) == 0 and int(ws[1]) == 0 and int(ws[3]) == 0 and not bool(ws[len(ws) - 8 * 32:].any())
    del keep
