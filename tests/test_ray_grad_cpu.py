"""CPU tests of the renderer's ray gradient: the float64 oracle's ray gradient is the derivative the GPU tests compare against (central
differences), the host-side predicate's truth table, the new export under the unchanged ABI version, render_backward's unchanged
default, and gnerf_harness.fit_camera on the PyTorch-op form."""

import ctypes
import inspect
import os
import re

import pytest
import torch

import ray_grad_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('cfg', [dict(N=1, res=4, S=12, F=0, hw=(8, 8)), dict(N=2, res=5, S=9, F=0, hw=(6, 10))])
def test_oracle_ray_gradient_is_the_derivative(cfg):
    """At F = 0 (no importance pass, so finite differences see no detached path): central differences in float64 along a random
    perturbation of every ray, step 1e-6, against autograd, per ray, to 1e-6 of the largest directional derivative -- on the rays with no
    sample within 1e-3 texels of a cell boundary, which a step of 1e-6 (x H/2 texels per unit at most) cannot move across it."""
    from oracle import render_ref as R
    planes, dec, o, d, nc, nf = RR.random_scene(RR.SEED, **cfg)
    N, M, S = cfg['N'], cfg['res'] ** 2, cfg['S']
    opts = RR.options(S, 0)
    gen = torch.Generator().manual_seed(5)
    g_rgb, g_depth, g_wsum = (torch.randn(N, M, k, generator=gen).double() for k in (32, 1, 1))
    do, dd = (torch.randn(N, M, 3, generator=gen).double() for _ in range(2))
    pl, dc, nc = planes.double(), [t.double() for t in dec], nc.double()

    def per_ray_loss(o_, d_, stages=None):
        rgb, depth, w = R.render(pl, dc, o_, d_, opts, nc, nf.double(), stages=stages)
        return (rgb * g_rgb).sum(-1) + (depth * g_depth).sum(-1) + (w * g_wsum).sum(-1)             # [N,M]: rays are independent

    o64, d64 = o.double().requires_grad_(True), d.double().requires_grad_(True)
    stages = {}
    per_ray_loss(o64, d64, stages).sum().backward()
    autograd = (o64.grad * do).sum(-1) + (d64.grad * dd).sum(-1)
    eps = 1e-6
    with torch.no_grad():
        central = (per_ray_loss(o.double() + eps * do, d.double() + eps * dd) - per_ray_loss(o.double() - eps * do, d.double() - eps * dd)) / (2 * eps)
    keep = (RR.boundary_distance(o.double(), d.double(), stages['depths_coarse'], cfg['hw'], 1.0) >= 1e-3).reshape(N, M)
    assert float(keep.double().mean()) >= 0.75, float(keep.double().mean())
    err = float((central - autograd)[keep].abs().max() / autograd[keep].abs().max())
    assert err <= 1e-6, err


def test_supported_truth_table(monkeypatch):
    import gnerf_hip
    sup, why = gnerf_hip.render_ray_grad_supported, gnerf_hip.render_ray_grad_refusal
    monkeypatch.delenv('GNERF_BWD_SCATTER', raising=False)
    assert gnerf_hip.render_ray_grad_available()
    assert sup(48, 48, 2.25, 3.3) and why(48, 48, 2.25, 3.3) is None
    assert sup(12, 0, 2.25, 3.3) and sup(2, 0) and sup(256, 256) and sup(145, 20, 0.1, 9)
    t = torch.zeros(4)
    for limits in (('auto', 'auto'), (t, t), (2.25, t), (t, 3.3)):
        assert not sup(48, 48, *limits) and "'auto'" in why(48, 48, *limits)
    assert not sup(48, 48, 2.25, 3.3, density_noise=0.5) and 'density_noise' in why(48, 48, 2.25, 3.3, density_noise=0.5)
    assert not sup(48, 48, 2.25, 3.3, views=True) and 'views' in why(48, 48, 2.25, 3.3, views=True)
    assert not sup(48, 48, 2.25, 3.3, staged_scatter=False) and 'single-pass' in why(48, 48, 2.25, 3.3, staged_scatter=False)
    for S, F in ((1, 0), (257, 0), (48, 257), (3, 5), (48, -1)):
        assert not sup(S, F, 2.25, 3.3) and 'samples' in why(S, F, 2.25, 3.3)
    monkeypatch.setenv('GNERF_BWD_SCATTER', 'direct')
    assert not sup(48, 48, 2.25, 3.3)


def test_export_is_declared_built_and_bound_without_an_abi_change():
    import gnerf_hip
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    m = re.search(r'\bint\s+gnerf_render_backward_rays\s*\(([^)]*)\)\s*;', header)
    assert m, 'gnerf_render_backward_rays is not declared'
    params = [a.strip() for a in m.group(1).split(',')]
    assert [a.split()[-1].lstrip('*') for a in params] == ['p', 'g', 'grad_origins', 'grad_dirs', 'stream']
    assert params[0].startswith('const gnerf_render_params*') and params[1].startswith('const gnerf_render_grads*')
    assert params[2].startswith('float*') and params[3].startswith('float*') and params[4].startswith('gnerf_stream_t')
    assert re.search(r'#define\s+GNERF_ABI_VERSION\s+15\b', header) and gnerf_hip.ABI_VERSION == 15
    res, args = gnerf_hip.SIGNATURES['gnerf_render_backward_rays']
    assert res is ctypes.c_int and len(args) == len(params)
    assert args[0]._type_ is gnerf_hip.RenderParams and args[1]._type_ is gnerf_hip.RenderGrads and all(a is ctypes.c_void_p for a in args[2:])
    assert 'gnerf_render_backward_rays' in gnerf_hip.OPTIONAL_SYMBOLS           # a library of the same version built before it still loads
    lib = gnerf_hip.load()
    assert lib.gnerf_abi_version() == 15
    assert lib.gnerf_render_backward_rays.argtypes == args
    # the struct the call shares with gnerf_render_backward has not grown
    assert [f[0] for f in gnerf_hip.RenderGrads._fields_] == ['grad_rgb', 'grad_depth', 'grad_wsum', 'grad_planes_nhwc', 'grad_w1', 'grad_b1', 'grad_w2',
                                                              'grad_b2', 'scatter_stage']


def test_render_backward_keeps_its_default_return():
    import gnerf_hip
    sig = inspect.signature(gnerf_hip.render_backward)
    assert sig.parameters['need_rays'].default is False and sig.parameters['need_rays'].kind is inspect.Parameter.KEYWORD_ONLY
    src = inspect.getsource(inspect.unwrap(gnerf_hip.render_backward))
    assert src.rstrip().endswith('return g_planes, g_dec')                     # the last statement: what every call without need_rays reaches
    assert src.count('return g_planes, g_dec, g_rays') == 1 and 'if need_rays:' in src
    from training.volumetric_rendering.renderer import ImportanceRenderer
    assert ImportanceRenderer.fused_ray_grad is False and ImportanceRenderer.fused_point_grad is True


class _TinyGenerator(torch.nn.Module):
    """What fit_camera needs of a generator: synthesis(ws, c, ...) -> {'image_raw'} through the ray sampler and the renderer."""

    def __init__(self):
        super().__init__()
        import gnerf_harness as H
        from training.volumetric_rendering.ray_sampler import RaySampler
        from training.volumetric_rendering.renderer import ImportanceRenderer
        gen = torch.Generator().manual_seed(2)
        self.planes = torch.nn.Parameter(torch.randn(1, 3, 32, 6, 6, generator=gen) * 3)
        self.decoder, self.renderer, self.ray_sampler = H.TriPlaneDecoder(), ImportanceRenderer(), RaySampler()
        self.opts = dict(depth_resolution=16, depth_resolution_importance=16, ray_start=2.25, ray_end=3.3, box_warp=1, clamp_mode='softplus',
                         disparity_space_sampling=False)

    def synthesis(self, ws, c, neural_rendering_resolution=None, **_):
        res = neural_rendering_resolution or 6
        o, d = self.ray_sampler(c[:, :16].view(-1, 4, 4), c[:, 16:25].view(-1, 3, 3), res)
        feat, depth, _ = self.renderer(self.planes, self.decoder, o, d, self.opts)
        img = feat.permute(0, 2, 1).reshape(1, 32, res, res)
        return {'image': img[:, :3], 'image_raw': img[:, :3], 'image_depth': depth.permute(0, 2, 1).reshape(1, 1, res, res)}


def test_fit_camera_reduces_its_loss_on_the_op_form():
    import gnerf_harness as H
    torch.manual_seed(0)
    G = _TinyGenerator()
    ws = torch.zeros(1, 1, 8)
    pose = (1.57, 1.52, 2.7)
    with torch.no_grad():
        target = G.synthesis(ws, H.camera_label(H.lookat_pose(*pose)), neural_rendering_resolution=6)['image_raw']
    traj = H.fit_camera(G, ws, target, pose[0] + 0.2, pose[1] - 0.1, pose[2] + 0.1, steps=12, lr=0.02, resolution=6)
    assert len(traj) == 13 and [t['step'] for t in traj] == list(range(13))
    assert all(not p.requires_grad for p in G.parameters())                     # frozen
    losses = [t['loss'] for t in traj]
    assert min(losses[-3:]) < 0.8 * losses[0], losses                           # (every step draws its own sample depths: the loss is noisy)
    moved = [abs(traj[-1][k] - traj[0][k]) for k in ('yaw', 'pitch', 'radius')]
    assert max(moved) > 0.01, moved
    # the pose is differentiable by its three parameters: the gradient fit_camera descends along is not zero
    loss, grad = H.camera_loss_gradient(G, ws, target, pose[0] + 0.2, pose[1] - 0.1, pose[2] + 0.1, resolution=6)
    assert loss > 0 and grad.shape == (3,) and bool((grad != 0).all())
