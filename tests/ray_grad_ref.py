"""Shared by tests/test_ray_grad_cpu.py and tests/test_ray_grad_gpu.py: the scenes, the float64 oracle's ray gradient (computed once per
case and kept), and the rays whose samples sit on a texel-cell boundary, where the bilinear derivative jumps."""

import functools

import numpy as np
import torch

RAY_START, RAY_END = 2.25, 3.3

# name -> (scene arguments, box_warp, white_back).  The smallest shapes at which the ray-gradient kernel can still go wrong.
CASES = {
    'one_masked_step': (dict(N=3, res=4, S=4, F=5, hw=(4, 4)), 1.0, False),                 # 9 samples: one masked step
    'ragged_everything': (dict(N=1, res=5, S=17, F=30, hw=(9, 11)), 1.0, False),            # 47 samples, 25 rays
    'ragged_items': (dict(N=3, res=5, S=20, F=24, hw=(12, 10)), 1.0, False),                # 25 rays per item: linear_pad
    'training_counts': (dict(N=2, res=8, S=48, F=48, hw=(32, 32)), 1.0, False),
    'several_trips': (dict(N=1, res=4, S=96, F=96, hw=(16, 16)), 1.0, False),               # 192 samples
    'several_trips_white': (dict(N=1, res=4, S=96, F=96, hw=(16, 16)), 1.0, True),
    'no_importance': (dict(N=1, res=4, S=12, F=0, hw=(8, 8)), 1.0, False),
    'wave_route': (dict(N=1, res=4, S=145, F=20, hw=(8, 8)), 1.0, False),                   # beyond the pipelined kernels: one wave per ray, staged
    'box_warp_2': (dict(N=2, res=8, S=48, F=48, hw=(32, 32)), 2.0, False),                  # rays scaled by 2: the same texels through box_scale = 1
}
PIPELINED = [k for k in CASES if k != 'wave_route']
SEED = 11
MAX_LEFT_OUT = 0.25


def random_scene(seed, N, res, S, F, hw, scale=1.5):
    """tests/test_gpu_parity.py's _random_scene."""
    from oracle import render_ref as R
    gen = torch.Generator().manual_seed(seed)
    planes = torch.randn(N, 3, 32, hw[0], hw[1], generator=gen) * scale
    dec = R.fold_decoder(torch.randn(64, 32, generator=gen), torch.randn(64, generator=gen) * 0.2,
                         torch.randn(33, 64, generator=gen), torch.randn(33, generator=gen) * 0.2)
    c2w = torch.cat([R.lookat_pose(3.14 / 2 + 0.5 * np.sin(1.0 + i), 3.14 / 2 - 0.05 + 0.2 * np.cos(2.0 * i), 2.7) for i in range(N)])
    intr = torch.tensor([[4.2647, 0, 0.5], [0, 4.2647, 0.5], [0, 0, 1]]).repeat(N, 1, 1)
    o, d = R.make_rays(c2w, intr, res)
    nc = torch.rand(N, res * res, S, generator=gen)
    nf = torch.rand(N * res * res, max(F, 1), generator=gen)[:, :F]
    return planes, dec, o, d, nc, nf


def options(S, F, box_warp=1.0, white_back=False):
    return dict(depth_resolution=S, depth_resolution_importance=F, ray_start=RAY_START, ray_end=RAY_END, box_warp=box_warp, clamp_mode='softplus',
                white_back=white_back)


def boundary_distance(o, d, depths, hw, box_warp):
    """[N*M]: per ray, the smallest distance in texels of any of its samples to a cell boundary of any plane (pixel coordinate an
    integer: there floor() switches taps and the bilinear derivative jumps).  o, d [N,M,3] and depths [N*M,K] in float64."""
    from oracle import render_ref as R
    pts = o.reshape(-1, 1, 3) + depths[:, :, None] * d.reshape(-1, 1, 3)
    uv = R.plane_uv(pts, box_warp)                                       # [3, R, K, 2]
    H, W = hw
    ix = ((uv[..., 0] + 1) * W - 1) / 2
    iy = ((uv[..., 1] + 1) * H - 1) / 2
    dist = torch.minimum((ix - torch.round(ix)).abs(), (iy - torch.round(iy)).abs())
    return dist.amin(dim=(0, 2))


class Reference:
    """One case: inputs (float32, CPU), upstream gradients, the float64 oracle's gradients and the rays compared."""

    def __init__(self, name, seed=SEED):
        from oracle import render_ref as R
        cfg, box_warp, white_back = CASES[name]
        self.name, self.cfg, self.box_warp, self.white_back = name, cfg, box_warp, white_back
        self.N, self.S, self.F, self.M = cfg['N'], cfg['S'], cfg['F'], cfg['res'] ** 2
        self.planes, self.dec, o, d, self.nc, self.nf = random_scene(seed, **cfg)
        self.o, self.d = o * box_warp, d * box_warp                      # p (2 / box_warp) is what the planes see
        gen = torch.Generator().manual_seed(5)
        self.g_rgb = torch.randn(self.N, self.M, 32, generator=gen)
        self.g_depth = torch.randn(self.N, self.M, 1, generator=gen)
        self.g_wsum = torch.randn(self.N, self.M, 1, generator=gen)
        self.opts = options(self.S, self.F, box_warp, white_back)
        self.grad_o, self.grad_d, self.grad_planes, self.grad_dec, depths = self.oracle(self.g_rgb, self.g_depth, self.g_wsum)
        self.distance = boundary_distance(self.o.double(), self.d.double(), depths, cfg['hw'], box_warp)
        self.keep = (self.distance >= 1e-4).reshape(self.N, self.M)      # rays compared; the rest must only be finite
        self.left_out = 1.0 - float(self.keep.double().mean())

    def oracle(self, g_rgb, g_depth, g_wsum, dtype=torch.float64):
        from oracle import render_ref as R
        o = self.o.to(dtype).requires_grad_(True)
        d = self.d.to(dtype).requires_grad_(True)
        pl = self.planes.to(dtype).requires_grad_(True)
        dc = [t.to(dtype).requires_grad_(True) for t in self.dec]
        stages = {}
        rgb, depth, w = R.render(pl, dc, o, d, self.opts, self.nc.to(dtype), self.nf.to(dtype), stages=stages)
        ((rgb * g_rgb.to(dtype)).sum() + (depth * g_depth.to(dtype)).sum() + (w * g_wsum.to(dtype)).sum()).backward()
        depths = stages['depths_all' if self.F > 0 else 'depths_coarse'].detach()
        return o.grad, d.grad, pl.grad, [t.grad for t in dc], depths


@functools.lru_cache(maxsize=None)
def reference(name, seed=SEED):
    return Reference(name, seed)


def rel_max(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))
