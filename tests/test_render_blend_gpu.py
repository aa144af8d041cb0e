"""The texel blend of the fused renderer (csrc/render_shade.inl, shade_tile: one FMA per tap and channel, chained through a sample's
12 taps) on planes whose every value says where it came from, at the smallest size that fills every lane group of a tile.

Scene: 64 rays (the four middle rows of a 16 x 16 image), 8 x 8 x 32 tri-planes with value(plane, y, x, c) = plane + 0.11 c + 0.1 x +
1.3 y (+ 0.37 per item), centred and scaled to |v| < 2.4, so the device-side choice stays on the f16x3 decoder.  A swapped channel
pair, tap or plane, or a wrong item stride, changes the image by ten times the tolerance or more (measured on the oracle: two
neighbouring channels exchanged move rgb by 3e-3, two planes by 4e-3, a one-texel shift by 7e-3, two items by 3e-2; the density bias is raised so that the rays'
weights sum to about 0.6 and the colours count).  Held against oracle.render_ref.render at the tolerance
tests/test_gpu_parity.py::test_render_vs_oracle uses (rgb MSE < 1e-8; rgb, depth and weight sums within 2e-4), through the FULL
instantiation (48+48 samples) and the general one (12+12), in both plane layouts, with one item and with two."""

import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = pytest.mark.gpu

RES, ROWS = 16, (6, 10)         # a 16 x 4 image: rows 6..9 of the 16 x 16 one
OPTS = dict(ray_start=2.25, ray_end=3.3, box_warp=1.0)


@pytest.fixture(scope='module')
def dev():
    if not has_gpu():
        pytest.fail('GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)')
    import gnerf_hip
    gnerf_hip.load()
    return torch.device('cuda', 0)


def _coded_planes(N):
    item = torch.arange(N, dtype=torch.float32).view(N, 1, 1, 1, 1)
    plane = torch.arange(3, dtype=torch.float32).view(1, 3, 1, 1, 1)
    c = torch.arange(32, dtype=torch.float32).view(1, 1, 32, 1, 1)
    y = torch.arange(8, dtype=torch.float32).view(1, 1, 1, 8, 1)
    x = torch.arange(8, dtype=torch.float32).view(1, 1, 1, 1, 8)
    v = plane + 0.11 * c + 0.1 * x + 1.3 * y + 0.37 * item          # 0 .. 15.6
    return ((v - 7.8) * 0.3).contiguous()                           # [N, 3, 32, 8, 8], |v| < 2.4


@functools.lru_cache(maxsize=None)
def _scene(N, S, F):
    """(planes, decoder, origins, dirs, coarse draws, fine draws, the oracle's (rgb, depth, weight sums)): made once per shape, shared
    by the tests, never written to."""
    from oracle import render_ref as R
    gen = torch.Generator().manual_seed(18)
    planes = _coded_planes(N)
    w1, b1, w2, b2 = torch.randn(64, 32, generator=gen), torch.randn(64, generator=gen) * 0.2, torch.randn(33, 64, generator=gen), torch.randn(33, generator=gen) * 0.2
    b2[0] += 2.0                                                    # density: opaque enough for the colours to count
    dec = R.fold_decoder(w1, b1, w2, b2)
    c2w = torch.cat([R.lookat_pose(3.14 / 2 + 0.4 * np.sin(1.0 + i), 3.14 / 2 - 0.05 + 0.2 * np.cos(2.0 * i), 2.7) for i in range(N)])
    intr = torch.tensor([[4.2647, 0, 0.5], [0, 4.2647, 0.5], [0, 0, 1]]).repeat(N, 1, 1)
    o, d = R.make_rays(c2w, intr, RES)
    o = o.reshape(N, RES, RES, 3)[:, ROWS[0]:ROWS[1]].reshape(N, -1, 3).contiguous()
    d = d.reshape(N, RES, RES, 3)[:, ROWS[0]:ROWS[1]].reshape(N, -1, 3).contiguous()
    M = o.shape[1]
    assert M == 64
    nc = torch.rand(N, M, S, generator=gen)
    nf = torch.rand(N * M, F, generator=gen)
    opts = dict(depth_resolution=S, depth_resolution_importance=F, clamp_mode='softplus', **OPTS)
    ref = R.render(planes, dec, o, d, opts, nc, nf)
    return planes, dec, o, d, nc, nf, ref


def _laid_out(planes, layout, dev):
    import gnerf_hip
    N, H, W = planes.shape[0], planes.shape[3], planes.shape[4]
    if layout == 'planes':
        return gnerf_hip.planes_to_nhwc(planes.to(dev))                                             # [3N, H, W, 32]
    return planes.reshape(N, 96, H, W).permute(0, 2, 3, 1).contiguous().to(dev)                     # [N, H, W, 96]


def _render(dev, scene, layout, S, F, **kw):
    import gnerf_hip
    planes, dec, o, d, nc, nf = scene[:6]
    out = gnerf_hip.render_forward(_laid_out(planes, layout, dev), planes.shape[0], [t.to(dev) for t in dec], o.to(dev), d.to(dev),
                                   nc.to(dev), nf.to(dev), depth_resolution=S, depth_resolution_importance=F, image_width=RES, **OPTS, **kw)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


@pytest.mark.parametrize('layout', ['planes', 'interleaved'])
@pytest.mark.parametrize('S,F', [(48, 48), (12, 12)])           # the FULL instantiation, the general one
@pytest.mark.parametrize('N', [1, 2])                           # (the second item: the item stride of the addresses the blend consumes)
def test_blend_vs_oracle(dev, N, S, F, layout):
    scene = _scene(N, S, F)
    ref_rgb, ref_depth, ref_w = scene[6]
    rgb, depth, wsum = _render(dev, scene, layout, S, F)
    mse = float(((rgb - ref_rgb) ** 2).mean())
    print(f'N={N} {S}+{F} {layout}: rgb mse {mse:.3e}, max |rgb err| {float((rgb - ref_rgb).abs().max()):.3e}, '
          f'max |depth err| {float((depth - ref_depth).abs().max()):.3e}, max |wsum err| {float((wsum - ref_w).abs().max()):.3e}')
    assert mse < 1e-8, mse
    np.testing.assert_allclose(rgb.numpy(), ref_rgb.numpy(), atol=2e-4)
    np.testing.assert_allclose(depth.numpy(), ref_depth.numpy(), atol=2e-4)
    np.testing.assert_allclose(wsum.numpy(), ref_w.numpy(), atol=2e-4)


def test_coded_planes_tell_channels_taps_planes_and_items_apart():
    """The scene can show what it is for: no two neighbouring channels of a texel, no two neighbouring texels of a plane, no two planes and no two items hold
    the same value at the same place (so an exchange of any of them is an exchange of different numbers)."""
    p = _coded_planes(2)
    assert float(p.abs().max()) < 2.4
    assert (p[:, :, 1:] != p[:, :, :-1]).all() and (p[:, :, :, 1:] != p[:, :, :, :-1]).all() and (p[:, :, :, :, 1:] != p[:, :, :, :, :-1]).all()
    assert (p[:, 1:] != p[:, :-1]).all() and (p[1] != p[0]).all()


@pytest.mark.parametrize('mlp', ['f32', 'auto'])
def test_blend_routes_agree_bit_for_bit(dev, mlp):
    """Same inputs, two consecutive calls: each arithmetic agrees with itself bit for bit, and the call with the decoder's pack equals
    the plain one (every workgroup preparing the decoder itself)."""
    import gnerf_hip
    S = F = 48
    scene = _scene(2, S, F)
    pack = gnerf_hip.pack_decoder(tuple(t.to(dev).contiguous() for t in scene[1]))
    torch.cuda.synchronize()
    first = _render(dev, scene, 'planes', S, F, mlp=mlp, decoder_pack=False)
    second = _render(dev, scene, 'planes', S, F, mlp=mlp, decoder_pack=False)
    packed = _render(dev, scene, 'planes', S, F, mlp=mlp, decoder_pack=pack)
    for name, a, b, c in zip(('rgb', 'depth', 'weights_sum'), first, second, packed):
        assert torch.equal(a, b), f'{mlp}: {name} differs between two consecutive calls'
        assert torch.equal(a, c), f'{mlp}: {name} differs between the packed-decoder call and the plain one'
    assert all(bool(torch.isfinite(t).all()) for t in first)
