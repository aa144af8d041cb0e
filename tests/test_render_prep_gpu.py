"""The launches in front of the render kernel in bench.py's step: the NCHW -> NHWC plane repack with max |planes| (no fill launch in
front of it) and the rays with the two uniform draws.  Bit-exact against the PyTorch ops they replace."""

import pytest
import torch

from conftest import has_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not has_gpu():
        pytest.fail('GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)')
    import gnerf_hip
    gnerf_hip.load()
    return torch.device('cuda', 0)


def _bits_max_abs(x):
    """max |x| as the kernels order it: the sign-stripped bits compared as unsigned integers (NaN above +inf)."""
    b = x.reshape(-1).view(torch.int32) & 0x7fffffff
    return int(b.max())


# 16-byte form (32k channels, h w % 4 == 0, a ragged last tile), and the general form: odd sizes, channel counts other than 32
_SHAPES = [(4, 3, 32, 256, 256), (1, 3, 32, 20, 24), (2, 64, 12, 12), (1, 3, 32, 7, 5), (6, 40, 9, 13), (3, 16, 8, 8), (2, 1, 3, 3),
           (5, 96, 2, 6)]


@pytest.mark.parametrize('shape', _SHAPES)
def test_repack_equals_permute(dev, shape):
    import gnerf_hip
    x = torch.randn(*shape, device=dev)
    ref = x.reshape(-1, *shape[-3:]).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(gnerf_hip.planes_to_nhwc(x), ref)
    out, amax = gnerf_hip.planes_to_nhwc(x, with_absmax=True)
    assert torch.equal(out, ref)
    assert int(amax.view(torch.int32)) == _bits_max_abs(x)


def test_repack_unaligned_source_takes_the_general_form(dev):
    import gnerf_hip
    base = torch.randn(1 + 3 * 32 * 16 * 16, device=dev)
    x = base[1:].view(1, 3, 32, 16, 16)                                    # 4 bytes past a 16-byte boundary
    out, amax = gnerf_hip.planes_to_nhwc(x, with_absmax=True)
    assert torch.equal(out, x.reshape(3, 32, 16, 16).permute(0, 2, 3, 1).contiguous())
    assert int(amax.view(torch.int32)) == _bits_max_abs(x)


@pytest.mark.parametrize('shape', [(2, 3, 32, 64, 64), (1, 3, 32, 7, 5)])
def test_absmax_special_values(dev, shape):
    """NaN wins over everything, +-inf over finite values, -0 counts as 0, all-zero input gives +0; repeated calls on one stream
    (the workspace is left idle by each) agree."""
    import gnerf_hip
    x = torch.zeros(*shape, device=dev)
    for _ in range(3):
        a = gnerf_hip.planes_to_nhwc(x, with_absmax=True)[1]
        assert int(a.view(torch.int32)) == 0
    x.view(-1)[5] = -0.0
    assert int(gnerf_hip.planes_to_nhwc(x, with_absmax=True)[1].view(torch.int32)) == 0
    x = torch.randn(*shape, device=dev)
    x.view(-1)[-1] = -123.25
    assert float(gnerf_hip.planes_to_nhwc(x, with_absmax=True)[1]) == 123.25
    x.view(-1)[x.numel() // 2] = float('-inf')
    assert float(gnerf_hip.planes_to_nhwc(x, with_absmax=True)[1]) == float('inf')
    x.view(-1)[0] = float('nan')
    a = gnerf_hip.planes_to_nhwc(x, with_absmax=True)[1]
    assert torch.isnan(a).all() and int(a.view(torch.int32)) == _bits_max_abs(x)
    y = torch.randn(*shape, device=dev)                                    # and back: nothing of the NaN call is left over
    assert float(gnerf_hip.planes_to_nhwc(y, with_absmax=True)[1]) == float(y.abs().max())


def test_absmax_two_streams_at_once(dev):
    import gnerf_hip
    xs = [torch.randn(4, 3, 32, 256, 256, device=dev) * (1 + k) for k in range(2)]
    streams = [torch.cuda.Stream(dev) for _ in xs]
    torch.cuda.synchronize(dev)
    for rep in range(4):
        res = []
        for x, s in zip(xs, streams):
            with torch.cuda.stream(s):
                res.append(gnerf_hip.planes_to_nhwc(x, with_absmax=True))
        torch.cuda.synchronize(dev)
        for x, (out, amax) in zip(xs, res):
            assert int(amax.view(torch.int32)) == _bits_max_abs(x), rep
            assert torch.equal(out, x.reshape(-1, 32, 256, 256).permute(0, 2, 3, 1).contiguous())


def test_step_prep_has_no_fill_launch(dev):
    """bench.py's step in front of the render kernel: the repack with max |planes| and the rays with the draws are one launch
    each -- no memset / fill launch."""
    import gnerf_hip
    import gnerf_harness as H
    from torch.profiler import ProfilerActivity, profile
    planes = torch.randn(4, 3, 32, 64, 64, device=dev)
    c2w = torch.cat([H.orbit_pose(3 + 5 * i, 120) for i in range(4)]).to(dev)
    intr = torch.tensor(H.FFHQ_INTRINSICS, device=dev).reshape(1, 3, 3).repeat(4, 1, 1)
    gnerf_hip.planes_to_nhwc(planes, with_absmax=True)
    gnerf_hip.make_rays_and_draws(c2w, intr, 16, 48, 48)
    torch.cuda.synchronize(dev)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        gnerf_hip.planes_to_nhwc(planes, with_absmax=True)
        gnerf_hip.make_rays_and_draws(c2w, intr, 16, 48, 48)
        torch.cuda.synchronize(dev)
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [n for n in names if 'kernel' in n.lower() or 'fill' in n.lower()]
    assert any('nchw_to_nhwc' in n for n in kernels) and any('rays_and_draws' in n for n in kernels), names
    assert not any('fill' in n.lower() or 'memset' in n.lower() for n in names), names
    assert len(kernels) == 2, kernels
