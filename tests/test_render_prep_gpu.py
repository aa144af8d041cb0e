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


def test_render_params_four_forms(dev):
    """The one builder of gnerf_render_params: tensor rays or cameras, crossed with tensor noise or an rng plan.  Float32 contiguous
    arguments are passed by pointer (no conversion copy), every scalar field is its argument, and the fields of the alternative not
    taken stay null / zero.  Launches nothing."""
    import gnerf_hip
    N, res, S, F = 2, 4, 48, 48
    M = res * res
    planes = torch.randn(3 * N, 4, 4, 32, device=dev)
    dec = (torch.randn(64, 32, device=dev), torch.randn(64, device=dev), torch.randn(33, 64, device=dev), torch.randn(33, device=dev))
    o, d = torch.randn(N, M, 3, device=dev), torch.randn(N, M, 3, device=dev)
    c2w, intr = torch.randn(N, 4, 4, device=dev), torch.randn(N, 3, 3, device=dev)
    nc, nf = torch.rand(N * M, S, device=dev), torch.rand(N * M, F, device=dev)
    amax = torch.ones(1, device=dev)
    plan = gnerf_hip.torch_philox_plan(dev, N, M, S, F, advance=False)
    plan_fields = dict(rng_mode=1, rng_per_item=0, rng_seed=plan.seed, rng_offset_coarse=plan.offset_coarse, rng_offset_fine=plan.offset_fine,
                       rng_offset_item_stride=plan.item_stride, rng_threads_coarse=plan.threads_coarse, rng_threads_fine=plan.threads_fine)

    def build(rays, noise, rs=2.25, re=3.25, image_width=7, cameras=None, rng=None, F=F):
        return gnerf_hip._render_params(planes, N, dec, rays[0], rays[1], noise[0], noise[1], S, F, rs, re, 1.5, True, False, image_width, 'render_forward',
                                        amax, 'f32', False, True, cameras, rng)

    for with_cameras in (False, True):
        for with_rng in (False, True):
            p, keep, m = build((None, None) if with_cameras else (o, d), (None, None) if with_rng else (nc, nf),
                               cameras=(c2w, intr, res) if with_cameras else None, rng=plan if with_rng else None)
            tag = (with_cameras, with_rng)
            assert m == M and p.rays_per_item == M, tag
            want_ptr = dict(planes_nhwc=planes, w1=dec[0], b1=dec[1], w2=dec[2], b2=dec[3], planes_absmax=amax,
                            ray_origins=None if with_cameras else o, ray_dirs=None if with_cameras else d,
                            cam2world=c2w if with_cameras else None, intrinsics=intr if with_cameras else None,
                            noise_coarse=None if with_rng else nc, noise_fine=None if with_rng else nf,
                            ray_start_per_ray=None, ray_end_per_ray=None, sigma_noise_coarse=None, sigma_noise_fine=None,
                            out_rgb=None, out_depth=None, out_wsum=None, workspace=None, debug=None)
            for name, t in want_ptr.items():
                assert getattr(p, name) == (None if t is None else t.data_ptr()), (tag, name)
            want = dict(n_items=N, plane_h=4, plane_w=4, image_width=res if with_cameras else 7, depth_resolution=S, depth_resolution_importance=F,
                        ray_start=2.25, ray_end=3.25, box_warp=1.5, white_back=1, disparity_space_sampling=0,
                        mlp_mode=gnerf_hip.MLP_MODES['f32'], planes_interleaved=0, planes_shared=0, depth_clamp_per_item=1)
            want.update(plan_fields if with_rng else dict.fromkeys(plan_fields, 0))
            for name, v in want.items():
                assert getattr(p, name) == v, (tag, name)
    cams = (c2w, intr, res)
    with pytest.raises(RuntimeError, match='give rays or cameras, not both'):
        build((o, d), (nc, nf), cameras=cams)
    with pytest.raises(RuntimeError, match='give noise tensors or an rng plan, not both'):
        build((o, d), (nc, nf), rng=plan)
    with pytest.raises(RuntimeError, match='in-kernel rays / draws take scalar ray limits'):
        build((None, None), (nc, nf), rs=torch.full([N, M, 1], 2.25, device=dev), re=torch.full([N, M, 1], 3.3, device=dev), cameras=cams)
    with pytest.raises(RuntimeError, match='render_forward: noise_fine required when depth_resolution_importance > 0'):
        build((None, None), (nc, None), cameras=cams)
