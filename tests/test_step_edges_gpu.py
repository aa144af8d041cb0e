"""The two launches in front of the render kernel in bench.py's step, at the edges of their own loops: the 16-byte plane repack's walk
over its units (fewer pixels than one trip, ragged ends, a grid smaller than the walks, the workload's plane) with max |planes| placed
where a clamped or a last vector would lose it, and the rays-and-draws launch's quads of Philox threads (fewer elements than one block
per thread, several blocks per thread, odd sizes).  Exact equality against the PyTorch ops they replace."""

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


def _ref(x):
    return x.reshape(-1, *x.shape[-3:]).permute(0, 2, 3, 1).contiguous()


def _check_repack(x):
    import gnerf_hip
    ref = _ref(x)
    assert torch.equal(gnerf_hip.planes_to_nhwc(x), ref)
    out, amax = gnerf_hip.planes_to_nhwc(x, with_absmax=True)
    assert torch.equal(out, ref)
    assert amax.shape == (1,) and float(amax) == float(x.abs().max())


# fewer pixels than one trip; h w % 4 == 0 and ragged against every tile size; several units per plane; one item of the workload's planes
_SHAPES = [(1, 3, 32, 4, 4), (1, 3, 32, 12, 12), (2, 3, 32, 20, 52), (1, 3, 32, 256, 256)]


@pytest.mark.parametrize('shape', _SHAPES)
def test_repack_16_byte_form(dev, shape):
    _check_repack(torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))).to(dev))


@pytest.mark.parametrize('grid', [1, 4])
def test_repack_walks_a_small_grid(dev, monkeypatch, grid):
    """[2,3,32,20,52] has 54 units of 128 pixels, far fewer than the resident grid: GNERF_REPACK_GRID (test only) makes the launch one of
    `grid` workgroups, each of which then takes several walks -- and the absmax reduction has `grid` members instead of one per walk."""
    monkeypatch.setenv('GNERF_REPACK_GRID', str(grid))
    x = torch.randn(2, 3, 32, 20, 52, generator=torch.Generator().manual_seed(grid)).to(dev)
    _check_repack(x)
    x.view(-1)[-1] = -77.5                                                 # the last walk's last vector
    _check_repack(x)
    monkeypatch.delenv('GNERF_REPACK_GRID')
    _check_repack(x)


@pytest.mark.parametrize('where,value', [('first', 9.5), ('last', 9.5), ('first', -9.5), ('last', -9.5), ('first', float('inf')), ('last', float('inf'))])
def test_repack_absmax_in_the_first_and_last_vector(dev, where, value):
    """[1,3,32,12,12]: 144 pixels, so the second unit's lanes past pixel 143 load a clamped duplicate of the last vector.  The maximum is
    returned exactly from the first vector, from the last one, when it is negative, and when it is +inf."""
    import gnerf_hip
    x = torch.randn(1, 3, 32, 12, 12, generator=torch.Generator().manual_seed(5)).clamp(-4, 4).to(dev)
    for k in range(4):                                                     # every element of that 16-byte vector in turn
        y = x.clone()
        y.view(-1)[k if where == 'first' else y.numel() - 4 + k] = value
        out, amax = gnerf_hip.planes_to_nhwc(y, with_absmax=True)
        assert torch.equal(out, _ref(y))
        assert float(amax) == abs(value), (where, value, k)


def test_repack_refuses_odd_pixel_counts(dev):
    """h w % 4 != 0 is not for the 16-byte form: the general kernel's result."""
    _check_repack(torch.randn(1, 3, 32, 5, 7, generator=torch.Generator().manual_seed(2)).to(dev))


def _draw_cases(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    big = (1, 256, 48, 1)
    assert big[0] * big[1] ** 2 * big[2] > 256 * cus * 8 * 4               # more elements than four per thread of ATen's largest grid
    # fewer elements than one Philox block per thread; several blocks per thread; threads walk the grid stride more than once; S, F odd
    # (the second with element counts that are no multiple of four)
    return [(1, 2, 3, 2), (2, 16, 48, 48), big, (1, 5, 7, 3), (3, 33, 47, 45)]


def test_draws_equal_torch_rand(dev):
    import gnerf_hip
    import gnerf_harness as H
    gen = torch.cuda.default_generators[dev.index]
    for case, (n, res, S, F) in enumerate(_draw_cases(dev)):
        c2w = torch.cat([H.orbit_pose(3 + 5 * i, 120) for i in range(n)]).to(dev)
        intr = torch.tensor(H.FFHQ_INTRINSICS, device=dev).reshape(1, 3, 3).repeat(n, 1, 1)
        torch.cuda.manual_seed(2 ** 33 + case)
        torch.rand(5, device=dev)                                          # (an offset that is not zero)
        state = torch.cuda.get_rng_state(dev)
        o0, d0 = gnerf_hip.make_rays(c2w, intr, res)
        a0 = torch.rand([n, res * res, S, 1], device=dev)
        b0 = torch.rand(n * res * res, F, device=dev)
        after = int(gen.get_offset())
        torch.cuda.set_rng_state(state, dev)
        o1, d1, a1, b1 = gnerf_hip.make_rays_and_draws(c2w, intr, res, S, F)
        tag = (n, res, S, F)
        assert int(gen.get_offset()) == after, tag
        assert torch.equal(o0, o1) and torch.equal(d0, d1), tag
        assert a1.shape == a0.shape and torch.equal(a0.view(torch.int32), a1.view(torch.int32)), tag
        assert b1.shape == b0.shape and torch.equal(b0.view(torch.int32), b1.view(torch.int32)), tag
