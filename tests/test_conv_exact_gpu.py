"""The matrix-core convolutions of csrc/conv3x3.hip -- the plain 3x3 form with its fused epilogue, the stride-2 transposed form in its three
job shapes, the fp32-grade OUT32 form, the ToRGB tail -- held to EXACT results over the WHOLE output tensor.

The operands (tests/conv_exact_ref.py) are integers from {+-1, +-2, +-3} with dyadic epilogue operands: every product and every partial sum,
in any order, is an exact float32 number, so the kernel must reproduce an integer reference (nine shifted float64 matmuls / the scatter
definition of the transposed convolution, no code shared with torch's convolutions) bit for bit.  Every comparison below is torch.equal on
the full tensor; the conditions that make this the right demand are asserted on the reference inside the helper
(tests/test_conv_exact_cpu.py runs them without a GPU).  The shapes are the smallest at which each mechanism of the kernel exists: one tile
with a partly filled chunk, chunk changes under the weight double buffer's parity, interior tile seams, several channel groups, every
epilogue template, launches above the chip's 512 workgroup slots checked at every pixel, tile grids that overhang the odd phases.
A failure prints where the wrong outputs lie in the tile / wave / channel-block structure (conv_exact_ref.mismatch_report)."""

import itertools

import pytest
import torch

import conv_exact_ref as CX
from conftest import has_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not has_gpu():
        pytest.fail('GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)')
    import gnerf_hip
    gnerf_hip.load()
    yield torch.device('cuda', 0)
    CX.clear_cases()                                                # the cached references live on the device
    torch.cuda.empty_cache()


def _case(shape, dev, transposed=False):
    return CX.conv_case(tuple(shape), transposed, str(dev))


def _half_nhwc(t):
    return t.half().contiguous(memory_format=torch.channels_last)


def _same(got, want, transposed=False):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    assert torch.equal(got, want), CX.mismatch_report(got, want, transposed)


def _plain(case, **kw):
    import gnerf_hip
    x = _half_nhwc(case.x)
    assert gnerf_hip.conv3x3_epilogue_supported(x, case.weight.shape[0])
    return gnerf_hip.conv3x3_epilogue(x, gnerf_hip.pack_conv3x3_weights(case.weight), **kw)


def _epilogue_pair(shape, variant, dev):
    """(keyword arguments for the kernel: float32 tensors on the device, keyword arguments for the reference: float64 tensors there)."""
    kw = CX.epilogue_kwargs(shape, *variant)
    return CX.tensors_to(kw, dev, torch.float32), CX.tensors_to(kw, dev)


@pytest.mark.parametrize('shape', CX.PLAIN_IDENTITY, ids=str)
def test_plain_identity_epilogue_stores_the_integer_accumulator(dev, shape):
    """alpha = gain = 1, nothing else: y = fp16(acc), and |acc| <= 2048 is a float16 integer.  One tile with 56 zero-filled channels and all
    four borders; nine steps; a second, almost empty chunk; three chunks = 27 steps across interior tile seams, two images, two channel
    groups; eight chunks."""
    case = _case(shape, dev)
    CX.assert_bare_accumulator_fits_half(case.acc, str(shape))
    _same(_plain(case, alpha=1.0, gain=1.0), CX.to_half(case.acc))


@pytest.mark.parametrize('scale,noise,next_scale', list(itertools.product((False, True), repeat=3)))
def test_plain_every_epilogue_template(dev, scale, noise, next_scale):
    """The eight (scale, noise, next_scale) instantiations, each with and without the clamp (the epilogue's two register paths) and with
    round_noise both ways (integer noise: the rounding changes nothing), bias always: clamp(lrelu(acc scale + noise + bias) gain) next_scale
    in float64, rounded once."""
    shape = CX.VARIANTS_SHAPE
    case = _case(shape, dev)
    for clamp in (False, True):
        kw, kw_ref = _epilogue_pair(shape, (scale, noise, next_scale, clamp), dev)
        want = CX.to_half(CX.epilogue_ref(case.acc, **kw_ref, what=f'{shape} {scale, noise, next_scale, clamp}'))
        for round_noise in (False, True):
            _same(_plain(case, round_noise=round_noise, **kw), want)


def test_plain_launch_above_the_workgroup_slots_is_exact_everywhere(dev):
    """189 tiles (not a multiple of 8: the grid carries idle padded workgroups) x 3 channel groups = 567 workgroups on 512 slots: co-resident
    workgroups and a second round of slots, every pixel of every tile row checked -- with the full epilogue and with the identity one."""
    shape = CX.SLOTS_SHAPE
    n, cin, cout, h, w = shape
    tiles = n * (h // 8) * (w // 32)
    assert tiles % 8 != 0 and tiles * (cout // 128) > 512
    case = _case(shape, dev)
    kw, kw_ref = _epilogue_pair(shape, (True, True, True, True), dev)
    _same(_plain(case, round_noise=True, **kw), CX.to_half(CX.epilogue_ref(case.acc, **kw_ref, what=str(shape))))
    CX.assert_bare_accumulator_fits_half(case.acc, str(shape))
    _same(_plain(case, alpha=1.0, gain=1.0), CX.to_half(case.acc))


@pytest.mark.parametrize('shape', CX.OUT32_SHAPES, ids=str)
def test_out32_kernel_on_integer_operands_in_all_three_slots(dev, shape):
    """The OUT32 instantiation as what it is -- the same kernel with float32 stores: integer fp16 tensors straight in as x3 (C3 = 24, 72,
    192 channels, every one non-zero) against pack_conv3x3_weights of an integer weight.  Nothing is rounded on the way out, so every bit
    of the accumulator is visible; identity epilogue, and scale + noise + float32 bias + clamp + next_scale."""
    import gnerf_hip
    case = _case(shape, dev)
    x3, w3 = _half_nhwc(case.x), gnerf_hip.pack_conv3x3_weights(case.weight)
    _same(gnerf_hip.conv3x3_f32x3_epilogue(x3, w3, alpha=1.0), case.acc.float())
    kw, kw_ref = _epilogue_pair(shape, (True, True, True, True), dev)
    _same(gnerf_hip.conv3x3_f32x3_epilogue(x3, w3, **kw), CX.epilogue_ref(case.acc, **kw_ref, what=str(shape)).float())


def test_out32_through_the_split_route(dev):
    """The real route: split_f16x3 of integer-valued float32 activations, pack_conv3x3_weights_f32x3 of integer weights.  The lo halves are
    exactly zero and the result is the same integers."""
    import gnerf_hip
    shape = CX.OUT32_ROUTE_SHAPE
    cin = shape[1]
    case = _case(shape, dev)
    flag = gnerf_hip.split_overflow_flag(dev)
    flag.zero_()
    x32 = case.x.float().contiguous(memory_format=torch.channels_last)
    assert gnerf_hip.conv3x3_f32x3_supported(x32, shape[2])
    x3 = gnerf_hip.split_f16x3(x32)
    assert torch.equal(x3[:, :cin], x32.half()) and torch.equal(x3[:, 2 * cin:], x32.half()) and not bool(x3[:, cin:2 * cin].any())
    w3 = gnerf_hip.pack_conv3x3_weights_f32x3(case.weight.float())
    _same(gnerf_hip.conv3x3_f32x3_epilogue(x3, w3, alpha=1.0), case.acc.float())
    kw, kw_ref = _epilogue_pair(shape, (True, True, True, True), dev)
    _same(gnerf_hip.conv3x3_f32x3_epilogue(x3, w3, **kw), CX.epilogue_ref(case.acc, **kw_ref, what=str(shape)).float())
    assert int(flag.item()) == 0


def _transposed_both_forms(case):
    """(fp16 result, OUT32 result) of the transposed convolution on the case's integer operands."""
    import gnerf_hip
    x = _half_nhwc(case.x)
    wp = gnerf_hip.pack_conv_transpose3x3_weights(case.weight)
    assert gnerf_hip.conv_transpose3x3_s2_supported(x, case.weight.shape[0])
    return gnerf_hip.conv_transpose3x3_s2(x, wp), gnerf_hip.conv_transpose3x3_s2_f32x3(x, wp)


@pytest.mark.parametrize('shape', CX.TRANSPOSED, ids=str)
def test_transposed_every_job_shape_equals_the_scatter_definition(dev, monkeypatch, shape):
    """A single position; 9 x 33 positions over 8 x 32 inputs (the tile grid overhangs and the odd phases lack the last tiles); an even
    phase of exactly one tile with three chunks.  Whole position tiles, single phases, phase pairs and the launcher's own choice, fp16 and
    OUT32: all equal out[2m + ky, 2n + kx] += x[m, n] . w[:, :, ky, kx]."""
    case = _case(shape, dev, transposed=True)
    CX.assert_bare_accumulator_fits_half(case.acc, str(shape))
    want16, want32 = CX.to_half(case.acc), case.acc.float()
    for mode in (None, '0', '1', '2'):
        if mode is None:
            monkeypatch.delenv('GNERF_CONVT_PHASE_JOBS', raising=False)
        else:
            monkeypatch.setenv('GNERF_CONVT_PHASE_JOBS', mode)
        got16, got32 = _transposed_both_forms(case)
        _same(got16, want16, transposed=True)
        _same(got32, want32, transposed=True)


def test_transposed_launch_above_the_workgroup_slots_is_exact_everywhere(dev, monkeypatch):
    """The launch above 512 slots of test_conv_transpose_job_shapes_agree, in the launcher's own job shape, every output checked."""
    shape = CX.TRANSPOSED_SLOTS
    n, cin, cout, h, w = shape
    assert n * ((h + 8) // 8) * ((w + 32) // 32) * (cout // 128) > 512
    monkeypatch.delenv('GNERF_CONVT_PHASE_JOBS', raising=False)
    case = _case(shape, dev, transposed=True)
    CX.assert_bare_accumulator_fits_half(case.acc, str(shape))
    got16, got32 = _transposed_both_forms(case)
    _same(got16, CX.to_half(case.acc), transposed=True)
    _same(got32, case.acc.float(), transposed=True)


@pytest.mark.parametrize('shape', CX.TORGB_SHAPES, ids=str)
def test_torgb_tail_adds_the_exact_image(dev, shape):
    """The layer's result rounded to fp16, its exact 128-term dot product with torgb_weights rounded to fp16, + bias, clamp, rounded again,
    added to an integer-valued float32 image: with and without noise, ToRGB bias and the two clamps."""
    import gnerf_hip
    n, cin, cout, h, w = shape
    case = _case(shape, dev)
    x, wpk = _half_nhwc(case.x), gnerf_hip.pack_conv3x3_weights(case.weight)
    assert gnerf_hip.conv3x3_epilogue_torgb_supported(x, cout)
    rgb = CX.tensors_to(CX.torgb_operands(n, h, w), dev)
    rgb_w = gnerf_hip.torgb_weights(rgb['rgb_weight'].float(), rgb['rgb_styles'].float())
    assert torch.equal(rgb_w.double(), rgb['rgb_weight'].reshape(1, 3, 128) * rgb['rgb_styles'][:, None, :])
    for with_noise, with_rgb_bias, clamps in itertools.product((False, True), repeat=3):
        kw, kw_ref = _epilogue_pair(shape, (True, with_noise, False, clamps), dev)
        del kw['next_scale']
        rgb_bias, rgb_clamp = rgb['rgb_bias'] if with_rgb_bias else None, CX.RGB_CLAMP if clamps else None
        what = f'{shape} {with_noise, with_rgb_bias, clamps}'
        want = CX.torgb_ref(CX.epilogue_ref(case.acc, **kw_ref, what=what), rgb_w, rgb_bias, rgb_clamp, rgb['img'], what=what).float()
        got = gnerf_hip.conv3x3_epilogue_torgb(x, wpk, rgb['img'].float(), rgb_w, None if rgb_bias is None else rgb_bias.float(), rgb_clamp, round_noise=True, **kw)
        assert torch.equal(got, want), what + '\n' + CX.mismatch_report(got, want)


def test_split_f16x3_beyond_its_first_grid_stride(dev):
    """gnerf_split_f16x3_nhwc with three lanes per pixel on a capped grid: 786 432 lane items against 524 288 lanes, which three does not
    divide -- the stride is rounded down to whole pixels, the lanes beyond it leave, and every lane takes a second trip.  hi, lo and hi
    exactly as .half() arithmetic gives them, with and without a power-of-two scale, nothing reported as out of range."""
    import gnerf_hip
    n, c, h, w = CX.SPLIT_SHAPE
    assert (h * w * (c // 8)) > 2048 * 256 and (2048 * 256) % (c // 8) != 0
    gen = torch.Generator().manual_seed(24)
    x = (torch.randn(n, c, h, w, generator=gen) * 1.5).to(dev).contiguous(memory_format=torch.channels_last)
    st = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0, 8.0])[torch.randint(0, 6, (n, c), generator=gen)].to(dev)
    flag = gnerf_hip.split_overflow_flag(dev)
    flag.zero_()
    for scale in (None, st):
        x3 = gnerf_hip.split_f16x3(x, scale)
        assert x3.shape == (n, 3 * c, h, w) and x3.dtype == torch.float16 and gnerf_hip.is_channels_last(x3)
        xs = x if scale is None else x * scale[:, :, None, None]
        hi = x3[:, :c].float()
        assert torch.equal(hi, xs.half().float()) and torch.equal(x3[:, 2 * c:], x3[:, :c]) and torch.equal(x3[:, c:2 * c].float(), (xs - hi).half().float())
    assert int(flag.item()) == 0
