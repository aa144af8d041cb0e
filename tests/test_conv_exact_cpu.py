"""Conditions on the operands and references of tests/test_conv_exact_gpu.py (tests/conv_exact_ref.py), so that its bit-for-bit comparisons
are the right demand and cannot pass vacuously: the two references are torch's convolutions, the operands hold no zeros, every named case
meets the exactness conditions (they are asserted inside the helper whenever a reference is built; here they run without a GPU), the
references do not depend on the order of the epilogue's operations, and the mismatch report points at the right place.  No GPU."""

import itertools

import pytest
import torch
import torch.nn.functional as F

import conv_exact_ref as CX


@pytest.mark.parametrize('shape', [(2, 5, 7, 4, 6), (1, 16, 3, 8, 32), (3, 1, 2, 1, 1), (1, 3, 4, 1, 9)])
def test_references_are_the_framework_convolutions(shape):
    """Exactly on integers, to a float64 rounding of the largest value on Gaussian operands (the sums are taken in another order)."""
    n, cin, cout, h, w = shape
    x, wt = CX.integer_operands(n, cin, cout, h, w)
    assert torch.equal(CX.conv3x3_ref(x, wt), F.conv2d(x, wt, padding=1))
    assert torch.equal(CX.conv_transpose3x3_s2_ref(x, wt), F.conv_transpose2d(x, wt.transpose(0, 1), stride=2))
    gen = torch.Generator().manual_seed(3)
    x, wt = torch.randn(n, cin, h, w, generator=gen, dtype=torch.float64), torch.randn(cout, cin, 3, 3, generator=gen, dtype=torch.float64)
    for got, want in ((CX.conv3x3_ref(x, wt), F.conv2d(x, wt, padding=1)), (CX.conv_transpose3x3_s2_ref(x, wt), F.conv_transpose2d(x, wt.transpose(0, 1), stride=2))):
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))


def test_operand_makers_produce_no_zeros_and_only_dyadic_numbers():
    x, wt = CX.integer_operands(2, 24, 128, 8, 32)
    for t in (x, wt):
        assert sorted(t.unique().tolist()) == sorted(CX.VALUES)                     # every value of the alphabet, nothing else
    CX.assert_operands(x, wt)
    with pytest.raises(AssertionError):
        CX.assert_operands(x * (x != 3.0), wt)                                      # a zero among the activations is refused
    ops = CX.epilogue_operands(3, 256, 16, 64)
    assert set(ops['scale'].unique().tolist()) == set(CX.DYADIC) == set(ops['next_scale'].unique().tolist())
    assert torch.equal(ops['bias'] * 2, (ops['bias'] * 2).round()) and float(ops['bias'].abs().max()) <= 8 and ops['bias'].half().double().equal(ops['bias'])
    assert torch.equal(ops['noise'], ops['noise'].round()) and float(ops['noise'].abs().max()) == 4
    rgb = CX.torgb_operands(2, 16, 64)
    w16 = (rgb['rgb_weight'].reshape(1, 3, 128) * rgb['rgb_styles'][:, None, :])
    assert torch.equal(w16.float().half().double(), w16) and float(w16.abs().min()) > 0          # torgb_weights rounds nothing away
    assert torch.equal(rgb['rgb_bias'].half().double(), rgb['rgb_bias']) and torch.equal(rgb['img'], rgb['img'].round())
    # seeded by the shape: the same operands on every call, other operands for another shape
    assert torch.equal(CX.integer_operands(2, 24, 128, 8, 32)[0], x) and not torch.equal(CX.integer_operands(2, 24, 128, 8, 32, salt=1)[0], x)


def test_conditions_refuse_what_would_not_be_exact():
    with pytest.raises(AssertionError):
        CX.assert_float32_exact(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), 'probe')
    with pytest.raises(AssertionError):
        CX.assert_bare_accumulator_fits_half(torch.tensor([2049.0], dtype=torch.float64), 'probe')
    with pytest.raises(AssertionError):
        CX.assert_clamp_bites(torch.arange(100, dtype=torch.float64), 1000.0, 'probe')
    with pytest.raises(AssertionError):                                             # 2^12 products of 2^12 + 2^-1: 25 bits
        CX.any_order_exact_in_float32(torch.full((4096,), 4096.5, dtype=torch.float64), torch.ones(4096, dtype=torch.float64), 0, 'probe')
    CX.any_order_exact_in_float32(torch.full((4096,), 2047.5, dtype=torch.float64), torch.ones(4096, dtype=torch.float64), 0, 'probe')


@pytest.mark.parametrize('shape', CX.PLAIN_IDENTITY + [CX.VARIANTS_SHAPE, CX.SLOTS_SHAPE], ids=str)
def test_plain_cases_meet_the_conditions(shape):
    """Identity epilogue: the bare accumulator is stored as fp16, so max |acc| <= 2048; the sixteen variants and the full epilogue: every
    intermediate a float32 number, the clamp reached by a real share (asserted inside epilogue_ref)."""
    case = CX.conv_case(shape)
    print(shape, 'max |acc|', case.max_acc)
    CX.assert_bare_accumulator_fits_half(case.acc, str(shape))
    variants = CX.epilogue_variants() if shape == CX.VARIANTS_SHAPE else [(True, True, True, True)] if shape == CX.SLOTS_SHAPE else []
    for v in variants:
        ref = CX.epilogue_ref(case.acc, **CX.epilogue_kwargs(shape, *v), what=f'{shape} {v}')
        assert bool(torch.isfinite(CX.to_half(ref)).all()) and bool((ref != case.acc).any())


@pytest.mark.parametrize('shape', CX.OUT32_SHAPES + [CX.OUT32_ROUTE_SHAPE], ids=str)
def test_out32_cases_meet_the_conditions(shape):
    case = CX.conv_case(shape)
    print(shape, 'max |acc|', case.max_acc)
    CX.epilogue_ref(case.acc, **CX.epilogue_kwargs(shape, True, True, True, True), what=str(shape))


@pytest.mark.parametrize('shape', CX.TRANSPOSED + [CX.TRANSPOSED_SLOTS], ids=str)
def test_transposed_cases_meet_the_conditions(shape):
    case = CX.conv_case(shape, transposed=True)
    print(shape, 'max |acc|', case.max_acc)
    n, cin, cout, h, w = shape
    assert case.acc.shape == (n, cout, 2 * h + 1, 2 * w + 1)
    CX.assert_bare_accumulator_fits_half(case.acc, str(shape))
    # the odd-odd phase has ONE tap: it is the 1 x 1 convolution with the centre weights
    assert torch.equal(case.acc[:, :, 1::2, 1::2], torch.einsum('nchw,oc->nohw', case.x, case.weight[:, :, 1, 1]))


@pytest.mark.parametrize('shape', CX.TORGB_SHAPES, ids=str)
def test_torgb_cases_meet_the_conditions_and_do_not_depend_on_the_operation_order(shape):
    """Every combination of noise / ToRGB bias / clamps: the reference's own conditions hold (asserted inside torgb_ref), and a float32
    emulation of the kernel's order -- gain folded into the operands, channel pairs summed one after the other in two halves -- gives
    the same bits."""
    n, cin, cout, h, w = shape
    case = CX.conv_case(shape)
    rgb = CX.torgb_operands(n, h, w)
    rgb_w = (rgb['rgb_weight'].reshape(1, 3, 128) * rgb['rgb_styles'][:, None, :]).float().half()
    for with_noise, with_rgb_bias, clamps in itertools.product((False, True), repeat=3):
        kw = CX.epilogue_kwargs(shape, True, with_noise, False, clamps)
        layer = CX.epilogue_ref(case.acc, **kw, what=f'{shape} layer')
        rgb_bias, rgb_clamp = rgb['rgb_bias'] if with_rgb_bias else None, CX.RGB_CLAMP if clamps else None
        want = CX.torgb_ref(layer, rgb_w, rgb_bias, rgb_clamp, rgb['img'], what=f'{shape} {with_noise, with_rgb_bias, clamps}')
        layer16 = CX.epilogue_kernel_order_f32(case.acc, **kw).half()
        assert torch.equal(layer16, CX.to_half(layer))
        got = CX.torgb_kernel_order_f32(layer16, rgb_w, None if rgb_bias is None else rgb_bias.float(), rgb_clamp, rgb['img'].float())
        assert torch.equal(got, want.float())
        assert float((want - rgb['img']).abs().max()) <= (rgb_clamp or 65504.0) and bool((want != rgb['img']).any())


def test_epilogue_reference_does_not_depend_on_the_operation_order():
    """All sixteen variants: the float64 chain, rounded once, against float32 arithmetic in the kernel's order (gain folded into scale, bias
    and noise; fused multiply-add; max(u, alpha u) for the lrelu).  Exact operands: the order cannot matter, for the fp16 and the fp32 result."""
    shape = CX.VARIANTS_SHAPE
    case = CX.conv_case(shape)
    for v in CX.epilogue_variants():
        kw = CX.epilogue_kwargs(shape, *v)
        ref = CX.epilogue_ref(case.acc, **kw)
        emu = CX.epilogue_kernel_order_f32(case.acc, **kw)
        assert torch.equal(emu, ref.float()) and torch.equal(emu.half(), CX.to_half(ref)), v
    ident = CX.epilogue_ref(case.acc)
    assert torch.equal(ident, case.acc) and torch.equal(CX.epilogue_kernel_order_f32(case.acc).double(), case.acc)


def test_a_single_pixel_image_counts_as_channels_last_memory():
    """The transposed form's smallest case, 1 x 1 inputs: dense memory [N, C] is NHWC and NCHW at once.  is_channels_last tells layouts
    apart and says NCHW; the convolution wrappers ask about the MEMORY and take it (they refused it before this suite ran the case)."""
    from gnerf_hip import conv3x3 as C
    one = torch.zeros(2, 8, 1, 1, dtype=torch.float16).contiguous(memory_format=torch.channels_last)
    assert not C.is_channels_last(one) and C._nhwc_memory(one)
    assert C._nhwc_memory(torch.zeros(2, 8, 4, 4).contiguous(memory_format=torch.channels_last))
    assert not C._nhwc_memory(torch.zeros(2, 8, 4, 4)) and not C._nhwc_memory(torch.zeros(2, 8, 2, 1)) and not C._nhwc_memory(torch.zeros(2, 16, 1, 1)[:, ::2])


def test_mismatch_report_decodes_a_planted_error():
    want = torch.zeros(3, 256, 16, 64, dtype=torch.float16)
    got = want.clone()
    assert CX.mismatch_report(got, want) == ''
    got[2, 150, 13, 37] = 4.0                                   # image 2, second group, channel 22 of it; tile row 5 of tile row 1, column 5 of tile column 1
    got[0, 3, 0, 0] = -1.0
    text = CX.mismatch_report(got, want)
    assert text.startswith('2 of ') and '4 x1' in text and '-1 x1' in text
    at = CX.locate((2, 150, 13, 37), want.shape)
    assert at == dict(image=2, channel=150, y=13, x=37, tile_y=5, tile_x=5, tile=2 * 4 + 1 * 2 + 1, block_x=(11 % 2) * 8 + 11 // 2, wave_rows=2,
                      block16=1, group128=1, phase=None)
    assert 'image=2, channel=150, y=13, x=37, tile_y=5, tile_x=5, tile=11' in text and 'group128=1' in text and 'got 4, want 0' in text
    assert 'wrong by tile row (y mod 8): [1, 0, 0, 0, 0, 1, 0, 0]' in text
    # transposed form: output (2m + py, 2n + px) belongs to position (m, n) of phase (py, px); the tiles lie over the (h + 1) x (w + 1) positions
    want_t = torch.zeros(2, 128, 2 * 9 + 1, 2 * 40 + 1)
    got_t = want_t.clone()
    got_t[1, 100, 17, 70] = 1.0                                 # phase (1, 0), position (8, 35): the second tile row and column, first row of its tile
    at = CX.locate((1, 100, 17, 70), want_t.shape, transposed=True)
    assert (at['phase'], at['tile_y'], at['tile_x'], at['tile'], at['block16'], at['group128']) == ((1, 0), 0, 3, (1 * 2 + 1) * 2 + 1, 6, 0)
    text = CX.mismatch_report(got_t, want_t, transposed=True)
    assert 'phase=(1, 0)' in text and 'wrong by phase (2 py + px): [0, 0, 1, 0]' in text
    # a NaN is a mismatch, not an equal
    got_t[0, 0, 0, 0] = float('nan')
    assert CX.mismatch_report(got_t, want_t, transposed=True).startswith('2 of ')
