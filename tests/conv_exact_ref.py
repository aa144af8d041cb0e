"""Integer operands and exact references for the matrix-core convolutions (csrc/conv3x3.hip), shared by tests/test_conv_exact_cpu.py and
tests/test_conv_exact_gpu.py.  No test functions, nothing here needs a GPU.

Why integers.  Activations and weights are drawn from {+-1, +-2, +-3}: every product is a non-zero integer of magnitude <= 9, and the sum of
the magnitudes of the 9 cin products of an output is at most 81 cin <= 41 472 < 2^24.  Every partial sum, taken in ANY order and grouping,
is therefore an integer that float32 holds exactly: whatever the kernel's chunking, tap order, k-step split or matrix-instruction
accumulation order, its accumulator must EQUAL the integer reference.  A dropped, doubled or mispaired product changes the sum by at
least 1 (there are no zero operands), so nothing hides below a tolerance.  The epilogue's operands are dyadic (scale and next_scale from
{1/4, 1/2, 1, 2}, bias a multiple of 1/2, integer noise, gain 2, slope 1/4, integer clamp), so every intermediate of the chain is exact in
float32 in whatever order it is evaluated (the kernel folds the gain into the operands, the reference does not), and the only rounding
left is the output's: one rounding to float16 for the fp16 forms, none for the fp32-grade form.

The references share no code with torch's convolutions: the plain one is nine shifted matmuls over the zero-padded input, the transposed
one the scatter definition out[2m + ky, 2n + kx] += x[m, n] . w[:, :, ky, kx]; both in float64 on whatever device the operands live on
(integers below 2^53 are exact in a float64 matmul of any blocking).  The CONDITIONS under which "bit for bit" is the right demand are
asserted here, on the reference, every time one is built -- not on the kernel, and no output is exempt from the comparison:
  * 81 cin < 2^24 (sum of |products|);
  * every epilogue intermediate and every reference value is a float32 (ref.float().double() == ref), which also makes the
    double -> float -> half conversion a single rounding;
  * where a bare accumulator is stored as float16 (transposed form, identity epilogue), max |acc| <= 2048, so the store rounds nothing;
  * a clamp is reached by a real share of the outputs (and missed by a real share)."""

import collections
import functools

import torch

VALUES = (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0)          # operand alphabet: no zeros
DYADIC = (0.25, 0.5, 1.0, 2.0)                      # scale / next_scale alphabet
GAIN, ALPHA = 2.0, 0.25
TILE_H, TILE_W, GROUP, BLOCK = 8, 32, 128, 16       # the kernel's pixel tile, output-channel group per workgroup, channel block per MFMA

# ---- the named cases of tests/test_conv_exact_gpu.py: (images, input channels, output channels, height, width) ------------------------
PLAIN_IDENTITY = [(1, 8, 128, 8, 32), (1, 64, 128, 8, 32), (1, 72, 128, 8, 32), (2, 192, 256, 16, 64), (1, 512, 128, 8, 32)]
VARIANTS_SHAPE = (2, 128, 256, 16, 64)
SLOTS_SHAPE = (3, 64, 384, 72, 224)                 # 189 tiles x 3 channel groups = 567 workgroups > 512 slots
OUT32_SHAPES = [(2, 24, 128, 8, 64), (1, 72, 256, 16, 32), (2, 192, 128, 16, 64)]      # the second entry is C3, the kernel's input channels
OUT32_ROUTE_SHAPE = (1, 24, 128, 8, 32)             # float32 activations through split_f16x3: C = 24, C3 = 72
TRANSPOSED = [(1, 8, 128, 1, 1), (1, 64, 128, 8, 32), (2, 136, 256, 7, 31)]
TRANSPOSED_SLOTS = (10, 136, 256, 70, 65)           # 10 x 9 x 3 position tiles x 2 channel groups = 540 workgroups > 512 slots
TORGB_SHAPES = [(2, 64, 128, 16, 64), (1, 136, 128, 8, 96)]
CLAMP = {8: 32.0, 24: 64.0, 64: 128.0, 72: 128.0, 128: 256.0, 136: 256.0, 192: 256.0, 512: 512.0}     # by input channels: about one sigma of the result
RGB_CLAMP = 128.0
SPLIT_SHAPE = (1, 24, 512, 512)                     # 786 432 lane items against the 524 288 lanes of a capped grid, three lanes per pixel


def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _draw(alphabet, shape, gen):
    table = torch.tensor(alphabet, dtype=torch.float64)
    return table[torch.randint(0, len(alphabet), tuple(shape), generator=gen)]


def integer_operands(n, cin, cout, h, w, salt=0):
    """(x [n, cin, h, w], weight [cout, cin, 3, 3]) float64 on the CPU, values from {+-1, +-2, +-3}, seeded by the shape."""
    gen = _gen(n, cin, cout, h, w, salt)
    return _draw(VALUES, (n, cin, h, w), gen), _draw(VALUES, (cout, cin, 3, 3), gen)


def epilogue_operands(n, cout, h, w, salt=0):
    """dict(scale [n, cout], next_scale [n, cout], bias [cout], noise [h, w]) float64 on the CPU: scale / next_scale from {1/4, 1/2, 1, 2},
    bias a multiple of 1/2 with |b| <= 8, noise an integer with |nz| <= 4."""
    gen = _gen(n, cout, h, w, salt, 99)
    return dict(scale=_draw(DYADIC, (n, cout), gen), next_scale=_draw(DYADIC, (n, cout), gen),
                bias=torch.randint(-16, 17, (cout,), generator=gen).double() / 2, noise=torch.randint(-4, 5, (h, w), generator=gen).double())


def torgb_operands(n, h, w, salt=0):
    """dict(rgb_weight [3, 128, 1, 1] from {+-1, +-2, +-3}, rgb_styles [n, 128] from {1/32, 1/16, 1/8}, rgb_bias [3] multiples of 1/8,
    img [n, 3, h, w] integers with |v| <= 100) float64 on the CPU: the products weight x styles are float16 numbers."""
    gen = _gen(n, h, w, salt, 7)
    return dict(rgb_weight=_draw(VALUES, (3, 128, 1, 1), gen), rgb_styles=_draw((1 / 32, 1 / 16, 1 / 8), (n, 128), gen),
                rgb_bias=torch.randint(-32, 33, (3,), generator=gen).double() / 8, img=torch.randint(-100, 101, (n, 3, h, w), generator=gen).double())


# ---- conditions ---------------------------------------------------------------------------------------------------------------------------
def assert_float32_exact(t, what):
    """Every value of the float64 tensor t is a float32 number."""
    assert t.dtype == torch.float64
    bad = t.float().double() != t
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {t.numel()} values are not float32 numbers; the comparison would not be exact'
    return t


def assert_operands(x, weight):
    """Integers from the alphabet, none zero, and few enough that the sum of |products| of an output stays below 2^24."""
    for name, t in (('x', x), ('weight', weight)):
        assert bool((t == t.round()).all()) and float(t.abs().min()) >= 1.0 and float(t.abs().max()) <= 3.0, f'{name}: values must come from +-1, +-2, +-3'
    assert 81 * x.shape[1] < 2 ** 24


def assert_bare_accumulator_fits_half(acc, what):
    top = float(acc.abs().max())
    assert top <= 2048.0, f'{what}: max |acc| = {top} > 2048, a float16 store would round'
    return top


def assert_clamp_bites(pre, clamp, what, low=0.02, high=0.9):
    """A real share of the values reaches the clamp and a real share stays inside it."""
    share = float((pre.abs() >= clamp).double().mean())
    assert low <= share <= high, f'{what}: {share:.3f} of the outputs reach the clamp {clamp}'
    return share


# ---- references ---------------------------------------------------------------------------------------------------------------------------
def conv3x3_ref(x, weight):
    """conv2d(x, weight, padding=1) as nine shifted matmuls over the zero-padded input, float64; x [n, cin, h, w], weight [cout, cin, 3, 3]."""
    assert x.dtype == torch.float64 and weight.dtype == torch.float64
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    xp = torch.zeros(n, h + 2, w + 2, cin, dtype=torch.float64, device=x.device)
    xp[:, 1:h + 1, 1:w + 1] = x.permute(0, 2, 3, 1)
    out = torch.zeros(n * h * w, cout, dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + h, kx:kx + w].reshape(n * h * w, cin) @ weight[:, :, ky, kx].t()
    return out.reshape(n, h, w, cout).permute(0, 3, 1, 2)


def conv_transpose3x3_s2_ref(x, weight):
    """conv_transpose2d(x, weight.transpose(0, 1), stride=2) by its scatter definition, float64: out[:, :, 2m + ky, 2n + kx] +=
    x[:, :, m, n] . weight[:, :, ky, kx]; x [n, cin, h, w], weight [cout, cin, 3, 3] -> [n, cout, 2h + 1, 2w + 1]."""
    assert x.dtype == torch.float64 and weight.dtype == torch.float64
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    xf = x.permute(0, 2, 3, 1).reshape(n * h * w, cin)
    out = torch.zeros(n, 2 * h + 1, 2 * w + 1, cout, dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            out[:, ky:ky + 2 * h - 1:2, kx:kx + 2 * w - 1:2] += (xf @ weight[:, :, ky, kx].t()).reshape(n, h, w, cout)
    return out.permute(0, 3, 1, 2)


def epilogue_ref(acc, bias=None, scale=None, noise=None, alpha=1.0, gain=1.0, clamp=None, next_scale=None, what='epilogue'):
    """clamp(lrelu(acc * scale + noise + bias) * gain) * next_scale in float64, every intermediate asserted to be a float32 number."""
    t = acc
    if scale is not None:
        t = assert_float32_exact(t * scale[:, :, None, None], what + ': acc * scale')
    if noise is not None:
        t = assert_float32_exact(t + noise, what + ': + noise')
    if bias is not None:
        t = assert_float32_exact(t + bias[None, :, None, None], what + ': + bias')
    t = assert_float32_exact(torch.where(t < 0, t * alpha, t), what + ': lrelu')
    t = assert_float32_exact(t * gain, what + ': * gain')
    if clamp is not None:
        assert_clamp_bites(t, clamp, what)
        t = t.clamp(-clamp, clamp)
    if next_scale is not None:
        t = t * next_scale[:, :, None, None]
    return assert_float32_exact(t, what + ': result')


def to_half(ref):
    """The ONE rounding of the fp16 forms: ref is a float32 number, so double -> float is exact and float -> half rounds once."""
    return assert_float32_exact(ref, 'to_half').float().half()


def any_order_exact_in_float32(a, b, dim, what):
    """Assert that sum over `dim` of a * b is exact in float32 in any order: all products are multiples of one power of two q, and the
    sum of their magnitudes is below 2^24 q."""
    p = (a * b).abs()
    k = 0
    while k < 60 and not bool((p * 2.0 ** k == (p * 2.0 ** k).round()).all()):
        k += 1
    top = float(p.sum(dim).max()) * 2.0 ** k
    assert k < 60 and top < 2 ** 24, f'{what}: sum of |products| is {top} units of 2^-{k}, not below 2^24'


def torgb_ref(layer, rgb_w, rgb_bias, rgb_clamp, img, what='torgb'):
    """The ToRGB tail with the roundings csrc/conv3x3.hip states: the layer's result (float64, unrounded) rounded to fp16; the exact 128-term
    dot product with rgb_w [n, 3, 128] rounded to fp16; + bias, clamp; rounded to fp16 again; added to the fp32 image.  float64 [n, 3, h, w]."""
    y16 = to_half(layer).double()
    w = rgb_w.double()
    any_order_exact_in_float32(y16[:, None], w[:, :, :, None, None], 2, what + ': dot product')
    s = assert_float32_exact(torch.einsum('nchw,nkc->nkhw', y16, w), what + ': dot product')
    assert float(s.abs().max()) < 65504.0
    rv = s.float().half().double()
    if rgb_bias is not None:
        rv = assert_float32_exact(rv + rgb_bias[None, :, None, None], what + ': + bias')
    if rgb_clamp is not None:
        assert_clamp_bites(rv, rgb_clamp, what)
        rv = rv.clamp(-rgb_clamp, rgb_clamp)
    return assert_float32_exact(img + rv.float().half().double(), what + ': image')


# ---- float32 emulations of the kernel's stated operation order (csrc/conv3x3.hip, registers_to_lds and the RGB tail), for the CPU tests ---
def epilogue_kernel_order_f32(acc, bias=None, scale=None, noise=None, alpha=1.0, gain=1.0, clamp=None, next_scale=None):
    """u = fma(acc, scale gain, bias gain) + noise gain; r = max(u, alpha u); med3(r, -c, c); * next_scale -- in float32, gain folded into
    the operands first as the kernel does."""
    g = torch.tensor(gain, dtype=torch.float32)
    a = acc.float()
    scg = (scale.float() * g)[:, :, None, None] if scale is not None else g
    bg = (bias.float() * g)[None, :, None, None] if bias is not None else torch.zeros((), dtype=torch.float32)
    u = torch.addcmul(bg.expand_as(a), a, scg.expand_as(a))
    if noise is not None:
        u = u + noise.float() * g
    r = torch.maximum(u, u * torch.tensor(alpha, dtype=torch.float32))
    if clamp is not None:
        r = r.clamp(-clamp, clamp)
    if next_scale is not None:
        r = r * next_scale.float()[:, :, None, None]
    assert r.dtype == torch.float32
    return r


def torgb_kernel_order_f32(layer16, rgb_w16, rgb_bias, rgb_clamp, img32):
    """Two lanes per pixel, 64 channels each, channel PAIRS accumulated into a float32 sum one after the other (v_dot2_f32_f16), the two
    halves added; rounded to fp16; + bias; clamp; rounded to fp16; added to the float32 image."""
    n, c, h, w = layer16.shape
    assert c == 128 and layer16.dtype == torch.float16 and rgb_w16.dtype == torch.float16 and img32.dtype == torch.float32
    y, wt = layer16.float(), rgb_w16.float()
    halves = []
    for half in range(2):
        acc = torch.zeros(n, 3, h, w, dtype=torch.float32)
        for c0 in range(64 * half, 64 * half + 64, 2):
            pair = y[:, None, c0] * wt[:, :, c0, None, None] + y[:, None, c0 + 1] * wt[:, :, c0 + 1, None, None]
            acc = acc + pair
        halves.append(acc)
    rv = (halves[0] + halves[1]).half().float()
    if rgb_bias is not None:
        rv = rv + rgb_bias.half().float()[None, :, None, None]
    if rgb_clamp is not None:
        rv = rv.clamp(-rgb_clamp, rgb_clamp)
    return img32 + rv.half().float()


# ---- cases, built once and shared ---------------------------------------------------------------------------------------------------------
ConvCase = collections.namedtuple('ConvCase', 'x weight acc max_acc')


@functools.lru_cache(maxsize=None)
def conv_case(shape, transposed=False, device='cpu'):
    """Operands and the integer accumulator of a named case, float64 on `device`, made once and never written to.  The operands are drawn
    on the CPU (the same on every device); the reference is computed where they live."""
    n, cin, cout, h, w = shape
    x, weight = integer_operands(n, cin, cout, h, w, salt=int(transposed))
    assert_operands(x, weight)
    x, weight = x.to(device), weight.to(device)
    acc = (conv_transpose3x3_s2_ref if transposed else conv3x3_ref)(x, weight)
    assert_float32_exact(acc, f'accumulator of {shape}')
    return ConvCase(x, weight, acc, float(acc.abs().max()))


def clear_cases():
    conv_case.cache_clear()


def epilogue_variants():
    """The plain form's sixteen template / clamp variants: (scale, noise, next_scale, clamp) present or not."""
    return [(sc, nz, nx, cl) for sc in (False, True) for nz in (False, True) for nx in (False, True) for cl in (False, True)]


def epilogue_kwargs(shape, scale, noise, next_scale, clamp, salt=0):
    """The float64 CPU operands of one variant of the full epilogue (bias always, gain 2, slope 1/4) as keyword arguments of epilogue_ref."""
    n, cin, cout, h, w = shape
    ops = epilogue_operands(n, cout, h, w, salt)
    return dict(bias=ops['bias'], scale=ops['scale'] if scale else None, noise=ops['noise'] if noise else None, alpha=ALPHA, gain=GAIN,
                clamp=CLAMP[cin] if clamp else None, next_scale=ops['next_scale'] if next_scale else None)


def tensors_to(kw, device, dtype=None):
    """A dict's tensors moved to `device` (and to `dtype`); everything else unchanged."""
    return {k: (v.to(device=device, dtype=dtype or v.dtype) if torch.is_tensor(v) else v) for k, v in kw.items()}


# ---- the mismatch report ------------------------------------------------------------------------------------------------------------------
def locate(index, shape, transposed=False):
    """Where output (image, channel, y, x) of a result of `shape` [n, cout, H, W] was computed: position inside the 8 x 32 tile, tile index
    (image-major, then tile rows: the kernel's `tile`), the workgroup's blockIdx.x for it (an XCD owns a contiguous eighth of the tiles),
    wave row pair, channel block of 16 within the group of 128, the group.  Transposed form: the tiles lie over the POSITIONS (y >> 1,
    x >> 1) of the output's phase (y & 1, x & 1)."""
    n, c, y, x = (int(v) for v in index)
    n_img, _, out_h, out_w = shape
    if transposed:
        phase, m, q = (y & 1, x & 1), y >> 1, x >> 1
        tiles_y, tiles_x = -(-((out_h + 1) // 2) // TILE_H), -(-((out_w + 1) // 2) // TILE_W)
    else:
        phase, m, q = None, y, x
        tiles_y, tiles_x = out_h // TILE_H, out_w // TILE_W
    tile = (n * tiles_y + m // TILE_H) * tiles_x + q // TILE_W
    per_xcd = -(-(n_img * tiles_y * tiles_x) // 8)
    return dict(image=n, channel=c, y=y, x=x, tile_y=m % TILE_H, tile_x=q % TILE_W, tile=tile, block_x=(tile % per_xcd) * 8 + tile // per_xcd,
                wave_rows=(m % TILE_H) // 2, block16=(c % GROUP) // BLOCK, group128=c // GROUP, phase=phase)


def mismatch_report(got, want, transposed=False, first=8):
    """'' when got equals want everywhere; otherwise the number of wrong outputs, a histogram of got - want, where in the tile / channel
    structure they lie, and the first few located."""
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    bad = ~(got == want)
    count = int(bad.sum())
    if count == 0:
        return ''
    idx = bad.nonzero().cpu()
    diff = (got.double() - want.double())[bad].cpu()
    values, counts = torch.unique(diff, return_counts=True)
    order = torch.argsort(counts, descending=True)[:12]
    lines = [f'{count} of {got.numel()} outputs differ ({"transposed" if transposed else "plain"} form, shape {tuple(got.shape)})',
             'got - want: ' + ', '.join(f'{float(values[i]):g} x{int(counts[i])}' for i in order)]
    m, q = (idx[:, 2] >> 1, idx[:, 3] >> 1) if transposed else (idx[:, 2], idx[:, 3])
    for name, key, size in (('tile row (y mod 8)', m % TILE_H, TILE_H), ('tile column (x mod 32)', q % TILE_W, TILE_W),
                            ('channel block of 16', idx[:, 1] % GROUP // BLOCK, GROUP // BLOCK), ('group of 128', idx[:, 1] // GROUP, got.shape[1] // GROUP),
                            ('image', idx[:, 0], got.shape[0])):
        lines.append(f'wrong by {name}: {torch.bincount(key, minlength=size).tolist()}')
    if transposed:
        lines.append(f'wrong by phase (2 py + px): {torch.bincount(2 * (idx[:, 2] & 1) + (idx[:, 3] & 1), minlength=4).tolist()}')
    for row in idx[:first]:
        at = locate(row.tolist(), got.shape, transposed)
        n, c, y, x = row.tolist()
        lines.append(', '.join(f'{k}={v}' for k, v in at.items() if v is not None) + f': got {float(got[n, c, y, x]):g}, want {float(want[n, c, y, x]):g}')
    return '\n'.join(lines)
