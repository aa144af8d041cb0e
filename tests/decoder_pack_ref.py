"""What gnerf_render_pack_decoder writes at the head of a decoder pack, restated in numpy float32 in the kernel's summation order
(csrc/decoder_choice.inl: decoder_stats).  Shared by tests/test_render_decoder_pack_cpu.py and tests/test_render_decoder_pack_gpu.py."""

import numpy as np

LOG2E = np.float32(1.44269504088896341)
STAT_NAMES = ('l1', 'sq1', 'mx1', 'sq2', 'mx2', 'mb1', 'mb2')         # words 0..6 of the pack; word 7 is the `bad` flag (an int)
STAT_WORDS = 16                                                        # floats in front of the two LDS images
IMAGE_FLOATS_F16 = (2 * 4 * 64 * 8 + 2 * 2048) // 2 + 64 + 128 + 64 + 36     # W1 hi+lo, W2 hi+lo as halves; density row; colour biases x4; b1; b2
IMAGE_FLOATS_F32 = 64 * 36 + 33 * 68 + 64 + 36                         # padded fp32 rows; b1; b2
PACK_BYTES = 4 * (STAT_WORDS + IMAGE_FLOATS_F16 + IMAGE_FLOATS_F32)


def _fma32(a, b, c):
    """fmaf on float32 arrays, correctly rounded.  The product of two float32 is exact in float64; the sum s = fl64(p + c) has an exact
    error term e (TwoSum).  Rounding s to float32 gives fmaf's result unless s sits exactly half way between two float32 neighbours: then
    the true value p + c = s + e lies on e's side of that midpoint (rounding to float64 cannot carry a value across a number float64
    represents, and it represents every such midpoint)."""
    with np.errstate(invalid='ignore', over='ignore'):
        p, c64 = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)
        r = s.astype(np.float32)
        d = s - r.astype(np.float64)                                   # exact
        other = np.nextafter(r, np.where(d > 0, np.inf, -np.inf).astype(np.float32))
        tie = (d != 0) & (2 * np.abs(d) == np.abs(other.astype(np.float64) - r.astype(np.float64)))
        return np.where(tie & (e != 0) & (np.sign(e) == np.sign(d)), other, r).astype(np.float32)


def row_statistics(w, scale):
    """Per row of w, one lane each, columns in order, every operation one float32 rounding as the kernel pins them (w1_row_stats /
    w2_row_stats, csrc/decoder_choice.inl): |w| s a multiply of its own, its sum plain adds, the sum of squares fused multiply-adds, the maximum."""
    w = np.abs(np.asarray(w, np.float32)) * np.float32(scale)
    l1, sq, mx = (np.zeros(w.shape[0], np.float32) for _ in range(3))
    for c in range(w.shape[1]):
        l1 = l1 + w[:, c]
        sq = _fma32(w[:, c], w[:, c], sq)
        mx = np.fmax(mx, w[:, c])                                       # fmaxf drops NaNs
    return l1, sq, mx


def statistics(w1, b1, w2, b2):
    """The seven float statistics and the flag, as float32 / bool.  Maxima over rows do not depend on an order."""
    l1, sq1, mx1 = row_statistics(w1, LOG2E)
    _, sq2, mx2 = row_statistics(w2, 1.0)
    mb1 = np.abs(np.asarray(b1, np.float32)) * LOG2E
    mb2 = np.abs(np.asarray(b2, np.float32)) * LOG2E
    with np.errstate(invalid='ignore'):
        bad = bool((~(l1 < np.inf)).any() or (~(sq2 < np.inf)).any() or (~(mb1 < np.inf)).any() or (~(mb2 < np.inf)).any())
    fmax = lambda v: np.float32(np.fmax.reduce(v))                 # fmaxf drops NaNs
    return dict(l1=fmax(l1), sq1=fmax(sq1), mx1=fmax(mx1), sq2=fmax(sq2), mx2=fmax(mx2), mb1=fmax(mb1), mb2=fmax(mb2)), bad


RANGE_LIMIT, ERR_LIMIT, SOFTPLUS_DIRECT_LIMIT = 30000.0, 2.0 ** -12, 100.0


def decision(w1, b1, w2, b2, absmax):
    """choose_mlp's inequalities (csrc/decoder_choice.inl) in float64 on the restated statistics: (arithmetic 'f16x3' | 'f32', short softplus,
    e_o, h_hard).  A test that expects a choice keeps e_o and h_hard a few per cent away from their limits: the kernel evaluates the
    same expressions in float32."""
    s, bad = statistics(w1, b1, w2, b2)
    s = {k: float(v) for k, v in s.items()}
    A = float(absmax)
    R1, R2 = s['sq1'] ** 0.5, s['sq2'] ** 0.5
    h_hard = s['l1'] * A + s['mb1'] + 1.0
    e_p = 2.0 ** -22 * R1 * A + 2.0 ** -25 * (R1 + 5.657 * A)
    h = R1 * A + s['mb1'] + 1.0
    e_o = R2 * e_p + 2.0 ** -22 * R2 * h + 2.0 ** -25 * (R2 + 8.0 * h)
    ok = (not bad) and A <= RANGE_LIMIT and s['mx1'] <= RANGE_LIMIT and s['mx2'] <= RANGE_LIMIT and h_hard <= RANGE_LIMIT and s['mb2'] <= RANGE_LIMIT and e_o <= ERR_LIMIT
    return ('f16x3' if ok else 'f32'), bool(ok and h_hard <= SOFTPLUS_DIRECT_LIMIT), e_o, h_hard
