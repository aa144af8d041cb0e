"""Reference of the plane-gradient scatter (csrc/scatter_binned.inl, plane_scatter_kernel) and the cases its tests run; numpy only.

The operation: sample k of ray r sits at p = (o + t d) * (2 / box_warp); in plane pl it has the coordinates (u, v) = (x, y), (x, z),
(z, x) and a bilinear footprint (zero padding, align_corners = False); grad[item, pl, y, x, :] += w_tap * dX[r, k, :], w_tap with the 1/3
of the plane mean.

Cases live on a dyadic lattice (direction components in {0, +-1/2, +-1}, origins and depths multiples of 2^-6, box_warp 1 or 2), on
which o + t d, the texel coordinates and the fractions are exact in float32 whatever the compiler contracts; footprints() asserts that
against a float64 recomputation.  The four weights are then single float32 operations on exact operands ((1 - fy) * fl(1/3), its product
with 1 - fx), which numpy reproduces bit for bit, and so is every contribution rn32(w * dx).  reference() sums those contributions in
integers: S is exact."""

import numpy as np

F32 = np.float32
THIRD = F32(1.0) / F32(3.0)
TILE = 16
U_FIXED = 129           # units of 2^-s a record's conversion can be off floor-free: 128 of bin_to_fixed_model plus the floor itself


def _nbits(n):
    return int(n - 1).bit_length() if n > 1 else 0


def footprints(case):
    """Per (item, ray, sample, plane): x0, y0 (int), the four weights (float32, order x0y0 x1y0 x0y1 x1y1; zero where the tap is off
    the plane).  Asserts the lattice's exactness: every coordinate that can reach the plane equals its float64 value."""
    o, d, t = (np.asarray(case[k], dtype=F32) for k in ('origins', 'dirs', 'depths'))
    H, W = case['H'], case['W']
    scale = F32(2.0 / case['box_warp'])
    p = (o[:, :, None, :] + t[..., None] * d[:, :, None, :]) * scale                       # float32: one rounding per operation, as the kernels
    p64 = (o.astype(np.float64)[:, :, None, :] + t.astype(np.float64)[..., None] * d.astype(np.float64)[:, :, None, :]) * float(scale)
    out = []
    for uax, vax in ((0, 1), (0, 2), (2, 0)):
        geo = []
        for ax, n in ((uax, W), (vax, H)):
            i32 = ((p[..., ax] + F32(1)) * F32(n) - F32(1)) * F32(0.5)
            i64 = ((p64[..., ax] + 1.0) * n - 1.0) * 0.5
            near = (i64 > -2.0) & (i64 < n + 1.0)
            assert np.array_equal(i32[near].astype(np.float64), i64[near]), 'a coordinate is not exact in float32: the case is off the lattice'
            assert np.all((i32[~near] <= F32(-2)) | (i32[~near] >= F32(n + 1))), 'float32 and float64 disagree on what is outside'
            c = np.clip(i32, F32(-1.5), F32(n + 0.5))
            f0 = np.floor(c)
            geo.append((f0.astype(np.int64), c - f0))
        (x0, fx), (y0, fy) = geo
        one = F32(1)
        wx0 = np.where((x0 >= 0) & (x0 < W), one - fx, F32(0)); wx1 = np.where((x0 + 1 >= 0) & (x0 + 1 < W), fx, F32(0))
        wy0 = np.where((y0 >= 0) & (y0 < H), (one - fy) * THIRD, F32(0)); wy1 = np.where((y0 + 1 >= 0) & (y0 + 1 < H), fy * THIRD, F32(0))
        w = np.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1], axis=-1).astype(F32)
        out.append((x0, y0, w, fx, fy))
    x0, y0, w, fx, fy = (np.stack([pl[i] for pl in out], axis=3) for i in range(5))    # [N,M,K,3(,4)]
    return x0, y0, w, fx, fy


def _exact_sums(idx, c, size):
    """idx [n] flat texel index, c [n,32] float32 contributions (finite) -> (rn32(S) float32, S float64) of the exact sums, [size,32]."""
    m, k = np.frexp(c.astype(np.float64))
    mi = np.round(m * float(1 << 24)).astype(np.int64)
    assert np.array_equal(mi.astype(np.float64) * 2.0 ** -24, m)
    k = k.astype(np.int64) - 24
    nz = mi != 0
    if not nz.any():
        return np.zeros([size, 32], F32), np.zeros([size, 32], np.float64)
    kmin = int(k[nz].min())
    shift = np.where(nz, k - kmin, 0)
    per = np.bincount(idx, minlength=size).max()
    cols = np.broadcast_to(np.arange(32), c.shape)
    rows = np.broadcast_to(idx[:, None], c.shape)
    if int(shift.max()) + 25 + _nbits(per) <= 62:
        acc = np.zeros([size, 32], np.int64)
        np.add.at(acc, (rows, cols), mi << shift)
        assert np.abs(acc).max() < (1 << 62)
        s32 = np.ldexp(acc.astype(F32), kmin)                  # int64 -> float32 rounds once; the scaling is exact (checked: normal range)
        s64 = np.ldexp(acc.astype(np.float64), kmin)
        big = acc != 0
        assert np.all(np.abs(s32[big]) >= np.finfo(F32).tiny)
        return s32.astype(F32), s64
    acc = np.zeros([size, 32], dtype=object)
    acc[...] = 0
    vals = np.array([int(a) << int(b) for a, b in zip(mi.ravel(), shift.ravel())], dtype=object).reshape(mi.shape)
    np.add.at(acc, (rows, cols), vals)
    s32 = np.zeros([size, 32], F32); s64 = np.zeros([size, 32], np.float64)
    for i, j in zip(*np.nonzero(acc)):
        v = int(acc[i, j]); a = abs(v); extra = max(a.bit_length() - 24, 0)
        q = a >> extra
        rem = a - (q << extra)
        half = (1 << extra) >> 1
        if extra and (rem > half or (rem == half and (q & 1))):
            q += 1
        r = np.ldexp(float(q), extra + kmin)
        assert np.finfo(F32).tiny <= r <= np.finfo(F32).max
        s32[i, j] = F32(r if v > 0 else -r)
        s64[i, j] = np.ldexp(float(v), kmin) if a.bit_length() <= 1000 else 0.0           # float(int) rounds to nearest
    return s32, s64


def reference(case, rows=None):
    """The scatter of `case` (rows: another [N,M,K,32] float32 array in place of the case's; finite).  A dict of
       S32 [N,3,H,W,32] float32   rn32 of the exact sum S = sum_i rn32(w_i d_i)
       S   [N,3,H,W,32] float64   S to double precision
       A   [N,3,H,W,32] float64   sum_i |rn32(w_i d_i)|
       n   [N,3,H,W]    int       contributions (taps with non-zero weight) per texel
       n_t, B_t [N,3,TY,TX]       records per plane tile and max |dX| over them (the tile of a record: its top-left tap moved onto the plane)
       E_fix [N,3,H,W] float64    the fixed-point allowance per texel: sum over its contributions of U 2^(nbits + e - 61) of the record's tile
       taps: (texel index [n], tile index [n], sample index [n], weight [n]) of every contribution, for the precondition checks."""
    N, M, K, H, W = case['N'], case['M'], case['K'], case['H'], case['W']
    dx = np.asarray(case['rows'] if rows is None else rows, dtype=F32).reshape(N * M * K, 32)
    assert np.isfinite(dx).all()
    x0, y0, w, _, _ = footprints(case)
    TY, TX = -(-H // TILE), -(-W // TILE)
    item = np.broadcast_to(np.arange(N)[:, None, None, None], x0.shape)
    pl = np.broadcast_to(np.arange(3)[None, None, None, :], x0.shape)
    smp = np.broadcast_to(np.arange(N * M * K).reshape(N, M, K, 1), x0.shape)
    rec = (w != 0).any(-1)
    tile = (item * 3 + pl) * (TY * TX) + (np.clip(y0, 0, H - 1) // TILE) * TX + np.clip(x0, 0, W - 1) // TILE
    n_t = np.bincount(tile[rec], minlength=N * 3 * TY * TX)
    B_t = np.zeros(N * 3 * TY * TX, F32)
    np.maximum.at(B_t, tile[rec], np.abs(dx).max(1)[smp[rec]])
    tex, til, sm, wt = [], [], [], []
    for j in range(4):
        on = w[..., j] != 0
        tex.append(((item[on] * 3 + pl[on]) * H + y0[on] + j // 2) * W + x0[on] + j % 2)
        til.append(tile[on]); sm.append(smp[on]); wt.append(w[..., j][on])
    tex, til, sm, wt = (np.concatenate(a) for a in (tex, til, sm, wt))
    c = wt[:, None] * dx[sm]                                               # float32 products: rn32(w d)
    assert c.dtype == F32 and np.isfinite(c).all()
    size = N * 3 * H * W
    S32, S = _exact_sums(tex, c, size)
    A = np.zeros([size, 32], np.float64)
    np.add.at(A, tex, np.abs(c).astype(np.float64))
    n = np.bincount(tex, minlength=size)
    e_t = np.frexp(B_t)[1].astype(np.int64)
    nb_t = np.array([_nbits(v) for v in n_t], np.int64)
    E = np.zeros(size, np.float64)
    np.add.at(E, tex, U_FIXED * 2.0 ** (nb_t[til] + e_t[til] - 61).astype(np.float64))
    shp = (N, 3, H, W)
    return dict(S32=S32.reshape(*shp, 32), S=S.reshape(*shp, 32), A=A.reshape(*shp, 32), n=n.reshape(shp), n_t=n_t.reshape(N, 3, TY, TX),
                B_t=B_t.reshape(N, 3, TY, TX), E_fix=E.reshape(shp), taps=(tex, til, sm, wt), c=c)


def exact_tier_violations(case, ref):
    """Contributions that break the exact tier's cap: non-zero and below 2^(nbits - 27) B_t of their record's tile.  With
    s = 61 - nbits - e and B_t >= 2^(e-1) such a contribution c = rn32(w d) has ulp(c) 2^s >= 2^(e + nbits - 28 - 23 + s) = 2^10 >= 2^8:
    c 2^s is an integer multiple of 256, which converts exactly whatever its sign (bin_to_fixed_model)."""
    tex, til, sm, wt = ref['taps']
    c = np.abs(ref['c'])
    nb = np.array([_nbits(v) for v in ref['n_t'].ravel()], np.int64)
    cap = np.ldexp(ref['B_t'].ravel().astype(np.float64), nb - 27)[til]
    return int(((c != 0) & (c.astype(np.float64) < cap[:, None])).sum())


def fractions_in_eighths(case):
    x0, y0, w, fx, fy = footprints(case)
    on = (w != 0).any(-1)
    return bool(np.all(fx[on] * 8 == np.round(fx[on] * 8)) and np.all(fy[on] * 8 == np.round(fy[on] * 8)))


def bin_to_fixed_model(t):
    """bin_to_fixed of scatter_binned.inl in numpy float32 (an fma with one rounding; saturating, truncating conversions that send NaN to
    zero) -> the signed 64-bit value as a Python int."""
    t = F32(t)
    hi = np.floor(F32(t * F32(2.0 ** -32)))
    lo = F32(np.float64(hi) * -4294967296.0 + np.float64(t))        # exact in float64 (see the test), rounded once: the fma
    lo_u = 0 if not lo == lo else int(min(max(float(np.trunc(lo)), 0.0), 4294967295.0))
    hi_i = 0 if not hi == hi else int(min(max(float(hi), -2147483648.0), 2147483647.0))
    v = ((hi_i & 0xffffffff) << 32) | lo_u
    return v - (1 << 64) if v >= (1 << 63) else v


# ---------------------------------------------------------------------------------------------------------------------------------
# Cases.  A case: dict(name, N, M, K, H, W, box_warp, image_width, origins [N,M,3], dirs [N,M,3], depths [N,M,K], rows [N,M,K,32]).

FAR = 8.0           # a coordinate (in units of box_warp) far off every plane


def lattice_step(H, W, box_warp):
    """The coarsest-needed lattice step q >= 2^-6 for origins and depths at which every fraction is a multiple of 1/8: a half-step
    direction moves a texel coordinate by (q / 2) (2 / box_warp) (n / 2)."""
    q = 2.0 ** -6
    while any(((q / box_warp) * n / 2 * 8) % 1 for n in (H, W)):
        q *= 2
    return q


def int_rows(rng, shape, m=0, mixed=True):
    """Small non-zero integers (|v| <= 15: a spread below 2^4) times 2^m.  mixed: a random sign per value; otherwise one sign per
    channel (even channels positive, odd ones negative), so that no texel's sum cancels."""
    sign = rng.choice([-1, 1], size=shape) if mixed else np.broadcast_to(np.where(np.arange(shape[-1]) % 2 == 0, 1, -1), shape)
    return np.ldexp((rng.integers(1, 16, size=shape) * sign).astype(F32), m).astype(F32)


def random_case(name, seed, N, M, K, H, W, box_warp=1.0, image_width=0, m=0):
    """Rays on the lattice across the plane and a little beyond it, integer rows at scale 2^m.
    A texel on a tile's first row or column is the float32 sum of up to four partial sums, each rounded on its own: it is within 4 ulp
    of rn32(S) (four roundings and three additions of half an ulp each) PROVIDED no partial sum is larger than S, i.e. nothing cancels.
    So planes of more than one tile get rows with one sign per channel; one-tile planes, which have no halo, get mixed signs."""
    rng = np.random.default_rng(seed)
    q = lattice_step(H, W, box_warp)
    lim = int(round(0.5625 * box_warp / q))
    o = rng.integers(-lim, lim + 1, size=(N, M, 3)) * q
    d = rng.choice([0.0, 0.5, -0.5, 1.0, -1.0], size=(N, M, 3))
    t = rng.integers(0, int(round(0.375 * box_warp / q)) + 1, size=(N, M, K)) * q
    return dict(name=name, N=N, M=M, K=K, H=H, W=W, box_warp=box_warp, image_width=image_width, origins=o.astype(F32), dirs=d.astype(F32),
                depths=t.astype(F32), rows=int_rows(rng, (N, M, K, 32), m, mixed=H <= TILE and W <= TILE))


def coord_of(i, n, box_warp):
    """The world coordinate whose texel coordinate is i on an axis of n texels."""
    return ((2.0 * i + 1.0) / n - 1.0) * box_warp / 2.0


def placed_case(name, seed, H, W, targets, K=8, box_warp=1.0, image_width=0, m=0, M=None):
    """One ray per target (ix, iy) of plane 0 (on the lattice: asserted), directed along (1/2, 1/2, 1) from a z far outside: its K samples
    sit at the target plus 0 .. 3 lattice steps along the diagonal in plane 0 and make no record in the planes that read z.  Rays beyond
    the targets are fully outside."""
    rng = np.random.default_rng(seed)
    M = M or -(-len(targets) // 16) * 16
    o = np.full((1, M, 3), FAR * box_warp)
    for r, (ix, iy) in enumerate(targets):
        o[0, r, 0], o[0, r, 1] = coord_of(ix, W, box_warp), coord_of(iy, H, box_warp)
    assert np.all(o * 64 == np.round(o * 64)), 'a target is off the lattice'
    d = np.zeros((1, M, 3)); d[..., :2] = 0.5; d[..., 2] = 1.0
    t = rng.integers(0, 4, size=(1, M, K)) / 64.0
    return dict(name=name, N=1, M=M, K=K, H=H, W=W, box_warp=box_warp, image_width=image_width, origins=o.astype(F32), dirs=d.astype(F32),
                depths=t.astype(F32), rows=int_rows(rng, (1, M, K, 32), m))


def merge_items(name, a, b):
    """Two one-item cases of the same shape as one two-item case."""
    out = dict(a, name=name, N=a['N'] + b['N'])
    for k in ('origins', 'dirs', 'depths', 'rows'):
        out[k] = np.concatenate([a[k], b[k]], axis=0)
    return out


def count_case(n_t, seed=0, m=0):
    """Exactly n_t records, all in the one tile of plane 0 of a 16 x 16 plane; every other sample is fully outside.  The rays run along
    (1/2, 0, 1) from z far outside: a depth of j / 64 (j < 8) moves a sample by j / 8 of a texel, a depth of 64 takes it off the plane."""
    rng = np.random.default_rng(1000 + n_t + seed)
    H = W = 16
    M, K = (16, 8) if n_t <= 128 else (80, 64)
    o = np.zeros((1, M, 3)); o[..., 2] = FAR
    o[0, :, 0] = coord_of(rng.integers(0, 14 * 4, size=M) / 4.0, W, 1.0)
    o[0, :, 1] = coord_of(rng.integers(0, 15 * 4, size=M) / 4.0, H, 1.0)
    d = np.zeros((1, M, 3)); d[..., 0] = 0.5; d[..., 2] = 1.0
    t = np.full(M * K, 64.0)
    inside = rng.permutation(M * K)[:n_t]
    t[inside] = rng.integers(0, 8, size=n_t) / 64.0
    return dict(name=f'count{n_t}', N=1, M=M, K=K, H=H, W=W, box_warp=1.0, image_width=0, origins=o.astype(F32), dirs=d.astype(F32),
                depths=t.reshape(1, M, K).astype(F32), rows=int_rows(rng, (1, M, K, 32), m))


# (on a 32-texel axis the lattice's origins sit on half texels, on a 16-texel axis on quarter texels; the diagonal steps refine both)
SEAM_TARGETS = [(x + fx, y + fy) for x in (14, 15, 16) for y in (14, 15, 16) for fx, fy in ((0.5, 0.5), (0.0, 0.5), (0.5, 0.0))]
EDGE_TARGETS = lambda H, W: ([(-0.5, 3.25), (-1.0, -0.25), (4.5, -0.5), (-1.0, 5.0), (W - 0.5, 2.0), (W - 1.0, H - 0.75), (W - 0.5, H - 0.5),
                              (7.5, H - 0.5), (-1.5, 4.0), (-3.0, -3.0), (W + 0.0, 5.0), (W + 2.0, H + 2.0), (5.0, H + 0.0), (3.5, 6.5)])

TILINGS = {'image': dict(N=2, M=64, image_width=8), 'padded': dict(N=3, M=25, image_width=0)}


def geometry_case(geometry, tiling):
    """The exact tier's geometry cases in one of the two ray tilings.  Placed rays (seams, edges) are item 0's first rays; the others are
    random lattice rays."""
    tl = TILINGS[tiling]
    N, M, iw = tl['N'], tl['M'], tl['image_width']
    H, W = {'one_tile': (16, 16), 'seams': (32, 32), 'partial': (24, 40), 'edges': (16, 32), 'tiles1092': (208, 224)}[geometry]
    K = 16 if geometry == 'tiles1092' else 8
    if geometry == 'tiles1092':
        N, M = 2, (64 if tiling == 'image' else 25)
        iw = 8 if tiling == 'image' else 0
    seed = sum(map(ord, geometry + tiling))
    case = random_case(f'{geometry}-{tiling}', seed, N, M, K, H, W, 1.0, iw)
    targets = SEAM_TARGETS if geometry == 'seams' else EDGE_TARGETS(H, W) if geometry == 'edges' else []
    if targets:
        targets = targets[:M]
        pc = placed_case('', seed, H, W, targets, K=K, M=len(targets))
        n = len(targets)
        for k in ('origins', 'dirs', 'depths'):
            case[k][0, :n] = pc[k][0]
    return case


GEOMETRIES = ('one_tile', 'seams', 'partial', 'edges', 'tiles1092')


def magnitude_case():
    return random_case('magnitudes', 7, 1, 32, 8, 32, 32)


MAGNITUDES = (-100, -60, -30, -4, -3, -2, 0, 20, 60, 100)
COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 4096, 4097)


def padding_case():
    """Row 0 of the staging buffer -- what the padding records of every segment read -- holds ray 0's depths: 2^100 each, with K = 32 in
    all 32 channels.  Ray 0 points away along all three axes and makes no record; the rows are at 2^-60, so every tile rescales its rows
    by 2^(s - 64) and a padding record's 0 * (2^100 2^(s-64)) is 0 * inf."""
    case = random_case('padding', 21, 1, 32, 32, 32, 32, m=-60)
    case['dirs'][0, 0] = (1.0, -0.5, 0.5)
    case['depths'][0, 0] = F32(2.0 ** 100)
    return case


def wide_case():
    """Mixed magnitudes inside one tile: randn rows, each row at its own scale out of 2^-20 .. 2^20."""
    rng = np.random.default_rng(3)
    case = random_case('wide', 3, 1, 32, 16, 16, 16)
    rows = rng.standard_normal(case['rows'].shape) * np.ldexp(1.0, rng.integers(-20, 21, size=case['rows'].shape[:3]))[..., None]
    case['rows'] = rows.astype(F32)
    return case


def sign_case():
    """One row of ones at texel (1, 1) sets tile (0, 0)'s bound; 31 rays sit on texels of their own (integer coordinates: one tap of
    weight fl(1/3)) with negative rows of magnitude 2^-22 .. 2^-50 x [1, 2): between 1 and 2^32 units of the tile's 2^-s (s = 52 at
    these 256 records)."""
    rng = np.random.default_rng(9)
    targets = [(1.0, 1.0)] + [(3.0 + (i % 6) * 2, 3.0 + (i // 6) * 2) for i in range(31)]
    case = placed_case('sign', 9, 16, 16, targets, K=8, M=32)
    case['dirs'][..., :2] = 0          # every sample of a ray on the ray's own texel
    mag = np.ldexp(1.0 + rng.random((31, 8, 32)), -rng.integers(22, 51, size=(31, 8, 1)))
    case['rows'][0, 0] = F32(1.0)
    case['rows'][0, 1:] = (-mag).astype(F32)
    return case


NONFINITE_AT = ((0, 0, 0), (0, 1, 0))           # (item, ray, sample) of the inf row and of the NaN row


def nonfinite_case():
    """randn rows over a 64 x 64 plane; rays 0 and 1 are placed inside tiles (0, 0) and (2, 2) of plane 0 and are the carriers of
    the inf row and the NaN row (values only: every depth, origin and direction stays finite).  Returns (case with the two rows zeroed,
    rows with them set)."""
    rng = np.random.default_rng(4)
    case = random_case('nonfinite', 4, 1, 32, 8, 64, 64)
    pc = placed_case('', 4, 64, 64, [(5.5, 5.5), (40.5, 41.5)], K=8, M=2)
    for k in ('origins', 'dirs', 'depths'):
        case[k][0, :2] = pc[k][0]
    case['rows'] = rng.standard_normal(case['rows'].shape).astype(F32)
    for at in NONFINITE_AT:
        case['rows'][at] = 0
    bad = case['rows'].copy()
    bad[NONFINITE_AT[0]] = np.inf
    bad[NONFINITE_AT[1]] = np.nan
    return case, bad
