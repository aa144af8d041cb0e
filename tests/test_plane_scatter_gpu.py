"""The plane-gradient scatter alone on the GPU (gnerf_render_scatter_rows: csrc/scatter_binned.inl, and plane_scatter_kernel under
GNERF_BWD_SCATTER=sorted) against the exact reference of tests/scatter_ref.py, on rows and depths the tests write themselves.

Exact tier.  The binned form adds floor(c 2^s) per contribution c = rn32(w dx), one scale s = 61 - nbits - e per plane tile
(nbits = ceil(log2 n_t), B_t < 2^e).  Where every non-zero c is at least 2^(nbits - 27) B_t, c 2^s is an integer multiple of 256, the
conversion is exact for either sign (test_plane_scatter_cpu.py: the model of bin_to_fixed), the integer sum is exact and the one rounding
to float32 gives rn32(S) -- whatever the scale logic did, so the expected bits do not depend on it.  The cases' generators keep that cap
(checked on the CPU).  Texels on a tile's first row or column add up to four such rounded sums in a fixed order: within 4 ulp of rn32(S)
-- seven roundings of half an ulp, of S as long as no partial sum exceeds S: planes with halos get rows with one sign per channel.

Tolerance tier.  got = rn32(S + d) with |d| <= E_fix, the sum over the texel's contributions of U 2^-s of the contribution's tile:
a conversion is off c 2^s by less than 1 (the floor) plus up to 128 (the low word's rounding for negative values below 2^32 units), so
U = 129, and 2^-s = 2^(nbits + e - 61).  Rounding S + d costs 1/2 ulp32(S) where it stays in S's binade; a change of binade and the
roundings of the seam texels' partial sums are inside 2^-24 A (each partial sum is at most A = sum |c|).  So
|got - S| <= 1/2 ulp32(S) + 2^-24 A + E_fix.  The sorted form adds n float32 products in some order: the standard n 2^-24 A."""

import functools

import numpy as np
import pytest
import torch

import scatter_ref as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda', 0)


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    for k in ('GNERF_BWD_KERNEL', 'GNERF_BWD_MLP', 'GNERF_BWD_SCATTER'):
        monkeypatch.delenv(k, raising=False)


def _run(dev, case, rows=None, interleaved=False, prefill=None):
    """The scatter of `case` on the GPU -> float32 [N,3,H,W,32] (prefill: the same shape, added into)."""
    import gnerf_hip
    N, H, W = case['N'], case['H'], case['W']
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def lay(a):         # [N,3,H,W,32] -> the layout
        return a.permute(0, 2, 3, 1, 4).reshape(N, H, W, 96).contiguous() if interleaved else a.reshape(N * 3, H, W, 32).contiguous()
    like = lay(torch.zeros(N, 3, H, W, 32, device=dev))
    out = None if prefill is None else lay(t(prefill))
    g = gnerf_hip.scatter_plane_rows(like, N, t(case['origins']), t(case['dirs']), t(case['depths']), t(case['rows'] if rows is None else rows),
                                     box_warp=case['box_warp'], image_width=case['image_width'], out=out)
    torch.cuda.synchronize()
    g = g.reshape(N, H, W, 3, 32).permute(0, 3, 1, 2, 4) if interleaved else g.reshape(N, 3, H, W, 32)
    return g.cpu().numpy().copy()


def _seams(H, W):
    return (np.arange(H)[:, None] % 16 == 0) | (np.arange(W)[None, :] % 16 == 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_exact(got, want32, what):
    """Bit equality with rn32(S) off the tiles' first rows and columns, 4 ulp on them."""
    H, W = got.shape[2:4]
    seam = _seams(H, W)
    inner = ~seam
    bad = _bits(got)[:, :, inner] != _bits(want32)[:, :, inner]
    ulps = np.abs(got[:, :, seam].astype(np.float64) - want32[:, :, seam]) / np.spacing(np.abs(want32[:, :, seam])).astype(np.float64)
    print(f'{what}: {int(bad.sum())} of {bad.size} interior values differ; seam texels worst {ulps.max() if ulps.size else 0:.2f} ulp')
    assert not bad.any(), (what, int(bad.sum()), got[:, :, inner][bad][:4], want32[:, :, inner][bad][:4])
    assert np.all(ulps <= 4), (what, float(ulps.max()))


@functools.lru_cache(maxsize=None)
def _geometry(geometry, tiling):
    case = SR.geometry_case(geometry, tiling)
    return case, SR.reference(case)


@functools.lru_cache(maxsize=None)
def _magnitudes():
    case = SR.magnitude_case()
    return case, SR.reference(case)


@pytest.mark.parametrize('m', SR.MAGNITUDES)
def test_magnitudes(dev, m):
    """Rows at 2^m: bounds below 2^-3 (the rescaling loop, s > 64) up to large bounds (negative s).  Exact, and exactly 2^m times m = 0."""
    case, ref = _magnitudes()
    got = _run(dev, case, rows=np.ldexp(case['rows'], m))
    _assert_exact(got, np.ldexp(ref['S32'], m), f'2^{m}')
    unit = _run(dev, case)
    assert np.array_equal(_bits(got), _bits(np.ldexp(unit, m)))


@pytest.mark.parametrize('n_t', SR.COUNTS)
def test_record_counts(dev, n_t):
    """n_t records in one tile: segments with padding records, the steps of nbits, more than one batch per wave."""
    case = SR.count_case(n_t)
    _assert_exact(_run(dev, case), SR.reference(case)['S32'], f'n_t = {n_t}')


@pytest.mark.parametrize('interleaved', [False, True], ids=['planar', 'interleaved'])
@pytest.mark.parametrize('tiling', list(SR.TILINGS))
@pytest.mark.parametrize('geometry', SR.GEOMETRIES)
def test_geometry(dev, geometry, tiling, interleaved):
    """One tile, seams and the four-tile corner, partial tiles, footprints at and beyond the plane's edges, more than 1024 plane tiles;
    image-tiled and padded ray sequences; both plane layouts."""
    case, ref = _geometry(geometry, tiling)
    _assert_exact(_run(dev, case, interleaved=interleaved), ref['S32'], case['name'])


def test_padding_records_read_row_zero(dev):
    """Segments that are no multiple of four records, padded with weight-zero records that read the first ray's depths (2^100, rescaled
    beyond the float range: 0 * inf): they must add nothing."""
    case = SR.padding_case()
    _assert_exact(_run(dev, case), SR.reference(case)['S32'], 'padding')


def test_accumulates_into_out(dev):
    case, ref = _geometry('seams', 'image')
    rng = np.random.default_rng(0)
    prefill = rng.integers(-1000, 1001, size=ref['S32'].shape).astype(np.float32)
    got = _run(dev, case, prefill=prefill)
    want = (prefill.astype(np.float64) + ref['S32'].astype(np.float64)).astype(np.float32)         # (the float64 sum is exact: both within 2^29 of each other)
    inner = ~_seams(case['H'], case['W'])
    assert np.array_equal(_bits(got)[:, :, inner], _bits(want)[:, :, inner])
    untouched = ref['n'] == 0
    assert np.array_equal(_bits(got)[untouched], _bits(prefill)[untouched])


def test_order_independence(dev):
    """The binned form: the same bits for two plain repeats and for the rays of every item in another order."""
    case, _ = _geometry('seams', 'padded')
    first = _run(dev, case)
    assert np.array_equal(_bits(first), _bits(_run(dev, case)))
    rng = np.random.default_rng(1)
    other = dict(case)
    for k in ('origins', 'dirs', 'depths', 'rows'):
        other[k] = case[k].copy()
    for i in range(case['N']):
        perm = rng.permutation(case['M'])
        for k in ('origins', 'dirs', 'depths', 'rows'):
            other[k][i] = case[k][i][perm]
    assert np.array_equal(_bits(first), _bits(_run(dev, other)))


def test_refusals(dev, monkeypatch):
    """Before any launch: the single-pass form stages no rows; a ragged call of several items has no sorted form."""
    import gnerf_hip
    ragged, _ = _geometry('one_tile', 'padded')
    whole, _ = _geometry('one_tile', 'image')
    monkeypatch.setenv('GNERF_BWD_SCATTER', 'direct')
    with pytest.raises(gnerf_hip.NativeError, match='stages no dX rows') as info:
        _run(dev, whole)
    assert info.value.code == gnerf_hip.E_UNSUPPORTED
    monkeypatch.setenv('GNERF_BWD_SCATTER', 'sorted')
    with pytest.raises(gnerf_hip.NativeError, match='straddle items') as info:
        _run(dev, ragged)
    assert info.value.code == gnerf_hip.E_UNSUPPORTED


def _binned_bound(ref):
    return 0.5 * np.spacing(np.abs(ref['S']).astype(np.float32)).astype(np.float64) + 2.0 ** -24 * ref['A'] + ref['E_fix'][..., None]


def _sorted_bound(ref):
    return ref['n'][..., None] * 2.0 ** -24 * ref['A']


def _assert_within(got, ref, bound, what, where=None):
    err = np.abs(got.astype(np.float64) - ref['S'])
    ok = err <= bound
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    if where is not None:
        ok, ratio = ok | ~where[..., None], np.where(where[..., None], ratio, 0.0)
    print(f'{what}: worst error / bound {ratio.max():.3g}, {int((~ok).sum())} outside')
    assert ok.all(), (what, float(ratio.max()))


@pytest.mark.parametrize('form', ['binned', 'sorted'])
def test_mixed_magnitudes_in_one_tile(dev, monkeypatch, form):
    case = SR.wide_case()
    ref = SR.reference(case)
    if form == 'sorted':
        monkeypatch.setenv('GNERF_BWD_SCATTER', 'sorted')
    _assert_within(_run(dev, case), ref, _binned_bound(ref) if form == 'binned' else _sorted_bound(ref), f'wide {form}')


@pytest.mark.parametrize('form', ['binned', 'sorted'])
def test_small_negative_rows_under_a_large_bound(dev, monkeypatch, form):
    """The sign case: what the low word's rounding does to texels that receive only small negative contributions.  Prints the worst
    per-texel error in units of the tile's 2^-s before it asserts the bound.
    Measured on an MI355X: binned -652.8 .. +672.8 units per texel of 8 contributions (flooring alone would stay within -8 .. 0; the
    allowance at U = 129 is 1032), sorted -144.1 .. +126.7 (float32 roundings of sums near 2^-22).  The conversion's error is as its
    model predicts; bin_to_fixed's comment, the head of scatter_binned.inl and include/gnerf_hip.h state it."""
    case = SR.sign_case()
    ref = SR.reference(case)
    if form == 'sorted':
        monkeypatch.setenv('GNERF_BWD_SCATTER', 'sorted')
    got = _run(dev, case)
    units = (got.astype(np.float64) - ref['S']) * 2.0 ** 52
    small = ref['S'] < 0
    print(f'sign case, {form}: error of the negative texels in units of 2^-52: min {units[small].min():.1f} max {units[small].max():.1f} '
          f'(8 contributions per texel; allowance {8 * SR.U_FIXED})')
    _assert_within(got, ref, _binned_bound(ref) if form == 'binned' else _sorted_bound(ref), f'sign {form}')


@pytest.mark.parametrize('form', ['binned', 'sorted'])
def test_nonfinite_rows_stay_in_their_tiles(dev, monkeypatch, form):
    """An inf row and a NaN row (values only) in two tiles: the texels they reach are non-finite; outside those tiles and the first row /
    column of their right, lower and diagonal neighbours the binned result is bit-identical to the run with the two rows zeroed (the
    sorted form, which is not reproducible from run to run: inside its bound of the reference)."""
    case, bad_rows = SR.nonfinite_case()
    ref = SR.reference(case)
    if form == 'sorted':
        monkeypatch.setenv('GNERF_BWD_SCATTER', 'sorted')
    clean, bad = _run(dev, case), _run(dev, case, rows=bad_rows)
    x0, y0, w, _, _ = SR.footprints(case)
    H, W = case['H'], case['W']
    excluded = np.zeros((case['N'], 3, H, W), bool)
    for i, r, k in SR.NONFINITE_AT:
        for j in range(4):
            if w[i, r, k, 0, j] != 0:
                assert not np.isfinite(bad[i, 0, y0[i, r, k, 0] + j // 2, x0[i, r, k, 0] + j % 2]).any()
        ty, tx = y0[i, r, k, 0] // 16, x0[i, r, k, 0] // 16
        excluded[i, 0, 16 * ty:16 * ty + 17, 16 * tx:16 * tx + 17] = True
    if form == 'binned':
        assert np.array_equal(_bits(bad)[~excluded], _bits(clean)[~excluded])
        _assert_within(clean, ref, _binned_bound(ref), 'nonfinite (zeroed) binned')
    else:
        _assert_within(bad, ref, _sorted_bound(ref), 'nonfinite sorted', where=~excluded)


# ---- through the whole call: the backward at scaled incoming gradients, on the default route

@functools.lru_cache(maxsize=None)
def _whole_call(key):
    from test_gpu_parity import _oracle_grads, _random_scene
    cfg = dict(key)
    scene = _random_scene(11, **cfg)
    N, M = cfg['N'], cfg['res'] ** 2
    gen = torch.Generator().manual_seed(5)
    grads = torch.randn(N, M, 32, generator=gen), torch.randn(N, M, 1, generator=gen), torch.randn(N, M, 1, generator=gen)
    opts = dict(depth_resolution=cfg['S'], depth_resolution_importance=cfg['F'], ray_start=2.25, ray_end=3.3, box_warp=1.0, clamp_mode='softplus', white_back=False)
    return scene, grads, _oracle_grads(*scene, opts, *grads)


@pytest.mark.parametrize('scale', [1e-6, 1e6])
@pytest.mark.parametrize('cfg', [dict(N=1, res=4, S=12, F=0, hw=(8, 8)), dict(N=2, res=8, S=48, F=48, hw=(32, 32))], ids=['12+0', '48+48'])
def test_render_backward_vs_oracle_at_scaled_gradients(dev, cfg, scale):
    """gnerf_render_backward on its default route with the incoming gradients times 1e-6 / 1e6, against the float64 oracle's gradients
    times the same factor (the backward is linear in them): test_render_backward_vs_oracle's relative tolerances."""
    import gnerf_hip
    from test_gpu_parity import _entrywise_ok, _rel, _rel_l2
    (planes, dec, o, d, nc, nf), grads, (ref_planes, ref_dec) = _whole_call(tuple(sorted((k, v) for k, v in cfg.items())))
    N, S, F = cfg['N'], cfg['S'], cfg['F']
    nhwc = gnerf_hip.planes_to_nhwc(planes.to(dev))
    gp, gdec = gnerf_hip.render_backward(nhwc, N, [t.to(dev) for t in dec], o.to(dev), d.to(dev), nc.to(dev), nf.to(dev) if F else None,
                                         *[(g * scale).to(dev) for g in grads], depth_resolution=S, depth_resolution_importance=F,
                                         ray_start=2.25, ray_end=3.3, box_warp=1.0, image_width=cfg['res'])
    gp = gp.reshape(N, 3, *cfg['hw'], 32).permute(0, 1, 4, 2, 3).cpu()
    want = ref_planes * scale
    print(f'scale {scale}: planes rel {_rel(gp, want):.3g} rel_l2 {_rel_l2(gp, want):.3g}')
    assert _rel(gp, want) < 2e-3 and _rel_l2(gp, want) < 1e-3 and _entrywise_ok(gp, want)
    for name, a, b in zip(['w1', 'b1', 'w2', 'b2'], gdec, ref_dec):
        assert _rel(a.cpu(), b * scale) < 2e-3 and _rel_l2(a.cpu(), b * scale) < 1e-3, name
