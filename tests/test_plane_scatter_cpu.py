"""The plane-gradient scatter's reference and cases, without a GPU (tests/scatter_ref.py; the GPU tests are test_plane_scatter_gpu.py):
the reference against autograd through grid_sample, every case generator against the preconditions its GPU test states -- so that a
failure there is the kernel's and not the case's -- and a float32 model of bin_to_fixed against floor(t)."""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import scatter_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_CASES = ([('magnitudes', SR.magnitude_case), ('padding', SR.padding_case)] + [(f'count{n}', lambda n=n: SR.count_case(n)) for n in SR.COUNTS] +
               [(f'{g}-{t}', lambda g=g, t=t: SR.geometry_case(g, t)) for g in SR.GEOMETRIES for t in SR.TILINGS])


def test_export_is_declared_bound_and_optional():
    import gnerf_hip
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    m = re.search(r'\bint\s+gnerf_render_scatter_rows\s*\(([^)]*)\)\s*;', header)
    assert m, 'gnerf_render_scatter_rows is not declared'
    params = [a.strip() for a in m.group(1).split(',')]
    assert [a.split()[-1].lstrip('*') for a in params] == ['p', 'stage', 'grad_planes_nhwc', 'stream']
    assert params[0].startswith('const gnerf_render_params*') and params[1].startswith('float*') and params[2].startswith('float*')
    assert re.search(r'#define\s+GNERF_ABI_VERSION\s+15\b', header) and gnerf_hip.ABI_VERSION == 15
    res, args = gnerf_hip.SIGNATURES['gnerf_render_scatter_rows']
    assert res is ctypes.c_int and len(args) == 4 and args[0]._type_ is gnerf_hip.RenderParams and all(a is ctypes.c_void_p for a in args[1:])
    assert 'gnerf_render_scatter_rows' in gnerf_hip.OPTIONAL_SYMBOLS
    assert gnerf_hip.load().gnerf_render_scatter_rows.argtypes == args
    assert gnerf_hip.scatter_plane_rows_available()
    with pytest.raises(RuntimeError, match='not on a GPU'):
        z = torch.zeros(3, 16, 16, 32)
        gnerf_hip.scatter_plane_rows(z, 1, torch.zeros(1, 16, 3), torch.zeros(1, 16, 3), torch.zeros(1, 16, 8), torch.zeros(1, 16, 8, 32), box_warp=1.0)


@pytest.mark.parametrize('seed,N,M,K,H,W,box_warp', [(1, 2, 16, 8, 16, 16, 1.0), (2, 1, 25, 9, 24, 40, 2.0), (3, 3, 7, 8, 33, 17, 1.0), (4, 1, 32, 16, 64, 32, 2.0)])
def test_reference_agrees_with_grid_sample_autograd(seed, N, M, K, H, W, box_warp):
    """S against float64 autograd through F.grid_sample on the same points, rows divided by 3: to 2^-22 A per texel.  This guards the
    reference's geometry and its plane-axis convention, nothing finer."""
    case = SR.random_case('x', seed, N, M, K, H, W, box_warp)
    rng = np.random.default_rng(seed)
    case['rows'] = rng.standard_normal(case['rows'].shape).astype(np.float32)
    ref = SR.reference(case)
    o, d, t, rows = (torch.from_numpy(case[k]).double() for k in ('origins', 'dirs', 'depths', 'rows'))
    p = (o[:, :, None, :] + t[..., None] * d[:, :, None, :]) * (2.0 / box_warp)                  # [N,M,K,3]
    uv = torch.stack([p[..., [0, 1]], p[..., [0, 2]], p[..., [2, 0]]], dim=1).reshape(N * 3, 1, M * K, 2)
    planes = torch.zeros(N * 3, 32, H, W, dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.grid_sample(planes, uv, mode='bilinear', padding_mode='zeros', align_corners=False)      # [3N,32,1,MK]
    g = (rows / 3.0).reshape(N, 1, M * K, 32).expand(N, 3, M * K, 32).reshape(N * 3, 1, M * K, 32).permute(0, 3, 1, 2)
    (out * g).sum().backward()
    got = planes.grad.reshape(N, 3, 32, H, W).permute(0, 1, 3, 4, 2).numpy()
    assert (ref['n'] > 0).sum() > 50
    assert np.all(np.abs(got - ref['S']) <= 2.0 ** -22 * ref['A'])
    assert np.all(np.abs(ref['S32'].astype(np.float64) - ref['S']) <= 2.0 ** -24 * np.abs(ref['S']))


def test_exact_sum_paths_agree():
    """The int64 and the Python-integer summation of the reference give the same bits where both apply."""
    case = SR.magnitude_case()
    x0, y0, w, _, _ = SR.footprints(case)
    ref = SR.reference(case)
    tex, _, sm, wt = ref['taps']
    c = ref['c'].copy()
    size = ref['n'].size
    a32, a64 = SR._exact_sums(tex, c, size)
    c2 = np.concatenate([c, np.full((1, 32), 2.0 ** 60, np.float32), np.full((1, 32), -2.0 ** 60, np.float32)])       # forces the wide path, adds zero
    b32, b64 = SR._exact_sums(np.concatenate([tex, [0, 0]]), c2, size)
    assert np.array_equal(a32.view(np.uint32), b32.view(np.uint32)) and np.array_equal(a64, b64)


@pytest.mark.parametrize('name,make', EXACT_CASES, ids=[n for n, _ in EXACT_CASES])
def test_exact_tier_cases_meet_their_preconditions(name, make):
    """Lattice exactness (asserted inside footprints), fractions in eighths, integer rows times one power of two with a spread of at
    most 2^4 per tile, and the cap: every non-zero contribution is at least 2^(nbits - 27) B_t of its record's tile."""
    case = make()
    ref = SR.reference(case)
    assert SR.fractions_in_eighths(case)
    assert SR.exact_tier_violations(case, ref) == 0
    rows = case['rows'].astype(np.float64)
    unit = np.abs(rows[rows != 0]).min()
    assert math.log2(unit) == round(math.log2(unit)) and np.all(rows / unit == np.round(rows / unit)) and np.abs(rows / unit).max() <= 16
    for k in ('origins', 'depths'):
        v = case[k].astype(np.float64)
        assert np.all(v * 64 == np.round(v * 64))
    assert set(np.unique(case['dirs'])) <= {0.0, 0.5, -0.5, 1.0, -1.0} and case['box_warp'] in (1.0, 2.0)
    assert np.isfinite(case['depths']).all() and (ref['n'] > 0).sum() > 0
    # the seam criterion's precondition: on a tile's first row or column of a plane with halos nothing cancels (|S| = A, both exact here)
    if case['H'] > SR.TILE or case['W'] > SR.TILE:
        seam = (np.arange(case['H'])[:, None] % SR.TILE == 0) | (np.arange(case['W'])[None, :] % SR.TILE == 0)
        assert np.array_equal(np.abs(ref['S'])[:, :, seam], ref['A'][:, :, seam]) and (ref['n'][:, :, seam] > 1).any()
    elif ref['n'].max() >= 8:
        assert (np.abs(ref['S']) < ref['A']).any()            # one-tile planes carry the mixed signs


@pytest.mark.parametrize('n_t', SR.COUNTS)
def test_count_cases_put_exactly_n_records_in_one_tile(n_t):
    ref = SR.reference(SR.count_case(n_t))
    assert ref['n_t'].max() == n_t and (ref['n_t'] > 0).sum() == 1 and ref['n_t'][0, 0, 0, 0] == n_t


def _records(case):
    x0, y0, w, fx, fy = SR.footprints(case)
    return x0, y0, (w != 0).any(-1), w


@pytest.mark.parametrize('tiling', list(SR.TILINGS))
def test_geometry_cases_reach_what_they_are_for(tiling):
    tl = SR.TILINGS[tiling]
    assert (tl['image_width'] > 0 and tl['M'] == tl['image_width'] ** 2 and tl['image_width'] % 4 == 0) or (tl['N'] > 1 and tl['M'] % 16 != 0)
    # seams: footprints across the right seam, the lower seam and the four-tile corner; texel (16, 16) is fed by four tiles
    case = SR.geometry_case('seams', tiling)
    x0, y0, rec, w = _records(case)
    assert (rec & (x0 == 15) & (y0 < 15) & (w[..., 1] != 0)).any() and (rec & (y0 == 15) & (x0 < 15) & (w[..., 2] != 0)).any()
    assert (rec & (x0 == 15) & (y0 == 15) & (w[..., 3] != 0)).any()
    ref = SR.reference(case)
    tex, til = ref['taps'][:2]
    assert len(set(til[tex == (0 * 32 + 16) * 32 + 16])) == 4
    # partial tiles
    case = SR.geometry_case('partial', tiling)
    x0, y0, rec, w = _records(case)
    assert (case['H'], case['W']) == (24, 40) and (rec & (x0 >= 32)).any() and (rec & (y0 >= 16)).any() and (rec & (x0 == 39)).any() and (rec & (y0 == 23)).any()
    # edges: footprints that start at -1 and are moved onto the plane, footprints that end at W / H, samples fully outside
    case = SR.geometry_case('edges', tiling)
    x0, y0, rec, w = _records(case)
    H, W = case['H'], case['W']
    assert (rec & (x0 == -1)).any() and (rec & (y0 == -1)).any() and (rec & (x0 == -1) & (y0 == -1)).any()
    assert (rec & (x0 == W - 1)).any() and (rec & (y0 == H - 1)).any() and (rec & (x0 == W - 1) & (y0 == H - 1)).any()
    assert (~rec).any() and (~rec & ((x0 == -2) | (x0 == W))).any()
    # more than 1024 plane tiles, records on both sides of index 1024 -- below it in the same item too
    case = SR.geometry_case('tiles1092', tiling)
    n_t = SR.reference(case)['n_t'].ravel()
    assert n_t.size == 1092 and (n_t[1024:] > 0).sum() >= 10 and (n_t[546:1024] > 0).sum() >= 10 and (n_t[:546] > 0).sum() >= 10


def test_padding_case():
    """Ray 0: all three direction components non-zero, finite depths of 2^100, no record; segments that are no multiple of four, in
    tiles whose scale exceeds 64 (so that the padding records' rows are rescaled beyond the float range)."""
    case = SR.padding_case()
    assert np.all(case['dirs'][0, 0] != 0) and np.all(case['depths'][0, 0] == np.float32(2.0 ** 100)) and case['K'] == 32
    x0, y0, rec, w = _records(case)
    assert not rec[0, 0].any() and rec[0, 1:].any()
    ref = SR.reference(case)
    n_t, B_t = ref['n_t'].ravel(), ref['B_t'].ravel()
    assert {1, 2, 3} <= set((n_t[n_t > 0] % 4).tolist())
    for n, b in zip(n_t[n_t > 0], B_t[n_t > 0]):
        s = 61 - SR._nbits(n) - math.frexp(float(b))[1]
        assert s - 64 + 100 > 128                     # 2^100 2^(s-64) is beyond float32: the padding record's product is 0 * inf


def test_sign_case():
    """One record of ones sets the bound of the one tile; every other contribution is negative, sits on a texel of its own ray and lies
    between 1 and 2^32 units of the tile's scale."""
    case = SR.sign_case()
    ref = SR.reference(case)
    assert (ref['n_t'] > 0).sum() == 1 and ref['n_t'][0, 0, 0, 0] == 256 and ref['B_t'][0, 0, 0, 0] == 1.0
    s = 61 - 8 - 1
    c = ref['c'].astype(np.float64)
    neg = c < 0
    assert neg.sum() == 31 * 8 * 32 and np.all(c[~neg] > 0) and (~neg).sum() == 8 * 32
    units = -c[neg] * 2.0 ** s
    assert units.min() >= 1 and units.max() < 2.0 ** 32
    assert ref['n'][0, 0].max() == 8 and (ref['n'][0, 0] == 8).sum() == 32 and not (ref['n'][0, 0, 0, :] > 0).any() and not (ref['n'][0, 0, :, 0] > 0).any()


def test_nonfinite_case():
    """The carriers of the inf and the NaN row make one record each, in the interior of tiles (0, 0) and (2, 2) of plane 0."""
    case, bad = SR.nonfinite_case()
    assert np.isfinite(case['origins']).all() and np.isfinite(case['dirs']).all() and np.isfinite(case['depths']).all()
    assert np.isinf(bad[SR.NONFINITE_AT[0]]).all() and np.isnan(bad[SR.NONFINITE_AT[1]]).all() and (~np.isfinite(bad)).sum() == 64
    x0, y0, rec, w = _records(case)
    for (i, r, k), tile in zip(SR.NONFINITE_AT, ((0, 0), (2, 2))):
        assert rec[i, r, k].tolist() == [True, False, False]
        assert (y0[i, r, k, 0] // 16, x0[i, r, k, 0] // 16) == tile and 1 <= x0[i, r, k, 0] % 16 <= 13 and 1 <= y0[i, r, k, 0] % 16 <= 13


def test_wide_case_mixes_magnitudes_inside_a_tile():
    case = SR.wide_case()
    ref = SR.reference(case)
    assert ref['n_t'].shape[2:] == (1, 1)
    mags = np.abs(case['rows']).max(-1)
    assert mags.max() / mags.min() > 2.0 ** 30


def test_bin_to_fixed_model_against_floor():
    """What the conversion of scatter_binned.inl guarantees, from its float32 model: exact (= floor(t)) for t >= 0 and for t <= -2^32;
    for -2^32 < t < 0 the low word 2^32 - |t| needs up to 32 bits, is rounded to 24 (and saturates at the top), and the result is off
    floor(t) by up to 128 units, in either direction."""
    model = SR.bin_to_fixed_model
    assert [model(t) for t in (-5.0, -129.0, -12345.0)] == [-1, -256, -12288]
    assert [model(t) for t in (0.0, -0.0, 1.5, 5.0, -1.5, float('nan'))] == [0, 0, 1, 5, -1, 0]
    rng = np.random.default_rng(0)
    worst = {}
    for k in range(0, 41):
        for sign in (1.0, -1.0):
            ts = [sign * 2.0 ** k, sign * (2.0 ** (k + 1) - 2.0 ** (k - 23))] + list(sign * np.ldexp(1.0 + rng.random(200), k))
            ts += [sign * (2.0 ** k + 2.0 ** (k - 1)), sign * (2.0 ** k + 2.0 ** (k - 2))]
            err = 0
            for t in ts:
                t = float(np.float32(t))
                # the model's fma is exact in float64 before its one rounding: hi 2^32 and t overlap within 53 bits
                e = model(t) - math.floor(t)
                err = max(err, abs(e))
            worst[(k, sign)] = err
    for k in range(0, 41):
        assert worst[(k, 1.0)] == 0, k
        if k >= 32:
            assert worst[(k, -1.0)] == 0, k
        else:
            assert worst[(k, -1.0)] <= 128, (k, worst[(k, -1.0)])
    assert max(worst[(k, -1.0)] for k in range(8, 32)) == 128            # attained: e.g. t = -384 -> -512
    assert model(-384.0) == -512 and model(-128.0) == -1
    assert SR.U_FIXED == 128 + 1
