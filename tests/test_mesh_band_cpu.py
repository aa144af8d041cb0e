"""CPU tests of the narrow-band density volume (shape_mi355x.band_volume_numpy, the numpy port of csrc/mesh_band.hip and the CPU path of
band_volume): the mesh of the band volume against the dense volume's, byte for byte; what the evaluated and the unevaluated points hold; the
edge cases of the rules; the index form of voxel_samples and extract_density_grid(band=...) on the CPU; the CLI flag and the declarations of the
native layer."""

import os
import re

import numpy as np
import pytest
import torch

import shape_mi355x as S
from mesh_band_cases import NOISE_KEEP, SPHERE_KEEP, CountingField, cropped, field, restricted_dense, same_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_band(dense, level, s, keep=None):
    """-> (band volume before the crop, report, the counting field, band mesh, dense mesh), both meshes of the cropped volumes."""
    f = CountingField(dense)
    vol, report = S.band_volume_numpy(f, dense.shape[0], level, s, keep)
    assert vol.shape == dense.shape and vol.dtype == np.float32
    assert f.calls.max() <= 1, 'an index was asked for twice'
    assert report['points'] == int(f.calls.sum()) and report['share'] == report['points'] / dense.size
    assert report['rounds'] == len(report['new_bricks']) and report['host_reads'] == report['rounds'] + 1 and report['brick'] == s
    return vol, report, f, S.marching_cubes_numpy(cropped(vol, keep), level), S.marching_cubes_numpy(cropped(dense, keep), level)


def assert_values(vol, dense, f, n, level, s, keep):
    """Every evaluated point holds the field's value, every other point the effective value of its coarse corner."""
    seen = f.calls.reshape(dense.shape) > 0
    assert np.array_equal(vol[seen], dense[seen])
    corner = np.arange(n) // s * s
    kept = np.zeros(n ** 3, dtype=bool).reshape(n, n, n)
    kept[tuple(slice(lo, hi) for lo, hi in (keep or [(0, n)] * 3))] = True
    effective = np.where(kept, dense, np.float32(0))[np.ix_(corner, corner, corner)]
    assert seen[np.ix_(corner, corner, corner)].all(), 'a coarse point was not evaluated'
    assert np.array_equal(vol[~seen], effective[~seen])


@pytest.mark.parametrize('s', [2, 4, 8, 16])
@pytest.mark.parametrize('keep', [None, SPHERE_KEEP], ids=['whole', 'crop'])
def test_rough_sphere_band_mesh_is_the_dense_mesh(s, keep):
    """47 cells: a partial last brick at every size.  One component, so the band mesh is the dense mesh byte for byte."""
    dense, level = field('rough_sphere')
    vol, report, f, band_mesh, dense_mesh = run_band(dense, level, s, keep)
    assert len(dense_mesh[0]) > 4000 and same_mesh(band_mesh, dense_mesh)
    if keep is None:
        assert (len(dense_mesh[0]), len(dense_mesh[1])) == (7012, 14020)
    if s in (4, 8):
        assert report['rounds'] >= 2 and report['new_bricks'][0] > 0 and report['new_bricks'][-1] == 0        # the growth rule did something
    assert 0 < report['seeds'] <= report['bricks'] == (-(-47 // s)) ** 3 and report['points'] < dense.size
    assert_values(vol, dense, f, 48, level, s, keep)


@pytest.mark.parametrize('s', [4, 8])
def test_four_balls_lose_exactly_the_smallest(s):
    dense, level = field('four_balls')
    vol, report, f, band_mesh, dense_mesh = run_band(dense, level, s)
    assert (len(dense_mesh[0]), len(dense_mesh[1])) == (4114, 8212) and (len(band_mesh[0]), len(band_mesh[1])) == (4088, 8164)
    verts, faces, lost, partly = restricted_dense(dense_mesh, band_mesh)
    assert lost == [(26, 48)] and partly == 0                  # the ball of radius 1.2, whole
    assert same_mesh(band_mesh, (verts, faces))
    assert_values(vol, dense, f, 48, level, s, None)


@pytest.mark.parametrize('s', [4, 8])
def test_filtered_noise_under_a_crop_keeps_whole_components(s):
    dense, level = field('noise')
    vol, report, f, band_mesh, dense_mesh = run_band(dense, level, s, NOISE_KEEP)
    verts, faces, lost, partly = restricted_dense(dense_mesh, band_mesh)
    assert partly == 0 and len(band_mesh[1]) > 1000
    assert same_mesh(band_mesh, (verts, faces))
    assert len(band_mesh[0]) + sum(v for v, _ in lost) == len(dense_mesh[0])
    assert_values(vol, dense, f, 43, level, s, NOISE_KEEP)


def test_values_equal_to_the_level_are_outside():
    dense, level = field('integer')
    assert (dense == level).sum() > 500
    vol, report, f, band_mesh, dense_mesh = run_band(dense, level, 4)
    assert len(dense_mesh[0]) > 500 and same_mesh(band_mesh, dense_mesh)
    assert_values(vol, dense, f, 30, level, 4, None)
    flat = np.full((10, 10, 10), level, dtype=np.float32)       # all ties: all outside, no seed
    vol, report, f, band_mesh, _ = run_band(flat, level, 4)
    assert report['seeds'] == 0 and report['rounds'] == 0 and len(band_mesh[0]) == 0


def test_a_single_brick():
    i = np.arange(6, dtype=np.float64)
    x, y, z = np.meshgrid(i, i, i, indexing='ij')
    dense = (1.7 - np.sqrt((x - 2.4) ** 2 + (y - 2.6) ** 2 + (z - 2.5) ** 2)).astype(np.float32)
    vol, report, f, band_mesh, dense_mesh = run_band(dense, 0.0, 8)              # n - 1 = 5 < s
    assert report['bricks'] == 1 and report['seeds'] == 0 and report['points'] == 8
    assert len(band_mesh[0]) == 0 and len(dense_mesh[0]) > 0           # a closed floater inside one brick: lost whole
    corner = dense.copy()
    corner[0, 0, 0] = 5                                          # one corner inside: the brick is seeded, and a brick is all or nothing
    vol, report, f, band_mesh, dense_mesh = run_band(corner, 0.0, 8)
    assert report['seeds'] == 1 and report['new_bricks'] == [0] and report['points'] == 6 ** 3 and same_mesh(band_mesh, dense_mesh)
    assert np.array_equal(vol, corner)


def test_all_outside_evaluates_the_coarse_points_only():
    dense = np.full((21, 21, 21), -3, dtype=np.float32)
    vol, report, f, band_mesh, _ = run_band(dense, 0.0, 4)
    assert report['seeds'] == 0 and report['new_bricks'] == [] and report['points'] == 6 ** 3 and len(band_mesh[0]) == 0 and len(band_mesh[1]) == 0
    assert np.array_equal(np.flatnonzero(f.calls), S.band_coarse_index(21, 4)) and np.array_equal(vol, dense)


@pytest.mark.parametrize('s', [4, 8])
def test_all_inside_under_a_crop_gives_the_walls(s):
    dense = np.full((23, 23, 23), 5, dtype=np.float32)
    keep = [(3, 20), (2, 18), (5, 21)]
    vol, report, f, band_mesh, dense_mesh = run_band(dense, 0.0, s, keep)
    assert len(dense_mesh[1]) > 1000 and same_mesh(band_mesh, dense_mesh)
    _, whole, _, none, _ = run_band(dense, 0.0, s)             # without the crop nothing crosses
    assert whole['seeds'] == 0 and len(none[0]) == 0


def test_empty_kept_range_is_all_outside():
    dense, level = field('rough_sphere')
    keep = S.band_keep_of_crop(48, [(0, 0), (5, 5), (5, 5)])   # python's vol[-0:] = 0 zeroes the whole axis
    assert keep == [(0, 0), (5, 43), (5, 43)]
    vol, report, f, band_mesh, dense_mesh = run_band(dense, level, 8, keep)
    assert report['seeds'] == 0 and len(band_mesh[0]) == 0 == len(dense_mesh[0])


def owners(index, state, n, s):
    """The lowest brick of state 2 that holds each listed point (written apart from the port: per axis the bricks i // s and, on a face, i // s - 1)."""
    nb = -(-(n - 1) // s)
    coords = np.stack(np.unravel_index(index.astype(np.int64), (n, n, n)), axis=1)
    best = np.full(len(index), nb ** 3, dtype=np.int64)
    for d in np.ndindex(2, 2, 2):
        q = coords // s - np.array(d)
        ok = ((np.array(d) == 0) | (coords % s == 0)).all(1) & (q >= 0).all(1) & (q < nb).all(1)
        lin = (q[:, 0] * nb + q[:, 1]) * nb + q[:, 2]
        ok &= np.asarray(state)[np.where(ok, lin, 0)] == 2
        best = np.where(ok & (lin < best), lin, best)
    assert (best < nb ** 3).all()
    return best


def test_lists_are_brick_major_and_stages_compose():
    """The stages one by one, as the GPU route calls them: the lists hold new points only, brick by brick, and the driver's result is theirs."""
    dense, level = field('rough_sphere')
    n, s = 48, 8
    f = CountingField(dense)
    trace = []
    vol, report = S.band_volume_numpy(f, n, level, s, SPHERE_KEEP, trace=trace)
    assert len(trace) == report['rounds'] == 2
    state0, seeds = S.band_seed_numpy(dense, n, level, s, SPHERE_KEEP)
    assert seeds == report['seeds'] and set(np.unique(state0)) <= {0, 2}
    index = S.band_points_numpy(state0, n, s)
    assert index.dtype == np.int32 and np.array_equal(index, trace[0][1]) and len(np.unique(index)) == len(index)
    # the set: every point of a seeded brick that is not coarse (what band_fill_numpy leaves alone, with every value its own index)
    marks = np.arange(n ** 3, dtype=np.float32)
    filled = S.band_fill_numpy(marks.copy(), n, s, state0) != marks
    expected = np.setdiff1d(np.flatnonzero(~filled), S.band_coarse_index(n, s))
    assert np.array_equal(np.sort(index), expected)
    # the order: by owner -- the lowest new brick that holds the point --, then row-major within it (ascending index: axis 2 is the fastest)
    owner = owners(index, state0, n, s)
    assert (np.diff(owner) >= 0).all() and (np.diff(index.astype(np.int64))[np.diff(owner) == 0] > 0).all()
    assert len(np.unique(owner)) > 50
    assert not np.isin(index, S.band_coarse_index(n, s)).any()
    state1, new = S.band_grow_numpy(dense, n, level, s, state0, SPHERE_KEEP)
    assert new == report['new_bricks'][0] and np.array_equal(state1, trace[0][0]) and set(np.unique(state1)) <= {0, 1, 2}
    second = S.band_points_numpy(state1, n, s)
    assert np.array_equal(second, trace[1][1]) and not np.isin(second, index).any()
    with pytest.raises(ValueError):
        S.band_volume_numpy(f, n, level, 3)
    with pytest.raises(ValueError):
        S.band_volume_numpy(f, 1, level, 4)


def test_voxel_samples_takes_an_index_tensor():
    import gen_videos_mi355x as gv
    n = 37
    every = gv.voxel_samples(0, n ** 3, n, 1.0, 'cpu')
    index = torch.from_numpy(np.random.default_rng(0).integers(0, n ** 3, 500)).to(torch.int32)
    assert torch.equal(gv.voxel_samples(index, None, n, 1.0, 'cpu'), every[:, index.long()])
    assert gv.crop_ranges(512) == [(60, 60), (60, 76), (60, 60)]


@pytest.fixture(scope='module')
def generator_volume():
    """test_density_volume_gpu_vs_cpu's generator on the CPU: the dense volume at resolution 40 and its planes, made once."""
    import gnerf_generator
    import gen_videos_mi355x as gv
    torch.manual_seed(5)
    G = gnerf_generator.Generator().eval().requires_grad_(False)
    with torch.no_grad():
        ws = G.mapping(torch.randn(1, 512), torch.zeros(1, 25))
        dense, planes = gv.extract_density_grid(G, ws, resolution=40, crop=True, return_planes=True)
    return G, ws, dense, planes


def test_extract_density_grid_band_on_the_cpu(generator_volume):
    """The CPU path end to end: query_sigma_lattice composes voxel_samples at the indices with query_sigma, so the evaluated points hold the
    dense volume's bits and the band mesh is the dense mesh restricted to whole components."""
    import gen_videos_mi355x as gv
    G, ws, dense, planes = generator_volume
    level = float(dense[4:-4, 4:-5, 4:-4].median())
    reports = {}
    band = gv.extract_density_grid(G, ws, resolution=40, crop=True, planes=planes, band=4, level=level, report=reports)
    r = reports['band']
    assert band.shape == dense.shape and 0 < r['points'] < 40 ** 3 and r['seeds'] > 0
    with pytest.raises(ValueError, match='level'):
        gv.extract_density_grid(G, ws, resolution=40, planes=planes, band=4)
    mesh, _ = gv.mesh_of_density_grid(band, level, band=r)
    dense_mesh, _ = gv.mesh_of_density_grid(dense, level)
    assert list(mesh.reports) == ['band'] and mesh.reports['band'] is r and list(dense_mesh.reports) == []
    verts, faces, lost, partly = restricted_dense((dense_mesh.verts, dense_mesh.faces), (mesh.verts, mesh.faces))
    assert partly == 0 and len(mesh.faces) > 1000 and same_mesh((mesh.verts, mesh.faces), (verts, faces))
    assert 'bricks of 4^3 cells' in S.band_report_line(r) and str(r['points']) in S.band_report_line(r)


def test_cli_flag_and_native_declarations():
    import gen_videos_mi355x as gv
    import gnerf_hip
    ap = gv.arg_parser()
    assert ap.parse_args([]).mesh_band == 0 and ap.parse_args(['--mesh-band', '8']).mesh_band == 8
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    assert int(re.search(r'#define GNERF_ABI_VERSION (\d+)', header).group(1)) == gnerf_hip.ABI_VERSION == 15
    names = ('gnerf_query_lattice', 'gnerf_band_workspace_bytes', 'gnerf_band_seed', 'gnerf_band_points_count', 'gnerf_band_points_emit', 'gnerf_band_grow',
             'gnerf_band_fill')
    lib = gnerf_hip.load()
    for name in names:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header) and hasattr(lib, name)
        assert name in gnerf_hip.SIGNATURES and name in gnerf_hip.OPTIONAL_SYMBOLS       # a library of the same version built before them still loads
    assert gnerf_hip.band_available() and gnerf_hip.query_lattice_available() and gnerf_hip.BAND_BRICKS == S.BAND_BRICKS == (2, 4, 8, 16)
    e = gnerf_hip.ext()
    if e is not None:
        for name in ('query_lattice', 'band_seed', 'band_points_count', 'band_points_emit', 'band_grow', 'band_fill'):
            assert hasattr(e, name)
    units = open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'compile_unit.sh')).read()
    assert re.search(r'^UNITS=.*\bmesh_band\b', units, re.M) and re.search(r'^UNITS=.*\bquery_lattice\b', units, re.M)
    assert '#include "query_lattice.inl"' in open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'query_lattice.hip')).read()
    nbytes = gnerf_hip.band_workspace_bytes(512, 8)
    assert 12 * 64 ** 3 <= nbytes < 13 * 64 ** 3
    with pytest.raises(gnerf_hip.NativeError):
        gnerf_hip.band_workspace_bytes(512, 3)
