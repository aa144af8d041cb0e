"""CPU tests of the brick-wise band mesh: the numpy port (shape_mi355x.band_marching_cubes_numpy, band_mesh) against the existing route --
marching_cubes_numpy of band_volume_numpy's volume after the crop, the flips and the transpose -- same bytes, dtypes and shapes, across fields,
brick edges and views; that unvisited memory is never read (poison); the non-finite count; empty cases; refused arguments; the declarations."""

import os
import re

import numpy as np
import pytest

import shape_mi355x as S
from band_mesh_cases import BRICKS, FIELDS, VIEWS, band_run, case_field, existing_mesh, poisoned
from mesh_band_cases import same_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def port(run, s, view, volume=None, **kw):
    perm, flip = VIEWS[view]
    return S.band_marching_cubes_numpy(run['raw'] if volume is None else volume, run['state'], run['n'], s, run['level'], run['keep'], perm, flip, **kw)


@pytest.mark.parametrize('view', list(VIEWS))
@pytest.mark.parametrize('s', BRICKS)
@pytest.mark.parametrize('name', list(FIELDS))
def test_port_is_the_existing_route(name, s, view):
    run = band_run(name, s)
    want = existing_mesh(name, s, view)
    verts, faces, counts = port(run, s, view, return_counts=True)
    assert same_mesh((verts, faces), want)
    assert counts.dtype == np.int64 and list(counts) == [len(want[0]), len(want[1]), 0, int(run['visited'].sum())]
    if name != 'four_balls':                                            # (some of the balls are thinner than the large bricks: fewer faces, still a mesh)
        assert len(faces) > 0


@pytest.mark.parametrize('name', ['rough_sphere', 'noise', 'cut_ball'])
def test_port_without_the_crop(name):
    for s in (2, 8):
        run = band_run(name, s, False)
        assert run['keep'] is None
        for view in VIEWS:
            assert same_mesh(port(run, s, view), existing_mesh(name, s, view, False))


def test_band_mesh_runs_the_rounds_without_the_fill():
    dense, level = case_field('noise')
    n, keep = dense.shape[0], FIELDS['noise']
    flat = dense.reshape(-1)
    asked = np.zeros(n ** 3, dtype=np.int64)

    def host_field(index, out):
        np.add.at(asked, index, 1)
        out[index] = flat[index]

    perm, flip = VIEWS['pipeline']
    verts, faces, report = S.band_mesh(host_field, n, level, 4, keep, perm, flip)
    run = band_run('noise', 4)
    assert same_mesh((verts, faces), existing_mesh('noise', 4, 'pipeline'))
    assert asked.max() == 1 and int(asked.sum()) == report['points'] == run['report']['points']
    assert {k: report[k] for k in run['report']} == run['report']
    assert report['active'] == int((run['state'] == 1).sum()) and report['visited'] == int(run['visited'].sum()) and report['mesh'] == (len(verts), len(faces))
    # band_volume / band_volume_numpy themselves still fill: what they return is what they returned
    filled, _ = S.band_volume_numpy(lambda index, out: out.__setitem__(index, flat[index]), n, level, 4, keep)
    assert not np.array_equal(filled.reshape(-1), run['raw']) and np.array_equal(filled[run['visited']], dense[run['visited']])


@pytest.mark.parametrize('name,s', [('rough_sphere', 2), ('rough_sphere', 4), ('four_balls', 2), ('integer', 2), ('integer', 4), ('four_balls', 4), ('cut_ball', 2)])
def test_unvisited_memory_is_never_read(name, s):
    run = band_run(name, s)
    assert run['visited'].mean() < 0.5                                   # or the poison shows nothing
    for view in VIEWS:
        want = existing_mesh(name, s, view)
        for value in (np.nan, 1e30, -1e30):
            verts, faces, counts = port(run, s, view, volume=poisoned(run, np.float32(value)), return_counts=True)
            assert same_mesh((verts, faces), want) and counts[2] == 0


def test_non_finite_values_count_only_where_they_are_seen():
    run = band_run('rough_sphere', 4)
    n, keep = run['n'], run['keep']
    i = np.arange(n)
    kept = S._band_kept(keep, i[:, None, None], i[None, :, None], i[None, None, :])
    inside = np.argwhere(run['visited'] & kept)
    outside = np.argwhere(run['visited'] & ~kept)
    assert len(inside) and len(outside)
    want = existing_mesh('rough_sphere', 4, 'pipeline')
    for value in (np.nan, np.inf):
        vol = np.array(run['raw']).reshape(n, n, n)
        vol[tuple(outside[len(outside) // 2])] = value                   # visited but cropped away: its effective value is 0
        verts, faces, counts = port(run, 4, 'pipeline', volume=vol.reshape(-1), return_counts=True)
        assert counts[2] == 0 and same_mesh((verts, faces), want)
        vol[tuple(inside[len(inside) // 2])] = value
        vol[tuple(inside[0])] = value
        verts, faces, counts = port(run, 4, 'pipeline', volume=vol.reshape(-1), return_counts=True)
        assert counts[2] == 2 and verts.shape == (0, 3) and faces.shape == (0, 3)      # counted, and nothing is emitted
        with pytest.raises(ValueError, match='non-finite'):
            port(run, 4, 'pipeline', volume=vol.reshape(-1))


def test_band_mesh_raises_on_a_non_finite_value_it_sees():
    """Like the route it replaces (band_volume, the crop, marching_cubes): a NaN or Inf at a visited, kept point is an error, not an empty mesh."""
    run = band_run('rough_sphere', 4)
    n, level, keep = run['n'], run['level'], run['keep']
    i = np.arange(n)
    kept = S._band_kept(keep, i[:, None, None], i[None, :, None], i[None, None, :])
    coarse = np.zeros((n, n, n), dtype=bool)
    coarse.reshape(-1)[S.band_coarse_index(n, 4)] = True
    inside = np.argwhere(run['visited'] & kept & ~coarse)                 # (not a coarse point: the seeds stay as they are)
    outside = np.argwhere(run['visited'] & ~kept)
    perm, flip = VIEWS['pipeline']
    for value in (np.nan, np.inf):
        flat = np.array(run['dense']).reshape(-1)
        flat[np.ravel_multi_index(tuple(outside[len(outside) // 2]), (n, n, n))] = value      # cropped away: its effective value is 0

        def host_field(index, out):
            out[index] = flat[index]

        verts, faces, report = S.band_mesh(host_field, n, level, 4, keep, perm, flip)
        assert same_mesh((verts, faces), existing_mesh('rough_sphere', 4, 'pipeline'))
        flat[np.ravel_multi_index(tuple(inside[len(inside) // 2]), (n, n, n))] = value
        with pytest.raises(ValueError, match='non-finite'):
            S.band_mesh(host_field, n, level, 4, keep, perm, flip)


def test_empty_cases():
    dense, level = case_field('rough_sphere')
    n = dense.shape[0]
    flat = dense.reshape(-1)

    def host_field(index, out):
        out[index] = flat[index]

    above = float(dense.max()) + 1                                       # no seeds: no brick is active
    whole_axis = S.band_keep_of_crop(n, [(3, 3), (4, 0), (3, 3)])        # b = 0 zeroes a whole axis
    assert whole_axis[1] == (0, 0)
    for lev, keep in ((above, None), (level, whole_axis)):
        for perm, flip in VIEWS.values():
            verts, faces, report = S.band_mesh(host_field, n, lev, 4, keep, perm, flip)
            assert verts.shape == (0, 3) and verts.dtype == np.float32 and faces.shape == (0, 3) and faces.dtype == np.int32
            assert report['active'] == 0 and report['visited'] == 0 and report['mesh'] == (0, 0) and report['seeds'] == 0
    nb = -(-(n - 1) // 4)
    verts, faces = S.band_marching_cubes_numpy(np.zeros(n ** 3, dtype=np.float32), np.zeros(nb ** 3, dtype=np.uint8), n, 4, 0.0)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)


def test_bad_arguments_are_refused():
    run = band_run('integer', 4)
    n, raw, state, level = run['n'], run['raw'], run['state'], run['level']
    with pytest.raises(ValueError, match='brick edge'):
        S.band_marching_cubes_numpy(raw, state, n, 3, level)
    with pytest.raises(ValueError, match='brick edge'):
        S.band_marching_cubes_numpy(raw, state, n, 32, level)
    for perm in ((0, 1, 1), (0, 1, 3), (1, 2), (0, 0, 0)):
        with pytest.raises(ValueError, match='permutation'):
            S.band_marching_cubes_numpy(raw, state, n, 4, level, perm=perm)
    for value in (2, 3):
        bad = np.array(state)
        bad[len(bad) // 2] = value
        with pytest.raises(ValueError, match='0 or 1'):
            S.band_marching_cubes_numpy(raw, bad, n, 4, level)
    with pytest.raises(ValueError, match='n\\^3'):
        S.band_marching_cubes_numpy(raw[:-1], state, n, 4, level)
    with pytest.raises(ValueError, match='nb\\^3'):
        S.band_marching_cubes_numpy(raw, state[:-1], n, 4, level)
    with pytest.raises(ValueError):
        S.band_marching_cubes_numpy(raw, state, 1, 4, level)


def test_declarations():
    import gnerf_hip
    from gnerf_hip import _native
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    names = ('gnerf_band_mesh_workspace_bytes', 'gnerf_band_mesh_count', 'gnerf_band_mesh_emit')
    for name in names:
        assert re.search(r'^int ' + name + r'\(', header, re.M), name
        assert name in _native.SIGNATURES and name in _native.OPTIONAL_SYMBOLS
    assert re.search(r'^#define GNERF_ABI_VERSION 15$', header, re.M) and gnerf_hip.ABI_VERSION == 15
    assert callable(gnerf_hip.band_marching_cubes) and callable(gnerf_hip.band_mesh_available)
    units = open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'compile_unit.sh')).read()
    assert 'mesh_band_cubes' in units and os.path.isfile(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'mesh_band_cubes.hip'))
    import gen_videos_mi355x as gv
    args = gv.arg_parser().parse_args(['--random-init', '--mesh-band', '4', '--mesh-direct'])
    assert args.mesh_direct and not gv.arg_parser().parse_args(['--random-init']).mesh_direct
