"""CPU tests of the mesh cleaning (shape_mi355x.mesh_components_numpy / mesh_select / mesh_compact_numpy / mesh_smooth_numpy / clean_mesh,
the numpy ports of csrc/mesh_clean.hip): components against scipy, the selection's order and ties, the compaction's order and gathers, the
smoothing's invariants and a float64 restatement, the CLI flags, and the declarations of the native layer."""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage
import scipy.sparse
import scipy.sparse.csgraph
import torch

import shape_mi355x as S
from test_mesh_cpu import area_volume, assert_closed_oriented, euler, sphere_field, zero_border

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- meshes (made once, never changed)
def random_mesh(shape, level, seed=0, border=True):
    vol = np.random.default_rng(seed).random(shape).astype(np.float32)
    return S.marching_cubes_numpy(zero_border(vol) if border else vol, level)


def ball(n, centre, r):
    i = np.arange(n, dtype=np.float64)
    x, y, z = np.meshgrid(i, i, i, indexing='ij')
    return (r - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(np.float32)


def four_balls_field():
    """A "head plus floaters": balls of radius 14, 4, 2.5 and 1.2 in a 48^3 volume, far enough apart to stay four surfaces."""
    return np.maximum.reduce([ball(48, (24, 24, 20), 14), ball(48, (39.5, 39.5, 39.5), 4), ball(48, (6.3, 40.2, 8.1), 2.5), ball(48, (41.1, 5.2, 42.3), 1.2)])


def rough_sphere_field():
    noise = np.random.default_rng(5).standard_normal((48, 48, 48)) * 2.5
    return (sphere_field(48, 18) + scipy.ndimage.uniform_filter(noise, 3)).astype(np.float32)


def largest_component(verts, faces):
    c = S.clean_mesh(verts, faces, keep_largest=1)
    return c.verts, c.faces


def grid_mesh(n=9):
    """An n x n flat grid of integer coordinates, every square split along the same diagonal."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    verts = np.stack([i, j, np.zeros_like(i)], axis=-1).reshape(-1, 3).astype(np.float32)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([a, a + n, a + n + 1], axis=1), np.stack([a, a + n + 1, a + 1], axis=1)]).astype(np.int32)
    return verts, faces


@pytest.fixture(scope='module')
def meshes():
    made = {'random': random_mesh((33, 34, 35), 0.5), 'balls': S.marching_cubes_numpy(four_balls_field(), 0.0)}
    made['rough'] = largest_component(*S.marching_cubes_numpy(rough_sphere_field(), 0.0))
    for v, f in made.values():
        v.setflags(write=False)
        f.setflags(write=False)
    return made


def scipy_components(faces, n_verts):
    """(label, faces_of, counts) from scipy.sparse.csgraph.connected_components, relabelled to the smallest index per component."""
    f = np.asarray(faces, dtype=np.int64)
    i, j = np.concatenate([f[:, 0], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2]])
    graph = scipy.sparse.coo_matrix((np.ones(len(i), dtype=np.int8), (i, j)), shape=(n_verts, n_verts))
    n, comp = scipy.sparse.csgraph.connected_components(graph, directed=False)
    first = np.full(n, n_verts, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(n_verts))
    label = first[comp]
    used = np.zeros(n_verts, dtype=bool)
    used[f.reshape(-1)] = True
    faces_of = np.bincount(label[f[:, 0]], minlength=n_verts)
    return label, faces_of, np.array([len(np.unique(label[used])), n_verts - used.sum(), 0])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- components
@pytest.mark.parametrize('name', ['random', 'balls'])
def test_components_match_scipy(meshes, name):
    verts, faces = meshes[name]
    label, faces_of, counts = S.mesh_components_numpy(faces, len(verts))
    ref_label, ref_faces_of, ref_counts = scipy_components(faces, len(verts))
    print(f'{name}: {counts[0]} components, {len(verts)} vertices, {len(faces)} faces; largest: {np.sort(faces_of)[::-1][:4]}')
    assert label.dtype == np.int32 and faces_of.dtype == np.int32 and counts.dtype == np.int64
    assert np.array_equal(label, ref_label) and np.array_equal(faces_of, ref_faces_of) and np.array_equal(counts, ref_counts)
    assert np.all(label <= np.arange(len(verts))) and np.array_equal(label[label], label)
    assert faces_of.sum() == len(faces) and counts[1] == 0
    if name == 'balls':
        assert counts[0] == 4 and np.sort(faces_of[faces_of > 0])[::-1].tolist() == [7304, 620, 240, 48]
    else:                                                                # (pins the fixture: seed 0 of default_rng)
        assert (counts[0], len(verts), len(faces)) == (376, 50710, 106652)
    # the same for every order of the faces and every rotation of their ids
    rng = np.random.default_rng(3)
    shuffled = np.roll(faces[rng.permutation(len(faces))], 1, axis=1)
    again = S.mesh_components_numpy(shuffled, len(verts))
    assert np.array_equal(again[0], label) and np.array_equal(again[2], counts) and again[1].sum() == len(faces)


def test_components_of_degenerate_and_empty_meshes():
    tet = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)
    # vertices 0-3 and 5-8: two tetrahedra; 4: in no face; 9, 10: joined by a face (9, 9, 10)
    faces = np.concatenate([tet + 5, tet, np.array([[9, 9, 10]], dtype=np.int32)])
    label, faces_of, counts = S.mesh_components_numpy(faces, 11)
    assert label.tolist() == [0, 0, 0, 0, 4, 5, 5, 5, 5, 9, 9]
    assert faces_of.tolist() == [4, 0, 0, 0, 0, 4, 0, 0, 0, 1, 0] and counts.tolist() == [3, 1, 0]
    label, faces_of, counts = S.mesh_components_numpy(np.zeros((0, 3), np.int32), 3)
    assert label.tolist() == [0, 1, 2] and faces_of.tolist() == [0, 0, 0] and counts.tolist() == [0, 3, 0]
    label, faces_of, counts = S.mesh_components_numpy(np.zeros((0, 3), np.int32), 0)
    assert label.shape == (0,) and faces_of.shape == (0,) and counts.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match='outside'):
        S.mesh_components_numpy(np.array([[0, 1, 3]], np.int32), 3)
    with pytest.raises(ValueError, match='outside'):
        S.mesh_components_numpy(np.array([[0, -1, 2]], np.int32), 3)
    label, faces_of, counts = S.mesh_components_numpy(np.array([[0, 1, 3], [1, 2, 1]], np.int32), 3, check=False)
    assert label.tolist() == [0, 1, 1] and faces_of.tolist() == [0, 1, 0] and counts.tolist() == [1, 1, 1]


# ---------------------------------------------------------------------------------------------------------------- selection
def tie_mesh():
    """copy A of a small closed mesh, a sphere, copies B and C: three components of one size behind a larger one."""
    small = S.marching_cubes_numpy(sphere_field(8, 2.0), 0.0)
    big = S.marching_cubes_numpy(sphere_field(20, 7.0), 0.0)
    parts = [(small[0], small[1]), (big[0] + np.float32(20), big[1]), (small[0] + np.float32(50), small[1]), (small[0] + np.float32(70), small[1])]
    verts, faces, base = [], [], 0
    for v, f in parts:
        verts.append(v)
        faces.append(f + base)
        base += len(v)
    return np.concatenate(verts), np.concatenate(faces).astype(np.int32), [len(v) for v, _ in parts], [len(f) for _, f in parts]


def test_selection_orders_by_size_then_label_and_breaks_ties_by_label():
    verts, faces, nv, nf = tie_mesh()
    assert nf[1] > nf[0] == nf[2] == nf[3] > 0
    label, faces_of, counts = S.mesh_components_numpy(faces, len(verts))
    starts = np.cumsum([0] + nv[:-1])
    assert counts.tolist() == [4, 0, 0] and np.nonzero(faces_of)[0].tolist() == starts.tolist()
    assert S.mesh_select(faces_of).tolist() == [starts[1], starts[0], starts[2], starts[3]]
    assert S.mesh_select(faces_of, keep_largest=2).tolist() == [starts[1], starts[0]]          # the tie at the cut goes to the lower label
    assert S.mesh_select(faces_of, keep_largest=9).tolist() == [starts[1], starts[0], starts[2], starts[3]]
    assert S.mesh_select(faces_of, min_faces=nf[0] + 1).tolist() == [starts[1]]                # min_faces alone selects
    assert S.mesh_select(faces_of, min_faces=nf[0]).tolist() == [starts[1], starts[0], starts[2], starts[3]]
    assert S.mesh_select(faces_of, keep_largest=3, min_faces=nf[1] + 1).tolist() == []
    # the sparse form a GPU caller uses: the labels and their face counts only
    assert S.mesh_select(faces_of[starts], keep_largest=2, labels=starts).tolist() == [starts[1], starts[0]]
    with pytest.raises(ValueError):
        S.mesh_select(faces_of, keep_largest=-1)
    c = S.clean_mesh(verts, faces, keep_largest=2)
    assert c.src_vertex.tolist() == list(range(0, nv[0] + nv[1]))
    assert c.report == dict(components=4, kept=2, faces=sum(nf), kept_faces=nf[0] + nf[1], share=(nf[0] + nf[1]) / sum(nf), vertices=sum(nv), kept_vertices=nv[0] + nv[1])
    assert same_bits(c.verts, verts[:nv[0] + nv[1]]) and np.array_equal(c.faces, faces[:nf[0] + nf[1]])


def test_keep_largest_of_the_four_balls_is_one_closed_surface(meshes):
    verts, faces = meshes['balls']
    c = S.clean_mesh(verts, faces, keep_largest=1)
    _, faces_of, _ = S.mesh_components_numpy(faces, len(verts))
    assert c.report['components'] == 4 and c.report['kept'] == 1 and len(c.faces) == faces_of.max() == c.report['kept_faces']
    assert euler(c.verts, c.faces) == 2
    assert S.mesh_components_numpy(c.faces, len(c.verts))[2].tolist() == [1, 0, 0]
    by_size = S.clean_mesh(verts, faces, min_faces=int(np.sort(faces_of)[-2]))
    assert by_size.report['kept'] == 2 and euler(by_size.verts, by_size.faces) == 4


# ---------------------------------------------------------------------------------------------------------------- compaction
def test_compaction_is_stable_and_gathers(meshes):
    verts, faces = meshes['random']
    rng = np.random.default_rng(11)
    normals = rng.standard_normal((len(verts), 3)).astype(np.float32)
    colors = rng.integers(0, 256, (len(verts), 3), dtype=np.uint8)
    label, faces_of, _ = S.mesh_components_numpy(faces, len(verts))
    c = S.clean_mesh(verts, faces, keep_largest=3, normals=normals, colors=colors)
    kept = S.mesh_select(faces_of, keep_largest=3)
    vkeep, fkeep = np.isin(label, kept), np.isin(label[faces[:, 0]], kept)
    assert 0 < len(c.verts) < len(verts) and c.report['kept'] == 3
    assert np.all(np.diff(c.src_vertex) > 0) and np.array_equal(c.src_vertex, np.nonzero(vkeep)[0]) and c.src_vertex.dtype == np.int32
    assert same_bits(c.verts, verts[vkeep]) and same_bits(c.normals, normals[c.src_vertex]) and same_bits(c.colors, colors[c.src_vertex])
    assert c.faces.dtype == np.int32 and np.array_equal(c.src_vertex[c.faces], faces[fkeep])         # kept faces, in order, remapped
    assert_closed_oriented(c.faces)


def test_compaction_identity_unused_vertices_and_bad_faces(meshes):
    verts, faces = meshes['random']
    c = S.clean_mesh(verts, faces)
    assert same_bits(c.verts, verts) and same_bits(c.faces, faces) and np.array_equal(c.src_vertex, np.arange(len(verts)))
    assert c.report['share'] == 1.0 and c.report['kept'] == c.report['components']
    # unused vertices are dropped, wherever they sit, even when their label is marked as kept
    v, f = meshes['balls']
    extra = np.concatenate([np.full((2, 3), -1, np.float32), v, np.full((3, 3), -2, np.float32)])
    c = S.clean_mesh(extra, f + 2)
    assert same_bits(c.verts, v) and np.array_equal(c.faces, f) and np.array_equal(c.src_vertex, np.arange(len(v)) + 2)
    label, faces_of, counts = S.mesh_components_numpy(f + 2, len(extra))
    assert counts.tolist() == [4, 5, 0]
    all_kept = S.mesh_compact_numpy(extra, f + 2, label, faces_of, np.ones(len(extra), np.uint8))
    assert same_bits(all_kept[0], v) and np.array_equal(all_kept[1], f)
    none = S.mesh_compact_numpy(extra, f + 2, label, faces_of, np.zeros(len(extra), bool))
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3) and none[2].shape == (0,)
    bad = f.copy()
    bad[7, 1] = len(v)
    with pytest.raises(ValueError, match='outside'):
        S.clean_mesh(v, bad)
    empty = S.clean_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), keep_largest=1, smooth=2)
    assert empty.verts.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.report['components'] == 0 and empty.report['share'] == 1.0


def test_cpu_tensors_take_the_ports(meshes):
    verts, faces = meshes['balls']
    a = S.clean_mesh(verts, faces, keep_largest=2, smooth=1)
    b = S.clean_mesh(torch.from_numpy(verts.copy()), torch.from_numpy(faces.copy()), keep_largest=2, smooth=1)
    assert isinstance(b.verts, np.ndarray) and same_bits(a.verts, b.verts) and same_bits(a.faces, b.faces) and a.report == b.report


# ---------------------------------------------------------------------------------------------------------------- smoothing
def test_smoothing_that_does_nothing_returns_the_input_bits(meshes):
    verts, faces = meshes['rough']
    assert same_bits(S.mesh_smooth_numpy(verts, faces, 0), verts)
    assert same_bits(S.mesh_smooth_numpy(verts, faces, 3, lam=0.0, mu=0.0), verts)
    with pytest.raises(ValueError):
        S.mesh_smooth_numpy(verts, faces, -1)
    lone = np.array([[1, 2, 3], [4, 5, 6]], np.float32)                       # vertices in no face never move
    assert same_bits(S.mesh_smooth_numpy(lone, np.zeros((0, 3), np.int32), 2), lone)


def test_flat_grid_stays_put_with_its_border_pinned():
    verts, faces = grid_mesh(9)
    _, deg, _, odd = S._mesh_rows(faces, len(verts))
    assert odd.sum() == 32 and deg.min() > 0
    assert same_bits(S.mesh_smooth_numpy(verts, faces, 4), verts)
    free = S.mesh_smooth_numpy(verts, faces, 4, pin_boundary=False)
    moved = np.any(free != verts, axis=1)
    assert moved.any() and np.all(free[:, 2] == 0)
    assert moved[odd].any()                                                 # it is the border that gives way


def test_smoothing_does_not_depend_on_the_order_or_rotation_of_the_faces(meshes):
    rng = np.random.default_rng(2)
    for name, pin in (('rough', True), ('random', True), ('rough', False)):
        verts, faces = meshes[name]
        shuffled = faces[rng.permutation(len(faces))]
        turn = rng.integers(0, 3, len(faces))
        shuffled = np.stack([shuffled[np.arange(len(faces)), (turn + k) % 3] for k in range(3)], axis=1)
        assert same_bits(S.mesh_smooth_numpy(verts, faces, 2, pin_boundary=pin), S.mesh_smooth_numpy(verts, shuffled, 2, pin_boundary=pin))


def test_half_step_matches_a_float64_restatement(meshes):
    """Both sides round a float64 value to float32 once; the two float64 values differ only by the order of a short sum (relative 1e-16, far
    below half a float32 ulp), so the results differ by at most one float32 ulp per coordinate -- and in practice nowhere."""
    verts, faces = meshes['rough']
    f = faces.astype(np.int64)
    i = np.concatenate([f[:, 0], f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2]])
    j = np.concatenate([f[:, 1], f[:, 2], f[:, 2], f[:, 0], f[:, 0], f[:, 1]])
    A = scipy.sparse.coo_matrix((np.ones(len(i)), (i, j)), shape=(len(verts), len(verts))).tocsr()      # multiplicities add up
    m = np.asarray(A.sum(axis=1)).reshape(-1, 1)
    v64 = verts.astype(np.float64)
    want = (v64 + np.float64(np.float32(0.5)) * (A @ v64 / m - v64)).astype(np.float32)
    got = S.mesh_smooth_numpy(verts, faces, 1, lam=0.5, mu=0.0, pin_boundary=False)      # the half-step with mu = 0 moves nothing
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print(f'half-step against the float64 restatement: {np.count_nonzero(ulps)} of {ulps.size} coordinates differ, at most {ulps.max()} ulp')
    assert np.all(verts > 0) and ulps.max() <= 1
    assert np.any(got != verts)


def test_taubin_smooths_the_rough_sphere_without_shrinking_it(meshes):
    verts, faces = meshes['rough']
    print(f'rough sphere: {len(verts)} vertices, {len(faces)} faces')
    assert euler(verts, faces) == 2

    def measure(v):
        area, volume = area_volume(v, faces)
        radius = np.linalg.norm(v.astype(np.float64) - 23.5, axis=1)
        return area, volume, radius.std()
    a0, v0, s0 = measure(verts)
    a1, v1, s1 = measure(S.mesh_smooth_numpy(verts, faces, 10, lam=0.5, mu=-0.53))
    a2, v2, s2 = measure(S.mesh_smooth_numpy(verts, faces, 10, lam=0.5, mu=0.5))            # twenty plain Laplacian half-steps
    print(f'area {a0:.1f} -> {a1:.1f}, radius deviation {s0:.4f} -> {s1:.4f}, volume {100 * (v1 / v0 - 1):+.3f} % (Taubin) against '
          f'{100 * (v2 / v0 - 1):+.3f} % (plain)')
    assert a1 < a0 and s1 < s0
    assert abs(v1 - v0) < abs(v2 - v0)


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_flags_at_zero_write_the_same_bytes_and_cleaning_matches_the_ports(tmp_path, capsys):
    vol = four_balls_field() + 10.0                           # the surfaces sit at level 10, the CLI's default
    mrc = str(tmp_path / 'shape.mrc')
    ply = str(tmp_path / 'shape.ply')
    S.write_mrc(mrc, vol)
    assert S.main([mrc, '--device', 'cpu']) == 0
    plain = open(ply, 'rb').read()
    assert 'mesh cleaning' not in capsys.readouterr().out
    assert S.main([mrc, '--device', 'cpu', '--mesh-keep', '0', '--mesh-min-faces', '0', '--mesh-smooth', '0']) == 0
    assert open(ply, 'rb').read() == plain
    assert S.main([mrc, '--device', 'cpu', '--mesh-keep', '1', '--mesh-smooth', '2']) == 0
    out = capsys.readouterr().out
    assert 'mesh cleaning: kept 1 of 4 component(s)' in out and '2 Taubin iteration(s)' in out
    verts, faces = S.read_ply(ply)
    mv, mf = S.marching_cubes_numpy(np.ascontiguousarray(S.read_mrc(mrc).transpose(2, 1, 0)), 10.0)
    label, faces_of, _ = S.mesh_components_numpy(mf, len(mv))
    keep = np.zeros(len(mv), np.uint8)
    keep[S.mesh_select(faces_of, keep_largest=1)] = 1
    cv, cf, _ = S.mesh_compact_numpy(mv, mf, label, faces_of, keep)
    assert same_bits(verts, S.mesh_smooth_numpy(cv, cf, 2)) and np.array_equal(faces, cf) and 0 < len(cf) < len(mf)
    assert S.main([mrc, '--device', 'cpu', '--mesh-min-faces', '100']) == 0
    assert 'kept 3 of 4' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        S.main([mrc, '--device', 'cpu', '--mesh-smooth', '-1'])


def run_gen_videos(tmp_path, tag, *extra):
    """Start gen_videos_mi355x.py on the CPU device at a 32^3 volume -> (process, volume path, ply path)."""
    npy, ply = str(tmp_path / f'{tag}.npy'), str(tmp_path / f'{tag}.ply')
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.join(ROOT, 'g-nerf_amd'), ROOT, env.get('PYTHONPATH', '')])
    cmd = [sys.executable, os.path.join(ROOT, 'g-nerf_amd', 'gen_videos_mi355x.py'), '--random-init', '--device', 'cpu', '--frames', '2', '--res', '16',
           '--no-double-depth', '--voxel-res', '32', '--shapes', npy, '--mesh', ply, '--mesh-level', '0', *extra]
    return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env), npy, ply


def test_gen_videos_cli_on_the_cpu_device(tmp_path):
    """The CLI itself, four processes side by side: without the flags, with the three at 0, with --mesh-keep 1 --mesh-smooth 2 (and
    --geometry-out, which the flags apply to as well), and with a negative flag."""
    import gen_videos_mi355x as gv
    import gnerf_harness as H
    geo = str(tmp_path / 'geo.npy')
    runs = {'plain': run_gen_videos(tmp_path, 'plain'),
            'zeros': run_gen_videos(tmp_path, 'zeros', '--mesh-keep', '0', '--mesh-min-faces', '0', '--mesh-smooth', '0'),
            'clean': run_gen_videos(tmp_path, 'clean', '--mesh-keep', '1', '--mesh-smooth', '2', '--geometry-out', geo, '--geometry-res', '32'),
            'bad': run_gen_videos(tmp_path, 'bad', '--mesh-smooth', '-1')}
    out = {}
    for name, (proc, _, _) in runs.items():
        stdout, stderr = proc.communicate(timeout=600)
        assert (proc.returncode == 0) == (name != 'bad'), stderr[-3000:]
        out[name] = stdout, stderr
    assert 'must be >= 0' in out['bad'][1] and not os.path.exists(runs['bad'][2])
    # the three flags at 0: the bytes of the files written without them
    assert 'mesh cleaning' not in out['plain'][0] and 'mesh cleaning' not in out['zeros'][0]
    assert open(runs['plain'][2], 'rb').read() == open(runs['zeros'][2], 'rb').read()
    assert np.array_equal(np.load(runs['plain'][1]), np.load(runs['zeros'][1]))
    # --mesh-keep 1 --mesh-smooth 2: the ports applied to marching cubes of the saved volume
    vol = np.load(runs['clean'][1])
    mv, mf = S.marching_cubes_numpy(np.ascontiguousarray(vol.transpose(2, 1, 0)), 0.0)
    want = S.clean_mesh(mv, mf, keep_largest=1, smooth=2)
    verts, faces = S.read_ply(runs['clean'][2])
    assert same_bits(verts, want.verts) and np.array_equal(faces, want.faces) and len(faces) > 0
    stdout = out['clean'][0]
    assert stdout.count(S.clean_report_line(want.report, 2)) == 1 and stdout.count('mesh cleaning') == 1       # one line, though two options clean
    # ... and the geometry frames are drawn from that cleaned, smoothed mesh
    frames = np.load(geo)
    labels = H.orbit_labels(range(2), 2, 2.7)
    drawn = S.render_mesh(verts, faces, labels[:, :16].reshape(-1, 4, 4).numpy(), labels[:, 16:].reshape(-1, 3, 3).numpy(), 32,
                          mesh2world=gv.mesh_to_world_matrix(32, 1.0), outputs=('frame',))
    assert frames.shape == (2, 32, 32, 3) and np.array_equal(frames, drawn['frame']) and (frames != 255).any()


def test_mesh_density_grid_hands_the_report_out(tmp_path):
    """--mesh's call on a CPU volume: the report comes back on the returned record, the return value keeps its three entries."""
    import gen_videos_mi355x as gv
    vol = torch.from_numpy(four_balls_field())
    plain, cleaned = str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply')
    written = gv.mesh_density_grid(vol, plain, 0.0)
    assert len(written) == 3 and 'clean' not in written.mesh.reports
    written = gv.mesh_density_grid(vol, cleaned, 0.0, clean=S.clean_options(0, 0, 0))
    assert len(written) == 3 and 'clean' not in written.mesh.reports
    assert open(plain, 'rb').read() == open(cleaned, 'rb').read()
    nv, nf, dt = written = gv.mesh_density_grid(vol, cleaned, 0.0, clean=S.clean_options(2, 0, 3))
    report = written.mesh.reports['clean']
    assert report['components'] == 4 and report['kept'] == 2 and report['kept_faces'] == nf == 7304 + 620 and report['kept_vertices'] == nv
    mv, mf = S.marching_cubes_numpy(vol.permute(2, 1, 0).contiguous().numpy(), 0.0)
    want = S.clean_mesh(mv, mf, keep_largest=2, smooth=3)
    verts, faces = S.read_ply(cleaned)
    assert same_bits(verts, want.verts) and np.array_equal(faces, want.faces) and report == want.report
    assert gv.mesh_density_grid(vol, cleaned, 0.0, clean=S.clean_options(1, 0, 0))[:2] == (len(S.clean_mesh(mv, mf, keep_largest=1).verts), 7304)


# ---------------------------------------------------------------------------------------------------------------- the pipeline
def stand_in_stages(calls):
    """Stand-ins for the stages that need a generator: each records its name and the arrays it was handed."""
    def snap(verts, faces):
        calls.append(('snap', verts.copy(), faces.copy()))
        return verts + np.float32(0.25), dict(vertices=len(verts))

    def attributes(verts):
        calls.append(('attributes', verts.copy()))
        return verts * np.float32(2), verts.astype(np.int64).astype(np.uint8)

    def bake(verts, faces, normals, colors):
        calls.append(('bake', verts.copy(), faces.copy(), normals, colors))
        return dict(colors=255 - colors, weight=np.ones(len(verts), np.float32), seen=np.ones(len(verts), np.int32))
    return snap, attributes, bake


@pytest.mark.parametrize('with_snap', [False, True])
def test_finish_mesh_runs_the_stages_in_the_one_order(meshes, with_snap):
    """The pipeline against the primitives composed by hand, without a generator: where the attributes are evaluated with and without a snap,
    the bake last with the attributes' colours, the reports of the stages that ran."""
    mv, mf = meshes['balls']
    calls = []
    snap, attributes, bake = stand_in_stages(calls)
    got = S.finish_mesh(mv, mf, clean=S.clean_options(2, 0, 3), simplify=S.simplify_options(3.0, 0), snap=snap if with_snap else None,
                        attributes=attributes, bake=bake)
    label, faces_of, _ = S.mesh_components_numpy(mf, len(mv))
    keep = np.zeros(len(mv), np.uint8)
    keep[S.mesh_select(faces_of, keep_largest=2)] = 1
    cv, cf, _ = S.mesh_compact_numpy(mv, mf, label, faces_of, keep)
    sv, sf = S.mesh_simplify_numpy(cv, cf, 3.0, cv.min(axis=0))[:2]
    smoothed = S.mesh_smooth_numpy(sv, sf, 3)
    assert 0 < len(sf) < len(cf) < len(mf) and not same_bits(smoothed, sv)
    if with_snap:
        assert [c[0] for c in calls] == ['snap', 'attributes', 'bake']
        assert same_bits(calls[0][1], smoothed) and same_bits(calls[0][2], sf)
        final = smoothed + np.float32(0.25)
        seen_by_attributes = final                                       # the smoothed, then snapped positions
        assert list(got.reports) == ['clean', 'simplify', 'snap', 'bake'] and got.reports['snap'] == dict(vertices=len(sv))
    else:
        assert [c[0] for c in calls] == ['attributes', 'bake']
        final, seen_by_attributes = smoothed, sv                         # the unsmoothed simplified positions
        assert list(got.reports) == ['clean', 'simplify', 'bake']
    assert same_bits(calls[-2][1], seen_by_attributes)
    assert same_bits(got.verts, final) and same_bits(got.faces, sf)
    assert same_bits(got.normals, seen_by_attributes * np.float32(2)) and same_bits(got.colors, seen_by_attributes.astype(np.int64).astype(np.uint8))
    _, baked_verts, baked_faces, baked_normals, baked_colors = calls[-1]
    assert same_bits(baked_verts, final) and same_bits(baked_faces, sf) and baked_normals is got.normals and baked_colors is got.colors
    assert got.baked is got.reports['bake'] and same_bits(got.baked['colors'], 255 - got.colors)
    kept = S.clean_mesh(mv, mf, keep_largest=2)
    assert got.reports['clean'] == kept.report and got.reports['simplify'] == S.simplify_mesh(kept.verts, kept.faces, cell=3.0).report
    lines = S.report_lines({k: got.reports[k] for k in ('bake', 'simplify', 'clean')}, smooth=3, bake_views=4)       # in stage order, whatever the dict's
    assert lines == [S.clean_report_line(kept.report, 3), S.simplify_report_line(got.reports['simplify']), S.bake_report_line(got.baked, 4)]


def test_finish_mesh_runs_only_what_is_asked(meshes):
    mv, mf = meshes['balls']
    plain = S.finish_mesh(mv, mf)
    assert same_bits(plain.verts, mv) and same_bits(plain.faces, mf) and plain[2:] == (None, None, None, {}) and S.report_lines(plain.reports) == []
    smoothed = S.finish_mesh(torch.from_numpy(mv.copy()), torch.from_numpy(mf.copy()), clean=S.clean_options(0, 0, 2))     # CPU tensors: numpy out
    assert isinstance(smoothed.verts, np.ndarray) and same_bits(smoothed.verts, S.mesh_smooth_numpy(mv, mf, 2)) and list(smoothed.reports) == ['clean']
    simplified = S.finish_mesh(mv, mf, simplify=S.simplify_options(0, 500))
    assert list(simplified.reports) == ['simplify'] and 0 < len(simplified.faces) <= 500


def test_both_clis_take_the_shared_flags_from_one_declaration(monkeypatch, capsys):
    import gen_videos_mi355x as gv
    flags = ['--mesh-keep', '2', '--mesh-min-faces', '5', '--mesh-smooth', '3', '--mesh-simplify', '1.5', '--mesh-target-faces', '700']
    shape, videos = S.arg_parser(), gv.arg_parser()
    from_shape = S.mesh_options_from_args(shape.parse_args(['volume.mrc', *flags]), shape)
    from_videos = S.mesh_options_from_args(videos.parse_args([*flags, '--mesh-snap', '1.5']), videos)
    assert from_shape[:2] == from_videos[:2] == (S.clean_options(2, 5, 3), S.simplify_options(1.5, 700))
    assert from_shape[2] is None and from_videos[2] == S.snap_options(1.5)               # the shape tool has no generator to snap to
    assert S.mesh_options_from_args(videos.parse_args([]), videos) == (None, None, None)
    for bad in (['--mesh-smooth', '-1'], ['--mesh-keep', '-2'], ['--mesh-simplify', '-0.5'], ['--mesh-simplify', 'inf'], ['--mesh-target-faces', '-1']):
        for run in (lambda: S.main(['volume.mrc', *bad]), gv.main):
            monkeypatch.setattr(sys, 'argv', ['gen_videos_mi355x.py', '--random-init', *bad])
            with pytest.raises(SystemExit) as exit_:
                run()
            assert exit_.value.code == 2 and 'must be >= 0' in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------------------- interface
def test_mesh_clean_declarations():
    import gnerf_hip
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    assert int(re.search(r'#define GNERF_ABI_VERSION (\d+)', header).group(1)) == gnerf_hip.ABI_VERSION == 15
    assert 'fp contract(off)' in open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'mesh_clean.hip')).read()
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    want = {'gnerf_mesh_workspace_bytes': (i, [i, i, ctypes.POINTER(ctypes.c_size_t)]),
            'gnerf_mesh_components': (i, [p, i, i, p, p, p, p, p]),
            'gnerf_mesh_compact_count': (i, [p, i, i, p, p, p, p, p, p]),
            'gnerf_mesh_compact_emit': (i, [p, p, i, i, p, p, p, p, p, p, p, p]),
            'gnerf_mesh_smooth': (i, [p, i, p, i, i, f, f, i, p, p, p])}
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    binding = open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'torch_binding.cpp')).read()
    for name, sig in want.items():
        assert gnerf_hip.SIGNATURES[name] == sig
        assert name in gnerf_hip.OPTIONAL_SYMBOLS                   # a library of the same version built before them still loads
        args = re.search(name + r'\s*\((.*?)\)\s*;', header, flags=re.S).group(1)
        assert len(args.split(',')) == len(sig[1]), name
        assert hasattr(gnerf_hip.load(), name)
        assert name + '(' in binding
    assert gnerf_hip.mesh_clean_available()
    for name in ('mesh_components', 'mesh_compact', 'mesh_smooth', 'mesh_clean_available', 'mesh_workspace_bytes', '_mesh_components_ctypes',
                 '_mesh_compact_ctypes', '_mesh_smooth_ctypes'):
        assert callable(getattr(gnerf_hip, name))
    for name in ('mesh_components', 'mesh_compact', 'mesh_smooth'):
        assert re.search(r'm\.def\("%s"' % name, binding)
    csrc = os.path.join(ROOT, 'g-nerf_amd', 'csrc')             # build.sh builds the units that compile_unit.sh lists
    assert re.search(r'^for src in \$UNITS;', open(os.path.join(csrc, 'build.sh')).read(), flags=re.M)
    assert re.search(r'^UNITS="[^"]*\bmesh_clean\b', open(os.path.join(csrc, 'compile_unit.sh')).read(), flags=re.M)


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    import gnerf_hip
    lib = gnerf_hip.load()
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)
    n = ctypes.c_size_t()
    assert lib.gnerf_mesh_workspace_bytes(1000, 2000, ctypes.byref(n)) == 0 and n.value >= 24 * 2000 + 37 * 1000
    assert gnerf_hip.mesh_workspace_bytes(1000, 2000) == n.value
    assert lib.gnerf_mesh_workspace_bytes(0, 0, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.gnerf_mesh_workspace_bytes(10, 20, None) == -1 and b'null' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_workspace_bytes(-1, 20, ctypes.byref(n)) == -1 and b'negative' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_components(ptr, 3, 1, None, ptr, ptr, ptr, None) == -1 and b'null' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_components(None, 3, 1, ptr, ptr, ptr, ptr, None) == -1 and b'null' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_components(ptr, 3, -1, ptr, ptr, ptr, ptr, None) == -1 and b'negative' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_compact_count(ptr, 3, 1, ptr, ptr, None, ptr, ptr, None) == -1 and b'null' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_compact_count(ptr, -3, 1, ptr, ptr, ptr, ptr, ptr, None) == -1 and b'negative' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_compact_emit(ptr, ptr, 3, 1, ptr, ptr, ptr, ptr, ptr, ptr, None, None) == -1 and b'null' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_smooth(ptr, 3, ptr, 1, -1, 0.5, -0.53, 1, ptr, ptr, None) == -1 and b'iterations' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_smooth(ptr, 3, ptr, 1, 1, 0.5, -0.53, 1, None, ptr, None) == -1 and b'null' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_smooth(None, 3, ptr, 1, 1, 0.5, -0.53, 1, ptr, ptr, None) == -1 and b'null' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_smooth(ptr, 3, ptr, 2 ** 30, 1, 0.5, -0.53, 1, ptr, ptr, None) == -1 and b'faces' in lib.gnerf_last_error()
    # CPU tensors never reach the library
    with pytest.raises(RuntimeError):
        gnerf_hip.mesh_components(torch.zeros(1, 3, dtype=torch.int32), 3)
    with pytest.raises(RuntimeError):
        gnerf_hip.mesh_smooth(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), 1)
