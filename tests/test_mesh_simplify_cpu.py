"""CPU tests of the mesh simplification (shape_mi355x.mesh_simplify_numpy / simplify_mesh, the numpy port of csrc/mesh_simplify.hip): pinned
counts of the fixture meshes, the clustering's invariants, order independence, identity, planes and corners, degenerate inputs, the target
search, the CLI flags, and the declarations of the native layer."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import shape_mi355x as S
from test_mesh_clean_cpu import four_balls_field, grid_mesh, largest_component, random_mesh, rough_sphere_field, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIGIN = (-0.3, 0.1, 0.2)
CELLS = (0.25, 0.5, 0.75, 1.3, 2.0, 5.3)


# ---------------------------------------------------------------------------------------------------------------- meshes (made once, never changed)
def cube_mesh(n=8):
    """The surface of the cube [0, n]^3 on the integer lattice, welded along its edges, every square split in two, normals outward."""
    index = -np.ones((n + 1, n + 1, n + 1), dtype=np.int64)
    g = np.arange(n + 1)
    x, y, z = np.meshgrid(g, g, g, indexing='ij')
    surface = (x == 0) | (x == n) | (y == 0) | (y == n) | (z == 0) | (z == n)
    index[surface] = np.arange(np.count_nonzero(surface))
    verts = np.stack([x[surface], y[surface], z[surface]], axis=1).astype(np.float32)
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing='ij'))
    faces = []
    for axis in range(3):
        for side in (0, n):
            def at(di, dj):
                p = [None, None, None]
                p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = np.full_like(i, side), i + di, j + dj
                return index[p[0], p[1], p[2]]
            a, b, c, d = at(0, 0), at(1, 0), at(1, 1), at(0, 1)          # counter-clockwise seen from +axis
            quad = [np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]
            faces += quad if side else [q[:, ::-1] for q in quad]
    return verts, np.concatenate(faces).astype(np.int32)


@pytest.fixture(scope='module')
def meshes():
    made = {'random': random_mesh((33, 34, 35), 0.5), 'balls': S.marching_cubes_numpy(four_balls_field(), 0.0)}
    made['rough'] = largest_component(*S.marching_cubes_numpy(rough_sphere_field(), 0.0))
    for v, f in made.values():
        v.setflags(write=False)
        f.setflags(write=False)
    return made


def edge_counts(faces):
    """(undirected edges that lie in an odd number of faces, directed edges without their reverse)."""
    f = np.asarray(faces, dtype=np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, n = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    code = lambda e: e[:, 0] << 32 | e[:, 1]
    fwd, bwd = np.unique(code(d), return_counts=True), np.unique(code(d[:, ::-1]), return_counts=True)
    unmatched = not (np.array_equal(fwd[0], bwd[0]) and np.array_equal(fwd[1], bwd[1]))
    return int(np.count_nonzero(n % 2)), unmatched


def shuffled(faces, seed):
    """The faces in another order, each with its ids rotated."""
    rng = np.random.default_rng(seed)
    f = faces[rng.permutation(len(faces))]
    turn = rng.integers(0, 3, len(f))
    return np.stack([f[np.arange(len(f)), (turn + k) % 3] for k in range(3)], axis=1)


def face_set(faces):
    f = np.asarray(faces)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


# ---------------------------------------------------------------------------------------------------------------- pinned fixtures
PINNED = {('balls', 0.75): (2955, 5882), ('balls', 2.0): (846, 1676), ('balls', 5.3): (146, 264), ('balls', 100.0): (1, 0),
          ('rough', 0.75): (5062, 10118), ('rough', 2.0): (1383, 2748), ('rough', 5.3): (198, 388), ('random', 2.0): (4593, 17654)}


def test_pinned_counts_of_the_fixture_meshes(meshes):
    assert [(len(v), len(f)) for v, f in (meshes[k] for k in ('balls', 'rough', 'random'))] == [(4114, 8212), (7012, 14020), (50710, 106652)]
    for (name, cell), want in PINNED.items():
        verts, faces = meshes[name]
        v, f, src, vmap, counts = S.mesh_simplify_numpy(verts, faces, cell, ORIGIN)
        print(f'{name} at cell {cell}: {counts.tolist()}')
        assert (len(v), len(f)) == want == (counts[0], counts[1])
        assert S.mesh_simplify_numpy(verts, faces, cell, ORIGIN, count_only=True).tolist() == counts.tolist()
        assert v.dtype == np.float32 and f.dtype == np.int32 and src.dtype == np.int32 and vmap.dtype == np.int32 and counts.dtype == np.int64
    counts = S.mesh_simplify_numpy(*meshes['random'], 2.0, ORIGIN, count_only=True)
    assert counts[3] == 83698 and counts[4] == 5300


# ---------------------------------------------------------------------------------------------------------------- invariants
@pytest.mark.parametrize('name', ['random', 'balls', 'rough'])
def test_invariants_of_the_clustering(meshes, name):
    verts, faces = meshes[name]
    for cell in CELLS:
        v, f, src, vmap, counts = S.mesh_simplify_numpy(verts, faces, cell, ORIGIN)
        # the cluster map is a labelling: cluster[v] <= v, cluster[cluster[v]] == cluster[v]; new ids number the representatives in ascending order
        assert np.all(vmap >= 0) and len(src) == counts[0] == vmap.max() + 1 and len(f) == counts[1]
        cluster = src[vmap]
        assert np.all(cluster <= np.arange(len(verts))) and np.array_equal(cluster[cluster], cluster) and np.all(np.diff(src) > 0)
        assert np.array_equal(vmap[src], np.arange(len(src)))
        # no vertex leaves its cell: within one cell per axis of its new vertex, plus the float32 rounding of the coordinates
        moved = np.abs(verts.astype(np.float64) - v[vmap].astype(np.float64)).max()
        bound = float(np.float32(cell)) + 2.0 ** -23 * float(np.abs(verts).max() + 1)
        odd, unmatched = edge_counts(f)
        print(f'{name} at cell {cell}: {counts.tolist()}, moved at most {moved / cell:.4f} cells, {odd} odd edges, directed edges unmatched: {unmatched}')
        assert moved <= bound
        assert odd == 0                                                   # the mod-2 image of a closed mesh is closed
        assert np.all(f >= 0) and np.all(f < len(v)) and np.all(f[:, 0] < f[:, 1]) and np.all(f[:, 0] < f[:, 2]) and np.all(f[:, 1] != f[:, 2])
        assert counts[1] + counts[2] + counts[3] + counts[4] == len(faces) and counts[2] == 0 and counts[6] == 0 and counts[7] == 0
        if name != 'random':
            assert counts[5] == 0 and not unmatched


def test_order_of_the_faces_and_rotation_of_their_ids_do_not_matter(meshes):
    for name, cell in (('rough', 0.75), ('random', 2.0), ('balls', 5.3)):
        verts, faces = meshes[name]
        v, f, src, vmap, counts = S.mesh_simplify_numpy(verts, faces, cell, ORIGIN)
        v2, f2, src2, vmap2, counts2 = S.mesh_simplify_numpy(verts, shuffled(faces, 7), cell, ORIGIN)
        assert same_bits(v, v2) and same_bits(src, src2) and same_bits(vmap, vmap2) and counts.tolist() == counts2.tolist()
        assert np.array_equal(face_set(f), face_set(f2))


def test_a_grid_finer_than_the_mesh_gives_the_mesh_back():
    verts, faces = grid_mesh(9)
    v, f, src, vmap, counts = S.mesh_simplify_numpy(verts, faces, 0.5, (-0.25, -0.25, -0.25))
    print(f'largest difference {np.abs(v - verts).max()}')
    assert same_bits(v, verts) and same_bits(f, faces) and np.array_equal(src, np.arange(81)) and np.array_equal(vmap, np.arange(81))
    assert counts.tolist() == [81, 128, 0, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- planes and corners
def test_flat_regions_stay_on_their_plane():
    verts, faces = grid_mesh(9)
    c, s = np.cos(0.4), np.sin(0.3)
    turn = np.array([[c, -np.sin(0.4), 0], [np.sin(0.4), c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(0.3), -s], [0, s, np.cos(0.3)]])
    for cell in (1.7, 3.0):
        v, f, _, _, counts = S.mesh_simplify_numpy(verts, faces, cell, (-0.4, -0.3, -0.7))
        assert 1 < counts[0] < 81 and np.abs(v[:, 2]).max() <= 1e-6 * cell
        tilted = (verts.astype(np.float64) @ turn.T + 5.0).astype(np.float32)
        normal = turn[:, 2]
        height = (tilted.astype(np.float64) - 5.0) @ normal               # the float32 rounding of the input itself
        v, f, _, _, counts = S.mesh_simplify_numpy(tilted, faces, cell, (0.0, 0.0, 0.0))
        off = np.abs((v.astype(np.float64) - 5.0) @ normal)
        print(f'cell {cell}: {counts[0]} vertices, off the tilted plane by at most {off.max():.3g} (the input: {np.abs(height).max():.3g})')
        assert 1 < counts[0] < 81 and off.max() <= 1e-6 * cell


def test_corner_clusters_of_a_cube_land_on_the_corner():
    verts, faces = cube_mesh(8)
    assert len(verts) == 386 and len(faces) == 768 and edge_counts(faces) == (0, False)
    v, f, src, vmap, counts = S.mesh_simplify_numpy(verts, faces, 4.5, (-0.5, -0.5, -0.5))
    assert counts[0] == 8 and edge_counts(f)[0] == 0
    corner = np.where(verts[src] < 4, 0.0, 8.0)
    for c in range(8):
        centroid = verts[vmap == c].astype(np.float64).mean(axis=0)
        ratio = np.linalg.norm(v[c] - corner[c]) / np.linalg.norm(centroid - corner[c])
        print(f'corner {corner[c]}: the vertex {v[c]}, {ratio:.4f} of the centroid\'s distance (3 / 259 = {3 / 259:.4f})')
        assert ratio <= 0.1


# ---------------------------------------------------------------------------------------------------------------- degenerate inputs
def test_degenerate_inputs():
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    verts = np.array([[0.2, 0.2, 0.2], [2.2, 0.1, 0.3], [0.3, 2.4, 0.2], [0.1, 0.3, 2.2], [9, 9, 9]], np.float32)
    for v_in in (none_v, verts):
        v, f, src, vmap, counts = S.mesh_simplify_numpy(v_in, none_f, 1.0, (0, 0, 0))
        assert v.shape == (0, 3) and f.shape == (0, 3) and src.shape == (0,) and vmap.tolist() == [-1] * len(v_in) and counts.tolist() == [0] * 8
    tet = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    v, f, src, vmap, counts = S.mesh_simplify_numpy(verts, tet, 1.0, (0, 0, 0))
    assert counts.tolist() == [4, 4, 0, 0, 0, 0, 0, 0] and vmap.tolist() == [0, 1, 2, 3, -1] and src.tolist() == [0, 1, 2, 3]
    # ids out of range, a NaN vertex, repeated ids: counted, skipped
    bad = np.concatenate([tet, np.array([[0, 1, 5], [0, -1, 2], [1, 1, 2], [4, 0, 1]], np.int32)])
    nan_verts = verts.copy()
    nan_verts[4, 1] = np.nan
    v2, f2, src2, vmap2, counts2 = S.mesh_simplify_numpy(nan_verts, bad, 1.0, (0, 0, 0))
    assert counts2.tolist() == [4, 4, 3, 1, 0, 0, 0, 0] and vmap2.tolist() == [0, 1, 2, 3, -1]
    assert same_bits(v2, v) and same_bits(f2, f)                             # (1, 1, 2) has a zero normal: no quadric
    # a face of zero area across three cells contributes no quadric: the vertices are the centroids' clusters as without it
    line = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.25, 0.75, 0.5]], np.float32)
    v3, f3, _, vmap3, counts3 = S.mesh_simplify_numpy(line, np.array([[0, 1, 2]], np.int32), 1.0, (0, 0, 0))
    assert counts3.tolist() == [3, 1, 0, 0, 0, 0, 0, 0] and same_bits(v3, line[:3]) and f3.tolist() == [[0, 1, 2]]
    with pytest.raises(ValueError):
        S.mesh_simplify_numpy(verts, tet, 0.0, (0, 0, 0))
    with pytest.raises(ValueError):
        S.mesh_simplify_numpy(verts, tet, np.inf, (0, 0, 0))
    with pytest.raises(ValueError):
        S.mesh_simplify_numpy(verts, tet, 1.0, (0, np.nan, 0))
    # a vertex far outside the 2^21-cell grid is clamped into its last cell; simplify_mesh refuses such an extent
    far = verts.copy()
    far[3] = [0.1, 0.3, 3e6]
    v4, _, _, _, counts4 = S.mesh_simplify_numpy(far, tet, 1.0, (0, 0, 0))
    assert counts4[0] == 4 and np.all(np.isfinite(v4)) and 2 ** 21 - 1 <= v4[3, 2] <= 2 ** 21
    with pytest.raises(ValueError, match='cells'):
        S.simplify_mesh(far, tet, cell=1.0)


# ---------------------------------------------------------------------------------------------------------------- the public layer
def test_simplify_mesh_gathers_and_reports(meshes):
    verts, faces = meshes['balls']
    rng = np.random.default_rng(3)
    normals, colors = rng.standard_normal((len(verts), 3)).astype(np.float32), rng.integers(0, 256, (len(verts), 3), dtype=np.uint8)
    got = S.simplify_mesh(verts, faces, cell=2.0, origin=ORIGIN, normals=normals, colors=colors)
    v, f, src, vmap, counts = S.mesh_simplify_numpy(verts, faces, 2.0, ORIGIN)
    assert same_bits(got.verts, v) and same_bits(got.faces, f) and same_bits(got.src_vertex, src) and same_bits(got.vertex_map, vmap)
    assert same_bits(got.normals, normals[src]) and same_bits(got.colors, colors[src])
    assert got.report == dict(cell=2.0, origin=tuple(float(np.float32(x)) for x in ORIGIN), target_faces=0, j=None, count_calls=0, met=True, vertices=4114,
                              faces=8212, new_vertices=846, new_faces=1676, invalid=0, collapsed=6536, absorbed=0, multi=0)
    assert 'cell 2' in S.simplify_report_line(got.report) and '1676 of 8212 triangles' in S.simplify_report_line(got.report)
    # the default origin: the minimum of the finite vertices; CPU tensors take the port
    low = verts.min(axis=0)
    a = S.simplify_mesh(verts, faces, cell=2.0)
    b = S.simplify_mesh(torch.from_numpy(verts.copy()), torch.from_numpy(faces.copy()), cell=2.0)
    assert a.report['origin'] == tuple(float(x) for x in low) and isinstance(b.verts, np.ndarray) and same_bits(a.verts, b.verts) and same_bits(a.faces, b.faces)
    assert same_bits(a.verts, S.mesh_simplify_numpy(verts, faces, 2.0, low)[0])
    with pytest.raises(ValueError):
        S.simplify_mesh(verts, faces)
    with pytest.raises(ValueError):
        S.simplify_mesh(verts, faces, cell=1.0, target_faces=-1)
    assert S.simplify_options(0, 0) is None and S.simplify_options(2.0, 0) == dict(cell=2.0, target_faces=0)
    assert S.simplify_options(0, 500, voxel=0.5) == dict(cell=0.5, target_faces=500)
    with pytest.raises(ValueError):
        S.simplify_options(-1.0, 0)


def test_target_search_bisects_to_the_smallest_passing_candidate(meshes):
    verts, faces = meshes['balls']
    cells = S.simplify_candidates(1.0)
    assert len(cells) == 41 and cells[0] == 1.0 and cells[4] == 2.0 and cells[40] == 1024.0
    left = [int(S.mesh_simplify_numpy(verts, faces, c, verts.min(axis=0), count_only=True)[1]) for c in cells]
    print(f'faces left per candidate: {left}')
    for target in (1000, 200):
        got = S.simplify_mesh(verts, faces, target_faces=target)
        want = min(j for j in range(41) if left[j] <= target)
        print(f'target {target}: candidate {got.report["j"]} (cell {got.report["cell"]:g}, {got.report["new_faces"]} faces) after {got.report["count_calls"]} count calls')
        assert got.report['j'] == want and got.report['met'] and got.report['count_calls'] <= 7
        assert got.report['cell'] == cells[want] and got.report['new_faces'] == left[want] <= target and len(got.faces) == left[want]
        assert f'candidate {want} for at most {target} faces' in S.simplify_report_line(got.report)
    # a base of its own, and a target nothing meets
    got = S.simplify_mesh(verts, faces, cell=0.5, target_faces=1000)
    assert got.report['cell'] == S.simplify_candidates(0.5)[got.report['j']] and got.report['new_faces'] <= 1000
    calls = []
    assert S.simplify_search(lambda j: calls.append(j) or 10, 5) == (40, len(calls), False) and len(calls) <= 7
    assert S.simplify_search(lambda j: 0, 5)[:1] == (0,)


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_flags_at_zero_write_the_same_bytes_and_simplification_matches_simplify_mesh(tmp_path, capsys):
    vol = four_balls_field() + 10.0                           # the surfaces sit at level 10, the CLI's default
    mrc, ply = str(tmp_path / 'shape.mrc'), str(tmp_path / 'shape.ply')
    S.write_mrc(mrc, vol)
    assert S.main([mrc, '--device', 'cpu']) == 0
    plain = open(ply, 'rb').read()
    assert S.main([mrc, '--device', 'cpu', '--mesh-simplify', '0', '--mesh-target-faces', '0']) == 0
    assert open(ply, 'rb').read() == plain and 'mesh simplification' not in capsys.readouterr().out
    mv, mf = S.marching_cubes_numpy(np.ascontiguousarray(S.read_mrc(mrc).transpose(2, 1, 0)), 10.0)
    assert S.main([mrc, '--device', 'cpu', '--mesh-simplify', '2.5']) == 0
    want = S.simplify_mesh(mv, mf, cell=2.5)
    verts, faces = S.read_ply(ply)
    assert same_bits(verts, want.verts) and same_bits(faces, want.faces) and 0 < len(faces) < len(mf)
    out = capsys.readouterr().out
    assert out.count(S.simplify_report_line(want.report)) == 1 and 'mesh cleaning' not in out
    # with the cleaning flags: components and compaction, then simplification, then smoothing
    assert S.main([mrc, '--device', 'cpu', '--mesh-keep', '1', '--mesh-smooth', '2', '--mesh-target-faces', '900']) == 0
    kept = S.clean_mesh(mv, mf, keep_largest=1)
    want = S.simplify_mesh(kept.verts, kept.faces, target_faces=900)
    verts, faces = S.read_ply(ply)
    assert same_bits(verts, S.mesh_smooth_numpy(want.verts, want.faces, 2)) and same_bits(faces, want.faces) and 0 < len(faces) <= 900
    out = capsys.readouterr().out
    assert 'mesh cleaning: kept 1 of 4' in out and S.simplify_report_line(want.report) in out
    with pytest.raises(SystemExit):
        S.main([mrc, '--device', 'cpu', '--mesh-simplify', '-1'])


def test_mesh_density_grid_simplifies_between_compaction_and_smoothing(tmp_path):
    import gen_videos_mi355x as gv
    vol = torch.from_numpy(four_balls_field())
    plain, other = str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply')
    assert len(gv.mesh_density_grid(vol, plain, 0.0)) == 3
    written = gv.mesh_density_grid(vol, other, 0.0, simplify=S.simplify_options(0, 0))
    assert len(written) == 3 and open(plain, 'rb').read() == open(other, 'rb').read() and written.mesh.reports == {}
    nv, nf, _ = written = gv.mesh_density_grid(vol, other, 0.0, clean=S.clean_options(2, 0, 3), simplify=S.simplify_options(3.0, 0))
    assert list(written.mesh.reports) == ['clean', 'simplify']
    report, simplify_report = written.mesh.reports['clean'], written.mesh.reports['simplify']
    mv, mf = S.marching_cubes_numpy(vol.permute(2, 1, 0).contiguous().numpy(), 0.0)
    kept = S.clean_mesh(mv, mf, keep_largest=2)
    want = S.simplify_mesh(kept.verts, kept.faces, cell=3.0)
    verts, faces = S.read_ply(other)
    assert same_bits(verts, S.mesh_smooth_numpy(want.verts, want.faces, 3)) and same_bits(faces, want.faces) and (nv, nf) == (len(verts), len(faces))
    assert report == kept.report and simplify_report == want.report and nf < kept.report['kept_faces']


# ---------------------------------------------------------------------------------------------------------------- interface
def test_mesh_simplify_declarations():
    import gnerf_hip
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    assert int(re.search(r'#define GNERF_ABI_VERSION (\d+)', header).group(1)) == gnerf_hip.ABI_VERSION == 15
    assert 'fp contract(off)' in open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'mesh_simplify.hip')).read()
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    want = {'gnerf_mesh_simplify_workspace_bytes': (i, [i, i, ctypes.POINTER(ctypes.c_size_t)]),
            'gnerf_mesh_simplify_count': (i, [p, p, i, i, f, ctypes.POINTER(f), p, p, p]),
            'gnerf_mesh_simplify_emit': (i, [p, p, i, i, f, ctypes.POINTER(f), p, p, p, p, p, p])}
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    binding = open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'torch_binding.cpp')).read()
    for name, sig in want.items():
        assert gnerf_hip.SIGNATURES[name] == sig
        assert name in gnerf_hip.OPTIONAL_SYMBOLS                   # a library of the same version built before them still loads
        args = re.search(name + r'\s*\((.*?)\)\s*;', header, flags=re.S).group(1)
        assert len(args.split(',')) == len(sig[1]), name
        assert hasattr(gnerf_hip.load(), name)
        assert name + '(' in binding
    assert gnerf_hip.mesh_simplify_available()
    for name in ('mesh_simplify', 'mesh_simplify_count', 'mesh_simplify_available', 'mesh_simplify_workspace_bytes', '_mesh_simplify_ctypes'):
        assert callable(getattr(gnerf_hip, name))
    for name in ('mesh_simplify', 'mesh_simplify_count'):
        assert re.search(r'm\.def\("%s"' % name, binding)
    csrc = os.path.join(ROOT, 'g-nerf_amd', 'csrc')             # build.sh builds the units that compile_unit.sh lists
    assert re.search(r'^for src in \$UNITS;', open(os.path.join(csrc, 'build.sh')).read(), flags=re.M)
    assert re.search(r'^UNITS="[^"]*\bmesh_simplify\b', open(os.path.join(csrc, 'compile_unit.sh')).read(), flags=re.M)


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    import gnerf_hip
    lib = gnerf_hip.load()
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)
    n = ctypes.c_size_t()
    origin = (ctypes.c_float * 3)(0, 0, 0)
    assert lib.gnerf_mesh_simplify_workspace_bytes(1000, 2000, ctypes.byref(n)) == 0 and n.value >= 13 * 8 * 1000 + 2 * 4 * 2048 + 2 * 4 * 4096
    assert gnerf_hip.mesh_simplify_workspace_bytes(1000, 2000) == n.value
    assert lib.gnerf_mesh_simplify_workspace_bytes(0, 0, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.gnerf_mesh_simplify_workspace_bytes(10, 20, None) == -1 and b'null' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_simplify_workspace_bytes(-1, 20, ctypes.byref(n)) == -1 and b'negative' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_simplify_workspace_bytes(2 ** 30 + 1, 20, ctypes.byref(n)) == -1 and b'2^30' in lib.gnerf_last_error()
    count, emit = lib.gnerf_mesh_simplify_count, lib.gnerf_mesh_simplify_emit
    assert count(ptr, ptr, 3, 1, 1.0, origin, None, ptr, None) == -1 and b'null' in lib.gnerf_last_error()
    assert count(None, ptr, 3, 1, 1.0, origin, ptr, ptr, None) == -1 and b'null' in lib.gnerf_last_error()
    assert count(ptr, ptr, 3, 1, 1.0, None, ptr, ptr, None) == -1 and b'null' in lib.gnerf_last_error()
    assert count(ptr, ptr, 3, -1, 1.0, origin, ptr, ptr, None) == -1 and b'negative' in lib.gnerf_last_error()
    for cell in (0.0, -1.0, float('inf'), float('nan')):
        assert count(ptr, ptr, 3, 1, cell, origin, ptr, ptr, None) == -1 and b'cell' in lib.gnerf_last_error()
        assert emit(ptr, ptr, 3, 1, cell, origin, ptr, ptr, ptr, ptr, ptr, None) == -1 and b'cell' in lib.gnerf_last_error()
    assert count(ptr, ptr, 3, 1, 1.0, (ctypes.c_float * 3)(0, float('nan'), 0), ptr, ptr, None) == -1 and b'origin' in lib.gnerf_last_error()
    assert emit(ptr, ptr, 3, 1, 1.0, origin, ptr, None, ptr, ptr, ptr, None) == -1 and b'null' in lib.gnerf_last_error()
    assert emit(ptr, ptr, 3, 1, 1.0, origin, ptr, ptr, ptr, None, None, None) == -1 and b'null' in lib.gnerf_last_error()
    assert emit(ptr, ptr, -3, 1, 1.0, origin, ptr, ptr, ptr, ptr, ptr, None) == -1 and b'negative' in lib.gnerf_last_error()
    assert emit(ptr, ptr, 0, 1, 1.0, origin, ptr, ptr, ptr, ptr, ptr, None) == -1 and b'empty' in lib.gnerf_last_error()
    # CPU tensors never reach the library
    with pytest.raises(RuntimeError):
        gnerf_hip.mesh_simplify(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), 1.0, (0, 0, 0))
    with pytest.raises(RuntimeError):
        gnerf_hip.mesh_simplify_count(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), 1.0, (0, 0, 0))
