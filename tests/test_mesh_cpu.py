"""CPU tests of the mesh extraction (g-nerf_amd/shape_mi355x.py, the counterpart of shape_utils.py): the committed case table is the
generator's, the numpy port of the marching-cubes kernel makes closed, consistently oriented, outward meshes of the right size and
topology, also on volumes full of ambiguous faces, and the PLY / MRC files round-trip."""

import os

import numpy as np
import pytest
import torch

import shape_mi355x as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sphere_field(n, r):
    i = np.arange(n, dtype=np.float64) - (n - 1) / 2
    x, y, z = np.meshgrid(i, i, i, indexing='ij')
    return (r - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


def torus_field(n, big, small):
    i = np.arange(n, dtype=np.float64) - (n - 1) / 2
    x, y, z = np.meshgrid(i, i, i, indexing='ij')
    return (small - np.sqrt((np.sqrt(x * x + y * y) - big) ** 2 + z * z)).astype(np.float32)


def zero_border(v):
    v = v.copy()
    v[0] = v[-1] = 0
    v[:, 0] = v[:, -1] = 0
    v[:, :, 0] = v[:, :, -1] = 0
    return v


def noise_volumes(seed=0, count=6):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        shape = tuple(int(d) for d in rng.integers(12, 21, 3))
        yield zero_border(rng.random(shape).astype(np.float32))


def integer_volumes(seed=1, count=6):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        shape = tuple(int(d) for d in rng.integers(12, 21, 3))
        yield zero_border(rng.integers(0, 4, shape).astype(np.float32))


def assert_closed_oriented(faces):
    """Every directed edge appears exactly once and its reverse exactly once.  Returns the number of undirected edges."""
    f = np.asarray(faces, dtype=np.int64)
    if len(f) == 0:
        return 0
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = d[:, 0] << 32 | d[:, 1]
    uniq, counts = np.unique(key, return_counts=True)
    assert counts.max() == 1, 'a directed edge is used twice'
    assert np.all(np.isin(d[:, 1] << 32 | d[:, 0], uniq)), 'an edge has no reverse (the mesh is open or inconsistently oriented)'
    return len(uniq) // 2


def euler(verts, faces):
    return len(verts) - assert_closed_oriented(faces) + len(faces)


def area_volume(verts, faces):
    p = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    cr = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return 0.5 * np.linalg.norm(cr, axis=1).sum(), np.einsum('ij,ij->i', p[:, 0], cr).sum() / 6


def test_case_table_header_is_the_generators_output():
    with open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'mesh_tables.h')) as f:
        assert f.read() == S.case_table_header()
    count, table, edges = S.case_table()
    assert count[0] == 0 and count[255] == 0 and count.max() == table.shape[1]
    assert len(edges) == 12 and edges == sorted(edges)


def test_sphere_is_closed_outward_and_sized():
    r = 20.0
    verts, faces = S.marching_cubes(sphere_field(48, r), 0.0)
    assert verts.dtype == np.float32 and faces.dtype == np.int32 and verts.shape[1] == 3 and faces.shape[1] == 3
    assert euler(verts, faces) == 2
    area, vol = area_volume(verts, faces)
    assert abs(area / (4 * np.pi * r * r) - 1) < 0.01
    assert vol > 0 and abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.01


def test_torus_has_euler_characteristic_zero():
    verts, faces = S.marching_cubes(torus_field(48, 13.0, 5.0), 0.0)
    assert euler(verts, faces) == 0
    assert area_volume(verts, faces)[1] > 0


@pytest.mark.parametrize('level', [0.0, 0.25, 0.5, 0.75, 0.95])
def test_noise_volumes_stay_closed_and_oriented(level):
    for v in noise_volumes():
        verts, faces = S.marching_cubes(v, level)
        assert len(faces) > 0
        assert_closed_oriented(faces)
        assert area_volume(verts, faces)[1] > 0


@pytest.mark.parametrize('level', [0.0, 1.0, 2.0])
def test_integer_volumes_with_values_on_the_level_stay_closed(level):
    for v in integer_volumes():
        assert np.count_nonzero(v == level) > 100
        verts, faces = S.marching_cubes(v, level)
        assert len(faces) > 0
        assert_closed_oriented(faces)


def test_vertices_lie_on_the_edge_interpolant():
    v = next(noise_volumes(seed=3, count=1))
    level = np.float32(0.4)
    verts, faces = S.marching_cubes(v, level)
    base = np.floor(verts).astype(np.int64)
    frac = verts - base
    axis = np.argmax(frac, axis=1)                           # the one coordinate off the lattice (t = 0 lands on the point itself)
    a = v[base[:, 0], base[:, 1], base[:, 2]].astype(np.float64)
    nb = base.copy()
    nb[np.arange(len(nb)), axis] += 1
    nb = np.minimum(nb, np.array(v.shape) - 1)
    b = v[nb[:, 0], nb[:, 1], nb[:, 2]].astype(np.float64)
    t = frac[np.arange(len(frac)), axis]
    interp = a + t * (b - a)
    on_edge = frac.max(axis=1) > 0
    assert np.all(np.abs(interp[on_edge] - level) < 1e-5)
    assert np.all(np.count_nonzero(frac, axis=1) <= 1)
    assert faces.min() >= 0 and faces.max() < len(verts)


def test_vertex_and_face_order_follow_the_indices():
    v = sphere_field(24, 8.0)
    verts, faces = S.marching_cubes(v, 0.0)
    owner = np.floor(verts).astype(np.int64)
    axis = np.argmax(verts - owner, axis=1)
    key = (owner[:, 0] * 24 + owner[:, 1]) * 24 + owner[:, 2]
    order = key * 3 + axis
    assert np.all(np.diff(order) > 0)                         # lexicographic by (linear index of p, axis), no duplicates


def test_empty_and_full_volumes_give_empty_meshes():
    for v in (np.zeros((5, 6, 7), np.float32), np.ones((5, 6, 7), np.float32)):
        verts, faces = S.marching_cubes(v, 0.5)
        assert verts.shape == (0, 3) and faces.shape == (0, 3)
        assert verts.dtype == np.float32 and faces.dtype == np.int32


def test_non_finite_input_raises():
    for bad in (np.nan, np.inf, -np.inf):
        v = sphere_field(10, 3.0)
        v[4, 5, 6] = bad
        with pytest.raises(ValueError, match='non-finite'):
            S.marching_cubes(v, 0.0)


def test_bad_shapes_raise():
    with pytest.raises(ValueError):
        S.marching_cubes(np.zeros((1, 4, 4), np.float32), 0.0)
    with pytest.raises(ValueError):
        S.marching_cubes(np.zeros((4, 4), np.float32), 0.0)


def test_cpu_tensor_goes_to_the_numpy_port_with_spacing_and_origin():
    v = sphere_field(16, 5.0)
    verts, faces = S.marching_cubes(torch.from_numpy(v), 0.0)
    ref_v, ref_f = S.marching_cubes_numpy(v, 0.0)
    assert np.array_equal(verts, ref_v) and np.array_equal(faces, ref_f)
    sv, sf = S.marching_cubes(v, 0.0, spacing=(0.5, 2.0, 1.0), origin=(1.0, -1.0, 3.0))
    assert np.array_equal(sf, ref_f)
    assert np.allclose(sv, ref_v * np.float32([0.5, 2.0, 1.0]) + np.float32([1.0, -1.0, 3.0]))


def test_ply_round_trip_and_exact_header(tmp_path):
    verts, faces = S.marching_cubes(sphere_field(12, 3.5), 0.0)
    path = str(tmp_path / 'm.ply')
    nv, nf = S.convert_sdf_samples_to_ply(sphere_field(12, 3.5), [0, 0, 0], 1, path, level=0.0)
    assert (nv, nf) == (len(verts), len(faces))
    data = open(path, 'rb').read()
    header = ('ply\nformat binary_little_endian 1.0\n'
              f'element vertex {nv}\nproperty float x\nproperty float y\nproperty float z\n'
              f'element face {nf}\nproperty list uchar int vertex_indices\nend_header\n').encode('ascii')
    assert data.startswith(header)
    body = data[len(header):]
    assert len(body) == nv * 12 + nf * 13
    assert np.array_equal(np.frombuffer(body[:nv * 12], '<f4').reshape(-1, 3), verts)
    rec = np.frombuffer(body[nv * 12:], dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    assert np.all(rec['n'] == 3) and np.array_equal(rec['i'], faces)
    rv, rf = S.read_ply(path)
    assert np.array_equal(rv, verts) and np.array_equal(rf, faces)


def test_ply_applies_origin_scale_offset_like_shape_utils(tmp_path):
    v = sphere_field(12, 3.5)
    verts, faces = S.marching_cubes(v, 0.0, spacing=0.5)
    path = str(tmp_path / 'm.ply')
    S.convert_sdf_samples_to_ply(v, [1.0, 2.0, 3.0], 0.5, path, offset=np.float32(0.25), scale=np.float32(2.0), level=0.0)
    rv, rf = S.read_ply(path)
    expect = ((verts + np.float32([1.0, 2.0, 3.0])) / np.float32(2.0)) - np.float32(0.25)
    assert np.array_equal(rf, faces) and np.array_equal(rv, expect.astype(np.float32))


def test_mrc_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    vol = rng.standard_normal((5, 6, 7)).astype(np.float32)
    path = str(tmp_path / 'v.mrc')
    S.write_mrc(path, vol)
    assert os.path.getsize(path) == 1024 + vol.nbytes
    h = S.mrc_header(path)
    assert (h['nx'], h['ny'], h['nz'], h['mode']) == (7, 6, 5, 2)
    assert h['m'] == (7, 6, 5) and h['map'] == b'MAP ' and h['machst'][:2] == b'\x44\x44' and h['nsymbt'] == 0
    assert h['map_crs'] == (1, 2, 3) and h['cellb'] == (90.0, 90.0, 90.0)
    assert np.isclose(h['dmin_dmax_dmean'][0], vol.min()) and np.isclose(h['dmin_dmax_dmean'][1], vol.max())
    back = S.read_mrc(path)
    assert back.dtype == np.float32 and np.array_equal(back, vol)


def test_read_mrc_skips_the_extended_header(tmp_path):
    vol = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    plain = str(tmp_path / 'a.mrc')
    S.write_mrc(plain, vol)
    raw = bytearray(open(plain, 'rb').read())
    raw[92:96] = np.int32(80).tobytes()
    ext = str(tmp_path / 'b.mrc')
    open(ext, 'wb').write(bytes(raw[:1024]) + b'\x7f' * 80 + bytes(raw[1024:]))
    assert np.array_equal(S.read_mrc(ext), vol)


def test_convert_mrc_and_cli_honour_the_level(tmp_path):
    vol = sphere_field(20, 6.0) + 10.0                       # the surface sits at level 10, the CLI's default
    mrc = str(tmp_path / 'shape.mrc')
    S.write_mrc(mrc, vol)
    assert S.main([mrc, '--device', 'cpu']) == 0
    verts, faces = S.read_ply(str(tmp_path / 'shape.ply'))
    ref_v, ref_f = S.marching_cubes_numpy(np.ascontiguousarray(vol.transpose(2, 1, 0)), 10.0)
    assert np.array_equal(verts, ref_v) and np.array_equal(faces, ref_f) and euler(verts, faces) == 2
    # --level is honoured for a single file, and a directory converts .mrc and .npy alike
    assert S.main([mrc, '--level', '13', '--device', 'cpu']) == 0
    v13, _ = S.read_ply(str(tmp_path / 'shape.ply'))
    assert 0 < len(v13) < len(verts)
    np.save(str(tmp_path / 'other.npy'), vol)
    assert S.main([str(tmp_path), '--level', '12', '--device', 'cpu']) == 0
    a, _ = S.read_ply(str(tmp_path / 'shape.ply'))
    b, _ = S.read_ply(str(tmp_path / 'other.ply'))
    assert np.array_equal(a, b) and len(a) > 0


def test_generator_density_volume_meshes_with_the_mesh_flag_calls(tmp_path):
    """--mesh's calls on a random-init generator's 32^3 CPU volume (the CLI would render the orbit first, slow on a CPU)."""
    import gen_videos_mi355x as gv
    dev = torch.device('cpu')
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1))
    vol = gv.extract_density_grid(G, gv.orbit_latents(G, z, dev), 32)
    level = 0.0                                               # a random-init generator's densities are far below the default 10
    path = str(tmp_path / 'g.ply')
    nv, nf, dt = gv.mesh_density_grid(vol, path, level)
    verts, faces = S.read_ply(path)
    assert (len(verts), len(faces)) == (nv, nf) and nf > 0
    ref_v, ref_f = S.marching_cubes_numpy(vol.permute(2, 1, 0).contiguous().numpy(), level)
    assert np.array_equal(verts, ref_v) and np.array_equal(faces, ref_f)
    assert_closed_oriented(faces)
    assert gv.mesh_density_grid(vol, path, 10.0)[:2] == (0, 0)  # nothing crosses the default level: an empty, valid file
    assert S.read_ply(path)[0].shape == (0, 3)
