"""GPU tests of the mesh-cleaning kernels (csrc/mesh_clean.hip through gnerf_hip.mesh_components / mesh_compact / mesh_smooth and
shape_mi355x.clean_mesh): the same bits as the numpy ports on tiny, noisy, deep-chained and open meshes, reproducible and independent of the
order of the faces, both bindings agree, gen_videos_mi355x.py --mesh-keep / --mesh-smooth end to end."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import shape_mi355x as S
from test_mesh_cpu import assert_closed_oriented
from test_mesh_clean_cpu import grid_mesh, largest_component, random_mesh, rough_sphere_field, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def meshes():
    """Made once on the host and never changed; 'ports' caches what the numpy ports make of them."""
    made = {'random33': random_mesh((33, 34, 35), 0.5), 'noise48': random_mesh((48, 49, 50), 0.55),
            'open': random_mesh((20, 21, 22), 0.5, seed=4, border=False)}
    made['rough'] = largest_component(*S.marching_cubes_numpy(rough_sphere_field(), 0.0))
    for v, f in made.values():
        v.setflags(write=False)
        f.setflags(write=False)
    return made


def on(dev, *arrays):
    return tuple(torch.tensor(np.ascontiguousarray(a), device=dev) for a in arrays)


def host(t):
    return t.cpu().numpy()


def components_match(faces, n_verts, dev, port=None):
    import gnerf_hip
    port = S.mesh_components_numpy(faces, n_verts) if port is None else port
    label, faces_of, counts = gnerf_hip.mesh_components(on(dev, faces)[0], n_verts)
    assert label.is_cuda and label.dtype == torch.int32 and faces_of.dtype == torch.int32 and not counts.is_cuda and counts.dtype == torch.int64
    assert same_bits(host(label), port[0]) and same_bits(host(faces_of), port[1]) and counts.tolist() == port[2].tolist()
    return port


def smooth_matches(verts, faces, dev, iterations, **kw):
    import gnerf_hip
    want = S.mesh_smooth_numpy(verts, faces, iterations, **kw)
    got = gnerf_hip.mesh_smooth(*on(dev, verts, faces), iterations, **kw)
    assert got.is_cuda and got.dtype == torch.float32 and same_bits(host(got), want)
    return want


# ---------------------------------------------------------------------------------------------------------------- components
def test_tiny_meshes_match_the_ports(dev):
    import gnerf_hip
    tet = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)
    faces = np.concatenate([tet + 5, tet, np.array([[9, 9, 10]], dtype=np.int32)])           # vertex 4 is in no face
    verts = np.random.default_rng(0).standard_normal((11, 3)).astype(np.float32)
    label, faces_of, counts = components_match(faces, 11, dev)
    assert label.tolist() == [0, 0, 0, 0, 4, 5, 5, 5, 5, 9, 9] and counts.tolist() == [3, 1, 0]
    for kw in (dict(keep_largest=1), dict(min_faces=2), dict(), dict(keep_largest=2, smooth=2)):
        want = S.clean_mesh(verts, faces, **kw)
        got = S.clean_mesh(*on(dev, verts, faces), **kw)
        assert same_bits(host(got.verts), want.verts) and same_bits(host(got.faces), want.faces) and same_bits(host(got.src_vertex), want.src_vertex)
        assert got.report == want.report
    for pin in (True, False):
        smooth_matches(verts, faces, dev, 3, pin_boundary=pin)
    # V = 0 and T = 0
    none_f = np.zeros((0, 3), np.int32)
    components_match(none_f, 3, dev)
    components_match(none_f, 0, dev)
    for v in (verts[:3], verts[:0]):
        got = S.clean_mesh(*on(dev, v, none_f), keep_largest=1, smooth=1)
        assert got.verts.shape == (0, 3) and got.faces.shape == (0, 3) and got.src_vertex.shape == (0,) and got.report['components'] == 0
        assert same_bits(host(gnerf_hip.mesh_smooth(*on(dev, v, none_f), 2)), v)
    # a face that names a vertex outside [0, V) is counted, joins nothing, and the Python layer raises
    bad = np.array([[0, 1, 11], [1, 2, 1], [3, -1, 4]], np.int32)
    port = S.mesh_components_numpy(bad, 5, check=False)
    label, faces_of, counts = gnerf_hip._mesh_components_ctypes(on(dev, bad)[0], 5)
    assert same_bits(host(label), port[0]) and same_bits(host(faces_of), port[1]) and counts.tolist() == port[2].tolist() == [1, 3, 2]
    with pytest.raises(ValueError, match='outside'):
        gnerf_hip.mesh_components(on(dev, bad)[0], 5)


def test_many_components_over_many_workgroups(dev, meshes):
    import gnerf_hip
    verts, faces = meshes['noise48']
    port = components_match(faces, len(verts), dev)
    print(f'{len(verts)} vertices, {len(faces)} faces, {port[2][0]} components')
    assert port[2][0] > 1000 and len(faces) > 256 * 1000
    components_match(faces, len(verts), dev, port)                                          # a second run
    shuffled = faces[np.random.default_rng(1).permutation(len(faces))]
    label, faces_of, counts = gnerf_hip.mesh_components(on(dev, shuffled)[0], len(verts))
    assert same_bits(host(label), port[0]) and same_bits(host(faces_of), port[1]) and counts.tolist() == port[2].tolist()


def strip_faces(ids):
    """The triangle strip over the vertices ids[0], ids[1], ...: len(ids) - 2 faces."""
    return np.stack([ids[:-2], ids[1:-1], ids[2:]], axis=1).astype(np.int32)


def test_deep_chains_end_on_the_smallest_index(dev):
    import gnerf_hip
    rng = np.random.default_rng(8)
    n = 200002
    faces = strip_faces(rng.permutation(n))
    faces = faces[rng.permutation(len(faces))]
    label, faces_of, counts = gnerf_hip.mesh_components(on(dev, faces)[0], n)
    assert len(faces) == 200000 and int(label.max()) == 0 and counts.tolist() == [1, 0, 0] and int(faces_of[0]) == len(faces)
    # two strips interleaved: one on the even ids, one on the odd
    faces = np.concatenate([strip_faces(2 * rng.permutation(n)), strip_faces(2 * rng.permutation(n) + 1)])
    faces = faces[rng.permutation(len(faces))]
    label, faces_of, counts = gnerf_hip.mesh_components(on(dev, faces)[0], 2 * n)
    assert torch.equal(label.cpu(), torch.arange(2 * n, dtype=torch.int32) % 2) and counts.tolist() == [2, 0, 0]
    assert faces_of[:2].tolist() == [200000, 200000] and int(faces_of.sum()) == len(faces)


def test_one_hot_label_on_the_generator_mesh(dev):
    import gen_videos_mi355x as gv
    import gnerf_hip
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    vol = gv.extract_density_grid(G, gv.orbit_latents(G, z, dev), 512).permute(2, 1, 0).contiguous()
    verts, faces = S.marching_cubes(vol, 0.0)
    label, faces_of, counts = gnerf_hip.mesh_components(faces, len(verts))
    assert int(faces_of.sum()) == len(faces) > 10000 and int(counts[1]) == 0
    a = S.clean_mesh(verts, faces, keep_largest=1)
    b = S.clean_mesh(verts, faces, keep_largest=1)
    print(f'{len(verts)} vertices, {len(faces)} faces, {int(counts[0])} components; the largest holds {100 * a.report["share"]:.2f} % of the faces')
    assert a.report == b.report and a.report['kept'] == 1 and a.report['kept_faces'] == int(faces_of.max()) == len(a.faces)
    assert torch.equal(a.verts.view(torch.int32), b.verts.view(torch.int32)) and torch.equal(a.faces, b.faces) and torch.equal(a.src_vertex, b.src_vertex)
    assert torch.equal(a.verts.view(torch.int32), verts[a.src_vertex.long()].view(torch.int32))
    assert_closed_oriented(host(a.faces))
    assert gnerf_hip.mesh_components(a.faces, len(a.verts))[2].tolist() == [1, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- compaction
def test_compaction_matches_the_port(dev, meshes):
    verts, faces = meshes['random33']
    rng = np.random.default_rng(6)
    normals = rng.standard_normal((len(verts), 3)).astype(np.float32)
    colors = rng.integers(0, 256, (len(verts), 3), dtype=np.uint8)
    for kw in (dict(keep_largest=3), dict(min_faces=41), dict()):
        want = S.clean_mesh(verts, faces, normals=normals, colors=colors, **kw)
        got = S.clean_mesh(*on(dev, verts, faces), normals=on(dev, normals)[0], colors=on(dev, colors)[0], **kw)
        assert got.verts.is_cuda and got.faces.dtype == torch.int32 and got.src_vertex.dtype == torch.int32
        assert same_bits(host(got.verts), want.verts) and same_bits(host(got.faces), want.faces) and same_bits(host(got.src_vertex), want.src_vertex)
        assert same_bits(host(got.normals), want.normals) and same_bits(host(got.colors), want.colors) and got.report == want.report
        if kw:
            assert 0 < want.report['kept'] < want.report['components']
        else:                                                                               # everything kept: the input, bit for bit
            assert same_bits(host(got.verts), verts) and same_bits(host(got.faces), faces)


# ---------------------------------------------------------------------------------------------------------------- smoothing
def test_smoothing_matches_the_port_on_closed_and_open_meshes(dev, meshes):
    verts, faces = meshes['rough']
    smoothed = smooth_matches(verts, faces, dev, 10)
    assert np.any(smoothed != verts)
    smooth_matches(verts, faces, dev, 1, lam=0.3, mu=0.0, pin_boundary=False)
    smooth_matches(*meshes['noise48'], dev, 2)
    verts, faces = meshes['open']                                                           # no zero border: the surface is cut by the box
    _, _, _, odd = S._mesh_rows(faces, len(verts))
    assert 0 < odd.sum() < len(verts)
    pinned = smooth_matches(verts, faces, dev, 3)
    assert same_bits(pinned[odd], verts[odd]) and np.any(pinned != verts)
    free = smooth_matches(verts, faces, dev, 3, pin_boundary=False)
    assert np.any(free[odd] != verts[odd])


def test_smoothing_sorts_long_rows(dev):
    """A fan of 300 triangles round vertex 0: its row holds 600 neighbours (past the insertion sort), the rim's rows four."""
    rng = np.random.default_rng(12)
    ang = np.arange(300) * (2 * np.pi / 300)
    rim = np.stack([np.cos(ang) * 5, np.sin(ang) * 5, rng.standard_normal(300)], axis=1)
    verts = np.concatenate([[[0.3, -0.2, 2.0]], rim]).astype(np.float32)
    i = np.arange(300)
    faces = np.stack([np.zeros(300, np.int64), 1 + i, 1 + (i + 1) % 300], axis=1).astype(np.int32)
    faces = faces[rng.permutation(300)]
    pinned = smooth_matches(verts, faces, dev, 2)
    assert same_bits(pinned[1:], verts[1:]) and np.any(pinned[0] != verts[0])
    smooth_matches(verts, faces, dev, 2, pin_boundary=False)
    # rows on either side of the insertion sort's limit of 32 entries: fans of 15, 16, 17 and 40 triangles
    for n in (15, 16, 17, 40):
        smooth_matches(verts[:n + 1], np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], axis=1).astype(np.int32)[::-1], dev, 1)


def test_smoothing_grid_order_independence_and_zero_iterations(dev, meshes):
    import gnerf_hip
    verts, faces = grid_mesh(9)
    assert same_bits(smooth_matches(verts, faces, dev, 4), verts)
    assert np.any(smooth_matches(verts, faces, dev, 4, pin_boundary=False) != verts)
    verts, faces = meshes['random33']
    rng = np.random.default_rng(2)
    shuffled = np.roll(faces[rng.permutation(len(faces))], 1, axis=1)
    a = gnerf_hip.mesh_smooth(*on(dev, verts, faces), 2)
    b = gnerf_hip.mesh_smooth(*on(dev, verts, shuffled), 2)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and same_bits(host(a), S.mesh_smooth_numpy(verts, faces, 2))
    tv, tf = on(dev, verts, faces)
    same = gnerf_hip.mesh_smooth(tv, tf, 0)
    assert same_bits(host(same), verts) and same.data_ptr() != tv.data_ptr()
    assert same_bits(host(gnerf_hip.mesh_smooth(tv, tf, 2, lam=0.0, mu=0.0)), verts)
    with pytest.raises(ValueError):
        gnerf_hip.mesh_smooth(tv, tf, -1)


# ---------------------------------------------------------------------------------------------------------------- bindings
def test_pybind_and_ctypes_agree(dev, meshes):
    import gnerf_hip
    e = gnerf_hip.ext()
    assert e is not None and all(hasattr(e, n) for n in ('mesh_components', 'mesh_compact', 'mesh_smooth')), 'the pybind extension is built by csrc/build.sh'
    verts, faces = on(dev, *meshes['random33'])
    pl, pf, pc = e.mesh_components(faces, len(verts))
    cl, cf, cc = gnerf_hip._mesh_components_ctypes(faces, len(verts))
    assert torch.equal(pl, cl) and torch.equal(pf, cf) and torch.equal(pc, cc) and not pc.is_cuda
    keep = torch.zeros(len(verts), dtype=torch.uint8, device=dev)
    keep[torch.from_numpy(S.mesh_select(host(pf), keep_largest=5)).to(dev)] = 1
    pv, pt, ps, pn = e.mesh_compact(verts, faces, pl, pf, keep)
    cv, ct, cs, cn = gnerf_hip._mesh_compact_ctypes(verts, faces, cl, cf, keep)
    assert torch.equal(pn, cn) and pn.tolist() == [len(pv), len(pt)] and 0 < len(pv) < len(verts)
    assert torch.equal(pv.view(torch.int32), cv.view(torch.int32)) and torch.equal(pt, ct) and torch.equal(ps, cs)
    ps_ = e.mesh_smooth(pv, pt, 3, 0.5, -0.53, True)
    cs_ = gnerf_hip._mesh_smooth_ctypes(cv, ct, 3, 0.5, -0.53, True)
    assert torch.equal(ps_.view(torch.int32), cs_.view(torch.int32)) and not torch.equal(ps_, pv)
    # label and faces_of that do not belong together can keep a vertex and no face: both bindings hand back an empty face list
    tv, tf = on(dev, np.arange(12, dtype=np.float32).reshape(4, 3), np.array([[0, 1, 2]], np.int32))
    label, faces_of, keep = on(dev, np.array([0, 0, 0, 3], np.int32), np.array([1, 0, 0, 1], np.int32), np.array([0, 0, 0, 1], np.uint8))
    want = S.mesh_compact_numpy(host(tv), host(tf), host(label), host(faces_of), host(keep))
    assert want[0].shape == (1, 3) and want[1].shape == (0, 3) and want[2].tolist() == [3]
    for got in (e.mesh_compact(tv, tf, label, faces_of, keep), gnerf_hip._mesh_compact_ctypes(tv, tf, label, faces_of, keep)):
        assert got[3].tolist() == [1, 0] and all(same_bits(host(g), w) for g, w in zip(got[:3], want))


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_gen_videos_clean_mesh_end_to_end(dev, tmp_path):
    import gen_videos_mi355x as gv
    ply, npy = str(tmp_path / 'g.ply'), str(tmp_path / 'g.npy')
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.join(ROOT, 'g-nerf_amd'), ROOT, env.get('PYTHONPATH', '')])
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'g-nerf_amd', 'gen_videos_mi355x.py'), '--random-init', '--frames', '2', '--res', '32',
                        '--no-double-depth', '--voxel-res', '128', '--shapes', npy, '--mesh', ply, '--mesh-level', '0', '--mesh-keep', '1',
                        '--mesh-smooth', '2', '--mesh-attrs', 'all'],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count('mesh cleaning: kept 1 of ') == 1 and '2 Taubin iteration(s)' in r.stdout and 'mesh at level 0' in r.stdout
    vol = np.load(npy)
    verts, faces = S.read_ply(ply)
    mv, mf = S.marching_cubes_numpy(np.ascontiguousarray(vol.transpose(2, 1, 0)), 0.0)
    want = S.clean_mesh(mv, mf, keep_largest=1, smooth=2)
    assert same_bits(verts, want.verts) and np.array_equal(faces, want.faces) and len(faces) > 1000
    assert want.report['components'] > 1 and f'kept 1 of {want.report["components"]} component(s)' in r.stdout
    attrs = S.read_ply_attrs(ply)
    assert attrs['normals'].shape == verts.shape and attrs['colors'].shape == verts.shape and attrs['colors'].dtype == np.uint8
    length = np.linalg.norm(attrs['normals'].astype(np.float64), axis=1)
    assert np.all((np.abs(length - 1) < 1e-5) | (length == 0))
    # The attributes are those of the EXTRACTED surface at the kept vertices: what --mesh calls, with and without the flags, on one set of
    # planes (another process's planes need not have this one's bits) -- the cleaned file's attributes are the plain file's, gathered.
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    vol, planes = gv.extract_density_grid(G, gv.orbit_latents(G, z, dev), 128, return_planes=True)
    plain, cleaned = str(tmp_path / 'plain.ply'), str(tmp_path / 'cleaned.ply')
    gv.mesh_density_grid(vol, plain, 0.0, attrs='all', G=G, planes=planes)
    nv, nf, _ = written = gv.mesh_density_grid(vol, cleaned, 0.0, attrs='all', G=G, planes=planes, clean=S.clean_options(1, 0, 2))
    report = written.mesh.reports['clean']
    want = S.clean_mesh(*S.read_ply(plain), keep_largest=1, smooth=2)
    got_v, got_f = S.read_ply(cleaned)
    assert report == want.report and report['components'] > 1 and 0 < nv < report['vertices']
    assert same_bits(got_v, want.verts) and np.array_equal(got_f, want.faces)
    full, part = S.read_ply_attrs(plain), S.read_ply_attrs(cleaned)
    assert same_bits(part['normals'], full['normals'][want.src_vertex]) and same_bits(part['colors'], full['colors'][want.src_vertex])
