"""GPU tests of the mesh-simplification kernels (csrc/mesh_simplify.hip through gnerf_hip.mesh_simplify / mesh_simplify_count and
shape_mi355x.simplify_mesh): the same bits as the numpy port on meshes of one and of many scan blocks, one cluster for everything and one per
vertex, reproducible and independent of the order of the faces, both bindings agree, invalid faces, and the rasteriser on the result."""

import numpy as np
import pytest
import torch

import shape_mi355x as S
from test_mesh_clean_cpu import four_balls_field, grid_mesh, largest_component, random_mesh, rough_sphere_field, same_bits
from test_mesh_simplify_cpu import ORIGIN, cube_mesh, face_set, shuffled

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def meshes():
    """Made once on the host and never changed."""
    made = {'random': random_mesh((33, 34, 35), 0.5), 'balls': S.marching_cubes_numpy(four_balls_field(), 0.0), 'grid': grid_mesh(9), 'cube': cube_mesh(8)}
    made['rough'] = largest_component(*S.marching_cubes_numpy(rough_sphere_field(), 0.0))
    for v, f in made.values():
        v.setflags(write=False)
        f.setflags(write=False)
    return made


def on(dev, *arrays):
    return tuple(torch.tensor(np.ascontiguousarray(a), device=dev) for a in arrays)


def host(t):
    return t.cpu().numpy()


def matches(got, want):
    """got: gnerf_hip.mesh_simplify's tuple (tensors), want: the port's (arrays) -- the same bits in all five."""
    v, f, src, vmap, counts = got
    assert v.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32 and src.dtype == torch.int32 and vmap.dtype == torch.int32
    assert not counts.is_cuda and counts.dtype == torch.int64
    assert counts.tolist() == want[4].tolist()
    assert same_bits(host(src), want[2]) and same_bits(host(vmap), want[3]) and same_bits(host(f), want[1])
    assert same_bits(host(v), want[0])


@pytest.mark.parametrize('name', ['random', 'balls', 'rough', 'grid', 'cube'])
def test_kernels_and_port_give_the_same_bits(dev, meshes, name):
    import gnerf_hip
    verts, faces = meshes[name]
    tv, tf = on(dev, verts, faces)
    for cell in (0.75, 2.0, 5.3):
        want = S.mesh_simplify_numpy(verts, faces, cell, ORIGIN)
        print(f'{name} at cell {cell}: {want[4].tolist()}')
        matches(gnerf_hip.mesh_simplify(tv, tf, cell, ORIGIN), want)
        assert gnerf_hip.mesh_simplify_count(tv, tf, cell, ORIGIN).tolist() == want[4].tolist()
    if name == 'random':
        assert len(faces) > 50 * 2048 and len(verts) > 20 * 2048            # many scan blocks; the grid and the cube fit in one
    if name in ('grid', 'cube'):
        assert len(faces) < 2048 and len(verts) < 2048


def test_one_cluster_for_everything_and_one_per_vertex(dev, meshes):
    import gnerf_hip
    # cell 100: every vertex of the four balls in one cluster (every atomic on the same 13 words), T' = 0 and no out_faces
    verts, faces = meshes['balls']
    want = S.mesh_simplify_numpy(verts, faces, 100.0, ORIGIN)
    assert want[4].tolist() == [1, 0, 0, len(faces), 0, 0, 0, 0]
    got = gnerf_hip.mesh_simplify(*on(dev, verts, faces), 100.0, ORIGIN)
    matches(got, want)
    assert got[1].shape == (0, 3) and host(got[3]).tolist() == [0] * len(verts)
    matches(gnerf_hip._mesh_simplify_ctypes(*on(dev, verts, faces), 100.0, [float(np.float32(x)) for x in ORIGIN]), want)
    # cell 2^-6 on the cube: every vertex its own cluster, every face its own group -- the fullest tables
    verts, faces = meshes['cube']
    want = S.mesh_simplify_numpy(verts, faces, 2.0 ** -6, ORIGIN)
    assert want[4].tolist() == [len(verts), len(faces), 0, 0, 0, 0, 0, 0]
    matches(gnerf_hip.mesh_simplify(*on(dev, verts, faces), 2.0 ** -6, ORIGIN), want)
    # V = 0 and T = 0
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    for v in (verts, none_v):
        matches(gnerf_hip.mesh_simplify(*on(dev, v, none_f), 1.0, ORIGIN), S.mesh_simplify_numpy(v, none_f, 1.0, ORIGIN))
    matches(gnerf_hip.mesh_simplify(*on(dev, none_v, faces), 1.0, ORIGIN), S.mesh_simplify_numpy(none_v, faces, 1.0, ORIGIN))


def test_reproducible_order_independent_and_the_same_through_both_bindings(dev, meshes):
    import gnerf_hip
    verts, faces = meshes['random']
    tv, tf = on(dev, verts, faces)
    origin = [float(np.float32(x)) for x in ORIGIN]
    first = gnerf_hip.mesh_simplify(tv, tf, 2.0, ORIGIN)
    again = gnerf_hip.mesh_simplify(tv, tf, 2.0, ORIGIN)
    other = gnerf_hip._mesh_simplify_ctypes(tv, tf, 2.0, origin)
    for a in (again, other):
        assert all(same_bits(host(x), host(y)) for x, y in zip(first, a))
    mixed = gnerf_hip.mesh_simplify(tv, on(dev, shuffled(faces, 5))[0], 2.0, ORIGIN)
    assert same_bits(host(mixed[0]), host(first[0])) and same_bits(host(mixed[2]), host(first[2])) and same_bits(host(mixed[3]), host(first[3]))
    assert mixed[4].tolist() == first[4].tolist() and np.array_equal(face_set(host(mixed[1])), face_set(host(first[1])))


def test_invalid_faces_and_a_nan_vertex_are_counted_and_skipped(dev, meshes):
    import gnerf_hip
    verts, faces = meshes['balls']
    verts, faces = verts.copy(), faces.copy()
    verts[100, 2] = np.nan
    verts[200, 0] = np.inf
    faces[5, 1] = len(verts)
    faces[6, 0] = -1
    faces[7, 2] = faces[7, 0]
    want = S.mesh_simplify_numpy(verts, faces, 2.0, ORIGIN)
    assert want[4][2] > 4 and want[3][100] == -1 and want[3][200] == -1
    for route in (gnerf_hip.mesh_simplify, lambda v, f, c, o: gnerf_hip._mesh_simplify_ctypes(v, f, c, [float(np.float32(x)) for x in o])):
        matches(route(*on(dev, verts, faces), 2.0, ORIGIN), want)


def test_simplify_mesh_end_to_end_and_the_rasteriser_on_its_result(dev, meshes):
    import gen_videos_mi355x as gv
    import gnerf_harness as H
    verts, faces = meshes['balls']
    rng = np.random.default_rng(2)
    normals, colors = rng.standard_normal((len(verts), 3)).astype(np.float32), rng.integers(0, 256, (len(verts), 3), dtype=np.uint8)
    for kw in (dict(cell=2.0), dict(target_faces=1000), dict(cell=0.7, target_faces=300, origin=ORIGIN)):
        want = S.simplify_mesh(verts, faces, normals=normals, colors=colors, **kw)
        got = S.simplify_mesh(*on(dev, verts, faces), normals=on(dev, normals)[0], colors=on(dev, colors)[0], **kw)
        assert got.verts.is_cuda and got.report == want.report
        for a, b in zip(got[:6], want[:6]):
            assert same_bits(host(a), b)
    want = S.simplify_mesh(verts, faces, cell=2.0)
    got = S.simplify_mesh(*on(dev, verts, faces), cell=2.0)
    labels = H.orbit_labels(range(2), 2, 2.7)
    cams = labels[:, :16].reshape(-1, 4, 4).numpy(), labels[:, 16:].reshape(-1, 3, 3).numpy()
    kw = dict(mesh2world=gv.mesh_to_world_matrix(48, 1.0), outputs=('tri_id', 'depth'))
    drawn, ref = S.render_mesh(got.verts, got.faces, *cams, 48, **kw), S.render_mesh(want.verts, want.faces, *cams, 48, **kw)
    assert same_bits(host(drawn['tri_id']), ref['tri_id']) and same_bits(host(drawn['depth']), ref['depth'])
    assert (ref['tri_id'] >= 0).mean() > 0.02 and drawn['counts'].tolist() == ref['counts'].tolist()


def test_finish_mesh_on_the_device_gives_the_numpy_routes_bits(dev, meshes):
    """The pipeline's stages that need no generator, on CUDA tensors: verts, faces and reports of the numpy route."""
    verts, faces = meshes['balls']
    clean, simplify = S.clean_options(2, 0, 3), S.simplify_options(3.0, 0)
    want = S.finish_mesh(verts, faces, clean=clean, simplify=simplify)
    got = S.finish_mesh(*on(dev, verts, faces), clean=clean, simplify=simplify)
    assert got.verts.is_cuda and got.faces.is_cuda and same_bits(host(got.verts), want.verts) and same_bits(host(got.faces), want.faces)
    assert list(got.reports) == ['clean', 'simplify'] and got.reports == want.reports and 0 < len(want.faces) < len(faces)
