"""GPU tests of the multi-view colour bake (csrc/raster.hip, gnerf_mesh_bake_colors, through gnerf_hip.bake_colors and
shape_mi355x.bake_mesh_colors): the same bits as the numpy port -- colours, weights and view counts -- on the two squares, random soups
across the wave and workgroup edges and a sphere; empty meshes; both bindings, repeats and dirty buffers; graph capture together with the
rasteriser; and gen_videos_mi355x.py --mesh-bake end to end."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gnerf_harness as H
import shape_mi355x as S
from test_mesh_bake_cpu import FRAME_SIZE, SOUPS, SPHERE_TOL, SQUARES_SIZE, VIS_SIZE, bake_soup, orbit_views, random_frames, soup_cases, two_squares
from test_raster_cpu import sphere_mesh
from test_raster_gpu import to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def same_bits(dev, verts, mesh2cam, intrinsics, vis, frames, normals=None, normal_mat=None, fallback=None, **rules):
    """Kernel against port on colors, weight (as uint32) and seen, bit for bit; returns the port's result."""
    import gnerf_hip
    ref = S.bake_colors_numpy(verts, mesh2cam, intrinsics, vis, frames, normals=normals, normal_mat=normal_mat, fallback=fallback, **rules)
    tv, tA, tK, tvis, tf, tn, tN, tfb = to_dev(dev, verts, mesh2cam, intrinsics, vis.view(np.int64), frames, normals, normal_mat, fallback)
    got = gnerf_hip.bake_colors(tv, tA, tK, tvis, tf, normals=tn, normal_mat=tN, fallback=tfb, **rules)
    assert got['colors'].dtype == torch.uint8 and got['weight'].dtype == torch.float32 and got['seen'].dtype == torch.int32 and got['colors'].is_cuda
    assert tuple(got['colors'].shape) == (len(verts), 3) and tuple(got['weight'].shape) == (len(verts),) and tuple(got['seen'].shape) == (len(verts),)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    for name, view in (('seen', np.int32), ('weight', np.uint32), ('colors', np.uint8)):
        differ = got[name].view(view) != ref[name].view(view)
        assert not differ.any(), f'{name}: {differ.sum()} of {differ.size} values differ, first at {np.argwhere(differ)[0].tolist()}: ' \
                                 f'{got[name][differ][0]!r} != {ref[name][differ][0]!r}'
    return ref


# ---------------------------------------------------------------------------------------------------------------- kernel = port
def test_two_squares_match_the_port(dev):
    verts, faces, is_back, pos, A, K = two_squares()
    vis, _ = S.rasterize_numpy(verts, faces, A, K, SQUARES_SIZE)
    frames = random_frames(2, (32, 32), seed=4)
    for guard in (0, 1, 2, 4):
        ref = same_bits(dev, verts, A, K, vis, frames, guard=guard)
        assert (ref['seen'] == 0).any() and (ref['seen'] == 1).any() and ((ref['seen'] == 2).any() or guard == 4)
    normals = np.tile(np.array([[0, 0, -1]], dtype=np.float32), (len(verts), 1))      # facing the front camera, away from the one behind
    N = np.stack([np.eye(3, dtype=np.float32).reshape(9), np.diag([-1, 1, -1]).astype(np.float32).reshape(9)])
    ref = same_bits(dev, verts, A, K, vis, frames, normals=normals, normal_mat=N, power=3)
    assert ref['seen'].max() == 1 and (ref['seen'][~is_back] == 1).all()


@pytest.mark.parametrize('n_tri', SOUPS)
def test_random_soups_match_the_port(dev, n_tri):
    for case in soup_cases(n_tri):
        same_bits(dev, **case)
    # the other rules, once per soup: no fallback, another tolerance, the widest window, min_cos and every power
    verts, faces, normals, fallback = bake_soup(n_tri)
    A, K, N = orbit_views(3)
    vis, _ = S.rasterize_numpy(verts, faces, A, K, VIS_SIZE)
    frames = random_frames(3, FRAME_SIZE, seed=n_tri)
    same_bits(dev, verts, A, K, vis, frames, depth_tol=0.0, guard=0)
    same_bits(dev, verts, A, K, vis, frames, depth_tol=0.25, guard=4, near=2.6)
    for power in range(9):
        same_bits(dev, verts, A, K, vis, frames, normals=normals, normal_mat=N, power=power, min_cos=-0.5 if power % 2 == 0 else 0.3, guard=0)


def test_sphere_matches_the_port(dev):
    verts, faces, normals, mesh2world = sphere_mesh()
    A, K, N = orbit_views(3, mesh2world)
    vis, _ = S.rasterize_numpy(verts, faces, A, K, 96)
    frames = random_frames(3, (96, 96), seed=9)
    fallback = random_frames(1, (len(verts),), seed=10)[0]
    for kw in (dict(), dict(normals=normals, normal_mat=N), dict(normals=normals, normal_mat=N, depth_tol=SPHERE_TOL, fallback=fallback)):
        ref = same_bits(dev, verts, A, K, vis, frames, **kw)
        assert (ref['seen'] > 0).sum() > 1500 and (ref['seen'] == 0).sum() > 1500
    # bake_mesh_colors: rasterise + bake through the public entry, CUDA tensors in, tensors out, against the ports in a row
    from test_raster_cpu import orbit_cameras
    cam2world, K33 = orbit_cameras()
    tv, tf, tn, tfr, tfb = to_dev(dev, verts, faces, normals, frames, fallback)
    got = S.bake_mesh_colors(tv, tf, tfr, cam2world, K33, mesh2world=mesh2world, normals=tn, depth_tol=SPHERE_TOL, fallback=tfb)
    assert got['colors'].is_cuda
    for k in ('colors', 'weight', 'seen'):
        assert np.array_equal(got[k].cpu().numpy().view(np.uint8), ref[k].view(np.uint8)), k


def test_empty_mesh_returns_empty_tensors(dev):
    import gnerf_hip
    from gnerf_hip import raster as R
    A, K, N = orbit_views(2)
    tA, tK, tN = to_dev(dev, A, K, N)
    vis = torch.full([2, 8, 8], -1, dtype=torch.int64, device=dev)
    frames = torch.zeros([2, 8, 8, 3], dtype=torch.uint8, device=dev)
    empty = torch.zeros(0, 3, device=dev)
    for out in (gnerf_hip.bake_colors(empty, tA, tK, vis, frames), gnerf_hip.bake_colors(empty, tA, tK, vis, frames, normals=empty, normal_mat=tN),
                R._bake_colors_ctypes(empty, tA, tK, vis, frames, None, None, (0.01, 2.0 ** -8, 1, 0.1, 2), None)):
        assert tuple(out['colors'].shape) == (0, 3) and tuple(out['weight'].shape) == (0,) and tuple(out['seen'].shape) == (0,)
        assert out['colors'].dtype == torch.uint8 and out['weight'].dtype == torch.float32 and out['seen'].dtype == torch.int32


# ---------------------------------------------------------------------------------------------------------------- routes and repeats
def test_bindings_repeats_and_dirty_buffers(dev):
    import gnerf_hip
    from gnerf_hip import raster as R
    e = gnerf_hip.ext()
    assert e is not None and hasattr(e, 'mesh_bake_colors'), 'the pybind extension is built by csrc/build.sh'
    verts, faces, normals, fallback = bake_soup(2000)
    A, K, N = orbit_views(3)
    vis, _ = S.rasterize_numpy(verts, faces, A, K, VIS_SIZE)
    frames = random_frames(3, FRAME_SIZE, seed=5)
    tv, tA, tK, tvis, tf, tn, tN, tfb = to_dev(dev, verts, A, K, vis.view(np.int64), frames, normals, N, fallback)
    rules = (0.01, 2.0 ** -8, 1, 0.1, 2)

    def same(a, b):
        return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in gnerf_hip.BAKE_OUTPUTS)
    first = gnerf_hip.bake_colors(tv, tA, tK, tvis, tf, normals=tn, normal_mat=tN, fallback=tfb)
    assert int((first['seen'] > 0).sum()) >= 50 and int((first['seen'] == 0).sum()) >= 50
    assert same(first, R._bake_colors_ctypes(tv, tA, tK, tvis, tf, tn, tN, rules, tfb))           # the ctypes route
    assert same(first, gnerf_hip.bake_colors(tv, tA, tK, tvis, tf, normals=tn, normal_mat=tN, fallback=tfb))      # again
    for route in ('ext', 'ctypes'):                                                     # dirty outputs, through both bindings
        dirty = dict(colors=torch.full([len(verts), 3], 0x5A, dtype=torch.uint8, device=dev),
                     weight=torch.full([len(verts)], 0x5A5A5A5A, dtype=torch.int32, device=dev).view(torch.float32),
                     seen=torch.full([len(verts)], 0x5A5A5A5A, dtype=torch.int32, device=dev))
        if route == 'ext':
            got = gnerf_hip.bake_colors(tv, tA, tK, tvis, tf, normals=tn, normal_mat=tN, fallback=tfb, out=dirty)
        else:
            got = R._bake_colors_ctypes(tv, tA, tK, tvis, tf, tn, tN, rules, tfb, **dirty)
        assert all(got[k].data_ptr() == dirty[k].data_ptr() for k in dirty) and same(first, got)
    with pytest.raises(ValueError):
        gnerf_hip.bake_colors(tv, tA, tK, tvis, tf, out=dict(colors=torch.zeros(3, 3, dtype=torch.uint8, device=dev)))
    with pytest.raises(ValueError):
        gnerf_hip.bake_colors(tv, tA, tK, tvis[:2], tf)
    with pytest.raises(ValueError):
        gnerf_hip.bake_colors(tv, tA, tK, tvis, tf, normals=tn)
    with pytest.raises(ValueError):
        gnerf_hip.bake_colors(tv, tA, tK, tvis, tf, fallback=tfb[:5])


def test_graph_capture_of_rasterise_and_bake_replays_with_new_cameras_and_frames(dev):
    import gnerf_hip
    verts, faces, normals, fallback = bake_soup(257)
    A, K, N = orbit_views(3)
    K2 = K.copy()
    K2[:, 0] *= 0.9                                                                    # another focal length too
    sets = [([2, 0, 1], K2, random_frames(3, FRAME_SIZE, seed=7)), ([0, 1, 2], K, random_frames(3, FRAME_SIZE, seed=8))]
    tv, tf, tn, tfb = to_dev(dev, verts, faces, normals, fallback)
    sA, sK, sN, sF = to_dev(dev, A, K, N, sets[0][2])
    ws = torch.empty(gnerf_hip.raster_workspace_bytes(len(verts), len(faces), 3, VIS_SIZE), dtype=torch.uint8, device=dev)
    vis = torch.empty([3, *VIS_SIZE], dtype=torch.int64, device=dev)
    out = dict(colors=torch.empty([len(verts), 3], dtype=torch.uint8, device=dev), weight=torch.empty([len(verts)], device=dev),
               seen=torch.empty([len(verts)], dtype=torch.int32, device=dev))

    def run():
        v, _ = gnerf_hip.rasterize(tv, tf, sA, sK, VIS_SIZE, workspace=ws, vis=vis)
        return gnerf_hip.bake_colors(tv, sA, sK, v, sF, normals=tn, normal_mat=sN, fallback=tfb, out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run()
    results = []
    for order, k, frames in sets:
        sA.copy_(torch.from_numpy(A[order]).to(dev))
        sK.copy_(torch.from_numpy(k).to(dev))
        sN.copy_(torch.from_numpy(N[order]).to(dev))
        sF.copy_(torch.from_numpy(frames).to(dev))
        graph.replay()
        replayed = {name: t.clone() for name, t in static.items()}
        eA, eK, eN, eF = to_dev(dev, A[order], k, N[order], frames)
        v, _ = gnerf_hip.rasterize(tv, tf, eA, eK, VIS_SIZE)
        eager = gnerf_hip.bake_colors(tv, eA, eK, v, eF, normals=tn, normal_mat=eN, fallback=tfb)
        port_vis, _ = S.rasterize_numpy(verts, faces, A[order], k, VIS_SIZE)
        port = S.bake_colors_numpy(verts, A[order], k, port_vis, frames, normals=normals, normal_mat=N[order], fallback=fallback)
        for name in gnerf_hip.BAKE_OUTPUTS:
            assert torch.equal(replayed[name].view(torch.uint8), eager[name].view(torch.uint8)), name
            assert np.array_equal(replayed[name].cpu().numpy().view(np.uint8), port[name].view(np.uint8)), name
        assert (port['seen'] > 0).sum() >= 50
        results.append(replayed)
    assert not torch.equal(results[0]['colors'], results[1]['colors'])                # the two sets give different colours


# ---------------------------------------------------------------------------------------------------------------- end to end
# gen_videos_mi355x.py's own main() on the command line given after the first argument, with one recorder around mesh_vertex_attributes: the
# decoder's colours (the bake's fallback) are saved as they come back.  Two runs of the CLI do not serve: their vertices differ in the
# last bits (the backbone's library kernels are picked per process).
DRIVER = """
import sys
import numpy as np
import gen_videos_mi355x as gv
path, inner = sys.argv[1], gv.mesh_vertex_attributes
def recording(*args, **kw):
    normals, colors = inner(*args, **kw)
    np.save(path, colors.cpu().numpy())
    return normals, colors
gv.mesh_vertex_attributes = recording
sys.argv = ['gen_videos_mi355x.py'] + sys.argv[2:]
gv.main()
"""


def test_gen_videos_mesh_bake_end_to_end(dev, tmp_path):
    import gen_videos_mi355x as gv
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.join(ROOT, 'g-nerf_amd'), ROOT, env.get('PYTHONPATH', '')])
    ply, out, fallback = str(tmp_path / 'g.ply'), str(tmp_path / 'frames.npy'), str(tmp_path / 'decoder.npy')
    r = subprocess.run([sys.executable, '-c', DRIVER, fallback, '--random-init', '--frames', '4', '--res', '64', '--voxel-res', '64', '--no-double-depth',
                        '--mesh', ply, '--mesh-level', '0', '--mesh-attrs', 'all', '--mesh-bake', '2', '--out', out],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'mesh bake: 2 views, ' in r.stdout and 'vertices seen' in r.stdout and 'views per seen vertex' in r.stdout, r.stdout[-2000:]
    (verts, faces), attrs = S.read_ply(ply), S.read_ply_attrs(ply)
    normals, colors, decoder = attrs['normals'], attrs['colors'], np.load(fallback)
    assert len(faces) > 100 and decoder.shape == colors.shape and decoder.dtype == np.uint8
    frames = np.load(out)
    assert frames.shape == (4, 512, 512, 3) and frames.dtype == np.uint8
    labels = H.orbit_labels([0, 2], 4, 2.7)
    want = S.bake_mesh_colors(verts, faces, frames[[0, 2]], labels[:, :16].reshape(-1, 4, 4).numpy(), labels[:, 16:25].reshape(-1, 3, 3).numpy(),
                              mesh2world=gv.mesh_to_world_matrix(64, 1.0), normals=normals, fallback=decoder)
    seen = want['seen'] > 0
    print(S.bake_report_line(want, 2))
    assert seen.sum() > 100 and np.array_equal(colors, want['colors'])
    assert (colors != decoder).any() and np.array_equal(colors[~seen], decoder[~seen])
    assert S.bake_report_line(want, 2) in r.stdout
