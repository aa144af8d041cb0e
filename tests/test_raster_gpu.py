"""GPU tests of the triangle rasteriser (csrc/raster.hip through gnerf_hip.rasterize / resolve and shape_mi355x.render_mesh): the same bits as
the numpy port -- visibility keys (ids and z), tri_id, depth, normal, frame and the counts -- on hand cases, random soups, the queued route for
large triangles and a sphere; independence of the triangles' order; both bindings; repeats, dirty buffers, graph capture; and
gen_videos_mi355x.py --geometry-out end to end."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gnerf_harness as H
import shape_mi355x as S
from test_raster_cpu import EMPTY, PIXEL_CAMERA, at_pixels, fan_scene, orbit_cameras, sphere_mesh, square_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHADING = dict(light=(0.3, -0.4, -0.8660254), ambient=0.2, diffuse=0.9, albedo=(0.9, 0.7, 0.5), background=(0.1, 0.2, 0.3))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def to_dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def same_bits(dev, verts, faces, A, K, size, near=0.01, cull='none', normals=None, normal_mat=None, colors=None, shading=SHADING, port=None):
    """Kernel against port: vis, counts and every resolved image, bit for bit.  port: a (vis, counts) the caller already has.  Returns the
    kernel's (vis, counts, images) as numpy and the port's images."""
    import gnerf_hip
    ref_vis, ref_counts = port if port is not None else S.rasterize_numpy(verts, faces, A, K, size, near=near, cull=cull)
    ref = S.resolve_numpy(ref_vis, verts, faces, A, K, normals=normals, normal_mat=normal_mat, colors=colors, shading=shading)
    tv, tf, tA, tK, tn, tN, tc = to_dev(dev, verts, faces, A, K, normals, normal_mat, colors)
    vis, counts = gnerf_hip.rasterize(tv, tf, tA, tK, size, near=near, cull=cull)
    assert vis.dtype == torch.int64 and counts.dtype == torch.int64 and vis.is_cuda
    got = gnerf_hip.resolve(vis, tv, tf, tA, tK, normals=tn, normal_mat=tN, colors=tc, shading=shading)
    vis_np = vis.cpu().numpy().view(np.uint64)
    assert counts.cpu().numpy().tolist() == ref_counts.tolist(), (counts.cpu().numpy().tolist(), ref_counts.tolist())
    wrong = vis_np != ref_vis
    assert not wrong.any(), f'{wrong.sum()} of {wrong.size} visibility keys differ, first at {np.argwhere(wrong)[0].tolist()}: ' \
                            f'{vis_np[wrong][0]:#018x} != {ref_vis[wrong][0]:#018x}'
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert got['tri_id'].dtype == np.int32 and got['depth'].dtype == np.float32 and got['normal'].dtype == np.float32 and got['frame'].dtype == np.uint8
    for name in ('tri_id', 'depth', 'normal', 'frame'):
        differ = bits(got[name]) != bits(ref[name])
        assert not differ.any(), f'{name}: {differ.sum()} of {differ.size} values differ, first at {np.argwhere(differ)[0].tolist()}: ' \
                                 f'{got[name][differ][0]!r} != {ref[name][differ][0]!r}'
    return vis_np, counts.cpu().numpy(), got, ref


def cameras(n_views):
    cam2world, K = orbit_cameras((0, 40, 80)[:n_views])
    A, N = S.mesh_to_camera(cam2world.numpy())
    return A.reshape(-1, 12), K.numpy().reshape(-1, 9), N.reshape(-1, 9)


def soup(n_tri, seed, smallest=0.002, largest=0.3):
    """Random triangles in the unit box around the origin, sizes log-uniform: mostly micro-triangles, some spanning many pixels."""
    rng = np.random.default_rng(seed)
    centre = rng.random((n_tri, 1, 3)) * 0.5 - 0.25
    scale = np.exp(rng.uniform(np.log(smallest), np.log(largest), (n_tri, 1, 1)))
    verts = (centre + (rng.random((n_tri, 3, 3)) - 0.5) * scale).reshape(-1, 3).astype(np.float32)
    faces = np.arange(n_tri * 3, dtype=np.int32).reshape(-1, 3)
    normals = rng.standard_normal((n_tri * 3, 3)).astype(np.float32)
    colors = rng.integers(0, 256, (n_tri * 3, 3), dtype=np.uint8)
    return verts, faces, normals, colors


# ---------------------------------------------------------------------------------------------------------------- hand cases
@pytest.mark.parametrize('scene', [square_scene, fan_scene], ids=['square8', 'fan16'])
def test_hand_cases_match_the_port(dev, scene):
    verts, faces, ring, size = scene()
    for f in (faces, faces[:, ::-1].copy(), np.concatenate([faces, faces[:, ::-1]])):
        for cull in ('none', 'back', 'front'):
            same_bits(dev, verts, f, *PIXEL_CAMERA, size, cull=cull)
    for k in range(len(faces)):                                                       # one triangle at a time: the fill rule's owners
        same_bits(dev, verts, faces[k:k + 1], *PIXEL_CAMERA, size)


def test_sub_pixel_triangles_match_the_port(dev):
    f = np.array([[0, 1, 2]], dtype=np.int32)
    for size in (8, 16):
        vis, counts, got, _ = same_bits(dev, at_pixels([(3.6, 3.6), (3.9, 3.6), (3.6, 3.9)], size), f, *PIXEL_CAMERA, size)
        assert np.all(vis == EMPTY) and counts.tolist() == [1, 0, 0, 0]
        vis, counts, got, _ = same_bits(dev, at_pixels([(3.3, 3.3), (3.8, 3.4), (3.4, 3.8)], size), f, *PIXEL_CAMERA, size)
        assert (got['tri_id'] >= 0).sum() == 1 and got['tri_id'][0, 3, 3] == 0


def test_empty_meshes_are_background(dev):
    import gnerf_hip
    A, K = to_dev(dev, *PIXEL_CAMERA)
    some_v = torch.from_numpy(at_pixels([(1.5, 1.5), (6.5, 1.5), (1.5, 6.5)], 8)).to(dev)
    empty_v, empty_f = torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev)
    for v, f in ((empty_v, empty_f), (some_v, empty_f), (empty_v, torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev))):
        vis, counts = gnerf_hip.rasterize(v, f, A, K, (8, 11))
        assert vis.shape == (1, 8, 11) and bool((vis == -1).all()) and counts.tolist() == [0, 0, 0, 0]
        out = gnerf_hip.resolve(vis, v, f, A, K, shading=dict(background=(0.0, 0.5, 1.0)))
        assert bool((out['tri_id'] == -1).all()) and bool(torch.isposinf(out['depth']).all()) and bool((out['normal'] == 0).all())
        assert bool((out['frame'] == torch.tensor([0, 128, 255], dtype=torch.uint8, device=dev)).all())


# ---------------------------------------------------------------------------------------------------------------- random soups
@pytest.mark.parametrize('n_tri', [1, 63, 64, 65, 257, 2000])
def test_random_soups_match_the_port(dev, n_tri):
    size = (37, 53)
    verts, faces, normals, colors = soup(n_tri, seed=n_tri)
    for n_views in (1, 3):
        A, K, N = cameras(n_views)
        ports = {}
        for cull in ('none', 'back', 'front'):
            ports[cull] = S.rasterize_numpy(verts, faces, A, K, size, cull=cull)
            assert ports[cull][1].sum() == n_views * n_tri
            same_bits(dev, verts, faces, A, K, size, cull=cull, port=ports[cull])
            same_bits(dev, verts, faces, A, K, size, cull=cull, normals=normals, normal_mat=N, colors=colors, port=ports[cull])
        same_bits(dev, verts, faces, A, K, size, normals=normals, normal_mat=N, port=ports['none'])
        same_bits(dev, verts, faces, A, K, size, colors=colors, port=ports['none'])
        if n_tri >= 257:
            assert (ports['none'][0] != EMPTY).sum() > 100


# ---------------------------------------------------------------------------------------------------------------- the queued route
def box_pixels(verts, faces, A, K, size):
    """Pixel centres in each triangle's clipped bounding box (0 for a dropped one): what chooses between the two routes."""
    _, iz, X, Y, bad = S._raster_project(verts, A, K, size, size, 0.01)
    return S._raster_setup(faces, len(verts), X, Y, iz, bad, 0, size, size)['npx']


def test_large_triangles_match_the_port(dev):
    import gnerf_hip
    size, small = 64, gnerf_hip.RASTER_SMALL_PIXELS
    assert small == 64
    f = np.array([[0, 1, 2]], dtype=np.int32)

    def corner(x0, y0, bw, bh, z=1.0):                     # a right triangle whose clipped bounding box holds bw x bh centres
        return at_pixels([(x0, y0, z), (x0 + bw, y0, z), (x0, y0 + bh, z)], size)
    vis, counts, got, _ = same_bits(dev, at_pixels([(-10, -10), (200, -10), (-10, 200)], size), f, *PIXEL_CAMERA, size)
    assert (got['tri_id'] == 0).all() and counts.tolist() == [1, 0, 0, 0]                        # the whole image
    for bw, bh in ((7, 9), (8, 8), (5, 13), (9, 7), (13, 5), (1, 44), (44, 1), (54, 44)):        # small - 1, small, small + 1 pixels, and others
        tri = corner(10.0, 20.0, bw, bh)
        assert box_pixels(tri, f, PIXEL_CAMERA[0][0], PIXEL_CAMERA[1][0], size).tolist() == [bw * bh]
        vis, counts, got, _ = same_bits(dev, tri, f, *PIXEL_CAMERA, size)
        rows, cols = np.nonzero(got['tri_id'][0] >= 0)
        assert counts[0] == 1 and cols.min() == 10 and rows.min() == 20 and cols.max() <= 10 + bw - 1 and rows.max() <= 20 + bh - 1
    same_bits(dev, at_pixels([(40, 40), (160, 30), (50, 170)], size), f, *PIXEL_CAMERA, size)              # three quarters off-screen
    same_bits(dev, at_pixels([(-300, 5), (30, 20), (-200, 90)], size), f, *PIXEL_CAMERA, size)
    vis, counts, _, _ = same_bits(dev, at_pixels([(5, 5), (9000, 20), (5, 60)], size), f, *PIXEL_CAMERA, size)
    assert counts.tolist() == [0, 0, 1, 0] and np.all(vis == EMPTY)                              # a vertex past the guard band
    vis, counts, _, _ = same_bits(dev, at_pixels([(5, 5, 1.0), (60, 20, 0.005), (5, 60, 1.0)], size), f, *PIXEL_CAMERA, size)
    assert counts.tolist() == [0, 1, 0, 0] and np.all(vis == EMPTY)                              # a vertex behind near
    # 300 triangles of both routes, three views, attributes
    verts, faces, normals, colors = soup(300, seed=11, smallest=0.01, largest=0.6)
    A, K, N = cameras(3)
    t = box_pixels(verts, faces, A[0], K[0], size)
    assert (t > small).sum() > 20 and ((t > 0) & (t <= small)).sum() > 20, 'the soup mixes both routes'
    for cull in ('none', 'back'):
        same_bits(dev, verts, faces, A, K, size, cull=cull, normals=normals, normal_mat=N, colors=colors)


# ---------------------------------------------------------------------------------------------------------------- sphere
@pytest.fixture(scope='module')
def sphere(dev):
    verts, faces, normals, mesh2world = sphere_mesh()
    cam2world, K = orbit_cameras()
    A, N = S.mesh_to_camera(cam2world.numpy(), mesh2world)
    return verts, faces, normals, A.reshape(-1, 12), K.numpy().reshape(-1, 9), N.reshape(-1, 9), cam2world, mesh2world


def test_sphere_matches_the_port(dev, sphere):
    verts, faces, normals, A, K, N, cam2world, mesh2world = sphere
    vis, counts, got, _ = same_bits(dev, verts, faces, A, K, 96, normals=normals, normal_mat=N)
    hit = got['tri_id'] >= 0
    assert hit.sum() > 3 * 4000 and counts.tolist() == [3 * len(faces), 0, 0, 0]
    assert np.all(got['tri_id'][hit] < len(faces)) and np.all(got['tri_id'][~hit] == -1)
    assert np.all(np.isposinf(got['depth'][~hit])) and np.all(np.isfinite(got['depth'][hit]))
    # render_mesh: the same through the public entry, CUDA tensors in, tensors out
    tv, tf, tn = to_dev(dev, verts, faces, normals)
    out = S.render_mesh(tv, tf, cam2world, torch.from_numpy(K).reshape(-1, 3, 3), 96, mesh2world=mesh2world, normals=tn, shading=SHADING)
    assert out['frame'].is_cuda and np.array_equal(out['frame'].cpu().numpy(), got['frame']) and out['counts'].tolist() == counts.tolist()
    assert np.array_equal(bits(out['depth'].cpu().numpy()), bits(got['depth']))


def test_the_order_of_the_triangles_does_not_matter(dev):
    import gnerf_hip
    size = (37, 53)
    verts, faces, normals, colors = soup(500, seed=21)
    A, K, N = cameras(3)
    perm = np.random.default_rng(5).permutation(len(faces))
    tv, tn, tc, tA, tK, tN = to_dev(dev, verts, normals, colors, A, K, N)
    outs = []
    for f in (faces, faces[perm]):
        tf = torch.from_numpy(np.ascontiguousarray(f)).to(dev)
        vis, counts = gnerf_hip.rasterize(tv, tf, tA, tK, size)
        smooth = gnerf_hip.resolve(vis, tv, tf, tA, tK, normals=tn, normal_mat=tN, colors=tc, shading=SHADING)
        flat = gnerf_hip.resolve(vis, tv, tf, tA, tK, shading=SHADING, outputs=('frame', 'normal'))
        outs.append((counts.cpu().numpy(), {k: v.cpu().numpy() for k, v in smooth.items()}, {k: v.cpu().numpy() for k, v in flat.items()}))
    (c0, s0, f0), (c1, s1, f1) = outs
    assert c0.tolist() == c1.tolist()
    assert np.array_equal(bits(s0['depth']), bits(s1['depth']))
    hit = s0['tri_id'] >= 0
    assert hit.sum() > 500 and np.array_equal(hit, s1['tri_id'] >= 0)
    moved = perm[s1['tri_id'][hit]] != s0['tri_id'][hit]
    for view, r, c in np.argwhere(hit)[moved]:                                        # only where two triangles tie in depth
        a, b = faces[s0['tri_id'][view, r, c]], faces[perm[s1['tri_id'][view, r, c]]]
        za, zb = (S.rasterize_numpy(verts, t[None], A[view:view + 1], K[view:view + 1], size)[0][0, r, c] >> np.uint64(32) for t in (a, b))
        assert za == zb
    if not moved.any():
        assert np.array_equal(s0['frame'], s1['frame']) and np.array_equal(f0['frame'], f1['frame'])
        assert np.array_equal(bits(s0['normal']), bits(s1['normal'])) and np.array_equal(bits(f0['normal']), bits(f1['normal']))
    assert moved.sum() <= 2


# ---------------------------------------------------------------------------------------------------------------- routes and repeats
def test_bindings_repeats_and_dirty_buffers(dev):
    import gnerf_hip
    from gnerf_hip import raster as R
    e = gnerf_hip.ext()
    assert e is not None and hasattr(e, 'raster_visibility') and hasattr(e, 'raster_resolve'), 'the pybind extension is built by csrc/build.sh'
    size = (64, 64)
    verts, faces, normals, colors = soup(300, seed=11, smallest=0.01, largest=0.6)
    A, K, N = cameras(3)
    tv, tf, tn, tc, tA, tK, tN = to_dev(dev, verts, faces, normals, colors, A, K, N)
    sh = gnerf_hip.shading_vector(SHADING)

    def same(a, b):
        return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))
    vis, counts = gnerf_hip.rasterize(tv, tf, tA, tK, size)
    out = gnerf_hip.resolve(vis, tv, tf, tA, tK, normals=tn, normal_mat=tN, colors=tc, shading=SHADING)
    first = [vis, counts] + [out[k] for k in gnerf_hip.RASTER_OUTPUTS]
    # the ctypes route
    cvis, ccounts = R._rasterize_ctypes(tv, tf, tA, tK, 64, 64, 0.01, 0)
    cout = R._resolve_ctypes(cvis, tv, tf, tA, tK, tn, tN, tc, sh, gnerf_hip.RASTER_OUTPUTS)
    assert same(first, [cvis, ccounts] + [cout[k] for k in gnerf_hip.RASTER_OUTPUTS])
    # again
    vis2, counts2 = gnerf_hip.rasterize(tv, tf, tA, tK, size)
    out2 = gnerf_hip.resolve(vis2, tv, tf, tA, tK, normals=tn, normal_mat=tN, colors=tc, shading=SHADING)
    assert same(first, [vis2, counts2] + [out2[k] for k in gnerf_hip.RASTER_OUTPUTS])
    # dirty workspace and vis, through both bindings
    nbytes = gnerf_hip.raster_workspace_bytes(len(verts), len(faces), 3, size)
    for route in ('ext', 'ctypes'):
        ws = torch.full([nbytes], 0x5A, dtype=torch.uint8, device=dev)
        dirty = torch.full([3, 64, 64], 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
        if route == 'ext':
            vis3, counts3 = gnerf_hip.rasterize(tv, tf, tA, tK, size, workspace=ws, vis=dirty)
        else:
            vis3, counts3 = R._rasterize_ctypes(tv, tf, tA, tK, 64, 64, 0.01, 0, workspace=ws, vis=dirty)
        assert vis3.data_ptr() == dirty.data_ptr() and same([vis, counts], [vis3, counts3])
    # a subset of the outputs
    only = gnerf_hip.resolve(vis, tv, tf, tA, tK, outputs=('depth',))
    assert list(only) == ['depth'] and same([only['depth']], [out['depth']])


def test_graph_capture_replays_with_new_cameras(dev):
    import gnerf_hip
    size = (37, 53)
    verts, faces, normals, colors = soup(257, seed=31)
    A, K, N = cameras(3)
    tv, tf, tn, tc = to_dev(dev, verts, faces, normals, colors)
    first = [0, 1, 2]
    other = [2, 0, 1]
    K2 = K.copy()
    K2[:, 0] *= 0.9                                                                    # another focal length too
    sA, sK, sN = to_dev(dev, A[first], K, N[first])
    ws = torch.empty(gnerf_hip.raster_workspace_bytes(len(verts), len(faces), 3, size), dtype=torch.uint8, device=dev)
    vis = torch.empty([3, *size], dtype=torch.int64, device=dev)

    def run():
        v, counts = gnerf_hip.rasterize(tv, tf, sA, sK, size, workspace=ws, vis=vis)
        out = gnerf_hip.resolve(v, tv, tf, sA, sK, normals=tn, normal_mat=sN, colors=tc, shading=SHADING)
        return [v, counts] + [out[k] for k in gnerf_hip.RASTER_OUTPUTS]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run()
    results = []
    for order, k in ((other, K2), (first, K)):
        sA.copy_(torch.from_numpy(A[order]).to(dev))
        sK.copy_(torch.from_numpy(k).to(dev))
        sN.copy_(torch.from_numpy(N[order]).to(dev))
        graph.replay()
        replayed = [t.clone() for t in static]
        eA, eK, eN = to_dev(dev, A[order], k, N[order])
        v, counts = gnerf_hip.rasterize(tv, tf, eA, eK, size)
        out = gnerf_hip.resolve(v, tv, tf, eA, eK, normals=tn, normal_mat=eN, colors=tc, shading=SHADING)
        eager = [v, counts] + [out[name] for name in gnerf_hip.RASTER_OUTPUTS]
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(replayed, eager))
        results.append(replayed)
    assert not torch.equal(results[0][0], results[1][0])                              # the two sets of cameras give different images
    port_vis, port_counts = S.rasterize_numpy(verts, faces, A, K, size)
    assert np.array_equal(replayed[0].cpu().numpy().view(np.uint64), port_vis) and replayed[1].tolist() == port_counts.tolist()


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_gen_videos_geometry_end_to_end(dev, tmp_path):
    import gen_videos_mi355x as gv
    geo, ply = str(tmp_path / 'geo.npy'), str(tmp_path / 'g.ply')
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.join(ROOT, 'g-nerf_amd'), ROOT, env.get('PYTHONPATH', '')])
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'g-nerf_amd', 'gen_videos_mi355x.py'), '--random-init', '--frames', '4', '--res', '64',
                        '--voxel-res', '64', '--geometry-res', '64', '--geometry-out', geo, '--no-double-depth', '--mesh', ply, '--mesh-level', '0',
                        '--frames-per-call', '3'],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'geometry frames: 4 at 64x64' in r.stdout and r.stdout.count('density volume 64^3') == 1
    frames = np.load(geo)
    assert frames.shape == (4, 64, 64, 3) and frames.dtype == np.uint8 and len(np.unique(frames)) > 10
    verts, faces = S.read_ply(ply)
    assert len(faces) > 100
    labels = H.orbit_labels(range(4), 4, 2.7)
    want = S.render_mesh(verts, faces, labels[:, :16].reshape(-1, 4, 4).numpy(), labels[:, 16:].reshape(-1, 3, 3).numpy(), 64,
                         mesh2world=gv.mesh_to_world_matrix(64, 1.0), outputs=('frame',))
    assert np.array_equal(frames, want['frame'])
    assert (frames != 255).any(axis=-1).mean() > 0.02                                 # the mesh is in view
