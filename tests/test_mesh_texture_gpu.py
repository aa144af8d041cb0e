"""GPU tests of the texture atlas (csrc/raster.hip: gnerf_mesh_bake_texture and gnerf_raster_resolve_textured, through gnerf_hip.bake_texture /
resolve_textured and shape_mi355x.bake_mesh_texture / render_mesh): the same bits as the numpy ports -- texels, weights, view counts and
resolved frames -- on the two squares, random soups and a sphere, across the patch sizes that change how texels fall onto waves; faces out of
range and empty meshes; both bindings, repeats and dirty buffers; graph capture together with the rasteriser; and gen_videos_mi355x.py
--mesh-texture end to end."""

import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import shape_mi355x as S
from test_mesh_bake_cpu import SPHERE_TOL, SQUARES_SIZE, bake_soup, orbit_views, random_frames, two_squares
from test_mesh_texture_cpu import decode_png
from test_raster_cpu import orbit_cameras, sphere_mesh
from test_raster_gpu import to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIS = (96, 96)
# P = 4: four cells to a wave; 5: 25 texels to a cell, cells straddle waves and the last workgroup is partial; 8: a cell is a wave; 16: a cell
# is four waves
PATCHES = (4, 5, 8, 16)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def differing(name, got, ref):
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    differ = a.view(np.uint8) != b.view(np.uint8)
    assert not differ.any(), f'{name}: {differ.sum()} of {differ.size} bytes differ, first at {np.argwhere(differ)[0].tolist()}'


def same_bits(dev, verts, faces, mesh2cam, intrinsics, vis, frames, patch, normals=None, normal_mat=None, fallback=None, resolve=True, **rules):
    """Kernel against port on texture, weight and seen, bit for bit, then the textured resolve of that texture from the same visibility buffers;
    returns the port's bake."""
    import gnerf_hip
    ref = S.bake_texture_numpy(verts, faces, mesh2cam, intrinsics, vis, frames, patch=patch, normals=normals, normal_mat=normal_mat, fallback=fallback, **rules)
    tv, tf, tA, tK, tvis, tfr, tn, tN, tfb = to_dev(dev, verts, faces, mesh2cam, intrinsics, vis.view(np.int64), frames, normals, normal_mat, fallback)
    got = gnerf_hip.bake_texture(tv, tf, tA, tK, tvis, tfr, patch=patch, normals=tn, normal_mat=tN, fallback=tfb, **rules)
    assert got['texture'].dtype == torch.uint8 and got['weight'].dtype == torch.float32 and got['seen'].dtype == torch.int32 and got['texture'].is_cuda
    for name in gnerf_hip.TEXTURE_OUTPUTS:
        differing(f'{name} (patch {patch}, {len(faces)} triangles, {rules})', got[name].cpu().numpy(), ref[name])
    if resolve:
        want = S.resolve_textured_numpy(vis, verts, faces, mesh2cam, intrinsics, ref['texture'], patch=patch, background=(3, 2, 1))
        frame = gnerf_hip.resolve_textured(tvis, tv, tf, tA, tK, got['texture'], patch=patch, background=(3, 2, 1))
        assert frame.dtype == torch.uint8 and frame.is_cuda
        differing(f'textured frame (patch {patch}, {len(faces)} triangles)', frame.cpu().numpy(), want)
    return ref


# ---------------------------------------------------------------------------------------------------------------- kernel = port
@pytest.mark.parametrize('patch', PATCHES)
def test_two_squares_match_the_port(dev, patch):
    verts, faces, is_back, pos, A, K = two_squares()                                    # 1490 triangles: the last row of cells is partly filled
    cells, th, tw = S.atlas_layout(len(faces), patch)
    assert ((len(faces) + 1) // 2) % cells != 0
    vis, _ = S.rasterize_numpy(verts, faces, A, K, SQUARES_SIZE)
    frames = random_frames(2, (32, 32), seed=4)
    fallback = random_frames(1, (len(verts),), seed=5)[0]
    for guard in (0, 1, 2):
        ref = same_bits(dev, verts, faces, A, K, vis, frames, patch, guard=guard, fallback=fallback if guard == 1 else None, background=(9, 8, 7))
        assert (ref['seen'] == 0).any() and (ref['seen'] == 1).any() and (ref['seen'] == 2).any() and (ref['seen'] == -1).any()
    normals = np.tile(np.array([[0, 0, -1]], dtype=np.float32), (len(verts), 1))      # facing the front camera, away from the one behind
    N = np.stack([np.eye(3, dtype=np.float32).reshape(9), np.diag([-1, 1, -1]).astype(np.float32).reshape(9)])
    ref = same_bits(dev, verts, faces, A, K, vis, frames, patch, normals=normals, normal_mat=N, power=3, guard=4)
    assert ref['seen'].max() == 1


SOUP_RULES = list(itertools.product((0, 1, 2), (False, True), (False, True)))          # guard, with normals, with fallback


@pytest.mark.parametrize('patch', PATCHES)
@pytest.mark.parametrize('n_tri', [1, 7, 50])
def test_random_soups_match_the_port(dev, n_tri, patch):
    verts, faces, normals, fallback = bake_soup(n_tri)                                  # (1 and 7 triangles: the last cell is half empty)
    seen_some = unseen_some = 0
    for n_views in (1, 3):
        A, K, N = orbit_views(n_views)
        vis, _ = S.rasterize_numpy(verts, faces, A, K, VIS)
        for k, (guard, with_normals, with_fallback) in enumerate(SOUP_RULES):
            frames = random_frames(n_views, (64, 64) if k % 2 else (96, 96), seed=n_tri + n_views + k)
            ref = same_bits(dev, verts, faces, A, K, vis, frames, patch, normals=normals if with_normals else None, normal_mat=N if with_normals else None,
                            fallback=fallback if with_fallback else None, guard=guard, background=(k, 2 * k, 255 - k), resolve=k in (1, 4))
            seen_some += int((ref['seen'] > 0).sum())
            unseen_some += int((ref['seen'] == 0).sum())
    assert seen_some > 0 and (unseen_some > 0 or n_tri == 1)


@pytest.fixture(scope='module')
def sphere():
    verts, faces, normals, mesh2world = sphere_mesh()
    A, K, N = orbit_views(3, mesh2world)
    vis, _ = S.rasterize_numpy(verts, faces, A, K, VIS)
    return dict(verts=verts, faces=faces, normals=normals, mesh2world=mesh2world, A=A, K=K, N=N, vis=vis, frames=random_frames(3, (96, 96), seed=9),
                fallback=random_frames(1, (len(verts),), seed=10)[0])


def test_sphere_matches_the_port(dev, sphere):
    s = sphere
    ref = same_bits(dev, s['verts'], s['faces'], s['A'], s['K'], s['vis'], s['frames'], 4, normals=s['normals'], normal_mat=s['N'], depth_tol=SPHERE_TOL,
                    fallback=s['fallback'])
    assert (ref['seen'] > 0).sum() > 5000 and (ref['seen'] == 0).sum() > 5000
    same_bits(dev, s['verts'], s['faces'], s['A'][:1], s['K'][:1], s['vis'][:1], s['frames'][:1, :64, :64].copy(), 8, guard=2, resolve=False)
    # bake_mesh_texture and render_mesh: rasterise + bake + textured resolve through the public entries, CUDA tensors in, tensors out
    cam2world, K33 = orbit_cameras()
    tv, tf, tn, tfr, tfb = to_dev(dev, s['verts'], s['faces'], s['normals'], s['frames'], s['fallback'])
    got = S.bake_mesh_texture(tv, tf, tfr, cam2world, K33, patch=4, mesh2world=s['mesh2world'], normals=tn, depth_tol=SPHERE_TOL, fallback=tfb)
    assert got['texture'].is_cuda
    for k in ('texture', 'weight', 'seen'):
        differing(k, got[k].cpu().numpy(), ref[k])
    drawn = S.render_mesh(tv, tf, cam2world, K33, VIS, mesh2world=s['mesh2world'], texture=got['texture'], patch=4, outputs=('frame', 'tri_id'))
    want = S.render_mesh(s['verts'], s['faces'], cam2world.numpy(), K33.numpy(), VIS, mesh2world=s['mesh2world'], texture=ref['texture'], patch=4,
                         outputs=('frame', 'tri_id'))
    assert drawn['frame'].is_cuda
    differing('frame', drawn['frame'].cpu().numpy(), want['frame'])
    differing('tri_id', drawn['tri_id'].cpu().numpy(), want['tri_id'])


def test_faces_out_of_range_and_empty_meshes(dev):
    import gnerf_hip
    from gnerf_hip import raster as R
    verts, faces, normals, fallback = bake_soup(50)
    faces = faces.copy()
    faces[3, 0], faces[10, 2], faces[49, 1] = len(verts), -1, 2 ** 30
    A, K, N = orbit_views(3)
    vis, _ = S.rasterize_numpy(verts, faces, A, K, VIS)
    frames = random_frames(3, (64, 64), seed=11)
    for patch in (5, 8):
        ref = same_bits(dev, verts, faces, A, K, vis, frames, patch, normals=normals, normal_mat=N, fallback=fallback, background=(11, 12, 13))
        tri = S._atlas_texels(len(faces), patch)[0]
        bad = np.isin(tri, (3, 10, 49))
        assert bad.sum() > 0 and np.all(ref['seen'][bad] == -1) and np.all(ref['texture'][bad] == np.array([11, 12, 13], dtype=np.uint8))
    tA, tK, tN, tvis, tfr = to_dev(dev, A, K, N, vis.view(np.int64), frames)
    no_verts, no_faces = torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev)
    rules = (0.01, 2.0 ** -8, 1, 0.1, 2)
    for out in (gnerf_hip.bake_texture(no_verts, no_faces, tA, tK, tvis, tfr), gnerf_hip.bake_texture(no_verts, no_faces, tA, tK, tvis, tfr, patch=5, normals=no_verts, normal_mat=tN),
                R._bake_texture_ctypes(no_verts, no_faces, 8, tA, tK, tvis, tfr, None, None, rules, None, (0, 0, 0))):
        assert tuple(out['texture'].shape) == (0, 0, 3) and tuple(out['weight'].shape) == (0, 0) and tuple(out['seen'].shape) == (0, 0)
        assert out['texture'].dtype == torch.uint8 and out['weight'].dtype == torch.float32 and out['seen'].dtype == torch.int32
    for frame in (gnerf_hip.resolve_textured(tvis, no_verts, no_faces, tA, tK, torch.zeros(0, 0, 3, dtype=torch.uint8, device=dev), background=(4, 5, 6)),
                  R._resolve_textured_ctypes(tvis, no_verts, no_faces, tA, tK, torch.zeros(0, 0, 3, dtype=torch.uint8, device=dev), 8, (4, 5, 6))):
        assert tuple(frame.shape) == (3, *VIS, 3) and bool((frame == torch.tensor([4, 5, 6], dtype=torch.uint8, device=dev)).all())
    # faces without a single vertex: every face is out of range, every texel the background
    tf = torch.from_numpy(faces).to(dev)
    out = gnerf_hip.bake_texture(no_verts, tf, tA, tK, tvis, tfr, background=(1, 1, 2))
    assert bool((out['seen'] == -1).all()) and bool((out['texture'] == torch.tensor([1, 1, 2], dtype=torch.uint8, device=dev)).all())


# ---------------------------------------------------------------------------------------------------------------- routes and repeats
def test_bindings_repeats_and_dirty_buffers(dev):
    import gnerf_hip
    from gnerf_hip import raster as R
    e = gnerf_hip.ext()
    assert e is not None and all(hasattr(e, name) for name in ('mesh_atlas_layout', 'mesh_bake_texture', 'raster_resolve_textured')), \
        'the pybind extension is built by csrc/build.sh'
    assert tuple(e.mesh_atlas_layout(7, 5)) == gnerf_hip.atlas_layout(7, 5) == (2, 10, 10)
    verts, faces, normals, fallback = bake_soup(257)
    A, K, N = orbit_views(3)
    vis, _ = S.rasterize_numpy(verts, faces, A, K, VIS)
    frames = random_frames(3, (64, 64), seed=5)
    tv, tf, tA, tK, tvis, tfr, tn, tN, tfb = to_dev(dev, verts, faces, A, K, vis.view(np.int64), frames, normals, N, fallback)
    rules, patch, bg = (0.01, 2.0 ** -8, 1, 0.1, 2), 5, [20, 30, 40]
    _, th, tw = gnerf_hip.atlas_layout(len(faces), patch)

    def same(a, b):
        return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in gnerf_hip.TEXTURE_OUTPUTS)
    kw = dict(patch=patch, normals=tn, normal_mat=tN, fallback=tfb, background=bg)
    first = gnerf_hip.bake_texture(tv, tf, tA, tK, tvis, tfr, **kw)
    assert int((first['seen'] > 0).sum()) >= 50 and int((first['seen'] == 0).sum()) >= 50 and int((first['seen'] < 0).sum()) >= 10
    assert same(first, R._bake_texture_ctypes(tv, tf, patch, tA, tK, tvis, tfr, tn, tN, rules, tfb, bg))      # the ctypes route
    assert same(first, gnerf_hip.bake_texture(tv, tf, tA, tK, tvis, tfr, **kw))                              # again
    for route in ('ext', 'ctypes'):                                                     # dirty outputs, through both bindings
        dirty = dict(texture=torch.full([th, tw, 3], 0x5A, dtype=torch.uint8, device=dev),
                     weight=torch.full([th, tw], 0x5A5A5A5A, dtype=torch.int32, device=dev).view(torch.float32),
                     seen=torch.full([th, tw], 0x5A5A5A5A, dtype=torch.int32, device=dev))
        if route == 'ext':
            got = gnerf_hip.bake_texture(tv, tf, tA, tK, tvis, tfr, out=dirty, **kw)
        else:
            got = R._bake_texture_ctypes(tv, tf, patch, tA, tK, tvis, tfr, tn, tN, rules, tfb, bg, **dirty)
        assert all(got[k].data_ptr() == dirty[k].data_ptr() for k in dirty) and same(first, got)
    frame = gnerf_hip.resolve_textured(tvis, tv, tf, tA, tK, first['texture'], patch=patch, background=bg)
    assert torch.equal(frame, R._resolve_textured_ctypes(tvis, tv, tf, tA, tK, first['texture'], patch, bg))
    assert torch.equal(frame, gnerf_hip.resolve_textured(tvis, tv, tf, tA, tK, first['texture'], patch=patch, background=bg))
    with pytest.raises(ValueError):
        gnerf_hip.bake_texture(tv, tf, tA, tK, tvis, tfr, out=dict(texture=torch.zeros(3, 3, 3, dtype=torch.uint8, device=dev)))
    with pytest.raises(ValueError):
        gnerf_hip.bake_texture(tv, tf, tA, tK, tvis[:2], tfr)
    with pytest.raises(ValueError):
        gnerf_hip.bake_texture(tv, tf, tA, tK, tvis, tfr, normals=tn)
    with pytest.raises(ValueError):
        gnerf_hip.resolve_textured(tvis, tv, tf, tA, tK, first['texture'], patch=patch + 1)


def test_graph_capture_of_rasterise_and_texture_bake_replays_with_new_cameras_and_frames(dev):
    import gnerf_hip
    verts, faces, normals, fallback = bake_soup(257)
    A, K, N = orbit_views(3)
    K2 = K.copy()
    K2[:, 0] *= 0.9                                                                    # another focal length too
    size = (64, 64)
    sets = [([2, 0, 1], K2, random_frames(3, size, seed=7)), ([0, 1, 2], K, random_frames(3, size, seed=8))]
    tv, tf, tn, tfb = to_dev(dev, verts, faces, normals, fallback)
    sA, sK, sN, sF = to_dev(dev, A, K, N, sets[0][2])
    ws = torch.empty(gnerf_hip.raster_workspace_bytes(len(verts), len(faces), 3, VIS), dtype=torch.uint8, device=dev)
    vis = torch.empty([3, *VIS], dtype=torch.int64, device=dev)
    _, th, tw = gnerf_hip.atlas_layout(len(faces), 8)
    out = dict(texture=torch.empty([th, tw, 3], dtype=torch.uint8, device=dev), weight=torch.empty([th, tw], device=dev),
               seen=torch.empty([th, tw], dtype=torch.int32, device=dev))

    def run():
        v, _ = gnerf_hip.rasterize(tv, tf, sA, sK, VIS, workspace=ws, vis=vis)
        return gnerf_hip.bake_texture(tv, tf, sA, sK, v, sF, normals=tn, normal_mat=sN, fallback=tfb, out=out)
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
        v, _ = gnerf_hip.rasterize(tv, tf, eA, eK, VIS)
        eager = gnerf_hip.bake_texture(tv, tf, eA, eK, v, eF, normals=tn, normal_mat=eN, fallback=tfb)
        port_vis, _ = S.rasterize_numpy(verts, faces, A[order], k, VIS)
        port = S.bake_texture_numpy(verts, faces, A[order], k, port_vis, frames, normals=normals, normal_mat=N[order], fallback=fallback)
        for name in gnerf_hip.TEXTURE_OUTPUTS:
            assert torch.equal(replayed[name].view(torch.uint8), eager[name].view(torch.uint8)), name
            differing(name, replayed[name].cpu().numpy(), port[name])
        assert (port['seen'] > 0).sum() >= 50
        results.append(replayed)
    assert not torch.equal(results[0]['texture'], results[1]['texture'])              # the two sets give different textures


# ---------------------------------------------------------------------------------------------------------------- end to end
# gen_videos_mi355x.py's own main() on the command line given after the first three arguments, with the texture flags.  Two runs of the CLI do
# not serve for the comparison of the .ply files: their volumes differ in the last bits (the backbone's library kernels are picked per run).
# So the run without the texture flags is made inside this one, at the point where the flags first matter: mesh_density_grid is called a
# second time with the volume, planes, frames and options of the first and bake['texture'] = 0, which is that call of a run without the flags.
# The texture, as finish_mesh's report holds it, is saved for the comparison with the PNG.
DRIVER = """
import sys
import numpy as np
import shape_mi355x as S
import gen_videos_mi355x as gv
plain, saved = sys.argv[1], sys.argv[2]
write = gv.mesh_density_grid
def both(vol, ply_path, level, **options):
    assert options['bake']['texture'] == 4
    write(vol, plain, level, **dict(options, bake=dict(options['bake'], texture=0)))
    written = write(vol, ply_path, level, **options)
    np.save(saved, S.to_host(written.mesh.reports['texture']['texture']))
    return written
gv.mesh_density_grid = both
sys.argv = ['gen_videos_mi355x.py'] + sys.argv[3:]
gv.main()
"""


def test_gen_videos_mesh_texture_end_to_end(dev, tmp_path):
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.join(ROOT, 'g-nerf_amd'), ROOT, env.get('PYTHONPATH', '')])
    plain, textured, saved = str(tmp_path / 'plain.ply'), str(tmp_path / 'textured.ply'), str(tmp_path / 'texture.npy')
    r = subprocess.run([sys.executable, '-c', DRIVER, plain, saved, '--random-init', '--frames', '4', '--res', '64', '--voxel-res', '64',
                        '--no-double-depth', '--mesh-level', '0', '--mesh-attrs', 'all', '--mesh-bake', '2', '--mesh', textured, '--mesh-texture', '4',
                        '--mesh-texture-out', str(tmp_path / 'textured.obj')],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(plain, 'rb').read() == open(textured, 'rb').read(), 'the texture flags changed the .ply'
    verts, faces = S.read_ply(textured)
    assert len(faces) > 100
    obj, mtl, png = (str(tmp_path / ('textured' + ext)) for ext in ('.obj', '.mtl', '.png'))
    assert all(os.path.isfile(p) for p in (obj, mtl, png))
    texture = np.load(saved)
    _, th, tw = S.atlas_layout(len(faces), 4)
    assert texture.shape == (th, tw, 3) and np.array_equal(decode_png(png)[1], texture)
    assert 'map_Kd textured.png' in open(mtl).read()
    rows = [line.split() for line in open(obj).read().split('\n') if line]
    kinds = [row[0] for row in rows]
    assert kinds.count('v') == len(verts) and kinds.count('vt') == 3 * len(faces) and kinds.count('f') == len(faces) and kinds.count('vn') == len(verts)
    f = np.array([[int(corner.split('/')[0]) for corner in row[1:]] for row in rows if row[0] == 'f'])
    assert np.array_equal(f, faces + 1)
    v = np.array([row[1:] for row in rows if row[0] == 'v'], dtype=np.float64).astype(np.float32)
    assert np.array_equal(v, verts)
    vt = np.array([row[1:] for row in rows if row[0] == 'vt'], dtype=np.float64)
    uvs = S.atlas_uvs(len(faces), 4).reshape(-1, 2).astype(np.float64)
    assert np.allclose(vt[:, 0], uvs[:, 0], atol=1e-7) and np.allclose(vt[:, 1], 1 - uvs[:, 1], atol=1e-7)
    line = [x for x in r.stdout.split('\n') if x.startswith('mesh texture: ')]
    assert len(line) == 1 and f'{tw} x {th} atlas (patch 4), 2 views' in line[0] and 'owned texels seen' in line[0] and 'views per seen texel' in line[0], r.stdout[-2000:]
    assert line[0].endswith(f'-> {obj}') and len(np.unique(texture.reshape(-1, 3), axis=0)) > 50
