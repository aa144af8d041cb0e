"""GPU tests of the brick-wise band mesh (csrc/mesh_band_cubes.hip): the kernels against the numpy port, same bytes, on volumes that hold NaN
wherever the band never evaluated; against the dense marching-cubes kernel at a size that leaves one tile of every scan; the generator route
(extract_band_mesh against extract_density_grid(band=...) + mesh_of_density_grid), the finished mesh, and the CLI's --mesh-direct.  The CPU
fields and the port's results are those of tests/band_mesh_cases.py, made once."""

import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import shape_mi355x as S
from band_mesh_cases import BRICKS, FIELDS, VIEWS, band_run, case_field
from conftest import has_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the per-workgroup tiles of the scans in csrc/mesh_band_cubes.hip: kItems segments per block of the segment prefix (csrc/mesh_scan.h), and
# kScanThreads brick columns per tile of the column scan.  A third scan, scan_block_counts in bmc_totals_kernel, takes the blocks' totals in
# tiles of kMcScanThreads = 1024 blocks = 2 M segments: no quick case leaves its first tile (n = 130 has some 40 blocks), so in this unit its
# carry across tiles is reached only by tools/bench_band_mesh.py's n = 1024 sphere; the code is csrc/mesh_cubes.h's, which csrc/mesh.hip's
# dense tests take past one tile (a 128^3 volume has 1024 blocks of 2048 points, a 512^3 one 65 536).
SEGMENTS_PER_BLOCK = 2048
COLUMNS_PER_TILE = 1024
LARGEST_SCAN_TILE = max(SEGMENTS_PER_BLOCK, COLUMNS_PER_TILE)


@pytest.fixture(scope='module')
def dev():
    if not has_gpu():
        pytest.fail('GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)')
    import gnerf_hip
    gnerf_hip.load()
    assert gnerf_hip.band_mesh_available()
    return torch.device('cuda', 0)


def same_tensors(a, b):
    """Same shapes, dtypes and bits (floats are compared as their int32 patterns)."""
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize('binding', [None, 'ctypes'])
@pytest.mark.parametrize('s', BRICKS)
@pytest.mark.parametrize('name', list(FIELDS))
def test_kernels_give_the_ports_bits(dev, name, s, binding):
    """Vertices, faces and the four counts in the three views, twice, on a volume that is NaN wherever the band's lists never pointed."""
    import gnerf_hip
    assert binding == 'ctypes' or gnerf_hip.ext() is not None
    run = band_run(name, s)
    n, level, keep = run['n'], run['level'], run['keep']
    dense_dev = torch.from_numpy(np.array(case_field(name)[0]).reshape(-1)).to(dev)

    def dev_field(index, out):
        out[index.long()] = dense_dev[index.long()]

    vol = torch.full([n ** 3], float('nan'), dtype=torch.float32, device=dev)
    band = gnerf_hip.BandVolume(vol, n, s, level, keep, binding=binding)
    report = S._band_driver(n, s, lambda index: dev_field(index, vol) if len(index) else None, torch.from_numpy(S.band_coarse_index(n, s)).to(dev), band, None,
                            fill=False)
    assert report == run['report'] and np.array_equal(band.state.cpu().numpy(), run['state'])
    evaluated = ~torch.isnan(vol)
    assert int(evaluated.sum()) == report['points'] and bool(evaluated.reshape(n, n, n)[torch.from_numpy(np.array(run['visited'])).to(dev)].all())
    active = int(run['state'].sum())
    for view, (perm, flip) in VIEWS.items():
        want = S.band_marching_cubes_numpy(run['raw'], run['state'], n, s, level, keep, perm, flip, return_counts=True)
        for given in (active, None, active):                             # (None: the wrapper counts the active bricks itself)
            verts, faces, counts = gnerf_hip.band_marching_cubes(vol, band.state, n, s, level, keep, perm, flip, binding=binding, active=given,
                                                                 return_counts=True)
            assert verts.is_cuda and faces.is_cuda and not counts.is_cuda
            assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and counts.dtype == torch.int64
            assert counts.tolist() == want[2].tolist(), view
            assert verts.cpu().numpy().tobytes() == want[0].tobytes() and tuple(verts.shape) == want[0].shape, view
            assert faces.cpu().numpy().tobytes() == want[1].tobytes() and tuple(faces.shape) == want[1].shape, view


@pytest.mark.parametrize('binding', [None, 'ctypes'])
def test_band_mesh_on_the_device(dev, binding):
    """shape_mi355x.band_mesh end to end on an uninitialised volume: the port's mesh and report; a non-finite value is counted only where it is
    seen; bad arguments are refused."""
    import gnerf_hip
    run = band_run('rough_sphere', 4)
    n, level, keep = run['n'], run['level'], run['keep']
    dense_dev = torch.from_numpy(np.array(run['dense']).reshape(-1)).to(dev)
    perm, flip = VIEWS['pipeline']
    want = S.band_marching_cubes_numpy(run['raw'], run['state'], n, 4, level, keep, perm, flip)
    verts, faces, report = S.band_mesh(lambda index, out: out.__setitem__(index.long(), dense_dev[index.long()]), n, level, 4, keep, perm, flip, device=dev,
                                       binding=binding)
    assert verts.cpu().numpy().tobytes() == want[0].tobytes() and faces.cpu().numpy().tobytes() == want[1].tobytes()
    assert {k: report[k] for k in run['report']} == run['report']
    assert report['active'] == int(run['state'].sum()) and report['visited'] == int(run['visited'].sum()) and report['mesh'] == (len(want[0]), len(want[1]))

    state = torch.from_numpy(np.array(run['state'])).to(dev)
    i = np.arange(n)
    kept = S._band_kept(S._band_geometry(n, 4, keep)[3], i[:, None, None], i[None, :, None], i[None, None, :])
    inside, outside = np.argwhere(run['visited'] & kept), np.argwhere(run['visited'] & ~kept)
    vol = np.array(run['raw']).reshape(n, n, n)
    vol[tuple(outside[len(outside) // 2])] = np.nan                       # visited but cropped away: not counted
    got = gnerf_hip.band_marching_cubes(torch.from_numpy(vol.reshape(-1)).to(dev), state, n, 4, level, keep, perm, flip, binding=binding)
    assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and got[1].cpu().numpy().tobytes() == want[1].tobytes()
    vol[tuple(inside[len(inside) // 2])] = np.nan
    vol[tuple(inside[0])] = np.inf
    bad = torch.from_numpy(vol.reshape(-1)).to(dev)
    want_bad = S.band_marching_cubes_numpy(vol.reshape(-1), run['state'], n, 4, level, keep, perm, flip, return_counts=True)
    verts, faces, counts = gnerf_hip.band_marching_cubes(bad, state, n, 4, level, keep, perm, flip, binding=binding, return_counts=True)
    assert counts.tolist() == want_bad[2].tolist() and counts[2] == 2 and verts.shape == (0, 3) and faces.shape == (0, 3)
    with pytest.raises(ValueError, match='non-finite'):
        gnerf_hip.band_marching_cubes(bad, state, n, 4, level, keep, perm, flip, binding=binding)

    good = torch.from_numpy(np.array(run['raw'])).to(dev)
    with pytest.raises(ValueError, match='brick edge'):
        gnerf_hip.band_marching_cubes(good, state, n, 3, level, binding=binding)
    with pytest.raises(ValueError, match='permutation'):
        gnerf_hip.band_marching_cubes(good, state, n, 4, level, perm=(0, 2, 2), binding=binding)
    with pytest.raises(ValueError):
        gnerf_hip.band_marching_cubes(good[:-1], state, n, 4, level, binding=binding)
    for value in (2, 3):
        odd = state.clone()
        odd[len(odd) // 2] = value
        with pytest.raises(ValueError, match='0 or 1'):
            gnerf_hip.band_marching_cubes(good, odd, n, 4, level, binding=binding)
    with pytest.raises(ValueError, match='more active bricks'):
        gnerf_hip.band_marching_cubes(good, state, n, 4, level, binding=binding, active=int(state.sum()) - 1)
    lib = gnerf_hip.load()
    import ctypes
    nbytes = ctypes.c_size_t()
    assert lib.gnerf_band_mesh_workspace_bytes(n, 5, 1, ctypes.byref(nbytes)) != 0 and b'brick edge' in lib.gnerf_last_error()
    assert lib.gnerf_band_mesh_workspace_bytes(1300, 4, 1, ctypes.byref(nbytes)) != 0 and b'2^31' in lib.gnerf_last_error()
    empty = gnerf_hip.band_marching_cubes(good, torch.zeros_like(state), n, 4, level, binding=binding)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)


@pytest.mark.parametrize('binding', [None, 'ctypes'])
def test_band_mesh_raises_on_a_non_finite_value_it_sees(dev, binding):
    """band_mesh on the device, like the route it replaces: a NaN or Inf at a visited, kept point raises; the same value where the crop zeroes
    it changes nothing."""
    run = band_run('rough_sphere', 4)
    n, level, keep = run['n'], run['level'], run['keep']
    i = np.arange(n)
    kept = S._band_kept(keep, i[:, None, None], i[None, :, None], i[None, None, :])
    coarse = np.zeros((n, n, n), dtype=bool)
    coarse.reshape(-1)[S.band_coarse_index(n, 4)] = True
    inside = np.argwhere(run['visited'] & kept & ~coarse)                 # (not a coarse point: the seeds stay as they are)
    outside = np.argwhere(run['visited'] & ~kept)
    perm, flip = VIEWS['pipeline']
    want = S.band_marching_cubes_numpy(run['raw'], run['state'], n, 4, level, keep, perm, flip)
    for value in (float('nan'), float('inf')):
        flat = torch.from_numpy(np.array(run['dense']).reshape(-1)).to(dev)
        flat[int(np.ravel_multi_index(tuple(outside[len(outside) // 2]), (n, n, n)))] = value

        def dev_field(index, out):
            out[index.long()] = flat[index.long()]

        verts, faces, _ = S.band_mesh(dev_field, n, level, 4, keep, perm, flip, device=dev, binding=binding)
        assert verts.cpu().numpy().tobytes() == want[0].tobytes() and faces.cpu().numpy().tobytes() == want[1].tobytes()
        flat[int(np.ravel_multi_index(tuple(inside[len(inside) // 2]), (n, n, n)))] = value
        with pytest.raises(ValueError, match='non-finite'):
            S.band_mesh(dev_field, n, level, 4, keep, perm, flip, device=dev, binding=binding)


@pytest.mark.parametrize('s', [2, 4])
def test_kernels_against_the_dense_kernel(dev, s):
    """A rough sphere and a small ball at n = 130: more active bricks than any scan's tile holds, compared with gnerf_hip.marching_cubes of
    the filled, cropped, flipped and permuted volume.  No numpy port at this size."""
    import gnerf_hip
    n, level = 130, 0.0
    i = torch.arange(n, dtype=torch.float32, device=dev)
    x, y, z = torch.meshgrid(i, i, i, indexing='ij')
    rough = 1.5 * torch.sin(0.37 * x + 0.2 * y) * torch.cos(0.29 * y - 0.1 * z) + 0.8 * torch.sin(0.53 * z + 0.3 * x)
    sphere = 47.3 - torch.sqrt((x - 63.4) ** 2 + (y - 66.1) ** 2 + (z - 64.7) ** 2) + rough
    ball = 9.2 - torch.sqrt((x - 118.3) ** 2 + (y - 112.6) ** 2 + (z - 14.9) ** 2)
    dense = torch.maximum(sphere, ball).reshape(-1).contiguous()
    keep = [(4, 126), (22, 128), (3, 104)]                               # cuts the sphere on two sides

    def dev_field(index, out):
        out[index.long()] = dense[index.long()]

    perm, flip = VIEWS['pipeline']
    filled, report = S.band_volume(dev_field, n, level, s, keep, device=dev)
    cropped = torch.zeros_like(filled)
    sl = tuple(slice(lo, hi) for lo, hi in keep)
    cropped[sl] = filled[sl]
    want = gnerf_hip.marching_cubes(cropped.flip([a for a in range(3) if flip[a]]).permute(*perm).contiguous(), level)
    runs = [S.band_mesh(dev_field, n, level, s, keep, perm, flip, device=dev) for _ in range(2)]
    for verts, faces, direct in runs:
        assert {k: direct[k] for k in report} == report
        assert direct['active'] > LARGEST_SCAN_TILE and len(verts) > 2048 and direct['mesh'] == (len(want[0]), len(want[1]))
        assert (-(-(n - 1) // s)) ** 2 > COLUMNS_PER_TILE and direct['visited'] < 0.5 * n ** 3
        assert same_tensors((verts, faces), want)
    label, _, _ = gnerf_hip.mesh_components(want[1], len(want[0]))
    assert len(torch.unique(label)) >= 2                                 # the small ball is there


@pytest.fixture(scope='module')
def model(dev):
    """tests/test_mesh_band_gpu.py's random-init generator on the GPU with its planes, and a level at which its 64^3 volume has a mesh: the
    median of the volume's kept region."""
    import gnerf_generator
    import gen_videos_mi355x as gv
    torch.manual_seed(5)
    G = gnerf_generator.Generator().eval().requires_grad_(False)
    with torch.no_grad():
        ws = G.mapping(torch.randn(1, 512), torch.zeros(1, 25))
        G = copy.deepcopy(G).to(dev)
        ws = ws.to(dev)
        planes = G.backbone.synthesis(ws, noise_mode='const')
        planes = planes.view(len(planes), 3, 32, planes.shape[-2], planes.shape[-1])
        dense = gv.extract_density_grid(G, ws, resolution=64, crop=True, planes=planes)
    (a0, b0), (a1, b1), (a2, b2) = gv.crop_ranges(64)
    level = float(dense[a0:64 - b0, a1:64 - b1, a2:64 - b2].median())
    return dict(G=G, ws=ws, planes=planes, level=level)


@pytest.mark.parametrize('crop', [True, False])
@pytest.mark.parametrize('band', [4, 8])
def test_extract_band_mesh_is_the_band_route(dev, model, band, crop):
    import gen_videos_mi355x as gv
    G, ws, planes, level = model['G'], model['ws'], model['planes'], model['level']
    reports, direct_reports = {}, {}
    with torch.no_grad():
        vol = gv.extract_density_grid(G, ws, resolution=64, crop=crop, planes=planes, band=band, level=level, report=reports)
        want, _ = gv.mesh_of_density_grid(vol, level)
        verts, faces = gv.extract_band_mesh(G, ws, 64, level, band, crop=crop, planes=planes, report=direct_reports)
    assert len(want.faces) > 0 and verts.is_cuda and same_tensors((verts, faces), (want.verts, want.faces))
    report = direct_reports['band']
    assert {k: report[k] for k in reports['band']} == reports['band'] and report['mesh'] == (len(verts), len(faces))


def test_finished_mesh_from_the_direct_mesh(dev, model):
    import gen_videos_mi355x as gv
    G, ws, planes, level = model['G'], model['ws'], model['planes'], model['level']
    reports, direct_reports = {}, {}
    stages = dict(attrs='all', G=G, planes=planes, clean=S.clean_options(keep_largest=1, smooth=2))
    with torch.no_grad():
        vol = gv.extract_density_grid(G, ws, resolution=64, planes=planes, band=8, level=level, report=reports)
        want, _ = gv.mesh_of_density_grid(vol, level, band=reports['band'], **stages)
        verts, faces = gv.extract_band_mesh(G, ws, 64, level, 8, planes=planes, report=direct_reports)
        mesh, _ = gv.mesh_of_density_grid(gv.DirectMesh(verts, faces, 64), level, band=direct_reports['band'], **stages)
    assert list(mesh.reports) == list(want.reports) and list(mesh.reports)[0] == 'band' and mesh.reports['band'] is direct_reports['band']
    assert len(want.faces) > 0 and want.normals is not None and want.colors is not None
    assert same_tensors((mesh.verts, mesh.faces, mesh.normals, mesh.colors), (want.verts, want.faces, want.normals, want.colors))


# gen_videos_mi355x.py's own main() on each command line of the list given as the second argument, in one process: a refused command line
# prints "EXIT <code>" and the next one runs.  Two runs of the CLI do not serve for the comparison of the .ply files: their planes differ in the
# last bits (the backbone's library kernels are picked per run).  So the run without the flag is made inside the run with it, at the point where
# the flag first matters: when mesh_density_grid is handed the direct mesh, the volume of --mesh-band alone is made from the same planes and
# written first, with the same options -- that call of a run without the flag.
DRIVER = r'''
import json, sys
import gen_videos_mi355x as gv
plain = sys.argv[1]
seen = {}
extract, write = gv.extract_band_mesh, gv.mesh_density_grid
def recorded(G, ws, resolution, level, band, **kw):
    seen.update(G=G, ws=ws, resolution=resolution, level=level, band=band)
    return extract(G, ws, resolution, level, band, **kw)
def both(vol, ply_path, level, **options):
    assert isinstance(vol, gv.DirectMesh) and level == seen['level']
    volume = gv.extract_density_grid(seen['G'], seen['ws'], seen['resolution'], planes=options['planes'], band=seen['band'], level=level)
    write(volume, plain, level, **options)
    return write(vol, ply_path, level, **options)
gv.extract_band_mesh, gv.mesh_density_grid = recorded, both
for argv in json.loads(sys.argv[2]):
    sys.argv = ['gen_videos_mi355x.py'] + argv
    try:
        gv.main()
    except SystemExit as e:
        print('EXIT', e.code, flush=True)
'''


def test_cli_mesh_direct(dev, tmp_path):
    import json
    plain, direct = str(tmp_path / 'plain.ply'), str(tmp_path / 'direct.ply')
    common = ['--random-init', '--frames', '2', '--res', '32', '--no-double-depth', '--no-solver-search', '--voxel-res', '48', '--mesh-level', '0']
    lines = [common + ['--mesh-direct', '--mesh', direct],                                         # needs --mesh-band
             common + ['--mesh-band', '4', '--mesh-direct', '--mesh', direct, '--shapes', str(tmp_path / 'v.npy')],
             common + ['--mesh-band', '4', '--mesh-direct', '--mesh', direct]]
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.join(ROOT, 'g-nerf_amd'), ROOT, env.get('PYTHONPATH', '')])
    r = subprocess.run([sys.executable, '-c', DRIVER, plain, json.dumps(lines)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count('EXIT 2') == 2 and '--mesh-direct requires --mesh-band' in r.stderr and 'cannot be combined with --shapes' in r.stderr
    assert 'band mesh of the 48^3 lattice' in r.stdout and r.stdout.count('band: bricks of 4^3 cells') == 1 and 'density volume' not in r.stdout
    assert not os.path.exists(str(tmp_path / 'v.npy'))
    assert open(plain, 'rb').read() == open(direct, 'rb').read(), '--mesh-direct changed the .ply'
    assert len(S.read_ply(direct)[1]) > 0
