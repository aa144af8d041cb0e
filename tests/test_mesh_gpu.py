"""GPU tests of the marching-cubes kernel (csrc/mesh.hip through gnerf_hip.marching_cubes / shape_mi355x.marching_cubes): the same bits
as the numpy port on spheres, noise and integer volumes, odd shapes and generator volumes; closed and reproducible at 512^3; both
bindings agree; gen_videos_mi355x.py --mesh end to end."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import shape_mi355x as S
from test_mesh_cpu import assert_closed_oriented, euler, integer_volumes, noise_volumes, sphere_field

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', 0)


def same_bits(vol, level, dev):
    ref_v, ref_f = S.marching_cubes_numpy(vol, level)
    verts, faces = S.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).to(dev), level)
    assert verts.is_cuda and verts.dtype == torch.float32 and faces.dtype == torch.int32
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    assert v.shape == ref_v.shape and f.shape == ref_f.shape
    assert np.array_equal(v.view(np.uint32), ref_v.view(np.uint32))
    assert np.array_equal(f, ref_f)
    return v, f


def generator_volume(dev, resolution):
    import gen_videos_mi355x as gv
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    return gv.extract_density_grid(G, gv.orbit_latents(G, z, dev), resolution)


def test_sphere_matches_the_numpy_port(dev):
    v, f = same_bits(sphere_field(48, 20.0), 0.0, dev)
    assert euler(v, f) == 2


def test_noise_and_integer_volumes_match_the_numpy_port(dev):
    for vol in noise_volumes():
        for level in (0.0, 0.3, 0.6, 0.9):
            same_bits(vol, level, dev)
    for vol in integer_volumes():
        for level in (0.0, 1.0, 2.0):
            same_bits(vol, level, dev)


def test_odd_shapes_match_the_numpy_port(dev):
    rng = np.random.default_rng(7)
    vol = rng.standard_normal((17, 33, 65)).astype(np.float32)
    for level in (-0.5, 0.0, 0.7):
        same_bits(vol, level, dev)
    for case in range(256):                                   # every case of the one cell of a 2 x 2 x 2 volume
        tiny = np.array([(case >> c) & 1 for c in range(8)], dtype=np.float32).reshape(2, 2, 2) * 2 - 1
        same_bits(tiny * np.float32(0.5 + case / 512), 0.0, dev)


def test_empty_and_non_finite(dev):
    verts, faces = S.marching_cubes(torch.zeros(4, 5, 6, device=dev), 0.5)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)
    vol = torch.from_numpy(sphere_field(10, 3.0)).to(dev)
    vol[2, 3, 4] = float('nan')
    with pytest.raises(ValueError, match='non-finite'):
        S.marching_cubes(vol, 0.0)


def test_generator_volume_128_matches_the_numpy_port(dev):
    vol = generator_volume(dev, 128)
    v, f = same_bits(vol.cpu().numpy(), 0.0, dev)
    assert len(f) > 1000
    assert_closed_oriented(f)


def test_generator_volume_512_is_closed_and_reproducible(dev):
    vol = generator_volume(dev, 512).permute(2, 1, 0).contiguous()
    v1, f1 = S.marching_cubes(vol, 0.0)
    v2, f2 = S.marching_cubes(vol, 0.0)
    assert len(f1) > 10000
    assert torch.equal(v1.view(torch.int32), v2.view(torch.int32)) and torch.equal(f1, f2)
    assert_closed_oriented(f1.cpu().numpy())


def test_pybind_and_ctypes_agree(dev):
    import gnerf_hip
    e = gnerf_hip.ext()
    assert e is not None, 'the pybind extension is built by csrc/build.sh'
    vol = torch.from_numpy(next(noise_volumes(seed=9, count=1))).to(dev)
    pv, pf, pc = e.marching_cubes(vol, 0.4)
    cv, cf, cc = gnerf_hip._marching_cubes_ctypes(vol, 0.4)
    assert torch.equal(pc, cc) and int(pc[0]) == len(pv) and int(pc[1]) == len(pf)
    assert torch.equal(pv.view(torch.int32), cv.view(torch.int32)) and torch.equal(pf, cf)


def test_gen_videos_mesh_end_to_end(dev, tmp_path):
    ply, mrc, npy = str(tmp_path / 'g.ply'), str(tmp_path / 'g.mrc'), str(tmp_path / 'g.npy')
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.join(ROOT, 'g-nerf_amd'), ROOT, env.get('PYTHONPATH', '')])
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'g-nerf_amd', 'gen_videos_mi355x.py'), '--random-init', '--frames', '2', '--res', '32',
                        '--no-double-depth', '--voxel-res', '128', '--shapes', npy, '--shapes-mrc', mrc, '--mesh', ply, '--mesh-level', '0'],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'density volume 128^3' in r.stdout and 'mesh at level 0' in r.stdout
    vol = np.load(npy)
    assert np.array_equal(S.read_mrc(mrc), vol)
    verts, faces = S.read_ply(ply)
    ref_v, ref_f = S.marching_cubes_numpy(np.ascontiguousarray(vol.transpose(2, 1, 0)), 0.0)
    assert np.array_equal(verts, ref_v) and np.array_equal(faces, ref_f) and len(faces) > 1000
