"""BASELINE config 1 (plumbing, CPU): one 64x64 frame of the random-init FFHQ-config generator rendered by this repository
alone equals the same frame rendered by the reference alone; everything is on the PyTorch CPU paths.  The reference's frame
is tests/golden/config1_frame_reference.npz, which tests/golden/make_reference_runs.py records from a G-NeRF checkout by
running the script below on the reference tree."""

import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OURS = os.path.join(ROOT, 'g-nerf_amd')
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'config1_frame_reference.npz')

SCRIPT = r'''
import sys, types, numpy as np, torch
sys.dont_write_bytecode = True
for p in reversed(%(paths)r): sys.path.insert(0, p)
tvr = types.ModuleType("torchvision.models.resnet"); tvr.ResNet = type("ResNet", (torch.nn.Module,), {}); tvr.Bottleneck = type("B", (torch.nn.Module,), {})
sys.modules.update({"torchvision": types.ModuleType("torchvision"), "torchvision.models": types.ModuleType("torchvision.models"), "torchvision.models.resnet": tvr})
import importlib.util
def load(name):      # the two harness files are loaded BY PATH so that the reference-only recording never sees g-nerf_amd/ on sys.path
    spec = importlib.util.spec_from_file_location(name, %(pkg)r + "/" + name + ".py")
    m = importlib.util.module_from_spec(spec); sys.modules[name] = m; spec.loader.exec_module(m); return m
load("gnerf_harness"); gv = load("gen_videos_mi355x")
import training.volumetric_rendering.renderer as rr
torch.set_num_threads(8)
G = gv.build_random_generator(0, torch.device("cpu"))
z = torch.randn(1, 512, generator=torch.Generator().manual_seed(1))
frames, raws, (lo, hi) = gv.render_orbit(G, z, n_frames=120, res=64, device=torch.device("cpu"), rank=%(rank)d, world=120, double_depth=False, frame_seed=7)
np.savez(%(out)r, frame=frames.numpy(), raw=raws.numpy(), renderer_file=np.array(rr.__file__))
print("done", lo, hi)
'''


def _run(paths, out, rank):
    code = SCRIPT % dict(paths=paths, pkg=os.path.join(ROOT, 'g-nerf_amd'), out=out, rank=rank)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd='/tmp', timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]


def test_config1_frame_matches_reference(tmp_path):
    b = str(tmp_path / 'ours.npz')
    _run([OURS], b, rank=30)
    ra, rb = np.load(FIXTURE), np.load(b)
    assert 'g-nerf_amd' not in str(ra['renderer_file']) and 'g-nerf_amd' in str(rb['renderer_file'])
    assert ra['frame'].shape == (1, 512, 512, 3) and ra['raw'].shape == (1, 64, 64, 3)
    assert rb['frame'].shape == ra['frame'].shape and rb['raw'].shape == ra['raw'].shape
    # uint8 images: allow off-by-one on a handful of pixels (different but equivalent fp32 operation orders)
    for k in ('frame', 'raw'):
        d = np.abs(ra[k].astype(np.int32) - rb[k].astype(np.int32))
        assert d.max() <= 1, (k, d.max())
        assert (d > 0).mean() < 0.01, (k, (d > 0).mean())
    assert ra['frame'].std() > 1.0          # not a constant image


def record_reference(ref):
    """The reference alone renders the frame: its own generator, renderer and ops (tests/golden/make_reference_runs.py)."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        _run([ref], os.path.join(tmp, 'ref.npz'), rank=30)
        d = dict(np.load(os.path.join(tmp, 'ref.npz')))
    d['renderer_file'] = np.array(os.path.relpath(str(d['renderer_file']), ref))
    np.savez_compressed(FIXTURE, **d)
