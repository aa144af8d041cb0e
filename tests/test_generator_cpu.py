"""gnerf_generator.Generator (the inference-only stand-in for the hot path's callers, used where the reference tree is
absent) against the reference's own TriPlaneGenerator: same parameter / buffer names and shapes and the same images for the
same seeded weights, latent, camera and seed; CPU, fp32.  The reference's side is tests/golden/generator_reference.npz, which
tests/golden/make_reference_runs.py records from a G-NeRF checkout by running the scripts below with the reference tree
behind the overlay; the tests run the same scripts on this repository alone.  Because the recording runs this repository's
CPU renderer and ops in front of the reference's generator (as the comparison always did), the fixture holds their output as it
was when recorded: a deliberate change to the CPU paths of the overlay's renderer or ops calls for re-running the recording."""

import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OURS = os.path.join(ROOT, 'g-nerf_amd')
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'generator_reference.npz')


def _run(script, paths, out, record=False, timeout=900):
    code = script % dict(paths=paths, out=out, record=record, fixture=FIXTURE)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'),
                       cwd='/tmp', timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


SCRIPT = r'''
import json, sys, types, numpy as np, torch
sys.dont_write_bytecode = True
for p in reversed(%(paths)r): sys.path.insert(0, p)
tvr = types.ModuleType("torchvision.models.resnet"); tvr.ResNet = type("ResNet", (torch.nn.Module,), {}); tvr.Bottleneck = type("B", (torch.nn.Module,), {})
sys.modules.update({"torchvision": types.ModuleType("torchvision"), "torchvision.models": types.ModuleType("torchvision.models"), "torchvision.models.resnet": tvr})
import gen_videos_mi355x as gv, gnerf_generator, gnerf_harness as H
torch.set_num_threads(8)
# the reference tree behind the overlay: its TriPlaneGenerator; this repository alone: gnerf_generator.Generator (same seeded init)
G = gv.build_random_generator(0, torch.device("cpu"))
assert (type(G).__name__ == "TriPlaneGenerator") == %(record)r and isinstance(G, gnerf_generator.Generator) != %(record)r
# make the comparison bite: non-zero noise strengths and biases (both are zero at initialisation)
g = torch.Generator().manual_seed(5)
with torch.no_grad():
    for n, p_ in G.named_parameters():
        if n.endswith("noise_strength") or n.endswith(".bias"):
            p_.add_(torch.randn(p_.shape, generator=g) * 0.1)
z = torch.randn(2, 512, generator=g)
c = torch.cat([H.camera_label(H.orbit_pose(i, 120)) for i in (3, 40)])
with torch.no_grad():
    ws = G.mapping(z, c)
    torch.manual_seed(11); a = G.synthesis(ws, c, noise_mode="const", neural_rendering_resolution=64)
    planes = G.backbone.synthesis(ws, noise_mode="const")
# full tensors where they are small; a fixed strided sample plus whole-tensor statistics of the 512^2 image and the planes
res = dict(state=np.array(json.dumps([[k, list(v.shape)] for k, v in G.state_dict().items()])), ws=ws.numpy(),
           planes_sub=planes[:, :, ::16, ::16].numpy(), image_shape=np.array(a["image"].shape), image_sub=a["image"][:, :, ::8, ::8].numpy(),
           image_raw=a["image_raw"].numpy(), image_depth=a["image_depth"].numpy())
for k, t in (("planes", planes), ("image", a["image"]), ("image_raw", a["image_raw"]), ("image_depth", a["image_depth"])):
    res[k + "_scale"] = t.abs().max().numpy(); res[k + "_mean"] = t.double().mean().numpy(); res[k + "_ms"] = (t.double() ** 2).mean().numpy()
np.savez_compressed(%(out)r, **res)
'''


def test_generator_matches_reference(tmp_path):
    d, ref = _run(SCRIPT, [OURS], str(tmp_path / 'ours.npz')), _ref('gen_')
    assert str(d['state']) == str(ref['state'])             # the same parameter / buffer names and shapes (a strict state_dict load)
    assert tuple(d['ws'].shape) == (2, 14, 512) and tuple(d['image_shape']) == (2, 3, 512, 512)
    assert float(np.abs(d['ws'] - ref['ws']).max()) < 1e-5
    tol = {'planes': 1e-4, 'image': 2e-4, 'image_raw': 2e-4, 'image_depth': 2e-4}
    for k, rel in tol.items():
        scale = max(1.0, float(ref[k + '_scale']))
        full = d[k] if k in ('image_raw', 'image_depth') else d[k + '_sub']
        want = ref[k] if k in ('image_raw', 'image_depth') else ref[k + '_sub']
        assert float(np.abs(full - want).max()) < rel * scale, (k, float(np.abs(full - want).max()), scale)
        assert abs(float(d[k + '_scale']) - float(ref[k + '_scale'])) < rel * scale, k
        assert abs(float(d[k + '_mean']) - float(ref[k + '_mean'])) < rel * scale, k
        assert abs(float(d[k + '_ms']) - float(ref[k + '_ms'])) < 2 * rel * scale * scale, k


def _ref(prefix):
    with np.load(FIXTURE) as f:
        return {k[len(prefix):]: f[k] for k in f.files if k.startswith(prefix)}


SHAPES_SCRIPT = r'''
import sys, types, numpy as np, torch
sys.dont_write_bytecode = True
for p in reversed(%(paths)r): sys.path.insert(0, p)
tvr = types.ModuleType("torchvision.models.resnet"); tvr.ResNet = type("ResNet", (torch.nn.Module,), {}); tvr.Bottleneck = type("B", (torch.nn.Module,), {})
stubs = {"torchvision": types.ModuleType("torchvision"), "torchvision.models": types.ModuleType("torchvision.models"), "torchvision.models.resnet": tvr}
for name in ("cv2", "imageio", "mrcfile", "scipy.interpolate"):        # the reference CLI's imports that this container lacks or does not need
    stubs.setdefault(name, types.ModuleType(name))
sys.modules.update(stubs)
import gen_videos_mi355x as gv, gnerf_generator
torch.manual_seed(0)
G = gnerf_generator.Generator().eval().requires_grad_(False)
# (n, cube_length, first point): the large lattice only from its tail (indices above 2^24)
LATTICES = ((16, 1.0, 0), (37, 2.0, 0), (300, 1.0, 300 ** 3 - 4000), (20, G.rendering_kwargs["box_warp"], 0))
if %(record)r:
    import gen_videos as ref_cli                  # the reference's gen_videos.py, for its create_samples()
    np.savez_compressed(%(out)r, **{"lattice_%%d" %% n: ref_cli.create_samples(N=n, voxel_origin=[0, 0, 0], cube_length=cube)[0][:, lo:].numpy()
                                    for n, cube, lo in LATTICES})
    sys.exit(0)
recorded = np.load(%(fixture)r)
def create_samples(n):                            # the reference's create_samples(N=n, ...) points, as recorded
    return torch.from_numpy(recorded["shapes_lattice_%%d" %% n])
res = {}
for n, cube, lo in LATTICES[:3]:
    got = gv.voxel_samples(lo, n ** 3, n, cube, torch.device("cpu"))
    res["samples_%%d" %% n] = float((got - create_samples(n)).abs().max())
# the density volume: chunked run_model on cached planes == the reference-style loop over sample_mixed
ws = G.mapping(torch.randn(1, 512), torch.zeros(1, 25))
n = 20
vol = gv.extract_density_grid(G, ws, resolution=n, max_batch=3000, crop=False)
samples = create_samples(n)
dirs = torch.zeros_like(samples); dirs[..., -1] = -1
with torch.no_grad():
    sig = G.sample_mixed(samples, dirs, ws, noise_mode="const")["sigma"].reshape(n, n, n).flip(0)
res["volume"] = float((vol - sig).abs().max()); res["volume_scale"] = float(sig.abs().max())
c = gv.extract_density_grid(G, ws, resolution=n, max_batch=3000, crop=True)
res["crop_ok"] = float(c[:2].abs().max() + c[-2:].abs().max() + c[:, :2].abs().max() + c[:, -2:].abs().max() + c[:, :, :2].abs().max() + c[:, :, -2:].abs().max())
res["crop_inner"] = float((c[3:-3, 3:-3, 3:-3] - vol[3:-3, 3:-3, 3:-3]).abs().max())
np.savez(%(out)r, **res)
'''


def test_density_volume_matches_reference_lattice(tmp_path):
    """gen_videos.py --shapes counterpart: the lattice points equal the reference's create_samples() (float-division quirk and
    fp32 index rounding included) and the chunked extraction equals the per-chunk sample_mixed loop."""
    d = _run(SHAPES_SCRIPT, [OURS], str(tmp_path / 'shapes.npz'))
    for n in (16, 37, 300):
        assert float(d[f'samples_{n}']) == 0.0, (n, float(d[f'samples_{n}']))
    assert float(d['volume']) <= 1e-5 * max(1.0, float(d['volume_scale']))
    assert float(d['crop_ok']) == 0.0 and float(d['crop_inner']) == 0.0


def record_reference(ref):
    """The reference's side of the two tests above, run with the reference tree behind the overlay (tests/golden/make_reference_runs.py)."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        gen = _run(SCRIPT, [OURS, ref], os.path.join(tmp, 'gen.npz'), record=True)
        shapes = _run(SHAPES_SCRIPT, [OURS, ref], os.path.join(tmp, 'shapes.npz'), record=True)
    np.savez_compressed(FIXTURE, **{'gen_' + k: v for k, v in gen.items()}, **{'shapes_' + k: v for k, v in shapes.items()})


def test_clear_latent_caches_drops_every_cache():
    """gnerf_generator.clear_latent_caches drops the per-latent / per-parameter caches the fast path hangs on the modules (ADVICE r3:
    several hundred MB over the backbone with no release hook): the converted biases, the pre-normalised weights and the packed weights of
    our own kernels (fp16 and fp32-grade, plain and transposed) included."""
    import torch
    import gnerf_generator as GG
    m = torch.nn.Linear(2, 2)
    m.__dict__['_gnerf_latent_cache'] = {'x': (None, None, torch.zeros(3))}
    conv = GG.StyledConv(8, 128, 16, 8).requires_grad_(False)
    with torch.no_grad():
        cached = [GG._cast_param(conv, 'bias', torch.float16), GG._prenormalised_weight(conv, torch.float16, channels_last=True),
                  GG._packed_prenormalised_weight(conv, torch.float16), GG._packed_prenormalised_weight(conv, torch.float16, transposed=True),
                  GG._packed_weight_f32x3(conv), GG._packed_weight_f32x3(conv, transposed=True)]
        again = [GG._cast_param(conv, 'bias', torch.float16), GG._prenormalised_weight(conv, torch.float16, channels_last=True),
                 GG._packed_prenormalised_weight(conv, torch.float16), GG._packed_prenormalised_weight(conv, torch.float16, transposed=True),
                 GG._packed_weight_f32x3(conv), GG._packed_weight_f32x3(conv, transposed=True)]
    assert all(a is b for a, b in zip(cached, again))                  # each is made once per parameter version
    root = torch.nn.Sequential(m, conv)
    assert len(GG.latent_cache_tensors(root)) == 1
    GG.clear_latent_caches(root)
    assert GG.latent_cache_tensors(root) == [] and not any(k.startswith('_gnerf') for mod in root.modules() for k in mod.__dict__)
