"""GPU tests of the narrow-band density volume: gnerf_query_lattice (csrc/query_lattice.inl) against the existing route --
query_sigma(voxel_samples(...)) gathered, torch.equal -- across plane layouts and bindings; the bookkeeping kernels (csrc/mesh_band.hip)
against their numpy port, same bits, round by round; extract_density_grid(band=...) end to end with the generator; --mesh-band's report through
mesh_of_density_grid.  The CPU fields and their port results are those of tests/mesh_band_cases.py, made once."""

import copy

import numpy as np
import pytest
import torch

import shape_mi355x as S
from conftest import has_gpu
from mesh_band_cases import NOISE_KEEP, SPHERE_KEEP, field, restricted_dense, same_mesh

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


@pytest.fixture(scope='module')
def dev():
    if not has_gpu():
        pytest.fail('GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)')
    import gnerf_hip
    gnerf_hip.load()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def model(dev):
    """test_density_volume_gpu_vs_cpu's random-init generator on the GPU, its planes in both layouts, its folded decoder, and the dense
    references: every density of the 40^3 lattice and those of the 260^3 lattice above index 2^24."""
    import gnerf_generator
    import gnerf_hip
    import gen_videos_mi355x as gv
    from training.volumetric_rendering.renderer import _osg_decoder_weights
    torch.manual_seed(5)
    G = gnerf_generator.Generator().eval().requires_grad_(False)
    with torch.no_grad():
        ws = G.mapping(torch.randn(1, 512), torch.zeros(1, 25))
        G = copy.deepcopy(G).to(dev)
        ws = ws.to(dev)
        planes = G.backbone.synthesis(ws, noise_mode='const')
        planes = planes.view(len(planes), 3, 32, planes.shape[-2], planes.shape[-1])
        kw = G.rendering_kwargs
        ref40 = G.renderer.query_sigma(planes, G.decoder, gv.voxel_samples(0, 40 ** 3, 40, kw['box_warp'], dev), kw).reshape(-1)
        ref260 = G.renderer.query_sigma(planes, G.decoder, gv.voxel_samples(2 ** 24, 260 ** 3, 260, kw['box_warp'], dev), kw).reshape(-1)
    N, P, C, H, W = planes.shape
    return dict(G=G, ws=ws, planes=planes, kw=kw, dec=G.renderer._decoder_cache(_osg_decoder_weights(G.decoder)),
                nhwc=gnerf_hip.planes_to_nhwc(planes), inter=planes.permute(0, 3, 4, 1, 2).reshape(N, H, W, P * C).contiguous(),
                ref40=ref40, ref260=ref260)


def lattice(model, layout, binding, index, n):
    import gnerf_hip
    out = torch.full([n ** 3], SENTINEL, dtype=torch.float32, device=index.device)
    back = gnerf_hip.query_lattice(model[layout], model['dec'], index, n, model['kw']['box_warp'], model['kw']['box_warp'], out, binding=binding)
    assert back is out
    return out


@pytest.mark.parametrize('binding', [None, 'ctypes'])
@pytest.mark.parametrize('layout', ['nhwc', 'inter'])
def test_query_lattice_is_the_existing_route(dev, model, layout, binding):
    import gnerf_hip
    assert binding == 'ctypes' or gnerf_hip.ext() is not None
    g = torch.Generator().manual_seed(3)
    ref = model['ref40']
    every = torch.randperm(40 ** 3, generator=g).to(torch.int32).to(dev)                # a shuffled list of all indices
    assert torch.equal(lattice(model, layout, binding, every, 40), ref)
    for index in (torch.tensor([31337], dtype=torch.int32),                            # a list of 1
                  torch.randint(0, 40 ** 3, (1003,), generator=g).to(torch.int32),      # ragged: 1003 = 62 * 16 + 11 (with duplicates by chance)
                  torch.tensor([5, 5, 63999, 17, 5, 0, 17] * 9, dtype=torch.int32)):    # duplicates
        index = index.to(dev)
        out = lattice(model, layout, binding, index, 40)
        hit = torch.zeros(40 ** 3, dtype=torch.bool, device=dev)
        hit[index.long()] = True
        assert torch.equal(out[hit], ref[hit]) and bool((out[~hit] == SENTINEL).all())  # untouched entries keep the sentinel
    # above 2^24 float(idx) rounds: only the listed points cost anything
    lo = 2 ** 24
    index = (lo + torch.randint(0, 260 ** 3 - lo, (4096,), generator=g)).to(torch.int32).to(dev)
    assert int(index.min()) >= lo and bool((index.float().long() != index.long()).any())
    out = lattice(model, layout, binding, index, 260)
    assert torch.equal(out[index.long()], model['ref260'][index.long() - lo])
    assert int((out != SENTINEL).sum()) == len(torch.unique(index))


def test_query_lattice_refuses_bad_arguments(dev, model):
    import gnerf_hip
    out = torch.zeros(40 ** 3, device=dev)
    index = torch.zeros(4, dtype=torch.int32, device=dev)
    args = (model['nhwc'], model['dec'], index, 40, 1.0, 1.0)
    with pytest.raises(RuntimeError):
        gnerf_hip.query_lattice(*args, out[:-1])
    with pytest.raises(RuntimeError):
        gnerf_hip.query_lattice(model['nhwc'], model['dec'], index, 1300, 1.0, 1.0, out)                 # n^3 >= 2^31
    with pytest.raises(gnerf_hip.NativeError):
        gnerf_hip.query_lattice(model['nhwc'], model['dec'], index, 40, 0.0, 1.0, out, binding='ctypes')  # cube_length
    lib = gnerf_hip.load()
    too_many = (2 ** 31 - 16) // 3 + 1
    rc = lib.gnerf_query_lattice(model['nhwc'].data_ptr(), model['nhwc'].shape[1], model['nhwc'].shape[2], index.data_ptr(), too_many, 40, 1.0, 1.0, *[t.data_ptr() for t in model['dec']],
                                 out.data_ptr(), 0, None)
    assert rc != 0 and b'too many points' in lib.gnerf_last_error()
    assert gnerf_hip.query_lattice(*args[:2], index[:0], *args[3:], out) is out                          # an empty list does nothing
    outside = torch.tensor([-1, 40 ** 3, 7], dtype=torch.int32, device=dev)                            # outside the lattice: nothing is written
    got = lattice(model, 'nhwc', 'ctypes', outside, 40)
    assert int((got != SENTINEL).sum()) == 1 and float(got[7]) == float(model['ref40'][7])


def test_query_sigma_lattice_takes_the_kernel(dev, model, monkeypatch):
    import gnerf_hip
    G, kw = model['G'], model['kw']
    calls = []
    real = gnerf_hip.query_lattice
    monkeypatch.setattr(gnerf_hip, 'query_lattice', lambda *a, **k: calls.append(len(a[2])) or real(*a, **k))
    index = torch.arange(0, 40 ** 3, 7, dtype=torch.int32, device=dev)
    out = torch.full([40 ** 3], SENTINEL, device=dev)
    with torch.no_grad():
        assert G.renderer.query_sigma_lattice(model['planes'], G.decoder, index, 40, kw, out) is out
    assert calls == [len(index)] and torch.equal(out[::7], model['ref40'][::7]) and bool((out[1::7] == SENTINEL).all())
    with torch.no_grad():                                                               # density noise is not the kernel's: the composed route
        noisy = G.renderer.query_sigma_lattice(model['planes'], G.decoder, index[:50], 40, dict(kw, density_noise=0.5), torch.zeros(40 ** 3, device=dev))
    assert calls == [len(index)] and not torch.equal(noisy[:350:7], model['ref40'][:350:7])


CASES = [('rough_sphere', 4, None), ('rough_sphere', 8, SPHERE_KEEP), ('rough_sphere', 2, SPHERE_KEEP), ('rough_sphere', 16, None),
         ('four_balls', 4, None), ('four_balls', 8, None), ('noise', 4, NOISE_KEEP), ('noise', 8, NOISE_KEEP), ('integer', 4, None)]


@pytest.mark.parametrize('binding', [None, 'ctypes'])
@pytest.mark.parametrize('name,s,keep', CASES, ids=[f'{c[0]}-{c[1]}' for c in CASES])
def test_band_kernels_give_the_ports_bits(dev, name, s, keep, binding):
    """States after every round, the emitted lists, the counts and the final volume, against band_volume_numpy; two runs are identical."""
    import gnerf_hip
    dense, level = field(name)
    n = dense.shape[0]
    flat = dense.reshape(-1)
    dense_dev = torch.from_numpy(np.array(flat)).to(dev)

    def host_field(index, out):
        out[index] = flat[index]

    def dev_field(index, out):
        assert index.dtype == torch.int32 and index.is_cuda
        out[index.long()] = dense_dev[index.long()]

    want_trace = []
    want, want_report = S.band_volume_numpy(host_field, n, level, s, keep, trace=want_trace)
    runs = []
    for _ in range(2):
        trace = []
        if binding is None:
            vol, report = S.band_volume(dev_field, n, level, s, keep, device=dev, trace=trace)
        else:                                                                           # the driver's steps on the ctypes route
            vol = torch.empty(n ** 3, dtype=torch.float32, device=dev)
            band = gnerf_hip.BandVolume(vol, n, s, level, keep, binding='ctypes')
            report = S._band_driver(n, s, lambda index: dev_field(index, vol) if len(index) else None, torch.from_numpy(S.band_coarse_index(n, s)).to(dev),
                                    band, trace)
            vol = vol.reshape(n, n, n)
        assert vol.is_cuda and report == want_report
        assert len(trace) == len(want_trace)
        for (state, index), (want_state, want_index) in zip(trace, want_trace):
            assert state.dtype == np.uint8 and np.array_equal(state, want_state)
            assert index.dtype == np.int32 and np.array_equal(index, want_index)
        runs.append(vol.cpu().numpy())
    assert runs[0].tobytes() == want.tobytes() == runs[1].tobytes()


def test_band_kernels_refuse_bad_arguments(dev):
    import gnerf_hip
    vol = torch.zeros(20 ** 3, device=dev)
    with pytest.raises(ValueError):
        gnerf_hip.BandVolume(vol, 20, 3, 0.0)
    with pytest.raises(ValueError):
        gnerf_hip.BandVolume(vol[:-1], 20, 4, 0.0)
    band = gnerf_hip.BandVolume(vol, 20, 4, 0.0, binding='ctypes')
    with pytest.raises(gnerf_hip.NativeError):
        gnerf_hip.band_fill(vol, 20, 5, None, band.state, binding='ctypes')
    new = band.seed()                                                                   # all outside: nothing to do, nothing listed
    assert new == 0 and band.points_next == 0 and not bool(band.state.any()) and len(band.points()) == 0


@pytest.fixture(scope='module')
def volumes(dev, model):
    """The dense GPU volume at resolution 40 under the crop, the level (the median of the kept region), and the band volume with its report."""
    import gen_videos_mi355x as gv
    G, ws, planes = model['G'], model['ws'], model['planes']
    with torch.no_grad():
        dense = gv.extract_density_grid(G, ws, resolution=40, crop=True, planes=planes)
        (a0, b0), (a1, b1), (a2, b2) = gv.crop_ranges(40)
        level = float(dense[a0:40 - b0, a1:40 - b1, a2:40 - b2].median())
        reports = {}
        band = gv.extract_density_grid(G, ws, resolution=40, crop=True, planes=planes, band=4, level=level, report=reports)
    return dense, level, band, reports['band']


def test_extract_density_grid_band_end_to_end(dev, model, volumes):
    import gen_videos_mi355x as gv
    dense, level, band, report = volumes
    assert band.is_cuda and band.shape == (40, 40, 40) and band.dtype == torch.float32
    assert 0 < report['points'] < 40 ** 3 and report['seeds'] > 0 and report['brick'] == 4
    # the port, fed with the dense GPU densities (before flip and crop: the uncropped lattice in linear order)
    with torch.no_grad():
        sigmas = gv.extract_density_grid(model['G'], model['ws'], resolution=40, crop=False, planes=model['planes']).flip(0).reshape(-1).cpu().numpy()
    (a0, b0), r1, r2 = gv.crop_ranges(40)
    keep = S.band_keep_of_crop(40, [(b0, a0), r1, r2])
    calls = np.zeros(40 ** 3, dtype=np.int64)

    def host_field(index, out):
        np.add.at(calls, index, 1)
        out[index] = sigmas[index]

    want, want_report = S.band_volume_numpy(host_field, 40, level, 4, keep)
    assert want_report == report
    want = torch.from_numpy(want).flip(0)
    mask = torch.zeros(40, 40, 40, dtype=torch.bool)
    mask[a0:40 - b0, r1[0]:40 - r1[1], r2[0]:40 - r2[1]] = True
    want = torch.where(mask, want, torch.zeros(()))
    assert torch.equal(band.cpu(), want)                                                # the band volume is the port's
    seen = torch.from_numpy(calls.reshape(40, 40, 40) > 0).flip(0)
    assert calls.max() == 1 and torch.equal(band.cpu()[seen], dense.cpu()[seen])        # and the dense volume at every evaluated point
    band_mesh = S.marching_cubes(band.permute(2, 1, 0).contiguous(), level)
    dense_mesh = S.marching_cubes(dense.permute(2, 1, 0).contiguous(), level)
    band_mesh, dense_mesh = [tuple(S.to_host(x) for x in m) for m in (band_mesh, dense_mesh)]
    verts, faces, lost, partly = restricted_dense(dense_mesh, band_mesh)
    assert len(band_mesh[1]) > 0 and partly == 0 and same_mesh(band_mesh, (verts, faces))
    label, faces_of, _ = S.mesh_components_numpy(dense_mesh[1], len(dense_mesh[0]))
    assert int(faces_of.max()) > max([f for _, f in lost], default=0)                   # the largest component is present
    assert max(np.bincount(S.mesh_components_numpy(band_mesh[1], len(band_mesh[0]))[0])) == max(np.bincount(label))


def test_mesh_band_report_through_mesh_of_density_grid(dev, model, volumes):
    import gen_videos_mi355x as gv
    dense, level, band, report = volumes
    mesh, _ = gv.mesh_of_density_grid(band, level, band=report, clean=S.clean_options(keep_largest=1))
    plain, _ = gv.mesh_of_density_grid(dense, level, clean=S.clean_options(keep_largest=1))
    assert list(mesh.reports) == ['band', 'clean'] and mesh.reports['band'] is report and list(plain.reports) == ['clean']
    assert mesh.verts.is_cuda and torch.equal(mesh.verts, plain.verts) and torch.equal(mesh.faces, plain.faces)
    line = S.band_report_line(report)
    assert f'{report["points"]} points evaluated' in line and f'{report["rounds"]} round(s)' in line
