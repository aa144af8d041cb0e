"""GPU tests of gnerf_project_points_to_level (csrc/project_level.inl) and gnerf_mesh_flip_guard (csrc/mesh_clean.hip) on the oracle case of
tests/mesh_snap_cases.py: the projection against its rules (float64 densities at the kernel's own output), against the float64 port,
across layouts, bindings, batches and frames, on its edges; the guard bit for bit against its numpy port; the harness end to end.  The
float64 volume, the mesh and the port's result are made once per process on the CPU."""

import ctypes

import numpy as np
import pytest
import torch

from conftest import has_gpu
from mesh_snap_cases import RADIUS, STEPS, TOL, fan, lattice_affine, oracle_case, port_result

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not has_gpu():
        pytest.fail('GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)')
    import gnerf_hip
    gnerf_hip.load()
    return torch.device('cuda', 0)


def _interleaved(planes):
    N, P, C, H, W = planes.shape
    return planes.permute(0, 3, 4, 1, 2).reshape(N, H, W, P * C).contiguous()


@pytest.fixture(scope='module')
def case(dev):
    import gnerf_hip
    c = dict(oracle_case())
    planes = c['planes'].to(dev)
    c.update(nhwc=[gnerf_hip.planes_to_nhwc(planes[i:i + 1]) for i in range(2)], nhwc2=gnerf_hip.planes_to_nhwc(planes),
             inter=[_interleaved(planes[i:i + 1]) for i in range(2)], dec_dev=[t.to(dev) for t in c['dec']],
             verts_dev=torch.from_numpy(c['verts']).to(dev), faces_dev=torch.from_numpy(c['faces']).to(dev))
    return c


def _project(case, pts, item=0, layout='nhwc', box_warp=1.0, level=None, affine='lattice', steps=STEPS, radius=RADIUS, tol=TOL):
    """One item's projection of pts [P, 3] (a CUDA tensor) -> (points_out [P, 3], status [P], residual_in [P], residual_out [P])."""
    import gnerf_hip
    affine = case['affine'] if isinstance(affine, str) else affine
    out = gnerf_hip.project_points_to_level(case[layout][item], 1, case['dec_dev'], pts.reshape(1, -1, 3), box_warp, case['level'] if level is None else level,
                                            affine=affine, steps=steps, radius=radius, tol=tol)
    assert out[0].shape == (1, len(pts), 3) and out[0].dtype == torch.float32 and out[1].shape == (1, len(pts)) and out[1].dtype == torch.uint8
    assert out[2].shape == out[3].shape == (1, len(pts)) and out[2].dtype == out[3].dtype == torch.float32
    return tuple(t[0] for t in out)


def _world32(case, pts):
    """The world positions the kernel itself forms of mesh-frame points (float32 [P, 3]): the lattice affine is diagonal, so A p + b is one
    rounded product and one rounded sum per axis, contracted or not."""
    a, b = float(np.float32(case['affine'][0, 0])), float(np.float32(case['affine'][0, 3]))
    return pts.float() * a + b


def _epsilon(case, pts):
    """2 x the largest |sigma_gpu - sigma64| that gnerf_hip.query_points (not under test here) shows at these mesh-frame points, and its
    densities."""
    import gnerf_hip
    world = _world32(case, pts)
    gpu = gnerf_hip.query_points(case['nhwc'][0], 1, case['dec_dev'], world.reshape(1, -1, 3), 1.0, want_rgb=False)[0].reshape(-1).cpu()
    return 2 * float((gpu.double() - case['sigma64'](world.cpu())).abs().max()), gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- against the rules

@pytest.mark.parametrize('n_points', [1, 16, 17, 70, None])
def test_projection_obeys_its_rules(dev, case, n_points):
    pts = case['verts_dev'][:n_points].contiguous()
    out, status, res_in, res_out = _project(case, pts)
    assert int(status.max()) <= 2
    done = (status == 0).cpu()
    eps_out, _ = _epsilon(case, out)
    eps_in, sigma_in = _epsilon(case, pts)
    eps = max(eps_out, eps_in)
    err = (case['sigma64'](_world32(case, out).cpu()) - case['level']).abs()
    print(f'P = {len(pts)}: converged {int(done.sum())}, status counts {torch.bincount(status.long().cpu(), minlength=3).tolist()}, eps {eps:.3e}, '
          f'max |sigma64 - level| of the converged {float(err[done].max()) if done.any() else 0:.3e} (tol {TOL:.3e})')
    assert float(err[done].max() if done.any() else 0) <= TOL + eps
    r = torch.tensor(RADIUS, dtype=torch.float32, device=dev)
    assert bool((out <= pts + r).all()) and bool((out >= pts - r).all())                         # fl(p0 +- r), exactly
    assert torch.equal(_bits(out)[~done.to(dev)], _bits(pts)[~done.to(dev)])
    assert float((res_in.cpu().double() - (sigma_in.double() - case['level'])).abs().max()) <= eps
    assert torch.equal(res_out[~done.to(dev)], res_in[~done.to(dev)]) and float(res_out[done.to(dev)].abs().max() if done.any() else 0) <= TOL


def test_projection_converges_like_the_port(dev, case):
    _, port_status, _, port_res = port_result()
    out, status, res_in, res_out = _project(case, case['verts_dev'])
    V = len(port_status)
    share, port_share = float((status == 0).sum()) / V, float((port_status == 0).sum()) / V
    differ = int((status.cpu() != port_status).sum())
    print(f'{V} vertices: converged share {share:.4f} (kernel) against {port_share:.4f} (float64 port), {differ} statuses differ; median |residual| '
          f'{float(res_in.abs().median()):.3e} -> {float(res_out.abs().median()):.3e}')
    assert share >= port_share - 0.005
    assert float(res_out.abs().median()) < float(res_in.abs().median())


# ---------------------------------------------------------------------------------------------------------------- determinism and invariance

def test_layouts_bindings_and_reruns_are_bit_identical(dev, case, monkeypatch):
    import gnerf_hip
    from gnerf_hip import _native
    assert gnerf_hip.ext() is not None, 'the pybind extension is built by csrc/build.sh'
    pts = case['verts_dev'][:1000].contiguous()
    first = _project(case, pts)
    runs = [_project(case, pts), _project(case, pts, layout='inter')]
    with monkeypatch.context() as m:
        m.setattr(_native, '_ext', False)                                               # the ctypes route
        assert gnerf_hip.ext() is None
        runs += [_project(case, pts), _project(case, pts, layout='inter')]
    for run in runs:
        for a, b in zip(first, run):
            assert torch.equal(a.view(torch.uint8) if a.dtype == torch.uint8 else _bits(a), b.view(torch.uint8) if b.dtype == torch.uint8 else _bits(b))
    assert int((first[1] == 0).sum()) > 900


def test_a_point_alone_is_the_point_in_its_batch(dev, case):
    batch = _project(case, case['verts_dev'][:70].contiguous())
    alone = _project(case, case['verts_dev'][37:38].contiguous())
    for a, b in zip(alone, batch):
        assert torch.equal(a[0], b[37]) and (a.dtype == torch.uint8 or torch.equal(_bits(a)[0], _bits(b)[37]))


def test_two_items_are_two_calls(dev, case):
    import gnerf_hip
    pts = torch.stack([case['verts_dev'][:70], case['verts_dev'][100:170]]).contiguous()
    both = gnerf_hip.project_points_to_level(case['nhwc2'], 2, case['dec_dev'], pts, 1.0, case['level'], affine=case['affine'], steps=STEPS, radius=RADIUS, tol=TOL)
    for item in range(2):
        single = _project(case, pts[item], item=item)
        for a, b in zip(single, both):
            assert torch.equal(a, b[item])
    assert not torch.equal(both[2][0], _project(case, pts[0], item=1)[2])                   # other planes, other densities


def test_box_warp_2_scales_exactly(dev, case):
    pts = case['verts_dev'][:1000].contiguous()
    ref = _project(case, pts)
    # the same mesh frame, a world twice as large: the same status, the same bits
    got = _project(case, pts, box_warp=2.0, affine=lattice_affine(2.0))
    assert torch.equal(got[1], ref[1]) and torch.equal(_bits(got[0]), _bits(ref[0])) and torch.equal(got[3], ref[3])
    # no affine: points, radius and box doubled -> the output doubled, exactly
    world = pts * float(np.float32(case['affine'][0, 0])) + float(np.float32(case['affine'][0, 3]))
    one = _project(case, world, affine=None, radius=0.03)
    two = _project(case, world * 2, box_warp=2.0, affine=None, radius=0.06)
    assert torch.equal(two[1], one[1]) and torch.equal(_bits(two[0]), _bits(one[0] * 2)) and torch.equal(two[2], one[2]) and torch.equal(two[3], one[3])
    assert int((one[1] == 0).sum()) > 500


# ---------------------------------------------------------------------------------------------------------------- edges

def test_edges(dev, case):
    pts = case['verts_dev'][:70].contiguous()
    # every tap outside the planes: the gradient is exactly zero
    far = torch.full([20, 3], 5.0, device=dev) + torch.arange(20, device=dev).reshape(-1, 1).float()
    out, status, res_in, res_out = _project(case, far, affine=None)
    assert status.eq(2).all() and torch.equal(_bits(out), _bits(far)) and torch.equal(res_in, res_out) and torch.isfinite(res_in).all()
    # K = 0: nothing moves; exactly the points already within tol are converged
    out, status, res_in, res_out = _project(case, pts, steps=0, tol=0.02)
    assert torch.equal(_bits(out), _bits(pts)) and torch.equal(status == 0, res_in.abs() <= 0.02) and torch.equal(res_in, res_out)
    assert 0 < int((status == 0).sum()) < 70 and set(status.tolist()) <= {0, 1}
    # r = 0: the input's bits
    out, status, _, _ = _project(case, pts, radius=0.0)
    assert torch.equal(_bits(out), _bits(pts)) and not bool((status == 0).any())
    # NaN in a point: status 2, the input's bits, and nobody else notices
    bad = pts.clone()
    bad[5, 1] = float('nan')
    bad[40] = float('inf')
    out, status, res_in, _ = _project(case, bad)
    ref = _project(case, pts)
    assert status[5] == 2 and status[40] == 2 and torch.equal(_bits(out)[[5, 40]], _bits(bad)[[5, 40]]) and bool(torch.isnan(res_in[[5, 40]]).all())
    keep = torch.ones(70, dtype=torch.bool, device=dev)
    keep[[5, 40]] = False
    assert torch.equal(_bits(out)[keep], _bits(ref[0])[keep]) and torch.equal(status[keep], ref[1][keep])


def test_argument_checks(dev, case):
    import gnerf_hip
    lib = gnerf_hip.load()
    pts = case['verts_dev'][:16].contiguous()
    out, st = torch.empty_like(pts), torch.empty(16, dtype=torch.uint8, device=dev)
    r0, r1 = torch.empty(16, device=dev), torch.empty(16, device=dev)
    nhwc, (w1, b1, w2, b2) = case['nhwc'][0], case['dec_dev']

    def call(**kw):
        a = dict(planes=nhwc.data_ptr(), h=nhwc.shape[1], w=nhwc.shape[2], points=pts.data_ptr(), n=16, steps=6, radius=1.0, tol=1e-3, out=out.data_ptr(),
                 r0=r0.data_ptr(), r1=r1.data_ptr(), st=st.data_ptr())
        a.update(kw)
        return lib.gnerf_project_points_to_level(a['planes'], 1, a['h'], a['w'], a['points'], a['n'], 1.0, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                                 case['level'], None, a['steps'], a['radius'], a['tol'], a['out'], a['r0'], a['r1'], a['st'], 0, None)

    assert call() == 0
    torch.cuda.synchronize()
    for kw in (dict(points=None), dict(out=None), dict(r0=None), dict(r1=None), dict(st=None), dict(planes=None), dict(n=0), dict(n=-3), dict(n=(2 ** 31 - 16) // 3 + 1),
               dict(steps=-1), dict(radius=-0.5), dict(radius=float('inf')), dict(radius=float('nan')), dict(tol=0.0), dict(tol=-1.0), dict(tol=float('inf')),
               dict(tol=float('nan'))):
        assert call(**kw) == -1, kw                                                          # GNERF_E_ARG
    assert call(h=8192, w=8192) == gnerf_hip.E_UNSUPPORTED and b'32-bit' in lib.gnerf_last_error()       # refused before any launch
    for kw in (dict(steps=-1), dict(radius=-1), dict(radius=float('inf')), dict(tol=0), dict(tol=float('nan')), dict(affine=[1.0] * 5)):
        with pytest.raises(ValueError):
            _project(case, pts, **kw)
    # the guard's
    v = case['verts_dev']
    f = case['faces_dev']
    counts = torch.empty(5, dtype=torch.int32, device=dev)
    vo, s = torch.empty_like(v), torch.zeros(len(v), dtype=torch.uint8, device=dev)
    g = lib.gnerf_mesh_flip_guard
    assert g(v.data_ptr(), v.data_ptr(), f.data_ptr(), len(v), len(f), 4, vo.data_ptr(), s.data_ptr(), counts.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [0] * 5
    assert g(v.data_ptr(), v.data_ptr(), f.data_ptr(), len(v), len(f), 0, vo.data_ptr(), s.data_ptr(), counts.data_ptr(), None) == -1
    assert g(v.data_ptr(), v.data_ptr(), f.data_ptr(), -1, len(f), 4, vo.data_ptr(), s.data_ptr(), counts.data_ptr(), None) == -1
    assert g(None, v.data_ptr(), f.data_ptr(), len(v), len(f), 4, vo.data_ptr(), s.data_ptr(), counts.data_ptr(), None) == -1
    assert g(v.data_ptr(), v.data_ptr(), f.data_ptr(), len(v), len(f), 4, vo.data_ptr(), s.data_ptr(), None, None) == -1
    assert g(v.data_ptr(), v.data_ptr(), f.data_ptr(), len(v), len(f), 4, v.data_ptr(), s.data_ptr(), counts.data_ptr(), None) == -1        # verts_out is verts_in
    with pytest.raises(ValueError):
        gnerf_hip.mesh_flip_guard(v, v, f, rounds=0)
    with pytest.raises(ValueError):
        gnerf_hip.mesh_flip_guard(v, v[:10], f)


# ---------------------------------------------------------------------------------------------------------------- the guard against its port

def _guard_both_bindings(v0, v1, faces, status, rounds, monkeypatch):
    import gnerf_hip
    from gnerf_hip import _native
    got = gnerf_hip.mesh_flip_guard(v0, v1, faces, status, rounds)
    with monkeypatch.context() as m:
        m.setattr(_native, '_ext', False)
        again = gnerf_hip.mesh_flip_guard(v0, v1, faces, status, rounds)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    return got


def _assert_guard_is_the_port(got, v0, v1, faces, status, rounds):
    import shape_mi355x as S
    ref_v, ref_s, ref_c = S.mesh_flip_guard_numpy(v0.cpu().numpy(), v1.cpu().numpy(), faces.cpu().numpy(), None if status is None else status.cpu().numpy(), rounds)
    out, st, counts = got
    assert out.dtype == torch.float32 and st.dtype == torch.uint8 and counts.dtype == torch.int32 and counts.shape == (rounds + 1,) and counts.is_cuda
    assert np.array_equal(counts.cpu().numpy(), ref_c), (counts.tolist(), ref_c.tolist())
    assert np.array_equal(st.cpu().numpy(), ref_s)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref_v.view(np.uint32))
    return ref_c


def test_guard_on_the_fan(dev, monkeypatch):
    verts, moved, faces, touched = fan()
    v0, v1, f = (torch.from_numpy(a).to(dev) for a in (verts, moved, faces))
    got = _guard_both_bindings(v0, v1, f, None, 4, monkeypatch)
    counts = _assert_guard_is_the_port(got, v0, v1, f, None, 4)
    assert counts.tolist() == [2, 0, 0, 0, 0] and sorted(torch.nonzero(got[1] == 3).reshape(-1).tolist()) == touched
    status = torch.tensor([0, 1, 2, 1, 0, 2, 0, 1], dtype=torch.uint8, device=dev)
    _assert_guard_is_the_port(_guard_both_bindings(v0, v1, f, status, 1, monkeypatch), v0, v1, f, status, 1)


def test_guard_on_the_snapped_oracle_mesh(dev, case, monkeypatch):
    v0, f = case['verts_dev'], case['faces_dev']
    moved, status, _, _ = _project(case, v0)
    got = _guard_both_bindings(v0, moved, f, status, 4, monkeypatch)
    counts = _assert_guard_is_the_port(got, v0, moved, f, status, 4)
    print(f'snapped mesh: flips per round {counts[:4].tolist()}, left {int(counts[4])}, reverted {int((got[1] == 3).sum())}')
    assert counts[0] > 0 and counts[4] == 0
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(f))).to(dev)
    again = _guard_both_bindings(v0, moved, f[perm].contiguous(), status, 4, monkeypatch)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_guard_on_a_noisy_mesh(dev, case, monkeypatch):
    v0, f = case['verts_dev'], case['faces_dev']
    noise = (torch.rand(v0.shape, generator=torch.Generator().manual_seed(5)) * 3 - 1.5).to(dev)
    moved = v0 + noise
    for rounds in (1, 2, 6):
        got = _guard_both_bindings(v0, moved, f, None, rounds, monkeypatch)
        counts = _assert_guard_is_the_port(got, v0, moved, f, None, rounds)
        print(f'+-1.5 voxels of noise, {rounds} round(s): flips {counts.tolist()}, reverted {int((got[1] == 3).sum())}')
        assert counts[0] > 1000
    assert np.count_nonzero(counts[:6]) >= 2                                                 # several rounds had work
    perm = torch.from_numpy(np.random.default_rng(4).permutation(len(f))).to(dev)
    again = _guard_both_bindings(v0, moved, f[perm].contiguous(), None, 6, monkeypatch)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- end to end

def test_snap_end_to_end(dev, tmp_path):
    import gen_videos_mi355x as gv
    import shape_mi355x as S
    res = 32
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    vol, planes = gv.extract_density_grid(G, gv.orbit_latents(G, z, dev), res, return_planes=True)
    level = float(vol[vol != 0].median())
    verts, faces = S.marching_cubes(vol.permute(2, 1, 0).contiguous(), level)
    assert verts.is_cuda and len(faces) > 100
    snapped, r = gv.snap_extracted_mesh(G, planes, verts, faces, res, S.snap_options(1.0), level=level)
    print(S.snap_report_line(r))
    assert snapped.is_cuda and snapped.shape == verts.shape and snapped.dtype == torch.float32
    assert r['vertices'] == len(verts) and r['converged'] + r['not_converged'] + r['flat'] + r['reverted'] == len(verts) and r['converged'] > 0
    assert len(r['flips']) == 4 and r['flips_left'] >= 0
    assert r['flips_left'] == 0 or f'{r["flips_left"]} LEFT' in S.snap_report_line(r)       # the remainder is named
    assert r['median_after'] < r['median_before']
    assert float((snapped - verts).abs().max()) <= 1.0
    # the densities at the snapped vertices, from the query kernel: the converged ones are on the level set
    world = gv.lattice_to_world(gv.mesh_to_lattice(snapped, res), res, G.rendering_kwargs['box_warp']).unsqueeze(0)
    sigma = G.renderer.query_sigma(planes[:1], G.decoder, world, G.rendering_kwargs).reshape(-1)
    moved = (snapped != verts).any(dim=1)
    assert float((sigma[moved] - level).abs().max()) <= 2 * r['tol']                        # tol is the kernel's own criterion; as much again for
                                                                                            # the world position rounded along another route
    # the file route, with attributes at the snapped positions, and the rasteriser draws the result
    path = str(tmp_path / 'snapped.ply')
    nv, nf, _ = written = gv.mesh_density_grid(vol, path, level, attrs='normals', G=G, planes=planes, snap=S.snap_options(1.0))
    assert written.mesh.reports['snap'] == r and (nv, nf) == (len(verts), len(faces))
    file_verts, _ = S.read_ply(path)
    assert np.array_equal(file_verts.view(np.uint32), snapped.cpu().numpy().view(np.uint32))
    normals, _ = gv.mesh_vertex_attributes(G, planes, snapped, res, True, False)
    assert np.array_equal(S.read_ply_attrs(path)['normals'], normals.cpu().numpy())
    frames, _ = gv.render_geometry_orbit(snapped, faces, 2, 64, res, G.rendering_kwargs['box_warp'], G.rendering_kwargs['avg_camera_radius'], normals=normals)
    assert frames.shape == (2, 64, 64, 3) and frames.dtype == torch.uint8 and int(frames.float().std()) > 0
