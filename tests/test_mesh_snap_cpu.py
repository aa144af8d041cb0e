"""CPU tests of the last mesh stage, snapping vertices onto the density's level set: the two exports are declared, built and bound; the rule
loop (training.volumetric_rendering.renderer.project_to_level_rules, the float64 port of gnerf_project_points_to_level) on an analytic field
and on the float64 oracle; the numpy port of the flip guard; the harness and its options on a CPU generator."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import shape_mi355x as S
from mesh_snap_cases import RADIUS, STEPS, TOL, fan, oracle_case, port_result
from training.volumetric_rendering.renderer import project_to_level_rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_are_declared_built_and_bound_without_an_abi_change():
    import gnerf_hip
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    assert re.search(r'#define\s+GNERF_ABI_VERSION\s+15\b', header) and gnerf_hip.ABI_VERSION == 15
    lib = gnerf_hip.load()                                          # the library csrc/build.sh made
    assert lib.gnerf_abi_version() == 15
    for name, n_args in (('gnerf_project_points_to_level', 22), ('gnerf_mesh_flip_guard', 10)):
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m, f'{name} is not declared'
        assert len(m.group(1).split(',')) == n_args
        res, args = gnerf_hip.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n_args
        assert name in gnerf_hip.OPTIONAL_SYMBOLS                   # a library of the same version built before it still loads
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args
    assert gnerf_hip.project_to_level_available() and gnerf_hip.mesh_flip_guard_available()
    assert gnerf_hip.project_points_to_level is gnerf_hip.render.project_points_to_level and gnerf_hip.mesh_flip_guard is gnerf_hip.mesh.mesh_flip_guard
    ext = gnerf_hip.ext()
    assert ext is not None, 'the pybind extension is built by csrc/build.sh'
    assert callable(ext.project_points_to_level) and callable(ext.mesh_flip_guard)


# ---------------------------------------------------------------------------------------------------------------- the rules on an analytic field

def _sphere(r):
    return lambda p: (r * r - (p * p).sum(-1), -2 * p)


def test_rules_on_a_sphere():
    gen = torch.Generator().manual_seed(0)
    R_, r = 2.0, 0.5
    dirs = torch.randn(200, 3, generator=gen, dtype=torch.float64)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    near = dirs * (R_ + (torch.rand(200, 1, generator=gen, dtype=torch.float64) - 0.5) * 0.5)        # within 0.25 of the sphere: inside the box
    far = dirs[:50] * (R_ + 1.5)                                                                      # farther than r sqrt(3)
    origin = torch.zeros(1, 3, dtype=torch.float64)
    pts = torch.cat([near, far, origin])
    out, status, res_in, res_out = project_to_level_rules(_sphere(R_), pts, 0.0, steps=8, radius=r, tol=1e-13)
    assert status.dtype == torch.uint8 and out.dtype == torch.float64
    assert status[:200].eq(0).all() and status[200:250].eq(1).all() and int(status[250]) == 2
    assert float((out[:200].norm(dim=-1) - R_).abs().max()) <= 1e-12
    assert float((out[:200] - pts[:200]).abs().max()) <= r
    assert torch.equal(out[200:].view(torch.int64), pts[200:].view(torch.int64))                     # the input's bits
    assert torch.equal(res_in, R_ * R_ - (pts * pts).sum(-1)) and torch.equal(res_out[200:], res_in[200:])
    assert float(res_out[:200].abs().max()) <= 1e-13
    # K = 0 moves nothing and converges exactly the points already within tol
    tol = 0.3
    out0, status0, in0, out_res0 = project_to_level_rules(_sphere(R_), pts, 0.0, steps=0, radius=r, tol=tol)
    assert torch.equal(out0.view(torch.int64), pts.view(torch.int64))
    assert torch.equal(status0 == 0, in0.abs() <= tol) and 0 < int((status0 == 0).sum()) < 200 and not (status0 == 2).any()
    assert torch.equal(in0, out_res0)
    # r = 0 returns the input's bits
    out1, status1, _, _ = project_to_level_rules(_sphere(R_), pts, 0.0, steps=8, radius=0.0, tol=1e-13)
    assert torch.equal(out1.view(torch.int64), pts.view(torch.int64)) and not (status1 == 0).any()
    # an affine frame: points in half-size units
    A = np.concatenate([np.eye(3) * 2.0, np.array([[0.5], [0.0], [0.0]])], axis=1)
    out2, status2, _, _ = project_to_level_rules(_sphere(R_), (near - torch.tensor([0.5, 0, 0])) / 2, 0.0, steps=8, radius=r, tol=1e-13, affine=A)
    assert status2.eq(0).all() and float(((out2 * 2 + torch.tensor([0.5, 0, 0])).norm(dim=-1) - R_).abs().max()) <= 1e-12
    # not finite: status 2, the input's bits
    bad = near[:3].clone()
    bad[1, 2] = float('nan')
    out3, status3, _, _ = project_to_level_rules(_sphere(R_), bad, 0.0, steps=8, radius=r, tol=1e-13)
    assert status3.tolist() == [0, 2, 0] and torch.equal(out3[1].view(torch.int64), bad[1].view(torch.int64))
    for kw in (dict(steps=-1), dict(radius=-1.0), dict(radius=float('inf')), dict(tol=0.0), dict(tol=float('nan'))):
        with pytest.raises(ValueError):
            project_to_level_rules(_sphere(R_), pts, 0.0, **kw)


# ---------------------------------------------------------------------------------------------------------------- the rules on the oracle field

def test_port_field_is_the_oracle():
    """The batch-independent form of the field that the port is run on agrees with oracle.render_ref.query_points and its autograd gradient
    to float64 rounding (its two decoder products are summed in another order, nothing else differs)."""
    from oracle import render_ref as R
    c = oracle_case()
    A = torch.from_numpy(c['affine'])
    world = torch.from_numpy(c['verts'][:500]).double() @ A[:, :3].t() + A[:, 3]
    sig, grad = c['field64'](world)
    with torch.enable_grad():
        p = world.reshape(1, -1, 3).clone().requires_grad_(True)
        ref = R.query_points(c['planes'][:1].double(), [t.double() for t in c['dec']], p, 1.0)[0]
        ref_grad, = torch.autograd.grad(ref.sum(), p)
    ref = ref.detach()
    assert float((sig - ref[0, :, 0]).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float((grad - ref_grad[0]).abs().max()) <= 1e-12 * float(ref_grad.abs().max())
    assert float((c['sigma64'](world) - sig).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_port_converges_on_the_oracle_mesh():
    c = oracle_case()
    verts = torch.from_numpy(c['verts']).double()
    out, status, res_in, res_out = port_result()
    V = len(verts)
    share = float((status == 0).sum()) / V
    print(f'{V} vertices, {len(c["faces"])} faces, level {c["level"]:.6g}: converged {share:.4f}, median |residual| {float(res_in.abs().median()):.3e} -> '
          f'{float(res_out.abs().median()):.3e}, status counts {torch.bincount(status.long(), minlength=3).tolist()}')
    assert V > 5000 and share >= 0.99
    done = status == 0
    A = torch.from_numpy(c['affine'])
    sig = c['field64'](out @ A[:, :3].t() + A[:, 3])[0]
    assert float((sig[done] - c['level']).abs().max()) <= TOL
    assert torch.equal(sig[done] - c['level'], res_out[done])
    assert float((out - verts).abs().max()) <= RADIUS
    assert torch.equal(out[~done].view(torch.int64), verts[~done].view(torch.int64))
    assert torch.equal(res_out[~done], res_in[~done])
    assert float(res_out.abs().median()) < float(res_in.abs().median())


@pytest.mark.parametrize('index', [0, 37, 5000])
def test_port_point_alone_and_inside_the_batch(index):
    c = oracle_case()
    batch = port_result()
    alone = project_to_level_rules(c['field64'], torch.from_numpy(c['verts'][index:index + 1]).double(), c['level'], steps=STEPS, radius=RADIUS, tol=TOL,
                                   affine=c['affine'])
    assert int(alone[1][0]) == int(batch[1][index])
    assert torch.equal(alone[0][0].view(torch.int64), batch[0][index].view(torch.int64))
    assert torch.equal(alone[2][0], batch[2][index]) and torch.equal(alone[3][0], batch[3][index])


# ---------------------------------------------------------------------------------------------------------------- the flip guard's port

def test_flip_guard_port_on_the_fan():
    verts, moved, faces, touched = fan()
    out, status, counts = S.mesh_flip_guard_numpy(verts, moved, faces, rounds=4)
    assert counts.dtype == np.int32 and counts.tolist() == [2, 0, 0, 0, 0]            # the zero-area face and the invalid face are not counted
    assert sorted(np.nonzero(status == 3)[0].tolist()) == touched
    expect = moved.copy()
    expect[touched] = verts[touched]
    assert np.array_equal(out.view(np.uint32), expect.view(np.uint32)) and out.dtype == np.float32
    assert S.mesh_flipped_faces(verts, moved, faces).tolist() == [True, False, False, True, False, False]
    # a status that comes in is kept where nothing is reverted
    status_in = np.array([0, 1, 2, 1, 0, 2, 0, 1], dtype=np.uint8)
    _, status2, _ = S.mesh_flip_guard_numpy(verts, moved, faces, status_in, rounds=1)
    assert status2.tolist() == [3, 3, 3, 1, 3, 2, 0, 1]
    # a face collapsed to zero area by the move counts as flipped
    flat = verts.copy()
    flat[2] = [1, 0, 0]
    assert S.mesh_flipped_faces(verts, flat, faces)[0]
    # nothing moved: nothing flipped, one round suffices
    out3, status3, counts3 = S.mesh_flip_guard_numpy(verts, verts, faces, rounds=2)
    assert counts3.tolist() == [0, 0, 0] and not status3.any() and np.array_equal(out3, verts)
    with pytest.raises(ValueError):
        S.mesh_flip_guard_numpy(verts, moved, faces, rounds=0)
    with pytest.raises(ValueError):
        S.mesh_flip_guard_numpy(verts, moved[:4], faces)


def _independent_flips(v0, v1, faces):
    """Faces with n0.n1 < 0 among the valid faces of non-zero input area, from plain float64 numpy cross products."""
    f = faces[np.all((faces >= 0) & (faces < len(v0)), axis=1)]
    a0, b0, c0 = (v0[f[:, k]].astype(np.float64) for k in range(3))
    a1, b1, c1 = (v1[f[:, k]].astype(np.float64) for k in range(3))
    n0, n1 = np.cross(b0 - a0, c0 - a0), np.cross(b1 - a1, c1 - a1)
    return int(np.count_nonzero(((n0 * n1).sum(1) < 0) & ((n0 * n0).sum(1) > 0)))


def test_flip_guard_port_on_the_oracle_mesh():
    c = oracle_case()
    out, status, _, _ = port_result()
    verts, faces = c['verts'], c['faces']
    moved = out.float().numpy()
    before = _independent_flips(verts, moved, faces)
    got, st, counts = S.mesh_flip_guard_numpy(verts, moved, faces, status.numpy(), rounds=4)
    print(f'flips before {before}, per round {counts[:4].tolist()}, left {int(counts[4])}, reverted {int((st == 3).sum())}')
    assert before > 0 and int(counts[0]) >= before and int(counts[4]) == 0
    assert _independent_flips(verts, got, faces) == 0
    back = st == 3
    assert np.array_equal(got[back].view(np.uint32), verts[back].view(np.uint32)) and np.array_equal(got[~back].view(np.uint32), moved[~back].view(np.uint32))
    assert np.array_equal(st[~back], status.numpy()[~back])
    # invariant under a permutation of the faces
    perm = np.random.default_rng(3).permutation(len(faces))
    got2, st2, counts2 = S.mesh_flip_guard_numpy(verts, moved, faces[perm], status.numpy(), rounds=4)
    assert np.array_equal(got2.view(np.uint32), got.view(np.uint32)) and np.array_equal(st2, st) and np.array_equal(counts2, counts)


# ---------------------------------------------------------------------------------------------------------------- harness

def test_snap_options_and_report_line():
    assert S.snap_options(0) is None and S.snap_options(0.0, 3, 1e-3) is None
    assert S.snap_options(1.5, 4, None, 2) == dict(radius=1.5, steps=4, tol=None, guard_rounds=2)
    assert S.snap_options(1) == dict(radius=1.0, steps=6, tol=None, guard_rounds=4)
    for bad in ((-1,), (float('inf'),), (float('nan'),), (1, -1), (1, 6, 0.0), (1, 6, float('inf')), (1, 6, None, 0)):
        with pytest.raises(ValueError):
            S.snap_options(*bad)
    line = S.snap_report_line(dict(vertices=10, converged=7, not_converged=1, flat=0, reverted=2, median_before=0.5, max_before=2.0, median_after=1e-4,
                                   max_after=2.0, flips=[3, 0, 0, 0], flips_left=0, tol=1e-3))
    assert line.startswith('mesh snap: 7 of 10 vertices') and 'none left' in line and '2 reverted' in line


def test_harness_snaps_a_cpu_generator_mesh(tmp_path):
    import gen_videos_mi355x as gv
    dev = torch.device('cpu')
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1))
    res = 24
    vol, planes = gv.extract_density_grid(G, gv.orbit_latents(G, z, dev), res, return_planes=True)
    level = float(vol[vol != 0].median())
    plain, same, snapped = (str(tmp_path / n) for n in ('plain.ply', 'same.ply', 'snapped.ply'))
    # snap off: the bytes of a call that does not know the option
    gv.mesh_density_grid(vol, plain, level, attrs='all', G=G, planes=planes, clean=S.clean_options(0, 0, 2))
    written = gv.mesh_density_grid(vol, same, level, attrs='all', G=G, planes=planes, clean=S.clean_options(0, 0, 2), snap=S.snap_options(0))
    assert open(plain, 'rb').read() == open(same, 'rb').read() and 'snap' not in written.mesh.reports
    # snap on
    nv, nf, _ = written = gv.mesh_density_grid(vol, snapped, level, attrs='normals', G=G, planes=planes, snap=S.snap_options(1.0))
    r = written.mesh.reports['snap']
    print(S.snap_report_line(r))
    assert r['vertices'] == nv and r['converged'] + r['not_converged'] + r['flat'] + r['reverted'] == nv and r['converged'] > 0
    assert len(r['flips']) == 4 and r['flips_left'] == 0
    assert r['median_after'] < r['median_before']
    verts, faces = S.read_ply(snapped)
    v0, f0 = S.read_ply(plain)
    assert np.array_equal(faces, f0) and not np.array_equal(verts, S.marching_cubes_numpy(vol.permute(2, 1, 0).contiguous().numpy(), level)[0])
    assert float(np.abs(verts - S.marching_cubes_numpy(vol.permute(2, 1, 0).contiguous().numpy(), level)[0]).max()) <= 1.0
    # the attributes are those of the snapped positions
    normals, _ = gv.mesh_vertex_attributes(G, planes, torch.from_numpy(verts), res, True, False)
    assert np.array_equal(S.read_ply_attrs(snapped)['normals'], normals.numpy())
    # the function itself: numpy in, numpy out; None does nothing
    mv, mf = S.marching_cubes_numpy(vol.permute(2, 1, 0).contiguous().numpy(), level)
    same_v, none = gv.snap_extracted_mesh(G, planes, mv, mf, res, None, level=level)
    assert same_v is mv and none is None
    got, rep = gv.snap_extracted_mesh(G, planes, mv, mf, res, S.snap_options(1.0), level=level)
    assert isinstance(got, np.ndarray) and np.array_equal(got.view(np.uint32), verts.view(np.uint32)) and rep == r
    with pytest.raises(ValueError):
        gv.mesh_density_grid(vol, snapped, level, snap=S.snap_options(1.0))              # the snap needs the generator
