#!/usr/bin/env python3
"""Snapping mesh vertices onto the density's level set on the MI355X (csrc/project_level.inl, the flip guard of csrc/mesh_clean.hip), on the
two 512^3 meshes of tools/bench_mesh.py -- a random-init generator's density volume at level 0 and the sphere -- raw and simplified at 2 voxels.

  fused     gnerf_project_points_to_level: one launch for all K + 1 evaluations of the field (points that are done stop early).
  composed  the same rules (renderer.project_to_level_rules, early_exit=False: no host read) on the two kernels that existed before it:
            K + 1 x (gnerf_hip.query_points, densities only, + gnerf_hip.query_points_grad) and the PyTorch elementwise steps between them.
  guard     gnerf_mesh_flip_guard, 4 rounds, on the fused call's output.
Each is captured ten times in a HIP graph whose replay is timed with HIP events (tools/bench_raster.py's method), median / min over the
rounds.  The generator's own mesh is the case the stage is made for; the sphere's vertices have nothing to do with the generator's field, so
hardly any of them converges and every one takes all K + 1 evaluations: the fused kernel's worst case.

The coarse-grid question: the generator's volume extracted at 128^3 and 256^3, meshed and snapped (radius one voxel of that grid), against
the unsnapped 512^3 mesh: |sigma - level| at the vertices, and the point queries each route needs (the lattice plus, for a snapped mesh, the
evaluations of the projection: at most K + 1 per vertex).

    python tools/bench_mesh_snap.py | tee profiles/rNN_mesh_snap.jsonl"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'g-nerf_amd'), ROOT, os.path.join(ROOT, 'tools')]
import torch

import gnerf_hip
import shape_mi355x as S

STEPS, GUARD_ROUNDS = 6, 4


def stats(x):
    x = x[torch.isfinite(x)].abs().double()
    return {'median': float(x.median()), 'mean': float(x.mean()), 'p99': float(x.quantile(0.99)) if len(x) <= 16_000_000 else None, 'max': float(x.max())}


def snap_case(name, G, planes, verts, faces, n, level, rounds, head, time_it=True, tol=None):
    import gen_videos_mi355x as gv
    from bench_raster import replay_ms
    from training.volumetric_rendering.renderer import _osg_decoder_weights, project_to_level_rules
    kw = G.rendering_kwargs
    nhwc, dec = G.renderer._planes_nhwc(planes[:1])[0], G.renderer._decoder_cache(_osg_decoder_weights(G.decoder))
    affine = gv.mesh_to_world_matrix(n, kw['box_warp'])
    affine_dev = torch.tensor(affine, dtype=torch.float32, device=verts.device)         # (the composed route must not copy from the host while captured)
    tol = 2.0 ** -10 * max(1.0, abs(level)) if tol is None else tol
    pts = verts.reshape(1, -1, 3).contiguous()
    V = len(verts)

    def fused():
        return gnerf_hip.project_points_to_level(nhwc, 1, dec, pts, kw['box_warp'], level, affine=affine, steps=STEPS, radius=1.0, tol=tol)

    def field(world):
        sigma = gnerf_hip.query_points(nhwc, 1, dec, world, kw['box_warp'], want_rgb=False)[0]
        return sigma[..., 0], gnerf_hip.query_points_grad(nhwc, 1, dec, world, kw['box_warp'], torch.ones_like(sigma), None)

    def composed():
        return project_to_level_rules(field, pts, level, steps=STEPS, radius=1.0, tol=tol, affine=affine_dev, early_exit=False)

    out, status, res_in, res_out = (t[0] for t in fused())
    c_out, c_status, _, _ = (t[0] for t in composed())
    guarded, g_status, counts = gnerf_hip.mesh_flip_guard(verts, out, faces, status, GUARD_ROUNDS)
    counts = counts.tolist()
    res_after = torch.where(g_status == 3, res_in, res_out)
    tally = torch.bincount(g_status.long(), minlength=4).tolist()
    line = {'case': name, 'vertices': V, 'triangles': len(faces), 'level': level, 'steps': STEPS, 'radius_voxels': 1.0, 'tol': tol,
            'converged_share_before_guard': float((status == 0).sum()) / V, 'status_after_guard': dict(zip(('converged', 'not_converged', 'flat', 'reverted'), tally)),
            'flips_per_round': counts[:GUARD_ROUNDS], 'flips_left': counts[GUARD_ROUNDS],
            'abs_residual_before': stats(res_in), 'abs_residual_after': stats(res_after),
            'composed_route': {'statuses_that_differ': int((c_status != status).sum()), 'max_position_difference_voxels': float((c_out - out).abs().max())},
            'rounds': rounds, 'build': head}
    if time_it:
        ms = {}
        for stage, call in (('fused', fused), ('composed', composed), ('guard', lambda: gnerf_hip.mesh_flip_guard(verts, out, faces, status, GUARD_ROUNDS))):
            med, low = replay_ms(call, rounds)
            ms[stage] = {'median': round(med, 4), 'min': round(low, 4)}
        line['gpu_ms'] = ms
        line['composed_over_fused'] = round(ms['composed']['median'] / ms['fused']['median'], 3)
        line['composed_launches'] = f'{STEPS + 1} x (query_points + query_points_grad) + elementwise'
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--voxel-res', type=int, default=512)
    ap.add_argument('--coarse', type=int, nargs='*', default=[128, 256], help='the coarse grids of the coarse-grid question')
    ap.add_argument('--only', default='', help='only the cases whose name contains this')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mesh_snap.py needs a GPU'
    dev = torch.device('cuda', 0)
    import gen_videos_mi355x as gv
    from bench_mesh import sphere
    head_file = os.path.join(ROOT, 'g-nerf_amd', 'gnerf_hip', 'BUILD_HEAD')
    head = open(head_file).read().strip() if os.path.isfile(head_file) else 'unknown'
    n, level = args.voxel_res, 0.0
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    ws = gv.orbit_latents(G, z, dev)
    vol, planes = gv.extract_density_grid(G, ws, n, return_planes=True)
    # the default tolerance (2^-10 max(1, |level|)) and one scaled to the field, 1e-4 std(sigma) over the volume inside the crop
    tols = {'tol_default': None, 'tol_1e-4_std': 1e-4 * float(vol[vol != 0].std())}
    meshes = [(f'generator_{n}', S.marching_cubes(vol.permute(2, 1, 0).contiguous(), level))]
    del vol
    meshes.append((f'sphere_{n}', S.marching_cubes(sphere(n, dev), 0.0)))
    fine = None
    for name, (verts, faces) in meshes:
        for cell in (0.0, 2.0):
            case = name + (f'_simplified_{cell:g}' if cell else '')
            if args.only not in case:
                continue
            v, f = verts, faces
            if cell:
                simplified = S.simplify_mesh(verts, faces, cell=cell)
                v, f = simplified.verts, simplified.faces
            for tol_name, tol in tols.items():
                line = snap_case(f'{case}_{tol_name}', G, planes, v, f, n, level, args.rounds, head, tol=tol)
                if case == f'generator_{n}' and tol is None:
                    fine = line
    if fine is not None:
        for m in args.coarse:
            vol = gv.extract_density_grid(G, ws, m, planes=planes)
            verts, faces = S.marching_cubes(vol.permute(2, 1, 0).contiguous(), level)
            for tol_name, tol in tols.items():
                line = snap_case(f'generator_{m}_coarse_{tol_name}', G, planes, verts, faces, m, level, args.rounds, head, time_it=False, tol=tol)
                print(json.dumps({'case': f'coarse_grid_{m}_snapped_against_{n}_unsnapped_{tol_name}', 'tol': line['tol'], 'vertices': [line['vertices'], fine['vertices']],
                                  'abs_residual': {f'{m}_unsnapped': line['abs_residual_before'], f'{m}_snapped': line['abs_residual_after'],
                                                   f'{n}_unsnapped': fine['abs_residual_before']},
                                  'point_queries': {f'{m}_snapped_at_most': m ** 3 + (STEPS + 1) * line['vertices'], f'{n}_unsnapped': n ** 3},
                                  'build': head}), flush=True)


if __name__ == '__main__':
    main()
