#!/usr/bin/env python3
"""The multi-view colour bake on the MI355X (csrc/raster.hip, gnerf_mesh_bake_colors, through gnerf_hip.bake_colors): GPU time per call on
the 512^3 mesh of a random-init generator's density volume at level 0 and on its 2-voxel simplification, from 8 and 32 of the orbit's
cameras, visibility buffers and frames at 512^2 (the frames are the rasteriser's own shaded ones: what a frame holds does not change what
the kernel reads), with the mesh's face-derived vertex normals.  The call is captured ten times in a HIP graph whose replay is timed with
HIP events (tools/bench_raster.py's method), median / min over the rounds.  No target: the ratios to two yardsticks are what is recorded.

  (a) the numpy port on the host (shape_mi355x.bake_colors_numpy, one run): the same bits, checked here.
  (b) the call's byte floor at 6.3 TB/s: per vertex its position, normal and fallback read and its colour, weight and view count written
      (38 bytes); every visibility key in the window of a vertex that projects into a view, counted once per view (8 bytes; a hidden
      vertex's window ends at its first failing pixel, so this counts a few keys too many); every texel under the four taps of a
      (vertex, view) that counted, once per view (3 bytes).  Positions are recomputed with torch for the count.

    python tools/bench_mesh_bake.py | tee profiles/rNN_mesh_bake.jsonl"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'g-nerf_amd'), ROOT, os.path.join(ROOT, 'tools')]
import numpy as np
import torch

import gnerf_harness as H
import gnerf_hip
import shape_mi355x as S

HBM = 6.3e12
SIZE = 512


def vertex_normals(verts, faces):
    """Area-weighted face normals summed onto the vertices (any smooth unit field would do: it only feeds the facing test)."""
    v, f = verts.double(), faces.long()
    n = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)
    out = torch.zeros_like(v)
    for k in range(3):
        out.index_add_(0, f[:, k], n)
    return torch.nn.functional.normalize(out, dim=1).float().contiguous()


def touched_bytes(verts, tA, tK, vis, frames, normals, tN, guard):
    """(distinct visibility keys, distinct texels) the call touches, summed over the views (see the module's text)."""
    n, h, w = vis.shape
    fh, fw = frames.shape[1:3]
    keys = texels = 0
    for view in range(n):
        A, K = tA[view].reshape(3, 4), tK[view].reshape(3, 3)
        p = verts @ A[:, :3].T + A[:, 3]
        xc = (K[0, 0] * p[:, 0] + K[0, 1] * p[:, 1]) / p[:, 2] + K[0, 2]
        yc = K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]
        inside = (p[:, 2] > 0.01) & (xc >= 0) & (xc * w < w) & (yc >= 0) & (yc * h < h)
        col, row = (xc[inside] * w).floor().long(), (yc[inside] * h).floor().long()
        mask = torch.zeros(h, w, dtype=torch.bool, device=verts.device)
        for dr in range(-guard, guard + 1):
            for dc in range(-guard, guard + 1):
                mask[(row + dr).clamp(0, h - 1), (col + dc).clamp(0, w - 1)] = True
        keys += int(mask.sum())
        one = gnerf_hip.bake_colors(verts, tA[view:view + 1], tK[view:view + 1], vis[view:view + 1], frames[view:view + 1], normals=normals,
                                    normal_mat=tN[view:view + 1], guard=guard)
        counted = one['seen'] > 0
        x0, y0 = (xc[counted] * fw - 0.5).floor().long(), (yc[counted] * fh - 0.5).floor().long()
        mask = torch.zeros(fh, fw, dtype=torch.bool, device=verts.device)
        for dy in (0, 1):
            for dx in (0, 1):
                mask[(y0 + dy).clamp(0, fh - 1), (x0 + dx).clamp(0, fw - 1)] = True
        texels += int(mask.sum())
    return keys, texels


def bench_case(name, verts, faces, mesh2world, n_views, rounds, head):
    from bench_raster import replay_ms
    dev = verts.device
    labels = H.orbit_labels([(j * 120) // n_views for j in range(n_views)], 120, 2.7)
    A, N = S.mesh_to_camera(labels[:, :16].reshape(-1, 4, 4).numpy(), mesh2world)
    tA, tN = torch.from_numpy(A.reshape(-1, 12)).to(dev), torch.from_numpy(N.reshape(-1, 9)).to(dev)
    tK = labels[:, 16:25].contiguous().to(dev)
    normals = vertex_normals(verts, faces)
    vis, _ = gnerf_hip.rasterize(verts, faces, tA, tK, SIZE)
    frames = gnerf_hip.resolve(vis, verts, faces, tA, tK, normals=normals, normal_mat=tN, outputs=('frame',))['frame']
    fallback = torch.full([len(verts), 3], 128, dtype=torch.uint8, device=dev)
    rules = S.BAKE_RULES
    out = {k: t.clone() for k, t in gnerf_hip.bake_colors(verts, tA, tK, vis, frames, normals=normals, normal_mat=tN, fallback=fallback).items()}
    med, low = replay_ms(lambda: gnerf_hip.bake_colors(verts, tA, tK, vis, frames, normals=normals, normal_mat=tN, fallback=fallback, out=out), rounds)
    host = [t.cpu().numpy() for t in (verts, tA, tK, vis, frames, normals, tN, fallback)]
    t0 = time.perf_counter()
    port = S.bake_colors_numpy(host[0], host[1], host[2], host[3], host[4], normals=host[5], normal_mat=host[6], fallback=host[7])
    port_ms = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(out[k].cpu().numpy().view(np.uint8), port[k].view(np.uint8)) for k in gnerf_hip.BAKE_OUTPUTS)
    keys, texels = touched_bytes(verts, tA, tK, vis, frames, normals, tN, rules['guard'])
    floor_bytes = len(verts) * 38 + keys * 8 + texels * 3
    floor_ms = floor_bytes / HBM * 1e3
    seen = out['seen']
    print(json.dumps({'case': name, 'views': n_views, 'vis_size': SIZE, 'frame_size': SIZE, 'vertices': len(verts), 'triangles': len(faces), 'rules': rules,
                      'seen_share': round(float((seen > 0).float().mean()), 4), 'median_views_per_seen_vertex': float(seen[seen > 0].float().median()),
                      'gpu_ms': {'median': round(med, 4), 'min': round(low, 4)}, 'numpy_port_ms': round(port_ms, 1), 'same_bits_as_port': same,
                      'port_over_gpu': round(port_ms / med, 1), 'touched': {'keys': keys, 'texels': texels, 'bytes': floor_bytes},
                      'floor_ms': round(floor_ms, 5), 'gpu_over_floor': round(med / floor_ms, 2), 'rounds': rounds, 'build': head}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--views', type=int, nargs='+', default=[8, 32])
    ap.add_argument('--voxel-res', type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mesh_bake.py needs a GPU'
    dev = torch.device('cuda', 0)
    import gen_videos_mi355x as gv
    head_file = os.path.join(ROOT, 'g-nerf_amd', 'gnerf_hip', 'BUILD_HEAD')
    head = open(head_file).read().strip() if os.path.isfile(head_file) else 'unknown'
    n = args.voxel_res
    mesh2world = gv.mesh_to_world_matrix(n, 1.0)
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    vol = gv.extract_density_grid(G, gv.orbit_latents(G, z, dev), n).permute(2, 1, 0).contiguous()
    verts, faces = S.marching_cubes(vol, 0.0)
    del vol
    simplified = S.simplify_mesh(verts, faces, cell=2.0)
    for name, v, f in ((f'generator_{n}', verts, faces), (f'generator_{n}_simplified_2', simplified.verts, simplified.faces)):
        for n_views in args.views:
            bench_case(name, v.contiguous(), f.contiguous(), mesh2world, n_views, args.rounds, head)


if __name__ == '__main__':
    main()
