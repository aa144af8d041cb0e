#!/usr/bin/env python3
"""The texture bake on the MI355X (csrc/raster.hip, gnerf_mesh_bake_texture, through gnerf_hip.bake_texture): GPU time per call on the 512^3
mesh of a random-init generator's density volume at level 0, simplified at 2 and at 4 voxels, patch 8, from 8 and 32 of the orbit's cameras,
visibility buffers and frames at 512^2 (the frames are the rasteriser's own shaded ones: what a frame holds does not change what the kernel
reads), with the mesh's face-derived vertex normals.  The call is captured ten times in a HIP graph whose replay is timed with HIP events
(tools/bench_raster.py's method), median / min over the rounds.  No target time: what is recorded is

  (a) the vertex bake (gnerf_hip.bake_colors) on the same mesh and views IN THE SAME PROCESS, and both kernels' time per (point, view):
      the two are built from one stage function, so this is the figure to judge the texel mapping by;
  (b) the textured resolve of the baked atlas from the same views, for scale;
  (c) the numpy port (shape_mi355x.bake_texture_numpy) on the mesh's first --port-faces triangles against the kernel on the same sub-mesh:
      the same bits, checked here, and the port's time per (texel, view);
  (d) the call's byte floor at 6.3 TB/s: faces, positions, normals and fallback read once (12 bytes a triangle, 27 a vertex), every texel of
      the atlas written (3 + 4 + 4 bytes), every visibility key in the window of an owned texel that projects into a view, counted once per
      view (8 bytes), every frame texel under the four taps of a (texel, view) that counted, once per view (3 bytes); tools/bench_mesh_bake.py's
      count, on the texels' points.

    python tools/bench_mesh_texture.py        # writes the next free profiles/rNN_mesh_texture.jsonl (or --out)"""
import argparse
import glob
import json
import os
import re
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


def next_profile():
    taken = [int(m.group(1)) for m in (re.match(r'r(\d+)_', os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, 'profiles', 'r*_*'))) if m]
    return os.path.join(ROOT, 'profiles', f'r{max(taken, default=0) + 1:02d}_mesh_texture.jsonl')


def texel_points(verts, faces, normals, patch):
    """(points [M, 3], normals [M, 3]) of the owned texels, on verts' device (float32 by torch: for the traffic count, not for bits)."""
    tri, li, lj = S._atlas_texels(len(faces), patch)
    own = tri.ravel() >= 0
    dev = verts.device
    t = torch.from_numpy(tri.ravel()[own]).to(dev)
    b1 = torch.from_numpy(li.ravel()[own].astype(np.float32)).to(dev) / (patch - 3)
    b2 = torch.from_numpy(lj.ravel()[own].astype(np.float32)).to(dev) / (patch - 3)
    b0 = 1 - b1 - b2
    g = faces.long()[t]

    def mix(x):
        return b0[:, None] * x[g[:, 0]] + b1[:, None] * x[g[:, 1]] + b2[:, None] * x[g[:, 2]]
    return mix(verts).contiguous(), mix(normals).contiguous()


def bench_case(name, verts, faces, mesh2world, n_views, patch, rounds, port_faces, head, emit):
    from bench_mesh_bake import touched_bytes, vertex_normals
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
    kw = dict(normals=normals, normal_mat=tN, fallback=fallback)
    out = {k: t.clone() for k, t in gnerf_hip.bake_texture(verts, faces, tA, tK, vis, frames, patch=patch, **kw).items()}
    med, low = replay_ms(lambda: gnerf_hip.bake_texture(verts, faces, tA, tK, vis, frames, patch=patch, out=out, **kw), rounds)
    vout = {k: t.clone() for k, t in gnerf_hip.bake_colors(verts, tA, tK, vis, frames, **kw).items()}
    vmed, vlow = replay_ms(lambda: gnerf_hip.bake_colors(verts, tA, tK, vis, frames, out=vout, **kw), rounds)
    rmed, rlow = replay_ms(lambda: gnerf_hip.resolve_textured(vis, verts, faces, tA, tK, out['texture'], patch=patch), rounds)
    seen = out['seen']
    th, tw = seen.shape
    owned = int((seen >= 0).sum())
    # the port, on a sub-mesh (its atlas is its own: the kernel bakes the same sub-mesh for the comparison; the visibility buffers stay the whole mesh's)
    sub = faces[:port_faces].contiguous()
    sub_out = gnerf_hip.bake_texture(verts, sub, tA, tK, vis, frames, patch=patch, **kw)
    host = [t.cpu().numpy() for t in (verts, sub, tA, tK, vis, frames, normals, tN, fallback)]
    t0 = time.perf_counter()
    port = S.bake_texture_numpy(host[0], host[1], host[2], host[3], host[4], host[5], patch=patch, normals=host[6], normal_mat=host[7], fallback=host[8])
    port_ms = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(sub_out[k].cpu().numpy().view(np.uint8), port[k].view(np.uint8)) for k in gnerf_hip.TEXTURE_OUTPUTS)
    sub_owned = int((port['seen'] >= 0).sum())
    points, point_normals = texel_points(verts, faces, normals, patch)
    keys, texels = touched_bytes(points, tA, tK, vis, frames, point_normals, tN, rules['guard'])
    floor_bytes = len(faces) * 12 + len(verts) * 27 + th * tw * 11 + keys * 8 + texels * 3
    floor_ms = floor_bytes / HBM * 1e3
    per_texel_view = med * 1e9 / (owned * n_views)                                       # picoseconds
    per_vertex_view = vmed * 1e9 / (len(verts) * n_views)
    emit({'case': name, 'views': n_views, 'patch': patch, 'vis_size': SIZE, 'frame_size': SIZE, 'vertices': len(verts), 'triangles': len(faces),
          'atlas': [th, tw], 'owned_texels': owned, 'rules': rules, 'seen_share': round(float((seen > 0).sum()) / owned, 4),
          'median_views_per_seen_texel': float(seen[seen > 0].float().median()),
          'texture_gpu_ms': {'median': round(med, 4), 'min': round(low, 4)}, 'vertex_bake_gpu_ms': {'median': round(vmed, 4), 'min': round(vlow, 4)},
          'ps_per_texel_view': round(per_texel_view, 2), 'ps_per_vertex_view': round(per_vertex_view, 2),
          'texel_over_vertex': round(per_texel_view / per_vertex_view, 3),
          'resolve_textured_gpu_ms': {'median': round(rmed, 4), 'min': round(rlow, 4)},
          'numpy_port': {'faces': len(sub), 'owned_texels': sub_owned, 'ms': round(port_ms, 1), 'ns_per_texel_view': round(port_ms * 1e6 / (sub_owned * n_views), 1),
                         'same_bits_as_kernel': same},
          'touched': {'keys': keys, 'texels': texels, 'bytes': floor_bytes}, 'floor_ms': round(floor_ms, 5), 'gpu_over_floor': round(med / floor_ms, 2),
          'rounds': rounds, 'build': head})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--views', type=int, nargs='+', default=[8, 32])
    ap.add_argument('--cells', type=float, nargs='+', default=[2.0, 4.0], help='simplification cells in voxels')
    ap.add_argument('--patch', type=int, default=8)
    ap.add_argument('--voxel-res', type=int, default=512)
    ap.add_argument('--port-faces', type=int, default=4096, help='the numpy port runs on this many of the mesh\'s first triangles')
    ap.add_argument('--out', default=None, help='the JSON lines go here (default: the next free profiles/rNN_mesh_texture.jsonl)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mesh_texture.py needs a GPU'
    dev = torch.device('cuda', 0)
    import gen_videos_mi355x as gv
    head_file = os.path.join(ROOT, 'g-nerf_amd', 'gnerf_hip', 'BUILD_HEAD')
    head = open(head_file).read().strip() if os.path.isfile(head_file) else 'unknown'
    path = args.out or next_profile()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    n = args.voxel_res
    mesh2world = gv.mesh_to_world_matrix(n, 1.0)
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    vol = gv.extract_density_grid(G, gv.orbit_latents(G, z, dev), n).permute(2, 1, 0).contiguous()
    verts, faces = S.marching_cubes(vol, 0.0)
    del vol
    with open(path, 'w') as f:
        def emit(record):
            line = json.dumps(record)
            print(line, flush=True)
            f.write(line + '\n')
            f.flush()
        for cell in args.cells:
            simplified = S.simplify_mesh(verts, faces, cell=cell)
            for n_views in args.views:
                bench_case(f'generator_{n}_simplified_{cell:g}', simplified.verts.contiguous(), simplified.faces.contiguous(), mesh2world, n_views, args.patch,
                           args.rounds, args.port_faces, head, emit)
    print(f'-> {path}')


if __name__ == '__main__':
    main()
