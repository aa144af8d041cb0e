#!/usr/bin/env python3
"""The triangle rasteriser on the MI355X (csrc/raster.hip through gnerf_hip.rasterize / resolve): GPU time per view of the visibility pass
(init + thread-per-triangle + queued launches) and of the resolve pass (shaded frame only, as gen_videos_mi355x.py --geometry-out asks),
on the 512^3 meshes the project extracts -- a random-init generator's density volume at level 0 and tools/bench_mesh.py's sphere --
drawn from the orbit's cameras at 64^2, 256^2 and 512^2, 1 and 8 views per call.  Each pass is captured ten times in a HIP graph and the
replay is timed with HIP events (the host's enqueueing is left out); min / median over the rounds.  One JSON line per case, then the orbit's
RGB frame time from the same process for scale.

Traffic floor: the mesh read once per view (12 bytes per vertex, 12 per triangle) plus the visibility buffer written once and read once
(8 bytes per pixel each way) for the visibility pass; the buffer read and the frame written for the resolve pass; priced at 6.3 TB/s.  The
sphere (radius 0.4 of the box) overflows the orbit's field of view: part of it is clipped, as a close-up would be.

    python tools/bench_raster.py | tee profiles/rNN_raster.jsonl"""
import argparse
import json
import os
import statistics
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
CAPTURED = 10


def replay_ms(call, rounds):
    """Median and min GPU milliseconds of one `call`, from replays of a graph that holds CAPTURED of them."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(CAPTURED):
            call()
    graph.replay()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / CAPTURED)
    return statistics.median(ms), min(ms)


def bench_mesh(name, verts, faces, mesh2world, sizes, views, rounds, dev, head):
    radius = 2.7
    for n_views in views:
        labels = H.orbit_labels(range(0, 120, 120 // n_views)[:n_views], 120, radius)
        A, _ = S.mesh_to_camera(labels[:, :16].reshape(-1, 4, 4).numpy(), mesh2world)
        tA = torch.from_numpy(A.reshape(-1, 12)).to(dev)
        tK = labels[:, 16:25].contiguous().to(dev)
        for size in sizes:
            ws = torch.empty(gnerf_hip.raster_workspace_bytes(len(verts), len(faces), n_views, size), dtype=torch.uint8, device=dev)
            vis = torch.empty([n_views, size, size], dtype=torch.int64, device=dev)
            _, counts = gnerf_hip.rasterize(verts, faces, tA, tK, size, workspace=ws, vis=vis)
            vis_ms, vis_min = replay_ms(lambda: gnerf_hip.rasterize(verts, faces, tA, tK, size, workspace=ws, vis=vis), rounds)
            gnerf_hip.rasterize(verts, faces, tA, tK, size, workspace=ws, vis=vis)
            res_ms, res_min = replay_ms(lambda: gnerf_hip.resolve(vis, verts, faces, tA, tK, outputs=('frame',)), rounds)
            covered = int((vis != -1).sum())
            queued = int(ws[:4].view(torch.int32)[0])
            pixels = n_views * size * size
            vis_floor = (n_views * (verts.numel() * 4 + faces.numel() * 4) + pixels * 16) / HBM * 1e3
            res_floor = (pixels * 8 + pixels * 3) / HBM * 1e3
            print(json.dumps({'case': name, 'size': size, 'views_per_call': n_views, 'vertices': len(verts), 'triangles': len(faces),
                              'counts_drawn_near_guard_culled': counts.tolist(), 'queued_large_triangles': queued,
                              'covered_pixel_fraction': round(covered / pixels, 4),
                              'visibility_ms_per_view': {'median': round(vis_ms / n_views, 4), 'min': round(vis_min / n_views, 4)},
                              'resolve_ms_per_view': {'median': round(res_ms / n_views, 4), 'min': round(res_min / n_views, 4)},
                              'Mtriangles_per_s': round(len(faces) * n_views / vis_ms / 1e3, 1),
                              'visibility_floor_ms_per_view': round(vis_floor / n_views, 5), 'resolve_floor_ms_per_view': round(res_floor / n_views, 6),
                              'visibility_floor_fraction': round(vis_floor / vis_ms, 4), 'rounds': rounds, 'build': head}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--sizes', type=int, nargs='+', default=[64, 256, 512])
    ap.add_argument('--views', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--voxel-res', type=int, default=512)
    ap.add_argument('--orbit-frames', type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_raster.py needs a GPU'
    dev = torch.device('cuda', 0)
    import gen_videos_mi355x as gv
    from bench_mesh import sphere
    head_file = os.path.join(ROOT, 'g-nerf_amd', 'gnerf_hip', 'BUILD_HEAD')
    head = open(head_file).read().strip() if os.path.isfile(head_file) else 'unknown'
    n = args.voxel_res
    mesh2world = gv.mesh_to_world_matrix(n, 1.0)
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    vol = gv.extract_density_grid(G, gv.orbit_latents(G, z, dev), n).permute(2, 1, 0).contiguous()
    verts, faces = S.marching_cubes(vol, 0.0)
    del vol
    bench_mesh(f'generator_{n}', verts, faces, mesh2world, args.sizes, args.views, args.rounds, dev, head)
    verts, faces = S.marching_cubes(sphere(n, dev), 0.0)
    bench_mesh(f'sphere_{n}', verts, faces, mesh2world, args.sizes, args.views, args.rounds, dev, head)
    del verts, faces
    torch.cuda.empty_cache()
    # the orbit's RGB frames from the same process, for scale (eager, one camera per call, the CLI's doubled depth resolutions)
    gv.render_orbit(G, z, args.orbit_frames, 64, dev, rank=0, world=args.orbit_frames, double_depth=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frames, _, _ = gv.render_orbit(G, z, args.orbit_frames, 64, dev, double_depth=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({'case': 'orbit_rgb_frame', 'frames': args.orbit_frames, 'neural_rendering': 64, 'image': list(frames.shape[1:3]),
                      'ms_per_frame': round(dt / args.orbit_frames * 1e3, 3), 'device': torch.cuda.get_device_name(0), 'build': head}), flush=True)


if __name__ == '__main__':
    main()
