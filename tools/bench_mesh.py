#!/usr/bin/env python3
"""Marching cubes on the MI355X (csrc/mesh.hip): the whole shape_mi355x.marching_cubes call -- count pass, the host read of the counts,
output allocation, emit pass -- on a sphere field and on a random-init generator's 512^3 density volume (what gen_videos_mi355x.py
--mesh meshes), against the traffic floor of its passes, and the numpy port at 128^3 for scale.  One JSON line per case.

Traffic floor: the count pass reads the volume and writes 4 bytes per point, the emit pass reads both again, plus the mesh itself;
priced at 6.3 TB/s."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'g-nerf_amd'), ROOT]
import numpy as np
import torch

import shape_mi355x as S

HBM = 6.3e12


def sphere(n, dev):
    i = torch.arange(n, dtype=torch.float32, device=dev) - (n - 1) / 2
    x, y, z = torch.meshgrid(i, i, i, indexing='ij')
    return (0.4 * n - torch.sqrt(x * x + y * y + z * z)).contiguous()


def timed(vol, level, reps=20):
    for _ in range(3):
        S.marching_cubes(vol, level)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        verts, faces = S.marching_cubes(vol, level)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, verts, faces


def report(name, vol, level):
    dt, verts, faces = timed(vol, level)
    n = vol.numel()
    floor_bytes = 4 * n * 4 + verts.numel() * 4 + faces.numel() * 4
    floor = floor_bytes / HBM
    print(json.dumps({'case': name, 'shape': list(vol.shape), 'level': level, 'vertices': len(verts), 'triangles': len(faces),
                      'ms': round(dt * 1e3, 3), 'Mtriangles_s': round(len(faces) / dt / 1e6, 1), 'floor_ms': round(floor * 1e3, 3),
                      'floor_fraction': round(floor / dt, 3), 'target_ms': 5.0}), flush=True)


def main():
    dev = torch.device('cuda', 0)
    report('sphere', sphere(512, dev), 0.0)
    import gen_videos_mi355x as gv
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    vol = gv.extract_density_grid(G, gv.orbit_latents(G, z, dev), 512).permute(2, 1, 0).contiguous()
    del G
    report('generator_512', vol, 0.0)
    small = vol[::4, ::4, ::4].contiguous().cpu().numpy()
    t0 = time.perf_counter()
    verts, faces = S.marching_cubes_numpy(small, 0.0)
    dt = time.perf_counter() - t0
    print(json.dumps({'case': 'numpy_port_128', 'shape': list(small.shape), 'triangles': len(faces), 'ms': round(dt * 1e3, 1)}), flush=True)


if __name__ == '__main__':
    main()
