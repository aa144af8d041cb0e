#!/usr/bin/env python3
"""The mesh-simplification kernels on the MI355X (csrc/mesh_simplify.hip): GPU time of the count call, the emit call and both on the two 512^3
meshes of tools/bench_mesh.py -- a random-init generator's density volume at level 0 and the sphere -- at cells of 2 and 4 voxels, beside two
yardsticks: the numpy port on the host, and each call's traffic floor (the bytes it must read and write, at 6.3 TB/s); and the rasteriser's
visibility pass (one 256^2 view) on the mesh before and after.

Each call is the native one on preallocated buffers, captured ten times in a HIP graph whose replay is timed with HIP events (the host's
enqueueing, the wrappers' allocations and the host read between the two calls are left out; tools/bench_raster.py's method), median / min
over the rounds.  The emit call issues up to 27 64-bit integer atomics per valid face (nine words into the cluster of each corner) and 4 per
used vertex; words that are zero are not sent, a wave whose lanes share one cluster adds up in registers first, and a block of 1 024 faces or
vertices adds up in LDS before anything goes to memory.
The split of a call into its kernels comes from a kernel trace of `--trace N` (both calls N times per case, eagerly, nothing else), a run
of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_mesh_simplify.py --trace 20 --only sphere --cells 2

Traffic floors (V vertices, T faces, V' / T' left): count 12 V + 12 T read (verts, faces), 8 V + 4 T written (slot and new id per vertex, slot
per face); emit 12 V + 12 T + 4 V + 4 T read, 104 V' written and read (the accumulators), 16 V' + 4 V + 12 T' written.

    python tools/bench_mesh_simplify.py | tee profiles/rNN_mesh_simplify.jsonl"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'g-nerf_amd'), ROOT, os.path.join(ROOT, 'tools')]
import numpy as np
import torch

import gnerf_hip
import shape_mi355x as S
from gnerf_hip._native import _launch, _ptr

HBM = 6.3e12


class Calls:
    """The two native calls of one mesh and one cell on buffers allocated once."""

    def __init__(self, verts, faces, cell, origin):
        self.v, self.f = verts, faces
        self.nv, self.nt = len(verts), len(faces)
        dev = verts.device
        self.ws = torch.empty(gnerf_hip.mesh_simplify_workspace_bytes(self.nv, self.nt), dtype=torch.uint8, device=dev)
        self.counts = torch.empty(8, dtype=torch.int64, device=dev)
        self.mesh = (_ptr(self.v), _ptr(self.f), self.nv, self.nt, float(cell), (ctypes.c_float * 3)(*origin), _ptr(self.ws))
        self.count()
        self.report = self.counts.tolist()
        kv, kt = self.report[:2]
        self.out_v = torch.empty([kv, 3], dtype=torch.float32, device=dev)
        self.out_f = torch.empty([max(kt, 1), 3], dtype=torch.int32, device=dev)
        self.src = torch.empty(kv, dtype=torch.int32, device=dev)
        self.vmap = torch.empty(self.nv, dtype=torch.int32, device=dev)

    def count(self):
        _launch('gnerf_mesh_simplify_count', self.v, *self.mesh, _ptr(self.counts))

    def emit(self):
        _launch('gnerf_mesh_simplify_emit', self.v, *self.mesh, _ptr(self.out_v), _ptr(self.out_f), _ptr(self.src), _ptr(self.vmap))

    def both(self):
        self.count()
        self.emit()


def visibility_ms(verts, faces, tA, tK, size, rounds):
    from bench_raster import replay_ms
    ws = torch.empty(gnerf_hip.raster_workspace_bytes(len(verts), len(faces), 1, size), dtype=torch.uint8, device=verts.device)
    vis = torch.empty([1, size, size], dtype=torch.int64, device=verts.device)
    gnerf_hip.rasterize(verts, faces, tA, tK, size, workspace=ws, vis=vis)
    med, low = replay_ms(lambda: gnerf_hip.rasterize(verts, faces, tA, tK, size, workspace=ws, vis=vis), rounds)
    return {'median': round(med, 4), 'min': round(low, 4)}


def bench(name, verts, faces, cell, rounds, head, host, camera, before):
    from bench_mesh_clean import host_ms
    from bench_raster import replay_ms
    origin = [float(x) for x in verts.min(dim=0).values.cpu()]
    st = Calls(verts, faces, cell, origin)
    V, T = st.nv, st.nt
    kv, kt = st.report[:2]
    ms = {}
    for stage, call in (('count', st.count), ('emit', st.emit), ('count_and_emit', st.both)):
        med, low = replay_ms(call, rounds)
        ms[stage] = {'median': round(med, 4), 'min': round(low, 4)}
    floors = {'count': (20 * V + 16 * T) / HBM * 1e3, 'emit': (20 * V + 16 * T + 224 * kv + 12 * kt) / HBM * 1e3}
    line = {'case': name, 'cell_voxels': cell, 'vertices': V, 'triangles': T, 'counts': st.report, 'left_vertices': kv, 'left_triangles': kt,
            'gpu_ms': ms, 'floor_ms': {k: round(x, 5) for k, x in floors.items()},
            'floor_fraction': {k: round(floors[k] / ms[k]['median'], 4) for k in floors},
            'atomics_64bit_issued_at_most': {'per_face': 27, 'per_vertex': 4, 'in_all': 27 * (T - st.report[2]) + 4 * V},
            'visibility_256_ms': {'before': before, 'after': visibility_ms(st.out_v, st.out_f[:kt].contiguous(), *camera, 256, rounds)},
            'rounds': rounds, 'build': head}
    if host:
        hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
        made = {}
        line['numpy_port_ms'] = {'count': round(host_ms(lambda: S.mesh_simplify_numpy(hv, hf, cell, origin, count_only=True), 1), 1),
                                 'count_and_emit': round(host_ms(lambda: made.update(m=S.mesh_simplify_numpy(hv, hf, cell, origin)), 1), 1)}
        same = all(np.array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))
                   for a, b in zip(made['m'][:4], (st.out_v, st.out_f[:kt], st.src, st.vmap))) and made['m'][4].tolist() == st.report
        line['same_bits_as_the_port'] = bool(same)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--voxel-res', type=int, default=512)
    ap.add_argument('--cells', type=float, nargs='+', default=[2.0, 4.0], help='cells, in voxels')
    ap.add_argument('--no-host', action='store_true', help='skip the numpy port on the host')
    ap.add_argument('--only', default='', help='only the meshes whose name contains this (generator / sphere)')
    ap.add_argument('--trace', type=int, default=0, help='run both calls this many times per case eagerly and nothing else (for a kernel trace)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mesh_simplify.py needs a GPU'
    dev = torch.device('cuda', 0)
    import gen_videos_mi355x as gv
    import gnerf_harness as H
    from bench_mesh import sphere
    head_file = os.path.join(ROOT, 'g-nerf_amd', 'gnerf_hip', 'BUILD_HEAD')
    head = open(head_file).read().strip() if os.path.isfile(head_file) else 'unknown'
    n = args.voxel_res
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    vol = gv.extract_density_grid(G, gv.orbit_latents(G, z, dev), n).permute(2, 1, 0).contiguous()
    del G
    meshes = [(f'generator_{n}', S.marching_cubes(vol, 0.0))]
    del vol
    meshes.append((f'sphere_{n}', S.marching_cubes(sphere(n, dev), 0.0)))
    labels = H.orbit_labels(range(1), 120, 2.7)
    A, _ = S.mesh_to_camera(labels[:, :16].reshape(-1, 4, 4).numpy(), gv.mesh_to_world_matrix(n, 1.0))
    camera = torch.from_numpy(A.reshape(-1, 12)).to(dev), labels[:, 16:25].contiguous().to(dev)
    for name, (verts, faces) in meshes:
        if args.only not in name:
            continue
        before = None if args.trace else visibility_ms(verts, faces, *camera, 256, args.rounds)
        for cell in args.cells:
            if args.trace:
                st = Calls(verts, faces, cell, [float(x) for x in verts.min(dim=0).values.cpu()])
                for _ in range(args.trace):
                    st.both()
                torch.cuda.synchronize()
            else:
                bench(name, verts, faces, cell, args.rounds, head, not args.no_host, camera, before)


if __name__ == '__main__':
    main()
