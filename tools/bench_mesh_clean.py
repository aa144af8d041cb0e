#!/usr/bin/env python3
"""The mesh-cleaning kernels on the MI355X (csrc/mesh_clean.hip): GPU time of each stage on the two 512^3 meshes of tools/bench_mesh.py and
tools/bench_raster.py -- a random-init generator's density volume at level 0 and the sphere -- beside two yardsticks: the same stage of
the numpy port on the host, and the stage's traffic floor (the bytes it must read and write, at 6.3 TB/s).

Stages, each the native call(s) on preallocated buffers, captured ten times in a HIP graph whose replay is timed with HIP events (the host's
enqueueing and the wrappers' allocations are left out; tools/bench_raster.py's method), median / min over the rounds:
  components   gnerf_mesh_components: init, hook (the union-find), flatten, faces_of, tally.
  compaction   gnerf_mesh_compact_count + _emit for keep_largest = 1, without the host read between them (the sizes are known from a first run).
  smooth_1/11  gnerf_mesh_smooth with 1 and with 11 iterations.  Ten Taubin iterations = their difference; the adjacency build (degrees, row
               starts, fill, sort + pin flags) = smooth_1 minus one iteration.
The host yardstick times each stage of the numpy port once or twice; its ten-iteration figure is EXTRAPOLATED, ten times one measured
iteration (a one-iteration call minus the adjacency build: `taubin_10_from_one_iteration`).
The split of a call into its kernels (faces_of alone, the hook alone, ...) comes from a kernel trace of `--trace N` (every stage N times,
eagerly, nothing else), a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_mesh_clean.py --trace 20

Traffic floors (V vertices, T faces, V' / T' kept): components 12 T read + 8 V written (label, faces_of); faces_of alone 12 T + 4 V read, 4 V
written; compaction 12 V + 12 T + 9 V read (verts, faces, label, faces_of, keep), 16 V' + 12 T' written; adjacency 12 T read, 24 T + 5 V written
(rows, degrees, pin flags); a half-step 24 T + 12 V + 5 V read, 12 V written.

    python tools/bench_mesh_clean.py | tee profiles/rNN_mesh_clean.jsonl"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'g-nerf_amd'), ROOT, os.path.join(ROOT, 'tools')]
import numpy as np
import torch

import gnerf_hip
import shape_mi355x as S
from gnerf_hip._native import _launch, _ptr

HBM = 6.3e12


class Stages:
    """The native calls of one mesh on buffers allocated once."""

    def __init__(self, verts, faces):
        self.v, self.f = verts, faces
        self.nv, self.nt = len(verts), len(faces)
        dev = verts.device
        self.ws = torch.empty(gnerf_hip.mesh_workspace_bytes(self.nv, self.nt), dtype=torch.uint8, device=dev)
        self.label = torch.empty(self.nv, dtype=torch.int32, device=dev)
        self.faces_of = torch.empty(self.nv, dtype=torch.int32, device=dev)
        self.counts = torch.empty(3, dtype=torch.int64, device=dev)
        self.components()
        torch.cuda.synchronize()
        self.report = self.counts.tolist()
        self.keep = torch.zeros(self.nv, dtype=torch.uint8, device=dev)
        self.keep[int(self.faces_of.argmax())] = 1                           # keep_largest = 1 (ties aside: a benchmark)
        self.kept = torch.empty(2, dtype=torch.int64, device=dev)
        _launch('gnerf_mesh_compact_count', self.v, *self._mesh(), _ptr(self.kept))
        self.kv, self.kt = (int(c) for c in self.kept.tolist())
        self.out_v = torch.empty([self.kv, 3], dtype=torch.float32, device=dev)
        self.out_f = torch.empty([self.kt, 3], dtype=torch.int32, device=dev)
        self.src = torch.empty(self.kv, dtype=torch.int32, device=dev)
        self.smoothed = torch.empty_like(verts)

    def _mesh(self):
        return _ptr(self.f), self.nv, self.nt, _ptr(self.label), _ptr(self.faces_of), _ptr(self.keep), _ptr(self.ws)

    def components(self):
        _launch('gnerf_mesh_components', self.f, _ptr(self.f), self.nv, self.nt, _ptr(self.ws), _ptr(self.label), _ptr(self.faces_of), _ptr(self.counts))

    def compaction(self):
        _launch('gnerf_mesh_compact_count', self.v, *self._mesh(), _ptr(self.kept))
        _launch('gnerf_mesh_compact_emit', self.v, _ptr(self.v), *self._mesh(), _ptr(self.out_v), _ptr(self.out_f), _ptr(self.src))

    def smooth(self, iterations):
        _launch('gnerf_mesh_smooth', self.v, _ptr(self.v), self.nv, _ptr(self.f), self.nt, iterations, 0.5, -0.53, 1, _ptr(self.ws), _ptr(self.smoothed))


def host_ms(fn, reps=2):
    best = 1e30
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def bench(name, verts, faces, rounds, head, host):
    from bench_raster import replay_ms
    st = Stages(verts, faces)
    V, T, kv, kt = st.nv, st.nt, st.kv, st.kt
    ms = {}
    for stage, call in (('components', st.components), ('compaction', st.compaction), ('smooth_1', lambda: st.smooth(1)), ('smooth_11', lambda: st.smooth(11))):
        med, low = replay_ms(call, rounds)
        ms[stage] = {'median': round(med, 4), 'min': round(low, 4)}
    st.components()                                                          # (the smoothing shares the workspace; leave the labels valid)
    ten = ms['smooth_11']['median'] - ms['smooth_1']['median']
    build = ms['smooth_1']['median'] - ten / 10
    floors = {'components': (12 * T + 8 * V) / HBM * 1e3, 'faces_of': (12 * T + 8 * V) / HBM * 1e3,
              'compaction': (21 * V + 12 * T + 16 * kv + 12 * kt) / HBM * 1e3, 'adjacency_build': (36 * T + 5 * V) / HBM * 1e3,
              'taubin_10': 20 * (24 * T + 29 * V) / HBM * 1e3}
    line = {'case': name, 'vertices': V, 'triangles': T, 'components_unused_bad': st.report, 'kept_vertices': kv, 'kept_triangles': kt,
            'gpu_ms': dict(ms, taubin_10={'median': round(ten, 4)}, adjacency_build={'median': round(build, 4)}),
            'floor_ms': {k: round(x, 5) for k, x in floors.items()},
            'floor_fraction': {k: round(floors[k] / m, 4) for k, m in (('components', ms['components']['median']), ('compaction', ms['compaction']['median']),
                                                                         ('adjacency_build', build), ('taubin_10', ten)) if m > 0},
            'rounds': rounds, 'build': head}
    if host:
        hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
        made = {}
        line['numpy_port_ms'] = {
            'components': round(host_ms(lambda: made.update(c=S.mesh_components_numpy(hf, V)), 1), 1)}
        label, faces_of, _ = made['c']
        line['numpy_port_ms']['faces_of'] = round(host_ms(lambda: np.bincount(label[hf[:, 0]], minlength=V)), 2)
        keep = np.zeros(V, np.uint8)
        keep[S.mesh_select(faces_of, keep_largest=1)] = 1
        line['numpy_port_ms']['compaction'] = round(host_ms(lambda: S.mesh_compact_numpy(hv, hf, label, faces_of, keep)), 1)
        line['numpy_port_ms']['adjacency_build'] = round(host_ms(lambda: S._mesh_rows(hf, V), 1), 1)
        one = host_ms(lambda: S.mesh_smooth_numpy(hv, hf, 1), 1)
        line['numpy_port_ms']['taubin_10_from_one_iteration'] = round((one - line['numpy_port_ms']['adjacency_build']) * 10, 1)
    print(json.dumps(line), flush=True)


def trace(verts, faces, n):
    st = Stages(verts, faces)
    for _ in range(n):
        st.components()
        st.compaction()
        st.smooth(1)
    st.components()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--voxel-res', type=int, default=512)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy port on the host')
    ap.add_argument('--trace', type=int, default=0, help='run every stage this many times eagerly and nothing else (for a kernel trace)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mesh_clean.py needs a GPU'
    dev = torch.device('cuda', 0)
    import gen_videos_mi355x as gv
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
    for name, (verts, faces) in meshes:
        if args.trace:
            trace(verts, faces, args.trace)
        else:
            bench(name, verts, faces, args.rounds, head, not args.no_host)


if __name__ == '__main__':
    main()
