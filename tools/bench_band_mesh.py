#!/usr/bin/env python3
"""The brick-wise band mesh on the MI355X (csrc/mesh_band_cubes.hip) against the route it replaces, in one process: the 512^3
volume of a random-init generator at level 0 under extract_density_grid's crop, and the sphere of tools/bench_mesh.py.

  parent   from the planes (the sphere: from its field) to (verts, faces) as --mesh-band makes them: extract_density_grid(band=s) +
           mesh_of_density_grid with no stages -- the whole call, then split, with a synchronise around every part, into the band call (rounds
           and fill), the flip + crop copies, the transpose copy and marching cubes.
  direct   extract_band_mesh (the sphere: shape_mi355x.band_mesh in the pipeline's view) -- the whole call, then split into the rounds
           (no fill), count + scan and emit.
The two meshes are compared with torch.equal first: the tool stops when they differ.  Every time is the median (and min) of --rounds warm calls,
a host clock around work that ends in a device synchronise; the split runs synchronise around every part, so they do not add up to the whole
call exactly.  The floor of count + emit is the bytes of the visited points, read once per pass, plus the outputs, at HBM_TBS.
One pair at n = 1024 on the sphere: both routes' whole calls and their peak allocations (torch.cuda.max_memory_allocated above what the field
itself holds).  The sphere has no generator behind it: its field is a gather from the dense volume.

    python tools/bench_band_mesh.py | tee profiles/rNN_band_mesh.jsonl"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'g-nerf_amd'), ROOT, os.path.join(ROOT, 'tools')]
import torch

import gnerf_hip
import shape_mi355x as S
from gnerf_hip._native import _launch, _ptr

HBM_TBS = 6.3                                                           # the project's figure for streaming reads (README)
VIEW = S.BAND_MESH_PIPELINE_VIEW
# what the parent's route does to the n^3 volume between the queries and the triangles, pass by pass
PARENT_PASSES = ['band_fill: write', 'flip(0): read + write', 'crop clone: read + write (with a crop)', 'permute(2, 1, 0).contiguous(): read + write',
                 'marching cubes count: read, and a 4-byte word per point written', 'marching cubes emit: read, and the words read']


def clock(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def timed_ms(call, rounds, warm=2):
    for _ in range(warm):
        call()
    ms = [clock(call)[1] for _ in range(rounds)]
    return {'median': round(statistics.median(ms), 3), 'min': round(min(ms), 3)}


def med(values):
    return round(statistics.median(values), 3)


def crop_of(keep_crop, n):
    """extract_density_grid's crop of the flipped volume (ranges: three (front, back) or None), as the function itself does it."""
    def apply(vol):
        if keep_crop is None:
            return vol
        (a0, b0), (a1, b1), (a2, b2) = keep_crop
        vol = vol.clone()
        vol[:a0] = 0
        vol[-b0:] = 0
        vol[:, :a1] = 0
        vol[:, -b1:] = 0
        vol[:, :, :a2] = 0
        vol[:, :, -b2:] = 0
        return vol
    return apply


def parent_route(field, n, level, s, keep, crop):
    """extract_density_grid(band=s) + mesh_of_density_grid on a field: band call, flip, crop, transpose, marching cubes."""
    vol, _ = S.band_volume(field, n, level, s, keep, device='cuda')
    return gnerf_hip.marching_cubes(crop(vol.reshape(n, n, n).flip(0)).permute(2, 1, 0).contiguous(), level)


def parent_split(field, n, level, s, keep, crop, rounds):
    parts = {'band_call': [], 'flip_crop_copies': [], 'transpose_copy': [], 'marching_cubes': []}
    for _ in range(rounds):
        (vol, _), ms = clock(lambda: S.band_volume(field, n, level, s, keep, device='cuda'))
        parts['band_call'].append(ms)
        flipped, ms = clock(lambda: crop(vol.reshape(n, n, n).flip(0)))
        parts['flip_crop_copies'].append(ms)
        turned, ms = clock(lambda: flipped.permute(2, 1, 0).contiguous())
        parts['transpose_copy'].append(ms)
        _, ms = clock(lambda: gnerf_hip.marching_cubes(turned, level))
        parts['marching_cubes'].append(ms)
        del vol, flipped, turned
    return {k: med(v) for k, v in parts.items()}


def direct_split(field, n, level, s, keep, rounds):
    """The direct route's parts: the rounds without the fill, gnerf_band_mesh_count (bricks, count, scans), gnerf_band_mesh_emit."""
    dev = torch.device('cuda', 0)
    parts = {'rounds': [], 'count_scan': [], 'emit': []}
    coarse = torch.from_numpy(S.band_coarse_index(n, s)).to(dev)
    kept = (ctypes.c_int * 6)(*gnerf_hip.mesh._band_keep(n, keep))
    perm, flip = (ctypes.c_int * 3)(*VIEW['perm']), (ctypes.c_int * 3)(*[int(f) for f in VIEW['flip']])
    for _ in range(rounds):
        vol = torch.empty(n ** 3, dtype=torch.float32, device=dev)
        band = gnerf_hip.BandVolume(vol, n, s, level, keep)
        report, ms = clock(lambda: S._band_driver(n, s, lambda index: field(index, vol) if len(index) else None, coarse, band, None, fill=False))
        parts['rounds'].append(ms)
        active = report['seeds'] + sum(report['new_bricks'])
        ws = torch.empty(gnerf_hip.band_mesh_workspace_bytes(n, s, active), dtype=torch.uint8, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        view = (n, s, float(level), kept, perm, flip, active, _ptr(ws))
        host, ms = clock(lambda: (_launch('gnerf_band_mesh_count', vol, _ptr(vol), _ptr(band.state), *view, _ptr(counts)), counts.cpu())[1])
        parts['count_scan'].append(ms)
        nv, nt, bad, visited = (int(c) for c in host)
        assert bad == 0 and nv > 0
        verts = torch.empty([nv, 3], dtype=torch.float32, device=dev)
        faces = torch.empty([nt, 3], dtype=torch.int32, device=dev)
        _, ms = clock(lambda: _launch('gnerf_band_mesh_emit', vol, _ptr(vol), _ptr(band.state), *view, _ptr(verts), _ptr(faces)))
        parts['emit'].append(ms)
    out = {k: med(v) for k, v in parts.items()}
    floor_bytes = 2 * 4 * visited + 12 * nv + 12 * nt
    floor_ms = floor_bytes / (HBM_TBS * 1e12) * 1e3
    return out, dict(active=active, visited=visited, workspace_bytes=int(ws.numel()), floor_bytes=floor_bytes, floor_ms=round(floor_ms, 4),
                     count_emit_over_floor=round((out['count_scan'] + out['emit']) / floor_ms, 1))


def same(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def report_case(name, n, level, s, parent, direct, field, keep, crop, rounds, head, full):
    want, got = parent(), direct()
    assert same(want, got), f'{name} s = {s}: the direct mesh is not the parent route\'s'
    assert same(got, direct()), f'{name} s = {s}: two direct runs differ'
    a, b = [], []
    for call in (parent, direct):                                       # warm both, then alternate them
        call(); call()
    for _ in range(rounds):
        a.append(clock(parent)[1])
        b.append(clock(direct)[1])
    line = {'case': f'{name}_{n}_s{s}', 'level': level, 'mesh': [len(got[0]), len(got[1])], 'same_mesh': True,
            'parent_ms': {'median': med(a), 'min': round(min(a), 3)}, 'direct_ms': {'median': med(b), 'min': round(min(b), 3)},
            'parent_over_direct': round(statistics.median(a) / statistics.median(b), 2)}
    if full:
        line['parent_split_ms_synchronised'] = parent_split(field, n, level, s, keep, crop, rounds)
        line['direct_split_ms_synchronised'], extra = direct_split(field, n, level, s, keep, rounds)
        line.update(extra)
    print(json.dumps(dict(line, rounds_timed=rounds, hbm_tbs=HBM_TBS, build=head)), flush=True)


def generator_cases(args, dev, head):
    import gen_videos_mi355x as gv
    n, level = args.voxel_res, args.level
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    ws = gv.orbit_latents(G, z, dev)
    with torch.no_grad():
        planes = G.backbone.synthesis(ws, noise_mode='const')
        planes = planes.view(len(planes), 3, 32, planes.shape[-2], planes.shape[-1])
    field, keep = gv._band_field(G, planes, n, True)
    crop = crop_of(gv.crop_ranges(n), n)

    for s in args.bricks:
        def parent():
            with torch.no_grad():
                mesh, _ = gv.mesh_of_density_grid(gv.extract_density_grid(G, ws, n, planes=planes, band=s, level=level), level)
            return mesh.verts, mesh.faces

        def direct():
            with torch.no_grad():
                return gv.extract_band_mesh(G, ws, n, level, s, planes=planes)

        def quiet_field(index, out):
            with torch.no_grad():
                field(index, out)

        report_case('generator', n, level, s, parent, direct, quiet_field, keep, crop, args.rounds, head, s == args.bricks[0])


def sphere_cases(args, dev, head):
    from bench_mesh import sphere
    n = args.voxel_res
    flat = sphere(n, dev).reshape(-1)

    def field(index, out):
        out[index.long()] = flat[index.long()]

    crop = crop_of(None, n)
    for s in args.bricks:
        report_case('sphere', n, 0.0, s, lambda: parent_route(field, n, 0.0, s, None, crop), lambda: S.band_mesh(field, n, 0.0, s, None, device=dev, **VIEW)[:2],
                    field, None, crop, args.rounds, head, s == args.bricks[0])


def large_case(args, dev, head):
    """n = 1024 on the sphere at the first brick edge: both whole calls, and what each allocates above the field."""
    from bench_mesh import sphere
    n, s = 1024, args.bricks[0]
    flat = sphere(n, dev).reshape(-1)

    def field(index, out):
        out[index.long()] = flat[index.long()]

    crop = crop_of(None, n)
    routes = {'parent': lambda: parent_route(field, n, 0.0, s, None, crop), 'direct': lambda: S.band_mesh(field, n, 0.0, s, None, device=dev, **VIEW)[:2]}
    line = {'case': f'sphere_{n}_s{s}', 'level': 0.0, 'volume_bytes': 4 * n ** 3, 'parent_passes_over_the_volume': PARENT_PASSES}
    meshes = {}
    for name, call in routes.items():
        meshes[name] = call()
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ms = timed_ms(call, args.rounds, warm=1)
        line[name + '_ms'] = ms
        line[name + '_peak_bytes_above_the_field'] = int(torch.cuda.max_memory_allocated() - held)
    assert same(meshes['parent'], meshes['direct']), 'n = 1024: the direct mesh is not the parent route\'s'
    line.update(mesh=[len(meshes['direct'][0]), len(meshes['direct'][1])], same_mesh=True,
                parent_over_direct=round(line['parent_ms']['median'] / line['direct_ms']['median'], 2))
    print(json.dumps(dict(line, rounds_timed=args.rounds, build=head)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--voxel-res', type=int, default=512)
    ap.add_argument('--bricks', type=int, nargs='*', default=[8, 4, 16], help='the first one also gets the splits and the n = 1024 pair')
    ap.add_argument('--level', type=float, default=0.0)
    ap.add_argument('--cases', nargs='*', default=['generator', 'sphere', 'large'], choices=['generator', 'sphere', 'large'])
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_band_mesh.py needs a GPU'
    dev = torch.device('cuda', 0)
    head_file = os.path.join(ROOT, 'g-nerf_amd', 'gnerf_hip', 'BUILD_HEAD')
    head = open(head_file).read().strip() if os.path.isfile(head_file) else 'unknown'
    if 'generator' in args.cases:
        generator_cases(args, dev, head)
    if 'sphere' in args.cases:
        sphere_cases(args, dev, head)
    if 'large' in args.cases:
        large_case(args, dev, head)


if __name__ == '__main__':
    main()
