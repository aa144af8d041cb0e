#!/usr/bin/env python3
"""The narrow-band density volume on the MI355X (csrc/query_lattice.inl, csrc/mesh_band.hip) against the dense one, in one
process: the 512^3 volume of a random-init generator at level 0 under extract_density_grid's crop, and the sphere of tools/bench_mesh.py.

  dense       extract_density_grid as it was: every lattice point through gnerf_query_points.
  band s      extract_density_grid(band=s) for s = 4, 8, 16: the whole call, then -- in a second, instrumented run that synchronises around
              every stage, so its parts do not add up to the whole call exactly -- the split into lattice queries, bookkeeping (seed, lists,
              growth) and fill; rounds, host reads, points evaluated; the band mesh against the dense mesh (counts, lost components, whether
              it is the dense mesh restricted to whole components, bit for bit).
  lattice     gnerf_query_lattice on the band's own lists (concatenated, as emitted) against gnerf_query_points on as many points -- the
              same points, handed over as positions --: nanoseconds per point and the ratio.
Every time is the median (and min) of --rounds warm calls, a host clock around work that ends in a device synchronise (the band reads counts
to the host every round, so it cannot be captured in a graph).  The sphere has no generator behind it: its field is a gather from the dense
volume, so its rounds, points, bookkeeping and fill are the band's and its "lattice" time is the gather's.

    python tools/bench_mesh_band.py | tee profiles/rNN_mesh_band.jsonl"""
import argparse
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


def timed_ms(call, rounds, warm=2):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {'median': round(statistics.median(ms), 3), 'min': round(min(ms), 3)}


class Split:
    """band_volume's stages with a synchronise and a host clock around each: where the time of a band call goes."""

    def __init__(self):
        self.ms = {'lattice': 0.0, 'bookkeeping': 0.0, 'fill': 0.0}
        self.lists = []

    def wrap(self, stage, call):
        def timed(*args):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = call(*args)
            torch.cuda.synchronize()
            self.ms[stage] += (time.perf_counter() - t0) * 1e3
            return out
        return timed


def band_split(field, n, level, s, keep, dev):
    """One instrumented band call -> (volume, report, Split)."""
    split = Split()
    vol = torch.empty(n ** 3, dtype=torch.float32, device=dev)
    band = gnerf_hip.BandVolume(vol, n, s, level, keep)

    def evaluate(index):
        if len(index):
            split.lists.append(index)
            field(index, vol)

    for stage in ('seed', 'points', 'grow'):
        setattr(band, stage, split.wrap('bookkeeping', getattr(band, stage)))
    band.fill = split.wrap('fill', band.fill)
    report = S._band_driver(n, s, split.wrap('lattice', evaluate), torch.from_numpy(S.band_coarse_index(n, s)).to(dev), band, None)
    return vol.reshape(n, n, n), report, split


def compare_meshes(band_mesh, dense_mesh):
    """Counts of both meshes, the components the band lost, and whether the band mesh is the dense mesh restricted to whole components."""
    (bv, bf), (dv, df) = band_mesh, dense_mesh
    line = {'band_mesh': [len(bv), len(bf)], 'dense_mesh': [len(dv), len(df)]}
    if len(dv) == 0:
        return dict(line, lost_components=0, partly_present=0, is_restricted_dense=len(bv) == 0)
    label, faces_of, counts = gnerf_hip.mesh_components(df, len(dv))
    rows, inverse = torch.unique(torch.cat([dv, bv]).view(torch.int32), dim=0, return_inverse=True)
    present = torch.isin(inverse[:len(dv)], inverse[len(dv):])
    # integer counts only: bincount with float64 weights adds by a compare-and-swap loop on this device, and on a one-component mesh (the
    # sphere) every vertex carries the same label -- 0.8 M threads retrying on one address do not finish in minutes
    size = torch.bincount(label.long(), minlength=len(dv))
    some = torch.bincount(label.long()[present], minlength=len(dv))
    roots = size > 0
    lost = roots & (some == 0)
    keep = (some > 0).to(torch.uint8)
    rv, rf, _ = gnerf_hip.mesh_compact(dv, df, label, faces_of, keep)
    return dict(line, dense_components=int(counts[0]), lost_components=int(lost.sum()), lost_vertices=int(size[lost].sum()), lost_faces=int(faces_of[lost].sum()),
                largest_lost_faces=int(faces_of[lost].max()) if bool(lost.any()) else 0, partly_present=int((roots & (some > 0) & (some < size)).sum()),
                is_restricted_dense=bool(rv.shape == bv.shape and rf.shape == bf.shape and torch.equal(rv, bv) and torch.equal(rf, bf)))


def lattice_yardstick(G, planes, lists, n, rounds):
    """gnerf_query_lattice on the band's lists against gnerf_query_points on the same points given as positions."""
    import gen_videos_mi355x as gv
    from training.volumetric_rendering.renderer import _osg_decoder_weights
    kw = G.rendering_kwargs
    nhwc, dec = G.renderer._planes_nhwc(planes[:1])[0], G.renderer._decoder_cache(_osg_decoder_weights(G.decoder))
    index = torch.cat(lists)
    out = torch.empty(n ** 3, dtype=torch.float32, device=index.device)
    pts = gv.voxel_samples(index, None, n, kw['box_warp'], index.device)
    a = timed_ms(lambda: gnerf_hip.query_lattice(nhwc, dec, index, n, kw['box_warp'], kw['box_warp'], out), rounds)
    b = timed_ms(lambda: gnerf_hip.query_points(nhwc, 1, dec, pts, kw['box_warp'], want_rgb=False), rounds)
    sigma = gnerf_hip.query_points(nhwc, 1, dec, pts, kw['box_warp'], want_rgb=False)[0].reshape(-1)
    return {'points': len(index), 'query_lattice_ms': a, 'query_points_ms': b, 'query_lattice_ns_per_point': round(a['median'] * 1e6 / len(index), 4),
            'query_points_ns_per_point': round(b['median'] * 1e6 / len(index), 4), 'lattice_over_points': round(a['median'] / b['median'], 3),
            'same_bits': bool(torch.equal(out[index.long()], sigma))}


def generator_cases(args, dev, head):
    import gen_videos_mi355x as gv
    n, level = args.voxel_res, args.level
    G = gv.build_random_generator(0, dev)
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(dev)
    ws = gv.orbit_latents(G, z, dev)
    kw = G.rendering_kwargs
    with torch.no_grad():
        dense, planes = gv.extract_density_grid(G, ws, n, return_planes=True)
        dense_ms = timed_ms(lambda: gv.extract_density_grid(G, ws, n, planes=planes), args.rounds)
    dense_mesh = S.marching_cubes(dense.permute(2, 1, 0).contiguous(), level)
    print(json.dumps({'case': f'generator_{n}_dense', 'level': level, 'ms': dense_ms, 'points': n ** 3, 'mesh': [len(dense_mesh[0]), len(dense_mesh[1])],
                      'rounds_timed': args.rounds, 'build': head}), flush=True)
    (a0, b0), r1, r2 = gv.crop_ranges(n)
    keep = S.band_keep_of_crop(n, [(b0, a0), r1, r2])

    def generator_field(index, out):
        G.renderer.query_sigma_lattice(planes, G.decoder, index, n, kw, out)

    for s in args.bricks:
        with torch.no_grad():
            whole = timed_ms(lambda: gv.extract_density_grid(G, ws, n, planes=planes, band=s, level=level), args.rounds)
            band = gv.extract_density_grid(G, ws, n, planes=planes, band=s, level=level)
            splits = [band_split(generator_field, n, level, s, keep, dev) for _ in range(3)]
        _, report, split = splits[-1]
        parts = {k: round(statistics.median(sp.ms[k] for _, _, sp in splits), 3) for k in split.ms}
        mesh = S.marching_cubes(band.permute(2, 1, 0).contiguous(), level)
        with torch.no_grad():
            yard = lattice_yardstick(G, planes, split.lists, n, args.rounds)
        print(json.dumps({'case': f'generator_{n}_band_{s}', 'level': level, 'ms': whole, 'dense_over_band': round(dense_ms['median'] / whole['median'], 2),
                          'split_ms_synchronised': parts, **{k: report[k] for k in ('bricks', 'seeds', 'new_bricks', 'rounds', 'host_reads', 'points')},
                          'share': round(report['share'], 5), **compare_meshes(mesh, dense_mesh), 'lattice_kernel': yard, 'rounds_timed': args.rounds, 'build': head}),
              flush=True)
        del band, splits, mesh



def sphere_cases(args, dev, head):
    from bench_mesh import sphere
    n = args.voxel_res
    ball = sphere(n, dev)
    flat = ball.reshape(-1)
    ball_mesh = S.marching_cubes(ball, 0.0)
    print(json.dumps({'case': f'sphere_{n}_dense', 'level': 0.0, 'points': n ** 3, 'mesh': [len(ball_mesh[0]), len(ball_mesh[1])], 'build': head}), flush=True)

    def sphere_field(index, out):
        out[index.long()] = flat[index.long()]

    for s in args.bricks:
        whole = timed_ms(lambda: S.band_volume(sphere_field, n, 0.0, s, None, device=dev), args.rounds)
        vol, report, split = band_split(sphere_field, n, 0.0, s, None, dev)
        mesh = S.marching_cubes(vol, 0.0)
        print(json.dumps({'case': f'sphere_{n}_band_{s}', 'level': 0.0, 'ms_with_a_gather_as_the_field': whole,
                          'split_ms_synchronised': {k: round(v, 3) for k, v in split.ms.items()},
                          **{k: report[k] for k in ('bricks', 'seeds', 'new_bricks', 'rounds', 'host_reads', 'points')}, 'share': round(report['share'], 5),
                          **compare_meshes(mesh, ball_mesh), 'rounds_timed': args.rounds, 'build': head}), flush=True)
        del vol, mesh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--voxel-res', type=int, default=512)
    ap.add_argument('--bricks', type=int, nargs='*', default=[4, 8, 16])
    ap.add_argument('--level', type=float, default=0.0)
    ap.add_argument('--cases', nargs='*', default=['generator', 'sphere'], choices=['generator', 'sphere'])
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mesh_band.py needs a GPU'
    dev = torch.device('cuda', 0)
    head_file = os.path.join(ROOT, 'g-nerf_amd', 'gnerf_hip', 'BUILD_HEAD')
    head = open(head_file).read().strip() if os.path.isfile(head_file) else 'unknown'
    if 'generator' in args.cases:
        generator_cases(args, dev, head)
    if 'sphere' in args.cases:
        sphere_cases(args, dev, head)


if __name__ == '__main__':
    main()
