#!/usr/bin/env python3
"""Time the fused renderer's ray gradient (gnerf_render_backward_rays, csrc/render_ray_grad.inl).  HIP events, one process, the variants
of one shape alternating round by round:
  bwd            render_backward as it is (planes + decoder)
  bwd_rays       ... with need_rays=True (the same launches plus render_ray_grad_kernel)
  rays_only      need_rays=True, no plane and no decoder gradient (frozen generator: first pass, ray kernel, no scatter)
at BASELINE config 2 (4 x 128^2 rays, 48+48 samples) and at the training shape (4 x 64^2); at the training shape also forward + backward
of the PyTorch-op form for the same ray gradients, with its peak memory.  The ray kernel's own time is the difference bwd_rays - bwd
(no kernel trace here); its gather floor is rays (S+F) 12 taps 128 B at 64 B/cycle/CU.
usage: python tools/bench_ray_grad.py [--rounds 7] [--calls 20] [--out profiles/rNN_ray_grad.jsonl] [--no-torch]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'g-nerf_amd'))
import torch

import gnerf_harness as H
import gnerf_hip

NUM_CU, BYTES_PER_CYCLE_CU = 256, 64


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ray_grad.py measures on the GPU; there is no CPU form of it'
    dev = torch.device('cuda', 0)
    lines = []
    for label, N, res in (('config2', 4, 128), ('training', 4, 64)):
        S = F = 48
        torch.manual_seed(0)
        planes = torch.randn(N, 3, 32, 256, 256, device=dev)
        dec = [torch.randn(64, 32, device=dev) * 0.18, torch.randn(64, device=dev) * 0.1, torch.randn(33, 64, device=dev) * 0.12, torch.randn(33, device=dev) * 0.1]
        c2w = torch.cat([H.lookat_pose(3.14 / 2 + 0.3 * i, 3.14 / 2 - 0.05, 2.7) for i in range(N)])
        intr = torch.tensor(H.FFHQ_INTRINSICS).reshape(1, 3, 3).repeat(N, 1, 1)
        o, d = gnerf_hip.make_rays(c2w.to(dev), intr.to(dev), res)
        M = res * res
        nc, nf = torch.rand(N * M, S, device=dev), torch.rand(N * M, F, device=dev)
        g = [torch.randn(N, M, k, device=dev) for k in (32, 1, 1)]
        nhwc, amax = gnerf_hip.planes_to_nhwc(planes, with_absmax=True)
        kw = dict(depth_resolution=S, depth_resolution_importance=F, ray_start=2.25, ray_end=3.3, box_warp=1.0, image_width=res, planes_absmax=amax)
        variants = {
            'bwd': lambda: gnerf_hip.render_backward(nhwc, N, dec, o, d, nc, nf, *g, **kw),
            'bwd_rays': lambda: gnerf_hip.render_backward(nhwc, N, dec, o, d, nc, nf, *g, need_rays=True, **kw),
            'rays_only': lambda: gnerf_hip.render_backward(nhwc, N, dec, o, d, nc, nf, *g, need_rays=True, need_planes=False, need_decoder=False, **kw),
        }
        for fn in variants.values():                         # warm-up: code objects, the allocator's blocks
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        series = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                series[k].append(timed(fn, args.calls))
        floor_ms = N * M * (S + F) * 12 * 128 / (BYTES_PER_CYCLE_CU * NUM_CU) / 2.0e9 * 1e3
        line = dict(shape=label, n_items=N, res=res, S=S, F=F, rounds=args.rounds, calls_per_round=args.calls, unit='ms per call (HIP events)',
                    gather_floor_ms_at_2GHz=floor_ms, build=gnerf_hip.load().gnerf_build_info().decode())
        for k, v in series.items():
            line[k] = dict(min=min(v), median=statistics.median(v), max=max(v))
        diffs = [a - b for a, b in zip(series['bwd_rays'], series['bwd'])]
        line['ray_kernel_ms_by_difference'] = dict(min=min(diffs), median=statistics.median(diffs), max=max(diffs))
        line['gather_floor_over_ray_kernel'] = floor_ms / statistics.median(diffs) if statistics.median(diffs) > 0 else None
        if label == 'training' and not args.no_torch:
            from training.volumetric_rendering.renderer import ImportanceRenderer
            ren = ImportanceRenderer().to(dev)
            dmod = H.TriPlaneDecoder().to(dev).requires_grad_(False)
            opts = dict(depth_resolution=S, depth_resolution_importance=F, ray_start=2.25, ray_end=3.3, box_warp=1.0, clamp_mode='softplus',
                        disparity_space_sampling=False, white_back=False)
            og, dg = o.clone().requires_grad_(True), d.clone().requires_grad_(True)

            def torch_step():
                og.grad = dg.grad = None
                rgb, depth, w = ren._forward_torch(planes, dmod, og, dg, opts)
                ((rgb * g[0]).sum() + (depth * g[1]).sum() + (w * g[2]).sum()).backward()
            torch_step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t = [timed(torch_step, 3) for _ in range(3)]
            line['torch_ops_fwd_bwd_ms'] = dict(min=min(t), median=statistics.median(t), max=max(t))
            line['torch_ops_peak_GB_above_inputs'] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
            fused_fwd = [timed(lambda: gnerf_hip.render_forward(nhwc, N, dec, o, d, nc, nf, **kw), args.calls) for _ in range(3)]
            line['fused_forward_ms'] = dict(min=min(fused_fwd), median=statistics.median(fused_fwd), max=max(fused_fwd))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
