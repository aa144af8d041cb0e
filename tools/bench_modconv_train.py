#!/usr/bin/env python3
"""Forward + backward of ONE generator layer under autograd on its two un-fused routes: `_train` (the elementwise passes around the convolution
on csrc/modconv.hip's kernels, forward and backward) against `_reference_unfused` (the PyTorch-op chain), at the two shapes that carry the
training step -- 512 -> 512 at 64^2 float32 (the backbone) and 128 -> 128 at 256^2 float16 channels_last (the superresolution) --, batch 4.

Per shape and route: milliseconds per forward + backward (median of --repeats timings of --iters iterations) and GPU kernel launches per
iteration (torch.profiler).  Per shape: the backward kernels alone, their time and their rate against the traffic floor -- the epilogue backward
reads dy, y and x and writes dx (four activation-sized tensors), the scale_channels backward reads dxs and x and writes dx (three).

One JSON object per line on stdout (and appended to --out).  Usage: python tools/bench_modconv_train.py [--out profiles/r10_modconv_train.jsonl]"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'g-nerf_amd'), ROOT]

import torch  # noqa: E402

SHAPES = [
    dict(name='512->512 @ 64^2 float32', c=512, res=64, dtype=torch.float32, memory_format=torch.contiguous_format, clamp=None),
    dict(name='128->128 @ 256^2 float16 channels_last', c=128, res=256, dtype=torch.float16, memory_format=torch.channels_last, clamp=256),
]


def timed(fn, iters, repeats):
    """Median / min / max milliseconds per call of fn over `repeats` timings of `iters` calls each."""
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA and 'Memcpy' not in e.key and 'Memset' not in e.key)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import gnerf_generator as G
    import gnerf_hip
    dev = torch.device('cuda', 0)
    lines = []
    for s in SHAPES:
        torch.manual_seed(0)
        layer = G.StyledConv(s['c'], s['c'], 512, s['res'], conv_clamp=s['clamp']).to(dev)
        with torch.no_grad():
            layer.noise_strength.fill_(0.1)
        x = torch.randn(args.batch, s['c'], s['res'], s['res'], device=dev).to(s['dtype']).contiguous(memory_format=s['memory_format']).requires_grad_(True)
        w = torch.randn(args.batch, 512, device=dev)
        up = torch.randn_like(x)

        def step():
            for p in layer.parameters():
                p.grad = None
            x.grad = None
            layer(x, w, 'const', fused=False).backward(up)

        row = dict(what='layer forward + backward', shape=s['name'], batch=args.batch)
        for route, on in (('_train', True), ('_reference_unfused', False)):
            G._MODCONV_TRAIN = on
            assert layer.route(x, w, 'const', fused=False) == route
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            med, lo, hi = timed(step, args.iters, args.repeats)
            row[route] = dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), launches=launches(step))
        G._MODCONV_TRAIN = True
        row['speedup'] = round(row['_reference_unfused']['ms'] / row['_train']['ms'], 3)
        lines.append(row)

        # the backward kernels alone
        xd = x.detach()
        scale = torch.rand(args.batch, s['c'], device=dev) + 0.5
        y = gnerf_hip.modconv_epilogue(xd, layer.bias.detach(), scale=scale, noise=layer.noise_const, round_noise=True, gain=1.414, clamp=s['clamp'])
        nbytes = xd.numel() * xd.element_size()
        kernels = {
            'modconv_epilogue_backward (dx, dscale, dbias, dnoise)': (4, lambda: gnerf_hip.modconv_epilogue_backward(
                up, y, xd, scale, gain=1.414, clamp=s['clamp'], need_dx=True, need_dscale=True, need_dbias=True, need_dnoise='plane')),
            'modconv_epilogue_backward (dx only)': (3, lambda: gnerf_hip.modconv_epilogue_backward(up, y, None, scale, gain=1.414, clamp=s['clamp'])),
            'scale_channels_backward (dx, dscale)': (3, lambda: gnerf_hip.scale_channels_backward(up, xd, scale)),
        }
        for name, (tensors, fn) in kernels.items():
            for _ in range(3):
                fn()
            med, lo, hi = timed(fn, args.iters, args.repeats)
            lines.append(dict(what=name, shape=s['name'], batch=args.batch, us=round(1e3 * med, 2), us_min=round(1e3 * lo, 2), us_max=round(1e3 * hi, 2),
                              traffic_floor_bytes=tensors * nbytes, TB_per_s=round(tensors * nbytes / (med * 1e-3) / 1e12, 3),
                              note='time of the wrapper call: the main pass plus its finishing launches and the workspace allocation'))
    for row in lines:
        print(json.dumps(row))
    if args.out:
        with open(args.out, 'a') as f:
            for row in lines:
                f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
