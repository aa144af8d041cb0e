#!/usr/bin/env python3
"""One forward + backward of the superresolution module (SuperRes8XDC, default sizes, batch 1, fixed seed) under torch.profiler: which resize
ran -- ATen's `_upsample_bilinear2d_aa` ops or gnerf_hip's kernel -- and what came out.  The route is the process' (GNERF_RESIZE_AA, read by
torch_utils/ops/resize.py); `--fp32` runs the float32 form of the same module, the yardstick both fp16 routes are measured against.

    python tools/resize_sr_probe.py --out /tmp/kernel.pt
    GNERF_RESIZE_AA=0 python tools/resize_sr_probe.py --out /tmp/torch.pt --fp32-out /tmp/fp32.pt

tests/test_resize_gpu.py and tools/bench_resize.py import run() and distances()."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.join(ROOT, 'g-nerf_amd'), ROOT) if p not in sys.path]
import torch


def run(fp32=False, device=None):
    """-> dict(out, grads [g_x, g_rgb] (float32, CPU), aa_ops, kernel_ops: the profiled op names of either resize)."""
    import gnerf_generator as GG
    dev = device if device is not None else torch.device('cuda', 0)
    torch.manual_seed(0)
    sr = GG.SuperRes8XDC(32, 512, use_fp16=not fp32, antialias=True).to(dev)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(1, 32, 64, 64, generator=gen).to(dev).requires_grad_(True)
    rgb = (torch.randn(1, 3, 64, 64, generator=gen) * 0.5).to(dev).requires_grad_(True)
    ws = torch.randn(1, 14, 512, generator=gen).to(dev)
    cot = torch.randn(1, 3, 512, 512, generator=gen).to(dev)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        out, _ = sr(rgb, x, ws)
        (out.float() * cot).sum().backward()
        torch.cuda.synchronize(dev)
    names = sorted({e.key for e in prof.key_averages()})
    return dict(out=out.detach().float().cpu(), grads=[x.grad.float().cpu(), rgb.grad.float().cpu()],
                aa_ops=[n for n in names if '_upsample_bilinear2d_aa' in n], kernel_ops=[n for n in names if 'gnerf_hip::resize_aa' in n])


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def distances(kernel, torch_route, fp32):
    """Relative L2 distances of the two fp16 routes from the float32 form and from each other: of the output image and of the input
    gradients (all of them as one vector, and each alone)."""
    cat = lambda r: torch.cat([g.flatten() for g in r['grads']])
    d = {}
    for name, r in (('kernel', kernel), ('torch', torch_route)):
        d[name] = dict(out=_rel(r['out'], fp32['out']), grads=_rel(cat(r), cat(fp32)), grad_x=_rel(r['grads'][0], fp32['grads'][0]),
                       grad_rgb=_rel(r['grads'][1], fp32['grads'][1]))
    d['kernel_vs_torch'] = dict(out=_rel(kernel['out'], torch_route['out']), grads=_rel(cat(kernel), cat(torch_route)))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='where the fp16 run is saved (torch.save)')
    ap.add_argument('--fp32-out', help='where the float32 form is saved')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'resize_sr_probe.py needs a GPU'
    if args.out:
        torch.save(run(False), args.out)
    if args.fp32_out:
        torch.save(run(True), args.fp32_out)


if __name__ == '__main__':
    main()
