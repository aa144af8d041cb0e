#!/usr/bin/env python3
"""The fused SSIM kernel (csrc/ssim.hip) against the composed PyTorch-op form of the same function (torch_utils/ops/ssim.py:
ssim_pair_torch -- ten grouped convolutions and a dozen elementwise launches forward, autograd's mirror of them backward) on one GPU:
the loss term of the training step, 1 - ssim(real, generated, data_range=1, size_average=False), at [4,3,512,512] and [4,3,64,64], float32
and float16, forward alone and forward + backward (gradient for the generated image).  The two forms alternate round by round in one
process, each round timed with HIP events around `--iters` calls; the median round is reported.  One JSON line per case.

Traffic floor: the forward reads X and Y once, the backward reads them again and writes one gradient, priced at 6.3 TB/s -- about 2 us per
pass at 512^2.  That is below the cost of a launch, so these calls are at launch-latency scale and the floor is printed for scale only: the
lines carry times and the ratio of the two forms, no bandwidth fraction.

`--step` also runs g-nerf_amd/train_step_mi355x.py --steps 10 with and without --ssim (child processes, alternating) and prints their
ms per step."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'g-nerf_amd'), ROOT]
import torch

from torch_utils.ops import ssim as S

HBM = 6.3e12


def loss_of(route, X, Y):
    per_channel, _ = route(X, Y, S.gaussian_window(), 1e-4, 9e-4)
    return 1 - per_channel.mean(1)


def make_call(route, X, Y, backward):
    if not backward:
        def call():
            with torch.no_grad():
                return loss_of(route, X, Y)
        return call
    Yg = Y.clone().requires_grad_(True)

    def call():
        Yg.grad = None
        loss_of(route, X, Yg).float().sum().backward()
        return Yg.grad
    return call


def time_round(call, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters                          # us per call


def bench_case(shape, dtype, backward, rounds, iters, dev):
    gen = torch.Generator().manual_seed(0)
    X, Y = torch.rand(shape, generator=gen).to(dev, dtype), torch.rand(shape, generator=gen).to(dev, dtype)
    forms = {'kernel': make_call(S.ssim_pair, X, Y, backward), 'composed': make_call(S.ssim_pair_torch, X, Y, backward)}
    for call in forms.values():
        for _ in range(10):
            call()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, call in forms.items():
            times[k].append(time_round(call, iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    nbytes = X.numel() * X.element_size()
    floor = (2 * nbytes + (3 * nbytes if backward else 0)) / HBM * 1e6
    print(json.dumps({'case': 'ssim_loss', 'shape': list(shape), 'dtype': str(dtype).replace('torch.', ''), 'pass': 'forward+backward' if backward else 'forward',
                      'kernel_us': round(med['kernel'], 2), 'composed_us': round(med['composed'], 2), 'composed_over_kernel': round(med['composed'] / med['kernel'], 2),
                      'kernel_us_min_max': [round(min(times['kernel']), 2), round(max(times['kernel']), 2)],
                      'composed_us_min_max': [round(min(times['composed']), 2), round(max(times['composed']), 2)],
                      'traffic_floor_us': round(floor, 2), 'rounds': rounds, 'iters_per_round': iters,
                      'note': 'launch-latency scale: host-side enqueue included, the floor is for scale only'}), flush=True)


def step_lines(pairs, steps):
    """The step off and on, alternating, each in a child process; then one line with the medians and the spread of the paired
    differences: a step differs by several percent between two processes, so a single pair says nothing about a sub-millisecond term."""
    script = os.path.join(ROOT, 'g-nerf_amd', 'train_step_mi355x.py')
    ms = {False: [], True: []}
    for i in range(pairs):
        for flag in ([], ['--ssim']):
            out = subprocess.run(['timeout', '-k', '10', '900', sys.executable, script, '--steps', str(steps)] + flag, capture_output=True, text=True)
            if out.returncode != 0:
                raise SystemExit(f'train_step_mi355x.py {flag} failed ({out.returncode}):\n{out.stdout[-1500:]}{out.stderr[-1500:]}')
            line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1])
            print(json.dumps({'case': 'train_step', 'ssim_terms': line['ssim_terms'], 'pair': i, 'steps': steps, 'ms_per_step': round(line['ms_per_step'], 3),
                              'phase_ms_rank0': line['phase_ms_rank0'], 'losses': line['losses']}), flush=True)
            ms[bool(line['ssim_terms'])].append(line['ms_per_step'])
    delta = sorted(on - off for off, on in zip(ms[False], ms[True]))
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else sum(sorted(v)[len(v) // 2 - 1:len(v) // 2 + 1]) / 2
    print(json.dumps({'case': 'train_step_summary', 'pairs': pairs, 'steps': steps, 'ms_per_step_median': {'off': round(med(ms[False]), 3), 'on': round(med(ms[True]), 3)},
                      'ms_per_step_min_max': {'off': [round(min(ms[False]), 3), round(max(ms[False]), 3)], 'on': [round(min(ms[True]), 3), round(max(ms[True]), 3)]},
                      'paired_difference_ms': {'median': round(med(delta), 3), 'min': round(delta[0], 3), 'max': round(delta[-1], 3)}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--step', action='store_true', help='also time the training step with and without --ssim')
    ap.add_argument('--step-pairs', type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ssim.py needs a GPU'
    dev = torch.device('cuda', 0)
    for shape in ((4, 3, 512, 512), (4, 3, 64, 64)):
        for dtype in (torch.float32, torch.float16):
            for backward in (False, True):
                bench_case(shape, dtype, backward, args.rounds, args.iters, dev)
    if args.step:
        torch.cuda.empty_cache()
        step_lines(args.step_pairs, 10)


if __name__ == '__main__':
    main()
