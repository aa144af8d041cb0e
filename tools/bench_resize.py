#!/usr/bin/env python3
"""The antialiased resize kernel (csrc/resize.hip through torch_utils/ops/resize.py) against ATen's F.interpolate(antialias=True) on one
GPU, at the three hot tensors: [4,32,64,64] float16 channels_last and [4,3,64,64] float32 NCHW up x2 (the superresolution's pair; forward
alone and forward + backward), [4,3,512,512] float32 NCHW down x8 (the step's real images; forward alone).  The two forms alternate round
by round in one process, each round timed with HIP events around `--iters` calls (host-side enqueue included: these calls are at
launch-latency scale) and, to leave the host out, around replays of a HIP graph that holds 20 of them; min / median / max over the rounds.
One JSON line per case.

Traffic floor: every tensor the pass reads or writes moved once at 6.3 TB/s; printed for scale.

`--sr` adds the superresolution probe (tools/resize_sr_probe.py): the relative L2 distance of either fp16 route from the float32 form of the
module.  `--step` runs g-nerf_amd/train_step_mi355x.py --steps 10 with and without GNERF_RESIZE_AA=0 (child processes, alternating) and prints
their ms per step and the paired differences.

    python tools/bench_resize.py --sr --step | tee profiles/rNN_resize.jsonl"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'g-nerf_amd'), ROOT, os.path.join(ROOT, 'tools')]
import torch
import torch.nn.functional as F

from torch_utils.ops import resize as RZ

HBM = 6.3e12

CASES = [((4, 32, 64, 64), (128, 128), torch.float16, True, True), ((4, 3, 64, 64), (128, 128), torch.float32, False, True),
         ((4, 3, 512, 512), (64, 64), torch.float32, False, False)]


def torch_op(x, size):
    return F.interpolate(x, size=size, mode='bilinear', align_corners=False, antialias=True)


def kernel_op(x, size):
    return RZ.interpolate_aa(x, size=size, mode='bilinear')


def make_call(route, x, size, backward):
    if not backward:
        def call():
            with torch.no_grad():
                return route(x, size)
        return call
    xg = x.clone().requires_grad_(True)
    g = torch.rand_like(route(x, size))

    def call():
        xg.grad = None
        route(xg, size).backward(g)
        return xg.grad
    return call


def time_round(call, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters                          # us per call


def graph_of(call, iters):
    """`iters` calls captured in one HIP graph: a replay costs their GPU time, not the host's enqueueing."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            call()
    return graph


def bench_case(shape, size, dtype, channels_last, backward, rounds, iters, dev):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(0)).to(dev, dtype)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    forms = {'kernel': make_call(kernel_op, x, size, backward), 'torch': make_call(torch_op, x, size, backward)}
    for call in forms.values():
        for _ in range(10):
            call()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, call in forms.items():
            times[k].append(time_round(call, iters))
    graphs = {k: graph_of(call, 20) for k, call in forms.items()}
    gpu = {k: [] for k in forms}
    for _ in range(rounds):
        for k, graph in graphs.items():
            gpu[k].append(time_round(graph.replay, 5) / 20)
    in_bytes = x.numel() * x.element_size()
    out_bytes = in_bytes // (shape[2] * shape[3]) * size[0] * size[1]
    floor = (in_bytes + out_bytes) * (2 if backward else 1) / HBM * 1e6
    stats = lambda v: {'min': round(min(v), 2), 'median': round(statistics.median(v), 2), 'max': round(max(v), 2)}
    print(json.dumps({'case': 'resize_aa', 'shape': list(shape), 'size': list(size), 'dtype': str(dtype).replace('torch.', ''),
                      'layout': 'channels_last' if channels_last else 'nchw', 'pass': 'forward+backward' if backward else 'forward',
                      'kernel_us': stats(times['kernel']), 'torch_us': stats(times['torch']),
                      'torch_over_kernel': round(statistics.median(times['torch']) / statistics.median(times['kernel']), 2),
                      'graph_replay_kernel_us': stats(gpu['kernel']), 'graph_replay_torch_us': stats(gpu['torch']),
                      'graph_replay_torch_over_kernel': round(statistics.median(gpu['torch']) / statistics.median(gpu['kernel']), 2),
                      'traffic_floor_us': round(floor, 3), 'rounds': rounds, 'iters_per_round': iters,
                      'note': 'kernel_us / torch_us: eager calls, host-side enqueue included; graph_replay_*: 20 calls captured in one HIP graph, per call; the floor is for scale only'}), flush=True)


def sr_line(dev):
    import resize_sr_probe as P
    os.environ.pop('GNERF_RESIZE_AA', None)
    kernel = P.run(False, dev)
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, 'torch.pt'), os.path.join(tmp, 'fp32.pt')
        out = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'tools', 'resize_sr_probe.py'), '--out', a, '--fp32-out', b],
                             env=dict(os.environ, GNERF_RESIZE_AA='0'), capture_output=True, text=True)
        if out.returncode != 0:
            raise SystemExit(f'resize_sr_probe.py failed ({out.returncode}):\n{out.stdout[-1500:]}{out.stderr[-1500:]}')
        d = P.distances(kernel, torch.load(a), torch.load(b))
    print(json.dumps({'case': 'superresolution_fp16_vs_float32_form', 'measure': 'relative L2, one forward + backward of SuperRes8XDC at batch 1',
                      'distances': {k: {m: float(f'{v:.4e}') for m, v in d[k].items()} for k in d}}), flush=True)


def step_lines(pairs, steps):
    """The step with the kernel and with GNERF_RESIZE_AA=0, alternating, each in a child process; then one line with the medians and the
    spread of the paired differences: a step differs by several percent between two processes."""
    script = os.path.join(ROOT, 'g-nerf_amd', 'train_step_mi355x.py')
    ms = {'kernel': [], 'torch': []}
    for i in range(pairs):
        for route in ('torch', 'kernel'):
            env = dict(os.environ)
            env.pop('GNERF_RESIZE_AA', None)
            if route == 'torch':
                env['GNERF_RESIZE_AA'] = '0'
            out = subprocess.run(['timeout', '-k', '10', '600', sys.executable, script, '--steps', str(steps)], env=env, capture_output=True, text=True)
            if out.returncode != 0:
                raise SystemExit(f'train_step_mi355x.py ({route}) failed ({out.returncode}):\n{out.stdout[-1500:]}{out.stderr[-1500:]}')
            line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1])
            print(json.dumps({'case': 'train_step', 'resize': route, 'pair': i, 'steps': steps, 'ms_per_step': round(line['ms_per_step'], 3),
                              'phase_ms_rank0': line['phase_ms_rank0']}), flush=True)
            ms[route].append(line['ms_per_step'])
    delta = sorted(k - t for t, k in zip(ms['torch'], ms['kernel']))
    print(json.dumps({'case': 'train_step_summary', 'pairs': pairs, 'steps': steps,
                      'ms_per_step_median': {k: round(statistics.median(v), 3) for k, v in ms.items()},
                      'ms_per_step_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                      'paired_difference_ms_kernel_minus_torch': {'median': round(statistics.median(delta), 3), 'min': round(delta[0], 3), 'max': round(delta[-1], 3)}}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--sr', action='store_true', help='also measure the superresolution module on either route against its float32 form')
    ap.add_argument('--step', action='store_true', help='also time the training step with and without GNERF_RESIZE_AA=0')
    ap.add_argument('--step-pairs', type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_resize.py needs a GPU'
    assert RZ.kernel_enabled(), 'bench_resize.py alternates the two routes itself: unset GNERF_RESIZE_AA'
    dev = torch.device('cuda', 0)
    for shape, size, dtype, channels_last, with_backward in CASES:
        for backward in ((False, True) if with_backward else (False,)):
            bench_case(shape, size, dtype, channels_last, backward, args.rounds, args.iters, dev)
    if args.sr:
        sr_line(dev)
    if args.step:
        torch.cuda.empty_cache()
        step_lines(args.step_pairs, 10)


if __name__ == '__main__':
    main()
