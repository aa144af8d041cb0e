#!/usr/bin/env python3
"""When do the workgroups of the pipelined render kernel start and end?  Runs the headline step of bench.py (repack, rays + draws,
render call: config 2, FULL instantiation, decoder chosen on the device) on the -DGNERF_WG_STAMPS build, whose workgroups write
three 100 MHz stamps each (start, first shader tile, end: nothing inside the loops, so the run time stays that of the shipped kernel --
check with --plain under rocprofv3 --kernel-trace --stats on both libraries) plus where they ran, and reports the spread of their
lifetimes -- what share of the launch's workgroup slots sits idle behind the last workgroup, i.e. what any other dealing of rays could
return -- and the workgroups' PROLOGUE: the time from a workgroup's start to its first shader tile (the choice of decoder arithmetic, the
decoder's way into LDS, the first ray's proposals).  The call hands the kernels a decoder pack as gnerf_hip.render_forward does;
--no-pack makes the plain call.  --res / --items pick another launch (--res 64 --items 1 --samples 96: one orbit frame).

    tools/build_variants.sh D:GNERF_WG_STAMPS
    GNERF_HIP_LIB=g-nerf_amd/gnerf_hip/variants/libgnerf_D:GNERF_WG_STAMPS.so python tools/wg_lifetimes.py [--calls 7] [--samples 96] [--json OUT]
    python tools/wg_lifetimes.py --plain          (same calls, no stamps read: for timing the kernel of any library)"""
import argparse, ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'g-nerf_amd'), ROOT]
import numpy as np


def summarize(xcd, cu, start, end, first_tile=None):
    """Per-launch figures from per-workgroup arrays (ticks of 10 ns; first_tile: ticks from a workgroup's start to its first shader tile).  Pure numpy."""
    start, end = np.asarray(start, np.float64), np.asarray(end, np.float64)
    t0, t1 = start.min(), end.max()
    span = t1 - t0
    life = end - start

    def dist(v):
        return {'mean': float(v.mean()) / 100, 'median': float(np.median(v)) / 100, 'p95': float(np.percentile(v, 95)) / 100, 'max': float(v.max()) / 100,
                'max_over_mean': float(v.max() / v.mean())}
    out = {'workgroups': int(life.size), 'span_us': span / 100, 'start_spread_us': float(start.max() - t0) / 100, 'lifetime_us': dist(life),
           # slot-time left idle behind the last workgroup: sum over workgroups of (last end - own end) over (workgroups x span)
           'idle_slot_time': float((t1 - end).sum() / (life.size * span)),
           'per_xcd': {}}
    if first_tile is not None:
        out['prologue_us'] = dist(np.asarray(first_tile, np.float64))
    for x in sorted(set(int(v) for v in xcd)):
        m = np.asarray(xcd) == x
        d = dist(life[m])
        d.update(workgroups=int(m.sum()), cus=int(len(set(np.asarray(cu)[m].tolist()))), last_end_us=float(end[m].max() - t0) / 100,
                 idle_slot_time_in_xcd=float((end[m].max() - end[m]).sum() / (m.sum() * span)))
        out['per_xcd'][str(x)] = d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=7)
    ap.add_argument('--samples', type=int, default=0, help='coarse = fine sample count (default: config 2\'s 48; 96 runs pipe<2>, 144 pipe<3>)')
    ap.add_argument('--plain', action='store_true', help='run the calls only (any library)')
    ap.add_argument('--no-pack', action='store_true', help='the plain call: every workgroup prepares the decoder itself')
    ap.add_argument('--res', type=int, default=0, help='image side (default: config 2\'s)')
    ap.add_argument('--items', type=int, default=0, help='items (default: config 2\'s)')
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    import torch
    import bench, gnerf_hip
    dev = torch.device('cuda', 0)
    planes, dec, c2w, intr = bench._scene(dev, 1000)
    N, RES = args.items or bench.N_ITEMS, args.res or bench.RES
    planes, c2w, intr = planes[:N], c2w[:N], intr[:N]
    lib = gnerf_hip.load()
    pack = None if args.no_pack or not hasattr(lib, 'gnerf_render_forward_packed') else gnerf_hip.pack_decoder(dec)
    S = F = args.samples or bench.S_COARSE
    kw = dict(depth_resolution=S, depth_resolution_importance=F, ray_start=bench.RAY_START, ray_end=bench.RAY_END, box_warp=bench.BOX_WARP, image_width=RES)
    stamps = torch.zeros(4096 * 4, dtype=torch.int64, device=dev)
    per_call = []
    for call in range(3 + args.calls):
        nhwc, amax = gnerf_hip.planes_to_nhwc(planes, with_absmax=True)
        o, d, nc, nf = gnerf_hip.make_rays_and_draws(c2w, intr, RES, S, F)
        if args.plain:
            gnerf_hip.render_forward(nhwc, N, dec, o, d, nc, nf, planes_absmax=amax, decoder_pack=pack is not None, **kw)
            continue
        # render_forward(debug=True) with a stamp buffer of our own in place of its [rays, 8, S+F] stage dump (200 MB zeroed per call)
        p, keep, m = gnerf_hip._render_params(nhwc, N, dec, o, d, nc, nf, S, F, kw['ray_start'], kw['ray_end'], kw['box_warp'], False, False, RES,
                                              'render_forward', amax, 'auto', False, False, None, None)
        rgb, depth, wsum = (torch.empty([N, m, c], device=dev) for c in (32, 1, 1))
        p.out_rgb, p.out_depth, p.out_wsum = rgb.data_ptr(), depth.data_ptr(), wsum.data_ptr()
        p.workspace, p.debug = gnerf_hip._workspace(dev).data_ptr(), stamps.data_ptr()
        stamps.zero_()
        if pack is not None:
            gnerf_hip._check(lib.gnerf_render_forward_packed(ctypes.byref(p), pack.data_ptr(), gnerf_hip._stream(nhwc)), 'gnerf_render_forward_packed')
        else:
            gnerf_hip._check(lib.gnerf_render_forward(ctypes.byref(p), gnerf_hip._stream(nhwc)), 'gnerf_render_forward')
        torch.cuda.synchronize()
        if call < 3:
            continue
        st = stamps.cpu().numpy().view(np.uint64).reshape(-1, 4)
        st = st[st[:, 1] > 0]
        if not len(st):
            sys.exit('no stamps: is GNERF_HIP_LIB the -DGNERF_WG_STAMPS build?')
        hw = st[:, 0].astype(np.int64)
        xcd = (hw >> 32) & 15
        cu = ((hw >> 8) & 15) | (((hw >> 12) & 1) << 4) | (((hw >> 13) & 7) << 5) | (xcd << 8)         # (HW_ID: cu, sh, se; unique with the XCD)
        rays, first = st[:, 3] & np.uint64(0xffffffff), st[:, 3] >> np.uint64(32)      # (a build from before the third stamp leaves the high half zero)
        r = summarize(xcd, cu, st[:, 1], st[:, 2], first if first.any() else None)
        r['rays_per_workgroup'] = {'min': int(rays.min()), 'max': int(rays.max())}
        per_call.append(r)
    torch.cuda.synchronize()
    if args.plain:
        return
    key = lambda r: r['span_us']
    mid = sorted(per_call, key=key)[len(per_call) // 2]
    out = {'tool': 'tools/wg_lifetimes.py', 'library': os.path.basename(os.environ.get('GNERF_HIP_LIB', 'libgnerf_hip.so')), 'device': torch.cuda.get_device_name(0),
           'shape': f'{N}x{RES}x{RES} rays, {S}+{F} samples', 'calls': len(per_call), 'decoder_pack': pack is not None,
           'prologue_median_us_per_call': [round(r['prologue_us']['median'], 2) for r in per_call if 'prologue_us' in r],
           'span_us_per_call': [round(r['span_us'], 1) for r in per_call], 'idle_slot_time_per_call': [round(r['idle_slot_time'], 4) for r in per_call],
           'max_over_mean_per_call': [round(r['lifetime_us']['max_over_mean'], 4) for r in per_call], 'median_call': mid}
    if args.json:
        json.dump(out, open(args.json, 'w'), indent=1)
    L = mid['lifetime_us']
    print(f"{out['shape']} on {out['library']}: {mid['workgroups']} workgroups, call with the median span of {len(per_call)}")
    print(f"  span {mid['span_us']:.1f} us (start spread {mid['start_spread_us']:.1f}); lifetime mean {L['mean']:.1f} median {L['median']:.1f} p95 {L['p95']:.1f} max {L['max']:.1f} us; "
          f"max / mean {L['max_over_mean']:.4f}; idle slot-time {100 * mid['idle_slot_time']:.2f} % of the launch")
    print(f"  over the calls: span {min(out['span_us_per_call'])}-{max(out['span_us_per_call'])} us, idle slot-time "
          f"{100 * min(out['idle_slot_time_per_call']):.2f}-{100 * max(out['idle_slot_time_per_call']):.2f} %")
    if 'prologue_us' in mid:
        Pq = mid['prologue_us']
        print(f"  prologue (workgroup start -> first shader tile, decoder pack: {out['decoder_pack']}): median {Pq['median']:.2f} mean {Pq['mean']:.2f} p95 {Pq['p95']:.2f} max {Pq['max']:.2f} us; "
              f"median over the calls {min(out['prologue_median_us_per_call'])}-{max(out['prologue_median_us_per_call'])} us")
    for x, d in mid['per_xcd'].items():
        print(f"  XCD {x}: {d['workgroups']:4d} workgroups on {d['cus']:3d} CUs, lifetime mean {d['mean']:.1f} p95 {d['p95']:.1f} max {d['max']:.1f} us, last end {d['last_end_us']:.1f} us, "
              f"idle inside the XCD {100 * d['idle_slot_time_in_xcd']:.2f} %")


if __name__ == '__main__':
    main()
