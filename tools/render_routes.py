#!/usr/bin/env python3
"""Every route of the render launchers (csrc/render.hip and csrc/render_backward.hip, host halves) on the smallest call that reaches it: one process walks the table
below and prints one JSON line per case -- name, return code (and the library's error text when the call is refused), a hash of every
output tensor.  Run it under `rocprofv3 --kernel-trace -f csv -d DIR -- python3 tools/render_routes.py` and reduce the trace with
`tools/render_routes.py --reduce DIR`: the dispatch-ordered list of (kernel, grid, workgroup, LDS bytes) of the library's kernels.
Two builds launch the same work when both listings and every code and text agree (GNERF_HIP_LIB selects the library);
profiles/render_routes_*.txt keeps the pair taken around a host-side change.  Hashes are comparable where no float atomic is behind the
tensor: not the decoder gradients of any backward route or of query_points_backward, nor the plane gradients of the single-pass and sorted
scatters -- two runs of ONE build say which (everything the forward and the binned scatter write is bit-stable).
`--host-cost` times 1000 back-to-back calls of the 64x64 forward and the 8x8 backward, five repeats each: the launchers' host time."""
import contextlib, csv, ctypes, glob, hashlib, json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'g-nerf_amd'), ROOT]


def reduce_trace(directory):
    """(kernel, grid, workgroup, LDS bytes) per dispatch of the library's kernels, in dispatch order.  LDS is the dispatch's whole group
    segment: the kernel's static part, the same in any two builds of the same device code, plus the launch's dynamic bytes."""
    rows = []
    for path in glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True):
        with open(path, newline='') as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r['Dispatch_Id']))
    for r in rows:
        name = r['Kernel_Name']
        if 'at::' in name or name.startswith('__amd_rocclr'):      # torch's own fills and copies, the runtime's memsets
            continue
        name = name.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
        lds = r.get('LDS_Block_Size', r.get('Group_Segment_Size', '?'))
        print(f"{name} grid={r['Grid_Size_X']}x{r['Grid_Size_Y']}x{r['Grid_Size_Z']} wg={r['Workgroup_Size_X']}x{r['Workgroup_Size_Y']}x{r['Workgroup_Size_Z']} lds={lds}")


if len(sys.argv) > 2 and sys.argv[1] == '--reduce':
    reduce_trace(sys.argv[2])
    sys.exit(0)

import torch
import gnerf_hip
from oracle import render_ref as R

dev = torch.device('cuda', 0)
PLANE = 32


def scene(n_items, rays_per_item, res, S, F, seed=3):
    """32x32 planes, decoder, camera rays (res > 0) or rays of random pixels of such cameras, the two draws, output gradients."""
    g = torch.Generator().manual_seed(seed)
    planes = torch.randn(n_items, 3, 32, PLANE, PLANE, generator=g)
    dec = (torch.randn(64, 32, generator=g) / math.sqrt(32), torch.randn(64, generator=g) * 0.1, torch.randn(33, 64, generator=g) / math.sqrt(64), torch.randn(33, generator=g) * 0.1)
    c2w = torch.cat([R.lookat_pose(3.14 / 2 + 0.2 * i, 3.14 / 2 - 0.1 * i, 2.7) for i in range(n_items)])
    intr = torch.tensor([[4.2647, 0, 0.5], [0, 4.2647, 0.5], [0, 0, 1]]).repeat(n_items, 1, 1)
    if res > 0:
        o, d = R.make_rays(c2w, intr, res)
    else:
        o, d = R.make_rays(c2w, intr, 64)
        pick = torch.stack([torch.randperm(64 * 64, generator=g)[:rays_per_item] for _ in range(n_items)])
        o, d = torch.gather(o, 1, pick[..., None].expand(-1, -1, 3)), torch.gather(d, 1, pick[..., None].expand(-1, -1, 3))
    total = n_items * rays_per_item
    sc = dict(n=n_items, m=rays_per_item, res=res, S=S, F=F, c2w=c2w.to(dev), intr=intr.to(dev), dec=tuple(t.to(dev) for t in dec),
              o=o.to(dev).contiguous(), d=d.to(dev).contiguous(), nc=torch.rand(total, S, generator=g).to(dev),
              nf=torch.rand(total, F, generator=g).to(dev) if F else None,
              grads=tuple(torch.randn(n_items, rays_per_item, c, generator=g).to(dev) for c in (32, 1, 1)),
              sigma_noise=(torch.randn(total, S, generator=g).to(dev) * 0.1, torch.randn(total, F, generator=g).to(dev) * 0.1 if F else None))
    sc['nhwc'], sc['amax'] = gnerf_hip.planes_to_nhwc(planes.to(dev), with_absmax=True)
    sc['nhwc_one'] = gnerf_hip.planes_to_nhwc(planes[:1].to(dev))
    return sc


def options(sc, **kw):
    return dict(dict(depth_resolution=sc['S'], depth_resolution_importance=sc['F'], ray_start=2.25, ray_end=3.3, box_warp=1.0, image_width=sc['res']), **kw)


def forward(sc, **kw):
    return gnerf_hip.render_forward(sc['nhwc'], sc['n'], sc['dec'], sc['o'], sc['d'], sc['nc'], sc['nf'], **options(sc, **kw))


def backward(sc, **kw):
    return gnerf_hip.render_backward(sc['nhwc'], sc['n'], sc['dec'], sc['o'], sc['d'], sc['nc'], sc['nf'], *sc['grads'], **options(sc, **kw))


def forward_generated(sc):
    torch.manual_seed(1234)                 # the in-kernel draws follow the device generator
    plan = gnerf_hip.torch_philox_plan(dev, sc['n'], sc['m'], sc['S'], sc['F'])
    return gnerf_hip.render_forward(sc['nhwc'], sc['n'], sc['dec'], None, None, None, None, cameras=(sc['c2w'], sc['intr'], sc['res']), rng=plan, **options(sc))


def forward_views(sc):
    return gnerf_hip.render_forward(sc['nhwc_one'], sc['n'], sc['dec'], sc['o'], sc['d'], sc['nc'], sc['nf'], planes_shared=True, depth_clamp_per_item=True, **options(sc))


@contextlib.contextmanager
def environment(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def tensors(out):
    if isinstance(out, torch.Tensor):
        yield out
    elif isinstance(out, (tuple, list)):
        for t in out:
            yield from tensors(t)


def run(name, fn, env=None):
    line = {'case': name, 'code': 0}
    try:
        with environment(env or {}):
            out = fn()
        torch.cuda.synchronize()
        line['hashes'] = [hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16] for t in tensors(out)]
    except gnerf_hip.NativeError as e:
        line['code'], line['error'] = e.code, str(e)
    print(json.dumps(line), flush=True)


def host_cost():
    """Wall time per call over 1000 back-to-back calls (ending in a device synchronise), five repeats: on calls this small the GPU keeps
    up with the host, so the figure is the host's cost of a call -- wrapper, binding, launcher, launches."""
    res = {'lib': os.path.relpath(gnerf_hip.LIB_PATH, ROOT), 'binding': 'ctypes' if gnerf_hip.ext() is None else 'gnerf_torch_ext'}
    fwd, bwd = scene(1, 64 * 64, 64, 48, 48), scene(1, 64, 8, 48, 48)
    for name, fn in (('forward 64x64 48+48', lambda: forward(fwd, planes_absmax=fwd['amax'])), ('backward 8x8 48+48', lambda: backward(bwd, planes_absmax=bwd['amax']))):
        for _ in range(100):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(1000):
                fn()
            torch.cuda.synchronize()
            us.append(round((time.perf_counter() - t0) / 1000 * 1e6, 2))
        res[name + ' us/call'] = {'repeats': us, 'median': statistics.median(us), 'spread': round(max(us) - min(us), 2)}
    print(json.dumps(res), flush=True)


def main():
    img = scene(1, 64, 8, 48, 48)                           # 8x8 image, N = 1
    ragged = scene(2, 24, 0, 48, 48)                        # N = 2, 24 rays each, no image: 16-ray tiles straddle the items
    run('fwd 8x8 48+48', lambda: forward(img))
    run('fwd 8x8 disparity', lambda: forward(img, disparity_space_sampling=True))
    run('fwd 8x8 GNERF_PIPE_FULL=0', lambda: forward(img), {'GNERF_PIPE_FULL': '0'})
    run('fwd 8x8 48+0', lambda: forward(scene(1, 64, 8, 48, 0)))
    run('fwd 8x8 96+96', lambda: forward(scene(1, 64, 8, 96, 96)))
    run('fwd 8x8 128+128', lambda: forward(scene(1, 64, 8, 128, 128)))
    run('fwd 8x8 160+160', lambda: forward(scene(1, 64, 8, 160, 160)))
    run('fwd 8x8 GNERF_RENDER_KERNEL=generic', lambda: forward(img), {'GNERF_RENDER_KERNEL': 'generic'})
    for mlp in ('f32', 'f16x3', 'auto'):
        run(f'fwd 8x8 mlp={mlp}', lambda: forward(img, mlp=mlp))
        run(f'fwd 8x8 mlp={mlp} planes_absmax', lambda: forward(img, mlp=mlp, planes_absmax=img['amax']))
    big = scene(1, 96 * 96, 96, 48, 48)                     # 9216 rays >= 4 x 256 x 8: units are dealt on demand
    run('fwd 96x96 dealing default', lambda: forward(big))
    for dealing in ('static', 'uniform', 'guided:2:2', 'guided:x'):
        run(f'fwd 96x96 GNERF_PIPE_DEALING={dealing}', lambda: forward(big), {'GNERF_PIPE_DEALING': dealing})
    run('fwd 64x64 cameras + rng', lambda: forward_generated(scene(1, 64 * 64, 64, 48, 48)))
    run('fwd 3 views of one item, depth_clamp_per_item', lambda: forward_views(scene(3, 64, 8, 48, 48)))
    run('fwd ragged 2x24', lambda: forward(ragged))
    run('fwd 8x8 sigma_noise', lambda: forward(img, sigma_noise=img['sigma_noise']))

    for tag, sc in (('8x8', img), ('ragged', ragged)):
        run(f'bwd {tag} default', lambda: backward(sc))
        run(f'bwd {tag} planes only', lambda: backward(sc, need_decoder=False))
        run(f'bwd {tag} decoder only', lambda: backward(sc, need_planes=False))
        run(f'bwd {tag} staged_scatter=False', lambda: backward(sc, staged_scatter=False))
        run(f'bwd {tag} GNERF_BWD_KERNEL=wave', lambda: backward(sc), {'GNERF_BWD_KERNEL': 'wave'})
        run(f'bwd {tag} GNERF_BWD_SCATTER=direct', lambda: backward(sc), {'GNERF_BWD_SCATTER': 'direct'})
        run(f'bwd {tag} GNERF_BWD_SCATTER=sorted', lambda: backward(sc), {'GNERF_BWD_SCATTER': 'sorted'})
        run(f'bwd {tag} GNERF_BWD_SCATTER=staged', lambda: backward(sc), {'GNERF_BWD_SCATTER': 'staged'})
        run(f'bwd {tag} GNERF_BWD_MLP=f32', lambda: backward(sc), {'GNERF_BWD_MLP': 'f32'})
        run(f'bwd {tag} GNERF_BWD_MLP_K1=f32 _K2=f16x3', lambda: backward(sc), {'GNERF_BWD_MLP_K1': 'f32', 'GNERF_BWD_MLP_K2': 'f16x3'})
        run(f'bwd {tag} need_rays', lambda: backward(sc, need_rays=True))
        run(f'bwd {tag} need_rays, no planes', lambda: backward(sc, need_rays=True, need_planes=False))
        run(f'bwd {tag} need_rays, rays alone', lambda: backward(sc, need_rays=True, need_planes=False, need_decoder=False))
        run(f'bwd {tag} need_rays GNERF_BWD_SCATTER=direct', lambda: backward(sc, need_rays=True), {'GNERF_BWD_SCATTER': 'direct'})
        run(f'bwd {tag} need_rays per-ray limits', lambda: backward(sc, need_rays=True, ray_start=torch.full([sc['n'] * sc['m']], 2.25, device=dev)))
    run('bwd ragged GNERF_BWD_SCATTER=staged GNERF_BWD_KERNEL=wave', lambda: backward(ragged), {'GNERF_BWD_SCATTER': 'staged', 'GNERF_BWD_KERNEL': 'wave'})
    run('bwd ragged need_rays GNERF_BWD_KERNEL=wave', lambda: backward(ragged, need_rays=True), {'GNERF_BWD_KERNEL': 'wave'})
    run('bwd 8x8 160+160', lambda: backward(scene(1, 64, 8, 160, 160)))
    run('bwd ragged 160+160', lambda: backward(scene(2, 24, 0, 160, 160)))

    g = torch.Generator().manual_seed(5)
    pts = (torch.rand(2, 40, 3, generator=g) - 0.5).to(dev)
    g_sigma, g_rgb = torch.randn(2, 40, 1, generator=g).to(dev), torch.randn(2, 40, 32, generator=g).to(dev)
    two = scene(2, 16, 4, 48, 48)
    run('query_points', lambda: gnerf_hip.query_points(two['nhwc'], 2, two['dec'], pts, 1.0))
    run('query_points_backward', lambda: gnerf_hip.query_points_backward(two['nhwc'], 2, two['dec'], pts, 1.0, g_sigma, g_rgb))
    run('query_points_backward, no decoder', lambda: gnerf_hip.query_points_backward(two['nhwc'], 2, two['dec'], pts, 1.0, g_sigma, g_rgb, need_decoder=False))
    run('query_points_grad', lambda: gnerf_hip.query_points_grad(two['nhwc'], 2, two['dec'], pts, 1.0, g_sigma, g_rgb))
    run('query_points_grad, no grad_rgb', lambda: gnerf_hip.query_points_grad(two['nhwc'], 2, two['dec'], pts, 1.0, g_sigma, None))
    # n_points over the cap with null pointers: the cap is checked first
    lib, over = gnerf_hip.load(), (2 ** 31 - 1 - 15) // 3 + 1
    null = [None] * 4
    for name, args in (('gnerf_query_points', (*null, None, None, 0)), ('gnerf_query_points_backward', (*null, None, None, None, None, None, None, None, 0)),
                       ('gnerf_query_points_grad', (*null, None, None, None, 0))):
        code = getattr(lib, name)(None, 2, PLANE, PLANE, None, over, 1.0, *args, None)
        print(json.dumps({'case': f'{name} over the cap, null pointers', 'code': code, 'error': lib.gnerf_last_error().decode()}), flush=True)


if __name__ == '__main__':
    host_cost() if '--host-cost' in sys.argv[1:] else main()
