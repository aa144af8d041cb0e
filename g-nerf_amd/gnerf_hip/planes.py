"""Tri-plane repacking, image conversion, ray generation and torch's Philox draws (csrc/planes.hip, raygen.h)."""

import ctypes

import torch

from . import _native
from ._native import _check, _launch, _ptr, _require_cuda, _workspace, load, profiled


@profiled('gnerf_hip::planes_to_nhwc')
def planes_to_nhwc(planes, with_absmax=False):
    """[N,3,C,H,W] (or [NP,C,H,W]) float32 NCHW -> [NP,H,W,C] contiguous.  with_absmax: also return max |planes| as a
    one-element device tensor, measured by the same pass (render_forward's planes_absmax)."""
    _require_cuda(planes)
    if planes.dtype != torch.float32:
        raise RuntimeError('planes_to_nhwc: planes must be float32')
    p = planes.reshape(-1, *planes.shape[-3:]).contiguous()
    np_, c, h, w = p.shape
    out = torch.empty([np_, h, w, c], dtype=torch.float32, device=p.device)
    if with_absmax:
        amax = torch.empty([1], dtype=torch.float32, device=p.device)
        _launch('gnerf_planes_to_nhwc_stats', p, _ptr(p), _ptr(out), np_, c, h, w, _ptr(amax), _workspace(p.device).data_ptr())
        return out, amax
    _launch('gnerf_planes_to_nhwc', p, _ptr(p), _ptr(out), np_, c, h, w)
    return out


@profiled('gnerf_hip::planes_absmax')
def planes_absmax(planes):
    """max |x| of a contiguous float32 device tensor -> one-element device tensor (NaN if any element is NaN)."""
    _require_cuda(planes)
    if planes.dtype != torch.float32 or not planes.is_contiguous() or planes.numel() == 0:
        raise RuntimeError('planes_absmax: expected a non-empty contiguous float32 tensor')
    amax = torch.empty([1], dtype=torch.float32, device=planes.device)
    _launch('gnerf_planes_absmax', planes, _ptr(planes), planes.numel(), _ptr(amax))
    return amax


@profiled('gnerf_hip::planes_from_nhwc')
def planes_from_nhwc(planes_nhwc, n_items=None):
    """[NP,H,W,C] float32 -> [NP,C,H,W] contiguous ([N,3,C,H,W] when n_items is given)."""
    _require_cuda(planes_nhwc)
    if planes_nhwc.dtype != torch.float32 or planes_nhwc.ndim != 4 or not planes_nhwc.is_contiguous():
        raise RuntimeError('planes_from_nhwc: expected a contiguous float32 [NP,H,W,C] tensor')
    np_, h, w, c = planes_nhwc.shape
    out = torch.empty([np_, c, h, w], dtype=torch.float32, device=planes_nhwc.device)
    _launch('gnerf_planes_from_nhwc', planes_nhwc, _ptr(planes_nhwc), _ptr(out), np_, c, h, w)
    return out if n_items is None else out.view(n_items, np_ // n_items, c, h, w)


@profiled('gnerf_hip::to_uint8_nhwc')
def to_uint8_nhwc(img):
    """(img * 127.5 + 128).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous() for a float32 [N,C,H,W] GPU tensor in one launch
    (gen_videos.py:173 + the frame writer's layout).  Returns uint8 [N,H,W,C]."""
    _require_cuda(img)
    if img.dtype != torch.float32 or img.ndim != 4 or not (1 <= img.shape[1] <= 64):
        raise RuntimeError('to_uint8_nhwc: expected a float32 [N,C,H,W] tensor with 1..64 channels')
    x = img.detach().contiguous()
    n, c, h, w = x.shape
    out = torch.empty([n, h, w, c], dtype=torch.uint8, device=x.device)
    _launch('gnerf_to_uint8_nhwc', x, _ptr(x), _ptr(out), n, c, h, w)
    return out


@profiled('gnerf_hip::make_rays')
def make_rays(cam2world, intrinsics, resolution):
    _require_cuda(cam2world, intrinsics)
    c2w = cam2world.to(torch.float32).contiguous()
    k = intrinsics.to(torch.float32).contiguous()
    n = c2w.shape[0]
    if c2w.shape != (n, 4, 4) or k.shape != (n, 3, 3):
        raise RuntimeError('make_rays: expected cam2world [N,4,4] and intrinsics [N,3,3]')
    o = torch.empty([n, resolution * resolution, 3], dtype=torch.float32, device=c2w.device)
    d = torch.empty_like(o)
    _launch('gnerf_make_rays', c2w, _ptr(c2w), _ptr(k), n, int(resolution), _ptr(o), _ptr(d))
    return o, d


@profiled('gnerf_hip::make_rays_and_draws')
def make_rays_and_draws(cam2world, intrinsics, resolution, S, F, generator=None):
    """make_rays(cam2world, intrinsics, resolution) AND the renderer's two uniform draws -- torch.rand([N,M,S,1]) then torch.rand(N*M, F)
    (renderer.py:190,241) -- in ONE launch (gnerf_make_rays_and_draws).  The draws are the device generator's: the values torch.rand would
    have returned, bit for bit, and the generator is left where those two calls would have left it (torch_philox_plan).  Returns
    (origins [N,M,3], dirs [N,M,3], noise_coarse [N,M,S,1], noise_fine [N*M,F] or None).  Not inside a graph capture (the generator's
    offset lives on the device then): the caller draws with torch.rand."""
    _require_cuda(cam2world, intrinsics)
    c2w = cam2world.to(torch.float32).contiguous()
    k = intrinsics.to(torch.float32).contiguous()
    n, dev = c2w.shape[0], c2w.device
    if c2w.shape != (n, 4, 4) or k.shape != (n, 3, 3):
        raise RuntimeError('make_rays_and_draws: expected cam2world [N,4,4] and intrinsics [N,3,3]')
    m = int(resolution) * int(resolution)
    plan = torch_philox_plan(dev, n, m, int(S), int(F), generator=generator, advance=False)
    o = torch.empty([n, m, 3], dtype=torch.float32, device=dev)
    d = torch.empty_like(o)
    nc = torch.empty([n, m, int(S), 1], dtype=torch.float32, device=dev)
    nf = torch.empty([n * m, int(F)], dtype=torch.float32, device=dev) if F > 0 else None
    _launch('gnerf_make_rays_and_draws', c2w, _ptr(c2w), _ptr(k), n, int(resolution), _ptr(o), _ptr(d), _ptr(nc), nc.numel(), plan.offset_coarse,
            plan.threads_coarse, _ptr(nf), 0 if nf is None else nf.numel(), plan.offset_fine, plan.threads_fine, plan.seed)
    commit_philox_plan(plan)
    return o, d, nc, nf


@profiled('gnerf_hip::upsample2x_add_nhwc')
def upsample2x_add_nhwc(img, y, f, flip=False, gain=4.0, with_absmax=False):
    """upfirdn2d(img, f, up=2, padding=[2,1,2,1], gain) + y written channels_last in one launch (the tri-plane producer's last
    step, networks_stylegan2.py:456-463).  img [N,C,h,w], y [N,C,2h,2w] or None, both float32 NCHW-contiguous; f the 4x4 filter.
    Returns a [N,C,2h,2w] tensor with channels_last strides (its memory is [N,2h,2w,C]) and, with_absmax, max |out| [1].
    Returns None when the kernel does not cover the shape (C % 32, w % 16, h % 2) -- the caller composes the ops instead."""
    _require_cuda(img, y)
    if img.dtype != torch.float32 or img.ndim != 4 or not img.is_contiguous() or tuple(f.shape) != (4, 4):
        return None
    n, c, h, w = img.shape
    if c % 32 or w % 16 or h % 2:
        return None
    if y is not None and (y.dtype != torch.float32 or tuple(y.shape) != (n, c, 2 * h, 2 * w) or not y.is_contiguous()):
        return None
    taps = _filter_taps(f)
    out = torch.empty([n, c, 2 * h, 2 * w], dtype=torch.float32, device=img.device, memory_format=torch.channels_last)
    amax = torch.empty([1], dtype=torch.float32, device=img.device) if with_absmax else None
    _launch('gnerf_upsample2x_add_nhwc', img, _ptr(img), _ptr(y), taps, 1 if flip else 0, float(gain), _ptr(out), n, c, h, w, _ptr(amax))
    return (out, amax) if with_absmax else out


def _filter_taps(f):
    """The 16 taps of a 4x4 filter as a host float array (one device read per filter tensor and version, then cached)."""
    key = (f.data_ptr(), f._version if not f.is_inference() else None, f.device)
    taps = _native._filter_tap_cache.get(key)
    if taps is None:
        if len(_native._filter_tap_cache) > 64:
            _native._filter_tap_cache.clear()
        taps = (ctypes.c_float * 16)(*f.detach().float().cpu().reshape(-1).tolist())
        _native._filter_tap_cache[key] = taps
    return taps


class TorchPhiloxPlan:
    """Where torch's device generator stands before the renderer's two uniform draws (renderer.py:190 rand_like([N,M,S,1]), :241
    rand(N*M, F)) and how ATen would have laid them out on this device -- what gnerf_render_params.rng_* carry (include/gnerf_hip.h,
    oracle/philox_ref.py).  per_item: N separate calls of one item each (the draws of the batched-views form)."""
    __slots__ = ('seed', 'offset_coarse', 'offset_fine', 'item_stride', 'threads_coarse', 'threads_fine', 'per_item', 'end_offset',
                 'numel_coarse', 'numel_fine', 'generator')


def torch_rand_geometry(numel, device):
    """(threads, philox offset increment) of `torch.rand(numel, device=device)` (gnerf_torch_rand_plan)."""
    geo = _native._device_geometry.get(device.index)
    if geo is None:
        pr = torch.cuda.get_device_properties(device)
        geo = _native._device_geometry[device.index] = (int(pr.multi_processor_count), int(pr.max_threads_per_multi_processor))
    thr, inc = ctypes.c_uint32(0), ctypes.c_uint64(0)
    _check(load().gnerf_torch_rand_plan(int(numel), geo[0], geo[1], ctypes.byref(thr), ctypes.byref(inc)), 'gnerf_torch_rand_plan')
    return thr.value, inc.value


def torch_philox_plan(device, n_items, rays_per_item, S, F, per_item=False, generator=None, advance=True):
    """Plan the renderer's two draws on `device`'s generator (default: torch's default generator of that device) and -- advance=True --
    move the generator past them, exactly as the torch.rand calls would have: a seeded run that renders with in-kernel draws leaves the
    generator where the reference's run leaves it.  Not usable while the stream is capturing a graph (graph-safe generators keep their
    offset on the device): the caller draws tensors then."""
    gen = generator if generator is not None else torch.cuda.default_generators[device.index]
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('torch_philox_plan: the stream is capturing a graph; draw with torch.rand instead')
    plan = TorchPhiloxPlan()
    plan.seed = int(gen.initial_seed()) & 0xFFFFFFFFFFFFFFFF
    plan.per_item = bool(per_item)
    units = rays_per_item if per_item else n_items * rays_per_item
    plan.threads_coarse, inc_c = torch_rand_geometry(units * S, device)
    plan.threads_fine, inc_f = torch_rand_geometry(units * F, device) if F > 0 else (0, 0)
    plan.numel_coarse, plan.numel_fine = units * S, units * F
    plan.generator = gen
    off = int(gen.get_offset())
    plan.offset_coarse, plan.offset_fine = off, off + inc_c
    plan.item_stride = inc_c + inc_f if per_item else 0
    plan.end_offset = off + (inc_c + inc_f) * (n_items if per_item else 1)
    if advance:
        gen.set_offset(plan.end_offset)
    return plan


def commit_philox_plan(plan):
    """Move the plan's generator past its two draws (for plans made with advance=False: a caller that wants to know that the launch was
    accepted before the generator moves)."""
    plan.generator.set_offset(plan.end_offset)


@profiled('gnerf_hip::torch_rand')
def torch_rand(numel, device, seed, offset):
    """Element for element what torch.rand(numel, device=device) returns with the device generator at (seed, offset): the render
    kernels' in-kernel draw as a stand-alone kernel (gnerf_torch_rand).  The generator is not touched."""
    threads, _ = torch_rand_geometry(numel, device)
    out = torch.empty(int(numel), dtype=torch.float32, device=device)
    _launch('gnerf_torch_rand', out, out.data_ptr(), int(numel), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), threads)
    return out
