"""The fused volume renderer and the point queries (csrc/render.hip, render_pipe.hip, render_backward.hip, render_query.hip and the .inl files they include): the one builder of gnerf_render_params and the calls."""

import ctypes
import os

import torch

from . import _native
from ._native import DEBUG_SLOTS, MLP_MODES, RenderGrads, RenderParams, _EMPTY, _launch, _on_device, _ptr, _require_cuda, _stream, _workspace, load, profiled


def planes_layout(planes_nhwc, n_items, what):
    """0 for [3N,H,W,32] (one NHWC image per plane), 1 for [N,H,W,96] (planes interleaved per texel: channels_last memory of the
    backbone's [N,96,H,W] output).  Anything else raises."""
    if planes_nhwc.dtype != torch.float32 or not planes_nhwc.is_contiguous() or planes_nhwc.ndim != 4:
        raise RuntimeError(f'{what}: planes must be a contiguous float32 4-D tensor')
    if planes_nhwc.shape[3] == 32 and planes_nhwc.shape[0] == 3 * n_items:
        return 0
    if planes_nhwc.shape[3] == 96 and planes_nhwc.shape[0] == n_items:
        return 1
    raise RuntimeError(f'{what}: planes_nhwc must be [3N,H,W,32] or [N,H,W,96] (3 planes of 32 channels per item)')


def last_mlp_choice(device):
    """Decoder arithmetic the last mlp='auto' render call on `device`'s current stream picked: 'f16x3' or 'f32' (None if no such
    call ran).  Reads the render workspace (synchronises); for tests and diagnostics."""
    ws = _native._workspaces.get((device.index, torch.cuda.current_stream(device).cuda_stream))
    if ws is None:
        return None
    return {1: 'f16x3', 2: 'f32'}.get(int(ws.view(torch.int32)[4].item()))


def _f32c(t):
    """t as a contiguous float32 tensor: t itself when it already is one (no copy, no dispatch)."""
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


def _mlp_mode(mlp, what):
    if mlp not in MLP_MODES:
        raise RuntimeError(f"{what}: mlp must be one of {sorted(MLP_MODES)}")
    return MLP_MODES[mlp]


def _ray_limits(ray_start, ray_end, n_items, m, dev, what):
    """(ray_start, ray_end, start_per_ray, end_per_ray): two floats and two Nones for scalar limits; when either limit is a tensor, both
    as float32 [N*M] tensors (a scalar one broadcast) and 0.0 for the floats."""
    if not (isinstance(ray_start, torch.Tensor) or isinstance(ray_end, torch.Tensor)):
        return float(ray_start), float(ray_end), None, None
    rs_t, re_t = (_f32c(v if isinstance(v, torch.Tensor) else torch.as_tensor(v, device=dev).expand(n_items, m, 1)).reshape(-1) for v in (ray_start, ray_end))
    if rs_t.numel() != n_items * m or re_t.numel() != n_items * m:
        raise RuntimeError(f'{what}: per-ray ray_start / ray_end must have N*M elements')
    return 0.0, 0.0, rs_t, re_t


def _render_params(planes_nhwc, n_items, decoder, ray_origins, ray_dirs, noise_coarse, noise_fine,
                   depth_resolution, depth_resolution_importance, ray_start, ray_end, box_warp,
                   white_back, disparity_space_sampling, image_width, what, planes_absmax=None, mlp='auto',
                   planes_shared=False, depth_clamp_per_item=False, cameras=None, rng=None):
    """Validate the arguments shared by render_forward / render_backward and fill a RenderParams.
    Returns (params, keepalive, rays_per_item); `keepalive` holds the converted tensors the pointers refer to.
    Two independent choices after the common part.  Rays: tensors, or cameras = (cam2world [N,4,4], intrinsics [N,3,3], res) with
    ray_origins = ray_dirs = None -- made in the kernel.  Draws: tensors, or rng = a TorchPhiloxPlan with noise_coarse = noise_fine = None
    -- made in the kernel (gnerf_render_params, ABI 8).  Either in-kernel form takes scalar ray limits."""
    w1, b1, w2, b2 = decoder
    _require_cuda(planes_nhwc, ray_origins, ray_dirs, noise_coarse, noise_fine, w1, b1, w2, b2)
    dev = planes_nhwc.device
    p = RenderParams()
    p.planes_interleaved = planes_layout(planes_nhwc, 1 if planes_shared else n_items, what)
    if tuple(w1.shape) != (64, 32) or tuple(b1.shape) != (64,) or tuple(w2.shape) != (33, 64) or tuple(b2.shape) != (33,):
        raise RuntimeError(f'{what}: decoder must be the 32->64->33 OSGDecoder MLP')
    if (cameras is not None or rng is not None) and (isinstance(ray_start, torch.Tensor) or isinstance(ray_end, torch.Tensor)):
        raise RuntimeError(f'{what}: in-kernel rays / draws take scalar ray limits')
    S, F = int(depth_resolution), int(depth_resolution_importance)
    if cameras is not None:
        if ray_origins is not None or ray_dirs is not None:
            raise RuntimeError(f'{what}: give rays or cameras, not both')
        c2w, intr, res = cameras
        _require_cuda(c2w, intr)
        rays = c2w, intr = _f32c(c2w), _f32c(intr)
        if tuple(c2w.shape) != (n_items, 4, 4) or tuple(intr.shape) != (n_items, 3, 3):
            raise RuntimeError(f'{what}: cameras must be cam2world [N,4,4] and intrinsics [N,3,3]')
        m, image_width = int(res) * int(res), int(res)
        p.cam2world, p.intrinsics = c2w.data_ptr(), intr.data_ptr()
    else:
        rays = o, d = _f32c(ray_origins), _f32c(ray_dirs)
        if o.shape != d.shape or o.ndim != 3 or o.shape[0] != n_items or o.shape[2] != 3:
            raise RuntimeError(f'{what}: rays must be [N,M,3]')
        m = o.shape[1]
        p.ray_origins, p.ray_dirs = o.data_ptr(), d.data_ptr()
    nc = nf = None
    if rng is not None:
        if noise_coarse is not None or noise_fine is not None:
            raise RuntimeError(f'{what}: give noise tensors or an rng plan, not both')
        p.rng_mode = 1
        p.rng_per_item = int(rng.per_item)
        p.rng_seed, p.rng_offset_coarse, p.rng_offset_fine = rng.seed, rng.offset_coarse, rng.offset_fine
        p.rng_offset_item_stride, p.rng_threads_coarse, p.rng_threads_fine = rng.item_stride, rng.threads_coarse, rng.threads_fine
    else:
        nc = _f32c(noise_coarse)
        if nc.numel() != n_items * m * S:
            raise RuntimeError(f'{what}: noise_coarse must have N*M*S elements')
        if F > 0:
            if noise_fine is None:
                raise RuntimeError(f'{what}: noise_fine required when depth_resolution_importance > 0')
            nf = _f32c(noise_fine)
            if nf.numel() != n_items * m * F:
                raise RuntimeError(f'{what}: noise_fine must have N*M*F elements')
        p.noise_coarse, p.noise_fine = nc.data_ptr(), _ptr(nf)
    w1, b1, w2, b2 = _f32c(w1), _f32c(b1), _f32c(w2), _f32c(b2)
    p.ray_start, p.ray_end, rs_t, re_t = _ray_limits(ray_start, ray_end, n_items, m, dev, what)
    p.ray_start_per_ray, p.ray_end_per_ray = _ptr(rs_t), _ptr(re_t)
    p.planes_nhwc = planes_nhwc.data_ptr(); p.n_items = n_items; p.plane_h = planes_nhwc.shape[1]; p.plane_w = planes_nhwc.shape[2]
    p.rays_per_item = m; p.image_width = int(image_width)
    p.w1, p.b1, p.w2, p.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    p.depth_resolution = S; p.depth_resolution_importance = F
    p.box_warp = float(box_warp); p.white_back = int(bool(white_back)); p.disparity_space_sampling = int(bool(disparity_space_sampling))
    p.mlp_mode = _mlp_mode(mlp, what)
    if planes_absmax is not None:
        _require_cuda(planes_absmax)
        if planes_absmax.dtype != torch.float32 or planes_absmax.numel() != 1:
            raise RuntimeError(f'{what}: planes_absmax must be a one-element float32 device tensor')
    p.planes_absmax = _ptr(planes_absmax)
    p.planes_shared = int(bool(planes_shared)); p.depth_clamp_per_item = int(bool(depth_clamp_per_item))
    return p, (planes_nhwc, *rays, nc, nf, w1, b1, w2, b2, rs_t, re_t, planes_absmax), m


def _zero_decoder_grads(device):
    """Zeroed float32 (grad_w1, grad_b1, grad_w2, grad_b2) for the kernels to accumulate into."""
    return tuple(torch.zeros(shape, dtype=torch.float32, device=device) for shape in ([64, 32], [64], [33, 64], [33]))


def _points(points, n_items, what):
    pts = points.to(torch.float32).contiguous()
    if pts.ndim != 3 or pts.shape[0] != n_items or pts.shape[2] != 3:
        raise RuntimeError(f'{what}: points must be [N,P,3]')
    return pts


def render_generated_supported(S, F, ray_start=0.0, ray_end=1.0, disparity_space_sampling=False, plan=None, numel_planes=None):
    """Do the render kernels make rays / draws themselves for these options?  (48+48 and 96+96 samples, plain stratified sampling; the
    pipelined kernel at its compile-time sample counts, which GNERF_RENDER_KERNEL / GNERF_PIPE_FULL=0 can take away; planes of one item
    below 4 GB.)  plan: a TorchPhiloxPlan whose generator geometry is checked too -- the kernel reproduces ATen's draw only when its
    thread count is a power of two or covers the draw (raygen.h: torch_rand_draw), which depends on the device's CU count."""
    if not (int(S) == int(F) and int(S) in (48, 96) and not disparity_space_sampling and not isinstance(ray_start, torch.Tensor) and not isinstance(ray_end, torch.Tensor)):
        return False
    if os.environ.get('GNERF_RENDER_KERNEL', 'pipe') != 'pipe' or os.environ.get('GNERF_PIPE_FULL', '1') == '0':
        return False
    if numel_planes is not None and int(numel_planes) * 4 >= (1 << 32):
        return False
    if plan is not None:
        for thr, numel in ((plan.threads_coarse, plan.numel_coarse), (plan.threads_fine, plan.numel_fine)):
            if numel and not (thr >= numel or (thr > 0 and thr & (thr - 1) == 0)):
                return False
        if plan.offset_coarse % 4 or plan.offset_fine % 4 or plan.item_stride % 4:
            return False
    return True


def render_ray_grad_available():
    """Does the loaded library export gnerf_render_backward_rays?  (Added without a new ABI version: a variant build of the same version
    made before it loads and answers False.)"""
    return hasattr(load(), 'gnerf_render_backward_rays')


def render_ray_grad_refusal(S, F, ray_start=0.0, ray_end=1.0, density_noise=0, views=False, staged_scatter=True):
    """Why render_backward(need_rays=True) does not cover these options, or None when it does: the host-side form of
    gnerf_render_backward_rays' refusals (include/gnerf_hip.h), for callers that must choose a route before the forward runs.
    Covered: numeric ray limits (with tensor limits -- 'auto' -- the coarse depths depend on the rays), no density noise, one set of
    planes per item of rays, sample counts the renderer takes, the staged two-pass backward."""
    S, F = int(S), int(F)
    if isinstance(ray_start, (torch.Tensor, str)) or isinstance(ray_end, (torch.Tensor, str)):
        return "per-ray ray limits ('auto') make the coarse depths depend on the rays"
    if density_noise:
        return 'density_noise is a forward-only option of the kernels'
    if views:
        return 'several views of one set of planes (planes_shared) are a forward-only launch'
    if not (2 <= S <= _native.MAX_SAMPLES and 0 <= F <= _native.MAX_SAMPLES and (F == 0 or S >= 4)):
        return f'{S}+{F} samples per ray are outside what the renderer takes'
    if not staged_scatter or os.environ.get('GNERF_BWD_SCATTER') == 'direct':
        return 'the single-pass backward stages no per-sample gradients'
    if not render_ray_grad_available():
        return 'the loaded library has no gnerf_render_backward_rays'
    return None


def render_ray_grad_supported(S, F, ray_start=0.0, ray_end=1.0, density_noise=0, views=False, staged_scatter=True):
    """render_ray_grad_refusal(...) is None."""
    return render_ray_grad_refusal(S, F, ray_start, ray_end, density_noise, views, staged_scatter) is None


def decoder_pack_available():
    """Does the loaded library export the decoder pack (gnerf_render_pack_decoder, gnerf_render_forward_packed)?  (Added without a new
    ABI version: a variant build of the same version made before it loads and answers False; render_forward then makes the plain call.)"""
    lib = load()
    return hasattr(lib, 'gnerf_render_pack_decoder') and hasattr(lib, 'gnerf_render_forward_packed')


def pack_decoder(decoder):
    """The decoder pack of decoder = (w1, b1, w2, b2), contiguous float32 on one GPU: a uint8 tensor that holds what the pipelined render
    kernels otherwise work out of the decoder in every workgroup (range statistics, the weights in their LDS layout), made by one small
    launch on the current stream.  Valid for the decoder's values at the time of the call.  render_forward makes and caches packs itself;
    this is for callers of the C ABI and for tests."""
    w1, b1, w2, b2 = decoder
    _require_cuda(w1, b1, w2, b2)
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in decoder) or \
            tuple(w1.shape) != (64, 32) or tuple(b1.shape) != (64,) or tuple(w2.shape) != (33, 64) or tuple(b2.shape) != (33,):
        raise RuntimeError('pack_decoder: decoder must be the 32->64->33 OSGDecoder MLP as contiguous float32 tensors')
    e = _native.ext()
    if e is not None:
        with _on_device(w1.device):
            return e.pack_decoder(w1, b1, w2, b2)
    pack = torch.empty([int(load().gnerf_render_decoder_pack_bytes())], dtype=torch.uint8, device=w1.device)
    _launch('gnerf_render_pack_decoder', w1, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), pack.data_ptr())
    return pack


DECODER_PACK_CACHE = 8      # packs render_forward keeps (and, apart from them, as many keys it has seen once)


def _decoder_pack(decoder):
    """The cached pack of `decoder` for a render call on the current stream, or None where the call goes without one.
    Keyed on the device, the STREAM and each tensor's data_ptr() and _version: an in-place update (an optimizer step) bumps the version
    and misses -- the contract ImportanceRenderer._decoder_cache already has; a pack is only ever used on the stream that made it (stream
    order is what says it is complete), so two streams that share a decoder hold a pack each.
    A pack is made when a key is seen the SECOND time: the launch that makes it (one workgroup, ~10 us in front of the render kernel)
    costs more than the call it serves gains, so a caller whose weights change before every call (a training loop: measured 0.440 ->
    0.447 ms per call with a pack made at first sight) goes without and runs as it did before there were packs, and a caller whose
    decoder stays (inference, an orbit, fit_camera, every call between two optimizer steps) pays one plain call and one tiny launch,
    then has the pack.  Keys seen once are remembered apart from the packs (_native._decoder_seen, as many, oldest out first) and take
    no pack's place; the packs are kept least-recently-USED first, so a stream of changing decoders never pushes out the pack of a
    decoder that is still being rendered.  An entry keeps its four tensors alive, so that an address cannot come back with other values
    under the same key.
    Inside a graph capture the answer is always None, whatever the cache holds: a captured launch keeps the ADDRESS of what it was
    given, the cache may drop any pack before a replay (the block would be handed out again and a replay would copy whatever is there
    into LDS as weights), and a plain captured call reads w1 .. b2 at replay time, so it follows in-place updates as it always has.  A
    caller that wants a pack inside a graph passes its own (render_forward's decoder_pack=<tensor>) and owns what that means."""
    w1, b1, w2, b2 = decoder
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in decoder):
        return None                 # (converted copies are new tensors on every call: nothing to key on)
    if torch.cuda.is_current_stream_capturing():
        return None
    try:
        key = (w1.device.index, _stream(w1), w1.data_ptr(), w1._version, b1.data_ptr(), b1._version, w2.data_ptr(), w2._version, b2.data_ptr(), b2._version)
    except RuntimeError:            # inference tensors track no version
        return None
    packs, seen = _native._decoder_packs, _native._decoder_seen
    hit = packs.pop(key, None)
    if hit is not None:
        packs[key] = hit            # most recently used: last out
        return hit[0]
    if not decoder_pack_available():
        return None
    if seen.pop(key, None) is None:             # first sight: remember the key, make nothing
        while len(seen) >= DECODER_PACK_CACHE:
            del seen[next(iter(seen))]
        seen[key] = decoder
        return None
    while len(packs) >= DECODER_PACK_CACHE:
        del packs[next(iter(packs))]            # the least recently used
    pack = pack_decoder(decoder)                # second sight
    packs[key] = (pack, decoder)
    return pack


@profiled('gnerf_hip::render_forward')
def render_forward(planes_nhwc, n_items, decoder, ray_origins, ray_dirs, noise_coarse, noise_fine, *,
                   depth_resolution, depth_resolution_importance, ray_start, ray_end, box_warp,
                   white_back=False, disparity_space_sampling=False, image_width=0, debug=False, planes_absmax=None, mlp='auto',
                   planes_shared=False, depth_clamp_per_item=False, cameras=None, rng=None, sigma_noise=None, decoder_pack=True):
    """planes_nhwc [3N,H,W,32]; decoder = (w1,b1,w2,b2) effective fp32 weights; rays [N,M,3];
    decoder_pack: True (the default) = the call hands the kernels the decoder's pack (pack_decoder), cached per stream, decoder tensors
    and their versions and made when a decoder is seen the second time (_decoder_pack); never inside a graph capture, where the call is
    the plain one.  False = the plain call, in which every workgroup prepares the decoder itself.  A tensor = a pack the caller made of
    THESE weights.  Same results bit for bit either way -- PROVIDED the pack is of the weights' current values, which with True is the
    CALLER'S OBLIGATION in one respect: the cache notices a change of w1 .. b2 by the tensors' version counters alone, so a write that
    bumps none (through `w.data`, from another library, by a kernel given the raw address) must be followed by decoder_pack=False calls
    or by any in-place torch operation on the tensor; the plain call reads the tensors every time.  With a pack of the caller's own the
    weights are FROZEN at pack_decoder's call for as long as that pack is passed -- also in every replay of a graph that captured it,
    whose owner must keep the pack tensor alive as long as the graph.
    sigma_noise = (coarse [N*M,S], fine [N*M,F] or None): density noise ALREADY multiplied by density_noise, added to the two passes'
    densities before their ray marches (renderer.py:146-147); forward only, tensor rays and draws only.
    cameras = (cam2world [N,4,4], intrinsics [N,3,3], res) with ray_origins = ray_dirs = None: the kernel makes the rays gnerf_make_rays
    would (RaySampler.forward); rng = torch_philox_plan(...) with noise_coarse = noise_fine = None: the kernel makes the draws torch.rand
    would (both: render_generated_supported; bit-identical to the tensor forms, tests/test_gpu_parity.py).
    noise_coarse [N*M,S]; noise_fine [N*M,F] or None; ray_start/ray_end floats or [N*M] tensors.
    planes_shared: planes_nhwc holds ONE item's planes ([3,H,W,32] or [1,H,W,96]) that all N items of rays read (N views of one
    object in one launch).  depth_clamp_per_item: the final depth clamp (ray_marcher.py:49-50) takes its range from each item's
    own samples instead of the whole call's, so that item i's outputs equal those of a call with item i alone.
    mlp: decoder arithmetic, 'auto' (decided on the device from planes_absmax -- the one-element tensor planes_to_nhwc(...,
    with_absmax=True) returns; measured by the call itself when None -- and the decoder's weights), 'f16x3' or 'f32'.
    Returns (rgb [N,M,32], depth [N,M,1], wsum [N,M,1][, debug [N*M,8,S+F]])."""
    if decoder_pack is True:
        _require_cuda(*decoder)
        pack = _decoder_pack(tuple(decoder))
    else:
        pack = None if decoder_pack is False else decoder_pack
    e = _native.ext()
    if e is not None and not debug and planes_nhwc.dtype == torch.float32 and planes_nhwc.is_contiguous() and cameras is None and rng is None and sigma_noise is None:
        # the C++ binding: same validation and the same C ABI call, without ctypes marshalling.  It takes tensor rays and tensor draws
        # only: a call with cameras= or rng= (the renderer's in-kernel draws, which read NativeError.code) always goes through ctypes below
        mode = _mlp_mode(mlp, 'render_forward')
        dev = planes_nhwc.device
        rs, re, rs_t, re_t = _ray_limits(ray_start, ray_end, n_items, ray_origins.shape[1], dev, 'render_forward')
        w1, b1, w2, b2 = decoder
        with _on_device(dev):
            if pack is not None:
                return e.render_forward_packed(planes_nhwc, n_items, _f32c(w1), _f32c(b1), _f32c(w2), _f32c(b2), _f32c(ray_origins), _f32c(ray_dirs),
                                               _f32c(noise_coarse), _EMPTY if noise_fine is None else _f32c(noise_fine),
                                               int(depth_resolution), int(depth_resolution_importance), rs, re, _EMPTY if rs_t is None else rs_t,
                                               _EMPTY if re_t is None else re_t, float(box_warp), bool(white_back), bool(disparity_space_sampling),
                                               int(image_width), _EMPTY if planes_absmax is None else planes_absmax, mode, _workspace(dev),
                                               bool(planes_shared), bool(depth_clamp_per_item), pack)
            return e.render_forward(planes_nhwc, n_items, _f32c(w1), _f32c(b1), _f32c(w2), _f32c(b2), _f32c(ray_origins), _f32c(ray_dirs),
                                    _f32c(noise_coarse), _EMPTY if noise_fine is None else _f32c(noise_fine),
                                    int(depth_resolution), int(depth_resolution_importance), rs, re, _EMPTY if rs_t is None else rs_t,
                                    _EMPTY if re_t is None else re_t, float(box_warp), bool(white_back), bool(disparity_space_sampling),
                                    int(image_width), _EMPTY if planes_absmax is None else planes_absmax, mode, _workspace(dev),
                                    bool(planes_shared), bool(depth_clamp_per_item))
    p, keep, m = _render_params(planes_nhwc, n_items, decoder, ray_origins, ray_dirs, noise_coarse, noise_fine,
                                depth_resolution, depth_resolution_importance, ray_start, ray_end, box_warp,
                                white_back, disparity_space_sampling, image_width, 'render_forward', planes_absmax, mlp,
                                planes_shared, depth_clamp_per_item, cameras, rng)
    dev = planes_nhwc.device
    rgb = torch.empty([n_items, m, 32], dtype=torch.float32, device=dev)
    depth = torch.empty([n_items, m, 1], dtype=torch.float32, device=dev)
    wsum = torch.empty([n_items, m, 1], dtype=torch.float32, device=dev)
    dbg = torch.zeros([n_items * m, DEBUG_SLOTS, p.depth_resolution + p.depth_resolution_importance], dtype=torch.float32, device=dev) if debug else None
    ws = _workspace(dev)
    p.out_rgb, p.out_depth, p.out_wsum = rgb.data_ptr(), depth.data_ptr(), wsum.data_ptr()
    p.workspace = ws.data_ptr(); p.debug = None if dbg is None else dbg.data_ptr()
    if sigma_noise is not None:
        sc, sf = sigma_noise
        _require_cuda(sc, sf)
        sc = sc.detach().to(torch.float32).contiguous()
        sf = None if sf is None else sf.detach().to(torch.float32).contiguous()
        if sc.numel() != n_items * m * p.depth_resolution or (p.depth_resolution_importance > 0 and (sf is None or sf.numel() != n_items * m * p.depth_resolution_importance)):
            raise RuntimeError('render_forward: sigma_noise must be ([N*M,S], [N*M,F]) tensors')
        p.sigma_noise_coarse, p.sigma_noise_fine = sc.data_ptr(), None if sf is None else sf.data_ptr()
        keep = keep + (sc, sf)
    if pack is not None:
        if pack.device != dev or pack.dtype != torch.uint8 or not pack.is_contiguous() or pack.numel() < int(load().gnerf_render_decoder_pack_bytes()):
            raise RuntimeError("render_forward: decoder_pack is not a pack on the planes' device")
        _launch('gnerf_render_forward_packed', planes_nhwc, ctypes.byref(p), pack.data_ptr())
    else:
        _launch('gnerf_render_forward', planes_nhwc, ctypes.byref(p))
    del keep
    if debug:
        return rgb, depth, wsum, dbg
    return rgb, depth, wsum


@profiled('gnerf_hip::render_backward')
def render_backward(planes_nhwc, n_items, decoder, ray_origins, ray_dirs, noise_coarse, noise_fine, grad_rgb, grad_depth, grad_wsum, *,
                    depth_resolution, depth_resolution_importance, ray_start, ray_end, box_warp,
                    white_back=False, disparity_space_sampling=False, image_width=0, need_planes=True, need_decoder=True,
                    staged_scatter=True, planes_absmax=None, need_rays=False, sigma_noise=None):
    """Gradient of render_forward for the same arguments (the forward pass is recomputed inside the kernel).
    grad_rgb [N,M,32], grad_depth [N,M,1], grad_wsum [N,M,1]; any of them may be None (zeros).
    staged_scatter: make the plane gradient in two passes through a staging buffer (per-texel aggregation in LDS before the
    atomics; see include/gnerf_hip.h) -- the default; False = the single-pass form.
    planes_absmax: max |planes| as for render_forward (the staged form's first pass picks its decoder arithmetic from it on the
    device; measured by the call when None).
    need_rays: also the gradient with respect to the rays (gnerf_render_backward_rays; render_ray_grad_supported says which calls it
    covers, anything else raises NativeError with code E_UNSUPPORTED before a launch).  The staging buffer is then made whether or not
    a plane gradient is asked for, and the return value gains a third element (grad_origins, grad_dirs), both [N,M,3] float32.
    sigma_noise: as render_forward's; the backward refuses it (E_UNSUPPORTED), so that a forward call's options can be passed on as they are.
    Returns (grad_planes_nhwc [3N,H,W,32] or None, (grad_w1, grad_b1, grad_w2, grad_b2) or None), all float32."""
    p, keep, m = _render_params(planes_nhwc, n_items, decoder, ray_origins, ray_dirs, noise_coarse, noise_fine,
                                depth_resolution, depth_resolution_importance, ray_start, ray_end, box_warp,
                                white_back, disparity_space_sampling, image_width, 'render_backward', planes_absmax)
    dev = planes_nhwc.device
    _require_cuda(grad_rgb, grad_depth, grad_wsum)
    grads_in = []
    for t, n in ((grad_rgb, 32), (grad_depth, 1), (grad_wsum, 1)):
        if t is not None:
            t = t.to(torch.float32).contiguous()
            if t.numel() != n_items * m * n:
                raise RuntimeError('render_backward: output gradients must match the forward outputs')
        grads_in.append(t)
    g = RenderGrads()
    g.grad_rgb, g.grad_depth, g.grad_wsum = [None if t is None else t.data_ptr() for t in grads_in]
    g_planes = torch.zeros_like(planes_nhwc) if need_planes else None
    g_dec = _zero_decoder_grads(dev) if need_decoder else None
    if g_dec is not None:
        g.grad_w1, g.grad_b1, g.grad_w2, g.grad_b2 = [t.data_ptr() for t in g_dec]
    g.grad_planes_nhwc = None if g_planes is None else g_planes.data_ptr()
    if sigma_noise is not None:
        sc, sf = sigma_noise
        _require_cuda(sc, sf)
        sc, sf = _f32c(sc.detach()), None if sf is None else _f32c(sf.detach())
        p.sigma_noise_coarse, p.sigma_noise_fine = sc.data_ptr(), _ptr(sf)
        keep = keep + (sc, sf)
    stage = None
    if (g_planes is not None or need_rays) and staged_scatter:
        # Staging buffer of the two-pass scatter (gnerf_render_backward_stage_bytes: bounded, the passes run over batches of ray
        # tiles).  Allocated per call on the current stream: torch's caching allocator hands the block back to the rest of the
        # step afterwards (a buffer cached here would be invisible to it).  Out of memory -> the single-pass form, same result.
        nbytes = int(load().gnerf_render_backward_stage_bytes(ctypes.byref(p)))
        try:
            stage = torch.empty([nbytes], dtype=torch.uint8, device=dev)
            g.scatter_stage = stage.data_ptr()
        except torch.OutOfMemoryError:
            stage = None
    elif g_planes is None and g_dec is not None and staged_scatter:
        # decoder gradients only: the small per-sample exchange buffer of the pipelined path (1.5 KB per ray at 48+48)
        try:
            stage = torch.empty([int(load().gnerf_render_backward_exchange_bytes(ctypes.byref(p)))], dtype=torch.uint8, device=dev)
            g.scatter_stage = stage.data_ptr()
        except torch.OutOfMemoryError:
            stage = None
    if need_rays:
        # an allocation that failed leaves no staging buffer: the call below says so (E_UNSUPPORTED), there is no single-pass ray gradient
        e = _native.ext()
        if e is not None and sigma_noise is None and stage is not None and \
                render_ray_grad_refusal(p.depth_resolution, p.depth_resolution_importance, ray_start, ray_end, staged_scatter=staged_scatter) is None:
            # the C++ binding: the same C ABI call on the same buffers.  What the call refuses (the host-side predicate knows) goes through
            # ctypes, whose failures carry the C ABI's return code (NativeError.code)
            o, d, nc, nf, w1, b1, w2, b2 = keep[1:9]
            with _on_device(dev):
                g_rays = e.render_backward_rays(planes_nhwc, n_items, w1, b1, w2, b2, o, d, nc, nf, p.depth_resolution, p.depth_resolution_importance,
                                                p.ray_start, p.ray_end, None, None, float(box_warp), bool(white_back), bool(disparity_space_sampling),
                                                int(image_width), planes_absmax, *grads_in, g_planes, list(g_dec or ()), stage)
        else:
            g_o = torch.empty([n_items, m, 3], dtype=torch.float32, device=dev)
            g_d = torch.empty([n_items, m, 3], dtype=torch.float32, device=dev)
            _launch('gnerf_render_backward_rays', planes_nhwc, ctypes.byref(p), ctypes.byref(g), g_o.data_ptr(), g_d.data_ptr())
            g_rays = (g_o, g_d)
        del keep, grads_in, stage
        return g_planes, g_dec, g_rays
    _launch('gnerf_render_backward', planes_nhwc, ctypes.byref(p), ctypes.byref(g))
    del keep, grads_in, stage
    return g_planes, g_dec


def scatter_plane_rows_available():
    """Does the loaded library export gnerf_render_scatter_rows?  (Added without a new ABI version: a variant build of the same version
    made before it loads and answers False.)"""
    return hasattr(load(), 'gnerf_render_scatter_rows')


def scatter_plane_rows(planes_like, n_items, origins, dirs, depths, rows, *, box_warp, image_width=0, out=None):
    """The second pass of the staged backward alone (gnerf_render_scatter_rows): the plane gradient of rows the caller wrote.
    planes_like: a float32 GPU tensor laid out as the planes, [3N,H,W,32] or interleaved [N,H,W,96] (only shape and layout are read);
    origins, dirs [N,M,3]; depths [N,M,K] (any order: the scatter sums); rows [N,M,K,32], dL/d(mean feature) of the sample at that depth.
    The call fills a staging buffer as the staged first pass would and runs the scatter gnerf_render_backward would pick
    (GNERF_BWD_SCATTER=sorted: the LDS-merged atomic form).  out: a gradient tensor like planes_like to ADD into; a zeroed one otherwise.
    Returns the gradient, laid out like planes_like."""
    what = 'scatter_plane_rows'
    _require_cuda(planes_like, origins, dirs, depths, rows, out)
    o, d, t, r = _f32c(origins), _f32c(dirs), _f32c(depths), _f32c(rows)
    if t.ndim != 3 or tuple(t.shape[:2]) != tuple(o.shape[:2]) or tuple(r.shape) != (*t.shape, 32):
        raise RuntimeError(f'{what}: depths must be [N,M,K] and rows [N,M,K,32]')
    dev, n_all = planes_like.device, int(t.shape[2])
    # the scatter dereferences neither planes, decoder nor draws: the params carry them because the whole call's validation asks for them
    spare = torch.zeros([64 * 33], dtype=torch.float32, device=dev)
    p, keep, m = _render_params(planes_like, n_items, (spare[:64 * 32].view(64, 32), spare[:64], spare.view(33, 64), spare[:33]), o, d, t, None,
                                n_all, 0, 1.0, 2.0, box_warp, False, False, image_width, what)
    if out is None:
        out = torch.zeros_like(planes_like)
    elif out.dtype != torch.float32 or out.shape != planes_like.shape or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f'{what}: out must be a contiguous float32 tensor like planes_like')
    stage = torch.empty([int(load().gnerf_render_backward_stage_bytes(ctypes.byref(p)))], dtype=torch.uint8, device=dev)
    rays = n_items * m
    front = stage[:rays * 33 * n_all * 4].view(torch.float32).view(rays, 33 * n_all)
    front[:, :n_all] = t.reshape(rays, n_all)
    front[:, n_all:] = r.reshape(rays, n_all * 32)
    _launch('gnerf_render_scatter_rows', planes_like, ctypes.byref(p), stage.data_ptr(), out.data_ptr())
    del keep, stage
    return out


@profiled('gnerf_hip::query_points')
def query_points(planes_nhwc, n_items, decoder, points, box_warp, want_rgb=True):
    """run_model for arbitrary points [N,P,3] -> sigma [N,P,1], rgb [N,P,32] (rgb None when want_rgb is False)."""
    w1, b1, w2, b2 = [t.to(torch.float32).contiguous() for t in decoder]
    _require_cuda(planes_nhwc, points, w1)
    pts = _points(points, n_items, 'query_points')
    n_pts = pts.shape[1]
    interleaved = planes_layout(planes_nhwc, n_items, 'query_points')
    sigma = torch.empty([n_items, n_pts, 1], dtype=torch.float32, device=pts.device)
    rgb = torch.empty([n_items, n_pts, 32], dtype=torch.float32, device=pts.device) if want_rgb else None
    _launch('gnerf_query_points', pts, _ptr(planes_nhwc), n_items, planes_nhwc.shape[1], planes_nhwc.shape[2], _ptr(pts), n_pts, float(box_warp),
            _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(sigma), _ptr(rgb), interleaved)
    return sigma, rgb


@profiled('gnerf_hip::query_points_backward')
def query_points_backward(planes_nhwc, n_items, decoder, points, box_warp, grad_sigma, grad_rgb, need_planes=True, need_decoder=True):
    """Gradient of query_points for the same arguments: grad_sigma [N,P,1] / grad_rgb [N,P,32] (either may be None).
    Returns (grad_planes_nhwc or None, (grad_w1, grad_b1, grad_w2, grad_b2) or None), float32."""
    w1, b1, w2, b2 = [t.to(torch.float32).contiguous() for t in decoder]
    _require_cuda(planes_nhwc, points, w1, grad_sigma, grad_rgb)
    interleaved = planes_layout(planes_nhwc, n_items, 'query_points_backward')
    pts = _points(points, n_items, 'query_points_backward')
    n_pts = pts.shape[1]
    gs = None if grad_sigma is None else grad_sigma.to(torch.float32).contiguous()
    gc = None if grad_rgb is None else grad_rgb.to(torch.float32).contiguous()
    if (gs is not None and gs.numel() != n_items * n_pts) or (gc is not None and gc.numel() != n_items * n_pts * 32):
        raise RuntimeError('query_points_backward: output gradients must match the forward outputs')
    dev = pts.device
    g_planes = torch.zeros_like(planes_nhwc) if need_planes else None
    g_dec = _zero_decoder_grads(dev) if need_decoder else None
    gd = g_dec if g_dec is not None else (None, None, None, None)
    _launch('gnerf_query_points_backward', pts, _ptr(planes_nhwc), n_items, planes_nhwc.shape[1], planes_nhwc.shape[2], _ptr(pts), n_pts,
            float(box_warp), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(gs), _ptr(gc), _ptr(g_planes), _ptr(gd[0]), _ptr(gd[1]), _ptr(gd[2]),
            _ptr(gd[3]), interleaved)
    return g_planes, g_dec


@profiled('gnerf_hip::query_points_grad')
def query_points_grad(planes_nhwc, n_items, decoder, points, box_warp, grad_sigma, grad_rgb):
    """Gradient of query_points with respect to the POINTS: grad_sigma [N,P,1] / grad_rgb [N,P,32] (either may be None, not both)
    -> grad_points [N,P,3] float32 (include/gnerf_hip.h states the maths).  grad_rgb None skips the decoder's colour half: with
    grad_sigma = ones the result is the density field's gradient, whose negative is the surface normal.  No atomics: the same bits
    on every run and through either binding."""
    w1, b1, w2, b2 = [_f32c(t) for t in decoder]
    _require_cuda(planes_nhwc, points, w1, grad_sigma, grad_rgb)
    interleaved = planes_layout(planes_nhwc, n_items, 'query_points_grad')
    pts = _points(points, n_items, 'query_points_grad')
    n_pts = pts.shape[1]
    if grad_sigma is None and grad_rgb is None:
        raise RuntimeError('query_points_grad: grad_sigma and grad_rgb are both None')
    gs = None if grad_sigma is None else _f32c(grad_sigma)
    gc = None if grad_rgb is None else _f32c(grad_rgb)
    if (gs is not None and gs.numel() != n_items * n_pts) or (gc is not None and gc.numel() != n_items * n_pts * 32):
        raise RuntimeError('query_points_grad: output gradients must match the forward outputs')
    e = _native.ext()
    if e is not None:
        with _on_device(pts.device):
            return e.query_points_grad(planes_nhwc, n_items, w1, b1, w2, b2, pts, float(box_warp), gs, gc)
    g_pts = torch.empty([n_items, n_pts, 3], dtype=torch.float32, device=pts.device)
    _launch('gnerf_query_points_grad', pts, _ptr(planes_nhwc), n_items, planes_nhwc.shape[1], planes_nhwc.shape[2], _ptr(pts), n_pts, float(box_warp),
            _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(gs), _ptr(gc), _ptr(g_pts), interleaved)
    return g_pts


def query_lattice_available():
    """Whether the loaded library has the lattice query (a version-15 library built before it does not)."""
    return hasattr(load(), 'gnerf_query_lattice')


def _query_lattice_ctypes(planes_nhwc, decoder, index, n, cube_length, box_warp, out, interleaved):
    """The ctypes route of query_lattice (arguments as query_lattice prepares them)."""
    w1, b1, w2, b2 = decoder
    _launch('gnerf_query_lattice', out, _ptr(planes_nhwc), planes_nhwc.shape[1], planes_nhwc.shape[2], _ptr(index), index.numel(), n, float(cube_length),
            float(box_warp), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(out), interleaved)


@profiled('gnerf_hip::query_lattice')
def query_lattice(planes_nhwc, decoder, index, n, cube_length, box_warp, out, binding=None):
    """Densities at lattice points named by their linear index: out[index] = sigma of ONE item's planes at the points
    voxel_samples(index, ..., n, cube_length) -- the positions are formed in the kernel with that function's fp32 arithmetic, so the bits are
    those of query_points(..., want_rgb=False) at them (include/gnerf_hip.h, gnerf_query_lattice).  index: CUDA int32 [m] (duplicates allowed; an
    empty list does nothing); out: a contiguous float32 CUDA tensor of n^3 values, written in place at the listed entries only.  Returns out.
    binding='ctypes' forces that route."""
    if not query_lattice_available():
        raise RuntimeError('gnerf_hip: this libgnerf_hip.so was built without gnerf_query_lattice: rebuild it (csrc/build.sh)')
    dec = [_f32c(t) for t in decoder]
    _require_cuda(planes_nhwc, index, out, dec[0])
    interleaved = planes_layout(planes_nhwc, 1, 'query_lattice')
    n = int(n)
    if n < 2 or n ** 3 >= 2 ** 31 or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n ** 3:
        raise RuntimeError('query_lattice: out must be a contiguous float32 tensor of n^3 < 2^31 values')
    if index.ndim != 1 or index.device != out.device:
        raise RuntimeError('query_lattice: index must be [m] on out\'s device')
    idx = index if (index.dtype == torch.int32 and index.is_contiguous()) else index.to(torch.int32).contiguous()
    if idx.numel() == 0:
        return out
    e = None if binding == 'ctypes' else _native.ext()
    if e is not None and hasattr(e, 'query_lattice'):
        with _on_device(out.device):
            e.query_lattice(planes_nhwc, *dec, idx, n, float(cube_length), float(box_warp), out)
    else:
        _query_lattice_ctypes(planes_nhwc, dec, idx, n, cube_length, box_warp, out, interleaved)
    return out


def project_to_level_available():
    """Whether the loaded library has the level-set projection kernel (a version-15 library built before it does not)."""
    return hasattr(load(), 'gnerf_project_points_to_level')


def _project_affine(affine):
    """affine as twelve Python floats that are exact C floats (row-major 3x4 [A | b]), or None."""
    if affine is None:
        return None
    a = torch.as_tensor(affine, dtype=torch.float64).detach().cpu().reshape(-1)
    if a.numel() == 16:                                                      # a 4x4 whose last row is 0 0 0 1
        if a[12:].tolist() != [0.0, 0.0, 0.0, 1.0]:
            raise ValueError('project_points_to_level: a 4x4 affine must end in the row 0 0 0 1')
        a = a[:12]
    if a.numel() != 12 or not bool(torch.isfinite(a).all()):
        raise ValueError('project_points_to_level: affine must hold twelve finite values (3x4 [A | b]) or be None')
    return [float(x) for x in a.to(torch.float32)]


def _project_points_to_level_ctypes(planes_nhwc, n_items, dec, pts, box_warp, level, affine, steps, radius, tol, interleaved):
    """The ctypes route of project_points_to_level (arguments as project_points_to_level prepares them)."""
    w1, b1, w2, b2 = dec
    n_pts, dev = pts.shape[1], pts.device
    out = torch.empty([n_items, n_pts, 3], dtype=torch.float32, device=dev)
    res_in = torch.empty([n_items, n_pts], dtype=torch.float32, device=dev)
    res_out = torch.empty([n_items, n_pts], dtype=torch.float32, device=dev)
    status = torch.empty([n_items, n_pts], dtype=torch.uint8, device=dev)
    _launch('gnerf_project_points_to_level', pts, _ptr(planes_nhwc), n_items, planes_nhwc.shape[1], planes_nhwc.shape[2], _ptr(pts), n_pts, float(box_warp),
            _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), level, None if affine is None else (ctypes.c_float * 12)(*affine), steps, radius, tol,
            _ptr(out), _ptr(res_in), _ptr(res_out), _ptr(status), interleaved)
    return out, status, res_in, res_out


@profiled('gnerf_hip::project_points_to_level')
def project_points_to_level(planes_nhwc, n_items, decoder, points, box_warp, level, affine=None, steps=6, radius=1.0, tol=2.0 ** -10):
    """Newton projection of points [N,P,3] onto the level set sigma = level of query_points' density, in one launch (include/gnerf_hip.h,
    gnerf_project_points_to_level, states the rules): at most `steps` steps along the gradient, never more than `radius` per axis from the
    start, done when |sigma - level| <= tol.  affine: None, or a 3x4 (or 4x4) [A | b] with world = A p + b for points in another frame
    (radius is in the points' frame).  -> (points_out [N,P,3] float32: the input's bits unless converged; status uint8 [N,P]: 0 converged,
    1 not converged, 2 flat or not finite; residual_in, residual_out float32 [N,P]: sigma - level before and after).  No atomics: the same
    bits on every run and through either binding."""
    if not project_to_level_available():
        raise RuntimeError('gnerf_hip: this libgnerf_hip.so was built without gnerf_project_points_to_level: rebuild it (csrc/build.sh)')
    dec = [_f32c(t) for t in decoder]
    _require_cuda(planes_nhwc, points, dec[0])
    interleaved = planes_layout(planes_nhwc, n_items, 'project_points_to_level')
    pts = _points(points, n_items, 'project_points_to_level')
    affine = _project_affine(affine)
    steps = int(steps)
    level, radius, tol = (float(torch.tensor(float(x), dtype=torch.float32)) for x in (level, radius, tol))
    if steps < 0:
        raise ValueError(f'project_points_to_level: steps must be >= 0, got {steps}')
    if not 0 <= radius < float('inf'):
        raise ValueError(f'project_points_to_level: radius must be finite and >= 0, got {radius}')
    if not 0 < tol < float('inf'):
        raise ValueError(f'project_points_to_level: tol must be a finite float32 > 0, got {tol}')
    if level != level or abs(level) == float('inf'):
        raise ValueError(f'project_points_to_level: level must be finite, got {level}')
    e = _native.ext()
    if e is not None and hasattr(e, 'project_points_to_level'):
        with _on_device(pts.device):
            return tuple(e.project_points_to_level(planes_nhwc, n_items, *dec, pts, float(box_warp), level, affine or [], steps, radius, tol))
    return _project_points_to_level_ctypes(planes_nhwc, n_items, dec, pts, box_warp, level, affine, steps, radius, tol, interleaved)
