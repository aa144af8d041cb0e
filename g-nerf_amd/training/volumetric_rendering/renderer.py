"""ImportanceRenderer with the reference's interface
(training/volumetric_rendering/renderer.py: generate_planes :23, project_onto_planes :39,
sample_from_planes :55, sample_from_3dgrid :67, ImportanceRenderer :82-253).

On a GPU the whole of `forward` -- depth proposals, tri-plane lookups, the decoder MLP, both ray
marches, importance resampling, the depth merge and the composite -- is ONE hand-written gfx950
kernel (csrc/render.hip through gnerf_hip.render_forward).  The random draws are still made by
torch, in the reference's order and shapes (rand_like([N,M,S,1]) then rand(N*M, F)), so a seeded
run consumes the generator exactly like the reference and produces the same image.

When autograd needs the gradient of the planes and/or the decoder (training), the same kernel runs
inside an autograd.Function whose backward is the second kernel (gnerf_hip.render_backward): it
recomputes the ray's forward pass and keeps nothing between the passes, where upstream autograd saves
every intermediate of the op chain (~3 GB at the training shape).

`run_model` (arbitrary points: sample / sample_mixed, incl. the density regulariser of training) has the
same pair of kernels (query_points / query_points_backward), and a third for the gradient of the points
themselves (query_points_grad: normals of the density field, `query_normals`).

The PyTorch-op form below is what runs for CPU tensors (the reference's own behaviour: all of its
renderer is PyTorch ops), when the rays themselves need a gradient, when the points need a SECOND-order
gradient (`ImportanceRenderer.fused_point_grad = False`), or when `decoder` is not the OSGDecoder
32->64->33 MLP.  A GPU call never silently degrades because the native library is absent:
gnerf_hip raises.
"""

import functools
import math
import warnings
import weakref

import torch
import torch.nn as nn

from training.volumetric_rendering.ray_marcher import MipRayMarcher2
from training.volumetric_rendering import math_utils

import os

import gnerf_hip

_KEEP_NHWC = os.environ.get('GNERF_KEEP_NHWC', '1') != '0'
# The two uniform draws made inside the render kernel (torch's own Philox stream, generator advanced as torch.rand would: same
# image, same generator state afterwards) instead of by two torch.rand launches.  Inference calls at 48+48 / 96+96 samples only.
_INKERNEL_RNG = os.environ.get('GNERF_INKERNEL_RNG', '0') == '1'
_NHWC_HINT = os.environ.get('GNERF_NHWC_PLANES', '0') == '1'


def generate_planes():
    """The three plane frames [3,3,3]; rows are the plane's axes.  With project_onto_planes they make
    plane 0 read (x,y), plane 1 (x,z) and plane 2 (z,x) -- EG3D's original choice, kept bit for bit."""
    return torch.tensor([[[1, 0, 0], [0, 1, 0], [0, 0, 1]],
                         [[1, 0, 0], [0, 0, 1], [0, 1, 0]],
                         [[0, 0, 1], [1, 0, 0], [0, 1, 0]]], dtype=torch.float32)


def project_onto_planes(planes, coordinates):
    """planes [P,3,3], coordinates [N,M,3] -> [N*P, M, 2]: coordinates expressed in each plane's frame,
    first two components."""
    N, M, _ = coordinates.shape
    P = planes.shape[0]
    pts = coordinates.unsqueeze(1).expand(-1, P, -1, -1).reshape(N * P, M, 3)
    frames = torch.linalg.inv(planes).unsqueeze(0).expand(N, -1, -1, -1).reshape(N * P, 3, 3)
    return torch.bmm(pts, frames)[..., :2]


def sample_from_planes(plane_axes, plane_features, coordinates, mode='bilinear', padding_mode='zeros', box_warp=None):
    """plane_features [N,P,C,H,W], coordinates [N,M,3] in world units -> [N,P,M,C]."""
    assert padding_mode == 'zeros'
    N, P, C, H, W = plane_features.shape
    M = coordinates.shape[1]
    # float64 planes and points -- an error in the reference, whose frames and grid are float32 -- keep their precision (query_normals
    # is checked against the float64 oracle that way); every other call is the reference's, grid.float() included
    f64 = plane_features.dtype == torch.float64 and coordinates.dtype == torch.float64
    grid = project_onto_planes(plane_axes.double() if f64 else plane_axes, (2 / box_warp) * coordinates).unsqueeze(1)
    grid = grid if f64 else grid.float()
    out = torch.nn.functional.grid_sample(plane_features.view(N * P, C, H, W), grid, mode=mode,
                                          padding_mode=padding_mode, align_corners=False)
    return out.permute(0, 3, 2, 1).reshape(N, P, M, C)


def sample_from_3dgrid(grid, coordinates):
    """grid [1 or B,C,H,W,D], coordinates [B,P,3] -> [B,P,C] (trilinear, zero padding)."""
    B, P, nd = coordinates.shape
    out = torch.nn.functional.grid_sample(grid.expand(B, -1, -1, -1, -1), coordinates.reshape(B, 1, 1, -1, nd),
                                          mode='bilinear', padding_mode='zeros', align_corners=False)
    N, C, H, W, D = out.shape
    return out.permute(0, 4, 3, 2, 1).reshape(N, H * W * D, C)


def _interleaved_view(planes):
    """If `planes` [N,3,32,H,W] is a view of a channels_last [N,96,H,W] tensor -- memory [N,H,W,96], what a producer that writes
    channels_last hands over (torch_utils.ops.upfirdn2d.upsample2d_add_channels_last; triplane.py:74's view keeps the strides) --
    return that memory as a contiguous [N,H,W,96] view; else None.  The render kernels address this layout in place."""
    if planes.ndim != 5 or planes.dtype != torch.float32:
        return None
    N, P, C, H, W = planes.shape
    want = (P * C * H * W, C, 1, P * C * W, P * C)
    # (the stride of a size-1 dimension is arbitrary -- `view` of a one-item batch reports 96 for dim 0 -- and irrelevant)
    if N * P * C * H * W == 0 or any(sz > 1 and st != w for sz, st, w in zip(planes.shape, planes.stride(), want)):
        return None
    return planes.as_strided((N, H, W, P * C), (P * C * H * W, P * C * W, P * C, 1), planes.storage_offset())


def _planes_from_interleaved(g, like):
    """[N,H,W,96] gradient in the interleaved layout -> a [N,3,32,H,W] view of it (the strides of `like`)."""
    N, P, C, H, W = like.shape
    return g.view(N, H, W, P, C).permute(0, 3, 4, 1, 2)


def _osg_decoder_weights(decoder):
    """Return the effective (w1,b1,w2,b2) of an OSGDecoder-shaped module (triplane.py:113-122:
    FullyConnectedLayer(32,64) -> Softplus -> FullyConnectedLayer(64,33), both 'linear' with bias),
    or None if `decoder` is anything else."""
    net = getattr(decoder, 'net', None)
    if not isinstance(net, nn.Sequential) or len(net) != 3 or not isinstance(net[1], nn.Softplus):
        return None
    if net[1].beta != 1 or net[1].threshold != 20:
        return None
    fc1, fc2 = net[0], net[2]
    for fc in (fc1, fc2):
        if getattr(fc, 'activation', None) != 'linear' or getattr(fc, 'bias', None) is None or not hasattr(fc, 'weight_gain'):
            return None
    if tuple(fc1.weight.shape) != (64, 32) or tuple(fc2.weight.shape) != (33, 64):
        return None
    return fc1, fc2


def _once_differentiable(message):
    """torch.autograd.function.once_differentiable with two differences: the error of a double backward is `message`, which says what
    to do, and it is raised whenever the first backward ran with a graph (create_graph=True) -- torch's decorator looks at the
    incoming gradients only, and the gradient of `sigma.sum()` requires none: an eikonal term on the fused route would otherwise fail
    with "does not require grad" or, worse, treat the first-order gradient as a constant."""
    def deco(fn):
        @functools.wraps(fn)
        def wrapper(ctx, *args):
            with torch.no_grad():
                outputs = fn(ctx, *args)
            if not torch.is_grad_enabled():
                return outputs
            err_fn = torch._C._functions.DelayedError(message, len(outputs))
            return err_fn(*[None if v is None else v.detach().requires_grad_(True) for v in outputs])
        return wrapper
    return deco


_once_differentiable_points = _once_differentiable(
    b'the fused point query (gnerf_hip.query_points_backward / query_points_grad) is differentiable once: for a second-order '
    b'gradient (e.g. an eikonal term) set ImportanceRenderer.fused_point_grad = False, which runs run_model as PyTorch ops')


def _once_differentiable_render(fn):
    """_FusedRender.backward: torch's once_differentiable as it always was, and the stricter form above when the rays get a gradient."""
    lax = torch.autograd.function.once_differentiable(fn)
    strict = _once_differentiable(
        b'the fused ray gradient (gnerf_hip.render_backward with need_rays) is differentiable once: for a second-order gradient set '
        b'ImportanceRenderer.fused_ray_grad = False, which runs the renderer as PyTorch ops')(fn)

    @functools.wraps(fn)
    def wrapper(ctx, *args):
        return (strict if (ctx.needs_input_grad[5] or ctx.needs_input_grad[6]) else lax)(ctx, *args)
    return wrapper


class _FusedRender(torch.autograd.Function):
    """render_forward / render_backward as one differentiable op.  Inputs with a gradient: planes [N,3,32,H,W], the
    decoder's effective weights and -- when the caller hands them in attached, which ImportanceRenderer does only where
    gnerf_hip.render_ray_grad_supported allows -- the rays (render_backward's need_rays); everything else is constant (importance
    depths are constants upstream as well, renderer.py:198/211).  `cfg` is the dict of static keyword arguments of
    gnerf_hip.render_forward.  Differentiable once."""

    @staticmethod
    def forward(ctx, planes, w1, b1, w2, b2, ray_origins, ray_dirs, noise_c, noise_f, ray_start, ray_end, cfg):
        N = planes.shape[0]
        nhwc = _interleaved_view(planes.detach())
        ctx.interleaved = nhwc is not None
        if ctx.interleaved:
            amax = _producer_absmax(planes)                 # None: the launcher measures it
        else:
            nhwc, amax = gnerf_hip.planes_to_nhwc(planes.detach().float(), with_absmax=True)
        # (decoder_pack=False: the effective weights of a differentiable call are new tensors on every call -- nothing a cached pack
        #  could be found by, and remembering them would push the packs of inference decoders out of gnerf_hip's small cache)
        out = gnerf_hip.render_forward(nhwc, N, (w1, b1, w2, b2), ray_origins, ray_dirs, noise_c, noise_f,
                                       ray_start=ray_start, ray_end=ray_end, planes_absmax=amax, decoder_pack=False, **cfg)
        ctx.amax = amax if not ctx.interleaved else None     # (of the NHWC copy made here; a producer's tag is looked up again in backward)
        tensors = [planes, w1, b1, w2, b2, ray_origins, ray_dirs, noise_c]
        # The NHWC copy is kept for the backward pass (the planes' size again: 25 MB per item) unless GNERF_KEEP_NHWC=0, in
        # which case the backward pass repacks the saved NCHW planes a second time (37 us per 100 MB).
        ctx.nhwc = nhwc if (_KEEP_NHWC and not ctx.interleaved) else None
        ctx.has_fine = noise_f is not None
        ctx.limits_are_tensors = isinstance(ray_start, torch.Tensor)
        if ctx.has_fine:
            tensors.append(noise_f)
        if ctx.limits_are_tensors:
            tensors += [ray_start, ray_end]
        else:
            ctx.limits = (ray_start, ray_end)
        ctx.save_for_backward(*tensors)
        ctx.cfg = cfg
        return out

    @staticmethod
    @_once_differentiable_render
    def backward(ctx, g_rgb, g_depth, g_wsum):
        saved = list(ctx.saved_tensors)
        planes, w1, b1, w2, b2, ray_origins, ray_dirs, noise_c = saved[:8]
        rest = saved[8:]
        noise_f = rest.pop(0) if ctx.has_fine else None
        ray_start, ray_end = (rest[0], rest[1]) if ctx.limits_are_tensors else ctx.limits
        need_planes = ctx.needs_input_grad[0]
        need_decoder = any(ctx.needs_input_grad[1:5])
        need_rays = ctx.needs_input_grad[5] or ctx.needs_input_grad[6]
        N = planes.shape[0]
        if ctx.interleaved:
            nhwc = _interleaved_view(planes.detach())
            amax = _producer_absmax(planes)
        else:
            nhwc = ctx.nhwc if ctx.nhwc is not None else gnerf_hip.planes_to_nhwc(planes.detach().float())
            amax = ctx.amax
        extra = dict(need_rays=True) if need_rays else {}
        g_planes, g_dec, *g_rays = gnerf_hip.render_backward(nhwc, N, (w1, b1, w2, b2), ray_origins, ray_dirs, noise_c, noise_f, g_rgb, g_depth, g_wsum,
                                                             ray_start=ray_start, ray_end=ray_end, need_planes=need_planes, need_decoder=need_decoder,
                                                             planes_absmax=amax, **extra, **ctx.cfg)
        grads = [None] * 12
        if need_rays:
            for i, (g, t) in enumerate(zip(g_rays[0], (ray_origins, ray_dirs))):
                if ctx.needs_input_grad[5 + i]:
                    grads[5 + i] = g.to(t.dtype)
        if need_planes:
            if ctx.interleaved:
                grads[0] = _planes_from_interleaved(g_planes, planes)                # laid out like the planes themselves: no repack
            else:
                grads[0] = gnerf_hip.planes_from_nhwc(g_planes, N).to(planes.dtype)     # contiguous NCHW, like the planes themselves
        if need_decoder:
            for i, (g, t) in enumerate(zip(g_dec, (w1, b1, w2, b2))):
                if ctx.needs_input_grad[1 + i]:
                    grads[1 + i] = g.to(t.dtype)
        return tuple(grads)


def _producer_absmax(planes):
    """max |planes| left on the producer's output by upsample2d_add_channels_last (valid while that tensor is unmodified)."""
    base = planes._base if planes._base is not None else planes
    tag = getattr(base, '_gnerf_absmax', None)
    if tag is not None and not base.is_inference() and tag[0] == base._version:
        return tag[1]
    return None


class _FusedQuery(torch.autograd.Function):
    """query_points / query_points_backward / query_points_grad as one differentiable op (run_model for arbitrary points):
    gradients for the planes, the decoder's effective weights and the points, each from its own kernel and only when asked for.
    First order only: a double backward raises (see `_once_differentiable_points`)."""

    @staticmethod
    def forward(ctx, planes, w1, b1, w2, b2, points, box_warp):
        ctx.set_materialize_grads(False)        # an output the loss does not use arrives as None: the kernels skip its half of the decoder
        nhwc = _interleaved_view(planes.detach())
        if nhwc is None:
            nhwc = gnerf_hip.planes_to_nhwc(planes.detach().float())
        sigma, rgb = gnerf_hip.query_points(nhwc, planes.shape[0], (w1, b1, w2, b2), points, box_warp)
        ctx.save_for_backward(planes, w1, b1, w2, b2, points)
        ctx.box_warp = box_warp
        return sigma, rgb

    @staticmethod
    @_once_differentiable_points
    def backward(ctx, g_sigma, g_rgb):
        grads = [None] * 7
        if g_sigma is None and g_rgb is None:
            return tuple(grads)
        planes, w1, b1, w2, b2, points = ctx.saved_tensors
        need_planes = ctx.needs_input_grad[0]
        need_decoder = any(ctx.needs_input_grad[1:5])
        N = planes.shape[0]
        nhwc = _interleaved_view(planes.detach())
        interleaved = nhwc is not None
        if not interleaved:
            nhwc = gnerf_hip.planes_to_nhwc(planes.detach().float())
        if need_planes or need_decoder:
            g_planes, g_dec = gnerf_hip.query_points_backward(nhwc, N, (w1, b1, w2, b2), points, ctx.box_warp, g_sigma, g_rgb,
                                                              need_planes=need_planes, need_decoder=need_decoder)
        if ctx.needs_input_grad[5]:
            grads[5] = gnerf_hip.query_points_grad(nhwc, N, (w1, b1, w2, b2), points, ctx.box_warp, g_sigma, g_rgb).to(points.dtype)
        if need_planes:
            grads[0] = _planes_from_interleaved(g_planes, planes) if interleaved else gnerf_hip.planes_from_nhwc(g_planes, N).to(planes.dtype)
        if need_decoder:
            for i, (g, t) in enumerate(zip(g_dec, (w1, b1, w2, b2))):
                if ctx.needs_input_grad[1 + i]:
                    grads[1 + i] = g.to(t.dtype)
        return tuple(grads)


def _affine_3x4(affine, like):
    """affine (3x4 or 4x4 [A | b], anything torch.as_tensor takes) -> (A [3,3], b [3]) in `like`'s dtype on its device, or (None, None)."""
    if affine is None:
        return None, None
    if isinstance(affine, torch.Tensor) and affine.device == like.device and affine.numel() == 12:      # already there: no host round trip
        m = affine.detach().reshape(3, 4).to(like.dtype)
        return m[:, :3], m[:, 3]
    a = torch.as_tensor(affine).detach().to(torch.float64).cpu().reshape(-1)
    if a.numel() == 16:
        a = a[:12]
    if a.numel() != 12:
        raise ValueError('project_to_level: affine must be a 3x4 or 4x4 [A | b]')
    m = a.reshape(3, 4).to(device=like.device, dtype=like.dtype)
    return m[:, :3], m[:, 3]


def project_to_level_rules(field, points, level, steps=6, radius=1.0, tol=2.0 ** -10, affine=None, early_exit=True):
    """The rules of gnerf_project_points_to_level (include/gnerf_hip.h) as tensor operations in the points' own dtype, for any field:
    field(world [..., 3]) -> (s [...], g_world [..., 3]), the field and its gradient at world = A p + b.  Per point, independently:
        p = p0
        for k = 0 .. steps:
            e = s(A p + b) - level;  k == 0: residual_in = e
            e not finite -> status 2, stop;  |e| <= tol -> status 0, stop;  k == steps -> status 1, stop
            g = A^T g_world;  gg = g.g;  gg not > 0 or not finite -> status 2, stop
            p = clamp(p - (e / gg) g, p0 - radius, p0 + radius)         (a NaN coordinate takes the box's lower face)
    -> (points_out: p where status == 0, else p0's bits; status uint8; residual_in; residual_out: e where status == 0, else residual_in).
    The float64 port the kernel's tests compare against, and ImportanceRenderer.project_to_level off the kernel's path.  early_exit False
    never reads a tensor on the host (all steps run, the same result): the form a HIP graph can capture."""
    steps = int(steps)
    if steps < 0 or not 0 <= float(radius) < float('inf') or not 0 < float(tol) < float('inf'):
        raise ValueError('project_to_level: steps >= 0, a finite radius >= 0 and a finite tol > 0 are needed')
    p0 = points.detach()
    A, b = _affine_3x4(affine, p0)
    p = p0.clone()
    lo, hi = p0 - radius, p0 + radius
    status = torch.full(p0.shape[:-1], 255, dtype=torch.uint8, device=p0.device)
    e_last = torch.zeros(p0.shape[:-1], dtype=p0.dtype, device=p0.device)
    res_in = e_last
    for k in range(steps + 1):
        active = status == 255
        if early_exit and not bool(active.any()):
            break
        world = p if A is None else p @ A.t() + b
        s, g_world = field(world)
        e = torch.where(torch.isfinite(world).all(-1), s.to(p0.dtype) - level, torch.full_like(e_last, float('nan')))
        if k == 0:
            res_in = e.clone()
        e_last = torch.where(active, e, e_last)
        status = torch.where(active & ~torch.isfinite(e), torch.full_like(status, 2), status)
        status = torch.where((status == 255) & (e.abs() <= tol), torch.zeros_like(status), status)
        if k == steps:
            status = torch.where(status == 255, torch.ones_like(status), status)
            break
        g = g_world.to(p0.dtype) if A is None else g_world.to(p0.dtype) @ A
        gg = (g * g).sum(-1)
        status = torch.where((status == 255) & ~((gg > 0) & torch.isfinite(gg)), torch.full_like(status, 2), status)
        move = status == 255
        q = p - (e / gg)[..., None] * g
        q = torch.where(torch.isnan(q), lo, q)
        p = torch.where(move[..., None], torch.minimum(torch.maximum(q, lo), hi), p)
    done = status == 0
    return torch.where(done[..., None], p, p0), status, res_in, torch.where(done, e_last, res_in)


_warned_fallbacks = set()


def _warn_gpu_fallback(reason, what='ImportanceRenderer.forward'):
    """One RuntimeWarning per (entry point, reason) and process when a call on GPU tensors runs the PyTorch-op form instead of the
    fused gfx950 kernels: correct, the reference's own arithmetic, but ~100x slower -- it must not happen unseen."""
    if (what, reason) not in _warned_fallbacks:
        _warned_fallbacks.add((what, reason))
        warnings.warn(f'{what}: GPU tensors, but {reason}: running the PyTorch-op form, not the fused HIP kernel', RuntimeWarning, stacklevel=3)


class ImportanceRenderer(torch.nn.Module):
    # run_model with points that require a gradient: True = the fused kernels (first-order gradients only: gnerf_hip.query_points_grad),
    # False = the PyTorch-op form with its warning, which autograd can differentiate twice (an eikonal term needs that)
    fused_point_grad = True
    # forward() with rays that require a gradient (camera fitting): True = the fused kernels wherever gnerf_hip.render_ray_grad_supported
    # says so (numeric ray limits, no density noise; first-order gradients only), False = the PyTorch-op form with its warning
    fused_ray_grad = False

    def __init__(self):
        super().__init__()
        self.ray_marcher = MipRayMarcher2()
        self.plane_axes = generate_planes()

    # ------------------------------------------------------------------ dispatch

    def forward(self, planes, decoder, ray_origins, ray_directions, rendering_options):
        """planes [N,3,32,H,W]; decoder(sampled_features [N,3,P,32], ray_directions) -> {'rgb','sigma'};
        rays [N,M,3]; rendering_options: the generator's rendering_kwargs dict (unknown keys ignored).
        Returns rgb [N,M,32], depth [N,M,1], weight_sum [N,M,1]."""
        self.plane_axes = self.plane_axes.to(ray_origins.device)
        # Extension (the reference requires one set of planes per item of rays): planes of ONE item with N > 1 items of rays are N
        # views of that object in one call, each with the results a call of its own would give -- its own pair of uniform draws, in
        # the order N calls would make them, and the final depth clamp (ray_marcher.py:49-50) over its own samples.
        views = planes.shape[0] == 1 and ray_origins.shape[0] > 1
        if planes.device.type == 'cuda':
            fcs = _osg_decoder_weights(decoder)
            rays_need_grad = torch.is_grad_enabled() and (ray_origins.requires_grad or ray_directions.requires_grad)
            needs_graph = torch.is_grad_enabled() and (planes.requires_grad or any(p.requires_grad for p in decoder.parameters()))
            noisy = rendering_options.get('density_noise', 0) != 0             # renderer.py:146-147: inside the kernels for forward calls (round 6)
            ray_refusal = None
            if rays_need_grad:
                ray_refusal = 'ImportanceRenderer.fused_ray_grad is False' if not self.fused_ray_grad else gnerf_hip.render_ray_grad_refusal(
                    rendering_options['depth_resolution'], rendering_options['depth_resolution_importance'], rendering_options['ray_start'],
                    rendering_options['ray_end'], density_noise=noisy)
                needs_graph = needs_graph or ray_refusal is None
            if fcs is not None and ray_refusal is None and planes.ndim == 5 and planes.shape[1] == 3 and planes.shape[2] == 32 \
                    and not (noisy and needs_graph):
                if views and needs_graph:
                    # the several-views launch is forward-only: with a graph, one differentiable call per view (same draws, same order)
                    outs = [self._forward_hip(planes, fcs, ray_origins[i:i + 1], ray_directions[i:i + 1], rendering_options, differentiable=True)
                            for i in range(ray_origins.shape[0])]
                    return tuple(torch.cat(t) for t in zip(*outs))
                return self._forward_hip(planes, fcs, ray_origins, ray_directions, rendering_options, differentiable=needs_graph)
            # A GPU call that leaves the fused kernel says so, once per reason (none of these occurs in gen_videos.py / train.py)
            _warn_gpu_fallback('the decoder is not the OSGDecoder 32->64->33 MLP' if fcs is None else
                               f'the rays need a gradient and {ray_refusal}' if ray_refusal is not None else
                               'density_noise > 0 (renderer.py:146-147) under autograd: the kernels take it for forward calls only' if noisy else
                               f'planes of shape {tuple(planes.shape)} are not [N,3,32,H,W]')
        if views:
            outs = [self._forward_torch(planes, decoder, ray_origins[i:i + 1], ray_directions[i:i + 1], rendering_options)
                    for i in range(ray_origins.shape[0])]
            return tuple(torch.cat(t) for t in zip(*outs))
        return self._forward_torch(planes, decoder, ray_origins, ray_directions, rendering_options)

    # ------------------------------------------------------------------ fused gfx950 path

    def _decoder_cache(self, fcs):
        fc1, fc2 = fcs
        params = (fc1.weight, fc1.bias, fc2.weight, fc2.bias)
        key = tuple((id(p), None if p.is_inference() else p._version, p.device) for p in params) + (float(fc1.weight_gain), float(fc1.bias_gain),
                                                                        float(fc2.weight_gain), float(fc2.bias_gain))
        cache = self.__dict__.get('_gnerf_decoder_cache')
        if cache is None or cache[0] != key or any(p.is_inference() for p in params):
            with torch.no_grad():
                eff = (fc1.weight.float() * fc1.weight_gain, fc1.bias.float() * fc1.bias_gain,        # networks_stylegan2.py:121-127
                       fc2.weight.float() * fc2.weight_gain, fc2.bias.float() * fc2.bias_gain)
                eff = tuple(t.contiguous() for t in eff)
            cache = (key, eff, params)      # keep params alive so ids stay unique
            self.__dict__['_gnerf_decoder_cache'] = cache
        return cache[1]

    def _planes_nhwc(self, planes):
        """(NHWC copy, max |planes|) of `planes`, cached on the tensor's identity and version: an orbit with cached backbone
        planes (triplane.py:66-71) converts once.  Inference tensors carry no version counter: they are converted every call.
        The cached copy is only handed to work on the stream that made it (another stream converts again, for itself)."""
        inter = _interleaved_view(planes.detach() if not planes.is_inference() else planes)
        if inter is not None:                               # already the renderer's layout (a channels_last producer): no copy
            amax = _producer_absmax(planes)
            if amax is not None or planes.is_inference():
                return inter, amax                          # (None: the launcher measures max |planes| itself)
        elif _NHWC_HINT and planes.ndim == 5 and planes.shape[1] == 3:
            from torch_utils.ops import upfirdn2d           # opt-in: ask the producer for channels_last planes from now on
            upfirdn2d.channels_last_output_shapes.add((planes.shape[1] * planes.shape[2], planes.shape[3], planes.shape[4]))
        if planes.is_inference():
            return gnerf_hip.planes_to_nhwc(planes.float(), with_absmax=True)
        base = planes._base if planes._base is not None else planes
        stream = torch.cuda.current_stream(planes.device).cuda_stream
        cache = self.__dict__.get('_gnerf_planes_cache')
        if cache is not None:
            ref, version, ptr, shape, made_on, out = cache
            if ref() is base and version == base._version and ptr == planes.data_ptr() and shape == tuple(planes.shape) \
                    and (made_on is None or made_on == stream):
                return out
        if inter is not None:
            out = (inter, gnerf_hip.planes_absmax(inter))   # measured once per planes tensor and version, like the repack
        else:
            out = gnerf_hip.planes_to_nhwc(planes.detach().float(), with_absmax=True)
        self.__dict__['_gnerf_planes_cache'] = (weakref.ref(base), base._version, planes.data_ptr(), tuple(planes.shape), stream, out)
        return out

    def pin_planes(self, planes):
        """Convert `planes` [N,3,32,H,W] now, wait for the device, and make the copy valid on EVERY stream (a HIP-graph
        capture runs on its own stream).  Returns an opaque handle that keeps the converted tensors alive: a captured
        graph bakes in their addresses, so whoever replays it must hold the handle and call `repin(handle)` before a replay
        if other planes went through this renderer in between (gen_videos_mi355x.FrameProgram does)."""
        base = planes._base if planes._base is not None else planes
        inter = _interleaved_view(planes.detach())
        if inter is not None:
            amax = _producer_absmax(planes)
            out = (inter, gnerf_hip.planes_absmax(inter) if amax is None else amax)
        else:
            out = gnerf_hip.planes_to_nhwc(planes.detach().float(), with_absmax=True)
        torch.cuda.synchronize(planes.device)
        handle = (weakref.ref(base), base._version, planes.data_ptr(), tuple(planes.shape), None, out)
        self.__dict__['_gnerf_planes_cache'] = handle
        return handle

    def repin(self, handle):
        self.__dict__['_gnerf_planes_cache'] = handle

    def _forward_hip(self, planes, fcs, ray_origins, ray_directions, opts, differentiable=False):
        N, M, _ = ray_origins.shape
        S = int(opts['depth_resolution'])
        F = int(opts['depth_resolution_importance'])
        if S > gnerf_hip.MAX_SAMPLES or F > gnerf_hip.MAX_SAMPLES:
            raise RuntimeError(f'ImportanceRenderer: at most {gnerf_hip.MAX_SAMPLES} coarse and fine samples per ray are supported')
        dev = ray_origins.device
        views = planes.shape[0] == 1 and N > 1              # N views of one item's planes (see forward)
        assert not (views and differentiable)               # forward() makes one differentiable call per view

        def limits(o, d):
            ray_start, ray_end = math_utils.get_ray_limits_box(o, d, box_side_length=opts['box_warp'])
            ok = ray_end > ray_start
            if torch.any(ok).item():                                     # renderer.py:94-96
                ray_start[~ok] = ray_start[ok].min()
                ray_end[~ok] = ray_start[ok].max()
            return ray_start, ray_end
        if opts['ray_start'] == opts['ray_end'] == 'auto':
            if views:                                                    # the fill-in values above are per call: per view here
                ray_start, ray_end = (torch.cat(t) for t in zip(*[limits(ray_origins[i:i + 1], ray_directions[i:i + 1]) for i in range(N)]))
            else:
                ray_start, ray_end = limits(ray_origins, ray_directions)
        else:
            ray_start, ray_end = opts['ray_start'], opts['ray_end']
        side = math.isqrt(M)
        if opts['clamp_mode'] != 'softplus':
            assert False, "MipRayMarcher only supports `clamp_mode`=`softplus`!"
        cfg = dict(depth_resolution=S, depth_resolution_importance=F, box_warp=opts['box_warp'],
                   white_back=bool(opts.get('white_back', False)), disparity_space_sampling=bool(opts.get('disparity_space_sampling', False)),
                   image_width=side if side * side == M else 0)
        dn = float(opts.get('density_noise', 0) or 0)
        assert not (dn and differentiable)                   # forward() sends that combination to the PyTorch-op form
        if _INKERNEL_RNG and not differentiable and not dn and gnerf_hip.render_generated_supported(S, F, ray_start, ray_end, cfg['disparity_space_sampling']) \
                and not torch.cuda.is_current_stream_capturing():
            # the same two draws (per view: the draws of a call of its own), made by the render kernel from the generator's state.  The
            # generator moves only once the launch has been accepted: a geometry the kernel does not reproduce (a device whose CU count
            # makes ATen's grid neither a power of two nor as large as the draw), an environment override of the kernel choice or planes
            # beyond 4 GB leave it where it was, and the call draws tensors below like any other.
            plan = gnerf_hip.torch_philox_plan(dev, N, M, S, F, per_item=views, advance=False)
            nhwc, amax = self._planes_nhwc(planes)
            if gnerf_hip.render_generated_supported(S, F, ray_start, ray_end, cfg['disparity_space_sampling'], plan=plan, numel_planes=nhwc.numel() // (1 if views else N)):
                try:
                    # rng= is not taken by render_forward's extension branch: this call always goes through ctypes, whose failures
                    # carry the C ABI's return code (gnerf_hip.NativeError.code)
                    out = gnerf_hip.render_forward(nhwc, N, self._decoder_cache(fcs), ray_origins.detach(), ray_directions.detach(), None, None,
                                                   ray_start=ray_start, ray_end=ray_end, planes_absmax=amax, planes_shared=views, depth_clamp_per_item=views,
                                                   rng=plan, **cfg)
                except RuntimeError as e:
                    if getattr(e, 'code', None) != gnerf_hip.E_UNSUPPORTED:      # GNERF_E_UNSUPPORTED: the tensor form below; anything else is an error
                        raise
                else:
                    gnerf_hip.commit_philox_plan(plan)
                    return out
        # the reference's two draws, same shapes, same order (renderer.py:176/186/190 then :241)
        # ... and with density_noise the two normal draws of run_model between and behind them: rand_like, randn_like (coarse), rand, randn_like (fine)
        def draw(n):
            c = torch.rand([n, M, S, 1], device=dev, dtype=torch.float32)
            sc = torch.randn([n, M * S, 1], device=dev, dtype=torch.float32) if dn else None
            f = torch.rand(n * M, F, device=dev) if F > 0 else None
            sf = torch.randn([n, M * F, 1], device=dev, dtype=torch.float32) if (dn and F > 0) else None
            return c, sc, f, sf
        if views:
            draws = [draw(1) for _ in range(N)]
            noise_c, sig_c, noise_f, sig_f = (torch.cat(t) if t[0] is not None else None for t in zip(*draws))
        else:
            noise_c, sig_c, noise_f, sig_f = draw(N)
        sigma_noise = (sig_c.reshape(N * M, S) * dn, None if sig_f is None else sig_f.reshape(N * M, F) * dn) if dn else None
        if differentiable:
            fc1, fc2 = fcs
            eff = (fc1.weight.float() * fc1.weight_gain, fc1.bias.float() * fc1.bias_gain,          # networks_stylegan2.py:121-127
                   fc2.weight.float() * fc2.weight_gain, fc2.bias.float() * fc2.bias_gain)
            # (rays arrive attached only when forward() has decided that the fused ray gradient covers the call)
            return _FusedRender.apply(planes, *eff, ray_origins, ray_directions, noise_c.reshape(N * M, S), noise_f,
                                      ray_start, ray_end, cfg)
        nhwc, amax = self._planes_nhwc(planes)
        return gnerf_hip.render_forward(nhwc, N, self._decoder_cache(fcs), ray_origins.detach(), ray_directions.detach(),
                                        noise_c, noise_f, ray_start=ray_start, ray_end=ray_end, planes_absmax=amax,
                                        planes_shared=views, depth_clamp_per_item=views, sigma_noise=sigma_noise, **cfg)

    # ------------------------------------------------------------------ PyTorch-op path

    def _forward_torch(self, planes, decoder, ray_origins, ray_directions, rendering_options):
        if rendering_options['ray_start'] == rendering_options['ray_end'] == 'auto':
            ray_start, ray_end = math_utils.get_ray_limits_box(ray_origins, ray_directions, box_side_length=rendering_options['box_warp'])
            ok = ray_end > ray_start
            if torch.any(ok).item():
                ray_start[~ok] = ray_start[ok].min()
                ray_end[~ok] = ray_start[ok].max()
        else:
            ray_start, ray_end = rendering_options['ray_start'], rendering_options['ray_end']
        depths_coarse = self.sample_stratified(ray_origins, ray_start, ray_end, rendering_options['depth_resolution'],
                                               rendering_options['disparity_space_sampling'])
        N, M, S, _ = depths_coarse.shape

        def shade(depths):
            count = depths.shape[2]
            pts = (ray_origins.unsqueeze(-2) + depths * ray_directions.unsqueeze(-2)).reshape(N, -1, 3)
            dirs = ray_directions.unsqueeze(-2).expand(-1, -1, count, -1).reshape(N, -1, 3)
            # (forward() has said why already; the rays' gradient reaches these points, and this route stays PyTorch ops throughout,
            #  as it always was: they do not go to the fused query)
            out = self._run_model(planes, decoder, pts, dirs, rendering_options, warn=False, fused_points=False)
            return out['rgb'].reshape(N, M, count, out['rgb'].shape[-1]), out['sigma'].reshape(N, M, count, 1)

        colors_coarse, densities_coarse = shade(depths_coarse)
        n_fine = rendering_options['depth_resolution_importance']
        if n_fine > 0:
            _, _, weights = self.ray_marcher(colors_coarse, densities_coarse, depths_coarse, rendering_options)
            depths_fine = self.sample_importance(depths_coarse, weights, n_fine)
            colors_fine, densities_fine = shade(depths_fine)
            all_depths, all_colors, all_densities = self.unify_samples(depths_coarse, colors_coarse, densities_coarse,
                                                                       depths_fine, colors_fine, densities_fine)
            rgb_final, depth_final, weights = self.ray_marcher(all_colors, all_densities, all_depths, rendering_options)
        else:
            rgb_final, depth_final, weights = self.ray_marcher(colors_coarse, densities_coarse, depths_coarse, rendering_options)
        return rgb_final, depth_final, weights.sum(2)

    def run_model(self, planes, decoder, sample_coordinates, sample_directions, options):
        """Decoder outputs at arbitrary points [N,P,3] -> {'rgb' [N,P,32], 'sigma' [N,P,1]}
        (entry point of TriPlaneGenerator.sample / sample_mixed, triplane.py:91-102)."""
        return self._run_model(planes, decoder, sample_coordinates, sample_directions, options)

    def _run_model(self, planes, decoder, sample_coordinates, sample_directions, options, warn=True, fused_points=None):
        fused_points = self.fused_point_grad if fused_points is None else fused_points
        self.plane_axes = self.plane_axes.to(sample_coordinates.device)
        density_noise = options.get('density_noise', 0)
        if planes.device.type == 'cuda' and planes.ndim == 5 and planes.shape[1] == 3 and planes.shape[2] == 32:
            fcs = _osg_decoder_weights(decoder)
            points_need_grad = torch.is_grad_enabled() and sample_coordinates.requires_grad
            if fcs is not None and (not points_need_grad or fused_points):
                needs_graph = points_need_grad or (torch.is_grad_enabled() and (planes.requires_grad or any(p.requires_grad for p in decoder.parameters())))
                if needs_graph:
                    fc1, fc2 = fcs
                    eff = (fc1.weight.float() * fc1.weight_gain, fc1.bias.float() * fc1.bias_gain,      # networks_stylegan2.py:121-127
                           fc2.weight.float() * fc2.weight_gain, fc2.bias.float() * fc2.bias_gain)
                    sigma, rgb = _FusedQuery.apply(planes, *eff, sample_coordinates if points_need_grad else sample_coordinates.detach(), options['box_warp'])
                else:
                    sigma, rgb = gnerf_hip.query_points(self._planes_nhwc(planes)[0], planes.shape[0], self._decoder_cache(fcs),
                                                        sample_coordinates.detach(), options['box_warp'])
                out = {'rgb': rgb, 'sigma': sigma}
                if density_noise > 0:
                    out['sigma'] = out['sigma'] + torch.randn_like(out['sigma']) * density_noise
                return out
        if warn and planes.device.type == 'cuda':
            _warn_gpu_fallback('the points need a gradient and fused_point_grad is False, the decoder is not the OSGDecoder MLP or the planes are not [N,3,32,H,W]',
                               'ImportanceRenderer.run_model')
        feats = sample_from_planes(self.plane_axes, planes, sample_coordinates, padding_mode='zeros', box_warp=options['box_warp'])
        out = decoder(feats, sample_directions)
        if density_noise > 0:
            out['sigma'] += torch.randn_like(out['sigma']) * density_noise
        return out

    def query_sigma(self, planes, decoder, sample_coordinates, options):
        """Densities [N,P,1] only -- run_model(...)['sigma'] without evaluating or writing the 32 colour channels (not part of the
        reference's interface: used by this repo's shape-extraction harness, where rgb would be 17 GB of unread output at 512^3)."""
        if planes.device.type == 'cuda' and planes.ndim == 5 and planes.shape[1] == 3 and planes.shape[2] == 32 and not torch.is_grad_enabled():
            fcs = _osg_decoder_weights(decoder)
            if fcs is not None and options.get('density_noise', 0) == 0:
                return gnerf_hip.query_points(self._planes_nhwc(planes)[0], planes.shape[0], self._decoder_cache(fcs),
                                              sample_coordinates.detach(), options['box_warp'], want_rgb=False)[0]
        dirs = torch.zeros_like(sample_coordinates)
        dirs[..., -1] = -1
        return self.run_model(planes, decoder, sample_coordinates, dirs, options)['sigma']

    def query_sigma_lattice(self, planes, decoder, index, n, options, out, cube_length=None):
        """Densities at points of gen_videos.py's n^3 sample lattice named by their linear indices: out[index] = query_sigma at
        voxel_samples' positions of those indices (cube_length: the lattice's, options['box_warp'] by default), written into the flat float32
        `out` [n^3] in place; the other entries are left alone.  On CUDA tensors, under query_sigma's conditions, one kernel forms the
        positions itself and stores straight into `out` (gnerf_hip.query_lattice: the same bits); otherwise voxel_samples at those indices,
        query_sigma and an indexed store.  Not part of the reference's interface: extract_density_grid's narrow band evaluates through it."""
        cube_length = options['box_warp'] if cube_length is None else cube_length
        if len(index) == 0:
            return out
        if (planes.device.type == 'cuda' and planes.ndim == 5 and planes.shape[0] == 1 and planes.shape[1] == 3 and planes.shape[2] == 32
                and not torch.is_grad_enabled() and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n ** 3):
            fcs = _osg_decoder_weights(decoder)
            if fcs is not None and options.get('density_noise', 0) == 0:
                return gnerf_hip.query_lattice(self._planes_nhwc(planes)[0], self._decoder_cache(fcs), index, n, cube_length, options['box_warp'], out)
        from gnerf_lattice import voxel_samples
        index = torch.as_tensor(index).to(out.device).long()
        out.view(-1)[index] = self.query_sigma(planes, decoder, voxel_samples(index, None, n, cube_length, out.device), options).reshape(-1).to(out.dtype)
        return out

    def query_normals(self, planes, decoder, sample_coordinates, options):
        """(sigma [N,P,1], normals [N,P,3]) at arbitrary points: normals = -grad sigma / |grad sigma|, outward for a surface whose inside
        is sigma > level (the mesh's convention); a point where the gradient is zero gets the exact zero vector.  density_noise is not
        applied.  On a GPU one densities-only query and one gnerf_hip.query_points_grad (grad_sigma = ones, no colour half); on CPU
        tensors (or a decoder the kernels do not take) autograd through the PyTorch-op form.  Not part of the reference's interface."""
        fcs = _osg_decoder_weights(decoder) if planes.device.type == 'cuda' else None
        if fcs is not None and planes.ndim == 5 and planes.shape[1] == 3 and planes.shape[2] == 32:
            nhwc, dec, pts = self._planes_nhwc(planes)[0], self._decoder_cache(fcs), sample_coordinates.detach()
            sigma = gnerf_hip.query_points(nhwc, planes.shape[0], dec, pts, options['box_warp'], want_rgb=False)[0]
            grad = gnerf_hip.query_points_grad(nhwc, planes.shape[0], dec, pts, options['box_warp'], torch.ones_like(sigma), None)
        else:
            with torch.enable_grad():
                pts = sample_coordinates.detach().requires_grad_(True)
                sigma = self._run_model(planes.detach(), decoder, pts, torch.zeros_like(pts), dict(options, density_noise=0))['sigma']
                grad, = torch.autograd.grad(sigma.sum(), pts)
            sigma = sigma.detach()
        length = grad.norm(dim=-1, keepdim=True)
        return sigma, torch.where(length > 0, -grad / length, torch.zeros_like(grad))

    def project_to_level(self, planes, decoder, points, level, options, affine=None, steps=6, radius=1.0, tol=None):
        """Newton projection of points [N,P,3] onto the density's level set sigma = level -> (points_out [N,P,3], status uint8 [N,P]: 0
        converged / 1 not converged / 2 flat or not finite, residual_in [N,P], residual_out [N,P]: sigma - level before and after).  At most
        `steps` steps, never more than `radius` per axis from the start (in the points' frame), done when |sigma - level| <= tol (None:
        2^-10 max(1, |level|)); a point that does not converge keeps its input's bits.  affine: a 3x4 (or 4x4) [A | b], world = A p + b,
        for points in another frame (a mesh in its index frame).  On a GPU with the OSG decoder and [N,3,32,H,W] planes one launch of
        gnerf_hip.project_points_to_level; otherwise (CPU tensors, float64, another decoder) project_to_level_rules on autograd through
        the PyTorch-op form, as query_normals falls back.  density_noise is not applied.  Not part of the reference's interface."""
        tol = 2.0 ** -10 * max(1.0, abs(float(level))) if tol is None else float(tol)
        fcs = _osg_decoder_weights(decoder) if planes.device.type == 'cuda' else None
        if fcs is not None and planes.ndim == 5 and planes.shape[1] == 3 and planes.shape[2] == 32 and points.dtype != torch.float64:
            return gnerf_hip.project_points_to_level(self._planes_nhwc(planes)[0], planes.shape[0], self._decoder_cache(fcs), points.detach(),
                                                     options['box_warp'], level, affine=affine, steps=steps, radius=radius, tol=tol)
        opts = dict(options, density_noise=0)

        def field(world):
            with torch.enable_grad():
                pts = world.detach().to(planes.dtype).requires_grad_(True)         # the field in the planes' dtype, the rules in the points'
                sigma = self._run_model(planes.detach(), decoder, pts, torch.zeros_like(pts), opts, fused_points=False)['sigma']      # (GPU tensors here: the fallback warning)
                grad, = torch.autograd.grad(sigma.sum(), pts)
            return sigma.detach()[..., 0], grad

        return project_to_level_rules(field, points.detach(), level, steps=steps, radius=radius, tol=tol, affine=affine)

    def sort_samples(self, all_depths, all_colors, all_densities):
        _, order = torch.sort(all_depths, dim=-2)
        all_depths = torch.gather(all_depths, -2, order)
        all_colors = torch.gather(all_colors, -2, order.expand(-1, -1, -1, all_colors.shape[-1]))
        all_densities = torch.gather(all_densities, -2, order.expand(-1, -1, -1, 1))
        return all_depths, all_colors, all_densities

    def unify_samples(self, depths1, colors1, densities1, depths2, colors2, densities2):
        return self.sort_samples(torch.cat([depths1, depths2], dim=-2), torch.cat([colors1, colors2], dim=-2),
                                 torch.cat([densities1, densities2], dim=-2))

    def sample_stratified(self, ray_origins, ray_start, ray_end, depth_resolution, disparity_space_sampling=False):
        """Jittered, roughly uniform depths [N,M,S,1] along each ray."""
        N, M, _ = ray_origins.shape
        dev = ray_origins.device
        if disparity_space_sampling:
            d = torch.linspace(0, 1, depth_resolution, device=dev).reshape(1, 1, depth_resolution, 1).repeat(N, M, 1, 1)
            d += torch.rand_like(d) * (1 / (depth_resolution - 1))
            return 1. / (1. / ray_start * (1. - d) + 1. / ray_end * d)
        if type(ray_start) == torch.Tensor:
            depths = math_utils.linspace(ray_start, ray_end, depth_resolution).permute(1, 2, 0, 3)
            step = (ray_end - ray_start) / (depth_resolution - 1)
            depths += torch.rand_like(depths) * step[..., None]
            return depths
        depths = torch.linspace(ray_start, ray_end, depth_resolution, device=dev).reshape(1, 1, depth_resolution, 1).repeat(N, M, 1, 1)
        depths += torch.rand_like(depths) * ((ray_end - ray_start) / (depth_resolution - 1))
        return depths

    def sample_importance(self, z_vals, weights, N_importance):
        """Depths [N,M,F,1] drawn from the smoothed coarse weights (NeRF-style hierarchical sampling)."""
        with torch.no_grad():
            N, M, S, _ = z_vals.shape
            z = z_vals.reshape(N * M, S)
            w = weights.reshape(N * M, -1)          # S-1 interval weights
            w = torch.nn.functional.max_pool1d(w.unsqueeze(1).float(), 2, 1, padding=1)
            w = torch.nn.functional.avg_pool1d(w, 2, 1).squeeze() + 0.01
            mids = 0.5 * (z[:, :-1] + z[:, 1:])
            fine = self.sample_pdf(mids, w[:, 1:-1], N_importance).detach()
        return fine.reshape(N, M, N_importance, 1)

    def sample_pdf(self, bins, weights, N_importance, det=False, eps=1e-5):
        """Inverse-transform sampling: bins [R,K+1], weights [R,K] -> samples [R,N_importance]."""
        R, K = weights.shape
        weights = weights + eps
        pdf = weights / torch.sum(weights, -1, keepdim=True)
        cdf = torch.cumsum(pdf, -1)
        cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)
        if det:
            u = torch.linspace(0, 1, N_importance, device=bins.device).expand(R, N_importance)
        else:
            u = torch.rand(R, N_importance, device=bins.device)
        u = u.contiguous()
        idx = torch.searchsorted(cdf, u, right=True)
        lo = torch.clamp_min(idx - 1, 0)
        hi = torch.clamp_max(idx, K)
        pair = torch.stack([lo, hi], -1).view(R, 2 * N_importance)
        cdf_g = torch.gather(cdf, 1, pair).view(R, N_importance, 2)
        bins_g = torch.gather(bins, 1, pair).view(R, N_importance, 2)
        denom = cdf_g[..., 1] - cdf_g[..., 0]
        denom[denom < eps] = 1          # empty bin: never drawn, any value works
        return bins_g[..., 0] + (u - cdf_g[..., 0]) / denom * (bins_g[..., 1] - bins_g[..., 0])
