#!/usr/bin/env python3
"""Counterpart of G-NeRF's gen_videos.py for MI355X (BASELINE configs 1, 3, 4).

What it keeps from the reference (g_nerf/gen_videos.py:83-224): network pickle loading through the reference's own
`legacy`/`dnnlib`, the orbit cameras and intrinsics, `ws = G.mapping(z, c=0)` once, the x2 rule on the checkpoint's
depth resolutions, `G.synthesis(ws, c, noise_mode='const', neural_rendering_resolution=res)` per frame, the uint8
conversion.  What it changes: no cv2/imageio/mrcfile (frames are returned / saved as a uint8 array), `torch.no_grad()`,
the StyleGAN2 backbone runs ONCE per orbit (`cache_backbone` / `use_cached_backbone`, triplane.py:66-71; `ws` is constant),
the device is whatever `--device` says, and frames are sharded over ranks -- one process per GPU under
`torch.distributed.run`, a contiguous block of frames each, one gather of uint8 frames at the end.

Run with this repo's g-nerf_amd/ in front of the reference's g_nerf/ on PYTHONPATH:

    PYTHONPATH=.../g-nerf_amd:.../G-NeRF/g_nerf python g-nerf_amd/gen_videos_mi355x.py --network G.pkl --encoder E.pkl --id-image face.png
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 g-nerf_amd/gen_videos_mi355x.py --random-init --frames 240 ...

`--random-init` builds the FFHQ-config TriPlaneGenerator with seeded random weights and a random z instead of loading
pickles (there are no checkpoints or network access in the build environment); where the reference tree is absent it is
this repo's inference-only equivalent (gnerf_generator.Generator).  `--graph` replays the per-frame launch sequence from a
HIP graph captured once (FrameProgram); `--shapes out.npy` also extracts the 512^3 density volume of gen_videos.py --shapes,
`--shapes-mrc out.mrc` writes it as the reference's .mrc, and `--mesh out.ply` meshes it (shape_utils.py's step, shape_mi355x) while it
is still on the device; `--mesh-attrs normals|colors|all` adds the density field's normals and the decoder's colours per vertex.
`--geometry-out geo.npy` draws that mesh from every orbit camera with the triangle rasteriser (csrc/raster.hip): shaded geometry frames on
the renderer's pixel grid, uint8 [F, H, W, 3] at `--geometry-res`, smooth-shaded / coloured with `--mesh-attrs`.
`--mesh-band S` (2, 4, 8 or 16; 0: off) evaluates the volume of both only in a narrow band of bricks of S^3 cells that follows the level set of
`--mesh-level` (csrc/mesh_band.hip, csrc/query_lattice.inl): the same mesh in the same order, minus detached components thinner than a brick.
`--mesh-direct` (with `--mesh-band S`) meshes that band brick by brick, on the lattice as the queries left it (csrc/mesh_band_cubes.hip): no fill,
no flip / crop / transpose copies, the same mesh byte for byte.
`--mesh-keep K`, `--mesh-min-faces N` and `--mesh-smooth ITERS` clean the mesh of both first (csrc/mesh_clean.hip): only the K largest connected
components / those with at least N triangles stay, then ITERS Taubin iterations fair the surface; all 0 by default, which changes nothing.
`--mesh-simplify CELL` (voxels) and `--mesh-target-faces N` simplify it in between (csrc/mesh_simplify.hip): one vertex per occupied cell of a
uniform grid, placed by the cell's quadric; both 0 by default, which changes nothing.
`--mesh-snap R` (voxels; `--mesh-snap-steps`, `--mesh-snap-tol`) comes last, after the smoothing: every vertex goes onto the level set of the
density itself by Newton steps along its gradient, at most R voxels per axis from where it stood (csrc/project_level.inl), faces that this
turns over get their vertices back (the flip guard of csrc/mesh_clean.hip), and the attributes are evaluated at the final positions; 0 by
default, which changes nothing.
`--mesh-bake N` (with `--mesh`) colours the final mesh from N of the orbit's own 512^2 frames, evenly spaced (no extra synthesis): the mesh is
rasterised from their cameras at `--mesh-bake-res`, every vertex takes the frames' colours where the visibility buffers say it is seen
(csrc/raster.hip, gnerf_mesh_bake_colors; `--mesh-bake-tol`, `--mesh-bake-guard`, `--mesh-bake-power`), blended by how squarely each view faces
the surface when `--mesh-attrs` made normals; the decoder's colours, when it made them, stay on the vertices no frame sees.
`--mesh-texture P --mesh-texture-out PATH.obj` (with `--mesh-bake N`) also bakes those N frames into a texture atlas of the final mesh, two
triangles to a cell of P x P texels (gnerf_mesh_bake_texture: the vertex bake's rules per texel), and writes the mesh with its UVs as PATH.obj,
its .mtl and its .png; the .ply of `--mesh` is the same file as without it.
"""

import argparse
import collections
import sys
import time

import numpy as np
import torch

import gnerf_harness as H
import shape_mi355x
from gnerf_lattice import voxel_samples  # noqa: F401  (gv.voxel_samples stays)


def ffhq_generator_kwargs(depth_resolution=48, depth_resolution_importance=48):
    """G_kwargs of the FFHQ configuration, as train.py:238-377 assembles them from its option defaults."""
    rendering = {
        'image_resolution': 512, 'disparity_space_sampling': False, 'clamp_mode': 'softplus',
        'superresolution_module': 'training.superresolution.SuperresolutionHybrid8XDC',
        'c_gen_conditioning_zero': False, 'gpc_reg_prob': 0.5, 'c_scale': 1, 'superresolution_noise_mode': 'none',
        'density_reg': 0.25, 'density_reg_p_dist': 0.004, 'reg_type': 'l1', 'decoder_lr_mul': 1, 'sr_antialias': True,
        'depth_resolution': depth_resolution, 'depth_resolution_importance': depth_resolution_importance,
        'ray_start': 2.25, 'ray_end': 3.3, 'box_warp': 1, 'avg_camera_radius': 2.7, 'avg_camera_pivot': [0, 0, 0.2],
    }
    return dict(z_dim=512, w_dim=512, c_dim=25, img_resolution=512, img_channels=3,
                mapping_kwargs=dict(num_layers=2), channel_base=32768, channel_max=512, fused_modconv_default='inference_only',
                rendering_kwargs=rendering, num_fp16_res=0, conv_clamp=None, sr_num_fp16_res=4,
                sr_kwargs=dict(channel_base=32768, channel_max=512, fused_modconv_default='inference_only', w_dim=512))


def build_random_generator(seed, device, **kw):
    """Seeded random-init FFHQ-config generator: the reference's TriPlaneGenerator when its tree is importable (its renderer
    and ops then resolve to this repo through the overlay), else this repo's inference-only equivalent with the same layer
    graph and parameter names (gnerf_generator.Generator; the GPU box has no reference tree)."""
    torch.manual_seed(seed)
    try:
        from training.triplane import TriPlaneGenerator
        G = TriPlaneGenerator(**ffhq_generator_kwargs(**kw))
    except ImportError:
        import gnerf_generator
        G = gnerf_generator.Generator(rendering_kwargs=ffhq_generator_kwargs(**kw)['rendering_kwargs'])
    return G.eval().requires_grad_(False).to(device)


def load_generator(network_pkl, device):
    import dnnlib
    import legacy
    with dnnlib.util.open_url(network_pkl) as f:
        return legacy.load_network_pkl(f)['G_ema'].to(device).eval().requires_grad_(False)


def identity_latent(args, device, z_dim):
    if args.encoder and args.id_image:
        import dnnlib
        import legacy
        from PIL import Image
        with dnnlib.util.open_url(args.encoder) as f:
            E = legacy.load_network_pkl(f)['E'].to(device).eval()
        img = np.asarray(Image.open(args.id_image).convert('RGB')).transpose(2, 0, 1)[None]
        return E(torch.from_numpy(img.copy()).to(device) / 127.5 - 1)                       # gen_videos.py:119,131
    return torch.randn(1, z_dim, generator=torch.Generator().manual_seed(args.seed + 1)).to(device)


def orbit_latents(G, z, device):
    """ws of the whole orbit: the mapping network runs once, on a zero camera label (gen_videos.py:147-150)."""
    c0 = H.camera_label(H.lookat_pose(3.14 / 2, 3.14 / 2, G.rendering_kwargs['avg_camera_radius'], device))
    return G.mapping(z=z, c=torch.zeros_like(c0).repeat(z.shape[0], 1))


class FrameProgram:
    """One orbit frame -- rays, the two uniform draws, the fused render, superresolution, uint8 conversion, ~190 launches --
    captured ONCE into a HIP graph and replayed per camera.  No entry point of the native library allocates or synchronises,
    and torch's graph-safe generator advances the draws from replay to replay.  The backbone runs once, before the capture
    (ws is constant over the orbit).  Reusable across orbits of the same generator, latent and resolution.

    The graph bakes in the ADDRESSES of everything the captured frame read: the cached backbone planes, the renderer's NHWC
    copy of them and its folded decoder weights.  The program therefore owns strong references to all three and puts them
    back in place before every replay -- an eager frame with cache_backbone=True in between would otherwise replace (and
    free) them and the replay would read recycled memory."""

    @torch.no_grad()
    def __init__(self, G, ws, res, device, batch=1):
        self.G, self.ws, self.res = G, ws, res
        self.c = H.camera_label(H.orbit_pose(0, 120, G.rendering_kwargs['avg_camera_radius'], device=device)).repeat(batch, 1)
        self._frame(cache=True, cached=False)
        self.planes = G._last_planes
        self._pin = None
        if hasattr(G.renderer, 'pin_planes'):
            p = self.planes
            self._pin = G.renderer.pin_planes(p.view(len(p), 3, 32, p.shape[-2], p.shape[-1]))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._frame()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.frame, self.raw = self._frame()
        self._decoder = G.renderer.__dict__.get('_gnerf_decoder_cache')
        # ... and the per-latent constants of the layers (styles, modulated weights: gnerf_generator._per_latent), which the captured
        # kernels read in place; another latent through the same generator replaces the cache entries, not these tensors
        self._latent_constants = getattr(sys.modules.get(type(G).__module__), 'latent_cache_tensors', lambda g: [])(G)

    def _frame(self, cache=False, cached=True):
        out = self.G.synthesis(ws=self.ws, c=self.c, noise_mode='const', neural_rendering_resolution=self.res,
                               cache_backbone=cache, use_cached_backbone=cached)
        return H.to_uint8(out['image']), H.to_uint8(out['image_raw'])

    def __call__(self, c):
        self.c.copy_(c)
        self.G._last_planes = self.planes                         # what an eager use_cached_backbone frame after this one reads, too
        if self._pin is not None:
            self.G.renderer.repin(self._pin)
        self.graph.replay()
        return self.frame.clone(), self.raw.clone()


@torch.no_grad()
def render_orbit(G, z, n_frames, res, device, rank=0, world=1, double_depth=True, frame_seed=None, use_graph=False, program=None,
                 frames_per_call=1):
    """This rank's frames of the orbit: (uint8 [n_local,512,512,3], uint8 raw [n_local,res,res,3], (lo, hi)).
    use_graph (GPU only): frames come from a FrameProgram (`program`, or one captured here).
    frames_per_call > 1 (one latent only): that many cameras go through the renderer and the superresolution as one batch; the
    renderer treats them as views of the one set of planes, each with the draws and the depth clamp of a call of its own."""
    if double_depth:                                                                        # gen_videos.py:127-128
        G.rendering_kwargs['depth_resolution'] = int(G.rendering_kwargs['depth_resolution'] * 2)
        G.rendering_kwargs['depth_resolution_importance'] = int(G.rendering_kwargs['depth_resolution_importance'] * 2)
    radius = G.rendering_kwargs['avg_camera_radius']
    lo, hi = H.shard_range(n_frames, rank, world)
    if hi == lo:
        return None, None, (lo, hi)
    k = max(int(frames_per_call), 1)
    if k > 1 and (z.shape[0] != 1 or frame_seed is not None):
        raise ValueError('frames_per_call > 1 needs a single latent and no per-frame reseeding')
    # every camera of this rank's block made on the host in one set of batched ops (per frame: ~0.15 ms of small tensor ops each) and
    # moved in ONE copy (per frame: a pose and an intrinsics upload, two blocking host-to-device copies in front of every frame's launches)
    labels = H.orbit_labels(range(lo, hi), n_frames, radius).to(device)
    if k > 1:
        cams = [labels[j:j + k] for j in range(0, hi - lo, k)]
    else:
        cams = [labels[j:j + 1].repeat(z.shape[0], 1) if z.shape[0] > 1 else labels[j:j + 1] for j in range(hi - lo)]
    frames, raws = [], []
    if (use_graph or program is not None) and device.type == 'cuda':
        assert frame_seed is None, 'per-frame reseeding and graph replay do not mix'
        if program is None:
            program = FrameProgram(G, orbit_latents(G, z, device), res, device, batch=z.shape[0] if k == 1 else k)
        for c in cams:
            n = c.shape[0]
            if n < program.c.shape[0]:                                                      # the last, shorter block of an orbit
                c = torch.cat([c, c[-1:].expand(program.c.shape[0] - n, -1)])
            f, r = program(c)
            frames.append(f[:n])
            raws.append(r[:n])
    else:
        ws = orbit_latents(G, z, device)
        for j, c in enumerate(cams):
            if frame_seed is not None:
                torch.manual_seed(frame_seed + lo + j)                                      # reproducible renderer draws per frame
            n = c.shape[0]
            if k > 1 and n < k:
                # the last, shorter block of an orbit keeps the batch size of the others (repeat its last camera, drop the extra frames):
                # a new batch size is a new set of convolution shapes -- a MIOpen solver search in the middle of the orbit
                c = torch.cat([c, c[-1:].expand(k - n, -1)])
            out = G.synthesis(ws=ws, c=c, noise_mode='const', neural_rendering_resolution=res, cache_backbone=(j == 0), use_cached_backbone=(j > 0))
            frames.append(H.to_uint8(out['image'][:n]))
            raws.append(H.to_uint8(out['image_raw'][:n]))
    return torch.cat(frames), torch.cat(raws), (lo, hi)


def _stack3(a, b, c):
    return torch.stack([a, b, c], dim=-1) if isinstance(a, torch.Tensor) else np.stack([a, b, c], axis=-1)


def lattice_to_world(index_coords, resolution, cube_length):
    """The continuous extension of voxel_samples: lattice coordinates (s0, s1, s2) [..., 3] (a torch tensor or a numpy array; integers
    are the lattice points, point s0 n^2 + s1 n + s2 of create_samples) -> world positions.  The reference's lattice is sheared --
    its first two indices are float divisions of the linear index without a floor --, so the point is
    ((s0 + s1/n + s2/n^2), (s1 + s2/n), s2) * size + origin with size = cube_length / (n - 1), origin = -cube_length / 2."""
    n = resolution
    origin, size = -cube_length / 2, cube_length / (n - 1)
    s0, s1, s2 = index_coords[..., 0], index_coords[..., 1], index_coords[..., 2]
    return _stack3((s0 + s1 / n + s2 / (n * n)) * size + origin, (s1 + s2 / n) * size + origin, s2 * size + origin)


def mesh_to_lattice(verts, resolution):
    """Mesh vertices (index space of vol.permute(2, 1, 0), vol = sigmas.reshape(r, r, r).flip(0): what mesh_density_grid meshes)
    -> lattice coordinates (s0, s1, s2) of lattice_to_world: the permute swaps the outer axes, the flip mirrors the first."""
    return _stack3((resolution - 1) - verts[..., 2], verts[..., 1], verts[..., 0])


def mesh_to_world_jacobian(resolution, cube_length):
    """J = d world / d mesh-index of lattice_to_world(mesh_to_lattice(v)): a constant 3x3 (float64 numpy), rows = world axes."""
    n, size = resolution, cube_length / (resolution - 1)
    return size * np.array([[1 / (n * n), 1 / n, -1.0], [1 / n, 1.0, 0.0], [1.0, 0.0, 0.0]])


def mesh_to_world_matrix(resolution, cube_length):
    """The affine map lattice_to_world(mesh_to_lattice(v)) of a mesh vertex v (index space) as a 3x4 [J | b] (float64 numpy): J is
    mesh_to_world_jacobian, b the world position of v = 0 (lattice point (n - 1, 0, 0))."""
    half = cube_length / 2
    return np.concatenate([mesh_to_world_jacobian(resolution, cube_length), np.array([[half], [-half], [-half]])], axis=1)


def normals_to_mesh_frame(normals_world, resolution, cube_length):
    """World-space normals [..., 3] -> the mesh's index frame, in which the .ply's vertices stay: a normal is a covector (the gradient
    of a scalar field), so it transforms with the transpose, normalise(J^T n); zero vectors stay zero."""
    J = mesh_to_world_jacobian(resolution, cube_length)
    if isinstance(normals_world, torch.Tensor):
        m = normals_world @ torch.as_tensor(J, dtype=normals_world.dtype, device=normals_world.device)        # rows: (J^T n)^T = n^T J
        length = m.norm(dim=-1, keepdim=True)
        return torch.where(length > 0, m / length, torch.zeros_like(m))
    m = np.asarray(normals_world) @ J.astype(np.asarray(normals_world).dtype)
    length = np.linalg.norm(m, axis=-1, keepdims=True)
    return np.where(length > 0, m / np.where(length > 0, length, 1), 0).astype(m.dtype)


def crop_ranges(resolution):
    """extract_density_grid's crop (gen_videos.py:213-220) as (zeroed at the front, zeroed at the back) per axis of the flipped volume."""
    pad, pad_top = int(30 * resolution / 256), int(38 * resolution / 256)
    return [(pad, pad), (pad, pad_top), (pad, pad)]


@torch.no_grad()
def _dense_density(G, planes, resolution, max_batch):
    """extract_density_grid's sigmas [resolution^3]: every lattice point, chunk by chunk."""
    device = planes.device
    total = resolution ** 3
    sigmas = torch.empty(total, dtype=torch.float32, device=device)
    for head in range(0, total, max_batch):
        hi = min(total, head + max_batch)
        pts = voxel_samples(head, hi, resolution, G.rendering_kwargs['box_warp'], device)
        if hasattr(G.renderer, 'query_sigma'):                                              # this repo's renderer: densities only
            sigmas[head:hi] = G.renderer.query_sigma(planes, G.decoder, pts, G.rendering_kwargs).reshape(-1)
        else:
            dirs = torch.zeros_like(pts)
            dirs[..., -1] = -1
            sigmas[head:hi] = G.renderer.run_model(planes, G.decoder, pts, dirs, G.rendering_kwargs)['sigma'].reshape(-1)
    return sigmas


def _band_field(G, planes, resolution, crop):
    """What the narrow band is given for extract_density_grid's lattice -> (field(index, out), keep).  The crop is handed over as the kept
    index range per axis of the UNFLIPPED lattice: flip(0) mirrors axis 0, so its front and back exchange."""
    keep = None
    if crop:
        (a0, b0), r1, r2 = crop_ranges(resolution)
        keep = shape_mi355x.band_keep_of_crop(resolution, [(b0, a0), r1, r2])
    kw = G.rendering_kwargs

    def field(index, out):
        out = out if isinstance(out, torch.Tensor) else torch.from_numpy(out)           # (the numpy port's array: shares its memory)
        G.renderer.query_sigma_lattice(planes, G.decoder, torch.as_tensor(index), resolution, kw, out)

    return field, keep


@torch.no_grad()
def _band_density(G, planes, resolution, crop, band, level):
    """extract_density_grid's sigmas [resolution^3] through shape_mi355x.band_volume: densities where the level set runs, the coarse corners'
    values elsewhere -> (sigmas, report)."""
    if level is None:
        raise ValueError('extract_density_grid: band needs the isosurface level the volume will be meshed at')
    field, keep = _band_field(G, planes, resolution, crop)
    vol, report = shape_mi355x.band_volume(field, resolution, level, band, keep, device=planes.device)
    return torch.as_tensor(vol).reshape(-1).to(planes.device), report


@torch.no_grad()
def extract_density_grid(G, ws, resolution=512, max_batch=10000000, crop=True, planes=None, return_planes=False, band=None, level=None, report=None):
    """The density volume gen_videos.py --shapes writes to .mrc (gen_videos.py:189-224): sigma at resolution^3 lattice points of
    the box, flipped along the first axis, borders zeroed.  The reference calls G.sample_mixed per chunk of 10^7 points, which
    re-runs the StyleGAN2 backbone for every chunk (14 passes at 512^3); here the planes are made once and every chunk goes
    through ImportanceRenderer.run_model (the fused point-query kernel on a GPU).  Returns a float32 tensor [r, r, r] on ws' device.
    planes / return_planes: take the tri-planes [N,3,32,H,W] instead of running the backbone, and hand them back as (vol, planes) --
    mesh_density_grid evaluates vertex attributes on the same planes.
    band=s (2, 4, 8 or 16; None: off) evaluates only a narrow band of bricks of s^3 cells around the level set sigma = `level`
    (shape_mi355x.band_volume with ImportanceRenderer.query_sigma_lattice as the field; needs this repo's renderer): the mesh of the
    volume at that level is the dense volume's, minus whole components thinner than a brick that the band never met, but the other
    values of the volume are NOT densities.  report: a dict that receives the band's report under 'band'."""
    device = ws.device
    if planes is None:
        planes = G.backbone.synthesis(ws, noise_mode='const')
        planes = planes.view(len(planes), 3, 32, planes.shape[-2], planes.shape[-1])
    if band:
        sigmas, band_report = _band_density(G, planes, resolution, crop, band, level)
        if report is not None:
            report['band'] = band_report
    else:
        sigmas = _dense_density(G, planes, resolution, max_batch)
    vol = sigmas.reshape(resolution, resolution, resolution).flip(0)
    if crop:                                                                                # gen_videos.py:213-220
        (a0, b0), (a1, b1), (a2, b2) = crop_ranges(resolution)
        vol = vol.clone()
        vol[:a0] = 0
        vol[-b0:] = 0
        vol[:, :a1] = 0
        vol[:, -b1:] = 0
        vol[:, :, :a2] = 0
        vol[:, :, -b2:] = 0
    return (vol, planes) if return_planes else vol


DirectMesh = collections.namedtuple('DirectMesh', 'verts faces resolution')     # extract_band_mesh's mesh, for mesh_of_density_grid in place of a volume


@torch.no_grad()
def extract_band_mesh(G, ws, resolution=512, level=10.0, band=8, crop=True, planes=None, return_planes=False, report=None):
    """The mesh mesh_of_density_grid makes of extract_density_grid(..., band=band, level=level)'s volume at `level`, without that volume's
    passes: the narrow band's rounds evaluate the densities (no fill), and marching cubes runs over the active bricks alone, reading the
    lattice as the queries left it -- the flip and the transpose as a view, the crop as the kept range (shape_mi355x.band_mesh) -> (verts
    float32 [V, 3], faces int32 [T, 3]) on ws' device, in the index space mesh_of_density_grid meshes in, bit for bit and in the same order.
    planes / return_planes as extract_density_grid's ((verts, faces), planes); report: a dict that receives the band's report under 'band'."""
    if planes is None:
        planes = G.backbone.synthesis(ws, noise_mode='const')
        planes = planes.view(len(planes), 3, 32, planes.shape[-2], planes.shape[-1])
    field, keep = _band_field(G, planes, resolution, crop)
    verts, faces, band_report = shape_mi355x.band_mesh(field, resolution, level, band, keep, device=planes.device, **shape_mi355x.BAND_MESH_PIPELINE_VIEW)
    verts, faces = torch.as_tensor(verts).to(planes.device), torch.as_tensor(faces).to(planes.device)
    if report is not None:
        report['band'] = band_report
    return ((verts, faces), planes) if return_planes else (verts, faces)


MESH_ATTRS = ('none', 'normals', 'colors', 'all')


@torch.no_grad()
def mesh_vertex_attributes(G, planes, verts, resolution, want_normals=True, want_colors=True, max_batch=4000000):
    """Per-vertex attributes of a mesh of extract_density_grid's volume, evaluated at the vertices' world positions on verts' device:
    (normals float32 [V, 3] in the mesh's index frame or None, colors uint8 [V, 3] or None).  Normals are those of the density field,
    -grad sigma normalised (ImportanceRenderer.query_normals: the position-gradient kernel on a GPU); colours the decoder's first
    three channels (image_raw is feature_image[:, :3]) as clip((c * 0.5 + 0.5) * 255), rounded."""
    kw = G.rendering_kwargs
    planes = planes[:1]
    normals, colors = [], []
    for head in range(0, len(verts), max_batch):
        world = lattice_to_world(mesh_to_lattice(verts[head:head + max_batch].float(), resolution), resolution, kw['box_warp']).unsqueeze(0)
        if want_normals:
            normals.append(normals_to_mesh_frame(G.renderer.query_normals(planes, G.decoder, world, kw)[1][0], resolution, kw['box_warp']))
        if want_colors:
            dirs = torch.zeros_like(world)
            dirs[..., -1] = -1
            rgb = G.renderer.run_model(planes, G.decoder, world, dirs, dict(kw, density_noise=0))['rgb'][0, :, :3]
            colors.append(((rgb * 0.5 + 0.5) * 255).clamp(0, 255).round().to(torch.uint8))
    empty = verts.new_zeros([0, 3])
    return (torch.cat(normals or [empty]) if want_normals else None), (torch.cat(colors or [empty.to(torch.uint8)]) if want_colors else None)


@torch.no_grad()
def snap_extracted_mesh(G, planes, verts, faces, resolution, snap, level=10.0):
    """--mesh-snap: the last stage, after the smoothing.  Every vertex (index space) goes back onto the level set sigma = level of generator
    G's own density on `planes`: Newton steps along the density's gradient inside a box of snap['radius'] voxels around where it stood
    (ImportanceRenderer.project_to_level with mesh_to_world_matrix as the affine: one kernel launch on a GPU), then the flip guard
    (gnerf_hip.mesh_flip_guard / shape_mi355x.mesh_flip_guard_numpy) sets back the vertices of every face the move turned over.  A vertex
    that does not converge keeps its position -- by design those on the walls that extract_density_grid's crop cuts into the volume and that
    lie farther than the radius from the true surface.  snap: shape_mi355x.snap_options' dict or None (nothing runs) -> (verts, report or None);
    report: vertices, converged, not_converged, flat, reverted, median_before / max_before / median_after / max_after of |sigma - level|,
    flips (per guard round), flips_left, tol."""
    if not snap:
        return verts, None
    kw = G.rendering_kwargs
    dev = planes.device
    v = (verts if isinstance(verts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(verts))).to(dev).float().reshape(-1, 3)
    f = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(faces))
    rounds = snap['guard_rounds']
    tol = snap['tol'] if snap['tol'] is not None else 2.0 ** -10 * max(1.0, abs(float(level)))
    if len(v) == 0:
        return verts, dict(vertices=0, converged=0, not_converged=0, flat=0, reverted=0, median_before=0.0, max_before=0.0, median_after=0.0,
                           max_after=0.0, flips=[0] * rounds, flips_left=0, tol=tol)
    moved, status, res_in, res_out = G.renderer.project_to_level(planes[:1], G.decoder, v.unsqueeze(0), level, kw, affine=mesh_to_world_matrix(resolution, kw['box_warp']),
                                                                 steps=snap['steps'], radius=snap['radius'], tol=tol)
    moved, status, res_in, res_out = moved[0].float(), status[0], res_in[0].float(), res_out[0].float()
    if v.is_cuda:
        import gnerf_hip
        out, status, counts = gnerf_hip.mesh_flip_guard(v, moved, f.to(dev), status, rounds)
        counts = counts.cpu().numpy()
    else:
        out, status, counts = shape_mi355x.mesh_flip_guard_numpy(v.numpy(), moved.numpy(), f.numpy(), status.numpy(), rounds)
        out, status = torch.from_numpy(out), torch.from_numpy(status)
    res_out = torch.where(status == 3, res_in, res_out)
    before, after = res_in.abs(), res_out.abs()

    def stats(x):
        x = x[torch.isfinite(x)]
        return (float(x.median()), float(x.max())) if len(x) else (float('nan'), float('nan'))

    (m0, x0), (m1, x1) = stats(before), stats(after)
    tally = torch.bincount(status.long().cpu(), minlength=4)
    report = dict(vertices=len(v), converged=int(tally[0]), not_converged=int(tally[1]), flat=int(tally[2]), reverted=int(tally[3]), median_before=m0,
                  max_before=x0, median_after=m1, max_after=x1, flips=[int(c) for c in counts[:rounds]], flips_left=int(counts[rounds]), tol=tol)
    if isinstance(verts, torch.Tensor):
        return out.to(verts.device), report
    return out.cpu().numpy(), report


def bake_frames_of_orbit(full, n_frames, n_bake, radius):
    """--mesh-bake's choice among the orbit's gathered frames `full` [n_frames, H, W, 3]: n_bake of them at indices (j n_frames) // n_bake, with
    their camera labels -> (indices, frames uint8 [n_bake, H, W, 3], labels [n_bake, 25] on the host)."""
    idx = [(j * n_frames) // n_bake for j in range(n_bake)]
    return idx, full[idx].contiguous(), H.orbit_labels(idx, n_frames, radius)


def bake_extracted_mesh(verts, faces, normals, fallback, bake, resolution, cube_length, patch=0):
    """--mesh-bake on the final mesh (index space; mesh_to_world_matrix puts it into the world): shape_mi355x.bake_mesh_colors from bake['frames']
    (uint8 [N, H, W, 3]) and their camera labels bake['labels'] [N, 25], rasterised at bake['res'] (None: the frames' size), with bake['rules'].
    normals / fallback: per-vertex arrays or tensors, or None.  Kernels when the frames are on a GPU, the numpy ports otherwise.
    patch > 0: --mesh-texture instead, shape_mi355x.bake_mesh_texture of the atlas at that patch size from the same frames, cameras and rules."""
    frames, labels = bake['frames'], bake['labels']
    dev = frames.device

    def place(x, dtype=None):
        if x is None:
            return None
        x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        x = x.to(dev) if dtype is None else x.to(dev, dtype)
        return x if dev.type == 'cuda' else x.numpy()
    stage = shape_mi355x.bake_mesh_colors if not patch else lambda *a, **kw: shape_mi355x.bake_mesh_texture(*a, patch=patch, **kw)
    return stage(place(verts, torch.float32), place(faces, torch.int32), place(frames), labels[:, :16].reshape(-1, 4, 4),
                 labels[:, 16:25].reshape(-1, 3, 3), mesh2world=mesh_to_world_matrix(resolution, cube_length),
                 normals=place(normals, torch.float32), vis_size=bake.get('res'), fallback=place(fallback), **bake.get('rules', {}))


def mesh_of_density_grid(vol, level=10.0, attrs=None, G=None, planes=None, clean=None, simplify=None, snap=None, bake=None, band=None):
    """The mesh shape_utils.convert_mrc makes of the .mrc of this volume (shape_utils.py:103-105: transpose(2, 1, 0), voxel size 1, origin 0),
    made where the volume lives -- on a GPU the marching-cubes kernel reads it in HBM -- and taken through shape_mi355x.finish_mesh, which
    states the order of the stages -> (its FinishedMesh, on the volume's route and in index space, as the reference's; seconds spent in
    marching cubes).
    attrs: None / 'none', 'normals', 'colors' or 'all' -- per-vertex attributes (mesh_vertex_attributes) of generator G on `planes`
    (extract_density_grid(..., return_planes=True)).  clean, simplify, snap: None or shape_mi355x.clean_options' / simplify_options' /
    snap_options' dict (snap_extracted_mesh on G and `planes`).  bake: None or bake_extracted_mesh's dict (frames, labels, res, rules) -- the
    final mesh is coloured from those frames, with the normals when attrs made them and the decoder's colours, when it made them, as the fallback;
    with bake['texture'] = P > 0 its texture atlas at patch P is baked from them too (the FinishedMesh's reports['texture']).
    band: None, or the report of the narrow band the volume was made in (extract_density_grid(..., band=s, report=...)['band']), which
    must have followed this `level`: it becomes the FinishedMesh's reports['band'], ahead of the stages'.
    vol may also be a DirectMesh (extract_band_mesh's vertices and faces, and the resolution): marching cubes has run already, the stages follow
    as on a volume.  With every option None nothing but marching cubes runs."""
    attrs = 'none' if attrs is None else attrs
    if attrs not in MESH_ATTRS:
        raise ValueError(f'mesh_density_grid: attrs must be one of {MESH_ATTRS}')
    if (attrs != 'none' or snap) and (G is None or planes is None):
        raise ValueError('mesh_density_grid: vertex attributes and the snap need the generator G and the planes the volume was made from')
    if bake and G is None:
        raise ValueError('mesh_density_grid: the bake needs the generator G (its box)')
    if isinstance(vol, DirectMesh):
        (verts, faces, res), device, dt = vol, vol.verts.device, 0.0
    else:
        res, device = vol.shape[0], vol.device
        t0 = time.perf_counter()
        verts, faces = shape_mi355x.marching_cubes(vol.permute(2, 1, 0).contiguous(), level)     # (reads its counts: synchronised)
        dt = time.perf_counter() - t0
    stages = {}
    if snap:
        stages['snap'] = lambda v, f: snap_extracted_mesh(G, planes, v, f, res, snap, level=level)
    if attrs != 'none':
        stages['attributes'] = lambda v: mesh_vertex_attributes(G, planes, torch.as_tensor(v).to(device), res, attrs in ('normals', 'all'),
                                                                attrs in ('colors', 'all'))
    if bake:
        stages['bake'] = lambda v, f, normals, colors: bake_extracted_mesh(v, f, normals, colors, bake, res, G.rendering_kwargs['box_warp'])
        if bake.get('texture'):
            stages['texture'] = lambda v, f, normals, colors: bake_extracted_mesh(v, f, normals, colors, bake, res, G.rendering_kwargs['box_warp'],
                                                                                  patch=bake['texture'])
    mesh = shape_mi355x.finish_mesh(verts, faces, clean=clean, simplify=simplify, **stages)
    if band is not None:
        mesh = mesh._replace(reports={'band': band, **mesh.reports})
    return mesh, dt


def mesh_density_grid(vol, ply_path, level=10.0, **options):
    """--mesh: write mesh_of_density_grid(vol, level, **options) to `ply_path`, with its normals and its colours -- the baked ones when it baked.
    Returns (vertex count, triangle count, seconds spent in marching cubes), with the FinishedMesh (the reports) as its attribute `mesh`."""
    mesh, dt = mesh_of_density_grid(vol, level, **options)
    verts, faces, normals, colors = (shape_mi355x.to_host(x) for x in (mesh.verts, mesh.faces, mesh.normals, mesh.baked['colors'] if mesh.baked else mesh.colors))
    shape_mi355x.write_ply(ply_path, verts, faces, normals=normals, colors=colors)
    return shape_mi355x.Written((len(verts), len(faces), dt), mesh)


@torch.no_grad()
def render_geometry_orbit(verts, faces, n_frames, res, voxel_res, cube_length, radius, rank=0, world=1, frames_per_call=1, normals=None, colors=None,
                          shading=None):
    """This rank's shaded geometry frames of the orbit, uint8 [n_local, res, res, 3] on verts' device (None for an empty share): the mesh of a
    voxel_res^3 density volume (index space; mesh_to_world_matrix puts it into the world) drawn from the orbit's cameras, frames_per_call
    views per rasteriser call, on the pixel grid of image_raw / image_depth at that resolution.  CUDA tensors take the kernels, CPU tensors
    and numpy arrays the numpy port (shape_mi355x.render_mesh)."""
    lo, hi = H.shard_range(n_frames, rank, world)
    if hi == lo:
        return None, (lo, hi)
    labels = H.orbit_labels(range(lo, hi), n_frames, radius)
    mesh2world = mesh_to_world_matrix(voxel_res, cube_length)
    k = max(int(frames_per_call), 1)
    frames = []
    for j in range(0, hi - lo, k):
        c = labels[j:j + k]
        out = shape_mi355x.render_mesh(verts, faces, c[:, :16].reshape(-1, 4, 4), c[:, 16:25].reshape(-1, 3, 3), res, mesh2world=mesh2world,
                                       normals=normals, colors=colors, shading=shading, outputs=('frame',))
        frames.append(torch.as_tensor(out['frame']))
    return torch.cat(frames), (lo, hi)


def arg_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--network', help='generator pickle (G_ema)')
    ap.add_argument('--encoder', help='identity encoder pickle (E)')
    ap.add_argument('--id-image', help='identity reference image')
    ap.add_argument('--random-init', action='store_true', help='seeded random generator + random z instead of pickles')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--frames', type=int, default=120)                  # gen_videos.py:151
    ap.add_argument('--res', type=int, default=64)                      # neural rendering resolution, gen_videos.py:81
    ap.add_argument('--no-double-depth', action='store_true', help='keep the checkpoint depth resolutions (the reference CLI doubles them)')
    ap.add_argument('--device', default='cuda' if torch.cuda.is_available() else 'cpu')
    ap.add_argument('--graph', action='store_true', help='replay the per-frame launch sequence from a captured HIP graph')
    ap.add_argument('--frames-per-call', type=int, default=1, help='cameras per synthesis call (views of the one latent in one renderer launch)')
    ap.add_argument('--out', default=None, help='write frames to this .npy (rank 0)')
    ap.add_argument('--shapes', default=None, help='also extract the 512^3 density volume (gen_videos.py --shapes) and save it to this .npy (rank 0)')
    ap.add_argument('--shapes-mrc', default=None, help='also write the density volume as the reference\'s .mrc (gen_videos.py:221-222; rank 0)')
    ap.add_argument('--mesh', default=None, help='also mesh the density volume on the device and write this .ply (shape_utils.py; rank 0)')
    ap.add_argument('--mesh-level', type=float, default=10, help='isosurface level of --mesh (shape_utils.py:111)')
    ap.add_argument('--mesh-band', type=int, default=0, metavar='S',
                    help='evaluate the density volume of --mesh / --geometry-out only in a narrow band of bricks of S^3 cells (2, 4, 8 or 16; 8 is a good start) '
                         'around the level set of --mesh-level: the same mesh, minus detached components thinner than a brick (0: off, every lattice point). '
                         'With --shapes / --shapes-mrc the dense volume is made once and meshed too: those files hold densities everywhere')
    ap.add_argument('--mesh-direct', action='store_true',
                    help='with --mesh-band S: mesh the band brick by brick, straight on the lattice as the queries left it (no fill, no crop / flip / '
                         'transpose passes, no pass over the whole volume): the same mesh, byte for byte (--mesh and --geometry-out; not with --shapes / '
                         '--shapes-mrc, which need densities everywhere)')
    ap.add_argument('--mesh-attrs', choices=MESH_ATTRS, default='none', help='per-vertex attributes of --mesh: normals of the density field and / or the decoder\'s colours')
    shape_mi355x.add_mesh_arguments(ap, attributes=True, texture=True)
    ap.add_argument('--mesh-snap', type=float, default=0, metavar='R',
                    help='last, after the smoothing: move every vertex onto the level set of the density itself (Newton steps along its gradient), at most '
                         'R voxels per axis from where it stood; faces that this turns over get their vertices back (--mesh and --geometry-out; 0: off)')
    ap.add_argument('--mesh-snap-steps', type=int, default=6, help='Newton steps of --mesh-snap at the most')
    ap.add_argument('--mesh-snap-tol', type=float, default=None, help='|sigma - level| at which a vertex of --mesh-snap is done (default: 2^-10 max(1, |level|))')
    ap.add_argument('--mesh-bake', type=int, default=0, metavar='N',
                    help='colour the vertices of --mesh from N of the orbit\'s frames, at indices (j * frames) // N: each vertex takes the frames\' colours where '
                         'it is visible, blended by how squarely the views face it (with the normals of --mesh-attrs); the decoder\'s colours stay where no frame sees (0: off)')
    ap.add_argument('--mesh-bake-res', type=int, default=None, help='resolution of the visibility buffers of --mesh-bake (default: the frames\' size)')
    ap.add_argument('--mesh-bake-tol', type=float, default=2.0 ** -8, help='relative depth tolerance of --mesh-bake\'s occlusion test')
    ap.add_argument('--mesh-bake-guard', type=int, default=1, help='--mesh-bake tests the (2 GUARD + 1)^2 pixels around a vertex (0..4)')
    ap.add_argument('--mesh-bake-power', type=int, default=2, help='--mesh-bake weights a view by cos^POWER of the angle between normal and line of sight (0..8)')
    ap.add_argument('--voxel-res', type=int, default=512)
    ap.add_argument('--geometry-out', default=None, help='also draw the mesh of the density volume from every orbit camera (shaded geometry frames, '
                                                         'uint8 [F, H, W, 3]) and write them to this .npy (rank 0); uses --voxel-res, --mesh-level, --mesh-attrs, --frames-per-call')
    ap.add_argument('--geometry-res', type=int, default=512, help='resolution of the geometry frames')
    ap.add_argument('--no-solver-search', action='store_true', help='leave torch.backends.cudnn.benchmark off (MIOpen takes its first heuristic pick per shape)')
    return ap


def main():
    ap = arg_parser()
    args = ap.parse_args()
    clean, simplify, snap = shape_mi355x.mesh_options_from_args(args, ap)
    if args.mesh_bake and not args.mesh:
        ap.error('--mesh-bake requires --mesh')
    texture_patch = shape_mi355x.texture_from_args(args, ap)
    if args.mesh_band not in (0,) + shape_mi355x.BAND_BRICKS:
        ap.error(f'--mesh-band must be 0 or one of {shape_mi355x.BAND_BRICKS}')
    if args.mesh_direct and not args.mesh_band:
        ap.error('--mesh-direct requires --mesh-band S')
    if args.mesh_direct and (args.shapes or args.shapes_mrc):
        ap.error('--mesh-direct cannot be combined with --shapes / --shapes-mrc: those files need densities everywhere, and the direct route makes no volume')
    if not 0 <= args.mesh_bake <= args.frames:
        ap.error('--mesh-bake must be 0 .. --frames')
    if (not args.mesh_bake_tol >= 0 or not 0 <= args.mesh_bake_guard <= 4 or not 0 <= args.mesh_bake_power <= 8
            or (args.mesh_bake_res is not None and not 1 <= args.mesh_bake_res <= 4096)):
        ap.error('--mesh-bake-tol must be >= 0, --mesh-bake-guard 0..4, --mesh-bake-power 0..8, --mesh-bake-res 1..4096')
    H.configure_backend(False if args.no_solver_search else None)

    rank, world, local_rank = H.init_from_env()
    # (modulo: a rehearsal of several ranks on a one-GPU box with GNERF_DIST_BACKEND=gloo shares the card)
    device = torch.device('cuda', local_rank % max(1, torch.cuda.device_count())) if args.device == 'cuda' else torch.device(args.device)
    if device.type == 'cuda':
        torch.cuda.set_device(device)
    if args.random_init:
        G = build_random_generator(args.seed, device)
    else:
        assert args.network, 'give --network or --random-init'
        G = load_generator(args.network, device)
    z = identity_latent(args, device, G.z_dim)

    # One untimed frame first: library load, MIOpen's per-shape kernel search (tens of seconds on a fresh machine) and the
    # allocator's first touches are one-off costs of the process, not of the orbit.
    render_orbit(G, z, args.frames, args.res, device, rank=0, world=args.frames, double_depth=False)
    if device.type == 'cuda':
        torch.cuda.synchronize()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    t0 = time.perf_counter()
    frames, raws, (lo, hi) = render_orbit(G, z, args.frames, args.res, device, rank, world, double_depth=not args.no_double_depth, use_graph=args.graph,
                                          frames_per_call=args.frames_per_call)
    full = H.gather_frames(frames, args.frames)
    if device.type == 'cuda':
        torch.cuda.synchronize()
    elapsed = H.max_over_ranks(time.perf_counter() - t0, device)
    if rank == 0:
        print(f'{args.frames} frames on {world} rank(s){" (HIP graph replay)" if args.graph else ""}: {elapsed:.3f} s = {args.frames / elapsed:.2f} frames/s '
              f'(neural rendering {args.res}x{args.res}, {G.rendering_kwargs["depth_resolution"]}+{G.rendering_kwargs["depth_resolution_importance"]} samples)')
        if args.out:
            np.save(args.out, full.cpu().numpy())
    made = {}
    stages = dict(attrs=args.mesh_attrs, G=G, clean=clean, simplify=simplify, snap=snap)         # of the mesh, for --mesh and --geometry-out alike

    def volume_and_planes():                                             # made once per process, whichever option asks first
        if 'vol' not in made:
            if device.type == 'cuda':
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            # --shapes / --shapes-mrc write the volume itself, which must hold densities everywhere: with them the dense volume is made
            # once and meshed too (the same choice on every rank: the geometry frames are drawn from one mesh)
            band = args.mesh_band if not (args.shapes or args.shapes_mrc) else 0
            if args.mesh_band and not band and rank == 0:
                print('--mesh-band: off, --shapes / --shapes-mrc need the dense volume; it is made once and meshed too')
            reports = {}
            if args.mesh_direct:                                         # no volume: the band's mesh itself, for mesh_of_density_grid
                mesh, made['planes'] = extract_band_mesh(G, orbit_latents(G, z, device), args.voxel_res, args.mesh_level, band, return_planes=True,
                                                         report=reports)
                made['vol'] = DirectMesh(*mesh, args.voxel_res)
            else:
                made['vol'], made['planes'] = extract_density_grid(G, orbit_latents(G, z, device), args.voxel_res, return_planes=True, band=band or None,
                                                                   level=args.mesh_level, report=reports)
            made['band'] = reports.get('band')
            if device.type == 'cuda':
                torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rank == 0:
                if args.mesh_direct:
                    print(f'band mesh of the {args.voxel_res}^3 lattice: {dt:.3f} s, {made["band"]["visited"]} points in {made["band"]["active"]} active bricks')
                else:
                    print(f'density volume {args.voxel_res}^3: {dt:.3f} s = {args.voxel_res ** 3 / dt / 1e9:.2f} G points/s')
                if made['band']:
                    print(shape_mi355x.band_report_line(made['band']))
        return made['vol'], made['planes']

    if rank == 0 and (args.shapes or args.shapes_mrc or args.mesh):
        vol, planes = volume_and_planes()
        if args.shapes:
            np.save(args.shapes, vol.cpu().numpy())
        if args.shapes_mrc:
            shape_mi355x.write_mrc(args.shapes_mrc, vol.cpu().numpy())
        if args.mesh:
            t0 = time.perf_counter()
            bake = None
            if args.mesh_bake:                                           # N of the frames this run has just gathered, and their cameras
                _, bake_frames, bake_labels = bake_frames_of_orbit(full, args.frames, args.mesh_bake, G.rendering_kwargs['avg_camera_radius'])
                bake = dict(frames=bake_frames, labels=bake_labels, res=args.mesh_bake_res,
                            rules=dict(depth_tol=args.mesh_bake_tol, guard=args.mesh_bake_guard, power=args.mesh_bake_power), texture=texture_patch)
            nv, nf, dt = written = mesh_density_grid(vol, args.mesh, args.mesh_level, planes=planes, bake=bake, band=made['band'], **stages)
            made['mesh'] = written.mesh
            for line in shape_mi355x.report_lines(written.mesh.reports, smooth=args.mesh_smooth, bake_views=args.mesh_bake):
                print(line)
            if texture_patch:                                            # the same mesh again as .obj + .mtl + .png, with the atlas' UVs
                mesh, textured = written.mesh, written.mesh.reports['texture']
                shape_mi355x.write_obj(args.mesh_texture_out, shape_mi355x.to_host(mesh.verts), shape_mi355x.to_host(mesh.faces),
                                       shape_mi355x.atlas_uvs(nf, texture_patch), shape_mi355x.to_host(textured['texture']),
                                       normals=shape_mi355x.to_host(mesh.normals))
                print(shape_mi355x.texture_report_line(textured, args.mesh_bake, texture_patch) + f' -> {args.mesh_texture_out}')
            print(f'mesh at level {args.mesh_level:g}: {dt * 1e3:.2f} ms, {nv} vertices, {nf} triangles -> {args.mesh}'
                  + (f' (with {args.mesh_attrs}: {(time.perf_counter() - t0) * 1e3:.2f} ms in all, file included)' if args.mesh_attrs != 'none' else ''))
    if args.geometry_out:
        # every rank meshes the volume itself (the same bits everywhere: no mesh travels between ranks), then draws its share of the cameras;
        # rank 0 draws the mesh --mesh has just made and reported, when it has
        vol, planes = volume_and_planes()
        if 'mesh' not in made:
            made['mesh'], _ = mesh_of_density_grid(vol, args.mesh_level, planes=planes, band=made['band'], **stages)
            if rank == 0:
                for line in shape_mi355x.report_lines(made['mesh'].reports, smooth=args.mesh_smooth):
                    print(line)
        verts, faces, normals, colors = made['mesh'][:4]                 # (the decoder's colours, also after a bake)
        if device.type == 'cuda':
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        geo, _ = render_geometry_orbit(verts, faces, args.frames, args.geometry_res, args.voxel_res, G.rendering_kwargs['box_warp'],
                                       G.rendering_kwargs['avg_camera_radius'], rank, world, args.frames_per_call, normals=normals, colors=colors)
        if geo is None:
            geo = torch.zeros([0, args.geometry_res, args.geometry_res, 3], dtype=torch.uint8)
        full_geo = H.gather_frames(geo.to(device), args.frames)
        if device.type == 'cuda':
            torch.cuda.synchronize()
        dt = H.max_over_ranks(time.perf_counter() - t0, device)
        if rank == 0:
            print(f'geometry frames: {args.frames} at {args.geometry_res}x{args.geometry_res} of {len(faces)} triangles in {dt:.3f} s = {args.frames / dt:.2f} frames/s '
                  f'-> {args.geometry_out}')
            np.save(args.geometry_out, full_geo.cpu().numpy())


if __name__ == '__main__':
    main()
