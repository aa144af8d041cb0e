"""The triangle rasteriser for extracted meshes (csrc/raster.hip): a visibility buffer per view, then depth / normal / shaded colour;
and its inverse, the multi-view colour bake: frames back onto the vertices, or into a texture atlas that a textured resolve draws."""

import ctypes

import torch

from . import _native
from ._native import _check, _launch, _on_device, _ptr, _require_cuda, load, profiled

RASTER_SMALL_PIXELS = 64            # GNERF_RASTER_SMALL_PIXELS (include/gnerf_hip.h): the largest bounding box a triangle's own thread walks
RASTER_MAX_SIZE = 4096              # GNERF_RASTER_MAX_SIZE
RASTER_CULL = {'none': 0, 'back': 1, 'front': 2}
RASTER_OUTPUTS = ('tri_id', 'depth', 'normal', 'frame')
# light: from the surface to the light, in the camera frame (the default is a headlight); colours in [0, 1]
RASTER_SHADING = dict(light=(0.0, 0.0, -1.0), ambient=0.25, diffuse=0.75, albedo=(0.8, 0.8, 0.8), background=(1.0, 1.0, 1.0))


def raster_available():
    """Whether the loaded library has the rasteriser (a version-15 library built before it does not)."""
    return all(hasattr(load(), name) for name in ('gnerf_raster_workspace_bytes', 'gnerf_raster_visibility', 'gnerf_raster_resolve'))


def _require_raster():
    if not raster_available():
        raise RuntimeError('gnerf_hip: this libgnerf_hip.so was built without the rasteriser (gnerf_raster_*): rebuild it (csrc/build.sh)')


def _f32(t, shape, what):
    t = t.detach()
    if t.numel() % shape[-1] != 0:
        raise ValueError(f'raster: {what} has shape {tuple(t.shape)}')
    t = t.reshape(-1, shape[-1])
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


def _mesh(verts, faces):
    _require_cuda(verts, faces)
    if faces.device != verts.device:
        raise RuntimeError('raster: verts and faces must be on one device')
    v = _f32(verts, (3,), 'verts')
    f = faces.detach().reshape(-1, 3)
    f = f if (f.dtype == torch.int32 and f.is_contiguous()) else f.to(torch.int32).contiguous()
    return v, f


def _cameras(mesh2cam, intrinsics, device):
    """[n, 12] and [n, 9] float32 on `device`.  Tensors that already are that are passed through untouched, so that a captured graph reads
    the caller's tensors in place (overwrite them and replay)."""
    _require_cuda(mesh2cam, intrinsics)
    if mesh2cam.device != device or intrinsics.device != device:
        raise RuntimeError('raster: the cameras must be on the mesh\'s device')
    A, K = _f32(mesh2cam, (12,), 'mesh2cam'), _f32(intrinsics, (9,), 'intrinsics')
    if len(A) != len(K) or len(A) < 1:
        raise ValueError(f'raster: {len(A)} mesh2cam for {len(K)} intrinsics')
    return A, K


def _size(size):
    h, w = (size, size) if isinstance(size, int) else size
    h, w = int(h), int(w)
    if not (1 <= h <= RASTER_MAX_SIZE and 1 <= w <= RASTER_MAX_SIZE):
        raise ValueError(f'raster: the image size must be 1..{RASTER_MAX_SIZE} in each direction (got {h} x {w})')
    return h, w


def shading_vector(shading=None):
    """The eleven floats gnerf_raster_resolve takes: light [3], ambient, diffuse, albedo [3], background [3] (RASTER_SHADING's keys)."""
    s = dict(RASTER_SHADING, **(shading or {}))
    unknown = set(s) - set(RASTER_SHADING)
    if unknown:
        raise ValueError(f'raster: unknown shading parameter(s) {sorted(unknown)}')
    vec = [float(x) for x in (*s['light'], s['ambient'], s['diffuse'], *s['albedo'], *s['background'])]
    if len(vec) != 11:
        raise ValueError('raster: light, albedo and background are triples, ambient and diffuse scalars')
    return vec


def _rasterize_ctypes(v, f, A, K, h, w, near, cull, workspace=None, vis=None):
    """The ctypes route of rasterize (arguments as _mesh / _cameras / _size return them)."""
    dev, n = v.device, len(A)
    if workspace is None:
        nbytes = ctypes.c_size_t()
        _check(load().gnerf_raster_workspace_bytes(len(v), len(f), n, h, w, ctypes.byref(nbytes)), 'gnerf_raster_workspace_bytes')
        workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    if vis is None:
        vis = torch.empty([n, h, w], dtype=torch.int64, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    _launch('gnerf_raster_visibility', v, _ptr(v) if len(v) else None, len(v), _ptr(f) if len(f) else None, len(f), _ptr(A), _ptr(K), n, h, w,
            float(near), cull, _ptr(workspace), _ptr(vis), _ptr(counts))
    return vis, counts


def raster_workspace_bytes(n_verts, n_tris, n_views, size):
    _require_raster()
    h, w = _size(size)
    nbytes = ctypes.c_size_t()
    _check(load().gnerf_raster_workspace_bytes(int(n_verts), int(n_tris), int(n_views), h, w, ctypes.byref(nbytes)), 'gnerf_raster_workspace_bytes')
    return int(nbytes.value)


@profiled('gnerf_hip::rasterize')
def rasterize(verts, faces, mesh2cam, intrinsics, size, near=0.01, cull='none', workspace=None, vis=None):
    """Visibility buffer of a mesh (verts float32 [V, 3], faces int32 [T, 3], CUDA) from n cameras: mesh2cam [n, 3, 4] (mesh frame -> the
    camera frame of csrc/raygen.h) and normalised intrinsics [n, 3, 3], CUDA tensors; size = (h, w) or one int.  -> (vis int64 [n, h, w]: the
    bits of the kernel's uint64 keys, float_as_uint(z) << 32 | triangle, -1 where empty; counts int64 [4] on the device = drawn, near, guard,
    culled).  Rules: include/gnerf_hip.h, gnerf_raster_*; shape_mi355x.rasterize_numpy gives the same bits.  No host read: capturable in a
    graph (float32 contiguous camera tensors are read in place).  workspace / vis: optional preallocated buffers (uint8 of
    raster_workspace_bytes, int64 [n, h, w]); neither needs initialising."""
    _require_raster()
    v, f = _mesh(verts, faces)
    A, K = _cameras(mesh2cam, intrinsics, v.device)
    h, w = _size(size)
    if cull not in RASTER_CULL:
        raise ValueError(f'raster: cull must be one of {tuple(RASTER_CULL)}')
    if not near > 0:
        raise ValueError('raster: near must be > 0')
    if vis is not None and (vis.dtype != torch.int64 or tuple(vis.shape) != (len(A), h, w) or not vis.is_contiguous() or vis.device != v.device):
        raise ValueError('raster: vis must be a contiguous int64 [n_views, h, w] tensor on the mesh\'s device')
    if workspace is not None and (workspace.dtype != torch.uint8 or workspace.device != v.device or not workspace.is_contiguous()
                                  or workspace.numel() < raster_workspace_bytes(len(v), len(f), len(A), (h, w))):
        raise ValueError('raster: workspace must be a contiguous uint8 tensor of raster_workspace_bytes(...) on the mesh\'s device')
    e = _native.ext()
    if e is not None and hasattr(e, 'raster_visibility'):
        with _on_device(v.device):
            return e.raster_visibility(v, f, A, K, h, w, float(near), RASTER_CULL[cull], workspace, vis)
    return _rasterize_ctypes(v, f, A, K, h, w, near, RASTER_CULL[cull], workspace, vis)


def _resolve_ctypes(vis, v, f, A, K, normals, normal_mat, colors, shading, want):
    dev = vis.device
    n, h, w = vis.shape
    out = {}
    if 'tri_id' in want:
        out['tri_id'] = torch.empty([n, h, w], dtype=torch.int32, device=dev)
    if 'depth' in want:
        out['depth'] = torch.empty([n, h, w], dtype=torch.float32, device=dev)
    if 'normal' in want:
        out['normal'] = torch.empty([n, h, w, 3], dtype=torch.float32, device=dev)
    if 'frame' in want:
        out['frame'] = torch.empty([n, h, w, 3], dtype=torch.uint8, device=dev)
    sh = (ctypes.c_float * 11)(*shading)
    _launch('gnerf_raster_resolve', vis, _ptr(vis), _ptr(v) if len(v) else None, len(v), _ptr(f) if len(f) else None, len(f), _ptr(A), _ptr(K), n, h, w,
            _ptr(normals), _ptr(normal_mat), _ptr(colors), sh, _ptr(out.get('tri_id')), _ptr(out.get('depth')), _ptr(out.get('normal')),
            _ptr(out.get('frame')))
    return out


@profiled('gnerf_hip::raster_resolve')
def resolve(vis, verts, faces, mesh2cam, intrinsics, normals=None, normal_mat=None, colors=None, shading=None, outputs=RASTER_OUTPUTS):
    """Per-pixel images of rasterize's visibility buffer, from the same mesh and cameras -> dict over `outputs`: tri_id int32 [n, h, w] (-1:
    background), depth float32 [n, h, w] (distance along the pixel's ray, what image_depth holds; +inf: background), normal float32
    [n, h, w, 3] (camera frame, unit, facing the camera), frame uint8 [n, h, w, 3].  normals float32 [V, 3] (mesh frame) need normal_mat
    [n, 3, 3] (mesh frame -> camera frame); colors uint8 [V, 3]; shading: dict over RASTER_SHADING's keys.  Without normals the face normals
    shade.  shape_mi355x.resolve_numpy gives the same bits."""
    _require_raster()
    v, f = _mesh(verts, faces)
    A, K = _cameras(mesh2cam, intrinsics, v.device)
    _require_cuda(vis)
    if vis.dtype != torch.int64 or vis.ndim != 3 or vis.shape[0] != len(A) or not vis.is_contiguous() or vis.device != v.device:
        raise ValueError('raster: vis must be rasterize\'s int64 [n_views, h, w] tensor')
    want = tuple(outputs)
    if not want or any(o not in RASTER_OUTPUTS for o in want):
        raise ValueError(f'raster: outputs must be a non-empty subset of {RASTER_OUTPUTS}')
    if normals is not None:
        if normal_mat is None:
            raise ValueError('raster: normals need normal_mat')
        _require_cuda(normals, normal_mat)
        normals, normal_mat = _f32(normals, (3,), 'normals'), _f32(normal_mat, (9,), 'normal_mat')
        if len(normals) != len(v) or len(normal_mat) != len(A) or normals.device != v.device or normal_mat.device != v.device:
            raise ValueError('raster: normals must be [V, 3] and normal_mat [n_views, 3, 3], on the mesh\'s device')
    else:
        normal_mat = None
    if colors is not None:
        _require_cuda(colors)
        if colors.dtype != torch.uint8 or tuple(colors.shape) != (len(v), 3) or colors.device != v.device:
            raise ValueError('raster: colors must be uint8 [V, 3] on the mesh\'s device')
        colors = colors.detach().contiguous()
    sh = shading_vector(shading)
    e = _native.ext()
    if e is not None and hasattr(e, 'raster_resolve'):
        with _on_device(v.device):
            got = e.raster_resolve(vis, v, f, A, K, normals, normal_mat, colors, sh, [o in want for o in RASTER_OUTPUTS])
        return {o: t for o, t in zip(RASTER_OUTPUTS, got) if o in want}
    return _resolve_ctypes(vis, v, f, A, K, normals, normal_mat, colors, sh, want)


# ---------------------------------------------------------------------------------------------------------------- the colour bake
BAKE_MAX_GUARD = 4                  # GNERF_BAKE_MAX_GUARD
BAKE_MAX_POWER = 8                  # GNERF_BAKE_MAX_POWER
BAKE_OUTPUTS = ('colors', 'weight', 'seen')
# arguments, not measurements (include/gnerf_hip.h, gnerf_mesh_bake_colors, derives depth_tol)
BAKE_RULES = dict(near=0.01, depth_tol=2.0 ** -8, guard=1, min_cos=0.1, power=2)


def bake_available():
    """Whether the loaded library has the colour bake (a version-15 library built before it does not)."""
    return hasattr(load(), 'gnerf_mesh_bake_colors')


def _bake_rules(near, depth_tol, guard, min_cos, power):
    """The five rule arguments as the C ABI takes them; ValueError for what gnerf_mesh_bake_colors would refuse."""
    if not near > 0:
        raise ValueError('bake: near must be > 0')
    if not depth_tol >= 0:
        raise ValueError('bake: depth_tol must be >= 0')
    if int(guard) != guard or not 0 <= guard <= BAKE_MAX_GUARD:
        raise ValueError(f'bake: guard must be an integer in 0..{BAKE_MAX_GUARD}')
    if int(power) != power or not 0 <= power <= BAKE_MAX_POWER:
        raise ValueError(f'bake: power must be an integer in 0..{BAKE_MAX_POWER}')
    return float(near), float(depth_tol), int(guard), float(min_cos), int(power)


def _bake_inputs(v, A, vis, frames, normals, normal_mat, fallback):
    """What bake_colors and bake_texture check alike, for verts v [V, 3] and cameras A [n, 12] -> (frames, normals, normal_mat, fallback) as the
    C ABI takes them; ValueError for a tensor of the wrong kind."""
    if vis.dtype != torch.int64 or vis.ndim != 3 or vis.shape[0] != len(A) or not vis.is_contiguous() or vis.device != v.device:
        raise ValueError('bake: vis must be rasterize\'s int64 [n_views, h, w] tensor')
    if (frames.dtype != torch.uint8 or frames.ndim != 4 or frames.shape[0] != len(A) or frames.shape[3] != 3 or frames.device != v.device
            or not (1 <= frames.shape[1] <= RASTER_MAX_SIZE and 1 <= frames.shape[2] <= RASTER_MAX_SIZE)):
        raise ValueError(f'bake: frames must be uint8 [n_views, fh, fw, 3] on the mesh\'s device, fh and fw in 1..{RASTER_MAX_SIZE}')
    frames = frames.detach().contiguous()
    if normals is not None:
        if normal_mat is None:
            raise ValueError('bake: normals need normal_mat')
        _require_cuda(normals, normal_mat)
        normals, normal_mat = _f32(normals, (3,), 'normals'), _f32(normal_mat, (9,), 'normal_mat')
        if len(normals) != len(v) or len(normal_mat) != len(A) or normals.device != v.device or normal_mat.device != v.device:
            raise ValueError('bake: normals must be [V, 3] and normal_mat [n_views, 3, 3], on the mesh\'s device')
    else:
        normal_mat = None
    if fallback is not None:
        _require_cuda(fallback)
        if fallback.dtype != torch.uint8 or tuple(fallback.shape) != (len(v), 3) or fallback.device != v.device:
            raise ValueError('bake: fallback must be uint8 [V, 3] on the mesh\'s device')
        fallback = fallback.detach().contiguous()
    return frames, normals, normal_mat, fallback


def _bake_colors_ctypes(v, A, K, vis, frames, normals, normal_mat, rules, fallback, colors=None, weight=None, seen=None):
    """The ctypes route of bake_colors (arguments as bake_colors has validated them; rules: _bake_rules' tuple)."""
    dev, V = v.device, len(v)
    colors = torch.empty([V, 3], dtype=torch.uint8, device=dev) if colors is None else colors
    weight = torch.empty([V], dtype=torch.float32, device=dev) if weight is None else weight
    seen = torch.empty([V], dtype=torch.int32, device=dev) if seen is None else seen
    n, h, w = vis.shape
    near, depth_tol, guard, min_cos, power = rules
    _launch('gnerf_mesh_bake_colors', vis, _ptr(v) if V else None, V, _ptr(A), _ptr(K), n, _ptr(vis), h, w, _ptr(frames), frames.shape[1],
            frames.shape[2], _ptr(normals), _ptr(normal_mat), near, depth_tol, guard, min_cos, power, _ptr(fallback), _ptr(colors) if V else None,
            _ptr(weight) if V else None, _ptr(seen) if V else None)
    return dict(colors=colors, weight=weight, seen=seen)


@profiled('gnerf_hip::bake_colors')
def bake_colors(verts, mesh2cam, intrinsics, vis, frames, normals=None, normal_mat=None, near=BAKE_RULES['near'], depth_tol=BAKE_RULES['depth_tol'],
                guard=BAKE_RULES['guard'], min_cos=BAKE_RULES['min_cos'], power=BAKE_RULES['power'], fallback=None, out=None):
    """Multi-view vertex colours: every vertex (verts float32 [V, 3], CUDA) gathers its colour from `frames` (uint8 [n, fh, fw, 3]) taken by the
    cameras (mesh2cam [n, 3, 4], intrinsics [n, 3, 3]) whose visibility buffers `vis` (rasterize's int64 [n, h, w], of the same mesh, cameras
    and near) decide where it is hidden; views are blended by cos^power of the angle between the vertex normal and the line of sight when
    normals float32 [V, 3] and normal_mat [n, 3, 3] (mesh frame -> camera frame) are given, equally otherwise.  -> dict(colors uint8 [V, 3],
    weight float32 [V], seen int32 [V]): a vertex no view sees (seen == 0, weight == 0) gets its `fallback` colour (uint8 [V, 3]) or 0.
    Rules: include/gnerf_hip.h, gnerf_mesh_bake_colors; shape_mi355x.bake_colors_numpy gives the same bits.  One launch, no host read:
    capturable (float32 contiguous camera tensors, vis and frames are read in place).  out: an optional dict of preallocated outputs."""
    if not bake_available():
        raise RuntimeError('gnerf_hip: this libgnerf_hip.so was built without the colour bake (gnerf_mesh_bake_colors): rebuild it (csrc/build.sh)')
    rules = _bake_rules(near, depth_tol, guard, min_cos, power)
    _require_cuda(verts, vis, frames)
    v = _f32(verts, (3,), 'verts')
    A, K = _cameras(mesh2cam, intrinsics, v.device)
    frames, normals, normal_mat, fallback = _bake_inputs(v, A, vis, frames, normals, normal_mat, fallback)
    out = dict(out or {})
    if set(out) - set(BAKE_OUTPUTS):
        raise ValueError(f'bake: out holds {BAKE_OUTPUTS} at the most')
    for name, dtype, shape in (('colors', torch.uint8, (len(v), 3)), ('weight', torch.float32, (len(v),)), ('seen', torch.int32, (len(v),))):
        t = out.get(name)
        if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != v.device):
            raise ValueError(f'bake: out[{name!r}] must be a contiguous {dtype} tensor of shape {shape} on the mesh\'s device')
    e = _native.ext()
    if e is not None and hasattr(e, 'mesh_bake_colors'):
        with _on_device(v.device):
            got = e.mesh_bake_colors(v, A, K, vis, frames, normals, normal_mat, *rules, fallback, out.get('colors'), out.get('weight'), out.get('seen'))
        return dict(zip(BAKE_OUTPUTS, got))
    return _bake_colors_ctypes(v, A, K, vis, frames, normals, normal_mat, rules, fallback, out.get('colors'), out.get('weight'), out.get('seen'))


# ---------------------------------------------------------------------------------------------------------------- the texture atlas
ATLAS_MIN_PATCH = 4                 # GNERF_ATLAS_MIN_PATCH
ATLAS_MAX_PATCH = 64                # GNERF_ATLAS_MAX_PATCH
ATLAS_MAX_SIZE = 16384              # GNERF_ATLAS_MAX_SIZE
TEXTURE_OUTPUTS = ('texture', 'weight', 'seen')
_TEXTURE_EXPORTS = ('gnerf_mesh_atlas_layout', 'gnerf_mesh_bake_texture', 'gnerf_raster_resolve_textured')


def texture_available():
    """Whether the loaded library has the texture bake and the textured resolve (a version-15 library built before them does not)."""
    return all(hasattr(load(), name) for name in _TEXTURE_EXPORTS)


def _require_texture():
    if not texture_available():
        raise RuntimeError('gnerf_hip: this libgnerf_hip.so was built without the texture atlas (gnerf_mesh_bake_texture): rebuild it (csrc/build.sh)')


def _patch(patch):
    if int(patch) != patch or not ATLAS_MIN_PATCH <= patch <= ATLAS_MAX_PATCH:
        raise ValueError(f'atlas: patch must be an integer in {ATLAS_MIN_PATCH}..{ATLAS_MAX_PATCH}')
    return int(patch)


def _rgb(colour, what):
    rgb = [int(c) for c in colour]
    if len(rgb) != 3 or any(not 0 <= c <= 255 for c in rgb):
        raise ValueError(f'{what}: background must be three values in 0..255')
    return rgb


def atlas_layout(n_tris, patch):
    """The atlas of a mesh of n_tris triangles at `patch` texels per patch side -> (cells per row, th, tw), from the library's own host
    function (include/gnerf_hip.h, gnerf_mesh_atlas_layout, states the rule; shape_mi355x.atlas_layout restates it).  ValueError for a patch
    out of range, NativeError (code E_UNSUPPORTED) for an atlas past ATLAS_MAX_SIZE a side."""
    _require_texture()
    cells, th, tw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _check(load().gnerf_mesh_atlas_layout(int(n_tris), _patch(patch), ctypes.byref(cells), ctypes.byref(th), ctypes.byref(tw)), 'gnerf_mesh_atlas_layout')
    return cells.value, th.value, tw.value


def _bake_texture_ctypes(v, f, patch, A, K, vis, frames, normals, normal_mat, rules, fallback, background, texture=None, weight=None, seen=None):
    """The ctypes route of bake_texture (arguments as bake_texture has validated them; rules: _bake_rules' tuple, background: three ints)."""
    dev, V, T = v.device, len(v), len(f)
    _, th, tw = atlas_layout(T, patch)
    texture = torch.empty([th, tw, 3], dtype=torch.uint8, device=dev) if texture is None else texture
    weight = torch.empty([th, tw], dtype=torch.float32, device=dev) if weight is None else weight
    seen = torch.empty([th, tw], dtype=torch.int32, device=dev) if seen is None else seen
    n, h, w = vis.shape
    near, depth_tol, guard, min_cos, power = rules
    bg = (ctypes.c_ubyte * 3)(*background)
    _launch('gnerf_mesh_bake_texture', vis, _ptr(v) if V else None, V, _ptr(f) if T else None, T, patch, _ptr(A), _ptr(K), n, _ptr(vis), h, w, _ptr(frames),
            frames.shape[1], frames.shape[2], _ptr(normals), _ptr(normal_mat), near, depth_tol, guard, min_cos, power, _ptr(fallback), bg,
            _ptr(texture) if T else None, _ptr(weight) if T else None, _ptr(seen) if T else None)
    return dict(texture=texture, weight=weight, seen=seen)


@profiled('gnerf_hip::bake_texture')
def bake_texture(verts, faces, mesh2cam, intrinsics, vis, frames, patch=8, normals=None, normal_mat=None, near=BAKE_RULES['near'],
                 depth_tol=BAKE_RULES['depth_tol'], guard=BAKE_RULES['guard'], min_cos=BAKE_RULES['min_cos'], power=BAKE_RULES['power'], fallback=None,
                 background=(0, 0, 0), out=None):
    """Multi-view TEXTURE of a mesh: bake_colors' rules for every texel of the atlas of (len(faces), patch) -- two triangles to a patch x patch
    cell, atlas_layout's size -- instead of every vertex; arguments as bake_colors takes them, plus faces int32 [T, 3]; fallback stays uint8
    [V, 3] per vertex and is mixed by a texel's barycentrics; background: three values 0..255 for the texels nobody owns (and the owned but
    unseen ones without a fallback).  -> dict(texture uint8 [th, tw, 3], weight float32 [th, tw], seen int32 [th, tw]: -1 where nobody owns).
    Rules: include/gnerf_hip.h, gnerf_mesh_bake_texture; shape_mi355x.bake_texture_numpy gives the same bits.  One launch, no host read:
    capturable, as bake_colors is.  out: an optional dict of preallocated outputs."""
    _require_texture()
    rules = _bake_rules(near, depth_tol, guard, min_cos, power)
    patch, background = _patch(patch), _rgb(background, 'bake')
    _require_cuda(vis, frames)
    v, f = _mesh(verts, faces)
    A, K = _cameras(mesh2cam, intrinsics, v.device)
    frames, normals, normal_mat, fallback = _bake_inputs(v, A, vis, frames, normals, normal_mat, fallback)
    _, th, tw = atlas_layout(len(f), patch)
    out = dict(out or {})
    if set(out) - set(TEXTURE_OUTPUTS):
        raise ValueError(f'bake: out holds {TEXTURE_OUTPUTS} at the most')
    for name, dtype, shape in (('texture', torch.uint8, (th, tw, 3)), ('weight', torch.float32, (th, tw)), ('seen', torch.int32, (th, tw))):
        t = out.get(name)
        if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != v.device):
            raise ValueError(f'bake: out[{name!r}] must be a contiguous {dtype} tensor of shape {shape} on the mesh\'s device')
    e = _native.ext()
    if e is not None and hasattr(e, 'mesh_bake_texture'):
        with _on_device(v.device):
            got = e.mesh_bake_texture(v, f, patch, A, K, vis, frames, normals, normal_mat, *rules, fallback, background, out.get('texture'), out.get('weight'),
                                      out.get('seen'))
        return dict(zip(TEXTURE_OUTPUTS, got))
    return _bake_texture_ctypes(v, f, patch, A, K, vis, frames, normals, normal_mat, rules, fallback, background, out.get('texture'), out.get('weight'),
                                out.get('seen'))


def _resolve_textured_ctypes(vis, v, f, A, K, texture, patch, background):
    n, h, w = vis.shape
    frame = torch.empty([n, h, w, 3], dtype=torch.uint8, device=vis.device)
    bg = (ctypes.c_ubyte * 3)(*background)
    _launch('gnerf_raster_resolve_textured', vis, _ptr(vis), _ptr(v) if len(v) else None, len(v), _ptr(f) if len(f) else None, len(f), _ptr(A), _ptr(K), n, h, w,
            _ptr(texture) if len(f) else None, patch, bg, _ptr(frame))
    return frame


@profiled('gnerf_hip::raster_resolve_textured')
def resolve_textured(vis, verts, faces, mesh2cam, intrinsics, texture, patch=8, background=(255, 255, 255)):
    """The frame of rasterize's visibility buffer with the mesh's atlas on it: resolve's sibling -> frame uint8 [n, h, w, 3], every covered
    pixel a bilinear sample of `texture` (bake_texture's uint8 [th, tw, 3], of the same faces and patch) at the point of its triangle's patch
    that the pixel's perspective-correct barycentrics name, unlit; background: three values 0..255 for the empty pixels.  Rules:
    include/gnerf_hip.h, gnerf_raster_resolve_textured; shape_mi355x.resolve_textured_numpy gives the same bits."""
    _require_texture()
    patch, background = _patch(patch), _rgb(background, 'raster')
    v, f = _mesh(verts, faces)
    A, K = _cameras(mesh2cam, intrinsics, v.device)
    _require_cuda(vis, texture)
    if vis.dtype != torch.int64 or vis.ndim != 3 or vis.shape[0] != len(A) or not vis.is_contiguous() or vis.device != v.device:
        raise ValueError('raster: vis must be rasterize\'s int64 [n_views, h, w] tensor')
    _, th, tw = atlas_layout(len(f), patch)
    if texture.dtype != torch.uint8 or tuple(texture.shape) != (th, tw, 3) or texture.device != v.device:
        raise ValueError(f'raster: texture must be the uint8 [{th}, {tw}, 3] atlas of this mesh and patch, on the mesh\'s device')
    texture = texture.detach().contiguous()
    e = _native.ext()
    if e is not None and hasattr(e, 'raster_resolve_textured'):
        with _on_device(v.device):
            return e.raster_resolve_textured(vis, v, f, A, K, texture, patch, background)
    return _resolve_textured_ctypes(vis, v, f, A, K, texture, patch, background)
