"""Marching cubes on the density volume (csrc/mesh.hip) the cleaning of its meshes (csrc/mesh_clean.hip): components, compaction, smoothing, and
their simplification (csrc/mesh_simplify.hip): vertex clustering with quadrics, and the bookkeeping of the narrow-band volume (csrc/mesh_band.hip)."""

import ctypes

import torch

from . import _native
from ._native import _check, _launch, _on_device, _ptr, _require_cuda, load, profiled


def _marching_cubes_volume(volume):
    _require_cuda(volume)
    vol = volume.detach()
    if vol.ndim != 3 or min(vol.shape) < 2:
        raise ValueError(f'marching_cubes: volume must be [D0, D1, D2] with every D >= 2, got {tuple(vol.shape)}')
    if vol.numel() >= 2 ** 31:
        raise ValueError('marching_cubes: the volume must have fewer than 2^31 points')
    return vol if (vol.dtype == torch.float32 and vol.is_contiguous()) else vol.to(torch.float32).contiguous()


def _marching_cubes_result(verts, faces, counts):
    n_verts, n_faces, n_bad = (int(c) for c in counts)
    if n_bad:
        raise ValueError(f'marching_cubes: the volume holds {n_bad} non-finite value(s)')
    if n_verts >= 2 ** 31:
        raise ValueError(f'marching_cubes: {n_verts} vertices do not fit int32 face indices')
    return verts, faces


def _marching_cubes_ctypes(vol, level):
    """The ctypes route of marching_cubes (vol: what _marching_cubes_volume returns)."""
    d0, d1, d2 = vol.shape
    dev = vol.device
    nbytes = ctypes.c_size_t()
    _check(load().gnerf_marching_cubes_workspace_bytes(d0, d1, d2, ctypes.byref(nbytes)), 'gnerf_marching_cubes_workspace_bytes')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    _launch('gnerf_marching_cubes_count', vol, _ptr(vol), d0, d1, d2, float(level), _ptr(ws), _ptr(counts))
    host = counts.cpu()                                                      # the op's one synchronisation
    n_verts, n_faces, n_bad = (int(c) for c in host)
    emit = n_bad == 0 and 0 < n_verts < 2 ** 31
    verts = torch.empty([n_verts if emit else 0, 3], dtype=torch.float32, device=dev)
    faces = torch.empty([n_faces if emit else 0, 3], dtype=torch.int32, device=dev)
    if emit:
        _launch('gnerf_marching_cubes_emit', vol, _ptr(vol), d0, d1, d2, float(level), _ptr(ws), _ptr(verts), _ptr(faces) if n_faces else None)
    return verts, faces, host


@profiled('gnerf_hip::marching_cubes')
def marching_cubes(volume, level):
    """Triangle mesh of {v > level} of a CUDA volume [D0, D1, D2] (float32; other dtypes are converted) on the gfx950 kernel ->
    (verts float32 [V, 3] in index space, faces int32 [T, 3]) on the volume's device, shapes (0, 3) when nothing crosses.  Rules, order and
    winding: include/gnerf_hip.h, gnerf_marching_cubes_*; shape_mi355x.marching_cubes_numpy gives the same bits on the CPU.  Reads three
    counts to the host between its two passes (so it is not graph-capturable).  Raises ValueError on a non-finite value."""
    vol = _marching_cubes_volume(volume)
    e = _native.ext()
    if e is not None:
        with _on_device(vol.device):
            return _marching_cubes_result(*e.marching_cubes(vol, float(level)))
    return _marching_cubes_result(*_marching_cubes_ctypes(vol, level))


# ---------------------------------------------------------------------------------------------------------------- cleaning (csrc/mesh_clean.hip)
_MESH_CLEAN_SYMBOLS = ('gnerf_mesh_workspace_bytes', 'gnerf_mesh_components', 'gnerf_mesh_compact_count', 'gnerf_mesh_compact_emit', 'gnerf_mesh_smooth')
MESH_SMOOTH_MAX_FACES = 2 ** 32 // 6 - 1            # gnerf_mesh_smooth addresses its 6 T row entries with 32 bits


def mesh_clean_available():
    """Whether the loaded library has the mesh-cleaning kernels (a version-15 library built before them does not)."""
    return all(hasattr(load(), name) for name in _MESH_CLEAN_SYMBOLS)


def _require_mesh_clean():
    if not mesh_clean_available():
        raise RuntimeError('gnerf_hip: this libgnerf_hip.so was built without the mesh-cleaning kernels (gnerf_mesh_*): rebuild it (csrc/build.sh)')


def _faces_i32(faces, what):
    _require_cuda(faces)
    f = faces.detach()
    if f.numel() % 3 != 0:
        raise ValueError(f'{what}: faces has shape {tuple(f.shape)}')
    f = f.reshape(-1, 3)
    return f if (f.dtype == torch.int32 and f.is_contiguous()) else f.to(torch.int32).contiguous()


def _verts_f32(verts, what):
    _require_cuda(verts)
    v = verts.detach()
    if v.numel() % 3 != 0:
        raise ValueError(f'{what}: verts has shape {tuple(v.shape)}')
    v = v.reshape(-1, 3)
    return v if (v.dtype == torch.float32 and v.is_contiguous()) else v.to(torch.float32).contiguous()


def _per_vertex(t, n_verts, dtype, dev, what, name):
    _require_cuda(t)
    t = t.detach().reshape(-1)
    if t.numel() != n_verts or t.device != dev:
        raise ValueError(f'{what}: {name} must hold one value per vertex, on the mesh\'s device')
    return t if (t.dtype == dtype and t.is_contiguous()) else t.to(dtype).contiguous()


def mesh_workspace_bytes(n_verts, n_tris):
    _require_mesh_clean()
    nbytes = ctypes.c_size_t()
    _check(load().gnerf_mesh_workspace_bytes(int(n_verts), int(n_tris), ctypes.byref(nbytes)), 'gnerf_mesh_workspace_bytes')
    return int(nbytes.value)


def _mesh_workspace(n_verts, n_tris, dev):
    return torch.empty(mesh_workspace_bytes(n_verts, n_tris), dtype=torch.uint8, device=dev)


def _mesh_components_ctypes(f, n_verts):
    """The ctypes route of mesh_components (f: int32 contiguous [T, 3] on a GPU) -> (label, faces_of, counts on the host)."""
    dev = f.device
    ws = _mesh_workspace(n_verts, len(f), dev)
    label = torch.empty(n_verts, dtype=torch.int32, device=dev)
    faces_of = torch.empty(n_verts, dtype=torch.int32, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    _launch('gnerf_mesh_components', f, _ptr(f) if len(f) else None, n_verts, len(f), _ptr(ws), _ptr(label) if n_verts else None,
            _ptr(faces_of) if n_verts else None, _ptr(counts))
    return label, faces_of, counts.cpu()


def _mesh_components_result(label, faces_of, counts):
    n_bad = int(counts[2])
    if n_bad:
        raise ValueError(f'mesh_components: {n_bad} face(s) name a vertex outside [0, {len(label)})')
    return label, faces_of, counts


@profiled('gnerf_hip::mesh_components')
def mesh_components(faces, n_verts):
    """Connected components of a mesh's vertices under its faces (CUDA int32 [T, 3]; n_verts = V) on the gfx950 union-find kernels ->
    (label int32 [V]: the smallest vertex index of each vertex's component, faces_of int32 [V]: faces per label, counts int64 [3] on the host:
    components with a face, vertices in no face, faces out of range).  Rules: include/gnerf_hip.h, gnerf_mesh_*;
    shape_mi355x.mesh_components_numpy gives the same bits.  Raises ValueError when a face names a vertex outside [0, V) (reads the counts)."""
    _require_mesh_clean()
    f = _faces_i32(faces, 'mesh_components')
    n_verts = int(n_verts)
    if not 0 <= n_verts < 2 ** 31:
        raise ValueError(f'mesh_components: n_verts must be in [0, 2^31), got {n_verts}')
    e = _native.ext()
    if e is not None and hasattr(e, 'mesh_components'):
        with _on_device(f.device):
            return _mesh_components_result(*e.mesh_components(f, n_verts))
    return _mesh_components_result(*_mesh_components_ctypes(f, n_verts))


def _mesh_compact_ctypes(v, f, label, faces_of, keep):
    """The ctypes route of mesh_compact (arguments as mesh_compact prepares them) -> (verts', faces', src_vertex, counts on the host)."""
    dev, nv, nt = v.device, len(v), len(f)
    ws = _mesh_workspace(nv, nt, dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    mesh = (_ptr(f) if nt else None, nv, nt, _ptr(label) if nv else None, _ptr(faces_of) if nv else None, _ptr(keep) if nv else None, _ptr(ws))
    _launch('gnerf_mesh_compact_count', v, *mesh, _ptr(counts))
    host = counts.cpu()                                                      # the op's one synchronisation
    kv, kt = (int(c) for c in host)
    out_v = torch.empty([kv, 3], dtype=torch.float32, device=dev)
    out_f = torch.empty([kt, 3], dtype=torch.int32, device=dev)
    src = torch.empty(kv, dtype=torch.int32, device=dev)
    if kv:
        _launch('gnerf_mesh_compact_emit', v, _ptr(v), *mesh, _ptr(out_v), _ptr(out_f) if kt else None, _ptr(src))
    return out_v, out_f, src, host


@profiled('gnerf_hip::mesh_compact')
def mesh_compact(verts, faces, label, faces_of, keep):
    """The mesh of the kept components: verts float32 [V, 3], faces int32 [T, 3], mesh_components' label and faces_of, and keep (bool / uint8
    [V], INDEXED BY LABEL), all CUDA -> (verts' [V', 3], faces' [T', 3] with remapped ids, src_vertex int32 [V']: the old index of every new
    vertex).  Order is stable, vertices in no face are dropped, and with everything kept the mesh comes back bit for bit (include/gnerf_hip.h,
    gnerf_mesh_compact_*; shape_mi355x.mesh_compact_numpy gives the same bits).  Reads two counts to the host between its passes (not
    graph-capturable)."""
    _require_mesh_clean()
    v, f = _verts_f32(verts, 'mesh_compact'), _faces_i32(faces, 'mesh_compact')
    if f.device != v.device:
        raise RuntimeError('mesh_compact: verts and faces must be on one device')
    label = _per_vertex(label, len(v), torch.int32, v.device, 'mesh_compact', 'label')
    faces_of = _per_vertex(faces_of, len(v), torch.int32, v.device, 'mesh_compact', 'faces_of')
    keep = _per_vertex(keep, len(v), torch.uint8, v.device, 'mesh_compact', 'keep')
    e = _native.ext()
    if e is not None and hasattr(e, 'mesh_compact'):
        with _on_device(v.device):
            return tuple(e.mesh_compact(v, f, label, faces_of, keep)[:3])
    return _mesh_compact_ctypes(v, f, label, faces_of, keep)[:3]


def _mesh_smooth_ctypes(v, f, iterations, lam, mu, pin_boundary):
    """The ctypes route of mesh_smooth (arguments as mesh_smooth prepares them)."""
    ws = _mesh_workspace(len(v), len(f), v.device)
    out = torch.empty_like(v)
    _launch('gnerf_mesh_smooth', v, _ptr(v) if len(v) else None, len(v), _ptr(f) if len(f) else None, len(f), iterations, lam, mu, int(pin_boundary),
            _ptr(ws), _ptr(out) if len(v) else None)
    return out


@profiled('gnerf_hip::mesh_smooth')
def mesh_smooth(verts, faces, iterations, lam=0.5, mu=-0.53, pin_boundary=True):
    """Taubin smoothing with uniform weights of verts float32 [V, 3] under faces int32 [T, 3] (CUDA): `iterations` times a half-step with lam,
    then one with mu -> the new positions [V, 3].  pin_boundary keeps vertices on boundary or non-manifold edges in place.  Rules:
    include/gnerf_hip.h, gnerf_mesh_smooth; shape_mi355x.mesh_smooth_numpy gives the same bits.  No host read: capturable."""
    _require_mesh_clean()
    v, f = _verts_f32(verts, 'mesh_smooth'), _faces_i32(faces, 'mesh_smooth')
    if f.device != v.device:
        raise RuntimeError('mesh_smooth: verts and faces must be on one device')
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f'mesh_smooth: iterations must be >= 0, got {iterations}')
    if len(f) > MESH_SMOOTH_MAX_FACES:
        raise ValueError(f'mesh_smooth: more than {MESH_SMOOTH_MAX_FACES} faces')
    e = _native.ext()
    if e is not None and hasattr(e, 'mesh_smooth'):
        with _on_device(v.device):
            return e.mesh_smooth(v, f, iterations, float(lam), float(mu), bool(pin_boundary))
    return _mesh_smooth_ctypes(v, f, iterations, float(lam), float(mu), bool(pin_boundary))


# ---------------------------------------------------------------------------------------------------------------- flip guard (csrc/mesh_clean.hip)
def mesh_flip_guard_available():
    """Whether the loaded library has the flip guard (a version-15 library built before it does not)."""
    return hasattr(load(), 'gnerf_mesh_flip_guard')


def _mesh_flip_guard_ctypes(v0, v1, f, status, rounds):
    """The ctypes route of mesh_flip_guard (arguments as mesh_flip_guard prepares them)."""
    nv, nt, dev = len(v0), len(f), v0.device
    out = torch.empty_like(v0)
    st = status.clone()
    counts = torch.empty(rounds + 1, dtype=torch.int32, device=dev)
    _launch('gnerf_mesh_flip_guard', v0, _ptr(v0) if nv else None, _ptr(v1) if nv else None, _ptr(f) if nt else None, nv, nt, rounds,
            _ptr(out) if nv else None, _ptr(st) if nv else None, _ptr(counts))
    return out, st, counts


@profiled('gnerf_hip::mesh_flip_guard')
def mesh_flip_guard(verts_in, verts_moved, faces, status=None, rounds=4):
    """Set back the vertices of every face that a move of the vertices turned over: verts_in and verts_moved float32 [V, 3], faces int32
    [T, 3], status uint8 [V] (the projection's 0 / 1 / 2; None: zeros), all CUDA -> (verts_out [V, 3]: verts_moved with the vertices of
    flipped faces back at verts_in, status' [V]: 3 for those, counts int32 [rounds + 1] ON THE DEVICE: faces flipped at the start of each of
    the `rounds` rounds, then those left).  Rules: include/gnerf_hip.h, gnerf_mesh_flip_guard; shape_mi355x.mesh_flip_guard_numpy gives the
    same bits.  No host read: capturable."""
    if not mesh_flip_guard_available():
        raise RuntimeError('gnerf_hip: this libgnerf_hip.so was built without gnerf_mesh_flip_guard: rebuild it (csrc/build.sh)')
    v0, v1, f = _verts_f32(verts_in, 'mesh_flip_guard'), _verts_f32(verts_moved, 'mesh_flip_guard'), _faces_i32(faces, 'mesh_flip_guard')
    if v1.shape != v0.shape or v1.device != v0.device or f.device != v0.device:
        raise ValueError('mesh_flip_guard: verts_in, verts_moved and faces must describe one mesh on one device')
    rounds = int(rounds)
    if not 1 <= rounds < 2 ** 31 - 1:
        raise ValueError(f'mesh_flip_guard: rounds must be >= 1, got {rounds}')
    status = torch.zeros(len(v0), dtype=torch.uint8, device=v0.device) if status is None else _per_vertex(status, len(v0), torch.uint8, v0.device,
                                                                                                        'mesh_flip_guard', 'status')
    e = _native.ext()
    if e is not None and hasattr(e, 'mesh_flip_guard'):
        with _on_device(v0.device):
            return tuple(e.mesh_flip_guard(v0, v1, f, status, rounds))
    return _mesh_flip_guard_ctypes(v0, v1, f, status, rounds)


# ---------------------------------------------------------------------------------------------------------------- simplification (csrc/mesh_simplify.hip)
_MESH_SIMPLIFY_SYMBOLS = ('gnerf_mesh_simplify_workspace_bytes', 'gnerf_mesh_simplify_count', 'gnerf_mesh_simplify_emit')


def mesh_simplify_available():
    """Whether the loaded library has the mesh-simplification kernels (a version-15 library built before them does not)."""
    return all(hasattr(load(), name) for name in _MESH_SIMPLIFY_SYMBOLS)


def _require_mesh_simplify():
    if not mesh_simplify_available():
        raise RuntimeError('gnerf_hip: this libgnerf_hip.so was built without the mesh-simplification kernels (gnerf_mesh_simplify_*): rebuild it (csrc/build.sh)')


def mesh_simplify_workspace_bytes(n_verts, n_tris):
    _require_mesh_simplify()
    nbytes = ctypes.c_size_t()
    _check(load().gnerf_mesh_simplify_workspace_bytes(int(n_verts), int(n_tris), ctypes.byref(nbytes)), 'gnerf_mesh_simplify_workspace_bytes')
    return int(nbytes.value)


def _mesh_simplify_args(verts, faces, cell, origin, what):
    """(verts float32 [V, 3], faces int32 [T, 3], cell and origin as Python floats that are exact C floats)."""
    _require_mesh_simplify()
    v, f = _verts_f32(verts, what), _faces_i32(faces, what)
    if f.device != v.device:
        raise RuntimeError(f'{what}: verts and faces must be on one device')
    cell = float(torch.tensor(float(cell), dtype=torch.float32))
    if not (0 < cell < float('inf')):
        raise ValueError(f'{what}: cell must be a finite float32 > 0, got {cell}')
    origin = [float(x) for x in torch.as_tensor(origin, dtype=torch.float64).reshape(-1).to(torch.float32).cpu()]
    if len(origin) != 3 or not all(abs(x) < float('inf') for x in origin):
        raise ValueError(f'{what}: origin must be three finite floats')
    return v, f, cell, origin


def _mesh_simplify_count_launch(v, f, cell, origin):
    """gnerf_mesh_simplify_count through ctypes -> (the mesh's arguments for the emit call, workspace, counts on the device)."""
    dev, nv, nt = v.device, len(v), len(f)
    ws = torch.empty(mesh_simplify_workspace_bytes(nv, nt), dtype=torch.uint8, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    mesh = (_ptr(v) if nv else None, _ptr(f) if nt else None, nv, nt, cell, (ctypes.c_float * 3)(*origin), _ptr(ws))
    _launch('gnerf_mesh_simplify_count', v, *mesh, _ptr(counts))
    return mesh, ws, counts


def _mesh_simplify_ctypes(v, f, cell, origin):
    """The ctypes route of mesh_simplify (arguments as _mesh_simplify_args prepares them) -> (verts', faces', src_vertex, vertex_map, counts on
    the host)."""
    dev = v.device
    mesh, ws, counts = _mesh_simplify_count_launch(v, f, cell, origin)
    host = counts.cpu()                                                      # the op's one synchronisation
    kv, kt = int(host[0]), int(host[1])
    out_v = torch.empty([kv, 3], dtype=torch.float32, device=dev)
    out_f = torch.empty([kt, 3], dtype=torch.int32, device=dev)
    src = torch.empty(kv, dtype=torch.int32, device=dev)
    vmap = torch.empty(len(v), dtype=torch.int32, device=dev) if kv else torch.full([len(v)], -1, dtype=torch.int32, device=dev)
    if kv:
        _launch('gnerf_mesh_simplify_emit', v, *mesh, _ptr(out_v), _ptr(out_f) if kt else None, _ptr(src), _ptr(vmap))
    return out_v, out_f, src, vmap, host


def _mesh_simplify_result(*result):
    counts = result[-1]
    if int(counts[6]):
        raise RuntimeError('mesh_simplify: internal error (a hash table of the kernels ran full)')
    return result if len(result) > 1 else counts


@profiled('gnerf_hip::mesh_simplify_count')
def mesh_simplify_count(verts, faces, cell, origin):
    """The counts of mesh_simplify alone (tables, ids and face grouping, no quadrics): int64 [8] on the host = V', T', invalid faces, collapsed
    faces, faces absorbed by grouping, groups with |sigma| >= 2, internal error, 0.  What a search for a cell calls."""
    v, f, cell, origin = _mesh_simplify_args(verts, faces, cell, origin, 'mesh_simplify_count')
    e = _native.ext()
    if e is not None and hasattr(e, 'mesh_simplify_count'):
        with _on_device(v.device):
            return _mesh_simplify_result(e.mesh_simplify_count(v, f, cell, origin))
    return _mesh_simplify_result(_mesh_simplify_count_launch(v, f, cell, origin)[2].cpu())


@profiled('gnerf_hip::mesh_simplify')
def mesh_simplify(verts, faces, cell, origin):
    """Vertex clustering with quadrics on the gfx950 kernels: verts float32 [V, 3], faces int32 [T, 3] (CUDA), cell (a float > 0: the edge of
    the grid's cells) and origin (three floats: the grid's corner) -> (verts' [V', 3]: one vertex per occupied cell, at the minimum of its
    cluster's quadric inside the cell; faces' [T', 3]; src_vertex int32 [V']: the old index of every new vertex's representative; vertex_map
    int32 [V]: the new id of every old vertex or -1; counts int64 [8] on the host, as mesh_simplify_count's).  Rules: include/gnerf_hip.h,
    gnerf_mesh_simplify_*; shape_mi355x.mesh_simplify_numpy gives the same bits.  Reads the counts to the host between its two passes (not
    graph-capturable; each pass alone is)."""
    v, f, cell, origin = _mesh_simplify_args(verts, faces, cell, origin, 'mesh_simplify')
    e = _native.ext()
    if e is not None and hasattr(e, 'mesh_simplify'):
        with _on_device(v.device):
            return _mesh_simplify_result(*e.mesh_simplify(v, f, cell, origin))
    return _mesh_simplify_result(*_mesh_simplify_ctypes(v, f, cell, origin))


# ---------------------------------------------------------------------------------------------------------------- narrow band (csrc/mesh_band.hip)
_BAND_SYMBOLS = ('gnerf_band_workspace_bytes', 'gnerf_band_seed', 'gnerf_band_points_count', 'gnerf_band_points_emit', 'gnerf_band_grow', 'gnerf_band_fill')
BAND_BRICKS = (2, 4, 8, 16)


def band_available():
    """Whether the loaded library has the narrow-band kernels (a version-15 library built before them does not)."""
    return all(hasattr(load(), name) for name in _BAND_SYMBOLS)


def band_workspace_bytes(n, s):
    nbytes = ctypes.c_size_t()
    _check(load().gnerf_band_workspace_bytes(int(n), int(s), ctypes.byref(nbytes)), 'gnerf_band_workspace_bytes')
    return int(nbytes.value)


def _band_keep(n, keep):
    keep = [(0, n)] * 3 if keep is None else [(int(lo), int(hi)) for lo, hi in keep]
    if len(keep) != 3:
        raise ValueError('band: keep must be three (lo, hi) index ranges')
    return [min(max(x, 0), n) for pair in keep for x in pair]


def _band_tensor(t, dtype, numel, what, name):
    _require_cuda(t)
    if t.dtype != dtype or not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f'{what}: {name} must be a contiguous {dtype} CUDA tensor of {numel} values')
    return t


def _band_ext(binding):
    return None if binding == 'ctypes' else _native.ext()


@profiled('gnerf_hip::band_seed')
def band_seed(volume, n, s, level, keep, state, workspace, count, binding=None):
    """gnerf_band_seed: state (uint8 [nb^3], written) = 2 for the bricks whose corners straddle `level`, count (int64 [1] on the device, written)
    = their number.  volume float32 [n^3] with the coarse points evaluated; keep: three (lo, hi) or None.  binding='ctypes' forces that route."""
    e = _band_ext(binding)
    if e is not None and hasattr(e, 'band_seed'):
        with _on_device(volume.device):
            return e.band_seed(volume, n, s, float(level), _band_keep(n, keep), state, workspace, count)
    _launch('gnerf_band_seed', volume, _ptr(volume), n, s, float(level), (ctypes.c_int * 6)(*_band_keep(n, keep)), _ptr(state), _ptr(workspace), _ptr(count))


@profiled('gnerf_hip::band_points_count')
def band_points_count(state, n, s, workspace, count, binding=None):
    """gnerf_band_points_count: count (int64 [1] on the device, written) = the length of the index list of the bricks of state 2.  Reads the
    list of those bricks that band_seed / band_grow left in `workspace`: it follows one of them on the same state."""
    e = _band_ext(binding)
    if e is not None and hasattr(e, 'band_points_count'):
        with _on_device(state.device):
            return e.band_points_count(state, n, s, workspace, count)
    _launch('gnerf_band_points_count', state, _ptr(state), n, s, _ptr(workspace), _ptr(count))


@profiled('gnerf_hip::band_points_emit')
def band_points_emit(state, n, s, workspace, m, binding=None):
    """gnerf_band_points_emit after band_points_count on the same state and workspace, m the count it gave -> the index list int32 [m]."""
    index = torch.empty(int(m), dtype=torch.int32, device=state.device)
    e = _band_ext(binding)
    if e is not None and hasattr(e, 'band_points_emit'):
        with _on_device(state.device):
            e.band_points_emit(state, n, s, workspace, index)
    else:
        _launch('gnerf_band_points_emit', state, _ptr(state), n, s, _ptr(workspace), _ptr(index) if m else None, int(m))
    return index


@profiled('gnerf_hip::band_grow')
def band_grow(volume, n, s, level, keep, state, workspace, count, binding=None):
    """gnerf_band_grow: the bricks of state 2 (their points evaluated in `volume`) name the neighbours their mixed faces lead to, the round
    closes (2 -> 1, named -> 2) in `state`, count (int64 [1] on the device, written) = the new bricks."""
    e = _band_ext(binding)
    if e is not None and hasattr(e, 'band_grow'):
        with _on_device(volume.device):
            return e.band_grow(volume, n, s, float(level), _band_keep(n, keep), state, workspace, count)
    _launch('gnerf_band_grow', volume, _ptr(volume), n, s, float(level), (ctypes.c_int * 6)(*_band_keep(n, keep)), _ptr(state), _ptr(workspace), _ptr(count))


@profiled('gnerf_hip::band_fill')
def band_fill(volume, n, s, keep, state, binding=None):
    """gnerf_band_fill, in place: every point of `volume` that is neither coarse nor in an active brick takes its coarse corner's effective value."""
    e = _band_ext(binding)
    if e is not None and hasattr(e, 'band_fill'):
        with _on_device(volume.device):
            return e.band_fill(volume, n, s, _band_keep(n, keep), state)
    _launch('gnerf_band_fill', volume, _ptr(volume), n, s, (ctypes.c_int * 6)(*_band_keep(n, keep)), _ptr(state))


class BandVolume:
    """The device side of shape_mi355x.band_volume for one volume (float32 [n^3] on a GPU, evaluated in place by the caller): the brick states,
    the workspace and the two counts, and the stages as the driver calls them.  seed() and grow() also count the next round's points, so the
    host reads (new bricks, points) together: one read per round."""

    def __init__(self, volume, n, s, level, keep=None, binding=None):
        if not band_available():
            raise RuntimeError('gnerf_hip: this libgnerf_hip.so was built without the narrow-band kernels (gnerf_band_*): rebuild it (csrc/build.sh)')
        self.n, self.s, self.level, self.keep, self.binding = int(n), int(s), float(level), keep, binding
        if self.s not in BAND_BRICKS:
            raise ValueError(f'band: the brick edge must be one of {BAND_BRICKS}, got {s}')
        if self.n < 2 or self.n ** 3 >= 2 ** 31:
            raise ValueError(f'band: n must be >= 2 with n^3 < 2^31, got {n}')
        self.volume = _band_tensor(volume, torch.float32, self.n ** 3, 'band', 'volume')
        dev = volume.device
        self.nb = -(-(self.n - 1) // self.s)
        self.state = torch.empty(self.nb ** 3, dtype=torch.uint8, device=dev)
        self.workspace = torch.empty(band_workspace_bytes(self.n, self.s), dtype=torch.uint8, device=dev)
        self.counts = torch.empty(2, dtype=torch.int64, device=dev)
        self.points_next = 0

    def _read(self):
        band_points_count(self.state, self.n, self.s, self.workspace, self.counts[1:], self.binding)
        new, self.points_next = (int(c) for c in self.counts.cpu())           # the round's one synchronisation
        return new

    def seed(self):
        """-> the seeded bricks."""
        band_seed(self.volume, self.n, self.s, self.level, self.keep, self.state, self.workspace, self.counts[:1], self.binding)
        return self._read()

    def points(self):
        """-> the index list of the bricks that the last seed() / grow() made new."""
        return band_points_emit(self.state, self.n, self.s, self.workspace, self.points_next, self.binding)

    def grow(self):
        """-> the bricks this round's growth made new."""
        band_grow(self.volume, self.n, self.s, self.level, self.keep, self.state, self.workspace, self.counts[:1], self.binding)
        return self._read()

    def fill(self):
        band_fill(self.volume, self.n, self.s, self.keep, self.state, self.binding)


# ---------------------------------------------------------------------------------------------------------------- band mesh (csrc/mesh_band_cubes.hip)
_BAND_MESH_SYMBOLS = ('gnerf_band_mesh_workspace_bytes', 'gnerf_band_mesh_count', 'gnerf_band_mesh_emit')


def band_mesh_available():
    """Whether the loaded library has the brick-wise marching cubes of the narrow band (a version-15 library built before it does not)."""
    return all(hasattr(load(), name) for name in _BAND_MESH_SYMBOLS)


def band_mesh_workspace_bytes(n, s, active):
    nbytes = ctypes.c_size_t()
    _check(load().gnerf_band_mesh_workspace_bytes(int(n), int(s), int(active), ctypes.byref(nbytes)), 'gnerf_band_mesh_workspace_bytes')
    return int(nbytes.value)


def _band_mesh_ctypes(vol, state, n, s, level, keep, perm, flip, active):
    """The ctypes route of band_marching_cubes (arguments as it prepares them) -> (verts, faces, counts on the host)."""
    dev = vol.device
    ws = torch.empty(band_mesh_workspace_bytes(n, s, active), dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    view = (n, s, float(level), (ctypes.c_int * 6)(*keep), (ctypes.c_int * 3)(*perm), (ctypes.c_int * 3)(*flip), active, _ptr(ws))
    _launch('gnerf_band_mesh_count', vol, _ptr(vol), _ptr(state), *view, _ptr(counts))
    host = counts.cpu()                                                      # the op's one synchronisation
    n_verts, n_faces, n_bad = (int(c) for c in host[:3])
    emit = n_bad == 0 and 0 < n_verts < 2 ** 31
    verts = torch.empty([n_verts if emit else 0, 3], dtype=torch.float32, device=dev)
    faces = torch.empty([n_faces if emit else 0, 3], dtype=torch.int32, device=dev)
    if emit:
        _launch('gnerf_band_mesh_emit', vol, _ptr(vol), _ptr(state), *view, _ptr(verts), _ptr(faces) if n_faces else None)
    return verts, faces, host


@profiled('gnerf_hip::band_marching_cubes')
def band_marching_cubes(volume, state, n, s, level, keep=None, perm=(0, 1, 2), flip=(False, False, False), binding=None, active=None,
                        return_counts=False):
    """Triangle mesh of {e > level} over the ACTIVE BRICKS of a narrow band, in a view of the lattice: volume float32 [n^3] (CUDA) as the
    band's rounds left it -- no band_fill; nothing outside the active bricks' closed point ranges is read --, state uint8 [nb^3] of 0 / 1, keep
    as band_seed takes it, perm a permutation of (0, 1, 2) and flip a flag per LATTICE axis: mesh coordinate m_k = l_perm[k], mirrored where
    that axis is flipped -> (verts float32 [V, 3] in mesh coordinates, faces int32 [T, 3]): marching_cubes' of the filled, cropped, flipped and
    permuted volume, bit for bit and in the same order (include/gnerf_hip.h, gnerf_band_mesh_*; shape_mi355x.band_marching_cubes_numpy gives the
    same bits).  active: the number of active bricks when the caller knows it (the band driver does); None reads state.sum() to the host first.
    Reads its counts to the host between its two passes, like marching_cubes.  return_counts: also the counts int64 [4] on the host (V, T,
    non-finite effective values among the visited points, visited points), and a non-finite value empties the mesh instead of raising.
    binding='ctypes' forces that route."""
    if not band_mesh_available():
        raise RuntimeError('gnerf_hip: this libgnerf_hip.so was built without the band-mesh kernels (gnerf_band_mesh_*): rebuild it (csrc/build.sh)')
    n, s = int(n), int(s)
    if s not in BAND_BRICKS:
        raise ValueError(f'band_marching_cubes: the brick edge must be one of {BAND_BRICKS}, got {s}')
    if n < 2 or n ** 3 >= 2 ** 31:
        raise ValueError(f'band_marching_cubes: n must be >= 2 with n^3 < 2^31, got {n}')
    perm, flip = [int(a) for a in perm], [int(bool(f)) for f in flip]
    if sorted(perm) != [0, 1, 2] or len(flip) != 3:
        raise ValueError(f'band_marching_cubes: perm must be a permutation of (0, 1, 2) and flip one flag per lattice axis, got {perm}, {flip}')
    nb = -(-(n - 1) // s)
    vol = _band_tensor(volume.detach().reshape(-1), torch.float32, n ** 3, 'band_marching_cubes', 'volume')
    state = _band_tensor(state.reshape(-1), torch.uint8, nb ** 3, 'band_marching_cubes', 'state')
    if state.device != vol.device:
        raise ValueError('band_marching_cubes: volume and state must be on one device')
    active = int(state.sum()) if active is None else int(active)
    if not 0 <= active <= nb ** 3:
        raise ValueError(f'band_marching_cubes: active must be a number of bricks in [0, {nb ** 3}], got {active}')
    keep = _band_keep(n, keep)
    e = _band_ext(binding)
    if e is not None and hasattr(e, 'band_marching_cubes'):
        with _on_device(vol.device):
            verts, faces, counts = e.band_marching_cubes(vol, state, n, s, float(level), keep, perm, flip, active)
    else:
        verts, faces, counts = _band_mesh_ctypes(vol, state, n, s, level, keep, perm, flip, active)
    n_verts, _, n_bad, _ = (int(c) for c in counts)
    if n_bad == -1:
        raise ValueError(f'band_marching_cubes: state holds more active bricks than active = {active}')
    if n_bad == -2:
        raise ValueError('band_marching_cubes: every brick state must be 0 or 1 (the band\'s rounds have not ended)')
    if n_verts >= 2 ** 31:
        raise ValueError(f'band_marching_cubes: {n_verts} vertices do not fit int32 face indices')
    if return_counts:
        return verts, faces, counts
    if n_bad:
        raise ValueError(f'band_marching_cubes: {n_bad} visited point(s) hold a non-finite value')
    return verts, faces
