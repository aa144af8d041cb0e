"""Marching cubes on the density volume (csrc/marching_cubes.hip)."""

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
