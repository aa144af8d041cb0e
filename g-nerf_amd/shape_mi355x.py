#!/usr/bin/env python3
"""Counterpart of G-NeRF's shape_utils.py (g_nerf/shape_utils.py:40-123): triangle meshes from a density volume, `.ply` output and
the `.mrc` volumes gen_videos.py --shapes writes -- without skimage, plyfile, mrcfile or trimesh.

Marching cubes here is one algorithm with two implementations that give the same bits:
  * a CUDA tensor goes to the gfx950 kernel (csrc/mesh.hip through gnerf_hip.marching_cubes);
  * a CPU tensor or a numpy array goes to the vectorised numpy port below (the CPU path and the tests' reference).
The rules both follow (include/gnerf_hip.h, gnerf_marching_cubes_*):
  * a lattice point is INSIDE iff v > level (strict);
  * one vertex per lattice edge p -> p + e_a (a = 0, 1, 2) whose endpoints disagree, at coord_a = i_a + t,
    t = (level - v_p) / (v_{p+e_a} - v_p) in float32 (correctly rounded division, no contraction), index space;
  * vertices in lexicographic order of (linear index of p, a); faces int32 in order of the cell's lower corner, then the table's order;
  * the right-hand normal of a face points from inside to outside (outward, for a density);
  * one 256-case table made by case_table() from a rule that looks only at a cube face's four corners (crack-free by construction):
    the crossed edges of a face pair into segments, an ambiguous face (inside corners on a diagonal) cuts each inside corner off on
    its own; the segments of a cube form disjoint cycles, each fan-triangulated from its lowest edge whose fan draws no diagonal
    on a cube face (a neighbouring cell could draw the same one).  csrc/mesh_tables.h is
    case_table_header()'s output.

render_mesh draws such a mesh from the renderer's cameras on the renderer's pixel grid (triangle ids, depth as image_depth measures it,
normals, shaded frames): CUDA tensors go to the rasteriser kernels (csrc/raster.hip through gnerf_hip.rasterize / resolve), numpy arrays to
rasterize_numpy / resolve_numpy below, which state the arithmetic (include/gnerf_hip.h, gnerf_raster_*) and give the same bits.

bake_mesh_colors goes the other way: it colours such a mesh's vertices from frames of it (the orbit's) and their cameras, through render_mesh's
visibility buffers.  CUDA tensors go to gnerf_hip.rasterize / bake_colors (csrc/raster.hip), numpy arrays to rasterize_numpy /
bake_colors_numpy below (include/gnerf_hip.h, gnerf_mesh_bake_colors): the same bits.

clean_mesh edits such a mesh between extraction and its consumers: connected components, the selection of the large ones, compaction and
Taubin smoothing.  CUDA tensors go to csrc/mesh_clean.hip (gnerf_hip.mesh_components / mesh_compact / mesh_smooth), numpy arrays to
mesh_components_numpy / mesh_select / mesh_compact_numpy / mesh_smooth_numpy below (include/gnerf_hip.h, gnerf_mesh_*): the same bits.

simplify_mesh shrinks such a mesh: vertex clustering on a uniform grid with a quadric-error representative per cell, for a given cell or a
target face count.  CUDA tensors go to csrc/mesh_simplify.hip (gnerf_hip.mesh_simplify / mesh_simplify_count), numpy arrays to
mesh_simplify_numpy below (include/gnerf_hip.h, gnerf_mesh_simplify_*): the same bits.

band_volume makes the volume itself cheaper: it evaluates the density field only in bricks that the level set runs through (surface following
from seeded bricks), and the mesh of its volume is the dense volume's in the same order, minus whole components thinner than a brick.  On a
CUDA device the bookkeeping runs on csrc/mesh_band.hip (gnerf_hip.BandVolume), anywhere else on band_volume_numpy below
(include/gnerf_hip.h, gnerf_band_*): the same brick states, index lists and volume.

band_mesh goes on from the band's rounds without the volume's fill: marching cubes over the active bricks alone, in a view of the lattice
(csrc/mesh_band_cubes.hip through gnerf_hip.band_marching_cubes; band_marching_cubes_numpy below): the mesh of band_volume's volume, bit for bit.

finish_mesh walks these stages, and those that need a generator (given as callables), in the one order both CLIs use.

CLI, as shape_utils.py's (:102-123):  python shape_mi355x.py INPUT [--level 10]   (INPUT: a .mrc / .npy file or a directory of them)
  [--mesh-keep K] [--mesh-min-faces N] [--mesh-smooth ITERS] clean the mesh first (all 0 by default: the file is the uncleaned one, byte for byte)
  [--mesh-simplify CELL] [--mesh-target-faces N] simplify it between the compaction and the smoothing (both 0 by default: nothing runs)
"""

import argparse
import collections
import glob
import os
import struct
import sys
import time
import zlib

import numpy as np


# ---------------------------------------------------------------------------------------------------------------- the two routes
# Every function below that names two implementations chooses between them here: a CUDA tensor takes the gfx950 kernels (gnerf_hip) and
# stays on its device, anything else -- a numpy array, a list, a CPU tensor -- is brought to the host as numpy and takes the ports.
def _torch():
    """torch, or None where it is not installed (the numpy route needs none)."""
    try:
        import torch
    except ImportError:                                                  # pragma: no cover - torch is part of the stack
        return None
    return torch


def is_gpu(x):
    """Whether x takes the GPU route: it is a CUDA tensor."""
    torch = sys.modules.get('torch')                                     # (a tensor in hand means torch is loaded)
    return torch is not None and isinstance(x, torch.Tensor) and x.is_cuda


def to_host(x):
    """x on the host as numpy: a tensor of any device is copied over, None stays None, anything else goes through np.asarray."""
    if x is None:
        return None
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


_MeshRoute = collections.namedtuple('_MeshRoute', 'xp rasterize resolve bake_colors components compact smooth simplify simplify_count bake_texture resolve_textured')


def _mesh_route(verts, faces):
    """The route a mesh takes, chosen once per call of render_mesh, bake_mesh_colors, bake_mesh_texture, clean_mesh, simplify_mesh and finish_mesh -> (route, verts,
    faces): the kernels and torch for CUDA tensors, left where they are; the numpy ports and numpy for anything else, brought to the host.
    route.xp is the array module: what the callers do to the arrays themselves is spelled alike in both."""
    if is_gpu(verts):
        import gnerf_hip as g
        return (_MeshRoute(_torch(), g.rasterize, g.resolve, g.bake_colors, g.mesh_components, g.mesh_compact, g.mesh_smooth, g.mesh_simplify,
                           g.mesh_simplify_count, g.bake_texture, g.resolve_textured), verts.detach().reshape(-1, 3).float(), faces)
    return (_MeshRoute(np, rasterize_numpy, resolve_numpy, bake_colors_numpy, mesh_components_numpy, mesh_compact_numpy, mesh_smooth_numpy, mesh_simplify_numpy,
                       lambda *mesh: mesh_simplify_numpy(*mesh, count_only=True), bake_texture_numpy, resolve_textured_numpy), np.asarray(to_host(verts), dtype=np.float32).reshape(-1, 3), to_host(faces))


def _on_route(x, like):
    """x (an array, a tensor or None) where `like` lives: a tensor on its device when `like` takes the GPU route, numpy on the host otherwise."""
    if x is None or not is_gpu(like):
        return to_host(x)
    torch = _torch()
    return (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x))).to(like.device)      # (a copy: x may be a read-only view)


# ---------------------------------------------------------------------------------------------------------------- the case table
# Corner c of a cell sits at offset (c >> 2 & 1, c >> 1 & 1, c & 1) along axes (0, 1, 2) from the cell's lower corner, so corners are
# numbered in the volume's linear order.  Edge (c, a) runs from corner c to c + e_a; the 12 edges are numbered in (c, a) order -- the
# order of the vertices they own.
_AXIS_BIT = (4, 2, 1)
CORNER_OFFSETS = np.array([((c >> 2) & 1, (c >> 1) & 1, c & 1) for c in range(8)], dtype=np.int64)
EDGES = [(c, a) for c in range(8) for a in range(3) if not c & _AXIS_BIT[a]]


def _cell_triangles(case):
    """Triangles (edge-id triples) of one cell case (bit c set = corner c inside)."""
    inside = [(case >> c) & 1 for c in range(8)]
    eid = {e: i for i, e in enumerate(EDGES)}
    pos = CORNER_OFFSETS.astype(np.float64)

    def crossed(e):
        c, a = EDGES[e]
        return inside[c] != inside[c | _AXIS_BIT[a]]

    def out_dir(e):                          # unit vector along edge e from its inside endpoint to its outside endpoint
        c, a = EDGES[e]
        u = np.zeros(3)
        u[a] = 1.0 if inside[c] else -1.0
        return u

    def mid(e):
        c, a = EDGES[e]
        m = pos[c].copy()
        m[a] += 0.5
        return m

    nxt = {}
    for a in range(3):                       # the six faces: corners with bit a equal to s, outward normal (2s - 1) e_a
        for s in (0, 1):
            n_f = np.zeros(3)
            n_f[a] = 1.0 if s else -1.0
            fedges = [eid[(c, b)] for c in range(8) for b in range(3)
                      if b != a and ((c >> (2 - a)) & 1) == s and (c, b) in eid]
            cut = [e for e in fedges if crossed(e)]
            if not cut:
                continue
            if len(cut) == 2:
                segs = [tuple(cut)]
            else:                            # ambiguous face: each inside corner is cut off by the two face edges that touch it
                segs = []
                for c in range(8):
                    if ((c >> (2 - a)) & 1) == s and inside[c]:
                        segs.append(tuple(e for e in cut if c in (EDGES[e][0], EDGES[e][0] | _AXIS_BIT[EDGES[e][1]])))
            for e1, e2 in segs:
                # the surface's normal in the face plane points along the edges' inside -> outside directions; the boundary of a
                # patch whose right-hand normal is N runs along N x (outward normal of the cube face)
                d = np.cross(out_dir(e1) + out_dir(e2), n_f)
                if np.dot(mid(e2) - mid(e1), d) > 0:
                    nxt[e1] = e2
                else:
                    nxt[e2] = e1

    def faces(e):                            # the two cube faces edge e lies on
        c, a = EDGES[e]
        return {(b, (c >> (2 - b)) & 1) for b in range(3) if b != a}

    def fan_stays_off_faces(cycle):          # no diagonal of the fan joins two vertices of one cube face (an ambiguous face: the
        n = len(cycle)                       # neighbouring cell could draw the same diagonal, and the edge would be used four times)
        return not any(faces(cycle[0]) & faces(cycle[i]) for i in range(2, n - 1))

    tris = []
    seen = set()
    for start in sorted(nxt):
        if start in seen:
            continue
        cycle = [start]
        seen.add(start)
        e = nxt[start]
        while e != start:
            cycle.append(e)
            seen.add(e)
            e = nxt[e]
        # fan from the lowest edge whose fan keeps its diagonals inside the cube (every case has one)
        rotations = sorted((cycle[k:] + cycle[:k] for k in range(len(cycle))), key=lambda r: r[0])
        cycle = next(r for r in rotations if fan_stays_off_faces(r))
        for i in range(1, len(cycle) - 1):
            tris.append((cycle[0], cycle[i], cycle[i + 1]))
    return tris


def case_table():
    """(tri_count uint8 [256], tri_edges uint8 [256, max_tris, 3] (unused rows 0), edges [(corner, axis)] * 12)."""
    per_case = [_cell_triangles(m) for m in range(256)]
    max_tris = max(len(t) for t in per_case)
    count = np.array([len(t) for t in per_case], dtype=np.uint8)
    table = np.zeros((256, max_tris, 3), dtype=np.uint8)
    for m, t in enumerate(per_case):
        if t:
            table[m, :len(t)] = t
    return count, table, list(EDGES)


def case_table_header():
    """The text of csrc/mesh_tables.h."""
    count, table, edges = case_table()
    max_tris = table.shape[1]
    lines = ['// csrc/mesh_tables.h -- GENERATED by shape_mi355x.case_table_header(); do not edit (tests/test_mesh_cpu.py regenerates',
             '// and compares).  Marching-cubes case table: bit c of a case = corner c inside, corner c at offset (c>>2&1, c>>1&1, c&1);',
             '// edge e = (corner, axis) runs from that corner along the axis; each triangle lists three edge ids, right-hand normal outward.',
             '#pragma once',
             '',
             f'#define GNERF_MC_MAX_TRIS {max_tris}',
             '',
             'static __constant__ const unsigned char kMcEdgeCorner[12] = {' + ', '.join(str(c) for c, _ in edges) + '};',
             'static __constant__ const unsigned char kMcEdgeAxis[12] = {' + ', '.join(str(a) for _, a in edges) + '};',
             'static __constant__ const unsigned char kMcTriCount[256] = {']
    for r in range(0, 256, 32):
        lines.append('    ' + ', '.join(str(int(v)) for v in count[r:r + 32]) + ',')
    lines.append('};')
    lines.append(f'static __constant__ const unsigned char kMcTriEdges[256][{max_tris * 3}] = {{')
    for m in range(256):
        lines.append('    {' + ', '.join(str(int(v)) for v in table[m].reshape(-1)) + '},')
    lines.append('};')
    return '\n'.join(lines) + '\n'


_TABLE = None


def _table():
    global _TABLE
    if _TABLE is None:
        count, table, edges = case_table()
        corner = np.array([c for c, _ in edges], dtype=np.int64)
        axis = np.array([a for _, a in edges], dtype=np.int64)
        _TABLE = (count.astype(np.int64), table.astype(np.int64), corner, axis)
    return _TABLE


# ---------------------------------------------------------------------------------------------------------------- marching cubes
def marching_cubes_numpy(volume, level):
    """The numpy port of the kernel: volume [D0, D1, D2] (any float dtype, converted to float32), level -> (verts float32 [V, 3] in
    index space, faces int32 [T, 3]), the kernel's vertices and faces bit for bit.  Raises ValueError on a non-finite value."""
    v = np.ascontiguousarray(np.asarray(volume), dtype=np.float32)
    if v.ndim != 3 or min(v.shape) < 2:
        raise ValueError(f'marching_cubes: volume must be [D0, D1, D2] with every D >= 2, got {tuple(v.shape)}')
    bad = int(v.size - np.count_nonzero(np.isfinite(v)))
    if bad:
        raise ValueError(f'marching_cubes: the volume holds {bad} non-finite value(s)')
    return _marching_cubes_masked(v, np.float32(level), None)


def _marching_cubes_masked(v, lev, seen):
    """Marching cubes' rules on the float32 volume v, restricted to the points of the mask `seen` (None: every point): an edge is examined iff
    both endpoints are seen, a cell iff all eight corners are; values at other points are never looked at."""
    d0, d1, d2 = v.shape
    strides = np.array([d1 * d2, d2, 1], dtype=np.int64)
    if seen is None:
        inside = v > lev
    else:
        inside = np.zeros(v.shape, dtype=bool)
        inside[seen] = v[seen] > lev
    cross = np.zeros(v.shape + (3,), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    if seen is not None:
        cross[:-1, :, :, 0] &= seen[:-1] & seen[1:]
        cross[:, :-1, :, 1] &= seen[:, :-1] & seen[:, 1:]
        cross[:, :, :-1, 2] &= seen[:, :, :-1] & seen[:, :, 1:]
    cross = cross.reshape(-1, 3)
    per_point = cross.sum(axis=1, dtype=np.int64)
    base = np.cumsum(per_point) - per_point                              # first vertex id of each point
    flat = v.reshape(-1)

    p, ax = np.nonzero(cross)                                            # C order: sorted by (point, axis)
    vp, vq = flat[p], flat[p + strides[ax]]
    t = (lev - vp) / (vq - vp)                                           # float32 throughout
    verts = np.stack([p // strides[0], (p // strides[1]) % d1, p % d2], axis=1).astype(np.float32)
    verts[np.arange(len(p)), ax] += t

    count, table, e_corner, e_axis = _table()
    case = np.zeros((d0 - 1, d1 - 1, d2 - 1), dtype=np.int64)
    whole = None if seen is None else np.ones(case.shape, dtype=bool)
    for c in range(8):
        o0, o1, o2 = CORNER_OFFSETS[c]
        case |= inside[o0:d0 - 1 + o0, o1:d1 - 1 + o1, o2:d2 - 1 + o2].astype(np.int64) << c
        if whole is not None:
            whole &= seen[o0:d0 - 1 + o0, o1:d1 - 1 + o1, o2:d2 - 1 + o2]
    case = case.reshape(-1)
    ntri = count[case] if whole is None else count[case] * whole.reshape(-1)
    cells = np.nonzero(ntri)[0]
    if len(cells) == 0:
        return verts, np.zeros((0, 3), dtype=np.int32)
    c0, rest = np.divmod(cells, (d1 - 1) * (d2 - 1))
    c1, c2 = np.divmod(rest, d2 - 1)
    lower = c0 * strides[0] + c1 * strides[1] + c2                       # linear index of each cell's lower corner
    n = ntri[cells]
    rep = np.repeat(np.arange(len(cells)), n)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    edges = table[case[cells][rep], k]                                   # [T, 3] edge ids
    q = lower[rep][:, None] + CORNER_OFFSETS[e_corner[edges]] @ strides  # the point that owns each edge
    a = e_axis[edges]
    vid = base[q] + (a > 0) * cross[q, 0] + (a > 1) * cross[q, 1]
    return verts, vid.astype(np.int32)


def _spacing_origin(spacing, origin):
    s = np.broadcast_to(np.asarray(spacing, dtype=np.float32), (3,))
    o = np.broadcast_to(np.asarray(origin, dtype=np.float32), (3,))
    return s, o


def marching_cubes(volume, level, spacing=1.0, origin=(0.0, 0.0, 0.0)):
    """Triangle mesh of the level set of `volume` [D0, D1, D2] (inside: v > level; normals outward).
    A CUDA tensor runs the gfx950 kernel and returns (verts [V, 3] float32, faces [T, 3] int32) as tensors on its device; a CPU tensor
    or a numpy array runs the numpy port and returns numpy arrays -- the same bits either way.  Vertices are in index space times
    `spacing` (a scalar or one per axis) plus `origin`; with the defaults nothing is applied."""
    s, o = _spacing_origin(spacing, origin)
    identity = bool(np.all(s == 1) and np.all(o == 0))
    if is_gpu(volume):
        import gnerf_hip
        verts, faces = gnerf_hip.marching_cubes(volume, level)
    else:
        verts, faces = marching_cubes_numpy(to_host(volume), level)
    if not identity:
        verts = verts * _on_route(s, verts) + _on_route(o, verts)
    return verts, faces


# ---------------------------------------------------------------------------------------------------------------- narrow band
# The density volume evaluated only where the surface is, by surface following on bricks (include/gnerf_hip.h, gnerf_band_*, states the rules;
# DESIGN.md 3.22 the argument): the mesh of the result is the dense volume's mesh in the same vertex and face order, minus whole components
# that no seeded or grown brick touched.  The lattice is n^3 points in linear order (axis 2 fastest); a brick is s^3 cells, its points the
# closed ranges, the last brick of an axis partial; the coarse points have every index in {0, s, 2s, ...} + {n - 1}.
# Brick states (one byte each): 0 inactive, 1 active (its points are evaluated), 2 new (active; its points are evaluated in this round),
# 3 named by this round's growth (becomes 2 when the round closes).
BAND_BRICKS = (2, 4, 8, 16)


def _band_geometry(n, s, keep):
    n, s = int(n), int(s)
    if s not in BAND_BRICKS:
        raise ValueError(f'band_volume: the brick edge must be one of {BAND_BRICKS}, got {s}')
    if n < 2 or n ** 3 >= 2 ** 31:
        raise ValueError(f'band_volume: n must be >= 2 with n^3 < 2^31, got {n}')
    keep = [(0, n)] * 3 if keep is None else [(min(max(int(lo), 0), n), min(max(int(hi), 0), n)) for lo, hi in keep]
    if len(keep) != 3:
        raise ValueError('band_volume: keep must be three (lo, hi) index ranges')
    return n, s, -(-(n - 1) // s), [(lo, max(hi, lo)) for lo, hi in keep]


def band_keep_of_crop(n, ranges):
    """The kept index range per axis of a crop `vol[:a] = 0; vol[-b:] = 0` per axis (ranges: three (a, b)), python's slices included: b == 0
    zeroes the whole axis.  For an axis stored flipped, swap a and b first."""
    return [(a, n - b) if b > 0 else (0, 0) for a, b in ranges]


def _band_coarse(n, s, nb):
    """(bounds [nb + 1]: brick b spans points bounds[b] .. bounds[b + 1]; is_coarse [n])."""
    bounds = np.minimum(np.arange(nb + 1, dtype=np.int64) * s, n - 1)
    is_coarse = np.zeros(n, dtype=bool)
    is_coarse[bounds] = True
    return bounds, is_coarse


def _band_kept(keep, i0, i1, i2):
    (a0, b0), (a1, b1), (a2, b2) = keep
    return (i0 >= a0) & (i0 < b0) & (i1 >= a1) & (i1 < b1) & (i2 >= a2) & (i2 < b2)


def band_points_numpy(state, n, s):
    """The index list of a round's new points (gnerf_band_points_*): the points of the bricks of state 2 that are neither coarse nor in a
    brick of state 1, each once -- a point that several new bricks share goes to the one of the lowest brick index --, brick-major, then
    row-major within the brick -> int32 [m]."""
    nb = -(-(n - 1) // s)
    bounds, is_coarse = _band_coarse(n, s, nb)
    state = np.asarray(state, dtype=np.uint8).reshape(nb, nb, nb)
    new = np.flatnonzero(state.reshape(-1) == 2)
    if not len(new):
        return np.zeros(0, dtype=np.int32)
    B = np.stack(np.unravel_index(new, (nb, nb, nb)), axis=1)                                  # [m, 3]
    lo, hi = bounds[B], bounds[B + 1]
    off = np.stack(np.meshgrid(*[np.arange(s + 1)] * 3, indexing='ij'), axis=-1).reshape(-1, 3)  # [L, 3], axis 2 fastest
    P = lo[:, None, :] + off[None]                                                             # [m, L, 3]
    listed = (P <= hi[:, None, :]).all(-1) & ~is_coarse[np.minimum(P, n - 1)].all(-1)
    at_lo, at_hi = P == lo[:, None, :], P == hi[:, None, :]
    for d0 in (-1, 0, 1):
        for d1 in (-1, 0, 1):
            for d2 in (-1, 0, 1):
                d = np.array([d0, d1, d2])
                if not d.any():
                    continue
                O = B + d
                shares = np.ones(P.shape[:2], dtype=bool)                                      # the point also lies in brick B + d
                for a in range(3):
                    if d[a] == -1:
                        shares &= at_lo[..., a] & (B[:, a] > 0)[:, None]
                    elif d[a] == 1:
                        shares &= at_hi[..., a] & (B[:, a] < nb - 1)[:, None]
                Oc = np.clip(O, 0, nb - 1)
                st = state[Oc[:, 0], Oc[:, 1], Oc[:, 2]]
                olin = (O[:, 0] * nb + O[:, 1]) * nb + O[:, 2]
                first = (st == 1) | ((st == 2) & (olin < new))
                listed &= ~(shares & first[:, None])
    idx = (P[..., 0] * n + P[..., 1]) * n + P[..., 2]
    return idx[listed].astype(np.int32)


def band_seed_numpy(vol, n, level, s, keep=None):
    """gnerf_band_seed: state 2 for every brick whose eight corner points (effective values) are not all on one side of `level`, 0 for
    the others -> (state uint8 [nb^3], seeds)."""
    n, s, nb, keep = _band_geometry(n, s, keep)
    bounds, _ = _band_coarse(n, s, nb)
    v = np.asarray(vol, dtype=np.float32).reshape(n, n, n)[np.ix_(bounds, bounds, bounds)]
    g = np.meshgrid(bounds, bounds, bounds, indexing='ij')
    inside = np.where(_band_kept(keep, *g), v, np.float32(0)) > np.float32(level)
    corners = [inside[a:nb + a, b:nb + b, c:nb + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    mixed = np.logical_or.reduce(corners) & ~np.logical_and.reduce(corners)
    state = np.where(mixed, 2, 0).astype(np.uint8).reshape(-1)
    return state, int(mixed.sum())


def band_grow_numpy(vol, n, level, s, state, keep=None):
    """gnerf_band_grow: every brick of state 2 tests its six faces whose neighbour has state 0 (or 3); a face whose points (effective values)
    are not all on one side names the neighbour (3).  Then the round closes: 2 -> 1, 3 -> 2 -> (state', new bricks)."""
    n, s, nb, keep = _band_geometry(n, s, keep)
    bounds, _ = _band_coarse(n, s, nb)
    level = np.float32(level)
    vol = np.asarray(vol, dtype=np.float32).reshape(-1)
    state = np.array(state, dtype=np.uint8).reshape(nb, nb, nb)
    new = np.flatnonzero(state.reshape(-1) == 2)
    if len(new):
        B = np.stack(np.unravel_index(new, (nb, nb, nb)), axis=1)
        lo, hi = bounds[B], bounds[B + 1]
        u, w = (x.reshape(-1) for x in np.meshgrid(np.arange(s + 1), np.arange(s + 1), indexing='ij'))
        for a in range(3):
            b, c = [x for x in range(3) if x != a]
            for side, d in ((lo, -1), (hi, 1)):
                O = B.copy()
                O[:, a] += d
                exists = (O[:, a] >= 0) & (O[:, a] < nb)
                Oc = np.clip(O, 0, nb - 1)
                open_ = exists & np.isin(state[Oc[:, 0], Oc[:, 1], Oc[:, 2]], (0, 3))
                P = np.empty((len(new), len(u), 3), dtype=np.int64)
                P[..., a] = side[:, a][:, None]
                P[..., b] = lo[:, b][:, None] + u[None]
                P[..., c] = lo[:, c][:, None] + w[None]
                valid = (P[..., b] <= hi[:, b][:, None]) & (P[..., c] <= hi[:, c][:, None])
                Pc = np.minimum(P, n - 1)
                v = vol[(Pc[..., 0] * n + Pc[..., 1]) * n + Pc[..., 2]]
                inside = np.where(_band_kept(keep, Pc[..., 0], Pc[..., 1], Pc[..., 2]), v, np.float32(0)) > level
                mixed = open_ & (inside & valid).any(1) & (~inside & valid).any(1)
                t = Oc[mixed]
                state[t[:, 0], t[:, 1], t[:, 2]] = 3
    state = state.reshape(-1)
    out = np.where(state == 2, 1, np.where(state == 3, 2, state)).astype(np.uint8)
    return out, int((out == 2).sum())


def band_fill_numpy(vol, n, s, state, keep=None):
    """gnerf_band_fill, in place: every point that is neither coarse nor in a brick of state 1 or 2 takes the effective value of the coarse
    point at (i // s * s, j // s * s, k // s * s)."""
    n, s, nb, keep = _band_geometry(n, s, keep)
    bounds, is_coarse = _band_coarse(n, s, nb)
    v = vol.reshape(n, n, n)
    active = np.isin(np.asarray(state).reshape(nb, nb, nb), (1, 2))
    sizes = np.diff(bounds)
    cells = np.pad(active.repeat(sizes, 0).repeat(sizes, 1).repeat(sizes, 2), 1)
    in_active = np.logical_or.reduce([cells[a:n + a, b:n + b, c:n + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    coarse = is_coarse[:, None, None] & is_coarse[None, :, None] & is_coarse[None, None, :]
    corner = np.arange(n) // s * s
    g = np.meshgrid(corner, corner, corner, indexing='ij')
    value = np.where(_band_kept(keep, *g), v[np.ix_(corner, corner, corner)], np.float32(0))
    target = ~coarse & ~in_active
    v[target] = value[target]
    return vol


def _band_driver(n, s, evaluate, coarse_index, band, trace, fill=True):
    """The steps of the rules, spelled once for both routes: evaluate(index) writes the densities; band holds the brick states and gives the
    route's stages -- seed() -> seeds, points() -> the round's index list, grow() -> new bricks, fill(), and state for the trace.
    fill=False leaves the volume as the rounds left it (band_mesh: marching cubes then reads the active bricks only)."""
    evaluate(coarse_index)
    evaluated = len(coarse_index)
    new = seeds = band.seed()
    per_round = []
    while new:
        index = band.points()
        evaluate(index)
        evaluated += len(index)
        new = band.grow()
        per_round.append(new)
        if trace is not None:
            trace.append((to_host(band.state).copy(), to_host(index).copy()))
    if fill:
        band.fill()
    return dict(brick=s, bricks=(-(-(n - 1) // s)) ** 3, seeds=seeds, new_bricks=per_round, rounds=len(per_round), host_reads=len(per_round) + 1,
                points=evaluated, share=evaluated / n ** 3)


class _BandNumpy:
    """The port's side of _band_driver: the brick states of one volume (float32 numpy [n^3], evaluated in place by the caller) and the stages."""

    def __init__(self, vol, n, s, level, keep):
        self.vol, self.n, self.s, self.level, self.keep, self.state = vol, n, s, level, keep, None

    def seed(self):
        self.state, seeds = band_seed_numpy(self.vol, self.n, self.level, self.s, self.keep)
        return seeds

    def points(self):
        return band_points_numpy(self.state, self.n, self.s)

    def grow(self):
        self.state, new = band_grow_numpy(self.vol, self.n, self.level, self.s, self.state, self.keep)
        return new

    def fill(self):
        band_fill_numpy(self.vol, self.n, self.s, self.state, self.keep)


def band_coarse_index(n, s):
    """The linear indices of the coarse points, ascending -> int32 numpy [(nb + 1)^3]."""
    bounds, _ = _band_coarse(n, s, -(-(n - 1) // s))
    return ((bounds[:, None, None] * n + bounds[None, :, None]) * n + bounds[None, None, :]).reshape(-1).astype(np.int32)


def band_volume_numpy(field, n, level, s, keep=None, trace=None):
    """The numpy port of band_volume (the CPU path, and the bits the kernels give): field(index int32 numpy [m], out float32 numpy [n^3])
    writes the densities at those indices -> (volume float32 [n, n, n] before the crop, report).  trace: a list that receives (state after
    the round, the round's index list) per round."""
    n, s, nb, keep = _band_geometry(n, s, keep)
    vol = np.zeros(n ** 3, dtype=np.float32)
    report = _band_driver(n, s, lambda index: field(index, vol) if len(index) else None, band_coarse_index(n, s), _BandNumpy(vol, n, s, level, keep), trace)
    return vol.reshape(n, n, n), report


def band_volume(field, n, level, s, keep=None, device=None, trace=None):
    """The density volume of an n^3 lattice evaluated in a narrow band around the level set (the rules above): field(index, out) writes the
    densities at the int32 linear indices `index` into the flat float32 `out` [n^3] -- called with every index at most once.  keep: the
    kept index range (lo, hi) per axis of the crop that follows, None for everything -> (volume [n, n, n] BEFORE the crop, report: brick,
    bricks, seeds, new_bricks per round, rounds, host_reads, points evaluated and their share of n^3).
    device: a CUDA device takes the kernels (csrc/mesh_band.hip through gnerf_hip.band_*; index and out are tensors there), anything else the
    numpy port -- the same brick states, lists and volume either way."""
    torch = _torch()
    dev = None if device is None or torch is None else torch.device(device)
    if dev is None or dev.type != 'cuda':
        return band_volume_numpy(field, n, level, s, keep, trace)
    import gnerf_hip
    n, s, nb, keep = _band_geometry(n, s, keep)
    vol = torch.empty(n ** 3, dtype=torch.float32, device=dev)
    report = _band_driver(n, s, lambda index: field(index, vol) if len(index) else None, torch.from_numpy(band_coarse_index(n, s)).to(dev),
                          gnerf_hip.BandVolume(vol, n, s, level, keep), trace)
    return vol.reshape(n, n, n), report


def band_report_line(report):
    return (f'band: bricks of {report["brick"]}^3 cells, {report["seeds"]} seeded + {sum(report["new_bricks"])} grown of {report["bricks"]} in '
            f'{report["rounds"]} round(s), {report["points"]} points evaluated ({100 * report["share"]:.2f} % of the lattice)')


# The mesh of a band run without the fill (include/gnerf_hip.h, gnerf_band_mesh_*, states the rules; DESIGN.md 3.23 the argument): marching cubes
# over the points of the active bricks only, in a VIEW of the lattice -- mesh coordinate m_k = l_perm[k], or n - 1 - l_perm[k] where lattice axis
# perm[k] is flipped, so the mesh volume is vol.reshape(n, n, n).flip(flipped axes).permute(perm) -- with the crop as `keep`.  The result is
# marching cubes' of the filled, cropped, flipped and permuted volume, bit for bit and in the same order.
BAND_MESH_PIPELINE_VIEW = dict(perm=(2, 1, 0), flip=(True, False, False))     # extract_density_grid's flip(0) + mesh_of_density_grid's permute


def _band_view(perm, flip):
    perm, flip = tuple(int(a) for a in perm), tuple(bool(f) for f in flip)
    if sorted(perm) != [0, 1, 2]:
        raise ValueError(f'band_marching_cubes: perm must be a permutation of (0, 1, 2), got {perm}')
    if len(flip) != 3:
        raise ValueError('band_marching_cubes: flip must hold one flag per lattice axis')
    return perm, flip


def band_visited_numpy(state, n, s):
    """The points in the closed range of at least one active brick -> bool [n, n, n] (state: the final 0 / 1 bytes)."""
    nb = -(-(n - 1) // s)
    bounds, _ = _band_coarse(n, s, nb)
    sizes = np.diff(bounds)
    active = np.asarray(state).reshape(nb, nb, nb) == 1
    cells = np.pad(active.repeat(sizes, 0).repeat(sizes, 1).repeat(sizes, 2), 1)
    return np.logical_or.reduce([cells[a:n + a, b:n + b, c:n + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])


def band_marching_cubes_numpy(volume, state, n, s, level, keep=None, perm=(0, 1, 2), flip=(False, False, False), return_counts=False):
    """The numpy port of gnerf_hip.band_marching_cubes, written from the rule with plain masks: volume float32 [n^3] as the band's rounds left
    it (no fill), state uint8 [nb^3] of 0 / 1, keep as band_volume takes it, the view (perm, flip per LATTICE axis) -> (verts float32 [V, 3],
    faces int32 [T, 3]) in mesh coordinates, the kernels' bits.  Only visited points are read.  Raises ValueError on a non-finite effective value
    at a visited point; with return_counts nothing is raised and (verts, faces, counts int64 [4]: V, T, non-finite, visited points) comes back,
    the mesh empty when the third count is not 0."""
    n, s, nb, keep = _band_geometry(n, s, keep)
    perm, flip = _band_view(perm, flip)
    vol = np.asarray(volume)
    state = np.asarray(state)
    if vol.size != n ** 3:
        raise ValueError(f'band_marching_cubes: the volume must hold n^3 = {n ** 3} values, got {vol.size}')
    if state.size != nb ** 3:
        raise ValueError(f'band_marching_cubes: state must hold nb^3 = {nb ** 3} bytes, got {state.size}')
    if state.size and int(state.max()) > 1:
        raise ValueError('band_marching_cubes: every brick state must be 0 or 1 (the band\'s rounds have not ended)')
    vol = vol.astype(np.float32, copy=False).reshape(n, n, n)
    seen = band_visited_numpy(state, n, s)
    i = np.arange(n)
    kept = _band_kept(keep, i[:, None, None], i[None, :, None], i[None, None, :])
    eff = np.zeros((n, n, n), dtype=np.float32)
    read = seen & kept
    eff[read] = vol[read]                                                # the only read of the volume
    axes = [a for a in range(3) if flip[a]]
    view = lambda x: np.ascontiguousarray(np.transpose(np.flip(x, axes) if axes else x, perm))
    eff, seen = view(eff), view(seen)
    bad = int(np.count_nonzero(seen & ~np.isfinite(eff)))
    if bad and not return_counts:
        raise ValueError(f'band_marching_cubes: {bad} visited point(s) hold a non-finite value')
    with np.errstate(all='ignore'):                                     # (a non-finite value is outside or inside by v > level, and counted)
        verts, faces = _marching_cubes_masked(eff, np.float32(level), seen)
    if not return_counts:
        return verts, faces
    counts = np.array([len(verts), len(faces), bad, int(seen.sum())], dtype=np.int64)
    if bad:
        verts, faces = np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32)
    return verts, faces, counts


def band_mesh(field, n, level, s, keep=None, perm=(0, 1, 2), flip=(False, False, False), device=None, trace=None, binding=None):
    """band_volume's rounds WITHOUT the fill, then marching cubes over the active bricks alone: field(index, out) as band_volume takes it ->
    (verts float32 [V, 3], faces int32 [T, 3], report) -- the mesh marching cubes makes of band_volume's volume after the crop `keep`, the flips
    and the permutation, bit for bit and in the same order, with no pass over the n^3 lattice.  report: band_volume's plus active (bricks),
    visited (points in an active brick's closed range) and mesh (V, T).  Raises ValueError, on either route, when a visited point holds a
    non-finite effective value, as marching_cubes does on such a volume.  device: a CUDA device takes the kernels (csrc/mesh_band.hip,
    csrc/mesh_band_cubes.hip; the volume is torch.empty there and nothing initialises it), anything else the numpy ports."""
    torch = _torch()
    dev = None if device is None or torch is None else torch.device(device)
    n, s, nb, keep = _band_geometry(n, s, keep)
    perm, flip = _band_view(perm, flip)
    if dev is None or dev.type != 'cuda':
        vol = np.zeros(n ** 3, dtype=np.float32)
        band = _BandNumpy(vol, n, s, level, keep)
        report = _band_driver(n, s, lambda index: field(index, vol) if len(index) else None, band_coarse_index(n, s), band, trace, fill=False)
        state = band.state if band.state is not None else np.zeros(nb ** 3, dtype=np.uint8)
        verts, faces, counts = band_marching_cubes_numpy(vol, state, n, s, level, keep, perm, flip, return_counts=True)
    else:
        import gnerf_hip
        vol = torch.empty(n ** 3, dtype=torch.float32, device=dev)
        band = gnerf_hip.BandVolume(vol, n, s, level, keep, binding=binding)
        report = _band_driver(n, s, lambda index: field(index, vol) if len(index) else None, torch.from_numpy(band_coarse_index(n, s)).to(dev),
                              band, trace, fill=False)
        verts, faces, counts = gnerf_hip.band_marching_cubes(vol, band.state, n, s, level, keep, perm, flip, binding=binding,
                                                             active=report['seeds'] + sum(report['new_bricks']), return_counts=True)
    if counts[2]:                                                       # (either route: the route this replaces raises on such a volume too)
        raise ValueError(f'band_marching_cubes: {int(counts[2])} visited point(s) hold a non-finite value')
    report.update(active=report['seeds'] + sum(report['new_bricks']), visited=int(counts[3]), mesh=(len(verts), len(faces)))
    return verts, faces, report


# ---------------------------------------------------------------------------------------------------------------- rasteriser
# The numpy port of csrc/raster.hip (include/gnerf_hip.h, gnerf_raster_*, states the rules): float32 throughout, one rounding per
# operation in the kernel's order, integers in int64 -- the kernel's visibility buffer, counts and resolved images bit for bit.
RASTER_SMALL_PIXELS = 64
RASTER_CULL = {'none': 0, 'back': 1, 'front': 2}
RASTER_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
RASTER_SHADING = dict(light=(0.0, 0.0, -1.0), ambient=0.25, diffuse=0.75, albedo=(0.8, 0.8, 0.8), background=(1.0, 1.0, 1.0))
_F = np.float32


def _raster_cameras(mesh2cam, intrinsics):
    A = np.ascontiguousarray(np.asarray(mesh2cam), dtype=np.float32)
    K = np.ascontiguousarray(np.asarray(intrinsics), dtype=np.float32)
    if A.size == 0 or A.size % 12 or K.size % 9 or A.size // 12 != K.size // 9:
        raise ValueError('raster: mesh2cam must be [n_views, 3, 4] and intrinsics [n_views, 3, 3] for the same n_views >= 1')
    return A.reshape(-1, 12), K.reshape(-1, 9)


def _raster_mesh(verts, faces):
    v = np.ascontiguousarray(np.asarray(verts), dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(np.asarray(faces), dtype=np.int32).reshape(-1, 3)
    return v, f


def _raster_size(size):
    h, w = (size, size) if np.isscalar(size) else size
    h, w = int(h), int(w)
    if not (1 <= h <= 4096 and 1 <= w <= 4096):
        raise ValueError(f'raster: the image size must be 1..4096 in each direction (got {h} x {w})')
    return h, w


def _raster_point(v, A, K, near):
    """The first half of the vertex stage for one view, which the rasteriser and the colour bake share: (cam float32 [V, 3], near_bad [V]:
    non-finite or not in front of near, iz float32 [V], xc, yc float32 [V]: the normalised image coordinates; iz is 0 where near_bad)."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all='ignore'):
        cam = np.stack([((A[4 * r] * x + A[4 * r + 1] * y) + A[4 * r + 2] * z) + A[4 * r + 3] for r in range(3)], axis=1)
        near_bad = ~np.isfinite(cam).all(axis=1) | ~(cam[:, 2] > _F(near))
        iz = np.where(near_bad, _F(0), _F(1) / np.where(near_bad, _F(1), cam[:, 2])).astype(np.float32)
        xn, yn = cam[:, 0] * iz, cam[:, 1] * iz
        fx, sk, cx, fy, cy = K[0], K[1], K[2], K[4], K[5]
        xc = (fx * xn + sk * yn) + cx
        yc = fy * yn + cy
    return cam.astype(np.float32), near_bad, iz, xc, yc


def _raster_project(v, A, K, h, w, near):
    """The vertex stage for one view: (cam float32 [V, 3], iz float32 [V], X int64 [V], Y int64 [V], bad uint8 [V]: 1 near, 2 guard)."""
    cam, near_bad, iz, xc, yc = _raster_point(v, A, K, near)
    with np.errstate(all='ignore'):
        fX = np.rint((xc * _F(w)) * _F(256))
        fY = np.rint((yc * _F(h)) * _F(256))
        guard_bad = ~near_bad & (~(np.abs(fX) <= _F(2097152)) | ~(np.abs(fY) <= _F(2097152)))
    bad = np.where(near_bad, 1, np.where(guard_bad, 2, 0)).astype(np.uint8)
    ok = bad == 0
    X = np.where(ok, fX, 0).astype(np.int64)
    Y = np.where(ok, fY, 0).astype(np.int64)
    return cam.astype(np.float32), np.where(ok, iz, _F(0)).astype(np.float32), X, Y, bad


def _raster_setup(f, n_verts, X, Y, iz, bad, cull, h, w):
    """Triangle setup for one view over faces f [T, 3] -> dict of arrays [T] (status: 0 drawn, 1 near, 2 guard, 3 culled)."""
    valid = ((f >= 0) & (f < n_verts)).all(axis=1)
    g = np.where(valid[:, None], f, 0).astype(np.int64)
    b = bad[g] if n_verts else np.zeros(g.shape, np.uint8)
    X3, Y3, iz3 = (X[g], Y[g], iz[g]) if n_verts else (np.zeros(g.shape, np.int64), np.zeros(g.shape, np.int64), np.zeros(g.shape, np.float32))
    area = (X3[:, 1] - X3[:, 0]) * (Y3[:, 2] - Y3[:, 0]) - (X3[:, 2] - X3[:, 0]) * (Y3[:, 1] - Y3[:, 0])
    culled = (area == 0) | ((cull == 1) & (area > 0)) | ((cull == 2) & (area < 0))
    status = np.where(~valid, 3, np.where((b == 1).any(axis=1), 1, np.where((b != 0).any(axis=1), 2, np.where(culled, 3, 0))))
    flipped = area < 0
    ib, ic = np.where(flipped, 2, 1), np.where(flipped, 1, 2)
    rows = np.arange(len(f))
    t = dict(status=status, flipped=flipped, area=np.abs(area), ia=g[:, 0], ib=g[rows, ib], ic=g[rows, ic],
             ax=X3[:, 0], ay=Y3[:, 0], iza=iz3[:, 0], bx=X3[rows, ib], by=Y3[rows, ib], izb=iz3[rows, ib],
             cx=X3[rows, ic], cy=Y3[rows, ic], izc=iz3[rows, ic])
    c0 = np.maximum((X3.min(axis=1) + 127) >> 8, 0)
    c1 = np.minimum((X3.max(axis=1) - 128) >> 8, w - 1)
    r0 = np.maximum((Y3.min(axis=1) + 127) >> 8, 0)
    r1 = np.minimum((Y3.max(axis=1) - 128) >> 8, h - 1)
    bw, bh = np.maximum(c1 - c0 + 1, 0), np.maximum(r1 - r0 + 1, 0)
    t.update(c0=c0, r0=r0, bw=bw, bh=bh, npx=np.where(status == 0, bw * bh, 0))
    return t


def _raster_owns(e, dx, dy):
    return (e > 0) | ((e == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))


def _raster_cover(t, row, col):
    """Edge functions at the centres of pixels (row, col) (broadcast against the triangle fields of t) -> (covered, wa, wb, wc)."""
    px, py = 256 * col + 128, 256 * row + 128
    wa = (t['cx'] - t['bx']) * (py - t['by']) - (t['cy'] - t['by']) * (px - t['bx'])
    wb = (t['ax'] - t['cx']) * (py - t['cy']) - (t['ay'] - t['cy']) * (px - t['cx'])
    wc = (t['bx'] - t['ax']) * (py - t['ay']) - (t['by'] - t['ay']) * (px - t['ax'])
    covered = (_raster_owns(wa, t['cx'] - t['bx'], t['cy'] - t['by']) & _raster_owns(wb, t['ax'] - t['cx'], t['ay'] - t['cy'])
               & _raster_owns(wc, t['bx'] - t['ax'], t['by'] - t['ay']))
    return covered, wa, wb, wc


def _raster_iz(t, wa, wb, wc):
    """(iz, ba, bb, bc): b_i = float32(w_i) / float32(area), iz = (ba iza + bb izb) + bc izc."""
    fa = np.asarray(t['area']).astype(np.float32)
    with np.errstate(all='ignore'):
        ba, bb, bc = (np.asarray(x).astype(np.float32) / fa for x in (wa, wb, wc))
        return (ba * t['iza'] + bb * t['izb']) + bc * t['izc'], ba, bb, bc


def _raster_merge(vis_view, w, t, row, col, tri):
    """Merge the centres of pixels (row, col) of the triangles t (indices tri; all broadcast against each other) into vis_view [h * w]."""
    covered, wa, wb, wc = _raster_cover(t, row, col)
    if not np.any(covered):
        return
    with np.errstate(all='ignore'):
        z = np.asarray(_F(1) / _raster_iz(t, wa, wb, wc)[0], dtype=np.float32)
    key = (np.ascontiguousarray(z).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.broadcast_to(np.asarray(tri, dtype=np.uint64), covered.shape)
    pix = np.broadcast_to(row * w + col, covered.shape)
    np.minimum.at(vis_view, pix[covered], key[covered])


def rasterize_numpy(verts, faces, mesh2cam, intrinsics, size, near=0.01, cull='none'):
    """The numpy port of gnerf_raster_visibility: (vis uint64 [n_views, h, w], counts int64 [4] = drawn, near, guard, culled)."""
    v, f = _raster_mesh(verts, faces)
    A, K = _raster_cameras(mesh2cam, intrinsics)
    h, w = _raster_size(size)
    if not near > 0:
        raise ValueError('raster: near must be > 0')
    if cull not in RASTER_CULL:
        raise ValueError(f'raster: cull must be one of {tuple(RASTER_CULL)}')
    n_views = len(A)
    vis = np.full((n_views, h * w), RASTER_EMPTY, dtype=np.uint64)
    counts = np.zeros(4, dtype=np.int64)
    if len(v) == 0 or len(f) == 0:
        return vis.reshape(n_views, h, w), counts
    for view in range(n_views):
        _, iz, X, Y, bad = _raster_project(v, A[view], K[view], h, w, near)
        t = _raster_setup(f, len(v), X, Y, iz, bad, RASTER_CULL[cull], h, w)
        counts += np.bincount(t['status'], minlength=4)[:4]
        npx = t['npx']
        small = np.nonzero((npx > 0) & (npx <= RASTER_SMALL_PIXELS))[0]
        if len(small):                                                   # the thread-per-triangle route: pixel i of every box at once
            ts = {k: x[small] for k, x in t.items()}
            for i in range(int(ts['npx'].max())):
                sel = np.nonzero(i < ts['npx'])[0]
                sub = {k: x[sel] for k, x in ts.items()}
                r = i // sub['bw']
                _raster_merge(vis[view], w, sub, sub['r0'] + r, sub['c0'] + (i - r * sub['bw']), small[sel])
        for k in np.nonzero(npx > RASTER_SMALL_PIXELS)[0]:               # the queued route: one triangle, its whole box
            one = {name: x[k] for name, x in t.items()}
            rr, cc = np.meshgrid(one['r0'] + np.arange(one['bh']), one['c0'] + np.arange(one['bw']), indexing='ij')
            _raster_merge(vis[view], w, one, rr, cc, k)
    return vis.reshape(n_views, h, w), counts


def _shading_vector(shading):
    s = dict(RASTER_SHADING, **(shading or {}))
    unknown = set(s) - set(RASTER_SHADING)
    if unknown:
        raise ValueError(f'raster: unknown shading parameter(s) {sorted(unknown)}')
    vec = np.array([*s['light'], s['ambient'], s['diffuse'], *s['albedo'], *s['background']], dtype=np.float32)
    if vec.shape != (11,):
        raise ValueError('raster: light, albedo and background are triples, ambient and diffuse scalars')
    return vec


def _to_u8(x):
    return np.rint(np.fmin(np.fmax(x, _F(0)), _F(1)) * _F(255)).astype(np.int32).astype(np.uint8)


def resolve_numpy(vis, verts, faces, mesh2cam, intrinsics, normals=None, normal_mat=None, colors=None, shading=None,
                  outputs=('tri_id', 'depth', 'normal', 'frame')):
    """The numpy port of gnerf_raster_resolve: dict of tri_id int32 [n, h, w], depth float32 [n, h, w], normal float32 [n, h, w, 3],
    frame uint8 [n, h, w, 3] (those named in `outputs`).  shading: dict over RASTER_SHADING's keys."""
    v, f = _raster_mesh(verts, faces)
    A, K = _raster_cameras(mesh2cam, intrinsics)
    vis = np.asarray(vis)
    n_views, h, w = vis.shape
    if len(A) != n_views:
        raise ValueError('raster: vis and the cameras disagree about n_views')
    sh = _shading_vector(shading)
    light, ambient, diffuse, albedo, background = sh[0:3], sh[3], sh[4], sh[5:8], sh[8:11]
    if normals is not None:
        normals = np.ascontiguousarray(np.asarray(normals), dtype=np.float32).reshape(-1, 3)
        N = np.ascontiguousarray(np.asarray(normal_mat), dtype=np.float32).reshape(n_views, 9)
        if len(normals) != len(v):
            raise ValueError('raster: normals must be [V, 3]')
    if colors is not None:
        colors = np.asarray(colors)
        if colors.dtype != np.uint8 or colors.shape != (len(v), 3):
            raise ValueError('raster: colors must be uint8 [V, 3]')
    tri_id = np.full((n_views, h, w), -1, dtype=np.int32)
    depth = np.full((n_views, h, w), np.inf, dtype=np.float32)
    normal = np.zeros((n_views, h, w, 3), dtype=np.float32)
    frame = np.empty((n_views, h, w, 3), dtype=np.uint8)
    frame[...] = _to_u8(background)
    n_tris = len(f) if len(v) else 0
    for view in range(n_views):
        key = vis[view].reshape(-1).astype(np.uint64)
        tri = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
        pix = np.nonzero((key != RASTER_EMPTY) & (tri < n_tris))[0]
        if len(pix) == 0:
            continue
        cam, iz_v, X, Y, bad = _raster_project(v, A[view], K[view], h, w, 0.0)
        t = _raster_setup(f[tri[pix]], len(v), X, Y, iz_v, bad, 0, h, w)
        keep = t['status'] == 0
        pix = pix[keep]
        t = {k: x[keep] for k, x in t.items()}
        tri = tri[pix]
        row, col = pix // w, pix % w
        _, wa, wb, wc = _raster_cover(t, row, col)
        with np.errstate(all='ignore'):
            iz, ba, bb, bc = _raster_iz(t, wa, wb, wc)
            z = _F(1) / iz
            fx, sk, cx, fy, cy = K[view][0], K[view][1], K[view][2], K[view][4], K[view][5]
            xc = col.astype(np.float32) * (_F(1) / _F(w)) + (_F(0.5) / _F(w))
            yc = row.astype(np.float32) * (_F(1) / _F(h)) + (_F(0.5) / _F(h))
            xl = xc - cx
            xl = xl + (cy * sk) / fy
            xl = xl - (sk * yc) / fy
            xl = xl / fx
            yl = (yc - cy) / fy
            tri_id[view].reshape(-1)[pix] = tri
            depth[view].reshape(-1)[pix] = z * np.sqrt((xl * xl + yl * yl) + _F(1))
            qa, qb, qc = (ba * t['iza']) / iz, (bb * t['izb']) / iz, (bc * t['izc']) / iz
            if normals is not None:
                na, nb, nc = normals[t['ia']], normals[t['ib']], normals[t['ic']]
                m = (qa[:, None] * na + qb[:, None] * nb) + qc[:, None] * nc
                Nv = N[view]
                n = np.stack([(Nv[3 * r] * m[:, 0] + Nv[3 * r + 1] * m[:, 1]) + Nv[3 * r + 2] * m[:, 2] for r in range(3)], axis=1)
            else:
                g = f[tri].astype(np.int64)
                p0, p1, p2 = cam[g[:, 0]], cam[g[:, 1]], cam[g[:, 2]]
                e1, e2 = p1 - p0, p2 - p0
                n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                              e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
            length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            ok = length > 0
            n = np.where(ok[:, None], n / np.where(ok, length, _F(1))[:, None], _F(0)).astype(np.float32)
            away = ((n[:, 0] * xl + n[:, 1] * yl) + n[:, 2]) > 0
            n = np.where(away[:, None], -n, n)
            normal[view].reshape(-1, 3)[pix] = n
            ndl = np.fmax(_F(0), (n[:, 0] * light[0] + n[:, 1] * light[1]) + n[:, 2] * light[2])
            shade = ambient + diffuse * ndl
            if colors is not None:
                ca, cb, cc = (colors[t[k]].astype(np.float32) for k in ('ia', 'ib', 'ic'))
                base = ((qa[:, None] * ca + qb[:, None] * cb) + qc[:, None] * cc) / _F(255)
            else:
                base = np.broadcast_to(albedo, (len(pix), 3))
            frame[view].reshape(-1, 3)[pix] = _to_u8(base * shade[:, None])
    out = dict(tri_id=tri_id, depth=depth, normal=normal, frame=frame)
    return {k: out[k] for k in outputs}


def mesh_to_camera(cam2world, mesh2world=None):
    """Per-view mesh2cam [n, 3, 4] and normal_mat [n, 3, 3] as float32, made in float64 and rounded once: mesh2cam = inverse(cam2world) @
    mesh2world (cam2world [n, 4, 4] or [4, 4]; mesh2world a 3x4 / 4x4 affine, identity when None); normal_mat takes a normal of the mesh frame
    to the camera frame as a covector, inverse(linear part)^T (its scale does not matter: the rasteriser normalises)."""
    c2w = np.asarray(cam2world, dtype=np.float64).reshape(-1, 4, 4)
    M = np.eye(4)
    if mesh2world is not None:
        mw = np.asarray(mesh2world, dtype=np.float64)
        M[:3] = mw[:3]
    full = np.linalg.inv(c2w) @ M
    lin = full[:, :3, :3]
    return full[:, :3, :].astype(np.float32), np.linalg.inv(lin).transpose(0, 2, 1).astype(np.float32)


def _cameras_on_route(verts, cam2world, intrinsics, mesh2world):
    """render_mesh's and bake_mesh_colors' cameras, made on the host (mesh_to_camera) and put where verts live -> (mesh2cam [n, 12],
    intrinsics [n, 9], normal_mat [n, 9]), float32."""
    mesh2cam, normal_mat = mesh_to_camera(to_host(cam2world), to_host(mesh2world))
    K = np.ascontiguousarray(to_host(intrinsics), dtype=np.float32).reshape(-1, 9)
    return tuple(_on_route(x, verts) for x in (mesh2cam.reshape(-1, 12), K, normal_mat.reshape(-1, 9)))


def render_mesh(verts, faces, cam2world, intrinsics, size, mesh2world=None, normals=None, colors=None, near=0.01, cull='none', shading=None,
                outputs=('tri_id', 'depth', 'normal', 'frame'), texture=None, patch=8):
    """Draw a triangle mesh from n cameras (cam2world [n, 4, 4] and normalised intrinsics [n, 3, 3]: what a camera label holds) on the
    renderer's pixel grid -> dict of `outputs` (tri_id, depth as image_depth measures it, camera-frame normal, shaded uint8 frame) plus
    'counts'.  CUDA tensors run the gfx950 kernels (gnerf_hip.rasterize / resolve) and return tensors on their device; numpy arrays run
    the numpy port -- the same bits either way.  normals [V, 3] are in the mesh's frame (mesh_vertex_attributes'), colors uint8 [V, 3].
    texture: bake_mesh_texture's uint8 [th, tw, 3] atlas at `patch`; with it 'frame' is the textured resolve's (resolve_textured: the
    texture's own colours, unlit, on the shading's background) and every other output is as without it."""
    route, verts, faces = _mesh_route(verts, faces)
    mesh2cam, K, normal_mat = _cameras_on_route(verts, cam2world, intrinsics, mesh2world)
    normals, colors = _on_route(normals, verts), _on_route(colors, verts)
    vis, counts = route.rasterize(verts, faces, mesh2cam, K, size, near=near, cull=cull)
    plain = tuple(o for o in outputs if texture is None or o != 'frame')
    out = {}
    if plain:
        out = route.resolve(vis, verts, faces, mesh2cam, K, normals=normals, normal_mat=normal_mat if normals is not None else None, colors=colors,
                            shading=shading, outputs=plain)
    if texture is not None and 'frame' in outputs:
        background = [int(c) for c in _to_u8(_shading_vector(shading)[8:11])]
        out['frame'] = route.resolve_textured(vis, verts, faces, mesh2cam, K, _on_route(texture, verts), patch=patch, background=background)
    out['counts'] = counts
    return out


# ---------------------------------------------------------------------------------------------------------------- colour bake
# The numpy port of gnerf_mesh_bake_colors (csrc/raster.hip; include/gnerf_hip.h states the rules): the rasteriser's inverse.  Every vertex
# gathers its colour from the views' frames: projected with the rasteriser's vertex stage, rejected where the view's visibility buffer holds
# nothing or a nearer surface anywhere in the (2 guard + 1)^2 window around its pixel, sampled bilinearly, blended by cos^power of the angle
# between its normal and the line of sight.  float32, one rounding per operation in the kernel's order: the same bits.
BAKE_RULES = dict(near=0.01, depth_tol=2.0 ** -8, guard=1, min_cos=0.1, power=2)       # arguments, not measurements (the header derives depth_tol)


def _dot3_f32(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _bake_arguments(n_points, mesh2cam, intrinsics, vis, frames, normals, normal_mat, near, depth_tol, guard, power, fallback):
    """The checks bake_colors_numpy and bake_texture_numpy share -> (A, K, vis as uint64, frames, normals, N, fallback); n_points: the length
    normals and fallback must have (the vertices)."""
    A, K = _raster_cameras(mesh2cam, intrinsics)
    vis = np.ascontiguousarray(np.asarray(vis))
    frames = np.asarray(frames)
    n_views = len(A)
    if vis.ndim != 3 or vis.dtype.itemsize != 8 or vis.dtype.kind not in 'iu' or vis.shape[0] != n_views:
        raise ValueError('bake: vis must be the 64-bit [n_views, h, w] visibility buffer of the same cameras')
    vis = vis.view(np.uint64)
    _raster_size(vis.shape[1:])
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[0] != n_views or frames.shape[3] != 3:
        raise ValueError('bake: frames must be uint8 [n_views, fh, fw, 3]')
    _raster_size(frames.shape[1:3])
    if not near > 0:
        raise ValueError('bake: near must be > 0')
    if not depth_tol >= 0:
        raise ValueError('bake: depth_tol must be >= 0')
    if int(guard) != guard or not 0 <= guard <= 4:
        raise ValueError('bake: guard must be an integer in 0..4')
    if int(power) != power or not 0 <= power <= 8:
        raise ValueError('bake: power must be an integer in 0..8')
    N = None
    if normals is not None:
        if normal_mat is None:
            raise ValueError('bake: normals need normal_mat')
        normals = np.ascontiguousarray(np.asarray(normals), dtype=np.float32).reshape(-1, 3)
        N = np.ascontiguousarray(np.asarray(normal_mat), dtype=np.float32).reshape(-1, 9)
        if len(normals) != n_points or len(N) != n_views:
            raise ValueError('bake: normals must be [V, 3] and normal_mat [n_views, 3, 3]')
    if fallback is not None:
        fallback = np.asarray(fallback)
        if fallback.dtype != np.uint8 or fallback.shape != (n_points, 3):
            raise ValueError('bake: fallback must be uint8 [V, 3]')
    return A, K, vis, frames, normals, N, fallback


def _bake_gather(v, A, K, vis, frames, normals, N, near, depth_tol, guard, min_cos, power):
    """The bake's rules for the points v float32 [M, 3] (normals [M, 3] with N [n_views, 9], or None), view after view: the port of the stage
    function the vertex bake and the texture bake are built from -> (acc float32 [M, 3], accw float32 [M], seen int32 [M])."""
    n_views = len(A)
    h, w = vis.shape[1:]
    fh, fw = frames.shape[1:3]
    guard, power, tol, min_cos = int(guard), int(power), _F(depth_tol), _F(min_cos)
    V = len(v)
    acc = np.zeros((V, 3), dtype=np.float32)
    accw = np.zeros(V, dtype=np.float32)
    seen = np.zeros(V, dtype=np.int32)
    for view in range(n_views if V else 0):
        with np.errstate(all='ignore'):
            cam, near_bad, _, xc, yc = _raster_point(v, A[view], K[view], near)         # the rasteriser's vertex stage, before it snaps
            sx, sy = xc * _F(w), yc * _F(h)
            idx = np.nonzero(~near_bad & (sx >= 0) & (sx < _F(w)) & (sy >= 0) & (sy < _F(h)))[0]
            p, xc, yc, sx, sy = cam[idx], xc[idx], yc[idx], sx[idx], sy[idx]
            col, row = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
            # occlusion: the whole window, clipped to the image
            open_ = np.ones(len(idx), dtype=bool)
            for dr in range(-guard, guard + 1):
                for dc in range(-guard, guard + 1):
                    r, c = row + dr, col + dc
                    inside = (r >= 0) & (r < h) & (c >= 0) & (c < w)
                    key = vis[view][np.clip(r, 0, h - 1), np.clip(c, 0, w - 1)]
                    z_pix = np.ascontiguousarray((key >> np.uint64(32)).astype(np.uint32)).view(np.float32)
                    passes = (key != RASTER_EMPTY) & (p[:, 2] <= z_pix + tol * z_pix)
                    open_ &= passes | ~inside
            idx, p, xc, yc = idx[open_], p[open_], xc[open_], yc[open_]
            wgt = np.ones(len(idx), dtype=np.float32)
            if normals is not None:
                n, Nv = normals[idx], N[view]
                nc = [_dot3_f32(Nv[3 * r], Nv[3 * r + 1], Nv[3 * r + 2], n[:, 0], n[:, 1], n[:, 2]) for r in range(3)]
                n_p = _dot3_f32(nc[0], nc[1], nc[2], p[:, 0], p[:, 1], p[:, 2])
                nn = _dot3_f32(nc[0], nc[1], nc[2], nc[0], nc[1], nc[2])
                pp = _dot3_f32(p[:, 0], p[:, 1], p[:, 2], p[:, 0], p[:, 1], p[:, 2])
                cosine = (-n_p) / np.sqrt(nn * pp)
                facing = cosine > min_cos
                idx, p, xc, yc, cosine = idx[facing], p[facing], xc[facing], yc[facing], cosine[facing]
                wgt = np.ones(len(idx), dtype=np.float32)
                if power > 0:
                    wgt = cosine
                    for _ in range(1, power):
                        wgt = wgt * cosine
            # bilinear sample at the vertex's own position, the taps clamped into the frame
            u, t = xc * _F(fw) - _F(0.5), yc * _F(fh) - _F(0.5)
            x0f, y0f = np.floor(u), np.floor(t)
            tx, ty = u - x0f, t - y0f
            ux, uy = _F(1) - tx, _F(1) - ty
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            x1, y1 = np.clip(x0 + 1, 0, fw - 1), np.clip(y0 + 1, 0, fh - 1)
            x0, y0 = np.clip(x0, 0, fw - 1), np.clip(y0, 0, fh - 1)
            f = frames[view]
            c00, c01, c10, c11 = (f[y, x].astype(np.float32) for y, x in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
            top = ux[:, None] * c00 + tx[:, None] * c01
            bot = ux[:, None] * c10 + tx[:, None] * c11
            s = uy[:, None] * top + ty[:, None] * bot
            acc[idx] = acc[idx] + wgt[:, None] * s
            accw[idx] = accw[idx] + wgt
            seen[idx] += 1
    return acc, accw, seen


def _bake_levels(acc, accw):
    """rintf(min(max(acc / accw, 0), 255)) as uint8, per row."""
    with np.errstate(all='ignore'):
        return np.rint(np.fmin(np.fmax(acc / accw[:, None], _F(0)), _F(255))).astype(np.int32).astype(np.uint8)


def bake_colors_numpy(verts, mesh2cam, intrinsics, vis, frames, normals=None, normal_mat=None, near=0.01, depth_tol=2.0 ** -8, guard=1, min_cos=0.1,
                      power=2, fallback=None):
    """The numpy port of gnerf_mesh_bake_colors: dict(colors uint8 [V, 3], weight float32 [V], seen int32 [V]).  vis: rasterize_numpy's
    uint64 [n_views, h, w] (or the kernel's int64 bits); frames uint8 [n_views, fh, fw, 3]; normals [V, 3] need normal_mat [n_views, 3, 3]."""
    v = np.ascontiguousarray(np.asarray(verts), dtype=np.float32).reshape(-1, 3)
    V = len(v)
    A, K, vis, frames, normals, N, fallback = _bake_arguments(V, mesh2cam, intrinsics, vis, frames, normals, normal_mat, near, depth_tol, guard, power, fallback)
    acc, accw, seen = _bake_gather(v, A, K, vis, frames, normals, N, near, depth_tol, guard, min_cos, power)
    colors = np.zeros((V, 3), dtype=np.uint8) if fallback is None else fallback.copy()
    hit = accw > 0
    colors[hit] = _bake_levels(acc[hit], accw[hit])
    return dict(colors=colors, weight=accw, seen=seen)


def bake_mesh_colors(verts, faces, frames, cam2world, intrinsics, mesh2world=None, normals=None, vis_size=None, **rules):
    """Colour a mesh's vertices from frames of it: rasterise it from the frames' cameras (cam2world [n, 4, 4] and normalised intrinsics
    [n, 3, 3], as render_mesh takes them) at vis_size (default: the frames' size), then bake (BAKE_RULES' keys and `fallback` pass through
    `rules`) -> dict(colors uint8 [V, 3], weight float32 [V], seen int32 [V]).  CUDA tensors run the gfx950 kernels (gnerf_hip.rasterize /
    bake_colors) and return tensors on their device; numpy arrays run the ports -- the same bits either way.  normals [V, 3] are in the mesh's
    frame; with them the views are weighted by how squarely they face the surface."""
    unknown = set(rules) - set(BAKE_RULES) - {'fallback'}
    if unknown:
        raise ValueError(f'bake: unknown rule(s) {sorted(unknown)}')
    size = tuple(frames.shape[1:3]) if vis_size is None else vis_size
    route, verts, faces = _mesh_route(verts, faces)
    mesh2cam, K, normal_mat = _cameras_on_route(verts, cam2world, intrinsics, mesh2world)
    frames, normals, fallback = (_on_route(x, verts) for x in (frames, normals, rules.get('fallback')))
    vis, _ = route.rasterize(verts, faces, mesh2cam, K, size, near=rules.get('near', BAKE_RULES['near']))
    return route.bake_colors(verts, mesh2cam, K, vis, frames, normals=normals, normal_mat=normal_mat if normals is not None else None,
                             **dict(rules, fallback=fallback))


def bake_report_line(baked, n_views):
    """One line about a bake_colors / bake_mesh_colors result (tensors or arrays) from n_views frames: the number of views, the share of
    vertices at least one of them sees, and the median number of views per seen vertex."""
    seen = to_host(baked['seen'])
    n_seen = int((seen > 0).sum())
    share = n_seen / len(seen) if len(seen) else 0.0
    median = float(np.median(seen[seen > 0])) if n_seen else 0.0
    return f'mesh bake: {int(n_views)} views, {n_seen} of {len(seen)} vertices seen ({100 * share:.1f} %), median {median:g} views per seen vertex'


# ---------------------------------------------------------------------------------------------------------------- texture atlas
# The numpy ports of gnerf_mesh_atlas_layout, gnerf_mesh_bake_texture and gnerf_raster_resolve_textured (csrc/raster.hip; include/gnerf_hip.h
# states the rules): the atlas is a function of (n_tris, patch) alone -- two triangles to a P x P cell, C = ceil(sqrt(n_pairs)) cells to a
# row, corners 0, 1, 2 of half 0 at the texel centres (0, 0), (L, 0), (0, L) of the cell with L = P - 3, half 1 the same rule on
# (P - 1 - i, P - 1 - j) --, the bake runs the colour bake's rules at every owned texel's point b0 v0 + b1 v1 + b2 v2, and the textured resolve
# samples the atlas where a pixel's perspective-correct barycentrics point.  float32, one rounding per operation: the same bits.
ATLAS_MIN_PATCH, ATLAS_MAX_PATCH, ATLAS_MAX_SIZE = 4, 64, 16384


def _atlas_patch(patch):
    if int(patch) != patch or not ATLAS_MIN_PATCH <= patch <= ATLAS_MAX_PATCH:
        raise ValueError(f'atlas: patch must be an integer in {ATLAS_MIN_PATCH}..{ATLAS_MAX_PATCH}')
    return int(patch)


def _atlas_rgb(colour):
    rgb = np.asarray(colour)
    if rgb.shape != (3,) or np.any(rgb < 0) or np.any(rgb > 255) or np.any(rgb != np.floor(rgb)):
        raise ValueError('atlas: background must be three integers in 0..255')
    return rgb.astype(np.uint8)


def atlas_layout(n_tris, patch):
    """The atlas of n_tris triangles at `patch` texels per patch side -> (cells per row C, th, tw): C the smallest integer with C C >= n_pairs,
    n_pairs = (n_tris + 1) // 2, ceil(n_pairs / C) rows of cells; (0, 0, 0) for no triangle.  ValueError past ATLAS_MAX_SIZE texels a side."""
    n_tris, patch = int(n_tris), _atlas_patch(patch)
    if n_tris < 0:
        raise ValueError('atlas: negative triangle count')
    n_pairs = (n_tris + 1) // 2
    cells = 0
    while cells * cells < n_pairs:
        cells += 1
    rows = -(-n_pairs // cells) if cells else 0
    th, tw = rows * patch, cells * patch
    if max(th, tw) > ATLAS_MAX_SIZE:
        raise ValueError(f'atlas: {n_tris} triangles at patch {patch} need {th} x {tw} texels, more than {ATLAS_MAX_SIZE} a side')
    return cells, th, tw


def _atlas_corners(n_tris, patch):
    """Texel indices (x, y) int64 [n_tris, 3] of the three corners of every triangle."""
    cells, _, _ = atlas_layout(n_tris, patch)
    t = np.arange(n_tris, dtype=np.int64)
    pair, half = t >> 1, t & 1
    row, col = (pair // cells, pair % cells) if cells else (pair, pair)
    L = patch - 3
    i, j = np.array([0, L, 0], dtype=np.int64), np.array([0, 0, L], dtype=np.int64)
    i = np.where(half[:, None] == 1, patch - 1 - i, i)
    j = np.where(half[:, None] == 1, patch - 1 - j, j)
    return col[:, None] * patch + i, row[:, None] * patch + j


def atlas_uvs(n_tris, patch):
    """UVs float32 [n_tris, 3, 2] of every face corner: (u, v) = ((x + 0.5) / tw, (y + 0.5) / th) of the corner's texel (x, y), v from the TOP
    row (write_obj flips it)."""
    _, th, tw = atlas_layout(n_tris, patch)
    x, y = _atlas_corners(n_tris, patch)
    if n_tris == 0:
        return np.zeros((0, 3, 2), dtype=np.float32)
    return np.stack([(x + 0.5) / tw, (y + 0.5) / th], axis=-1).astype(np.float32)


def _atlas_texels(n_tris, patch):
    """Per texel of the atlas: (tri int64 [th, tw]: the triangle that owns it or -1, li, lj int64 [th, tw]: its local indices under that
    half's rule, the ones the barycentrics are formed from)."""
    cells, th, tw = atlas_layout(n_tris, patch)
    y, x = np.meshgrid(np.arange(th, dtype=np.int64), np.arange(tw, dtype=np.int64), indexing='ij')
    i, j = x % patch, y % patch
    half = (i + j >= patch).astype(np.int64)
    tri = ((y // patch) * cells + x // patch) * 2 + half
    tri = np.where(tri < n_tris, tri, -1)
    return tri, np.where(half == 1, patch - 1 - i, i), np.where(half == 1, patch - 1 - j, j)


def bake_texture_numpy(verts, faces, mesh2cam, intrinsics, vis, frames, patch=8, normals=None, normal_mat=None, near=0.01, depth_tol=2.0 ** -8, guard=1,
                       min_cos=0.1, power=2, fallback=None, background=(0, 0, 0)):
    """The numpy port of gnerf_mesh_bake_texture: dict(texture uint8 [th, tw, 3], weight float32 [th, tw], seen int32 [th, tw]) of the atlas of
    (len(faces), patch); arguments as bake_colors_numpy takes them, plus faces; fallback uint8 [V, 3] per vertex; background: three values
    0..255.  seen is -1 (and weight 0, the texel the background) where nobody owns the texel or its face names a vertex that is not there."""
    v, f = _raster_mesh(verts, faces)
    V, T = len(v), len(f)
    A, K, vis, frames, normals, N, fallback = _bake_arguments(V, mesh2cam, intrinsics, vis, frames, normals, normal_mat, near, depth_tol, guard, power, fallback)
    background = _atlas_rgb(background)
    _, th, tw = atlas_layout(T, patch)
    texture = np.empty((th, tw, 3), dtype=np.uint8)
    texture[...] = background
    weight = np.zeros((th, tw), dtype=np.float32)
    seen = np.full((th, tw), -1, dtype=np.int32)
    if T == 0:
        return dict(texture=texture, weight=weight, seen=seen)
    tri, li, lj = _atlas_texels(T, patch)
    valid = ((f >= 0) & (f < V)).all(axis=1)
    idx = np.nonzero((tri.ravel() >= 0) & valid[np.maximum(tri.ravel(), 0)])[0]
    g = f[tri.ravel()[idx]].astype(np.int64)
    L = _F(int(patch) - 3)
    b1, b2 = li.ravel()[idx].astype(np.float32) / L, lj.ravel()[idx].astype(np.float32) / L
    b0 = (_F(1) - b1) - b2

    def mix(values):                                                     # (b0 a0 + b1 a1) + b2 a2 of a per-vertex float32 [V, 3]
        return (b0[:, None] * values[g[:, 0]] + b1[:, None] * values[g[:, 1]]) + b2[:, None] * values[g[:, 2]]
    with np.errstate(all='ignore'):
        x = mix(v)
        n = mix(normals) if normals is not None else None
        acc, accw, count = _bake_gather(x, A, K, vis, frames, n, N, near, depth_tol, guard, min_cos, power)
        out = np.broadcast_to(background, (len(idx), 3)).copy()
        if fallback is not None:
            out = np.rint(np.fmin(np.fmax(mix(fallback.astype(np.float32)), _F(0)), _F(255))).astype(np.int32).astype(np.uint8)
    hit = accw > 0
    out[hit] = _bake_levels(acc[hit], accw[hit])
    texture.reshape(-1, 3)[idx] = out
    weight.reshape(-1)[idx] = accw
    seen.reshape(-1)[idx] = count
    return dict(texture=texture, weight=weight, seen=seen)


def resolve_textured_numpy(vis, verts, faces, mesh2cam, intrinsics, texture, patch=8, background=(255, 255, 255)):
    """The numpy port of gnerf_raster_resolve_textured: frame uint8 [n_views, h, w, 3], every covered pixel a bilinear sample of `texture`
    (uint8 [th, tw, 3], the atlas of (len(faces), patch)), unlit; the empty pixels hold `background`."""
    v, f = _raster_mesh(verts, faces)
    A, K = _raster_cameras(mesh2cam, intrinsics)
    vis = np.asarray(vis)
    n_views, h, w = vis.shape
    if len(A) != n_views:
        raise ValueError('raster: vis and the cameras disagree about n_views')
    patch, background = _atlas_patch(patch), _atlas_rgb(background)
    cells, th, tw = atlas_layout(len(f), patch)
    texture = np.asarray(texture)
    if texture.dtype != np.uint8 or texture.shape != (th, tw, 3):
        raise ValueError(f'raster: texture must be the uint8 [{th}, {tw}, 3] atlas of this mesh and patch')
    frame = np.empty((n_views, h, w, 3), dtype=np.uint8)
    frame[...] = background
    n_tris = len(f) if len(v) else 0
    L, far = _F(patch - 3), _F(patch - 1)
    for view in range(n_views):
        key = vis[view].reshape(-1).astype(np.uint64)
        tri = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
        pix = np.nonzero((key != RASTER_EMPTY) & (tri < n_tris))[0]
        if len(pix) == 0:
            continue
        _, iz_v, X, Y, bad = _raster_project(v, A[view], K[view], h, w, 0.0)
        t = _raster_setup(f[tri[pix]], len(v), X, Y, iz_v, bad, 0, h, w)
        keep = t['status'] == 0
        pix = pix[keep]
        t = {k: x[keep] for k, x in t.items()}
        tri = tri[pix]
        _, wa, wb, wc = _raster_cover(t, pix // w, pix % w)
        with np.errstate(all='ignore'):
            iz, _, bb, bc = _raster_iz(t, wa, wb, wc)
            qb, qc = (bb * t['izb']) / iz, (bc * t['izc']) / iz
            q1, q2 = np.where(t['flipped'], qc, qb), np.where(t['flipped'], qb, qc)      # drawn as (0, 2, 1) when flipped
            pair, odd = tri >> 1, (tri & 1) == 1
            lx, ly = q1 * L, q2 * L
            lx, ly = np.where(odd, far - lx, lx), np.where(odd, far - ly, ly)
            u, s = ((pair % cells) * patch).astype(np.float32) + lx, ((pair // cells) * patch).astype(np.float32) + ly
            x0f, y0f = np.floor(u), np.floor(s)
            tx, ty = u - x0f, s - y0f
            ux, uy = _F(1) - tx, _F(1) - ty
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            x1, y1 = np.clip(x0 + 1, 0, tw - 1), np.clip(y0 + 1, 0, th - 1)
            x0, y0 = np.clip(x0, 0, tw - 1), np.clip(y0, 0, th - 1)
            c00, c01, c10, c11 = (texture[y, x].astype(np.float32) for y, x in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
            top = ux[:, None] * c00 + tx[:, None] * c01
            bot = ux[:, None] * c10 + tx[:, None] * c11
            sample = uy[:, None] * top + ty[:, None] * bot
            frame[view].reshape(-1, 3)[pix] = np.rint(np.fmin(np.fmax(sample, _F(0)), _F(255))).astype(np.int32).astype(np.uint8)
    return frame


def bake_mesh_texture(verts, faces, frames, cam2world, intrinsics, patch=8, mesh2world=None, normals=None, vis_size=None, **rules):
    """Texture a mesh from frames of it, as bake_mesh_colors colours its vertices: rasterise it from the frames' cameras at vis_size (default:
    the frames' size), then bake the atlas of (len(faces), patch) (BAKE_RULES' keys, `fallback` and `background` pass through `rules`) ->
    dict(texture uint8 [th, tw, 3], weight float32 [th, tw], seen int32 [th, tw]); atlas_uvs(len(faces), patch) are its UVs.  CUDA tensors run the
    gfx950 kernels (gnerf_hip.rasterize / bake_texture) and return tensors on their device; numpy arrays run the ports -- the same bits."""
    unknown = set(rules) - set(BAKE_RULES) - {'fallback', 'background'}
    if unknown:
        raise ValueError(f'bake: unknown rule(s) {sorted(unknown)}')
    size = tuple(frames.shape[1:3]) if vis_size is None else vis_size
    route, verts, faces = _mesh_route(verts, faces)
    mesh2cam, K, normal_mat = _cameras_on_route(verts, cam2world, intrinsics, mesh2world)
    frames, normals, fallback = (_on_route(x, verts) for x in (frames, normals, rules.get('fallback')))
    vis, _ = route.rasterize(verts, faces, mesh2cam, K, size, near=rules.get('near', BAKE_RULES['near']))
    return route.bake_texture(verts, faces, mesh2cam, K, vis, frames, patch=patch, normals=normals, normal_mat=normal_mat if normals is not None else None,
                              **dict(rules, fallback=fallback))


def texture_report_line(baked, n_views, patch):
    """One line about a bake_texture / bake_mesh_texture result from n_views frames: the atlas' size, the texels some triangle owns, the share
    of them at least one view sees, and the median number of views per seen texel."""
    seen = to_host(baked['seen'])
    th, tw = seen.shape
    owned, n_seen = int((seen >= 0).sum()), int((seen > 0).sum())
    share = n_seen / owned if owned else 0.0
    median = float(np.median(seen[seen > 0])) if n_seen else 0.0
    return (f'mesh texture: {tw} x {th} atlas (patch {int(patch)}), {int(n_views)} views, {n_seen} of {owned} owned texels seen ({100 * share:.1f} %), '
            f'median {median:g} views per seen texel')


# ---------------------------------------------------------------------------------------------------------------- mesh cleaning
# The numpy ports of csrc/mesh_clean.hip (include/gnerf_hip.h, gnerf_mesh_*, states the rules; restated here).  A mesh is verts float32
# [V, 3] and faces int32 [T, 3] as marching_cubes returns them; V == 0 or T == 0 is valid.  A face is VALID iff its three ids lie in [0, V)
# (ids may repeat); an invalid face joins nothing, is counted, dropped by the compaction and ignored by the smoothing.
#   components: a valid face joins its three vertices.  label[v] = the smallest vertex index of v's component; faces_of[l] = the number of
#     valid faces whose first vertex has label l; counts = (components with a face, vertices in no face, invalid faces).  Integers, unique.
#   selection: components with a face by face count descending, then label ascending; kept iff face count >= min_faces and (keep_largest == 0
#     or rank < keep_largest).
#   compaction: a vertex is kept iff its component is (vertices in no face never are), a face iff it is valid and its first vertex is kept;
#     both stay in ascending old index, face ids are remapped, src_vertex holds every new vertex's old index.
#   smoothing: Taubin lambda | mu with uniform weights.  Corner c of every valid face gives vertex f[c] the two neighbours f[c + 1], f[c + 2]
#     (cyclically); m_i = the size of that multiset N(i).  A half-step with factor s (a C float), per coordinate, in float64 with one rounding
#     per operation: c = (sum over N(i) in ascending j, from 0.0, of double(v_j)) / double(m_i); v_i' = float32(double(v_i) + double(s) *
#     (c - double(v_i))).  All vertices move together; an iteration is a half-step with lam, then one with mu.  m_i == 0 never moves; with
#     pin_boundary neither does a vertex with a neighbour that does not occur exactly twice in N(i).
CleanedMesh = collections.namedtuple('CleanedMesh', 'verts faces normals colors src_vertex report')


def _mesh_faces(faces, n_verts):
    """(faces as int64 [T, 3], valid [T])."""
    f = np.asarray(faces)
    if f.size % 3 != 0:
        raise ValueError(f'mesh: faces has shape {f.shape}')
    f = f.reshape(-1, 3).astype(np.int64)
    n_verts = int(n_verts)
    if not 0 <= n_verts < 2 ** 31:
        raise ValueError(f'mesh: n_verts must be in [0, 2^31), got {n_verts}')
    return f, np.all((f >= 0) & (f < n_verts), axis=1)


def mesh_components_numpy(faces, n_verts, check=True):
    """The numpy port of gnerf_mesh_components -> (label int32 [V], faces_of int32 [V], counts int64 [3]).  check: raise ValueError when a face
    names a vertex outside [0, V), as gnerf_hip.mesh_components does (False: such faces are only counted, in counts[2])."""
    f, ok = _mesh_faces(faces, n_verts)
    n_verts = int(n_verts)
    n_bad = int(len(f) - np.count_nonzero(ok))
    if n_bad and check:
        raise ValueError(f'mesh_components: {n_bad} face(s) name a vertex outside [0, {n_verts})')
    g = f[ok]
    parent = np.arange(n_verts, dtype=np.int64)
    a, b = np.concatenate([g[:, 0], g[:, 0]]), np.concatenate([g[:, 1], g[:, 2]])
    while len(a):                                                        # hook the larger root under the smaller, then flatten; an edge whose
        ra, rb = parent[a], parent[b]                                    # ends share a root is settled for good
        open_ = ra != rb
        if not open_.any():
            break
        a, b, ra, rb = a[open_], b[open_], ra[open_], rb[open_]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    label = parent.astype(np.int32)
    faces_of = np.bincount(parent[g[:, 0]], minlength=n_verts).astype(np.int32)
    root = parent == np.arange(n_verts)
    counts = np.array([np.count_nonzero(root & (faces_of > 0)), np.count_nonzero(root & (faces_of == 0)), n_bad], dtype=np.int64)
    return label, faces_of, counts


def mesh_select(faces_of, keep_largest=0, min_faces=0, labels=None):
    """The labels of the kept components, int64, in rank order (face count descending, then label ascending).  faces_of: mesh_components'
    array [V] -- or, with `labels` given, the face counts of just those labels (what a caller that holds faces_of on a GPU sends over)."""
    keep_largest, min_faces = int(keep_largest), int(min_faces)
    if keep_largest < 0 or min_faces < 0:
        raise ValueError('mesh_select: keep_largest and min_faces must be >= 0')
    n = np.asarray(faces_of).astype(np.int64).reshape(-1)
    if labels is None:
        labels = np.nonzero(n)[0]
        n = n[labels]
    else:
        labels = np.asarray(labels).astype(np.int64).reshape(-1)
        if labels.shape != n.shape:
            raise ValueError('mesh_select: one face count per label')
        labels, n = labels[n > 0], n[n > 0]
    order = np.lexsort((labels, -n))
    labels, n = labels[order], n[order]
    kept = n >= min_faces
    if keep_largest > 0:
        kept &= np.arange(len(n)) < keep_largest
    return labels[kept]


def mesh_compact_numpy(verts, faces, label, faces_of, keep):
    """The numpy port of gnerf_mesh_compact_*: keep is bool / uint8 [V], INDEXED BY LABEL -> (verts' float32 [V', 3], faces' int32 [T', 3],
    src_vertex int32 [V'])."""
    v = np.ascontiguousarray(np.asarray(verts), dtype=np.float32).reshape(-1, 3)
    f, ok = _mesh_faces(faces, len(v))
    label, faces_of, keep = (np.asarray(x).reshape(-1) for x in (label, faces_of, keep))
    if not len(label) == len(faces_of) == len(keep) == len(v):
        raise ValueError('mesh_compact: label, faces_of and keep hold one value per vertex')
    label = label.astype(np.int64)
    vkeep = (keep[label] != 0) & (faces_of[label] > 0)
    fkeep = ok.copy()
    fkeep[ok] = vkeep[f[ok, 0]]
    newid = np.cumsum(vkeep) - 1
    return v[vkeep], newid[f[fkeep]].astype(np.int32).reshape(-1, 3), np.nonzero(vkeep)[0].astype(np.int32)


def _mesh_rows(faces, n_verts):
    """The sorted neighbour rows: (nbr int64 [6 T'] row after row, each ascending; deg int64 [V]; start int64 [V]; odd bool [V]: some neighbour
    does not occur exactly twice)."""
    f, ok = _mesh_faces(faces, n_verts)
    g = f[ok]
    owner = np.concatenate([g[:, c] for c in range(3) for _ in range(2)])
    nbr = np.concatenate([g[:, (c + k) % 3] for c in range(3) for k in (1, 2)])
    order = np.lexsort((nbr, owner))
    owner, nbr = owner[order], nbr[order]
    deg = np.bincount(owner, minlength=n_verts).astype(np.int64)
    odd = np.zeros(n_verts, dtype=bool)
    pairs, times = np.unique(owner << 32 | nbr, return_counts=True)
    odd[pairs[times != 2] >> 32] = True
    return nbr, deg, np.cumsum(deg) - deg, odd


def mesh_smooth_numpy(verts, faces, iterations, lam=0.5, mu=-0.53, pin_boundary=True):
    """The numpy port of gnerf_mesh_smooth -> the new positions, float32 [V, 3], the kernel's bits."""
    cur = np.array(np.asarray(verts), dtype=np.float32).reshape(-1, 3)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f'mesh_smooth: iterations must be >= 0, got {iterations}')
    if iterations == 0 or len(cur) == 0:
        return cur
    nbr, deg, start, odd = _mesh_rows(faces, len(cur))
    move = np.nonzero((deg > 0) & ~(odd & bool(pin_boundary)))[0]
    m, first = deg[move], start[move]
    m64 = m.astype(np.float64)[:, None]
    for step in range(2 * iterations):
        s = np.float64(np.float32(mu if step & 1 else lam))
        x = cur.astype(np.float64)
        acc = np.zeros((len(move), 3), dtype=np.float64)
        for k in range(int(m.max()) if len(m) else 0):                  # the k-th neighbour of every row that has one: ascending j per row
            sel = m > k
            acc[sel] += x[nbr[first[sel] + k]]
        xm = x[move]
        nxt = cur.copy()
        nxt[move] = (xm + s * (acc / m64 - xm)).astype(np.float32)
        cur = nxt
    return cur


def _gather(attribute, src_vertex):
    """A per-vertex attribute (or None) at the vertices src_vertex names: with a device index on the GPU route, on the host otherwise."""
    if attribute is None:
        return None
    return _on_route(attribute, src_vertex)[src_vertex.long() if is_gpu(src_vertex) else src_vertex]


def clean_mesh(verts, faces, keep_largest=0, min_faces=0, smooth=0, lam=0.5, mu=-0.53, pin_boundary=True, normals=None, colors=None):
    """Keep the large pieces of a mesh, drop the rest, fair the surface: components -> selection (keep_largest: at most that many components,
    0 = no limit; min_faces: only components with at least that many faces) -> compaction -> `smooth` Taubin iterations.  CUDA tensors run the
    gfx950 kernels (gnerf_hip.mesh_components / mesh_compact / mesh_smooth) and return tensors on their device; numpy arrays and CPU tensors
    run the numpy ports and return numpy arrays -- the same bits either way.  -> CleanedMesh(verts, faces, normals, colors, src_vertex, report):
    normals / colors are the given per-vertex arrays gathered at the kept vertices (None when not given; smoothing does not touch them), src_vertex
    the old index of every new vertex, report a dict: components, kept, faces, kept_faces, share (kept_faces / faces), vertices, kept_vertices."""
    route, verts, faces = _mesh_route(verts, faces)
    xp = route.xp
    label, faces_of, counts = route.components(faces, len(verts))
    roots = xp.where(faces_of > 0)[0]                                    # of the GPU route's arrays only the labels with faces and
    roots, sizes = to_host(roots), to_host(faces_of[roots])             # their face counts travel to the host, for the selection
    kept = mesh_select(sizes, keep_largest, min_faces, labels=roots)
    keep = xp.zeros_like(faces_of, dtype=xp.uint8)
    keep[_on_route(kept, keep)] = 1
    v, f, src = route.compact(verts, faces, label, faces_of, keep)
    normals, colors = _gather(normals, src), _gather(colors, src)
    if smooth:
        v = route.smooth(v, f, smooth, lam, mu, pin_boundary)
    kept_faces, n_faces = int(sizes[np.isin(roots, kept)].sum(dtype=np.int64)), int(sizes.sum(dtype=np.int64))
    report = dict(components=int(counts[0]), kept=int(len(kept)), faces=n_faces, kept_faces=kept_faces, share=kept_faces / n_faces if n_faces else 1.0,
                  vertices=int(len(verts)), kept_vertices=int(len(v)))
    return CleanedMesh(v, f, normals, colors, src, report)


def clean_report_line(report, smooth=0):
    """The one stdout line of the CLIs about a clean_mesh report."""
    return (f'mesh cleaning: kept {report["kept"]} of {report["components"]} component(s), {report["kept_faces"]} of {report["faces"]} triangles '
            f'({100 * report["share"]:.2f} %), {report["kept_vertices"]} of {report["vertices"]} vertices' + (f'; {smooth} Taubin iteration(s)' if smooth else ''))


def clean_options(keep_largest=0, min_faces=0, smooth=0):
    """The CLIs' three flags (--mesh-keep, --mesh-min-faces, --mesh-smooth) as clean_mesh keywords, or None when all are 0 (nothing runs)."""
    opts = dict(keep_largest=int(keep_largest), min_faces=int(min_faces), smooth=int(smooth))
    if min(opts.values()) < 0:
        raise ValueError('--mesh-keep, --mesh-min-faces and --mesh-smooth must be >= 0')
    return opts if any(opts.values()) else None


# ---------------------------------------------------------------------------------------------------------------- mesh simplification
# The numpy port of csrc/mesh_simplify.hip (include/gnerf_hip.h, gnerf_mesh_simplify_*, states the rules; restated here): vertex clustering on
# a uniform grid with a quadric-error representative per cell.  Parameters: cell (a C float > 0) and origin (three C floats).  Every float64
# operation is rounded on its own (no contraction); only + - * /, floor, comparisons and integer conversion occur, so the kernels give these bits.
#   1 valid faces: a face is VALID iff its three ids lie in [0, V) and its three vertices are finite; invalid faces are counted and ignored.  A
#     vertex is USED iff a valid face names it; unused vertices are dropped.
#   2 cells: per axis p = (double(v) - double(origin)) / double(cell), k = floor(p) clamped to [0, 2^21 - 1]; key = kx 2^42 + ky 2^21 + kz.  A
#     cluster = the used vertices of one key, its representative = its smallest vertex index; new ids number the representatives in ascending
#     old index (src_vertex).  u = p - (k + 0.5), clamped to [-0.5, 0.5] (which only a vertex outside the 2^21-cell grid feels).
#   3 accumulation in int64 fixed point, q(x) = llrint(x 2^32) (sums wrap modulo 2^64), so any order gives the same bits:
#     per used vertex into its cluster: q(u) per axis and a member count;
#     per valid face, read from its corner with the smallest id (rotated, never reflected: 0, 1, 2 below are that order): e1 = p1 - p0,
#     e2 = p2 - p0, n = e1 x e2 (n0 = e1y e2z - e1z e2y, ...), s = (n0 n0 + n1 n1) + n2 n2; the face is skipped unless 0 < s < inf;
#     f = 16 / s if s > 16 else 1; per corner c into the cluster of its vertex: d = (n0 u0 + n1 u1) + n2 u2 with u of that vertex, the six
#     q((f n_a) n_b), a <= b, and the three q(n_a (f d)).
#   4 position: A, b = the sums / 2^32 as doubles; cen = (the u sums / 2^32) / members; tr = (A00 + A11) + A22, mu = tr / 256.  If tr > 0,
#     x solves (A + mu I) x = b + mu cen by the elimination written out in _simplify_solve (no pivoting; x = cen if a pivot is not > 0 or x is not finite),
#     else x = cen; x is clamped to [-0.5, 0.5]; the vertex is float32(double(origin) + ((k + 0.5) + x) double(cell)).
#   5 faces: a valid face mapped through the new ids is COLLAPSED when two ids coincide, and dropped; the others are grouped by their id set.
#     sigma = the sum over the group of +1 for a rotation of the ascending triple, -1 otherwise; the group gives one face iff sigma is odd:
#     (a, b, c) ascending when sigma > 0, else (a, c, b); output faces are ordered by their group's smallest old face index.
#   6 counts int64 [8] = V', T', invalid faces, collapsed faces, faces absorbed by grouping, groups with |sigma| >= 2, internal error, 0.
SimplifiedMesh = collections.namedtuple('SimplifiedMesh', 'verts faces normals colors src_vertex vertex_map report')
MESH_SIMPLIFY_GRID = 2 ** 21                                             # cells per axis that a key holds
MESH_SIMPLIFY_CANDIDATES = 41                                            # the target search's cells: base * 2^(j / 4), j = 0 .. 40
_Q32 = 4294967296.0


def _simplify_params(cell, origin):
    cell = np.float32(cell)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError(f'mesh_simplify: cell must be a finite float32 > 0, got {cell}')
    origin = np.asarray(origin, dtype=np.float32).reshape(-1)
    if origin.shape != (3,) or not np.all(np.isfinite(origin)):
        raise ValueError('mesh_simplify: origin must be three finite floats')
    return cell, origin


def _simplify_q(x):
    return np.rint(x * _Q32).astype(np.int64)


def _simplify_solve(A, b, cen, members):
    """Rule 4 for every cluster at once: A [6, C] (00 01 02 11 12 22), b [3, C], cen [3, C] -> x [3, C] in [-0.5, 0.5]."""
    m00, m01, m02, m11, m12, m22 = A
    tr = (m00 + m11) + m22
    mu = tr / 256.0
    with np.errstate(all='ignore'):
        m00, m11, m22 = m00 + mu, m11 + mu, m22 + mu
        r0, r1, r2 = b[0] + mu * cen[0], b[1] + mu * cen[1], b[2] + mu * cen[2]
        l10, l20 = m01 / m00, m02 / m00
        m11, m12b, m22 = m11 - l10 * m01, m12 - l10 * m02, m22 - l20 * m02
        r1, r2 = r1 - l10 * r0, r2 - l20 * r0
        l21 = m12b / m11
        m22, r2 = m22 - l21 * m12b, r2 - l21 * r1
        x2 = r2 / m22
        x1 = (r1 - m12b * x2) / m11
        x0 = ((r0 - m01 * x1) - m02 * x2) / m00
        solved = (tr > 0) & (m00 > 0) & (m11 > 0) & (m22 > 0) & np.isfinite(x0) & np.isfinite(x1) & np.isfinite(x2)
    x = np.where(solved, np.stack([x0, x1, x2]), cen)
    return np.minimum(np.maximum(x, -0.5), 0.5)


def mesh_simplify_numpy(verts, faces, cell, origin, count_only=False):
    """The numpy port of gnerf_mesh_simplify_count / _emit -> (verts' float32 [V', 3], faces' int32 [T', 3], src_vertex int32 [V'], vertex_map
    int32 [V]: the new id of every old vertex or -1, counts int64 [8]); count_only: just the counts (no quadrics, as the count call)."""
    v = np.ascontiguousarray(np.asarray(verts), dtype=np.float32).reshape(-1, 3)
    f, ok = _mesh_faces(faces, len(v))
    cell, origin = _simplify_params(cell, origin)
    nv, nt = len(v), len(f)
    finite = np.all(np.isfinite(v), axis=1)
    ok = ok.copy()
    ok[ok] = np.all(finite[f[ok]], axis=1)
    g = f[ok]                                                            # the valid faces, in order
    used = np.zeros(nv, dtype=bool)
    used[g.reshape(-1)] = True
    old = np.nonzero(used)[0]                                            # used vertices, ascending
    with np.errstate(all='ignore'):
        p = (v[old].astype(np.float64) - origin.astype(np.float64)) / np.float64(cell)
    k = np.minimum(np.maximum(np.floor(p), 0.0), float(MESH_SIMPLIFY_GRID - 1)).astype(np.int64)
    key = (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)       # first: the first (smallest) member of every key
    rank = np.argsort(np.argsort(first))                                 # unique-key number -> new id (representatives in ascending old index)
    src = old[np.sort(first)].astype(np.int32)
    cluster = rank[inverse.reshape(-1)]                                  # new id of every used vertex
    vmap = np.full(nv, -1, dtype=np.int32)
    vmap[old] = cluster
    # faces: collapse, group, parity
    h = vmap[g].astype(np.int64).reshape(-1, 3)
    a, b, c = h[:, 0], h[:, 1], h[:, 2]
    alive = (a != b) & (b != c) & (a != c)
    n_collapsed = int(len(g) - np.count_nonzero(alive))
    h = h[alive]
    a, b, c = h[:, 0], h[:, 1], h[:, 2]
    sign = np.where((a < b).astype(np.int64) + (b < c) + (c < a) == 2, 1, -1)
    tri = np.sort(h, axis=1)
    order = np.lexsort((np.arange(len(tri)), tri[:, 2], tri[:, 1], tri[:, 0]))
    ts = tri[order]
    head = np.ones(len(ts), dtype=bool)
    head[1:] = np.any(ts[1:] != ts[:-1], axis=1)
    group = np.cumsum(head) - 1                                          # group number of every sorted face
    sigma = np.bincount(group, weights=sign[order], minlength=int(head.sum())).astype(np.int64)
    leader = order[head]                                                 # the smallest face of every group (the sort is by face last)
    out = sigma % 2 != 0
    by_leader = np.argsort(leader[out])
    tri_out, sig_out = ts[head][out][by_leader], sigma[out][by_leader]
    new_faces = np.where((sig_out > 0)[:, None], tri_out, tri_out[:, [0, 2, 1]]).astype(np.int32).reshape(-1, 3)
    counts = np.array([len(src), len(new_faces), nt - len(g), n_collapsed, len(h) - len(new_faces), np.count_nonzero(np.abs(sigma) >= 2), 0, 0], dtype=np.int64)
    if count_only:
        return counts
    # quadrics
    n_new = len(src)
    u = np.minimum(np.maximum(p - (k.astype(np.float64) + 0.5), -0.5), 0.5)
    acc = np.zeros((13, n_new), dtype=np.int64)                          # u sums, members, the six of A, the three of b
    qu = _simplify_q(u)
    for axis in range(3):
        np.add.at(acc[axis], cluster, qu[:, axis])
    np.add.at(acc[3], cluster, 1)
    where = np.full(nv, -1, dtype=np.int64)
    where[old] = np.arange(len(old))
    lowest = np.argmin(g, axis=1) if len(g) else np.zeros(0, dtype=np.int64)
    rows = np.arange(len(g))
    g = np.stack([g[rows, (lowest + j) % 3] for j in range(3)], axis=1) if len(g) else g
    w = where[g].reshape(-1, 3)                                          # rows of p / u / cluster of the three corners
    with np.errstate(all='ignore'):
        e1, e2 = p[w[:, 1]] - p[w[:, 0]], p[w[:, 2]] - p[w[:, 0]]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        s = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        take = (s > 0) & (s < np.inf)
    n, s, w = n[take], s[take], w[take]
    scale = np.ones(len(s))
    scale[s > 16.0] = 16.0 / s[s > 16.0]
    fn = scale[:, None] * n
    quad = [_simplify_q(fn[:, i] * n[:, j]) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    for corner in range(3):
        uc, target = u[w[:, corner]], cluster[w[:, corner]]
        d = (n[:, 0] * uc[:, 0] + n[:, 1] * uc[:, 1]) + n[:, 2] * uc[:, 2]
        fd = scale * d
        for i in range(6):
            np.add.at(acc[4 + i], target, quad[i])
        for axis in range(3):
            np.add.at(acc[10 + axis], target, _simplify_q(n[:, axis] * fd))
    members = acc[3].astype(np.float64)
    cen = (acc[0:3].astype(np.float64) / _Q32) / members
    x = _simplify_solve(acc[4:10].astype(np.float64) / _Q32, acc[10:13].astype(np.float64) / _Q32, cen, members)
    krep = k[where[src.astype(np.int64)]].astype(np.float64).T           # [3, V']
    pos = origin.astype(np.float64)[:, None] + ((krep + 0.5) + x) * np.float64(cell)
    return np.ascontiguousarray(pos.T.astype(np.float32)).reshape(-1, 3), np.ascontiguousarray(new_faces), src, vmap, counts


def simplify_candidates(base):
    """The cells the target search may choose: float32(base * 2^(j / 4)), j = 0 .. 40 (a factor of 1024 in all)."""
    return [float(np.float32(float(base) * 2.0 ** (j / 4))) for j in range(MESH_SIMPLIFY_CANDIDATES)]


def simplify_search(count_faces, target_faces, n=MESH_SIMPLIFY_CANDIDATES):
    """Bisect j in [0, n) for the smallest candidate whose face count count_faces(j) is <= target_faces, taking the count to fall as the cell
    grows -> (j, calls, met): at most ceil(log2 n) + 1 calls; met is False when even the coarsest candidate leaves more faces (j = n - 1)."""
    seen = {}

    def passes(j):
        if j not in seen:
            seen[j] = count_faces(j) <= target_faces
        return seen[j]
    lo, hi = 0, n - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if passes(mid):
            hi = mid
        else:
            lo = mid + 1
    met = passes(lo)
    return lo, len(seen), met


def simplify_mesh(verts, faces, cell=None, target_faces=0, origin=None, normals=None, colors=None):
    """Simplify a mesh by vertex clustering with quadrics: one vertex per occupied cell of a grid of edge `cell` with its corner at `origin`
    (default: the per-axis minimum of the finite vertices).  target_faces > 0 picks the cell instead: the smallest of simplify_candidates(cell
    or 1.0) that leaves at most that many faces, found by bisection on the count call alone.  CUDA tensors run the gfx950 kernels
    (gnerf_hip.mesh_simplify / mesh_simplify_count) and return tensors on their device; numpy arrays and CPU tensors run mesh_simplify_numpy and
    return numpy arrays -- the same bits either way.  -> SimplifiedMesh(verts, faces, normals, colors, src_vertex, vertex_map, report): normals /
    colors are the given per-vertex arrays gathered at src_vertex (None when not given), report a dict: cell, origin, target_faces, j and
    count_calls (None / 0 without a target), met, vertices, faces, new_vertices, new_faces, invalid, collapsed, absorbed, multi."""
    target_faces = int(target_faces)
    if target_faces < 0:
        raise ValueError(f'simplify_mesh: target_faces must be >= 0, got {target_faces}')
    if cell is None and target_faces == 0:
        raise ValueError('simplify_mesh: give a cell, a target_faces > 0, or both')
    route, verts, faces = _mesh_route(verts, faces)
    xp = route.xp
    finite = verts[xp.isfinite(verts).all(1)]
    lo_hi = to_host(xp.stack([xp.amin(finite, 0), xp.amax(finite, 0)])) if len(finite) else np.zeros((2, 3), np.float32)
    origin = lo_hi[0] if origin is None else origin
    base, origin = _simplify_params(1.0 if cell is None else cell, origin)
    if np.any((lo_hi[1].astype(np.float64) - origin.astype(np.float64)) / np.float64(base) >= MESH_SIMPLIFY_GRID):
        raise ValueError(f'simplify_mesh: the mesh spans {MESH_SIMPLIFY_GRID} cells or more of edge {base} along an axis')
    j, calls, met = None, 0, True
    if target_faces:
        cells = simplify_candidates(base)
        j, calls, met = simplify_search(lambda i: int(route.simplify_count(verts, faces, cells[i], origin)[1]), target_faces)
        base = np.float32(cells[j])
    v, f, src, vmap, counts = route.simplify(verts, faces, float(base), origin)
    normals, colors = _gather(normals, src), _gather(colors, src)
    c = [int(x) for x in counts]
    report = dict(cell=float(base), origin=tuple(float(x) for x in origin), target_faces=target_faces, j=j, count_calls=calls, met=bool(met),
                  vertices=int(len(verts)), faces=int(c[1] + c[2] + c[3] + c[4]), new_vertices=c[0], new_faces=c[1], invalid=c[2], collapsed=c[3], absorbed=c[4],
                  multi=c[5])
    return SimplifiedMesh(v, f, normals, colors, src, vmap, report)


def simplify_report_line(report):
    """The one stdout line of the CLIs about a simplify_mesh report."""
    search = (f', candidate {report["j"]} for at most {report["target_faces"]} faces after {report["count_calls"]} count call(s)'
              + ('' if report['met'] else ' (not met)')) if report['target_faces'] else ''
    return (f'mesh simplification: cell {report["cell"]:g}{search}: {report["new_faces"]} of {report["faces"]} triangles, {report["new_vertices"]} of '
            f'{report["vertices"]} vertices ({report["collapsed"]} collapsed, {report["absorbed"]} absorbed, {report["invalid"]} invalid)')


def simplify_options(cell=0.0, target_faces=0, voxel=1.0):
    """The CLIs' two flags (--mesh-simplify CELL, in voxels of edge `voxel`, and --mesh-target-faces N) as simplify_mesh keywords, or None when
    both are 0 (nothing runs)."""
    cell, target_faces = float(cell), int(target_faces)
    if not 0 <= cell < float('inf') or target_faces < 0:
        raise ValueError('--mesh-simplify and --mesh-target-faces must be >= 0')
    if not cell and not target_faces:
        return None
    return dict(cell=(cell if cell else 1.0) * float(voxel), target_faces=target_faces)


# ---------------------------------------------------------------------------------------------------------------- snapping to the level set
# The last stage, after the smoothing: gen_videos_mi355x.snap_extracted_mesh projects the vertices onto sigma = level with the generator's own
# density and gradient (gnerf_hip.project_points_to_level) and then runs the flip guard below, the numpy port of gnerf_mesh_flip_guard
# (include/gnerf_hip.h states the rules; restated here).  The normal of a face (a, b, c) is n = (b - a) x (c - a) in float64 from the float32
# coordinates, a dot product (x0 y0 + x1 y1) + x2 y2, every operation rounded on its own.  With n0 at verts_in and n1 at the current positions a
# face is FLIPPED iff n0.n1 < 0, or n1.n1 == 0 and n0.n0 > 0 (an input face of zero area is never flipped); faces with an id outside [0, V)
# are skipped.  Round j: the vertices of all faces flipped at the start of the round get status 3 and counts[j] = the number of those faces;
# then every vertex of status 3 is set back to verts_in.  A round whose predecessor counted 0 does nothing.  counts[R] = the flips left.
def _face_normals64(v, g):
    a, b, c = (v[g[:, k]].astype(np.float64) for k in range(3))
    e1, e2 = b - a, c - a
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def mesh_flipped_faces(verts_in, verts_now, faces):
    """bool [T]: the faces the move verts_in -> verts_now turned over, by the rule above (False for a face with an id out of range)."""
    v0 = np.ascontiguousarray(np.asarray(verts_in), dtype=np.float32).reshape(-1, 3)
    v1 = np.ascontiguousarray(np.asarray(verts_now), dtype=np.float32).reshape(-1, 3)
    f, ok = _mesh_faces(faces, len(v0))
    flipped = np.zeros(len(f), dtype=bool)
    g = f[ok]
    with np.errstate(all='ignore'):
        n0, n1 = _face_normals64(v0, g), _face_normals64(v1, g)
        flipped[ok] = (_dot3(n0, n1) < 0) | ((_dot3(n1, n1) == 0) & (_dot3(n0, n0) > 0))
    return flipped


def mesh_flip_guard_numpy(verts_in, verts_moved, faces, status=None, rounds=4):
    """The numpy port of gnerf_mesh_flip_guard -> (verts_out float32 [V, 3], status uint8 [V], counts int32 [rounds + 1]), the kernels' bits."""
    v0 = np.ascontiguousarray(np.asarray(verts_in), dtype=np.float32).reshape(-1, 3)
    cur = np.array(np.asarray(verts_moved), dtype=np.float32).reshape(-1, 3)
    if cur.shape != v0.shape:
        raise ValueError('mesh_flip_guard: verts_in and verts_moved must have one shape')
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError(f'mesh_flip_guard: rounds must be >= 1, got {rounds}')
    st = np.zeros(len(v0), dtype=np.uint8) if status is None else np.array(np.asarray(status), dtype=np.uint8).reshape(-1)
    if len(st) != len(v0):
        raise ValueError('mesh_flip_guard: status must hold one value per vertex')
    if (st == 3).any():
        raise ValueError('mesh_flip_guard: status 3 (reverted) is the guard\'s to set')
    f, _ = _mesh_faces(faces, len(v0))
    counts = np.zeros(rounds + 1, dtype=np.int32)
    for j in range(rounds + 1):
        if j and counts[j - 1] == 0:
            break
        flipped = mesh_flipped_faces(v0, cur, f)
        counts[j] = np.count_nonzero(flipped)
        if j < rounds and counts[j]:
            st[f[flipped].reshape(-1)] = 3
            back = st == 3
            cur[back] = v0[back]
    return cur, st, counts


def snap_options(radius=0.0, steps=6, tol=None, guard_rounds=4):
    """The CLI's flags (--mesh-snap R in voxels, --mesh-snap-steps, --mesh-snap-tol) as snap_extracted_mesh's dict, or None when R is 0
    (nothing runs).  tol None: 2^-10 max(1, |level|), chosen where the level is known."""
    radius, steps, guard_rounds = float(radius), int(steps), int(guard_rounds)
    if not 0 <= radius < float('inf'):
        raise ValueError('--mesh-snap must be a finite number of voxels >= 0')
    if steps < 0:
        raise ValueError('--mesh-snap-steps must be >= 0')
    if tol is not None and not 0 < float(tol) < float('inf'):
        raise ValueError('--mesh-snap-tol must be finite and > 0')
    if guard_rounds < 1:
        raise ValueError('the flip guard needs at least one round')
    if not radius:
        return None
    return dict(radius=radius, steps=steps, tol=None if tol is None else float(tol), guard_rounds=guard_rounds)


def snap_report_line(report):
    """The one stdout line of the CLIs about a snap_extracted_mesh report."""
    left = report['flips_left']
    return (f'mesh snap: {report["converged"]} of {report["vertices"]} vertices on the level set, {report["not_converged"]} not converged, '
            f'{report["flat"]} flat, {report["reverted"]} reverted by the flip guard (flips per round {report["flips"]}, '
            + (f'{left} LEFT' if left else 'none left') + f'); |sigma - level| median {report["median_before"]:.3g} -> {report["median_after"]:.3g}, '
            f'max {report["max_before"]:.3g} -> {report["max_after"]:.3g}')


# ---------------------------------------------------------------------------------------------------------------- the pipeline
# What both CLIs do to a mesh marching cubes just made, in the one order there is.  The stages that need the generator (the snap, the vertex
# attributes, the bake) come in as callables, so that this module works from a volume alone.
MESH_STAGES = ('clean', 'simplify', 'snap', 'bake')                      # the stages that report, in the order they run
FinishedMesh = collections.namedtuple('FinishedMesh', 'verts faces normals colors baked reports')


class Written(tuple):
    """What a function that writes a mesh file returns: the plain tuple of counts its callers unpack, with the FinishedMesh it wrote (reports
    included) as the attribute `mesh`."""
    def __new__(cls, counts, mesh):
        self = super().__new__(cls, counts)
        self.mesh = mesh
        return self


def finish_mesh(verts, faces, clean=None, simplify=None, snap=None, attributes=None, bake=None, texture=None):
    """Every stage between marching cubes and the consumers of its mesh (verts [V, 3], faces [T, 3]: CUDA tensors take the kernels and stay
    on their device, numpy arrays take the ports, a CPU tensor becomes numpy here) -> FinishedMesh(verts, faces, normals, colors, baked, reports).
      clean, simplify: clean_options' / simplify_options' dict, or None (the stage does not run);
      snap(verts, faces) -> (verts, report); attributes(verts) -> (normals or None, colors or None);
      bake(verts, faces, normals, colors) -> bake_mesh_colors' dict: callables on this route's arrays, or None;
      texture(verts, faces, normals, colors) -> bake_mesh_texture's dict, run after the bake on the same final mesh: its result is
      reports['texture'] (the record keeps its six fields; MESH_STAGES and report_lines leave it to the caller, who knows the patch).
    normals and colors are the attributes' (the decoder's colours; the baked ones are baked['colors']), baked is the bake's dict or None, and
    reports holds the report of every stage of MESH_STAGES that ran, in that order (the bake's is its dict)."""
    route, verts, faces = _mesh_route(verts, faces)
    reports = {}
    if clean:                                                            # components, selection, compaction
        cleaned = clean_mesh(verts, faces, keep_largest=clean['keep_largest'], min_faces=clean['min_faces'])
        verts, faces, reports['clean'] = cleaned.verts, cleaned.faces, cleaned.report
    if simplify:
        simplified = simplify_mesh(verts, faces, **simplify)
        verts, faces, reports['simplify'] = simplified.verts, simplified.faces, simplified.report
    # Normally the attributes are those of the extracted surface: they are evaluated at the kept (or simplified) vertices where marching
    # cubes put them, and only then does the smoothing move the positions.  A snap puts the vertices where they stay, on the level set, so
    # with one the smoothing comes first, then the snap, and the attributes are evaluated at the final positions.
    smooth = clean['smooth'] if clean else 0
    normals = colors = baked = None
    if snap:
        if smooth:
            verts = route.smooth(verts, faces, smooth)
        verts, reports['snap'] = snap(verts, faces)
    if attributes:
        normals, colors = (_on_route(x, verts) for x in attributes(verts))
    if smooth and not snap:
        verts = route.smooth(verts, faces, smooth)
    if bake:                                                             # the final mesh; the attributes' colours stay where no frame sees
        baked = reports['bake'] = bake(verts, faces, normals, colors)
    if texture:
        reports['texture'] = texture(verts, faces, normals, colors)
    return FinishedMesh(verts, faces, normals, colors, baked, reports)


def report_lines(reports, smooth=0, bake_views=0):
    """The CLIs' stdout lines about finish_mesh's reports, one per stage that ran, in stage order (smooth: the Taubin iterations the cleaning
    line names; bake_views: the number of frames the bake took)."""
    line = dict(clean=lambda r: clean_report_line(r, smooth), simplify=simplify_report_line, snap=snap_report_line,
                bake=lambda r: bake_report_line(r, bake_views))
    return [line[stage](reports[stage]) for stage in MESH_STAGES if stage in reports]


def add_mesh_arguments(parser, attributes=False, texture=False):
    """Declare the flags of clean_options and simplify_options on a CLI's parser.  attributes: the CLI evaluates vertex attributes (the
    help says where in the order).  texture: the CLI has frames to bake, and gets --mesh-texture / --mesh-texture-out (texture_from_args
    checks them)."""
    parser.add_argument('--mesh-keep', type=int, default=0, help='keep only this many of the largest connected components of the mesh (0: all)')
    parser.add_argument('--mesh-min-faces', type=int, default=0, help='drop connected components with fewer triangles than this (0: none)')
    parser.add_argument('--mesh-smooth', type=int, default=0, help='Taubin smoothing iterations of the mesh (lambda 0.5, mu -0.53, boundaries pinned; 0: none)')
    parser.add_argument('--mesh-simplify', type=float, default=0, metavar='CELL',
                        help='simplify the mesh by vertex clustering on a grid of cells this many voxels wide, after the components, before '
                             + ('the attributes and ' if attributes else '') + 'the smoothing (0: off)')
    parser.add_argument('--mesh-target-faces', type=int, default=0, metavar='N',
                        help='pick the cell instead: the smallest of CELL (or one voxel) * 2^(j / 4), j = 0 .. 40, that leaves at most N triangles (0: off)')
    if texture:
        parser.add_argument('--mesh-texture', type=int, default=0, metavar='P',
                            help=f'also bake a texture atlas of the final mesh from the frames of --mesh-bake, two triangles to a cell of P x P texels '
                                 f'({ATLAS_MIN_PATCH}..{ATLAS_MAX_PATCH}; 0: off); needs --mesh-bake and --mesh-texture-out')
        parser.add_argument('--mesh-texture-out', default=None, metavar='PATH.obj',
                            help='where --mesh-texture writes the textured mesh: this .obj, its .mtl and its .png beside it')


def mesh_options_from_args(args, parser):
    """(clean, simplify, snap): the option dicts of the parsed flags (None: the stage does not run; snap is None on a parser without
    --mesh-snap).  A value out of range ends the program through parser.error."""
    try:
        return (clean_options(args.mesh_keep, args.mesh_min_faces, args.mesh_smooth), simplify_options(args.mesh_simplify, args.mesh_target_faces),
                snap_options(args.mesh_snap, args.mesh_snap_steps, args.mesh_snap_tol) if hasattr(args, 'mesh_snap') else None)
    except ValueError as err:
        parser.error(str(err))


def texture_from_args(args, parser):
    """The patch size of --mesh-texture (0: off) once the flags add_mesh_arguments(texture=True) declared are in range and have what they
    need; anything else ends the program through parser.error."""
    patch, out = args.mesh_texture, args.mesh_texture_out
    if patch == 0:
        if out:
            parser.error('--mesh-texture-out requires --mesh-texture')
        return 0
    if not ATLAS_MIN_PATCH <= patch <= ATLAS_MAX_PATCH:
        parser.error(f'--mesh-texture must be 0 or {ATLAS_MIN_PATCH}..{ATLAS_MAX_PATCH}')
    if not getattr(args, 'mesh_bake', 0):
        parser.error('--mesh-texture requires --mesh-bake')
    if not out or not out.lower().endswith('.obj'):
        parser.error('--mesh-texture requires --mesh-texture-out PATH.obj')
    return patch


# ---------------------------------------------------------------------------------------------------------------- OBJ and PNG
def _png_chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, rgb):
    """8-bit RGB PNG of rgb uint8 [h, w, 3] (h, w >= 1), written with zlib and struct alone: IHDR, one IDAT of rows with filter type 0, IEND."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError('write_png: rgb must be uint8 [h, w, 3] with h, w >= 1')
    h, w = rgb.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)                      # (filter byte 0 in front of every row)
    rows[:, 1:] = rgb.reshape(h, 3 * w)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n')
        f.write(_png_chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)))
        f.write(_png_chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)))
        f.write(_png_chunk(b'IEND', b''))


def write_obj(path, verts, faces, uvs, texture_png, normals=None):
    """Wavefront OBJ of a textured mesh: `path`, the material library <stem>.mtl beside it, and the texture.  uvs float [T, 3, 2] (atlas_uvs:
    one per face corner, v from the top row) become one `vt u 1-v` each, in OBJ's bottom-left origin; faces are `f a/ta b/tb c/tc`
    (`a/ta/a` with normals [V, 3]), 1-based.  texture_png: the texture itself, uint8 [th, tw, 3], written to <stem>.png -- or the path of a
    PNG that exists already; the .mtl's map_Kd names it by its base name.  -> the PNG's path."""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    uvs = np.asarray(uvs, dtype=np.float64)
    if uvs.shape != (len(faces), 3, 2):
        raise ValueError('write_obj: uvs must be [T, 3, 2], one per face corner')
    if normals is not None:
        normals = np.asarray(normals, dtype=np.float64)
        if normals.shape != verts.shape:
            raise ValueError('write_obj: normals must be [V, 3]')
    stem = os.path.splitext(path)[0]
    if isinstance(texture_png, (str, os.PathLike)):
        png = os.fspath(texture_png)
    else:
        png = stem + '.png'
        write_png(png, texture_png)
    name = os.path.basename(stem)
    with open(stem + '.mtl', 'w') as f:
        f.write(f'newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd {os.path.basename(png)}\n')
    vt = uvs.reshape(-1, 2).copy()
    vt[:, 1] = 1.0 - vt[:, 1]
    ta = np.arange(1, 3 * len(faces) + 1, dtype=np.int64).reshape(-1, 3)
    with open(path, 'w') as f:
        f.write(f'mtllib {name}.mtl\nusemtl {name}\n')
        np.savetxt(f, verts, fmt='v %.9g %.9g %.9g')
        if normals is not None:
            np.savetxt(f, normals, fmt='vn %.9g %.9g %.9g')
        np.savetxt(f, vt, fmt='vt %.9g %.9g')
        if normals is not None:
            np.savetxt(f, np.stack([faces + 1, ta, faces + 1], axis=2).reshape(-1, 9), fmt='f %d/%d/%d %d/%d/%d %d/%d/%d')
        else:
            np.savetxt(f, np.stack([faces + 1, ta], axis=2).reshape(-1, 6), fmt='f %d/%d %d/%d %d/%d')
    return png


# ---------------------------------------------------------------------------------------------------------------- PLY
def write_ply(path, verts, faces, normals=None, colors=None):
    """Binary little-endian PLY with the layout plyfile writes for shape_utils.py's two elements (vertex x/y/z float, face
    `list uchar int vertex_indices`).  normals float [V, 3] and / or colors uint8 [V, 3] add `property float nx/ny/nz` and
    `property uchar red/green/blue` to the vertex element, behind x y z, in that order: one packed record per vertex.  Without them the
    file is the geometry-only one, byte for byte."""
    verts = np.ascontiguousarray(verts, dtype='<f4').reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype='<i4').reshape(-1, 3)
    fields, props = [('xyz', '<f4', (3,))], 'property float x\nproperty float y\nproperty float z\n'
    if normals is not None:
        fields.append(('n', '<f4', (3,)))
        props += 'property float nx\nproperty float ny\nproperty float nz\n'
    if colors is not None:
        fields.append(('rgb', 'u1', (3,)))
        props += 'property uchar red\nproperty uchar green\nproperty uchar blue\n'
    vertex = np.zeros(len(verts), dtype=fields)                           # (a packed dtype: no padding between the fields)
    vertex['xyz'] = verts
    for name, arr, dtype in (('n', normals, '<f4'), ('rgb', colors, 'u1')):
        if arr is not None:
            arr = np.asarray(arr)
            if arr.shape != (len(verts), 3) or (name == 'rgb' and arr.dtype != np.uint8):
                raise ValueError('write_ply: normals must be float [V, 3] and colors uint8 [V, 3]')
            vertex[name] = arr.astype(dtype, copy=False)
    header = ('ply\nformat binary_little_endian 1.0\n'
              f'element vertex {len(verts)}\n{props}'
              f'element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n')
    body = np.zeros(len(faces), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    body['n'] = 3
    body['i'] = faces
    with open(path, 'wb') as f:
        f.write(header.encode('ascii'))
        f.write(vertex.tobytes())
        f.write(body.tobytes())


_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': '<i2', 'int16': '<i2', 'ushort': '<u2', 'uint16': '<u2',
              'int': '<i4', 'int32': '<i4', 'uint': '<u4', 'uint32': '<u4', 'float': '<f4', 'float32': '<f4', 'double': '<f8', 'float64': '<f8'}


def _read_ply_elements(path):
    """(vertex records as a structured array with one field per property, faces int32 [T, 3]) of a binary little-endian PLY whose
    elements are `vertex` (scalar properties only) then `face` (`list uchar int vertex_indices`, triangles): the property list of the
    header is parsed, so any set of per-vertex attributes reads."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    lines = data[:end].decode('ascii').split('\n')
    if lines[0] != 'ply' or lines[1] != 'format binary_little_endian 1.0':
        raise ValueError(f'{path}: not a binary little-endian PLY')
    elements = []                                                        # [name, count, [property token lists]]
    for line in lines[2:]:
        tok = line.split()
        if tok[:1] == ['element']:
            elements.append([tok[1], int(tok[2]), []])
        elif tok[:1] == ['property']:
            if not elements:
                raise ValueError(f'{path}: a property before any element')
            elements[-1][2].append(tok[1:])
    if [e[0] for e in elements] != ['vertex', 'face']:
        raise ValueError(f'{path}: expected the elements vertex and face')
    (_, nv, vprops), (_, nf, fprops) = elements
    if any(len(t) != 2 or t[0] not in _PLY_TYPES for t in vprops) or len({t[1] for t in vprops}) != len(vprops):
        raise ValueError(f'{path}: vertex properties must be distinct scalars')
    if fprops != [['list', 'uchar', 'int', 'vertex_indices']]:
        raise ValueError(f'{path}: the face element must be `property list uchar int vertex_indices`')
    vdtype = np.dtype([(name, _PLY_TYPES[t]) for t, name in vprops])
    vertex = np.frombuffer(data, dtype=vdtype, count=nv, offset=end)
    body = np.frombuffer(data, dtype=[('n', 'u1'), ('i', '<i4', (3,))], count=nf, offset=end + nv * vdtype.itemsize)
    if nf and not np.all(body['n'] == 3):
        raise ValueError(f'{path}: a face is not a triangle')
    return vertex, body['i'].astype(np.int32)


def _ply_columns(vertex, names, dtype, path):
    if any(n not in vertex.dtype.names for n in names):
        if any(n in vertex.dtype.names for n in names):
            raise ValueError(f'{path}: incomplete vertex attribute {"/".join(names)}')
        return None
    return np.stack([vertex[n] for n in names], axis=1).astype(dtype)


def read_ply(path):
    """The inverse of write_ply for the geometry, with or without per-vertex attributes: (verts float32 [V, 3], faces int32 [T, 3])."""
    vertex, faces = _read_ply_elements(path)
    verts = _ply_columns(vertex, ('x', 'y', 'z'), np.float32, path)
    if verts is None:
        raise ValueError(f'{path}: the vertex element has no x y z')
    return verts, faces


def read_ply_attrs(path):
    """The optional per-vertex arrays of a .ply write_ply made: {'normals': float32 [V, 3], 'colors': uint8 [V, 3]}, each key present
    only when the file holds it."""
    vertex, _ = _read_ply_elements(path)
    found = {'normals': _ply_columns(vertex, ('nx', 'ny', 'nz'), np.float32, path), 'colors': _ply_columns(vertex, ('red', 'green', 'blue'), np.uint8, path)}
    return {k: v for k, v in found.items() if v is not None}


def convert_sdf_samples_to_ply(volume, voxel_grid_origin, voxel_size, ply_filename_out, offset=None, scale=None, level=0.0, clean=None, simplify=None):
    """shape_utils.py:40-100: mesh `volume` at `level` with spacing voxel_size, move the vertices by voxel_grid_origin, then
    / scale and - offset when given, and write the .ply.  `volume` may be a CUDA tensor (the kernel) or a CPU array (the numpy port).
    clean, simplify: None, or clean_options' / simplify_options' dict (the cell in the mesh's units) -- finish_mesh's stages, run where the mesh
    was extracted, before it is moved.  Returns (vertex count, face count), with finish_mesh's record (the reports) as its attribute `mesh`."""
    mesh = finish_mesh(*marching_cubes(volume, level, spacing=voxel_size), clean=clean, simplify=simplify)
    verts, faces = to_host(mesh.verts), to_host(mesh.faces)
    mesh_points = np.zeros_like(verts)
    mesh_points[:, 0] = voxel_grid_origin[0] + verts[:, 0]
    mesh_points[:, 1] = voxel_grid_origin[1] + verts[:, 1]
    mesh_points[:, 2] = voxel_grid_origin[2] + verts[:, 2]
    if scale is not None:
        mesh_points = mesh_points / scale
    if offset is not None:
        mesh_points = mesh_points - offset
    write_ply(ply_filename_out, mesh_points, faces)
    return Written((len(verts), len(faces)), mesh)


# ---------------------------------------------------------------------------------------------------------------- MRC
_MRC_HEADER = 1024


def write_mrc(path, volume):
    """MRC2014, mode 2 (float32), little-endian, no extended header -- what gen_videos.py:221-222 writes through mrcfile:
    nx, ny, nz = the array's shape reversed (axis 2 fastest), 'MAP ' at byte 208."""
    data = np.ascontiguousarray(np.asarray(volume), dtype='<f4')
    if data.ndim != 3:
        raise ValueError('write_mrc: volume must be 3-D')
    nz, ny, nx = data.shape
    h = bytearray(_MRC_HEADER)
    struct.pack_into('<10i', h, 0, nx, ny, nz, 2, 0, 0, 0, nx, ny, nz)
    struct.pack_into('<6f', h, 40, 0.0, 0.0, 0.0, 90.0, 90.0, 90.0)             # cell lengths (voxel size 0: unset), angles
    struct.pack_into('<3i', h, 64, 1, 2, 3)                                     # mapc, mapr, maps
    finite = data[np.isfinite(data)]
    dmin, dmax, dmean = (float(finite.min()), float(finite.max()), float(finite.mean(dtype=np.float64))) if finite.size else (0.0, 0.0, 0.0)
    rms = float(finite.std(dtype=np.float64)) if finite.size else 0.0
    struct.pack_into('<3f', h, 76, dmin, dmax, dmean)
    struct.pack_into('<2i', h, 88, 1, 0)                                        # ispg 1 (a volume), nsymbt 0
    struct.pack_into('<i', h, 108, 20140)                                       # nversion
    h[208:212] = b'MAP '
    h[212:216] = bytes([0x44, 0x44, 0, 0])                                      # machine stamp: little-endian
    struct.pack_into('<f', h, 216, rms)
    with open(path, 'wb') as f:
        f.write(bytes(h))
        f.write(data.tobytes())


def read_mrc(path):
    """A mode-2 MRC volume as float32 [nz, ny, nx] (the layout mrcfile's `.data` has); skips the extended header (nsymbt bytes)."""
    with open(path, 'rb') as f:
        head = f.read(_MRC_HEADER)
        if len(head) < _MRC_HEADER or head[208:212] != b'MAP ':
            raise ValueError(f'{path}: not an MRC file')
        big = head[212] == 0x11
        e = '>' if big else '<'
        nx, ny, nz, mode = struct.unpack_from(e + '4i', head, 0)
        nsymbt = struct.unpack_from(e + 'i', head, 92)[0]
        if mode != 2:
            raise ValueError(f'{path}: MRC mode {mode}; only mode 2 (float32) is read')
        f.seek(_MRC_HEADER + nsymbt)
        data = np.frombuffer(f.read(nx * ny * nz * 4), dtype=e + 'f4')
    if data.size != nx * ny * nz:
        raise ValueError(f'{path}: truncated data')
    return data.reshape(nz, ny, nx).astype(np.float32)


def mrc_header(path):
    """The MRC header fields this module writes, as a dict (tests, diagnostics)."""
    with open(path, 'rb') as f:
        h = f.read(_MRC_HEADER)
    nx, ny, nz, mode, sx, sy, sz, mx, my, mz = struct.unpack_from('<10i', h, 0)
    return dict(nx=nx, ny=ny, nz=nz, mode=mode, start=(sx, sy, sz), m=(mx, my, mz), cella=struct.unpack_from('<3f', h, 40),
                cellb=struct.unpack_from('<3f', h, 52), map_crs=struct.unpack_from('<3i', h, 64), dmin_dmax_dmean=struct.unpack_from('<3f', h, 76),
                ispg=struct.unpack_from('<i', h, 88)[0], nsymbt=struct.unpack_from('<i', h, 92)[0], map=bytes(h[208:212]), machst=bytes(h[212:216]))


# ---------------------------------------------------------------------------------------------------------------- files and CLI
def load_volume(path):
    return read_mrc(path) if path.lower().endswith('.mrc') else np.load(path).astype(np.float32, copy=False)


def convert_mrc(input_filename, output_filename, level=10.0, device=None, clean=None, simplify=None):
    """shape_utils.py:103-105: mesh transpose(2, 1, 0) of the file's data (.mrc or .npy), voxel size 1, origin 0.  `device`: a torch
    device to run the kernel on (None: the numpy port).  clean, simplify and the return: as convert_sdf_samples_to_ply's."""
    vol = np.ascontiguousarray(np.transpose(load_volume(input_filename), (2, 1, 0)))
    if device is not None:
        vol = _torch().from_numpy(vol).to(device)
    return convert_sdf_samples_to_ply(vol, [0, 0, 0], 1, output_filename, level=level, clean=clean, simplify=simplify)


def arg_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter,
                                 epilog='Snapping the vertices onto the density\'s level set (--mesh-snap of gen_videos_mi355x.py) needs the generator the '
                                        'volume came from: this tool works from the volume alone and has no such flag.')
    ap.add_argument('input', help='a .mrc / .npy volume, or a directory of them (each gets a .ply next to it)')
    ap.add_argument('--level', type=float, default=10, help='the isosurface level (shape_utils.py:111)')
    ap.add_argument('--device', default=None, help="'cuda' runs the gfx950 kernel (default: cuda when available, else the numpy port)")
    add_mesh_arguments(ap)
    return ap


def main(argv=None):
    ap = arg_parser()
    args = ap.parse_args(argv)
    clean, simplify, _ = mesh_options_from_args(args, ap)
    device = args.device
    if device is None:
        device = 'cuda' if _torch() is not None and _torch().cuda.is_available() else None
    if device == 'cpu':
        device = None
    if os.path.isfile(args.input):
        paths = [args.input]
    elif os.path.isdir(args.input):
        paths = sorted(glob.glob(os.path.join(args.input, '*.mrc')) + glob.glob(os.path.join(args.input, '*.npy')))
    else:
        ap.error(f'{args.input}: no such file or directory')
    for path in paths:                                                   # --level is honoured for a single file too (the reference's
        t0 = time.perf_counter()                                         # single-file branch ignores it, shape_utils.py:114-116)
        out = os.path.splitext(path)[0] + '.ply'
        nv, nf = written = convert_mrc(path, out, level=args.level, device=device, clean=clean, simplify=simplify)
        for line in report_lines(written.mesh.reports, smooth=args.mesh_smooth):
            print(line)
        print(f'wrote {out}: {nv} vertices, {nf} triangles ({time.perf_counter() - t0:.3f} s)')
    return 0


if __name__ == '__main__':
    sys.exit(main())
