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

CLI, as shape_utils.py's (:102-123):  python shape_mi355x.py INPUT [--level 10]   (INPUT: a .mrc / .npy file or a directory of them)
"""

import argparse
import glob
import os
import struct
import sys
import time

import numpy as np

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
    lev = np.float32(level)
    d0, d1, d2 = v.shape
    strides = np.array([d1 * d2, d2, 1], dtype=np.int64)
    inside = v > lev
    cross = np.zeros(v.shape + (3,), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
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
    for c in range(8):
        o0, o1, o2 = CORNER_OFFSETS[c]
        case |= inside[o0:d0 - 1 + o0, o1:d1 - 1 + o1, o2:d2 - 1 + o2].astype(np.int64) << c
    case = case.reshape(-1)
    ntri = count[case]
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
    try:
        import torch
    except ImportError:                                                  # pragma: no cover - torch is part of the stack
        torch = None
    if torch is not None and isinstance(volume, torch.Tensor):
        if volume.is_cuda:
            import gnerf_hip
            verts, faces = gnerf_hip.marching_cubes(volume, level)
            if not identity:
                verts = verts * torch.from_numpy(s.copy()).to(verts.device) + torch.from_numpy(o.copy()).to(verts.device)
            return verts, faces
        volume = volume.detach().numpy()
    verts, faces = marching_cubes_numpy(volume, level)
    if not identity:
        verts = verts * s + o
    return verts, faces


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


def convert_sdf_samples_to_ply(volume, voxel_grid_origin, voxel_size, ply_filename_out, offset=None, scale=None, level=0.0):
    """shape_utils.py:40-100: mesh `volume` at `level` with spacing voxel_size, move the vertices by voxel_grid_origin, then
    / scale and - offset when given, and write the .ply.  `volume` may be a CUDA tensor (the kernel) or a CPU array (the numpy port).
    Returns (vertex count, face count)."""
    verts, faces = marching_cubes(volume, level, spacing=voxel_size)
    if not isinstance(verts, np.ndarray):
        verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
    mesh_points = np.zeros_like(verts)
    mesh_points[:, 0] = voxel_grid_origin[0] + verts[:, 0]
    mesh_points[:, 1] = voxel_grid_origin[1] + verts[:, 1]
    mesh_points[:, 2] = voxel_grid_origin[2] + verts[:, 2]
    if scale is not None:
        mesh_points = mesh_points / scale
    if offset is not None:
        mesh_points = mesh_points - offset
    write_ply(ply_filename_out, mesh_points, faces)
    return len(verts), len(faces)


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


def convert_mrc(input_filename, output_filename, level=10.0, device=None):
    """shape_utils.py:103-105: mesh transpose(2, 1, 0) of the file's data (.mrc or .npy), voxel size 1, origin 0.  `device`: a torch
    device to run the kernel on (None: the numpy port).  Returns (vertex count, face count)."""
    vol = np.ascontiguousarray(np.transpose(load_volume(input_filename), (2, 1, 0)))
    if device is not None:
        import torch
        vol = torch.from_numpy(vol).to(device)
    return convert_sdf_samples_to_ply(vol, [0, 0, 0], 1, output_filename, level=level)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('input', help='a .mrc / .npy volume, or a directory of them (each gets a .ply next to it)')
    ap.add_argument('--level', type=float, default=10, help='the isosurface level (shape_utils.py:111)')
    ap.add_argument('--device', default=None, help="'cuda' runs the gfx950 kernel (default: cuda when available, else the numpy port)")
    args = ap.parse_args(argv)
    device = args.device
    if device is None:
        try:
            import torch
            device = 'cuda' if torch.cuda.is_available() else None
        except ImportError:                                              # pragma: no cover
            device = None
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
        nv, nf = convert_mrc(path, out, level=args.level, device=device)
        print(f'wrote {out}: {nv} vertices, {nf} triangles ({time.perf_counter() - t0:.3f} s)')
    return 0


if __name__ == '__main__':
    sys.exit(main())
