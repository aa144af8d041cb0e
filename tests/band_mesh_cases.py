"""What the CPU and GPU tests of the brick-wise band mesh share (tests/test_band_mesh_cpu.py, tests/test_band_mesh_gpu.py): the cases -- the
fields of tests/mesh_band_cases.py with their crops, plus a ball that the lattice boundary cuts --, the three views, and per case the band run
of the port: the unfilled volume, the final states, and the mesh of the existing route (band_volume_numpy's filled volume, cropped, flipped,
permuted, through marching_cubes_numpy).  Everything is made once and never changed."""

import functools

import numpy as np

import shape_mi355x as S
from mesh_band_cases import NOISE_KEEP, SPHERE_KEEP, cropped, field

BRICKS = (2, 4, 8, 16)
VIEWS = {'identity': ((0, 1, 2), (False, False, False)),
         'pipeline': ((2, 1, 0), (True, False, False)),                  # extract_density_grid's flip(0) + mesh_of_density_grid's permute(2, 1, 0)
         'rotated': ((1, 2, 0), (False, True, True))}
CUT_KEEP = [(0, 18), (0, 17), (1, 18)]                       # (keeps the coarse point (16, 0, 16), inside the ball: the one seed at s = 16)
FIELDS = {'rough_sphere': SPHERE_KEEP, 'four_balls': None, 'noise': NOISE_KEEP, 'integer': None, 'cut_ball': CUT_KEEP}


@functools.lru_cache(maxsize=None)
def case_field(name):
    """name -> (dense float32 [n, n, n], level).  cut_ball: n = 18, so 17 % s = 1 gives a last brick one cell thick for every s; the ball
    reaches past the lattice on three sides."""
    if name != 'cut_ball':
        return field(name)
    i = np.arange(18, dtype=np.float64)
    x, y, z = np.meshgrid(i, i, i, indexing='ij')
    vol = (9.4 - np.sqrt((x - 13.3) ** 2 + (y - 3.6) ** 2 + (z - 12.2) ** 2) + 0.3 * np.sin(1.7 * x + 0.9 * y) * np.cos(1.3 * z)).astype(np.float32)
    vol.setflags(write=False)
    return vol, 0.0


def viewed(vol, perm, flip):
    axes = [a for a in range(3) if flip[a]]
    return np.ascontiguousarray(np.transpose(np.flip(vol, axes) if axes else vol, perm))


@functools.lru_cache(maxsize=None)
def band_run(name, s, with_keep=True):
    """The port's band run of a case -> dict(n, level, keep, dense, raw: the volume float32 [n^3] WITHOUT the fill (zeros where nothing was
    evaluated), state uint8 [nb^3], report, filled: band_volume_numpy's volume after the crop, visited: bool [n, n, n])."""
    dense, level = case_field(name)
    n = dense.shape[0]
    keep = FIELDS[name] if with_keep else None
    flat = dense.reshape(-1)

    def host_field(index, out):
        out[index] = flat[index]

    filled, report = S.band_volume_numpy(host_field, n, level, s, keep)
    raw = np.zeros(n ** 3, dtype=np.float32)
    _, s_, nb, keep_ = S._band_geometry(n, s, keep)
    band = S._BandNumpy(raw, n, s, level, keep_)
    raw_report = S._band_driver(n, s, lambda index: host_field(index, raw) if len(index) else None, S.band_coarse_index(n, s), band, None, fill=False)
    assert raw_report == report
    state = band.state if band.state is not None else np.zeros(nb ** 3, dtype=np.uint8)
    out = dict(n=n, level=level, keep=keep, dense=dense, raw=raw, state=state, report=report, filled=cropped(filled, keep),
               visited=S.band_visited_numpy(state, n, s))
    for x in (raw, state, out['filled'], out['visited']):
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def existing_mesh(name, s, view, with_keep=True):
    """The existing route's mesh of a case in a view: marching_cubes_numpy of the filled, cropped, flipped and permuted volume."""
    run = band_run(name, s, with_keep)
    verts, faces = S.marching_cubes_numpy(viewed(run['filled'], *VIEWS[view]), run['level'])
    verts.setflags(write=False)
    faces.setflags(write=False)
    return verts, faces


def poisoned(run, value):
    """The unfilled volume with every unvisited point overwritten by `value` (a copy)."""
    vol = np.array(run['raw']).reshape(run['visited'].shape)
    vol[~run['visited']] = value
    return vol.reshape(-1)
