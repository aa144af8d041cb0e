"""What the CPU and GPU tests of the narrow-band density volume share (tests/test_mesh_band_cpu.py, tests/test_mesh_band_gpu.py): the fields, a
counting `field` callable, the crop a kept range stands for, and the comparison of a band mesh with the dense mesh restricted to whole
components.  The fields are made once and never changed."""

import functools

import numpy as np
import scipy.ndimage

import shape_mi355x as S
from test_mesh_clean_cpu import four_balls_field, rough_sphere_field

SPHERE_KEEP = [(6, 42), (5, 40), (7, 43)]                     # a crop of the 48^3 fixtures that cuts the rough sphere (radius 18 about 23.5)
NOISE_KEEP = [(5, 39), (4, 36), (6, 40)]


@functools.lru_cache(maxsize=None)
def field(name):
    """name -> (dense float32 [n, n, n], level).  Read-only."""
    if name == 'rough_sphere':
        vol, level = rough_sphere_field(), 0.0
    elif name == 'four_balls':
        vol, level = four_balls_field(), 0.0
    elif name == 'noise':                                     # 43 points: 42 cells, a partial last brick at s = 4
        vol, level = scipy.ndimage.gaussian_filter(np.random.default_rng(11).standard_normal((43, 43, 43)), 2.0).astype(np.float32), 0.0
    elif name == 'integer':                                   # plateaus of integers around a ball: many points hold exactly the level
        i = np.arange(30, dtype=np.float64)
        x, y, z = np.meshgrid(i, i, i, indexing='ij')
        vol, level = np.floor(9.3 - np.sqrt((x - 14.2) ** 2 + (y - 15.1) ** 2 + (z - 13.7) ** 2)).astype(np.float32), 2.0
    else:
        raise KeyError(name)
    vol.setflags(write=False)
    return vol, level


class CountingField:
    """field(index, out) of band_volume over a dense volume, counting how often every index is asked for."""

    def __init__(self, dense):
        self.flat = np.ascontiguousarray(dense).reshape(-1)
        self.calls = np.zeros(self.flat.size, dtype=np.int64)

    def __call__(self, index, out):
        index = np.asarray(index)
        assert index.dtype == np.int32 and index.ndim == 1
        np.add.at(self.calls, index, 1)
        out[index] = self.flat[index]


def cropped(vol, keep):
    """vol with everything outside the kept ranges zeroed (a copy): the crop the band was told of."""
    if keep is None:
        return np.array(vol)
    out = np.zeros_like(vol)
    sl = tuple(slice(lo, hi) for lo, hi in keep)
    out[sl] = vol[sl]
    return out


def restricted_dense(dense_mesh, band_mesh):
    """The dense mesh restricted to the components that have a vertex in the band mesh -> (verts, faces, lost: [(vertices, faces)] of the
    components that are absent, partly: the number of components of which the band mesh holds some vertices but not all)."""
    dv, df = dense_mesh
    bv, _ = band_mesh
    label, faces_of, _ = S.mesh_components_numpy(df, len(dv))
    rows = {r.tobytes() for r in bv}
    present = np.fromiter((r.tobytes() in rows for r in dv), dtype=bool, count=len(dv))
    labels = np.unique(label)
    size = np.bincount(label, minlength=len(dv))
    some = np.bincount(label, weights=present, minlength=len(dv)).astype(np.int64)
    partly = int(((some[labels] > 0) & (some[labels] < size[labels])).sum())
    keep = (some > 0).astype(np.uint8)                                           # indexed by label
    verts, faces, _ = S.mesh_compact_numpy(dv, df, label, faces_of, keep)
    lost = [(int(size[c]), int(faces_of[c])) for c in labels if some[c] == 0]
    return verts, faces, lost, partly


def same_mesh(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))
