"""CPU tests of the multi-view colour bake's numpy port (shape_mi355x.bake_colors_numpy / bake_mesh_colors, the reference the kernel of
csrc/raster.hip matches bit for bit) and of the host logic around it: constant and ramp frames, occlusion between two squares, a sphere
(the depth test alone, then the facing test), independence of the vertices' order, the argument checks and declarations, and a round trip
through render_mesh."""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import shape_mi355x as S
from test_raster_cpu import PIXEL_CAMERA, SPHERE_R, SPHERE_SCALE, at_pixels, orbit_cameras, sphere_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------- scenes
def bake_soup(n_tri, seed=None):
    """test_raster_gpu's soup of random triangles, with larger triangles (enough covered pixels for whole windows of them) and the random
    normals turned towards the orbit's cameras (which stand at +z), so that the facing test passes some vertices and rejects others."""
    from test_raster_gpu import soup
    verts, faces, normals, colors = soup(n_tri, seed=n_tri if seed is None else seed, smallest=0.02, largest=0.6)
    normals[:, 2] = np.abs(normals[:, 2])
    return verts, faces, normals, colors


def orbit_views(n_views, mesh2world=None):
    """(mesh2cam [n, 12], intrinsics [n, 9], normal_mat [n, 9]) of the first n of the orbit cameras test_raster_cpu uses."""
    cam2world, K = orbit_cameras((0, 40, 80)[:n_views])
    A, N = S.mesh_to_camera(cam2world.numpy(), mesh2world)
    return A.reshape(-1, 12), K.numpy().reshape(-1, 9), N.reshape(-1, 9)


SQUARES_SIZE = 32
FRONT, BACK = (12, 20), (2, 30)                      # the squares' extents in pixels of the front camera, at z = 1 and z = 2


def two_squares():
    """Two parallel squares seen by PIXEL_CAMERA at 32 x 32: a small one in front (z = 1, pixels 12 .. 20, a 4 x 4 grid of quads) and a large
    one behind (z = 2, pixels 2 .. 30, a 28 x 28 grid of quads whose inner vertices sit on pixel centres k + 0.5), and a second camera that
    looks back from z = 4 (a half turn about y), for which the large square is the near one at z' = 2 and the small one hides behind it at
    z' = 3.  -> (verts, faces, is_back [V], pixel position of every vertex in the front camera [V, 2], mesh2cam [2, 12], intrinsics [2, 9])."""
    def grid(lo, hi, step):
        xs = np.arange(lo, hi + step / 2, step)
        px, py = np.meshgrid(xs, xs)
        pos = np.stack([px.ravel(), py.ravel()], axis=1)
        n = len(xs)
        i = np.arange(n * n).reshape(n, n)
        a, b, c, d = i[:-1, :-1].ravel(), i[:-1, 1:].ravel(), i[1:, 1:].ravel(), i[1:, :-1].ravel()
        return pos, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    front_pos, front_f = grid(FRONT[0], FRONT[1], 2)
    back_pos, back_f = grid(BACK[0] + 0.5, BACK[1] - 0.5, 1)              # vertices on the centres 2.5 .. 29.5
    verts = np.concatenate([at_pixels(front_pos, SQUARES_SIZE, 1.0), at_pixels(back_pos, SQUARES_SIZE, 2.0)])
    faces = np.concatenate([front_f, back_f + len(front_pos)]).astype(np.int32)
    is_back = np.arange(len(verts)) >= len(front_pos)
    behind = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 4]], dtype=np.float32).reshape(1, 12)
    A = np.concatenate([PIXEL_CAMERA[0], behind])
    K = np.concatenate([PIXEL_CAMERA[1], PIXEL_CAMERA[1]])
    return verts, faces, is_back, np.concatenate([front_pos, back_pos]), A, K


def wall_with_probes(size, n_probes=400, seed=0):
    """A wall at z = 1 that overflows PIXEL_CAMERA's image (two triangles), and probe vertices on it that belong to no face: random positions
    all over the image, the first 40 within half a frame pixel of its border.  -> (verts, faces, pixel positions [V, 2] in units of the
    image's width and height, i.e. (xc, yc))."""
    rng = np.random.default_rng(seed)
    wall = np.array([[-0.5, -0.5], [1.5, -0.5], [1.5, 1.5], [-0.5, 1.5]])
    probes = rng.random((n_probes, 2)) * 0.998 + 0.001
    edge = rng.random(40) * 0.012                    # half a pixel of a 40-wide frame is 0.0125
    probes[0:10, 0], probes[10:20, 0], probes[20:30, 1], probes[30:40, 1] = edge[:10], 1 - 1 / 1024 - edge[10:20], edge[20:30], 1 - 1 / 1024 - edge[30:]
    pos = np.concatenate([wall, probes])
    verts = np.stack([pos[:, 0] - 0.5, pos[:, 1] - 0.5, np.ones(len(pos))], axis=1).astype(np.float32)
    return verts, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), pos


@pytest.fixture(scope='module')
def sphere():
    """The sphere of test_raster_cpu (radius 0.25 around the world's origin) from the three orbit cameras at 96 x 96: visibility made once."""
    verts, faces, normals, mesh2world = sphere_mesh()
    A, K, N = orbit_views(3, mesh2world)
    vis, counts = S.rasterize_numpy(verts, faces, A, K, 96)
    assert counts[0] == counts.sum()
    cam2world, K33 = orbit_cameras()
    return dict(verts=verts, faces=faces, normals=normals, mesh2world=mesh2world, A=A, K=K, N=N, vis=vis, cam2world=cam2world.numpy(), K33=K33.numpy())


# The default depth_tol, 2^-8, is sized for 512 rows (include/gnerf_hip.h: twice the relative depth step across one pixel on a 75 degree slope).
# The sphere is drawn at 96 rows, where a pixel is 512 / 96 times as large: the same rule gives this tolerance.
SPHERE_TOL = 2.0 ** -8 * 512 / 96


def constant_frames(colors, fh, fw):
    return np.broadcast_to(np.asarray(colors, dtype=np.uint8)[:, None, None, :], (len(colors), fh, fw, 3)).copy()


# The soups the kernel is compared on (tests/test_mesh_bake_gpu.py): the cases live here so that their coverage is checked without a GPU.
VIS_SIZE, FRAME_SIZE = (37, 53), (40, 29)
SOUPS = (1, 63, 64, 65, 257, 2000)                   # V = 3, 189, 192, 195, 771, 6000: around one wave, one workgroup (256), and many


def random_frames(n_views, size, seed):
    return np.random.default_rng(seed).integers(0, 256, (n_views, *size, 3), dtype=np.uint8)


def soup_cases(n_tri):
    """Every configuration of one soup: (n_views, with normals, guard) with the port's visibility buffer and random frames."""
    verts, faces, normals, fallback = bake_soup(n_tri)
    for n_views in (1, 3):
        A, K, N = orbit_views(n_views)
        vis, _ = S.rasterize_numpy(verts, faces, A, K, VIS_SIZE)
        frames = random_frames(n_views, FRAME_SIZE, seed=n_tri + n_views)
        for with_normals in (False, True):
            for guard in (0, 1):
                yield dict(verts=verts, mesh2cam=A, intrinsics=K, vis=vis, frames=frames, normals=normals if with_normals else None,
                           normal_mat=N if with_normals else None, fallback=fallback, guard=guard)


@pytest.mark.parametrize('n_tri', [n for n in SOUPS if n >= 257])
def test_the_soups_have_seen_and_unseen_vertices(n_tri):
    """The kernel's comparison with the port cannot pass on empty output: every configuration has vertices of both kinds."""
    for case in soup_cases(n_tri):
        seen = S.bake_colors_numpy(**case)['seen'] > 0
        assert seen.sum() >= 50 and (~seen).sum() >= 50, (n_tri, len(case['mesh2cam']), case['normals'] is not None, case['guard'], int(seen.sum()))


# ---------------------------------------------------------------------------------------------------------------- constant frames
@pytest.mark.parametrize('with_normals', [False, True], ids=['plain', 'normals'])
def test_constant_frames_give_their_colour_and_unseen_vertices_their_fallback(with_normals):
    verts, faces, normals, fallback = bake_soup(500)
    A, K, N = orbit_views(3)
    vis, _ = S.rasterize_numpy(verts, faces, A, K, (37, 53))
    colour = (201, 17, 96)
    frames = constant_frames([colour] * 3, 40, 29)
    kw = dict(normals=normals, normal_mat=N) if with_normals else {}
    for fb in (fallback, None):
        for guard in (0, 1):
            out = S.bake_colors_numpy(verts, A, K, vis, frames, guard=guard, fallback=fb, **kw)
            seen = out['seen'] > 0
            assert out['colors'].dtype == np.uint8 and out['weight'].dtype == np.float32 and out['seen'].dtype == np.int32
            assert seen.sum() >= 50 and (~seen).sum() >= 50
            assert np.all(out['colors'][seen] == np.array(colour, dtype=np.uint8))
            assert np.all(out['colors'][~seen] == (fb[~seen] if fb is not None else 0))
            assert np.array_equal(out['weight'] > 0, seen) and np.all(out['weight'][~seen] == 0) and out['seen'].max() <= 3
            if not with_normals:
                assert np.array_equal(out['weight'], out['seen'].astype(np.float32))          # every view counts 1


# ---------------------------------------------------------------------------------------------------------------- two squares
def test_two_parallel_squares_hide_each_other():
    verts, faces, is_back, pos, A, K = two_squares()
    vis, counts = S.rasterize_numpy(verts, faces, A, K, SQUARES_SIZE)
    assert counts[0] == counts.sum()
    red, blue = (250, 10, 20), (5, 60, 240)
    frames = constant_frames([red, blue], 32, 32)
    for guard in (0, 1, 2):
        per_view = [S.bake_colors_numpy(verts, A[k:k + 1], K[k:k + 1], vis[k:k + 1], frames[k:k + 1], guard=guard)['seen'] > 0 for k in (0, 1)]
        col, row = np.floor(pos[:, 0]), np.floor(pos[:, 1])
        # the front square covers the pixel centres 12.5 .. 19.5 of the front camera: pixels 12 .. 19 in both directions
        under = is_back & (col >= FRONT[0]) & (col <= FRONT[1] - 1) & (row >= FRONT[0]) & (row <= FRONT[1] - 1)
        clear = np.maximum(np.maximum(FRONT[0] - col, col - (FRONT[1] - 1)), np.maximum(FRONT[0] - row, row - (FRONT[1] - 1)))      # in pixels; <= 0 under it
        # (a window must also lie on the back square itself, since an empty neighbour rejects.  Its outline runs through the centres 2.5 and
        # 29.5, and the fill rule gives it the top and left ones only: it covers the pixels 2 .. 28)
        inner = is_back & (np.minimum(np.minimum(col, row) - BACK[0], BACK[1] - 2 - np.maximum(col, row)) >= guard)
        far = inner & (clear > guard + 1)
        assert under.sum() == 64 and far.sum() > 100
        assert not per_view[0][under].any(), 'a back vertex under the front square is seen from the front'
        assert per_view[0][far].all(), 'a back vertex clear of the front square is hidden from the front'
        assert per_view[0][~is_back].all()                                               # the front square itself
        rim = is_back & ~inner
        assert rim.any() and not per_view[0][rim].any(), 'a window that reaches past the mesh is rejected on purpose'
        # from behind it is the other way round: the large square is in front of the small one (columns are mirrored there, 31 - col, so
        # in the front camera's columns that view covers 3 .. 29)
        inner_behind = is_back & (np.minimum(np.minimum(col - (BACK[0] + 1), row - BACK[0]), np.minimum(BACK[1] - 1 - col, BACK[1] - 2 - row)) >= guard)
        assert not per_view[1][~is_back].any() and per_view[1][inner_behind].all() and per_view[1][under].all()
        both = S.bake_colors_numpy(verts, A, K, vis, frames, guard=guard)
        assert np.array_equal(both['seen'], per_view[0].astype(np.int32) + per_view[1].astype(np.int32))
        only0, only1 = per_view[0] & ~per_view[1], per_view[1] & ~per_view[0]
        assert only0.sum() >= 25 and only1.sum() >= 64
        assert np.all(both['colors'][only0] == np.array(red, dtype=np.uint8)) and np.all(both['colors'][only1] == np.array(blue, dtype=np.uint8))
        two = per_view[0] & per_view[1]
        assert two.sum() > 100 and np.all(both['colors'][two] == np.array([128, 35, 130], dtype=np.uint8))    # equal weights: the mean, ties to even


# ---------------------------------------------------------------------------------------------------------------- sphere
def test_sphere_depth_test_alone_stops_at_the_silhouette(sphere):
    """Without normals only the visibility buffer hides the far side.  A vertex past the silhouette, whose outward normal makes the cosine
    -e with the direction to the camera, lies behind the near side by the chord of its line of sight, 2 R e to first order; it passes the
    depth test while 2 R e <= depth_tol z, i.e. e <= depth_tol z / (2 R).  The test is made against the (2 guard + 1)^2 pixel centres around
    the vertex and not on its own line of sight, which the factor 2 of the estimate depth_tol z / (2 R) * 2 allows for; the bound is twice
    that estimate, at the largest z of the scene: with z_max = 2.7 + R and R = 0.25 it is 0.092 for the default depth_tol = 2^-8 and 0.49
    for SPHERE_TOL = 0.0208.  The share of the vertices that is seen is asked of the single view 0 at SPHERE_TOL, the tolerance that fits
    this resolution (at 2^-8 a 96-row pixel's depth step hides slopes beyond 55 degrees; the cosine bound is checked there too)."""
    s = sphere
    radius = SPHERE_R * SPHERE_SCALE
    frames = constant_frames([(9, 99, 199)], 96, 96)
    for tol, view in [(SPHERE_TOL, 0), (SPHERE_TOL, 1), (SPHERE_TOL, 2), (2.0 ** -8, 0)]:
        out = S.bake_colors_numpy(s['verts'], s['A'][view:view + 1], s['K'][view:view + 1], s['vis'][view:view + 1], frames, depth_tol=tol)
        seen = out['seen'] > 0
        world = s['verts'].astype(np.float64) @ s['mesh2world'][:, :3].T + s['mesh2world'][:, 3]
        eye = s['cam2world'][view][:3, 3].astype(np.float64)
        to_eye = eye - world
        cos = (s['normals'].astype(np.float64) * to_eye).sum(1) / np.linalg.norm(to_eye, axis=1)
        z_max = float(np.linalg.norm(eye)) + radius
        bound = -2 * tol * z_max / radius
        print(f'view {view}: {seen.sum()} of {len(seen)} vertices seen, smallest cosine among them {cos[seen].min():.4f} (bound {bound:.4f})')
        assert seen.sum() > 1000 and np.all(cos[seen] >= bound)
        if (tol, view) == (SPHERE_TOL, 0):
            assert seen.sum() >= len(seen) / 3
        assert np.all(out['colors'][seen] == np.array([9, 99, 199], dtype=np.uint8)) and np.all(out['colors'][~seen] == 0)


def test_sphere_facing_test_keeps_what_faces_the_camera(sphere):
    s = sphere
    frames = constant_frames([(1, 2, 3)] * 3, 96, 96)
    world = s['verts'].astype(np.float64) @ s['mesh2world'][:, :3].T + s['mesh2world'][:, 3]
    for min_cos in (0.1, 0.5):
        total = np.zeros(len(world), dtype=np.int64)
        for view in range(3):
            out = S.bake_colors_numpy(s['verts'], s['A'][view:view + 1], s['K'][view:view + 1], s['vis'][view:view + 1], frames[:1],
                                      normals=s['normals'], normal_mat=s['N'][view:view + 1], min_cos=min_cos, depth_tol=SPHERE_TOL)
            seen = out['seen'] > 0
            to_eye = s['cam2world'][view][:3, 3].astype(np.float64) - world
            cos = (s['normals'].astype(np.float64) * to_eye).sum(1) / np.linalg.norm(to_eye, axis=1)
            assert seen.sum() > 500 and np.all(cos[seen] > min_cos - 1e-5)
            # power 2: the weight is the cosine's square
            assert np.allclose(out['weight'][seen], cos[seen] ** 2, rtol=1e-4, atol=1e-6)
            total += seen
        out = S.bake_colors_numpy(s['verts'], s['A'], s['K'], s['vis'], frames, normals=s['normals'], normal_mat=s['N'], min_cos=min_cos, depth_tol=SPHERE_TOL)
        assert np.array_equal(out['seen'], total.astype(np.int32))
    for power, expo in ((0, 0), (1, 1), (3, 3)):
        out = S.bake_colors_numpy(s['verts'], s['A'][:1], s['K'][:1], s['vis'][:1], frames[:1], normals=s['normals'], normal_mat=s['N'][:1], power=power, depth_tol=SPHERE_TOL)
        seen = out['seen'] > 0
        to_eye = s['cam2world'][0][:3, 3].astype(np.float64) - world
        cos = (s['normals'].astype(np.float64) * to_eye).sum(1) / np.linalg.norm(to_eye, axis=1)
        assert np.allclose(out['weight'][seen], cos[seen] ** expo, rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------- ramp frames
RAMP = ((3, 2), (1, 5), (4, 0))                      # (a, b) per channel: value = a col + b row, at most 4 * 39 + 5 * 28 < 256


@pytest.mark.parametrize('vis_size, frame_size', [((32, 32), (32, 32)), ((37, 53), (29, 40)), ((16, 64), (29, 40))])
def test_ramp_frames_are_sampled_where_the_vertex_projects(vis_size, frame_size):
    fh, fw = frame_size
    verts, faces, pos = wall_with_probes(vis_size)
    vis, _ = S.rasterize_numpy(verts, faces, *PIXEL_CAMERA, vis_size)
    assert np.all(vis != EMPTY)
    col, row = np.meshgrid(np.arange(fw), np.arange(fh))
    frame = np.stack([a * col + b * row for a, b in RAMP], axis=-1)
    assert frame.max() <= 255
    out = S.bake_colors_numpy(verts, *PIXEL_CAMERA, vis, frame.astype(np.uint8)[None])
    seen = out['seen'] > 0
    assert seen[4:].all() and not seen[:4].any()                                        # the wall's own corners are outside the image
    # texel k's centre is at k + 0.5: the frame's coordinates of a vertex are (xc fw - 0.5, yc fh - 0.5), held inside the frame as the taps are
    u, v = np.clip(pos[:, 0] * fw - 0.5, 0, fw - 1), np.clip(pos[:, 1] * fh - 0.5, 0, fh - 1)
    want = np.stack([a * u + b * v for a, b in RAMP], axis=-1)
    err = np.abs(out['colors'].astype(np.float64) - want)[seen]
    clamped = ((pos[:, 0] * fw < 0.5) | (pos[:, 0] * fw > fw - 0.5) | (pos[:, 1] * fh < 0.5) | (pos[:, 1] * fh > fh - 0.5))[seen]
    print(f'{seen.sum()} probes, {clamped.sum()} with clamped taps, largest error {err.max():.3f} levels')
    assert clamped.sum() >= 20 and err.max() <= 1.0


# ---------------------------------------------------------------------------------------------------------------- order
def test_permuting_the_vertices_permutes_the_outputs():
    verts, faces, normals, fallback = bake_soup(500)
    A, K, N = orbit_views(3)
    vis, _ = S.rasterize_numpy(verts, faces, A, K, (37, 53))
    frames = np.random.default_rng(2).integers(0, 256, (3, 40, 29, 3), dtype=np.uint8)
    out = S.bake_colors_numpy(verts, A, K, vis, frames, normals=normals, normal_mat=N, fallback=fallback)
    perm = np.random.default_rng(3).permutation(len(verts))
    moved = S.bake_colors_numpy(verts[perm], A, K, vis, frames, normals=normals[perm], normal_mat=N, fallback=fallback[perm])
    assert (out['seen'] > 0).sum() >= 50 and len(np.unique(out['colors'][out['seen'] > 0], axis=0)) > 20
    assert np.array_equal(moved['colors'], out['colors'][perm]) and np.array_equal(moved['seen'], out['seen'][perm])
    assert np.array_equal(moved['weight'].view(np.uint32), out['weight'][perm].view(np.uint32))
    # bake_mesh_colors on arrays is the two ports in a row
    cam2world, K33 = orbit_cameras()
    whole = S.bake_mesh_colors(verts, faces, frames, cam2world.numpy(), K33.numpy(), normals=normals, vis_size=(37, 53), fallback=fallback)
    assert all(np.array_equal(whole[k], out[k]) for k in ('colors', 'weight', 'seen'))
    with pytest.raises(ValueError):
        S.bake_mesh_colors(verts, faces, frames, cam2world.numpy(), K33.numpy(), tolerance=0.1)
    line = S.bake_report_line(out, 3)
    n_seen = int((out['seen'] > 0).sum())
    assert line.startswith('mesh bake: 3 views, ') and f'{n_seen} of {len(verts)} vertices seen' in line
    assert f'median {np.median(out["seen"][out["seen"] > 0]):g} views per seen vertex' in line
    empty = S.bake_colors_numpy(np.zeros((0, 3), np.float32), A, K, vis, frames)
    assert empty['colors'].shape == (0, 3) and empty['weight'].shape == (0,) and empty['seen'].shape == (0,)
    assert 'mesh bake: 3 views, 0 of 0' in S.bake_report_line(empty, 3)


# ---------------------------------------------------------------------------------------------------------------- interface
def test_argument_errors_need_no_gpu():
    import gnerf_hip
    verts, faces, _, _, A, K = two_squares()
    vis, _ = S.rasterize_numpy(verts, faces, A, K, 8)
    frames = np.zeros((2, 8, 8, 3), dtype=np.uint8)
    normals = np.ones_like(verts)
    for bad in (dict(near=0.0), dict(depth_tol=-1e-3), dict(depth_tol=float('nan')), dict(guard=5), dict(guard=-1), dict(guard=1.5), dict(power=9),
                dict(power=-1), dict(normals=normals), dict(fallback=np.zeros((3, 3), dtype=np.uint8)), dict(fallback=np.zeros((len(verts), 3)))):
        with pytest.raises(ValueError):
            S.bake_colors_numpy(verts, A, K, vis, frames, **bad)
    with pytest.raises(ValueError):
        S.bake_colors_numpy(verts, A, K, vis[:1], frames)
    with pytest.raises(ValueError):
        S.bake_colors_numpy(verts, A, K, vis, frames.astype(np.float32))
    # gnerf_hip.bake_colors checks the rules before it looks at a tensor; CPU tensors never reach the library
    t = [torch.from_numpy(x) for x in (verts, A, K, vis.view(np.int64), frames)]
    for bad in (dict(near=0.0), dict(depth_tol=-1e-3), dict(guard=5), dict(guard=1.5), dict(power=9), dict(power=-1)):
        with pytest.raises(ValueError):
            gnerf_hip.bake_colors(*t, **bad)
    with pytest.raises(RuntimeError):
        gnerf_hip.bake_colors(*t)
    assert gnerf_hip.BAKE_RULES == S.BAKE_RULES == dict(near=0.01, depth_tol=2.0 ** -8, guard=1, min_cos=0.1, power=2)


def test_bake_declarations_and_the_c_entry_point_without_a_gpu():
    import gnerf_hip
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    assert int(re.search(r'#define GNERF_ABI_VERSION (\d+)', header).group(1)) == gnerf_hip.ABI_VERSION == 15
    assert int(re.search(r'#define GNERF_BAKE_MAX_GUARD (\d+)', header).group(1)) == gnerf_hip.BAKE_MAX_GUARD == 4
    assert int(re.search(r'#define GNERF_BAKE_MAX_POWER (\d+)', header).group(1)) == gnerf_hip.BAKE_MAX_POWER == 8
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    sig = (i, [p, i, p, p, i, p, i, i, p, i, i, p, p, f, f, i, f, i, p, p, p, p, p])
    name = 'gnerf_mesh_bake_colors'
    assert gnerf_hip.SIGNATURES[name] == sig and name in gnerf_hip.OPTIONAL_SYMBOLS
    args = re.search(name + r'\s*\((.*?)\)\s*;', re.sub(r'/\*.*?\*/', '', header, flags=re.S), flags=re.S).group(1)
    assert len(args.split(',')) == len(sig[1])
    binding = open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'torch_binding.cpp')).read()
    assert name + '(' in binding and re.search(r'm\.def\("mesh_bake_colors"', binding)
    lib = gnerf_hip.load()
    assert hasattr(lib, name) and gnerf_hip.bake_available()
    for public in ('bake_colors', 'bake_available', '_bake_colors_ctypes'):
        assert callable(getattr(gnerf_hip, public))
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)

    def bake(verts=ptr, n_verts=3, views=1, vis=ptr, size=(8, 8), frames=ptr, fsize=(8, 8), normals=None, nmat=None, near=0.01, tol=2.0 ** -8, guard=1,
             min_cos=0.1, power=2, colors=ptr):
        return lib.gnerf_mesh_bake_colors(verts, n_verts, ptr, ptr, views, vis, *size, frames, *fsize, normals, nmat, near, tol, guard, min_cos, power, None,
                                          colors, None, None, None)
    for kw, word in ((dict(verts=None), b'null'), (dict(vis=None), b'null'), (dict(frames=None), b'null'), (dict(colors=None), b'null'),
                     (dict(n_verts=-1), b'negative'), (dict(views=0), b'n_views'), (dict(size=(8, 4097)), b'size'), (dict(fsize=(0, 8)), b'size'),
                     (dict(near=0.0), b'near'), (dict(tol=-1.0), b'depth_tol'), (dict(guard=5), b'guard'), (dict(guard=-1), b'guard'),
                     (dict(power=9), b'power'), (dict(power=-1), b'power'), (dict(normals=ptr), b'normal_mat')):
        assert bake(**kw) == -1 and word in lib.gnerf_last_error(), kw
    assert bake(n_verts=0, verts=None, colors=None) == 0                                # an empty mesh is valid, and launches nothing


def test_mesh_bake_flag_requires_mesh():
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.join(ROOT, 'g-nerf_amd'), ROOT, env.get('PYTHONPATH', '')])
    script = os.path.join(ROOT, 'g-nerf_amd', 'gen_videos_mi355x.py')
    for flags, word in ((['--mesh-bake', '2'], '--mesh-bake requires --mesh'), (['--mesh', 'g.ply', '--mesh-bake', '2', '--mesh-bake-guard', '5'], '--mesh-bake-guard')):
        r = subprocess.run([sys.executable, script, '--random-init', '--device', 'cpu'] + flags, capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 2 and word in r.stderr, r.stderr[-1000:]


# ---------------------------------------------------------------------------------------------------------------- round trip
def test_round_trip_through_render_mesh(sphere):
    """Colour the sphere by an affine function of position, draw it unlit from the three cameras, bake the frames back: a seen vertex gets
    its own colour back within the bound below.  The frame's pixels are the colour function at the surface points their centres see (the
    rasteriser mixes vertex colours linearly; an affine function survives that up to the vertex colours' rounding, 0.5 level, and the
    frame's own, 0.5 level: the + 1).  The bilinear sample at the vertex's position mixes pixel centres at most one pixel away in each
    direction, 1.5 pixels allowing for the diagonal; a pixel is z / (fx size) wide at depth z, and on a surface tilted to cosine c against
    the line of sight that footprint is 1 / c as long, c > min_cos.  So |error| <= G * 1.5 * footprint / min_cos + 1 for a colour gradient
    of G levels per unit of length."""
    s = sphere
    size, min_cos, G = 96, 0.1, 120.0
    radius = SPHERE_R * SPHERE_SCALE
    fx = float(s['K'][0][0])
    z_max = float(np.linalg.norm(s['cam2world'][0][:3, 3])) + radius
    footprint = z_max / (fx * size)
    bound = G * 1.5 * footprint / min_cos + 1
    assert bound < 16
    world = s['verts'].astype(np.float64) @ s['mesh2world'][:, :3].T + s['mesh2world'][:, 3]
    dirs = np.array([[1.0, 0, 0], [0, 1.0, 0], [0.6, 0, 0.8]])                          # unit gradients, one per channel
    exact = 128 + G * world @ dirs.T
    assert exact.min() >= 0 and exact.max() <= 255
    colors = np.rint(exact).astype(np.uint8)
    drawn = S.render_mesh(s['verts'], s['faces'], s['cam2world'], s['K33'], size, mesh2world=s['mesh2world'], colors=colors,
                          shading=dict(ambient=1.0, diffuse=0.0), outputs=('frame',))
    out = S.bake_colors_numpy(s['verts'], s['A'], s['K'], s['vis'], drawn['frame'], normals=s['normals'], normal_mat=s['N'], min_cos=min_cos,
                              depth_tol=SPHERE_TOL)
    seen = out['seen'] > 0
    err = np.abs(out['colors'].astype(np.float64) - exact)[seen]
    print(f'{seen.sum()} of {len(seen)} vertices seen, largest error {err.max():.2f} levels, bound {bound:.2f}')
    assert seen.sum() > len(seen) / 2 and err.max() <= bound
    assert np.ptp(out['colors'][seen].astype(int), axis=0).min() > 40                   # the colours do vary
    whole = S.bake_mesh_colors(s['verts'], s['faces'], drawn['frame'], s['cam2world'], s['K33'], mesh2world=s['mesh2world'], normals=s['normals'],
                               depth_tol=SPHERE_TOL)
    assert all(np.array_equal(whole[k], out[k]) for k in ('colors', 'weight', 'seen'))
