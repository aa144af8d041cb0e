"""CPU tests of the texture atlas (shape_mi355x.atlas_layout / atlas_uvs / bake_texture_numpy / resolve_textured_numpy, the references the
kernels of csrc/raster.hip match bit for bit) and of the host logic around it: the layout rule and its closure under bilinear sampling,
properties of the bake's port, a round trip through the textured resolve, the PNG and OBJ writers, the declarations and the argument
errors of the C entry points."""

import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest

import shape_mi355x as S
from test_mesh_bake_cpu import SQUARES_SIZE, VIS_SIZE, FRAME_SIZE, bake_soup, constant_frames, orbit_views, random_frames, two_squares
from test_raster_cpu import orbit_cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCHES = tuple(range(4, 18))
TRIANGLE_COUNTS = (0, 1, 2, 3, 7, 8, 9, 50)


# ---------------------------------------------------------------------------------------------------------------- the rule, restated
def owners(n_tris, P):
    """How many triangles own every texel, and which (the last to claim it), straight from the rule's text: a loop over the triangles."""
    n_pairs = (n_tris + 1) // 2
    C = next(c for c in range(n_pairs + 2) if c * c >= n_pairs)
    rows = -(-n_pairs // C) if C else 0
    count = np.zeros((rows * P, C * P), dtype=np.int64)
    owner = np.full((rows * P, C * P), -1, dtype=np.int64)
    for t in range(n_tris):
        pair, half = t >> 1, t & 1
        y0, x0 = (pair // C) * P, (pair % C) * P
        for j in range(P):
            for i in range(P):
                if (i + j <= P - 1) if half == 0 else (i + j >= P):
                    count[y0 + j, x0 + i] += 1
                    owner[y0 + j, x0 + i] = t
    return C, count, owner


def corner_texels(n_tris, P, C):
    """(x, y) int [n_tris, 3] of the three corners' texels, from the rule's text."""
    L = P - 3
    out = np.zeros((n_tris, 3, 2), dtype=np.int64)
    for t in range(n_tris):
        pair, half = t >> 1, t & 1
        for k, (i, j) in enumerate(((0, 0), (L, 0), (0, L))):
            if half:
                i, j = P - 1 - i, P - 1 - j
            out[t, k] = ((pair % C) * P + i, (pair // C) * P + j)
    return out


@pytest.mark.parametrize('P', PATCHES)
def test_layout_ownership_corners_uvs_and_closure(P):
    lib = __import__('gnerf_hip').load()
    for n_tris in TRIANGLE_COUNTS:
        C, count, owner = owners(n_tris, P)
        cells, th, tw = S.atlas_layout(n_tris, P)
        assert (cells, th, tw) == (C, *count.shape), (n_tris, P)
        c_cells, c_th, c_tw = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.gnerf_mesh_atlas_layout(n_tris, P, ctypes.byref(c_cells), ctypes.byref(c_th), ctypes.byref(c_tw)) == 0
        assert (c_cells.value, c_th.value, c_tw.value) == (cells, th, tw)
        uvs = S.atlas_uvs(n_tris, P)
        assert uvs.dtype == np.float32 and uvs.shape == (n_tris, 3, 2)
        if n_tris == 0:
            assert (cells, th, tw) == (0, 0, 0)
            continue
        assert C * C >= (n_tris + 1) // 2 > (C - 1) * (C - 1) and th <= tw
        assert count.max() == 1, 'a texel with two owners'
        per_tri = np.bincount(owner[owner >= 0], minlength=n_tris)
        assert np.all(per_tri[0::2] == P * (P + 1) // 2) and np.all(per_tri[1::2] == P * (P - 1) // 2)
        assert (owner >= 0).sum() == per_tri.sum() and (owner < 0).sum() == th * tw - per_tri.sum()
        # the port's own map of the texels is the rule's
        tri, li, lj = S._atlas_texels(n_tris, P)
        assert np.array_equal(tri, owner) and li.min() >= 0 and lj.min() >= 0 and (li + lj)[owner >= 0].max() <= P - 1
        # corners sit on texel centres, and those texels are the triangle's own; atlas_uvs names the same texels
        corners = corner_texels(n_tris, P, C)
        assert np.all(owner[corners[..., 1], corners[..., 0]] == np.arange(n_tris)[:, None])
        x, y = uvs[..., 0].astype(np.float64) * tw - 0.5, uvs[..., 1].astype(np.float64) * th - 0.5
        assert np.abs(x - corners[..., 0]).max() < 1e-3 and np.abs(y - corners[..., 1]).max() < 1e-3
        # closure: a bilinear sample anywhere in the triangle's image, its edges and corners included, touches the triangle's own texels only
        D = 12
        bary = np.array([(a, b, D - a - b) for a in range(D + 1) for b in range(D + 1 - a)], dtype=np.float64) / D
        bary = np.concatenate([bary, np.random.default_rng(P).dirichlet((1, 1, 1), 60)])
        pos = np.einsum('bk,tkc->tbc', bary, corners.astype(np.float64))                 # [n_tris, points, (x, y)]
        fx, fy = np.floor(pos[..., 0] + 1e-9), np.floor(pos[..., 1] + 1e-9)             # (1e-9: a point that should sit on a centre does)
        wx, wy = np.clip(pos[..., 0] - fx, 0, 1), np.clip(pos[..., 1] - fy, 0, 1)
        wx, wy = np.where(wx < 1e-8, 0.0, wx), np.where(wy < 1e-8, 0.0, wy)
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            weight = (wx if dx else 1 - wx) * (wy if dy else 1 - wy)
            tx, ty = (fx + dx).astype(np.int64), (fy + dy).astype(np.int64)
            used = weight > 0
            assert np.all((tx[used] >= 0) & (tx[used] < tw) & (ty[used] >= 0) & (ty[used] < th))
            got = owner[ty[used], tx[used]]
            want = np.broadcast_to(np.arange(n_tris)[:, None], used.shape)[used]
            assert np.array_equal(got, want), (n_tris, P, dx, dy)


def test_sizes_past_the_cap_and_patches_out_of_range_fail():
    import gnerf_hip
    lib = gnerf_hip.load()
    out = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int()]
    refs = [ctypes.byref(x) for x in out]
    fits, too_many = 2 * 2048 * 2048, 2 * 2048 * 2048 + 1                               # 2048 cells of 8 texels are 16384: the cap
    assert lib.gnerf_mesh_atlas_layout(fits, 8, *refs) == 0 and [x.value for x in out] == [2048, 16384, 16384]
    assert S.atlas_layout(fits, 8) == (2048, 16384, 16384)
    assert lib.gnerf_mesh_atlas_layout(too_many, 8, *refs) == gnerf_hip.E_UNSUPPORTED == -3 and b'atlas' in lib.gnerf_last_error()
    assert lib.gnerf_mesh_atlas_layout(2 * 257 * 257, 64, *refs) == -3
    with pytest.raises(ValueError):
        S.atlas_layout(too_many, 8)
    for patch in (3, 65, -1, 0):
        assert lib.gnerf_mesh_atlas_layout(10, patch, *refs) == -1 and b'patch' in lib.gnerf_last_error()
        with pytest.raises(ValueError):
            S.atlas_layout(10, patch)
    assert lib.gnerf_mesh_atlas_layout(-1, 8, *refs) == -1
    assert lib.gnerf_mesh_atlas_layout(10, 8, None, refs[1], refs[2]) == -1
    with pytest.raises(ValueError):
        S.atlas_layout(10, 7.5)
    assert (gnerf_hip.ATLAS_MIN_PATCH, gnerf_hip.ATLAS_MAX_PATCH, gnerf_hip.ATLAS_MAX_SIZE) == (S.ATLAS_MIN_PATCH, S.ATLAS_MAX_PATCH, S.ATLAS_MAX_SIZE) == (4, 64, 16384)
    assert gnerf_hip.atlas_layout(7, 5) == S.atlas_layout(7, 5) == (2, 10, 10)


# ---------------------------------------------------------------------------------------------------------------- the bake's port
@pytest.fixture(scope='module')
def soup():
    """A soup of 201 triangles (an odd count: the last cell is half empty, and the last row of cells partly) from the three orbit cameras."""
    verts, faces, normals, fallback = bake_soup(201)
    A, K, N = orbit_views(3)
    vis, _ = S.rasterize_numpy(verts, faces, A, K, VIS_SIZE)
    return dict(verts=verts, faces=faces, normals=normals, fallback=fallback, A=A, K=K, N=N, vis=vis)


def fallback_mix(faces, fallback, tri, li, lj, P):
    """(b0 c0 + b1 c1) + b2 c2 in float32, clamped and rounded, for the owned texels (tri >= 0)."""
    f32 = np.float32
    own = tri >= 0
    g = faces[tri[own]]
    b1, b2 = li[own].astype(f32) / f32(P - 3), lj[own].astype(f32) / f32(P - 3)
    b0 = (f32(1) - b1) - b2
    c = fallback.astype(f32)
    mix = (b0[:, None] * c[g[:, 0]] + b1[:, None] * c[g[:, 1]]) + b2[:, None] * c[g[:, 2]]
    return np.rint(np.clip(mix, 0, 255)).astype(np.uint8)


@pytest.mark.parametrize('with_normals', [False, True], ids=['plain', 'normals'])
def test_constant_frames_give_their_colour_in_every_seen_texel(soup, with_normals):
    s = soup
    colour, background = (201, 17, 96), (7, 8, 9)
    frames = constant_frames([colour] * 3, *FRAME_SIZE)
    kw = dict(normals=s['normals'], normal_mat=s['N']) if with_normals else {}
    for P in (4, 8):
        _, count, owner = owners(len(s['faces']), P)
        for fb in (s['fallback'], None):
            out = S.bake_texture_numpy(s['verts'], s['faces'], s['A'], s['K'], s['vis'], frames, patch=P, fallback=fb, background=background, **kw)
            assert out['texture'].dtype == np.uint8 and out['weight'].dtype == np.float32 and out['seen'].dtype == np.int32
            assert out['texture'].shape == (*owner.shape, 3) and out['weight'].shape == owner.shape and out['seen'].shape == owner.shape
            seen, unseen, nobody = out['seen'] > 0, out['seen'] == 0, out['seen'] < 0
            assert np.array_equal(nobody, owner < 0) and nobody.sum() >= P * (P - 1) // 2
            assert seen.sum() >= 100 and unseen.sum() >= 100                            # (neither kind is a handful: the checks below bite)
            assert np.all(out['texture'][seen] == np.array(colour, dtype=np.uint8))
            assert np.all(out['texture'][nobody] == np.array(background, dtype=np.uint8)) and np.all(out['weight'][nobody] == 0)
            assert np.array_equal(out['weight'] > 0, seen) and out['seen'].max() <= 3
            if fb is None:
                assert np.all(out['texture'][unseen] == np.array(background, dtype=np.uint8))
            else:
                tri, li, lj = S._atlas_texels(len(s['faces']), P)
                want = np.zeros_like(out['texture'])
                want[tri >= 0] = fallback_mix(s['faces'], fb, tri, li, lj, P)
                assert np.array_equal(out['texture'][unseen], want[unseen])


def test_an_unseen_mesh_holds_the_fallback_mix_or_the_background(soup):
    s = soup
    away = s['A'].copy().reshape(-1, 3, 4)
    away[:, 2] = -away[:, 2]                                                             # every point behind its camera
    away = away.reshape(-1, 12)
    frames = random_frames(3, FRAME_SIZE, seed=1)
    P = 6
    _, _, owner = owners(len(s['faces']), P)
    vis = np.full_like(s['vis'], 0xFFFFFFFFFFFFFFFF)
    out = S.bake_texture_numpy(s['verts'], s['faces'], away, s['K'], vis, frames, patch=P, fallback=s['fallback'], background=(1, 2, 3))
    assert out['seen'].max() == 0 and np.array_equal(out['seen'] == 0, owner >= 0) and not out['weight'].any()
    tri, li, lj = S._atlas_texels(len(s['faces']), P)
    assert np.array_equal(out['texture'][owner >= 0], fallback_mix(s['faces'], s['fallback'], tri, li, lj, P))
    corners = corner_texels(len(s['faces']), P, S.atlas_layout(len(s['faces']), P)[0])
    assert np.array_equal(out['texture'][corners[..., 1], corners[..., 0]], s['fallback'][s['faces']])      # b is 0 or 1 there: the vertex's own colour
    assert np.all(out['texture'][owner < 0] == np.array([1, 2, 3], dtype=np.uint8))
    bare = S.bake_texture_numpy(s['verts'], s['faces'], away, s['K'], vis, frames, patch=P, background=(1, 2, 3))
    assert np.all(bare['texture'] == np.array([1, 2, 3], dtype=np.uint8)) and np.array_equal(bare['seen'], out['seen'])


def texels_of(tri_map, li, lj, t):
    """Flat texel indices of triangle t, ordered by its local indices (lj, li): the order of its barycentrics."""
    idx = np.nonzero(tri_map.ravel() == t)[0]
    return idx[np.lexsort((li.ravel()[idx], lj.ravel()[idx]))]


def test_texels_do_not_depend_on_the_order_of_the_faces(soup):
    s = soup
    frames = random_frames(3, FRAME_SIZE, seed=2)
    P = 5
    perm = np.random.default_rng(3).permutation(len(s['faces']))
    moved_faces = s['faces'][perm]
    moved_vis, _ = S.rasterize_numpy(s['verts'], moved_faces, s['A'], s['K'], VIS_SIZE)
    kw = dict(patch=P, normals=s['normals'], normal_mat=s['N'], fallback=s['fallback'])
    out = S.bake_texture_numpy(s['verts'], s['faces'], s['A'], s['K'], s['vis'], frames, **kw)
    moved = S.bake_texture_numpy(s['verts'], moved_faces, s['A'], s['K'], moved_vis, frames, **kw)
    tri, li, lj = S._atlas_texels(len(s['faces']), P)
    assert (out['seen'] > 0).sum() >= 200 and len(np.unique(out['texture'][out['seen'] > 0], axis=0)) > 50
    halves_swapped = 0
    diagonal = (li + lj).ravel()
    for new, old in enumerate(perm):
        a, b = texels_of(tri, li, lj, old), texels_of(tri, li, lj, new)
        halves_swapped += len(a) != len(b)
        if len(a) != len(b):                                                            # (half 0 alone has the spare diagonal li + lj = P - 1)
            a, b = a[diagonal[a] <= P - 2], b[diagonal[b] <= P - 2]
        assert len(a) == len(b) >= P * (P - 1) // 2
        for name in ('texture', 'weight', 'seen'):
            x, y = out[name].reshape(tri.size, -1), moved[name].reshape(tri.size, -1)
            assert np.array_equal(x[a].view(np.uint8), y[b].view(np.uint8)), (name, old, new)
    assert halves_swapped > 20


def test_a_texel_on_a_vertex_is_that_vertex_of_the_vertex_bake(soup):
    s = soup
    frames = random_frames(1, FRAME_SIZE, seed=4)
    one = dict(mesh2cam=s['A'][:1], intrinsics=s['K'][:1], vis=s['vis'][:1], frames=frames)
    for P in (4, 7):
        # a corner's barycentrics are exactly 0 and 1, so its point is the vertex itself, bit for bit, in either half
        tri, li, lj = S._atlas_texels(len(s['faces']), P)
        corners = corner_texels(len(s['faces']), P, S.atlas_layout(len(s['faces']), P)[0])
        f32 = np.float32
        b1, b2 = li[corners[..., 1], corners[..., 0]].astype(f32) / f32(P - 3), lj[corners[..., 1], corners[..., 0]].astype(f32) / f32(P - 3)
        b0 = (f32(1) - b1) - b2
        assert np.array_equal(np.stack([b0, b1, b2], axis=-1), np.broadcast_to(np.eye(3, dtype=f32), (len(s['faces']), 3, 3)))
        v = s['verts'][s['faces']]                                                      # [T, corner, xyz]
        points = (b0[..., None] * v[:, None, 0] + b1[..., None] * v[:, None, 1]) + b2[..., None] * v[:, None, 2]
        assert points.dtype == f32 and np.array_equal(points.view(np.uint32), v.view(np.uint32))
        for guard in (0, 1):
            per_vertex = S.bake_colors_numpy(s['verts'], power=0, guard=guard, fallback=s['fallback'], **one)
            out = S.bake_texture_numpy(s['verts'], s['faces'], patch=P, power=0, guard=guard, fallback=s['fallback'], **one)
            corners = corner_texels(len(s['faces']), P, S.atlas_layout(len(s['faces']), P)[0])
            ys, xs = corners[..., 1], corners[..., 0]
            assert (per_vertex['seen'][s['faces']] > 0).sum() >= 30 and (per_vertex['seen'][s['faces']] == 0).sum() >= 30
            assert np.array_equal(out['texture'][ys, xs], per_vertex['colors'][s['faces']])
            assert np.array_equal(out['seen'][ys, xs], per_vertex['seen'][s['faces']])
            assert np.array_equal(out['weight'][ys, xs].view(np.uint32), per_vertex['weight'][s['faces']].view(np.uint32))


def test_mesh_level_entries_are_the_ports_in_a_row(soup):
    s = soup
    frames = random_frames(3, FRAME_SIZE, seed=5)
    cam2world, K33 = orbit_cameras()
    out = S.bake_texture_numpy(s['verts'], s['faces'], s['A'], s['K'], s['vis'], frames, patch=6, normals=s['normals'], normal_mat=s['N'],
                               fallback=s['fallback'], background=(9, 9, 9))
    whole = S.bake_mesh_texture(s['verts'], s['faces'], frames, cam2world.numpy(), K33.numpy(), patch=6, normals=s['normals'], vis_size=VIS_SIZE,
                                fallback=s['fallback'], background=(9, 9, 9))
    assert all(np.array_equal(whole[k].view(np.uint8), out[k].view(np.uint8)) for k in ('texture', 'weight', 'seen'))
    with pytest.raises(ValueError):
        S.bake_mesh_texture(s['verts'], s['faces'], frames, cam2world.numpy(), K33.numpy(), tolerance=0.1)
    # render_mesh with a texture: the frame is the textured resolve's, on the shading's background; the other outputs are as without it
    plain = S.render_mesh(s['verts'], s['faces'], cam2world.numpy(), K33.numpy(), VIS_SIZE)
    drawn = S.render_mesh(s['verts'], s['faces'], cam2world.numpy(), K33.numpy(), VIS_SIZE, texture=out['texture'], patch=6,
                          shading=dict(background=(0.0, 1.0, 0.2)))
    want = S.resolve_textured_numpy(s['vis'], s['verts'], s['faces'], s['A'], s['K'], out['texture'], patch=6, background=(0, 255, 51))
    assert np.array_equal(drawn['frame'], want) and not np.array_equal(drawn['frame'], plain['frame'])
    assert all(np.array_equal(drawn[k], plain[k]) for k in ('tri_id', 'depth', 'normal', 'counts'))
    assert np.all(want[plain['tri_id'] < 0] == np.array([0, 255, 51], dtype=np.uint8)) and (plain['tri_id'] >= 0).sum() > 100
    only = S.render_mesh(s['verts'], s['faces'], cam2world.numpy(), K33.numpy(), VIS_SIZE, texture=out['texture'], patch=6, outputs=('frame',))
    assert set(only) == {'frame', 'counts'}
    with pytest.raises(ValueError):
        S.resolve_textured_numpy(s['vis'], s['verts'], s['faces'], s['A'], s['K'], out['texture'], patch=7)
    line = S.texture_report_line(out, 3, 6)
    owned, n_seen = int((out['seen'] >= 0).sum()), int((out['seen'] > 0).sum())
    th, tw = out['seen'].shape
    assert line.startswith(f'mesh texture: {tw} x {th} atlas (patch 6), 3 views, {n_seen} of {owned} owned texels seen')
    assert f'median {np.median(out["seen"][out["seen"] > 0]):g} views per seen texel' in line
    # finish_mesh runs the texture stage after the bake and keeps its record's six fields
    calls = []
    done = S.finish_mesh(s['verts'], s['faces'], bake=lambda v, f, n, c: calls.append('bake') or dict(colors=None),
                         texture=lambda v, f, n, c: calls.append('texture') or out)
    assert calls == ['bake', 'texture'] and done.reports['texture'] is out and len(done) == 6 and S.FinishedMesh._fields[-1] == 'reports'
    assert 'texture' not in S.finish_mesh(s['verts'], s['faces']).reports
    empty = S.bake_texture_numpy(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), s['A'], s['K'], s['vis'], frames)
    assert empty['texture'].shape == (0, 0, 3) and empty['weight'].shape == (0, 0) and empty['seen'].shape == (0, 0)
    assert 'mesh texture: 0 x 0 atlas' in S.texture_report_line(empty, 3, 8)


def test_a_face_with_a_vertex_out_of_range_stays_background(soup):
    s = soup
    faces = s['faces'].copy()
    faces[4, 1], faces[9, 2] = len(s['verts']), -1
    frames = random_frames(3, FRAME_SIZE, seed=6)
    out = S.bake_texture_numpy(s['verts'], faces, s['A'], s['K'], s['vis'], frames, patch=8, fallback=s['fallback'], background=(50, 60, 70))
    _, _, owner = owners(len(faces), 8)
    bad = (owner == 4) | (owner == 9)
    assert bad.sum() == 36 + 28 and np.all(out['seen'][bad] == -1) and np.all(out['texture'][bad] == np.array([50, 60, 70], dtype=np.uint8))
    good = S.bake_texture_numpy(s['verts'], s['faces'], s['A'], s['K'], s['vis'], frames, patch=8, fallback=s['fallback'], background=(50, 60, 70))
    assert all(np.array_equal(out[k][~bad], good[k][~bad]) for k in out)


# ---------------------------------------------------------------------------------------------------------------- round trip
def test_round_trip_of_a_ramp_through_bake_and_textured_resolve():
    """The two squares face the front camera, fronto-parallel, and the frame is a ramp that is affine in image coordinates, so it is affine in
    every patch's coordinates too and bilinear sampling reproduces an affine function exactly.  What is left are the roundings to uint8: the
    frame's own (each tap within 0.5 level of the ramp, so their bilinear mix is), the bake's (0.5 more: a texel is within 1 level of the ramp
    at its point), the resolve's mix of such texels (within 1) and its rounding (0.5 more: 1.5 from the ramp at the pixel's centre), and the
    frame value it is compared with is itself within 0.5 of that.  |resolve - frame| <= 2 levels, an integer, so float32's own error of some
    1e-4 levels cannot add one.  Checked where the whole (2 (guard + 1) + 1)^2 window of a pixel lies on one square: away from every
    silhouette by guard + 1 pixels -- nearer, the bake's window test leaves texels unseen on purpose."""
    verts, faces, is_back, pos, A, K = two_squares()
    size = SQUARES_SIZE
    vis, counts = S.rasterize_numpy(verts, faces, A[:1], K[:1], size)
    assert counts[0] == counts.sum()
    col, row = np.meshgrid(np.arange(size), np.arange(size))
    exact = np.stack([3.3 * col + 2.9 * row + 10.2, 201.7 - 1.7 * col - 4.1 * row, 0.37 * col + 7.3 * row + 1.5], axis=-1)
    assert exact.min() >= 0 and exact.max() <= 255
    frame = np.rint(exact).astype(np.uint8)[None]
    tri_id = S.resolve_numpy(vis, verts, faces, A[:1], K[:1], outputs=('tri_id',))['tri_id'][0]
    square = np.where(tri_id < 0, -1, is_back[faces[np.maximum(tri_id, 0), 0]].astype(np.int64))       # -1 empty, 0 front, 1 back
    bound = 2
    for guard in (0, 1, 2):
        for P in (4, 8, 11):
            baked = S.bake_texture_numpy(verts, faces, A[:1], K[:1], vis, frame, patch=P, guard=guard, background=(255, 0, 255))
            drawn = S.resolve_textured_numpy(vis, verts, faces, A[:1], K[:1], baked['texture'], patch=P, background=(0, 0, 0))[0]
            m = guard + 1
            inner = np.zeros((size, size), dtype=bool)
            for r in range(m, size - m):
                for c in range(m, size - m):
                    window = square[r - m:r + m + 1, c - m:c + m + 1]
                    inner[r, c] = window[0, 0] >= 0 and np.all(window == window[0, 0])
            err = np.abs(drawn.astype(np.int64) - frame[0].astype(np.int64))[inner]
            print(f'guard {guard}, patch {P}: {inner.sum()} pixels ({(inner & (square == 0)).sum()} on the front square), largest error {err.max()} levels')
            assert (inner & (square == 0)).sum() >= 4 and (inner & (square == 1)).sum() >= 150
            assert err.max() <= bound
            assert np.ptp(drawn[inner].astype(int), axis=0).min() > 20                  # the frame does vary there


# ---------------------------------------------------------------------------------------------------------------- files
def decode_png(path):
    """A PNG of the kind write_png makes, by hand: (chunks as (kind, data, crc ok), rgb uint8 [h, w, 3])."""
    raw = open(path, 'rb').read()
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, []
    while at < len(raw):
        n, kind = struct.unpack('>I4s', raw[at:at + 8])
        data = raw[at + 8:at + 8 + n]
        crc, = struct.unpack('>I', raw[at + 8 + n:at + 12 + n])
        chunks.append((kind, data, crc == (zlib.crc32(kind + data) & 0xFFFFFFFF)))
        at += 12 + n
    assert at == len(raw)
    w, h, depth, colour, compression, filt, interlace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, compression, filt, interlace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b''.join(d for k, d, _ in chunks if k == b'IDAT')), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any(), 'filter type 0 on every row'
    return chunks, rows[:, 1:].reshape(h, w, 3)


@pytest.mark.parametrize('shape', [(1, 1), (5, 3), (64, 96)])
def test_write_png_round_trips(tmp_path, shape):
    rgb = np.random.default_rng(shape[0]).integers(0, 256, (*shape, 3), dtype=np.uint8)
    path = str(tmp_path / 't.png')
    S.write_png(path, rgb)
    chunks, back = decode_png(path)
    assert [k for k, _, _ in chunks][0] == b'IHDR' and [k for k, _, _ in chunks][-1] == b'IEND' and all(ok for _, _, ok in chunks)
    assert struct.unpack('>II', chunks[0][1][:8]) == (shape[1], shape[0]) and len(chunks[0][1]) == 13 and chunks[-1][1] == b''
    assert np.array_equal(back, rgb)
    for bad in (rgb.astype(np.float32), rgb[..., :2], rgb[:0]):
        with pytest.raises(ValueError):
            S.write_png(path, bad)


def test_write_png_is_read_by_pil(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    rgb = np.random.default_rng(0).integers(0, 256, (17, 31, 3), dtype=np.uint8)
    path = str(tmp_path / 't.png')
    S.write_png(path, rgb)
    with Image.open(path) as im:
        assert im.mode == 'RGB' and im.size == (31, 17) and np.array_equal(np.asarray(im), rgb)


@pytest.mark.parametrize('with_normals', [False, True], ids=['plain', 'normals'])
def test_write_obj_is_parsed_back(tmp_path, with_normals):
    verts, faces, normals, _ = bake_soup(7)
    P = 5
    uvs = S.atlas_uvs(len(faces), P)
    _, th, tw = S.atlas_layout(len(faces), P)
    texture = np.random.default_rng(1).integers(0, 256, (th, tw, 3), dtype=np.uint8)
    path = str(tmp_path / 'head.obj')
    png = S.write_obj(path, verts, faces, uvs, texture, normals=normals if with_normals else None)
    assert png == str(tmp_path / 'head.png') and np.array_equal(decode_png(png)[1], texture)
    mtl = open(str(tmp_path / 'head.mtl')).read().split('\n')
    assert 'newmtl head' in mtl and 'map_Kd head.png' in mtl
    rows = [line.split() for line in open(path).read().split('\n') if line]
    kinds = [r[0] for r in rows]
    assert rows[0] == ['mtllib', 'head.mtl'] and ['usemtl', 'head'] in rows
    assert kinds.count('v') == len(verts) and kinds.count('vt') == 3 * len(faces) and kinds.count('f') == len(faces)
    assert kinds.count('vn') == (len(verts) if with_normals else 0)
    v = np.array([r[1:] for r in rows if r[0] == 'v'], dtype=np.float64).astype(np.float32)
    vt = np.array([r[1:] for r in rows if r[0] == 'vt'], dtype=np.float64)
    assert np.array_equal(v, verts)                                                     # (nine digits bring a float32 back)
    assert np.allclose(vt[:, 0], uvs.reshape(-1, 2)[:, 0], atol=1e-7) and np.allclose(vt[:, 1], 1 - uvs.reshape(-1, 2)[:, 1].astype(np.float64), atol=1e-7)
    f = np.array([[[int(x) for x in corner.split('/')] for corner in r[1:]] for r in rows if r[0] == 'f'])
    assert f.shape == (len(faces), 3, 3 if with_normals else 2)
    assert np.array_equal(f[..., 0], faces + 1) and np.array_equal(f[..., 1], np.arange(1, 3 * len(faces) + 1).reshape(-1, 3))
    if with_normals:
        assert np.array_equal(f[..., 2], faces + 1)
        vn = np.array([r[1:] for r in rows if r[0] == 'vn'], dtype=np.float64).astype(np.float32)
        assert np.array_equal(vn, normals)
    # the texel a corner's vt names, counted from the bottom row as OBJ does, is the corner's texel
    x, y = vt[:, 0] * tw - 0.5, (1 - vt[:, 1]) * th - 0.5
    corners = corner_texels(len(faces), P, S.atlas_layout(len(faces), P)[0]).reshape(-1, 2)
    assert np.abs(x - corners[:, 0]).max() < 1e-4 and np.abs(y - corners[:, 1]).max() < 1e-4
    named = S.write_obj(str(tmp_path / 'other.obj'), verts, faces, uvs, png)            # a PNG that exists already is named, not written
    assert named == png and 'map_Kd head.png' in open(str(tmp_path / 'other.mtl')).read() and not os.path.exists(str(tmp_path / 'other.png'))
    with pytest.raises(ValueError):
        S.write_obj(path, verts, faces, uvs[:-1], texture)


# ---------------------------------------------------------------------------------------------------------------- interface
def test_texture_flags_are_declared_and_range_checked(capsys):
    import argparse
    import gen_videos_mi355x as gv
    ap = gv.arg_parser()
    ok = ap.parse_args(['--mesh', 'g.ply', '--mesh-bake', '2', '--mesh-texture', '4', '--mesh-texture-out', 'g.obj'])
    assert S.texture_from_args(ok, ap) == 4 and S.texture_from_args(ap.parse_args([]), ap) == 0
    for flags, word in ((['--mesh-texture', '3', '--mesh-bake', '2', '--mesh-texture-out', 'g.obj'], '--mesh-texture must be'),
                        (['--mesh-texture', '65', '--mesh-bake', '2', '--mesh-texture-out', 'g.obj'], '--mesh-texture must be'),
                        (['--mesh-texture', '8', '--mesh-texture-out', 'g.obj'], 'requires --mesh-bake'),
                        (['--mesh-texture', '8', '--mesh-bake', '2'], '--mesh-texture-out'),
                        (['--mesh-texture', '8', '--mesh-bake', '2', '--mesh-texture-out', 'g.ply'], '--mesh-texture-out'),
                        (['--mesh-texture-out', 'g.obj'], 'requires --mesh-texture')):
        with pytest.raises(SystemExit) as stop:
            S.texture_from_args(ap.parse_args(flags), ap)
        assert stop.value.code == 2 and word in capsys.readouterr().err, flags
    own = S.arg_parser()                                                                # the volume-only CLI gets no texture flag
    assert not any('--mesh-texture' in a.option_strings for a in own._actions) and isinstance(own, argparse.ArgumentParser)


def test_argument_errors_of_the_ports_and_the_wrappers_need_no_gpu():
    import gnerf_hip
    import torch
    verts, faces, _, _, A, K = two_squares()
    vis, _ = S.rasterize_numpy(verts, faces, A, K, 8)
    frames = np.zeros((2, 8, 8, 3), dtype=np.uint8)
    for bad in (dict(near=0.0), dict(depth_tol=-1e-3), dict(guard=5), dict(guard=1.5), dict(power=9), dict(power=-1), dict(normals=np.ones_like(verts)),
                dict(fallback=np.zeros((3, 3), dtype=np.uint8)), dict(patch=3), dict(patch=65), dict(patch=8.5), dict(background=(0, 0)),
                dict(background=(0, 0, 256)), dict(background=(0.5, 0, 0))):
        with pytest.raises(ValueError):
            S.bake_texture_numpy(verts, faces, A, K, vis, frames, **bad)
    with pytest.raises(ValueError):
        S.bake_texture_numpy(verts, faces, A, K, vis[:1], frames)
    t = [torch.from_numpy(x) for x in (verts, faces, A, K, vis.view(np.int64), frames)]
    for bad in (dict(near=0.0), dict(guard=5), dict(power=9), dict(patch=3), dict(patch=65), dict(patch=4.5), dict(background=(0, 0, 300))):
        with pytest.raises(ValueError):
            gnerf_hip.bake_texture(*t, **bad)
    with pytest.raises(RuntimeError):
        gnerf_hip.bake_texture(*t)                                                      # CPU tensors never reach the library
    with pytest.raises(ValueError):
        gnerf_hip.resolve_textured(t[4], t[0], t[1], t[2], t[3], torch.zeros(1, 1, 3, dtype=torch.uint8), patch=2)
    with pytest.raises(RuntimeError):
        gnerf_hip.resolve_textured(t[4], t[0], t[1], t[2], t[3], torch.zeros(1, 1, 3, dtype=torch.uint8))


def test_texture_declarations_and_the_c_entry_points_without_a_gpu():
    import gnerf_hip
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    assert int(re.search(r'#define GNERF_ABI_VERSION (\d+)', header).group(1)) == gnerf_hip.ABI_VERSION == 15
    for macro, value in (('GNERF_ATLAS_MIN_PATCH', 4), ('GNERF_ATLAS_MAX_PATCH', 64), ('GNERF_ATLAS_MAX_SIZE', 16384)):
        assert int(re.search(rf'#define {macro} (\d+)', header).group(1)) == value
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    pi, pb = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_ubyte)
    sigs = {'gnerf_mesh_atlas_layout': (i, [i, i, pi, pi, pi]),
            'gnerf_mesh_bake_texture': (i, [p, i, p, i, i, p, p, i, p, i, i, p, i, i, p, p, f, f, i, f, i, p, pb, p, p, p, p]),
            'gnerf_raster_resolve_textured': (i, [p, p, i, p, i, p, p, i, i, i, p, i, pb, p, p])}
    plain = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    binding = open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'torch_binding.cpp')).read()
    lib = gnerf_hip.load()
    for name, sig in sigs.items():
        assert gnerf_hip.SIGNATURES[name] == sig and name in gnerf_hip.OPTIONAL_SYMBOLS
        args = re.search(name + r'\s*\((.*?)\)\s*;', plain, flags=re.S).group(1)
        assert len(args.split(',')) == len(sig[1]), name
        assert name + '(' in binding and hasattr(lib, name)
    for bound in ('mesh_atlas_layout', 'mesh_bake_texture', 'raster_resolve_textured'):
        assert re.search(rf'm\.def\("{bound}"', binding)
    assert gnerf_hip.texture_available() and gnerf_hip.bake_available()
    for public in ('bake_texture', 'resolve_textured', 'atlas_layout', 'texture_available', '_bake_texture_ctypes', '_resolve_textured_ctypes'):
        assert callable(getattr(gnerf_hip, public))
    assert 'No UV atlas' not in header and 'no textures' not in header
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)
    bg = (ctypes.c_ubyte * 3)(1, 2, 3)

    def bake(verts=ptr, n_verts=3, faces=ptr, n_tris=1, patch=8, views=1, vis=ptr, size=(8, 8), frames=ptr, fsize=(8, 8), normals=None, nmat=None, near=0.01,
             tol=2.0 ** -8, guard=1, min_cos=0.1, power=2, background=bg, texture=ptr):
        return lib.gnerf_mesh_bake_texture(verts, n_verts, faces, n_tris, patch, ptr, ptr, views, vis, *size, frames, *fsize, normals, nmat, near, tol, guard,
                                           min_cos, power, None, background, texture, None, None, None)
    for kw, word in ((dict(verts=None), b'null'), (dict(faces=None), b'null'), (dict(vis=None), b'null'), (dict(frames=None), b'null'),
                     (dict(texture=None), b'null'), (dict(background=None), b'null'), (dict(n_verts=-1), b'negative'), (dict(n_tris=-1), b'negative'),
                     (dict(views=0), b'n_views'), (dict(size=(8, 4097)), b'size'), (dict(fsize=(0, 8)), b'size'), (dict(near=0.0), b'near'),
                     (dict(tol=-1.0), b'depth_tol'), (dict(guard=5), b'guard'), (dict(guard=-1), b'guard'), (dict(power=9), b'power'),
                     (dict(power=-1), b'power'), (dict(normals=ptr), b'normal_mat'), (dict(patch=3), b'patch'), (dict(patch=65), b'patch')):
        assert bake(**kw) == -1 and word in lib.gnerf_last_error(), kw
    assert bake(n_tris=2 * 2048 * 2048 + 1) == -3 and b'atlas' in lib.gnerf_last_error()   # past the cap: refused before any launch
    assert bake(n_tris=0, faces=None, texture=None) == 0                                # an empty mesh is valid, and launches nothing

    def resolve(vis=ptr, verts=ptr, n_verts=3, faces=ptr, n_tris=1, views=1, size=(8, 8), texture=ptr, patch=8, background=bg, frame=ptr):
        return lib.gnerf_raster_resolve_textured(vis, verts, n_verts, faces, n_tris, ptr, ptr, views, *size, texture, patch, background, frame, None)
    for kw, word in ((dict(vis=None), b'null'), (dict(verts=None), b'null'), (dict(faces=None), b'null'), (dict(texture=None), b'null'),
                     (dict(background=None), b'null'), (dict(frame=None), b'null'), (dict(n_verts=-1), b'negative'), (dict(views=0), b'n_views'),
                     (dict(size=(4097, 8)), b'size'), (dict(patch=3), b'patch'), (dict(patch=65), b'patch')):
        assert resolve(**kw) == -1 and word in lib.gnerf_last_error(), kw
    assert resolve(n_tris=2 * 2048 * 2048 + 1) == -3
