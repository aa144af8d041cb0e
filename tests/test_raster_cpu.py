"""CPU tests of the triangle rasteriser's numpy port (shape_mi355x.rasterize_numpy / resolve_numpy / render_mesh, the reference the kernels
of csrc/raster.hip match bit for bit) and of the host logic around it: the fill rule, alignment with the renderer's rays, a sphere against
its analytic depth and normals, dropped triangles and empty meshes, and the C ABI's declarations."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gnerf_harness as H
import shape_mi355x as S
from test_mesh_cpu import sphere_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)

# ---------------------------------------------------------------------------------------------------------------- hand-made scenes
# A camera whose image plane at z = 1 is the pixel grid itself: pixel-space (x, y) at depth z is the camera-frame point below, and with
# dyadic coordinates every step of the vertex stage is exact, so the snapped integers are exactly 256 x, 256 y.
PIXEL_CAMERA = (np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32).reshape(1, 12),
                np.array([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]], dtype=np.float32).reshape(1, 9))


def at_pixels(points, size, z=1.0):
    """Pixel-space points [(x, y)] or [(x, y, z)] -> float32 vertices for PIXEL_CAMERA at a size x size image."""
    out = []
    for p in points:
        d = float(p[2]) if len(p) > 2 else z
        out.append([(p[0] / size - 0.5) * d, (p[1] / size - 0.5) * d, d])
    return np.array(out, dtype=np.float32)


def square_scene(size=8):
    """A square from (1.5, 1.5) to (6.5, 6.5) split along its diagonal, which runs through pixel centres."""
    ring = [(1.5, 1.5), (6.5, 1.5), (6.5, 6.5), (1.5, 6.5)]
    return at_pixels(ring, size), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), ring, size


def fan_scene(size=16):
    """Eight triangles around an interior vertex on a pixel centre; the spokes run along pixel centres (axes and diagonals)."""
    c = (8.5, 8.5)
    ring = [(14.5, 8.5), (12.5, 12.5), (8.5, 14.5), (4.5, 12.5), (2.5, 8.5), (4.5, 4.5), (8.5, 2.5), (12.5, 4.5)]
    faces = np.array([[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)], dtype=np.int32)
    return at_pixels([c] + ring, size), faces, ring, size


def polygon_side(ring, size):
    """For every pixel centre of a size x size image: +1 strictly inside the convex polygon `ring`, 0 on its boundary, -1 outside
    (exact: integer arithmetic in 1/256 pixel)."""
    pts = [(int(round(x * 256)), int(round(y * 256))) for x, y in ring]
    side = np.zeros((size, size), dtype=np.int64)
    for r in range(size):
        for c in range(size):
            px, py = 256 * c + 128, 256 * r + 128
            cross = [(bx - ax) * (py - ay) - (by - ay) * (px - ax) for (ax, ay), (bx, by) in zip(pts, pts[1:] + pts[:1])]
            if all(v > 0 for v in cross) or all(v < 0 for v in cross):
                side[r, c] = 1
            elif all(v >= 0 for v in cross) or all(v <= 0 for v in cross):
                side[r, c] = 0
            else:
                side[r, c] = -1
    return side


def claims(verts, faces, size, cull='none'):
    """How many triangles claim each pixel when every triangle is drawn alone."""
    n = np.zeros((size, size), dtype=np.int64)
    for f in faces:
        vis, counts = S.rasterize_numpy(verts, f[None], *PIXEL_CAMERA, size, cull=cull)
        assert counts.sum() == 1
        n += vis[0] != EMPTY
    return n


@pytest.mark.parametrize('scene', [square_scene, fan_scene], ids=['square', 'fan'])
def test_fill_rule_every_inside_centre_has_exactly_one_owner(scene):
    verts, faces, ring, size = scene()
    side = polygon_side(ring, size)
    assert (side == 1).sum() > 10 and (side == 0).sum() > 0
    for winding in (faces, faces[:, ::-1].copy()):
        n = claims(verts, winding, size)
        assert np.all(n[side == 1] == 1), 'a centre inside (shared edges and the shared vertex included) has no or several owners'
        assert np.all(n[side == -1] == 0), 'a centre outside is claimed'
        assert np.all(n[side == 0] <= 1)
        # all at once: the same pixels, and the owner is one of the triangles
        vis, counts = S.rasterize_numpy(verts, winding, *PIXEL_CAMERA, size)
        assert counts.tolist() == [len(faces), 0, 0, 0]
        assert np.array_equal(vis[0] != EMPTY, n == 1)
    # the shared vertex of the fan / the diagonal of the square are centres on shared edges
    if scene is fan_scene:
        assert claims(verts, faces, size)[8, 8] == 1


def test_culling_drops_exactly_one_winding():
    verts, faces, ring, size = fan_scene()
    both = np.concatenate([faces, faces[:, ::-1]])
    n_each = {}
    for cull in ('none', 'back', 'front'):
        for name, f in (('as given', faces), ('reversed', faces[:, ::-1].copy()), ('both', both)):
            vis, counts = S.rasterize_numpy(verts, f, *PIXEL_CAMERA, size, cull=cull)
            n_each[cull, name] = (int(counts[0]), int(counts[3]), int((vis != EMPTY).sum()))
            assert counts[1] == counts[2] == 0 and counts.sum() == len(f)
    covered = n_each['none', 'as given'][2]
    assert n_each['none', 'reversed'] == n_each['none', 'as given'] == (8, 0, covered)
    assert n_each['none', 'both'] == (16, 0, covered)
    # one winding is the back one, the other the front one
    assert {n_each['back', 'as given'], n_each['back', 'reversed']} == {(8, 0, covered), (0, 8, 0)}
    assert n_each['front', 'as given'] == n_each['back', 'reversed'] and n_each['front', 'reversed'] == n_each['back', 'as given']
    assert n_each['back', 'both'] == n_each['front', 'both'] == (8, 8, covered)
    # the ring of fan_scene runs clockwise on the screen (y down): its right-hand normal points away from the camera -- the back winding
    assert n_each['back', 'as given'] == (0, 8, 0)


def test_sub_pixel_triangles_cover_zero_or_exactly_one_centre():
    size = 8
    none = at_pixels([(3.6, 3.6), (3.9, 3.6), (3.6, 3.9)], size)                      # between centres
    one = at_pixels([(3.3, 3.3), (3.8, 3.4), (3.4, 3.8)], size)                       # around the centre (3.5, 3.5)
    f = np.array([[0, 1, 2]], dtype=np.int32)
    vis, counts = S.rasterize_numpy(none, f, *PIXEL_CAMERA, size)
    assert counts.tolist() == [1, 0, 0, 0] and np.all(vis == EMPTY)
    vis, counts = S.rasterize_numpy(one, f, *PIXEL_CAMERA, size)
    assert counts.tolist() == [1, 0, 0, 0] and (vis != EMPTY).sum() == 1 and vis[0, 3, 3] != EMPTY


def test_dropped_triangles_are_counted_and_leave_the_image_untouched():
    size = 8
    good = [(1.5, 1.5, 2.0), (6.5, 1.5, 2.0), (1.5, 6.5, 2.0)]
    verts = at_pixels(good + [(2.0, 2.0, 0.005),                       # 3: behind near
                              (9000.0, 2.0, 1.0),                      # 4: past the guard band (8192 pixels)
                              (6.5, 1.5, 2.0)], size)                  # 5: a copy of vertex 1
    verts = np.concatenate([verts, np.array([[np.nan, 0, 1], [0, 0, -1]], dtype=np.float32)])      # 6: non-finite, 7: behind the camera
    only_good = np.array([[0, 1, 2]], dtype=np.int32)
    want_vis, _ = S.rasterize_numpy(verts, only_good, *PIXEL_CAMERA, size, near=0.01)
    faces = np.array([[0, 1, 2], [0, 1, 3], [0, 4, 2], [0, 1, 5], [0, 1, 1], [6, 1, 2], [0, 7, 2], [3, 4, 2], [0, 1, 99], [0, -1, 2]], dtype=np.int32)
    vis, counts = S.rasterize_numpy(verts, faces, *PIXEL_CAMERA, size, near=0.01)
    # near: faces 1, 5, 6 and 7 (near comes before guard); guard: 2; culled: the two degenerate ones and the two naming no vertex
    assert counts.tolist() == [1, 4, 1, 4]
    assert np.array_equal(vis, want_vis)
    for k in range(1, len(faces)):
        alone, c = S.rasterize_numpy(verts, faces[k:k + 1], *PIXEL_CAMERA, size, near=0.01)
        assert np.all(alone == EMPTY) and c[0] == 0 and c.sum() == 1
    with pytest.raises(ValueError):
        S.rasterize_numpy(verts, faces, *PIXEL_CAMERA, size, near=0.0)
    with pytest.raises(ValueError):
        S.rasterize_numpy(verts, faces, *PIXEL_CAMERA, size, cull='sideways')
    with pytest.raises(ValueError):
        S.rasterize_numpy(verts, faces, *PIXEL_CAMERA, 5000)


def test_empty_mesh_is_background_and_coincident_triangles_go_to_the_lower_index():
    size = 8
    empty_v, empty_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    some_v = at_pixels([(1.5, 1.5), (6.5, 1.5), (1.5, 6.5)], size)
    for v, f in ((empty_v, empty_f), (some_v, empty_f), (empty_v, np.array([[0, 1, 2]], np.int32))):
        vis, counts = S.rasterize_numpy(v, f, *PIXEL_CAMERA, (size, size + 3))
        assert vis.shape == (1, size, size + 3) and np.all(vis == EMPTY) and counts.tolist() == [0, 0, 0, 0]
        out = S.resolve_numpy(vis, v, f, *PIXEL_CAMERA, shading=dict(background=(0.0, 0.5, 1.0)))
        assert np.all(out['tri_id'] == -1) and np.all(np.isposinf(out['depth'])) and np.all(out['normal'] == 0)
        assert np.all(out['frame'] == np.array([0, 128, 255], dtype=np.uint8))
    f = np.array([[0, 1, 2], [0, 1, 2], [1, 2, 0], [0, 2, 1]], dtype=np.int32)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        vis, _ = S.rasterize_numpy(some_v, f[order], *PIXEL_CAMERA, size)
        out = S.resolve_numpy(vis, some_v, f[order], *PIXEL_CAMERA, outputs=('tri_id', 'depth'))
        hit = out['tri_id'] >= 0
        assert hit.sum() > 5 and np.all(out['tri_id'][hit] == 0) and np.all(out['depth'][~hit] == np.inf)


# ---------------------------------------------------------------------------------------------------------------- the renderer's rays
def orbit_cameras(frames=(0, 40, 80)):
    labels = H.orbit_labels(frames, 120, 2.7)
    return labels[:, :16].reshape(-1, 4, 4), labels[:, 16:25].reshape(-1, 3, 3)


def pixel_rays_f64(cam2world, K, size, dx=0.0, dy=0.0):
    """float64 rays (origin [3], unit directions [size, size, 3]) through pixel positions (col + 0.5 + dx, row + 0.5 + dy)."""
    c2w, K = np.asarray(cam2world, dtype=np.float64), np.asarray(K, dtype=np.float64)
    col, row = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64))
    x, y = (col + 0.5 + dx) / size, (row + 0.5 + dy) / size
    fx, sk, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    xl = (x - cx + cy * sk / fy - sk * y / fy) / fx
    yl = (y - cy) / fy
    d = np.stack([xl, yl, np.ones_like(xl)], axis=-1) @ c2w[:3, :3].T
    return c2w[:3, 3], d / np.linalg.norm(d, axis=-1, keepdims=True)


def hit_f64(origin, dirs, tri):
    """Moeller-Trumbore in float64 for rays origin + t dirs [..., 3] against one triangle [3, 3] -> (t, u, v) (nan where parallel)."""
    e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
    p = np.cross(dirs, e2)
    det = p @ e1
    with np.errstate(all='ignore'):
        inv = 1.0 / det
        s = origin - tri[0]
        u = (p @ s) * inv
        q = np.cross(s, e1)
        v = (dirs @ q) * inv
        t = (e2 @ q) * inv
    return t, u, v


def edge_distance_px(cam2world, K, size, tri):
    """[size, size]: distance in pixels from every pixel centre to the nearest edge of the projected triangle (float64)."""
    w2c = np.linalg.inv(np.asarray(cam2world, dtype=np.float64))
    K = np.asarray(K, dtype=np.float64)
    p = tri @ w2c[:3, :3].T + w2c[:3, 3]
    xn, yn = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    s = np.stack([(K[0, 0] * xn + K[0, 1] * yn + K[0, 2]) * size, (K[1, 1] * yn + K[1, 2]) * size], axis=1)
    col, row = np.meshgrid(np.arange(size) + 0.5, np.arange(size) + 0.5)
    c = np.stack([col, row], axis=-1)
    best = np.full((size, size), np.inf)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        ab = s[b] - s[a]
        t = np.clip(((c - s[a]) @ ab) / (ab @ ab), 0, 1)
        best = np.minimum(best, np.linalg.norm(c - (s[a] + t[..., None] * ab), axis=-1))
    return best


def test_depth_is_the_distance_along_the_renderers_rays():
    from training.volumetric_rendering.ray_sampler import RaySampler
    size, n_tri = 48, 14
    rng = np.random.default_rng(3)
    verts = (rng.random((n_tri * 3, 3)) * 0.5 - 0.25).astype(np.float32)
    faces = np.arange(n_tri * 3, dtype=np.int32).reshape(-1, 3)
    cam2world, K = orbit_cameras()
    origins, dirs = RaySampler()(cam2world, K, size)
    out = S.render_mesh(verts, faces, cam2world.numpy(), K.numpy(), size, outputs=('tri_id', 'depth'))
    assert out['counts'].tolist() == [3 * n_tri, 0, 0, 0]
    v64 = verts.astype(np.float64)
    step = 1.0 / 128                                                                  # twice the snapping step
    covered = differ = 0
    for view in range(3):
        o = origins[view, 0].double().numpy()
        d = dirs[view].double().numpy().reshape(size, size, 3)
        tri_id, depth = out['tri_id'][view], out['depth'][view]
        own_o, own_d = pixel_rays_f64(cam2world[view], K[view], size)
        assert np.abs(own_d - d).max() < 1e-6                                         # the sampler's rays are the pixel centres' rays
        shifted = [pixel_rays_f64(cam2world[view], K[view], size, sx * step, sy * step)[1] for sx in (-1, 1) for sy in (-1, 1)]
        nearest, nearest_t = np.full((size, size), -1), np.full((size, size), np.inf)
        for k in range(n_tri):
            tri = v64[faces[k]]
            t, u, v = hit_f64(o, d, tri)
            inside = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < nearest_t)
            nearest[inside], nearest_t[inside] = k, t[inside]
            mine = tri_id == k
            if not mine.any():
                continue
            # the float64 hit of the pixel's ray with the winning triangle, allowing for the snap: barycentrics may be negative by what they
            # change across 1/128 pixel, and the distance may differ by what it changes across 1/128 pixel plus 4 float32 ulps
            t0, u0, v0 = hit_f64(own_o, own_d, tri)
            dt = du = dv = 0
            for sd in shifted:
                t1, u1, v1 = hit_f64(own_o, sd, tri)
                dt, du, dv = np.maximum(dt, np.abs(t1 - t0)), np.maximum(du, np.abs(u1 - u0)), np.maximum(dv, np.abs(v1 - v0))
            assert np.all(np.isfinite(t[mine])) and np.all(t[mine] > 0)
            assert np.all(u[mine] >= -du[mine]) and np.all(v[mine] >= -dv[mine]) and np.all((u + v)[mine] <= 1 + (du + dv)[mine])
            bound = dt + 4 * np.spacing(depth.astype(np.float32)).astype(np.float64)
            err = np.abs(depth.astype(np.float64) - t)
            print(f'view {view} triangle {k}: {mine.sum()} pixels, max depth error {err[mine].max():.3e}, smallest margin {(bound - err)[mine].min():.3e}')
            assert np.all(err[mine] <= bound[mine])
        hit = tri_id >= 0
        covered += int(hit.sum())
        other = nearest != tri_id
        differ += int(other.sum())
        for r, c in zip(*np.nonzero(other)):                                          # only centres within 1/128 pixel of an edge may differ
            near_edge = min(edge_distance_px(cam2world[view], K[view], size, v64[faces[k]])[r, c] for k in (nearest[r, c], tri_id[r, c]) if k >= 0)
            assert near_edge <= step, (view, r, c, near_edge)
        assert np.all(np.isposinf(depth[~hit]))
    print(f'{covered} covered pixels, {differ} assigned differently by the float64 cast')
    assert covered > 500 and differ <= 0.01 * covered


# ---------------------------------------------------------------------------------------------------------------- the sphere
SPHERE_N, SPHERE_R, SPHERE_SCALE = 48, 20.0, 1.0 / 80


def sphere_mesh():
    """(verts in index space, faces, radial unit normals, mesh2world 3x4): the sphere of radius 0.25 around the world's origin."""
    verts, faces = S.marching_cubes_numpy(sphere_field(SPHERE_N, SPHERE_R), 0.0)
    centre = (SPHERE_N - 1) / 2
    radial = verts.astype(np.float64) - centre
    normals = (radial / np.linalg.norm(radial, axis=1, keepdims=True)).astype(np.float32)
    mesh2world = np.concatenate([np.eye(3) * SPHERE_SCALE, np.full((3, 1), -centre * SPHERE_SCALE)], axis=1)
    return verts, faces, normals, mesh2world


@pytest.fixture(scope='module')
def sphere_render():
    verts, faces, normals, mesh2world = sphere_mesh()
    cam2world, K = orbit_cameras()
    out = S.render_mesh(verts, faces, cam2world.numpy(), K.numpy(), 96, mesh2world=mesh2world, normals=normals)
    return out, cam2world.numpy(), K.numpy()


def test_sphere_depth_and_normals_against_the_analytic_sphere(sphere_render):
    out, cam2world, K = sphere_render
    size, radius, voxel = 96, SPHERE_R * SPHERE_SCALE, SPHERE_SCALE
    assert out['counts'][0] == out['counts'].sum() > 0
    for view in range(3):
        o, d = pixel_rays_f64(cam2world[view], K[view], size)
        b = d @ o
        disc = b * b - (o @ o - radius * radius)
        with np.errstate(invalid='ignore'):
            t = -b - np.sqrt(disc)                                                    # nan where the ray misses
        hit = out['tri_id'][view] >= 0
        full = hit.copy()                                                             # the 3 x 3 neighbourhood is covered
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                full &= np.roll(np.roll(hit, dr, 0), dc, 1)
        full[[0, -1]] = False
        full[:, [0, -1]] = False
        assert full.sum() > 1000
        err = np.abs(out['depth'][view].astype(np.float64) - t)
        print(f'view {view}: {full.sum()} pixels, max depth error {err[full].max() / voxel:.4f} voxel edges')
        assert np.all(err[full] <= np.sqrt(3) * voxel)
        # normals: the analytic one is the radial direction at the hit, in the camera frame; spread = the largest angle to a neighbour's
        n_world = (o + t[..., None] * d) / radius
        n_cam = n_world @ cam2world[view][:3, :3]                                     # R^T n
        got = out['normal'][view].astype(np.float64)
        assert np.allclose(np.linalg.norm(got[hit], axis=-1), 1, atol=1e-6) and np.all(got[~hit] == 0)
        assert np.all((got * np.stack([np.zeros_like(t), np.zeros_like(t), np.ones_like(t)], -1)).sum(-1)[full] < 0)      # facing the camera
        cos_spread = np.ones((size, size))
        with np.errstate(invalid='ignore'):
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    cos_spread = np.fmin(cos_spread, (n_cam * np.roll(np.roll(n_cam, dr, 0), dc, 1)).sum(-1))
        cos_got = (got * n_cam).sum(-1)
        angle, spread = np.arccos(np.clip(cos_got[full], -1, 1)), np.arccos(np.clip(cos_spread[full], -1, 1))
        print(f'view {view}: largest normal error {np.degrees(angle.max()):.3f} deg, smallest spread {np.degrees(spread.min()):.3f} deg')
        assert np.all(angle <= spread)
        assert len(np.unique(out['frame'][view][hit])) > 20 and np.all(out['frame'][view][~hit] == 255)


def test_face_normals_and_colours_shade_the_sphere(sphere_render):
    verts, faces, normals, mesh2world = sphere_mesh()
    out, cam2world, K = sphere_render
    rng = np.random.default_rng(0)
    colors = rng.integers(0, 256, (len(verts), 3), dtype=np.uint8)
    flat = S.render_mesh(verts, faces, cam2world[:1], K[:1], 96, mesh2world=mesh2world, colors=colors, shading=dict(ambient=1.0, diffuse=0.0))
    assert np.array_equal(flat['tri_id'][0], out['tri_id'][0]) and np.array_equal(flat['depth'][0], out['depth'][0])
    hit = flat['tri_id'][0] >= 0
    inner = hit & (out['normal'][0][..., 2] < -0.3)                                  # away from the silhouette, where "facing the camera" is moot
    cos = (flat['normal'][0][inner].astype(np.float64) * out['normal'][0][inner]).sum(-1)
    assert inner.sum() > 3000 and cos.min() > np.cos(np.radians(12))                  # face normals of a 48^3 sphere: within a facet's tilt
    # unlit colours: a convex mix of the three vertex colours
    tri = faces[flat['tri_id'][0][hit]]
    c = colors[tri].astype(np.int64)
    got = flat['frame'][0][hit].astype(np.int64)
    assert np.all(got >= c.min(axis=1) - 1) and np.all(got <= c.max(axis=1) + 1)


# ---------------------------------------------------------------------------------------------------------------- interface
def test_raster_declarations():
    import gnerf_hip
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    assert int(re.search(r'#define GNERF_ABI_VERSION (\d+)', header).group(1)) == gnerf_hip.ABI_VERSION == 15
    assert int(re.search(r'#define GNERF_RASTER_SMALL_PIXELS (\d+)', header).group(1)) == gnerf_hip.RASTER_SMALL_PIXELS == S.RASTER_SMALL_PIXELS
    assert int(re.search(r'#define GNERF_RASTER_MAX_SIZE (\d+)', header).group(1)) == gnerf_hip.RASTER_MAX_SIZE
    for mode, code in gnerf_hip.RASTER_CULL.items():
        assert int(re.search(r'#define GNERF_RASTER_CULL_%s (\d+)' % mode.upper(), header).group(1)) == code == S.RASTER_CULL[mode]
    assert gnerf_hip.RASTER_SHADING == S.RASTER_SHADING
    assert 'no near-plane clipping' in header.lower()
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    want = {'gnerf_raster_workspace_bytes': (i, [i, i, i, i, i, ctypes.POINTER(ctypes.c_size_t)]),
            'gnerf_raster_visibility': (i, [p, i, p, i, p, p, i, i, i, f, i, p, p, p, p]),
            'gnerf_raster_resolve': (i, [p, p, i, p, i, p, p, i, i, i, p, p, p, ctypes.POINTER(f), p, p, p, p, p])}
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    binding = open(os.path.join(ROOT, 'g-nerf_amd', 'csrc', 'torch_binding.cpp')).read()
    for name, sig in want.items():
        assert gnerf_hip.SIGNATURES[name] == sig
        assert name in gnerf_hip.OPTIONAL_SYMBOLS                   # a library of the same version built before them still loads
        args = re.search(name + r'\s*\((.*?)\)\s*;', header, flags=re.S).group(1)
        assert len(args.split(',')) == len(sig[1]), name
        assert hasattr(gnerf_hip.load(), name)
        assert name + '(' in binding
    assert gnerf_hip.raster_available()
    for name in ('rasterize', 'resolve', 'raster_available', 'raster_workspace_bytes'):
        assert callable(getattr(gnerf_hip, name))
    assert re.search(r'm\.def\("raster_visibility"', binding) and re.search(r'm\.def\("raster_resolve"', binding)
    csrc = os.path.join(ROOT, 'g-nerf_amd', 'csrc')             # build.sh builds the units that compile_unit.sh lists
    assert re.search(r'^for src in \$UNITS;', open(os.path.join(csrc, 'build.sh')).read(), flags=re.M)
    assert re.search(r'^UNITS="[^"]*\braster\b', open(os.path.join(csrc, 'compile_unit.sh')).read(), flags=re.M)


def test_c_entry_points_refuse_without_a_gpu():
    import gnerf_hip
    lib = gnerf_hip.load()
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)
    n = ctypes.c_size_t()
    assert lib.gnerf_raster_workspace_bytes(10, 20, 3, 64, 64, ctypes.byref(n)) == 0 and n.value >= 4 * 60
    assert gnerf_hip.raster_workspace_bytes(10, 20, 3, 64) == n.value
    assert lib.gnerf_raster_workspace_bytes(0, 0, 1, 8, 8, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.gnerf_raster_workspace_bytes(10, 20, 3, 64, 64, None) == -1 and b'null' in lib.gnerf_last_error()
    assert lib.gnerf_raster_workspace_bytes(10, 20, 0, 64, 64, ctypes.byref(n)) == -1 and b'n_views' in lib.gnerf_last_error()
    assert lib.gnerf_raster_workspace_bytes(10, 20, 1, 4097, 64, ctypes.byref(n)) == -1 and b'size' in lib.gnerf_last_error()
    assert lib.gnerf_raster_workspace_bytes(10, 1 << 30, 2, 64, 64, ctypes.byref(n)) == -1 and b'2^31' in lib.gnerf_last_error()
    assert lib.gnerf_raster_workspace_bytes(10, 20, 200, 4096, 4096, ctypes.byref(n)) == -1 and b'2^31' in lib.gnerf_last_error()

    def vis(near=0.01, cull=0, verts=ptr, ws=ptr, views=1):
        return lib.gnerf_raster_visibility(verts, 3, ptr, 1, ptr, ptr, views, 8, 8, near, cull, ws, ptr, ptr, None)
    assert vis(ws=None) == -1 and b'null' in lib.gnerf_last_error()
    assert vis(verts=None) == -1 and b'null' in lib.gnerf_last_error()
    assert vis(near=0.0) == -1 and b'near' in lib.gnerf_last_error()
    assert vis(cull=3) == -1 and b'cull' in lib.gnerf_last_error()
    assert vis(views=0) == -1 and b'n_views' in lib.gnerf_last_error()
    sh = (ctypes.c_float * 11)()

    def res(vis_p=ptr, normals=None, nmat=None, shading=sh, outs=(ptr, ptr, ptr, ptr)):
        return lib.gnerf_raster_resolve(vis_p, ptr, 3, ptr, 1, ptr, ptr, 1, 8, 8, normals, nmat, None, shading, *outs, None)
    assert res(vis_p=None) == -1 and b'null' in lib.gnerf_last_error()
    assert res(outs=(None, None, None, None)) == -1 and b'output' in lib.gnerf_last_error()
    assert res(normals=ptr) == -1 and b'normal_mat' in lib.gnerf_last_error()
    assert res(shading=None) == -1 and b'shading' in lib.gnerf_last_error()
    # CPU tensors never reach the library
    with pytest.raises(RuntimeError):
        gnerf_hip.rasterize(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, 12), torch.zeros(1, 9), 8)


def test_mesh_to_world_matrix_is_the_lattice_map():
    import gen_videos_mi355x as gv
    rng = np.random.default_rng(5)
    for n, cube in ((64, 1.0), (512, 1.0), (37, 2.5)):
        M = gv.mesh_to_world_matrix(n, cube)
        assert M.shape == (3, 4) and M.dtype == np.float64 and np.array_equal(M[:, :3], gv.mesh_to_world_jacobian(n, cube))
        v = rng.random((100, 3)) * (n - 1)
        want = gv.lattice_to_world(gv.mesh_to_lattice(v, n), n, cube)
        assert np.abs(v @ M[:, :3].T + M[:, 3] - want).max() <= 1e-12 * cube * 4


def test_mesh_to_camera_rounds_once_and_carries_normals_as_covectors():
    cam2world, _ = orbit_cameras()
    M = np.array([[0.5, 0.1, 0, 0.2], [0, 2.0, 0.3, -0.1], [0.2, 0, 1.5, 0.05]])
    A, N = S.mesh_to_camera(cam2world.numpy(), M)
    assert A.shape == (3, 3, 4) and N.shape == (3, 3, 3) and A.dtype == N.dtype == np.float32
    full = np.linalg.inv(cam2world.double().numpy()) @ np.concatenate([M, [[0, 0, 0, 1]]])
    assert np.array_equal(A, full[:, :3].astype(np.float32))
    # a plane n . x = d of the mesh frame stays a plane under the map: (N n) . (A x) is constant on it
    rng = np.random.default_rng(1)
    n = rng.standard_normal(3)
    x = rng.standard_normal((50, 3))
    x -= ((x @ n - 1.0) / (n @ n))[:, None] * n
    for k in range(3):
        y = x @ full[k, :3, :3].T + full[k, :3, 3]
        assert np.ptp(y @ (N[k].astype(np.float64) @ n)) < 1e-5


def test_geometry_orbit_on_the_cpu_equals_render_mesh():
    """render_geometry_orbit's host logic (cameras, sharding, frames per call) on the numpy port: a sphere in a 48^3 'volume'."""
    import gen_videos_mi355x as gv
    verts, faces = S.marching_cubes_numpy(sphere_field(48, 14.0), 0.0)
    tv, tf = torch.from_numpy(verts), torch.from_numpy(faces)
    full, _ = gv.render_geometry_orbit(tv, tf, 5, 24, 48, 1.0, 2.7, frames_per_call=2)
    assert full.shape == (5, 24, 24, 3) and full.dtype == torch.uint8 and len(torch.unique(full)) > 10
    parts = [gv.render_geometry_orbit(tv, tf, 5, 24, 48, 1.0, 2.7, rank=r, world=3, frames_per_call=1)[0] for r in range(3)]
    assert torch.equal(torch.cat(parts), full)
    labels = H.orbit_labels(range(5), 5, 2.7)
    want = S.render_mesh(verts, faces, labels[:, :16].reshape(-1, 4, 4).numpy(), labels[:, 16:].reshape(-1, 3, 3).numpy(), 24,
                         mesh2world=gv.mesh_to_world_matrix(48, 1.0), outputs=('frame',))
    assert np.array_equal(full.numpy(), want['frame'])
    assert gv.render_geometry_orbit(tv, tf, 2, 24, 48, 1.0, 2.7, rank=2, world=3)[0] is None
