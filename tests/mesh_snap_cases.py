"""What tests/test_mesh_snap_cpu.py and tests/test_mesh_snap_gpu.py share: the oracle case of the level-set projection (the planes and decoder
of seed 9 that tests/test_point_grad_gpu.py's case draws first, a 24^3 lattice spanning +-0.45 of a box of box_warp 1, the marching-cubes mesh
of its float32 volume at the median density), the float64 field with its autograd gradient, the float64 port's result -- each made once per
process on the CPU -- and a hand-made fan for the flip guard."""

import functools

import numpy as np
import torch

N_LATTICE = 24
SPAN = 0.45
STEPS, RADIUS, TOL = 6, 1.0, 2.0 ** -12


def lattice_affine(scale=1.0):
    """world = v * 0.9 / 23 - 0.45 as a 3x4 [A | b] (float64 numpy); scale multiplies the world."""
    a = np.zeros((3, 4))
    a[:, :3] = np.eye(3) * (2 * SPAN / (N_LATTICE - 1))
    a[:, 3] = -SPAN
    return a * scale


@functools.lru_cache(maxsize=None)
def oracle_case():
    from oracle import render_ref as R
    import shape_mi355x as S
    gen = torch.Generator().manual_seed(9)
    planes = torch.randn(2, 3, 32, 24, 20, generator=gen) * 1.5
    dec = R.fold_decoder(torch.randn(64, 32, generator=gen), torch.randn(64, generator=gen) * 0.2,
                         torch.randn(33, 64, generator=gen), torch.randn(33, generator=gen) * 0.2)
    planes64, dec64 = planes.double(), [t.double() for t in dec]

    def sigma64(world, item=0, box_warp=1.0):
        """float64 densities [P] of world points [P, 3] (any dtype) on one item's planes."""
        with torch.no_grad():
            return R.query_points(planes64[item:item + 1], dec64, world.double().reshape(1, -1, 3), box_warp)[0][0, :, 0]

    def field64(world, item=0, box_warp=1.0):
        """(sigma [P], grad sigma [P, 3]) in float64: the oracle's lookup and decoder with autograd.  The decoder's two products are written
        as broadcast multiplies and row sums instead of R.decoder_mlp's matmuls: a BLAS picks its summation order by the batch size, and a
        point's bits must not depend on its batch (test_port_field_is_the_oracle holds this form to R.query_points)."""
        W1, b1, W2, b2 = dec64
        with torch.enable_grad():
            p = world.detach().double().reshape(-1, 3).requires_grad_(True)
            x = R.triplane_features(planes64[item], p, box_warp)
            h = torch.nn.functional.softplus((x[:, None, :] * W1[None]).sum(-1) + b1)
            sig = (h * W2[0]).sum(-1) + b2[0]
            grad, = torch.autograd.grad(sig.sum(), p)
        return sig.detach(), grad

    n = N_LATTICE
    idx = torch.arange(n, dtype=torch.float64)
    lattice = torch.stack(torch.meshgrid(idx, idx, idx, indexing='ij'), dim=-1).reshape(-1, 3)
    A = torch.from_numpy(lattice_affine())
    vol64 = sigma64(lattice @ A[:, :3].t() + A[:, 3]).reshape(n, n, n)
    level = float(vol64.median().float())                    # an exact float32: the kernel and the port see the same level
    verts, faces = S.marching_cubes_numpy(vol64.float().numpy(), level)
    return dict(planes=planes, dec=dec, sigma64=sigma64, field64=field64, level=level, verts=verts, faces=faces, affine=lattice_affine())


@functools.lru_cache(maxsize=None)
def port_result():
    """The float64 port on every vertex of the oracle mesh: (points_out float64 [V, 3], status uint8 [V], residual_in, residual_out)."""
    from training.volumetric_rendering.renderer import project_to_level_rules
    c = oracle_case()
    return project_to_level_rules(c['field64'], torch.from_numpy(c['verts']).double(), c['level'], steps=STEPS, radius=RADIUS, tol=TOL, affine=c['affine'])


def fan():
    """A fan of four faces around vertex 0 in the plane z = 0, one face of zero area and one face with an id out of range; moving vertex 1
    across the hub to (-1, -0.5) turns the two faces that hold it over (0 4 1 and 0 1 2) and leaves 0 2 3 and 0 3 4 alone.
    -> (verts_in, verts_moved, faces, the vertices of the two flipped faces)."""
    verts = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [-2, 0, 0], [0, -2, 0], [5, 5, 0], [6, 6, 0], [7, 7, 0]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [5, 6, 7], [0, 1, 99]], dtype=np.int32)
    moved = verts.copy()
    moved[1] = [-1, -0.5, 0]
    moved[5] = [5, 6, 0]                      # the zero-area face gets an area: never a flip
    moved[3] = [-2, 0.25, 0]                  # moves, turns nothing over, stays
    return verts, moved, faces, [0, 1, 2, 4]
