// Ray gradient of the fused renderer: dL/d(ray origins) and dL/d(ray directions) from the staged backward's per-ray blocks.  Included by
// render_backward.hip alone (it holds a kernel); the derivative taps (plane_taps_grad.inl) are shared with the point queries, whose
// plane_position_grad states the rule of the per-plane block below (this kernel keeps its own text of it: see there).
//
// With numeric ray limits the coarse depths do not depend on the rays, the importance depths are constants (renderer.py:198-211) and the
// decoder ignores directions, so the rays reach the outputs only through the sample positions p_k = o + t_k d:
//     dL/do = sum_k dL/dp_k        dL/dd = sum_k t_k dL/dp_k        dL/dp_k = J_k^T dX_k
// dX_k = dL/d(mean feature) of sample k, J_k the derivative of the three bilinear lookups by position (grid_sample's coordinate gradient:
// zero padding, floor's one-sided derivative, the mean's 1/3 -- include/gnerf_hip.h states it at gnerf_query_points_grad).
//
// The first pass of the staged backward (render_bwd_tiles_kernel, or render_bwd_kernel<true>) leaves, per ray, n_all depths in depth
// order followed by n_all rows of 32 floats of dX (render_bwd.inl, "staged scatter").  This kernel joins the two:
//   * a wave owns whole rays (ray = wave index, grid stride); the blocks are indexed by ray, so the padding of ragged calls does not exist here;
//   * it walks the ray's samples 8 at a time: sample slot = lane >> 3, and the slot's 8 lanes hold 16 bytes each of a texel and of the
//     sample's dX row (128 bytes both: the lookup's lane mapping).  Every lane of a slot makes the slot's tap records itself, in registers;
//   * each lane keeps its share of sum dp and sum t dp across the steps (the sums are linear, so nothing is reduced per sample); a sample
//     slot past n_all adds zeros;
//   * one butterfly over the 64 lanes per ray at the end, six plain stores.
// No atomics, no LDS, and an order of additions fixed by n_all alone: the same bits on every run.
#pragma once
#include "render_bwd_tile.inl"
#include "plane_taps_grad.inl"

namespace {

struct RayGradArgs {
    const float* planes; const float* origins; const float* dirs;
    const float* stage;                     // per ray: n_all depths, then n_all rows of 32 floats
    float* grad_origins; float* grad_dirs;  // [total_rays, 3] each; either may be NULL
    int64_t plane_floats;                   // floats from one item's planes to the next
    int H, W, n_all, rays_per_item, total_rays;
    unsigned tex_pitch, row_pitch, plane_pitch;
    float box_scale;
};

typedef float v4f_dw __attribute__((ext_vector_type(4), aligned(4)));       // a dX row starts on a dword, not on 16 bytes (n_all is arbitrary)

constexpr int kRayGradThreads = 256, kRayGradWaves = kRayGradThreads / 64;

__global__ __launch_bounds__(kRayGradThreads) void render_ray_grad_kernel(RayGradArgs A) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int slot = lane >> 3, cq = lane & 7, cq16 = cq * 16;
    const int n_all = A.n_all;
    const int64_t waves = int64_t(gridDim.x) * kRayGradWaves;
    for (int64_t ray = int64_t(blockIdx.x) * kRayGradWaves + wv; ray < A.total_rays; ray += waves) {
        const int item = int(ray / A.rays_per_item);
        const char* planes = reinterpret_cast<const char*>(A.planes + int64_t(item) * A.plane_floats);
        const float ox = A.origins[ray * 3 + 0], oy = A.origins[ray * 3 + 1], oz = A.origins[ray * 3 + 2];
        const float dx = A.dirs[ray * 3 + 0], dy = A.dirs[ray * 3 + 1], dz = A.dirs[ray * 3 + 2];
        const float* block = A.stage + ray * (int64_t(n_all) * 33);
        const float* rows = block + n_all;
        float sx = 0.f, sy = 0.f, sz = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
        for (int k0 = 0; k0 < n_all; k0 += 8) {
            const bool live = k0 + slot < n_all;
            const int k = min(k0 + slot, n_all - 1);                       // a slot past the end reads the last sample and adds nothing
            const float t = block[k];
            const v4f dxv = *reinterpret_cast<const v4f_dw*>(rows + int64_t(k) * 32 + 4 * cq);
            const float px = __fadd_rn(ox, __fmul_rn(t, dx)) * A.box_scale;       // the forward's position arithmetic (DepthListPos)
            const float py = __fadd_rn(oy, __fmul_rn(t, dy)) * A.box_scale;
            const float pz = __fadd_rn(oz, __fmul_rn(t, dz)) * A.box_scale;
            float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
            for (int pl = 0; pl < 3; pl++) {
                const float u = pl == 2 ? pz : px;
                const float v = pl == 0 ? py : (pl == 1 ? pz : px);
                uint4 off; v4f wgt, du, dv;
                plane_taps_grad(A.H, A.W, u, v, A.tex_pitch, A.row_pitch, unsigned(pl) * A.plane_pitch, off, wgt, du, dv);
                // plane_position_grad (plane_taps_grad.inl), kept as a copy: through the helper this kernel measured 1 % slower
                const v4f t00 = *reinterpret_cast<const v4f*>(planes + off.x + cq16);
                const v4f t10 = *reinterpret_cast<const v4f*>(planes + off.y + cq16);
                const v4f t01 = *reinterpret_cast<const v4f*>(planes + off.z + cq16);
                const v4f t11 = *reinterpret_cast<const v4f*>(planes + off.w + cq16);
                const v4f fu = (t00 * du[0] + t10 * du[1] + t01 * du[2] + t11 * du[3]) * dxv;
                const v4f fv = (t00 * dv[0] + t10 * dv[1] + t01 * dv[2] + t11 * dv[3]) * dxv;
                const float su = (fu[0] + fu[1]) + (fu[2] + fu[3]), sv = (fv[0] + fv[1]) + (fv[2] + fv[3]);
                if (pl == 0) { gx += su; gy += sv; }                       // planes read (x,y), (x,z), (z,x)
                else if (pl == 1) { gx += su; gz += sv; }
                else { gz += su; gx += sv; }
            }
            if (live) {
                sx += gx; sy += gy; sz += gz;
                tx = fmaf(t, gx, tx); ty = fmaf(t, gy, ty); tz = fmaf(t, gz, tz);
            }
        }
        // ---- the ray's six sums over the 64 lanes (8 channel quads x 8 sample slots): every lane ends with the totals
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            sx += __shfl_xor(sx, m); sy += __shfl_xor(sy, m); sz += __shfl_xor(sz, m);
            tx += __shfl_xor(tx, m); ty += __shfl_xor(ty, m); tz += __shfl_xor(tz, m);
        }
        if (lane < 3) {
            if (A.grad_origins) A.grad_origins[ray * 3 + lane] = (lane == 0 ? sx : (lane == 1 ? sy : sz)) * A.box_scale;
            if (A.grad_dirs) A.grad_dirs[ray * 3 + lane] = (lane == 0 ? tx : (lane == 1 ? ty : tz)) * A.box_scale;
        }
    }
}

}  // namespace
