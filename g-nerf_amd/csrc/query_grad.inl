// Position gradient of run_model (renderer.py:142-148): dL/dpoints from dL/dsigma and / or dL/drgb.  Included by render_query.hip
// alone (it holds a kernel); it shares the decoder staging, MLP forward and MFMA conventions of render_bwd_tile.inl (D layout col = lane & 15, rows = 4 * (lane >> 4) + r).
//
// Upstream this is autograd through grid_sample's coordinate gradient (zero padding, align_corners=False) and the decoder.  Here a wave
// takes 16-point tiles through
//   1. the tap records of the tile (lanes 0..47: point = lane & 15, plane = lane >> 4): byte offsets, the blend weights, and the
//      weights of the blend's two derivatives d/du and d/dv (the pixel scale W/2, H/2 and the plane mean's 1/3 folded in);
//   2. the lookup (8 lanes x 16 B per texel) and the decoder forward of query_bwd_kernel;
//   3. the decoder backward to dX[16][32] = dL/d(mean feature) -- no weight gradients, and without the colour half when there is no
//      dL/drgb (normals) -- on exact fp32 matrix products;
//   4. a second lookup of the same texels against the derivative weights: per plane gu = sum_c dX[c] df_c/du, gv likewise, the 32-channel
//      dots reduced inside the 8-lane group, and
//        dL/dpoint = (2 / box_warp) * (gu_0 + gu_1 + gv_2,  gv_0,  gv_1 + gu_2)            planes read (x,y), (x,z), (z,x).
// Every point owns its three outputs: plain stores, no atomics, the same bits on every run.
//
// The four stages are functions of this file (grad_tap_records, grad_lookup, grad_dx_from_dh, grad_point_gradient), the one copy that
// project_level.inl's Newton loop runs too; the decoder staging, the colour slope and the colour half of dH are render_bwd_tile.inl's, the
// taps and the plane routing plane_taps_grad.inl's.  A kernel owns its tile loop, where the positions come from, what seeds dH, where the
// three components go, and every lds_wave_sync.

#pragma once
#include "render_bwd_tile.inl"
#include "plane_taps_grad.inl"

namespace {

constexpr int kGradRecDwords = 16;      // per (point, plane): 4 byte offsets, 4 blend weights, 4 d/du weights, 4 d/dv weights
__host__ __device__ inline size_t query_grad_wave_floats() { return 16 * kStagePitch + 16 * kTPitch + 16 * 3 * kGradRecDwords; }

struct QueryGradArgs {
    const float* points; const float* grad_sigma; const float* grad_rgb;      // either gradient may be NULL
    float* grad_points;
    int n_points, tiles_per_item, n_tiles;
};

// sum over the 8 lanes that share a point (lanes 8b .. 8b+7); every lane gets the total
__device__ __forceinline__ float group8_total(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
}

// ---- The four stages of a 16-point tile, shared by query_grad_kernel and project_level_kernel (project_level.inl).  No helper holds an
// lds_wave_sync: the kernels place them, between the stages.

// 1. the tap records of the tile (lanes 0..47: point j = lane & 15, plane = lane >> 4); (qx, qy, qz) = point j in the planes' [-1, 1] frame
__device__ __forceinline__ void grad_tap_records(const Params& P, float* recs, int lane, float qx, float qy, float qz) {
    if (lane < 48) {
        const int j = lane & 15, pl = lane >> 4;
        const float u = pl == 2 ? qz : qx;
        const float v = pl == 0 ? qy : (pl == 1 ? qz : qx);
        uint4 off; v4f wgt, du, dv;
        plane_taps_grad(P.p.plane_h, P.p.plane_w, u, v, P.tex_pitch, P.row_pitch, unsigned(pl) * P.plane_pitch, off, wgt, du, dv);
        float* rec = recs + (j * 3 + pl) * kGradRecDwords;
        *reinterpret_cast<uint4*>(rec) = off;
        *reinterpret_cast<v4f*>(rec + 4) = wgt;
        *reinterpret_cast<v4f*>(rec + 8) = du;
        *reinterpret_cast<v4f*>(rec + 12) = dv;
    }
}

// 2. lookup: 8 points per step (point 8a + b, b = lane >> 3), 8 lanes x 16 bytes per texel (cq = lane & 7); mean features staged as X[point][channel]
__device__ __forceinline__ void grad_lookup(const BwdLds& L, const float* recs, const char* planes, int b, int cq) {
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const int js = 8 * a + b;
        v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pl = 0; pl < 3; pl++) {
            const float* rec = recs + (js * 3 + pl) * kGradRecDwords;
            const uint4 off = *reinterpret_cast<const uint4*>(rec);
            const v4f wgt = *reinterpret_cast<const v4f*>(rec + 4);
            const v4f t00 = *reinterpret_cast<const v4f*>(planes + off.x + cq * 16);
            const v4f t10 = *reinterpret_cast<const v4f*>(planes + off.y + cq * 16);
            const v4f t01 = *reinterpret_cast<const v4f*>(planes + off.z + cq * 16);
            const v4f t11 = *reinterpret_cast<const v4f*>(planes + off.w + cq * 16);
            acc += t00 * wgt[0] + t10 * wgt[1] + t01 * wgt[2] + t11 * wgt[3];
        }
        *reinterpret_cast<v4f*>(L.stage + js * kStagePitch + 4 * cq) = acc;
    }
}

// 3, second half. dH^T -> through softplus -> dX^T (bwd_tile_core without the weight gradients); h = the hidden activations of bwd_mlp_forward
__device__ __forceinline__ void grad_dx_from_dh(const BwdLds& L, const v4f (&h)[4], const v4f (&dh)[4], int j, int g, v4f (&dx)[2]) {
    dx[0] = dx[1] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < 4; m++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float dpre = dh[m][r] * (1.f - exp_hw(-h[m][r]));          // d/dpre softplus(pre) = 1 - exp(-softplus(pre))
            const float* row = L.w1 + (16 * m + 4 * g + r) * kW1Pitch + j;
            dx[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[0], dpre, dx[0], 0, 0, 0);
            dx[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[16], dpre, dx[1], 0, 0, 0);
        }
    }
}

// 4. the texels of point js against the derivative weights and dX[point][channel] (in L.tbuf): the 32-channel dots reduced inside the
// point's 8-lane group, every lane of which gets dL/d(position in the [-1, 1] frame)
__device__ __forceinline__ void grad_point_gradient(const BwdLds& L, const float* recs, const char* planes, int js, int cq, float& gx, float& gy, float& gz) {
    const v4f dxv = *reinterpret_cast<const v4f*>(L.tbuf + js * kTPitch + 4 * cq);
    gx = gy = gz = 0.f;
#pragma unroll
    for (int pl = 0; pl < 3; pl++) {
        const float* rec = recs + (js * 3 + pl) * kGradRecDwords;
        const uint4 off = *reinterpret_cast<const uint4*>(rec);
        const v4f du = *reinterpret_cast<const v4f*>(rec + 8);
        const v4f dv = *reinterpret_cast<const v4f*>(rec + 12);
        plane_position_grad(planes, pl, off, du, dv, dxv, cq * 16, gx, gy, gz);
    }
    gx = group8_total(gx); gy = group8_total(gy); gz = group8_total(gz);
}

// RGB: a colour gradient is given.  Without it the colour half of layer 2 is evaluated in neither direction.
template <bool RGB>
__global__ __launch_bounds__(kBwdThreads, 3) void query_grad_kernel(Params P, QueryGradArgs Q) {
    extern __shared__ __align__(16) float smem[];
    const gnerf_render_params& p = P.p;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    BwdLds L = {};
    bwd_stage_decoder_f32<kBwdThreads>(L, smem, p, tid);
    L.stage = smem + kBwdWeightFloats + size_t(wv) * query_grad_wave_floats();
    L.tbuf = L.stage + 16 * kStagePitch;
    float* recs = L.tbuf + 16 * kTPitch;
    const int j = lane & 15, g = lane >> 4, b = lane >> 3, cq = lane & 7;
    const int64_t plane_floats = int64_t(3) * p.plane_h * p.plane_w * 32;
    for (int tile = blockIdx.x * kBwdWaves + wv; tile < Q.n_tiles; tile += gridDim.x * kBwdWaves) {
        const int item = tile / Q.tiles_per_item, t = tile % Q.tiles_per_item;
        const char* planes = reinterpret_cast<const char*>(p.planes_nhwc + int64_t(item) * plane_floats);
        const float* pts = Q.points + int64_t(item) * Q.n_points * 3;
        const int64_t pt0 = int64_t(item) * Q.n_points + 16 * t;
        // ---- 1. tap records (points past the end of a partial last tile repeat the last point; they are never written)
        const int64_t idx = min(16 * t + j, Q.n_points - 1);
        grad_tap_records(P, recs, lane, pts[idx * 3 + 0] * P.box_scale, pts[idx * 3 + 1] * P.box_scale, pts[idx * 3 + 2] * P.box_scale);
        lds_wave_sync();
        // ---- 2. lookup and decoder forward
        grad_lookup(L, recs, planes, b, cq);
        lds_wave_sync();
        v4f h[4], o[2];
        float sig;
        bwd_mlp_forward(L, lane, h, o, sig);
        // ---- 3. decoder backward: dO -> dH^T -> dX^T
        const float dsig = (Q.grad_sigma && 16 * t + j < Q.n_points) ? Q.grad_sigma[pt0 + j] : 0.f;
        v4f dh[4];
#pragma unroll
        for (int m = 0; m < 4; m++) dh[m] = *reinterpret_cast<const v4f*>(L.w2 + 16 * m + 4 * g) * dsig;
        if constexpr (RGB) {
#pragma unroll
            for (int n = 0; n < 2; n++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int q = 4 * g + r;
                    const float gc = 16 * t + q < Q.n_points ? Q.grad_rgb[(pt0 + q) * 32 + 16 * n + j] : 0.f;
                    L.tbuf[q * kTPitch + 16 * n + j] = gc * rgb_slope_hw(o[n][r]);
                }
            }
            lds_wave_sync();
            bwd_dh_add_colour(L, j, g, dh);
        }
        v4f dx[2];
        grad_dx_from_dh(L, h, dh, j, g, dx);
        lds_wave_sync();                                                         // every lane has read dO
        *reinterpret_cast<v4f*>(L.tbuf + j * kTPitch + 4 * g) = dx[0];           // dX[point][channel]
        *reinterpret_cast<v4f*>(L.tbuf + j * kTPitch + 16 + 4 * g) = dx[1];
        lds_wave_sync();
        // ---- 4. the same texels against the derivative weights
#pragma unroll
        for (int a = 0; a < 2; a++) {
            const int js = 8 * a + b;
            float gx, gy, gz;
            grad_point_gradient(L, recs, planes, js, cq, gx, gy, gz);
            if (cq < 3 && 16 * t + js < Q.n_points)
                Q.grad_points[(pt0 + js) * 3 + cq] = (cq == 0 ? gx : (cq == 1 ? gy : gz)) * P.box_scale;
        }
        lds_wave_sync();                                                         // the records and dX are the next tile's to overwrite
    }
}

}  // namespace
