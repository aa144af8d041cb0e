// gnerf_query_points_backward's kernel.  Included by render_query.hip alone (it holds a kernel).
#pragma once
#include "render_bwd_tile.inl"

namespace {

// Backward of run_model for arbitrary points (renderer.py:142-148; TriPlaneGenerator.sample_mixed, which the density
// regulariser of training differentiates): the gradient arrives per point -- dL/dsigma [n_items, n_points, 1] and
// dL/drgb [n_items, n_points, 32] -- so there is no composite to undo; each wave takes 16-point tiles through the same
// lookup + MLP forward + decoder backward + deferred plane scatter as the renderer's backward.
struct QueryBwdArgs {
    const float* points; const float* grad_sigma; const float* grad_rgb;      // any of the two gradients may be NULL
    int n_points, tiles_per_item, n_tiles;
    float* grad_planes_nhwc; float* grad_w1; float* grad_b1; float* grad_w2; float* grad_b2;
};

struct PointTilePos {
    const float* pts; int n_points, tile; float box_scale;
    __device__ __forceinline__ void operator()(int j, float& px, float& py, float& pz) const {
        const int idx = min(16 * tile + j, n_points - 1);
        px = pts[idx * 3 + 0] * box_scale; py = pts[idx * 3 + 1] * box_scale; pz = pts[idx * 3 + 2] * box_scale;
    }
};

__global__ __launch_bounds__(kBwdThreads, 2) void query_bwd_kernel(Params P, QueryBwdArgs Q) {
    extern __shared__ __align__(16) float smem[];
    const gnerf_render_params& p = P.p;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // ---- decoder into LDS: bwd_stage_decoder_f32 (render_bwd_tile.inl), kept as a copy -- through the helper this kernel's instructions change
    float* w1 = smem;
    float* w2 = w1 + 64 * kW1Pitch;
    float* b1 = w2 + 33 * kW2Pitch;
    float* b2 = b1 + 64;
    for (int i = tid; i < 64 * 32; i += kBwdThreads) w1[(i >> 5) * kW1Pitch + (i & 31)] = p.w1[i];
    for (int i = tid; i < 33 * 64; i += kBwdThreads) w2[(i >> 6) * kW2Pitch + (i & 63)] = p.w2[i];
    if (tid < 64) b1[tid] = p.b1[tid];
    if (tid < 36) b2[tid] = tid < 33 ? p.b2[tid] : 0.f;
    __syncthreads();
    BwdLds L = {};
    L.w1 = w1; L.w2 = w2; L.b1 = b1; L.b2 = b2;
    float* base = smem + kBwdWeightFloats + size_t(wv) * bwd_wave_floats(0);
    L.stage = base; L.tbuf = L.stage + 16 * kStagePitch; L.hbuf = L.tbuf + 16 * kTPitch; L.taps = L.hbuf + 16 * kHPitch;
    BwdAcc A;
#pragma unroll
    for (int m = 0; m < 4; m++) A.w1[m][0] = A.w1[m][1] = A.w2[0][m] = A.w2[1][m] = A.w2s[m] = A.b1[m] = (v4f){0.f, 0.f, 0.f, 0.f};
    A.b2[0] = A.b2[1] = A.b2s = 0.f;
    BwdPending pend = {nullptr, 0};
    const int j = lane & 15, g = lane >> 4;
    const int64_t plane_floats = int64_t(3) * p.plane_h * p.plane_w * 32;
    for (int tile = blockIdx.x * kBwdWaves + wv; tile < Q.n_tiles; tile += gridDim.x * kBwdWaves) {
        const int item = tile / Q.tiles_per_item, t = tile % Q.tiles_per_item;
        const char* planes = reinterpret_cast<const char*>(p.planes_nhwc + int64_t(item) * plane_floats);
        const float* pts = Q.points + int64_t(item) * Q.n_points * 3;
        bwd_gather_tile<true>(P, L, planes, PointTilePos{pts, Q.n_points, t, P.box_scale}, pend, lane);
        v4f h[4], o[2];
        float sig;
        bwd_mlp_forward(L, lane, h, o, sig);
        const int64_t pt0 = int64_t(item) * Q.n_points + 16 * t;
        const float dsig = (Q.grad_sigma && 16 * t + j < Q.n_points) ? Q.grad_sigma[pt0 + j] : 0.f;
#pragma unroll
        for (int n = 0; n < 2; n++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int q = 4 * g + r;
                const float gc = (Q.grad_rgb && 16 * t + q < Q.n_points) ? Q.grad_rgb[(pt0 + q) * 32 + 16 * n + j] : 0.f;
                const float d = gc * rgb_slope_hw(o[n][r]);
                L.tbuf[q * kTPitch + 16 * n + j] = d;
                A.b2[n] += d;
            }
        }
        bwd_tile_core(L, h, dsig, A, lane);
        if (Q.grad_planes_nhwc) { pend.base = Q.grad_planes_nhwc + int64_t(item) * plane_floats; pend.live = min(16, Q.n_points - 16 * t); }
        lds_wave_sync();
    }
    if (pend.live > 0) {
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int pl = 0; pl < 3; pl++) bwd_scatter_chunk(L, pend, a, pl, lane);
    }
    bwd_reduce_decoder_grads(A, smem, Q.grad_w1, Q.grad_b1, Q.grad_w2, Q.grad_b2, tid, lane, j);
}

}  // namespace
