// The point queries of the fused renderer's planes and decoder (run_model for arbitrary points): gnerf_query_points, its backward, its
// position gradient and the Newton projection onto a density level.  query_kernel is below; the others are query_bwd.inl, query_grad.inl
// and project_level.inl.  The four entry points share fill_query (query_fill.inl), and so does gnerf_query_lattice, the densities-only
// query_kernel at lattice points named by their index, which is a unit of its own (query_lattice.hip).
#include "query_bwd.inl"
#include "project_level.inl"

namespace {

// ---------------------------------------------------------------------------------------------
// run_model for arbitrary points (renderer.py:142-148): same lookup + MLP, 16 points per step.

__global__ __launch_bounds__(64) void query_kernel(gnerf_render_params p, float box_scale, int n_points, int n_tiles,
                                                   const float* __restrict__ points, float* __restrict__ out_sigma, float* __restrict__ out_rgb) {
    __shared__ __align__(16) float stage[16 * kStagePitch];
    const int lane = threadIdx.x;
    const int H = p.plane_h, W = p.plane_w;
    const int64_t item_stride = int64_t(3) * H * W * 32;
    const int64_t plane_stride = p.planes_interleaved ? 32 : int64_t(H) * W * 32;
    const unsigned tex_q = p.planes_interleaved ? 24 : 8, row_q = tex_q * unsigned(W);
    const int b = lane >> 3, cq = lane & 7, j = lane & 15, g = lane >> 4;
    Weights w;
    load_weights(w, p, lane);
    const int tiles_per_item = (n_points + 15) / 16;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int item = tile / tiles_per_item, t = tile % tiles_per_item;
        const float* planes_item = p.planes_nhwc + int64_t(item) * item_stride;
        const float* pts = points + int64_t(item) * n_points * 3;
#pragma unroll
        for (int a = 0; a < 2; a++) {
            const int js = 8 * a + b;
            const int idx = min(16 * t + js, n_points - 1);
            const float px = pts[idx * 3 + 0] * box_scale, py = pts[idx * 3 + 1] * box_scale, pz = pts[idx * 3 + 2] * box_scale;
            v4f acc = {0.f, 0.f, 0.f, 0.f};
            lookup_plane(acc, planes_item, H, W, tex_q, row_q, px, py, cq);
            lookup_plane(acc, planes_item + plane_stride, H, W, tex_q, row_q, px, pz, cq);
            lookup_plane(acc, planes_item + 2 * plane_stride, H, W, tex_q, row_q, pz, px, cq);
            acc *= (1.f / 3.f);
            *reinterpret_cast<v4f*>(stage + js * kStagePitch + 4 * cq) = acc;
        }
        __syncthreads();
        const v4f f_lo = *reinterpret_cast<const v4f*>(stage + j * kStagePitch + 8 * g);
        const v4f f_hi = *reinterpret_cast<const v4f*>(stage + j * kStagePitch + 8 * g + 4);
        __syncthreads();
        const float f[8] = {f_lo[0], f_lo[1], f_lo[2], f_lo[3], f_hi[0], f_hi[1], f_hi[2], f_hi[3]};
        v4f h[4];
#pragma unroll
        for (int m = 0; m < 4; m++) h[m] = (v4f){w.b1[m][0], w.b1[m][1], w.b1[m][2], w.b1[m][3]};
#pragma unroll
        for (int s = 0; s < 8; s++) {
#pragma unroll
            for (int m = 0; m < 4; m++) h[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.a1[m][s], f[s], h[m], 0, 0, 0);
        }
        float sig = 0.f;
#pragma unroll
        for (int m = 0; m < 4; m++) {
#pragma unroll
            for (int r = 0; r < 4; r++) { h[m][r] = softplus_fast(h[m][r]); sig += w.w2s[m][r] * h[m][r]; }
        }
        sig += __shfl_xor(sig, 16);
        sig += __shfl_xor(sig, 32);
        sig += w.b2s;
        const int pt = 16 * t + j;
        if (g == 0 && pt < n_points) out_sigma[int64_t(item) * n_points + pt] = sig;
        if (!out_rgb) continue;                 // densities only (shape extraction): the colour half of layer 2 is not evaluated
        v4f o[2];
#pragma unroll
        for (int n = 0; n < 2; n++) o[n] = (v4f){w.b2c[n], w.b2c[n], w.b2c[n], w.b2c[n]};
#pragma unroll
        for (int m = 0; m < 4; m++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
#pragma unroll
                for (int n = 0; n < 2; n++) o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(h[m][r], w.b2w[n][m * 4 + r], o[n], 0, 0, 0);
            }
        }
#pragma unroll
        for (int n = 0; n < 2; n++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int q = 16 * t + 4 * g + r;
                if (q < n_points) out_rgb[(int64_t(item) * n_points + q) * 32 + 16 * n + j] = sigmoid_fast(o[n][r]) * 1.002f - 0.001f;
            }
        }
    }
}

}  // namespace

#include "query_fill.inl"

extern "C" int gnerf_query_points(const float* planes_nhwc, int n_items, int plane_h, int plane_w,
                                  const float* points, int n_points, float box_warp,
                                  const float* w1, const float* b1, const float* w2, const float* b2,
                                  float* out_sigma, float* out_rgb, int planes_interleaved, gnerf_stream_t stream) {
    using namespace gnerf;
    Params P; int tiles_per_item; int64_t tiles;
    if (int e = fill_query("query_points", planes_nhwc, n_items, plane_h, plane_w, n_points, box_warp, w1, b1, w2, b2, planes_interleaved, P, tiles_per_item, tiles)) return e;
    if (!points || !out_sigma) return fail(GNERF_E_ARG, "query_points: null pointer");
    if (n_points < 1) return fail(GNERF_E_ARG, "query_points: n_points must be positive");
    if (tiles > INT32_MAX) return fail(GNERF_E_ARG, "query_points: too many points");
    const int blocks = int(tiles < int64_t(kNumCU) * 16 ? tiles : int64_t(kNumCU) * 16);
    hipLaunchKernelGGL(query_kernel, dim3(blocks), dim3(64), 0, as_stream(stream), P.p, P.box_scale, n_points, int(tiles),
                       points, out_sigma, out_rgb);
    return check_launch("query_kernel");
}

extern "C" int gnerf_query_points_backward(const float* planes_nhwc, int n_items, int plane_h, int plane_w,
                                           const float* points, int n_points, float box_warp,
                                           const float* w1, const float* b1, const float* w2, const float* b2,
                                           const float* grad_sigma, const float* grad_rgb,
                                           float* grad_planes_nhwc, float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2,
                                           int planes_interleaved, gnerf_stream_t stream) {
    using namespace gnerf;
    Params P; int tiles_per_item; int64_t tiles;
    if (int e = fill_query("query_points_backward", planes_nhwc, n_items, plane_h, plane_w, n_points, box_warp, w1, b1, w2, b2, planes_interleaved, P, tiles_per_item, tiles)) return e;
    if (!points) return fail(GNERF_E_ARG, "query_points_backward: points is null");
    if (n_points < 1) return fail(GNERF_E_ARG, "query_points_backward: n_points must be positive");
    const int n_dec = (grad_w1 != nullptr) + (grad_b1 != nullptr) + (grad_w2 != nullptr) + (grad_b2 != nullptr);
    if (n_dec != 0 && n_dec != 4) return fail(GNERF_E_ARG, "query_points_backward: the four decoder gradients are given together or not at all");
    if ((!grad_planes_nhwc && n_dec == 0) || (!grad_sigma && !grad_rgb)) return GNERF_OK;
    if (!planes_fit_32bit_taps(&P.p)) return fail(GNERF_E_UNSUPPORTED, "query_points_backward: planes too large for 32-bit tap offsets");
    if (tiles > INT32_MAX) return fail(GNERF_E_ARG, "query_points_backward: too many points");
    QueryBwdArgs Q;
    Q.points = points; Q.grad_sigma = grad_sigma; Q.grad_rgb = grad_rgb; Q.n_points = n_points;
    Q.tiles_per_item = tiles_per_item; Q.n_tiles = int(tiles);
    Q.grad_planes_nhwc = grad_planes_nhwc; Q.grad_w1 = grad_w1; Q.grad_b1 = grad_b1; Q.grad_w2 = grad_w2; Q.grad_b2 = grad_b2;
    const size_t lds_bytes = (kBwdWeightFloats + kBwdWaves * bwd_wave_floats(0)) * sizeof(float);
    int64_t blocks = (tiles + kBwdWaves - 1) / kBwdWaves;
    if (blocks > int64_t(kNumCU) * 2) blocks = int64_t(kNumCU) * 2;
    hipLaunchKernelGGL(query_bwd_kernel, dim3((unsigned)blocks), dim3(kBwdThreads), lds_bytes, as_stream(stream), P, Q);
    return check_launch("query_bwd_kernel");
}

extern "C" int gnerf_query_points_grad(const float* planes_nhwc, int n_items, int plane_h, int plane_w,
                                       const float* points, int n_points, float box_warp,
                                       const float* w1, const float* b1, const float* w2, const float* b2,
                                       const float* grad_sigma, const float* grad_rgb, float* grad_points,
                                       int planes_interleaved, gnerf_stream_t stream) {
    using namespace gnerf;
    Params P; int tiles_per_item; int64_t tiles;
    if (int e = fill_query("query_points_grad", planes_nhwc, n_items, plane_h, plane_w, n_points, box_warp, w1, b1, w2, b2, planes_interleaved, P, tiles_per_item, tiles)) return e;
    if (!points || !grad_points) return fail(GNERF_E_ARG, "query_points_grad: null pointer");
    if (n_points < 1) return fail(GNERF_E_ARG, "query_points_grad: n_points must be positive");
    if (!grad_sigma && !grad_rgb) return fail(GNERF_E_ARG, "query_points_grad: grad_sigma and grad_rgb are both null");
    if (!planes_fit_32bit_taps(&P.p)) return fail(GNERF_E_UNSUPPORTED, "query_points_grad: planes too large for 32-bit tap offsets");
    if (tiles > INT32_MAX) return fail(GNERF_E_ARG, "query_points_grad: too many points");
    QueryGradArgs Q;
    Q.points = points; Q.grad_sigma = grad_sigma; Q.grad_rgb = grad_rgb; Q.grad_points = grad_points; Q.n_points = n_points;
    Q.tiles_per_item = tiles_per_item; Q.n_tiles = int(tiles);
    const size_t lds_bytes = (kBwdWeightFloats + kBwdWaves * query_grad_wave_floats()) * sizeof(float);         // 49.3 KB: three workgroups per CU (the kernel is compiled for three waves per SIMD)
    int64_t blocks = (tiles + kBwdWaves - 1) / kBwdWaves;
    if (blocks > int64_t(kNumCU) * 3) blocks = int64_t(kNumCU) * 3;
    if (grad_rgb) hipLaunchKernelGGL(query_grad_kernel<true>, dim3((unsigned)blocks), dim3(kBwdThreads), lds_bytes, as_stream(stream), P, Q);
    else          hipLaunchKernelGGL(query_grad_kernel<false>, dim3((unsigned)blocks), dim3(kBwdThreads), lds_bytes, as_stream(stream), P, Q);
    return check_launch("query_grad_kernel");
}

extern "C" int gnerf_project_points_to_level(const float* planes_nhwc, int n_items, int plane_h, int plane_w,
                                             const float* points, int n_points, float box_warp,
                                             const float* w1, const float* b1, const float* w2, const float* b2,
                                             float level, const float* affine, int max_steps, float radius, float tol,
                                             float* points_out, float* residual_in, float* residual_out, unsigned char* status,
                                             int planes_interleaved, gnerf_stream_t stream) {
    using namespace gnerf;
    Params P; int tiles_per_item; int64_t tiles;
    if (int e = fill_query("project_points_to_level", planes_nhwc, n_items, plane_h, plane_w, n_points, box_warp, w1, b1, w2, b2, planes_interleaved, P, tiles_per_item, tiles)) return e;
    if (!points || !points_out || !residual_in || !residual_out || !status) return fail(GNERF_E_ARG, "project_points_to_level: null pointer");
    if (n_points < 1) return fail(GNERF_E_ARG, "project_points_to_level: n_points must be positive");
    if (max_steps < 0) return fail(GNERF_E_ARG, "project_points_to_level: max_steps must be >= 0 (got %d)", max_steps);
    if (!(radius >= 0.f) || !std::isfinite(radius)) return fail(GNERF_E_ARG, "project_points_to_level: radius must be finite and >= 0");
    if (!(tol > 0.f) || !std::isfinite(tol)) return fail(GNERF_E_ARG, "project_points_to_level: tol must be finite and > 0");
    if (!planes_fit_32bit_taps(&P.p)) return fail(GNERF_E_UNSUPPORTED, "project_points_to_level: planes too large for 32-bit tap offsets");
    if (tiles > INT32_MAX) return fail(GNERF_E_ARG, "project_points_to_level: too many points");
    ProjectArgs Q = {};
    Q.points = points; Q.points_out = points_out; Q.residual_in = residual_in; Q.residual_out = residual_out; Q.status = status;
    Q.has_affine = affine != nullptr;
    if (affine) for (int i = 0; i < 12; i++) Q.a[i] = affine[i];
    Q.level = level; Q.radius = radius; Q.tol = tol; Q.max_steps = max_steps;
    Q.n_points = n_points; Q.tiles_per_item = tiles_per_item; Q.n_tiles = int(tiles);
    const size_t lds_bytes = (kBwdWeightFloats + kBwdWaves * query_grad_wave_floats()) * sizeof(float);         // as query_grad_kernel: three workgroups per CU
    int64_t blocks = (tiles + kBwdWaves - 1) / kBwdWaves;
    if (blocks > int64_t(kNumCU) * 3) blocks = int64_t(kNumCU) * 3;
    hipLaunchKernelGGL(project_level_kernel, dim3((unsigned)blocks), dim3(kBwdThreads), lds_bytes, as_stream(stream), P, Q);
    return check_launch("project_level_kernel");
}
