// Fused tri-plane importance renderer for gfx950 (MI355X).
//
// One kernel does, per ray, everything ImportanceRenderer.forward does with a dozen whole-tensor PyTorch
// ops and ~4 GB of intermediates (reference training/volumetric_rendering/renderer.py:88-140,
// ray_marcher.py:25-57, triplane.py:113-136):
//
//   depth proposals -> tri-plane bilinear lookup -> 32->64->33 MLP -> coarse march -> importance
//   resampling -> fine lookup + MLP -> depth merge -> final composite.
//
// The renderer is four translation units, each including only what it uses (every .inl and render_params.h names its own needs):
//   render.hip            this file: the forward entry points, which choose each call's kernels; the GENERIC kernel described below (any
//                         sample count up to 256+256) and the depth clamp; the host helpers the other units call (render_params.h)
//   render_pipe.hip       the kernels that stage the decoder, and their launch functions: the pipelined kernels that run G-NeRF's actual
//                         configurations (render_pipe.inl: 3 shader waves + 1 scalar wave per workgroup, three rays in flight, up to
//                         144+144 samples; forward and the backward's first pass), the backward's tile kernel (render_bwd_tiles.inl)
//                         and the decoder pack (decoder_pack.inl).  Its header says why they are one unit.
//   render_backward.hip   the backward entry points and their other kernels (render_bwd.inl, scatter_binned.inl, render_ray_grad.inl)
//   render_query.hip      the point queries (query_bwd.inl, query_grad.inl, project_level.inl)
// Shared device code: render_core.inl (depth proposals, importance resampling, the ray march, DPP scans, the generic lookup),
// decoder_choice.inl (the decoder statistics and choose_mlp), render_shade.inl (the 16-sample shade tile, decoder staging and plane taps),
// render_pipe_layout.inl (the pipelined kernels' LDS layout and ray order), render_bwd_tile.inl (the backward's tile helpers),
// plane_taps_grad.inl (the derivative taps).
//
// Host half: fill_params validates a call and derives what every kernel reads; a handful of small helpers hold the facts more
// than one launcher needs (tiles per wave, the pipelined launch's unit and grid, 32-bit tap offsets, max |planes|).
// gnerf_render_forward picks generic or pipelined and launches through launch_pipe<TP>(full, gen, ...).
// Every A/B override is an environment variable read once per call, where its launcher starts deciding.
//
// Generic kernel: ONE WAVE (a 64-lane workgroup) owns a ray at a time and walks a small tile of rays
// (4x4 pixels when the rays form an image).  Nothing but the three outputs is ever written to HBM.
//
//  * Lookup ("gather") layout: 8 adjacent lanes read one whole 128-byte texel (32 fp32 channels of the NHWC
//    planes) with one global_load_dwordx4 each, so a wave instruction touches 8 cache lines, the minimum.
//    A wave does 8 samples per step, two steps per 16-sample MLP tile.
//  * MLP on the matrix cores in exact fp32: v_mfma_f32_16x16x4_f32.  Layer 1 is computed transposed
//    (hidden on the accumulator rows, samples on the lanes) so that its accumulator registers are directly
//    the A operand of layer 2 (which sums over hidden) -- no data movement between the layers.  Layer 2
//    puts samples on accumulator rows and colour channels on lanes, which is what compositing wants
//    (a per-lane sum over registers).  The density row of layer 2 is a 16-term per-lane dot product plus
//    two cross-lane adds: a 33rd column would cost a third more MFMAs.
//  * Per-sample scalars (depth, density, weights, cdf, ranks) live in a few hundred bytes of LDS per wave;
//    colours of all samples (needed until the final weights are known) live in LDS as a lane-private
//    spill, 1 KiB per 16 samples.
//  * The call-wide depth clamp of ray_marcher.py:49-50 needs min/max over every depth of the call: waves
//    publish their extrema with two integer atomics, and a tiny second kernel applies the clamp.

#include "render_core.inl"
#include "render_pipe_layout.inl"
#include <cstdlib>
#include <cstring>

namespace {

// Per-wave LDS carve-up (all float/int, 16-byte aligned pieces)
struct Scratch {
    float* t_e;      // [S_pad]  element depths: coarse k at k, fine i at 16*tiles_c + i
    float* sig_e;    // [S_pad]  densities, same indexing
    float* v_e;      // [S_pad]  final colour weight of each element (0 for padding)
    int*   rank_e;   // [S_pad]
    float* s_t;      // [S_pad]  depths in sorted order
    float* s_sig;    // [S_pad]
    float* w_s;      // [S_pad]  weights (coarse march, then final march)
    float* cdf;      // [S_pad]
    float* stage;    // [16 * kStagePitch]
    float* colors;   // [(tiles_c + tiles_f) * 2 * 256]
};

__host__ __device__ inline size_t scratch_floats(int s_pad, int tiles) {
    return size_t(8) * s_pad + 16 * kStagePitch + size_t(tiles) * 512;
}

// Shade `count` samples whose depths sit in lds.t_e[e0 ...]: densities -> lds.sig_e[e0 ...], colours ->
// lds.colors tiles tile0 ...
__device__ __forceinline__ void shade(const Params& P, const Weights& w, const Scratch& lds, const float* __restrict__ planes_item,
                                      float ox, float oy, float oz, float dx, float dy, float dz,
                                      int e0, int count, int ntiles, int tile0, int lane, const float* sig_noise = nullptr) {
    const int H = P.p.plane_h, W = P.p.plane_w;
    const int64_t plane_stride = P.plane_pitch / 4;
    const unsigned tex_q = P.tex_pitch / 16, row_q = P.row_pitch / 16;
    const int b = lane >> 3, cq = lane & 7;     // lookup layout: sample-in-step, channel quad
    const int j = lane & 15, g = lane >> 4;     // MFMA layout: sample-in-tile, k group
    for (int t = 0; t < ntiles; t++) {
        // ---- lookup: 2 steps x 8 samples, staged through LDS into the MFMA layout
#pragma unroll
        for (int a = 0; a < 2; a++) {
            const int js = 8 * a + b;
            const int idx = min(16 * t + js, count - 1);          // padding lanes re-shade the last sample
            const float depth = lds.t_e[e0 + idx];
            const float px = __fadd_rn(ox, __fmul_rn(depth, dx)) * P.box_scale;
            const float py = __fadd_rn(oy, __fmul_rn(depth, dy)) * P.box_scale;
            const float pz = __fadd_rn(oz, __fmul_rn(depth, dz)) * P.box_scale;
            v4f acc = {0.f, 0.f, 0.f, 0.f};
            lookup_plane(acc, planes_item, H, W, tex_q, row_q, px, py, cq);                          // plane 0: (x, y)
            lookup_plane(acc, planes_item + plane_stride, H, W, tex_q, row_q, px, pz, cq);           // plane 1: (x, z)
            lookup_plane(acc, planes_item + 2 * plane_stride, H, W, tex_q, row_q, pz, px, cq);       // plane 2: (z, x)
            acc *= (1.f / 3.f);                                                         // mean over planes, triplane.py:126
            *reinterpret_cast<v4f*>(lds.stage + js * kStagePitch + 4 * cq) = acc;
        }
        __syncthreads();
        const v4f f_lo = *reinterpret_cast<const v4f*>(lds.stage + j * kStagePitch + 8 * g);
        const v4f f_hi = *reinterpret_cast<const v4f*>(lds.stage + j * kStagePitch + 8 * g + 4);
        __syncthreads();
        const float f[8] = {f_lo[0], f_lo[1], f_lo[2], f_lo[3], f_hi[0], f_hi[1], f_hi[2], f_hi[3]};
        // ---- layer 1: H^T[64 x 16] = W1[64 x 32] . X^T[32 x 16], bias preloaded
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
            for (int r = 0; r < 4; r++) {
                h[m][r] = softplus_fast(h[m][r]);
                sig += w.w2s[m][r] * h[m][r];
            }
        }
        sig += __shfl_xor(sig, 16);
        sig += __shfl_xor(sig, 32);
        sig += w.b2s;
        if (g == 0 && 16 * t + j < count) lds.sig_e[e0 + 16 * t + j] = sig + (sig_noise ? sig_noise[16 * t + j] : 0.f);      // renderer.py:146-147
        // ---- layer 2: O[16 x 32] = H[16 x 64] . W2^T[64 x 32]
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
        // rgb = sigmoid(o) * 1.002 - 0.001 (triplane.py:134); lane (channel j of block n, samples 4g..4g+3)
#pragma unroll
        for (int n = 0; n < 2; n++) {
            v4f c;
#pragma unroll
            for (int r = 0; r < 4; r++) c[r] = sigmoid_fast(o[n][r]) * 1.002f - 0.001f;
            *reinterpret_cast<v4f*>(lds.colors + ((size_t(tile0 + t) * 2 + n) * 4 + g) * 64 + 4 * j) = c;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(64, 2) void render_kernel_generic(Params P) {
    extern __shared__ __align__(16) float smem[];
    const gnerf_render_params& p = P.p;
    const int lane = threadIdx.x;
    const int S = p.depth_resolution, F = p.depth_resolution_importance;
    const int s_pad = 16 * (P.tiles_c + P.tiles_f);
    Scratch lds;
    lds.t_e = smem;
    lds.sig_e = lds.t_e + s_pad;
    lds.v_e = lds.sig_e + s_pad;
    lds.rank_e = reinterpret_cast<int*>(lds.v_e + s_pad);
    lds.s_t = lds.v_e + 2 * s_pad;
    lds.s_sig = lds.s_t + s_pad;
    lds.w_s = lds.s_sig + s_pad;
    lds.cdf = lds.w_s + s_pad;
    lds.stage = lds.cdf + s_pad;
    lds.colors = lds.stage + 16 * kStagePitch;

    // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs, so give each XCD a
    // contiguous run of ray tiles (its L2 then sees neighbouring rays).  Speed only.
    const int n_groups = P.n_tiles << P.split_shift;
    const int per_xcd = (n_groups + kNumXCD - 1) / kNumXCD;
    const int group = (blockIdx.x % kNumXCD) * per_xcd + blockIdx.x / kNumXCD;
    const int tile = group >> P.split_shift;
    const int rr_count = group < n_groups ? (kRaysPerWave >> P.split_shift) : 0;        // surplus workgroups of the rounded-up grid only report in
    const int rr_first = (group & ((1 << P.split_shift) - 1)) * (kRaysPerWave >> P.split_shift);

    Weights w;
    load_weights(w, p, lane);
    const int fine_e0 = 16 * P.tiles_c;
    const int n_all = S + F;
    DepthRange range;

    for (int rr = rr_first; rr < rr_first + rr_count; rr++) {
        // ---- which ray
        int64_t ray;
        if (P.tiles_per_item > 0) {             // 4x4 pixel tiles, walked down image columns
            const int item = tile / P.tiles_per_item, tt = tile % P.tiles_per_item;
            const int tx = tt / P.tiles_y, ty = tt % P.tiles_y;
            const int x = tx * 4 + (rr & 3), y = ty * 4 + (rr >> 2);
            ray = int64_t(item) * p.rays_per_item + int64_t(y) * p.image_width + x;
        } else {
            ray = int64_t(tile) * kRaysPerWave + rr;
            if (ray >= P.total_rays) break;
        }
        const int item = int(ray / p.rays_per_item);
        const float ox = p.ray_origins[ray * 3 + 0], oy = p.ray_origins[ray * 3 + 1], oz = p.ray_origins[ray * 3 + 2];
        const float dx = p.ray_dirs[ray * 3 + 0], dy = p.ray_dirs[ray * 3 + 1], dz = p.ray_dirs[ray * 3 + 2];
        const float* planes_item = reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.planes_nhwc) + int64_t(item) * P.item_bytes);
        float* dbg = p.debug ? p.debug + ray * GNERF_DEBUG_SLOTS * n_all : nullptr;

        // ---- stratified depth proposals (renderer.py:169-192)
        for (int k = lane; k < S; k += 64) {
            const float d = coarse_depth(P, ray, k);
            lds.t_e[k] = d;
            if (dbg) dbg[GNERF_DBG_DEPTH_COARSE * n_all + k] = d;
        }
        for (int k = lane; k < s_pad; k += 64) lds.v_e[k] = 0.f;
        __syncthreads();

        // ---- coarse pass
        shade(P, w, lds, planes_item, ox, oy, oz, dx, dy, dz, 0, S, P.tiles_c, 0, lane, p.sigma_noise_coarse ? p.sigma_noise_coarse + ray * S : nullptr);
        if (dbg) for (int k = lane; k < S; k += 64) dbg[GNERF_DBG_SIGMA_COARSE * n_all + k] = lds.sig_e[k];

        float w_sum, wt_sum;
        if (F > 0) {
            march(lds.t_e, lds.sig_e, lds.w_s, S, lane, w_sum, wt_sum);
            __syncthreads();
            if (dbg) for (int k = lane; k < S - 1; k += 64) dbg[GNERF_DBG_WEIGHT_COARSE * n_all + k] = lds.w_s[k];

            resample_fine(P, ray, lds.t_e, lds.w_s, lds.s_sig, lds.cdf, lds.t_e + fine_e0, dbg, n_all, lane, [] { __syncthreads(); });

            // ---- fine pass
            shade(P, w, lds, planes_item, ox, oy, oz, dx, dy, dz, fine_e0, F, P.tiles_f, P.tiles_c, lane, p.sigma_noise_fine ? p.sigma_noise_fine + ray * F : nullptr);
            if (dbg) for (int k = lane; k < F; k += 64) dbg[GNERF_DBG_SIGMA_FINE * n_all + k] = lds.sig_e[fine_e0 + k];

            merge_by_depth(lds.t_e, lds.sig_e, lds.rank_e, lds.s_t, lds.s_sig, S, F, fine_e0, lane);
            __syncthreads();
            march(lds.s_t, lds.s_sig, lds.w_s, n_all, lane, w_sum, wt_sum);
            __syncthreads();
            // colour weight of the sample at sorted position r: (w[r-1] + w[r]) / 2  (midpoint colours, ray_marcher.py:27)
            for (int q = lane; q < n_all; q += 64) {
                const int e = q < S ? q : fine_e0 + (q - S);
                const int r = lds.rank_e[e];
                const float wl = r > 0 ? lds.w_s[r - 1] : 0.f, wr = r < n_all - 1 ? lds.w_s[r] : 0.f;
                lds.v_e[e] = (wl + wr) * 0.5f;
            }
            if (dbg) {
                for (int k = lane; k < n_all; k += 64) { dbg[GNERF_DBG_DEPTH_SORTED * n_all + k] = lds.s_t[k]; dbg[GNERF_DBG_SIGMA_SORTED * n_all + k] = lds.s_sig[k]; }
                for (int k = lane; k < n_all - 1; k += 64) dbg[GNERF_DBG_WEIGHT_FINAL * n_all + k] = lds.w_s[k];
            }
            range.add(P, item, lds.s_t[0], lds.s_t[n_all - 1]);
        } else {
            march(lds.t_e, lds.sig_e, lds.w_s, S, lane, w_sum, wt_sum);
            __syncthreads();
            for (int k = lane; k < S; k += 64) {
                const float wl = k > 0 ? lds.w_s[k - 1] : 0.f, wr = k < S - 1 ? lds.w_s[k] : 0.f;
                lds.v_e[k] = (wl + wr) * 0.5f;
            }
            if (dbg) for (int k = lane; k < S - 1; k += 64) dbg[GNERF_DBG_WEIGHT_FINAL * n_all + k] = lds.w_s[k];
            // the reference takes min/max over the depths tensor; coarse depths ascend (up to rounding ties)
            float mn = INFINITY, mx = -INFINITY;
            for (int k = lane; k < S; k += 64) { mn = fminf(mn, lds.t_e[k]); mx = fmaxf(mx, lds.t_e[k]); }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
            range.add(P, item, mn, mx);
        }
        __syncthreads();

        // ---- colours: rgb[c] = sum_e v_e * colour_e[c]; lane = (channel j of block n, samples 4g..4g+3 of each tile)
        const int j = lane & 15, g = lane >> 4;
        float acc[2] = {0.f, 0.f};
        const int ntile_all = P.tiles_c + P.tiles_f;
        for (int t = 0; t < ntile_all; t++) {
            const v4f v = *reinterpret_cast<const v4f*>(lds.v_e + 16 * t + 4 * g);
#pragma unroll
            for (int n = 0; n < 2; n++) {
                const v4f c = *reinterpret_cast<const v4f*>(lds.colors + ((size_t(t) * 2 + n) * 4 + g) * 64 + 4 * j);
                acc[n] += v[0] * c[0] + v[1] * c[1] + v[2] * c[2] + v[3] * c[3];
            }
        }
#pragma unroll
        for (int n = 0; n < 2; n++) {
            acc[n] += __shfl_xor(acc[n], 16);
            acc[n] += __shfl_xor(acc[n], 32);
            if (p.white_back) acc[n] = acc[n] + 1.f - w_sum;
            acc[n] = acc[n] * 2.f - 1.f;
        }
        if (g < 2) p.out_rgb[ray * 32 + 16 * g + j] = g == 0 ? acc[0] : acc[1];
        if (lane == 0) {
            float depth = wt_sum / w_sum;
            if (depth != depth) depth = INFINITY;        // nan_to_num(nan=inf), ray_marcher.py:49; clamp applied by clamp_depth_kernel
            p.out_depth[ray] = depth;
            p.out_wsum[ray] = w_sum;
        }
        __syncthreads();
    }
    if (lane == 0) range.flush(P);
}

// The clamp.  The last block to finish puts the workspace back to idle.
constexpr int kClampPerThread = 4;
__global__ __launch_bounds__(256) void clamp_depth_kernel(float* depth, unsigned* ws, int64_t n, int rays_per_item, int n_items_per_item_clamp) {
    const bool per_item = n_items_per_item_clamp > 0;
    float lo = 0.f, hi = 0.f;
    if (!per_item) { lo = ord_decode(~ws[0]); hi = ord_decode(ws[1]); }
#pragma unroll
    for (int k = 0; k < kClampPerThread; k++) {
        const int64_t i = (int64_t(blockIdx.x) * kClampPerThread + k) * 256 + threadIdx.x;
        if (i < n) {
            if (per_item) { const unsigned* w = ws + kClampItemWord0 + 2 * int(i / rays_per_item); lo = ord_decode(~w[0]); hi = ord_decode(w[1]); }
            depth[i] = fminf(fmaxf(depth[i], lo), hi);   // torch.clamp(x, min, max)
        }
    }
    __syncthreads();                                             // every thread of the block has read (and used) the range
    __shared__ int last;
    if (threadIdx.x == 0) last = atomicAdd(ws + 3, 1u) == gridDim.x - 1;
    __syncthreads();
    if (last) {                                                  // the last block puts the workspace back to idle
        if (threadIdx.x == 0) { ws[0] = 0u; ws[1] = 0u; ws[3] = 0u; }
        if (threadIdx.x < kNumXCD) ws[kDealWord0 + threadIdx.x * kDealLineWords] = 0u;      // the render kernel's dealing counters
        for (int i = threadIdx.x; i < 2 * n_items_per_item_clamp; i += 256) ws[kClampItemWord0 + i] = 0u;
    }
}

}  // namespace

// ---- the host helpers every render unit calls (render_params.h)
namespace gnerf {

int check_common(const gnerf_render_params* p) {
    if (!p) return fail(GNERF_E_ARG, "render: params is null");
    if (!p->planes_nhwc || !p->w1 || !p->b1 || !p->w2 || !p->b2) return fail(GNERF_E_ARG, "render: planes and decoder weights must not be null");
    if (p->n_items < 1 || p->plane_h < 1 || p->plane_w < 1) return fail(GNERF_E_ARG, "render: bad plane shape");
    if (int64_t(p->planes_shared ? 1 : p->n_items) * 3 * p->plane_h * p->plane_w * 32 > INT32_MAX * int64_t(4))
        return fail(GNERF_E_ARG, "render: planes too large");
    if (!(p->box_warp > 0.f)) return fail(GNERF_E_ARG, "render: box_warp must be positive");
    if (p->planes_interleaved != 0 && p->planes_interleaved != 1) return fail(GNERF_E_ARG, "render: planes_interleaved must be 0 or 1");
    return GNERF_OK;
}

void fill_pitches(Params& P) {
    const unsigned W = unsigned(P.p.plane_w), H = unsigned(P.p.plane_h);
    P.tex_pitch = P.p.planes_interleaved ? 384u : 128u;
    P.row_pitch = P.tex_pitch * W;
    P.plane_pitch = P.p.planes_interleaved ? 128u : H * W * 128u;
}

// Validation and derived launch parameters shared by the forward and backward entry points.
int fill_params(const gnerf_render_params* p, Params& P) {
    if (int e = check_common(p)) return e;
    const bool own_rays = !p->ray_origins && !p->ray_dirs && p->cam2world && p->intrinsics;
    if (!own_rays && (!p->ray_origins || !p->ray_dirs)) return fail(GNERF_E_ARG, "render: rays must not be null (or both null with cam2world and intrinsics given)");
    // ray tensors AND cameras: the generating instantiation keys on cam2world and would replace the caller's rays by camera rays
    // (and divide by image_width, which nothing has checked for this combination): one source of rays per call
    if (!own_rays && (p->cam2world || p->intrinsics)) return fail(GNERF_E_ARG, "render: give ray tensors or cam2world / intrinsics, not both");
    if (own_rays && (p->image_width < 1 || int64_t(p->image_width) * p->image_width != p->rays_per_item))
        return fail(GNERF_E_ARG, "render: in-kernel rays need rays_per_item = image_width^2");
    if (p->rng_mode != GNERF_RNG_TENSORS && p->rng_mode != GNERF_RNG_TORCH_PHILOX) return fail(GNERF_E_ARG, "render: rng_mode %d is not one of GNERF_RNG_*", p->rng_mode);
    if (p->rng_mode == GNERF_RNG_TENSORS && !p->noise_coarse) return fail(GNERF_E_ARG, "render: noise_coarse must not be null");
    if (p->rng_mode == GNERF_RNG_TORCH_PHILOX && (p->noise_coarse || p->noise_fine)) return fail(GNERF_E_ARG, "render: rng_mode = GNERF_RNG_TORCH_PHILOX takes no noise tensors");
    const int S = p->depth_resolution, F = p->depth_resolution_importance;
    if (S < 2 || S > GNERF_MAX_SAMPLES) return fail(GNERF_E_ARG, "render: depth_resolution %d outside [2, %d]", S, GNERF_MAX_SAMPLES);
    if (F < 0 || F > GNERF_MAX_SAMPLES) return fail(GNERF_E_ARG, "render: depth_resolution_importance %d outside [0, %d]", F, GNERF_MAX_SAMPLES);
    if (F > 0 && S < 4) return fail(GNERF_E_ARG, "render: importance sampling needs depth_resolution >= 4");
    if (F > 0 && !p->noise_fine && p->rng_mode == GNERF_RNG_TENSORS) return fail(GNERF_E_ARG, "render: noise_fine is null but depth_resolution_importance > 0");
    if (p->sigma_noise_fine && !p->sigma_noise_coarse) return fail(GNERF_E_ARG, "render: sigma_noise_fine without sigma_noise_coarse");
    if (p->sigma_noise_coarse && F > 0 && !p->sigma_noise_fine) return fail(GNERF_E_ARG, "render: sigma_noise_coarse is given but sigma_noise_fine is null with depth_resolution_importance > 0");
    if (p->sigma_noise_coarse && (own_rays || p->rng_mode != GNERF_RNG_TENSORS)) return fail(GNERF_E_UNSUPPORTED, "render: density noise comes with ray and noise tensors (not with in-kernel rays / draws)");
    if (p->rays_per_item < 1) return fail(GNERF_E_ARG, "render: rays_per_item must be positive");
    if ((p->ray_start_per_ray == nullptr) != (p->ray_end_per_ray == nullptr)) return fail(GNERF_E_ARG, "render: per-ray start and end must be given together");
    const int64_t total = int64_t(p->n_items) * p->rays_per_item;
    if (total * (S + F) > INT32_MAX * int64_t(8)) return fail(GNERF_E_ARG, "render: too many samples in one call");

    P.p = *p;
    fill_pitches(P);
    if ((p->planes_shared != 0 && p->planes_shared != 1) || (p->depth_clamp_per_item != 0 && p->depth_clamp_per_item != 1))
        return fail(GNERF_E_ARG, "render: planes_shared and depth_clamp_per_item must be 0 or 1");
    if (p->depth_clamp_per_item && p->n_items > kClampMaxItems) return fail(GNERF_E_ARG, "render: depth_clamp_per_item supports at most %d items", kClampMaxItems);
    P.item_bytes = p->planes_shared ? 0 : int64_t(3) * p->plane_h * p->plane_w * 128;
    if (P.row_pitch >= (1u << 24)) return fail(GNERF_E_UNSUPPORTED, "render: plane rows wider than 2^24 bytes");
    P.box_scale = float(2.0 / double(p->box_warp));
    P.delta = float((double(p->ray_end) - double(p->ray_start)) / double(S - 1));
    P.inv_start = float(1.0 / double(p->ray_start));
    P.inv_end = float(1.0 / double(p->ray_end));
    P.disp_delta = float(1.0 / double(S - 1));
    P.tiles_c = (S + 15) / 16;
    P.tiles_f = (F + 15) / 16;
    P.total_rays = int(total);
    P.split_shift = 0;
    P.pipe_unit = kPipeUnit;
    P.deal_counters = nullptr;
    P.pipe_guided = 0;
    P.absmax = nullptr;
    P.decoder_pack = nullptr;
    P.draw_c = P.draw_f = TorchRandDraw{};
    P.draw_item_ctr = 0;
    if (p->rng_mode == GNERF_RNG_TORCH_PHILOX) {
        const int64_t units = p->rng_per_item ? int64_t(p->rays_per_item) : total;       // rays one draw covers
        if ((p->rng_per_item != 0 && p->rng_per_item != 1) || p->rng_offset_item_stride % 4 != 0)
            return fail(GNERF_E_ARG, "render: rng_per_item must be 0 or 1 and rng_offset_item_stride a multiple of 4");
        if (!torch_rand_draw(p->rng_seed, p->rng_offset_coarse, p->rng_threads_coarse, units * S, P.draw_c) ||
            (F > 0 && !torch_rand_draw(p->rng_seed, p->rng_offset_fine, p->rng_threads_fine, units * F, P.draw_f)))
            return fail(GNERF_E_UNSUPPORTED, "render: the generator geometry (threads %u / %u, offsets %llu / %llu) is not one the in-kernel draws reproduce",
                        p->rng_threads_coarse, p->rng_threads_fine, (unsigned long long)p->rng_offset_coarse, (unsigned long long)p->rng_offset_fine);
        P.draw_item_ctr = p->rng_per_item ? p->rng_offset_item_stride / 4 : 0;
    }
    const int iw = p->image_width;
    if (iw > 0 && iw % 4 == 0 && p->rays_per_item % iw == 0 && (p->rays_per_item / iw) % 4 == 0) {
        P.tiles_y = p->rays_per_item / iw / 4;
        P.tiles_per_item = (iw / 4) * P.tiles_y;
        P.n_tiles = P.tiles_per_item * p->n_items;
    } else {
        P.tiles_y = 0;
        P.tiles_per_item = 0;
        P.n_tiles = int((total + kRaysPerWave - 1) / kRaysPerWave);
    }
    return GNERF_OK;
}

// resident workgroups per CU for a count of tiles per wave (the pipelined kernels' __launch_bounds__)
static int pipe_workgroups_per_cu(int tp) { return tp == 1 ? GNERF_PIPE_WAVES_PER_SIMD : (tp == 2 ? GNERF_PIPE2_WAVES_PER_SIMD : 2); }
// Dealing unit and grid of a pipelined launch (the forward's, the backward's first pass).  One dealing unit per workgroup until the chip
// is full: a small launch is latency-bound, and the three half-steps of pipeline fill cost less than leaving compute units idle (64x64
// rays: 167 -> 70 us); the unit shrinks from 8 rays down to what spreads the launch over every resident workgroup slot (a 64x64 frame:
// 4 rays each on pipe<1>, 6 on pipe<2>).
PipeLaunch pipe_launch(int tp, int64_t total_seq) {
    const int64_t capacity = int64_t(pipe_workgroups_per_cu(tp)) * kNumCU;
    PipeLaunch L;
    L.fills_chip = total_seq >= capacity * kPipeUnit;
    L.unit = L.fills_chip ? kPipeUnit : int((total_seq + capacity - 1) / capacity);        // >= 1: total_seq >= 1
    const int64_t g = ((total_seq + L.unit - 1) / L.unit + kNumXCD - 1) / kNumXCD * kNumXCD;
    L.grid = unsigned(g < kNumXCD ? kNumXCD : (g > capacity ? capacity : g));
    return L;
}
// max |planes| of this call's planes, measured into `word` (one device float)
static int measure_absmax(const gnerf_render_params* p, float* word, gnerf_stream_t stream) {
    return gnerf_planes_absmax(p->planes_nhwc, int64_t(p->planes_shared ? 1 : p->n_items) * 3 * p->plane_h * p->plane_w * 32, word, stream);
}
int absmax_or_measure(const gnerf_render_params* p, float* scratch, gnerf_stream_t stream, const float*& absmax) {
    absmax = p->planes_absmax ? p->planes_absmax : scratch;
    return p->planes_absmax ? GNERF_OK : measure_absmax(p, scratch, stream);
}

}  // namespace gnerf

static_assert(kClampItemWord0 + 2 * kClampMaxItems <= kStatsWord0, "render words overlap the plane statistics");
extern "C" size_t gnerf_render_workspace_bytes(void) { return size_t(kWorkspaceWords) * 4; }

// gnerf_render_forward (pack = null) and gnerf_render_forward_packed.  Only the pipelined kernels read a pack; the generic kernel loads its
// weight fragments into registers as it always has.
static int render_forward_impl(const gnerf_render_params* p, const void* pack, gnerf_stream_t stream) {
    using namespace gnerf;
    Params P;
    if (int e = fill_params(p, P)) return e;
    P.decoder_pack = static_cast<const float*>(pack);
    if (!p->out_rgb || !p->out_depth || !p->out_wsum || !p->workspace)
        return fail(GNERF_E_ARG, "render: outputs and workspace must not be null");
    const int S = p->depth_resolution, F = p->depth_resolution_importance;
    const int64_t total = P.total_rays;
    hipStream_t s = as_stream(stream);
    // Small launches (one 64x64 frame of gen_videos.py is 256 ray tiles on 256 CUs): a workgroup walking its 16 rays one
    // after the other leaves most of the chip idle and the launch takes 16 ray latencies.  Split each tile over up to four
    // workgroups while that still fits the chip in one wave of workgroups.
    while (P.split_shift < 2 && (int64_t(P.n_tiles) << (P.split_shift + 1)) <= int64_t(kNumCU) * 4) P.split_shift++;
    const dim3 grid(((P.n_tiles << P.split_shift) + kNumXCD - 1) / kNumXCD * kNumXCD);        // (the generic kernel's: whole XCDs)
    // Kernel choice (GNERF_RENDER_KERNEL=pipe|generic forces one, for A/B runs):
    //   pipe    3 shader waves + 1 scalar wave, three rays in flight: up to 144+144 samples, importance sampling optional (1, 2 or 3 tiles per wave)
    //   generic one wave per ray: everything else (up to 256+256, or planes too large for 32-bit tap offsets)
    // A/B and test overrides, read per call (the parity tests switch kernels inside one process): a getenv is a walk of the
    // environment, ~0.1 us against the ~10 us of a launch
    const char* force = getenv("GNERF_RENDER_KERNEL");
    const char* force_mlp = getenv("GNERF_RENDER_MLP");                      // f16x3 | f32: overrides params.mlp_mode
    const char* verify = getenv("GNERF_VERIFY_ABSMAX");
    const int pipe_tp = pipe_tiles_per_wave(P);
    bool pipe = pipe_tp != 0 && planes_fit_32bit_taps(p);
    if (force && !strcmp(force, "generic")) pipe = false;
    if (force && !strcmp(force, "pipe") && !pipe) return fail(GNERF_E_UNSUPPORTED, "render: pipelined kernel does not cover %d+%d samples", S, F);
    // Decoder arithmetic of the pipelined kernel (the generic kernel is fp32 throughout).
    int mlp = p->mlp_mode;
    if (force_mlp && !strcmp(force_mlp, "f16x3")) mlp = GNERF_MLP_F16X3;
    if (force_mlp && !strcmp(force_mlp, "f32")) mlp = GNERF_MLP_F32;
    if (mlp != GNERF_MLP_AUTO && mlp != GNERF_MLP_F16X3 && mlp != GNERF_MLP_F32) return fail(GNERF_E_ARG, "render: mlp_mode %d is not one of GNERF_MLP_*", mlp);
    if (pipe && mlp == GNERF_MLP_AUTO) {
        // the choice is made on the device, by every workgroup for itself (no host round trip, graph-capturable): see choose_mlp
        float* own = reinterpret_cast<float*>(static_cast<int*>(p->workspace) + 5);
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s, &capturing);                   // (the check synchronises the stream: not inside a graph capture)
        if (p->planes_absmax && capturing == hipStreamCaptureStatusNone && verify && !strcmp(verify, "1")) {
            // debug aid (include/gnerf_hip.h, planes_absmax contract): is the caller's value an upper bound of THESE planes?
            if (int e = measure_absmax(p, own, stream)) return e;
            float mine = 0.f, theirs = 0.f;
            if (hipMemcpyAsync(&mine, own, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipMemcpyAsync(&theirs, p->planes_absmax, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess)
                return fail(GNERF_E_LAUNCH, "render: GNERF_VERIFY_ABSMAX could not read the plane statistics back");
            if (theirs < mine)                                  // (NaN on either side compares false: NaN planes / NaN bound both select fp32)
                return fail(GNERF_E_ARG, "render: planes_absmax = %g is smaller than max |planes| = %g of this call's planes (stale value?)", theirs, mine);
        }
        if (int e = absmax_or_measure(p, own, stream, P.absmax)) return e;
    }
    const bool gen = !p->ray_origins || p->rng_mode != GNERF_RNG_TENSORS;       // the call makes its rays and / or its draws in the kernel
    if (pipe) {
        const PipeLaunch L = pipe_launch(pipe_tp, pipe_seq_len(P));
        P.pipe_unit = L.unit;
        // Units are dealt on demand where workgroups get more than one (nothing to balance otherwise); clamp_depth_kernel, which
        // follows every forward launch on this stream, returns the counters to zero.  -DGNERF_PIPE_STATIC_DEALING (a variant build) and
        // GNERF_PIPE_DEALING=static (read per call, like the overrides above: the tests compare the two in one process) keep the static form.
        // On demand the units shrink towards the end of every XCD's range (the GUIDED schedule of pipe_dealing.h; the kernel derives the
        // level boundaries of its XCD from these two numbers and nothing else); GNERF_PIPE_DEALING=uniform keeps 8-ray units throughout,
        // GNERF_PIPE_DEALING=guided:<c>:<smallest unit, 1 or 2> is the A/B form of the constants.
#ifndef GNERF_PIPE_STATIC_DEALING
        if (L.fills_chip) {
            const char* dealing = getenv("GNERF_PIPE_DEALING");
            if (!dealing || strcmp(dealing, "static") != 0) {
                P.deal_counters = static_cast<unsigned*>(p->workspace) + kDealWord0;
                int c = kPipeGuidedC, smallest = kPipeGuidedMin;
                if (dealing && !strcmp(dealing, "uniform")) c = 0;
                else if (dealing && !strncmp(dealing, "guided:", 7)) {
                    if (sscanf(dealing + 7, "%d:%d", &c, &smallest) != 2 || c < 1 || c > 255 || (smallest != 1 && smallest != 2))
                        return fail(GNERF_E_ARG, "render: GNERF_PIPE_DEALING=%s is not guided:<c in 1..255>:<1 or 2>", dealing);
                }
                if (P.pipe_unit == 8) P.pipe_guided = c > 0 ? c + 256 * smallest : 0;
            }
        }
#endif
        // the instantiation with compile-time sample counts (render_pipe_body<.., FULL>) where the call fills the slots exactly
        bool full = S == 48 * pipe_tp && F == 48 * pipe_tp && !p->disparity_space_sampling && !p->ray_start_per_ray && !p->sigma_noise_coarse;
#if !defined(GNERF_STAMPS) && !defined(GNERF_WG_STAMPS)
        full = full && !p->debug;                               // (the timing builds' `debug` is their stamp buffer)
#endif
        if (const char* f = getenv("GNERF_PIPE_FULL")) full = full && strcmp(f, "0") != 0;       // A/B runs and the tests' cross-check
        if (gen && (!full || pipe_tp > 2))
            return fail(GNERF_E_UNSUPPORTED, "render: in-kernel rays / draws are built for 48+48 and 96+96 samples with plain stratified sampling (got %d+%d)", S, F);
        const int e = pipe_tp == 1 ? launch_pipe<1>(full, gen, mlp, L.grid, s, P)
                    : pipe_tp == 2 ? launch_pipe<2>(full, gen, mlp, L.grid, s, P) : launch_pipe<3>(full, gen, mlp, L.grid, s, P);
        if (e) return e;
    } else if (gen) {
        return fail(GNERF_E_UNSUPPORTED, "render: in-kernel rays / draws need the pipelined kernel (48+48 or 96+96 samples); got %d+%d", S, F);
    } else {
        const size_t lds_bytes = scratch_floats(16 * (P.tiles_c + P.tiles_f), P.tiles_c + P.tiles_f) * sizeof(float);
        if (lds_bytes > 160 * 1024) return fail(GNERF_E_ARG, "render: %d+%d samples need %zu bytes of LDS (> 160 KiB)", S, F, lds_bytes);
        static PerDeviceOnce once;
        if (int e = once.raise_lds(render_kernel_generic, "render")) return e;
        hipLaunchKernelGGL(render_kernel_generic, grid, dim3(64), lds_bytes, s, P);
        if (int e = check_launch("render_kernel_generic")) return e;
    }
    hipLaunchKernelGGL(clamp_depth_kernel, dim3((unsigned)((total + 256 * kClampPerThread - 1) / (256 * kClampPerThread))), dim3(256), 0, s,
                       p->out_depth, static_cast<unsigned*>(p->workspace), total, p->rays_per_item, p->depth_clamp_per_item ? p->n_items : 0);
    return check_launch("clamp_depth_kernel");
}

extern "C" int gnerf_render_forward(const gnerf_render_params* p, gnerf_stream_t stream) { return render_forward_impl(p, nullptr, stream); }

extern "C" int gnerf_render_forward_packed(const gnerf_render_params* p, const void* pack, gnerf_stream_t stream) {
    if (!pack) return gnerf::fail(GNERF_E_ARG, "render_forward_packed: pack is null (gnerf_render_forward is that call)");
    if (reinterpret_cast<uintptr_t>(pack) % 16 != 0) return gnerf::fail(GNERF_E_ARG, "render_forward_packed: pack must be 16-byte aligned");
    return render_forward_impl(p, pack, stream);
}
