// Fused tri-plane importance renderer for gfx950 (MI355X).
//
// One kernel does, per ray, everything ImportanceRenderer.forward does with a dozen whole-tensor PyTorch
// ops and ~4 GB of intermediates (reference training/volumetric_rendering/renderer.py:88-140,
// ray_marcher.py:25-57, triplane.py:113-136):
//
//   depth proposals -> tri-plane bilinear lookup -> 32->64->33 MLP -> coarse march -> importance
//   resampling -> fine lookup + MLP -> depth merge -> final composite.
//
// This file holds the pieces every kernel shares (depth proposals, importance resampling, the ray march, DPP scans),
// the GENERIC kernel described below (any sample count up to 256+256) and, from check_common down, the host half: the entry points, which
// choose each call's kernels.  The kernels that run G-NeRF's actual configurations are in the .inl files included further down:
//   render_pipe.inl   3 shader waves + 1 scalar wave per workgroup, three rays in flight: up to 144+144 samples
//   render_shade.inl  the 16-sample shade tile, decoder staging and plane taps the pipelined and backward kernels share
//   render_bwd.inl   the backward pass (plane + decoder gradients) of the renderer and of run_model
//
// Host half: fill_params validates a call and derives what every kernel reads; a handful of small helpers behind it hold the facts more
// than one launcher needs (tiles per wave, the pipelined launch's unit and grid, 32-bit tap offsets, max |planes|, the binned scatter's
// coverage, the padded ray sequence).  gnerf_render_forward picks generic or pipelined and launches through launch_pipe<TP, FULL, GEN>;
// render_backward_impl refuses, decides its route once (BwdRoute) and then launches from that decision alone; the three point queries
// share fill_query.  Every A/B override is an environment variable read once per call, where its launcher starts deciding.
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

#include "common.h"
#include "raygen.h"
#include "pipe_dealing.h"
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

using namespace gnerf;

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kHidden = 64;
constexpr int kStagePitch = 36;        // dwords per staged sample row (32 channels + pad)
constexpr int kRaysPerWave = 16;

struct Params {
    gnerf_render_params p;
    float box_scale;        // 2 / box_warp
    float delta;            // (ray_end - ray_start) / (S - 1)
    float inv_start, inv_end, disp_delta;
    int tiles_c, tiles_f;   // 16-sample MLP tiles
    int n_tiles;            // ray tiles in the grid
    int tiles_per_item, tiles_y;   // image tiling (0 when rays are not an image).  tiles_per_item == 0 with tiles_y > 0 (set by the staged backward
                            // of RAGGED calls only: several items, rays per item not a multiple of 16): every item's rays are padded to tiles_y,
                            // a multiple of 16, in the ray SEQUENCE, so that no 16-ray tile straddles items -- linear_pad() below.  (Kept in a
                            // field the forward already has: one more kernel argument cost the headline kernel eight spilled SGPRs.)
    int total_rays;
    int split_shift;        // small launches: a 16-ray tile is shared by 1 << split_shift workgroups (generic / backward kernels)
    int pipe_unit;          // pipelined kernel: rays dealt to a workgroup at a time (kPipeUnit; fewer for launches that do not fill the chip)
    int pipe_guided;        // pipelined forward, on demand with 8-ray units: c + 256 * (smallest unit) of the guided schedule (pipe_dealing.h), 0 = uniform units
    unsigned* deal_counters;        // pipelined forward: the workspace's per-XCD counters when units are dealt on demand, else null (static dealing)
    unsigned tex_pitch, row_pitch, plane_pitch;     // byte addressing of a texel, see plane_taps (render_shade.inl)
    int64_t item_bytes;     // bytes from one item's planes to the next: 3 * H * W * 128, or 0 when every item reads the same planes (planes_shared)
    const float* absmax;    // GNERF_MLP_AUTO: max |planes| (one device float) for choose_mlp
    TorchRandDraw draw_c, draw_f;   // rng_mode: the two draws torch's generator would have made (raygen.h)
    uint64_t draw_item_ctr;         // rng_per_item: Philox counter stride from one item's draws to the next (offset stride / 4)
    // staged backward on the pipelined path: floats per ray of the exchange / staging buffer and from one 16-rank tile's block to the
    // next (33 n_all and 512 when the blocks are the dX rows of the staged scatter; n_all + 32 tiles and 32 for a decoder-only request)
    int64_t bwd_ray_stride;
    int bwd_tile_pitch;
    const float* decoder_pack;      // pipelined forward: what gnerf_render_pack_decoder made of this call's decoder (statistics + LDS images, render_shade.inl), or null
};
__host__ __device__ __forceinline__ int linear_pad(const Params& P) { return P.tiles_per_item == 0 ? P.tiles_y : 0; }


// ---- order-preserving float <-> uint so that integer atomics give float min/max
__device__ __forceinline__ unsigned ord_encode(float f) {
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_decode(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// min / max / clamp of values that are known not to be NaN.  Kernels run in IEEE mode, where fminf / fmaxf on an operand of unknown
// origin cost a canonicalising `v_max x, x, x` next to the compare (16 per 16-sample tile in the softplus).  clamp_nn is one
// v_med3_f32.  For min / max two ways around the canonicalisation were tried and measured: fmed3(a, b, +-inf) -- the compiler folds it
// straight back into fmaxf / fminf -- and the bare instruction as inline assembly -- 16 instructions fewer per tile (384 -> 368) and
// no change in kernel time (0.54 ms either way, inside the run-to-run spread).  So these are plain fminf / fmaxf.
__device__ __forceinline__ float max_nn(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ float min_nn(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float clamp_nn(float x, float lo, float hi) { return __builtin_amdgcn_fmed3f(x, lo, hi); }

__device__ __forceinline__ float softplus_f(float x) {          // torch softplus, beta 1, threshold 20
    return x > 20.f ? x : log1pf(expf(x));
}
// MLP activations: these run once per hidden unit per sample, so they use the hardware exp2/log2.
__device__ __forceinline__ float softplus_fast(float x) {
    const float e = __expf(-fabsf(x));
    return fmaxf(x, 0.f) + __logf(1.f + e);
}
__device__ __forceinline__ float sigmoid_fast(float x) {
    return __frcp_rn(1.f + __expf(-x));
}

// ---- wave-wide scans on the DPP network (row_shr within 16-lane rows, then row_bcast:15 / :31 across rows).
// No LDS traffic and ALU latency only -- the ds_bpermute shuffles they replace cost an LDS round trip per step,
// and these scans sit on the per-ray critical path (transmittance product, cdf).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_mov(float old, float src) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), CTRL, ROW_MASK, 0xf, false));
}
// Round 6: every step is ONE instruction that reads and writes the same register -- `v_op_dpp v, v, v <shift>`: lanes the shift gives
// no source (and rows the row_mask leaves out) are simply not written, i.e. keep their own value, which is the scan's identity step.
// Written through update_dpp + an arithmetic instruction the compiler can only fold the full-mask row shifts of the sum (old = 0 is
// its bound_ctrl zero); every row_bcast step and every step of the product scan came out as v_mov (old) + v_mov_dpp + op: 10 / 18
// vector instructions per scan instead of 6, on the wave whose per-ray pass is 476 of them.
// The s_nop 1 are the two wait states a DPP read needs after the VALU write of its source; the compiler's hazard recogniser does not
// look inside (or behind) inline assembly, so the blocks begin and end with one as well.
#define GNERF_SCAN6(OP, ZF)                                                                 \
    "s_nop 1\n\t"                                                                           \
    OP " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf" ZF "\n\ts_nop 1\n\t"              \
    OP " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf" ZF "\n\ts_nop 1\n\t"              \
    OP " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf" ZF "\n\ts_nop 1\n\t"              \
    OP " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf" ZF "\n\ts_nop 1\n\t"              \
    OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"                 \
    OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"
__device__ __forceinline__ float wave_scan_add(float v, int /*lane*/) {         // inclusive
    asm(GNERF_SCAN6("v_add_f32_dpp", " bound_ctrl:1") : "+v"(v));
    return v;
}
__device__ __forceinline__ float wave_scan_mul(float v, int /*lane*/) {         // inclusive
    asm(GNERF_SCAN6("v_mul_f32_dpp", "") : "+v"(v));
    return v;
}
// two independent sums at once: the steps of one fill a wait state of the other
__device__ __forceinline__ void wave_scan_add2(float& a, float& b) {
#define GNERF_STEP2(CTRL)                                                       \
    "v_add_f32_dpp %0, %0, %0 " CTRL "\n\tv_add_f32_dpp %1, %1, %1 " CTRL "\n\ts_nop 0\n\t"
    asm("s_nop 1\n\t"
        GNERF_STEP2("row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        GNERF_STEP2("row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        GNERF_STEP2("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        GNERF_STEP2("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        GNERF_STEP2("row_bcast:15 row_mask:0xa bank_mask:0xf")
        GNERF_STEP2("row_bcast:31 row_mask:0xc bank_mask:0xf")
        "s_nop 0"
        : "+v"(a), "+v"(b));
#undef GNERF_STEP2
}
#undef GNERF_SCAN6
__device__ __forceinline__ float wave_last(float v) {                            // lane 63's value, in every lane
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_shift_up(float v, float first) {           // lane i <- lane i-1, lane 0 <- first
    return dpp_mov<0x138, 0xf>(first, v);
}
__device__ __forceinline__ float wave_sum(float v) { return wave_last(wave_scan_add(v, 0)); }

// exp / softplus on the hardware exp2/log2 units (about 1 ulp each; absolute error ~1e-7 on the values used here)
__device__ __forceinline__ float exp_hw(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
__device__ __forceinline__ float softplus_march(float x) {      // softplus with torch's threshold 20 (ray_marcher.py:33)
    const float e = __builtin_amdgcn_exp2f(-fabsf(x) * 1.44269504088896341f);
    const float sp = fmaf(__builtin_amdgcn_logf(1.0f + e), 0.693147180559945309f, fmaxf(x, 0.f));
    return x > 20.f ? x : sp;
}

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

// The per-lane weight fragments (see the layout notes above).
struct Weights {
    float a1[4][8];     // layer 1 A operand: W1[16m + (lane&15)][8*(lane>>4) + s]
    float b1[4][4];     // layer 1 bias as accumulator init: b1[16m + 4*(lane>>4) + r]
    float w2s[4][4];    // density row of layer 2: W2[0][16m + 4*(lane>>4) + r]
    float b2w[2][16];   // layer 2 B operand: W2[1 + 16n + (lane&15)][16m + 4*(lane>>4) + r]  (index m*4+r)
    float b2c[2];       // b2[1 + 16n + (lane&15)]
    float b2s;          // b2[0]
};

__device__ __forceinline__ void load_weights(Weights& w, const gnerf_render_params& p, int lane) {
    const int j = lane & 15, g = lane >> 4;
#pragma unroll
    for (int m = 0; m < 4; m++) {
#pragma unroll
        for (int s = 0; s < 8; s++) w.a1[m][s] = p.w1[(16 * m + j) * 32 + 8 * g + s];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            w.b1[m][r] = p.b1[16 * m + 4 * g + r];
            w.w2s[m][r] = p.w2[16 * m + 4 * g + r];
        }
    }
#pragma unroll
    for (int n = 0; n < 2; n++) {
#pragma unroll
        for (int k = 0; k < 16; k++) w.b2w[n][k] = p.w2[(1 + 16 * n + j) * kHidden + 16 * (k >> 2) + 4 * g + (k & 3)];
        w.b2c[n] = p.b2[1 + 16 * n + j];
    }
    w.b2s = p.b2[0];
}

// Bilinear lookup of one plane for this lane's sample; adds (weight * 4 channels) into acc.
// u indexes W, v indexes H (grid_sample, align_corners=False, zero padding; renderer.py:64).
__device__ __forceinline__ void lookup_plane(v4f& acc, const float* __restrict__ plane, int H, int W, unsigned tex_q, unsigned row_q, float u, float v, int cq) {
    // tex_q / row_q: texel and row pitch in 16-byte units
    float ix = ((u + 1.f) * float(W) - 1.f) * 0.5f;
    float iy = ((v + 1.f) * float(H) - 1.f) * 0.5f;
    ix = fminf(fmaxf(ix, -1.5f), float(W) + 0.5f);     // keeps "everything out of range" out of range, and int conversion safe
    iy = fminf(fmaxf(iy, -1.5f), float(H) + 0.5f);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float fx = ix - x0f, fy = iy - y0f;
    const int x0 = int(x0f), y0 = int(y0f), x1 = x0 + 1, y1 = y0 + 1;
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W, vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
    const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x1, 0), W - 1);
    const int cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y1, 0), H - 1);
    const float w00 = (vx0 && vy0) ? (1.f - fx) * (1.f - fy) : 0.f;
    const float w01 = (vx1 && vy0) ? fx * (1.f - fy) : 0.f;
    const float w10 = (vx0 && vy1) ? (1.f - fx) * fy : 0.f;
    const float w11 = (vx1 && vy1) ? fx * fy : 0.f;
    const v4f* base = reinterpret_cast<const v4f*>(plane) + cq;
    const v4f t00 = base[cy0 * row_q + cx0 * tex_q];
    const v4f t01 = base[cy0 * row_q + cx1 * tex_q];
    const v4f t10 = base[cy1 * row_q + cx0 * tex_q];
    const v4f t11 = base[cy1 * row_q + cx1 * tex_q];
    acc += t00 * w00 + t01 * w01 + t10 * w10 + t11 * w11;
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

// Stratified depth proposal k of a ray (renderer.py:169-192); bit-exact with torch's linspace + jitter.
__device__ __forceinline__ float coarse_depth(const Params& P, int64_t ray, int k) {
    const gnerf_render_params& p = P.p;
    const int S = p.depth_resolution;
    const float u = p.noise_coarse[ray * S + k];
    if (p.disparity_space_sampling) {
        const float step = 1.0f / float(S - 1);
        const float lin = (k < S / 2) ? __fmul_rn(step, float(k)) : __fsub_rn(1.0f, __fmul_rn(step, float(S - 1 - k)));
        const float q = __fadd_rn(lin, __fmul_rn(u, P.disp_delta));
        return __fdiv_rn(1.0f, __fadd_rn(__fmul_rn(P.inv_start, __fsub_rn(1.0f, q)), __fmul_rn(P.inv_end, q)));
    }
    if (p.ray_start_per_ray) {
        const float rs = p.ray_start_per_ray[ray], re = p.ray_end_per_ray[ray];
        const float span = __fsub_rn(re, rs);
        const float lin = __fadd_rn(rs, __fmul_rn(__fdiv_rn(float(k), float(S - 1)), span));      // math_utils.py:107-116
        return __fadd_rn(lin, __fmul_rn(u, __fdiv_rn(span, float(S - 1))));
    }
    const float step = __fdiv_rn(__fsub_rn(p.ray_end, p.ray_start), float(S - 1));            // torch.linspace
    const float lin = (k < S / 2) ? __fadd_rn(p.ray_start, __fmul_rn(step, float(k)))
                                  : __fsub_rn(p.ray_end, __fmul_rn(step, float(S - 1 - k)));
    return __fadd_rn(lin, __fmul_rn(u, P.delta));
}

// Importance resampling (renderer.py:194-253): fine depths from the coarse interval weights w[0..S-2].
// n_w = S-3 pdf entries, cdf has n_w+1.  `pdf_tmp` is scratch of >= S floats; `sync` separates the phases.
template <typename Sync>
__device__ __forceinline__ void resample_fine(const Params& P, int64_t ray, const float* t_c, const float* w, float* pdf_tmp, float* cdf,
                                              float* t_f, float* dbg, int n_all, int lane, Sync sync) {
    const gnerf_render_params& p = P.p;
    const int S = p.depth_resolution, F = p.depth_resolution_importance;
    const int n_w = S - 3;
    float part = 0.f;
    for (int i = lane; i < n_w; i += 64) {
        // smoothed weight a_{i+1} = (max(w_i, w_{i+1}) + max(w_{i+1}, w_{i+2})) / 2 + 0.01, then + 1e-5
        const float w0 = w[i], w1 = w[i + 1], w2 = w[i + 2];
        const float a = (fmaxf(w0, w1) + fmaxf(w1, w2)) * 0.5f + 0.01f;
        const float pw = a + 1e-5f;
        pdf_tmp[i] = pw;
        part += pw;
    }
    const float total = wave_sum(part);
    sync();
    float carry = 0.f;
    for (int base = 0; base < n_w; base += 64) {
        const int i = base + lane;
        const float pdf = (i < n_w) ? pdf_tmp[i] / total : 0.f;
        const float incl = wave_scan_add(pdf, lane) + carry;
        if (i < n_w) cdf[i + 1] = incl;
        carry = wave_last(incl);
    }
    if (lane == 0) cdf[0] = 0.f;
    sync();
    for (int i = lane; i < F; i += 64) {
        const float u = p.noise_fine[ray * F + i];
        // searchsorted(cdf[0..n_w], u, right=True): number of entries <= u
        int lo = 0, hi = n_w + 1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (cdf[mid] <= u) lo = mid + 1; else hi = mid; }
        const int below = max(lo - 1, 0), above = min(lo, n_w);
        const float cb = cdf[below], ca = cdf[above];
        const float bb = (t_c[below] + t_c[below + 1]) * 0.5f;
        const float ba = (t_c[above] + t_c[above + 1]) * 0.5f;
        float denom = ca - cb;
        if (denom < 1e-5f) denom = 1.f;
        const float d = bb + (u - cb) / denom * (ba - bb);
        t_f[i] = d;
        if (dbg) dbg[GNERF_DBG_DEPTH_FINE * n_all + i] = d;
    }
    sync();
}

// Merge by depth (renderer.py:157-167): rank = number of elements ordered before this one, ties broken by
// position in cat([coarse, fine]) like a stable sort.  Writes rank_e and the sorted depth / density arrays.
__device__ __forceinline__ void merge_by_depth(const float* t_e, const float* sig_e, int* rank_e, float* s_t, float* s_sig,
                                               int S, int F, int fine_e0, int lane) {
    const int n_all = S + F;
    for (int q = lane; q < n_all; q += 64) {
        const int e = q < S ? q : fine_e0 + (q - S);
        const float key = t_e[e];
        int rank = 0;
        for (int o = 0; o < S; o++) { const float tk = t_e[o]; rank += (tk < key || (tk == key && o < q)) ? 1 : 0; }
        for (int o = 0; o < F; o++) { const float tk = t_e[fine_e0 + o]; rank += (tk < key || (tk == key && S + o < q)) ? 1 : 0; }
        rank_e[e] = rank;
        s_t[rank] = key;
        s_sig[rank] = sig_e[e];
    }
}

// Ray-march weights over n sorted samples (depth/density in LDS): writes w[0..n-2], returns sum(w) and
// sum(w * t_mid) in all lanes.  ray_marcher.py:26-42.
__device__ __forceinline__ void march(const float* t, const float* sig, float* w, int n, int lane, float& w_sum, float& wt_sum) {
    float carry = 1.f, acc_w = 0.f, acc_wt = 0.f;
    for (int base = 0; base < n - 1; base += 64) {
        const int k = base + lane;
        const bool ok = k < n - 1;
        float alpha = 0.f, tmid = 0.f;
        if (ok) {
            const float t0 = t[k], t1 = t[k + 1];
            const float delta = t1 - t0;
            const float smid = softplus_march((sig[k] + sig[k + 1]) * 0.5f - 1.f);
            tmid = (t0 + t1) * 0.5f;
            alpha = 1.f - exp_hw(-(smid * delta));
        }
        const float x = ok ? (1.f - alpha + 1e-10f) : 1.f;
        const float incl = wave_scan_mul(x, lane);
        const float excl = wave_shift_up(incl, 1.f);
        const float wk = alpha * (excl * carry);
        carry *= wave_last(incl);
        if (ok) { w[k] = wk; acc_w += wk; acc_wt += wk * tmid; }
    }
    wave_scan_add2(acc_w, acc_wt);
    w_sum = wave_last(acc_w);
    wt_sum = wave_last(acc_wt);
}

// ---- the call-wide depth range (ray_marcher.py:49-50).
// Workspace words: [0] ~ord_encode(min depth)  [1] ord_encode(max depth)  [3] clamp blocks finished;
// [kDealWord0 + 32 x]: units of XCD x's range dealt on demand by the pipelined kernel (render_pipe.inl).
// ALL ZERO means idle ("min = +inf, max = -inf"): the caller provides a zeroed workspace once and every call leaves it
// zeroed (clamp_depth_kernel's last block), so no launch is spent on initialising it.
// (Also tried: letting the last render workgroup to finish apply the clamp itself for small launches, to save the second
// launch -- the device-scope fences that needs at the end of every workgroup cost more than the launch: 86 -> 118 us per
// 64x64-ray frame.)
// depth_clamp_per_item: one (min, max) pair per item at words [16 + 2 item], [17 + 2 item] instead of the call-wide pair.
constexpr int kClampItemWord0 = 16, kClampMaxItems = 4096;
__device__ __forceinline__ void publish_depth_range(const Params& P, float blk_min, float blk_max, int item = 0) {
    unsigned* ws = static_cast<unsigned*>(P.p.workspace) + (P.p.depth_clamp_per_item ? kClampItemWord0 + 2 * item : 0);
    atomicMax(ws + 0, ~ord_encode(blk_min));
    atomicMax(ws + 1, ord_encode(blk_max));
}
// A workgroup's running depth range, published per item when the clamp is per item (a workgroup's rays may span items).
struct DepthRange {
    float mn = INFINITY, mx = -INFINITY;
    int item = -1;
    __device__ __forceinline__ void add(const Params& P, int it, float lo, float hi) {
        if (P.p.depth_clamp_per_item && it != item) { flush(P); item = it; }
        mn = fminf(mn, lo); mx = fmaxf(mx, hi);
    }
    __device__ __forceinline__ void flush(const Params& P) {
        if (mn <= mx) publish_depth_range(P, mn, mx, item < 0 ? 0 : item);
        mn = INFINITY; mx = -INFINITY;
    }
};

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

// ---- GNERF_MLP_AUTO: which decoder arithmetic may this call use?  Evaluated by every workgroup of the pipelined kernels before
// it stages the decoder: no separate launch.  Not free, though: stamped (profiles/r14_wg_prologue.json), a workgroup's way from its start to
// its first shader tile -- this choice, the decoder's way into LDS, the first ray's proposals -- took 12.0 us of a 486 us life at config 2
// (2.5 %, where a comment here used to say "~0.1 %") and 11.4 of 87 us on a 64x64 frame at 96+96.  With a decoder pack (below) it takes
// 3.4 and 3.0 us.  Without one (plain C ABI callers, the backward) everything runs as it did.
// The f16 hi/lo split (render_shade.inl) represents an operand v as hi + lo with |v - hi - lo| <= max(2^-22 |v|, 2^-25): fp32-grade
// for operands well inside f16's range, but an ABSOLUTE 2^-25 per operand once the low half goes subnormal, and inf/NaN once the high
// half overflows.  With A = max |planes| (the features are convex combinations of texels, so |x| <= A), W1' = log2(e) W1 and the
// row norms R1 = max_r ||W1'[r,:]||_2, R2 = max_r ||W2[r,:]||_2 the decision is
//   no overflow (hard bounds):  A, max |W1'|, max |W2|, and  max_r ||W1'[r,:]||_1 A + max |b1'| + 1  (>= every hidden activation) <= 30000
//   accuracy (random-sign error model, the same one that gives the fp32 reference its ~2^-24 sqrt(n) behaviour):
//     e_p = 2^-22 R1 A + 2^-25 (R1 + sqrt(32) A)                       error of a layer-1 pre-activation (base-2 scaled)
//     h   = R1 A + max |b1'| + 1                                        scale of the hidden activations
//     e_o = R2 e_p + 2^-22 R2 h + 2^-25 (R2 + 8 h)                      error of a layer-2 output
//   f16x3 iff e_o <= 2^-12: |d rgb| <= 0.25 ln2 e_o = 4e-5 in the worst case (pixel MSE < 2e-9), typically 1e-3 of that.
// Anything else -- including NaN/inf anywhere in the operands -- takes the exact-fp32 arithmetic.  BASELINE config 2 (randn planes,
// default-init decoder) has e_o = 1.1e-5; planes scaled by ~20 or decoder weights by ~5 cross over to fp32.
constexpr float kMlpRangeLimit = 30000.f;
constexpr float kMlpErrLimit = 1.0f / 4096.f;
// ... and the f16 body's softplus may take its short form log2(1 + 2^p') -- exp2, add, log2 instead of exp2, add, log2, add, max per
// hidden activation -- while no base-2 pre-activation can reach exp2's overflow: |p'| <= max_r ||W1'[r,:]||_1 A + max |b1'| <= 99
// (config 2: 37; on a random-init generator's planes: 57).  Beyond that the body keeps the form that is safe for any p'.
constexpr float kSoftplusDirectLimit = 100.f;
// The decision is made from eight statistics of the decoder and max |planes|.  The statistics depend on the decoder alone: a decoder pack
// (gnerf_render_pack_decoder, below) holds them ready-made, next to the two LDS images of the weights; without a pack every workgroup
// reduces them itself (choose_mlp, as it always has).  Either way mlp_decide evaluates the same inequalities on the same numbers.
constexpr int kStatL1 = 0, kStatSq1 = 1, kStatMx1 = 2, kStatSq2 = 3, kStatMx2 = 4, kStatMb1 = 5, kStatMb2 = 6, kStatBad = 7, kStatBad2 = 8;
constexpr int kStatFloats = 16;         // the pack's first 64 bytes ([kStatBad]: an int, either wave's flag); in the pack kernel, the LDS words in front of decoder_stats' rows
struct DecoderStats { float l1, sq1, mx1, sq2, mx2, mb1, mb2; bool bad; };
__device__ __forceinline__ void mlp_decide(const DecoderStats& s, float A, int& choice, int& direct) {
    const float R1 = sqrtf(s.sq1), R2 = sqrtf(s.sq2);
    const float h_hard = s.l1 * A + s.mb1 + 1.f;
    const float e_p = 0x1p-22f * R1 * A + 0x1p-25f * (R1 + 5.657f * A);
    const float h = R1 * A + s.mb1 + 1.f;
    const float e_o = R2 * e_p + 0x1p-22f * R2 * h + 0x1p-25f * (R2 + 8.f * h);
    const bool ok = !s.bad && A <= kMlpRangeLimit && s.mx1 <= kMlpRangeLimit && s.mx2 <= kMlpRangeLimit && h_hard <= kMlpRangeLimit
                    && s.mb2 <= kMlpRangeLimit && e_o <= kMlpErrLimit;         // every comparison is false for NaN
    choice = ok ? 1 : 2;                                                       // kMlpF16x3 : kMlpF32
    direct = (ok && h_hard <= kSoftplusDirectLimit) ? 1 : 0;
}
// The per-row sums, ONE copy for choose_mlp and for the pack kernel: a lane sums its row in column order with every operation pinned --
// the scaling a multiply of its own, the L1 sum plain adds, the squares fused -- so that no contraction can make two call sites round
// differently (tests/decoder_pack_ref.py restates exactly this; the GPU test compares the pack's statistics with it bit for bit).
constexpr int kStatP1 = 33, kStatP2 = 65;      // LDS pitches of the staged rows (odd: the row sums are conflict-free)
__device__ __forceinline__ void w1_row_stats(const float* s1, int row, float& l1, float& sq1, float& mx1) {
    constexpr float kL2e = 1.44269504088896341f;
    l1 = 0.f; sq1 = 0.f; mx1 = 0.f;
#pragma unroll 8
    for (int c = 0; c < 32; c++) { const float w = __fmul_rn(fabsf(s1[row * kStatP1 + c]), kL2e); l1 = __fadd_rn(l1, w); sq1 = __fmaf_rn(w, w, sq1); mx1 = fmaxf(mx1, w); }
}
__device__ __forceinline__ void w2_row_stats(const float* s2, int row, float& sq2, float& mx2) {
#pragma unroll 8
    for (int c = 0; c < 64; c++) { const float w = fabsf(s2[row * kStatP2 + c]); sq2 = __fmaf_rn(w, w, sq2); mx2 = fmaxf(mx2, w); }
}
__device__ __forceinline__ float bias_stat(float b) { return __fmul_rn(fabsf(b), 1.44269504088896341f); }
// The pack kernel's reduction: the eight statistics into smem[0 .. kStatFloats) (all threads of a workgroup of at least two waves; a barrier
// must follow before they are read).  Wave 0 sums the rows of W1, wave 1 the rows of W2, side by side, with the routines choose_mlp's one
// wave uses; the maxima over the rows do not depend on an order.
__device__ __forceinline__ void decoder_stats(const gnerf_render_params& p, float* smem) {
    constexpr int kP1 = kStatP1, kP2 = kStatP2;
    float* s1 = smem + kStatFloats;
    float* s2 = s1 + 64 * kP1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float mb = 0.f;
    if (wave == 0) mb = bias_stat(p.b1[lane]);
    else if (wave == 1 && lane < 33) mb = bias_stat(p.b2[lane]);
    for (int i = threadIdx.x; i < 64 * 32; i += blockDim.x) s1[(i >> 5) * kP1 + (i & 31)] = p.w1[i];
    for (int i = threadIdx.x; i < 33 * 64; i += blockDim.x) s2[(i >> 6) * kP2 + (i & 63)] = p.w2[i];
    __syncthreads();
    if (wave == 0) {                // lane r: row r of W1
        float l1, sq1, mx1;
        w1_row_stats(s1, lane, l1, sq1, mx1);
        // NaN-propagating maxima: fmaxf drops NaNs, so carry "anything not finite" separately
        bool bad = !(l1 < INFINITY) || !(mb < INFINITY);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            l1 = fmaxf(l1, __shfl_xor(l1, o)); sq1 = fmaxf(sq1, __shfl_xor(sq1, o)); mx1 = fmaxf(mx1, __shfl_xor(mx1, o));
            mb = fmaxf(mb, __shfl_xor(mb, o));
        }
        bad = __any(bad);
        if (lane == 0) { smem[kStatL1] = l1; smem[kStatSq1] = sq1; smem[kStatMx1] = mx1; smem[kStatMb1] = mb; reinterpret_cast<int*>(smem)[kStatBad] = bad ? 1 : 0; }
    } else if (wave == 1) {         // lane r < 33: row r of W2
        float sq2 = 0.f, mx2 = 0.f;
        if (lane < 33) w2_row_stats(s2, lane, sq2, mx2);
        bool bad = !(sq2 < INFINITY) || !(mb < INFINITY);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sq2 = fmaxf(sq2, __shfl_xor(sq2, o)); mx2 = fmaxf(mx2, __shfl_xor(mx2, o)); mb = fmaxf(mb, __shfl_xor(mb, o));
        }
        bad = __any(bad);
        if (lane == 0) { smem[kStatSq2] = sq2; smem[kStatMx2] = mx2; smem[kStatMb2] = mb; reinterpret_cast<int*>(smem)[kStatBad2] = bad ? 1 : 0; }
    }
}
// `stats`: the kStatFloats words at the head of a pack (wave-uniform loads); every thread evaluates the decision for itself.
__device__ __forceinline__ int mlp_choice_from(const float* stats, float A, bool* softplus_direct) {
    DecoderStats s;
    s.l1 = stats[kStatL1]; s.sq1 = stats[kStatSq1]; s.mx1 = stats[kStatMx1]; s.sq2 = stats[kStatSq2]; s.mx2 = stats[kStatMx2];
    s.mb1 = stats[kStatMb1]; s.mb2 = stats[kStatMb2];
    const int* flags = reinterpret_cast<const int*>(stats);
    s.bad = flags[kStatBad] != 0;
    int choice, direct;
    mlp_decide(s, A, choice, direct);
    if (softplus_direct) *softplus_direct = __builtin_amdgcn_readfirstlane(direct) != 0;
    return __builtin_amdgcn_readfirstlane(choice);
}
__device__ __forceinline__ void note_mlp_choice(const Params& P, int choice) {         // diagnostics (gnerf_hip.last_mlp_choice)
    if (blockIdx.x == 0 && threadIdx.x == 0 && P.p.workspace) static_cast<int*>(P.p.workspace)[4] = choice;
}
__device__ __forceinline__ int choose_mlp(const Params& P, float* smem, bool* softplus_direct = nullptr) {
    const gnerf_render_params& p = P.p;
    // the decoder into LDS with coalesced loads (rows padded to an odd pitch: the row sums below are conflict-free); a first
    // version read the rows straight from global memory, one row per lane -- 96 uncoalesced load instructions in front of every
    // workgroup's first ray cost 40 us per launch
    constexpr int kP1 = kStatP1, kP2 = kStatP2;
    float* s1 = smem + 4;
    float* s2 = s1 + 64 * kP1;
    for (int i = threadIdx.x; i < 64 * 32; i += blockDim.x) s1[(i >> 5) * kP1 + (i & 31)] = p.w1[i];
    for (int i = threadIdx.x; i < 33 * 64; i += blockDim.x) s2[(i >> 6) * kP2 + (i & 63)] = p.w2[i];
    __syncthreads();
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        // lane r < 64: row r of W1; lane r < 33: row r of W2
        float l1, sq1, mx1;
        w1_row_stats(s1, lane, l1, sq1, mx1);
        float sq2 = 0.f, mx2 = 0.f;
        if (lane < 33) w2_row_stats(s2, lane, sq2, mx2);
        float mb1 = bias_stat(p.b1[lane]);
        float mb2 = lane < 33 ? bias_stat(p.b2[lane]) : 0.f;
        // NaN-propagating maxima: fmaxf drops NaNs, so carry "anything not finite" separately
        bool bad = !(l1 < INFINITY) || !(sq2 < INFINITY) || !(mb1 < INFINITY) || !(mb2 < INFINITY);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            l1 = fmaxf(l1, __shfl_xor(l1, o)); sq1 = fmaxf(sq1, __shfl_xor(sq1, o)); mx1 = fmaxf(mx1, __shfl_xor(mx1, o));
            sq2 = fmaxf(sq2, __shfl_xor(sq2, o)); mx2 = fmaxf(mx2, __shfl_xor(mx2, o));
            mb1 = fmaxf(mb1, __shfl_xor(mb1, o)); mb2 = fmaxf(mb2, __shfl_xor(mb2, o));
        }
        bad = __any(bad);
        if (lane == 0) {
            DecoderStats s;
            s.l1 = l1; s.sq1 = sq1; s.mx1 = mx1; s.sq2 = sq2; s.mx2 = mx2; s.mb1 = mb1; s.mb2 = mb2; s.bad = bad;
            int choice, direct;
            mlp_decide(s, *P.absmax, choice, direct);
            reinterpret_cast<int*>(smem)[0] = choice;
            reinterpret_cast<int*>(smem)[1] = direct;
            if (blockIdx.x == 0 && p.workspace) static_cast<int*>(p.workspace)[4] = choice;         // diagnostics (gnerf_hip.last_mlp_choice)
        }
    }
    __syncthreads();
    const int choice = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(smem)[0]);
    if (softplus_direct) *softplus_direct = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(smem)[1]) != 0;
    __syncthreads();                                     // smem is the body's from here on
    return choice;
}
// With a decoder pack there is nothing to stage or reduce: nine wave-uniform words and the inequalities, no LDS, no barrier.
__device__ __forceinline__ int choose_mlp_packed(const Params& P, bool* softplus_direct) {
    const int choice = mlp_choice_from(P.decoder_pack, *P.absmax, softplus_direct);
    note_mlp_choice(P, choice);
    return choice;
}

#include "render_shade.inl"
#include "render_pipe.inl"
#include "render_bwd.inl"
#include "query_grad.inl"
#include "project_level.inl"
#include "render_ray_grad.inl"

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

#include "scatter_binned.inl"

}  // namespace

static_assert(kClampItemWord0 + 2 * kClampMaxItems <= kStatsWord0, "render words overlap the plane statistics");
extern "C" size_t gnerf_render_workspace_bytes(void) { return size_t(kWorkspaceWords) * 4; }

// Validation and derived launch parameters shared by the forward and backward entry points.
static int fill_params(const gnerf_render_params* p, Params& P) {
    using namespace gnerf;
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

// ---- facts that more than one launcher below needs, each worked out in one place
// (the pipelined, backward and query-gradient kernels address plane taps with 32-bit byte offsets)
static bool planes_fit_32bit_taps(const gnerf_render_params* p) { return int64_t(p->plane_h) * p->plane_w * 3 * 128 < (int64_t(1) << 32); }
// 16-sample tiles per shader wave and pass of the pipelined kernels (render_pipe.inl), 0 where they do not cover the sample counts
static int pipe_tiles_per_wave(const Params& P) {
    const int t = P.tiles_c > P.tiles_f ? P.tiles_c : P.tiles_f;
    return t <= 3 ? 1 : (t <= 6 ? 2 : (t <= 9 ? 3 : 0));
}
// resident workgroups per CU for that count (the kernels' __launch_bounds__)
static int pipe_workgroups_per_cu(int tp) { return tp == 1 ? GNERF_PIPE_WAVES_PER_SIMD : (tp == 2 ? GNERF_PIPE2_WAVES_PER_SIMD : 2); }
// positions of the ray sequence the pipelined kernels walk: whole 16-ray tiles where the rays are tiled or padded
static int64_t pipe_seq_len(const Params& P) { return (P.tiles_per_item > 0 || linear_pad(P) > 0) ? int64_t(P.n_tiles) * 16 : int64_t(P.total_rays); }
// Dealing unit and grid of a pipelined launch (the forward's, the backward's first pass).  One dealing unit per workgroup until the chip
// is full: a small launch is latency-bound, and the three half-steps of pipeline fill cost less than leaving compute units idle (64x64
// rays: 167 -> 70 us); the unit shrinks from 8 rays down to what spreads the launch over every resident workgroup slot (a 64x64 frame:
// 4 rays each on pipe<1>, 6 on pipe<2>).
struct PipeLaunch { int unit; unsigned grid; bool fills_chip; };
static PipeLaunch pipe_launch(int tp, int64_t total_seq) {
    using namespace gnerf;
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
// what choose_mlp reads: the caller's planes_absmax, else measured into `scratch`
static int absmax_or_measure(const gnerf_render_params* p, float* scratch, gnerf_stream_t stream, const float*& absmax) {
    absmax = p->planes_absmax ? p->planes_absmax : scratch;
    return p->planes_absmax ? GNERF_OK : measure_absmax(p, scratch, stream);
}
// The binned scatter (scatter_binned.inl) indexes the staging buffer with 32 bits and keeps an item's plane-tile histogram in LDS.
static bool binned_scatter_covers(const Params& P) {
    const gnerf_render_params& p = P.p;
    return int64_t(P.total_rays) * (p.depth_resolution + p.depth_resolution_importance) * 33 < (int64_t(1) << 32) &&
           (2 * size_t(3) * ((p.plane_h + kBinTile - 1) / kBinTile) * ((p.plane_w + kBinTile - 1) / kBinTile) + 128) * 4 <= 150 * 1024;
}
// A ragged call (several items whose ray count is no multiple of 16): the ray SEQUENCE pads every item to whole 16-ray tiles, so that no
// tile straddles items (linear_pad(P); pipe_seq_to_ray / bin_tile_ray answer -1 for the padding, which every kernel of the path skips).
static int padded_rays_per_item(const gnerf_render_params& p) { return (p.rays_per_item + kBwdRaysPerWave - 1) / kBwdRaysPerWave * kBwdRaysPerWave; }
static void pad_ray_sequence(Params& P) {
    P.tiles_y = padded_rays_per_item(P.p);                      // (tiles_per_item == 0 for such a call)
    P.n_tiles = P.p.n_items * (P.tiles_y / kBwdRaysPerWave);
}

// One pipelined forward launch.  These are all the instantiations of render_kernel_pipe: GEN (in-kernel rays / draws) is built with FULL
// for TP 1 and 2 and for nothing else.  TP = 3 takes 65 KB of LDS, above the default dynamic limit.
template <int TP, bool FULL, bool GEN>
static int launch_pipe(int mlp, unsigned grid, hipStream_t s, const Params& P) {
    static_assert(!GEN || (FULL && TP <= 2), "in-kernel rays / draws: 48+48 and 96+96 samples only");
    void (*kernel)(Params) = render_kernel_pipe<TP, kMlpAuto, FULL, GEN>;
    if (mlp == kMlpF16x3) kernel = render_kernel_pipe<TP, kMlpF16x3, FULL, GEN>;
    if (mlp == kMlpF32) kernel = render_kernel_pipe<TP, kMlpF32, FULL, GEN>;
    if constexpr (TP == 3) {
        static_assert(kMlpAuto == 0 && kMlpF16x3 == 1 && kMlpF32 == 2, "once[] is indexed by the MLP mode");
        static gnerf::PerDeviceOnce once[3];                    // one per kernel of this instantiation (mlp is one of the three: checked by the caller)
        if (int e = once[mlp].raise_lds(kernel, "render")) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPipeThreads), pipe_lds_floats(TP, mlp) * sizeof(float), s, P);
    return gnerf::check_launch("render_kernel_pipe");
}

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
        int e;
        if (gen) e = pipe_tp == 1 ? launch_pipe<1, true, true>(mlp, L.grid, s, P) : launch_pipe<2, true, true>(mlp, L.grid, s, P);
        else if (pipe_tp == 1) e = full ? launch_pipe<1, true, false>(mlp, L.grid, s, P) : launch_pipe<1, false, false>(mlp, L.grid, s, P);
        else if (pipe_tp == 2) e = full ? launch_pipe<2, true, false>(mlp, L.grid, s, P) : launch_pipe<2, false, false>(mlp, L.grid, s, P);
        else e = full ? launch_pipe<3, true, false>(mlp, L.grid, s, P) : launch_pipe<3, false, false>(mlp, L.grid, s, P);
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

extern "C" size_t gnerf_render_decoder_pack_bytes(void) { return size_t(kPackFloats) * sizeof(float); }

extern "C" int gnerf_render_pack_decoder(const float* w1, const float* b1, const float* w2, const float* b2, void* pack, gnerf_stream_t stream) {
    using namespace gnerf;
    if (!w1 || !b1 || !w2 || !b2 || !pack) return fail(GNERF_E_ARG, "render_pack_decoder: null pointer");
    if (reinterpret_cast<uintptr_t>(pack) % 16 != 0) return fail(GNERF_E_ARG, "render_pack_decoder: pack must be 16-byte aligned");
    gnerf_render_params p = {};
    p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2;
    hipLaunchKernelGGL(pack_decoder_kernel, dim3(1), dim3(kPipeThreads), 0, as_stream(stream), p, static_cast<float*>(pack));
    return check_launch("pack_decoder_kernel");
}

// What one backward call launches: decided once in render_backward_impl, then only read (DESIGN.md 3.2 has the table of routes).
struct BwdRoute {
    // first pass.  Wave: render_bwd_kernel<false / true>, one wave per ray, float atomics into the plane gradient / dX rows into the staging buffer.
    // Piped: render_kernel_pipe_bwd + render_bwd_tiles_kernel, dX rows into the staging buffer / a decoder-only request's exchange buffer (no dX rows)
    enum First { kWaveDirect, kWaveStaged, kPipedRows, kPipedExchange } first;
    enum Second { kNoScatter, kBinned, kSorted } second;       // dX rows -> plane gradient: scatter_binned.inl or plane_scatter_kernel
    bool padded;            // every kernel of the call walks the padded ray sequence (pad_ray_sequence)
    bool scatter_padded;    // only the scatter does: the first pass stages by ray whatever the tiling
    int mlp_first, mlp_tiles;       // decoder arithmetic of the two piped kernels (GNERF_MLP_*)
};

// gnerf_render_backward, and with grad_origins / grad_dirs gnerf_render_backward_rays: the same launches, plus render_ray_grad_kernel between
// the first pass and the scatter.  Three parts: (a) what the call refuses, (b) its route, decided once, (c) the launches, which read that
// decision and nothing else and build each kernel's Params from P and it.
static int render_backward_impl(const gnerf_render_params* p, const gnerf_render_grads* g_in, float* grad_origins, float* grad_dirs, gnerf_stream_t stream) {
    using namespace gnerf;
    // ---- (a) refusals
    Params P;
    if (int e = fill_params(p, P)) return e;
    if (!g_in) return fail(GNERF_E_ARG, "render_backward: grads is null");
    const bool need_rays = grad_origins != nullptr || grad_dirs != nullptr;
    const bool want_planes = g_in->grad_planes_nhwc != nullptr;
    // A ray request needs the dX rows of the staged first pass whether or not a plane gradient is made from them.  The first-pass kernels
    // only TEST grad_planes_nhwc (the staged forms never write through it), so a ray-only request hands them the staging buffer's address
    // in its place, and there is no scatter.
    gnerf_render_grads g_eff = *g_in;
    if (need_rays && !want_planes) g_eff.grad_planes_nhwc = g_in->scatter_stage;
    const gnerf_render_grads* g = &g_eff;
    if (p->planes_shared) return fail(GNERF_E_UNSUPPORTED, "render_backward: planes_shared is a forward-only option");
    if (!p->ray_origins || p->rng_mode != GNERF_RNG_TENSORS) return fail(GNERF_E_UNSUPPORTED, "render_backward: in-kernel rays / draws are forward-only options");
    if (p->sigma_noise_coarse || p->sigma_noise_fine) return fail(GNERF_E_UNSUPPORTED, "render_backward: density noise is a forward-only option");
    const int n_dec = (g->grad_w1 != nullptr) + (g->grad_b1 != nullptr) + (g->grad_w2 != nullptr) + (g->grad_b2 != nullptr);
    if (n_dec != 0 && n_dec != 4) return fail(GNERF_E_ARG, "render_backward: the four decoder gradients are given together or not at all");
    if (need_rays) {
        // what dL/do = sum dL/dp, dL/dd = sum t dL/dp does not cover, before any launch
        if (!g->scatter_stage) return fail(GNERF_E_UNSUPPORTED, "render_backward_rays: the ray gradient reads the staged first pass: scatter_stage must hold gnerf_render_backward_stage_bytes(p)");
        if (p->ray_start_per_ray) return fail(GNERF_E_UNSUPPORTED, "render_backward_rays: per-ray limits ('auto') make the coarse depths depend on the rays; numeric ray_start / ray_end only");
    }
    if (!g->grad_planes_nhwc && n_dec == 0) return GNERF_OK;
    if (!planes_fit_32bit_taps(p)) return fail(GNERF_E_UNSUPPORTED, "render_backward: planes too large for 32-bit tap offsets");
    static_assert(kBwdRaysPerWave == kRaysPerWave, "ray tiles are shared with the forward launcher");
    const size_t lds_bytes = (kBwdWeightFloats + kBwdWaves * bwd_wave_floats(16 * (P.tiles_c + P.tiles_f))) * sizeof(float);
    if (lds_bytes > 160 * 1024) return fail(GNERF_E_ARG, "render_backward: %d+%d samples need %zu bytes of LDS (> 160 KiB)", p->depth_resolution, p->depth_resolution_importance, lds_bytes);
    static PerDeviceOnce once, once_staged;
    if (int e = once.raise_lds(render_bwd_kernel<false>, "render_backward")) return e;
    if (int e = once_staged.raise_lds(render_bwd_kernel<true>, "render_backward")) return e;
    // ---- (b) the route.  Overrides for A/B runs and tests, read per call (the tests switch them inside one process):
    BwdRoute route;
    {
        const char* scatter = getenv("GNERF_BWD_SCATTER"), *kernel = getenv("GNERF_BWD_KERNEL");        // direct | staged | sorted;  wave
        const char* mlp = getenv("GNERF_BWD_MLP"), *mlp_k1 = getenv("GNERF_BWD_MLP_K1"), *mlp_k2 = getenv("GNERF_BWD_MLP_K2");
        auto is = [](const char* v, const char* word) { return v && !strcmp(v, word); };
        const bool force_direct = is(scatter, "direct"), force_sorted = is(scatter, "sorted"), force_staged = is(scatter, "staged");
        // decoder arithmetic of the piped kernels: chosen on the device like the forward's; GNERF_BWD_MLP=f32|f16x3|auto forces both, _K1 / _K2 one
        auto mode_of = [&](const char* v, int dflt) { return is(v, "f32") ? GNERF_MLP_F32 : is(v, "f16x3") ? GNERF_MLP_F16X3 : is(v, "auto") ? GNERF_MLP_AUTO : dflt; };
        route.mlp_first = mode_of(mlp_k1, mode_of(mlp, GNERF_MLP_AUTO));
        route.mlp_tiles = mode_of(mlp_k2, mode_of(mlp, GNERF_MLP_AUTO));
        // (F = 0 included: the pipeline's steps and barriers do not depend on the sample counts; a ray without an importance pass shades no
        //  fine tile, merges nothing and marches its coarse samples)
        const bool pipe_shape = pipe_tiles_per_wave(P) != 0 && !is(kernel, "wave");
        const bool rows = g->scatter_stage != nullptr && g->grad_planes_nhwc != nullptr;       // dX rows can be staged, and something reads them
        const bool whole_tiles = P.tiles_per_item > 0 || p->n_items == 1 || p->rays_per_item % kBwdRaysPerWave == 0;    // no 16-ray tile straddles items
        const bool binned = binned_scatter_covers(P);
        const bool can_pad = binned && int64_t(p->n_items) * padded_rays_per_item(*p) < INT32_MAX;
        // a ragged call stays off the one-wave-per-ray kernel and its float atomics where the piped kernels and the binned scatter cover it
        route.padded = !whole_tiles && rows && pipe_shape && !force_direct && !force_sorted && can_pad;
        bool staged = rows && (whole_tiles || route.padded) && !force_direct;
        // A ray request whose ray tiles straddle items on a route that does not pad them: the one-wave-per-ray kernel stages by ray whatever
        // the tiling, so it runs on the call as it is; a plane gradient then takes the binned scatter over the padded ray sequence.
        const bool rows_for_rays = need_rays && !staged;
        route.scatter_padded = rows_for_rays && want_planes;
        if (rows_for_rays) {
            if (force_direct) return fail(GNERF_E_UNSUPPORTED, "render_backward_rays: GNERF_BWD_SCATTER=direct stages no dX rows");
            if (want_planes && (!can_pad || force_sorted))
                return fail(GNERF_E_UNSUPPORTED, "render_backward_rays: ray tiles straddle items and the binned scatter does not cover this call");
            staged = true;
        }
        if (force_staged && !staged) return fail(GNERF_E_ARG, "render_backward: the staged scatter needs scatter_stage, a plane gradient and whole tiles per item");
        const bool exchange = g->scatter_stage != nullptr && g->grad_planes_nhwc == nullptr && n_dec == 4;       // (never a ray request: g_eff above)
        const bool piped = (staged || exchange) && pipe_shape && !force_direct && !rows_for_rays;
        route.first = piped ? (staged ? BwdRoute::kPipedRows : BwdRoute::kPipedExchange) : (staged ? BwdRoute::kWaveStaged : BwdRoute::kWaveDirect);
        // (sorted: the per-ray-tile sort with one atomic per texel and chunk; it also takes the calls the binned form does not cover)
        route.second = !(staged && want_planes) ? BwdRoute::kNoScatter : (binned && !force_sorted ? BwdRoute::kBinned : BwdRoute::kSorted);
    }
    // ---- (c) launches
    hipStream_t s = as_stream(stream);
    const int n_all = p->depth_resolution + p->depth_resolution_importance;
    Params K = P;                                            // the first pass's
    // up to two workgroups of four waves per CU: share tiles until the chip is full (read by the one-wave-per-ray kernel only; every route carries it)
    while (K.split_shift < 2 && (int64_t(K.n_tiles) << (K.split_shift + 1)) <= int64_t(kNumCU) * 2 * kBwdWaves) K.split_shift++;
    if (route.padded) pad_ray_sequence(K);
    if (route.first == BwdRoute::kPipedRows || route.first == BwdRoute::kPipedExchange) {
        // The ray-level part on the forward pipeline (render_kernel_pipe_bwd), the per-sample part as a kernel over sample tiles
        // (render_bwd_tiles_kernel).  Floats per ray of the staging / exchange buffer and from one 16-rank tile's block to the next:
        const bool rows = route.first == BwdRoute::kPipedRows;
        K.bwd_ray_stride = rows ? int64_t(n_all) * 33 : int64_t(n_all) + 32 * ((n_all + 15) / 16);
        K.bwd_tile_pitch = rows ? 512 : 32;
        // (max |planes| goes into the 256 bytes behind the rows when the caller has none)
        if (int e = absmax_or_measure(p, g->scatter_stage + size_t(P.total_rays) * K.bwd_ray_stride, stream, K.absmax)) return e;
        K.p.workspace = nullptr;                                   // (the backward's params carry no workspace)
        K.p.mlp_mode = route.mlp_first;
        const int tp = pipe_tiles_per_wave(K);
        const int64_t total_seq = pipe_seq_len(K);
        const PipeLaunch L = pipe_launch(tp, total_seq);
        K.pipe_unit = L.unit;
        const size_t lds1 = pipe_lds_floats(tp, kMlpAuto) * sizeof(float);
        if (tp == 1) hipLaunchKernelGGL(render_kernel_pipe_bwd<1>, dim3(L.grid), dim3(kPipeThreads), lds1, s, K, *g, g->scatter_stage);
        else if (tp == 2) hipLaunchKernelGGL(render_kernel_pipe_bwd<2>, dim3(L.grid), dim3(kPipeThreads), lds1, s, K, *g, g->scatter_stage);
        else {
            static PerDeviceOnce once3;
            if (int e = once3.raise_lds(render_kernel_pipe_bwd<3>, "render_backward")) return e;
            hipLaunchKernelGGL(render_kernel_pipe_bwd<3>, dim3(L.grid), dim3(kPipeThreads), lds1, s, K, *g, g->scatter_stage);
        }
        if (int e = check_launch("render_kernel_pipe_bwd")) return e;
        Params K2 = K;
        K2.p.mlp_mode = route.mlp_tiles;
        const size_t lds2 = (bwd_tiles_weight_floats() + kTileWaves * bwd_tiles_wave_floats()) * sizeof(float);
        static PerDeviceOnce once_tiles;
        if (int e = once_tiles.raise_lds(render_bwd_tiles_kernel, "render_backward")) return e;
        int64_t g2 = (total_seq * ((n_all + 15) / 16) + kTileWaves - 1) / kTileWaves;
        if (g2 > int64_t(kNumCU) * 2) g2 = int64_t(kNumCU) * 2;    // two workgroups of four waves per CU, each walking a contiguous run of tiles
        g2 = (g2 + kNumXCD - 1) / kNumXCD * kNumXCD;
        hipLaunchKernelGGL(render_bwd_tiles_kernel, dim3((unsigned)g2), dim3(kTileThreads), lds2, s, K2, *g, g->scatter_stage);
        if (int e = check_launch("render_bwd_tiles_kernel")) return e;
    } else {
        const int n_blocks = ((K.n_tiles << K.split_shift) + kBwdWaves - 1) / kBwdWaves;
        const dim3 grid((n_blocks + kNumXCD - 1) / kNumXCD * kNumXCD);
        if (route.first == BwdRoute::kWaveStaged) hipLaunchKernelGGL(render_bwd_kernel<true>, grid, dim3(kBwdThreads), lds_bytes, s, K, *g, g->scatter_stage);
        else hipLaunchKernelGGL(render_bwd_kernel<false>, grid, dim3(kBwdThreads), lds_bytes, s, K, *g, static_cast<float*>(nullptr));
        if (int e = check_launch("render_bwd_kernel")) return e;
    }
    if (need_rays) {
        RayGradArgs R;
        R.planes = p->planes_nhwc; R.origins = p->ray_origins; R.dirs = p->ray_dirs; R.stage = g->scatter_stage;
        R.grad_origins = grad_origins; R.grad_dirs = grad_dirs;
        R.plane_floats = int64_t(3) * p->plane_h * p->plane_w * 32;
        R.H = p->plane_h; R.W = p->plane_w; R.n_all = n_all;
        R.rays_per_item = p->rays_per_item; R.total_rays = P.total_rays;
        R.tex_pitch = P.tex_pitch; R.row_pitch = P.row_pitch; R.plane_pitch = P.plane_pitch; R.box_scale = P.box_scale;
        int64_t blocks = (int64_t(P.total_rays) + kRayGradWaves - 1) / kRayGradWaves;
        if (blocks > int64_t(kNumCU) * 8) blocks = int64_t(kNumCU) * 8;          // eight workgroups of four waves per CU, rays by grid stride
        hipLaunchKernelGGL(render_ray_grad_kernel, dim3((unsigned)blocks), dim3(kRayGradThreads), 0, s, R);
        if (int e = check_launch("render_ray_grad_kernel")) return e;
    }
    if (route.second == BwdRoute::kNoScatter) return GNERF_OK;
    Params KS = K;                                           // the scatter's
    if (route.scatter_padded) pad_ray_sequence(KS);
    KS.bwd_ray_stride = int64_t(n_all) * 33;
    if (route.second == BwdRoute::kBinned) {
        char* ws = reinterpret_cast<char*>(g->scatter_stage) + bin_workspace_offset(P.total_rays, n_all);
        return launch_binned_scatter(KS, g->scatter_stage, ws, g->grad_planes_nhwc, s);
    }
    static PerDeviceOnce once_scatter;
    if (int e = once_scatter.raise_lds(plane_scatter_kernel, "render_backward")) return e;
    hipLaunchKernelGGL(plane_scatter_kernel, dim3(KS.n_tiles), dim3(kScatterThreads), scatter_lds_floats() * sizeof(float), s,
                       KS, static_cast<const float*>(g->scatter_stage), g->grad_planes_nhwc);
    return check_launch("plane_scatter_kernel");
}

extern "C" int gnerf_render_backward(const gnerf_render_params* p, const gnerf_render_grads* g, gnerf_stream_t stream) {
    return render_backward_impl(p, g, nullptr, nullptr, stream);
}

extern "C" int gnerf_render_backward_rays(const gnerf_render_params* p, const gnerf_render_grads* g, float* grad_origins, float* grad_dirs, gnerf_stream_t stream) {
    if (!grad_origins && !grad_dirs) return gnerf::fail(GNERF_E_ARG, "render_backward_rays: grad_origins and grad_dirs are both null (gnerf_render_backward is that call)");
    return render_backward_impl(p, g, grad_origins, grad_dirs, stream);
}

extern "C" size_t gnerf_render_backward_stage_bytes(const gnerf_render_params* p) {
    if (!p || p->n_items < 1 || p->rays_per_item < 1) return 0;
    const size_t n_all = size_t(p->depth_resolution) + size_t(p->depth_resolution_importance);
    const int64_t rays = int64_t(p->n_items) * p->rays_per_item;
    // the staged rows (+ a spare line: max |planes| when the caller has none), then the binned scatter's workspace: counters, the
    // record array (16 bytes per sample and plane) and the tiles' halos (scatter_binned.inl)
    return bin_workspace_offset(rays, int(n_all)) + bin_workspace_bytes(rays, int(n_all), p->n_items, p->plane_h > 0 ? p->plane_h : 1, p->plane_w > 0 ? p->plane_w : 1);
}

extern "C" size_t gnerf_render_backward_exchange_bytes(const gnerf_render_params* p) {
    if (!p || p->n_items < 1 || p->rays_per_item < 1) return 0;
    const size_t n_all = size_t(p->depth_resolution) + size_t(p->depth_resolution_importance);
    return size_t(p->n_items) * size_t(p->rays_per_item) * (n_all + 32 * ((n_all + 15) / 16)) * sizeof(float) + 256;
}

// The three point-query kernels index pts[idx * 3 + k] and 16 * t + j in int.  The largest n_points for which neither overflows
// (include/gnerf_hip.h states it); checked before anything else of the call, the pointers included.
constexpr int kMaxQueryPoints = (INT32_MAX - 15) / 3;

// What the three point-query entry points open with: the n_points cap, the planes and decoder as render params (check_common), the
// derived fields the kernels read and the tile counts.  `tiles` may still exceed int: the entries refuse that after their own checks.
static int fill_query(const char* name, const float* planes_nhwc, int n_items, int plane_h, int plane_w, int n_points, float box_warp,
                      const float* w1, const float* b1, const float* w2, const float* b2, int planes_interleaved,
                      Params& P, int& tiles_per_item, int64_t& tiles) {
    if (n_points > kMaxQueryPoints) return gnerf::fail(GNERF_E_ARG, "%s: too many points (n_points %d > %d)", name, n_points, kMaxQueryPoints);
    P = Params{};
    gnerf_render_params& p = P.p;
    p.planes_interleaved = planes_interleaved;
    p.planes_nhwc = planes_nhwc; p.n_items = n_items; p.plane_h = plane_h; p.plane_w = plane_w;
    p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.box_warp = box_warp;
    if (int e = check_common(&p)) return e;
    P.box_scale = float(2.0 / double(box_warp));
    fill_pitches(P);
    tiles_per_item = (n_points + 15) / 16;
    tiles = int64_t(n_items) * tiles_per_item;
    return GNERF_OK;
}

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
