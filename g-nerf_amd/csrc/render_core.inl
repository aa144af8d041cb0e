// What every render kernel shares on the device: small numeric helpers, the DPP wave scans, the generic lookup (Weights, load_weights,
// lookup_plane), depth proposals, importance resampling, the depth merge, the ray march and the call-wide depth range.  No kernel is
// defined here: any unit of the renderer may include it.  Like every .inl of the renderer it opens the unit's anonymous namespace itself
// and includes what it needs.
#pragma once
#include "render_params.h"
#include <cmath>

namespace {

using namespace gnerf;

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kHidden = 64;
constexpr int kStagePitch = 36;        // dwords per staged sample row (32 channels + pad)
constexpr int kRaysPerWave = 16;


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

}  // namespace
