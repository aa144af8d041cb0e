// The staged backward's second kernel on the pipelined path, render_bwd_tiles_kernel.  Included by render_pipe.hip alone (it holds a kernel):
// it stages the decoder with stage_decoder, like the pipelined kernels and the decoder pack, and is compiled beside them (render_pipe.hip
// says why).
#pragma once
#include "decoder_choice.inl"
#include "render_pipe_layout.inl"
#include "render_bwd_tile.inl"

namespace {

// Second kernel of the staged backward on the pipelined path (round 4).  render_kernel_pipe_bwd (render_pipe.inl) has run the ray-level
// part -- forward pipeline, merge, composite gradient -- at the forward kernel's speed and left, per ray and in depth order, the sample
// depths, colour weights v_r and dL/dsigma_r in the staging buffer.  What is left is work per SAMPLE TILE with no ray-level state at all:
// lookup + decoder forward (exact fp32) + the four gradient products + dX rows.  One wave per 16-rank tile, tiles dealt in contiguous
// runs of the locality-ordered ray sequence; the dX rows of a tile are 2 KB of contiguous staging memory (the one-wave-per-ray kernel
// above writes them rank by rank behind a second forward recomputation, with 12 per-sample arrays per wave in LDS).
constexpr int kTileWaves = 4, kTileThreads = 64 * kTileWaves;       // waves of a tile-kernel workgroup

__host__ __device__ inline size_t bwd_tiles_wave_floats() { return 16 * kStagePitch + 16 * kTPitch + 16 * kHPitch + 48; }

// Decoder in LDS for the f16 hi/lo form of the tile kernel: the forward's fragments (stage_decoder<kMlpF16x3>: W1, W2 colour rows as
// hi/lo halves in MFMA fragment order, biases and density row with the base-2 factors folded in), then the two STATIC operands of the
// gradient products in the same hi/lo fragment form, then the density row in true units.
//   g1 [hi|lo][m][lane][8]:      A of dH^T block m = W2c^T:  element e of lane (j, g) = W2[1 + 8g + e][16m + j]
//   g3 [hi|lo][c][s][lane][8]:   A of dX^T block c, k-step s = W1^T: element jj of lane (j, g) = W1[32s + 16(jj>>2) + 4g + (jj&3)][16c + j]
//                                (the k order in which a lane's dPRE registers come: the forward's layer-2 trick)
constexpr int kBwdFragHalves = 4 * 64 * 8;          // one of g1 hi, g1 lo, g3 hi, g3 lo
constexpr int kBwdF16WeightFloats = kWeightFloatsF16 + 64 + 36 + (4 * kBwdFragHalves) / 2 + 64 + 4;
__host__ __device__ constexpr int bwd_tiles_weight_floats() { return kBwdF16WeightFloats > kBwdWeightFloats ? kBwdF16WeightFloats : kBwdWeightFloats; }
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef unsigned u2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h4 as_h4(unsigned a, unsigned b) { return __builtin_bit_cast(h4, (u2v){a, b}); }
#define GNERF_MFMA16K16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0)

// One 16-sample tile, exact fp32 products (v_mfma_f32_16x16x4_f32): any finite input.
struct BwdTileF32 {
    static constexpr int kMlp = kMlpF32;
    BwdLds L;
    float inv_scale;
    __device__ __forceinline__ void setup(const Params& P, float* smem, const float*, int tid) {
        L = BwdLds{};
        bwd_stage_decoder_f32<kTileThreads>(L, smem, P.p, tid);
        inv_scale = 1.f;
    }
    // X in L.stage, the tile's colour weights in vw, dL/dsigma in dsg, G = dL/d colour sum of channels 16n + j  ->  dX[16][32] in L.tbuf
    __device__ __forceinline__ void tile(const float* vw, const float* dsg, const float (&G)[2], BwdAcc& A, int lane) {
        const int j = lane & 15, g = lane >> 4;
        v4f h[4], o[2];
        float sig;
        bwd_mlp_forward(L, lane, h, o, sig);
        // ---- dO: colour c = 1.002 * s - 0.001 with s = sigmoid(o); dL/dc = G * v_sample  (triplane.py:134, ray_marcher.py:27-45)
        const v4f vs = *reinterpret_cast<const v4f*>(vw + 4 * g);
        const float dsig = dsg[j];
#pragma unroll
        for (int n = 0; n < 2; n++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float d = G[n] * vs[r] * rgb_slope_hw(o[n][r]);
                L.tbuf[(4 * g + r) * kTPitch + 16 * n + j] = d;
                A.b2[n] += d;
            }
        }
        bwd_tile_core(L, h, dsig, A, lane);
    }
    __device__ __forceinline__ void finish(BwdAcc&) {}
};

// The same tile with every product as an error-compensated f16 hi/lo split on the f16 matrix instructions (fp32 accumulation): the
// decoder forward as in the forward kernels (24 v_mfma_f32_16x16x32_f16), dH and dX against static hi/lo fragments (12 + 12), the two
// weight-gradient products -- both operands made at run time, K = the tile's 16 samples -- on v_mfma_f32_16x16x16_f16 (24 + 24): 96
// matrix instructions of 16.5 SIMD cycles where the fp32 form issues 192 of 32.  Loss gradients of 1e-6 are f16-subnormal, and a
// call's gradients span many orders of magnitude (a ray whose weights sum to 1e-6 sends dL/ddepth / 1e-6 down its samples): every
// matrix operand of the gradient side (dO, dsigma, dH, dPRE) is therefore carried MULTIPLIED BY A POWER OF TWO CHOSEN PER TILE from
// the tile's own largest |dO| and |dsigma|, so that the largest |dPRE| possible lands near 2^13.  The scale comes off, exactly, when
// dX is written; the wave's two matrix-accumulated weight gradients (dW1, dW2: 64 registers) are kept in the units of the CURRENT
// tile's scale -- when the scale changes from one tile to the next they are multiplied by the ratio, a power of two (exact; fp32 has
// the range) -- so that the matrix instructions accumulate into them directly.
// Valid under the same guard as the forward's f16 arithmetic (choose_mlp: features, weights, activations in f16's range).
struct BwdTileF16 {
    static constexpr int kMlp = kMlpF16x3;
    ShadeLds C;                      // the forward's fragments (w1 = fragment base, w2 = density row * ln2, b1 * log2e, b2 scaled)
    const _Float16* g1; const _Float16* g3;
    const float* ws_true;            // W2[0][:]
    float* stage; float* tbuf; float* hbuf;
    float l1_w2c, max_ws;            // max_hid sum_out |W2c[out][hid]|, max |W2[0]|: |dPRE| <= |dH| <= l1_w2c max|dO| + max_ws max|dsigma|
    float acc_scale;                 // the power of two A.w1 / A.w2 currently carry
    bool sp_direct = false;          // softplus as log2(1 + 2^p') (choose_mlp: every |p'| below exp2's overflow), as the forward kernels take it
    __device__ __forceinline__ void setup(const Params& P, float* smem, const float*, int tid) {
        const gnerf_render_params& p = P.p;
        stage_decoder<kMlpF16x3>(C, smem, p, tid, kTileThreads);
        _Float16* gh = reinterpret_cast<_Float16*>(smem + kWeightFloatsF16 + 64 + 36);
        g1 = gh; g3 = gh + 2 * kBwdFragHalves;
        float* wst = smem + kWeightFloatsF16 + 64 + 36 + (4 * kBwdFragHalves) / 2;
        ws_true = wst;
        for (int i = tid; i < 2048; i += kTileThreads) {
            const int e = i & 7, j = (i >> 3) & 15, g = (i >> 7) & 3, m = i >> 9;             // lane 16 g + j of block m
            const float x = p.w2[(1 + 8 * g + e) * 64 + 16 * m + j];
            const _Float16 hi = (_Float16)x;
            gh[i] = hi;
            gh[kBwdFragHalves + i] = (_Float16)(x - (float)hi);
        }
        for (int i = tid; i < 2048; i += kTileThreads) {
            const int jj = i & 7, j = (i >> 3) & 15, g = (i >> 7) & 3, sx = (i >> 9) & 1, c = i >> 10;     // lane 16 g + j of fragment (c, s)
            const float x = p.w1[(32 * sx + 16 * (jj >> 2) + 4 * g + (jj & 3)) * 32 + 16 * c + j];
            const _Float16 hi = (_Float16)x;
            gh[2 * kBwdFragHalves + i] = hi;
            gh[3 * kBwdFragHalves + i] = (_Float16)(x - (float)hi);
        }
        if (tid < 64) wst[tid] = p.w2[tid];
        __syncthreads();
        const int lane = tid & 63;
        float l1 = 0.f;
        for (int o = 0; o < 32; o++) l1 += fabsf(p.w2[(1 + o) * 64 + lane]);
        float wsm = fabsf(wst[lane]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { l1 = fmaxf(l1, __shfl_xor(l1, o)); wsm = fmaxf(wsm, __shfl_xor(wsm, o)); }
        l1_w2c = l1; max_ws = wsm; acc_scale = 1.f;
    }
    __device__ __forceinline__ void tile(const float* vw, const float* dsg, const float (&G)[2], BwdAcc& A, int lane) {
        const int j = lane & 15, g = lane >> 4;
        const _Float16* w1h = reinterpret_cast<const _Float16*>(C.w1);
        const _Float16* w2h = w1h + 2 * kW1FragHalves;
        // ---- decoder forward (shade_tile's f16 branch): p' = log2(e) pre-activation, hv = log2(1 + 2^p') = H / ln 2, o' = -log2(e) o
        const v4f f_lo = *reinterpret_cast<const v4f*>(stage + j * kStagePitch + 8 * g);
        const v4f f_hi = *reinterpret_cast<const v4f*>(stage + j * kStagePitch + 8 * g + 4);
        const float f[8] = {f_lo[0], f_lo[1], f_lo[2], f_lo[3], f_hi[0], f_hi[1], f_hi[2], f_hi[3]};
        unsigned fh_u[4], fl_u[4];
        split_f16x8(f, fh_u, fl_u);
        const h8 fh = as_h8((u4v){fh_u[0], fh_u[1], fh_u[2], fh_u[3]}), fl = as_h8((u4v){fl_u[0], fl_u[1], fl_u[2], fl_u[3]});
        v4f hv[4];
        {
            h8 a_hi[4], a_lo[4];
#pragma unroll
            for (int m = 0; m < 4; m++) {
                hv[m] = *reinterpret_cast<const v4f*>(C.b1 + 16 * m + 4 * g);
                a_hi[m] = *reinterpret_cast<const h8*>(w1h + (m * 64 + lane) * 8);
                a_lo[m] = *reinterpret_cast<const h8*>(w1h + kW1FragHalves + (m * 64 + lane) * 8);
            }
#pragma unroll
            for (int m = 0; m < 4; m++) hv[m] = GNERF_MFMA16(a_hi[m], fh, hv[m]);
#pragma unroll
            for (int m = 0; m < 4; m++) hv[m] = GNERF_MFMA16(a_hi[m], fl, hv[m]);
#pragma unroll
            for (int m = 0; m < 4; m++) hv[m] = GNERF_MFMA16(a_lo[m], fh, hv[m]);
        }
#pragma unroll
        for (int m = 0; m < 4; m++) {
            v4f e;
            if (sp_direct) {
#pragma unroll
                for (int r = 0; r < 4; r++) e[r] = __builtin_amdgcn_exp2f(hv[m][r]);
#pragma unroll
                for (int r = 0; r < 4; r++) hv[m][r] = __builtin_amdgcn_logf(1.0f + e[r]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++) e[r] = __builtin_amdgcn_exp2f(-fabsf(hv[m][r]));
#pragma unroll
                for (int r = 0; r < 4; r++) e[r] = __builtin_amdgcn_logf(1.0f + e[r]);
#pragma unroll
                for (int r = 0; r < 4; r++) hv[m][r] = fmaxf(hv[m][r] + e[r], e[r]);
            }
            *reinterpret_cast<v4f*>(hbuf + j * kHPitch + 16 * m + 4 * g) = hv[m];               // H / ln2 as [sample][hidden], for dW2's B operand
        }
        __builtin_amdgcn_sched_barrier(0);
        v4f o[2];
        {
            const float bc0 = C.b2[1 + j], bc1 = C.b2[17 + j];
            o[0] = (v4f){bc0, bc0, bc0, bc0}; o[1] = (v4f){bc1, bc1, bc1, bc1};
            h8 x_hi[2], x_lo[2];
#pragma unroll
            for (int s = 0; s < 2; s++) {
                unsigned xh[4], xl[4];
                const float xs[8] = {hv[2 * s][0], hv[2 * s][1], hv[2 * s][2], hv[2 * s][3], hv[2 * s + 1][0], hv[2 * s + 1][1], hv[2 * s + 1][2], hv[2 * s + 1][3]};
                split_f16x8(xs, xh, xl);
                x_hi[s] = as_h8((u4v){xh[0], xh[1], xh[2], xh[3]});
                x_lo[s] = as_h8((u4v){xl[0], xl[1], xl[2], xl[3]});
            }
#pragma unroll
            for (int s = 0; s < 2; s++) {
#pragma unroll
                for (int n = 0; n < 2; n++) {
                    const h8 w_hi = *reinterpret_cast<const h8*>(w2h + ((n * 2 + s) * 64 + lane) * 8);
                    const h8 w_lo = *reinterpret_cast<const h8*>(w2h + 2048 + ((n * 2 + s) * 64 + lane) * 8);
                    o[n] = GNERF_MFMA16(x_hi[s], w_hi, o[n]);
                    o[n] = GNERF_MFMA16(x_hi[s], w_lo, o[n]);
                    o[n] = GNERF_MFMA16(x_lo[s], w_hi, o[n]);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- dO: colour c = 1.002 s - 0.001, s = sigmoid(o) = 1 / (1 + 2^o'); kept in registers too (A operand of dW2)
        const v4f vs = *reinterpret_cast<const v4f*>(vw + 4 * g);
        const float dsig_true = dsg[j];
        float dO[8];
        float big = max_ws * fabsf(dsig_true);
#pragma unroll
        for (int n = 0; n < 2; n++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(o[n][r]));
                const float d = G[n] * vs[r] * rgb_slope_of_sigmoid(s);
                dO[4 * n + r] = d;
                A.b2[n] += d;
                big = fmaxf(big, l1_w2c * fabsf(d));
            }
        }
        if (g == 0) A.b2s += dsig_true;
        // the tile's scale: |dPRE| <= l1 max|dO| + max_ws max|dsigma| <= 2 max over the lanes of `big`  ->  scaled below 2^13
        // wave maximum of non-negative values on the DPP network (the forward kernels' scan idiom; lane 63 ends up with the maximum)
        big = fmaxf(big, dpp_mov<0x111, 0xf>(0.f, big));
        big = fmaxf(big, dpp_mov<0x112, 0xf>(0.f, big));
        big = fmaxf(big, dpp_mov<0x114, 0xf>(0.f, big));
        big = fmaxf(big, dpp_mov<0x118, 0xf>(0.f, big));
        big = fmaxf(big, dpp_mov<0x142, 0xa>(0.f, big));
        big = fmaxf(big, dpp_mov<0x143, 0xc>(0.f, big));
        big = wave_last(big);
        int ex = 0;
        if (big > 0.f && big < INFINITY) { (void)frexpf(big, &ex); ex = min(max(12 - ex, -60), 60); }
        ex = __builtin_amdgcn_readfirstlane(ex);                    // one value for the wave, whatever the lanes think
        const float scale = ldexpf(1.f, ex), inv = ldexpf(1.f, -ex);
        if (scale != acc_scale) {                                   // wave-uniform: bring the matrix accumulators to this tile's units
            const float ratio = scale * (1.f / acc_scale);          // both powers of two within 2^+-60: exact
#pragma unroll
            for (int m = 0; m < 4; m++) { A.w1[m][0] *= ratio; A.w1[m][1] *= ratio; A.w2[0][m] *= ratio; A.w2[1][m] *= ratio; }
            acc_scale = scale;
        }
        const float dsig = dsig_true * scale;
#pragma unroll
        for (int n = 0; n < 2; n++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                dO[4 * n + r] *= scale;
                tbuf[(4 * g + r) * kTPitch + 16 * n + j] = dO[4 * n + r];
            }
        }
        lds_wave_sync();
        __builtin_amdgcn_sched_barrier(0);
        // ---- dH^T[hidden][sample] = W2c^T dO^T (+ the density row on the vector ALU): B = this lane's sample row of dO, outputs 8g..8g+7
        v4f dh[4];
        {
            const v4f b_lo4 = *reinterpret_cast<const v4f*>(tbuf + j * kTPitch + 8 * g);
            const v4f b_hi4 = *reinterpret_cast<const v4f*>(tbuf + j * kTPitch + 8 * g + 4);
            const float bv[8] = {b_lo4[0], b_lo4[1], b_lo4[2], b_lo4[3], b_hi4[0], b_hi4[1], b_hi4[2], b_hi4[3]};
            unsigned bh_u[4], bl_u[4];
            split_f16x8(bv, bh_u, bl_u);
            const h8 bh = as_h8((u4v){bh_u[0], bh_u[1], bh_u[2], bh_u[3]}), bl = as_h8((u4v){bl_u[0], bl_u[1], bl_u[2], bl_u[3]});
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const v4f ws = *reinterpret_cast<const v4f*>(ws_true + 16 * m + 4 * g);
                dh[m] = ws * dsig;
                A.w2s[m] += hv[m] * dsig_true;                                                   // (x ln2 at the end)
                const h8 a_hi = *reinterpret_cast<const h8*>(g1 + (m * 64 + lane) * 8);
                const h8 a_lo = *reinterpret_cast<const h8*>(g1 + kBwdFragHalves + (m * 64 + lane) * 8);
                dh[m] = GNERF_MFMA16(a_hi, bh, dh[m]);
                dh[m] = GNERF_MFMA16(a_hi, bl, dh[m]);
                dh[m] = GNERF_MFMA16(a_lo, bh, dh[m]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- dW2c[out][hidden] += dO^T (H / ln2): A = the dO values this lane computed (samples 4g..4g+3 of outputs 16o + j), B from hbuf
        {
            unsigned ah_u[4], al_u[4];
            split_f16x8(dO, ah_u, al_u);
#pragma unroll
            for (int np = 0; np < 2; np++) {                       // hidden blocks 2 np, 2 np + 1
                float bvals[8];
#pragma unroll
                for (int q = 0; q < 2; q++)
#pragma unroll
                    for (int e = 0; e < 4; e++) bvals[4 * q + e] = hbuf[(4 * g + e) * kHPitch + 16 * (2 * np + q) + j];
                unsigned bh_u[4], bl_u[4];
                split_f16x8(bvals, bh_u, bl_u);
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const h4 b_hi = as_h4(bh_u[2 * q], bh_u[2 * q + 1]), b_lo = as_h4(bl_u[2 * q], bl_u[2 * q + 1]);
#pragma unroll
                    for (int oo = 0; oo < 2; oo++) {
                        const h4 a_hi = as_h4(ah_u[2 * oo], ah_u[2 * oo + 1]), a_lo = as_h4(al_u[2 * oo], al_u[2 * oo + 1]);
                        v4f acc = A.w2[oo][2 * np + q];
                        acc = GNERF_MFMA16K16(a_hi, b_hi, acc);
                        acc = GNERF_MFMA16K16(a_hi, b_lo, acc);
                        acc = GNERF_MFMA16K16(a_lo, b_hi, acc);
                        A.w2[oo][2 * np + q] = acc;
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- through softplus: d/dpre softplus(pre) = 1 - exp(-H) = 1 - 2^-(H / ln2)
#pragma unroll
        for (int m = 0; m < 4; m++) {
#pragma unroll
            for (int r = 0; r < 4; r++) dh[m][r] *= 1.f - __builtin_amdgcn_exp2f(-hv[m][r]);
            A.b1[m] += dh[m] * inv;
        }
        lds_wave_sync();                                            // every lane has read H from hbuf and its dO row from tbuf
        __builtin_amdgcn_sched_barrier(0);
        // ---- dX^T[channel][sample] = W1^T dPRE^T: B straight from this lane's dPRE registers (k order of the g3 fragments)
        v4f dx[2];
        dx[0] = dx[1] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const float pv[8] = {dh[2 * s][0], dh[2 * s][1], dh[2 * s][2], dh[2 * s][3], dh[2 * s + 1][0], dh[2 * s + 1][1], dh[2 * s + 1][2], dh[2 * s + 1][3]};
            unsigned ph_u[4], pl_u[4];
            split_f16x8(pv, ph_u, pl_u);
            const h8 p_hi = as_h8((u4v){ph_u[0], ph_u[1], ph_u[2], ph_u[3]}), p_lo = as_h8((u4v){pl_u[0], pl_u[1], pl_u[2], pl_u[3]});
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const h8 a_hi = *reinterpret_cast<const h8*>(g3 + ((c * 2 + s) * 64 + lane) * 8);
                const h8 a_lo = *reinterpret_cast<const h8*>(g3 + kBwdFragHalves + ((c * 2 + s) * 64 + lane) * 8);
                dx[c] = GNERF_MFMA16(a_hi, p_hi, dx[c]);
                dx[c] = GNERF_MFMA16(a_hi, p_lo, dx[c]);
                dx[c] = GNERF_MFMA16(a_lo, p_hi, dx[c]);
            }
        }
#pragma unroll
        for (int m = 0; m < 4; m++) *reinterpret_cast<v4f*>(hbuf + j * kHPitch + 16 * m + 4 * g) = dh[m];         // dPRE[sample][hidden]
        *reinterpret_cast<v4f*>(tbuf + j * kTPitch + 4 * g) = dx[0] * inv;                                         // dX[sample][channel], true units
        *reinterpret_cast<v4f*>(tbuf + j * kTPitch + 16 + 4 * g) = dx[1] * inv;
        lds_wave_sync();
        __builtin_amdgcn_sched_barrier(0);
        // ---- dW1[hidden][channel] += dPRE^T X: A = dPRE^T from hbuf, B = X^T from the staged features
        {
            float xv[8];
#pragma unroll
            for (int c = 0; c < 2; c++)
#pragma unroll
                for (int e = 0; e < 4; e++) xv[4 * c + e] = stage[(4 * g + e) * kStagePitch + 16 * c + j];
            unsigned xh_u[4], xl_u[4];
            split_f16x8(xv, xh_u, xl_u);
#pragma unroll
            for (int mp = 0; mp < 2; mp++) {
                float av[8];
#pragma unroll
                for (int q = 0; q < 2; q++)
#pragma unroll
                    for (int e = 0; e < 4; e++) av[4 * q + e] = hbuf[(4 * g + e) * kHPitch + 16 * (2 * mp + q) + j];
                unsigned ah_u[4], al_u[4];
                split_f16x8(av, ah_u, al_u);
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const h4 a_hi = as_h4(ah_u[2 * q], ah_u[2 * q + 1]), a_lo = as_h4(al_u[2 * q], al_u[2 * q + 1]);
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        const h4 b_hi = as_h4(xh_u[2 * c], xh_u[2 * c + 1]), b_lo = as_h4(xl_u[2 * c], xl_u[2 * c + 1]);
                        v4f acc = A.w1[2 * mp + q][c];
                        acc = GNERF_MFMA16K16(a_hi, b_hi, acc);
                        acc = GNERF_MFMA16K16(a_hi, b_lo, acc);
                        acc = GNERF_MFMA16K16(a_lo, b_hi, acc);
                        A.w1[2 * mp + q][c] = acc;
                    }
                }
            }
        }
    }
    // the matrix accumulators carry acc_scale, and dW2 was accumulated against H / ln2
    __device__ __forceinline__ void finish(BwdAcc& A) {
        const float k1 = 1.f / acc_scale, k2 = k1 * kLn2;
#pragma unroll
        for (int m = 0; m < 4; m++) { A.w1[m][0] *= k1; A.w1[m][1] *= k1; A.w2[0][m] *= k2; A.w2[1][m] *= k2; A.w2s[m] *= kLn2; }
    }
};

template <class Tile>
__device__ __forceinline__ void render_bwd_tiles_body(const Params& P, const gnerf_render_grads& Gr, float* stage, float* smem, bool sp_direct = false) {
    const gnerf_render_params& p = P.p;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n_all = p.depth_resolution + p.depth_resolution_importance;
    const float* tail = stage + int64_t(P.total_rays) * P.bwd_ray_stride;
    Tile K;
    K.setup(P, smem, tail, tid);
    if constexpr (Tile::kMlp != kMlpF32) K.sp_direct = sp_direct;
    float* base = smem + bwd_tiles_weight_floats() + size_t(wv) * bwd_tiles_wave_floats();
    BwdLds L = {};
    L.stage = base; L.tbuf = L.stage + 16 * kStagePitch; L.hbuf = L.tbuf + 16 * kTPitch;
    if constexpr (Tile::kMlp == kMlpF32) { K.L.stage = L.stage; K.L.tbuf = L.tbuf; K.L.hbuf = L.hbuf; }
    else { K.stage = L.stage; K.tbuf = L.tbuf; K.hbuf = L.hbuf; }
    float* dep = L.hbuf + 16 * kHPitch;            // [16] depths, [16] colour weights, [16] dL/dsigma of the tile
    float* vw = dep + 16;
    float* dsg = vw + 16;
    BwdAcc A;
#pragma unroll
    for (int m = 0; m < 4; m++) A.w1[m][0] = A.w1[m][1] = A.w2[0][m] = A.w2[1][m] = A.w2s[m] = A.b1[m] = (v4f){0.f, 0.f, 0.f, 0.f};
    A.b2[0] = A.b2[1] = A.b2s = 0.f;
    const int j = lane & 15;
    const int64_t plane_floats = int64_t(3) * p.plane_h * p.plane_w * 32;
    // tiles of the locality-ordered ray sequence (pipe_seq_to_ray): XCD x owns a contiguous eighth (workgroups b, b+8, ... share an
    // XCD), cut into equal contiguous runs for the XCD's waves
    const int tiles_per_ray = (n_all + 15) >> 4;
    const int64_t total_seq = (P.tiles_per_item > 0 || linear_pad(P) > 0) ? int64_t(P.n_tiles) * 16 : int64_t(P.total_rays);
    const int xcd = blockIdx.x % kNumXCD, wg = blockIdx.x / kNumXCD, wgs = gridDim.x / kNumXCD;
    const int64_t x0 = total_seq * xcd / kNumXCD * tiles_per_ray, x1 = total_seq * (xcd + 1) / kNumXCD * tiles_per_ray;
    const int64_t waves = int64_t(wgs) * kTileWaves, me = int64_t(wg) * kTileWaves + wv;
    const int64_t t0 = x0 + (x1 - x0) * me / waves, t1 = x0 + (x1 - x0) * (me + 1) / waves;
    for (int64_t t = t0; t < t1; t++) {
        const int64_t seq = t / tiles_per_ray;
        const int T = int(t - seq * tiles_per_ray);
        const int ray = pipe_seq_to_ray<true>(P, seq);
        if (ray < 0) continue;
        const int item = ray / p.rays_per_item;
        const int live = min(16, n_all - 16 * T);
        float* const ray_block = stage + int64_t(ray) * P.bwd_ray_stride;
        float* const rows = ray_block + n_all + T * P.bwd_tile_pitch;
        if (lane < 16) dep[lane] = ray_block[16 * T + min(lane, live - 1)];
        else if (lane < 48) dep[lane] = ((lane & 15) < live) ? rows[lane - 16] : 0.f;       // vw[0..15], dsg[0..15]
        BwdRay R;
        R.ox = p.ray_origins[int64_t(ray) * 3 + 0]; R.oy = p.ray_origins[int64_t(ray) * 3 + 1]; R.oz = p.ray_origins[int64_t(ray) * 3 + 2];
        R.dx = p.ray_dirs[int64_t(ray) * 3 + 0]; R.dy = p.ray_dirs[int64_t(ray) * 3 + 1]; R.dz = p.ray_dirs[int64_t(ray) * 3 + 2];
        R.planes = reinterpret_cast<const char*>(p.planes_nhwc + int64_t(item) * plane_floats);
        float G[2];
        G[0] = Gr.grad_rgb ? 2.f * Gr.grad_rgb[int64_t(ray) * 32 + j] : 0.f;
        G[1] = Gr.grad_rgb ? 2.f * Gr.grad_rgb[int64_t(ray) * 32 + 16 + j] : 0.f;
        lds_wave_sync();
        bwd_gather_tile_rolling(P, L, R.planes, DepthListPos{R, dep, P.box_scale}, lane);
        K.tile(vw, dsg, G, A, lane);
        if (Gr.grad_planes_nhwc) {                                  // the tile's dX rows: 16 x 128 contiguous bytes
            const int half = lane >> 5, ch = lane & 31;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int smp = 2 * q + half;
                if (smp < live) rows[smp * 32 + ch] = L.tbuf[smp * kTPitch + ch];
            }
        }
        lds_wave_sync();
    }
    K.finish(A);
    bwd_reduce_decoder_grads(A, smem, Gr.grad_w1, Gr.grad_b1, Gr.grad_w2, Gr.grad_b2, tid, lane, j, kTileThreads);
}

// Decoder arithmetic as in the forward: the f16 hi/lo form (1.45 ms at config 2; plane and decoder gradients within 1e-6 of the fp32
// form) when the device-side range check allows it, the exact-fp32 form (2.12 ms) otherwise.
// Until the middle of round 4 the f16 form was opt-in: with two workgroups per CU -- the launch shape that gives the speed -- a
// handful of samples per launch (of 2e5) came out wrong, different ones from run to run.  Root cause (tools/dbg_bwd_stage.py, assembly
// variants of this kernel; profiles/r04_pk_opsel_hazard.md): ONE instruction of the dO block, `v_pk_mul_f32 D, S0, S1 op_sel:[0,1]`
// (low half of the result from the HIGH register of src1), reads that register as 0.0 in lanes 48-63 now and then while the other
// wave of its SIMD has a v_mfma_f32_16x16x32_f16 in flight: sample 13 of a tile lost its first 16 dO entries.  The product with
// the operands exchanged (`op_sel:[1,0]`) is exact in every run; the build (csrc/compile_unit.sh, pk_opsel_fixup.py) rewrites every
// such instruction of the library and tools/isa_lint.py checks the result.
__global__ __launch_bounds__(kTileThreads, 2) void render_bwd_tiles_kernel(Params P, gnerf_render_grads Gr, float* stage) {
    extern __shared__ __align__(16) float smem[];
    int mlp = P.p.mlp_mode;
    bool sp_direct = false;
    if (mlp == kMlpAuto) mlp = choose_mlp(P, smem, &sp_direct);
    if (mlp == kMlpF32) render_bwd_tiles_body<BwdTileF32>(P, Gr, stage, smem);
    else                render_bwd_tiles_body<BwdTileF16>(P, Gr, stage, smem, sp_direct);
}

}  // namespace
