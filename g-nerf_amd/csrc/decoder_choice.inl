// GNERF_MLP_AUTO: the decoder statistics and the choice of the decoder arithmetic they allow (choose_mlp), for the pipelined kernels, the
// backward's tile kernel and the decoder pack.  No kernel is defined here.
#pragma once
#include "render_core.inl"

namespace {

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

}  // namespace
