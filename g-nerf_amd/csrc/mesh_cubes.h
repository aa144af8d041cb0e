// What the marching-cubes units share (csrc/mesh.hip on a dense volume, csrc/mesh_band_cubes.hip on the active bricks of a narrow band): the
// classification of a lattice point from its cell's eight corner values, the ballot prefixes, and the scan of the per-block counts.  Included
// inside each unit's anonymous namespace, after mesh_tables.h.
#pragma once

static_assert(GNERF_MC_MAX_TRIS < 8, "triangle counts are scanned with three ballots");

// One lattice point: its value, its three forward neighbours' values, its crossed-axis mask (bit a: edge p -> p + e_a exists and is
// crossed), its cell's case and triangle count (0 unless p is a cell's lower corner).
struct Point {
    float v, vn[3];
    uint32_t mask, cell_case, ntri;
    bool bad;
};

// cv: corner c = (c>>2, c>>1 & 1, c & 1) of the point's cell; h_a: the point has a forward neighbour along axis a.  A corner that does not
// exist holds any value (it is never used).
__device__ __forceinline__ Point classify_corners(const float (&cv)[8], float level, bool h0, bool h1, bool h2) {
    Point pt;
    pt.v = cv[0];
    pt.vn[0] = cv[4];
    pt.vn[1] = cv[2];
    pt.vn[2] = cv[1];
    pt.bad = !__builtin_isfinite(cv[0]);
    uint32_t cs = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) cs |= (cv[c] > level ? 1u : 0u) << c;
    const uint32_t in0 = cs & 1u;
    pt.mask = (h0 && ((cs >> 4) & 1u) != in0 ? 1u : 0u) | (h1 && ((cs >> 2) & 1u) != in0 ? 2u : 0u) | (h2 && ((cs >> 1) & 1u) != in0 ? 4u : 0u);
    pt.cell_case = cs;
    pt.ntri = (h0 && h1 && h2) ? uint32_t(kMcTriCount[cs]) : 0u;
    return pt;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
}

// Exclusive prefix of a small per-lane count (< 2^BITS) over the wave, and the wave's total: one ballot per bit.
template <int BITS>
__device__ __forceinline__ uint32_t wave_prefix(uint32_t x, uint32_t* total) {
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int b = 0; b < BITS; b++) {
        const uint64_t m = __ballot((x >> b) & 1u);
        pre += lanes_below(m) << b;
        tot += uint32_t(__popcll(m)) << b;
    }
    *total = tot;
    return pre;
}

// The body of a one-workgroup kernel of kMcScanThreads threads: exclusive 64-bit offsets of the per-block vertex and triangle counts, tile by
// tile with the carry in registers; totals -> counts[0..2] (vertices, triangles, the sum of blk_bad -- 0 when blk_bad is null).
constexpr int kMcScanThreads = 1024;
__device__ __forceinline__ void scan_block_counts(const uint32_t* __restrict__ blk_v, const uint32_t* __restrict__ blk_t,
                                                  const uint32_t* __restrict__ blk_bad, int64_t* __restrict__ voff, int64_t* __restrict__ toff,
                                                  uint32_t nb, int64_t* __restrict__ counts) {
    __shared__ int64_t sv[kMcScanThreads / 64], st[kMcScanThreads / 64], sb[kMcScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry_v = 0, carry_t = 0, bad = 0;
    for (uint32_t head = 0; head < nb; head += kMcScanThreads) {
        const uint32_t i = head + threadIdx.x;
        const int64_t v0 = i < nb ? int64_t(blk_v[i]) : 0, t0 = i < nb ? int64_t(blk_t[i]) : 0;
        bad += (blk_bad && i < nb) ? int64_t(blk_bad[i]) : 0;
        int64_t v = v0, t = t0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t xv = __shfl_up(v, o, 64), xt = __shfl_up(t, o, 64);
            if (lane >= o) { v += xv; t += xt; }
        }
        if (lane == 63) { sv[wave] = v; st[wave] = t; }
        __syncthreads();
        int64_t bv = 0, bt = 0, av = 0, at = 0;
        for (int w = 0; w < kMcScanThreads / 64; w++) {
            bv += w < wave ? sv[w] : 0;
            bt += w < wave ? st[w] : 0;
            av += sv[w];
            at += st[w];
        }
        if (i < nb) {
            voff[i] = carry_v + bv + v - v0;
            toff[i] = carry_t + bt + t - t0;
        }
        carry_v += av;
        carry_t += at;
        __syncthreads();                                 // sv / st are rewritten by the next tile
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    if (lane == 0) sb[wave] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t b = 0;
        for (int w = 0; w < kMcScanThreads / 64; w++) b += sb[w];
        counts[0] = carry_v;
        counts[1] = carry_t;
        counts[2] = b;
    }
}
