// The backward's per-tile helpers: LDS carve-up and the fp32 decoder's staging (bwd_stage_decoder_f32, the one copy of that preamble), the
// lookup with its deferred plane scatter, the decoder forward and backward of one 16-sample tile on the exact fp32 MFMA (the colour slope
// rgb_slope_hw and the colour half of dH, bwd_dh_add_colour, are here once for every backward), the decoder-gradient reduction.  Shared by the renderer's backward (render_bwd.inl,
// render_ray_grad.inl) and the point queries (query_bwd.inl, query_grad.inl, project_level.inl).  No kernel is defined here.
#pragma once
#include "render_shade.inl"

namespace {

constexpr int kBwdWaves = 4;
constexpr int kBwdThreads = 64 * kBwdWaves;
constexpr int kBwdRaysPerWave = 16;
constexpr int kTPitch = 36;          // dO [16 samples][32 colour outputs], later dX [16][32 channels]
constexpr int kHPitch = 68;          // H, later dPRE: [16 samples][64 hidden]
constexpr int kBwdWeightFloats = 64 * kW1Pitch + 33 * kW2Pitch + 64 + 36;      // w1, w2, b1, b2 in plain fp32 rows
constexpr int kBwdGradFloats = 64 * 32 + 64 + 33 * 64 + 33;                    // reduction area, aliases the weights
static_assert(kBwdGradFloats <= kBwdWeightFloats, "weight-gradient reduction area must fit in the weight area");

__host__ __device__ inline size_t bwd_wave_floats(int s_pad) {
    return size_t(12) * s_pad + 16 * kStagePitch + 16 * kTPitch + 16 * kHPitch + 16 * kTapDwords;
}

struct BwdLds {
    const float* w1; const float* w2; const float* b1; const float* b2;     // workgroup-shared decoder
    float* t_e; float* sig_e; float* q_e; float* v_e; float* dsig_e; int* rank_e;      // per element (coarse k at k, fine i at 16*tiles_c + i)
    float* s_t; float* s_sig; float* s_q; float* w_s; float* trans; float* ds;         // sorted order / per interval
    float* stage; float* tbuf; float* hbuf; float* taps;
};

// The decoder into the first kBwdWeightFloats of a workgroup's LDS as plain fp32 rows (every matrix is read in two orientations), b2 zero
// padded to 36; sets L.w1 / w2 / b1 / b2 and ends with the workgroup's barrier.  Every thread of the THREADS of the workgroup must call.
template <int THREADS>
__device__ __forceinline__ void bwd_stage_decoder_f32(BwdLds& L, float* smem, const gnerf_render_params& p, int tid) {
    float* w1 = smem;
    float* w2 = w1 + 64 * kW1Pitch;
    float* b1 = w2 + 33 * kW2Pitch;
    float* b2 = b1 + 64;
    for (int i = tid; i < 64 * 32; i += THREADS) w1[(i >> 5) * kW1Pitch + (i & 31)] = p.w1[i];
    for (int i = tid; i < 33 * 64; i += THREADS) w2[(i >> 6) * kW2Pitch + (i & 63)] = p.w2[i];
    if (tid < 64) b1[tid] = p.b1[tid];
    if (tid < 36) b2[tid] = tid < 33 ? p.b2[tid] : 0.f;
    __syncthreads();
    L.w1 = w1; L.w2 = w2; L.b1 = b1; L.b2 = b2;
}

// d(colour) / d(pre-activation): rgb = 1.002 sigmoid(o) - 0.001 (triplane.py:134; sigmoid_rgb_hw is the forward), from the sigmoid or from o
__device__ __forceinline__ float rgb_slope_of_sigmoid(float s) { return 1.002f * s * (1.f - s); }
__device__ __forceinline__ float rgb_slope_hw(float o) {
    const float e = __builtin_amdgcn_exp2f(o * -1.44269504088896341f);
    return rgb_slope_of_sigmoid(__builtin_amdgcn_rcpf(1.0f + e));
}


#ifdef GNERF_ABLATE_ATOMIC       // timing-only build: plain stores instead of atomics (wrong results)
#define GNERF_SCATTER_ADD(ptr, val) (*(ptr) = (val))
#else
#define GNERF_SCATTER_ADD(ptr, val) unsafeAtomicAdd(ptr, val)
#endif

struct BwdRay { float ox, oy, oz, dx, dy, dz; const char* planes; };

// sample j of tile `tile` of a ray: depth from t_list (clamped to the last real sample for tile padding)
struct RayTilePos {
    const BwdRay& R; const float* t_list; int count, tile; float box_scale;
    __device__ __forceinline__ void operator()(int j, float& px, float& py, float& pz) const {
        const float depth = t_list[min(16 * tile + j, count - 1)];
        px = __fadd_rn(R.ox, __fmul_rn(depth, R.dx)) * box_scale;
        py = __fadd_rn(R.oy, __fmul_rn(depth, R.dy)) * box_scale;
        pz = __fadd_rn(R.oz, __fmul_rn(depth, R.dz)) * box_scale;
    }
};
// sample j of a tile whose 16 depths are listed (the staged backward's blocks are in depth order)
struct DepthListPos {
    const BwdRay& R; const float* dep; float box_scale;
    __device__ __forceinline__ void operator()(int j, float& px, float& py, float& pz) const {
        const float depth = dep[j];
        px = __fadd_rn(R.ox, __fmul_rn(depth, R.dx)) * box_scale;
        py = __fadd_rn(R.oy, __fmul_rn(depth, R.dy)) * box_scale;
        pz = __fadd_rn(R.oz, __fmul_rn(depth, R.dz)) * box_scale;
    }
};

// A tile's plane-gradient scatter that has not been issued yet: dX[16][32] sits in tbuf, its tap records in taps.
// It is issued from inside the NEXT tile's lookup, after that tile's texel loads: the wave then waits only for the
// loads, and the atomics drain while the next tile's MLP runs.  (Issued right after dX is produced, the next lookup's
// s_waitcnt vmcnt would wait for every atomic to be acknowledged by L2 first: atomic and compute time simply add up.)
struct BwdPending { float* base; int live; };

// One sixth of a pending scatter: samples 8a..8a+7 of plane pl; lane = (sample parity, channel).
__device__ __forceinline__ void bwd_scatter_chunk(const BwdLds& L, const BwdPending& pd, int a, int pl, int lane) {
    const int half = lane >> 5, ch = lane & 31;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int smp = 8 * a + 2 * q + half;
        const float val = smp < pd.live ? L.tbuf[smp * kTPitch + ch] : 0.f;
        if (val != 0.f) {                   // exact zeros (padding, samples behind an opaque surface) cost no atomic
            const float* rec = L.taps + smp * kTapDwords + pl * 8;
            const uint4 off = *reinterpret_cast<const uint4*>(rec);
            const v4f wgt = *reinterpret_cast<const v4f*>(rec + 4);
            if (wgt[0] != 0.f) GNERF_SCATTER_ADD(pd.base + (off.x >> 2) + ch, val * wgt[0]);
            if (wgt[1] != 0.f) GNERF_SCATTER_ADD(pd.base + (off.y >> 2) + ch, val * wgt[1]);
            if (wgt[2] != 0.f) GNERF_SCATTER_ADD(pd.base + (off.z >> 2) + ch, val * wgt[2]);
            if (wgt[3] != 0.f) GNERF_SCATTER_ADD(pd.base + (off.w >> 2) + ch, val * wgt[3]);
        }
    }
}

// Tap records of the 16 samples of a tile (lanes 0..47: sample = lane & 15, plane = lane >> 4), then the lookup:
// 8 lanes per texel, 8 samples per step, blended features staged as X[sample][channel].  The records travel through
// hbuf (free between tiles) because `taps` may still hold the pending scatter's records; with KEEP_TAPS they are
// written to `taps` once the pending scatter has been issued.
// `pos(j, px, py, pz)` yields the position of sample j of the tile, already scaled into the planes' [-1,1] frame.
template <bool KEEP_TAPS, class PosFn, bool SCATTER = true>
__device__ __forceinline__ void bwd_gather_tile(const Params& P, const BwdLds& L, const char* planes, PosFn pos, BwdPending& pend, int lane) {
    const int H = P.p.plane_h, W = P.p.plane_w;
    uint4 my_off = make_uint4(0, 0, 0, 0);
    v4f my_wgt = {0.f, 0.f, 0.f, 0.f};
    if (lane < 48) {
        const int j = lane & 15, pl = lane >> 4;
        float px, py, pz;
        pos(j, px, py, pz);
        const float u = pl == 2 ? pz : px;
        const float v = pl == 0 ? py : (pl == 1 ? pz : px);
        plane_taps(H, W, u, v, P.tex_pitch, P.row_pitch, unsigned(pl) * P.plane_pitch, my_off, my_wgt);
        float* rec = L.hbuf + j * kTapDwords + pl * 8;
        *reinterpret_cast<uint4*>(rec) = my_off;
        *reinterpret_cast<v4f*>(rec + 4) = my_wgt;
    }
    lds_wave_sync();
    const int b = lane >> 3, cq16 = (lane & 7) * 16;
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const int js = 8 * a + b;
        v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pl = 0; pl < 3; pl++) {
            const float* rec = L.hbuf + js * kTapDwords + pl * 8;
            const uint4 off = *reinterpret_cast<const uint4*>(rec);
            const v4f wgt = *reinterpret_cast<const v4f*>(rec + 4);
            const v4f t00 = *reinterpret_cast<const v4f*>(planes + off.x + cq16);
            const v4f t01 = *reinterpret_cast<const v4f*>(planes + off.y + cq16);
            const v4f t10 = *reinterpret_cast<const v4f*>(planes + off.z + cq16);
            const v4f t11 = *reinterpret_cast<const v4f*>(planes + off.w + cq16);
            if constexpr (SCATTER) { if (pend.live > 0) bwd_scatter_chunk(L, pend, a, pl, lane); }
            acc += t00 * wgt[0] + t01 * wgt[1] + t10 * wgt[2] + t11 * wgt[3];
        }
        *reinterpret_cast<v4f*>(L.stage + js * kStagePitch + (cq16 >> 2)) = acc;
    }
    pend.live = 0;
    if (KEEP_TAPS && lane < 48) {
        float* rec = L.taps + (lane & 15) * kTapDwords + (lane >> 4) * 8;
        *reinterpret_cast<uint4*>(rec) = my_off;
        *reinterpret_cast<v4f*>(rec + 4) = my_wgt;
    }
    lds_wave_sync();
}

// The same lookup for kernels that hold no scatter state (render_bwd_tiles_kernel): the tile's 24 texel loads run as the forward's ROLLING
// window (shade_tile, render_shade.inl) -- the three planes of step 0 in flight together, and as soon as a plane of step 0 has been
// blended the same plane of step 1 is issued -- instead of six dependent rounds of four loads: with two waves per SIMD a round trip to
// L2 per round was a third of the tile's time.
template <class PosFn>
__device__ __forceinline__ void bwd_gather_tile_rolling(const Params& P, const BwdLds& L, const char* planes, PosFn pos, int lane) {
    const int H = P.p.plane_h, W = P.p.plane_w;
    if (lane < 48) {
        const int j = lane & 15, pl = lane >> 4;
        float px, py, pz;
        pos(j, px, py, pz);
        const float u = pl == 2 ? pz : px;
        const float v = pl == 0 ? py : (pl == 1 ? pz : px);
        uint4 my_off; v4f my_wgt;
        plane_taps(H, W, u, v, P.tex_pitch, P.row_pitch, unsigned(pl) * P.plane_pitch, my_off, my_wgt);
        float* rec = L.hbuf + j * kTapDwords + pl * 8;
        *reinterpret_cast<uint4*>(rec) = my_off;
        *reinterpret_cast<v4f*>(rec + 4) = my_wgt;
    }
    lds_wave_sync();
    const int b = lane >> 3, cq16 = (lane & 7) * 16;
    uint4 off[2][3];
    v4f wgt[2][3], tex[2][3][4];
    auto read_records = [&](int a) {
        const float* rec = L.hbuf + (8 * a + b) * kTapDwords;
#pragma unroll
        for (int pl = 0; pl < 3; pl++) {
            off[a][pl] = *reinterpret_cast<const uint4*>(rec + pl * 8);
            wgt[a][pl] = *reinterpret_cast<const v4f*>(rec + pl * 8 + 4);
        }
    };
    auto issue = [&](int a, int pl) {
#ifdef GNERF_ABLATE_K2GATHER     // timing-only build: no texel loads (outputs are wrong)
        tex[a][pl][0] = (v4f){float(off[a][pl].x + cq16), 1.f, 2.f, 3.f}; tex[a][pl][1] = (v4f){float(off[a][pl].y), 1.f, 2.f, 3.f};
        tex[a][pl][2] = (v4f){float(off[a][pl].z), 1.f, 2.f, 3.f};        tex[a][pl][3] = (v4f){float(off[a][pl].w), 1.f, 2.f, 3.f};
        return;
#endif
        tex[a][pl][0] = *reinterpret_cast<const v4f*>(planes + (off[a][pl].x + cq16));
        tex[a][pl][1] = *reinterpret_cast<const v4f*>(planes + (off[a][pl].y + cq16));
        tex[a][pl][2] = *reinterpret_cast<const v4f*>(planes + (off[a][pl].z + cq16));
        tex[a][pl][3] = *reinterpret_cast<const v4f*>(planes + (off[a][pl].w + cq16));
    };
    auto blend = [&](int a, int pl, v4f& acc) {                 // the forward's chain (shade_tile): same features, same bits
        auto bc = [](float w) { return (v4f){w, w, w, w}; };
        acc = pl == 0 ? tex[a][pl][0] * wgt[a][pl][0] : __builtin_elementwise_fma(tex[a][pl][0], bc(wgt[a][pl][0]), acc);
        acc = __builtin_elementwise_fma(tex[a][pl][1], bc(wgt[a][pl][1]), acc);
        acc = __builtin_elementwise_fma(tex[a][pl][2], bc(wgt[a][pl][2]), acc);
        acc = __builtin_elementwise_fma(tex[a][pl][3], bc(wgt[a][pl][3]), acc);
    };
    v4f acc0, acc1;
    read_records(0);
    issue(0, 0); issue(0, 1); issue(0, 2);
    read_records(1);
    __builtin_amdgcn_sched_barrier(0);
    blend(0, 0, acc0); issue(1, 0);
    __builtin_amdgcn_sched_barrier(0);
    blend(0, 1, acc0); issue(1, 1);
    __builtin_amdgcn_sched_barrier(0);
    blend(0, 2, acc0); issue(1, 2);
    __builtin_amdgcn_sched_barrier(0);
    *reinterpret_cast<v4f*>(L.stage + b * kStagePitch + (lane & 7) * 4) = acc0;
    blend(1, 0, acc1); blend(1, 1, acc1); blend(1, 2, acc1);
    *reinterpret_cast<v4f*>(L.stage + (8 + b) * kStagePitch + (lane & 7) * 4) = acc1;
    lds_wave_sync();
}

// MLP forward on the staged tile: h = softplus(W1 x + b1) in the H^T layout (lane: sample j, hidden 16m+4g+r),
// o = colour pre-activations (lane: sample 4g+r, output 1+16n+j), sig = density of sample j.
__device__ __forceinline__ void bwd_mlp_forward(const BwdLds& L, int lane, v4f (&h)[4], v4f (&o)[2], float& sig) {
    const int j = lane & 15, g = lane >> 4;
    const v4f f_lo = *reinterpret_cast<const v4f*>(L.stage + j * kStagePitch + 8 * g);
    const v4f f_hi = *reinterpret_cast<const v4f*>(L.stage + j * kStagePitch + 8 * g + 4);
    const float f[8] = {f_lo[0], f_lo[1], f_lo[2], f_lo[3], f_hi[0], f_hi[1], f_hi[2], f_hi[3]};
#pragma unroll
    for (int m = 0; m < 4; m++) {
        h[m] = *reinterpret_cast<const v4f*>(L.b1 + 16 * m + 4 * g);
        const v4f a_lo = *reinterpret_cast<const v4f*>(L.w1 + (16 * m + j) * kW1Pitch + 8 * g);
        const v4f a_hi = *reinterpret_cast<const v4f*>(L.w1 + (16 * m + j) * kW1Pitch + 8 * g + 4);
#pragma unroll
        for (int s = 0; s < 4; s++) h[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_lo[s], f[s], h[m], 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 4; s++) h[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_hi[s], f[4 + s], h[m], 0, 0, 0);
    }
    sig = 0.f;
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const v4f ws = *reinterpret_cast<const v4f*>(L.w2 + 16 * m + 4 * g);          // density row W2[0][:]
#pragma unroll
        for (int r = 0; r < 4; r++) {
            h[m][r] = softplus_hw(h[m][r]);
            sig += ws[r] * h[m][r];
        }
    }
    sig += __shfl_xor(sig, 16);
    sig += __shfl_xor(sig, 32);
    sig += L.b2[0];
#pragma unroll
    for (int n = 0; n < 2; n++) {
        const float bias = L.b2[1 + 16 * n + j];
        o[n] = (v4f){bias, bias, bias, bias};
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const v4f bw = *reinterpret_cast<const v4f*>(L.w2 + (1 + 16 * n + j) * kW2Pitch + 16 * m + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; r++) o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(h[m][r], bw[r], o[n], 0, 0, 0);
        }
    }
}

// Forward-only walk of `ntiles` tiles: densities -> sig_e[e0...], q -> q_e[e0...].
// G[n] = dL/d(colour sum) of channel 16n + (lane & 15), i.e. 2 * grad_rgb.
template <bool STAGED>
__device__ __forceinline__ void bwd_forward_tiles(const Params& P, const BwdLds& L, const BwdRay& R, int e0, int count, int ntiles,
                                                  const float (&G)[2], BwdPending& pend, int lane) {
    const int j = lane & 15, g = lane >> 4;
    for (int t = 0; t < ntiles; t++) {
        bwd_gather_tile<false, RayTilePos, !STAGED>(P, L, R.planes, RayTilePos{R, L.t_e + e0, count, t, P.box_scale}, pend, lane);
        v4f h[4], o[2];
        float sig;
        bwd_mlp_forward(L, lane, h, o, sig);
        if (g == 0 && 16 * t + j < count) L.sig_e[e0 + 16 * t + j] = sig;
        v4f q;
#pragma unroll
        for (int r = 0; r < 4; r++) q[r] = row_total(G[0] * sigmoid_rgb_hw(o[0][r]) + G[1] * sigmoid_rgb_hw(o[1][r]));
        if (j == 15) *reinterpret_cast<v4f*>(L.q_e + e0 + 16 * t + 4 * g) = q;
    }
    lds_wave_sync();
}

// Per-wave accumulators of the decoder gradients (summed over every sample the wave shades).
struct BwdAcc {
    v4f w1[4][2];     // dW1[16m + 4g + r][16c + j]
    v4f w2[2][4];     // dW2[1 + 16o + 4g + r][16n + j]
    v4f w2s[4];       // dW2[0][16m + 4g + r], partial over the samples on this lane's column
    v4f b1[4];        // db1[16m + 4g + r], partial likewise
    float b2[2];      // db2[1 + 16n + j], partial over this lane's sample rows
    float b2s;        // db2[0], partial
};

// The colour half of dH^T[hidden][sample] = sum_out W2[out][hidden] dO[sample][out], dO[16][32] in `tbuf`, added to dh (the H^T layout)
__device__ __forceinline__ void bwd_dh_add_colour(const BwdLds& L, int j, int g, v4f (&dh)[4]) {
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const float bT = L.tbuf[j * kTPitch + 4 * s + g];
#pragma unroll
        for (int m = 0; m < 4; m++)
            dh[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(L.w2[(1 + 4 * s + g) * kW2Pitch + 16 * m + j], bT, dh[m], 0, 0, 0);
    }
}

// The decoder's backward pass for one staged tile.  On entry: X in `stage`, dO[16][32] (colour pre-activation gradients)
// in `tbuf`, h = the hidden activations (H^T layout), dsig = dL/dsigma of this lane's sample.  Accumulates the weight
// gradients into A and leaves dX[16][32] in `tbuf`.
__device__ __forceinline__ void bwd_tile_core(const BwdLds& L, v4f (&h)[4], float dsig, BwdAcc& A, int lane) {
    const int j = lane & 15, g = lane >> 4;
    if (g == 0) A.b2s += dsig;
    lds_wave_sync();
    // ---- dH^T[hidden][sample] = sum_out W2[out][hidden] dO[sample][out]  (+ the density row on the vector ALU)
    v4f dh[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const v4f ws = *reinterpret_cast<const v4f*>(L.w2 + 16 * m + 4 * g);
        dh[m] = ws * dsig;
        A.w2s[m] += h[m] * dsig;
    }
    bwd_dh_add_colour(L, j, g, dh);
    // ---- through softplus: d/dpre softplus(pre) = 1 - exp(-softplus(pre))
#pragma unroll
    for (int m = 0; m < 4; m++) {
#pragma unroll
        for (int r = 0; r < 4; r++) dh[m][r] *= 1.f - exp_hw(-h[m][r]);
        A.b1[m] += dh[m];
        *reinterpret_cast<v4f*>(L.hbuf + j * kHPitch + 16 * m + 4 * g) = h[m];
    }
    lds_wave_sync();
    // ---- dW2[out][hidden] += sum_sample dO[sample][out] H[sample][hidden]
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float a0 = L.tbuf[(4 * g + r) * kTPitch + j], a1 = L.tbuf[(4 * g + r) * kTPitch + 16 + j];
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const float bh = L.hbuf[(4 * g + r) * kHPitch + 16 * n + j];
            A.w2[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bh, A.w2[0][n], 0, 0, 0);
            A.w2[1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bh, A.w2[1][n], 0, 0, 0);
        }
    }
    lds_wave_sync();
    // ---- dX^T[channel][sample] = sum_hidden W1[hidden][channel] dPRE^T[hidden][sample]
    v4f dx[2];
    dx[0] = dx[1] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < 4; m++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float* row = L.w1 + (16 * m + 4 * g + r) * kW1Pitch + j;
            dx[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[0], dh[m][r], dx[0], 0, 0, 0);
            dx[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[16], dh[m][r], dx[1], 0, 0, 0);
        }
        *reinterpret_cast<v4f*>(L.hbuf + j * kHPitch + 16 * m + 4 * g) = dh[m];             // dPRE[sample][hidden]
    }
    *reinterpret_cast<v4f*>(L.tbuf + j * kTPitch + 4 * g) = dx[0];                            // dX[sample][channel]
    *reinterpret_cast<v4f*>(L.tbuf + j * kTPitch + 16 + 4 * g) = dx[1];
    lds_wave_sync();
    // ---- dW1[hidden][channel] += sum_sample dPRE[sample][hidden] X[sample][channel]
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float b0 = L.stage[(4 * g + r) * kStagePitch + j], b1 = L.stage[(4 * g + r) * kStagePitch + 16 + j];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const float ap = L.hbuf[(4 * g + r) * kHPitch + 16 * m + j];
            A.w1[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap, b0, A.w1[m][0], 0, 0, 0);
            A.w1[m][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap, b1, A.w1[m][1], 0, 0, 0);
        }
    }
}

// `stage_ray`: when not NULL the plane gradient is NOT scattered from here: each sample's dX row (32 floats) is written to
// stage_ray[rank * 32 ...], rank = the sample's position in the ray's merged depth order, for plane_scatter_kernel below.
template <bool STAGED>
__device__ __forceinline__ void bwd_backward_tiles(const Params& P, const BwdLds& L, const BwdRay& R, float* grad_planes_item, float* stage_ray,
                                                   int e0, int count, int ntiles, const float (&G)[2], BwdAcc& A, BwdPending& pend, int lane) {
    const int j = lane & 15, g = lane >> 4;
    for (int t = 0; t < ntiles; t++) {
        bwd_gather_tile<!STAGED, RayTilePos, !STAGED>(P, L, R.planes, RayTilePos{R, L.t_e + e0, count, t, P.box_scale}, pend, lane);
#ifdef GNERF_ABLATE_BWDMLP      // timing-only build: lookup + scatter without the decoder's backward pass (wrong results)
        for (int i = lane; i < 16 * kTPitch; i += 64) L.tbuf[i] = L.stage[i];
        if (grad_planes_item) { pend.base = grad_planes_item; pend.live = min(16, count - 16 * t); }
        lds_wave_sync();
        continue;
#endif
        v4f h[4], o[2];
        float sig;
        bwd_mlp_forward(L, lane, h, o, sig);
        // ---- dO: colour c = 1.002 * s - 0.001 with s = sigmoid(o); dL/dc = G * v_sample  (triplane.py:134, ray_marcher.py:27-45)
        const v4f vs = *reinterpret_cast<const v4f*>(L.v_e + e0 + 16 * t + 4 * g);
        const float dsig = L.dsig_e[e0 + 16 * t + j];
#pragma unroll
        for (int n = 0; n < 2; n++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                // rgb_slope_hw, kept as a copy: through the helper render_bwd_kernel's instructions change
                const float e = __builtin_amdgcn_exp2f(o[n][r] * -1.44269504088896341f);
                const float s = __builtin_amdgcn_rcpf(1.0f + e);
                const float d = G[n] * vs[r] * (1.002f * s * (1.f - s));
                L.tbuf[(4 * g + r) * kTPitch + 16 * n + j] = d;
                A.b2[n] += d;
            }
        }
        bwd_tile_core(L, h, dsig, A, lane);
        if constexpr (STAGED) {
            // ---- dX rows to the staging buffer in depth order: two 128-byte rows per store instruction
            const int half = lane >> 5, ch = lane & 31;
            const int live = min(16, count - 16 * t);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int smp = 2 * q + half;
                if (smp < live) stage_ray[L.rank_e[e0 + 16 * t + smp] * 32 + ch] = L.tbuf[smp * kTPitch + ch];
            }
        } else if (grad_planes_item) {
            // ---- dX goes to the plane gradient from inside the next lookup (see BwdPending)
            pend.base = grad_planes_item; pend.live = min(16, count - 16 * t);
        }
        lds_wave_sync();
    }
}

// Decoder gradients: wave registers -> workgroup LDS (aliases the staged decoder) -> one global atomic per element.
// Every thread of the workgroup must call (barriers inside).
__device__ __forceinline__ void bwd_reduce_decoder_grads(const BwdAcc& A, float* smem, float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2,
                                                         int tid, int lane, int j, int nthreads = kBwdThreads) {
    if (!grad_w1) return;
    __syncthreads();                                   // every wave is done with the LDS decoder
    float* red = smem;
    float* red_w1 = red, *red_b1 = red_w1 + 64 * 32, *red_w2 = red_b1 + 64, *red_b2 = red_w2 + 33 * 64;
    for (int i = tid; i < kBwdGradFloats; i += nthreads) red[i] = 0.f;
    __syncthreads();
    {
        const int g = lane >> 4;
#pragma unroll
        for (int m = 0; m < 4; m++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int hid = 16 * m + 4 * g + r;
                atomicAdd(red_w1 + hid * 32 + j, A.w1[m][0][r]);
                atomicAdd(red_w1 + hid * 32 + 16 + j, A.w1[m][1][r]);
                const float s0 = row_total(A.w2s[m][r]), s1 = row_total(A.b1[m][r]);
                if (j == 15) { atomicAdd(red_w2 + hid, s0); atomicAdd(red_b1 + hid, s1); }
            }
        }
#pragma unroll
        for (int o = 0; o < 2; o++) {
#pragma unroll
            for (int n = 0; n < 4; n++) {
#pragma unroll
                for (int r = 0; r < 4; r++) atomicAdd(red_w2 + (1 + 16 * o + 4 * g + r) * 64 + 16 * n + j, A.w2[o][n][r]);
            }
            float s = A.b2[o];
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            if (g == 0) atomicAdd(red_b2 + 1 + 16 * o + j, s);
        }
        const float s = wave_sum(A.b2s);
        if (lane == 0) atomicAdd(red_b2, s);
    }
    __syncthreads();
    for (int i = tid; i < 64 * 32; i += nthreads) unsafeAtomicAdd(grad_w1 + i, red_w1[i]);
    for (int i = tid; i < 33 * 64; i += nthreads) unsafeAtomicAdd(grad_w2 + i, red_w2[i]);
    if (tid < 64) unsafeAtomicAdd(grad_b1 + tid, red_b1[tid]);
    if (tid < 33) unsafeAtomicAdd(grad_b2 + tid, red_b2[tid]);
}

}  // namespace
