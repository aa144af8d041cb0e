// Backward pass of the fused renderer: the one-wave-per-ray kernel and the sorted scatter.  Included by render_backward.hip alone; the tile
// helpers that the point queries borrow are in render_bwd_tile.inl, the tile kernel of the pipelined path in render_bwd_tiles.inl.
//
// Upstream this is autograd walking the graph of ImportanceRenderer.forward (renderer.py:88-140) backwards:
// the composite of ray_marcher.py:25-57, the sort/gather of renderer.py:150-167, the decoder's two linear layers
// (triplane.py:113-136) and grid_sample's backward (grid_sample_gradfix.py:62-77), with ~4 GB of saved
// intermediates at the training shape.  Here nothing is saved: ONE WAVE OWNS A RAY and
//   1. recomputes the forward pass of its ray (same depth proposals, lookups, MLP, coarse march, importance
//      resampling, merge, final march) keeping only per-sample scalars in LDS -- in place of each sample's
//      32 colours it keeps q_j = sum_c dL/drgb[c] * colour_j[c], which is all the composite's gradient needs;
//   2. runs the composite's gradient as wave scans over the sorted intervals: dL/dw_k, the suffix sums that
//      carry the transmittance dependence, dL/dsigma of every sample and the colour weights v_j;
//   3. walks the sample tiles once more: lookup + MLP forward again, then dO -> dH -> dPRE -> dX on the matrix
//      cores (exact fp32 v_mfma_f32_16x16x4_f32; operands change roles through small LDS transposes), the
//      weight gradients dW2 += dO^T H and dW1 += dPRE^T X accumulated in registers across all rays of the wave,
//      and dX scattered into the plane gradient with one hardware float atomic per (tap, channel).
// Four waves (four rays) share a workgroup and one LDS copy of the decoder; the weight gradients are reduced
// in LDS per workgroup and leave with one atomic per element.
//
// Conventions as in render.hip's generic kernel: MFMA D layout col = lane & 15, rows = 4 * (lane >> 4) + r.

#pragma once
#include "render_bwd_tile.inl"

namespace {

// STAGED: the plane gradient leaves through the staging buffer (`stage` != NULL, a plane gradient is requested): no tap records are
// kept and no scatter code is compiled in.
#ifndef GNERF_BWD_WAVE_OCC
#define GNERF_BWD_WAVE_OCC 2        // waves per SIMD the one-wave-per-ray kernel is compiled for (1: up to 512 registers, no spills)
#endif
template <bool STAGED>
__global__ __launch_bounds__(kBwdThreads, GNERF_BWD_WAVE_OCC) void render_bwd_kernel(Params P, gnerf_render_grads Gr, float* stage) {
    extern __shared__ __align__(16) float smem[];
    const gnerf_render_params& p = P.p;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int S = p.depth_resolution, F = p.depth_resolution_importance;
    const int s_pad = 16 * (P.tiles_c + P.tiles_f);
    const int n_all = S + F;
    const int fine_e0 = 16 * P.tiles_c;

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

    BwdLds L;
    L.w1 = w1; L.w2 = w2; L.b1 = b1; L.b2 = b2;
    float* base = smem + kBwdWeightFloats + size_t(wv) * bwd_wave_floats(s_pad);
    L.t_e = base;               L.sig_e = L.t_e + s_pad;   L.q_e = L.sig_e + s_pad;  L.v_e = L.q_e + s_pad;
    L.dsig_e = L.v_e + s_pad;   L.rank_e = reinterpret_cast<int*>(L.dsig_e + s_pad);
    L.s_t = L.dsig_e + 2 * s_pad;  L.s_sig = L.s_t + s_pad;  L.s_q = L.s_sig + s_pad;  L.w_s = L.s_q + s_pad;
    L.trans = L.w_s + s_pad;    L.ds = L.trans + s_pad;
    L.stage = L.ds + s_pad;     L.tbuf = L.stage + 16 * kStagePitch;  L.hbuf = L.tbuf + 16 * kTPitch;  L.taps = L.hbuf + 16 * kHPitch;

    BwdAcc A;
#pragma unroll
    for (int m = 0; m < 4; m++) {
        A.w1[m][0] = A.w1[m][1] = A.w2[0][m] = A.w2[1][m] = A.w2s[m] = A.b1[m] = (v4f){0.f, 0.f, 0.f, 0.f};
    }
    A.b2[0] = A.b2[1] = A.b2s = 0.f;
    BwdPending pend = {nullptr, 0};

    // ray tiles: workgroup `blk` owns tiles 4*blk .. 4*blk+3 (one per wave); XCD-contiguous like the forward kernels
    // Small launches (the training shape is 1 024 tiles = one wave per SIMD): a tile's 16 rays are shared by 1 << split_shift waves
    const int n_groups = P.n_tiles << P.split_shift;
    const int n_blocks = (n_groups + kBwdWaves - 1) / kBwdWaves;
    const int per_xcd = (n_blocks + kNumXCD - 1) / kNumXCD;
    const int blk = (blockIdx.x % kNumXCD) * per_xcd + blockIdx.x / kNumXCD;
    const int group = blk * kBwdWaves + wv;
    const int tile = group >> P.split_shift;
    const bool have_tile = blk < n_blocks && group < n_groups;
    const int rr_count = kBwdRaysPerWave >> P.split_shift;
    const int rr_first = (group & ((1 << P.split_shift) - 1)) * rr_count;
    const int64_t plane_floats = int64_t(3) * p.plane_h * p.plane_w * 32;
    const int j = lane & 15;

    for (int rr = rr_first; have_tile && rr < rr_first + rr_count; rr++) {
        int64_t ray;
        if (P.tiles_per_item > 0) {
            const int item = tile / P.tiles_per_item, tt = tile % P.tiles_per_item;
            const int tx = tt / P.tiles_y, ty = tt % P.tiles_y;
            ray = int64_t(item) * p.rays_per_item + int64_t(ty * 4 + (rr >> 2)) * p.image_width + tx * 4 + (rr & 3);
        } else {
            ray = int64_t(tile) * kBwdRaysPerWave + rr;
            if (ray >= P.total_rays) break;
        }
        const int item = int(ray / p.rays_per_item);
        BwdRay R;
        R.ox = p.ray_origins[ray * 3 + 0]; R.oy = p.ray_origins[ray * 3 + 1]; R.oz = p.ray_origins[ray * 3 + 2];
        R.dx = p.ray_dirs[ray * 3 + 0]; R.dy = p.ray_dirs[ray * 3 + 1]; R.dz = p.ray_dirs[ray * 3 + 2];
        R.planes = reinterpret_cast<const char*>(p.planes_nhwc + int64_t(item) * plane_floats);
        float* grad_planes_item = Gr.grad_planes_nhwc ? Gr.grad_planes_nhwc + int64_t(item) * plane_floats : nullptr;
        // incoming gradients; rgb = 2 * composite - 1 (ray_marcher.py:55)
        float G[2];
        G[0] = Gr.grad_rgb ? 2.f * Gr.grad_rgb[ray * 32 + j] : 0.f;
        G[1] = Gr.grad_rgb ? 2.f * Gr.grad_rgb[ray * 32 + 16 + j] : 0.f;
        const float g_depth = Gr.grad_depth ? Gr.grad_depth[ray] : 0.f;
        const float g_wsum = Gr.grad_wsum ? Gr.grad_wsum[ray] : 0.f;
        const float g_sum = wave_sum(lane < 16 ? G[0] + G[1] : 0.f);

        // ---- 1. forward recomputation
        for (int k = lane; k < S; k += 64) L.t_e[k] = coarse_depth(P, ray, k);
        for (int k = lane; k < s_pad; k += 64) { L.v_e[k] = 0.f; L.dsig_e[k] = 0.f; L.q_e[k] = 0.f; }
        lds_wave_sync();
        bwd_forward_tiles<STAGED>(P, L, R, 0, S, P.tiles_c, G, pend, lane);
        if (F > 0) {
            float w_sum, wt_sum;
            march(L.t_e, L.sig_e, L.w_s, S, lane, w_sum, wt_sum);
            lds_wave_sync();
            resample_fine(P, ray, L.t_e, L.w_s, L.s_sig, L.trans, L.t_e + fine_e0, nullptr, n_all, lane, [] { lds_wave_sync(); });
            bwd_forward_tiles<STAGED>(P, L, R, fine_e0, F, P.tiles_f, G, pend, lane);
            merge_by_depth(L.t_e, L.sig_e, L.rank_e, L.s_t, L.s_sig, S, F, fine_e0, lane);
        } else {
            for (int k = lane; k < S; k += 64) { L.rank_e[k] = k; L.s_t[k] = L.t_e[k]; L.s_sig[k] = L.sig_e[k]; }
        }
        lds_wave_sync();
        for (int q = lane; q < n_all; q += 64) {
            const int e = q < S ? q : fine_e0 + (q - S);
            L.s_q[L.rank_e[e]] = L.q_e[e];
        }
        // final march, keeping the transmittance in front of every interval (ray_marcher.py:26-42)
        float w_sum, wt_sum;
        {
            float carry = 1.f, acc_w = 0.f, acc_wt = 0.f;
            for (int kb = 0; kb < n_all - 1; kb += 64) {
                const int k = kb + lane;
                const bool ok = k < n_all - 1;
                float alpha = 0.f, tmid = 0.f;
                if (ok) {
                    const float t0 = L.s_t[k], t1 = L.s_t[k + 1];
                    const float smid = softplus_march((L.s_sig[k] + L.s_sig[k + 1]) * 0.5f - 1.f);
                    tmid = (t0 + t1) * 0.5f;
                    alpha = 1.f - exp_hw(-(smid * (t1 - t0)));
                }
                const float x = ok ? (1.f - alpha + 1e-10f) : 1.f;
                const float incl = wave_scan_mul(x, lane);
                const float tr = wave_shift_up(incl, 1.f) * carry;
                carry *= wave_last(incl);
                if (ok) { const float wk = alpha * tr; L.w_s[k] = wk; L.trans[k] = tr; acc_w += wk; acc_wt += wk * tmid; }
            }
            w_sum = wave_sum(acc_w);
            wt_sum = wave_sum(acc_wt);
        }
        lds_wave_sync();

        // ---- 2. gradient of the composite.  With q_k = sum_c G[c] colour_k[c]:
        //   dL/dw_k = (q_k + q_{k+1}) / 2 - [white_back] sum_c G[c] + g_depth (tmid_k - depth) / W + g_wsum
        //   dL/dalpha_k = dL/dw_k T_k - (sum_{m>k} dL/dw_m w_m) / (1 - alpha_k + 1e-10)
        const float depth = wt_sum / w_sum;
        const float gd_scale = (w_sum > 0.f && depth == depth) ? g_depth / w_sum : 0.f;     // nan_to_num'd rays pass no depth gradient
        const float gw_const = g_wsum - (p.white_back ? g_sum : 0.f);
        const int n_int = n_all - 1;
        float carry = 0.f;
        for (int kb = 0; kb < n_int; kb += 64) {               // walk the intervals from the far end: suffix sums are prefix sums here
            const int k = n_int - 1 - (kb + lane);
            const bool ok = k >= 0;
            float gw = 0.f, wk = 0.f, t0 = 0.f, t1 = 0.f, smid_in = 0.f;
            if (ok) {
                t0 = L.s_t[k]; t1 = L.s_t[k + 1];
                smid_in = (L.s_sig[k] + L.s_sig[k + 1]) * 0.5f - 1.f;
                wk = L.w_s[k];
                gw = (L.s_q[k] + L.s_q[k + 1]) * 0.5f + gw_const + gd_scale * ((t0 + t1) * 0.5f - depth);
            }
            const float incl = wave_scan_add(gw * wk, lane) + carry;
            carry = wave_last(incl);
            if (ok) {
                const float after = incl - gw * wk;                      // sum over m > k
                const float delta = t1 - t0;
                const float dens = softplus_march(smid_in);
                const float one_minus_alpha = exp_hw(-(dens * delta));
                const float alpha = 1.f - one_minus_alpha;
                const float d_alpha = gw * L.trans[k] - after / (1.f - alpha + 1e-10f);
                const float d_dens = d_alpha * delta * one_minus_alpha;
                const float e = exp_hw(-smid_in);
                const float d_smid = smid_in > 20.f ? d_dens : d_dens * __builtin_amdgcn_rcpf(1.f + e);      // softplus' = sigmoid
                L.ds[k] = d_smid;
            }
        }
        lds_wave_sync();
        for (int q = lane; q < n_all; q += 64) {
            const int e = q < S ? q : fine_e0 + (q - S);
            const int r = L.rank_e[e];
            const float wl = r > 0 ? L.w_s[r - 1] : 0.f, wr = r < n_int ? L.w_s[r] : 0.f;
            const float dl = r > 0 ? L.ds[r - 1] : 0.f, dr = r < n_int ? L.ds[r] : 0.f;
            L.v_e[e] = (wl + wr) * 0.5f;                 // colour of sample r enters intervals r-1 and r with weight 1/2 each
            L.dsig_e[e] = (dl + dr) * 0.5f;              // so does its density
        }
        lds_wave_sync();

        // ---- 3. decoder + lookup gradients
        float* stage_ray = nullptr;
        if constexpr (STAGED) {                         // staged scatter: per ray n_all depths, then n_all rows of 32 floats
            stage_ray = stage + ray * int64_t(n_all) * 33 + n_all;
            for (int k = lane; k < n_all; k += 64) stage[ray * int64_t(n_all) * 33 + k] = L.s_t[k];
        }
        bwd_backward_tiles<STAGED>(P, L, R, grad_planes_item, stage_ray, 0, S, P.tiles_c, G, A, pend, lane);
        if (F > 0) bwd_backward_tiles<STAGED>(P, L, R, grad_planes_item, stage_ray, fine_e0, F, P.tiles_f, G, A, pend, lane);
    }
    if constexpr (!STAGED) {
        if (pend.live > 0) {                           // the last tile's scatter has no next lookup to hide in
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int pl = 0; pl < 3; pl++) bwd_scatter_chunk(L, pend, a, pl, lane);
        }
    }

    bwd_reduce_decoder_grads(A, smem, Gr.grad_w1, Gr.grad_b1, Gr.grad_w2, Gr.grad_b2, tid, lane, j);
}

// ---------------------------------------------------------------------------------------------
// Staged plane-gradient scatter, second pass (round 2).  render_bwd_kernel above is bound by the device's float-atomic rate: every
// (sample, tap) costs two 64-byte atomic requests that are resolved at the memory side, 149 M per launch at BASELINE config 2.  A
// 4x4-pixel ray tile touches each texel ~4-5 times, mostly from samples at similar depth on neighbouring rays, but the first
// pass has neither LDS (2 x 79 KB per CU) nor registers (256) left to aggregate them.  So, when the caller provides a staging
// buffer, the first pass writes each sample's dX row in its ray's merged DEPTH ORDER and this kernel does the scatter: one
// workgroup per 16-ray tile walks the tile's samples in chunks of kScatterRanks depth ranks (all 16 rays at once) and SORTS the
// chunk's 2 304 tap contributions by texel with a counting sort in LDS -- texel -> table slot by compare-and-swap on integer tags
// (open addressing at a load of ~0.3), a counter per slot that also hands each contribution its place in the slot's bucket, a prefix
// sum, a scatter of (sample, weight) pairs -- after which every half-wave sums whole buckets from the chunk's dX rows in LDS and
// sends ONE global atomic per texel and channel.  (A first version accumulated into an LDS table with float LDS atomics: those
// run at ~0.4 lanes per cycle here and made this pass 14 ms; the sort needs integer atomics only, 2 304 per chunk.)
// A contribution that finds no free slot goes straight to global memory, so correctness never depends on the table.
constexpr int kScatterThreads = 1024, kScatterSlots = 2048, kScatterRanks = 16, kScatterProbes = 16;
constexpr unsigned kScatterEmpty = 0xffffffffu;
constexpr int kScatterSamples = 16 * kScatterRanks;             // samples of one chunk
constexpr int kScatterEntries = kScatterSamples * 12;           // tap contributions of one chunk
static_assert(kScatterSlots <= (1 << 11) && kScatterSamples * 32 <= (1 << 13), "an entry packs slot and dX row offset into 24 bits");
static_assert(kScatterSamples * 3 <= kScatterThreads && kScatterSlots == 2 * kScatterThreads, "one thread per (sample, plane), two slots per thread in the scan");
__host__ __device__ inline size_t scatter_lds_floats() {
    return 16 * 8 + size_t(kScatterSamples) * 32 + 2 * size_t(kScatterSlots) + 2 + 2 * size_t(kScatterEntries) + 32;
}

__global__ __launch_bounds__(kScatterThreads, 8) void plane_scatter_kernel(Params P, const float* __restrict__ stage, float* __restrict__ grad_planes) {
    extern __shared__ __align__(16) float smem[];
    const gnerf_render_params& p = P.p;
    float* rays = smem;                                                        // [16][o, d, ray id, -]
    float* dx = rays + 16 * 8;                                                 // [samples][32]
    unsigned* tag = reinterpret_cast<unsigned*>(dx + kScatterSamples * 32);    // [slots] texel key, or empty
    int* cnt = reinterpret_cast<int*>(tag + kScatterSlots);                    // [slots + 1] bucket sizes, then (in place) bucket starts
    float2* entry = reinterpret_cast<float2*>(cnt + kScatterSlots + 2);        // [entries] (sample of the chunk, bilinear weight)
    int* wave_tot = reinterpret_cast<int*>(entry + kScatterEntries);           // [16]
    const int tid = threadIdx.x, lane = tid & 63, ch = lane & 31, wv = tid >> 6;
    const int hw = tid >> 5;                                                   // half-wave index
    const int n_all = p.depth_resolution + p.depth_resolution_importance;
    const int tile = blockIdx.x;
    const int H = p.plane_h, W = p.plane_w;
    if (tid < 16) {                                                            // the tile's 16 rays (the first pass's tile order)
        int64_t ray = -1;
        if (P.tiles_per_item > 0) {
            const int item = tile / P.tiles_per_item, tt = tile % P.tiles_per_item;
            const int tx = tt / P.tiles_y, ty = tt % P.tiles_y;
            ray = int64_t(item) * p.rays_per_item + int64_t(ty * 4 + (tid >> 2)) * p.image_width + tx * 4 + (tid & 3);
        } else {
            ray = int64_t(tile) * 16 + tid;
            if (ray >= P.total_rays) ray = -1;
        }
        float* r = rays + tid * 8;
        if (ray >= 0) {
            r[0] = p.ray_origins[ray * 3 + 0]; r[1] = p.ray_origins[ray * 3 + 1]; r[2] = p.ray_origins[ray * 3 + 2];
            r[3] = p.ray_dirs[ray * 3 + 0];    r[4] = p.ray_dirs[ray * 3 + 1];    r[5] = p.ray_dirs[ray * 3 + 2];
        }
        reinterpret_cast<int*>(r)[6] = int(ray);
    }
    for (int i = tid; i < kScatterSlots; i += kScatterThreads) { tag[i] = kScatterEmpty; cnt[i] = 0; }
    __syncthreads();
    const int first_ray = reinterpret_cast<const int*>(rays)[6];
    if (first_ray < 0) return;                                                 // (uniform: tiles are filled from ray 0 of the tile)
    const int item = first_ray / p.rays_per_item;                             // a tile never straddles items (checked by the launcher)
    float* grad_item = grad_planes + int64_t(item) * 3 * H * W * 32;

    // A chunk's staged values (its dX rows: eight per half-wave; the depth of this thread's sample) are fetched into registers one chunk
    // AHEAD, at the top of the previous chunk, and made to land before that chunk's global atomics go out.  Loads, stores and
    // returnless atomics share one completion counter (vmcnt) and complete out of order with respect to each other, so a wait for a
    // load behind atomics is a wait for the atomics' acknowledgements too: fetching a chunk at its own top put every chunk behind the
    // round trips of the previous chunk's atomics.
    constexpr int kRowsPerHw = kScatterSamples / (kScatterThreads / 32);
    static_assert(kRowsPerHw * (kScatterThreads / 32) == kScatterSamples, "dX rows divide over the half-waves");
    float pre_dx[kRowsPerHw], pre_depth = 0.f;
    auto prefetch = [&](int k0) {
        const int nk = min(kScatterRanks, n_all - k0);
        const int n_smp = 16 * nk;
#pragma unroll
        for (int q = 0; q < kRowsPerHw; q++) {
            const int sr = hw + q * (kScatterThreads / 32);
            pre_dx[q] = 0.f;
            if (sr < n_smp) {
                const int ray = reinterpret_cast<const int*>(rays + (sr / nk) * 8)[6];
                if (ray >= 0) pre_dx[q] = stage[int64_t(ray) * n_all * 33 + n_all + int64_t(k0 + sr % nk) * 32 + ch];
            }
        }
        const int sr3 = tid / 3;
        pre_depth = 0.f;
        if (sr3 < n_smp) {
            const int ray = reinterpret_cast<const int*>(rays + (sr3 / nk) * 8)[6];
            if (ray >= 0) pre_depth = stage[int64_t(ray) * n_all * 33 + k0 + sr3 % nk];
        }
    };
    prefetch(0);

    for (int k0 = 0; k0 < n_all; k0 += kScatterRanks) {
        const int nk = min(kScatterRanks, n_all - k0);
        const int n_smp = 16 * nk;
        // ---- the chunk's dX rows into LDS (sample sr = ray-in-tile * nk + rank-in-chunk)
#pragma unroll
        for (int q = 0; q < kRowsPerHw; q++) {
            const int sr = hw + q * (kScatterThreads / 32);
            if (sr < n_smp) dx[sr * 32 + ch] = pre_dx[q];
        }
        const float my_depth = pre_depth;
        if (k0 + kScatterRanks < n_all) prefetch(k0 + kScatterRanks);         // in flight during the table / prefix / bucket phases below
        // ---- one thread per (sample, plane): its four taps, a table slot and a place in the slot's bucket for each
        int sp[4] = {-1, -1, -1, -1};                                        // table slot (low 12 bits) | place in its bucket << 12; -1 = no slot
        unsigned keys[4] = {0, 0, 0, 0};
        v4f wgt = {0.f, 0.f, 0.f, 0.f};
        const int my_sr = tid / 3, my_pl = tid % 3;
        const bool mine = my_sr < n_smp;
        if (mine) {
            const float* r = rays + (my_sr / nk) * 8;
            const int ray = reinterpret_cast<const int*>(r)[6];
            if (ray >= 0) {
                const float depth = my_depth;
                const float px = __fadd_rn(r[0], __fmul_rn(depth, r[3])) * P.box_scale;
                const float py = __fadd_rn(r[1], __fmul_rn(depth, r[4])) * P.box_scale;
                const float pz = __fadd_rn(r[2], __fmul_rn(depth, r[5])) * P.box_scale;
                const float u = my_pl == 2 ? pz : px;
                const float v = my_pl == 0 ? py : (my_pl == 1 ? pz : px);
                uint4 off;
                plane_taps(H, W, u, v, P.tex_pitch, P.row_pitch, unsigned(my_pl) * P.plane_pitch, off, wgt);
                keys[0] = off.x; keys[1] = off.y; keys[2] = off.z; keys[3] = off.w;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (wgt[t] != 0.f) {
                        const unsigned h = ((keys[t] >> 7) * 2654435761u) >> 21;               // 11 bits
                        for (int pr = 0; pr < kScatterProbes; pr++) {
                            const unsigned s2 = (h + pr) & (kScatterSlots - 1);
                            const unsigned old = atomicCAS(tag + s2, kScatterEmpty, keys[t]);
                            if (old == kScatterEmpty || old == keys[t]) { sp[t] = int(s2); break; }
                        }
                        if (sp[t] >= 0) sp[t] |= atomicAdd(cnt + sp[t], 1) << 12;
                    }
                }
            }
        }
        __syncthreads();
        // ---- exclusive prefix sum of the bucket sizes (two adjacent slots per thread)
        {
            const int c0 = cnt[2 * tid], c1 = cnt[2 * tid + 1];
            int incl = c0 + c1;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o); if (lane >= o) incl += up; }
            if (lane == 63) wave_tot[wv] = incl;
            __syncthreads();
            int base = 0;
            for (int w2 = 0; w2 < wv; w2++) base += wave_tot[w2];
            cnt[2 * tid] = base + incl - c0 - c1;                              // (every size was read before the barrier above)
            cnt[2 * tid + 1] = base + incl - c1;
            if (tid == kScatterThreads - 1) cnt[kScatterSlots] = base + incl;
        }
        __syncthreads();
        // ---- contributions to their buckets; the rare ones without a slot go straight to memory (32 channels from one lane)
        if (mine) {
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (wgt[t] != 0.f) {
                    if (sp[t] >= 0) {
                        entry[cnt[sp[t] & 4095] + (sp[t] >> 12)] = make_float2(__int_as_float(((sp[t] & 4095) << 13) | (my_sr * 32)), wgt[t]);
                    } else {
                        for (int c2 = 0; c2 < 32; c2++) {
                            const float c = dx[my_sr * 32 + c2] * wgt[t];
                            if (c != 0.f) unsafeAtomicAdd(grad_item + (keys[t] >> 2) + c2, c);
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---- every half-wave walks an equal share of the SORTED contributions (lane = channel), sums runs of one texel from the dX
        // rows in LDS and sends one global atomic per run and channel (a texel whose bucket straddles two shares gets two).
        // Walking entries, four per LDS round trip, instead of the table's slots (two dependent reads per slot, most of them
        // empty) took this pass from 3.16 to 2.70 ms at config 2 (its atomic requests alone need 2.15 ms).
        {
            // the next chunk's values have to be in their registers NOW, before this chunk's atomics are in flight (see above); an
            // empty asm that "rewrites" them makes the compiler wait here and nowhere later
#pragma unroll
            for (int q = 0; q < kRowsPerHw; q++) asm volatile("" : "+v"(pre_dx[q]));
            asm volatile("" : "+v"(pre_depth));
            const int total = cnt[kScatterSlots];
            const int share = (total + kScatterThreads / 32 - 1) / (kScatterThreads / 32);
            const int e0 = hw * share, e1 = min(total, e0 + share);
            int cur = -1;
            float sum = 0.f;
            for (int i = e0; i < e1; i += 4) {
                float2 e[4];
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) e[u] = entry[min(i + u, e1 - 1)];
#pragma unroll
                for (int u = 0; u < 4; u++) v[u] = dx[(__float_as_int(e[u].x) & 8191) + ch];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (i + u < e1) {
                        const int sl = __float_as_int(e[u].x) >> 13;
                        if (sl != cur) {
                            if (cur >= 0 && sum != 0.f) unsafeAtomicAdd(grad_item + (tag[cur] >> 2) + ch, sum);
                            cur = sl;
                            sum = 0.f;
                        }
                        sum = fmaf(e[u].y, v[u], sum);
                    }
                }
            }
            if (cur >= 0 && sum != 0.f) unsafeAtomicAdd(grad_item + (tag[cur] >> 2) + ch, sum);
        }
        __syncthreads();
        for (int i = tid; i < kScatterSlots; i += kScatterThreads) { tag[i] = kScatterEmpty; cnt[i] = 0; }
        __syncthreads();
    }
}

}  // namespace
