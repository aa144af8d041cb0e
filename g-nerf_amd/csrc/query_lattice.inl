// gnerf_query_lattice (csrc/query_lattice.hip includes this behind render_core.inl and query_fill.inl): csrc/render_query.hip's densities-only
// query_kernel with another point source and sink.
// The points are lattice points of gen_videos.py's create_samples(N = n, cube_length), named by their linear index; a wave forms its 16
// positions itself and stores sigma at out[index] of the dense n^3 array -- no position tensor, no compact output, no scatter pass.
//
// The positions are voxel_samples' (gen_videos_mi355x.py) as PyTorch computes them on the device, operation by operation in fp32:
//   f = float(idx)                      (rounds above 2^24)
//   s2 = float(idx % n)                 (integers)
//   q1 = f * inv_n, s1 = fmod(q1, n)    (`f / n` with a Python scalar is a multiplication by the fp32 reciprocal 1.0f / n there, not a
//   q0 = q1 * inv_n, s0 = fmod(q0, n)    division: the two agree for a power of two only; fmod is exact)
//   p = s * size + origin               (two roundings: no contraction)
// so out[idx] carries the bits of query_sigma(voxel_samples(idx, idx + 1, ...)).  A point's column of the 16x16x4 MFMAs does not depend
// on its neighbours: only this arithmetic could differ.

namespace {

struct LatticeArgs {
    const int32_t* index;        // [m] linear lattice indices, duplicates allowed
    float* out;                  // [n^3]
    int m, n, n_tiles;
    uint32_t n3;
    float nf, inv_n, size, origin;
};

__device__ __forceinline__ void lattice_position(const LatticeArgs& L, int32_t idx, float& x, float& y, float& z) {
#pragma clang fp contract(off)
    const float f = float(idx);
    const float s2 = float(idx % L.n);
    const float q1 = f * L.inv_n;
    const float s1 = fmodf(q1, L.nf);
    const float q0 = q1 * L.inv_n;
    const float s0 = fmodf(q0, L.nf);
    x = s0 * L.size + L.origin;
    y = s1 * L.size + L.origin;
    z = s2 * L.size + L.origin;
}

__global__ __launch_bounds__(64) void query_lattice_kernel(gnerf_render_params p, float box_scale, LatticeArgs L) {
    __shared__ __align__(16) float stage[16 * kStagePitch];
    const int lane = threadIdx.x;
    const int H = p.plane_h, W = p.plane_w;
    const int64_t plane_stride = p.planes_interleaved ? 32 : int64_t(H) * W * 32;
    const unsigned tex_q = p.planes_interleaved ? 24 : 8, row_q = tex_q * unsigned(W);
    const int b = lane >> 3, cq = lane & 7, j = lane & 15, g = lane >> 4;
    Weights w;
    load_weights(w, p, lane);
    const float* planes_item = p.planes_nhwc;
    for (int t = blockIdx.x; t < L.n_tiles; t += gridDim.x) {
#pragma unroll
        for (int a = 0; a < 2; a++) {
            const int js = 8 * a + b;
            const int32_t idx = L.index[min(16 * t + js, L.m - 1)];
            float x, y, z;
            lattice_position(L, idx, x, y, z);
            const float px = x * box_scale, py = y * box_scale, pz = z * box_scale;
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
        if (g == 0 && pt < L.m) {
            const uint32_t at = uint32_t(L.index[pt]);
            if (at < L.n3) L.out[at] = sig;          // an index outside the lattice writes nothing
        }
    }
}

}  // namespace

extern "C" int gnerf_query_lattice(const float* planes_nhwc, int plane_h, int plane_w, const int32_t* index, int m, int n, double cube_length,
                                   float box_warp, const float* w1, const float* b1, const float* w2, const float* b2, float* out,
                                   int planes_interleaved, gnerf_stream_t stream) {
    using namespace gnerf;
    Params P; int tiles_per_item; int64_t tiles;
    if (int e = fill_query("query_lattice", planes_nhwc, 1, plane_h, plane_w, m, box_warp, w1, b1, w2, b2, planes_interleaved, P, tiles_per_item, tiles)) return e;
    if (!index || !out) return fail(GNERF_E_ARG, "query_lattice: null pointer");
    if (m < 1) return fail(GNERF_E_ARG, "query_lattice: m must be positive");
    if (n < 2 || int64_t(n) * n * n >= (int64_t(1) << 31)) return fail(GNERF_E_ARG, "query_lattice: n must be >= 2 with n^3 < 2^31 (got %d)", n);
    if (!(cube_length > 0.0) || !std::isfinite(cube_length)) return fail(GNERF_E_ARG, "query_lattice: cube_length must be finite and > 0");
    LatticeArgs L;
    L.index = index; L.out = out; L.m = m; L.n = n; L.n_tiles = int(tiles);
    L.n3 = uint32_t(n) * uint32_t(n) * uint32_t(n);
    L.nf = float(n);
    L.inv_n = 1.0f / float(n);
    L.size = float(cube_length / double(n - 1));
    L.origin = float(-cube_length / 2.0);
    const int blocks = int(tiles < int64_t(kNumCU) * 16 ? tiles : int64_t(kNumCU) * 16);
    hipLaunchKernelGGL(query_lattice_kernel, dim3(blocks), dim3(64), 0, as_stream(stream), P.p, P.box_scale, L);
    return check_launch("query_lattice_kernel");
}
