// SSIM of two images with its gradient (the `ssim` / `_ssim` of the pytorch_msssim package that training_loop.py:341-376 calls):
// gnerf_ssim_workspace_bytes / _forward / _backward of include/gnerf_hip.h, which states the definition.
//
// Forward, two launches on the caller's stream:
//   tiles   one workgroup per (n, c, 32 x 32 tile of the map).  X and Y with their halo go to LDS as float32 (any strides, fp32 or fp16;
//           a sample outside the image is staged as 0 and only ever meets a map point outside the map), the horizontal pass makes the
//           five windowed sums g*X, g*Y, g*X^2, g*Y^2, g*XY for every staged row, the vertical pass finishes them four map rows per
//           thread, the map is evaluated in registers and summed over the workgroup in a fixed order: per thread, a butterfly over the
//           wave, the four waves in order.  One (ssim, cs) partial per tile goes to the workspace.
//   reduce  one wave per (n, c) adds that item's partials in a fixed order (strided per lane, then a butterfly) and scales by 1 / map size.
// No atomics: a result depends on its own (n, c) image pair and the shape alone -- the same bits run to run and whatever it is batched with.
//
// Backward, one launch: one workgroup per (n, c, 32 x 32 tile of the IMAGE).  It RECOMPUTES the moments of the (32 + k - 1)^2 map points
// whose windows touch the tile (nothing is saved by the forward: three saved maps would be 12.6 MB each at [4,3,512,512], written and
// read back once, against a second stencil pass over data that is in LDS anyway), turns them into the four maps
//   P1 = a1 - 2 mu1 b - mu2 c,  P2 = a2 - 2 mu2 b - mu1 c,  B = b,  C = c
// (a1 = dm/dmu1, a2 = dm/dmu2, b = dm/dsigma1^2 = dm/dsigma2^2, c = dm/dsigma12 of m = g_ssim ssim_map + g_cs cs_map, 0 outside the map),
// runs the transposed window over them (horizontal, vertical -- the full correlation with the flipped window) and writes
//   dX = (gT*P1 + 2 X gT*B + Y gT*C) / map size,   dY = (gT*P2 + 2 Y gT*B + X gT*C) / map size.
// Every output element is written by exactly one thread.
//
// Pitches of the LDS arrays are odd: the passes that walk ROWS per lane (horizontal ones) then touch 32 different banks per half wave, the
// ones that walk columns per lane are contiguous.  Each thread makes kRun adjacent outputs from kRun + k - 1 reads.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;                            // outputs per workgroup and side: map points (forward), pixels (backward)
constexpr int kRun = 4;                              // adjacent outputs per thread in a pass
constexpr int kMaxWin = GNERF_SSIM_MAX_WIN;

struct Window { float w[kMaxWin]; };
struct Strides { int64_t n, c, h, w; };              // in elements

struct Geo {
    int c, h, w, mh, mw;                             // channels, image and map size
    int tiles_y, tiles_x;                            // of the map (forward) or of the image (backward)
    float C1, C2, inv;                               // inv = 1 / (mh * mw)
};

// M = map points per side that a workgroup evaluates
template <int K, int M> struct Dims {
    static constexpr int MR = (M + kRun - 1) / kRun * kRun;          // ... rounded up to whole runs (the surplus is computed and dropped)
    static constexpr int IN = MR + K - 1;                            // staged pixels per side
    static constexpr int IP = IN | 1;                                // pitch of a staged image
    static constexpr int HP = MR | 1;                                // pitch of a horizontally filtered plane (IN rows)
    static constexpr int kStage = IN * IP, kPlane = IN * HP;
};

// Stage IN x IN pixels starting at (r0, c0) -- which may lie outside the image on every side -- as float32.
template <class T, int K, int M>
__device__ __forceinline__ void stage(float* __restrict__ s, const T* __restrict__ img, int64_t base, const Strides& st, int r0, int c0, int h, int w) {
    typedef Dims<K, M> D;
    for (int i = threadIdx.x; i < D::IN * D::IN; i += kThreads) {
        const int r = i / D::IN, c = i - r * D::IN;
        const int gr = r0 + r, gc = c0 + c;
        float v = 0.f;
        if (gr >= 0 && gr < h && gc >= 0 && gc < w) v = gnerf::load_as<T>(img, base + int64_t(gr) * st.h + int64_t(gc) * st.w);
        s[r * D::IP + c] = v;
    }
}

// Horizontal pass of the five moments: planes hb[0..4] = g*X, g*Y, g*X^2, g*Y^2, g*XY over IN rows x MR columns.
template <int K, int M>
__device__ __forceinline__ void moments_rows(const float* __restrict__ sx, const float* __restrict__ sy, float* __restrict__ hb, const Window& win) {
    typedef Dims<K, M> D;
    constexpr int kGroups = D::MR / kRun;
    for (int item = threadIdx.x; item < D::IN * kGroups; item += kThreads) {
        const int g = item / D::IN, r = item - g * D::IN;
        float xv[kRun + K - 1], yv[kRun + K - 1];
#pragma unroll
        for (int t = 0; t < kRun + K - 1; t++) {
            xv[t] = sx[r * D::IP + g * kRun + t];
            yv[t] = sy[r * D::IP + g * kRun + t];
        }
#pragma unroll
        for (int o = 0; o < kRun; o++) {
            float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
            for (int t = 0; t < K; t++) {
                const float wt = win.w[t], x = xv[o + t], y = yv[o + t];
                const float wx = wt * x, wy = wt * y;
                m1 += wx;
                m2 += wy;
                xx = fmaf(wx, x, xx);
                yy = fmaf(wy, y, yy);
                xy = fmaf(wx, y, xy);
            }
            const int at = r * D::HP + g * kRun + o;
            hb[0 * D::kPlane + at] = m1;
            hb[1 * D::kPlane + at] = m2;
            hb[2 * D::kPlane + at] = xx;
            hb[3 * D::kPlane + at] = yy;
            hb[4 * D::kPlane + at] = xy;
        }
    }
}

// Vertical pass for one item (column j, rows rg * kRun ...): out[m][o] = sum_t g[t] hb[m][rg * kRun + o + t][j].
template <int K, int M>
__device__ __forceinline__ void moments_cols(const float* __restrict__ hb, const Window& win, int j, int rg, float (&out)[5][kRun]) {
    typedef Dims<K, M> D;
#pragma unroll
    for (int m = 0; m < 5; m++) {
        float v[kRun + K - 1];
#pragma unroll
        for (int t = 0; t < kRun + K - 1; t++) v[t] = hb[m * D::kPlane + (rg * kRun + t) * D::HP + j];
#pragma unroll
        for (int o = 0; o < kRun; o++) {
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < K; t++) acc = fmaf(win.w[t], v[o + t], acc);
            out[m][o] = acc;
        }
    }
}

struct MapPoint { float lum, cs, ld, cd, mu1, mu2; };            // lum = (2 mu1 mu2 + C1) / ld, cs = (2 s12 + C2) / cd

__device__ __forceinline__ MapPoint evaluate(float mu1, float mu2, float xx, float yy, float xy, float C1, float C2) {
    MapPoint p;
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const float s1 = xx - mu1_sq, s2 = yy - mu2_sq, s12 = xy - mu12;
    p.mu1 = mu1;
    p.mu2 = mu2;
    p.ld = mu1_sq + mu2_sq + C1;
    p.cd = s1 + s2 + C2;
    p.lum = (2.f * mu12 + C1) / p.ld;
    p.cs = (2.f * s12 + C2) / p.cd;
    return p;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <class T, int K>
__global__ __launch_bounds__(kThreads) void ssim_tiles_kernel(const T* __restrict__ x, const T* __restrict__ y, Strides xs, Strides ys, Geo g, Window win,
                                                              float* __restrict__ partials) {
    typedef Dims<K, kTile> D;
    static_assert(D::MR == kTile && kTile * (kTile / kRun) == kThreads, "one vertical item per thread");
    __shared__ float sx[D::kStage], sy[D::kStage], hb[5 * D::kPlane];
    __shared__ float red[kThreads / 64][2];
    const int tiles = g.tiles_y * g.tiles_x;
    const int nc = blockIdx.x / tiles, tile = blockIdx.x - nc * tiles;
    const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    const int n = nc / g.c, c = nc - n * g.c;
    const int r0 = ty * kTile, c0 = tx * kTile;                    // first map point = first pixel of its window
    stage<T, K, kTile>(sx, x, int64_t(n) * xs.n + int64_t(c) * xs.c, xs, r0, c0, g.h, g.w);
    stage<T, K, kTile>(sy, y, int64_t(n) * ys.n + int64_t(c) * ys.c, ys, r0, c0, g.h, g.w);
    __syncthreads();
    moments_rows<K, kTile>(sx, sy, hb, win);
    __syncthreads();
    const int j = threadIdx.x % kTile, rg = threadIdx.x / kTile;
    float mo[5][kRun];
    moments_cols<K, kTile>(hb, win, j, rg, mo);
    float sum_ssim = 0.f, sum_cs = 0.f;
#pragma unroll
    for (int o = 0; o < kRun; o++) {
        const MapPoint p = evaluate(mo[0][o], mo[1][o], mo[2][o], mo[3][o], mo[4][o], g.C1, g.C2);
        const bool in = r0 + rg * kRun + o < g.mh && c0 + j < g.mw;
        sum_ssim += in ? p.lum * p.cs : 0.f;
        sum_cs += in ? p.cs : 0.f;
    }
    sum_ssim = wave_sum(sum_ssim);
    sum_cs = wave_sum(sum_cs);
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = sum_ssim;
        red[threadIdx.x >> 6][1] = sum_cs;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f;
        for (int wv = 0; wv < kThreads / 64; wv++) {
            a += red[wv][0];
            b += red[wv][1];
        }
        partials[2 * size_t(blockIdx.x)] = a;
        partials[2 * size_t(blockIdx.x) + 1] = b;
    }
}

__global__ __launch_bounds__(64) void ssim_reduce_kernel(const float* __restrict__ partials, int tiles, float inv, float* __restrict__ ssim_nc,
                                                         float* __restrict__ cs_nc) {
    const float* p = partials + 2 * size_t(blockIdx.x) * tiles;
    float a = 0.f, b = 0.f;
    for (int i = threadIdx.x; i < tiles; i += 64) {
        a += p[2 * i];
        b += p[2 * i + 1];
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (threadIdx.x == 0) {
        ssim_nc[blockIdx.x] = a * inv;
        cs_nc[blockIdx.x] = b * inv;
    }
}

// ---- backward

template <int K> struct BwdDims {
    static constexpr int M = kTile + K - 1;                         // map points per side whose windows touch the tile
    typedef Dims<K, M> D;
    static constexpr int MP = M | 1;                                 // pitch of a map plane (M rows)
    static constexpr int TP = kTile | 1;                             // pitch of a horizontally back-filtered plane (M rows x kTile columns)
    static constexpr int kMap = M * MP, kBack = M * TP;
    static_assert(4 * kBack <= 5 * D::kPlane, "the back-filtered planes reuse the moments' LDS");
    static constexpr int kFloats = 2 * D::kStage + 5 * D::kPlane + 4 * kMap;
};

template <class T, int K>
__global__ __launch_bounds__(kThreads) void ssim_backward_kernel(const T* __restrict__ x, const T* __restrict__ y, Strides xs, Strides ys, Geo g, Window win,
                                                                 const float* __restrict__ g_ssim, const float* __restrict__ g_cs,
                                                                 T* __restrict__ dx, Strides dxs, T* __restrict__ dy, Strides dys) {
    typedef BwdDims<K> B;
    typedef typename B::D D;
    constexpr int M = B::M;
    extern __shared__ float4 lds4[];
    float* sx = reinterpret_cast<float*>(lds4);
    float* sy = sx + D::kStage;
    float* hb = sy + D::kStage;                                      // five moment planes, later the four back-filtered planes
    float* maps = hb + 5 * D::kPlane;                                // P1, P2, B, C
    const int tiles = g.tiles_y * g.tiles_x;
    const int nc = blockIdx.x / tiles, tile = blockIdx.x - nc * tiles;
    const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    const int n = nc / g.c, c = nc - n * g.c;
    const int q0r = ty * kTile, q0c = tx * kTile;                    // first pixel of the tile
    const int p0r = q0r - (K - 1), p0c = q0c - (K - 1);              // first map point that reaches it = first staged pixel
    const int64_t xbase = int64_t(n) * xs.n + int64_t(c) * xs.c, ybase = int64_t(n) * ys.n + int64_t(c) * ys.c;
    stage<T, K, M>(sx, x, xbase, xs, p0r, p0c, g.h, g.w);
    stage<T, K, M>(sy, y, ybase, ys, p0r, p0c, g.h, g.w);
    __syncthreads();
    moments_rows<K, M>(sx, sy, hb, win);
    __syncthreads();
    const float gs = g_ssim ? g_ssim[nc] : 0.f, gc = g_cs ? g_cs[nc] : 0.f;
    for (int item = threadIdx.x; item < D::MR * (D::MR / kRun); item += kThreads) {
        const int rg = item / D::MR, j = item - rg * D::MR;
        float mo[5][kRun];
        moments_cols<K, M>(hb, win, j, rg, mo);
#pragma unroll
        for (int o = 0; o < kRun; o++) {
            const int u = rg * kRun + o;
            if (u >= M || j >= M) continue;
            const int pr = p0r + u, pc = p0c + j;
            float P1 = 0.f, P2 = 0.f, Bv = 0.f, Cv = 0.f;
            if (pr >= 0 && pr < g.mh && pc >= 0 && pc < g.mw) {
                const MapPoint p = evaluate(mo[0][o], mo[1][o], mo[2][o], mo[3][o], mo[4][o], g.C1, g.C2);
                const float k = gs * p.lum + gc;                     // m = cs * k
                const float la = 2.f * gs * p.cs / p.ld;             // dm/dmu1 = la (mu2 - lum mu1)
                const float a1 = la * (p.mu2 - p.lum * p.mu1), a2 = la * (p.mu1 - p.lum * p.mu2);
                Cv = 2.f * k / p.cd;
                Bv = -k * p.cs / p.cd;
                P1 = a1 - 2.f * p.mu1 * Bv - p.mu2 * Cv;
                P2 = a2 - 2.f * p.mu2 * Bv - p.mu1 * Cv;
            }
            const int at = u * B::MP + j;
            maps[0 * B::kMap + at] = P1;
            maps[1 * B::kMap + at] = P2;
            maps[2 * B::kMap + at] = Bv;
            maps[3 * B::kMap + at] = Cv;
        }
    }
    __syncthreads();
    // the transposed window, horizontally: back[m][u][v] = sum_s g[K - 1 - s] maps[m][u][v + s]   (pixel column q0c + v)
    float* back = hb;
    for (int item = threadIdx.x; item < 4 * M * (kTile / kRun); item += kThreads) {
        const int m = item / (M * (kTile / kRun)), rest = item - m * (M * (kTile / kRun));
        const int grp = rest / M, u = rest - grp * M;
        float v[kRun + K - 1];
#pragma unroll
        for (int t = 0; t < kRun + K - 1; t++) v[t] = maps[m * B::kMap + u * B::MP + grp * kRun + t];
#pragma unroll
        for (int o = 0; o < kRun; o++) {
            float acc = 0.f;
#pragma unroll
            for (int s = 0; s < K; s++) acc = fmaf(win.w[K - 1 - s], v[o + s], acc);
            back[m * B::kBack + u * B::TP + grp * kRun + o] = acc;
        }
    }
    __syncthreads();
    // ... vertically, and the result
    const int b = threadIdx.x % kTile, rg = threadIdx.x / kTile;
    float acc[4][kRun];
#pragma unroll
    for (int m = 0; m < 4; m++) {
        float v[kRun + K - 1];
#pragma unroll
        for (int t = 0; t < kRun + K - 1; t++) v[t] = back[m * B::kBack + (rg * kRun + t) * B::TP + b];
#pragma unroll
        for (int o = 0; o < kRun; o++) {
            float s_ = 0.f;
#pragma unroll
            for (int s = 0; s < K; s++) s_ = fmaf(win.w[K - 1 - s], v[o + s], s_);
            acc[m][o] = s_;
        }
    }
#pragma unroll
    for (int o = 0; o < kRun; o++) {
        const int a = rg * kRun + o;
        const int qr = q0r + a, qc = q0c + b;
        if (qr >= g.h || qc >= g.w) continue;
        const float xv = sx[(a + K - 1) * D::IP + b + K - 1], yv = sy[(a + K - 1) * D::IP + b + K - 1];
        if (dx) gnerf::store_as<T>(dx, int64_t(n) * dxs.n + int64_t(c) * dxs.c + int64_t(qr) * dxs.h + int64_t(qc) * dxs.w,
                            (acc[0][o] + 2.f * xv * acc[2][o] + yv * acc[3][o]) * g.inv);
        if (dy) gnerf::store_as<T>(dy, int64_t(n) * dys.n + int64_t(c) * dys.c + int64_t(qr) * dys.h + int64_t(qc) * dys.w,
                            (acc[1][o] + 2.f * yv * acc[2][o] + xv * acc[3][o]) * g.inv);
    }
}

// ---- host side

int check_shape(const char* what, int dtype, int n, int c, int h, int w, int win) {
    using namespace gnerf;
    if (dtype != GNERF_F32 && dtype != GNERF_F16) return fail(GNERF_E_ARG, "%s: dtype must be GNERF_F32 or GNERF_F16 (got %d)", what, dtype);
    if (n < 1 || c < 1 || h < 1 || w < 1) return fail(GNERF_E_ARG, "%s: empty image [%d, %d, %d, %d]", what, n, c, h, w);
    if (win < 1 || win > kMaxWin || win % 2 == 0) return fail(GNERF_E_ARG, "%s: the window must have an odd length of at most %d (got %d)", what, kMaxWin, win);
    if (h < win || w < win) return fail(GNERF_E_ARG, "%s: a %d x %d image is smaller than the window of %d", what, h, w, win);
    return GNERF_OK;
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

int make_geo(const char* what, int n, int c, int h, int w, int win, bool backward, float C1, float C2, Geo* g, int64_t* blocks) {
    using namespace gnerf;
    g->c = c; g->h = h; g->w = w; g->mh = h - win + 1; g->mw = w - win + 1;
    g->tiles_y = backward ? cdiv(h, kTile) : cdiv(g->mh, kTile);
    g->tiles_x = backward ? cdiv(w, kTile) : cdiv(g->mw, kTile);
    g->C1 = C1; g->C2 = C2;
    g->inv = float(1.0 / (double(g->mh) * double(g->mw)));
    *blocks = int64_t(n) * c * g->tiles_y * g->tiles_x;
    if (*blocks >= (int64_t(1) << 31)) return fail(GNERF_E_ARG, "%s: [%d, %d, %d, %d] needs more than 2^31 workgroups", what, n, c, h, w);
    return GNERF_OK;
}

inline Strides strides_of(const int64_t* s) { return Strides{s[0], s[1], s[2], s[3]}; }

template <class T, int K>
int launch_forward(const void* x, const void* y, const Strides& xs, const Strides& ys, const Geo& g, const Window& win, int64_t blocks, int nc,
                   float* partials, float* ssim_nc, float* cs_nc, hipStream_t stream) {
    using namespace gnerf;
    hipLaunchKernelGGL((ssim_tiles_kernel<T, K>), dim3(unsigned(blocks)), dim3(kThreads), 0, stream, static_cast<const T*>(x), static_cast<const T*>(y),
                       xs, ys, g, win, partials);
    if (int rc = check_launch("ssim_forward")) return rc;
    hipLaunchKernelGGL(ssim_reduce_kernel, dim3(unsigned(nc)), dim3(64), 0, stream, partials, g.tiles_y * g.tiles_x, g.inv, ssim_nc, cs_nc);
    return check_launch("ssim_forward (reduce)");
}

template <class T, int K>
int launch_backward(const void* x, const void* y, const Strides& xs, const Strides& ys, const Geo& g, const Window& win, int64_t blocks,
                    const float* g_ssim, const float* g_cs, void* dx, const Strides& dxs, void* dy, const Strides& dys, hipStream_t stream) {
    using namespace gnerf;
    constexpr int kBytes = BwdDims<K>::kFloats * 4;
    static_assert(kBytes <= 160 * 1024, "the backward tile must fit the LDS");
    static PerDeviceOnce once;
    if (int rc = once.raise_lds(ssim_backward_kernel<T, K>, "ssim_backward", kBytes)) return rc;
    hipLaunchKernelGGL((ssim_backward_kernel<T, K>), dim3(unsigned(blocks)), dim3(kThreads), kBytes, stream, static_cast<const T*>(x), static_cast<const T*>(y),
                       xs, ys, g, win, g_ssim, g_cs, static_cast<T*>(dx), dxs, static_cast<T*>(dy), dys);
    return check_launch("ssim_backward");
}

// Returns CALL(T, K) for the runtime dtype and window length.
#define SSIM_DISPATCH(CALL)                                                                                     \
    switch (win) {                                                                                              \
        case 1: return dtype == GNERF_F16 ? CALL(__half, 1) : CALL(float, 1);                                   \
        case 3: return dtype == GNERF_F16 ? CALL(__half, 3) : CALL(float, 3);                                   \
        case 5: return dtype == GNERF_F16 ? CALL(__half, 5) : CALL(float, 5);                                   \
        case 7: return dtype == GNERF_F16 ? CALL(__half, 7) : CALL(float, 7);                                   \
        case 9: return dtype == GNERF_F16 ? CALL(__half, 9) : CALL(float, 9);                                   \
        default: return dtype == GNERF_F16 ? CALL(__half, 11) : CALL(float, 11);                                \
    }

}  // namespace

extern "C" int gnerf_ssim_workspace_bytes(int n, int c, int h, int w, int win, size_t* bytes) {
    using namespace gnerf;
    if (!bytes) return fail(GNERF_E_ARG, "ssim_workspace_bytes: null pointer");
    if (int rc = check_shape("ssim_workspace_bytes", GNERF_F32, n, c, h, w, win)) return rc;
    Geo g;
    int64_t blocks;
    if (int rc = make_geo("ssim_workspace_bytes", n, c, h, w, win, false, 0.f, 0.f, &g, &blocks)) return rc;
    *bytes = size_t(blocks) * 2 * sizeof(float);
    return GNERF_OK;
}

extern "C" int gnerf_ssim_forward(const void* x, const void* y, int dtype, int n, int c, int h, int w, const int64_t* x_strides,
                                  const int64_t* y_strides, const float* window, int win, float C1, float C2, void* workspace, float* ssim_nc,
                                  float* cs_nc, gnerf_stream_t stream) {
    using namespace gnerf;
    if (!x || !y || !x_strides || !y_strides || !window || !workspace || !ssim_nc || !cs_nc) return fail(GNERF_E_ARG, "ssim_forward: null pointer");
    if (int rc = check_shape("ssim_forward", dtype, n, c, h, w, win)) return rc;
    Geo g;
    int64_t blocks;
    if (int rc = make_geo("ssim_forward", n, c, h, w, win, false, C1, C2, &g, &blocks)) return rc;
    Window wd = {};
    for (int i = 0; i < win; i++) wd.w[i] = window[i];
    const Strides xs = strides_of(x_strides), ys = strides_of(y_strides);
#define SSIM_FWD(T, K) launch_forward<T, K>(x, y, xs, ys, g, wd, blocks, n * c, static_cast<float*>(workspace), ssim_nc, cs_nc, as_stream(stream))
    SSIM_DISPATCH(SSIM_FWD)
#undef SSIM_FWD
}

extern "C" int gnerf_ssim_backward(const void* x, const void* y, int dtype, int n, int c, int h, int w, const int64_t* x_strides,
                                   const int64_t* y_strides, const float* window, int win, float C1, float C2, const float* g_ssim,
                                   const float* g_cs, void* dx, const int64_t* dx_strides, void* dy, const int64_t* dy_strides,
                                   gnerf_stream_t stream) {
    using namespace gnerf;
    if (!x || !y || !x_strides || !y_strides || !window) return fail(GNERF_E_ARG, "ssim_backward: null pointer");
    if (!g_ssim && !g_cs) return fail(GNERF_E_ARG, "ssim_backward: g_ssim and g_cs are both null");
    if (!dx && !dy) return fail(GNERF_E_ARG, "ssim_backward: dx and dy are both null");
    if ((dx && !dx_strides) || (dy && !dy_strides)) return fail(GNERF_E_ARG, "ssim_backward: an output without its strides");
    if (int rc = check_shape("ssim_backward", dtype, n, c, h, w, win)) return rc;
    Geo g;
    int64_t blocks;
    if (int rc = make_geo("ssim_backward", n, c, h, w, win, true, C1, C2, &g, &blocks)) return rc;
    Window wd = {};
    for (int i = 0; i < win; i++) wd.w[i] = window[i];
    const Strides xs = strides_of(x_strides), ys = strides_of(y_strides);
    const Strides dxs = dx ? strides_of(dx_strides) : Strides{0, 0, 0, 0}, dys = dy ? strides_of(dy_strides) : Strides{0, 0, 0, 0};
#define SSIM_BWD(T, K) launch_backward<T, K>(x, y, xs, ys, g, wd, blocks, g_ssim, g_cs, dx, dxs, dy, dys, as_stream(stream))
    SSIM_DISPATCH(SSIM_BWD)
#undef SSIM_BWD
}
