// Antialiased separable resize, forward and transposed (F.interpolate(mode='bilinear' | 'bicubic', align_corners=False, antialias=True) and
// its gradient): gnerf_resize_aa_forward / _backward of include/gnerf_hip.h, which states the definition.
//
// The operator is y = W_y x W_x^T per (n, c) with banded W (row i of an axis' W: `xsize` normalised filter taps from `xmin` on).  Both exports
// run ONE kernel, which applies a banded operator along x and then along y; what differs is how a workgroup fills its band tables:
//   forward     output i reads source xmin_i ... with the weights of row i;
//   transposed  output k (a pixel of the resize's INPUT) reads the contiguous run of rows i whose band holds k (xmin_i and xmin_i + xsize_i
//               are both monotone in i) with the weights W[i][k] -- a gather: every element of dx is written by one thread, which sums in a
//               fixed order.  No atomics, the same bits on every run and whatever the item is batched with.
// One workgroup owns th x tw outputs of tc channel vectors:
//   tables   lo / cnt / w[.][kMaxTaps] per tile row and column, in LDS.  Band edges, tap offsets, the filter and the row sums are evaluated in
//            float64 and each weight is rounded to float32 ONCE: a centre scale * (i + 0.5) held in float32 is off by 2^-24 * centre, which at
//            pixel 500 is 3e-5 of a tap -- far more than the products and sums below lose.  It is a few dozen flops per row and column.
//   pass 1   horizontal: for every source row of the tile's footprint and every tile column, the taps are read from global memory and summed
//            in float32 (fmaf, ascending taps) into an LDS plane;
//   pass 2   vertical: the same over the plane's rows; the result is rounded once, at the store.
// Lanes run along x (tc = 1, any strides), or -- when both tensors have a unit channel stride -- along c, one 16-byte vector of channels per
// lane where sizes, strides and pointers allow it (VEC = 4 float / 8 half), else one channel per lane.  The lane mapping changes which thread
// makes an element, never the arithmetic that makes it: NCHW and channels_last give the same bits.
// The tile shape is chosen by the host from the sizes alone (no table, no cache, no synchronisation: a first call inside a graph capture is
// like any other); LDS is static.
#include "common.h"

#include <climits>
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTile = 32;                         // outputs per workgroup and axis, at most
constexpr int kMaxTaps = GNERF_RESIZE_MAX_TAPS;      // taps per output and axis; odd, so also the conflict-free pitch of a weight row
constexpr int kPlaneFloats = 8192;                   // the horizontally filtered plane: footprint rows x tile columns x channels

struct Strides { int64_t n, c, h, w; };              // in elements

struct Axis {
    double scale, support, invscale;                 // of the RESIZE along this axis (in -> out)
    int in, out;                                     // ... and its sizes
    int n_dst, n_src;                                // what THIS call writes and reads along the axis: (out, in) forward, (in, out) transposed
    int tile, tile_shift, tiles;                     // outputs per workgroup (a power of two), tiles along the axis
    int cap;                                         // upper bound of the source indices one tile touches
    int taps;                                        // ... and of the taps of one output (one more than the bound in real arithmetic)
};

struct Geo {
    Axis y, x;
    int c, tc, tc_shift, ctiles;                     // channels; channel vectors per workgroup (a power of two) and tiles of them
    int mode, transposed;
};

__device__ __forceinline__ double filter_at(int mode, double x) {
    x = fabs(x);
    if (mode == GNERF_RESIZE_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
    if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;                          // Keys' cubic, a = -0.5
    if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
    return 0.0;
}

struct Band { int lo, n; double center; };

// Row i of the axis' matrix: taps lo ... lo + n - 1.  (No contraction: forward and transposed tables must see the same edges.)
__device__ __forceinline__ Band band_of(const Axis& a, int i) {
#pragma clang fp contract(off)
    Band b;
    b.center = a.scale * (double(i) + 0.5);
    const int lo = max(int(b.center - a.support + 0.5), 0);
    const int hi = min(int(b.center + a.support + 0.5), a.in);
    b.lo = lo;
    b.n = max(hi - lo, 0);
    return b;
}

__device__ __forceinline__ double tap_at(const Axis& a, int mode, const Band& b, int src) {
#pragma clang fp contract(off)
    return filter_at(mode, (double(src) - b.center + 0.5) * a.invscale);
}

// 1 / (the sum of the band's taps), or 1 where that is 0: the normalisation as a factor
__device__ __forceinline__ double band_norm(const Axis& a, int mode, const Band& b) {
    double s = 0.0;
    for (int j = 0; j < b.n; j++) s += tap_at(a, mode, b, b.lo + j);
    return s != 0.0 ? 1.0 / s : 1.0;
}

__device__ __forceinline__ float band_weight(const Axis& a, int mode, const Band& b, double norm, int src) {
#pragma clang fp contract(off)
    return float(tap_at(a, mode, b, src) * norm);
}

// lo / cnt of tile entry t (output o0 + t); forward also leaves the row's normalisation
__device__ __forceinline__ void table_range(const Axis& a, int mode, bool transposed, int o, int* lo, int* cnt, double* norm) {
    *lo = 0;
    *cnt = 0;
    *norm = 1.0;
    if (o >= a.n_dst) return;
    if (!transposed) {
        const Band b = band_of(a, o);
        *lo = b.lo;
        *cnt = min(b.n, a.taps);
        *norm = band_norm(a, mode, b);
        return;
    }
    // the rows whose band holds pixel o: centres in [o + 0.5 - support, o + 0.5 + support); an estimate, then exact steps
    const int k = o;
    int i = min(max(int(ceil((k + 0.5 - a.support) / a.scale - 0.5)), 0), a.out - 1);
    for (int it = 0; it < 8 && i > 0; it++) {                       // first row that ends past k
        const Band b = band_of(a, i - 1);
        if (b.lo + b.n > k) i--; else break;
    }
    for (int it = 0; it < 8 && i < a.out; it++) {
        const Band b = band_of(a, i);
        if (b.lo + b.n <= k) i++; else break;
    }
    const int first = i;
    i = min(max(int(floor((k + 0.5 + a.support) / a.scale - 0.5)), 0), a.out - 1);
    for (int it = 0; it < 8 && i < a.out - 1; it++) {               // last row that starts at or before k
        if (band_of(a, i + 1).lo <= k) i++; else break;
    }
    for (int it = 0; it < 8 && i >= 0; it++) {
        if (band_of(a, i).lo > k) i--; else break;
    }
    *lo = first;
    *cnt = min(max(i - first + 1, 0), a.taps);
}

__device__ __forceinline__ float table_weight(const Axis& a, int mode, bool transposed, int o, int lo, int m, double norm) {
    if (!transposed) return band_weight(a, mode, band_of(a, o), norm, lo + m);
    const Band b = band_of(a, lo + m);
    if (o < b.lo || o >= b.lo + b.n) return 0.f;
    return band_weight(a, mode, b, band_norm(a, mode, b), o);
}

template <class T, int VEC>
__device__ __forceinline__ void load_vec(const T* __restrict__ p, float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = gnerf::load_as<T>(p, 0);
    } else {
        const gnerf::Pk<T, VEC> pk = *reinterpret_cast<const gnerf::Pk<T, VEC>*>(p);
#pragma unroll
        for (int k = 0; k < VEC; k++) v[k] = gnerf::load_as<T>(pk.v, k);
    }
}

template <class T, int VEC>
__device__ __forceinline__ void store_vec(T* __restrict__ p, const float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        gnerf::store_as<T>(p, 0, v[0]);
    } else {
        gnerf::Pk<T, VEC> pk;
#pragma unroll
        for (int k = 0; k < VEC; k++) gnerf::store_as<T>(pk.v, k, v[k]);
        *reinterpret_cast<gnerf::Pk<T, VEC>*>(p) = pk;
    }
}

template <class T, int VEC>
__global__ __launch_bounds__(kThreads) void resize_aa_kernel(const T* __restrict__ src, T* __restrict__ dst, Strides ss, Strides ds, Geo g) {
    __shared__ float plane[kPlaneFloats];
    __shared__ float wy[kMaxTile * kMaxTaps], wx[kMaxTile * kMaxTaps];
    __shared__ double norms[2 * kMaxTile];
    __shared__ int lo[2 * kMaxTile], cnt[2 * kMaxTile];              // y entries, then x entries
    int b = blockIdx.x;
    const int tx = b % g.x.tiles; b /= g.x.tiles;
    const int ty = b % g.y.tiles; b /= g.y.tiles;
    const int ct = b % g.ctiles, n = b / g.ctiles;
    const int th = g.y.tile, tw = g.x.tile, tc = g.tc;
    const int oy0 = ty * th, ox0 = tx * tw;
    const bool transposed = g.transposed != 0;

    if (threadIdx.x < 2 * kMaxTile) {
        const bool is_x = threadIdx.x >= kMaxTile;
        const int t = threadIdx.x & (kMaxTile - 1);
        const Axis& a = is_x ? g.x : g.y;
        table_range(a, g.mode, transposed, t < a.tile ? (is_x ? ox0 : oy0) + t : INT_MAX, &lo[threadIdx.x], &cnt[threadIdx.x], &norms[threadIdx.x]);
    }
    __syncthreads();
    // the weights: entry (t, m) for m < taps (no entry past cnt[t] is ever read)
    const int ny = th * g.y.taps, nx = tw * g.x.taps;
    for (int idx = threadIdx.x; idx < ny + nx; idx += kThreads) {
        const bool is_x = idx >= ny;
        const Axis& a = is_x ? g.x : g.y;
        const int rest = is_x ? idx - ny : idx;
        const int t = rest / a.taps, m = rest - t * a.taps, e = is_x ? kMaxTile + t : t;
        if (m < cnt[e]) (is_x ? wx : wy)[t * kMaxTaps + m] = table_weight(a, g.mode, transposed, (is_x ? ox0 : oy0) + t, lo[e], m, norms[e]);
    }
    __syncthreads();

    // the source rows this tile touches: r0 ... r0 + fr - 1 (lo and lo + cnt are monotone along the tile)
    const int last = min(th, g.y.n_dst - oy0) - 1;
    const int r0 = lo[0], r1 = lo[last] + cnt[last];
    const int fr = r1 > r0 ? min(r1 - r0, g.y.cap) : 0;
    const int tws = g.x.tile_shift, tcs = g.tc_shift;
    const int64_t sbase = int64_t(n) * ss.n, dbase = int64_t(n) * ds.n;

    // pass 1, horizontal: plane[(r * tw + j) * tc + cg] (VEC floats each) = sum_t wx[j][t] src[r0 + r][lo_x[j] + t]
    for (int item = threadIdx.x; item < fr * tw * tc; item += kThreads) {
        const int cg = item & (tc - 1), j = (item >> tcs) & (tw - 1), r = item >> (tcs + tws);
        const int c = (ct * tc + cg) * VEC;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; k++) acc[k] = 0.f;
        const int nt = cnt[kMaxTile + j];
        if (c < g.c && nt > 0) {
            const T* p = src + sbase + int64_t(c) * ss.c + int64_t(r0 + r) * ss.h + int64_t(lo[kMaxTile + j]) * ss.w;
            const float* w = wx + j * kMaxTaps;
            for (int t = 0; t < nt; t++) {
                float v[VEC];
                load_vec<T, VEC>(p + int64_t(t) * ss.w, v);
#pragma unroll
                for (int k = 0; k < VEC; k++) acc[k] = fmaf(w[t], v[k], acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; k++) plane[item * VEC + k] = acc[k];
    }
    __syncthreads();

    // pass 2, vertical
    for (int item = threadIdx.x; item < th * tw * tc; item += kThreads) {
        const int cg = item & (tc - 1), j = (item >> tcs) & (tw - 1), i = item >> (tcs + tws);
        const int c = (ct * tc + cg) * VEC, oy = oy0 + i, ox = ox0 + j;
        if (c >= g.c || oy >= g.y.n_dst || ox >= g.x.n_dst) continue;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; k++) acc[k] = 0.f;
        const int nt = cnt[i], rb = lo[i] - r0;
        const float* w = wy + i * kMaxTaps;
        for (int t = 0; t < nt; t++) {
            const int rr = rb + t;
            if (unsigned(rr) >= unsigned(fr)) continue;
            const float* q = plane + ((rr * tw + j) * tc + cg) * VEC;
#pragma unroll
            for (int k = 0; k < VEC; k++) acc[k] = fmaf(w[t], q[k], acc[k]);
        }
        store_vec<T, VEC>(dst + dbase + int64_t(c) * ds.c + int64_t(oy) * ds.h + int64_t(ox) * ds.w, acc);
    }
}

// ---- host side

inline int pow2_ceil(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

inline int shift_of(int pow2) {
    int s = 0;
    while ((1 << s) < pow2) s++;
    return s;
}

// source indices that `tile` adjacent outputs can touch, at most (see the header of the file for the two directions)
int footprint_cap(const Axis& a, bool transposed, int tile) {
    const double span = transposed ? (tile + 1 + 2.0 * a.support) / a.scale : (tile - 1) * a.scale + 2.0 * a.support;
    const double cap = std::floor(span) + 3.0;
    return int(std::fmin(cap, double(a.n_src)));
}

int make_axis(const char* what, const char* name, int in, int out, double scale, int mode, bool transposed, Axis* a) {
    using namespace gnerf;
    a->in = in;
    a->out = out;
    a->scale = scale > 0.0 ? scale : double(in) / double(out);
    const double half = mode == GNERF_RESIZE_BICUBIC ? 2.0 : 1.0;
    a->support = a->scale >= 1.0 ? half * a->scale : half;
    a->invscale = a->scale >= 1.0 ? 1.0 / a->scale : 1.0;
    a->n_dst = transposed ? in : out;
    a->n_src = transposed ? out : in;
    // a band is also never longer than the axis it reads
    if (!std::isfinite(a->scale) || std::fmin(std::floor(2.0 * a->support) + 1.0, double(in)) > kMaxTaps)
        return fail(GNERF_E_UNSUPPORTED, "%s: %s %d -> %d (scale %g) needs more than %d taps per output", what, name, in, out, a->scale, kMaxTaps);
    if (std::fmin(std::floor(2.0 * a->support / a->scale) + 1.0, double(out)) > kMaxTaps)
        return fail(GNERF_E_UNSUPPORTED, "%s: %s %d -> %d (scale %g): more than %d outputs touch one input", what, name, in, out, a->scale, kMaxTaps);
    const double taps = transposed ? std::fmin(std::floor(2.0 * a->support / a->scale) + 1.0, double(out)) : std::fmin(std::floor(2.0 * a->support) + 1.0, double(in));
    a->taps = int(std::fmin(taps + 1.0, double(kMaxTaps)));
    return GNERF_OK;
}

void set_tile(Axis* a, bool transposed, int tile) {
    a->tile = tile;
    a->tile_shift = shift_of(tile);
    a->tiles = (a->n_dst + tile - 1) / tile;
    a->cap = footprint_cap(*a, transposed, tile);
}

template <class T, int VEC>
int launch(const void* src, void* dst, const Strides& ss, const Strides& ds, const Geo& g, int64_t blocks, hipStream_t stream, const char* what) {
    hipLaunchKernelGGL((resize_aa_kernel<T, VEC>), dim3(unsigned(blocks)), dim3(kThreads), 0, stream, static_cast<const T*>(src), static_cast<T*>(dst), ss, ds, g);
    return gnerf::check_launch(what);
}

inline bool multiple_of(const Strides& s, int v) { return s.n % v == 0 && s.h % v == 0 && s.w % v == 0; }

// src [n, c, (in or out)] -> dst [n, c, (out or in)]
int resize_aa(const char* what, const void* src, void* dst, int dtype, int n, int c, int in_h, int in_w, int out_h, int out_w, const int64_t* src_strides,
              const int64_t* dst_strides, int mode, double scale_h, double scale_w, bool transposed, hipStream_t stream) {
    using namespace gnerf;
    if (!src || !dst || !src_strides || !dst_strides) return fail(GNERF_E_ARG, "%s: null pointer", what);
    if (dtype != GNERF_F32 && dtype != GNERF_F16) return fail(GNERF_E_ARG, "%s: dtype must be GNERF_F32 or GNERF_F16 (got %d)", what, dtype);
    if (mode != GNERF_RESIZE_BILINEAR && mode != GNERF_RESIZE_BICUBIC) return fail(GNERF_E_ARG, "%s: mode must be GNERF_RESIZE_BILINEAR or GNERF_RESIZE_BICUBIC (got %d)", what, mode);
    if (n < 1 || c < 1 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1)
        return fail(GNERF_E_ARG, "%s: empty image [%d, %d, %d, %d] -> [%d, %d]", what, n, c, in_h, in_w, out_h, out_w);
    const int64_t limit = int64_t(1) << 31;
    if (int64_t(n) * c * in_h * in_w >= limit || int64_t(n) * c * out_h * out_w >= limit)
        return fail(GNERF_E_UNSUPPORTED, "%s: [%d, %d, %d, %d] -> [%d, %d] has 2^31 elements or more", what, n, c, in_h, in_w, out_h, out_w);
    Geo g = {};
    g.mode = mode;
    g.transposed = transposed ? 1 : 0;
    g.c = c;
    if (int rc = make_axis(what, "height", in_h, out_h, scale_h, mode, transposed, &g.y)) return rc;
    if (int rc = make_axis(what, "width", in_w, out_w, scale_w, mode, transposed, &g.x)) return rc;
    const Strides ss = {src_strides[0], src_strides[1], src_strides[2], src_strides[3]}, ds = {dst_strides[0], dst_strides[1], dst_strides[2], dst_strides[3]};
    // lanes along c when both tensors have the channels adjacent, in 16-byte vectors where everything is a multiple of one
    const bool along_c = c > 1 && ss.c == 1 && ds.c == 1;
    const int full = dtype == GNERF_F16 ? 8 : 4;
    const bool vec = along_c && c % full == 0 && multiple_of(ss, full) && multiple_of(ds, full) && reinterpret_cast<uintptr_t>(src) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(dst) % 16 == 0;
    const int per_lane = vec ? full : 1;
    const int cvecs = along_c ? c / per_lane : 1;
    int tc = along_c ? std::min(pow2_ceil(cvecs), kMaxTile) : 1;
    int tw = std::min(pow2_ceil(g.x.n_dst), along_c ? kMaxTile / 2 : kMaxTile);
    int th = std::min(std::min(pow2_ceil(g.y.n_dst), kMaxTile), std::max(1, 1024 / (tw * tc)));
    for (;;) {
        set_tile(&g.y, transposed, th);
        if (int64_t(g.y.cap) * tw * tc * per_lane <= kPlaneFloats) break;
        if (th > 1) th >>= 1;
        else if (tw > 1) tw >>= 1;
        else if (tc > 1) tc >>= 1;
        else return fail(GNERF_E_UNSUPPORTED, "%s: no tile of [%d, %d] -> [%d, %d] fits the LDS", what, in_h, in_w, out_h, out_w);
    }
    // enough workgroups for the machine while a tile's horizontal pass still gives every thread two items
    const int64_t images = int64_t(n) * (along_c ? (cvecs + tc - 1) / tc : c);
    while (images * g.y.tiles * ((g.x.n_dst + tw - 1) / tw) < 2 * kNumCU && int64_t(g.y.cap) * tw * tc > 2 * kThreads && (th > 1 || tw > 1)) {
        if (th >= tw) th >>= 1;
        else tw >>= 1;
        set_tile(&g.y, transposed, th);
    }
    set_tile(&g.x, transposed, tw);
    g.tc = tc;
    g.tc_shift = shift_of(tc);
    g.ctiles = along_c ? (cvecs + tc - 1) / tc : c;
    const int64_t blocks = int64_t(n) * g.ctiles * g.y.tiles * g.x.tiles;
    if (blocks >= limit) return fail(GNERF_E_UNSUPPORTED, "%s: [%d, %d, %d, %d] -> [%d, %d] needs 2^31 workgroups or more", what, n, c, in_h, in_w, out_h, out_w);
    if (dtype == GNERF_F16) return vec ? launch<__half, 8>(src, dst, ss, ds, g, blocks, stream, what) : launch<__half, 1>(src, dst, ss, ds, g, blocks, stream, what);
    return vec ? launch<float, 4>(src, dst, ss, ds, g, blocks, stream, what) : launch<float, 1>(src, dst, ss, ds, g, blocks, stream, what);
}

}  // namespace

extern "C" int gnerf_resize_aa_forward(const void* x, void* y, int dtype, int n, int c, int in_h, int in_w, int out_h, int out_w, const int64_t* x_strides,
                                       const int64_t* y_strides, int mode, double scale_h, double scale_w, gnerf_stream_t stream) {
    return resize_aa("resize_aa_forward", x, y, dtype, n, c, in_h, in_w, out_h, out_w, x_strides, y_strides, mode, scale_h, scale_w, false, gnerf::as_stream(stream));
}

extern "C" int gnerf_resize_aa_backward(const void* dy, void* dx, int dtype, int n, int c, int in_h, int in_w, int out_h, int out_w, const int64_t* dy_strides,
                                        const int64_t* dx_strides, int mode, double scale_h, double scale_w, gnerf_stream_t stream) {
    return resize_aa("resize_aa_backward", dy, dx, dtype, n, c, in_h, in_w, out_h, out_w, dy_strides, dx_strides, mode, scale_h, scale_w, true, gnerf::as_stream(stream));
}
