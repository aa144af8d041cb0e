// Marching cubes on a dense float32 volume (the mesh step of G-NeRF's shape_utils.py:40-100, skimage.measure.marching_cubes there):
// gnerf_marching_cubes_workspace_bytes / _count / _emit of include/gnerf_hip.h.  The rules (inside = v > level, one vertex per crossed
// lattice edge in (point, axis) order, faces in cell order, outward winding, the case table of mesh_tables.h) are shape_mi355x.py's; its
// numpy port is the reference these kernels match bit for bit.
//
// Three launches on the caller's stream:
//   count  one pass over the volume.  A block owns kPoints consecutive points (linear order, axis 2 fastest), 256 at a time so every load
//          is a coalesced row segment.  Per point: its crossed edges (0..3, one bit per axis) and its cell's triangle count (0..5); a wave
//          prefix from one ballot per bit (mbcnt) plus a block prefix over the four waves in LDS gives each point its first vertex inside
//          the block, stored as base[p] = (prefix << 3) | crossed-axis mask -- the workspace's 4 bytes per point.  Per block: vertex,
//          triangle and non-finite counts.
//   scan   one workgroup turns the per-block counts into 64-bit block offsets and writes the totals (vertices, triangles, non-finite).
//   emit   the volume again: each point writes its own vertices at block offset + base, each cell its triangles at block offset + the same
//          wave/block prefix of triangle counts; a triangle's vertex ids come from its owners' base words (+ the rank of the edge's axis
//          among the owner's crossed axes).
// Between count and emit the caller reads the totals (the op's one host synchronisation) and sizes the outputs.
#include "common.h"
#include "mesh_tables.h"

#pragma clang fp contract(off)

namespace {

#include "mesh_cubes.h"

constexpr int kThreads = 256;
constexpr int kChunks = 8;
constexpr int kPoints = kThreads * kChunks;          // points per block
constexpr int kPointsLog2 = 11;
static_assert(kPoints == 1 << kPointsLog2, "kPoints must be a power of two");

struct Geo {
    uint32_t d0, d1, d2, plane, n;                   // plane = d1 * d2, n = d0 * d1 * d2 < 2^31
};

struct Workspace {
    uint32_t* base;                                  // [n]   (first vertex inside the block << 3) | crossed-axis mask
    uint32_t* blk_v;                                 // [nb]  per-block vertex / triangle / non-finite counts
    uint32_t* blk_t;
    uint32_t* blk_bad;
    int64_t* voff;                                   // [nb]  exclusive block offsets
    int64_t* toff;
};

inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

inline Workspace carve(void* ws, uint32_t n, uint32_t nb, size_t* total) {
    char* p = static_cast<char*>(ws);
    Workspace w;
    size_t off = 0;
    w.base = reinterpret_cast<uint32_t*>(p + off); off += align256(size_t(n) * 4);
    w.blk_v = reinterpret_cast<uint32_t*>(p + off); off += align256(size_t(nb) * 4);
    w.blk_t = reinterpret_cast<uint32_t*>(p + off); off += align256(size_t(nb) * 4);
    w.blk_bad = reinterpret_cast<uint32_t*>(p + off); off += align256(size_t(nb) * 4);
    w.voff = reinterpret_cast<int64_t*>(p + off); off += align256(size_t(nb) * 8);
    w.toff = reinterpret_cast<int64_t*>(p + off); off += align256(size_t(nb) * 8);
    if (total) *total = off;
    return w;
}

// One lattice point (mesh_cubes.h) from the dense volume: its cell's corners are loaded here.
__device__ __forceinline__ Point classify(const float* __restrict__ vol, const Geo& g, float level, uint32_t idx) {
    const uint32_t r = idx / g.d2, i2 = idx - r * g.d2;
    const uint32_t i0 = r / g.d1, i1 = r - i0 * g.d1;
    const bool h0 = i0 + 1 < g.d0, h1 = i1 + 1 < g.d1, h2 = i2 + 1 < g.d2;
    // corner c = (c>>2, c>>1 & 1, c & 1) of the cell; a corner outside the volume reads the point itself (and is never used)
    float cv[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const bool ok = (!(c & 4) || h0) && (!(c & 2) || h1) && (!(c & 1) || h2);
        const uint32_t off = ((c & 4) ? g.plane : 0u) + ((c & 2) ? g.d2 : 0u) + ((c & 1) ? 1u : 0u);
        cv[c] = vol[ok ? idx + off : idx];
    }
    return classify_corners(cv, level, h0, h1, h2);
}

// Block-exclusive prefix of x over this chunk of kThreads points, carried across chunks in *running (uniform).  wsum: LDS for the four
// wave totals, double-buffered by chunk parity so that one barrier per chunk suffices.
template <int BITS>
__device__ __forceinline__ uint32_t block_prefix(uint32_t x, uint32_t (*wsum)[kThreads / 64], int parity, uint32_t* running) {
    const int wave = threadIdx.x >> 6;
    uint32_t wtot;
    const uint32_t pre = wave_prefix<BITS>(x, &wtot);
    if ((threadIdx.x & 63) == 0) wsum[parity][wave] = wtot;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) {
        const uint32_t s = wsum[parity][w];
        before += w < wave ? s : 0u;
        all += s;
    }
    const uint32_t r = *running + before + pre;
    *running += all;
    return r;
}

__global__ __launch_bounds__(kThreads) void mc_count_kernel(const float* __restrict__ vol, Geo g, float level, Workspace ws) {
    __shared__ uint32_t wv[2][kThreads / 64], wt[2][kThreads / 64], wb[kThreads / 64];
    uint32_t run_v = 0, run_t = 0, bad = 0;
    const uint32_t first = blockIdx.x * uint32_t(kPoints);
    for (int j = 0; j < kChunks; j++) {
        const uint32_t idx = first + uint32_t(j * kThreads) + threadIdx.x;
        Point pt = {};
        if (idx < g.n) pt = classify(vol, g, level, idx);
        const uint32_t nv = __popc(pt.mask);
        const uint32_t pv = block_prefix<2>(nv, wv, j & 1, &run_v);
        (void)block_prefix<3>(pt.ntri, wt, j & 1, &run_t);
        bad += uint32_t(__popcll(__ballot(pt.bad)));
        if (idx < g.n) ws.base[idx] = (pv << 3) | pt.mask;
    }
    if ((threadIdx.x & 63) == 0) wb[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t b = 0;
        for (int w = 0; w < kThreads / 64; w++) b += wb[w];
        ws.blk_v[blockIdx.x] = run_v;
        ws.blk_t[blockIdx.x] = run_t;
        ws.blk_bad[blockIdx.x] = b;
    }
}

// One workgroup: exclusive 64-bit offsets of the per-block counts; totals -> counts[0..2] (mesh_cubes.h).
__global__ __launch_bounds__(kMcScanThreads) void mc_scan_kernel(Workspace ws, uint32_t nb, int64_t* __restrict__ counts) {
    scan_block_counts(ws.blk_v, ws.blk_t, ws.blk_bad, ws.voff, ws.toff, nb, counts);
}

__device__ __forceinline__ int32_t vertex_id(const Workspace& ws, uint32_t q, uint32_t axis) {
    const uint32_t w = ws.base[q];
    return int32_t(ws.voff[q >> kPointsLog2] + int64_t(w >> 3) + int64_t(__popc(w & ((1u << axis) - 1u))));
}

__global__ __launch_bounds__(kThreads) void mc_emit_kernel(const float* __restrict__ vol, Geo g, float level, Workspace ws,
                                                           float* __restrict__ verts, int32_t* __restrict__ faces) {
    __shared__ uint32_t wt[2][kThreads / 64];
    const int64_t voff = ws.voff[blockIdx.x], toff = ws.toff[blockIdx.x];
    uint32_t run_t = 0;
    const uint32_t first = blockIdx.x * uint32_t(kPoints);
    for (int j = 0; j < kChunks; j++) {
        const uint32_t idx = first + uint32_t(j * kThreads) + threadIdx.x;
        Point pt = {};
        if (idx < g.n) pt = classify(vol, g, level, idx);
        const uint32_t tri_pre = block_prefix<3>(pt.ntri, wt, j & 1, &run_t);
        if (pt.mask) {
            const uint32_t r = idx / g.d2, i2 = idx - r * g.d2;
            const uint32_t i0 = r / g.d1, i1 = r - i0 * g.d1;
            const float pos[3] = {float(i0), float(i1), float(i2)};
            int64_t vid = voff + int64_t(ws.base[idx] >> 3);
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (!(pt.mask & (1u << a))) continue;
                const float t = (level - pt.v) / (pt.vn[a] - pt.v);          // correctly rounded, not contracted (the numpy port's bits)
                float* out = verts + vid * 3;
                out[0] = a == 0 ? pos[0] + t : pos[0];
                out[1] = a == 1 ? pos[1] + t : pos[1];
                out[2] = a == 2 ? pos[2] + t : pos[2];
                vid++;
            }
        }
        if (pt.ntri) {
            int32_t* out = faces + (toff + int64_t(tri_pre)) * 3;
            const unsigned char* tri = kMcTriEdges[pt.cell_case];
            for (uint32_t k = 0; k < pt.ntri * 3; k++) {
                const uint32_t e = tri[k], c = kMcEdgeCorner[e];
                const uint32_t q = idx + ((c & 4) ? g.plane : 0u) + ((c & 2) ? g.d2 : 0u) + (c & 1);
                out[k] = vertex_id(ws, q, kMcEdgeAxis[e]);
            }
        }
    }
}

int check_shape(int d0, int d1, int d2, const char* what, Geo* g, uint32_t* nb) {
    using namespace gnerf;
    if (d0 < 2 || d1 < 2 || d2 < 2) return fail(GNERF_E_ARG, "%s: every dimension must be >= 2 (got %d x %d x %d)", what, d0, d1, d2);
    const int64_t n = int64_t(d0) * d1 * d2;
    if (n >= (int64_t(1) << 31)) return fail(GNERF_E_ARG, "%s: the volume must have fewer than 2^31 points", what);
    g->d0 = uint32_t(d0); g->d1 = uint32_t(d1); g->d2 = uint32_t(d2); g->plane = uint32_t(d1) * uint32_t(d2); g->n = uint32_t(n);
    *nb = uint32_t((n + kPoints - 1) / kPoints);
    return GNERF_OK;
}

}  // namespace

extern "C" int gnerf_marching_cubes_workspace_bytes(int d0, int d1, int d2, size_t* bytes) {
    using namespace gnerf;
    if (!bytes) return fail(GNERF_E_ARG, "marching_cubes_workspace_bytes: null pointer");
    Geo g;
    uint32_t nb;
    if (int rc = check_shape(d0, d1, d2, "marching_cubes_workspace_bytes", &g, &nb)) return rc;
    carve(nullptr, g.n, nb, bytes);
    return GNERF_OK;
}

extern "C" int gnerf_marching_cubes_count(const float* volume, int d0, int d1, int d2, float level, void* workspace, int64_t* counts,
                                          gnerf_stream_t stream) {
    using namespace gnerf;
    if (!volume || !workspace || !counts) return fail(GNERF_E_ARG, "marching_cubes_count: null pointer");
    Geo g;
    uint32_t nb;
    if (int rc = check_shape(d0, d1, d2, "marching_cubes_count", &g, &nb)) return rc;
    const Workspace ws = carve(workspace, g.n, nb, nullptr);
    hipLaunchKernelGGL(mc_count_kernel, dim3(nb), dim3(kThreads), 0, as_stream(stream), volume, g, level, ws);
    if (int rc = check_launch("marching_cubes_count")) return rc;
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(kMcScanThreads), 0, as_stream(stream), ws, nb, counts);
    return check_launch("marching_cubes_count (scan)");
}

extern "C" int gnerf_marching_cubes_emit(const float* volume, int d0, int d1, int d2, float level, const void* workspace, float* verts,
                                         int32_t* faces, gnerf_stream_t stream) {
    using namespace gnerf;
    if (!volume || !workspace) return fail(GNERF_E_ARG, "marching_cubes_emit: null pointer");
    Geo g;
    uint32_t nb;
    if (int rc = check_shape(d0, d1, d2, "marching_cubes_emit", &g, &nb)) return rc;
    const Workspace ws = carve(const_cast<void*>(workspace), g.n, nb, nullptr);
    hipLaunchKernelGGL(mc_emit_kernel, dim3(nb), dim3(kThreads), 0, as_stream(stream), volume, g, level, ws, verts, faces);
    return check_launch("marching_cubes_emit");
}
