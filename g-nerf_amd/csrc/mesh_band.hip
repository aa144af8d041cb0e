// The bookkeeping of the narrow-band density volume (include/gnerf_hip.h, gnerf_band_*; shape_mi355x.band_volume is the driver and
// band_volume_numpy the port that gives the same bits): which bricks of the lattice the surface runs through, which of their points a round
// still has to evaluate, and what the points that nobody evaluates are filled with.
//
// The lattice is n^3 points in linear order (axis 2 fastest).  A brick is s^3 cells; along an axis brick b spans the points
// min(b s, n - 1) .. min((b + 1) s, n - 1), so neighbours share their face points and the last brick may be partial; nb = ceil((n - 1) / s).
// One byte of state per brick: 0 inactive, 1 active, 2 new (active; evaluated in this round), 3 named by this round's growth.
//
//   seed    a thread per brick: its eight corners' sides -> state 2 or 0; the seeds are counted by the scanned passes below.
//   points  seed and grow leave the new bricks compacted into a list in brick order (block prefix + scan of the block totals: by index, never
//           by arrival) in the workspace, which the point passes and the next grow read; a wave per new brick walks its points 64 at a time and lists those that are neither coarse nor in a brick of state 1, a point that
//           several new bricks share going to the lowest brick -- count, scan of the bricks' counts, emit.  The count and the emit run the same
//           test, so the emitted list is the counted one.
//   grow    a wave per new brick and face whose neighbour is not active: one ballot per 64 face points; a mixed face names the neighbour with
//           a byte store of 3 (every writer stores the same value; readers take 0 and 3 alike).  Then the round closes: 2 -> 1, 3 -> 2, and
//           the new bricks are counted.
//   fill    a thread per point: neither coarse nor in an active brick -> the effective value of its coarse corner.  Reads coarse points
//           only, writes the others only: in place.
// Nothing depends on the order in which waves run: states, lists and volume are the same from run to run.
#include "common.h"

namespace {

#include "mesh_scan.h"

struct Band {
    uint32_t n, s, nb, bricks, points;            // bricks = nb^3, points = n^3 < 2^31
    int32_t keep[6];                              // kept index range [lo, hi) per axis: outside it the effective value is 0
};

struct Workspace {
    uint32_t* blk;                                // [blocks_of(bricks)] new bricks per block of the compaction, and their offsets
    uint32_t* off;
    int64_t* n_new;                               // the compaction's total: the bricks of state 2
    uint32_t* list;                               // [bricks] the new bricks, ascending
    uint32_t* cnt;                                // [bricks] listed points per new brick, and their offsets
    uint32_t* poff;
};

inline Workspace carve(void* ws, const Band& g, size_t* total) {
    char* p = static_cast<char*>(ws);
    size_t off = 0;
    Workspace w;
    w.blk = take<uint32_t>(p, &off, size_t(blocks_of(g.bricks)) * 4);
    w.off = take<uint32_t>(p, &off, size_t(blocks_of(g.bricks)) * 4);
    w.n_new = take<int64_t>(p, &off, 8);
    w.list = take<uint32_t>(p, &off, size_t(g.bricks) * 4);
    w.cnt = take<uint32_t>(p, &off, size_t(g.bricks) * 4);
    w.poff = take<uint32_t>(p, &off, size_t(g.bricks) * 4);
    if (total) *total = off;
    return w;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
}

__device__ __forceinline__ uint32_t bound(const Band& g, uint32_t b) { return min(b * g.s, g.n - 1u); }

// Whether the point's effective value -- 0 outside the kept ranges, the volume's inside -- is above the level (ties and NaN are not).
__device__ __forceinline__ bool inside(const float* vol, const Band& g, float level, uint32_t i0, uint32_t i1, uint32_t i2) {
    const bool kept = int32_t(i0) >= g.keep[0] && int32_t(i0) < g.keep[1] && int32_t(i1) >= g.keep[2] && int32_t(i1) < g.keep[3] &&
                      int32_t(i2) >= g.keep[4] && int32_t(i2) < g.keep[5];
    const float v = kept ? vol[(i0 * g.n + i1) * g.n + i2] : 0.f;
    return v > level;
}

struct Brick {
    uint32_t b[3], lo[3], ext[3];                 // coordinates, first point and number of points per axis
};

__device__ __forceinline__ Brick brick_of(const Band& g, uint32_t B) {
    Brick k;
    const uint32_t r = B / g.nb;
    k.b[2] = B - r * g.nb;
    k.b[0] = r / g.nb;
    k.b[1] = r - k.b[0] * g.nb;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        k.lo[a] = bound(g, k.b[a]);
        k.ext[a] = bound(g, k.b[a] + 1u) - k.lo[a] + 1u;
    }
    return k;
}

__global__ __launch_bounds__(kThreads) void band_seed_kernel(const float* __restrict__ vol, Band g, float level, unsigned char* __restrict__ state) {
    const uint32_t B = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (B >= g.bricks) return;
    const Brick k = brick_of(g, B);
    uint32_t in = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const uint32_t i0 = k.lo[0] + ((c & 4) ? k.ext[0] - 1u : 0u), i1 = k.lo[1] + ((c & 2) ? k.ext[1] - 1u : 0u), i2 = k.lo[2] + ((c & 1) ? k.ext[2] - 1u : 0u);
        in += inside(vol, g, level, i0, i1, i2) ? 1u : 0u;
    }
    state[B] = (in != 0u && in != 8u) ? 2 : 0;
}

// The compaction of the bricks of state 2: per-block counts, then (after scan_blocks_kernel) each its place in the list.
__global__ __launch_bounds__(kThreads) void band_new_count_kernel(const unsigned char* __restrict__ state, uint32_t bricks, uint32_t* __restrict__ blk) {
    __shared__ uint32_t wsum[2][kThreads / 64];
    uint32_t run = 0;
    const uint32_t first = blockIdx.x * uint32_t(kItems);
    for (int j = 0; j < kChunks; j++) {
        const uint32_t B = first + uint32_t(j * kThreads) + threadIdx.x;
        (void)block_prefix(B < bricks && state[B] == 2 ? 1u : 0u, wsum, j & 1, &run);
    }
    if (threadIdx.x == 0) blk[blockIdx.x] = run;
}

__global__ __launch_bounds__(kThreads) void band_new_emit_kernel(const unsigned char* __restrict__ state, uint32_t bricks, const uint32_t* __restrict__ off,
                                                                 uint32_t* __restrict__ list) {
    __shared__ uint32_t wsum[2][kThreads / 64];
    uint32_t run = off[blockIdx.x];
    const uint32_t first = blockIdx.x * uint32_t(kItems);
    for (int j = 0; j < kChunks; j++) {
        const uint32_t B = first + uint32_t(j * kThreads) + threadIdx.x;
        const bool is_new = B < bricks && state[B] == 2;
        const uint32_t at = block_prefix(is_new ? 1u : 0u, wsum, j & 1, &run);
        if (is_new) list[at] = B;
    }
}

// Whether brick B (k) lists its point p: not coarse, in no brick of state 1, and in no new brick of a lower index.
__device__ __forceinline__ bool point_listed(const unsigned char* __restrict__ state, const Band& g, uint32_t B, const Brick& k, const uint32_t (&p)[3]) {
    bool coarse = true, at_lo[3], at_hi[3], shared = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        coarse = coarse && (p[a] % g.s == 0u || p[a] == g.n - 1u);
        at_lo[a] = p[a] == k.lo[a] && k.b[a] > 0u;
        at_hi[a] = p[a] == k.lo[a] + k.ext[a] - 1u && k.b[a] + 1u < g.nb;
        shared = shared || at_lo[a] || at_hi[a];
    }
    if (coarse) return false;
    if (!shared) return true;
    for (int d0 = -1; d0 <= 1; d0++) {
        if ((d0 < 0 && !at_lo[0]) || (d0 > 0 && !at_hi[0])) continue;
        for (int d1 = -1; d1 <= 1; d1++) {
            if ((d1 < 0 && !at_lo[1]) || (d1 > 0 && !at_hi[1])) continue;
            for (int d2 = -1; d2 <= 1; d2++) {
                if ((d2 < 0 && !at_lo[2]) || (d2 > 0 && !at_hi[2]) || (d0 == 0 && d1 == 0 && d2 == 0)) continue;
                const uint32_t O = uint32_t(int32_t(B) + (d0 * int32_t(g.nb) + d1) * int32_t(g.nb) + d2);
                const unsigned char st = state[O];
                if (st == 1 || (st == 2 && O < B)) return false;
            }
        }
    }
    return true;
}

constexpr int kWaves = kThreads / 64;             // a wave per new brick in the point and growth passes

template <bool EMIT>
__global__ __launch_bounds__(kThreads) void band_points_kernel(const unsigned char* __restrict__ state, Band g, Workspace ws, int32_t* __restrict__ index,
                                                               uint32_t capacity) {
    const uint32_t n_new = uint32_t(*ws.n_new);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t j = blockIdx.x * uint32_t(kWaves) + (threadIdx.x >> 6); j < n_new; j += gridDim.x * uint32_t(kWaves)) {
        const uint32_t B = ws.list[j];
        const Brick k = brick_of(g, B);
        const uint32_t count = k.ext[0] * k.ext[1] * k.ext[2];
        uint32_t run = EMIT ? ws.poff[j] : 0u;
        for (uint32_t head = 0; head < count; head += 64u) {
            const uint32_t l = head + lane;
            bool listed = false;
            uint32_t idx = 0;
            if (l < count) {
                const uint32_t r = l / k.ext[2], l0 = r / k.ext[1];
                const uint32_t p[3] = {k.lo[0] + l0, k.lo[1] + (r - l0 * k.ext[1]), k.lo[2] + (l - r * k.ext[2])};
                listed = point_listed(state, g, B, k, p);
                idx = (p[0] * g.n + p[1]) * g.n + p[2];
            }
            const uint64_t m = __ballot(listed);
            if (EMIT) {
                const uint32_t at = run + lanes_below(m);
                if (listed && at < capacity) index[at] = int32_t(idx);
            }
            run += uint32_t(__popcll(m));
        }
        if (!EMIT && lane == 0u) ws.cnt[j] = run;
    }
}

// One workgroup: exclusive offsets of the new bricks' point counts -- scan_blocks_kernel for a length that lives on the device.
__global__ __launch_bounds__(kScanThreads) void band_scan_points_kernel(Workspace ws, int64_t* __restrict__ total) {
    __shared__ uint32_t sa[kScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n = uint32_t(*ws.n_new);
    uint32_t carry = 0;
    for (uint32_t head = 0; head < n; head += kScanThreads) {
        const uint32_t i = head + threadIdx.x;
        const uint32_t a0 = i < n ? ws.cnt[i] : 0u;
        uint32_t a = a0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t x = __shfl_up(a, o, 64);
            if (lane >= o) a += x;
        }
        if (lane == 63) sa[wave] = a;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int w = 0; w < kScanThreads / 64; w++) {
            before += w < wave ? sa[w] : 0u;
            all += sa[w];
        }
        if (i < n) ws.poff[i] = carry + before + a - a0;
        carry += all;
        __syncthreads();                                 // sa is rewritten by the next tile
    }
    if (threadIdx.x == 0) *total = int64_t(carry);
}

__global__ __launch_bounds__(kThreads) void band_grow_kernel(const float* __restrict__ vol, Band g, float level, Workspace ws, unsigned char* state) {
    const uint32_t n_new = uint32_t(*ws.n_new);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t j = blockIdx.x * uint32_t(kWaves) + (threadIdx.x >> 6); j < n_new; j += gridDim.x * uint32_t(kWaves)) {
        const uint32_t B = ws.list[j];
        const Brick k = brick_of(g, B);
        const int32_t stride[3] = {int32_t(g.nb * g.nb), int32_t(g.nb), 1};
#pragma unroll
        for (int face = 0; face < 6; face++) {
            const int a = face >> 1, up = face & 1, u = a == 0 ? 1 : 0, w = a == 2 ? 1 : 2;      // the face's other two axes, u before w
            if (up ? k.b[a] + 1u >= g.nb : k.b[a] == 0u) continue;
            const uint32_t O = uint32_t(int32_t(B) + (up ? stride[a] : -stride[a]));
            const unsigned char st = state[O];
            if (st == 1 || st == 2) continue;                                                // active already (0 and 3 are alike here)
            const uint32_t fixed = k.lo[a] + (up ? k.ext[a] - 1u : 0u), count = k.ext[u] * k.ext[w];
            bool any_in = false, any_out = false;
            for (uint32_t head = 0; head < count; head += 64u) {
                const uint32_t l = head + lane;
                bool in = false, out = false;
                if (l < count) {
                    const uint32_t lu = l / k.ext[w];
                    uint32_t p[3];
                    p[a] = fixed;
                    p[u] = k.lo[u] + lu;
                    p[w] = k.lo[w] + (l - lu * k.ext[w]);
                    in = inside(vol, g, level, p[0], p[1], p[2]);
                    out = !in;
                }
                any_in = any_in || __ballot(in) != 0;
                any_out = any_out || __ballot(out) != 0;
            }
            if (any_in && any_out && lane == 0u) state[O] = 3;
        }
    }
}

__global__ __launch_bounds__(kThreads) void band_close_round_kernel(unsigned char* __restrict__ state, uint32_t bricks) {
    const uint32_t B = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (B >= bricks) return;
    const unsigned char st = state[B];
    if (st == 2) state[B] = 1;
    if (st == 3) state[B] = 2;
}

__global__ __launch_bounds__(kThreads) void band_fill_kernel(float* vol, Band g, const unsigned char* __restrict__ state) {
    const uint32_t idx = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (idx >= g.points) return;
    const uint32_t r = idx / g.n;
    uint32_t p[3];
    p[2] = idx - r * g.n;
    p[0] = r / g.n;
    p[1] = r - p[0] * g.n;
    bool coarse = true;
    uint32_t first[3], more[3];                   // the bricks that hold the point along each axis: first, and first - 1 when more
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const uint32_t q = p[a] / g.s, rem = p[a] - q * g.s;
        coarse = coarse && (rem == 0u || p[a] == g.n - 1u);
        first[a] = min(q, g.nb - 1u);
        more[a] = (q < g.nb && rem == 0u && q > 0u) ? 1u : 0u;
    }
    if (coarse) return;
    for (uint32_t d0 = 0; d0 <= more[0]; d0++)
        for (uint32_t d1 = 0; d1 <= more[1]; d1++)
            for (uint32_t d2 = 0; d2 <= more[2]; d2++) {
                const unsigned char st = state[((first[0] - d0) * g.nb + (first[1] - d1)) * g.nb + (first[2] - d2)];
                if (st == 1 || st == 2) return;
            }
    const uint32_t c0 = p[0] / g.s * g.s, c1 = p[1] / g.s * g.s, c2 = p[2] / g.s * g.s;
    const bool kept = int32_t(c0) >= g.keep[0] && int32_t(c0) < g.keep[1] && int32_t(c1) >= g.keep[2] && int32_t(c1) < g.keep[3] &&
                      int32_t(c2) >= g.keep[4] && int32_t(c2) < g.keep[5];
    vol[idx] = kept ? vol[(c0 * g.n + c1) * g.n + c2] : 0.f;
}

int check_band(int n, int s, const int* keep, const char* what, Band* g) {
    using namespace gnerf;
    if (s != 2 && s != 4 && s != 8 && s != 16) return fail(GNERF_E_ARG, "%s: the brick edge must be 2, 4, 8 or 16 (got %d)", what, s);
    if (n < 2 || int64_t(n) * n * n >= (int64_t(1) << 31)) return fail(GNERF_E_ARG, "%s: n must be >= 2 with n^3 < 2^31 (got %d)", what, n);
    g->n = uint32_t(n);
    g->s = uint32_t(s);
    g->nb = uint32_t((n - 1 + s - 1) / s);
    g->bricks = g->nb * g->nb * g->nb;
    g->points = uint32_t(n) * uint32_t(n) * uint32_t(n);
    for (int a = 0; a < 3; a++) {
        const int lo = keep ? keep[2 * a] : 0, hi = keep ? keep[2 * a + 1] : n;
        g->keep[2 * a] = lo < 0 ? 0 : (lo > n ? n : lo);
        g->keep[2 * a + 1] = hi < 0 ? 0 : (hi > n ? n : hi);
    }
    return GNERF_OK;
}

__global__ void band_copy_count_kernel(const int64_t* __restrict__ n_new, int64_t* __restrict__ count) { *count = *n_new; }

// The bricks of state 2 -> ws.list (ascending) and ws.n_new, their number also to *count: what seed and grow leave for the calls behind them.
int compact_new(const unsigned char* state, const Band& g, const Workspace& ws, int64_t* count, hipStream_t stream, const char* what) {
    using namespace gnerf;
    const uint32_t nblk = blocks_of(g.bricks);
    hipLaunchKernelGGL(band_new_count_kernel, dim3(nblk), dim3(kThreads), 0, stream, state, g.bricks, ws.blk);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kScanThreads), 0, stream, ws.blk, ws.off, nblk, static_cast<const uint32_t*>(nullptr),
                       static_cast<uint32_t*>(nullptr), 0u, ws.n_new, static_cast<int64_t*>(nullptr));
    hipLaunchKernelGGL(band_copy_count_kernel, dim3(1), dim3(1), 0, stream, ws.n_new, count);
    hipLaunchKernelGGL(band_new_emit_kernel, dim3(nblk), dim3(kThreads), 0, stream, state, g.bricks, ws.off, ws.list);
    return check_launch(what);
}

inline uint32_t wave_grid(const Band& g) {
    const uint32_t want = (g.bricks + uint32_t(kWaves) - 1u) / uint32_t(kWaves), most = uint32_t(gnerf::kNumCU) * 16u;
    return want < most ? want : most;
}

}  // namespace

extern "C" int gnerf_band_workspace_bytes(int n, int s, size_t* bytes) {
    using namespace gnerf;
    if (!bytes) return fail(GNERF_E_ARG, "band_workspace_bytes: null pointer");
    Band g;
    if (int rc = check_band(n, s, nullptr, "band_workspace_bytes", &g)) return rc;
    carve(nullptr, g, bytes);
    return GNERF_OK;
}

extern "C" int gnerf_band_seed(const float* volume, int n, int s, float level, const int* keep, unsigned char* state, void* workspace,
                               int64_t* count, gnerf_stream_t stream) {
    using namespace gnerf;
    if (!volume || !state || !workspace || !count) return fail(GNERF_E_ARG, "band_seed: null pointer");
    Band g;
    if (int rc = check_band(n, s, keep, "band_seed", &g)) return rc;
    const Workspace ws = carve(workspace, g, nullptr);
    hipLaunchKernelGGL(band_seed_kernel, dim3(grid_of(g.bricks)), dim3(kThreads), 0, as_stream(stream), volume, g, level, state);
    if (int rc = check_launch("band_seed")) return rc;
    return compact_new(state, g, ws, count, as_stream(stream), "band_seed (count)");
}

extern "C" int gnerf_band_points_count(const unsigned char* state, int n, int s, void* workspace, int64_t* count, gnerf_stream_t stream) {
    using namespace gnerf;
    if (!state || !workspace || !count) return fail(GNERF_E_ARG, "band_points_count: null pointer");
    Band g;
    if (int rc = check_band(n, s, nullptr, "band_points_count", &g)) return rc;
    const Workspace ws = carve(workspace, g, nullptr);
    hipLaunchKernelGGL(band_points_kernel<false>, dim3(wave_grid(g)), dim3(kThreads), 0, as_stream(stream), state, g, ws, static_cast<int32_t*>(nullptr), 0u);
    hipLaunchKernelGGL(band_scan_points_kernel, dim3(1), dim3(kScanThreads), 0, as_stream(stream), ws, count);
    return check_launch("band_points_count");
}

extern "C" int gnerf_band_points_emit(const unsigned char* state, int n, int s, const void* workspace, int32_t* index, int64_t m, gnerf_stream_t stream) {
    using namespace gnerf;
    if (!state || !workspace) return fail(GNERF_E_ARG, "band_points_emit: null pointer");
    Band g;
    if (int rc = check_band(n, s, nullptr, "band_points_emit", &g)) return rc;
    if (m < 0 || m > int64_t(g.points)) return fail(GNERF_E_ARG, "band_points_emit: m must be the count gnerf_band_points_count gave");
    if (m == 0) return GNERF_OK;
    if (!index) return fail(GNERF_E_ARG, "band_points_emit: null pointer");
    const Workspace ws = carve(const_cast<void*>(workspace), g, nullptr);
    hipLaunchKernelGGL(band_points_kernel<true>, dim3(wave_grid(g)), dim3(kThreads), 0, as_stream(stream), state, g, ws, index, uint32_t(m));
    return check_launch("band_points_emit");
}

extern "C" int gnerf_band_grow(const float* volume, int n, int s, float level, const int* keep, unsigned char* state, void* workspace,
                               int64_t* count, gnerf_stream_t stream) {
    using namespace gnerf;
    if (!volume || !state || !workspace || !count) return fail(GNERF_E_ARG, "band_grow: null pointer");
    Band g;
    if (int rc = check_band(n, s, keep, "band_grow", &g)) return rc;
    const Workspace ws = carve(workspace, g, nullptr);
    hipLaunchKernelGGL(band_grow_kernel, dim3(wave_grid(g)), dim3(kThreads), 0, as_stream(stream), volume, g, level, ws, state);
    hipLaunchKernelGGL(band_close_round_kernel, dim3(grid_of(g.bricks)), dim3(kThreads), 0, as_stream(stream), state, g.bricks);
    if (int rc = check_launch("band_grow")) return rc;
    return compact_new(state, g, ws, count, as_stream(stream), "band_grow (count)");
}

extern "C" int gnerf_band_fill(float* volume, int n, int s, const int* keep, const unsigned char* state, gnerf_stream_t stream) {
    using namespace gnerf;
    if (!volume || !state) return fail(GNERF_E_ARG, "band_fill: null pointer");
    Band g;
    if (int rc = check_band(n, s, keep, "band_fill", &g)) return rc;
    hipLaunchKernelGGL(band_fill_kernel, dim3(grid_of(g.points)), dim3(kThreads), 0, as_stream(stream), volume, g, state);
    return check_launch("band_fill");
}
