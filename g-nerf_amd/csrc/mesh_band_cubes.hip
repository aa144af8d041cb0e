// Marching cubes over the active bricks of a narrow band (include/gnerf_hip.h, gnerf_band_mesh_*; shape_mi355x.band_marching_cubes_numpy is the
// port that gives the same bits): the volume is read as the band's rounds left it -- no fill --, only inside the closed point ranges of the
// active bricks, and in a VIEW (a permutation of the lattice axes and a flip per axis) with the crop applied on the fly.  The mesh is
// gnerf_marching_cubes_*'s of the filled, cropped, flipped and permuted volume, bit for bit and in the same vertex and face order.
//
// Everything below speaks MESH coordinates: mesh axis k is lattice axis perm[k], mirrored where that axis is flipped; mesh brick (bm0, bm1, bm2)
// spans the mesh points mlo_k .. mhi_k (closed).  Every lattice point is DEALT to the brick that holds its mesh-forward cell (the far boundary
// of an axis to the last brick), so a brick owns e_k = mhi_k - mlo_k points per axis, one more in the last brick: the dealt points of the
// active bricks hold every crossed edge's owner and every non-empty cell's lower corner, and all their reads lie in that brick's closed range.
//
// Order.  A brick's owned points split into e_0 e_1 row SEGMENTS along mesh axis 2.  In the mesh's point order the segments of the active
// bricks come by (m0, m1, bm2), so a segment's rank is a closed form:
//     rank = slab_s[bm0] + r0 slab_row[bm0] + (off_x[col] - off_x[bm0 nb]) + r1 col_a[col] + (the brick's rank in its column)
// with col = bm0 nb + bm1 the brick column along mesh axis 2, col_a its active bricks, off_x the exclusive scan of col_a e_1 over the columns,
// slab_row[bm0] the segments of one row plane of slab bm0 and slab_s the exclusive scan of e_0 slab_row.  Per-segment vertex and triangle
// counts go to that rank, and ONE scan over the segments gives every offset: by index, never by arrival, no float atomics.
//
// Launches of gnerf_band_mesh_count, on the caller's stream:
//   columns  a thread per brick column: its active bricks (and any state other than 0 / 1).
//   scan     the columns' counts -> slots of the active bricks (column-major) and off_x; then the slabs (one workgroup).
//   slots    a thread per column: brick -> slot map, slot -> brick list.
//   count    a team of threads per active brick, several bricks per workgroup at small s: the brick's closed range goes to LDS once, in
//            lattice order (rows of s + 1 contiguous floats), with the crop applied; then a thread per row segment walks it along mesh axis 2:
//            per point the crossed-axis mask and the prefix within the segment (2 bytes in the workspace), per segment its counts.
//   prefix   blocks of kItems segments: counts -> exclusive prefixes within the block, and the block totals.
//   totals   one workgroup: 64-bit block offsets, and the counts.
// gnerf_band_mesh_emit stages the bricks again; every point writes its vertices, every cell its faces, a face's vertex ids through the 2-byte
// words of the owners -- in a neighbouring brick through the brick -> slot map (that neighbour is active whenever the edge is crossed).
#include "common.h"
#include "mesh_tables.h"

#pragma clang fp contract(off)

namespace {

#include "mesh_scan.h"
#include "mesh_cubes.h"

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

struct View {
    uint32_t n, s, nb, cap;                       // cap: the slots the workspace holds (the caller's count of active bricks)
    int32_t keep[6];                              // kept index range [lo, hi) per LATTICE axis
    int32_t pa[3], fl[3];                         // per mesh axis k: its lattice axis, and whether that axis is flipped
    int32_t bstride[3], bbase;                    // brick index of mesh brick bm = bbase + sum bm_k bstride[k]
    float level;
};

struct Head {                                     // the device-side totals
    int64_t n_active, x_total;
    unsigned long long bad, visited;
    uint32_t n_seg, bad_state;
};

struct Workspace {
    Head* head;
    uint32_t *col_a, *col_x, *off_a, *off_x;      // [nb^2]
    uint32_t *slab_row, *slab_s;                  // [nb]
    uint32_t* map;                                // [nb^3] brick -> slot
    uint32_t* list;                               // [cap]  slot -> bm0 | bm1 << 10 | bm2 << 20
    uint16_t* words;                              // [cap (s+1)^3] (prefix within the segment << 3) | crossed-axis mask
    uint32_t *seg_v, *seg_t;                      // [cap (s+1)^2] per segment: counts, then exclusive prefixes within the block
    uint32_t *blk_v, *blk_t;                      // [blocks_of(cap (s+1)^2)]
    int64_t *voff, *toff;
};

inline Workspace carve(void* ws, const View& v, size_t* total) {
    char* p = static_cast<char*>(ws);
    size_t off = 0;
    const size_t cols = size_t(v.nb) * v.nb, P = v.s + 1, segs = size_t(v.cap) * P * P;
    const size_t nblk = (segs + kItems - 1) >> kItemsLog2;
    Workspace w;
    w.head = take<Head>(p, &off, sizeof(Head));
    w.col_a = take<uint32_t>(p, &off, cols * 4);
    w.col_x = take<uint32_t>(p, &off, cols * 4);
    w.off_a = take<uint32_t>(p, &off, cols * 4);
    w.off_x = take<uint32_t>(p, &off, cols * 4);
    w.slab_row = take<uint32_t>(p, &off, size_t(v.nb) * 4);
    w.slab_s = take<uint32_t>(p, &off, size_t(v.nb) * 4);
    w.map = take<uint32_t>(p, &off, cols * v.nb * 4);
    w.list = take<uint32_t>(p, &off, size_t(v.cap) * 4);
    w.words = take<uint16_t>(p, &off, size_t(v.cap) * P * P * P * 2);
    w.seg_v = take<uint32_t>(p, &off, segs * 4);
    w.seg_t = take<uint32_t>(p, &off, segs * 4);
    w.blk_v = take<uint32_t>(p, &off, nblk * 4);
    w.blk_t = take<uint32_t>(p, &off, nblk * 4);
    w.voff = take<int64_t>(p, &off, nblk * 8);
    w.toff = take<int64_t>(p, &off, nblk * 8);
    if (total) *total = off;
    return w;
}

// Mesh brick bm of mesh axis k: its first and last mesh point.
__device__ __forceinline__ int32_t mesh_lo(const View& v, int k, uint32_t bm) {
    const uint32_t last = v.n - 1u;
    return v.fl[k] ? int32_t(last - min((v.nb - bm) * v.s, last)) : int32_t(min(bm * v.s, last));
}
__device__ __forceinline__ int32_t mesh_hi(const View& v, int k, uint32_t bm) {
    const uint32_t last = v.n - 1u;
    return v.fl[k] ? int32_t(last - min((v.nb - 1u - bm) * v.s, last)) : int32_t(min((bm + 1u) * v.s, last));
}
// The points mesh brick bm owns along axis k: its cells' lower corners, and the far boundary in the last brick.
__device__ __forceinline__ uint32_t owned(const View& v, int k, uint32_t bm) {
    return uint32_t(mesh_hi(v, k, bm) - mesh_lo(v, k, bm)) + (bm + 1u == v.nb ? 1u : 0u);
}

__device__ __forceinline__ bool stopped(const View& v, const Head* head) {       // the caller's count was too small, or a state is not 0 / 1
    return head->n_active > int64_t(v.cap) || head->bad_state != 0u;
}

// The brick column a thread of the column passes takes: neighbouring threads follow the mesh axis that is the faster one in the lattice.
__device__ __forceinline__ bool column_of(const View& v, uint32_t* bm0, uint32_t* bm1) {
    const uint32_t t = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (t >= v.nb * v.nb) return false;
    const uint32_t slow = t / v.nb, fast = t - slow * v.nb;
    *bm0 = v.pa[0] > v.pa[1] ? fast : slow;
    *bm1 = v.pa[0] > v.pa[1] ? slow : fast;
    return true;
}

__global__ __launch_bounds__(kThreads) void bmc_columns_kernel(const unsigned char* __restrict__ state, View v, Workspace ws) {
    uint32_t bm0, bm1;
    if (!column_of(v, &bm0, &bm1)) return;
    int32_t B = v.bbase + int32_t(bm0) * v.bstride[0] + int32_t(bm1) * v.bstride[1];
    uint32_t a = 0, other = 0;
    for (uint32_t bm2 = 0; bm2 < v.nb; bm2++, B += v.bstride[2]) {
        const unsigned char st = state[B];
        a += st == 1 ? 1u : 0u;
        other |= st > 1 ? 1u : 0u;
    }
    const uint32_t col = bm0 * v.nb + bm1;
    ws.col_a[col] = a;
    ws.col_x[col] = a * owned(v, 1, bm1);
    if (other) atomicOr(&ws.head->bad_state, 1u);
}

// One workgroup (nb <= kScanThreads): the segments of one row plane per slab, the slabs' first segments, and the number of segments.
__global__ __launch_bounds__(kScanThreads) void bmc_slabs_kernel(View v, Workspace ws) {
    __shared__ uint32_t sa[kScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t i = threadIdx.x;
    uint32_t row = 0;
    if (i < v.nb) row = (i + 1u < v.nb ? ws.off_x[(i + 1u) * v.nb] : uint32_t(ws.head->x_total)) - ws.off_x[i * v.nb];
    const uint32_t a0 = i < v.nb ? row * owned(v, 0, i) : 0u;
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
    if (i < v.nb) {
        ws.slab_row[i] = row;
        ws.slab_s[i] = before + a - a0;
    }
    if (i == 0) ws.head->n_seg = all;
}

__global__ __launch_bounds__(kThreads) void bmc_slots_kernel(const unsigned char* __restrict__ state, View v, Workspace ws) {
    uint32_t bm0, bm1;
    if (!column_of(v, &bm0, &bm1)) return;
    const bool stop = stopped(v, ws.head);
    int32_t B = v.bbase + int32_t(bm0) * v.bstride[0] + int32_t(bm1) * v.bstride[1];
    uint32_t slot = ws.off_a[bm0 * v.nb + bm1];
    for (uint32_t bm2 = 0; bm2 < v.nb; bm2++, B += v.bstride[2]) {
        const bool active = !stop && state[B] == 1;
        ws.map[B] = active ? slot : kNoSlot;
        if (active) ws.list[slot++] = bm0 | (bm1 << 10) | (bm2 << 20);
    }
}

// One active brick as its team sees it.
struct Brick {
    uint32_t bm[3], c[3], e[3];                   // mesh brick coordinates, points of the closed range and owned points per mesh axis
    int32_t mlo[3], B;                            // first mesh point per axis, the brick's index in `state`
    uint32_t seg0, sr0, sr1;                      // rank of the segment of row (r0, r1) = seg0 + r0 sr0 + r1 sr1
};

__device__ __forceinline__ void segments_of(const View& v, const Workspace& ws, uint32_t bm0, uint32_t bm1, uint32_t slot, uint32_t* seg0, uint32_t* sr0,
                                            uint32_t* sr1) {
    const uint32_t col = bm0 * v.nb + bm1;
    *seg0 = ws.slab_s[bm0] + (ws.off_x[col] - ws.off_x[bm0 * v.nb]) + (slot - ws.off_a[col]);
    *sr0 = ws.slab_row[bm0];
    *sr1 = ws.col_a[col];
}

__device__ __forceinline__ Brick brick_of(const View& v, const Workspace& ws, uint32_t slot) {
    Brick k;
    const uint32_t packed = ws.list[slot];
    k.bm[0] = packed & 1023u;
    k.bm[1] = (packed >> 10) & 1023u;
    k.bm[2] = packed >> 20;
    k.B = v.bbase;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        k.mlo[a] = mesh_lo(v, a, k.bm[a]);
        k.c[a] = uint32_t(mesh_hi(v, a, k.bm[a]) - k.mlo[a]) + 1u;
        k.e[a] = k.c[a] - (k.bm[a] + 1u == v.nb ? 0u : 1u);
        k.B += int32_t(k.bm[a]) * v.bstride[a];
    }
    segments_of(v, ws, k.bm[0], k.bm[1], slot, &k.seg0, &k.sr0, &k.sr1);
    return k;
}

__device__ __forceinline__ uint32_t sel3(int32_t which, uint32_t x0, uint32_t x1, uint32_t x2) { return which == 0 ? x0 : (which == 1 ? x1 : x2); }

// Whether THIS brick counts its point r (local mesh coordinates in the closed range) among the visited ones: every visited point is counted
// by one active brick -- the one it is dealt to when that is active, else the active brick of the lowest index that holds it.
__device__ __forceinline__ bool counts_point(const unsigned char* __restrict__ state, const View& v, const Brick& k, const uint32_t (&r)[3]) {
    bool up[3], down[3], any_up = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        up[a] = r[a] == k.e[a];                                  // on the far face of a brick that is not the last: dealt onwards
        down[a] = r[a] == 0u && k.bm[a] > 0u;
        any_up = any_up || up[a];
    }
    if (!any_up) return true;
    const int32_t dealt = k.B + (up[0] ? v.bstride[0] : 0) + (up[1] ? v.bstride[1] : 0) + (up[2] ? v.bstride[2] : 0);
    if (state[dealt] == 1) return false;
    for (int d0 = -1; d0 <= 1; d0++) {
        if ((d0 < 0 && !down[0]) || (d0 > 0 && !up[0])) continue;
        for (int d1 = -1; d1 <= 1; d1++) {
            if ((d1 < 0 && !down[1]) || (d1 > 0 && !up[1])) continue;
            for (int d2 = -1; d2 <= 1; d2++) {
                if ((d2 < 0 && !down[2]) || (d2 > 0 && !up[2]) || (d0 == 0 && d1 == 0 && d2 == 0)) continue;
                const int32_t O = k.B + d0 * v.bstride[0] + d1 * v.bstride[1] + d2 * v.bstride[2];
                if (O < k.B && state[O] == 1) return false;
            }
        }
    }
    return true;
}

template <int S> struct Tile {
    static constexpr int P = S + 1, P3 = P * P * P, ROWS = P * P;
    static constexpr int TEAM = S == 16 ? 256 : (S == 8 ? 128 : (S == 4 ? 32 : 16));     // threads per brick
    static constexpr int BRICKS = kThreads / TEAM;                                       // bricks per workgroup
};

// The brick's closed range -> tile (mesh-local order, axis 2 fastest), read in LATTICE order so that a row of s + 1 floats is contiguous, the
// crop applied; COUNT also counts the visited and the non-finite points this brick answers for.
template <int S, bool COUNT>
__device__ __forceinline__ void stage(const float* __restrict__ vol, const unsigned char* __restrict__ state, const View& v, const Brick& k, bool live,
                                      uint32_t tt, float* tile, uint32_t* visited, uint32_t* bad) {
    using T = Tile<S>;
    if (!live) return;
    uint32_t cl[3] = {0, 0, 0};                                  // the closed range per LATTICE axis, and its first lattice point
    int32_t llo[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int m = 0; m < 3; m++)
            if (v.pa[m] == a) {
                cl[a] = k.c[m];
                llo[a] = v.fl[m] ? int32_t(v.n) - 1 - (k.mlo[m] + int32_t(k.c[m]) - 1) : k.mlo[m];
            }
    for (uint32_t l = tt; l < uint32_t(T::P3); l += uint32_t(T::TEAM)) {
        const uint32_t q01 = l / uint32_t(T::P), q2 = l - q01 * uint32_t(T::P), q0 = q01 / uint32_t(T::P), q1 = q01 - q0 * uint32_t(T::P);
        if (q0 >= cl[0] || q1 >= cl[1] || q2 >= cl[2]) continue;
        uint32_t r[3];
#pragma unroll
        for (int m = 0; m < 3; m++) {
            const uint32_t q = sel3(v.pa[m], q0, q1, q2);
            r[m] = v.fl[m] ? k.c[m] - 1u - q : q;
        }
        const int32_t i0 = llo[0] + int32_t(q0), i1 = llo[1] + int32_t(q1), i2 = llo[2] + int32_t(q2);
        const bool kept = i0 >= v.keep[0] && i0 < v.keep[1] && i1 >= v.keep[2] && i1 < v.keep[3] && i2 >= v.keep[4] && i2 < v.keep[5];
        const float e = kept ? vol[(uint32_t(i0) * v.n + uint32_t(i1)) * v.n + uint32_t(i2)] : 0.f;
        tile[(r[0] * uint32_t(T::P) + r[1]) * uint32_t(T::P) + r[2]] = e;
        if (COUNT && counts_point(state, v, k, r)) {
            *visited += 1u;
            *bad += __builtin_isfinite(e) ? 0u : 1u;
        }
    }
}

// The point (r0, r1, r2) of the staged brick: its cell's corners from the tile (a corner past the closed range reads the point itself).
template <int S>
__device__ __forceinline__ Point classify_tile(const float* tile, const Brick& k, float level, uint32_t r0, uint32_t r1, uint32_t r2) {
    constexpr uint32_t P = Tile<S>::P;
    const bool h0 = r0 + 1u < k.c[0], h1 = r1 + 1u < k.c[1], h2 = r2 + 1u < k.c[2];
    const uint32_t at = (r0 * P + r1) * P + r2;
    float cv[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const bool ok = (!(c & 4) || h0) && (!(c & 2) || h1) && (!(c & 1) || h2);
        const uint32_t off = ((c & 4) ? P * P : 0u) + ((c & 2) ? P : 0u) + ((c & 1) ? 1u : 0u);
        cv[c] = tile[ok ? at + off : at];
    }
    return classify_corners(cv, level, h0, h1, h2);
}

template <int S>
__global__ __launch_bounds__(kThreads) void bmc_count_kernel(const float* __restrict__ vol, const unsigned char* __restrict__ state, View v, Workspace ws) {
    using T = Tile<S>;
    __shared__ float tiles[T::BRICKS][T::P3];
    if (stopped(v, ws.head)) return;
    const uint32_t team = threadIdx.x / uint32_t(T::TEAM), tt = threadIdx.x - team * uint32_t(T::TEAM);
    const uint32_t slot = blockIdx.x * uint32_t(T::BRICKS) + team;
    const bool live = slot < uint32_t(ws.head->n_active);
    Brick k = {};
    if (live) k = brick_of(v, ws, slot);
    uint32_t visited = 0, bad = 0;
    stage<S, true>(vol, state, v, k, live, tt, tiles[team], &visited, &bad);
    __syncthreads();
    if (live) {
        for (uint32_t row = tt; row < uint32_t(T::ROWS); row += uint32_t(T::TEAM)) {
            const uint32_t r0 = row / uint32_t(T::P), r1 = row - r0 * uint32_t(T::P);
            if (r0 >= k.e[0] || r1 >= k.e[1]) continue;
            uint32_t nv = 0, nt = 0;
            uint16_t* words = ws.words + size_t(slot) * T::P3 + (r0 * uint32_t(T::P) + r1) * uint32_t(T::P);
            for (uint32_t r2 = 0; r2 < k.e[2]; r2++) {
                const Point pt = classify_tile<S>(tiles[team], k, v.level, r0, r1, r2);
                words[r2] = uint16_t((nv << 3) | pt.mask);
                nv += __popc(pt.mask);
                nt += pt.ntri;
            }
            const uint32_t seg = k.seg0 + r0 * k.sr0 + r1 * k.sr1;
            ws.seg_v[seg] = nv;
            ws.seg_t[seg] = nt;
        }
    }
    // the wave's counts: one integer atomic each (a sum: the same from run to run)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        visited += __shfl_xor(visited, o, 64);
        bad += __shfl_xor(bad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (visited) atomicAdd(&ws.head->visited, (unsigned long long)visited);
        if (bad) atomicAdd(&ws.head->bad, (unsigned long long)bad);
    }
}

// Blocks of kItems segments: the counts become exclusive prefixes within the block; the block totals.
__global__ __launch_bounds__(kThreads) void bmc_prefix_kernel(View v, Workspace ws) {
    __shared__ uint32_t wv[2][kThreads / 64], wt[2][kThreads / 64];
    if (stopped(v, ws.head)) return;
    const uint32_t n_seg = ws.head->n_seg, first = blockIdx.x * uint32_t(kItems);
    if (first >= n_seg) return;
    uint32_t run_v = 0, run_t = 0;
    for (int j = 0; j < kChunks; j++) {
        const uint32_t i = first + uint32_t(j * kThreads) + threadIdx.x;
        const uint32_t pv = block_prefix(i < n_seg ? ws.seg_v[i] : 0u, wv, j & 1, &run_v);
        const uint32_t pt = block_prefix(i < n_seg ? ws.seg_t[i] : 0u, wt, j & 1, &run_t);
        if (i < n_seg) {
            ws.seg_v[i] = pv;
            ws.seg_t[i] = pt;
        }
    }
    if (threadIdx.x == 0) {
        ws.blk_v[blockIdx.x] = run_v;
        ws.blk_t[blockIdx.x] = run_t;
    }
}

// One workgroup: the block offsets and counts = {V, T, non-finite, visited}; a refused call gives {0, 0, -1 (the caller's count of active
// bricks is too small) or -2 (a state other than 0 / 1), 0}.
__global__ __launch_bounds__(kMcScanThreads) void bmc_totals_kernel(View v, Workspace ws, int64_t* __restrict__ counts) {
    const bool stop = stopped(v, ws.head);
    const uint32_t nblk = stop ? 0u : (ws.head->n_seg + uint32_t(kItems) - 1u) >> kItemsLog2;
    scan_block_counts(ws.blk_v, ws.blk_t, nullptr, ws.voff, ws.toff, nblk, counts);
    if (threadIdx.x == 0) {
        counts[2] = stop ? (ws.head->bad_state ? -2 : -1) : int64_t(ws.head->bad);
        counts[3] = stop ? 0 : int64_t(ws.head->visited);
    }
}

// The owners a face of this brick can name: the brick itself and its seven forward neighbours (bit 2 - a of the entry: + 1 along mesh axis a).
struct Owner {
    uint32_t slot, seg0, sr0, sr1;
};

template <int S>
__global__ __launch_bounds__(kThreads) void bmc_emit_kernel(const float* __restrict__ vol, View v, Workspace ws, float* __restrict__ verts,
                                                            int32_t* __restrict__ faces) {
    using T = Tile<S>;
    constexpr uint32_t P = T::P;
    __shared__ float tiles[T::BRICKS][T::P3];
    __shared__ Owner owners[T::BRICKS][8];
    if (stopped(v, ws.head)) return;
    const uint32_t team = threadIdx.x / uint32_t(T::TEAM), tt = threadIdx.x - team * uint32_t(T::TEAM);
    const uint32_t slot = blockIdx.x * uint32_t(T::BRICKS) + team;
    const bool live = slot < uint32_t(ws.head->n_active);
    Brick k = {};
    if (live) k = brick_of(v, ws, slot);
    stage<S, false>(vol, nullptr, v, k, live, tt, tiles[team], nullptr, nullptr);
    if (live && tt < 8u) {
        const uint32_t d0 = (tt >> 2) & 1u, d1 = (tt >> 1) & 1u, d2 = tt & 1u;
        Owner o = {kNoSlot, 0u, 0u, 0u};
        if (k.bm[0] + d0 < v.nb && k.bm[1] + d1 < v.nb && k.bm[2] + d2 < v.nb) {
            o.slot = ws.map[k.B + int32_t(d0) * v.bstride[0] + int32_t(d1) * v.bstride[1] + int32_t(d2) * v.bstride[2]];
            if (o.slot != kNoSlot) segments_of(v, ws, k.bm[0] + d0, k.bm[1] + d1, o.slot, &o.seg0, &o.sr0, &o.sr1);
        }
        owners[team][tt] = o;
    }
    __syncthreads();
    if (!live) return;
    for (uint32_t row = tt; row < uint32_t(T::ROWS); row += uint32_t(T::TEAM)) {
        const uint32_t r0 = row / P, r1 = row - r0 * P;
        if (r0 >= k.e[0] || r1 >= k.e[1]) continue;
        const uint32_t seg = k.seg0 + r0 * k.sr0 + r1 * k.sr1;
        int64_t vid = ws.voff[seg >> kItemsLog2] + int64_t(ws.seg_v[seg]);
        int64_t tid = ws.toff[seg >> kItemsLog2] + int64_t(ws.seg_t[seg]);
        for (uint32_t r2 = 0; r2 < k.e[2]; r2++) {
            const Point pt = classify_tile<S>(tiles[team], k, v.level, r0, r1, r2);
            if (pt.mask) {
                const float pos[3] = {float(k.mlo[0] + int32_t(r0)), float(k.mlo[1] + int32_t(r1)), float(k.mlo[2] + int32_t(r2))};
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    if (!(pt.mask & (1u << a))) continue;
                    const float t = (v.level - pt.v) / (pt.vn[a] - pt.v);        // correctly rounded, not contracted (the numpy port's bits)
                    float* out = verts + vid * 3;
                    out[0] = a == 0 ? pos[0] + t : pos[0];
                    out[1] = a == 1 ? pos[1] + t : pos[1];
                    out[2] = a == 2 ? pos[2] + t : pos[2];
                    vid++;
                }
            }
            if (pt.ntri) {
                int32_t* out = faces + tid * 3;
                const unsigned char* tri = kMcTriEdges[pt.cell_case];
                for (uint32_t j = 0; j < pt.ntri * 3; j++) {
                    const uint32_t ed = tri[j], c = kMcEdgeCorner[ed], axis = kMcEdgeAxis[ed];
                    uint32_t q0 = r0 + ((c >> 2) & 1u), q1 = r1 + ((c >> 1) & 1u), q2 = r2 + (c & 1u);
                    const uint32_t u0 = q0 == k.e[0] ? 1u : 0u, u1 = q1 == k.e[1] ? 1u : 0u, u2 = q2 == k.e[2] ? 1u : 0u;   // dealt onwards
                    const Owner o = owners[team][(u0 << 2) | (u1 << 1) | u2];
                    int32_t id = 0;
                    if (o.slot != kNoSlot) {                                     // (always, when state and volume belong together)
                        q0 = u0 ? 0u : q0;
                        q1 = u1 ? 0u : q1;
                        q2 = u2 ? 0u : q2;
                        const uint32_t sg = o.seg0 + q0 * o.sr0 + q1 * o.sr1;
                        const uint32_t w = ws.words[size_t(o.slot) * T::P3 + (q0 * P + q1) * P + q2];
                        id = int32_t(ws.voff[sg >> kItemsLog2] + int64_t(ws.seg_v[sg]) + int64_t(w >> 3) + int64_t(__popc(w & ((1u << axis) - 1u))));
                    }
                    out[j] = id;
                }
                tid += pt.ntri;
            }
        }
    }
}

int check_view(int n, int s, const int* keep, const int* perm, const int* flip, int64_t active, const char* what, View* v) {
    using namespace gnerf;
    if (s != 2 && s != 4 && s != 8 && s != 16) return fail(GNERF_E_ARG, "%s: the brick edge must be 2, 4, 8 or 16 (got %d)", what, s);
    if (n < 2 || int64_t(n) * n * n >= (int64_t(1) << 31)) return fail(GNERF_E_ARG, "%s: n must be >= 2 with n^3 < 2^31 (got %d)", what, n);
    const int p0 = perm ? perm[0] : 0, p1 = perm ? perm[1] : 1, p2 = perm ? perm[2] : 2;
    if (p0 < 0 || p0 > 2 || p1 < 0 || p1 > 2 || p2 < 0 || p2 > 2 || p0 == p1 || p0 == p2 || p1 == p2)
        return fail(GNERF_E_ARG, "%s: perm must be a permutation of (0, 1, 2) (got %d, %d, %d)", what, p0, p1, p2);
    const int nb = (n - 1 + s - 1) / s;
    if (active < 0 || active > int64_t(nb) * nb * nb) return fail(GNERF_E_ARG, "%s: active must be a number of bricks, 0 .. nb^3", what);
    v->n = uint32_t(n);
    v->s = uint32_t(s);
    v->nb = uint32_t(nb);
    v->cap = uint32_t(active > 0 ? active : 1);
    for (int a = 0; a < 3; a++) {
        const int lo = keep ? keep[2 * a] : 0, hi = keep ? keep[2 * a + 1] : n;
        v->keep[2 * a] = lo < 0 ? 0 : (lo > n ? n : lo);
        v->keep[2 * a + 1] = hi < 0 ? 0 : (hi > n ? n : hi);
    }
    const int pa[3] = {p0, p1, p2};
    const int32_t bst[3] = {nb * nb, nb, 1};
    v->bbase = 0;
    for (int k = 0; k < 3; k++) {
        const int a = pa[k], f = (flip && flip[a]) ? 1 : 0;
        v->pa[k] = a;
        v->fl[k] = f;
        v->bstride[k] = f ? -bst[a] : bst[a];
        if (f) v->bbase += (nb - 1) * bst[a];
    }
    v->level = 0.f;
    return GNERF_OK;
}

inline uint32_t groups_of(const View& v) {
    const uint32_t per = v.s == 16 ? Tile<16>::BRICKS : (v.s == 8 ? Tile<8>::BRICKS : (v.s == 4 ? Tile<4>::BRICKS : Tile<2>::BRICKS));
    return (v.cap + per - 1u) / per;
}

}  // namespace

extern "C" int gnerf_band_mesh_workspace_bytes(int n, int s, int64_t active, size_t* bytes) {
    using namespace gnerf;
    if (!bytes) return fail(GNERF_E_ARG, "band_mesh_workspace_bytes: null pointer");
    View v;
    if (int rc = check_view(n, s, nullptr, nullptr, nullptr, active, "band_mesh_workspace_bytes", &v)) return rc;
    carve(nullptr, v, bytes);
    return GNERF_OK;
}

extern "C" int gnerf_band_mesh_count(const float* volume, const unsigned char* state, int n, int s, float level, const int* keep, const int* perm,
                                     const int* flip, int64_t active, void* workspace, int64_t* counts, gnerf_stream_t stream) {
    using namespace gnerf;
    if (!volume || !state || !workspace || !counts) return fail(GNERF_E_ARG, "band_mesh_count: null pointer");
    View v;
    if (int rc = check_view(n, s, keep, perm, flip, active, "band_mesh_count", &v)) return rc;
    v.level = level;
    const Workspace ws = carve(workspace, v, nullptr);
    hipStream_t st = as_stream(stream);
    const uint32_t cols = v.nb * v.nb, P = v.s + 1u;
    if (hipMemsetAsync(ws.head, 0, sizeof(Head), st) != hipSuccess) return fail(GNERF_E_LAUNCH, "band_mesh_count: hipMemsetAsync failed");
    hipLaunchKernelGGL(bmc_columns_kernel, dim3(grid_of(cols)), dim3(kThreads), 0, st, state, v, ws);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kScanThreads), 0, st, ws.col_a, ws.off_a, cols, ws.col_x, ws.off_x, cols, &ws.head->n_active,
                       &ws.head->x_total);
    hipLaunchKernelGGL(bmc_slabs_kernel, dim3(1), dim3(kScanThreads), 0, st, v, ws);
    hipLaunchKernelGGL(bmc_slots_kernel, dim3(grid_of(cols)), dim3(kThreads), 0, st, state, v, ws);
    if (int rc = check_launch("band_mesh_count (bricks)")) return rc;
    const dim3 grid(groups_of(v));
    if (v.s == 16) hipLaunchKernelGGL(bmc_count_kernel<16>, grid, dim3(kThreads), 0, st, volume, state, v, ws);
    else if (v.s == 8) hipLaunchKernelGGL(bmc_count_kernel<8>, grid, dim3(kThreads), 0, st, volume, state, v, ws);
    else if (v.s == 4) hipLaunchKernelGGL(bmc_count_kernel<4>, grid, dim3(kThreads), 0, st, volume, state, v, ws);
    else hipLaunchKernelGGL(bmc_count_kernel<2>, grid, dim3(kThreads), 0, st, volume, state, v, ws);
    if (int rc = check_launch("band_mesh_count")) return rc;
    const size_t segs = size_t(v.cap) * P * P;
    hipLaunchKernelGGL(bmc_prefix_kernel, dim3(uint32_t((segs + kItems - 1) >> kItemsLog2)), dim3(kThreads), 0, st, v, ws);
    hipLaunchKernelGGL(bmc_totals_kernel, dim3(1), dim3(kMcScanThreads), 0, st, v, ws, counts);
    return check_launch("band_mesh_count (scan)");
}

extern "C" int gnerf_band_mesh_emit(const float* volume, const unsigned char* state, int n, int s, float level, const int* keep, const int* perm,
                                    const int* flip, int64_t active, const void* workspace, float* verts, int32_t* faces, gnerf_stream_t stream) {
    using namespace gnerf;
    if (!volume || !state || !workspace || !verts) return fail(GNERF_E_ARG, "band_mesh_emit: null pointer");
    View v;
    if (int rc = check_view(n, s, keep, perm, flip, active, "band_mesh_emit", &v)) return rc;
    v.level = level;
    const Workspace ws = carve(const_cast<void*>(workspace), v, nullptr);
    hipStream_t st = as_stream(stream);
    const dim3 grid(groups_of(v));
    if (v.s == 16) hipLaunchKernelGGL(bmc_emit_kernel<16>, grid, dim3(kThreads), 0, st, volume, v, ws, verts, faces);
    else if (v.s == 8) hipLaunchKernelGGL(bmc_emit_kernel<8>, grid, dim3(kThreads), 0, st, volume, v, ws, verts, faces);
    else if (v.s == 4) hipLaunchKernelGGL(bmc_emit_kernel<4>, grid, dim3(kThreads), 0, st, volume, v, ws, verts, faces);
    else hipLaunchKernelGGL(bmc_emit_kernel<2>, grid, dim3(kThreads), 0, st, volume, v, ws, verts, faces);
    return check_launch("band_mesh_emit");
}
