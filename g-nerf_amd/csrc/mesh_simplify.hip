// Simplifying an extracted triangle mesh (between csrc/mesh_clean.hip's compaction and its smoothing): vertex clustering on a uniform grid with
// a quadric-error representative per cell -- gnerf_mesh_simplify_workspace_bytes / _count / _emit of include/gnerf_hip.h, which states the
// rules; shape_mi355x.py's mesh_simplify_numpy is the numpy port these kernels match bit for bit.  Every face id is range-checked before it is
// used as an index, and every vertex a face names is checked for finiteness before the face counts as valid.
//
// tables      two open-addressing tables in the workspace, one keyed by cell (items: used vertices), one by the sorted triple of new vertex ids
//     (items: faces that did not collapse), each of power-of-two capacity >= twice its items.  A slot stores ONLY the smallest item index seen
//     with its key: claimed with a 32-bit compare-and-swap, lowered with an atomic minimum.  Keys are compared by recomputing them from the item
//     the slot names, and only items of the slot's key ever lower it, so a slot's key never changes.  A plain load in front may return an older
//     value of the slot (this XCD's L2): empty, then the swap fails and hands back the newer one; or a larger item of the same key, which
//     compares the same.  No thread waits for another; every probe loop is bounded by the capacity and sets the internal-error word when it
//     runs out (it cannot while the table is at most half full; the Python layer raises on it).
// count       mark (per face: validity, used[] of its vertices) -> cells (per used vertex: its slot) -> representatives counted per block ->
//     scan -> new ids for the representatives (block prefix + block offset: ascending old index, never arrival order) -> vmap[] for everyone
//     -> group (per face: new ids, collapsed or its slot in the face table, +-1 into the slot's sigma) -> leaders with odd sigma counted per
//     block -> scan -> counts.  No quadrics.
// emit        on the workspace the count call left: the representatives zero their 13 accumulators; every used vertex adds q(u) and 1 to its
//     cluster; every valid face adds nine words to the cluster of each corner (27 64-bit integer adds per face, 4 per vertex, zeros not
//     sent).  One word takes only ~88 atomics per microsecond, and the coarser the grid the fewer the words: sent to memory one by one the
//     adds made this call 0.87-2.6 ms on the two 512^3 meshes, slower on the coarser grid.  So a block of 1024 consecutive faces or vertices
//     adds up in an LDS table first (BlockSums below) and sends each cluster's sums out once, and a wave whose lanes all aim at one cluster
//     reduces in registers before that: 0.10-0.29 ms.  Then every representative solves its 3 x 3 system and writes its
//     vertex, and the leaders with odd sigma write their faces at block prefix + block offset.  Integer adds in any order: the same bits on
//     every run and for every order of the faces.
#include "common.h"

#pragma clang fp contract(off)

namespace {

#include "mesh_scan.h"

constexpr uint32_t kEmpty = 0xFFFFFFFFu;             // a table slot nobody claimed; vslot[] of an unused vertex
constexpr uint32_t kFaceInvalid = 0xFFFFFFFFu;       // fslot[]: id out of range or a non-finite vertex
constexpr uint32_t kFaceCollapsed = 0xFFFFFFFEu;     //          valid, two new ids coincide
constexpr uint32_t kFaceValid = 0xFFFFFFFDu;         //          valid, not grouped yet; anything below: its slot in the face table
constexpr int kMaxItems = 1 << 30;                   // vertices or faces: a table of twice as many slots is addressed with 32 bits
constexpr int kAcc = 13;                             // per cluster: q(u) x 3, members, A00 A01 A02 A11 A12 A22, b0 b1 b2
constexpr int64_t kGridMax = (int64_t(1) << 21) - 1;
constexpr double kQ32 = 4294967296.0;
enum { kTallyInvalid = 0, kTallyCollapsed, kTallyGrouped, kTallyMulti, kTallyError, kTallies = 8 };

typedef unsigned long long u64;

struct Grid {
    float cell, o[3];
};

struct SimplifyWs {
    uint32_t *vtable, *ftable;                       // [cap_v], [cap_t]  (adjacent: one memset empties both)
    int32_t* sigma;                                  // [cap_t]           (sigma, tally, used adjacent: one memset zeroes them)
    u64* tally;                                      // [kTallies]
    unsigned char* used;                             // [V]
    uint32_t* vslot;                                 // [V] the vertex's slot in vtable, kEmpty when unused
    int32_t* vmap;                                   // [V] new id or -1
    uint32_t* fslot;                                 // [T] kFace* or the face's slot in ftable
    uint32_t *blk_v, *blk_t, *off_v, *off_t;
    u64* acc;                                        // [kAcc V]
    uint32_t cap_v, cap_t;
};

inline uint32_t capacity_of(uint32_t items) {
    uint32_t cap = 2;
    while (cap < 2 * (items ? items : 1u)) cap <<= 1;
    return cap;
}

inline SimplifyWs carve(void* ws, uint32_t nv, uint32_t nt, size_t* total) {
    char* p = static_cast<char*>(ws);
    size_t off = 0;
    SimplifyWs w;
    const uint32_t nbv = blocks_of(nv), nbt = blocks_of(nt);
    w.cap_v = capacity_of(nv);
    w.cap_t = capacity_of(nt);
    w.vtable = take<uint32_t>(p, &off, size_t(w.cap_v) * 4);
    w.ftable = take<uint32_t>(p, &off, size_t(w.cap_t) * 4);
    w.sigma = take<int32_t>(p, &off, size_t(w.cap_t) * 4);
    w.tally = take<u64>(p, &off, kTallies * 8);
    w.used = take<unsigned char>(p, &off, size_t(nv));
    w.vslot = take<uint32_t>(p, &off, size_t(nv) * 4);
    w.vmap = take<int32_t>(p, &off, size_t(nv) * 4);
    w.fslot = take<uint32_t>(p, &off, size_t(nt) * 4);
    w.blk_v = take<uint32_t>(p, &off, size_t(nbv) * 4);
    w.blk_t = take<uint32_t>(p, &off, size_t(nbt) * 4);
    w.off_v = take<uint32_t>(p, &off, size_t(nbv) * 4);
    w.off_t = take<uint32_t>(p, &off, size_t(nbt) * 4);
    w.acc = take<u64>(p, &off, size_t(nv) * kAcc * 8);
    if (total) *total = off;
    return w;
}

// ---------------------------------------------------------------------------------------------------------------- device helpers
__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// rule 2: p and k of vertex v (finite), per axis
__device__ __forceinline__ void cell_of(const float* __restrict__ verts, uint32_t v, const Grid& g, double (&p)[3], int64_t (&k)[3]) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
        p[a] = (double(verts[size_t(v) * 3 + a]) - double(g.o[a])) / double(g.cell);
        double fl = floor(p[a]);
        fl = fl < 0.0 ? 0.0 : fl;
        fl = fl > double(kGridMax) ? double(kGridMax) : fl;
        k[a] = int64_t(fl);
    }
}

__device__ __forceinline__ uint64_t key_of(const int64_t (&k)[3]) { return uint64_t(k[0]) << 42 | uint64_t(k[1]) << 21 | uint64_t(k[2]); }

__device__ __forceinline__ uint64_t vertex_key(const float* __restrict__ verts, uint32_t v, const Grid& g) {
    double p[3];
    int64_t k[3];
    cell_of(verts, v, g, p, k);
    return key_of(k);
}

__device__ __forceinline__ void local_of(const double (&p)[3], const int64_t (&k)[3], double (&u)[3]) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double x = p[a] - (double(k[a]) + 0.5);
        x = x < -0.5 ? -0.5 : x;
        u[a] = x > 0.5 ? 0.5 : x;
    }
}

__device__ __forceinline__ long long q32(double x) { return __double2ll_rn(x * kQ32); }

__device__ __forceinline__ uint32_t load_slot(const uint32_t* table, uint32_t slot) {
    return __hip_atomic_load(const_cast<uint32_t*>(table) + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// The slot of `item` in `table` (capacity mask + 1), which afterwards holds an item of the same key that is <= item; same(other): whether item
// `other` (something the table holds) has item's key.  kEmpty when the probe ran through the whole table.
template <class Same> __device__ __forceinline__ uint32_t table_insert(uint32_t* table, uint32_t mask, uint64_t hash, uint32_t item, Same same) {
    uint32_t slot = uint32_t(hash) & mask;
    for (uint32_t tries = 0; tries <= mask; tries++, slot = (slot + 1) & mask) {
        uint32_t cur = load_slot(table, slot);
        if (cur == kEmpty) {
            if (__hip_atomic_compare_exchange_strong(table + slot, &cur, item, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return slot;
        }                                              // (a failed swap left the slot's value in cur)
        if (cur == item || same(cur)) {
            if (item < cur) __hip_atomic_fetch_min(table + slot, item, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return slot;
        }
    }
    return kEmpty;
}

// the three ids of face t, and whether all of them name a vertex
__device__ __forceinline__ bool load_face(const int32_t* __restrict__ faces, uint32_t t, uint32_t nv, int32_t (&f)[3]) {
    f[0] = faces[size_t(t) * 3];
    f[1] = faces[size_t(t) * 3 + 1];
    f[2] = faces[size_t(t) * 3 + 2];
    return uint32_t(f[0]) < nv && uint32_t(f[1]) < nv && uint32_t(f[2]) < nv;
}

// the new ids of face t (whose old ids are in range), ascending in s[]; false when it collapses (or a vertex has no new id: internal error);
// even: the face is a rotation of s[]
__device__ __forceinline__ bool face_triple(const int32_t* __restrict__ faces, const int32_t* __restrict__ vmap, uint32_t t, int32_t (&s)[3], bool* even) {
    const int32_t a = vmap[faces[size_t(t) * 3]], b = vmap[faces[size_t(t) * 3 + 1]], c = vmap[faces[size_t(t) * 3 + 2]];
    if ((a | b | c) < 0 || a == b || b == c || a == c) return false;
    *even = int(a < b) + int(b < c) + int(c < a) == 2;
    const int32_t lo = min(a, min(b, c)), hi = max(a, max(b, c));
    s[0] = lo;
    s[1] = a ^ b ^ c ^ lo ^ hi;
    s[2] = hi;
    return true;
}

__device__ __forceinline__ uint64_t triple_hash(const int32_t (&s)[3]) { return mix64(mix64(uint64_t(uint32_t(s[0])) << 32 | uint32_t(s[1])) + uint32_t(s[2])); }

__device__ __forceinline__ void count_into(u64* word, bool flag) {
    const uint64_t m = __ballot(flag);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(word, u64(__popcll(m)));
}

// The accumulating kernels add up in LDS first: a block owns kSumItems consecutive vertices or faces -- neighbours on the surface, so a few
// dozen to a few hundred clusters -- and keeps an open-addressing table of kSumSlots (cluster, N sums) entries.  A contribution claims or finds
// its cluster's entry within kSumTries probes (a 32-bit compare-and-swap in LDS) and adds there; one that finds none goes to memory as it is.
// At the end every entry goes to memory, one 64-bit add per non-zero word.  Integer adds throughout: the same sums whichever way.
constexpr int kSumSlots = 512, kSumSlotsLog2 = 9, kSumTries = 8, kSumChunks = 4, kSumItems = kSumChunks * kThreads;
static_assert(kSumSlots == 1 << kSumSlotsLog2, "kSumSlots must be a power of two");
inline uint32_t sum_blocks_of(uint32_t n) { return (n + uint32_t(kSumItems) - 1) / uint32_t(kSumItems); }

template <int N> struct BlockSums {
    int32_t id[kSumSlots];                           // -1: free
    u64 sum[kSumSlots][N];
};

template <int N> __device__ __forceinline__ void sums_clear(BlockSums<N>& b) {
    for (int s = threadIdx.x; s < kSumSlots; s += kThreads) {
        b.id[s] = -1;
#pragma unroll
        for (int i = 0; i < N; i++) b.sum[s][i] = 0ull;
    }
    __syncthreads();
}

// one lane's x[0 .. N) -> words first .. first + N of cluster id
template <int N> __device__ __forceinline__ void sums_add(BlockSums<N>& b, u64* acc, int first, int32_t id, const u64 (&x)[N]) {
    uint32_t slot = (uint32_t(id) * 2654435761u) >> (32 - kSumSlotsLog2);
    for (int tries = 0; tries < kSumTries; tries++, slot = (slot + 1) & uint32_t(kSumSlots - 1)) {
        int32_t seen = __hip_atomic_load(&b.id[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (seen == -1) seen = atomicCAS(&b.id[slot], -1, id);
        if (seen == -1 || seen == id) {
#pragma unroll
            for (int i = 0; i < N; i++)
                if (x[i]) atomicAdd(&b.sum[slot][i], x[i]);
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < N; i++)
        if (x[i]) atomicAdd(acc + size_t(id) * kAcc + first + i, x[i]);
}

template <int N> __device__ __forceinline__ void sums_flush(BlockSums<N>& b, u64* acc, int first) {
    __syncthreads();
    for (int s = threadIdx.x; s < kSumSlots; s += kThreads) {
        const int32_t id = b.id[s];
        if (id < 0) continue;
#pragma unroll
        for (int i = 0; i < N; i++)
            if (b.sum[s][i]) atomicAdd(acc + size_t(id) * kAcc + first + i, b.sum[s][i]);
    }
}

// x[0 .. N) of every active lane -> words first .. first + N of cluster id's accumulators, through the block's sums.  Called by whole waves
// (active or not).  When all active lanes aim at one cluster, the wave adds up in registers and its first active lane alone goes on.
template <int N> __device__ __forceinline__ void add_to_cluster(BlockSums<N>& b, u64* acc, int32_t id, bool active, const long long (&x)[N], int first) {
    const uint64_t live = __ballot(active);
    if (!live) return;
    const int lead = __ffsll((unsigned long long)live) - 1;
    const int32_t lead_id = __shfl(id, lead, 64);
    u64 y[N];
    if (__ballot(active && id == lead_id) == live) {
#pragma unroll
        for (int i = 0; i < N; i++) {
            u64 s = active ? u64(x[i]) : 0ull;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += u64(__shfl_xor((long long)s, o, 64));
            y[i] = s;
        }
        if (int(threadIdx.x & 63) == lead) sums_add<N>(b, acc, first, lead_id, y);
    } else if (active) {
#pragma unroll
        for (int i = 0; i < N; i++) y[i] = u64(x[i]);
        sums_add<N>(b, acc, first, id, y);
    }
}

// ---------------------------------------------------------------------------------------------------------------- count
__global__ __launch_bounds__(kThreads) void simplify_mark_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, SimplifyWs ws, uint32_t nv,
                                                                 uint32_t nt) {
    const uint32_t t = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    bool bad = false;
    if (t < nt) {
        int32_t f[3];
        bool ok = load_face(faces, t, nv, f);
        if (ok) {
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int a = 0; a < 3; a++) ok = ok && finite_bits(verts[size_t(f[c]) * 3 + a]);
        }
        if (ok) {
#pragma unroll
            for (int c = 0; c < 3; c++) ws.used[f[c]] = 1;
        }
        ws.fslot[t] = ok ? kFaceValid : kFaceInvalid;
        bad = !ok;
    }
    count_into(ws.tally + kTallyInvalid, bad);
}

__global__ __launch_bounds__(kThreads) void simplify_cells_kernel(const float* __restrict__ verts, Grid g, SimplifyWs ws, uint32_t nv) {
    const uint32_t v = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (v >= nv) return;
    uint32_t slot = kEmpty;
    if (ws.used[v]) {
        const uint64_t key = vertex_key(verts, v, g);
        slot = table_insert(ws.vtable, ws.cap_v - 1, mix64(key), v, [&](uint32_t other) { return vertex_key(verts, other, g) == key; });
        if (slot == kEmpty) ws.tally[kTallyError] = 1ull;
    }
    ws.vslot[v] = slot;
}

__device__ __forceinline__ bool is_representative(const SimplifyWs& ws, uint32_t v) {
    const uint32_t slot = ws.vslot[v];
    return slot != kEmpty && ws.vtable[slot] == v;
}

__global__ __launch_bounds__(kThreads) void simplify_count_verts_kernel(SimplifyWs ws, uint32_t nv) {
    __shared__ uint32_t wsum[kThreads / 64];
    const uint32_t first = blockIdx.x * uint32_t(kItems);
    uint32_t mine = 0;
    for (int j = 0; j < kChunks; j++) {
        const uint32_t v = first + uint32_t(j * kThreads) + threadIdx.x;
        mine += uint32_t(__popcll(__ballot(v < nv && is_representative(ws, v))));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kThreads / 64; w++) s += wsum[w];
        ws.blk_v[blockIdx.x] = s;
    }
}

// representatives: their new id; unused vertices: -1
__global__ __launch_bounds__(kThreads) void simplify_number_kernel(SimplifyWs ws, uint32_t nv) {
    __shared__ uint32_t wsum[2][kThreads / 64];
    uint32_t running = ws.off_v[blockIdx.x];
    const uint32_t first = blockIdx.x * uint32_t(kItems);
    for (int j = 0; j < kChunks; j++) {
        const uint32_t v = first + uint32_t(j * kThreads) + threadIdx.x;
        const bool rep = v < nv && is_representative(ws, v);
        const uint32_t id = block_prefix(rep ? 1u : 0u, wsum, j & 1, &running);
        if (rep) ws.vmap[v] = int32_t(id);
        else if (v < nv && ws.vslot[v] == kEmpty) ws.vmap[v] = -1;
    }
}

// everyone else: the id of their representative (whose entry the kernel before wrote and this one leaves alone)
__global__ __launch_bounds__(kThreads) void simplify_map_kernel(SimplifyWs ws, uint32_t nv) {
    const uint32_t v = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (v >= nv) return;
    const uint32_t slot = ws.vslot[v];
    if (slot == kEmpty) return;
    const uint32_t rep = ws.vtable[slot];
    if (rep != v) ws.vmap[v] = ws.vmap[rep];
}

// A block owns kItems consecutive faces and sends its two tallies out once: nearly every wave has collapsed and grouped faces, and one word
// takes only ~88 atomics per microsecond (an add per wave and word made this kernel 0.57 ms of a 0.71 ms call on 1.58 M faces; that call is 0.17 ms now).
__global__ __launch_bounds__(kThreads) void simplify_group_kernel(const int32_t* __restrict__ faces, SimplifyWs ws, uint32_t nt) {
    __shared__ uint32_t s_collapsed[kThreads / 64], s_grouped[kThreads / 64];
    uint32_t n_collapsed = 0, n_grouped = 0;             // wave-uniform
    const uint32_t first = blockIdx.x * uint32_t(kItems);
    for (int j = 0; j < kChunks; j++) {
        const uint32_t t = first + uint32_t(j * kThreads) + threadIdx.x;
        bool collapsed = false, grouped = false;
        if (t < nt && ws.fslot[t] == kFaceValid) {
            int32_t s[3];
            bool even;
            uint32_t slot = kFaceCollapsed;
            if (face_triple(faces, ws.vmap, t, s, &even)) {
                slot = table_insert(ws.ftable, ws.cap_t - 1, triple_hash(s), t, [&](uint32_t other) {
                    int32_t o[3];
                    bool e;
                    return face_triple(faces, ws.vmap, other, o, &e) && o[0] == s[0] && o[1] == s[1] && o[2] == s[2];
                });
                if (slot == kEmpty) {
                    ws.tally[kTallyError] = 1ull;
                    slot = kFaceCollapsed;
                } else {
                    atomicAdd(ws.sigma + slot, even ? 1 : -1);
                    grouped = true;
                }
            }
            collapsed = !grouped;
            ws.fslot[t] = slot;
        }
        n_collapsed += uint32_t(__popcll(__ballot(collapsed)));
        n_grouped += uint32_t(__popcll(__ballot(grouped)));
    }
    if ((threadIdx.x & 63) == 0) {
        s_collapsed[threadIdx.x >> 6] = n_collapsed;
        s_grouped[threadIdx.x >> 6] = n_grouped;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0, g = 0;
        for (int w = 0; w < kThreads / 64; w++) {
            c += s_collapsed[w];
            g += s_grouped[w];
        }
        if (c) atomicAdd(ws.tally + kTallyCollapsed, u64(c));
        if (g) atomicAdd(ws.tally + kTallyGrouped, u64(g));
    }
}

// whether face t leads its group (is its smallest face), and the group's sigma
__device__ __forceinline__ bool is_leader(const SimplifyWs& ws, uint32_t t, int32_t* sigma) {
    const uint32_t slot = ws.fslot[t];
    if (slot >= kFaceValid || ws.ftable[slot] != t) return false;
    *sigma = ws.sigma[slot];
    return true;
}

__global__ __launch_bounds__(kThreads) void simplify_count_faces_kernel(SimplifyWs ws, uint32_t nt) {
    __shared__ uint32_t wsum[kThreads / 64];
    const uint32_t first = blockIdx.x * uint32_t(kItems);
    uint32_t mine = 0, multi = 0;
    for (int j = 0; j < kChunks; j++) {
        const uint32_t t = first + uint32_t(j * kThreads) + threadIdx.x;
        int32_t sigma = 0;
        const bool lead = t < nt && is_leader(ws, t, &sigma);
        mine += uint32_t(__popcll(__ballot(lead && (sigma & 1))));
        multi += uint32_t(__popcll(__ballot(lead && (sigma >= 2 || sigma <= -2))));
    }
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6] = mine;
        if (multi) atomicAdd(ws.tally + kTallyMulti, u64(multi));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kThreads / 64; w++) s += wsum[w];
        ws.blk_t[blockIdx.x] = s;
    }
}

// counts[0] and [1] are the scans' totals
__global__ void simplify_counts_kernel(SimplifyWs ws, int64_t* __restrict__ counts) {
    if (threadIdx.x != 0) return;
    counts[2] = int64_t(ws.tally[kTallyInvalid]);
    counts[3] = int64_t(ws.tally[kTallyCollapsed]);
    counts[4] = int64_t(ws.tally[kTallyGrouped]) - counts[1];
    counts[5] = int64_t(ws.tally[kTallyMulti]);
    counts[6] = int64_t(ws.tally[kTallyError]);
    counts[7] = 0;
}

// ---------------------------------------------------------------------------------------------------------------- emit
__global__ __launch_bounds__(kThreads) void simplify_zero_kernel(SimplifyWs ws, uint32_t nv) {
    const uint32_t v = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (v >= nv || !is_representative(ws, v)) return;
    u64* a = ws.acc + size_t(ws.vmap[v]) * kAcc;
#pragma unroll
    for (int i = 0; i < kAcc; i++) a[i] = 0ull;
}

__global__ __launch_bounds__(kThreads) void simplify_accumulate_verts_kernel(const float* __restrict__ verts, Grid g, SimplifyWs ws, uint32_t nv) {
    __shared__ BlockSums<4> sums;
    sums_clear(sums);
    const uint32_t head = blockIdx.x * uint32_t(kSumItems);
    for (int j = 0; j < kSumChunks; j++) {
        const uint32_t v = head + uint32_t(j * kThreads) + threadIdx.x;
        int32_t id = -1;
        long long x[4] = {0, 0, 0, 1};
        if (v < nv && ws.vslot[v] != kEmpty) {
            id = ws.vmap[v];
            double p[3], u[3];
            int64_t k[3];
            cell_of(verts, v, g, p, k);
            local_of(p, k, u);
#pragma unroll
            for (int a = 0; a < 3; a++) x[a] = q32(u[a]);
        }
        add_to_cluster<4>(sums, ws.acc, id, id >= 0, x, 0);
    }
    sums_flush(sums, ws.acc, 0);
}

__global__ __launch_bounds__(kThreads) void simplify_accumulate_faces_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, Grid g, SimplifyWs ws,
                                                                             uint32_t nv, uint32_t nt) {
    __shared__ BlockSums<9> sums;
    sums_clear(sums);
    const uint32_t head = blockIdx.x * uint32_t(kSumItems);
    for (int j = 0; j < kSumChunks; j++) {
        const uint32_t t = head + uint32_t(j * kThreads) + threadIdx.x;
        bool live = false;
        int32_t id[3] = {-1, -1, -1};
        double n[3] = {0, 0, 0}, u[3][3] = {}, f = 1.0;
        int32_t raw[3];
        if (t < nt && ws.fslot[t] != kFaceInvalid && load_face(faces, t, nv, raw)) {
            const int first = raw[0] <= raw[1] ? (raw[0] <= raw[2] ? 0 : 2) : (raw[1] <= raw[2] ? 1 : 2);      // the first smallest id
            double p[3][3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int32_t v = raw[(first + c) % 3];
                int64_t k[3];
                cell_of(verts, uint32_t(v), g, p[c], k);
                local_of(p[c], k, u[c]);
                id[c] = ws.vmap[v];
            }
            double e1[3], e2[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                e1[a] = p[1][a] - p[0][a];
                e2[a] = p[2][a] - p[0][a];
            }
            n[0] = e1[1] * e2[2] - e1[2] * e2[1];
            n[1] = e1[2] * e2[0] - e1[0] * e2[2];
            n[2] = e1[0] * e2[1] - e1[1] * e2[0];
            const double s = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
            live = s > 0.0 && s < __builtin_inf();
            f = s > 16.0 ? 16.0 / s : 1.0;
        }
        long long x[9] = {};
        if (live) {
            const double fn[3] = {f * n[0], f * n[1], f * n[2]};
            x[0] = q32(fn[0] * n[0]);
            x[1] = q32(fn[0] * n[1]);
            x[2] = q32(fn[0] * n[2]);
            x[3] = q32(fn[1] * n[1]);
            x[4] = q32(fn[1] * n[2]);
            x[5] = q32(fn[2] * n[2]);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (live) {
                const double d = (n[0] * u[c][0] + n[1] * u[c][1]) + n[2] * u[c][2];
                const double fd = f * d;
#pragma unroll
                for (int a = 0; a < 3; a++) x[6 + a] = q32(n[a] * fd);
            }
            add_to_cluster<9>(sums, ws.acc, id[c], live && id[c] >= 0, x, 4);
        }
    }
    sums_flush(sums, ws.acc, 4);
}

// rule 4 on the sums of one cluster -> x in [-0.5, 0.5]
__device__ __forceinline__ void solve_cluster(const u64* __restrict__ a, double (&x)[3]) {
    double w[kAcc];
#pragma unroll
    for (int i = 0; i < kAcc; i++) w[i] = double((long long)a[i]);
    const double members = w[3];
    const double cen[3] = {(w[0] / kQ32) / members, (w[1] / kQ32) / members, (w[2] / kQ32) / members};
    double m00 = w[4] / kQ32, m01 = w[5] / kQ32, m02 = w[6] / kQ32, m11 = w[7] / kQ32, m12 = w[8] / kQ32, m22 = w[9] / kQ32;
    const double b0 = w[10] / kQ32, b1 = w[11] / kQ32, b2 = w[12] / kQ32;
    const double tr = (m00 + m11) + m22;
    const double mu = tr / 256.0;
    m00 = m00 + mu;
    m11 = m11 + mu;
    m22 = m22 + mu;
    const double r0 = b0 + mu * cen[0];
    double r1 = b1 + mu * cen[1], r2 = b2 + mu * cen[2];
    const double l10 = m01 / m00, l20 = m02 / m00;
    m11 = m11 - l10 * m01;
    m12 = m12 - l10 * m02;
    m22 = m22 - l20 * m02;
    r1 = r1 - l10 * r0;
    r2 = r2 - l20 * r0;
    const double l21 = m12 / m11;
    m22 = m22 - l21 * m12;
    r2 = r2 - l21 * r1;
    const double x2 = r2 / m22;
    const double x1 = (r1 - m12 * x2) / m11;
    const double x0 = ((r0 - m01 * x1) - m02 * x2) / m00;
    const bool solved = tr > 0.0 && m00 > 0.0 && m11 > 0.0 && m22 > 0.0 && x0 - x0 == 0.0 && x1 - x1 == 0.0 && x2 - x2 == 0.0;
    const double sol[3] = {x0, x1, x2};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double y = solved ? sol[i] : cen[i];
        y = y < -0.5 ? -0.5 : y;
        x[i] = y > 0.5 ? 0.5 : y;
    }
}

__global__ __launch_bounds__(kThreads) void simplify_place_kernel(const float* __restrict__ verts, Grid g, SimplifyWs ws, uint32_t nv, float* __restrict__ out_verts,
                                                                  int32_t* __restrict__ src_vertex, int32_t* __restrict__ vertex_map) {
    const uint32_t v = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (v >= nv) return;
    const int32_t id = ws.vmap[v];
    if (vertex_map) vertex_map[v] = id;
    if (id < 0 || !is_representative(ws, v)) return;
    double p[3], x[3];
    int64_t k[3];
    cell_of(verts, v, g, p, k);
    solve_cluster(ws.acc + size_t(id) * kAcc, x);
#pragma unroll
    for (int a = 0; a < 3; a++) out_verts[size_t(id) * 3 + a] = float(double(g.o[a]) + ((double(k[a]) + 0.5) + x[a]) * double(g.cell));
    src_vertex[id] = int32_t(v);
}

__global__ __launch_bounds__(kThreads) void simplify_emit_faces_kernel(const int32_t* __restrict__ faces, SimplifyWs ws, uint32_t nv, uint32_t nt,
                                                                       int32_t* __restrict__ out_faces) {
    __shared__ uint32_t wsum[2][kThreads / 64];
    uint32_t running = ws.off_t[blockIdx.x];
    const uint32_t first = blockIdx.x * uint32_t(kItems);
    for (int j = 0; j < kChunks; j++) {
        const uint32_t t = first + uint32_t(j * kThreads) + threadIdx.x;
        int32_t sigma = 0, s[3] = {0, 0, 0}, raw[3];
        bool even;
        const bool kept = t < nt && is_leader(ws, t, &sigma) && (sigma & 1) && load_face(faces, t, nv, raw) && face_triple(faces, ws.vmap, t, s, &even);
        const uint32_t id = block_prefix(kept ? 1u : 0u, wsum, j & 1, &running);
        if (kept) {
            out_faces[size_t(id) * 3] = s[0];
            out_faces[size_t(id) * 3 + 1] = sigma > 0 ? s[1] : s[2];
            out_faces[size_t(id) * 3 + 2] = sigma > 0 ? s[2] : s[1];
        }
    }
}

int check_mesh(int n_verts, int n_tris, float cell, const float* origin, Grid* g, const char* what) {
    using namespace gnerf;
    if (n_verts < 0 || n_tris < 0) return fail(GNERF_E_ARG, "%s: negative size (%d vertices, %d faces)", what, n_verts, n_tris);
    if (n_verts > kMaxItems || n_tris > kMaxItems) return fail(GNERF_E_ARG, "%s: more than 2^30 vertices or faces", what);
    if (!origin) return fail(GNERF_E_ARG, "%s: null pointer (origin)", what);
    if (!(cell > 0.f) || !(cell <= 3.402823466e38f)) return fail(GNERF_E_ARG, "%s: cell must be finite and > 0 (got %g)", what, double(cell));
    for (int a = 0; a < 3; a++)
        if (!(origin[a] >= -3.402823466e38f && origin[a] <= 3.402823466e38f)) return fail(GNERF_E_ARG, "%s: origin must be finite", what);
    g->cell = cell;
    for (int a = 0; a < 3; a++) g->o[a] = origin[a];
    return GNERF_OK;
}

}  // namespace

extern "C" int gnerf_mesh_simplify_workspace_bytes(int n_verts, int n_tris, size_t* bytes) {
    using namespace gnerf;
    if (!bytes) return fail(GNERF_E_ARG, "mesh_simplify_workspace_bytes: null pointer");
    if (n_verts < 0 || n_tris < 0) return fail(GNERF_E_ARG, "mesh_simplify_workspace_bytes: negative size (%d vertices, %d faces)", n_verts, n_tris);
    if (n_verts > kMaxItems || n_tris > kMaxItems) return fail(GNERF_E_ARG, "mesh_simplify_workspace_bytes: more than 2^30 vertices or faces");
    carve(nullptr, uint32_t(n_verts), uint32_t(n_tris), bytes);
    return GNERF_OK;
}

extern "C" int gnerf_mesh_simplify_count(const float* verts, const int32_t* faces, int n_verts, int n_tris, float cell, const float* origin,
                                         void* workspace, int64_t* counts, gnerf_stream_t stream) {
    using namespace gnerf;
    Grid g;
    if (int rc = check_mesh(n_verts, n_tris, cell, origin, &g, "mesh_simplify_count")) return rc;
    if (!workspace || !counts || (n_tris && !faces) || (n_verts && !verts)) return fail(GNERF_E_ARG, "mesh_simplify_count: null pointer");
    const uint32_t nv = uint32_t(n_verts), nt = uint32_t(n_tris), nbv = blocks_of(nv), nbt = blocks_of(nt);
    const SimplifyWs ws = carve(workspace, nv, nt, nullptr);
    hipStream_t s = as_stream(stream);
    // vtable and ftable are adjacent, and so are sigma, tally and used: one memset each
    if (hipMemsetAsync(ws.vtable, 0xFF, size_t(reinterpret_cast<char*>(ws.sigma) - reinterpret_cast<char*>(ws.vtable)), s) != hipSuccess ||
        hipMemsetAsync(ws.sigma, 0, size_t(reinterpret_cast<char*>(ws.vslot) - reinterpret_cast<char*>(ws.sigma)), s) != hipSuccess)
        return fail(GNERF_E_LAUNCH, "mesh_simplify_count: memset failed");
    if (nt) {                                            // (without vertices every face is invalid, and verts is never read)
        hipLaunchKernelGGL(simplify_mark_kernel, dim3(grid_of(nt)), dim3(kThreads), 0, s, verts, faces, ws, nv, nt);
        if (int rc = check_launch("mesh_simplify_count (mark)")) return rc;
    }
    if (nv) {
        hipLaunchKernelGGL(simplify_cells_kernel, dim3(grid_of(nv)), dim3(kThreads), 0, s, verts, g, ws, nv);
        if (int rc = check_launch("mesh_simplify_count (cells)")) return rc;
        hipLaunchKernelGGL(simplify_count_verts_kernel, dim3(nbv), dim3(kThreads), 0, s, ws, nv);
        if (int rc = check_launch("mesh_simplify_count (representatives)")) return rc;
    }
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kScanThreads), 0, s, ws.blk_v, ws.off_v, nbv, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, counts,
                       (int64_t*)nullptr);
    if (int rc = check_launch("mesh_simplify_count (vertex scan)")) return rc;
    if (nv) {
        hipLaunchKernelGGL(simplify_number_kernel, dim3(nbv), dim3(kThreads), 0, s, ws, nv);
        if (int rc = check_launch("mesh_simplify_count (ids)")) return rc;
        hipLaunchKernelGGL(simplify_map_kernel, dim3(grid_of(nv)), dim3(kThreads), 0, s, ws, nv);
        if (int rc = check_launch("mesh_simplify_count (map)")) return rc;
    }
    if (nt && nv) {
        hipLaunchKernelGGL(simplify_group_kernel, dim3(nbt), dim3(kThreads), 0, s, faces, ws, nt);
        if (int rc = check_launch("mesh_simplify_count (groups)")) return rc;
        hipLaunchKernelGGL(simplify_count_faces_kernel, dim3(nbt), dim3(kThreads), 0, s, ws, nt);
        if (int rc = check_launch("mesh_simplify_count (leaders)")) return rc;
    }
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kScanThreads), 0, s, ws.blk_t, ws.off_t, (nt && nv) ? nbt : 0u, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                       0u, counts + 1, (int64_t*)nullptr);
    if (int rc = check_launch("mesh_simplify_count (face scan)")) return rc;
    hipLaunchKernelGGL(simplify_counts_kernel, dim3(1), dim3(64), 0, s, ws, counts);
    return check_launch("mesh_simplify_count (counts)");
}

extern "C" int gnerf_mesh_simplify_emit(const float* verts, const int32_t* faces, int n_verts, int n_tris, float cell, const float* origin,
                                        void* workspace, float* out_verts, int32_t* out_faces, int32_t* src_vertex, int32_t* vertex_map,
                                        gnerf_stream_t stream) {
    using namespace gnerf;
    Grid g;
    if (int rc = check_mesh(n_verts, n_tris, cell, origin, &g, "mesh_simplify_emit")) return rc;
    if (!workspace || !verts || !faces || !out_verts || !src_vertex) return fail(GNERF_E_ARG, "mesh_simplify_emit: null pointer");
    if (n_verts == 0 || n_tris == 0) return fail(GNERF_E_ARG, "mesh_simplify_emit: an empty mesh has no new vertices (V' == 0: do not call)");
    const uint32_t nv = uint32_t(n_verts), nt = uint32_t(n_tris);
    const SimplifyWs ws = carve(workspace, nv, nt, nullptr);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(simplify_zero_kernel, dim3(grid_of(nv)), dim3(kThreads), 0, s, ws, nv);
    if (int rc = check_launch("mesh_simplify_emit (zero)")) return rc;
    hipLaunchKernelGGL(simplify_accumulate_verts_kernel, dim3(sum_blocks_of(nv)), dim3(kThreads), 0, s, verts, g, ws, nv);
    if (int rc = check_launch("mesh_simplify_emit (vertex sums)")) return rc;
    hipLaunchKernelGGL(simplify_accumulate_faces_kernel, dim3(sum_blocks_of(nt)), dim3(kThreads), 0, s, verts, faces, g, ws, nv, nt);
    if (int rc = check_launch("mesh_simplify_emit (quadrics)")) return rc;
    hipLaunchKernelGGL(simplify_place_kernel, dim3(grid_of(nv)), dim3(kThreads), 0, s, verts, g, ws, nv, out_verts, src_vertex, vertex_map);
    if (int rc = check_launch("mesh_simplify_emit (positions)")) return rc;
    if (out_faces) {                                     // (null out_faces: the caller counted T' == 0, nothing to write)
        hipLaunchKernelGGL(simplify_emit_faces_kernel, dim3(blocks_of(nt)), dim3(kThreads), 0, s, faces, ws, nv, nt, out_faces);
        if (int rc = check_launch("mesh_simplify_emit (faces)")) return rc;
    }
    return GNERF_OK;
}
