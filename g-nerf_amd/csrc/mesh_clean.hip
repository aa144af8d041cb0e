// Cleaning an extracted triangle mesh (what sits between csrc/mesh.hip and its consumers): connected components, compaction to the kept
// components, Taubin smoothing -- gnerf_mesh_workspace_bytes / _components / _compact_count / _compact_emit / _smooth of
// include/gnerf_hip.h, which states the rules; shape_mi355x.py's mesh_components_numpy / mesh_compact_numpy / mesh_smooth_numpy are the numpy
// ports these kernels match bit for bit.  Every face id is range-checked before it is used as an index: a face that names a vertex outside
// [0, V) joins nothing, is counted, is dropped by the compaction and ignored by the smoothing.
//
// components  a lock-free union-find over parent[] (workspace), six launches:
//     init     parent[v] = v, faces_of[v] = 0, the tallies = 0.
//     hook     one thread per face: unite(f0, f1), unite(f0, f2).  unite chases both ends to their roots and hooks the LARGER root under
//              the smaller with one 32-bit compare-and-swap at device scope; a failed swap goes on from the value it returned.  Every write to
//              parent[] lowers the stored value (parent[x] <= x), so every chase is strictly decreasing and ends on its own; no thread waits
//              for another (no flags, no spinning, no order between workgroups).  A chase's plain load may see an older, larger parent (its XCD's L2):
//              the chase then stops early on a vertex that is no longer a root, the swap fails and hands back the newer parent -- time, not
//              correctness.  After a chase of more than one step the start is pointed at the root it found with an atomic minimum (halves the
//              later chases; it lowers the value, as the invariant asks).
//     flatten  behind the hooking kernel: label[v] = the root of v, which by the rule above is the component's smallest index.
//     faces_of a block per kItems faces: equal labels of a wave are combined (ballot), a wave holds on to its current (label, count) pair
//              from round to round and the four waves' last pairs are merged in LDS, so a run of faces of one component costs one integer
//              add per block -- a head mesh sends almost every face to one address, and one word takes only ~88 atomics per microsecond.
//     tally    per vertex: roots with and without faces, one add per wave; with the hook kernel's bad-face count these are `counts`,
//     counts   which one last small launch copies out of the workspace.
//   Integer adds in any order: the same bits on every run and for every order of the faces.
// compaction  a vertex is kept iff keep[label] != 0 and its component has a face; a face iff its ids are in range and its first vertex is kept.
//     count    a block owns kItems consecutive vertices or faces and counts the kept ones.
//     scan     one workgroup: exclusive offsets of the block counts, totals -> counts.
//     emit     the flags again, a block prefix (wave scan + LDS) on top of the block's offset gives every kept item its place: order is by
//              index, never by arrival.  Vertices first (they write newid[]), then the faces, remapped through newid[].
// smoothing   the neighbour rows are built once per call: degrees by integer adds, row starts by the same block scan (block-local prefix +
//     block offset), rows filled through a returning add per vertex, then every row sorted ascending by its own thread (insertion sort for
//     short rows, heapsort beyond) and the pin flag read off the sorted row (some neighbour not exactly twice).  A half-step is then a pure
//     gather, one thread per vertex, no atomics, float64 sums in ascending-neighbour order, between ping-pong buffers.
// flip guard  (gnerf_mesh_flip_guard; port: mesh_flip_guard_numpy) behind a move of the vertices, such as the projection onto the level set
//     (csrc/project_level.inl): rounds of two launches, faces -> marks in status[] and one count per block, vertices -> marked ones set back.
#include "common.h"

#pragma clang fp contract(off)

namespace {

#include "mesh_scan.h"

constexpr int kInsertionMax = 32;                    // longest row the insertion sort takes
constexpr int64_t kMaxSmoothTris = (int64_t(1) << 32) / 6 - 1;      // 6 * T row entries are addressed with 32 bits

struct ComponentsWs {
    int32_t* parent;                                 // [V]
    unsigned long long* tally;                       // [3] components with a face, vertices in no face, faces out of range
};
struct CompactWs {
    int32_t* newid;                                  // [V]  new index of every kept vertex
    uint32_t *blk_v, *blk_t;                         // [nbv], [nbt] kept items per block
    uint32_t *off_v, *off_t;                         // exclusive block offsets
};
struct SmoothWs {
    uint32_t *deg, *local, *cursor;                  // [V] m_i; block-local exclusive prefix of m; fill cursor
    uint32_t *blk, *off;                             // [nbv] block totals of m and their exclusive offsets
    int32_t* adj;                                    // [6 T] the rows
    unsigned char* pin;                              // [V]
    float *buf0, *buf1;                              // [3 V] each
};

inline ComponentsWs carve_components(void* ws, uint32_t nv, size_t* total) {
    char* p = static_cast<char*>(ws);
    size_t off = 0;
    ComponentsWs w;
    w.parent = take<int32_t>(p, &off, size_t(nv) * 4);
    w.tally = take<unsigned long long>(p, &off, 3 * 8);
    if (total) *total = off;
    return w;
}

inline CompactWs carve_compact(void* ws, uint32_t nv, uint32_t nt, size_t* total) {
    char* p = static_cast<char*>(ws);
    size_t off = 0;
    CompactWs w;
    const uint32_t nbv = blocks_of(nv), nbt = blocks_of(nt);
    w.newid = take<int32_t>(p, &off, size_t(nv) * 4);
    w.blk_v = take<uint32_t>(p, &off, size_t(nbv) * 4);
    w.blk_t = take<uint32_t>(p, &off, size_t(nbt) * 4);
    w.off_v = take<uint32_t>(p, &off, size_t(nbv) * 4);
    w.off_t = take<uint32_t>(p, &off, size_t(nbt) * 4);
    if (total) *total = off;
    return w;
}

inline SmoothWs carve_smooth(void* ws, uint32_t nv, uint32_t nt, size_t* total) {
    char* p = static_cast<char*>(ws);
    size_t off = 0;
    SmoothWs w;
    const uint32_t nbv = blocks_of(nv);
    w.deg = take<uint32_t>(p, &off, size_t(nv) * 4);
    w.cursor = take<uint32_t>(p, &off, size_t(nv) * 4);          // (behind deg: the two are zeroed with one memset)
    w.local = take<uint32_t>(p, &off, size_t(nv) * 4);
    w.blk = take<uint32_t>(p, &off, size_t(nbv) * 4);
    w.off = take<uint32_t>(p, &off, size_t(nbv) * 4);
    w.adj = take<int32_t>(p, &off, size_t(nt) * 24);
    w.pin = take<unsigned char>(p, &off, size_t(nv));
    w.buf0 = take<float>(p, &off, size_t(nv) * 12);
    w.buf1 = take<float>(p, &off, size_t(nv) * 12);
    if (total) *total = off;
    return w;
}

// ---------------------------------------------------------------------------------------------------------------- shared device helpers
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
}

// the three ids of face t, and whether all of them name a vertex
__device__ __forceinline__ bool load_face(const int32_t* __restrict__ faces, uint32_t t, uint32_t nv, int32_t (&f)[3]) {
    f[0] = faces[size_t(t) * 3];
    f[1] = faces[size_t(t) * 3 + 1];
    f[2] = faces[size_t(t) * 3 + 2];
    return uint32_t(f[0]) < nv && uint32_t(f[1]) < nv && uint32_t(f[2]) < nv;
}

// ---------------------------------------------------------------------------------------------------------------- components
// A chase reads parent[] with the PLAIN load instruction (a relaxed load of the narrowest scope: no cache-control bits, but a load the
// compiler may neither tear nor assume unchanged).  It may return an older, larger parent out of this XCD's L2; the header comment says why
// that is safe, and unite() ends whatever the loads return: the larger of its two ends strictly decreases from round to round.  Measured on
// the two 512^3 meshes: the same chases with device-scope loads take the hooking kernel twice as long (0.9-1.1 ms against 0.47-0.53), and
// without the shortening below it takes 0.83-0.87 ms and leaves the flatten 60-140 us of chasing instead of 5.
__device__ __forceinline__ int32_t load_parent(const int32_t* parent, int32_t x) {
    return __hip_atomic_load(const_cast<int32_t*>(parent) + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// the root the chase from x ends on (strictly decreasing: parent[y] <= y)
__device__ __forceinline__ int32_t chase(const int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t p = load_parent(parent, x);
        if (p == x) return x;
        x = p;
    }
}

__device__ __forceinline__ int32_t chase_and_shorten(int32_t* parent, int32_t x) {
    const int32_t p = load_parent(parent, x);
    if (p == x) return x;
    const int32_t r = chase(parent, p);
    if (r != p) __hip_atomic_fetch_min(parent + x, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // r < p: lowers parent[x]
    return r;
}

__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b) {
    a = chase_and_shorten(parent, a);
    b = chase_and_shorten(parent, b);
    while (a != b) {
        if (a < b) { const int32_t t = a; a = b; b = t; }                     // a: the larger root, hooked under b
        int32_t seen = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        a = chase(parent, seen);                                             // a was no root any more: on from what it points at (< a)
        b = chase(parent, b);
    }
}

__global__ __launch_bounds__(kThreads) void components_init_kernel(ComponentsWs ws, int32_t* __restrict__ faces_of, uint32_t nv) {
    const uint32_t v = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (v < nv) {
        ws.parent[v] = int32_t(v);
        faces_of[v] = 0;
    }
    if (v < 3) ws.tally[v] = 0ull;
}

__global__ __launch_bounds__(kThreads) void components_hook_kernel(const int32_t* __restrict__ faces, ComponentsWs ws, uint32_t nv, uint32_t nt) {
    const uint32_t t = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    bool bad = false;
    if (t < nt) {
        int32_t f[3];
        if (load_face(faces, t, nv, f)) {
            if (f[1] != f[0]) unite(ws.parent, f[0], f[1]);
            if (f[2] != f[0]) unite(ws.parent, f[0], f[2]);
        } else {
            bad = true;
        }
    }
    const uint64_t m = __ballot(bad);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(ws.tally + 2, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kThreads) void components_flatten_kernel(ComponentsWs ws, int32_t* __restrict__ label, uint32_t nv) {
    const uint32_t v = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (v < nv) label[v] = chase(ws.parent, int32_t(v));
}

__global__ __launch_bounds__(kThreads) void components_faces_of_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ label,
                                                                       int32_t* __restrict__ faces_of, uint32_t nv, uint32_t nt) {
    // A block owns kItems consecutive faces.  Each wave carries one (label, count) pair in registers (wave-uniform): a round's label joins it
    // when equal and pushes it out to memory otherwise, so a run of faces of one component costs one add, however long; the four waves' last
    // pairs meet in LDS, where equal labels are merged once more.
    __shared__ int32_t s_label[kThreads / 64], s_count[kThreads / 64];
    int32_t held = -1, held_n = 0;
    const uint32_t first = blockIdx.x * uint32_t(kItems);
    for (int j = 0; j < kChunks; j++) {
        const uint32_t t = first + uint32_t(j * kThreads) + threadIdx.x;
        int32_t l = -1;
        if (t < nt) {
            int32_t f[3];
            if (load_face(faces, t, nv, f)) l = label[f[0]];
        }
        bool todo = l >= 0;
        for (uint64_t live = __ballot(todo); live; live = __ballot(todo)) {    // one round per distinct label of the wave
            const int32_t lead = __shfl(l, __ffsll((unsigned long long)live) - 1, 64);
            const uint64_t same = __ballot(todo && l == lead);
            if (lead != held) {
                if (held_n && (threadIdx.x & 63) == 0) atomicAdd(faces_of + held, held_n);
                held = lead;
                held_n = 0;
            }
            held_n += int32_t(__popcll(same));
            todo = todo && l != lead;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        s_label[threadIdx.x >> 6] = held;
        s_count[threadIdx.x >> 6] = held_n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 0; w < kThreads / 64; w++) {
            int32_t n = s_count[w];
            if (n == 0) continue;
            for (int u = w + 1; u < kThreads / 64; u++) {
                if (s_label[u] == s_label[w]) {
                    n += s_count[u];
                    s_count[u] = 0;
                }
            }
            atomicAdd(faces_of + s_label[w], n);
        }
    }
}

__global__ __launch_bounds__(kThreads) void components_tally_kernel(ComponentsWs ws, const int32_t* __restrict__ label,
                                                                    const int32_t* __restrict__ faces_of, uint32_t nv) {
    const uint32_t v = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    const bool root = v < nv && label[v] == int32_t(v);
    const bool with = root && faces_of[v] > 0;
    const uint64_t mw = __ballot(with), mo = __ballot(root && !with);
    if ((threadIdx.x & 63) == 0) {
        if (mw) atomicAdd(ws.tally + 0, (unsigned long long)__popcll(mw));
        if (mo) atomicAdd(ws.tally + 1, (unsigned long long)__popcll(mo));
    }
}

__global__ void components_counts_kernel(ComponentsWs ws, int64_t* __restrict__ counts) {
    if (threadIdx.x < 3) counts[threadIdx.x] = int64_t(ws.tally[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------------- compaction
struct Keep {
    const int32_t* label;
    const int32_t* faces_of;
    const unsigned char* keep;
    uint32_t nv;
};

__device__ __forceinline__ bool vertex_kept(const Keep& k, uint32_t v) {
    const int32_t l = k.label[v];
    return uint32_t(l) < k.nv && k.keep[l] != 0 && k.faces_of[l] > 0;
}

__device__ __forceinline__ bool face_kept(const Keep& k, const int32_t* __restrict__ faces, uint32_t t, int32_t (&f)[3]) {
    return load_face(faces, t, k.nv, f) && vertex_kept(k, uint32_t(f[0]));
}

// blocks [0, nbv) count vertices, blocks [nbv, nbv + nbt) faces
__global__ __launch_bounds__(kThreads) void compact_count_kernel(const int32_t* __restrict__ faces, Keep k, uint32_t nt, uint32_t nbv, CompactWs ws) {
    __shared__ uint32_t wsum[kThreads / 64];
    const bool is_face = blockIdx.x >= nbv;
    const uint32_t blk = is_face ? blockIdx.x - nbv : blockIdx.x;
    const uint32_t first = blk * uint32_t(kItems), n = is_face ? nt : k.nv;
    uint32_t mine = 0;
    for (int j = 0; j < kChunks; j++) {
        const uint32_t i = first + uint32_t(j * kThreads) + threadIdx.x;
        bool kept = false;
        if (i < n) {
            int32_t f[3];
            kept = is_face ? face_kept(k, faces, i, f) : vertex_kept(k, i);
        }
        mine += uint32_t(__popcll(__ballot(kept)));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kThreads / 64; w++) s += wsum[w];
        (is_face ? ws.blk_t : ws.blk_v)[blk] = s;
    }
}

__global__ __launch_bounds__(kThreads) void compact_emit_verts_kernel(const float* __restrict__ verts, Keep k, CompactWs ws, float* __restrict__ out_verts,
                                                                      int32_t* __restrict__ src_vertex) {
    __shared__ uint32_t wsum[2][kThreads / 64];
    uint32_t running = ws.off_v[blockIdx.x];
    const uint32_t first = blockIdx.x * uint32_t(kItems);
    for (int j = 0; j < kChunks; j++) {
        const uint32_t v = first + uint32_t(j * kThreads) + threadIdx.x;
        const bool kept = v < k.nv && vertex_kept(k, v);
        const uint32_t id = block_prefix(kept ? 1u : 0u, wsum, j & 1, &running);
        if (kept) {
            out_verts[size_t(id) * 3] = verts[size_t(v) * 3];
            out_verts[size_t(id) * 3 + 1] = verts[size_t(v) * 3 + 1];
            out_verts[size_t(id) * 3 + 2] = verts[size_t(v) * 3 + 2];
            src_vertex[id] = int32_t(v);
            ws.newid[v] = int32_t(id);
        }
    }
}

__global__ __launch_bounds__(kThreads) void compact_emit_faces_kernel(const int32_t* __restrict__ faces, Keep k, uint32_t nt, CompactWs ws,
                                                                      int32_t* __restrict__ out_faces) {
    __shared__ uint32_t wsum[2][kThreads / 64];
    uint32_t running = ws.off_t[blockIdx.x];
    const uint32_t first = blockIdx.x * uint32_t(kItems);
    for (int j = 0; j < kChunks; j++) {
        const uint32_t t = first + uint32_t(j * kThreads) + threadIdx.x;
        int32_t f[3] = {0, 0, 0};
        const bool kept = t < nt && face_kept(k, faces, t, f);
        const uint32_t id = block_prefix(kept ? 1u : 0u, wsum, j & 1, &running);
        if (kept) {                                        // the three vertices share f[0]'s label: all kept, all with a newid
            out_faces[size_t(id) * 3] = ws.newid[f[0]];
            out_faces[size_t(id) * 3 + 1] = ws.newid[f[1]];
            out_faces[size_t(id) * 3 + 2] = ws.newid[f[2]];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- smoothing
__device__ __forceinline__ uint32_t row_start(const SmoothWs& ws, uint32_t v) { return ws.off[v >> kItemsLog2] + ws.local[v]; }

__global__ __launch_bounds__(kThreads) void smooth_degree_kernel(const int32_t* __restrict__ faces, SmoothWs ws, uint32_t nv, uint32_t nt) {
    const uint32_t t = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (t >= nt) return;
    int32_t f[3];
    if (!load_face(faces, t, nv, f)) return;
#pragma unroll
    for (int c = 0; c < 3; c++) atomicAdd(ws.deg + f[c], 2u);
}

__global__ __launch_bounds__(kThreads) void smooth_local_kernel(SmoothWs ws, uint32_t nv) {
    __shared__ uint32_t wsum[2][kThreads / 64];
    uint32_t running = 0;
    const uint32_t first = blockIdx.x * uint32_t(kItems);
    for (int j = 0; j < kChunks; j++) {
        const uint32_t v = first + uint32_t(j * kThreads) + threadIdx.x;
        const uint32_t pre = block_prefix(v < nv ? ws.deg[v] : 0u, wsum, j & 1, &running);
        if (v < nv) ws.local[v] = pre;
    }
    if (threadIdx.x == 0) ws.blk[blockIdx.x] = running;
}

// corner c of a face gives vertex f[c] the face's two other ids, f[c + 1] and f[c + 2] (cyclically)
__global__ __launch_bounds__(kThreads) void smooth_fill_kernel(const int32_t* __restrict__ faces, SmoothWs ws, uint32_t nv, uint32_t nt) {
    const uint32_t t = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (t >= nt) return;
    int32_t f[3];
    if (!load_face(faces, t, nv, f)) return;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint32_t v = uint32_t(f[c]);
        const uint32_t slot = atomicAdd(ws.cursor + v, 2u);
        int32_t* row = ws.adj + size_t(row_start(ws, v)) + slot;
        row[0] = f[(c + 1) % 3];
        row[1] = f[(c + 2) % 3];
    }
}

__device__ __forceinline__ void sift_down(int32_t* a, uint32_t root, uint32_t end) {           // max-heap on a[0 .. end)
    const int32_t x = a[root];
    for (;;) {
        uint32_t child = 2 * root + 1;
        if (child >= end) break;
        if (child + 1 < end && a[child + 1] > a[child]) child++;
        if (a[child] <= x) break;
        a[root] = a[child];
        root = child;
    }
    a[root] = x;
}

__global__ __launch_bounds__(kThreads) void smooth_sort_kernel(SmoothWs ws, uint32_t nv, int pin_boundary) {
    const uint32_t v = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (v >= nv) return;
    const uint32_t m = ws.deg[v];
    int32_t* a = ws.adj + size_t(row_start(ws, v));
    if (m <= uint32_t(kInsertionMax)) {
        for (uint32_t i = 1; i < m; i++) {
            const int32_t x = a[i];
            uint32_t j = i;
            for (; j > 0 && a[j - 1] > x; j--) a[j] = a[j - 1];
            a[j] = x;
        }
    } else {
        for (uint32_t i = m / 2; i-- > 0;) sift_down(a, i, m);
        for (uint32_t end = m - 1; end > 0; end--) {
            const int32_t top = a[0];
            a[0] = a[end];
            a[end] = top;
            sift_down(a, 0, end);
        }
    }
    bool pinned = m == 0;                                // (a vertex in no face never moves)
    if (pin_boundary) {
        for (uint32_t i = 0; i < m;) {                   // runs of equal neighbours: every one must have length two
            uint32_t j = i + 1;
            while (j < m && a[j] == a[i]) j++;
            pinned |= j - i != 2;
            i = j;
        }
    }
    ws.pin[v] = pinned ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void smooth_step_kernel(const float* __restrict__ src, float* __restrict__ dst, SmoothWs ws, uint32_t nv, float s) {
    const uint32_t v = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (v >= nv) return;
    const float x0 = src[size_t(v) * 3], x1 = src[size_t(v) * 3 + 1], x2 = src[size_t(v) * 3 + 2];
    float y0 = x0, y1 = x1, y2 = x2;
    if (!ws.pin[v]) {
        const uint32_t m = ws.deg[v];
        const int32_t* __restrict__ a = ws.adj + size_t(row_start(ws, v));
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (uint32_t i = 0; i < m; i++) {
            const size_t j = size_t(uint32_t(a[i])) * 3;
            s0 += double(src[j]);
            s1 += double(src[j + 1]);
            s2 += double(src[j + 2]);
        }
        const double md = double(m), sd = double(s);
        const double c0 = s0 / md, c1 = s1 / md, c2 = s2 / md;
        y0 = float(double(x0) + sd * (c0 - double(x0)));
        y1 = float(double(x1) + sd * (c1 - double(x1)));
        y2 = float(double(x2) + sd * (c2 - double(x2)));
    }
    dst[size_t(v) * 3] = y0;
    dst[size_t(v) * 3 + 1] = y1;
    dst[size_t(v) * 3 + 2] = y2;
}

// ---------------------------------------------------------------------------------------------------------------- flip guard
// (include/gnerf_hip.h, gnerf_mesh_flip_guard, states the rules.)  The marks live in status[] itself: 3 = reverted.  A round is two launches,
// one over the faces (reads positions, writes status and one count per block) and one over the vertices (reads status, writes positions), so
// neither kernel reads what it writes.  `prev` is the count of the round before (null for the first): zero there means nothing moved since
// that round looked, and the whole launch leaves -- a device-side read, the launch sequence is the same whatever the data.
struct D3 { double x, y, z; };

__device__ __forceinline__ D3 face_normal(const float* __restrict__ v, const int32_t (&f)[3]) {
    const double ax = double(v[size_t(f[0]) * 3]), ay = double(v[size_t(f[0]) * 3 + 1]), az = double(v[size_t(f[0]) * 3 + 2]);
    const double e1x = double(v[size_t(f[1]) * 3]) - ax, e1y = double(v[size_t(f[1]) * 3 + 1]) - ay, e1z = double(v[size_t(f[1]) * 3 + 2]) - az;
    const double e2x = double(v[size_t(f[2]) * 3]) - ax, e2y = double(v[size_t(f[2]) * 3 + 1]) - ay, e2z = double(v[size_t(f[2]) * 3 + 2]) - az;
    return D3{e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x};
}

__device__ __forceinline__ double dot3(const D3& a, const D3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

template <bool MARK>
__global__ __launch_bounds__(kThreads) void flip_faces_kernel(const float* __restrict__ verts_in, const float* __restrict__ cur,
                                                              const int32_t* __restrict__ faces, uint32_t nv, uint32_t nt,
                                                              unsigned char* status, const int32_t* prev, int32_t* count) {
    __shared__ uint32_t s_n[kThreads / 64];
    if (prev && *prev == 0) return;
    uint32_t n = 0;                                      // wave-uniform: flipped faces this wave has seen
    const uint32_t first = blockIdx.x * uint32_t(kItems);
    for (int j = 0; j < kChunks; j++) {
        const uint32_t t = first + uint32_t(j * kThreads) + threadIdx.x;
        bool flipped = false;
        int32_t f[3];
        if (t < nt && load_face(faces, t, nv, f)) {
            const D3 n0 = face_normal(verts_in, f), n1 = face_normal(cur, f);
            flipped = dot3(n0, n1) < 0.0 || (dot3(n1, n1) == 0.0 && dot3(n0, n0) > 0.0);
            if (MARK && flipped) status[f[0]] = status[f[1]] = status[f[2]] = 3;
        }
        n += uint32_t(__popcll(__ballot(flipped)));
    }
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (int w = 0; w < kThreads / 64; w++) all += s_n[w];
        if (all) atomicAdd(count, int32_t(all));         // one add per block
    }
}

__global__ __launch_bounds__(kThreads) void flip_revert_kernel(const float* __restrict__ verts_in, float* __restrict__ cur,
                                                               const unsigned char* __restrict__ status, uint32_t nv, const int32_t* count) {
    if (*count == 0) return;                             // this round marked nothing
    const uint32_t v = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
    if (v < nv && status[v] == 3) {
        cur[size_t(v) * 3] = verts_in[size_t(v) * 3];
        cur[size_t(v) * 3 + 1] = verts_in[size_t(v) * 3 + 1];
        cur[size_t(v) * 3 + 2] = verts_in[size_t(v) * 3 + 2];
    }
}

int check_sizes(int n_verts, int n_tris, const char* what) {
    using namespace gnerf;
    if (n_verts < 0 || n_tris < 0) return fail(GNERF_E_ARG, "%s: negative size (%d vertices, %d faces)", what, n_verts, n_tris);
    return GNERF_OK;
}

}  // namespace

extern "C" int gnerf_mesh_workspace_bytes(int n_verts, int n_tris, size_t* bytes) {
    using namespace gnerf;
    if (!bytes) return fail(GNERF_E_ARG, "mesh_workspace_bytes: null pointer");
    if (int rc = check_sizes(n_verts, n_tris, "mesh_workspace_bytes")) return rc;
    size_t a = 0, b = 0, c = 0;
    carve_components(nullptr, uint32_t(n_verts), &a);
    carve_compact(nullptr, uint32_t(n_verts), uint32_t(n_tris), &b);
    carve_smooth(nullptr, uint32_t(n_verts), uint32_t(n_tris), &c);
    const size_t most = a > b ? (a > c ? a : c) : (b > c ? b : c);
    *bytes = most > 256 ? most : 256;
    return GNERF_OK;
}

extern "C" int gnerf_mesh_components(const int32_t* faces, int n_verts, int n_tris, void* workspace, int32_t* label, int32_t* faces_of,
                                     int64_t* counts, gnerf_stream_t stream) {
    using namespace gnerf;
    if (int rc = check_sizes(n_verts, n_tris, "mesh_components")) return rc;
    if (!workspace || !counts || (n_tris && !faces) || (n_verts && (!label || !faces_of))) return fail(GNERF_E_ARG, "mesh_components: null pointer");
    const uint32_t nv = uint32_t(n_verts), nt = uint32_t(n_tris);
    const ComponentsWs ws = carve_components(workspace, nv, nullptr);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(components_init_kernel, dim3(nv ? grid_of(nv) : 1), dim3(kThreads), 0, s, ws, faces_of, nv);
    if (int rc = check_launch("mesh_components (init)")) return rc;
    if (nt) {
        hipLaunchKernelGGL(components_hook_kernel, dim3(grid_of(nt)), dim3(kThreads), 0, s, faces, ws, nv, nt);
        if (int rc = check_launch("mesh_components (hook)")) return rc;
    }
    if (nv) {
        hipLaunchKernelGGL(components_flatten_kernel, dim3(grid_of(nv)), dim3(kThreads), 0, s, ws, label, nv);
        if (int rc = check_launch("mesh_components (flatten)")) return rc;
        if (nt) {
            hipLaunchKernelGGL(components_faces_of_kernel, dim3(blocks_of(nt)), dim3(kThreads), 0, s, faces, label, faces_of, nv, nt);
            if (int rc = check_launch("mesh_components (faces_of)")) return rc;
        }
        hipLaunchKernelGGL(components_tally_kernel, dim3(grid_of(nv)), dim3(kThreads), 0, s, ws, label, faces_of, nv);
        if (int rc = check_launch("mesh_components (tally)")) return rc;
    }
    hipLaunchKernelGGL(components_counts_kernel, dim3(1), dim3(64), 0, s, ws, counts);
    return check_launch("mesh_components (counts)");
}

extern "C" int gnerf_mesh_compact_count(const int32_t* faces, int n_verts, int n_tris, const int32_t* label, const int32_t* faces_of,
                                        const unsigned char* keep, void* workspace, int64_t* counts, gnerf_stream_t stream) {
    using namespace gnerf;
    if (int rc = check_sizes(n_verts, n_tris, "mesh_compact_count")) return rc;
    if (!workspace || !counts || (n_tris && !faces) || (n_verts && (!label || !faces_of || !keep)))
        return fail(GNERF_E_ARG, "mesh_compact_count: null pointer");
    const uint32_t nv = uint32_t(n_verts), nt = uint32_t(n_tris), nbv = blocks_of(nv), nbt = blocks_of(nt);
    const CompactWs ws = carve_compact(workspace, nv, nt, nullptr);
    const Keep k = {label, faces_of, keep, nv};
    hipStream_t s = as_stream(stream);
    if (nbv + nbt) {
        hipLaunchKernelGGL(compact_count_kernel, dim3(nbv + nbt), dim3(kThreads), 0, s, faces, k, nt, nbv, ws);
        if (int rc = check_launch("mesh_compact_count")) return rc;
    }
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kScanThreads), 0, s, ws.blk_v, ws.off_v, nbv, ws.blk_t, ws.off_t, nbt, counts, counts + 1);
    return check_launch("mesh_compact_count (scan)");
}

extern "C" int gnerf_mesh_compact_emit(const float* verts, const int32_t* faces, int n_verts, int n_tris, const int32_t* label,
                                       const int32_t* faces_of, const unsigned char* keep, void* workspace, float* out_verts, int32_t* out_faces,
                                       int32_t* src_vertex, gnerf_stream_t stream) {
    using namespace gnerf;
    if (int rc = check_sizes(n_verts, n_tris, "mesh_compact_emit")) return rc;
    if (!workspace || (n_tris && !faces) || (n_verts && (!verts || !label || !faces_of || !keep || !out_verts || !src_vertex)))
        return fail(GNERF_E_ARG, "mesh_compact_emit: null pointer");
    const uint32_t nv = uint32_t(n_verts), nt = uint32_t(n_tris), nbv = blocks_of(nv), nbt = blocks_of(nt);
    const CompactWs ws = carve_compact(workspace, nv, nt, nullptr);
    const Keep k = {label, faces_of, keep, nv};
    hipStream_t s = as_stream(stream);
    if (nbv) {
        hipLaunchKernelGGL(compact_emit_verts_kernel, dim3(nbv), dim3(kThreads), 0, s, verts, k, ws, out_verts, src_vertex);
        if (int rc = check_launch("mesh_compact_emit (vertices)")) return rc;
    }
    if (nbt && nbv && out_faces) {                       // (null out_faces: the caller counted T' == 0, nothing to write)
        hipLaunchKernelGGL(compact_emit_faces_kernel, dim3(nbt), dim3(kThreads), 0, s, faces, k, nt, ws, out_faces);
        if (int rc = check_launch("mesh_compact_emit (faces)")) return rc;
    }
    return GNERF_OK;
}

extern "C" int gnerf_mesh_smooth(const float* verts, int n_verts, const int32_t* faces, int n_tris, int iterations, float lam, float mu,
                                 int pin_boundary, void* workspace, float* out, gnerf_stream_t stream) {
    using namespace gnerf;
    if (int rc = check_sizes(n_verts, n_tris, "mesh_smooth")) return rc;
    if (iterations < 0) return fail(GNERF_E_ARG, "mesh_smooth: iterations must be >= 0 (got %d)", iterations);
    if (!workspace || (n_tris && !faces) || (n_verts && (!verts || !out))) return fail(GNERF_E_ARG, "mesh_smooth: null pointer");
    if (int64_t(n_tris) > kMaxSmoothTris) return fail(GNERF_E_ARG, "mesh_smooth: more than %lld faces (the rows are addressed with 32 bits)", (long long)kMaxSmoothTris);
    const uint32_t nv = uint32_t(n_verts), nt = uint32_t(n_tris), nbv = blocks_of(nv);
    hipStream_t s = as_stream(stream);
    if (nv == 0) return GNERF_OK;
    if (iterations == 0) {
        if (out != verts && hipMemcpyAsync(out, verts, size_t(nv) * 12, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(GNERF_E_LAUNCH, "mesh_smooth: copy failed");
        return GNERF_OK;
    }
    const SmoothWs ws = carve_smooth(workspace, nv, nt, nullptr);
    // deg and cursor are adjacent: one memset zeroes both
    if (hipMemsetAsync(ws.deg, 0, size_t(reinterpret_cast<char*>(ws.local) - reinterpret_cast<char*>(ws.deg)), s) != hipSuccess)
        return fail(GNERF_E_LAUNCH, "mesh_smooth: memset failed");
    if (nt) {
        hipLaunchKernelGGL(smooth_degree_kernel, dim3(grid_of(nt)), dim3(kThreads), 0, s, faces, ws, nv, nt);
        if (int rc = check_launch("mesh_smooth (degree)")) return rc;
    }
    hipLaunchKernelGGL(smooth_local_kernel, dim3(nbv), dim3(kThreads), 0, s, ws, nv);
    if (int rc = check_launch("mesh_smooth (row prefix)")) return rc;
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kScanThreads), 0, s, ws.blk, ws.off, nbv, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u,
                       (int64_t*)nullptr, (int64_t*)nullptr);
    if (int rc = check_launch("mesh_smooth (row scan)")) return rc;
    if (nt) {
        hipLaunchKernelGGL(smooth_fill_kernel, dim3(grid_of(nt)), dim3(kThreads), 0, s, faces, ws, nv, nt);
        if (int rc = check_launch("mesh_smooth (fill)")) return rc;
    }
    hipLaunchKernelGGL(smooth_sort_kernel, dim3(grid_of(nv)), dim3(kThreads), 0, s, ws, nv, pin_boundary ? 1 : 0);
    if (int rc = check_launch("mesh_smooth (sort)")) return rc;
    const int steps = 2 * iterations;                    // half-step k reads what k - 1 wrote; the first reads verts, the last writes out
    const float* src = verts;
    for (int k = 0; k < steps; k++) {
        float* dst = k == steps - 1 ? out : ((k & 1) ? ws.buf1 : ws.buf0);
        hipLaunchKernelGGL(smooth_step_kernel, dim3(grid_of(nv)), dim3(kThreads), 0, s, src, dst, ws, nv, (k & 1) ? mu : lam);
        if (int rc = check_launch("mesh_smooth (step)")) return rc;
        src = dst;
    }
    return GNERF_OK;
}

extern "C" int gnerf_mesh_flip_guard(const float* verts_in, const float* verts_moved, const int32_t* faces, int n_verts, int n_tris, int max_rounds,
                                     float* verts_out, unsigned char* status, int32_t* counts, gnerf_stream_t stream) {
    using namespace gnerf;
    if (int rc = check_sizes(n_verts, n_tris, "mesh_flip_guard")) return rc;
    if (max_rounds < 1) return fail(GNERF_E_ARG, "mesh_flip_guard: max_rounds must be >= 1 (got %d)", max_rounds);
    if (!counts || (n_tris && !faces) || (n_verts && (!verts_in || !verts_moved || !verts_out || !status)))
        return fail(GNERF_E_ARG, "mesh_flip_guard: null pointer");
    if (n_verts && verts_out == verts_in) return fail(GNERF_E_ARG, "mesh_flip_guard: verts_out must not be verts_in");
    const uint32_t nv = uint32_t(n_verts), nt = uint32_t(n_tris);
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(counts, 0, size_t(max_rounds + 1) * 4, s) != hipSuccess) return fail(GNERF_E_LAUNCH, "mesh_flip_guard: memset failed");
    if (nv && verts_out != verts_moved && hipMemcpyAsync(verts_out, verts_moved, size_t(nv) * 12, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(GNERF_E_LAUNCH, "mesh_flip_guard: copy failed");
    if (nv == 0 || nt == 0) return GNERF_OK;
    for (int j = 0; j < max_rounds; j++) {
        hipLaunchKernelGGL(flip_faces_kernel<true>, dim3(blocks_of(nt)), dim3(kThreads), 0, s, verts_in, (const float*)verts_out, faces, nv, nt, status,
                           (const int32_t*)(j ? counts + j - 1 : nullptr), counts + j);
        if (int rc = check_launch("mesh_flip_guard (faces)")) return rc;
        hipLaunchKernelGGL(flip_revert_kernel, dim3(grid_of(nv)), dim3(kThreads), 0, s, verts_in, verts_out, (const unsigned char*)status, nv,
                           (const int32_t*)(counts + j));
        if (int rc = check_launch("mesh_flip_guard (revert)")) return rc;
    }
    hipLaunchKernelGGL(flip_faces_kernel<false>, dim3(blocks_of(nt)), dim3(kThreads), 0, s, verts_in, (const float*)verts_out, faces, nv, nt, status,
                       (const int32_t*)(counts + max_rounds - 1), counts + max_rounds);
    return check_launch("mesh_flip_guard (check)");
}
