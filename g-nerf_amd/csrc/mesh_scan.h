// What the scanned passes of the mesh units share (csrc/mesh_clean.hip, csrc/mesh_simplify.hip): a block owns kItems consecutive items, a block
// prefix on top of a scan of the block totals gives every kept item its place -- by index, never by arrival.  Included inside each unit's
// anonymous namespace.
#pragma once

constexpr int kThreads = 256;
constexpr int kChunks = 8;
constexpr int kItems = kThreads * kChunks;          // vertices or faces per block of the scanned passes
constexpr int kItemsLog2 = 11;
static_assert(kItems == 1 << kItemsLog2, "kItems must be a power of two");
constexpr int kScanThreads = 1024;

inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }
inline uint32_t blocks_of(uint32_t n) { return (n + uint32_t(kItems) - 1) >> kItemsLog2; }
inline uint32_t grid_of(uint32_t n) { return (n + uint32_t(kThreads) - 1) / uint32_t(kThreads); }

template <class T> inline T* take(char* p, size_t* off, size_t bytes) {
    T* r = reinterpret_cast<T*>(p + *off);
    *off += align256(bytes);
    return r;
}

// Block-exclusive prefix of x over this chunk of kThreads items, carried across chunks in *running (uniform).  wsum: LDS for the four wave
// totals, double-buffered by chunk parity so that one barrier per chunk suffices (csrc/mesh.hip's scheme, with a shuffle scan for any x).
__device__ __forceinline__ uint32_t block_prefix(uint32_t x, uint32_t (*wsum)[kThreads / 64], int parity, uint32_t* running) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) wsum[parity][wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) {
        const uint32_t s = wsum[parity][w];
        before += w < wave ? s : 0u;
        all += s;
    }
    const uint32_t r = *running + before + incl - x;
    *running += all;
    return r;
}

// One workgroup: exclusive offsets of two arrays of block counts (either may be empty), tile by tile with the carry in registers; the totals
// -> tot_a / tot_b (int64, either may be null).
__global__ __launch_bounds__(kScanThreads) void scan_blocks_kernel(const uint32_t* __restrict__ blk_a, uint32_t* __restrict__ off_a, uint32_t na,
                                                                   const uint32_t* __restrict__ blk_b, uint32_t* __restrict__ off_b, uint32_t nb,
                                                                   int64_t* __restrict__ tot_a, int64_t* __restrict__ tot_b) {
    __shared__ uint32_t sa[kScanThreads / 64], sb[kScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry_a = 0, carry_b = 0;
    const uint32_t n = na > nb ? na : nb;
    for (uint32_t head = 0; head < n; head += kScanThreads) {
        const uint32_t i = head + threadIdx.x;
        const uint32_t a0 = i < na ? blk_a[i] : 0u, b0 = i < nb ? blk_b[i] : 0u;
        uint32_t a = a0, b = b0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t xa = __shfl_up(a, o, 64), xb = __shfl_up(b, o, 64);
            if (lane >= o) { a += xa; b += xb; }
        }
        if (lane == 63) { sa[wave] = a; sb[wave] = b; }
        __syncthreads();
        uint32_t ba = 0, bb = 0, aa = 0, ab = 0;
        for (int w = 0; w < kScanThreads / 64; w++) {
            ba += w < wave ? sa[w] : 0u;
            bb += w < wave ? sb[w] : 0u;
            aa += sa[w];
            ab += sb[w];
        }
        if (i < na) off_a[i] = carry_a + ba + a - a0;
        if (i < nb) off_b[i] = carry_b + bb + b - b0;
        carry_a += aa;
        carry_b += ab;
        __syncthreads();                                 // sa / sb are rewritten by the next tile
    }
    if (threadIdx.x == 0) {
        if (tot_a) *tot_a = int64_t(carry_a);
        if (tot_b) *tot_b = int64_t(carry_b);
    }
}
