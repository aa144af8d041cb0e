// Triangle rasteriser for the meshes csrc/mesh.hip extracts: gnerf_raster_workspace_bytes / _visibility / _resolve of include/gnerf_hip.h,
// whose header paragraph states every rule (vertex stage, dropped triangles, top-left fill rule on 1/256-pixel integers, perspective-correct
// depth, the 64-bit visibility key).  shape_mi355x.rasterize_numpy / resolve_numpy restate the arithmetic and give the same bits.
//
// The workload is marching cubes at 512^3 drawn at 64^2 - 512^2: triangles mostly smaller than a pixel.  So there are no tiles and no bins:
//   init     the visibility buffer to all ones, the four counts and the queue length to zero (the call needs no prepared memory);
//   small    one thread per (view, triangle): the three vertices are transformed and snapped (recomputed per triangle: 3 x 12 flops against
//            an atomic per covered pixel), the triangle is dropped and counted, or walks its clipped bounding box when that holds at most
//            GNERF_RASTER_SMALL_PIXELS pixel centres, or appends itself to the queue in the workspace (one returning atomicAdd per wave);
//   large    a fixed grid; every wave reads the queue length from device memory and takes queued triangles in turn, lanes across the pixels
//            of the bounding box;
//   resolve  one thread per pixel: the winning triangle is set up again (the same bits), its barycentrics recomputed, and depth / normal /
//            shaded colour written.
// A covered pixel merges key = float_as_uint(z) << 32 | triangle with a 64-bit atomicMin (a plain load in front filters what cannot win; a
// stale value costs an atomic, never a result).  The minimum does not depend on arrival order: the same bits on every run.
// No host read, no allocation, no synchronisation: the whole call is capturable.  Nothing here is contracted into a fused multiply-add.
//
// Below resolve: the colour bake, gnerf_mesh_bake_colors -- the inverse operation, frames back onto the vertices through the same vertex
// stage and the visibility buffers made above (one thread per vertex, gather-only; shape_mi355x.bake_colors_numpy: the same bits).
// Below that: the texture bake, gnerf_mesh_bake_texture -- the same stage function per texel of the atlas the header lays out -- and the
// textured resolve, gnerf_raster_resolve_textured (shape_mi355x.bake_texture_numpy / resolve_textured_numpy: the same bits).
#include "common.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kLargeBlocks = 1024;                   // x 4 waves: queued triangles are dealt to 4096 waves in turn
constexpr int kSmall = GNERF_RASTER_SMALL_PIXELS;
constexpr float kGuard = 2097152.0f;                 // 2^21 snapped units = 8192 pixels

// One rounding per operation: these are compiled under the pragma above, so none of them carries a licence to contract (the runtime
// header's __fmul_rn / __fadd_rn are compiled under the default mode and, once inlined, may fuse into a multiply-add).
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }           // correctly rounded (the compiler's default for HIP)

typedef unsigned long long u64;
constexpr u64 kEmpty = ~u64(0);

struct Workspace {
    uint32_t* qcount;                                // [1] (on a 256-byte line of its own)
    int32_t* queue;                                  // [n_views * n_tris] global triangle ids view * n_tris + t
};

inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

inline Workspace carve(void* ws, int64_t total, size_t* bytes) {
    char* p = static_cast<char*>(ws);
    Workspace w;
    w.qcount = reinterpret_cast<uint32_t*>(p);
    w.queue = reinterpret_cast<int32_t*>(p + 256);
    if (bytes) *bytes = 256 + align256(size_t(total > 0 ? total : 1) * 4);
    return w;
}

struct Camera {
    float A[12];                                     // mesh frame -> camera frame, rows of a 3x4
    float fx, sk, cx, fy, cy;
    float wf, hf;
};

__device__ __forceinline__ Camera load_camera(const float* __restrict__ mesh2cam, const float* __restrict__ intrinsics, int view, int h, int w) {
    Camera c;
#pragma unroll
    for (int i = 0; i < 12; i++) c.A[i] = mesh2cam[int64_t(view) * 12 + i];
    const float* K = intrinsics + int64_t(view) * 9;
    c.fx = K[0]; c.sk = K[1]; c.cx = K[2]; c.fy = K[4]; c.cy = K[5];
    c.wf = float(w); c.hf = float(h);
    return c;
}

// The first half of the vertex stage, which the rasteriser and the colour bake share: camera-frame position, 1/z and the normalised image
// coordinates (xc, yc); ok = finite and in front of near (the rest is only set then).
struct Point {
    float p[3], iz, xc, yc;
    bool ok;
};

__device__ __forceinline__ Point to_image(const Camera& c, const float* __restrict__ v, float near_z) {
    Point o;
    const float x = v[0], y = v[1], z = v[2];
#pragma unroll
    for (int r = 0; r < 3; r++)
        o.p[r] = add_rn(add_rn(add_rn(mul_rn(c.A[r * 4 + 0], x), mul_rn(c.A[r * 4 + 1], y)), mul_rn(c.A[r * 4 + 2], z)), c.A[r * 4 + 3]);
    o.iz = 0.f; o.xc = 0.f; o.yc = 0.f;
    const bool finite = __builtin_isfinite(o.p[0]) && __builtin_isfinite(o.p[1]) && __builtin_isfinite(o.p[2]);
    o.ok = finite && o.p[2] > near_z;
    if (!o.ok) return o;
    o.iz = div_rn(1.0f, o.p[2]);
    const float xn = mul_rn(o.p[0], o.iz), yn = mul_rn(o.p[1], o.iz);
    o.xc = add_rn(add_rn(mul_rn(c.fx, xn), mul_rn(c.sk, yn)), c.cx);
    o.yc = add_rn(mul_rn(c.fy, yn), c.cy);
    return o;
}

// One vertex: camera-frame position, 1/z, snapped pixel coordinates; bad = 1 (behind near / non-finite), 2 (past the guard band), else 0.
struct Vtx {
    float p[3], iz;
    int X, Y, bad;
};

__device__ __forceinline__ Vtx project(const Camera& c, const float* __restrict__ v, float near_z) {
    const Point q = to_image(c, v, near_z);
    Vtx o;
    o.p[0] = q.p[0]; o.p[1] = q.p[1]; o.p[2] = q.p[2];
    o.iz = 0.f; o.X = 0; o.Y = 0; o.bad = 1;
    if (!q.ok) return o;
    o.iz = q.iz;
    const float fX = rintf(mul_rn(mul_rn(q.xc, c.wf), 256.0f));
    const float fY = rintf(mul_rn(mul_rn(q.yc, c.hf), 256.0f));
    o.bad = 2;
    if (!(fabsf(fX) <= kGuard) || !(fabsf(fY) <= kGuard)) return o;
    o.X = int(fX); o.Y = int(fY); o.bad = 0;
    return o;
}

// A triangle ready to be drawn: vertices (a, b, c) = (0, 1, 2), or (0, 2, 1) when the snapped area is negative, so that area > 0.
struct Tri {
    int ax, ay, bx, by, cx, cy;
    float iza, izb, izc;
    int64_t area;
    int status;                                      // 0 drawn, 1 near, 2 guard, 3 culled (the order of counts[])
    bool flipped;
    int c0, r0, bw, bh;                              // clipped bounding box in pixels (bw * bh == 0: no centre inside)
};

__device__ __forceinline__ Tri setup(const Vtx& v0, const Vtx& v1, const Vtx& v2, int cull, int h, int w) {
    Tri t = {};
    if (v0.bad == 1 || v1.bad == 1 || v2.bad == 1) { t.status = 1; return t; }
    if (v0.bad | v1.bad | v2.bad) { t.status = 2; return t; }
    const int64_t area = int64_t(v1.X - v0.X) * int64_t(v2.Y - v0.Y) - int64_t(v2.X - v0.X) * int64_t(v1.Y - v0.Y);
    if (area == 0 || (cull == GNERF_RASTER_CULL_BACK && area > 0) || (cull == GNERF_RASTER_CULL_FRONT && area < 0)) { t.status = 3; return t; }
    t.flipped = area < 0;
    t.area = t.flipped ? -area : area;
    t.ax = v0.X; t.ay = v0.Y; t.iza = v0.iz;
    t.bx = t.flipped ? v2.X : v1.X; t.by = t.flipped ? v2.Y : v1.Y; t.izb = t.flipped ? v2.iz : v1.iz;
    t.cx = t.flipped ? v1.X : v2.X; t.cy = t.flipped ? v1.Y : v2.Y; t.izc = t.flipped ? v1.iz : v2.iz;
    const int minx = min(v0.X, min(v1.X, v2.X)), maxx = max(v0.X, max(v1.X, v2.X));
    const int miny = min(v0.Y, min(v1.Y, v2.Y)), maxy = max(v0.Y, max(v1.Y, v2.Y));
    // pixel centres 256 * i + 128 inside [min, max]  (>> floors: the operands may be negative)
    const int c0 = max((minx + 127) >> 8, 0), c1 = min((maxx - 128) >> 8, w - 1);
    const int r0 = max((miny + 127) >> 8, 0), r1 = min((maxy - 128) >> 8, h - 1);
    t.c0 = c0; t.r0 = r0;
    t.bw = max(c1 - c0 + 1, 0); t.bh = max(r1 - r0 + 1, 0);
    if (t.bw == 0 || t.bh == 0) { t.bw = 0; t.bh = 0; }
    return t;
}

// Edge functions of the centre of pixel (row, col); top-left rule: a centre on an edge belongs to the triangle iff the edge runs up
// (dy < 0: a left edge) or is horizontal and runs right (a top edge), for the orientation area > 0 with y down.
__device__ __forceinline__ bool owns(int64_t e, int dx, int dy) { return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0))); }

__device__ __forceinline__ bool cover(const Tri& t, int row, int col, int64_t& wa, int64_t& wb, int64_t& wc) {
    const int px = 256 * col + 128, py = 256 * row + 128;
    wa = int64_t(t.cx - t.bx) * int64_t(py - t.by) - int64_t(t.cy - t.by) * int64_t(px - t.bx);       // edge b -> c: the weight of a
    wb = int64_t(t.ax - t.cx) * int64_t(py - t.cy) - int64_t(t.ay - t.cy) * int64_t(px - t.cx);       // edge c -> a
    wc = int64_t(t.bx - t.ax) * int64_t(py - t.ay) - int64_t(t.by - t.ay) * int64_t(px - t.ax);       // edge a -> b
    return owns(wa, t.cx - t.bx, t.cy - t.by) && owns(wb, t.ax - t.cx, t.ay - t.cy) && owns(wc, t.bx - t.ax, t.by - t.ay);
}

__device__ __forceinline__ float interp_iz(const Tri& t, int64_t wa, int64_t wb, int64_t wc, float& ba, float& bb, float& bc) {
    const float fa = float(t.area);
    ba = div_rn(float(wa), fa);
    bb = div_rn(float(wb), fa);
    bc = div_rn(float(wc), fa);
    return add_rn(add_rn(mul_rn(ba, t.iza), mul_rn(bb, t.izb)), mul_rn(bc, t.izc));
}

__device__ __forceinline__ void plot(const Tri& t, int row, int col, u64* __restrict__ vis_view, int w, uint32_t tri) {
    int64_t wa, wb, wc;
    if (!cover(t, row, col, wa, wb, wc)) return;
    float ba, bb, bc;
    const float z = div_rn(1.0f, interp_iz(t, wa, wb, wc, ba, bb, bc));
    const u64 key = (u64(__float_as_uint(z)) << 32) | u64(tri);
    u64* cell = vis_view + (int64_t(row) * w + col);
    if (*reinterpret_cast<volatile u64*>(cell) > key) atomicMin(cell, key);
}

// faces of triangle t -> its three projected vertices; false when a face names a vertex outside [0, n_verts)
__device__ __forceinline__ bool fetch(const float* __restrict__ verts, int n_verts, const int32_t* __restrict__ faces, int64_t t, const Camera& cam,
                                      float near_z, Vtx& v0, Vtx& v1, Vtx& v2, int (&id)[3]) {
    id[0] = faces[t * 3 + 0]; id[1] = faces[t * 3 + 1]; id[2] = faces[t * 3 + 2];
    if (uint32_t(id[0]) >= uint32_t(n_verts) || uint32_t(id[1]) >= uint32_t(n_verts) || uint32_t(id[2]) >= uint32_t(n_verts)) return false;
    v0 = project(cam, verts + int64_t(id[0]) * 3, near_z);
    v1 = project(cam, verts + int64_t(id[1]) * 3, near_z);
    v2 = project(cam, verts + int64_t(id[2]) * 3, near_z);
    return true;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
}

__global__ __launch_bounds__(kThreads) void raster_init_kernel(u64* __restrict__ vis, int64_t n, u64* __restrict__ counts, Workspace ws) {
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads) vis[i] = kEmpty;
    if (blockIdx.x == 0 && threadIdx.x < 4) counts[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 4) *ws.qcount = 0u;
}

__global__ __launch_bounds__(kThreads) void raster_small_kernel(const float* __restrict__ verts, int n_verts, const int32_t* __restrict__ faces, int n_tris,
                                                                const float* __restrict__ mesh2cam, const float* __restrict__ intrinsics, int total, int h, int w,
                                                                float near_z, int cull, Workspace ws, u64* __restrict__ vis, u64* __restrict__ counts) {
    const int g = int(blockIdx.x) * kThreads + int(threadIdx.x);
    int status = 4;                                  // 4: no triangle for this thread
    Tri t = {};
    int view = 0, tri = 0;
    if (g < total) {
        view = g / n_tris;
        tri = g - view * n_tris;
        const Camera cam = load_camera(mesh2cam, intrinsics, view, h, w);
        Vtx v0, v1, v2;
        int id[3];
        if (fetch(verts, n_verts, faces, tri, cam, near_z, v0, v1, v2, id)) {
            t = setup(v0, v1, v2, cull, h, w);
            status = t.status;
        } else {
            status = 3;
        }
    }
    const bool first = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const uint64_t m = __ballot(status == s);
        if (first && m) atomicAdd(counts + s, u64(__popcll(m)));
    }
    const int npx = status == 0 ? t.bw * t.bh : 0;
    const bool large = npx > kSmall;
    const uint64_t m = __ballot(large);
    if (m) {
        uint32_t base = 0;
        if (first) base = atomicAdd(ws.qcount, uint32_t(__popcll(m)));
        base = __shfl(base, 0, 64);
        if (large) ws.queue[base + lanes_below(m)] = g;
    }
    if (npx == 0 || large) return;
    u64* vis_view = vis + int64_t(view) * h * w;
    for (int r = 0; r < t.bh; r++)
        for (int c = 0; c < t.bw; c++) plot(t, t.r0 + r, t.c0 + c, vis_view, w, uint32_t(tri));
}

__global__ __launch_bounds__(kThreads) void raster_large_kernel(const float* __restrict__ verts, int n_verts, const int32_t* __restrict__ faces, int n_tris,
                                                                const float* __restrict__ mesh2cam, const float* __restrict__ intrinsics, int total, int h, int w,
                                                                float near_z, int cull, Workspace ws, u64* __restrict__ vis) {
    const uint32_t qlen = min(*ws.qcount, uint32_t(total));
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * uint32_t(kThreads / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * uint32_t(kThreads / 64);
    for (uint32_t q = wave; q < qlen; q += n_waves) {
        const int g = ws.queue[q];
        if (uint32_t(g) >= uint32_t(total)) continue;
        const int view = g / n_tris, tri = g - view * n_tris;
        const Camera cam = load_camera(mesh2cam, intrinsics, view, h, w);
        Vtx v0, v1, v2;
        int id[3];
        if (!fetch(verts, n_verts, faces, tri, cam, near_z, v0, v1, v2, id)) continue;
        const Tri t = setup(v0, v1, v2, cull, h, w);
        if (t.status != 0) continue;
        u64* vis_view = vis + int64_t(view) * h * w;
        const int npx = t.bw * t.bh;
        for (int i = lane; i < npx; i += 64) {
            const int r = i / t.bw;
            plot(t, t.r0 + r, t.c0 + (i - r * t.bw), vis_view, w, uint32_t(tri));
        }
    }
}

struct Shading {
    float light[3], ambient, diffuse, albedo[3], background[3];
};

__device__ __forceinline__ float dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return add_rn(add_rn(mul_rn(a0, b0), mul_rn(a1, b1)), mul_rn(a2, b2));
}

__device__ __forceinline__ unsigned char to_u8(float v) { return (unsigned char)(int)rintf(mul_rn(fminf(fmaxf(v, 0.0f), 1.0f), 255.0f)); }

__global__ __launch_bounds__(kThreads) void raster_resolve_kernel(const u64* __restrict__ vis, const float* __restrict__ verts, int n_verts,
                                                                  const int32_t* __restrict__ faces, int n_tris, const float* __restrict__ mesh2cam,
                                                                  const float* __restrict__ intrinsics, int n_pixels, int h, int w,
                                                                  const float* __restrict__ normals, const float* __restrict__ normal_mat,
                                                                  const unsigned char* __restrict__ colors, Shading sh, int32_t* __restrict__ out_tri,
                                                                  float* __restrict__ out_depth, float* __restrict__ out_normal, unsigned char* __restrict__ out_frame) {
    const int p = int(blockIdx.x) * kThreads + int(threadIdx.x);
    if (p >= n_pixels) return;
    const int view = p / (h * w), rem = p - view * (h * w), row = rem / w, col = rem - row * w;
    const u64 key = vis[p];
    const uint32_t tri = uint32_t(key);
    bool hit = key != kEmpty && tri < uint32_t(n_tris);
    Vtx v0, v1, v2;
    int id[3];
    Camera cam;
    if (hit) {
        cam = load_camera(mesh2cam, intrinsics, view, h, w);
        hit = fetch(verts, n_verts, faces, tri, cam, 0.0f, v0, v1, v2, id);
    }
    Tri t = {};
    if (hit) {
        t = setup(v0, v1, v2, GNERF_RASTER_CULL_NONE, h, w);
        hit = t.status == 0;
    }
    if (!hit) {
        if (out_tri) out_tri[p] = -1;
        if (out_depth) out_depth[p] = __builtin_inff();
        if (out_normal) { out_normal[int64_t(p) * 3 + 0] = 0.f; out_normal[int64_t(p) * 3 + 1] = 0.f; out_normal[int64_t(p) * 3 + 2] = 0.f; }
        if (out_frame) {
#pragma unroll
            for (int k = 0; k < 3; k++) out_frame[int64_t(p) * 3 + k] = to_u8(sh.background[k]);
        }
        return;
    }
    int64_t wa, wb, wc;
    (void)cover(t, row, col, wa, wb, wc);
    float ba, bb, bc;
    const float iz = interp_iz(t, wa, wb, wc, ba, bb, bc);
    const float z = div_rn(1.0f, iz);
    // the pixel's ray as csrc/raygen.h forms it (camera frame, before normalisation): (xl, yl, 1)
    const float xc = add_rn(mul_rn(float(col), div_rn(1.0f, cam.wf)), div_rn(0.5f, cam.wf));
    const float yc = add_rn(mul_rn(float(row), div_rn(1.0f, cam.hf)), div_rn(0.5f, cam.hf));
    float xl = sub_rn(xc, cam.cx);
    xl = add_rn(xl, div_rn(mul_rn(cam.cy, cam.sk), cam.fy));
    xl = sub_rn(xl, div_rn(mul_rn(cam.sk, yc), cam.fy));
    xl = div_rn(xl, cam.fx);
    const float yl = div_rn(sub_rn(yc, cam.cy), cam.fy);
    if (out_tri) out_tri[p] = int32_t(tri);
    if (out_depth) out_depth[p] = mul_rn(z, sqrtf(add_rn(add_rn(mul_rn(xl, xl), mul_rn(yl, yl)), 1.0f)));
    if (!out_normal && !out_frame) return;
    // perspective-correct attribute weights of (a, b, c)
    const float qa = div_rn(mul_rn(ba, t.iza), iz), qb = div_rn(mul_rn(bb, t.izb), iz), qc = div_rn(mul_rn(bc, t.izc), iz);
    const int ia = id[0], ib = t.flipped ? id[2] : id[1], ic = t.flipped ? id[1] : id[2];
    float n[3];
    if (normals) {
        const float* na = normals + int64_t(ia) * 3;
        const float* nb = normals + int64_t(ib) * 3;
        const float* nc = normals + int64_t(ic) * 3;
        float m[3];
#pragma unroll
        for (int k = 0; k < 3; k++) m[k] = add_rn(add_rn(mul_rn(qa, na[k]), mul_rn(qb, nb[k])), mul_rn(qc, nc[k]));
        const float* N = normal_mat + int64_t(view) * 9;
#pragma unroll
        for (int r = 0; r < 3; r++) n[r] = dot3(N[r * 3 + 0], N[r * 3 + 1], N[r * 3 + 2], m[0], m[1], m[2]);
    } else {
        const float e1[3] = {sub_rn(v1.p[0], v0.p[0]), sub_rn(v1.p[1], v0.p[1]), sub_rn(v1.p[2], v0.p[2])};
        const float e2[3] = {sub_rn(v2.p[0], v0.p[0]), sub_rn(v2.p[1], v0.p[1]), sub_rn(v2.p[2], v0.p[2])};
        n[0] = sub_rn(mul_rn(e1[1], e2[2]), mul_rn(e1[2], e2[1]));
        n[1] = sub_rn(mul_rn(e1[2], e2[0]), mul_rn(e1[0], e2[2]));
        n[2] = sub_rn(mul_rn(e1[0], e2[1]), mul_rn(e1[1], e2[0]));
    }
    const float len = sqrtf(dot3(n[0], n[1], n[2], n[0], n[1], n[2]));
    const bool ok = len > 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) n[k] = ok ? div_rn(n[k], len) : 0.0f;
    if (add_rn(add_rn(mul_rn(n[0], xl), mul_rn(n[1], yl)), n[2]) > 0.0f) {       // turned to face the camera
#pragma unroll
        for (int k = 0; k < 3; k++) n[k] = -n[k];
    }
    if (out_normal) {
#pragma unroll
        for (int k = 0; k < 3; k++) out_normal[int64_t(p) * 3 + k] = n[k];
    }
    if (out_frame) {
        const float shade = add_rn(sh.ambient, mul_rn(sh.diffuse, fmaxf(0.0f, dot3(n[0], n[1], n[2], sh.light[0], sh.light[1], sh.light[2]))));
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float base = sh.albedo[k];
            if (colors) {
                const float ca = float(colors[int64_t(ia) * 3 + k]), cb = float(colors[int64_t(ib) * 3 + k]), cc = float(colors[int64_t(ic) * 3 + k]);
                base = div_rn(add_rn(add_rn(mul_rn(qa, ca), mul_rn(qb, cb)), mul_rn(qc, cc)), 255.0f);
            }
            out_frame[int64_t(p) * 3 + k] = to_u8(mul_rn(base, shade));
        }
    }
}

// ------------------------------------------------------------------------------------------------ colour bake (gnerf_mesh_bake_colors)
// The rasteriser's inverse: one thread per VERTEX gathers its colour from the views' frames.  The loop over the views is wave-uniform and the
// camera (and normal_mat) of an iteration is indexed by the loop counter alone, so it sits in scalar registers; what a lane gathers is the
// window of visibility keys around its pixel and the four taps of the frame (marching cubes numbers neighbouring vertices together, so the
// lanes of a wave hit neighbouring pixels).  No LDS, no atomics; every rule is in include/gnerf_hip.h and in shape_mi355x.bake_colors_numpy.
struct BakeRules {
    float near_z, depth_tol, min_cos;
    int power;
};

// One view of one point: the bake's rules from the vertex stage to the accumulation, the stage the vertex bake and the texture bake are both
// built from (the same bits in both).  v: the point in the mesh frame; n: its normal there, read only when normal_mat is given.  A view that
// fails a test leaves the sums as they are.
struct BakeSums {
    float acc0, acc1, acc2, accw;
    int count;
};

template <int GUARD>
__device__ __forceinline__ void bake_view(const float (&v)[3], const float (&n)[3], int view, const float* __restrict__ mesh2cam,
                                          const float* __restrict__ intrinsics, const u64* __restrict__ vis, int h, int w,
                                          const unsigned char* __restrict__ frames, int fh, int fw, const float* __restrict__ normal_mat,
                                          const BakeRules& rules, BakeSums& sums) {
    const float fwf = float(fw), fhf = float(fh);
    const Camera cam = load_camera(mesh2cam, intrinsics, view, h, w);
    const Point q = to_image(cam, v, rules.near_z);
    if (!q.ok) return;
    const float sx = mul_rn(q.xc, cam.wf), sy = mul_rn(q.yc, cam.hf);
    if (!(sx >= 0.0f && sx < cam.wf && sy >= 0.0f && sy < cam.hf)) return;
    const int col = int(floorf(sx)), row = int(floorf(sy));
    // occlusion: every pixel of the window holds a surface, and none of them lies in front of the point by more than the tolerance.
    // Coordinates held inside the image visit exactly the pixels of the clipped window (some of them twice).
    const u64* __restrict__ vis_view = vis + int64_t(view) * h * w;
    bool open = true;
#pragma unroll
    for (int dr = -GUARD; dr <= GUARD; dr++)
#pragma unroll
        for (int dc = -GUARD; dc <= GUARD; dc++) {
            const int r = min(max(row + dr, 0), h - 1), c = min(max(col + dc, 0), w - 1);
            const u64 key = vis_view[int64_t(r) * w + c];
            const float z_pix = __uint_as_float(uint32_t(key >> 32));
            open &= key != kEmpty && q.p[2] <= add_rn(z_pix, mul_rn(rules.depth_tol, z_pix));
        }
    if (!open) return;
    float wgt = 1.0f;
    if (normal_mat) {
        const float* N = normal_mat + int64_t(view) * 9;
        float nc[3];
#pragma unroll
        for (int r = 0; r < 3; r++) nc[r] = dot3(N[r * 3 + 0], N[r * 3 + 1], N[r * 3 + 2], n[0], n[1], n[2]);
        const float np_ = dot3(nc[0], nc[1], nc[2], q.p[0], q.p[1], q.p[2]);
        const float nn = dot3(nc[0], nc[1], nc[2], nc[0], nc[1], nc[2]), pp = dot3(q.p[0], q.p[1], q.p[2], q.p[0], q.p[1], q.p[2]);
        const float cosine = div_rn(-np_, sqrtf(mul_rn(nn, pp)));
        if (!(cosine > rules.min_cos)) return;
        if (rules.power > 0) {
            wgt = cosine;
            for (int k = 1; k < rules.power; k++) wgt = mul_rn(wgt, cosine);
        }
    }
    // bilinear sample of the frame at the point's own position (texel centres at integer + 0.5), the taps clamped into the frame
    const float u = sub_rn(mul_rn(q.xc, fwf), 0.5f), t = sub_rn(mul_rn(q.yc, fhf), 0.5f);
    const float x0f = floorf(u), y0f = floorf(t);
    const float tx = sub_rn(u, x0f), ty = sub_rn(t, y0f);
    const float ux = sub_rn(1.0f, tx), uy = sub_rn(1.0f, ty);
    const int x0 = min(max(int(x0f), 0), fw - 1), x1 = min(max(int(x0f) + 1, 0), fw - 1);
    const int y0 = min(max(int(y0f), 0), fh - 1), y1 = min(max(int(y0f) + 1, 0), fh - 1);
    const unsigned char* __restrict__ frame = frames + int64_t(view) * fh * fw * 3;
    const unsigned char* p00 = frame + (int64_t(y0) * fw + x0) * 3;
    const unsigned char* p01 = frame + (int64_t(y0) * fw + x1) * 3;
    const unsigned char* p10 = frame + (int64_t(y1) * fw + x0) * 3;
    const unsigned char* p11 = frame + (int64_t(y1) * fw + x1) * 3;
    float s[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float top = add_rn(mul_rn(ux, float(p00[k])), mul_rn(tx, float(p01[k])));
        const float bot = add_rn(mul_rn(ux, float(p10[k])), mul_rn(tx, float(p11[k])));
        s[k] = add_rn(mul_rn(uy, top), mul_rn(ty, bot));
    }
    sums.acc0 = add_rn(sums.acc0, mul_rn(wgt, s[0]));
    sums.acc1 = add_rn(sums.acc1, mul_rn(wgt, s[1]));
    sums.acc2 = add_rn(sums.acc2, mul_rn(wgt, s[2]));
    sums.accw = add_rn(sums.accw, wgt);
    sums.count++;
}

__device__ __forceinline__ unsigned char level_u8(float v) { return (unsigned char)(int)rintf(fminf(fmaxf(v, 0.0f), 255.0f)); }

// GUARD is a template parameter so that the window's loads have no branch between them and are all in flight together: a loop that left at
// the first failing pixel waited for every key in turn (guard = 1, 32 views of 512^2: 0.154 -> 0.071 ms for 78 k vertices, 0.163 -> 0.149 ms
// for 352 k).
template <int GUARD>
__global__ __launch_bounds__(kThreads) void mesh_bake_kernel(const float* __restrict__ verts, int n_verts, const float* __restrict__ mesh2cam,
                                                             const float* __restrict__ intrinsics, int n_views, const u64* __restrict__ vis, int h, int w,
                                                             const unsigned char* __restrict__ frames, int fh, int fw, const float* __restrict__ normals,
                                                             const float* __restrict__ normal_mat, BakeRules rules, const unsigned char* __restrict__ fallback,
                                                             unsigned char* __restrict__ colors, float* __restrict__ weight, int32_t* __restrict__ seen) {
    const int i = int(blockIdx.x) * kThreads + int(threadIdx.x);
    if (i >= n_verts) return;
    const float v[3] = {verts[int64_t(i) * 3 + 0], verts[int64_t(i) * 3 + 1], verts[int64_t(i) * 3 + 2]};
    float n[3] = {0.f, 0.f, 0.f};
    if (normals) { n[0] = normals[int64_t(i) * 3 + 0]; n[1] = normals[int64_t(i) * 3 + 1]; n[2] = normals[int64_t(i) * 3 + 2]; }
    BakeSums sums = {0.f, 0.f, 0.f, 0.f, 0};
    for (int view = 0; view < n_views; view++)
        bake_view<GUARD>(v, n, view, mesh2cam, intrinsics, vis, h, w, frames, fh, fw, normals ? normal_mat : nullptr, rules, sums);
    unsigned char out[3] = {0, 0, 0};
    if (sums.accw > 0.0f) {
        out[0] = level_u8(div_rn(sums.acc0, sums.accw));
        out[1] = level_u8(div_rn(sums.acc1, sums.accw));
        out[2] = level_u8(div_rn(sums.acc2, sums.accw));
    } else if (fallback) {
        out[0] = fallback[int64_t(i) * 3 + 0]; out[1] = fallback[int64_t(i) * 3 + 1]; out[2] = fallback[int64_t(i) * 3 + 2];
    }
    colors[int64_t(i) * 3 + 0] = out[0]; colors[int64_t(i) * 3 + 1] = out[1]; colors[int64_t(i) * 3 + 2] = out[2];
    if (weight) weight[i] = sums.accw;
    if (seen) seen[i] = sums.count;
}

// ------------------------------------------------------------------------------------------------ texture bake (gnerf_mesh_bake_texture)
// The same gather per TEXEL of the atlas include/gnerf_hip.h lays out (two triangles to a P x P cell): thread g is texel g % P^2 of cell
// g / P^2, so the texels of a cell are consecutive threads -- at P = 8 a wave is one cell, its lanes read two face records and six vertices
// between them (one request each), and what they gather from a view are neighbouring pixels.  The loop over the views is wave-uniform, the
// cameras sit in scalar registers as in the vertex bake.  The grid covers every cell of the texture, the empty ones of the last row too:
// every texel is written.
struct Atlas {
    int patch, cells_per_row, tw, n_pairs;
};

template <int GUARD>
__global__ __launch_bounds__(kThreads) void mesh_bake_texture_kernel(const float* __restrict__ verts, int n_verts, const int32_t* __restrict__ faces,
                                                                     int n_tris, Atlas atlas, int n_texels, const float* __restrict__ mesh2cam,
                                                                     const float* __restrict__ intrinsics, int n_views, const u64* __restrict__ vis,
                                                                     int h, int w, const unsigned char* __restrict__ frames, int fh, int fw,
                                                                     const float* __restrict__ normals, const float* __restrict__ normal_mat,
                                                                     BakeRules rules, const unsigned char* __restrict__ fallback, uchar3 background,
                                                                     unsigned char* __restrict__ texture, float* __restrict__ weight,
                                                                     int32_t* __restrict__ seen) {
    const int g = int(blockIdx.x) * kThreads + int(threadIdx.x);
    if (g >= n_texels) return;
    const int P = atlas.patch, pp = P * P;
    const int pair = g / pp, local = g - pair * pp, j = local / P, i = local - j * P;
    const int crow = pair / atlas.cells_per_row, ccol = pair - crow * atlas.cells_per_row;
    const int64_t texel = int64_t(crow * P + j) * atlas.tw + (ccol * P + i);
    const int half = i + j >= P ? 1 : 0;
    const int64_t t = int64_t(pair) * 2 + half;
    int id[3] = {0, 0, 0};
    bool owned = t < n_tris;
    if (owned) {
        id[0] = faces[t * 3 + 0]; id[1] = faces[t * 3 + 1]; id[2] = faces[t * 3 + 2];
        owned = uint32_t(id[0]) < uint32_t(n_verts) && uint32_t(id[1]) < uint32_t(n_verts) && uint32_t(id[2]) < uint32_t(n_verts);
    }
    if (!owned) {
        texture[texel * 3 + 0] = background.x; texture[texel * 3 + 1] = background.y; texture[texel * 3 + 2] = background.z;
        if (weight) weight[texel] = 0.0f;
        if (seen) seen[texel] = -1;
        return;
    }
    const float L = float(P - 3);
    const float b1 = div_rn(float(half ? P - 1 - i : i), L), b2 = div_rn(float(half ? P - 1 - j : j), L);
    const float b0 = sub_rn(sub_rn(1.0f, b1), b2);
    const float* v0 = verts + int64_t(id[0]) * 3;
    const float* v1 = verts + int64_t(id[1]) * 3;
    const float* v2 = verts + int64_t(id[2]) * 3;
    float x[3], n[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; k++) x[k] = add_rn(add_rn(mul_rn(b0, v0[k]), mul_rn(b1, v1[k])), mul_rn(b2, v2[k]));
    if (normals) {
        const float* n0 = normals + int64_t(id[0]) * 3;
        const float* n1 = normals + int64_t(id[1]) * 3;
        const float* n2 = normals + int64_t(id[2]) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) n[k] = add_rn(add_rn(mul_rn(b0, n0[k]), mul_rn(b1, n1[k])), mul_rn(b2, n2[k]));
    }
    // what an unseen texel holds, made before the loop over the views: the fallback's pointer, the corner ids and the barycentrics need not
    // live through it (the guard = 4 instantiation has no scalar register to spare)
    unsigned char unseen[3] = {background.x, background.y, background.z};
    if (fallback) {
        const unsigned char* c0 = fallback + int64_t(id[0]) * 3;
        const unsigned char* c1 = fallback + int64_t(id[1]) * 3;
        const unsigned char* c2 = fallback + int64_t(id[2]) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) unseen[k] = level_u8(add_rn(add_rn(mul_rn(b0, float(c0[k])), mul_rn(b1, float(c1[k]))), mul_rn(b2, float(c2[k]))));
    }
    unsigned char* __restrict__ out = texture + texel * 3;
    BakeSums sums = {0.f, 0.f, 0.f, 0.f, 0};
    for (int view = 0; view < n_views; view++)
        bake_view<GUARD>(x, n, view, mesh2cam, intrinsics, vis, h, w, frames, fh, fw, normals ? normal_mat : nullptr, rules, sums);
    const bool hit = sums.accw > 0.0f;
    out[0] = hit ? level_u8(div_rn(sums.acc0, sums.accw)) : unseen[0];
    out[1] = hit ? level_u8(div_rn(sums.acc1, sums.accw)) : unseen[1];
    out[2] = hit ? level_u8(div_rn(sums.acc2, sums.accw)) : unseen[2];
    if (weight) weight[texel] = sums.accw;
    if (seen) seen[texel] = sums.count;
}

// ------------------------------------------------------------------------------------------------ textured resolve
// raster_resolve_kernel's sibling: one thread per pixel, the winning triangle set up again (the same bits), its perspective-correct weights
// taken back from the drawn order to the face's own corners, and the atlas sampled bilinearly at the point they name in the triangle's patch.
__global__ __launch_bounds__(kThreads) void raster_resolve_textured_kernel(const u64* __restrict__ vis, const float* __restrict__ verts, int n_verts,
                                                                           const int32_t* __restrict__ faces, int n_tris, const float* __restrict__ mesh2cam,
                                                                           const float* __restrict__ intrinsics, int n_pixels, int h, int w,
                                                                           const unsigned char* __restrict__ texture, Atlas atlas, int th, uchar3 background,
                                                                           unsigned char* __restrict__ out_frame) {
    const int p = int(blockIdx.x) * kThreads + int(threadIdx.x);
    if (p >= n_pixels) return;
    const int view = p / (h * w), rem = p - view * (h * w), row = rem / w, col = rem - row * w;
    const u64 key = vis[p];
    const uint32_t tri = uint32_t(key);
    bool hit = key != kEmpty && tri < uint32_t(n_tris);
    Vtx v0, v1, v2;
    int id[3];
    if (hit) {
        const Camera cam = load_camera(mesh2cam, intrinsics, view, h, w);
        hit = fetch(verts, n_verts, faces, tri, cam, 0.0f, v0, v1, v2, id);
    }
    Tri t = {};
    if (hit) {
        t = setup(v0, v1, v2, GNERF_RASTER_CULL_NONE, h, w);
        hit = t.status == 0;
    }
    if (!hit) {
        out_frame[int64_t(p) * 3 + 0] = background.x; out_frame[int64_t(p) * 3 + 1] = background.y; out_frame[int64_t(p) * 3 + 2] = background.z;
        return;
    }
    int64_t wa, wb, wc;
    (void)cover(t, row, col, wa, wb, wc);
    float ba, bb, bc;
    const float iz = interp_iz(t, wa, wb, wc, ba, bb, bc);
    const float qb = div_rn(mul_rn(bb, t.izb), iz), qc = div_rn(mul_rn(bc, t.izc), iz);
    const float q1 = t.flipped ? qc : qb, q2 = t.flipped ? qb : qc;      // drawn as (0, 2, 1) when flipped: back to the face's corners 1 and 2
    const int P = atlas.patch, pair = int(tri >> 1);
    const int crow = pair / atlas.cells_per_row, ccol = pair - crow * atlas.cells_per_row;
    const float L = float(P - 3), far = float(P - 1);
    float lx = mul_rn(q1, L), ly = mul_rn(q2, L);
    if (tri & 1u) { lx = sub_rn(far, lx); ly = sub_rn(far, ly); }
    const float u = add_rn(float(ccol * P), lx), s = add_rn(float(crow * P), ly);
    const float x0f = floorf(u), y0f = floorf(s);
    const float tx = sub_rn(u, x0f), ty = sub_rn(s, y0f);
    const float ux = sub_rn(1.0f, tx), uy = sub_rn(1.0f, ty);
    const int tw = atlas.tw;
    const int x0 = min(max(int(x0f), 0), tw - 1), x1 = min(max(int(x0f) + 1, 0), tw - 1);
    const int y0 = min(max(int(y0f), 0), th - 1), y1 = min(max(int(y0f) + 1, 0), th - 1);
    const unsigned char* p00 = texture + (int64_t(y0) * tw + x0) * 3;
    const unsigned char* p01 = texture + (int64_t(y0) * tw + x1) * 3;
    const unsigned char* p10 = texture + (int64_t(y1) * tw + x0) * 3;
    const unsigned char* p11 = texture + (int64_t(y1) * tw + x1) * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float top = add_rn(mul_rn(ux, float(p00[k])), mul_rn(tx, float(p01[k])));
        const float bot = add_rn(mul_rn(ux, float(p10[k])), mul_rn(tx, float(p11[k])));
        out_frame[int64_t(p) * 3 + k] = level_u8(add_rn(mul_rn(uy, top), mul_rn(ty, bot)));
    }
}

int check_geometry(const char* what, int n_verts, int n_tris, int n_views, int h, int w, int64_t* total) {
    using namespace gnerf;
    if (n_verts < 0 || n_tris < 0) return fail(GNERF_E_ARG, "%s: negative vertex or triangle count", what);
    if (n_views < 1) return fail(GNERF_E_ARG, "%s: n_views must be >= 1 (got %d)", what, n_views);
    if (h < 1 || w < 1 || h > GNERF_RASTER_MAX_SIZE || w > GNERF_RASTER_MAX_SIZE)
        return fail(GNERF_E_ARG, "%s: the image size must be 1..%d in each direction (got %d x %d)", what, GNERF_RASTER_MAX_SIZE, h, w);
    if (int64_t(n_views) * n_tris >= (int64_t(1) << 31)) return fail(GNERF_E_ARG, "%s: n_views * n_tris must be below 2^31", what);
    if (int64_t(n_views) * h * w >= (int64_t(1) << 31)) return fail(GNERF_E_ARG, "%s: n_views * h * w must be below 2^31 pixels", what);
    *total = n_verts == 0 ? 0 : int64_t(n_views) * n_tris;                  // no vertices: nothing to draw
    return GNERF_OK;
}

}  // namespace

extern "C" int gnerf_raster_workspace_bytes(int n_verts, int n_tris, int n_views, int h, int w, size_t* bytes) {
    using namespace gnerf;
    if (!bytes) return fail(GNERF_E_ARG, "raster_workspace_bytes: null pointer");
    int64_t total;
    if (int rc = check_geometry("raster_workspace_bytes", n_verts, n_tris, n_views, h, w, &total)) return rc;
    carve(nullptr, int64_t(n_views) * n_tris, bytes);
    return GNERF_OK;
}

extern "C" int gnerf_raster_visibility(const float* verts, int n_verts, const int32_t* faces, int n_tris, const float* mesh2cam, const float* intrinsics,
                                       int n_views, int h, int w, float near_z, int cull, void* workspace, uint64_t* vis, int64_t* counts,
                                       gnerf_stream_t stream) {
    using namespace gnerf;
    const char* what = "raster_visibility";
    int64_t total;
    if (int rc = check_geometry(what, n_verts, n_tris, n_views, h, w, &total)) return rc;
    if (!workspace || !vis || !counts || !mesh2cam || !intrinsics) return fail(GNERF_E_ARG, "%s: null pointer", what);
    if (total > 0 && (!verts || !faces)) return fail(GNERF_E_ARG, "%s: null pointer (verts / faces of a non-empty mesh)", what);
    if (!(near_z > 0.0f)) return fail(GNERF_E_ARG, "%s: near must be > 0", what);
    if (cull != GNERF_RASTER_CULL_NONE && cull != GNERF_RASTER_CULL_BACK && cull != GNERF_RASTER_CULL_FRONT)
        return fail(GNERF_E_ARG, "%s: cull must be GNERF_RASTER_CULL_NONE, _BACK or _FRONT (got %d)", what, cull);
    const Workspace ws = carve(workspace, int64_t(n_views) * n_tris, nullptr);
    u64* v = reinterpret_cast<u64*>(vis);
    u64* c = reinterpret_cast<u64*>(counts);
    const int64_t n_pixels = int64_t(n_views) * h * w;
    const int init_blocks = int(std::min<int64_t>((n_pixels + kThreads - 1) / kThreads, 8192));
    hipLaunchKernelGGL(raster_init_kernel, dim3(init_blocks), dim3(kThreads), 0, as_stream(stream), v, n_pixels, c, ws);
    if (int rc = check_launch("raster_visibility (init)")) return rc;
    if (total == 0) return GNERF_OK;
    const int blocks = int((total + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(raster_small_kernel, dim3(blocks), dim3(kThreads), 0, as_stream(stream), verts, n_verts, faces, n_tris, mesh2cam, intrinsics,
                       int(total), h, w, near_z, cull, ws, v, c);
    if (int rc = check_launch("raster_visibility (small)")) return rc;
    hipLaunchKernelGGL(raster_large_kernel, dim3(std::min(kLargeBlocks, blocks * (kThreads / 64))), dim3(kThreads), 0, as_stream(stream), verts, n_verts, faces,
                       n_tris, mesh2cam, intrinsics, int(total), h, w, near_z, cull, ws, v);
    return check_launch("raster_visibility (large)");
}

extern "C" int gnerf_raster_resolve(const uint64_t* vis, const float* verts, int n_verts, const int32_t* faces, int n_tris, const float* mesh2cam,
                                    const float* intrinsics, int n_views, int h, int w, const float* normals, const float* normal_mat,
                                    const unsigned char* colors, const float* shading, int32_t* tri_id, float* depth, float* normal, unsigned char* frame,
                                    gnerf_stream_t stream) {
    using namespace gnerf;
    const char* what = "raster_resolve";
    int64_t total;
    if (int rc = check_geometry(what, n_verts, n_tris, n_views, h, w, &total)) return rc;
    if (!vis || !mesh2cam || !intrinsics) return fail(GNERF_E_ARG, "%s: null pointer", what);
    if (total > 0 && (!verts || !faces)) return fail(GNERF_E_ARG, "%s: null pointer (verts / faces of a non-empty mesh)", what);
    if (!tri_id && !depth && !normal && !frame) return fail(GNERF_E_ARG, "%s: no output is asked for", what);
    if (normals && !normal_mat) return fail(GNERF_E_ARG, "%s: normals need normal_mat", what);
    if (frame && !shading) return fail(GNERF_E_ARG, "%s: frame needs the shading parameters", what);
    Shading sh = {};
    if (shading) {
        for (int k = 0; k < 3; k++) { sh.light[k] = shading[k]; sh.albedo[k] = shading[5 + k]; sh.background[k] = shading[8 + k]; }
        sh.ambient = shading[3];
        sh.diffuse = shading[4];
    }
    const int n_pixels = n_views * h * w;
    hipLaunchKernelGGL(raster_resolve_kernel, dim3((n_pixels + kThreads - 1) / kThreads), dim3(kThreads), 0, as_stream(stream),
                       reinterpret_cast<const u64*>(vis), verts, n_verts, faces, total == 0 ? 0 : n_tris, mesh2cam, intrinsics, n_pixels, h, w, normals,
                       normal_mat, colors, sh, tri_id, depth, normal, frame);
    return check_launch("raster_resolve");
}

extern "C" int gnerf_mesh_bake_colors(const float* verts, int n_verts, const float* mesh2cam, const float* intrinsics, int n_views, const uint64_t* vis,
                                      int h, int w, const unsigned char* frames, int fh, int fw, const float* normals, const float* normal_mat,
                                      float near_z, float depth_tol, int guard, float min_cos, int power, const unsigned char* fallback,
                                      unsigned char* colors, float* weight, int32_t* seen, gnerf_stream_t stream) {
    using namespace gnerf;
    const char* what = "mesh_bake_colors";
    int64_t total;
    if (int rc = check_geometry(what, n_verts, 0, n_views, h, w, &total)) return rc;
    if (int rc = check_geometry("mesh_bake_colors (frames)", n_verts, 0, n_views, fh, fw, &total)) return rc;
    if (!mesh2cam || !intrinsics || !vis || !frames) return fail(GNERF_E_ARG, "%s: null pointer", what);
    if (n_verts > 0 && (!verts || !colors)) return fail(GNERF_E_ARG, "%s: null pointer (verts / colors of a non-empty mesh)", what);
    if (!(near_z > 0.0f)) return fail(GNERF_E_ARG, "%s: near must be > 0", what);
    if (!(depth_tol >= 0.0f)) return fail(GNERF_E_ARG, "%s: depth_tol must be >= 0", what);
    if (guard < 0 || guard > GNERF_BAKE_MAX_GUARD) return fail(GNERF_E_ARG, "%s: guard must be 0..%d (got %d)", what, GNERF_BAKE_MAX_GUARD, guard);
    if (power < 0 || power > GNERF_BAKE_MAX_POWER) return fail(GNERF_E_ARG, "%s: power must be 0..%d (got %d)", what, GNERF_BAKE_MAX_POWER, power);
    if (normals && !normal_mat) return fail(GNERF_E_ARG, "%s: normals need normal_mat", what);
    if (n_verts == 0) return GNERF_OK;
    const BakeRules rules = {near_z, depth_tol, min_cos, power};
    static_assert(GNERF_BAKE_MAX_GUARD == 4, "one instantiation per guard");
    const auto kernel = guard == 0 ? mesh_bake_kernel<0> : guard == 1 ? mesh_bake_kernel<1> : guard == 2 ? mesh_bake_kernel<2>
                      : guard == 3 ? mesh_bake_kernel<3> : mesh_bake_kernel<4>;
    hipLaunchKernelGGL(kernel, dim3((n_verts + kThreads - 1) / kThreads), dim3(kThreads), 0, as_stream(stream), verts, n_verts, mesh2cam, intrinsics,
                       n_views, reinterpret_cast<const u64*>(vis), h, w, frames, fh, fw, normals, normal_mat, rules, fallback, colors, weight, seen);
    return check_launch("mesh_bake_colors");
}

namespace {

// The atlas rule of include/gnerf_hip.h, in integers.  rc != 0: the error is set.
int atlas_layout(const char* what, int n_tris, int patch, int* cells_per_row, int* th, int* tw) {
    using namespace gnerf;
    if (n_tris < 0) return fail(GNERF_E_ARG, "%s: negative triangle count", what);
    if (patch < GNERF_ATLAS_MIN_PATCH || patch > GNERF_ATLAS_MAX_PATCH)
        return fail(GNERF_E_ARG, "%s: patch must be %d..%d (got %d)", what, GNERF_ATLAS_MIN_PATCH, GNERF_ATLAS_MAX_PATCH, patch);
    const int64_t n_pairs = (int64_t(n_tris) + 1) / 2;
    int64_t c = 0;
    while (c * c < n_pairs) c++;                     // (at most 32768 steps, on the host)
    const int64_t rows = c ? (n_pairs + c - 1) / c : 0;
    if (c * patch > GNERF_ATLAS_MAX_SIZE || rows * patch > GNERF_ATLAS_MAX_SIZE)
        return fail(GNERF_E_UNSUPPORTED, "%s: %d triangles at patch %d need an atlas of %lld x %lld texels, more than %d a side", what, n_tris, patch,
                    (long long)(rows * patch), (long long)(c * patch), GNERF_ATLAS_MAX_SIZE);
    *cells_per_row = int(c);
    *th = int(rows * patch);
    *tw = int(c * patch);
    return GNERF_OK;
}

}  // namespace

extern "C" int gnerf_mesh_atlas_layout(int n_tris, int patch, int* cells_per_row, int* th, int* tw) {
    using namespace gnerf;
    if (!cells_per_row || !th || !tw) return fail(GNERF_E_ARG, "mesh_atlas_layout: null pointer");
    return atlas_layout("mesh_atlas_layout", n_tris, patch, cells_per_row, th, tw);
}

extern "C" int gnerf_mesh_bake_texture(const float* verts, int n_verts, const int32_t* faces, int n_tris, int patch, const float* mesh2cam,
                                       const float* intrinsics, int n_views, const uint64_t* vis, int h, int w, const unsigned char* frames, int fh, int fw,
                                       const float* normals, const float* normal_mat, float near_z, float depth_tol, int guard, float min_cos, int power,
                                       const unsigned char* fallback, const unsigned char* background, unsigned char* texture, float* weight, int32_t* seen,
                                       gnerf_stream_t stream) {
    using namespace gnerf;
    const char* what = "mesh_bake_texture";
    int64_t total;
    if (int rc = check_geometry(what, n_verts, n_tris, n_views, h, w, &total)) return rc;
    if (int rc = check_geometry("mesh_bake_texture (frames)", n_verts, n_tris, n_views, fh, fw, &total)) return rc;
    if (!mesh2cam || !intrinsics || !vis || !frames || !background) return fail(GNERF_E_ARG, "%s: null pointer", what);
    if (n_tris > 0 && (!faces || !texture || (n_verts > 0 && !verts))) return fail(GNERF_E_ARG, "%s: null pointer (verts / faces / texture of a non-empty mesh)", what);
    if (!(near_z > 0.0f)) return fail(GNERF_E_ARG, "%s: near must be > 0", what);
    if (!(depth_tol >= 0.0f)) return fail(GNERF_E_ARG, "%s: depth_tol must be >= 0", what);
    if (guard < 0 || guard > GNERF_BAKE_MAX_GUARD) return fail(GNERF_E_ARG, "%s: guard must be 0..%d (got %d)", what, GNERF_BAKE_MAX_GUARD, guard);
    if (power < 0 || power > GNERF_BAKE_MAX_POWER) return fail(GNERF_E_ARG, "%s: power must be 0..%d (got %d)", what, GNERF_BAKE_MAX_POWER, power);
    if (normals && !normal_mat) return fail(GNERF_E_ARG, "%s: normals need normal_mat", what);
    int cells, th, tw;
    if (int rc = atlas_layout(what, n_tris, patch, &cells, &th, &tw)) return rc;
    if (n_tris == 0) return GNERF_OK;
    const int n_texels = th * tw;                                          // at most 2^28
    const Atlas atlas = {patch, cells, tw, (n_tris + 1) / 2};
    const BakeRules rules = {near_z, depth_tol, min_cos, power};
    const uchar3 bg = {background[0], background[1], background[2]};
    static_assert(GNERF_BAKE_MAX_GUARD == 4, "one instantiation per guard");
    const auto kernel = guard == 0 ? mesh_bake_texture_kernel<0> : guard == 1 ? mesh_bake_texture_kernel<1> : guard == 2 ? mesh_bake_texture_kernel<2>
                      : guard == 3 ? mesh_bake_texture_kernel<3> : mesh_bake_texture_kernel<4>;
    hipLaunchKernelGGL(kernel, dim3((n_texels + kThreads - 1) / kThreads), dim3(kThreads), 0, as_stream(stream), verts, n_verts, faces, n_tris, atlas, n_texels,
                       mesh2cam, intrinsics, n_views, reinterpret_cast<const u64*>(vis), h, w, frames, fh, fw, normals, normal_mat, rules, fallback, bg, texture,
                       weight, seen);
    return check_launch("mesh_bake_texture");
}

extern "C" int gnerf_raster_resolve_textured(const uint64_t* vis, const float* verts, int n_verts, const int32_t* faces, int n_tris, const float* mesh2cam,
                                             const float* intrinsics, int n_views, int h, int w, const unsigned char* texture, int patch,
                                             const unsigned char* background, unsigned char* frame, gnerf_stream_t stream) {
    using namespace gnerf;
    const char* what = "raster_resolve_textured";
    int64_t total;
    if (int rc = check_geometry(what, n_verts, n_tris, n_views, h, w, &total)) return rc;
    if (!vis || !mesh2cam || !intrinsics || !background || !frame) return fail(GNERF_E_ARG, "%s: null pointer", what);
    if (total > 0 && (!verts || !faces || !texture)) return fail(GNERF_E_ARG, "%s: null pointer (verts / faces / texture of a non-empty mesh)", what);
    int cells, th, tw;
    if (int rc = atlas_layout(what, n_tris, patch, &cells, &th, &tw)) return rc;
    const Atlas atlas = {patch, cells, tw, (n_tris + 1) / 2};
    const uchar3 bg = {background[0], background[1], background[2]};
    const int n_pixels = n_views * h * w;
    hipLaunchKernelGGL(raster_resolve_textured_kernel, dim3((n_pixels + kThreads - 1) / kThreads), dim3(kThreads), 0, as_stream(stream),
                       reinterpret_cast<const u64*>(vis), verts, n_verts, faces, total == 0 ? 0 : n_tris, mesh2cam, intrinsics, n_pixels, h, w, texture, atlas,
                       th, bg, frame);
    return check_launch("raster_resolve_textured");
}
