// Backward of the fused renderer: the entry points (gnerf_render_backward, gnerf_render_backward_rays and the two buffer sizes) and their
// kernels -- the one-wave-per-ray kernel and the sorted scatter (render_bwd.inl), the binned scatter (scatter_binned.inl)
// and the ray gradient (render_ray_grad.inl).  The two kernels of the pipelined path, render_kernel_pipe_bwd<TP> and render_bwd_tiles_kernel,
// live in render_pipe.hip and are launched through launch_pipe_bwd<TP> and launch_bwd_tiles.  render_backward_impl refuses, decides its route once (BwdRoute) and then launches from that
// decision alone.  Every A/B override is an environment variable read once per call, where the launcher starts deciding.
#include "render_bwd.inl"
#include "scatter_binned.inl"
#include "render_ray_grad.inl"
#include <cstdlib>
#include <cstring>

// The binned scatter (scatter_binned.inl) indexes the staging buffer with 32 bits and keeps an item's plane-tile histogram in LDS.
static bool binned_scatter_covers(const Params& P) {
    const gnerf_render_params& p = P.p;
    return int64_t(P.total_rays) * (p.depth_resolution + p.depth_resolution_importance) * 33 < (int64_t(1) << 32) &&
           (2 * size_t(3) * ((p.plane_h + kBinTile - 1) / kBinTile) * ((p.plane_w + kBinTile - 1) / kBinTile) + 128) * 4 <= 150 * 1024;
}
// A ragged call (several items whose ray count is no multiple of 16): the ray SEQUENCE pads every item to whole 16-ray tiles, so that no
// tile straddles items (linear_pad(P); pipe_seq_to_ray / bin_tile_ray answer -1 for the padding, which every kernel of the path skips).
static int padded_rays_per_item(const gnerf_render_params& p) { return (p.rays_per_item + kBwdRaysPerWave - 1) / kBwdRaysPerWave * kBwdRaysPerWave; }
static void pad_ray_sequence(Params& P) {
    P.tiles_y = padded_rays_per_item(P.p);                      // (tiles_per_item == 0 for such a call)
    P.n_tiles = P.p.n_items * (P.tiles_y / kBwdRaysPerWave);
}

// The second pass: the staged dX rows (ray stride 33 n_all) -> the plane gradient, binned or sorted.  P: the call's Params, its ray sequence
// padded where the route says so.
static int launch_scatter(const Params& P, bool binned, float* stage, float* grad_planes, hipStream_t s) {
    using namespace gnerf;
    const int n_all = P.p.depth_resolution + P.p.depth_resolution_importance;
    Params KS = P;
    KS.bwd_ray_stride = int64_t(n_all) * 33;
    if (binned) {
        char* ws = reinterpret_cast<char*>(stage) + bin_workspace_offset(P.total_rays, n_all);
        return launch_binned_scatter(KS, stage, ws, grad_planes, s);
    }
    static PerDeviceOnce once_scatter;
    if (int e = once_scatter.raise_lds(plane_scatter_kernel, "render_backward")) return e;
    hipLaunchKernelGGL(plane_scatter_kernel, dim3(KS.n_tiles), dim3(kScatterThreads), scatter_lds_floats() * sizeof(float), s,
                       KS, static_cast<const float*>(stage), grad_planes);
    return check_launch("plane_scatter_kernel");
}

// What one backward call launches: decided once in render_backward_impl, then only read (DESIGN.md 3.2 has the table of routes).
struct BwdRoute {
    // first pass.  Wave: render_bwd_kernel<false / true>, one wave per ray, float atomics into the plane gradient / dX rows into the staging buffer.
    // Piped: render_kernel_pipe_bwd + render_bwd_tiles_kernel, dX rows into the staging buffer / a decoder-only request's exchange buffer (no dX rows)
    enum First { kWaveDirect, kWaveStaged, kPipedRows, kPipedExchange } first;
    enum Second { kNoScatter, kBinned, kSorted } second;       // dX rows -> plane gradient: scatter_binned.inl or plane_scatter_kernel
    bool padded;            // every kernel of the call walks the padded ray sequence (pad_ray_sequence)
    bool scatter_padded;    // only the scatter does: the first pass stages by ray whatever the tiling
    int mlp_first, mlp_tiles;       // decoder arithmetic of the two piped kernels (GNERF_MLP_*)
};

// gnerf_render_backward, and with grad_origins / grad_dirs gnerf_render_backward_rays: the same launches, plus render_ray_grad_kernel between
// the first pass and the scatter.  Three parts: (a) what the call refuses, (b) its route, decided once, (c) the launches, which read that
// decision and nothing else and build each kernel's Params from P and it.
static int render_backward_impl(const gnerf_render_params* p, const gnerf_render_grads* g_in, float* grad_origins, float* grad_dirs, gnerf_stream_t stream) {
    using namespace gnerf;
    // ---- (a) refusals
    Params P;
    if (int e = fill_params(p, P)) return e;
    if (!g_in) return fail(GNERF_E_ARG, "render_backward: grads is null");
    const bool need_rays = grad_origins != nullptr || grad_dirs != nullptr;
    const bool want_planes = g_in->grad_planes_nhwc != nullptr;
    // A ray request needs the dX rows of the staged first pass whether or not a plane gradient is made from them.  The first-pass kernels
    // only TEST grad_planes_nhwc (the staged forms never write through it), so a ray-only request hands them the staging buffer's address
    // in its place, and there is no scatter.
    gnerf_render_grads g_eff = *g_in;
    if (need_rays && !want_planes) g_eff.grad_planes_nhwc = g_in->scatter_stage;
    const gnerf_render_grads* g = &g_eff;
    if (p->planes_shared) return fail(GNERF_E_UNSUPPORTED, "render_backward: planes_shared is a forward-only option");
    if (!p->ray_origins || p->rng_mode != GNERF_RNG_TENSORS) return fail(GNERF_E_UNSUPPORTED, "render_backward: in-kernel rays / draws are forward-only options");
    if (p->sigma_noise_coarse || p->sigma_noise_fine) return fail(GNERF_E_UNSUPPORTED, "render_backward: density noise is a forward-only option");
    const int n_dec = (g->grad_w1 != nullptr) + (g->grad_b1 != nullptr) + (g->grad_w2 != nullptr) + (g->grad_b2 != nullptr);
    if (n_dec != 0 && n_dec != 4) return fail(GNERF_E_ARG, "render_backward: the four decoder gradients are given together or not at all");
    if (need_rays) {
        // what dL/do = sum dL/dp, dL/dd = sum t dL/dp does not cover, before any launch
        if (!g->scatter_stage) return fail(GNERF_E_UNSUPPORTED, "render_backward_rays: the ray gradient reads the staged first pass: scatter_stage must hold gnerf_render_backward_stage_bytes(p)");
        if (p->ray_start_per_ray) return fail(GNERF_E_UNSUPPORTED, "render_backward_rays: per-ray limits ('auto') make the coarse depths depend on the rays; numeric ray_start / ray_end only");
    }
    if (!g->grad_planes_nhwc && n_dec == 0) return GNERF_OK;
    if (!planes_fit_32bit_taps(p)) return fail(GNERF_E_UNSUPPORTED, "render_backward: planes too large for 32-bit tap offsets");
    static_assert(kBwdRaysPerWave == kRaysPerWave, "ray tiles are shared with the forward launcher");
    const size_t lds_bytes = (kBwdWeightFloats + kBwdWaves * bwd_wave_floats(16 * (P.tiles_c + P.tiles_f))) * sizeof(float);
    if (lds_bytes > 160 * 1024) return fail(GNERF_E_ARG, "render_backward: %d+%d samples need %zu bytes of LDS (> 160 KiB)", p->depth_resolution, p->depth_resolution_importance, lds_bytes);
    static PerDeviceOnce once, once_staged;
    if (int e = once.raise_lds(render_bwd_kernel<false>, "render_backward")) return e;
    if (int e = once_staged.raise_lds(render_bwd_kernel<true>, "render_backward")) return e;
    // ---- (b) the route.  Overrides for A/B runs and tests, read per call (the tests switch them inside one process):
    BwdRoute route;
    {
        const char* scatter = getenv("GNERF_BWD_SCATTER"), *kernel = getenv("GNERF_BWD_KERNEL");        // direct | staged | sorted;  wave
        const char* mlp = getenv("GNERF_BWD_MLP"), *mlp_k1 = getenv("GNERF_BWD_MLP_K1"), *mlp_k2 = getenv("GNERF_BWD_MLP_K2");
        auto is = [](const char* v, const char* word) { return v && !strcmp(v, word); };
        const bool force_direct = is(scatter, "direct"), force_sorted = is(scatter, "sorted"), force_staged = is(scatter, "staged");
        // decoder arithmetic of the piped kernels: chosen on the device like the forward's; GNERF_BWD_MLP=f32|f16x3|auto forces both, _K1 / _K2 one
        auto mode_of = [&](const char* v, int dflt) { return is(v, "f32") ? GNERF_MLP_F32 : is(v, "f16x3") ? GNERF_MLP_F16X3 : is(v, "auto") ? GNERF_MLP_AUTO : dflt; };
        route.mlp_first = mode_of(mlp_k1, mode_of(mlp, GNERF_MLP_AUTO));
        route.mlp_tiles = mode_of(mlp_k2, mode_of(mlp, GNERF_MLP_AUTO));
        // (F = 0 included: the pipeline's steps and barriers do not depend on the sample counts; a ray without an importance pass shades no
        //  fine tile, merges nothing and marches its coarse samples)
        const bool pipe_shape = pipe_tiles_per_wave(P) != 0 && !is(kernel, "wave");
        const bool rows = g->scatter_stage != nullptr && g->grad_planes_nhwc != nullptr;       // dX rows can be staged, and something reads them
        const bool whole_tiles = P.tiles_per_item > 0 || p->n_items == 1 || p->rays_per_item % kBwdRaysPerWave == 0;    // no 16-ray tile straddles items
        const bool binned = binned_scatter_covers(P);
        const bool can_pad = binned && int64_t(p->n_items) * padded_rays_per_item(*p) < INT32_MAX;
        // a ragged call stays off the one-wave-per-ray kernel and its float atomics where the piped kernels and the binned scatter cover it
        route.padded = !whole_tiles && rows && pipe_shape && !force_direct && !force_sorted && can_pad;
        bool staged = rows && (whole_tiles || route.padded) && !force_direct;
        // A ray request whose ray tiles straddle items on a route that does not pad them: the one-wave-per-ray kernel stages by ray whatever
        // the tiling, so it runs on the call as it is; a plane gradient then takes the binned scatter over the padded ray sequence.
        const bool rows_for_rays = need_rays && !staged;
        route.scatter_padded = rows_for_rays && want_planes;
        if (rows_for_rays) {
            if (force_direct) return fail(GNERF_E_UNSUPPORTED, "render_backward_rays: GNERF_BWD_SCATTER=direct stages no dX rows");
            if (want_planes && (!can_pad || force_sorted))
                return fail(GNERF_E_UNSUPPORTED, "render_backward_rays: ray tiles straddle items and the binned scatter does not cover this call");
            staged = true;
        }
        if (force_staged && !staged) return fail(GNERF_E_ARG, "render_backward: the staged scatter needs scatter_stage, a plane gradient and whole tiles per item");
        const bool exchange = g->scatter_stage != nullptr && g->grad_planes_nhwc == nullptr && n_dec == 4;       // (never a ray request: g_eff above)
        const bool piped = (staged || exchange) && pipe_shape && !force_direct && !rows_for_rays;
        route.first = piped ? (staged ? BwdRoute::kPipedRows : BwdRoute::kPipedExchange) : (staged ? BwdRoute::kWaveStaged : BwdRoute::kWaveDirect);
        // (sorted: the per-ray-tile sort with one atomic per texel and chunk; it also takes the calls the binned form does not cover)
        route.second = !(staged && want_planes) ? BwdRoute::kNoScatter : (binned && !force_sorted ? BwdRoute::kBinned : BwdRoute::kSorted);
    }
    // ---- (c) launches
    hipStream_t s = as_stream(stream);
    const int n_all = p->depth_resolution + p->depth_resolution_importance;
    Params K = P;                                            // the first pass's
    // up to two workgroups of four waves per CU: share tiles until the chip is full (read by the one-wave-per-ray kernel only; every route carries it)
    while (K.split_shift < 2 && (int64_t(K.n_tiles) << (K.split_shift + 1)) <= int64_t(kNumCU) * 2 * kBwdWaves) K.split_shift++;
    if (route.padded) pad_ray_sequence(K);
    if (route.first == BwdRoute::kPipedRows || route.first == BwdRoute::kPipedExchange) {
        // The ray-level part on the forward pipeline (render_kernel_pipe_bwd), the per-sample part as a kernel over sample tiles
        // (render_bwd_tiles_kernel).  Floats per ray of the staging / exchange buffer and from one 16-rank tile's block to the next:
        const bool rows = route.first == BwdRoute::kPipedRows;
        K.bwd_ray_stride = rows ? int64_t(n_all) * 33 : int64_t(n_all) + 32 * ((n_all + 15) / 16);
        K.bwd_tile_pitch = rows ? 512 : 32;
        // (max |planes| goes into the 256 bytes behind the rows when the caller has none)
        if (int e = absmax_or_measure(p, g->scatter_stage + size_t(P.total_rays) * K.bwd_ray_stride, stream, K.absmax)) return e;
        K.p.workspace = nullptr;                                   // (the backward's params carry no workspace)
        K.p.mlp_mode = route.mlp_first;
        const int tp = pipe_tiles_per_wave(K);
        const int64_t total_seq = pipe_seq_len(K);
        const PipeLaunch L = pipe_launch(tp, total_seq);
        K.pipe_unit = L.unit;
        if (int e = tp == 1 ? launch_pipe_bwd<1>(L.grid, s, K, *g) : tp == 2 ? launch_pipe_bwd<2>(L.grid, s, K, *g) : launch_pipe_bwd<3>(L.grid, s, K, *g)) return e;
        Params K2 = K;
        K2.p.mlp_mode = route.mlp_tiles;
        if (int e = launch_bwd_tiles(total_seq * ((n_all + 15) / 16), s, K2, *g)) return e;
    } else {
        const int n_blocks = ((K.n_tiles << K.split_shift) + kBwdWaves - 1) / kBwdWaves;
        const dim3 grid((n_blocks + kNumXCD - 1) / kNumXCD * kNumXCD);
        if (route.first == BwdRoute::kWaveStaged) hipLaunchKernelGGL(render_bwd_kernel<true>, grid, dim3(kBwdThreads), lds_bytes, s, K, *g, g->scatter_stage);
        else hipLaunchKernelGGL(render_bwd_kernel<false>, grid, dim3(kBwdThreads), lds_bytes, s, K, *g, static_cast<float*>(nullptr));
        if (int e = check_launch("render_bwd_kernel")) return e;
    }
    if (need_rays) {
        RayGradArgs R;
        R.planes = p->planes_nhwc; R.origins = p->ray_origins; R.dirs = p->ray_dirs; R.stage = g->scatter_stage;
        R.grad_origins = grad_origins; R.grad_dirs = grad_dirs;
        R.plane_floats = int64_t(3) * p->plane_h * p->plane_w * 32;
        R.H = p->plane_h; R.W = p->plane_w; R.n_all = n_all;
        R.rays_per_item = p->rays_per_item; R.total_rays = P.total_rays;
        R.tex_pitch = P.tex_pitch; R.row_pitch = P.row_pitch; R.plane_pitch = P.plane_pitch; R.box_scale = P.box_scale;
        int64_t blocks = (int64_t(P.total_rays) + kRayGradWaves - 1) / kRayGradWaves;
        if (blocks > int64_t(kNumCU) * 8) blocks = int64_t(kNumCU) * 8;          // eight workgroups of four waves per CU, rays by grid stride
        hipLaunchKernelGGL(render_ray_grad_kernel, dim3((unsigned)blocks), dim3(kRayGradThreads), 0, s, R);
        if (int e = check_launch("render_ray_grad_kernel")) return e;
    }
    if (route.second == BwdRoute::kNoScatter) return GNERF_OK;
    Params KS = K;                                           // the scatter's
    if (route.scatter_padded) pad_ray_sequence(KS);
    return launch_scatter(KS, route.second == BwdRoute::kBinned, g->scatter_stage, g->grad_planes_nhwc, s);
}

extern "C" int gnerf_render_backward(const gnerf_render_params* p, const gnerf_render_grads* g, gnerf_stream_t stream) {
    return render_backward_impl(p, g, nullptr, nullptr, stream);
}

extern "C" int gnerf_render_backward_rays(const gnerf_render_params* p, const gnerf_render_grads* g, float* grad_origins, float* grad_dirs, gnerf_stream_t stream) {
    if (!grad_origins && !grad_dirs) return gnerf::fail(GNERF_E_ARG, "render_backward_rays: grad_origins and grad_dirs are both null (gnerf_render_backward is that call)");
    return render_backward_impl(p, g, grad_origins, grad_dirs, stream);
}

// The second pass alone, on rows and depths the caller wrote (include/gnerf_hip.h): the refusals and the choice of scatter are those of
// render_backward_impl for a staged plane gradient, the launches are launch_scatter's.
extern "C" int gnerf_render_scatter_rows(const gnerf_render_params* p, float* stage, float* grad_planes_nhwc, gnerf_stream_t stream) {
    using namespace gnerf;
    Params P;
    if (int e = fill_params(p, P)) return e;
    if (!stage || !grad_planes_nhwc) return fail(GNERF_E_ARG, "render_scatter_rows: stage and grad_planes_nhwc must not be null");
    if (p->planes_shared) return fail(GNERF_E_UNSUPPORTED, "render_scatter_rows: planes_shared is a forward-only option");
    if (!p->ray_origins || p->rng_mode != GNERF_RNG_TENSORS) return fail(GNERF_E_UNSUPPORTED, "render_scatter_rows: in-kernel rays / draws are forward-only options");
    if (p->sigma_noise_coarse || p->sigma_noise_fine) return fail(GNERF_E_UNSUPPORTED, "render_scatter_rows: density noise is a forward-only option");
    if (!planes_fit_32bit_taps(p)) return fail(GNERF_E_UNSUPPORTED, "render_scatter_rows: planes too large for 32-bit tap offsets");
    const char* scatter = getenv("GNERF_BWD_SCATTER");
    const bool force_direct = scatter && !strcmp(scatter, "direct"), force_sorted = scatter && !strcmp(scatter, "sorted");
    if (force_direct) return fail(GNERF_E_UNSUPPORTED, "render_scatter_rows: GNERF_BWD_SCATTER=direct stages no dX rows");
    const bool whole_tiles = P.tiles_per_item > 0 || p->n_items == 1 || p->rays_per_item % kBwdRaysPerWave == 0;
    const bool binned = binned_scatter_covers(P);
    const bool can_pad = binned && int64_t(p->n_items) * padded_rays_per_item(*p) < INT32_MAX;
    const bool padded = !whole_tiles && pipe_tiles_per_wave(P) != 0 && !force_sorted && can_pad;        // (route.padded of the whole call)
    if (!whole_tiles && !padded) return fail(GNERF_E_UNSUPPORTED, "render_scatter_rows: ray tiles straddle items and the binned scatter does not cover this call");
    if (padded) pad_ray_sequence(P);
    return launch_scatter(P, binned && !force_sorted, stage, grad_planes_nhwc, as_stream(stream));
}

extern "C" size_t gnerf_render_backward_stage_bytes(const gnerf_render_params* p) {
    if (!p || p->n_items < 1 || p->rays_per_item < 1) return 0;
    const size_t n_all = size_t(p->depth_resolution) + size_t(p->depth_resolution_importance);
    const int64_t rays = int64_t(p->n_items) * p->rays_per_item;
    // the staged rows (+ a spare line: max |planes| when the caller has none), then the binned scatter's workspace: counters, the
    // record array (16 bytes per sample and plane) and the tiles' halos (scatter_binned.inl)
    return bin_workspace_offset(rays, int(n_all)) + bin_workspace_bytes(rays, int(n_all), p->n_items, p->plane_h > 0 ? p->plane_h : 1, p->plane_w > 0 ? p->plane_w : 1);
}

extern "C" size_t gnerf_render_backward_exchange_bytes(const gnerf_render_params* p) {
    if (!p || p->n_items < 1 || p->rays_per_item < 1) return 0;
    const size_t n_all = size_t(p->depth_resolution) + size_t(p->depth_resolution_importance);
    return size_t(p->n_items) * size_t(p->rays_per_item) * (n_all + 32 * ((n_all + 15) / 16)) * sizeof(float) + 256;
}
