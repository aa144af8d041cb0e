// The renderer's kernels that stage the decoder with stage_decoder (render_shade.inl), and their launch functions (render_params.h declares
// them): the pipelined forward kernels render_kernel_pipe<TP, ...> and the backward's first pass render_kernel_pipe_bwd<TP> (render_pipe.inl),
// the backward's tile kernel (render_bwd_tiles.inl) and the decoder pack (decoder_pack.inl) with its two exports.
//
// They are one unit, and must stay one, for the sake of reproducible code.  The toolchain gives every non-kernel device function internal
// linkage, and before it inlines them it propagates constants and value ranges into their arguments from all call sites of the unit.
// Every kernel here but pack_decoder_kernel hands stage_decoder the same dynamic LDS array; the pack kernel hands it an array of its own,
// which keeps that argument (and decoder_lds's, and the row pointers of w1_row_stats / w2_row_stats) a variable for all of them.  Compiled
// without the pack kernel, the others get the array's address folded into the staging code ahead of inlining, and come out with other
// address arithmetic and register numbers in every kernel: same arithmetic, different instruction streams (tools/asm_same_kernels.py shows
// it).  One unit can hold the pack kernel, so a unit per TP cannot be had with the instruction streams kept.
// What that costs: this unit is 29 of the renderer's 45 kernels and about nine tenths of its device assembly, and it is the build's
// longest unit.  Its device-assembly pass, run alone, took 139 and 130 s where the single render.hip it came from took 154 and 156 s on
// the same machine (alternated); the build is not meaningfully shorter for the split, which is a clean-up of dependencies and no more.
// (Only the eight kMlpF32 instantiations of render_kernel_pipe compile to the same code outside this unit -- about an eighth of its
// assembly: not worth a second launch path.)
#include "render_pipe.inl"
#include "render_bwd_tiles.inl"
#include "decoder_pack.inl"

namespace {

// One pipelined forward launch.  These are all the instantiations of render_kernel_pipe: GEN (in-kernel rays / draws) is built with FULL
// for TP 1 and 2 and for nothing else.  TP = 3 takes 65 KB of LDS, above the default dynamic limit.
template <int TP, bool FULL, bool GEN>
int launch_pipe_kernel(int mlp, unsigned grid, hipStream_t s, const Params& P) {
    static_assert(!GEN || (FULL && TP <= 2), "in-kernel rays / draws: 48+48 and 96+96 samples only");
    void (*kernel)(Params) = render_kernel_pipe<TP, kMlpAuto, FULL, GEN>;
    if (mlp == kMlpF16x3) kernel = render_kernel_pipe<TP, kMlpF16x3, FULL, GEN>;
    if (mlp == kMlpF32) kernel = render_kernel_pipe<TP, kMlpF32, FULL, GEN>;
    if constexpr (TP == 3) {
        static_assert(kMlpAuto == 0 && kMlpF16x3 == 1 && kMlpF32 == 2, "once[] is indexed by the MLP mode");
        static gnerf::PerDeviceOnce once[3];                    // one per kernel of this instantiation (mlp is one of the three: checked by the caller)
        if (int e = once[mlp].raise_lds(kernel, "render")) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPipeThreads), pipe_lds_floats(TP, mlp) * sizeof(float), s, P);
    return gnerf::check_launch("render_kernel_pipe");
}

}  // namespace

template <int TP> int gnerf::launch_pipe(bool full, bool gen, int mlp, unsigned grid, hipStream_t s, const Params& P) {
    if (gen) {
        if constexpr (TP <= 2) { if (full) return launch_pipe_kernel<TP, true, true>(mlp, grid, s, P); }
        return fail(GNERF_E_UNSUPPORTED, "render: in-kernel rays / draws are built for 48+48 and 96+96 samples with plain stratified sampling");
    }
    return full ? launch_pipe_kernel<TP, true, false>(mlp, grid, s, P) : launch_pipe_kernel<TP, false, false>(mlp, grid, s, P);
}
template int gnerf::launch_pipe<1>(bool, bool, int, unsigned, hipStream_t, const Params&);
template int gnerf::launch_pipe<2>(bool, bool, int, unsigned, hipStream_t, const Params&);
template int gnerf::launch_pipe<3>(bool, bool, int, unsigned, hipStream_t, const Params&);

template <int TP> int gnerf::launch_pipe_bwd(unsigned grid, hipStream_t s, const Params& P, const gnerf_render_grads& g) {
    if constexpr (TP == 3) {
        static PerDeviceOnce once;
        if (int e = once.raise_lds(render_kernel_pipe_bwd<TP>, "render_backward")) return e;
    }
    hipLaunchKernelGGL(render_kernel_pipe_bwd<TP>, dim3(grid), dim3(kPipeThreads), pipe_lds_floats(TP, kMlpAuto) * sizeof(float), s, P, g, g.scatter_stage);
    return check_launch("render_kernel_pipe_bwd");
}
template int gnerf::launch_pipe_bwd<1>(unsigned, hipStream_t, const Params&, const gnerf_render_grads&);
template int gnerf::launch_pipe_bwd<2>(unsigned, hipStream_t, const Params&, const gnerf_render_grads&);
template int gnerf::launch_pipe_bwd<3>(unsigned, hipStream_t, const Params&, const gnerf_render_grads&);

int gnerf::launch_bwd_tiles(int64_t n_tiles, hipStream_t s, const Params& P, const gnerf_render_grads& g) {
    const size_t lds2 = (bwd_tiles_weight_floats() + kTileWaves * bwd_tiles_wave_floats()) * sizeof(float);
    static PerDeviceOnce once_tiles;
    if (int e = once_tiles.raise_lds(render_bwd_tiles_kernel, "render_backward")) return e;
    int64_t g2 = (n_tiles + kTileWaves - 1) / kTileWaves;
    if (g2 > int64_t(kNumCU) * 2) g2 = int64_t(kNumCU) * 2;    // two workgroups of four waves per CU, each walking a contiguous run of tiles
    g2 = (g2 + kNumXCD - 1) / kNumXCD * kNumXCD;
    hipLaunchKernelGGL(render_bwd_tiles_kernel, dim3((unsigned)g2), dim3(kTileThreads), lds2, s, P, g, g.scatter_stage);
    return check_launch("render_bwd_tiles_kernel");
}

extern "C" size_t gnerf_render_decoder_pack_bytes(void) { return size_t(kPackFloats) * sizeof(float); }

extern "C" int gnerf_render_pack_decoder(const float* w1, const float* b1, const float* w2, const float* b2, void* pack, gnerf_stream_t stream) {
    using namespace gnerf;
    if (!w1 || !b1 || !w2 || !b2 || !pack) return fail(GNERF_E_ARG, "render_pack_decoder: null pointer");
    if (reinterpret_cast<uintptr_t>(pack) % 16 != 0) return fail(GNERF_E_ARG, "render_pack_decoder: pack must be 16-byte aligned");
    gnerf_render_params p = {};
    p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2;
    hipLaunchKernelGGL(pack_decoder_kernel, dim3(1), dim3(kPipeThreads), 0, as_stream(stream), p, static_cast<float*>(pack));
    return check_launch("pack_decoder_kernel");
}
