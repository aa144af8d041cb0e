// The pipelined render kernels' constants, LDS layout and ray order: what their launchers (render.hip, render_pipe.hip) and the
// backward's tile kernel (render_bwd_tiles.inl walks the same ray sequence) need of render_pipe.inl.  No kernel is defined here.
// (scatter_binned.inl restates the order for 16-ray tiles in bin_tile_ray and needs nothing from here.)
#pragma once
#include "render_shade.inl"

namespace {

#ifndef GNERF_PIPE_UNIT
#define GNERF_PIPE_UNIT 8
#endif
constexpr int kPipeUnit = GNERF_PIPE_UNIT;      // rays dealt to a workgroup at a time (see render_kernel_pipe)
// guided dealing (pipe_dealing.h): each shrinking level covers kPipeGuidedC x (workgroups of the XCD) units; the smallest unit, 1 or 2 rays
#ifndef GNERF_PIPE_GUIDED_C
#define GNERF_PIPE_GUIDED_C 1
#endif
#ifndef GNERF_PIPE_GUIDED_MIN
#define GNERF_PIPE_GUIDED_MIN 1
#endif
constexpr int kPipeGuidedC = GNERF_PIPE_GUIDED_C, kPipeGuidedMin = GNERF_PIPE_GUIDED_MIN;
constexpr int kPipeThreads = 256;
constexpr int kPipeSlots = 4;
// TP = 16-sample tiles per shader wave and pass: 1 covers up to 48+48 samples (the reference's default), 2 up to 96+96, 3 up to 144+144
// (gen_videos.py doubles the ShapeNet configuration's 64+64 to 128+128)
// (gen_videos.py doubles the counts, gen_videos.py:127-128; the ShapeNet config uses 64+64).
template <int TP> struct PipeDims {
    static constexpr int kMaxS = 48 * TP;                  // samples per pass
    static constexpr int kSPad = 2 * kMaxS;                // coarse [0, kMaxS) + fine [kMaxS, 2 kMaxS)
    static constexpr int kRounds = (kMaxS + 63) / 64;      // lanes x rounds cover the samples of a pass
    static constexpr int kSlotFloats = 7 * kSPad + 2 * kMaxS + 96 + 16;        // seven per-sample arrays, cdf + fine noise (per pass), partials, ray
};

struct PipeSlot {
    float* t_e; float* sig_e; float* v_e; int* rank_e; float* s_t; float* s_sig; float* w_s; float* cdf;
    float* nf;      // [kMaxS] fine noise of this ray
    float* part;    // [3][32] colour partial sums of the shader waves
    float* misc;    // [0..11] the ray per plane: (ou, du, ov, dv) x 3 (ShadeRay, render_shade.inl)  [12] item (int)  [13] ray (int)  [14] w_sum  [15] wt_sum
};
constexpr int kMiscItem = 12, kMiscRay = 13, kMiscWsum = 14, kMiscWtsum = 15;
// lane l < 12 of the scalar wave carries component misc_comp(l) of (origin xyz, direction xyz): plane l / 4, then ou, du, ov, dv
__device__ __forceinline__ int misc_comp(int l) {
    const int pl = l >> 2, q = l & 3;
    const int axis = q < 2 ? (pl == 2 ? 2 : 0) : (pl == 0 ? 1 : (pl == 1 ? 2 : 0));       // u: x, x, z   v: y, z, x
    return (q & 1) * 3 + axis;
}

template <int TP>
__device__ __forceinline__ PipeSlot pipe_slot(float* base, int slot) {
    typedef PipeDims<TP> D;
    float* p = base + slot * D::kSlotFloats;
    PipeSlot s;
    s.t_e = p; s.sig_e = p + D::kSPad; s.v_e = p + 2 * D::kSPad; s.rank_e = reinterpret_cast<int*>(p + 3 * D::kSPad);
    s.s_t = p + 4 * D::kSPad; s.s_sig = p + 5 * D::kSPad; s.w_s = p + 6 * D::kSPad; s.cdf = p + 7 * D::kSPad;
    s.nf = s.cdf + D::kMaxS; s.part = s.nf + D::kMaxS; s.misc = s.part + 96;       // cdf: kMaxS entries (n_w + 1 <= S - 2 used, the rest +inf / histogram)
    return s;
}

__host__ __device__ inline size_t pipe_lds_floats(int tp, int mlp) {
    const size_t slot_floats = tp == 1 ? PipeDims<1>::kSlotFloats : (tp == 2 ? PipeDims<2>::kSlotFloats : PipeDims<3>::kSlotFloats);
    return size_t(weight_floats(mlp)) + 64 + 36 + size_t(kPipeSlots) * slot_floats + 3 * 16 * kStagePitch       // (tap records live in the staging rows)
           + kPipeUnit * 8                                                                                         // GEN: the dealing unit's rays
           + 4;                                                                                                    // on-demand dealing: the run's length
}
// Four TP = 1 workgroups share a CU's 160 KiB of LDS (GNERF_PIPE_WAVES_PER_SIMD): growth past that would silently drop to three.
static_assert(4 * sizeof(float) * (size_t(weight_floats(kMlpF32) > weight_floats(kMlpF16x3) ? weight_floats(kMlpF32) : weight_floats(kMlpF16x3)) + 64 + 36
                                   + size_t(kPipeSlots) * PipeDims<1>::kSlotFloats + 3 * 16 * kStagePitch + kPipeUnit * 8 + 4) <= 160 * 1024,
              "a TP = 1 workgroup of the pipelined render kernel must fit a CU's LDS four times");

// position `seq` of the locality-ordered ray sequence -> ray index (or -1 past the end)
// PADDED: instantiations of the backward only (linear_pad(P) is never set on a forward call: the forward kernels do not carry the branch)
template <bool PADDED = false>
__device__ __forceinline__ int pipe_seq_to_ray(const Params& P, int64_t seq) {
    const gnerf_render_params& p = P.p;
    if (P.tiles_per_item > 0) {
        const int tile = int(seq >> 4), rr = int(seq & 15);
        const int item = tile / P.tiles_per_item, tt = tile % P.tiles_per_item;
        const int tx = tt / P.tiles_y, ty = tt % P.tiles_y;
        return item * p.rays_per_item + (ty * 4 + (rr >> 2)) * p.image_width + tx * 4 + (rr & 3);
    }
    if constexpr (PADDED) {
        if (const int pad = linear_pad(P); pad > 0) {         // (the staged backward of ragged calls: items padded to whole 16-ray tiles)
            const int item = int(unsigned(seq) / unsigned(pad)), local = int(unsigned(seq) - unsigned(item) * unsigned(pad));     // (seq < 2^31: checked by the launcher)
            return (item < p.n_items && local < p.rays_per_item) ? item * p.rays_per_item + local : -1;
        }
    }
    return seq < P.total_rays ? int(seq) : -1;
}

#ifndef GNERF_PIPE2_WAVES_PER_SIMD
#define GNERF_PIPE2_WAVES_PER_SIMD 3
#endif
#ifndef GNERF_PIPE_WAVES_PER_SIMD
#define GNERF_PIPE_WAVES_PER_SIMD 4
#endif

}  // namespace
