// What the renderer's translation units share on the host side (render.hip, render_pipe.hip, render_backward.hip, render_query.hip):
// Params, which every render kernel takes by value, the validation that fills it, the facts more than one launcher needs, and the
// launch functions of the kernels of render_pipe.hip.  Defined in render.hip unless stated otherwise.
#pragma once
#include "common.h"
#include "raygen.h"

namespace gnerf {

struct Params {
    gnerf_render_params p;
    float box_scale;        // 2 / box_warp
    float delta;            // (ray_end - ray_start) / (S - 1)
    float inv_start, inv_end, disp_delta;
    int tiles_c, tiles_f;   // 16-sample MLP tiles
    int n_tiles;            // ray tiles in the grid
    int tiles_per_item, tiles_y;   // image tiling (0 when rays are not an image).  tiles_per_item == 0 with tiles_y > 0 (set by the staged backward
                            // of RAGGED calls only: several items, rays per item not a multiple of 16): every item's rays are padded to tiles_y,
                            // a multiple of 16, in the ray SEQUENCE, so that no 16-ray tile straddles items -- linear_pad() below.  (Kept in a
                            // field the forward already has: one more kernel argument cost the headline kernel eight spilled SGPRs.)
    int total_rays;
    int split_shift;        // small launches: a 16-ray tile is shared by 1 << split_shift workgroups (generic / backward kernels)
    int pipe_unit;          // pipelined kernel: rays dealt to a workgroup at a time (kPipeUnit; fewer for launches that do not fill the chip)
    int pipe_guided;        // pipelined forward, on demand with 8-ray units: c + 256 * (smallest unit) of the guided schedule (pipe_dealing.h), 0 = uniform units
    unsigned* deal_counters;        // pipelined forward: the workspace's per-XCD counters when units are dealt on demand, else null (static dealing)
    unsigned tex_pitch, row_pitch, plane_pitch;     // byte addressing of a texel, see plane_taps (render_shade.inl)
    int64_t item_bytes;     // bytes from one item's planes to the next: 3 * H * W * 128, or 0 when every item reads the same planes (planes_shared)
    const float* absmax;    // GNERF_MLP_AUTO: max |planes| (one device float) for choose_mlp
    TorchRandDraw draw_c, draw_f;   // rng_mode: the two draws torch's generator would have made (raygen.h)
    uint64_t draw_item_ctr;         // rng_per_item: Philox counter stride from one item's draws to the next (offset stride / 4)
    // staged backward on the pipelined path: floats per ray of the exchange / staging buffer and from one 16-rank tile's block to the
    // next (33 n_all and 512 when the blocks are the dX rows of the staged scatter; n_all + 32 tiles and 32 for a decoder-only request)
    int64_t bwd_ray_stride;
    int bwd_tile_pitch;
    const float* decoder_pack;      // pipelined forward: what gnerf_render_pack_decoder made of this call's decoder (statistics + LDS images, render_shade.inl), or null
};
__host__ __device__ __forceinline__ int linear_pad(const Params& P) { return P.tiles_per_item == 0 ? P.tiles_y : 0; }

// Validation and derived launch parameters: check_common for every entry point (planes and decoder), fill_params for the forward and
// backward render calls, fill_pitches for the byte addressing of a texel.
int check_common(const gnerf_render_params* p);
void fill_pitches(Params& P);
int fill_params(const gnerf_render_params* p, Params& P);

// ---- facts that more than one launcher needs, each worked out in one place
// (the pipelined, backward and query-gradient kernels address plane taps with 32-bit byte offsets)
inline bool planes_fit_32bit_taps(const gnerf_render_params* p) { return int64_t(p->plane_h) * p->plane_w * 3 * 128 < (int64_t(1) << 32); }
// 16-sample tiles per shader wave and pass of the pipelined kernels (render_pipe.inl), 0 where they do not cover the sample counts
inline int pipe_tiles_per_wave(const Params& P) {
    const int t = P.tiles_c > P.tiles_f ? P.tiles_c : P.tiles_f;
    return t <= 3 ? 1 : (t <= 6 ? 2 : (t <= 9 ? 3 : 0));
}
// positions of the ray sequence the pipelined kernels walk: whole 16-ray tiles where the rays are tiled or padded
inline int64_t pipe_seq_len(const Params& P) { return (P.tiles_per_item > 0 || linear_pad(P) > 0) ? int64_t(P.n_tiles) * 16 : int64_t(P.total_rays); }
// Dealing unit and grid of a pipelined launch (the forward's, the backward's first pass): see pipe_launch in render.hip
struct PipeLaunch { int unit; unsigned grid; bool fills_chip; };
PipeLaunch pipe_launch(int tp, int64_t total_seq);
// what choose_mlp reads: the caller's planes_absmax, else measured into `scratch`
int absmax_or_measure(const gnerf_render_params* p, float* scratch, gnerf_stream_t stream, const float*& absmax);

// The launch functions of render_pipe.hip, the unit of the kernels that stage the decoder.  launch_pipe: one pipelined forward launch,
// render_kernel_pipe<TP, mlp, full, gen> for TP = 1, 2, 3 tiles per shader wave and pass (gen: in-kernel rays / draws, built with full
// for TP 1 and 2 and refused for anything else).  launch_pipe_bwd: render_kernel_pipe_bwd<TP>, the first pass of the staged backward.
// launch_bwd_tiles: render_bwd_tiles_kernel over n_tiles 16-rank tiles, its second pass.
template <int TP> int launch_pipe(bool full, bool gen, int mlp, unsigned grid, hipStream_t s, const Params& P);
template <int TP> int launch_pipe_bwd(unsigned grid, hipStream_t s, const Params& P, const gnerf_render_grads& g);
int launch_bwd_tiles(int64_t n_tiles, hipStream_t s, const Params& P, const gnerf_render_grads& g);

}  // namespace gnerf
