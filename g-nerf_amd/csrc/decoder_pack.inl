// The decoder pack's kernel.  Included by render_pipe.hip alone (it holds a kernel).
#pragma once
#include "decoder_choice.inl"
#include "render_pipe_layout.inl"

namespace {

// gnerf_render_pack_decoder: one workgroup makes the decoder pack (render_shade.inl has the layout).  The statistics come from
// decoder_stats, which sums the rows with the routines choose_mlp uses (w1_row_stats, w2_row_stats: decoder_choice.inl) on two waves; the images
// are what stage_decoder, the code the render kernels run without a pack, leaves in LDS.
__global__ __launch_bounds__(kPipeThreads) void pack_decoder_kernel(gnerf_render_params p, float* pack) {
    constexpr int kLds = kImageFloatsF32 > kImageFloatsF16 ? kImageFloatsF32 : kImageFloatsF16;
    static_assert(kLds >= kStatFloats + 64 * 33 + 33 * 65, "decoder_stats' rows fit the image area");
    __shared__ __align__(16) float smem[kLds];
    const int tid = threadIdx.x;
    decoder_stats(p, smem);
    __syncthreads();
    if (tid < kStatFloats) {
        const int* words = reinterpret_cast<const int*>(smem);
        reinterpret_cast<int*>(pack)[tid] = tid < kStatBad ? words[tid] : (tid == kStatBad ? ((words[kStatBad] | words[kStatBad2]) != 0 ? 1 : 0) : 0);
    }
    ShadeLds L;
    __syncthreads();
    for (int i = tid; i < kLds; i += kPipeThreads) smem[i] = 0.f;
    __syncthreads();
    stage_decoder<kMlpF16x3>(L, smem, p, tid, kPipeThreads);
    __syncthreads();
    for (int i = tid; i < kImageFloatsF16; i += kPipeThreads) pack[kPackImageF16 + i] = smem[i];
    __syncthreads();
    for (int i = tid; i < kLds; i += kPipeThreads) smem[i] = 0.f;
    __syncthreads();
    stage_decoder<kMlpF32>(L, smem, p, tid, kPipeThreads);
    __syncthreads();
    for (int i = tid; i < kImageFloatsF32; i += kPipeThreads) pack[kPackImageF32 + i] = smem[i];
}

}  // namespace
