/*
 * gnerf_hip.h -- C ABI of libgnerf_hip.so, the MI355X (gfx950) implementation of G-NeRF's
 * hot path: the tri-plane importance renderer and the StyleGAN custom ops.
 *
 * Plain pointers and sizes only; every pointer is a DEVICE pointer unless it says "host".
 * All entry points enqueue work on `stream` (a hipStream_t passed as void*) and return
 * immediately; they return 0 on success and a negative GNERF_E_* code on failure
 * (gnerf_last_error() then holds a message for the calling thread).  No entry point
 * allocates, frees or synchronises, so all of them are hipGraph-capturable (marching cubes as a whole is
 * not: its caller reads counts to the host between its two passes, see gnerf_marching_cubes_count).
 *
 * Reference interfaces replaced (paths relative to the reference's g_nerf/):
 *   gnerf_bias_act          <- bias_act_plugin.bias_act            torch_utils/ops/bias_act.cpp:36
 *   gnerf_upfirdn2d         <- upfirdn2d_plugin.upfirdn2d          torch_utils/ops/upfirdn2d.cpp:20
 *   gnerf_filtered_lrelu    <- filtered_lrelu_plugin.filtered_lrelu      torch_utils/ops/filtered_lrelu.cpp:20
 *   gnerf_filtered_lrelu_act<- filtered_lrelu_plugin.filtered_lrelu_act_ torch_utils/ops/filtered_lrelu.cpp:217
 *   gnerf_grid_sample_2d(_backward) <- torch_utils/ops/grid_sample_gradfix.py:45, :62-77 (ATen's sampler upstream)
 *   gnerf_modulate_weights / gnerf_scale_channels / gnerf_modconv_epilogue <- the ATen elementwise chains of modulated_conv2d
 *                              and SynthesisLayer.forward                training/networks_stylegan2.py:41-98, :315-334
 *   gnerf_render_forward    <- ImportanceRenderer.forward          training/volumetric_rendering/renderer.py:88-140
 *                              (pure PyTorch in the reference; there is no native counterpart)
 *   gnerf_query_points      <- ImportanceRenderer.run_model        training/volumetric_rendering/renderer.py:142-148
 *   gnerf_make_rays         <- RaySampler.forward                  training/volumetric_rendering/ray_sampler.py:24-63
 *   gnerf_planes_to_nhwc    <- (layout change feeding the renderer; the reference keeps NCHW, triplane.py:74)
 *   gnerf_planes_to_nhwc_stats / gnerf_planes_absmax <- (the same + max |planes|, which picks the decoder arithmetic)
 *   gnerf_upsample2x_add_nhwc <- the backbone's last `upsample2d(img) + torgb(x)` (networks_stylegan2.py:456-463), channels_last
 *   gnerf_planes_from_nhwc  <- (the same for the plane gradient on the way back)
 *   gnerf_render_backward   <- autograd through renderer.py:88-140 (grid_sample_gradfix.py:62-77 for the planes)
 *   gnerf_marching_cubes_*  <- skimage.measure.marching_cubes as shape_utils.py:58-61 calls it (new rules, table and order:
 *                              shape_mi355x.py; the one family of entry points that needs a host synchronisation in between)
 *   gnerf_ssim_*            <- pytorch_msssim's ssim / ms_ssim as training_loop.py:341-376 calls them (a Python package of grouped
 *                              convolutions there; no native counterpart)
 *   gnerf_resize_aa_*       <- F.interpolate(mode='bilinear', align_corners=False, antialias=True) as superresolution.py:290-293 and
 *                              training_loop.py's ssim_resize call it, and its gradient (ATen's kernels there)
 *   gnerf_mesh_*            <- (no counterpart: the reference only zeroes fixed borders of the volume, gen_videos.py:214-221; the compaction,
 *                              like marching cubes, needs a host read between its two passes)
 */
#ifndef GNERF_HIP_H
#define GNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNERF_ABI_VERSION 15

/* error codes */
#define GNERF_OK            0
#define GNERF_E_ARG        -1   /* invalid argument (shape, size, null pointer, unsupported value) */
#define GNERF_E_LAUNCH     -2   /* HIP reported an error at launch */
#define GNERF_E_UNSUPPORTED -3  /* valid request, but no kernel for it (caller may use a generic path) */

/* element types of activation tensors */
#define GNERF_F32 0
#define GNERF_F16 1
#define GNERF_F64 2

typedef void* gnerf_stream_t;   /* hipStream_t */

int         gnerf_abi_version(void);
const char* gnerf_last_error(void);          /* thread-local, host pointer */
/* (ABI 9) Measurement aid: one wave samples the shader-cycle counter against the 100 MHz reference counter for `microseconds` and writes
 * out[0] = shader cycles, out[1] = reference ticks (device memory, 16 bytes): clock = out[0] / out[1] x 100 MHz.  Launch it on a side
 * stream while the kernels of interest run: the chip's clock under THAT load (bench.py's roofline quotes it). */
int gnerf_clock_sample(unsigned long long* out, double microseconds, gnerf_stream_t stream);
const char* gnerf_build_info(void);          /* e.g. "gfx950 hipcc ..." , host pointer */

/* ------------------------------------------------------------------------------------------
 * bias_act.  y = clamp(act(x + b) * gain)  and its first / second derivative forms.
 * Same contract as bias_act.cpp:36-94: x dense with `numel` elements in any memory format;
 * b has size_b elements and element i of x uses b[(i / step_b) % size_b] (step_b = stride of
 * the bias dimension); absent tensors are NULL.  grad: 0 forward (x = input),
 * 1 first order (x = dy, needs xref or yref as the activation dictates),
 * 2 second order (x = d_dx, dy = the first-order incoming gradient).
 * act: 1 linear 2 relu 3 lrelu 4 tanh 5 sigmoid 6 elu 7 selu 8 softplus 9 swish.
 * clamp < 0 disables clamping.
 * NaN: with clamp >= 0 a NaN result is returned as -clamp (the clamp is one v_med3_f32; the reference's kernel does the same,
 * bias_act.cu:143), in every native epilogue (gnerf_bias_act, gnerf_modconv_epilogue*, gnerf_torgb_nhwc*, gnerf_blur4_epilogue_nhwc); the
 * PyTorch-op forms that CPU tensors take keep the NaN. */
int gnerf_bias_act(const void* x, const void* b, const void* xref, const void* yref, const void* dy,
                   void* y, int dtype, int64_t numel, int size_b, int64_t step_b,
                   int grad, int act, float alpha, float gain, float clamp, gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The surroundings of StyleGAN2's modulated convolution (networks_stylegan2.py:41-98 modulated_conv2d, :315-334
 * SynthesisLayer.forward; the convolution itself stays MIOpen's).  SURVEY.md section 8f.3.
 *
 * gnerf_modulate_weights: out[n,o,i,k] = weight[o,i,k] * styles[n,i] * dcoef[n,o] with dcoef = rsqrt(sum_ik (weight styles)^2 + 1e-8)
 * when `demodulate` (:66-75), after the fp16 pre-normalisation of :62-64 when `prenorm` (weight[o] / (sqrt(n_in*kk) max|weight[o]|),
 * styles[n] / max|styles[n]|).  weight [n_out, n_in, kk] and styles [n, n_in] float32; out [n, n_out, n_in, kk] in out_dtype
 * (GNERF_F32 / GNERF_F16) or NULL; dcoefs [n, n_out] float32 or NULL (the un-fused form needs only these, :71-72).
 * out_layout: memory order of each sample's weights -- GNERF_W_OIK [n_out, n_in, kk] (conv2d), GNERF_W_IOK [n_in, n_out, kk]
 * (what conv_transpose2d takes: the x2-upsampling layers, conv2d_resample.py:114-123, otherwise a strided copy of all weights
 * per call), GNERF_W_OKI / GNERF_W_IKO: the channels_last memory of those two ([O,k,k,I] / [I,k,k,O]). */
#define GNERF_W_OIK 0
#define GNERF_W_IOK 1
#define GNERF_W_OKI 2
#define GNERF_W_IKO 3
int gnerf_modulate_weights(const float* weight, const float* styles, void* out, int out_dtype, float* dcoefs,
                           int n, int n_out, int n_in, int kk, int demodulate, int prenorm, int out_layout, gnerf_stream_t stream);
/* styles[n,:] / max|styles[n,:]| (the pre-normalised styles the un-fused form scales the activations with, :64 and :77). */
int gnerf_normalise_styles(const float* styles, float* out, int n, int n_in, gnerf_stream_t stream);
/* y[r, :] = x[r, :] * scale[r] for r < rows (rows = batch * channels of an NCHW tensor, row_len = H*W); the product is formed in
 * the activations' dtype like `x * styles.to(x.dtype)` (:77). */
int gnerf_scale_channels(const void* x, const float* scale, void* y, int dtype, int rows, int row_len, gnerf_stream_t stream);
/* One pass for everything after the convolution:
 *   t = x * scale[row] + noise            (un-fused demodulation + noise, fma.fma at :79-80; or `x.add_(noise)` at :96-97; rounded to
 *                                          the activations' dtype as the materialised tensor would be; skipped when both are NULL)
 *   y = clamp(act(t + bias[row % channels]) * gain)                                          (bias_act, :331-333)
 * x, y: [rows, row_len] NCHW activations (rows = batch * channels <= 65535); scale: float32 [rows] or NULL; noise: float32
 * [row_len] (or [batch, row_len] when noise_per_item: 'random' mode) or NULL, rounded to the activations' dtype first when
 * round_noise or when scale is given (the un-fused form's fma takes a noise tensor of the activations' dtype, :79-80); bias: [channels] in the activations' dtype or NULL; act: 1 linear or 3 lrelu (GNERF_E_UNSUPPORTED otherwise). */
int gnerf_modconv_epilogue(const void* x, void* y, int dtype, int rows, int row_len, int channels,
                           const float* scale, const float* noise, int noise_per_item, int round_noise, const void* bias,
                           int act, float alpha, float gain, float clamp, gnerf_stream_t stream);
/* The same three steps for CHANNELS_LAST activations (memory [n, pixels, channels]; the layout the fp16 blocks run in so that
 * MIOpen's fp16 convolutions need no transposes, and what the reference's `fp16_channels_last` produces, networks_stylegan2.py:385).
 * scale / next_scale: float32 [n, channels] or NULL; noise: float32 [pixels] (or [n, pixels] when noise_per_item) or NULL.
 * next_scale: the result, rounded to the activations' dtype, is additionally multiplied by next_scale[n, c] -- the NEXT layer's
 * `x * styles` (:77) folded into this pass (bit-identical to gnerf_modconv_epilogue_nhwc followed by gnerf_scale_channels_nhwc). */
int gnerf_scale_channels_nhwc(const void* x, const float* scale, void* y, int dtype, int n, int pixels, int channels, gnerf_stream_t stream);
int gnerf_modconv_epilogue_nhwc(const void* x, void* y, int dtype, int n, int pixels, int channels,
                                const float* scale, const float* noise, int noise_per_item, int round_noise, const void* bias,
                                int act, float alpha, float gain, float clamp, const float* next_scale, gnerf_stream_t stream);
/* The backward of the two passes above (training: the convolution between them keeps the framework's own backward).  New exports of
 * ABI 15: detect them by symbol (gnerf_hip.modconv_backward_available()), not by version.  Activations float32 / float16 as [n, channels,
 * pixels] (NCHW) or, in the _nhwc forms, [n, pixels, channels]; every reduction is accumulated in float32 without atomics in an order
 * the shape alone fixes (two runs give the same bits; an item's dx and dscale do not depend on the rest of the batch).  Every output
 * may be NULL.  workspace: gnerf_modconv_backward_workspace_bytes(...) bytes of device memory, no initialisation needed (NULL is
 * accepted when only dx is asked for).
 *   gnerf_scale_channels_backward(_nhwc): dx = round_T(dxs * T(scale[n,c])), dscale[n,c] = sum_pixels dxs * x (float32).
 *   gnerf_modconv_epilogue_backward(_nhwc): the adjoint of t = x * scale + noise, y = clamp(act(t + bias) * gain), act 1 linear or
 *     3 lrelu, with bias_act's gradient convention (the mask is read from the SAVED output: lrelu's slope by the sign of y / gain, the
 *     clamp passes where -clamp < y < clamp): g = dy * act' * gain * [inside],
 *       dx = round_T(g * T(scale[n,c])) (g without a scale), dscale[n,c] = sum_pixels g * x, dbias[c] = sum_{n,pixels} g,
 *       dnoise[pixels] (or [n, pixels] when noise_per_item) = sum_c g          (all sums float32).
 *     y may be NULL for act 1 without a clamp, x when dscale is NULL.
 * Launches: one pass over the activations (reads dy, y and -- for dscale -- x, writes dx) and up to two small finishing ones. */
int gnerf_modconv_backward_workspace_bytes(int channels_last, int dtype, int n, int channels, int pixels, size_t* bytes);
int gnerf_scale_channels_backward(const void* dxs, const void* x, const float* scale, int dtype, int n, int channels, int pixels,
                                  void* dx, float* dscale, void* workspace, gnerf_stream_t stream);
int gnerf_scale_channels_backward_nhwc(const void* dxs, const void* x, const float* scale, int dtype, int n, int pixels, int channels,
                                       void* dx, float* dscale, void* workspace, gnerf_stream_t stream);
int gnerf_modconv_epilogue_backward(const void* dy, const void* y, const void* x, const float* scale, int dtype, int n, int channels, int pixels,
                                    int noise_per_item, int act, float alpha, float gain, float clamp,
                                    void* dx, float* dscale, float* dbias, float* dnoise, void* workspace, gnerf_stream_t stream);
int gnerf_modconv_epilogue_backward_nhwc(const void* dy, const void* y, const void* x, const float* scale, int dtype, int n, int pixels, int channels,
                                         int noise_per_item, int act, float alpha, float gain, float clamp,
                                         void* dx, float* dscale, float* dbias, float* dnoise, void* workspace, gnerf_stream_t stream);
/* The 4x4 blur that follows a x2-upsampling transposed convolution (conv2d_resample.py:114-131) and the epilogue above in ONE pass over
 * channels_last activations: y = epilogue(round_T(blur(x) * blur_gain)), bit-identical to gnerf_upfirdn2d followed by
 * gnerf_modconv_epilogue_nhwc (no noise term: the layers that add noise run in NCHW float32 here).  x: [n, in_h, in_w, c] dense,
 * y: [n, out_h, out_w, c] dense, both 16-byte aligned with c filling whole 16-byte vectors; f: float32 [4,4] dense; padx0 / pady0 / flip
 * as in gnerf_upfirdn2d (up = down = 1); scale / next_scale: float32 [n, c] or NULL; bias: [c] in the activations' dtype or NULL. */
int gnerf_blur4_epilogue_nhwc(const void* x, const float* f, void* y, int dtype, int n, int c, int in_h, int in_w, int out_h, int out_w,
                              int padx0, int pady0, int flip, float blur_gain,
                              const float* scale, const void* bias, int act, float alpha, float gain, float clamp, const float* next_scale,
                              gnerf_stream_t stream);
/* (ABI 9) The 3x3 convolution of a modulated-convolution layer AND its epilogue in one launch, for float16 channels_last activations
 * in the shared-weight form (networks_stylegan2.py:41-98 as called from :315-334; the superresolution's 128 -> 128 @ 512^2 and
 * 256 -> 256 @ 256^2 layers, superresolution.py:285-303):
 *   y[n, p, o] = epilogue( half( sum_{ky,kx,c} w[o, c, ky, kx] * x[n, p + (ky - 1, kx - 1), c] ) )      zero padding, stride 1
 * with the epilogue of gnerf_modconv_epilogue_nhwc (act = lrelu; the convolution's fp32 accumulator is rounded to float16 first, as
 * a stand-alone convolution would have stored it, so the roundings match that function applied to the convolution's output).
 * x: [n, h, w, cin] float16; w_packed: [9, cout, cin] float16, tap-major (tap = ky * 3 + kx of the correlation form torch's conv2d
 * computes: w_packed[t, o, c] = weight[o, c, t / 3, t % 3]); y: [n, h, w, cout] float16; scale / next_scale: float32 [n, cout] or
 * NULL; noise: float32 [h * w] or NULL; bias: float16 [cout] or NULL; clamp < 0: none.  All 16-byte aligned.
 * w_packed's input-channel axis is cin ROUNDED UP to a multiple of 64, zero-filled (the kernel reads weights in 64-channel chunks and
 * masks the activations' missing channels).  GNERF_E_UNSUPPORTED unless h % 8 == 0, w % 32 == 0, cin % 8 == 0, cout % 128 == 0 (the caller
 * runs the two-launch form). */
int gnerf_conv3x3_epilogue_nhwc(const void* x, const void* w_packed, void* y, int n, int h, int w, int cin, int cout,
                                const float* scale, const float* noise, int round_noise, const void* bias,
                                float alpha, float gain, float clamp, const float* next_scale, gnerf_stream_t stream);
/* (ABI 11) The convolution of a block's LAST layer with the block's ToRGB taken in its epilogue -- SynthesisBlock.forward's
 * `x = conv1(x); y = torgb(x); img = img.add_(y)` (networks_stylegan2.py:452-463) where nothing else reads x (the superresolution's final block,
 * superresolution.py:285-303) -- as ONE launch that writes no x at all:
 *   img[n, o, p] += half( clamp( half( sum_c half(layer(x))[n, p, c] * rgb_w[n, o, c] ) + rgb_bias[o] ) )
 * i.e. gnerf_conv3x3_epilogue_nhwc (cout = 128, next_scale = NULL, a demodulation scale given) followed by gnerf_torgb_nhwc_accumulate, with the
 * same roundings: the layer's result is rounded to float16 where it would have been stored, the 1 x 1 products are v_dot2_f32_f16 on it.
 * rgb_w: float16 [n, 3, 128] = half(ToRGB weight[o, c] * ToRGB styles[n, c]); rgb_bias: float32 [3] (the float16 bias's values) or NULL;
 * rgb_clamp < 0: none; img: float32 [n, 3, h, w], dense, accumulated in place.  Other arguments and shape rules as gnerf_conv3x3_epilogue_nhwc. */
int gnerf_conv3x3_epilogue_torgb_nhwc(const void* x, const void* w_packed, int n, int h, int w, int cin,
                                      const float* scale, const float* noise, int round_noise, const void* bias,
                                      float alpha, float gain, float clamp,
                                      const void* rgb_w, const float* rgb_bias, float rgb_clamp, float* img, gnerf_stream_t stream);
/* (ABI 9) The stride-2 transposed 3x3 convolution of the x2 layers -- conv_transpose2d(x, w, stride = 2), what conv2d_resample.py:109-119
 * hands to the framework for up = 2 -- for float16 channels_last activations, as its four output phases on the matrix cores (the kernel
 * of gnerf_conv3x3_epilogue_nhwc with 4 / 2 / 2 / 1 of its taps; fp32 accumulation, the result rounded to float16 once).
 * x: [n, h, w, cin]; w_phases: [9, cout, cin rounded up to a multiple of 64, zero-filled] float16, the taps grouped by output phase (py, px) = (oy & 1, ox & 1):
 * (ky, kx) = (0,0), (0,2), (2,0), (2,2) | (0,1), (2,1) | (1,0), (1,2) | (1,1), with w_phases[t, o, c] = weight[c, o, ky, kx] of the transposed
 * convolution; y: [n, 2h + 1, 2w + 1, cout].  All 16-byte aligned.  GNERF_E_UNSUPPORTED unless cin % 8 == 0 and cout % 128 == 0. */
int gnerf_conv_transpose3x3_s2_nhwc(const void* x, const void* w_phases, void* y, int n, int h, int w, int cin, int cout, gnerf_stream_t stream);
/* (ABI 10) The same two convolutions in fp32-GRADE arithmetic, for the backbone's float32 layers (networks_stylegan2.py:41-98 and
 * conv2d_resample.py:48-143 on float32 activations; the reference hands them to the framework's fp32 convolution): every product x w is
 * evaluated as hi(x) hi(w) + lo(x) hi(w) + hi(x) lo(w) with hi(v) = half(v), lo(v) = half(v - hi(v)) on the f16 matrix instruction with
 * float32 accumulation -- the arithmetic of the fused renderer's decoder (dropped term and split roundings ~2^-21 relative, i.e. float32-
 * grade as long as the operands stay inside float16's RANGE: |x| < 65504) --, which for a convolution is the float16 kernel on three times
 * the input channels.
 *   gnerf_split_f16x3_nhwc: x float32 [n, pixels, channels] (channels_last), scale float32 [n, channels] or NULL -> y float16
 *     [n, pixels, 3 channels] = [hi | lo | hi] of v = x * scale (the layer's `x * styles`, :77, folded in).  channels % 8 == 0, 16-byte
 *     aligned.  |v| >= 65504 saturates to the largest finite half and sets *overflow (a device int the caller zeroed; NULL: not reported)
 *     to 1 -- the result of a convolution on such an operand is finite but wrong, and a caller that cannot bound its activations checks it.
 *   gnerf_conv3x3_f32x3_epilogue_nhwc: x3 as above with cin3 = 3 channels; w3_packed float16 [9, cout, cin3 rounded up to a multiple of 64,
 *     zero-filled] = [hi(w) | hi(w) | lo(w)] along the input-channel axis, tap-major like w_packed; bias float32 [cout] or NULL; y float32
 *     [n, h, w, cout]; epilogue operands and shape rules as gnerf_conv3x3_epilogue_nhwc (the epilogue runs in float32, nothing is rounded).
 *   gnerf_conv_transpose3x3_s2_f32x3_nhwc: likewise for the stride-2 transposed form, w3_phases in gnerf_conv_transpose3x3_s2_nhwc's tap
 *     order; y float32 [n, 2h + 1, 2w + 1, cout]. */
int gnerf_split_f16x3_nhwc(const float* x, const float* scale, void* y, int n, int pixels, int channels, int* overflow, gnerf_stream_t stream);
int gnerf_conv3x3_f32x3_epilogue_nhwc(const void* x3, const void* w3_packed, float* y, int n, int h, int w, int cin3, int cout,
                                      const float* scale, const float* noise, const float* bias,
                                      float alpha, float gain, float clamp, const float* next_scale, gnerf_stream_t stream);
int gnerf_conv_transpose3x3_s2_f32x3_nhwc(const void* x3, const void* w3_phases, float* y, int n, int h, int w, int cin3, int cout, gnerf_stream_t stream);
/* ToRGBLayer with three output channels on a channels_last float16 tensor (networks_stylegan2.py:349-367, modulation as in the
 * fused form :89-96): y[n, o, p] = clamp(half(sum_c x[n, p, c] * half(weight[o, c] * styles[n, c])) + bias[o]), products exact, fp32
 * accumulation.  x: float16 [n, pixels, channels] (channels 32, 64, 128, 256 or 512, 16-byte aligned); weight float32 [3, channels];
 * styles float32 [n, channels] (weight_gain already applied, :364); bias float16 [3] or NULL; y: float16 [n, 3, pixels] (NCHW: it is
 * added to the running image); clamp < 0 = none.  One streaming read of x instead of scale pass + 1x1 convolution + bias pass. */
int gnerf_torgb_nhwc(const void* x, const float* weight, const float* styles, const void* bias, void* y,
                     int n, int pixels, int channels, float clamp, gnerf_stream_t stream);
/* (ABI 7) The same layer ADDED to the block's running image instead of stored: img[n, o, p] += float(y[n, o, p]) with y as above
 * (rounded to float16 first), img float32 [n, 3, pixels] dense -- `img.add_(y.to(torch.float32))` of the 'skip' architecture
 * (networks_stylegan2.py:461-463) without materialising y or converting it: two launches fewer per block. */
int gnerf_torgb_nhwc_accumulate(const void* x, const float* weight, const float* styles, const void* bias, float* img,
                                int n, int pixels, int channels, float clamp, gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * upfirdn2d.  Zero-insert upsample, pad/crop, 2-D FIR, decimate (upfirdn2d.cpp:20-102).
 * x: [n, c, in_h, in_w] with element strides xs[4] = {stride_n, stride_c, stride_h, stride_w}
 * (NCHW and channels_last both allowed); y likewise with ys[4]; f: float32 [fh, fw] with
 * element strides fs[2] = {stride_h, stride_w}.
 * out_h = (in_h*upy + pady0 + pady1 - fh + downy) / downy, out_w likewise; the caller
 * allocates y with that shape (only pad*0 is needed by the kernel). */
int gnerf_upfirdn2d(const void* x, const float* f, void* y, int dtype,
                    int n, int c, int in_h, int in_w, const int64_t xs[4],
                    int fh, int fw, const int64_t fs[2],
                    int out_h, int out_w, const int64_t ys[4],
                    int upx, int upy, int downx, int downy, int padx0, int pady0,
                    int flip, float gain, gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * filtered_lrelu_act_: in-place gain * lrelu * clamp on x [n,c,h,w] (strides xs) with the
 * bit-packed 2-bit sign tensor (1 = negative, 2 = clamped; 4 pixels per byte, row pitch
 * s_w/4 bytes, s_w a multiple of 16) -- filtered_lrelu.cpp:217-294.
 * mode: 0 no signs, 1 write signs to s, 2 read signs from s (then x *= per-sign factor).
 * sx, sy: offset of x inside the sign tensor. */
int gnerf_filtered_lrelu_act(void* x, uint8_t* s, int dtype, int n, int c, int h, int w,
                             const int64_t xs[4], int s_h, int s_w, int sx, int sy,
                             float gain, float slope, float clamp, int mode, gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * filtered_lrelu, fused (filtered_lrelu.cpp:20-213): y = downfir(clamp(lrelu(upfir(x + b) * up^2 * gain))) in one
 * launch.  x: [n, c, xh, xw] float16/float32 with element strides xs[4]; b: [c], same dtype, contiguous;
 * fu, fd: float32 filters with fu_taps / fd_taps taps per axis, contiguous; *_rank 1 = separable (applied along
 * both axes), 2 = a 1x1 rank-2 filter (applied once).  y: [n, c, yh, yw] (strides ys) allocated by the caller with
 * yw = (xw*up + px0 + px1 - (fu_taps-1) - (fd_taps-1) + down-1) / down (only px0 / py0 are needed here).
 * Signs: s is the bit-packed tensor of gnerf_filtered_lrelu_act ([n, c, s_h, s_w/4] bytes), sign_mode 0 none,
 * 1 write (s_h = yh*down-(down-1)+fd_taps-1 rows, forward pass), 2 read (gradient pass: slope / zero factors come
 * from s at offset (sx, sy), values outside s pass through with the gain only).
 * Returns GNERF_E_UNSUPPORTED when no fused kernel covers the configuration (resampling factors other than
 * 1/2/4, more than 8 taps per polyphase branch, non-separable filters, float64): the caller then composes
 * gnerf_upfirdn2d + gnerf_filtered_lrelu_act + gnerf_upfirdn2d, which is what the reference does on return code -1
 * (filtered_lrelu.cpp:55-60, filtered_lrelu.py:225-231). */
int gnerf_filtered_lrelu(const void* x, const float* fu, const float* fd, const void* b, uint8_t* s, void* y,
                         int dtype, int n, int c, int xh, int xw, const int64_t xs[4],
                         int yh, int yw, const int64_t ys[4],
                         int fu_taps, int fu_rank, int fd_taps, int fd_rank,
                         int up, int down, int px0, int py0,
                         int s_h, int s_w, int sx, int sy, int sign_mode,
                         float gain, float slope, float clamp, int flip, gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bilinear 2-D grid sampling (mode bilinear, zero padding, align_corners = False): what grid_sample_gradfix.grid_sample
 * evaluates upstream through torch.nn.functional.grid_sample (grid_sample_gradfix.py:45) and, in the backward,
 * aten::grid_sampler_2d_backward (grid_sample_gradfix.py:62-77).
 * image: [n, c, h, w] float16/float32 with element strides image_strides[4]; grid: [n, ho, wo, 2] float32 contiguous,
 * (x, y) in [-1, 1]; out: [n, c, ho, wo] contiguous, image's dtype. */
int gnerf_grid_sample_2d(const void* image, const float* grid, void* out, int dtype,
                         int n, int c, int h, int w, const int64_t image_strides[4], int ho, int wo, gnerf_stream_t stream);
/* The adjoint.  grad_out: [n, c, ho, wo] contiguous, image's dtype.  grad_image: float32 [n, c, h, w] contiguous or NULL;
 * grad_grid: float32 [n, ho, wo, 2] or NULL (needs image).  Both are ACCUMULATED into (the caller zeroes them). */
int gnerf_grid_sample_2d_backward(const void* grad_out, const void* image, const float* grid, float* grad_image, float* grad_grid,
                                  int dtype, int n, int c, int h, int w, const int64_t image_strides[4], int ho, int wo,
                                  gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Tri-plane layout change: NCHW float32 [np, c, h, w] -> NHWC [np, h, w, c] (np = 3*batch).
 * The renderer reads whole 128-byte texels (32 channels) from the NHWC copy. */
int gnerf_planes_to_nhwc(const float* planes_nchw, float* planes_nhwc, int np, int c, int h, int w,
                         gnerf_stream_t stream);
/* The same layout change, also measuring max |planes| on the way (the planes are read anyway): *absmax (one device
 * float, overwritten) feeds gnerf_render_params.planes_absmax.  A NaN anywhere in the planes makes *absmax NaN.
 * workspace: this stream's render workspace (gnerf_render_workspace_bytes(), zeroed once; every call leaves it zeroed, as
 * gnerf_render_forward does); calls on different streams need different workspaces. */
int gnerf_planes_to_nhwc_stats(const float* planes_nchw, float* planes_nhwc, int np, int c, int h, int w,
                               float* absmax, void* workspace, gnerf_stream_t stream);
/* max |x| over `numel` floats (any layout) -> *absmax (one device float, overwritten). */
int gnerf_planes_absmax(const float* planes, int64_t numel, float* absmax, gnerf_stream_t stream);
/* The tri-plane producer's last step, writing the renderer's layout directly (no layout change afterwards):
 *   out = upfirdn2d(img, f, up=2, padding=[2,1,2,1], gain) + y          (networks_stylegan2.py:456-463, upfirdn2d.py:315-350)
 * img [n, c, h, w] float32 NCHW contiguous; y [n, c, 2h, 2w] float32 NCHW contiguous or NULL; f_host: the 4x4 filter, 16 floats
 * in HOST memory (row-major; flipped inside unless `flip`, like gnerf_upfirdn2d); out: [n, 2h, 2w, c] = channels_last memory of
 * [n, c, 2h, 2w], i.e. for c = 96 the interleaved plane layout (gnerf_render_params.planes_interleaved = 1).
 * absmax: optional device float receiving max |out| (gnerf_render_params.planes_absmax).
 * Returns GNERF_E_UNSUPPORTED unless c % 32 == 0, w % 16 == 0 and h % 2 == 0. */
int gnerf_upsample2x_add_nhwc(const float* img, const float* y, const float* f_host, int flip, float gain, float* out,
                              int n, int c, int h, int w, float* absmax, gnerf_stream_t stream);
/* The inverse, NHWC [np, h, w, c] -> NCHW [np, c, h, w]: hands gnerf_render_backward's plane gradient back in the layout
 * of the reference's planes (triplane.py:74). */
int gnerf_planes_from_nhwc(const float* planes_nhwc, float* planes_nchw, int np, int c, int h, int w,
                           gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Ray generation (ray_sampler.py:24-63): cam2world [n,4,4], intrinsics [n,3,3] row-major ->
 * origins, dirs [n, res*res, 3]; ray m = row*res + col looks through pixel centre
 * ((col+.5)/res, (row+.5)/res). */
/* Frame conversion of the video writer (gen_videos.py:173 and the permute in front of it): out[n, y, x, ch] =
 * uint8(clamp(img[n, ch, y, x] * 127.5 + 128, 0, 255)), product and sum rounded separately, truncating cast, NaN -> 0.
 * img float32 [n, c, h, w] dense, out uint8 [n, h, w, c] dense, 1 <= c <= 64.  One launch instead of four elementwise passes. */
int gnerf_to_uint8_nhwc(const float* img, unsigned char* out, int n, int c, int h, int w, gnerf_stream_t stream);

int gnerf_make_rays(const float* cam2world, const float* intrinsics, int n, int res,
                    float* origins, float* dirs, gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The fused renderer (renderer.py:88-140 with MipRayMarcher2, ray_marcher.py:25-57, and the
 * OSGDecoder MLP, triplane.py:113-136, inside).  One launch does, per ray: stratified depth
 * proposals, tri-plane bilinear lookups, the 32->64->33 MLP on the matrix cores, the coarse
 * ray march, importance resampling, the fine pass, the depth merge and the final composite.
 */
typedef struct gnerf_render_params {
    /* planes, NHWC float32 [n_items*3, plane_h, plane_w, 32] (see gnerf_planes_to_nhwc) */
    const float* planes_nhwc;
    int32_t n_items, plane_h, plane_w;
    /* rays: [n_items, rays_per_item, 3] float32 each */
    const float* ray_origins;
    const float* ray_dirs;
    int32_t rays_per_item;
    int32_t image_width;        /* >0: rays of an item form a row-major image of this width (locality hint only) */
    /* decoder: EFFECTIVE weights (FullyConnectedLayer gains folded in, networks_stylegan2.py:118-127),
       row-major w1 [64,32], b1 [64], w2 [33,64], b2 [33]; output 0 is the density */
    const float* w1; const float* b1; const float* w2; const float* b2;
    /* sampling options (rendering_kwargs, renderer.py:91-116) */
    int32_t depth_resolution;             /* coarse samples per ray, 2..GNERF_MAX_SAMPLES */
    int32_t depth_resolution_importance;  /* fine samples per ray, 0..GNERF_MAX_SAMPLES */
    float   ray_start, ray_end;           /* used when ray_start_per_ray is NULL */
    const float* ray_start_per_ray;       /* optional [n_items*rays_per_item] ('auto' box limits, renderer.py:93-98) */
    const float* ray_end_per_ray;
    float   box_warp;
    int32_t white_back;                   /* ray_marcher.py:52-53 */
    int32_t disparity_space_sampling;     /* renderer.py:174-181 */
    /* uniform [0,1) draws, in the reference's order: noise_coarse = rand_like([n,m,S,1]) as [n*m, S],
       noise_fine = rand(n*m, F) (renderer.py:190 and :241).  noise_fine may be NULL iff F == 0 */
    const float* noise_coarse;
    const float* noise_fine;
    /* outputs */
    float* out_rgb;      /* [n_items, rays_per_item, 32]  in (-1,1) */
    float* out_depth;    /* [n_items, rays_per_item, 1] */
    float* out_wsum;     /* [n_items, rays_per_item, 1]   sum of the final weights */
    /* workspace of gnerf_render_workspace_bytes() bytes (holds the call-wide depth range used by the
       global clamp of ray_marcher.py:49-50, or one range per item: depth_clamp_per_item).  ZERO it once after allocation;
       every call leaves it zeroed.  (ABI 14) It also holds the pipelined kernel's eight ray-dealing counters, and is larger for it.
       One workspace per stream that renders concurrently. */
    void*  workspace;
    /* optional stage dump for debugging/parity: float32 [n*m, GNERF_DEBUG_SLOTS, S+F]; NULL in production */
    float* debug;
    /* Decoder arithmetic (the reference's decoder is fp32 addmm, triplane.py:124-136 / networks_stylegan2.py:121-134).
       GNERF_MLP_F32: exact fp32 products on v_mfma_f32_16x16x4_f32, any finite input.
       GNERF_MLP_F16X3: each product as an error-compensated f16 hi/lo split on v_mfma_f32_16x16x32_f16 (fp32-grade, 1.6x
       faster) -- only valid while features, weights and hidden activations are inside f16's range.
       GNERF_MLP_AUTO (0, default): decided ON THE DEVICE per call from max |planes| and the decoder's weights (bounds
       in DESIGN.md section 2.1): out-of-range or ill-conditioned inputs take the fp32 path, so results never depend on
       f16's range.  (AUTO's f16 body also evaluates softplus as log2(1 + 2^p') when the same norms keep every pre-activation
       below exp2's overflow, and in the form that is safe for any p' otherwise -- as a forced GNERF_MLP_F16X3 always does: the
       two forms differ by fp32 rounding.)  planes_absmax: one device float from gnerf_planes_to_nhwc_stats / gnerf_planes_absmax /
       gnerf_upsample2x_add_nhwc; NULL makes the AUTO launcher measure it itself (one extra pass over the planes).
       CONTRACT of a caller-supplied planes_absmax: at the time the render kernel runs (stream order) the float must be
       >= max |planes_nhwc| of THIS call's planes -- an upper bound is fine (it only sends more calls to the fp32 body, or to
       the f16 body's overflow-safe softplus form: the same values up to fp32 rounding), a
       value that is too small (a stale measurement of other or since-modified planes) is NOT detected: the f16x3 body then
       runs on features outside the range its bounds were checked for and can return inf / NaN or lose its fp32-grade
       accuracy.  NaN or +inf there selects the fp32 body.  Debug aid: with the environment variable GNERF_VERIFY_ABSMAX=1
       gnerf_render_forward measures max |planes| itself, synchronises the stream, and fails with GNERF_E_ARG when the
       supplied value is smaller (a test-suite switch: it costs a pass over the planes and a host round trip per call).
       The kernels that always compute in fp32 (more than 144+144 samples or no importance pass beyond 96 samples: the generic
       kernel, gnerf_query_points, both backward passes) ignore these two fields. */
    const float* planes_absmax;
    int32_t mlp_mode;
    /* Layout of `planes_nhwc` (and of gnerf_render_grads.grad_planes_nhwc, which always mirrors it):
       0: [n_items*3, plane_h, plane_w, 32]  one NHWC image per plane (what gnerf_planes_to_nhwc makes);
       1: [n_items, plane_h, plane_w, 96]    the three planes of an item interleaved per texel = the channels_last memory of the
          backbone's own [n_items, 96, plane_h, plane_w] output (triplane.py:69-74), plane p = channels 32p..32p+31.  A
          producer that writes channels_last (gnerf_upsample2x_add_nhwc) feeds the renderer with no layout change at all. */
    int32_t planes_interleaved;
    /* (ABI 6) Batching several views of ONE scene in a call -- gen_videos.py's orbit renders every frame from the same planes:
       planes_shared = 1: `planes_nhwc` holds ONE item's planes ([3,h,w,32] or [1,h,w,96]) and every item of the call reads them
         (n_items still counts the items = views of the call: rays, noise and outputs are per item).  Forward only.
       depth_clamp_per_item = 1: the depth clamp of ray_marcher.py:49-50 (min / max sample depth of the whole forward call) is taken
         per ITEM instead of over the call, so that an item's result does not depend on what it is batched with: a batch of k views
         equals k calls of one view bit for bit.  0 (default): the reference's call-wide clamp.  n_items <= 4096 when set. */
    int32_t planes_shared;
    int32_t depth_clamp_per_item;
    /* (ABI 8) Rays and uniform draws made INSIDE the render kernel (SURVEY.md section 8a row 1 / 8d "in-kernel Philox"): the call then
       reads no ray tensors and no noise tensors (26.7 MB per 65 536 rays at 48+48) and needs no launch in front of it.
       cam2world / intrinsics: [n_items,4,4] and [n_items,3,3] row-major device floats, used when ray_origins == ray_dirs == NULL.
         Ray m of an item looks through pixel centre ((m % w + .5) / w, (m / w + .5) / w), w = image_width, which must be > 0 with
         rays_per_item == w * w: the arithmetic of gnerf_make_rays (ray_sampler.py:24-63), same bits.
       rng_mode = GNERF_RNG_TORCH_PHILOX: noise_coarse / noise_fine must be NULL; the kernel draws what torch's device generator
         would have put into them -- `torch.rand_like([n,m,S,1])` then `torch.rand(n*m, F)` (renderer.py:190,241) -- Philox4x32-10
         keyed by rng_seed, element li of a draw taken from thread li % threads of ATen's grid-stride kernel at the generator's
         philox offset (oracle/philox_ref.py states the recipe; gnerf_torch_rand_plan gives threads and the offset increment of a
         draw).  rng_offset_coarse / rng_offset_fine: philox offset of the generator BEFORE the respective draw (multiples of 4).
         The caller advances its generator by the two increments afterwards, exactly as the two torch.rand calls would have.
       rng_per_item = 1: the draws are per ITEM instead of per call (what n_items separate calls with one item each would draw:
         the batched views of planes_shared): element indices count inside the item, and item i's offsets are
         rng_offset_* + i * rng_offset_item_stride.
       Supported by the pipelined kernels at their compile-time sample counts (48+48 and 96+96, no disparity sampling, no per-ray
       limits, no stage dump): anything else returns GNERF_E_UNSUPPORTED and the caller passes tensors.  Forward only. */
    const float* cam2world;
    const float* intrinsics;
    int32_t  rng_mode;
    int32_t  rng_per_item;
    uint64_t rng_seed;
    uint64_t rng_offset_coarse, rng_offset_fine, rng_offset_item_stride;
    uint32_t rng_threads_coarse, rng_threads_fine;
    /* (ABI 10) density noise (renderer.py:146-147: `sigma += randn_like(sigma) * density_noise` in run_model, i.e. once on the coarse
       pass's densities and once on the fine pass's, before either ray march): the two tensors ALREADY multiplied by density_noise,
       float32 [n_items * rays_per_item, depth_resolution] and [.., depth_resolution_importance], or NULL (off).  Forward only
       (gnerf_render_backward returns GNERF_E_UNSUPPORTED); not with in-kernel rays / draws. */
    const float* sigma_noise_coarse;
    const float* sigma_noise_fine;
} gnerf_render_params;

#define GNERF_RNG_TENSORS      0
#define GNERF_RNG_TORCH_PHILOX 1

/* Launch geometry of ATen's uniform kernel for a draw of `numel` floats on a device whose torch properties are
 * multi_processor_count / max_threads_per_multi_processor: *threads = 256 * min(ceil(numel / 256), mpc * (mtpm / 256)) and
 * *offset_increment = 4 * ceil(numel / (4 * threads)), what the generator's philox offset advances by.  Host-only arithmetic. */
int gnerf_torch_rand_plan(int64_t numel, int multi_processor_count, int max_threads_per_multi_processor,
                          uint32_t* threads, uint64_t* offset_increment);
/* The draw itself as a stand-alone kernel: out[i] = element i of torch.rand(numel) at (seed, offset) -- the same device function the
 * render kernels use, exposed so that it can be held to torch.rand directly (tests) and for callers that want tensors. */
int gnerf_torch_rand(float* out, int64_t numel, uint64_t seed, uint64_t offset, uint32_t threads, gnerf_stream_t stream);
/* (ABI 10) The rays of gnerf_make_rays AND the renderer's two uniform draws in one launch: draw_a / draw_b = what torch.rand(numel_a) then
 * torch.rand(numel_b) return with the device generator at seed and philox offsets offset_a / offset_b (threads_* from gnerf_torch_rand_plan;
 * the caller advances its generator by the two increments, as for gnerf_render_params.rng_mode).  draw_b may be NULL.  One Philox block per
 * four elements, ATen's own thread-to-element map: the same values as gnerf_torch_rand, i.e. as torch.rand, bit for bit. */
int gnerf_make_rays_and_draws(const float* cam2world, const float* intrinsics, int n, int res, float* origins, float* dirs,
                              float* draw_a, int64_t numel_a, uint64_t offset_a, uint32_t threads_a,
                              float* draw_b, int64_t numel_b, uint64_t offset_b, uint32_t threads_b, uint64_t seed, gnerf_stream_t stream);

#define GNERF_MLP_AUTO  0
#define GNERF_MLP_F16X3 1
#define GNERF_MLP_F32   2

#define GNERF_MAX_SAMPLES   256
#define GNERF_DEBUG_SLOTS   8
/* debug slots */
#define GNERF_DBG_DEPTH_COARSE 0
#define GNERF_DBG_SIGMA_COARSE 1
#define GNERF_DBG_WEIGHT_COARSE 2
#define GNERF_DBG_DEPTH_FINE   3
#define GNERF_DBG_SIGMA_FINE   4
#define GNERF_DBG_DEPTH_SORTED 5
#define GNERF_DBG_SIGMA_SORTED 6
#define GNERF_DBG_WEIGHT_FINAL 7

size_t gnerf_render_workspace_bytes(void);
int    gnerf_render_forward(const gnerf_render_params* p, gnerf_stream_t stream);

/* Gradient of the renderer: what autograd computes upstream by walking the graph of
 * renderer.py:88-140 backwards (grid_sample_gradfix.py's backward op for the planes, the decoder's
 * linear layers, ray_marcher.py's composite).  The forward pass is recomputed per ray from the same
 * params (same noise), nothing is saved between the two calls.  Importance depths are constants, as
 * upstream (renderer.py:198 no_grad / :211 detach); rays and noise get no gradient.
 * All output buffers are ACCUMULATED into (the caller zeroes them, or keeps summing across calls). */
typedef struct gnerf_render_grads {
    const float* grad_rgb;      /* [n_items, rays_per_item, 32] or NULL (= zeros) */
    const float* grad_depth;    /* [n_items, rays_per_item, 1]  or NULL */
    const float* grad_wsum;     /* [n_items, rays_per_item, 1]  or NULL */
    float* grad_planes_nhwc;    /* [n_items*3, plane_h, plane_w, 32] or NULL (skip) */
    float* grad_w1;             /* [64,32]; the four decoder gradients are given together or all NULL */
    float* grad_b1;             /* [64] */
    float* grad_w2;             /* [33,64] */
    float* grad_b2;             /* [33] */
    /* Optional workspace (contents irrelevant before and after the call; 256-byte aligned).  The struct carries no size field: what the
       buffer must hold follows from the request, and the call trusts that it was sized by the matching function for the SAME params:
         * with grad_planes_nhwc: gnerf_render_backward_stage_bytes(p) bytes; the plane gradient is made in two passes.  Layout: [rays * (S + F)] rows of 33
           floats (32 feature gradients in the ray's depth order + one spare), one spare 256-byte line, then (ABI 9) the binned
           scatter's workspace: per-plane-tile counts / starts / scales / order, the record arrays (8 + 16 bytes per (sample, plane)
           record) and the tile halos.  The second pass sums every 16 x 16-texel plane tile in LDS in 64-bit fixed point and writes it
           with plain stores -- no float atomics, bit-identical gradients from run to run (GNERF_BWD_SCATTER=sorted selects round 4's
           LDS-merged atomic pass instead, which uses only the rows).  Precision of the fixed-point sum: with n_t records in a tile
           (nbits = ceil(log2 n_t)) and B the largest |row value| among them, a texel that n records reach is within
           n * 129 * 2^(nbits - 60) * B of the exact sum of its float32 products before its one rounding to float32 (129: the conversion
           of a negative product of less than 2^32 units is off by up to 128 units, the floor adds one); products of at least
           2^(nbits - 27) * B convert exactly;
         * without grad_planes_nhwc (decoder gradients only): gnerf_render_backward_exchange_bytes(p) bytes suffice (below): per sample
           depth, colour weight, dL/dsigma.
       NULL: single pass (one float atomic per tap and channel). */
    float* scatter_stage;
} gnerf_render_grads;

size_t gnerf_render_backward_stage_bytes(const gnerf_render_params* p);
/* (ABI 8) A decoder-only request (grad_planes_nhwc NULL) may pass a much smaller buffer of this many bytes as scatter_stage: what the
 * backward's two kernels on the pipelined path exchange per sample (depth, colour weight, dL/dsigma).  Without it such a request
 * runs the one-wave-per-ray kernel. */
size_t gnerf_render_backward_exchange_bytes(const gnerf_render_params* p);

/* p: the forward call's params (outputs, workspace and debug are ignored). */
int gnerf_render_backward(const gnerf_render_params* p, const gnerf_render_grads* g, gnerf_stream_t stream);

/* gnerf_render_backward plus the gradient with respect to the RAYS (added without a new ABI version: no existing signature or struct
 * changes): grad_origins, grad_dirs [n_items, rays_per_item, 3] float32, every element WRITTEN (nothing accumulated); either may be
 * NULL, not both.  Everything gnerf_render_backward does for (p, g) is done as there, with the same launches.
 * With numeric ray_start / ray_end the coarse depths do not depend on the rays, the importance depths are constants and the decoder
 * ignores directions, so the rays act through the sample positions p_k = o + t_k d only:
 *     dL/do = sum_k dL/dp_k      dL/dd = sum_k t_k dL/dp_k      dL/dp_k = J_k^T dX_k
 * dX_k = dL/d(mean feature) of sample k (the staged first pass's rows), J_k the position derivative of the three lookups exactly as
 * in gnerf_query_points_grad above (steps 3 and 4).  One kernel (csrc/render_ray_grad.inl) between the first pass and the scatter, a
 * wave per ray, no atomics: bit-reproducible, and the same bits with or without the other gradients.
 * g->scatter_stage must hold gnerf_render_backward_stage_bytes(p) bytes -- also when g->grad_planes_nhwc is NULL (frozen planes: the
 * rows are staged, the scatter is skipped); the decoder gradients stay optional.
 * GNERF_E_UNSUPPORTED, before any launch: scatter_stage NULL (the single-pass form stages nothing; GNERF_BWD_SCATTER=direct likewise);
 * per-ray limits (ray_start_per_ray: the coarse depths then depend on the rays); and what gnerf_render_backward refuses (density
 * noise, in-kernel rays / draws, planes_shared).  The call cannot tell a buffer of exchange size from one of stage size: the caller
 * sizes it. */
int gnerf_render_backward_rays(const gnerf_render_params* p, const gnerf_render_grads* g, float* grad_origins, float* grad_dirs, gnerf_stream_t stream);

/* The SECOND pass of the staged backward alone (added without a new ABI version, like gnerf_render_backward_rays): the plane gradient
 * of rows and depths the caller wrote, for tests and tools that hold the scatter to a reference of its own.
 * p: params as for gnerf_render_backward; the scatter reads the rays, the sample counts (n_all = depth_resolution +
 * depth_resolution_importance), the plane shape and layout, box_warp and image_width, and dereferences nothing else of it.
 * stage: gnerf_render_backward_stage_bytes(p) bytes, 256-byte aligned.  Its front holds, per ray, n_all depths and then n_all rows of 32
 * floats (dL/d(mean feature) of the sample at that depth) -- what the staged first pass leaves, ray stride 33 n_all floats; the rest is
 * the call's workspace.  Sample k of ray r adds w_tap * row to the four texels of its bilinear footprint (zero padding, align_corners =
 * false, w_tap with the 1/3 of the plane mean) in each of the three planes, at p = (o + t d) * 2 / box_warp.
 * grad_planes_nhwc is ACCUMULATED into, laid out as p's planes.
 * The scatter is chosen as gnerf_render_backward chooses it: the binned fixed-point form where it covers the call, GNERF_BWD_SCATTER=sorted
 * the LDS-merged atomic form; a ragged call of several items walks the padded ray sequence.  GNERF_E_UNSUPPORTED, before any launch:
 * what gnerf_render_backward refuses, GNERF_BWD_SCATTER=direct, and ragged calls the padded binned form does not cover. */
int gnerf_render_scatter_rows(const gnerf_render_params* p, float* stage, float* grad_planes_nhwc, gnerf_stream_t stream);

/* The decoder pack (added without a new ABI version, like gnerf_render_backward_rays).
 * Before its first ray every workgroup of the pipelined render kernels reduces the decoder's range statistics (which pick the decoder
 * arithmetic under GNERF_MLP_AUTO) and rewrites the weights into their LDS layout.  Both depend on the decoder alone, and a decoder is
 * the same from call to call between two optimizer steps.  gnerf_render_pack_decoder does that work ONCE, in one small launch (one
 * workgroup), into `pack`: gnerf_render_decoder_pack_bytes() bytes of device memory, 16-byte aligned, holding the statistics and the LDS
 * image of either arithmetic.  gnerf_render_forward_packed is gnerf_render_forward for a caller that has a pack of p's CURRENT w1, b1,
 * w2, b2: a workgroup then evaluates the same inequalities on the stored statistics and copies the image it needs.  Same results bit
 * for bit, same choice of arithmetic.  A pack made of other weight values than p's gives the other weights' results: the caller remakes
 * it when the weights change (gnerf_hip.render_forward keeps a small cache keyed on the tensors' versions, and packs a decoder the second
 * time it sees it: making a pack costs more than one call gains).  p->w1 .. p->b2 must still
 * be given: kernels that do not read a pack (the generic kernel) use them.  The pack is only read by the call, so one pack serves any
 * number of calls, streams permitting.  A call captured into a graph keeps the pack's ADDRESS: its owner keeps that memory alive and
 * unchanged for as long as the graph is replayed, and every replay renders with the weights the pack was made of, whatever w1 .. b2 hold by
 * then (a captured gnerf_render_forward reads them at replay time).  gnerf_hip.render_forward therefore hands no pack of its cache to a
 * captured call. */
size_t gnerf_render_decoder_pack_bytes(void);
int gnerf_render_pack_decoder(const float* w1, const float* b1, const float* w2, const float* b2, void* pack, gnerf_stream_t stream);
int gnerf_render_forward_packed(const gnerf_render_params* p, const void* pack, gnerf_stream_t stream);

/* Density / colour of arbitrary points (run_model, renderer.py:142-148; used by
 * TriPlaneGenerator.sample / sample_mixed for shape extraction):
 * points [n_items, n_points, 3] -> sigma [n_items, n_points, 1], rgb [n_items, n_points, 32].
 * out_rgb may be NULL: densities only (the 512^3 shape extraction of gen_videos.py:189-224 reads nothing else).
 * planes_interleaved: layout of planes_nhwc, as gnerf_render_params.planes_interleaved.
 * n_points <= (INT32_MAX - 15) / 3 = 715 827 877 per item, for this call and for the two gradients below: the kernels index a point's
 * three coordinates and a tile's 16 points in int.  A larger n_points is GNERF_E_ARG ("too many points"), checked before the pointers. */
int gnerf_query_points(const float* planes_nhwc, int n_items, int plane_h, int plane_w,
                       const float* points, int n_points, float box_warp,
                       const float* w1, const float* b1, const float* w2, const float* b2,
                       float* out_sigma, float* out_rgb, int planes_interleaved, gnerf_stream_t stream);

/* Gradient of gnerf_query_points: grad_sigma [n_items, n_points, 1] and grad_rgb [n_items, n_points, 32] (either may be
 * NULL) -> ACCUMULATED into grad_planes_nhwc and the four decoder gradients (same conventions as gnerf_render_backward).
 * Points get no gradient.  Upstream: autograd through renderer.py:142-148 (sample_mixed in the density regulariser). */
int gnerf_query_points_backward(const float* planes_nhwc, int n_items, int plane_h, int plane_w,
                                const float* points, int n_points, float box_warp,
                                const float* w1, const float* b1, const float* w2, const float* b2,
                                const float* grad_sigma, const float* grad_rgb,
                                float* grad_planes_nhwc, float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2,
                                int planes_interleaved, gnerf_stream_t stream);

/* Gradient of gnerf_query_points with respect to the POINTS (added without a new ABI version: no existing signature or struct
 * changes): grad_sigma [n_items, n_points, 1] and grad_rgb [n_items, n_points, 32] (either may be NULL, not both) ->
 * grad_points [n_items, n_points, 3] float32, every element WRITTEN (nothing accumulated, no zeroing needed).  Per point:
 *   1. forward: the three lookups (planes read (x,y), (x,z), (z,x) of 2 p / box_warp), their mean, the decoder;
 *   2. decoder backward to dX[32] = dL/d(mean feature): rgb = 1.002 sigmoid(o) - 0.001, the sigma row, layer 2^T, softplus' = sigmoid,
 *      layer 1^T (the colour half is skipped when grad_rgb is NULL: normals of the density field);
 *   3. per plane k with pixel coordinates (ix, iy), fractions (fx, fy) and taps t00 t10 t01 t11 (first index x; a tap outside
 *      the image is zero; floor has its one-sided derivative, as in grid_sample with zero padding and align_corners=False):
 *        df/dix = (t10 - t00)(1 - fy) + (t11 - t01) fy        df/diy = (t01 - t00)(1 - fx) + (t11 - t10) fx
 *        gu_k = (W/2)(1/3) sum_c dX[c] df_c/dix               gv_k = (H/2)(1/3) sum_c dX[c] df_c/diy
 *   4. grad_points = (2 / box_warp) (gu_0 + gu_1 + gv_2,  gv_0,  gv_1 + gu_2).
 * Exact fp32 products (any finite planes), no atomics: bit-reproducible.  GNERF_E_UNSUPPORTED when one item's planes exceed 32-bit
 * tap offsets (as gnerf_query_points_backward); GNERF_E_ARG for null pointers, n_points < 1 or both gradients NULL.
 * Upstream: autograd through renderer.py:142-148 with sample_coordinates.requires_grad. */
int gnerf_query_points_grad(const float* planes_nhwc, int n_items, int plane_h, int plane_w,
                            const float* points, int n_points, float box_warp,
                            const float* w1, const float* b1, const float* w2, const float* b2,
                            const float* grad_sigma, const float* grad_rgb, float* grad_points,
                            int planes_interleaved, gnerf_stream_t stream);

/* (ABI 15, added without a new version) Newton projection of points onto the level set sigma = level of gnerf_query_points' density, with
 * the gradient of gnerf_query_points_grad (grad_sigma = 1, no colour half) -- one launch (csrc/project_level.inl) for all steps.
 *   points [n_items, n_points, 3] float32; affine: float32 [12] ON THE HOST (read during the call), a row-major 3x4 [A | b] with world = A p + b (b = affine[3], [7],
 *   [11]), or NULL for the identity (no arithmetic at all then); max_steps K >= 0; radius r >= 0 in the points' own frame; tol > 0 in
 *   sigma units.  Per point, independent of every other point (tile, batch and position do not matter), all in float32:
 *     p = p0
 *     for k = 0 .. K:
 *         s, g_world = sigma and grad sigma at A p + b
 *         e = s - level (NaN when A p + b has a non-finite coordinate);  if k == 0: residual_in = e
 *         if e is not finite:  status = 2; break
 *         if |e| <= tol:       status = 0; break            (converged; the point takes no further step)
 *         if k == K:           status = 1; break            (not converged)
 *         g = A^T g_world                                   (a covector)
 *         gg = (g0 g0 + g1 g1) + g2 g2;  if gg is not > 0 or not finite: status = 2; break       (flat)
 *         q = p - (e / gg) g                                (the nearest point of the linearised level set)
 *         p = min(max(q, p0 - r), p0 + r) per axis          (a trust box around the START; a NaN q takes the box's lower face)
 *     points_out   = status == 0 ? p : p0                   (the input's bits when not converged)
 *     residual_out = status == 0 ? e : residual_in
 *   points_out [n_items, n_points, 3], residual_in / residual_out float32 [n_items, n_points], status uint8 [n_items, n_points]: every
 *   element WRITTEN.  points_out may be points.  Plain stores, no atomics: bit-reproducible.
 * GNERF_E_ARG for null pointers (affine excepted), n_points < 1 or beyond gnerf_query_points' cap, K < 0, r < 0 or not finite, tol <= 0 or
 * not finite; GNERF_E_UNSUPPORTED when one item's planes exceed 32-bit tap offsets (as gnerf_query_points_grad). */
int gnerf_project_points_to_level(const float* planes_nhwc, int n_items, int plane_h, int plane_w,
                                  const float* points, int n_points, float box_warp,
                                  const float* w1, const float* b1, const float* w2, const float* b2,
                                  float level, const float* affine, int max_steps, float radius, float tol,
                                  float* points_out, float* residual_in, float* residual_out, unsigned char* status,
                                  int planes_interleaved, gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 13) Marching cubes: the triangle mesh of a level set of a dense float32 volume [d0, d1, d2] (axis 2 fastest, contiguous,
 * every d >= 2, d0 * d1 * d2 < 2^31) -- what shape_utils.py:58-61 asks skimage.measure.marching_cubes for, with this project's own rules
 * (g-nerf_amd/shape_mi355x.py states them and holds a numpy port that gives the same bits):
 *   a lattice point is INSIDE iff v > level; one vertex per lattice edge p -> p + e_a (a = 0, 1, 2) whose endpoints disagree, at
 *   coord_a = i_a + t, t = (level - v_p) / (v_{p+e_a} - v_p) (float32, correctly rounded, no contraction), the other two coordinates p's
 *   indices (index space: spacing and origin are the caller's); vertices in lexicographic order of (linear index of p, a); faces as
 *   int32 vertex triples in order of the cell's lower corner, then csrc/mesh_tables.h's order, right-hand normal from inside to outside.
 * Three calls:
 *   gnerf_marching_cubes_workspace_bytes: *bytes = the workspace both passes share (4 bytes per lattice point + small per-block arrays).
 *   gnerf_marching_cubes_count: counts (device int64 [3]) = {vertices V, triangles T, non-finite values}; the workspace then holds
 *     what the emit pass needs (no initialisation needed before).
 *   gnerf_marching_cubes_emit: the same volume, level and workspace -> verts float32 [V, 3], faces int32 [T, 3] (NULL when the count
 *     is 0).  The caller reads the counts to the host in between (the op's only synchronisation), sizes the outputs from them, and
 *     does not call emit when the volume holds a non-finite value or V >= 2^31 (faces hold int32 ids).
 * Because of that read the op cannot be captured in a graph (count and emit alone are capturable, the sizing in between is not). */
int gnerf_marching_cubes_workspace_bytes(int d0, int d1, int d2, size_t* bytes);
int gnerf_marching_cubes_count(const float* volume, int d0, int d1, int d2, float level, void* workspace, int64_t* counts,
                               gnerf_stream_t stream);
int gnerf_marching_cubes_emit(const float* volume, int d0, int d1, int d2, float level, const void* workspace, float* verts,
                              int32_t* faces, gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 15) SSIM of two images X, Y [n, c, h, w] (float32 or float16, any strides, given in elements) and its gradient -- the
 * per-channel pair that pytorch_msssim's `_ssim` returns, from which its ssim and ms_ssim are built (torch_utils/ops/ssim.py):
 *   window: `win` HOST floats g[0..win-1] (odd win <= GNERF_SSIM_MAX_WIN, h >= win and w >= win), applied separably per channel as a
 *   VALID correlation, so the map is (h - win + 1) x (w - win + 1);
 *   mu1 = g*X, mu2 = g*Y, s1 = g*X^2 - mu1^2, s2 = g*Y^2 - mu2^2, s12 = g*XY - mu1 mu2;
 *   cs_map = (2 s12 + C2) / (s1 + s2 + C2), ssim_map = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs_map;
 *   ssim_nc[n * c] / cs_nc[n * c] (float32) = the means of ssim_map / cs_map over the map.  Arithmetic in float32.
 * Sums are taken in a fixed order without atomics: the same bits on every run, and an item's results do not depend on the batch around it.
 *   gnerf_ssim_workspace_bytes: *bytes = what gnerf_ssim_forward needs as workspace (per-tile partial sums; no initialisation needed).
 *   gnerf_ssim_forward: two launches.
 *   gnerf_ssim_backward: one launch that recomputes the moments (the forward saves nothing).  g_ssim / g_cs [n * c] float32 are the
 *     gradients of the loss w.r.t. ssim_nc / cs_nc; either may be NULL (= zeros), not both.  dx / dy (X's dtype, [n, c, h, w] with
 *     their own strides) receive the gradients w.r.t. X / Y; either may be NULL (not computed), not both.  Every element is written. */
#define GNERF_SSIM_MAX_WIN 11
int gnerf_ssim_workspace_bytes(int n, int c, int h, int w, int win, size_t* bytes);
int gnerf_ssim_forward(const void* x, const void* y, int dtype, int n, int c, int h, int w, const int64_t* x_strides,
                       const int64_t* y_strides, const float* window, int win, float C1, float C2, void* workspace, float* ssim_nc,
                       float* cs_nc, gnerf_stream_t stream);
int gnerf_ssim_backward(const void* x, const void* y, int dtype, int n, int c, int h, int w, const int64_t* x_strides,
                        const int64_t* y_strides, const float* window, int win, float C1, float C2, const float* g_ssim,
                        const float* g_cs, void* dx, const int64_t* dx_strides, void* dy, const int64_t* dy_strides,
                        gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 15, added without a new version) Antialiased resize of x [n, c, in_h, in_w] to y [n, c, out_h, out_w] and its transpose --
 * F.interpolate(mode='bilinear' | 'bicubic', align_corners=False, antialias=True) and its gradient.  float32 or float16; both tensors are
 * addressed through four element strides (n, c, h, w), so NCHW, channels_last and strided views run without a copy.  Per axis:
 *   scale = the given scale_h / scale_w (1 / scale_factor of a caller that does not recompute it) or, when that is <= 0, in / out;
 *   S = 2 (bilinear: f(x) = 1 - |x| on |x| < 1) or 4 (bicubic: Keys' cubic with a = -0.5 on |x| < 2);
 *   support = S/2 * scale if scale >= 1 else S/2;  invscale = 1 / scale if scale >= 1 else 1;
 *   for output i: center = scale * (i + 0.5), xmin = max(int(center - support + 0.5), 0), xsize = min(int(center + support + 0.5), in) - xmin,
 *   w_j = f((j + xmin - center + 0.5) * invscale) for j < xsize, divided by their sum if that is not 0;
 *   y = W_y x W_x^T per (n, c).
 * Band edges and weights are evaluated in float64 inside the kernel and each weight is rounded to float32 once; products and sums are float32,
 * horizontal pass first, the intermediate stays float32 and the result is rounded once, at the store.  No atomics, sums in a fixed order: the
 * same bits on every run, for every memory layout, and whatever an item is batched with.  No workspace, no host-side table, no synchronisation.
 *   gnerf_resize_aa_forward:  y = W_y x W_x^T.
 *   gnerf_resize_aa_backward: dx [n, c, in_h, in_w] = W_y^T dy W_x, dy [n, c, out_h, out_w] (a gather: every element of dx is written once).
 *     The operator is linear: the backward's own gradient is the forward again.
 * GNERF_E_UNSUPPORTED, before any launch: more than GNERF_RESIZE_MAX_TAPS taps per output along an axis (scale > 32 bilinear, > 16 bicubic, on an
 * axis longer than that), more than that many outputs touching one input (scale < 1/32), or 2^31 or more elements in a tensor. */
#define GNERF_RESIZE_MAX_TAPS 65
#define GNERF_RESIZE_BILINEAR 0
#define GNERF_RESIZE_BICUBIC 1
int gnerf_resize_aa_forward(const void* x, void* y, int dtype, int n, int c, int in_h, int in_w, int out_h, int out_w, const int64_t* x_strides,
                            const int64_t* y_strides, int mode, double scale_h, double scale_w, gnerf_stream_t stream);
int gnerf_resize_aa_backward(const void* dy, void* dx, int dtype, int n, int c, int in_h, int in_w, int out_h, int out_w, const int64_t* dy_strides,
                             const int64_t* dx_strides, int mode, double scale_h, double scale_w, gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 15, added without a new version) Triangle rasteriser for the meshes gnerf_marching_cubes_* extracts: a visibility buffer per view,
 * then depth / normal / shaded colour per pixel.  No gradients, no antialiasing, no transparency (textures: gnerf_raster_resolve_textured, below), and NO NEAR-PLANE CLIPPING:
 * a triangle with a vertex at or behind `near` is dropped whole (the shipped cameras sit 2.7 from a unit box).  Everything is float32 with
 * every operation rounded on its own, in the order written here (no fused multiply-add); g-nerf_amd/shape_mi355x.py's rasterize_numpy /
 * resolve_numpy restate it and give the same bits.
 *   inputs: verts float32 [n_verts, 3] and faces int32 [n_tris, 3] (as marching cubes returns them, in the mesh's own frame); per view a
 *     3x4 mesh2cam (device float32 [n_views, 12], rows) into the camera frame csrc/raygen.h implies (+z forward, x along columns, y along
 *     rows) and the camera label's normalised 3x3 intrinsics (device float32 [n_views, 9]); an h x w image (1..GNERF_RASTER_MAX_SIZE each);
 *     near > 0; n_views * n_tris < 2^31 and n_views * h * w < 2^31.  n_tris == 0 or n_verts == 0 is valid: nothing is drawn.
 *   vertex: p = ((A0 x + A1 y) + A2 z) + A3 per row; iz = 1 / p.z; xn = p.x iz, yn = p.y iz; xc = (fx xn + sk yn) + cx, yc = fy yn + cy (the
 *     inverse of ray_sampler.py:51-52); sx = xc w, sy = yc h, so that the centre of pixel (row, col) is (col + 0.5, row + 0.5);
 *     X = (int)rintf(sx * 256), Y likewise: 1/256-pixel integers.
 *   dropped, counted and never drawn, tested in this order: a vertex with non-finite p or p.z <= near ("near"); a vertex with |X| or |Y| > 2^21,
 *     an 8192-pixel guard band ("guard"); area = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0) == 0, or the culled winding -- GNERF_RASTER_CULL_BACK
 *     drops area > 0 (with y down that is the winding whose right-hand normal cross(p1 - p0, p2 - p0) points away from the camera),
 *     GNERF_RASTER_CULL_FRONT drops area < 0 --, or a face that names a vertex outside [0, n_verts) ("culled").  Everything else is "drawn".
 *   coverage: a triangle with area < 0 is drawn as (0, 2, 1).  Integer edge functions in int64 at pixel centres (256 col + 128, 256 row + 128)
 *     inside the bounding box clipped to the image; a centre exactly on an edge belongs to the triangle iff that edge runs up (dy < 0, a left
 *     edge) or is horizontal and runs right (a top edge), so of two triangles sharing an edge or a fan sharing a vertex exactly one owns it.
 *   depth: b_i = float(w_i) / float(area) (int64 -> float32, round to nearest even), iz = (b_a iz_a + b_b iz_b) + b_c iz_c, z = 1 / iz.
 *   vis: uint64 [n_views, h, w], key = float_as_uint(z) << 32 | triangle index, merged with a 64-bit atomic minimum; empty = all ones.  The
 *     nearest wins, equal z: the lowest index; the result does not depend on the order of arrival (the same bits on every run).
 *   routes: a triangle whose clipped bounding box holds at most GNERF_RASTER_SMALL_PIXELS centres is drawn by its own thread; a larger one is
 *     appended to a queue in the workspace and drawn by a whole wave of a second, fixed-size launch that reads the queue length on the device.
 * gnerf_raster_workspace_bytes: *bytes = the workspace of gnerf_raster_visibility (the queue: 4 bytes per (view, triangle) + 256).
 * gnerf_raster_visibility: initialises vis, counts and the workspace itself (no prepared memory needed), then draws: three launches, no host
 *   read, capturable.  counts: device int64 [4] = {drawn, near, guard, culled}, which sum to n_views * n_tris.
 * gnerf_raster_resolve: one thread per pixel, from vis and the same mesh and cameras.  Optional inputs: normals float32 [n_verts, 3] with the
 *   per-view 3x3 normal_mat (device float32 [n_views, 9]) that takes them to the camera frame; colors uint8 [n_verts, 3].  shading: ELEVEN HOST
 *   floats {light direction in the camera frame [3] (from the surface to the light, used as given), ambient, diffuse, albedo [3], background [3]},
 *   needed for `frame`.  Outputs, each optional (NULL = not wanted, not all NULL):
 *     tri_id int32 [n_views, h, w], -1 for background;
 *     depth float32 [n_views, h, w]: the distance along the pixel's ray, z * sqrt((xl xl + yl yl) + 1) with (xl, yl) as camera_ray forms them
 *       from (row, col) (1 / w and 1 / h in place of 1 / res) -- what image_depth holds; background = +inf;
 *     normal float32 [n_views, h, w, 3]: camera frame, unit length (zero where the length is not > 0), negated where (n . (xl, yl, 1)) > 0 so that
 *       it faces the camera, zero for background.  With `normals`: normal_mat times the perspective-correct mix (q_a n_a + q_b n_b) + q_c n_c,
 *       q_i = (b_i iz_i) / iz; without: the face normal cross(p1 - p0, p2 - p0) of the camera-frame positions;
 *     frame uint8 [n_views, h, w, 3]: rintf(min(max(c * (ambient + diffuse * max(0, n . light)), 0), 1) * 255), c = albedo or the mix of the
 *       vertex colours / 255; background pixels hold the background colour.
 *   The barycentrics are those of the depth step, recomputed from the winning triangle (the same bits).
 * GNERF_E_ARG for null pointers, sizes out of range, near <= 0, an unknown cull mode, normals without normal_mat, frame without shading. */
#define GNERF_RASTER_SMALL_PIXELS 64
#define GNERF_RASTER_MAX_SIZE 4096
#define GNERF_RASTER_CULL_NONE 0
#define GNERF_RASTER_CULL_BACK 1
#define GNERF_RASTER_CULL_FRONT 2
int gnerf_raster_workspace_bytes(int n_verts, int n_tris, int n_views, int h, int w, size_t* bytes);
int gnerf_raster_visibility(const float* verts, int n_verts, const int32_t* faces, int n_tris, const float* mesh2cam, const float* intrinsics,
                            int n_views, int h, int w, float near_z, int cull, void* workspace, uint64_t* vis, int64_t* counts,
                            gnerf_stream_t stream);
int gnerf_raster_resolve(const uint64_t* vis, const float* verts, int n_verts, const int32_t* faces, int n_tris, const float* mesh2cam,
                         const float* intrinsics, int n_views, int h, int w, const float* normals, const float* normal_mat,
                         const unsigned char* colors, const float* shading, int32_t* tri_id, float* depth, float* normal, unsigned char* frame,
                         gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 15, added without a new version) Multi-view colour bake, the rasteriser's inverse (csrc/raster.hip): every vertex of a mesh gathers
 * its colour from n_views frames taken by the cameras whose visibility buffers gnerf_raster_visibility made of that mesh.  Gather-only: one
 * thread per vertex, no atomics, no workspace, one launch, no host read, capturable.  Float32, every operation rounded on its own in the order
 * written here (no fused multiply-add); a dot product a . b is (a0 b0 + a1 b1) + a2 b2.  g-nerf_amd/shape_mi355x.py's bake_colors_numpy
 * restates it and gives the same bits.  No gradients, no filling of unseen vertices from their neighbours (the texture atlas: below).
 *   inputs: verts, mesh2cam, intrinsics, n_views, vis [n_views, h, w] and near as gnerf_raster_visibility takes and makes them; frames uint8
 *     [n_views, fh, fw, 3] (fh, fw in 1..GNERF_RASTER_MAX_SIZE, need not equal h, w; n_views * fh * fw < 2^31); optional normals float32
 *     [n_verts, 3] with the per-view 3x3 normal_mat [n_views, 9] of gnerf_raster_resolve; optional fallback uint8 [n_verts, 3].
 *   per vertex, the views in ascending order; a view is SKIPPED at the first of these tests that fails:
 *     vertex: p, iz, xn, yn, xc, yc as the rasteriser's vertex stage forms them (the same bits); p finite and p.z > near.
 *     pixel: sx = xc w, sy = yc h; 0 <= sx < w and 0 <= sy < h, tested on the floats; col = (int)floorf(sx), row = (int)floorf(sy).
 *     occlusion: every pixel of the (2 guard + 1)^2 window around (row, col), clipped to the image, holds a non-empty key, and with z_pix =
 *       uint_as_float(key >> 32): p.z <= z_pix + depth_tol z_pix.  guard = 0 tests the one pixel.  An empty neighbour rejects ON PURPOSE: at a
 *       silhouette a frame blends the surface with its background.
 *     facing (only with normals): n_c = normal_mat n per row; c = -(n_c . p) / sqrtf((n_c . n_c)(p . p)); c > min_cos (a NaN fails).
 *   weight: wgt = 1 without normals or with power == 0, else c multiplied by itself power - 1 times (((c c) c) ...).
 *   sample: u = xc fw - 0.5, v = yc fh - 0.5 (texel centres at integer + 0.5); x0 = floorf(u), tx = u - x0, y0 = floorf(v), ty = v - y0; the taps
 *     x0, x0 + 1, y0, y0 + 1 are clamped into the frame; per channel, with the uint8 texels as floats: top = (1 - tx) c00 + tx c01,
 *     bot = (1 - tx) c10 + tx c11, s = (1 - ty) top + ty bot.
 *   accumulate: acc[k] += wgt s[k]; accw += wgt; seen += 1.
 *   outputs: colors uint8 [n_verts, 3] = (uint8)rintf(min(max(acc[k] / accw, 0), 255)) where accw > 0, else the vertex's fallback colour (0
 *     without one); weight float32 [n_verts] = accw and seen int32 [n_verts] = the number of views that counted (each optional, NULL = not wanted).
 *   The defaults of the Python layer are arguments, not measurements: depth_tol = 2^-8, guard = 1, min_cos = 0.1, power = 2.  Across one pixel of
 *     an h-row image a surface whose normal makes the angle t with the line of sight changes its depth by z tan(t) / (fy h), relatively
 *     tan(t) / (fy h): at the shipped camera (fy = 4.2647) and 512 rows, t = 75 degrees gives 3.73 / 2183 = 1.7e-3, and 2^-8 = 3.9e-3 is about
 *     twice that -- a vertex anywhere inside its pixel passes on slopes up to there, a surface further behind than that is hidden.
 * GNERF_E_ARG for null required pointers, sizes out of the rasteriser's ranges, near <= 0, depth_tol < 0, guard outside
 * 0..GNERF_BAKE_MAX_GUARD, power outside 0..GNERF_BAKE_MAX_POWER, normals without normal_mat.  n_verts == 0 is valid: nothing is launched. */
#define GNERF_BAKE_MAX_GUARD 4
#define GNERF_BAKE_MAX_POWER 8
int gnerf_mesh_bake_colors(const float* verts, int n_verts, const float* mesh2cam, const float* intrinsics, int n_views, const uint64_t* vis,
                           int h, int w, const unsigned char* frames, int fh, int fw, const float* normals, const float* normal_mat,
                           float near_z, float depth_tol, int guard, float min_cos, int power, const unsigned char* fallback,
                           unsigned char* colors, float* weight, int32_t* seen, gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 15, added without a new version) Texture atlas of a mesh, baked from the same frames (csrc/raster.hip): the colour bake's rules per
 * TEXEL instead of per vertex, and a textured resolve to look at the result.  g-nerf_amd/shape_mi355x.py's atlas_layout / atlas_uvs /
 * bake_texture_numpy / resolve_textured_numpy restate all of it and give the same bits.  No mip-maps, no chart-based atlas, no filling of
 * unseen texels from their neighbours.
 * THE ATLAS is a function of (n_tris, patch) alone; no kernel takes a UV buffer.  P = patch texels per patch side, GNERF_ATLAS_MIN_PATCH <= P
 *   <= GNERF_ATLAS_MAX_PATCH; two triangles share one P x P cell: pair = t >> 1, half = t & 1, n_pairs = (n_tris + 1) / 2.  C = the smallest
 *   integer with C C >= n_pairs (in integers), rows = ceil(n_pairs / C); the texture is tw = C P wide and th = rows P high, cell
 *   (pair / C, pair % C) starts at texel (row P, col P).  tw and th are at most GNERF_ATLAS_MAX_SIZE each, GNERF_E_UNSUPPORTED otherwise,
 *   before any launch; n_tris == 0 gives a 0 x 0 atlas and no launch.
 *   Inside a cell, with local texel indices (i = column, j = row) in 0 .. P - 1 and L = P - 3: half 0 owns the texels with i + j <= P - 1,
 *   its corners 0, 1, 2 lie at the texel centres (0, 0), (L, 0), (0, L); half 1 owns i + j >= P and is the same rule on (P - 1 - i, P - 1 - j).
 *   The texels of half 1 in the last cell of an odd n_tris, and whole cells past n_pairs, are owned by nobody.  A texel's barycentrics, formed
 *   in this order, may be negative (an owned texel outside its triangle is extrapolated on the triangle's plane):
 *     b1 = float(i) / float(L), b2 = float(j) / float(L), b0 = (1 - b1) - b2.
 *   Why L = P - 3: a bilinear sample at a point (x, y) inside the triangle, x, y >= 0 and x + y <= L, has non-zero weight only on the taps
 *   (floor x + {0, 1}, floor y + {0, 1}), a tap + 1 only where that fractional part is positive, and floor x + floor y <= L - 1 whenever a
 *   fractional part is positive: every such tap has i + j <= L + 1 = P - 2 (half 0; i + j >= P + 1 for half 1).  So a triangle never reads its
 *   neighbour's texels and no dilation pass is needed; the spare diagonal i + j = P - 1 goes to half 0 (with L = P - 2 the halves would
 *   collide on it).  UV of corner k of triangle t, with (x, y) its texel index: u = (x + 0.5) / tw, v = (y + 0.5) / th from the top row.
 * gnerf_mesh_atlas_layout: host only; *cells_per_row = C, *th, *tw.
 * gnerf_mesh_bake_texture: one thread per texel, gather-only: one launch, no atomics, no LDS, no workspace, no host read, capturable.  Inputs
 *   as gnerf_mesh_bake_colors takes them, plus faces int32 [n_tris, 3] and patch; fallback uint8 [n_verts, 3] per VERTEX; background: three
 *   HOST uint8 values.  Per owned texel: x = (b0 v0 + b1 v1) + b2 v2 per component, and with normals n = (b0 n0 + b1 n1) + b2 n2 (left
 *   unnormalised: the cosine normalises); then per view, in ascending order, exactly the vertex bake's rules with x in place of the vertex
 *   (vertex, pixel, occlusion, facing, weight, sample, accumulate): both kernels are built from one stage function.
 *   outputs: texture uint8 [th, tw, 3]; optional weight float32 [th, tw] and seen int32 [th, tw].  accw > 0: rintf(min(max(acc[k] / accw, 0),
 *     255)); owned with accw == 0: with a fallback the mix (b0 c0 + b1 c1) + b2 c2 of the corners' fallback colours, clamped to 0 .. 255 and
 *     rounded with rintf, else background; weight = accw, seen = the views that counted.  A texel nobody owns, and every texel of a face that
 *     names a vertex outside [0, n_verts): background, weight = 0, seen = -1.  Every texel of the texture is written.
 * gnerf_raster_resolve_textured: gnerf_raster_resolve's sibling, one thread per pixel -> frame uint8 [n_views, h, w, 3] from vis, the same
 *   mesh and cameras, and texture uint8 [th, tw, 3] of gnerf_mesh_atlas_layout(n_tris, patch).  The winning triangle's barycentrics are those
 *   of the depth step (the same bits as resolve); they are taken back from the drawn order to the face's own corners (a triangle with
 *   area < 0 is drawn as (0, 2, 1)), q_i = (b_i iz_i) / iz; local position x = q1 L, y = q2 L (half 0) or x = (P - 1) - q1 L, y = (P - 1) - q2 L
 *   (half 1); u = float(col P) + x, v = float(row P) + y; x0 = floorf(u), tx = u - x0, y0 = floorf(v), ty = v - y0, taps x0, x0 + 1, y0, y0 + 1
 *   clamped into the texture, top / bot / s as the frame sampler of gnerf_mesh_bake_colors; frame = rintf(min(max(s, 0), 255)), UNLIT (the
 *   texture holds the frames' lit colours); empty pixels: background (three HOST uint8 values).
 *   KNOWN LIMIT: float rounding can put x + y a few ulp past L; the over-run tap then carries a weight of that size and lands on the spare
 *   diagonal.  That is part of the rule and of the port, not an error.
 * GNERF_E_ARG as gnerf_mesh_bake_colors / gnerf_raster_resolve, and for patch out of range. */
#define GNERF_ATLAS_MIN_PATCH 4
#define GNERF_ATLAS_MAX_PATCH 64
#define GNERF_ATLAS_MAX_SIZE 16384
int gnerf_mesh_atlas_layout(int n_tris, int patch, int* cells_per_row, int* th, int* tw);
int gnerf_mesh_bake_texture(const float* verts, int n_verts, const int32_t* faces, int n_tris, int patch, const float* mesh2cam,
                            const float* intrinsics, int n_views, const uint64_t* vis, int h, int w, const unsigned char* frames, int fh, int fw,
                            const float* normals, const float* normal_mat, float near_z, float depth_tol, int guard, float min_cos, int power,
                            const unsigned char* fallback, const unsigned char* background, unsigned char* texture, float* weight, int32_t* seen,
                            gnerf_stream_t stream);
int gnerf_raster_resolve_textured(const uint64_t* vis, const float* verts, int n_verts, const int32_t* faces, int n_tris, const float* mesh2cam,
                                  const float* intrinsics, int n_views, int h, int w, const unsigned char* texture, int patch,
                                  const unsigned char* background, unsigned char* frame, gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 15, added without a new version) Cleaning the meshes gnerf_marching_cubes_* extracts: connected components, compaction to the kept
 * components, Taubin smoothing (csrc/mesh_clean.hip).  g-nerf_amd/shape_mi355x.py restates the rules and holds numpy ports
 * (mesh_components_numpy, mesh_select, mesh_compact_numpy, mesh_smooth_numpy) that give the same bits.
 *   a mesh: verts float32 [V, 3] and faces int32 [T, 3] as marching cubes returns them; V == 0 or T == 0 is valid (the pointer of an empty
 *   array may be NULL).  A face is VALID iff its three ids lie in [0, V); ids may repeat.  An invalid face joins nothing, is counted, is dropped
 *   by the compaction and ignored by the smoothing; the Python layer raises ValueError when the count is not 0.
 * COMPONENTS (gnerf_mesh_components): a valid face joins its three vertices.
 *   label int32 [V]: the smallest vertex index of v's connected component (label[v] <= v, label[label[v]] == label[v]; a vertex in no face:
 *     label[v] == v);
 *   faces_of int32 [V]: faces_of[l] = the number of valid faces whose first vertex has label l (0 where l is no label);
 *   counts (device int64 [3]) = {components with at least one face, vertices in no valid face, invalid faces}.
 *   All integers and unique: the same bits on every run and for every order of the faces.  Six launches, no host read, capturable.
 * SELECTION (integers only, on the host; shape_mi355x.mesh_select): the components with at least one face, ordered by face count descending,
 *   then label ascending; a component is kept iff its face count >= min_faces and (keep_largest == 0 or its rank < keep_largest).
 * COMPACTION (gnerf_mesh_compact_count, then _emit): keep uint8 [V] is indexed by LABEL.  A vertex is kept iff keep[label[v]] != 0 and
 *   faces_of[label[v]] > 0 (vertices in no face are always dropped); a face iff it is valid and its first vertex is kept.  Kept vertices stay in
 *   ascending old index, kept faces in ascending old face index with their ids remapped; src_vertex int32 [V'] = the old index of every new
 *   vertex (gather normals and colours with it).  If everything is kept the output equals the input bit for bit.
 *   _count: counts (device int64 [2]) = {V', T'}; the caller reads them (the op's one synchronisation, so it is not capturable), sizes
 *   out_verts [V', 3], out_faces [T', 3], src_vertex [V'] and calls _emit with the same inputs and workspace -- not at all when V' == 0.
 *   out_faces may be NULL when the counted T' is 0 (the face pass is then skipped): label and faces_of that do not belong together can give V' > 0 with T' == 0.
 *   Positions come from a block scan plus a scan of the block totals, never from the order of arrival.
 * SMOOTHING (gnerf_mesh_smooth): Taubin lambda | mu smoothing with uniform weights; positions change, faces do not.
 *   N(i), the neighbour multiset of vertex i: corner c (0, 1, 2) of every valid face gives vertex f[c] the two ids f[c + 1], f[c + 2]
 *   (cyclically), so a neighbour j occurs once per face that contains the edge {i, j}; m_i = |N(i)|.
 *   One half-step with factor s (a C float), per coordinate: c = (sum of double(v_j)) / double(m_i), summed over N(i) in ascending j
 *   (duplicates adjacent, starting from 0.0), sum and division in float64; v_i' = float32(double(v_i) + double(s) * (c - double(v_i))).  Every
 *   operation is rounded on its own, no contraction.  All vertices move together from the previous positions; one iteration = a half-step
 *   with lam, then one with mu.  A vertex with m_i == 0 never moves; with pin_boundary != 0 neither does a vertex some neighbour of which
 *   does not occur exactly twice in N(i) (a boundary or non-manifold edge).  The ascending order makes the result independent of the order of
 *   the faces and of the rotation of a face's ids.  iterations == 0 copies verts to out (out may be verts).  The neighbour rows are built
 *   once per call (counts, row starts by a scan, fill, one sort per row, any length); the 2 * iterations half-steps are pure gathers.
 *   No host read: capturable.
 * gnerf_mesh_workspace_bytes: *bytes = a workspace large enough for each of the calls on a mesh of that size (the smoothing's is the
 *   largest: 24 bytes per face + 37 per vertex); no initialisation needed.
 * GNERF_E_ARG for null pointers, negative sizes, negative iterations, or more than 2^32 / 6 - 1 faces in gnerf_mesh_smooth. */
int gnerf_mesh_workspace_bytes(int n_verts, int n_tris, size_t* bytes);
int gnerf_mesh_components(const int32_t* faces, int n_verts, int n_tris, void* workspace, int32_t* label, int32_t* faces_of,
                          int64_t* counts, gnerf_stream_t stream);
int gnerf_mesh_compact_count(const int32_t* faces, int n_verts, int n_tris, const int32_t* label, const int32_t* faces_of,
                             const unsigned char* keep, void* workspace, int64_t* counts, gnerf_stream_t stream);
int gnerf_mesh_compact_emit(const float* verts, const int32_t* faces, int n_verts, int n_tris, const int32_t* label,
                            const int32_t* faces_of, const unsigned char* keep, void* workspace, float* out_verts, int32_t* out_faces,
                            int32_t* src_vertex, gnerf_stream_t stream);
int gnerf_mesh_smooth(const float* verts, int n_verts, const int32_t* faces, int n_tris, int iterations, float lam, float mu,
                      int pin_boundary, void* workspace, float* out, gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 15, added without a new version) Simplifying such a mesh between the compaction and the smoothing: vertex clustering on a uniform grid
 * with a quadric-error representative per cell (Lindstrom's out-of-core simplification; csrc/mesh_simplify.hip).  One pass over vertices and
 * faces, order-independent and bit-reproducible (integer accumulation), and no vertex leaves its cell.  g-nerf_amd/shape_mi355x.py restates
 * the rules and holds the numpy port (mesh_simplify_numpy) that gives the same bits.  Every float64 operation is rounded on its own, no
 * contraction; only + - * /, floor, comparisons and integer conversion occur.
 *   a mesh as above (V == 0 or T == 0 is valid); cell: a C float > 0, finite; origin: three finite C floats ON THE HOST.
 * 1 VALID FACES: a face is valid iff its three ids lie in [0, V) and its three vertices are finite (ids are range-checked before they index
 *   anything).  Invalid faces are counted and otherwise ignored.  A vertex is USED iff a valid face names it; unused vertices are dropped.
 * 2 CELLS: for a used vertex, per axis p = (double(v) - double(origin)) / double(cell), k = floor(p) clamped to [0, 2^21 - 1];
 *   key = kx 2^42 + ky 2^21 + kz.  A CLUSTER is the set of used vertices of one key, its representative its smallest vertex index
 *   (cluster[v] <= v, cluster[cluster[v]] == cluster[v]).  New vertex ids number the representatives in ascending old index; src_vertex [V']
 *   holds those old indices (gather normals and colours with it).  u = p - (k + 0.5), clamped to [-0.5, 0.5] per axis (the clamp is felt
 *   only by a vertex outside the grid's 2^21 cells).
 * 3 ACCUMULATION in int64 fixed point, q(x) = llrint(x 2^32), sums modulo 2^64, so any order gives the same bits:
 *   per used vertex, into its cluster: q(u) per axis and a member count;
 *   per valid face, read from its corner with the smallest vertex id (the first of them; the face is rotated, never reflected, which makes
 *   the result independent of the rotation of a face's ids) -- corners 0, 1, 2 in that order: e1 = p1 - p0, e2 = p2 - p0, n = e1 x e2
 *   (n0 = e1y e2z - e1z e2y, n1 = e1z e2x - e1x e2z, n2 = e1x e2y - e1y e2x), s = (n0 n0 + n1 n1) + n2 n2 in grid units.  The face is
 *   skipped unless 0 < s < inf.  Its scale is f = 16 / s if s > 16, else 1: area-squared weighting, which mutes marching-cubes slivers; the
 *   cap only bounds oversized triangles so that the fixed point stays small.
 *   per corner c of such a face, into the cluster of that corner's vertex, with d = (n0 u0 + n1 u1) + n2 u2 for u of that vertex: the six
 *   q((f n_a) n_b), a <= b, and the three q(n_a (f d)).
 * 4 POSITION: A and b are the sums / 2^32 as doubles, cen = (the u sums / 2^32) / members, tr = (A00 + A11) + A22, mu = tr / 256.
 *   If tr > 0, x solves (A + mu I) x = b + mu cen by this elimination (M = A + mu I, r = b + mu cen; no pivoting):
 *     l10 = M01 / M00, l20 = M02 / M00; M11 -= l10 M01, M12 -= l10 M02, M22 -= l20 M02; r1 -= l10 r0, r2 -= l20 r0;
 *     l21 = M12 / M11; M22 -= l21 M12, r2 -= l21 r1; x2 = r2 / M22, x1 = (r1 - M12 x2) / M11, x0 = ((r0 - M01 x1) - M02 x2) / M00;
 *   x = cen instead if tr is not > 0, if one of the pivots M00, M11, M22 (as eliminated) is not > 0 or if x is not finite.  x is clamped to
 *   [-0.5, 0.5] per axis; the new vertex is float32(double(origin) + ((k + 0.5) + x) double(cell)) with k of the representative.  The mu
 *   term pulls flat regions to the centroid's foot on their plane and leaves corners alone.
 * 5 FACES: a valid face mapped through the new ids is COLLAPSED if two ids coincide, and dropped.  The rest are grouped by their unordered id
 *   set; sigma of a group = the sum over its members of +1 for a rotation of the ascending triple and -1 otherwise.  The group yields one
 *   face iff sigma is odd: the ascending triple (a, b, c) when sigma > 0, (a, c, b) otherwise.  Output faces are ordered by their group's
 *   smallest old face index.  This is the mod-2 image of the input chain: a closed input gives an output every edge of which lies in an even
 *   number of faces.
 * 6 counts (device int64 [8]) = {V', T', invalid faces, collapsed faces, faces absorbed by grouping (T - T' - invalid - collapsed), groups
 *   with |sigma| >= 2, internal error (a probe ran through a whole table: cannot happen, the Python layer raises), 0}.
 * gnerf_mesh_simplify_count does the tables, the ids and the face grouping, no quadrics; the caller reads the counts (the op's one
 *   synchronisation), sizes out_verts [V', 3], out_faces [T', 3], src_vertex [V'] and calls _emit with the same inputs and workspace -- not at
 *   all when V' == 0.  out_faces may be NULL when T' == 0; vertex_map int32 [V] (the new id of every old vertex, or -1) may be NULL.
 *   Neither call reads on the host, allocates or synchronises.  New positions of vertices and faces come from a block scan plus a scan of
 *   the block totals, never from the order of arrival.
 * gnerf_mesh_simplify_workspace_bytes: a workspace for both calls on a mesh of that size (about 137 bytes per vertex and 28 per face); no
 *   initialisation needed.  At most 2^30 vertices and 2^30 faces.
 * GNERF_E_ARG for null pointers, negative or oversized sizes, cell not > 0 or not finite, origin not finite, or _emit on an empty mesh. */
int gnerf_mesh_simplify_workspace_bytes(int n_verts, int n_tris, size_t* bytes);
int gnerf_mesh_simplify_count(const float* verts, const int32_t* faces, int n_verts, int n_tris, float cell, const float* origin,
                              void* workspace, int64_t* counts, gnerf_stream_t stream);
int gnerf_mesh_simplify_emit(const float* verts, const int32_t* faces, int n_verts, int n_tris, float cell, const float* origin,
                             void* workspace, float* out_verts, int32_t* out_faces, int32_t* src_vertex, int32_t* vertex_map,
                             gnerf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 15, added without a new version) Flip guard: after the vertices of a mesh have been moved (gnerf_project_points_to_level), set back the
 * vertices of every face that the move turned over (csrc/mesh_clean.hip; shape_mi355x.mesh_flip_guard_numpy gives the same bits).
 *   verts_in, verts_moved float32 [V, 3]; faces int32 [T, 3]; max_rounds R >= 1; verts_out float32 [V, 3] (written; may be verts_moved, not
 *   verts_in); status uint8 [V], IN AND OUT; counts int32 [R + 1] on the device, written.
 *   The normal of a face (a, b, c) at given positions is n = (b - a) x (c - a) = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),
 *   formed in float64 from the float32 coordinates; a dot product is (x0 y0 + x1 y1) + x2 y2; every operation is rounded on its own, no
 *   contraction.  With n0 at verts_in and n1 at the current positions a face is FLIPPED iff n0.n1 < 0, or n1.n1 == 0 and n0.n0 > 0: an
 *   input face of zero area is never flipped.  A face is valid iff its three ids lie in [0, V); the others are skipped.
 *   The current positions start as verts_moved.  Status 3 means REVERTED; status comes in with other values only (the
 *   projection's 0, 1, 2), which the vertices that are not reverted keep.
 *   Round j = 0 .. R - 1: status = 3 for the three vertices of every face flipped at the positions of the start of the round (plain stores
 *   of the same value), the number of those faces -> counts[j] (one integer add per block); then every vertex of status 3 is set to verts_in.
 *   A round whose predecessor counted 0 does nothing and counts 0 (a device-side read of counts[j - 1]).  A last pass writes the number of
 *   faces still flipped into counts[R].  The reverted set only grows and a fully reverted mesh has no flip, so the counts reach 0.
 *   No workspace, no host read, no allocation: capturable.  Integer adds only: the same bits for every order of the faces.
 * GNERF_E_ARG for null pointers, negative sizes, R < 1 or verts_out == verts_in. */
int gnerf_mesh_flip_guard(const float* verts_in, const float* verts_moved, const int32_t* faces, int n_verts, int n_tris, int max_rounds,
                          float* verts_out, unsigned char* status, int32_t* counts, gnerf_stream_t stream);

/* (ABI 15, added without a new version) The densities-only point query at LATTICE points named by their linear index (csrc/query_lattice.inl):
 * what extract_density_grid's narrow band evaluates, gnerf_query_points' kernel with another point source and sink.
 *   planes_nhwc, plane_h, plane_w, box_warp, w1 .. b2, planes_interleaved: as gnerf_query_points, for ONE item.
 *   index int32 [m]: linear indices into the n^3 lattice of gen_videos.py's create_samples(N = n, cube_length), duplicates allowed (they write
 *   the same value); out float32 [n^3]: out[index[i]] = sigma, every other entry is left alone (an index outside [0, n^3) writes nothing).
 *   The position of index idx is voxel_samples' (gen_videos_mi355x.py) as PyTorch computes it on the device, in fp32, one rounding per
 *   operation, no contraction: f = float(idx); s2 = float(idx % n) in integers; q1 = f * r, s1 = fmod(q1, n); q0 = q1 * r, s0 = fmod(q0, n)
 *   with r = 1.0f / float(n) -- a float tensor divided by a Python scalar is multiplied by the scalar's fp32 reciprocal there, which is the
 *   quotient for a power of two only --; p = (s0, s1, s2) * float(cube_length / (n - 1)) + float(-cube_length / 2), two roundings each.
 *   So out[idx] holds the bits gnerf_query_points gives at voxel_samples(idx, idx + 1, n, cube_length): a point's result does not depend on the
 *   other points of its tile.
 * GNERF_E_ARG for null pointers, m < 1, m beyond gnerf_query_points' cap on n_points, n < 2, n^3 >= 2^31 or a cube_length that is not finite and > 0. */
int gnerf_query_lattice(const float* planes_nhwc, int plane_h, int plane_w, const int32_t* index, int m, int n, double cube_length, float box_warp,
                        const float* w1, const float* b1, const float* w2, const float* b2, float* out, int planes_interleaved,
                        gnerf_stream_t stream);

/* (ABI 15, added without a new version) The narrow band of a density volume: surface following on bricks (csrc/mesh_band.hip; the driver is
 * shape_mi355x.band_volume, and band_volume_numpy gives the same bits).  Only the lattice points near the level set are evaluated, and the
 * mesh of the result is the dense volume's in the same vertex and face order, minus whole components that no brick below ever touched.
 *   SETTING.  The lattice is n^3 points in linear order (axis 2 fastest), volume float32 [n^3].  `level` is the isosurface level, s in
 *   {2, 4, 8, 16} the brick edge in cells.  A point is INSIDE iff its effective value is > level (ties and NaN are outside: marching cubes'
 *   rule).  The effective value e(p) is 0 where the caller's crop will zero p and the volume's value elsewhere; keep: six ints on the HOST,
 *   the kept index range [lo, hi) of axes 0, 1, 2 (null: everything; clamped to [0, n]).
 *   BRICKS.  nb = ceil((n - 1) / s) bricks per axis; brick b owns the cells [b s, min((b + 1) s, n - 1)) and its points are the closed range
 *   [b s, min((b + 1) s, n - 1)]: neighbours share their face points, the last brick may be partial.  Brick (b0, b1, b2) has index
 *   (b0 nb + b1) nb + b2.  The COARSE points have every index in {0, s, 2 s, ...} + {n - 1}: the bricks' corners.
 *   state: one byte per brick [nb^3]: 0 inactive, 1 active, 2 new (active; its points are evaluated in this round), 3 named by the growth of
 *   this round (only inside gnerf_band_grow).
 *   STEPS, as the driver takes them: evaluate the coarse points; gnerf_band_seed; while there are new bricks: gnerf_band_points_count /
 *   _emit, evaluate the listed points, gnerf_band_grow; gnerf_band_fill; the crop; marching cubes.
 *   gnerf_band_workspace_bytes: *bytes = the workspace the calls below share (12 bytes per brick + small per-block arrays).  gnerf_band_seed
 *     and gnerf_band_grow leave the list of the new bricks in it; gnerf_band_points_count / _emit and the next gnerf_band_grow read that list,
 *     so they follow a seed or grow on the same state and workspace, with the state left as it was.
 *   gnerf_band_seed: state = 2 for every brick whose eight corner points are not all on one side, 0 for the others; *count = the seeds.
 *   gnerf_band_points_count: *count = the length of the round's index list: the points of the bricks of state 2 that are not evaluated yet --
 *     neither coarse nor in a brick of state 1 --, each once: a point that several new bricks share belongs to the one of the lowest index.
 *   gnerf_band_points_emit: index int32 [m] = that list, m as counted (same state, same workspace, no call between the two): brick-major in
 *     brick order, then row-major within the brick (axis 2 fastest), so that neighbouring entries share plane texels.
 *   gnerf_band_grow: every brick of state 2 tests each of its six faces whose neighbour exists and has state 0: if the face's points are
 *     not all on one side, the neighbour is named (a byte store of 3; every writer stores the same value and a reader takes 0 and 3 alike).
 *     Then the round closes: 2 -> 1, 3 -> 2; *count = the new bricks.
 *   gnerf_band_fill: every point that is neither coarse nor in a brick of state 1 or 2 takes the effective value of the coarse point at
 *     (i0 / s * s, i1 / s * s, i2 / s * s).  It reads coarse points only and writes the others only: in place.
 *   count: int64 on the DEVICE, written; the driver reads the new bricks and the list's length together, once per round.  Every result is
 *   placed by index (block prefixes and scans), never by arrival: states, lists and the volume are the same from run to run.
 * GNERF_E_ARG for null pointers, another s, n < 2, n^3 >= 2^31 or an m that is not a count. */
int gnerf_band_workspace_bytes(int n, int s, size_t* bytes);
int gnerf_band_seed(const float* volume, int n, int s, float level, const int* keep, unsigned char* state, void* workspace, int64_t* count,
                    gnerf_stream_t stream);
int gnerf_band_points_count(const unsigned char* state, int n, int s, void* workspace, int64_t* count, gnerf_stream_t stream);
int gnerf_band_points_emit(const unsigned char* state, int n, int s, const void* workspace, int32_t* index, int64_t m, gnerf_stream_t stream);
int gnerf_band_grow(const float* volume, int n, int s, float level, const int* keep, unsigned char* state, void* workspace, int64_t* count,
                    gnerf_stream_t stream);
int gnerf_band_fill(float* volume, int n, int s, const int* keep, const unsigned char* state, gnerf_stream_t stream);

/* (ABI 15, added without a new version) Marching cubes over the active bricks of a narrow band, brick by brick (csrc/mesh_band_cubes.hip;
 * shape_mi355x.band_marching_cubes_numpy gives the same bits): no gnerf_band_fill, no crop, flip or transpose pass, nothing proportional to n^3.
 *   INPUT.  volume float32 [n^3] of a band run BEFORE gnerf_band_fill: true densities at the coarse points and at every point of an active
 *   brick, unwritten memory elsewhere.  state [nb^3]: the final brick states, every byte 0 or 1 (after the last gnerf_band_grow).  n, s, level
 *   and keep as gnerf_band_* take them (keep: the kept range of the unflipped lattice).  A VIEW: perm, three ints on the host, a permutation of
 *   (0, 1, 2) (null: the identity), and flip, three ints on the host, non-zero where that LATTICE axis is flipped (null: none).
 *   VIEW.  Mesh coordinate m_k = l_perm[k], or n - 1 - l_perm[k] where lattice axis perm[k] is flipped: the mesh volume is
 *   vol.reshape(n, n, n).flip(flipped axes).permute(perm).
 *   VALUES.  The effective value e(p) is 0 outside keep and the stored value inside; a point is inside iff e(p) > level (ties and NaN outside).
 *   VISITED.  A point is visited iff it lies in the closed point range of at least one active brick.  Only visited points are ever read.  An
 *   edge is examined iff both endpoints are visited, a cell iff all eight corners are.
 *   OUTPUT.  gnerf_marching_cubes_*'s, in the mesh view: one vertex per examined, crossed edge, owned by the edge's lower endpoint in MESH
 *   coordinates, ordered by (owner's mesh-linear index with m2 fastest, mesh axis), at the owner's float(m) plus t = (level - v) / (v_next - v)
 *   on the edge's axis (correctly rounded, not contracted); faces in cell mesh-linear order, then mesh_tables.h's order within the case,
 *   outward winding, ids into that vertex order.  When state and volume come from one band run this is the mesh gnerf_marching_cubes_* makes of
 *   the filled, cropped, flipped and permuted volume, bit for bit: once growth has ended a face between an active and an inactive brick lies on
 *   one side of the level, so every crossed edge and every non-empty cell lies within active bricks, and gnerf_band_fill never writes a point
 *   of an active brick.
 *   active: the number of active bricks as the caller knows it (the band driver's seeds + new bricks); it sizes the workspace, which is
 *   proportional to it (2 bytes per point and 8 bytes per row of s + 1 points of an active brick) plus 4 bytes per brick for a brick -> slot
 *   map and small per-column arrays -- no 4 bytes per lattice point.
 *   gnerf_band_mesh_count: counts int64 [4] on the DEVICE = {V, T, non-finite effective values among the visited points, visited points}.
 *     A refused input gives {0, 0, -1, 0} when the state holds more active bricks than `active`, {0, 0, -2, 0} when a state is neither 0 nor 1.
 *   gnerf_band_mesh_emit, after a count on the same arguments and workspace: verts float32 [V, 3], faces int32 [T, 3] (null when T = 0).  The
 *     caller reads the counts between the two and does not emit when counts[2] != 0 or V is 0 or >= 2^31.
 *   Everything is placed by index: a segment of a brick's row has a closed-form rank in the mesh's point order, and one scan over the segments
 *   gives every offset.  No float atomics; two runs give the same bytes.
 * GNERF_E_ARG for null pointers, another s, n < 2, n^3 >= 2^31, a perm that is no permutation or an `active` outside [0, nb^3]. */
int gnerf_band_mesh_workspace_bytes(int n, int s, int64_t active, size_t* bytes);
int gnerf_band_mesh_count(const float* volume, const unsigned char* state, int n, int s, float level, const int* keep, const int* perm,
                          const int* flip, int64_t active, void* workspace, int64_t* counts, gnerf_stream_t stream);
int gnerf_band_mesh_emit(const float* volume, const unsigned char* state, int n, int s, float level, const int* keep, const int* perm,
                         const int* flip, int64_t active, const void* workspace, float* verts, int32_t* faces, gnerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GNERF_HIP_H */
