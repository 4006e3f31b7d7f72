/*
 * elvis_amd.h - C ABI of the MI355X-native ELVIS client-side restoration hot path.
 *
 * The reference (emanuele-artioli/elvis) is pure Python and has NO FFI of its own
 * (SURVEY.md F2, section 8b): its drop-in boundary is three Python callable protocols
 * (P1 upsample_fn, P2 process_fn, P3 restore_fn) plus the sharding helpers.  This header
 * is the C-ABI that the Python shim in `elvis_amd/` calls through ctypes to implement
 * those protocols; each entry point cites the reference code whose arithmetic it
 * replaces.  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *  - every function returns 0 on success, a negative ELVIS_E_* code on failure; the
 *    message for the calling thread is available from elvis_last_error().
 *  - all pointers are DEVICE pointers (HBM) unless the name ends in `_host`.
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *  - no entry point allocates, frees or synchronises: callers own all buffers
 *    (hipGraph-capturable, cdna guide G9).
 *  - images are NHWC, C-contiguous.  u8 frames are (n,h,w,3).  Float tensors carry an
 *    explicit channel pitch (`*_pitch`, in elements, multiple of 8) so producers can write
 *    straight into channel slices of a wider buffer.
 *  - dtype codes: ELVIS_F32 = 0 (exact-parity mode), ELVIS_F16 = 1 (MFMA fast mode,
 *    fp32 accumulate); elvis_conv2d / elvis_conv_pack_weights also take ELVIS_F32X3 = 2
 *    (fp32 tensors, f16 MFMA with the rounding error compensated: fp32-grade results at
 *    2-2.5x the fp32 MFMA's rate, for the shapes elvis_conv_x3_eligible accepts).
 */
#ifndef ELVIS_AMD_H
#define ELVIS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ELVIS_ABI_VERSION 1

#define ELVIS_OK 0
#define ELVIS_E_INVALID (-1)   /* bad shape / argument  -> Python ValueError   */
#define ELVIS_E_RUNTIME (-2)   /* HIP launch failure    -> Python RuntimeError */
#define ELVIS_E_UNSUPPORTED (-3)

#define ELVIS_F32 0
#define ELVIS_F16 1
#define ELVIS_F32X3 2   /* conv only: fp32 tensors; products on the f16 matrix pipe with the rounding error compensated
                         (operands split hi + lo, ~1e-6 relative), 2-4x the fp32 MFMA's rate.  See elvis_conv_x3_eligible.
                         OPERAND RANGE: hi = f16(v), so every activation (after the fused prologue) and weight must
                         satisfy |v| < 65504; beyond that the result is non-finite (inf / NaN), never silently wrong.
                         Run a layer whose operands can exceed the f16 range as ELVIS_F32. */

#define ELVIS_ROUND_CV2 0      /* 2x2: (s+2)>>2 ; else rint(float(s)*(1.f/area)) half-even */
#define ELVIS_ROUND_HALF_UP 1  /* (s + area/2) / area */

typedef void* elvis_stream_t;

int elvis_abi_version(void);
const char* elvis_last_error(void);

/* ------------------------------------------------------------------ block-map glue (u8) */

/* out[blk(i,j)] = (map[n,i,j] <= thr) ? a : b, per b x b block; pixels outside the
 * by*block x bx*block grid take `b`.  Replaces the python By x Bx paste loop of
 * upscale_realesrgan_adaptive (elvis.py:2584-2595) and the boolean-mask block copy of
 * _instantir_chunk_worker (elvis.py:2975-2978).  If map_out != NULL it receives the clamped
 * map of elvis.py:2592: map_out = (map <= thr) ? map : clamp_to. */
int elvis_recompose_u8(const uint8_t* a, const uint8_t* b, const int32_t* map, uint8_t* out,
                       int32_t* map_out, int n, int h, int w, int c, int block, int by, int bx,
                       int thr, int clamp_to, elvis_stream_t stream);

/* Integer-factor box-mean downscale; replaces cv2.resize(..., INTER_AREA) at
 * elvis.py:2565 and elvis.py:2581.  h,w must be divisible by factor. */
int elvis_area_downscale_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                            int factor, int rounding, elvis_stream_t stream);

/* out = trunc(clip(orig*(1-alpha*m) + rest*(alpha*m), 0, 255)), m = (map>0) upsampled by
 * `block` (nearest).  Replaces blended_restoration's per-frame fp32 blend (utils.py:1581-1599). */
int elvis_blend_u8(const uint8_t* orig, const uint8_t* rest, const int32_t* map, uint8_t* out,
                   int n, int h, int w, int c, int block, int by, int bx, float alpha,
                   elvis_stream_t stream);

/* Per-level select: out block (i,j) of frame f = versions[level_slot[map[f,i,j]]][f] block;
 * pixels outside the floored grid are 0.  `versions` is a DEVICE array of n_versions device
 * pointers, each (n,h,w,c) u8; `slot_of_level` is a DEVICE int32 table of size n_levels.
 * Replaces the F x By x Bx python loop of restore_video_adaptively (presley.py:1262-1273). */
int elvis_select_levels_u8(const uint8_t* const* versions, const int32_t* slot_of_level, int n_levels,
                           const int32_t* map, uint8_t* out, int n, int h, int w, int c, int block,
                           int by, int bx, elvis_stream_t stream);

/* Feathered tile accumulate, bit-exact with numpy's float32 evaluation order:
 *   sw = f32(f64(f32(f64(wy[y]) * wx[x])) * wx2[x]); wgt = sw * temporal_weight;
 *   acc[y0+y, x0+x, :] += f32(tile) * wgt;  wsum[y0+y, x0+x] += wgt.
 * wy (th floats) holds the top/bottom ramps already applied in float32, wx / wx2 (tw doubles)
 * the left / right np.linspace ramps (1.0 where no ramp).  Replaces resource_aware_restore's
 * blend loop (utils.py:275-314).  acc is (h,w,c) f32, wsum (h,w) f32, tile (th,tw,c) u8. */
int elvis_tile_accumulate_f32(float* acc, float* wsum, const uint8_t* tile, const float* wy,
                              const double* wx, const double* wx2, int h, int w, int y0, int x0, int th,
                              int tw, int c, float temporal_weight, elvis_stream_t stream);

/* out = trunc(clip(acc / (wsum>0 ? wsum : 1), 0, 255)) (utils.py:317-324). */
int elvis_tile_normalize_u8(const float* acc, const float* wsum, uint8_t* out, int h, int w, int c,
                            elvis_stream_t stream);

/* Integer-exact sum of squared u8 differences per frame, for PSNR/MSE (elvis.py:627-671,
 * presley.py:226-245).  mask (n,h,w) u8 may be NULL.  sse_out / cnt_out: n u64 each (sum, number
 * of compared elements); both must be zeroed by the caller. */
int elvis_sse_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, unsigned long long* sse_out,
                 unsigned long long* cnt_out, int n, int h, int w, int c, elvis_stream_t stream);

/* Per-block SSIM (utils.py:572-608 = pytorch_msssim.ssim per block_size x block_size patch: data_range 1, 11-tap
 * Gaussian window sigma 1.5 passed in as win11 (device f32[11], normalised), "valid" smoothing that is skipped for
 * blocks shorter than the window, K = (0.01, 0.03), mean over the map then over channels).  The block grid is
 * floored (H // block_size, W // block_size); ssim_out: f32 [n, H // b, W // b]. */
int elvis_block_ssim_u8(const uint8_t* a, const uint8_t* b, float* ssim_out, const float* win11, int n, int h, int w, int c,
                        int block_size, elvis_stream_t stream);

/* ------------------------------------------------------------------ quality report (quality.hip) */

/* Per-frame bounding box of a [n,h,w] u8 mask (non-zero = set), the crop of elvis.py:688-690 and presley.py:431-436:
 * bbox_out int32 [n,4] = y0, y1, x0, x1 with exclusive ends, 0,0,0,0 for an empty mask.  Integer min/max only. */
int elvis_mask_bbox_u8(const uint8_t* mask, int32_t* bbox_out, int n, int h, int w, elvis_stream_t stream);

/* out = ((mask != 0) != invert) ? frames : 0 per pixel (_apply_binary_mask, elvis.py:615-624).  frames, out: [n,h,w,c] u8;
 * mask: [n,h,w] u8.  16-byte vectors for c = 1, 3, 4 on 16-byte aligned tensors. */
int elvis_apply_mask_u8(const uint8_t* frames, const uint8_t* mask, uint8_t* out, int n, int h, int w, int c, int invert,
                        elvis_stream_t stream);

#define ELVIS_SSIM_LUMA 0      /* source: Y = (1868 B + 9617 G + 4899 R + 8192) >> 14 of a BGR pixel, one output per frame */
#define ELVIS_SSIM_CHANNELS 1  /* source: every channel on its own, value / scale */
#define ELVIS_SSIM_REFLECT 0   /* border: scipy.ndimage `reflect` at the work area's edge, repeated as often as needed */
#define ELVIS_SSIM_VALID 1     /* border: none, the map is 10 shorter; a dimension under 11 is not smoothed */
#define ELVIS_SSIM_PAD_AUTO (-1)

/* Bytes of the partial-sum workspace elvis_ssim_mean_f64 needs for [n,h,w,c] frames (host query, 0 for a bad shape). */
size_t elvis_ssim_workspace_bytes(int n, int h, int w, int c);

/* Mean of the windowed SSIM map, float64 throughout (no fused contraction), for both evaluators of the reference:
 *   _masked_ssim (elvis.py:674-721: skimage structural_similarity, gaussian_weights, on masked luma):
 *       LUMA, REFLECT, C1 = 6.5025, C2 = 58.5225, scale unused, pad = ELVIS_SSIM_PAD_AUTO
 *   calculate_ssim (presley.py:248-259: pytorch_msssim.ssim): CHANNELS, VALID, scale = 255, C1 = 1e-4, C2 = 9e-4,
 *       cov_norm = 1, pad = 0
 * a, b: [n,h,w,c] u8 (c <= 4; LUMA needs c = 3).  mask: [n,h,w] u8 or NULL, samples are zeroed where it is 0
 * (elvis.py:696-697).  rects: int32 [n,4] = y0, y1, x0, x1 per frame (exclusive ends, clipped to the frame) or NULL for
 * whole frames: the work area the window reflects in and the map is taken over.  win11: device f64[11].
 * With moments ux, uy, uxx, uyy, uxy: vx = cov_norm (uxx - ux^2), likewise vy, vxy;
 * S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)); out f64 [n, C] (C = 1 for LUMA) is the mean of S
 * over the map shrunk by pad on every side.  pad = ELVIS_SSIM_PAD_AUTO takes pad and cov_norm per frame from the work
 * area by elvis.py:702-711 (win = 7, or the largest odd number <= a smallest side of 3..6; pad = (win-1)/2,
 * cov_norm = win^2/(win^2-1)), so a batch of unequal crops is one call.  A frame with nothing to average (empty
 * rectangle, smallest side < 3 under the automatic rule, pad >= half a side) gives 1.0 (elvis.py:685-686, 704-706).
 * One workgroup per 16x32 map tile writes one partial sum to workspace (elvis_ssim_workspace_bytes); a second launch
 * adds a frame's partials in a fixed order: no float atomics, and a frame's result does not depend on n. */
int elvis_ssim_mean_f64(const uint8_t* a, const uint8_t* b, const uint8_t* mask, const int32_t* rects, const double* win11,
                        double* workspace, double* out, int n, int h, int w, int c, int source, int border, double C1,
                        double C2, double cov_norm, int pad, double scale, elvis_stream_t stream);

/* ------------------------------------------------------------------ u8 <-> float */

/* dst[n,h,w,pitch] = (div255 ? src_u8/255 : src_u8) * scale + bias for the first 3 channels
 * (optionally swapping R and B), zero for the pad channels.  Replaces the cvtColor/PIL//255 conversions of
 * elvis.py:2959-2960 and RealESRGANer.enhance's pre-processing (elvis.py:2515). */
int elvis_u8_to_float(const uint8_t* src, void* dst, int dtype, int n, int h, int w, int pitch,
                      float scale, float bias, int swap_rb, int div255, elvis_stream_t stream);

/* t = clip(src*scale + bias, 0, 1); dst_u8 = cast(t*255); mode 0 = round-half-even, 1 = truncate
 * (utils.py:324).  Optionally also writes the pre-quantisation t as f32 (n,h,w,3) to `f32_out`
 * (may be NULL) for the max-abs parity report. */
int elvis_float_to_u8(const void* src, int dtype, uint8_t* dst, float* f32_out, int n, int h, int w,
                      int pitch, float scale, float bias, int mode, int swap_rb, elvis_stream_t stream);

/* ------------------------------------------------------------------ model kernels */

typedef struct elvis_conv_desc {
    int dtype;          /* ELVIS_F32 / ELVIS_F16 (activations, weights; fp32 accumulate)      */
    int n, h, w;        /* INPUT spatial size (before the optional nearest 2x upsample)        */
    int cin, cin_pitch; /* channels of input 1 and its pitch                                   */
    int cin2, cin2_pitch; /* optional second input (virtual channel concat), 0 if unused       */
    int cout, cout_pitch; /* logical output channels, output pitch                             */
    int ksize;          /* 1 or 3 (2: one parity of a sub-pixel upsample conv, see `subpixel`)  */
    int stride;         /* 1 or 2                                                              */
    int pad_before;     /* zero padding before (top/left); after is implied by ho/wo           */
    int upsample;       /* 1: input is nearest-upsampled 2x before the conv                    */
    int ho, wo;         /* output spatial size                                                 */
    int act;            /* epilogue activation: 0 none, 1 GELU(erf), 2 SiLU, 3 ReLU            */
    int prologue;       /* 0 none, 1: x <- silu(x*pa[n,c]+pb[n,c]) on load (fused GroupNorm)   */
    int subpixel;       /* ksize == 2 only.  1..4: 1 + parity (2a+b) of the sub-pixel decomposition of
                           "nearest-2x upsample + 3x3 conv": this launch writes output pixels
                           (2y+a, 2x+b) of the 2h x 2w output from 2x2 pre-summed taps.
                           ELVIS_CONV_S2D (5): the space-to-depth form of "pad (0,1,0,1) + 3x3 conv,
                           stride 2" (the autoencoder's Downsample): x is the full-res h x w tensor of
                           C = cin/4 channels, the kernel reads its four (row, column) phases as
                           4C channels of an ho x wo image (ho = h/2, wo = w/2) and applies a 2x2
                           conv whose OIHW weights [cout][4C][2][2] hold W[2ry+py][2rx+px] at input
                           channel (2py+px)*C + c, tap (ry, rx) (zero where 2r+p > 2).  f16, C % 32 == 0.
                           With pad_before = 1 the same kernel runs "3x3 conv, stride 2, pad 1" (the Blur / DCT
                           slots' down convs): the 2x2 taps then sit at phase rows y-1, y and hold
                           W[2ry+py-1][2rx+px-1] (zero where 2r+p < 1).  */
} elvis_conv_desc;
#define ELVIS_CONV_S2D 5

/* Number of bytes of the packed weight buffer for a conv (depends on cin/cin2/cout/ksize/dtype). */
size_t elvis_conv_packed_weight_bytes(const elvis_conv_desc* d);

/* Pack PyTorch OIHW fp32 weights (host or device pointer given by `w_oihw_device`) into the
 * kernel's [tap][kchunk][cout_pad][kvec] layout, converting to `dtype`. */
int elvis_conv_pack_weights(const elvis_conv_desc* d, const float* w_oihw, void* packed,
                            elvis_stream_t stream);

/* y = act(conv(prologue(x [,x2])) + bias) + residual.  Implicit-GEMM on MFMA.  `bias` f32[cout] or
 * NULL, `residual` same dtype as out or NULL, `pa`,`pb` f32[n, cin+cin2] for the prologue.
 * `stats` (may be NULL): per-tile GroupNorm partial sums of the STORED output,
 * f32[elvis_conv_stats_tiles(d)][cout][2]; only for convs where elvis_conv_stats_tiles(d) > 0
 * (3x3 / stride 1 / pad 1 / cout >= 64, the LDS halo-tile kernel).
 * This is the slot where the reference calls RealESRGANer.enhance (elvis.py:2515) /
 * restore_images_batch (elvis.py:2963-2970): the conv/linear layers of the restorer. */
int elvis_conv2d(const elvis_conv_desc* d, const void* x, const void* x2, const void* w_packed,
                 const float* bias, const void* residual, int residual_pitch, const float* pa,
                 const float* pb, void* out, float* stats, elvis_stream_t stream);

/* Number of per-tile statistics rows `elvis_conv2d` writes for this conv (n * tiles per image),
 * 0 when the conv cannot produce fused statistics. */
int elvis_conv_stats_tiles(const elvis_conv_desc* d);

/* Writes the name of the kernel instantiation `elvis_conv2d` dispatches this conv to (the template
 * name rocprofv3's kernel trace shows, e.g. "conv3x3_halo_kernel<half,128,256,6,true,3,false>")
 * into buf (NUL-terminated, truncated to n).  For per-kernel profiling (bench.py roofline). */
int elvis_conv_kernel_name(const elvis_conv_desc* d, char* buf, size_t n);

/* The same for a call that passes a residual (has_residual != 0) and / or a statistics buffer (has_stats != 0): such
 * a call never runs on the weight-stationary kernel, whatever its shape.  elvis_conv_kernel_name(d, ...) is
 * elvis_conv_kernel_name_for_call(d, 0, 0, ...); both come from the selection rule elvis_conv2d dispatches by. */
int elvis_conv_kernel_name_for_call(const elvis_conv_desc* d, int has_residual, int has_stats, char* buf, size_t n);

/* Test switch: "no_halo" = 1 routes every conv to the generic implicit-GEMM kernel (tests compare the halo kernels with
 * it); 0 and -1 return to the default dispatch. */
int elvis_conv_debug_set(const char* key, int value);

/* 1 when a descriptor with dtype ELVIS_F32X3 has a compensated-f16 kernel (3x3 stride 1 / sub-pixel 2x2 / 1x1 on the
 * halo-tile kernels with a 64- or 128-channel output tile), else 0.  ELVIS_F32X3 weights are packed by
 * elvis_conv_pack_weights as f16 (hi, lo) parts - planes of 32 channels for 3x3 layers (three MFMAs per 32 channels),
 * interleaved pairs otherwise (four) - which only those kernels read: run every other conv as ELVIS_F32 with weights
 * packed as ELVIS_F32 (elvis_conv2d refuses an ELVIS_F32X3 descriptor that is not eligible). */
int elvis_conv_x3_eligible(const elvis_conv_desc* d);

/* sums[n, sums_coff + c, 0..1] = sum over the image's tiles of partials[tile][c][0..1] (f64). */
int elvis_gn_partials_to_sums(const float* partials, int tiles_per_image, int n, int c, double* sums,
                              int sums_ctot, int sums_coff, elvis_stream_t stream);

/* GroupNorm statistics of a tensor that has no fused statistics: per-(n,channel) sum and sum of
 * squares into sums[n, sums_ctot, 2] f64 at channels [sums_coff, sums_coff+c) (a virtual concat of
 * two tensors shares one buffer).  One partial row per workgroup is written to `workspace`
 * (elvis_groupnorm_workspace_floats(...) floats) and reduced in a fixed order: bit-reproducible,
 * no atomics. */
size_t elvis_groupnorm_workspace_floats(int dtype, int n, int hw, int c);
int elvis_groupnorm_sums(const void* x, int dtype, int n, int hw, int c, int pitch, double* sums,
                         int sums_ctot, int sums_coff, float* workspace, elvis_stream_t stream);

/* Turn sums into per-(n,channel) affine pa,pb so that GN(x)*(1+scale)+shift == x*pa+pb.
 * gamma,beta f32[c]; scale,shift f32[c] may be NULL (then 0). */
int elvis_groupnorm_affine(const double* sums, const float* gamma, const float* beta, const float* scale,
                           const float* shift, float* pa, float* pb, int n, int hw, int c, int groups,
                           float eps, elvis_stream_t stream);

/* elvis_gn_partials_to_sums followed by elvis_groupnorm_affine in one launch, for the case where all c channels come from
 * one partials buffer [n * tiles_per_image, c, 2]: same fp64 operations in the same order, bit-identical pa / pb
 * (csrc/gn_fused.hip).  elvis_gn_partials_affine_span(c, groups) is the number of channels one workgroup covers, 0 when
 * the shape is not served (more than 32 channels per group): callers then keep the two entries above. */
int elvis_gn_partials_affine_span(int c, int groups);
int elvis_gn_partials_affine(const float* partials, int tiles_per_image, const float* gamma, const float* beta,
                             const float* scale, const float* shift, float* pa, float* pb, int n, int hw, int c,
                             int groups, float eps, elvis_stream_t stream);

/* Pad channels.  pitch_for(c) = c rounded up to a multiple of 8 is the pitch a tensor of c channels needs; the convs
 * read whole 8-channel groups, so what an op leaves in [c, pitch_out) is part of its contract:
 *   elvis_affine_act, elvis_layernorm        zero [c, pitch_for(c)) (f16 and f32), leave [pitch_for(c), pitch_out) alone
 *   elvis_u8_to_float (c = 3), elvis_bicubic_upsample, elvis_vq_nearest, elvis_crop_copy     zero [c, pitch_out)
 *   elvis_pad_reflect_axpy                   writes [ch_offset_out, ch_offset_out + c) only
 *   elvis_convert_act                        converts all `pitch` channels
 * Pad channels of an INPUT are loaded with the vectors they share and ignored (they may hold anything, NaN included).
 * elvis_groupnorm_sums, elvis_affine_act and elvis_layernorm move 16-byte vectors: x (and y) must be 16-byte aligned
 * and the pitches multiples of 8, else ELVIS_E_INVALID before anything is launched. */

/* y = act(x*pa[n,c] + pb[n,c]); act 0 none / 2 SiLU.  In-place allowed. */
int elvis_affine_act(const void* x, void* y, int dtype, int n, int hw, int c, int pitch_in,
                     int pitch_out, const float* pa, const float* pb, int act, elvis_stream_t stream);

/* LayerNorm over the channel dim of each token. */
int elvis_layernorm(const void* x, void* y, int dtype, long long tokens, int c, int pitch_in,
                    int pitch_out, const float* gamma, const float* beta, float eps, elvis_stream_t stream);

/* Fused per-token blocks of a Swin layer, f16 tensors, fp32 accumulate (csrc/swin.hip; model slots a5 / a7 of SURVEY.md 8a:
 * the reference delegates these layers to absent pip packages, there is no reference file:line for them).
 *   elvis_swin_mlp       : out = x + fc2(GELU(fc1(LayerNorm(x))))   - one launch, the hidden tensor never reaches HBM
 *   elvis_swin_ln_linear : out = W . LayerNorm(x) + bias            - LayerNorm fused into a projection (qkv)
 * c (channels) in {64, 128, 192, 256}; hidden / n_out multiples of 64; x[tokens, x_pitch], out[tokens, out_pitch] f16;
 * biases, gamma, beta f32; all pointers 16-byte aligned.  Weights are packed once by elvis_swin_pack_weights from
 * row-major f32 matrices w1[n1, c] (fc1 or the projection) and, for the MLP, w2[c, n1] (fc2) into
 * elvis_swin_packed_bytes(c, n1, mlp) bytes. */
size_t elvis_swin_packed_bytes(int c, int n1, int mode);   /* mode 0: LN + linear, 1: MLP, 2: projection + MLP */
int elvis_swin_pack_weights(const float* w1, const float* w2, void* packed, int c, int n1, int mlp, elvis_stream_t stream);
int elvis_swin_mlp(const void* x, void* out, const void* packed, const float* b1, const float* b2, const float* gamma,
                   const float* beta, long long tokens, int c, int hidden, int x_pitch, int out_pitch, float eps,
                   elvis_stream_t stream);
int elvis_swin_ln_linear(const void* x, void* out, const void* packed, const float* bias, const float* gamma, const float* beta,
                         long long tokens, int c, int n_out, int x_pitch, int out_pitch, float eps, elvis_stream_t stream);
/*   elvis_swin_proj_mlp  : y' = y + Wp . attn + bp ; out = y' + fc2(GELU(fc1(LayerNorm(y'))))  - the attention output projection
 *                          folded in front of the MLP (y' never reaches HBM).  Weights packed by elvis_swin_pack_proj_mlp from
 *                          wp[c, c], w1[hidden, c], w2[c, hidden] into elvis_swin_packed_bytes(c, hidden, 2) bytes. */
int elvis_swin_pack_proj_mlp(const float* wp, const float* w1, const float* w2, void* packed, int c, int hidden, elvis_stream_t stream);
int elvis_swin_proj_mlp(const void* attn, const void* y, void* out, const void* packed, const float* bp, const float* b1,
                        const float* b2, const float* gamma, const float* beta, long long tokens, int c, int hidden,
                        int attn_pitch, int y_pitch, int out_pitch, float eps, elvis_stream_t stream);

/* Normalised instantiation name (e.g. "swin_fused_kernel<192,2,1,true>", "dcnv2_tile_kernel<7>") of the last kernel that
 * elvis_window_attention, elvis_swin_*, elvis_dcnv2, elvis_block_gather_u8, elvis_inpaint_prepare ("inpaint_scatter_kernel", its
 * last), elvis_inpaint_fill ("inpaint_fill_kernel<3>"; unchanged when it launches nothing), elvis_tfill ("tfill_kernel<3>"),
 * elvis_gn_partials_affine ("gn_partials_affine_kernel<8>" / "<4>"), elvis_vq_nearest_indexed ("vq_grid_nearest_kernel<half>" / "<float>"),
 * or an entry point of csrc/norm.hip / csrc/misc.hip
 * (elvis_groupnorm_sums reports its gn_channel_sums_kernel, elvis_gn_partials_to_sums which of its two reductions it chose)
 * launched on the calling thread; "" before the first.  Static storage:
 * no allocation, no device synchronisation. */
const char* elvis_last_launch(void);

/* Swin (shifted-)window attention on a token image qkv[n,h,w,3*E] (q|k|v, head-major inside
 * each), window ws, `shift` cyclic shift (0 or ws/2) with the standard region mask, relative
 * position bias table [(2ws-1)^2, heads] f32.  out[n,h,w,E] in image order (un-shifted).  Pitches are multiples of 8;
 * f16 tensors are 16-byte aligned. */
int elvis_window_attention(const void* qkv, void* out, int dtype, int n, int h, int w, int heads,
                           int head_dim, int ws, int shift, int qkv_pitch, int out_pitch,
                           const float* bias_table, float scale, elvis_stream_t stream);

/* PyTorch bicubic (A=-0.75, align_corners=False) x`sf` upsample of a float NHWC image. */
int elvis_bicubic_upsample(const void* x, void* y, int dtype, int n, int h, int w, int c, int pitch_in,
                           int pitch_out, int sf, elvis_stream_t stream);

/* Nearest-codebook lookup: zq = codebook[argmin_k sum_c (z_c - e_kc)^2] (first index wins). */
int elvis_vq_nearest(const void* z, void* zq, int32_t* idx_out, int dtype, long long pixels, int c,
                     int pitch_in, int pitch_out, const float* codebook, int n_embed, elvis_stream_t stream);

/* The same lookup through a uniform grid over the codebook, c == 3 only (csrc/vq_index.hip): value for value the result of
 * elvis_vq_nearest - indices, zq and pad channels - for finite inputs, visiting only the cells that can hold the minimum.
 * elvis_vq_index_build lays a finite device codebook out into `workspace` (elvis_vq_index_bytes(n_embed, c) bytes of device
 * memory, 16-byte aligned; 0 bytes: no index for this shape); it synchronises the stream and is meant to run once per
 * loaded codebook.  elvis_vq_nearest_indexed takes elvis_vq_nearest's arguments and that index. */
size_t elvis_vq_index_bytes(int n_embed, int c);
int elvis_vq_index_build(const float* codebook, int n_embed, int c, void* workspace, elvis_stream_t stream);
int elvis_vq_nearest_indexed(const void* z, void* zq, int32_t* idx_out, int dtype, long long pixels, int c,
                             int pitch_in, int pitch_out, const float* codebook, int n_embed, const void* index,
                             elvis_stream_t stream);

/* Reflect-pad (right/bottom) copy of a float NHWC image into a larger one, optionally into a
 * channel slice, with y = x*mul + add_mul*add[...] (used for x_T = z_y + kappa*sqrt(eta)*eps
 * and the 1/sqrt(eta*kappa^2+1) input scaling; `add` is f32 NCHW noise or NULL). */
int elvis_pad_reflect_axpy(const void* x, void* y, int dtype, int n, int h, int w, int c, int pitch_in,
                           int hp, int wp, int pitch_out, int ch_offset_out, float mul, const float* add,
                           float add_mul, elvis_stream_t stream);

/* y[n,h,w,:c] = x[n,:h,:w,:c] crop-copy between pitched tensors (dtype-preserving). */
int elvis_crop_copy(const void* x, void* y, int dtype, int n, int h_in, int w_in, int pitch_in, int h,
                    int w, int c, int pitch_out, elvis_stream_t stream);

/* y = (dst dtype) x for a pitched NHWC tensor of `pixels` x `pitch` elements (pitch % 8 == 0; f16 <-> f32):
 * the section boundaries of the mixed-precision mode.  No reference counterpart. */
int elvis_convert_act(const void* x, int src_dtype, void* y, int dst_dtype, long long pixels, int pitch,
                      elvis_stream_t stream);

/* ------------------------------------------------------------------ server-side degrade filters
 * Every block_size x block_size block of a uint8 NHWC frame is filtered as its own image (nothing leaks between
 * blocks); map[n, by, bx] int32 with by = H / block_size, bx = W / block_size (H, W divisible by block_size). */

/* filter_frame_downsample (elvis.py:2141-2169): per block, INTER_AREA downscale by 2**level then INTER_LINEAR
 * back to block_size (OpenCV's u8 fixed-point rules restated; block_size a power of two <= 16).  Levels are clamped
 * to [0, 4] (a negative level copies the block; the factor is at most 16); a factor above block_size averages the
 * whole block (s = max(1, block_size >> level)). */
int elvis_degrade_downsample_u8(const uint8_t* src, const int32_t* levels, uint8_t* dst, int n, int h, int w, int c,
                                int block_size, int by, int bx, elvis_stream_t stream);

/* filter_frame_gaussian (elvis.py:2171-2196): per block, `rounds` passes of a separable 5-tap Gaussian with the
 * symmetric taps (tap0, tap1, tap2, tap1, tap0), BORDER_REFLECT_101 at the block's own edges, float32
 * arithmetic, round-half-even to uint8 after every pass pair (any block_size in [1, 16]).  `rounds` is clamped to
 * [0, 32] (a negative count copies the block). */
int elvis_degrade_gaussian_u8(const uint8_t* src, const int32_t* rounds, uint8_t* dst, int n, int h, int w, int c,
                              int block_size, int by, int bx, float tap0, float tap1, float tap2, elvis_stream_t stream);

/* DCT-coefficient dampening (the build's definition of ELVIS v2 DCT's degrade; README.md:44 names it, the reference
 * holds no code): 8x8 blocks; basis64 = f32[8][8] DCT-II basis, gain = f32[n_levels][8][8] per-level coefficient
 * gains (both device pointers), level clamped to [0, n_levels) (a negative level copies the block, a level of
 * n_levels or more takes the gains of n_levels - 1). */
int elvis_degrade_dct_u8(const uint8_t* src, const int32_t* levels, uint8_t* dst, const float* basis64, const float* gain,
                         int n_levels, int n, int h, int w, int c, int by, int bx, elvis_stream_t stream);

/* ------------------------------------------------------------------ Presley's adaptive degraders
 * utils.py:1101-1217 and presley.py:968-1039 in OpenCV's 8-bit arithmetic (restated, parity with cv2 unpinned).
 * One wave per block; map[n, by, bx] int32 with by = H / block_size, bx = W / block_size (floor).  PIXELS OUTSIDE
 * THE BLOCK GRID are never written: dst keeps there what the caller put (the Python layer starts from a copy of src).
 * Any block_size in [2, 32], 1 <= C <= 4. */

#define ELVIS_DEGRADE_MAX_ROUNDS 64

/* downscale_block (presley.py:978-983) and the block loop of degrade_adaptive_downsample (utils.py:1153-1161): a block
 * of scale >= 2 is INTER_AREA-resized to d = max(1, block_size / scale) and INTER_LINEAR-resized back; scale <= 1
 * copies the block.  block_size % d == 0 takes the integer-ratio rule of elvis_degrade_downsample_u8; any other d
 * takes cv::ResizeArea_<uchar, float> with the computeResizeAreaTab table of block_size -> d, built by
 * elvis_amd/degrade.py for every d in [1, block_size / 2] (device pointers): the entries of destination index i are
 * tab_src / tab_w[tab_starts[d * (block_size / 2 + 2) + i] .. tab_starts[d * (block_size / 2 + 2) + i + 1]), all
 * below tab_len; a d has at most 2 * block_size entries. */
int elvis_degrade_scale_u8(const uint8_t* src, const int32_t* scales, uint8_t* dst, int n, int h, int w, int c,
                           int block_size, int by, int bx, const int32_t* tab_starts, const int32_t* tab_src,
                           const float* tab_w, int tab_len, elvis_stream_t stream);

/* blur_block (presley.py:986-990) and the block loop of degrade_adaptive_blur (utils.py:1203-1210): `rounds` passes of
 * cv2.GaussianBlur(block, (5, 5), 1.0) on CV_8U: 8.8 fixed-point taps (tap0, tap1, tap2, tap1, tap0) that sum to 256
 * (14, 62, 104 from the host), u8 x tap summed in u16, u16 x tap summed in u32, one rounding (acc + 0x8000) >> 16,
 * BORDER_REFLECT_101 at the block's own edges.  `rounds` is clamped to [0, ELVIS_DEGRADE_MAX_ROUNDS] (a negative
 * count copies the block; the Python layer rejects larger ones). */
int elvis_degrade_gaussian_fx_u8(const uint8_t* src, const int32_t* rounds, uint8_t* dst, int n, int h, int w, int c,
                                 int block_size, int by, int bx, int tap0, int tap1, int tap2, elvis_stream_t stream);

/* ------------------------------------------------------------------ encoder hand-off (handoff.hip) */

/* cv2.cvtColor(frame, COLOR_RGB2YUV_I420) per frame (write_y4m, utils.py:453-462 and presley.py:590-599;
 * convert_frames_to_yuv420p, presley.py:217-223); bgr != 0 reads B,G,R (COLOR_BGR2YUV_I420).  src: [n,h,w,3] u8;
 * dst: [n, h*3/2, w] u8 - per frame the Y plane h x w, then U h/2 x w/2, then V h/2 x w/2, each dense.  OpenCV 4.x
 * RGB8toYUV420pInvoker restated (parity with cv2 unpinned), int32, 20-bit fixed point:
 *   Y = ( 269484 R + 528482 G + 102760 B + (1 << 19) +  (16 << 20)) >> 20   for every pixel,
 *   U = (-155188 R - 305135 G + 460324 B + (1 << 19) + (128 << 20)) >> 20
 *   V = ( 460324 R - 385875 G -  74448 B + (1 << 19) + (128 << 20)) >> 20   of the pixel at the even row and even column
 * of each 2x2 quad (not the quad's average).  Every output lies in [16, 240].  An odd h or w, a negative dimension or a
 * null pointer with work to do is ELVIS_E_INVALID before anything is launched; n == 0 does nothing and succeeds.  Rows
 * go out as dwords when w % 4 == 0 and both pointers are 4-byte aligned, byte by byte otherwise. */
int elvis_rgb_to_i420_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int bgr, elvis_stream_t stream);

/* ------------------------------------------------------------------ decoder hand-off (i420_in.hip) */

/* cv2.cvtColor(planes, COLOR_YUV2RGB_I420) per frame, the way back from elvis_rgb_to_i420_u8: what a decoder emits
 * (ffmpeg -f yuv4mpegpipe / rawvideo yuv420p in place of the decode_video(...%05d.png) of run_elvis) to the resident
 * clip every restorer takes; bgr != 0 writes B,G,R (COLOR_YUV2BGR_I420).  src: [n, h*3/2, w] u8 - per frame the Y
 * plane h x w, then U h/2 x w/2, then V h/2 x w/2, each dense; dst: [n,h,w,3] u8.  OpenCV 4.x YUV420p2RGB8Invoker
 * restated (parity with cv2 unpinned), int32, 20-bit fixed point: with u = U[y/2][x/2] - 128, v = V[y/2][x/2] - 128
 * (the quad's one chroma pair, replicated, not interpolated) and yy = max(0, Y[y][x] - 16) * 1220542 + (1 << 19),
 *   R = sat8((yy + 1673527 v)             >> 20)
 *   G = sat8((yy -  852492 v - 409993 u)  >> 20)
 *   B = sat8((yy + 2116026 u)             >> 20)
 * where >> is an arithmetic shift (a negative sum floors, then saturates to 0) and sat8 clamps to [0, 255].  An odd h
 * or w, a negative dimension or a null pointer with work to do is ELVIS_E_INVALID before anything is launched; n == 0
 * does nothing and succeeds.  Rows move 16 bytes at a time when w % 16 == 0 and both pointers are 16-byte aligned
 * (i420_to_rgb_x16_kernel), as dwords when w % 4 == 0 and both are 4-byte aligned, byte by byte otherwise
 * (i420_to_rgb_kernel); elvis_last_launch names the kernel, "<rgb>" or "<bgr>". */
int elvis_i420_to_rgb_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int bgr, elvis_stream_t stream);

/* ------------------------------------------------------------------ classical restorers
 * The OpenCV baselines of ELVIS and Presley, per block of a uint8 NHWC frame; map[n, by, bx] int32 with
 * by = H / block_size, bx = W / block_size (floor).  PIXELS OUTSIDE THE BLOCK GRID (the rows and columns past the last
 * whole block) are never written: dst keeps there what the caller put (the Python layer starts from a copy of src);
 * they are read, as halo, by the unsharp mask of a neighbouring block.
 * block_size is a power of two in [2, 32], 1 <= C <= 4.  OpenCV's 8-bit fixed-point rules are restated
 * (parity with cv2 unpinned); the tap tables are device pointers built by elvis_amd/classical.py. */

#define ELVIS_CLASSICAL_MAX_LEVEL 16

/* restore_downsample_opencv_lanczos (elvis.py:2773-2820): a block of level L > 0 is INTER_AREA-downscaled to
 * s = max(1, block_size >> L) and INTER_LANCZOS4-resized back; level 0 is copied.  Levels are clamped to
 * [0, ELVIS_CLASSICAL_MAX_LEVEL] (a negative level copies the block; the Python layer rejects larger ones; every
 * level above log2(block_size) gives s = 1, so the upper clamp changes no output).  taps = int16[5][32][8]: the 11-bit
 * Lanczos taps of destination index d for the factor 2^(i+1). */
int elvis_classical_lanczos_u8(const uint8_t* src, const int32_t* levels, uint8_t* dst, int n, int h, int w, int c,
                               int block_size, int by, int bx, const int16_t* taps, elvis_stream_t stream);

/* restore_blur_opencv_unsharp_mask (elvis.py:2822-2866) and restore_with_opencv_lanczos / _unsharp
 * (utils.py:1253-1392): a block of level L > 0 gets GaussianBlur(sigma L, ksize 6L+1, BORDER_REFLECT_101) and
 * addWeighted(tile, 1 + L/2, blurred, -L/2, 0) on its tile - the block grown by `halo` (0..32) pixels and
 * clipped at the frame; only the block is written.  taps = int16 8-bit Gaussian taps of level L at
 * taps[tap_offsets[L] ...], 6L+1 of them, for L in [1, max_level]; levels are clamped to [0, max_level]
 * (a negative level copies the block, a larger one is sharpened as max_level; max_level <=
 * ELVIS_CLASSICAL_MAX_LEVEL; the Python layer rejects larger ones). */
int elvis_classical_unsharp_u8(const uint8_t* src, const int32_t* levels, uint8_t* dst, int n, int h, int w, int c,
                               int block_size, int by, int bx, int halo, const int16_t* taps, const int32_t* tap_offsets,
                               int max_level, elvis_stream_t stream);

/* temporal_blend of utils.py:1308-1312 over a clip of `nframes` frames of `pixels` u8 elements each:
 * out[0] = cur[0]; out[f] = trunc(tb * out[f-1] + one_minus_tb * cur[f]) in float64, 0 <= tb, one_minus_tb <= 1.
 * In-place (out == cur) allowed. */
int elvis_temporal_blend_u8(const uint8_t* cur, uint8_t* out, int nframes, long long pixels, double tb,
                            double one_minus_tb, elvis_stream_t stream);

/* ------------------------------------------------------------------ ELVIS v1 block removal
 * Shrink (the server removes the least important blocks of a frame) and stretch (the client puts the kept blocks
 * back and gets the hole mask for the inpainter) on uint8 NHWC clips.  Every shrink and every stretch is one
 * block gather driven by an int32 index map; the entry points below build the maps on the device.  Scores are
 * float64 and FINITE (no NaN; the Python layer rejects them); they are only compared, never rounded. */

#define ELVIS_SHRINK_ROWS 0        /* shrink_frame_row_only: row passes only */
#define ELVIS_SHRINK_ROWS_COLS 1   /* shrink_frame_position_map / _removal_indices: row pass, column pass, ... */
#define ELVIS_STRETCH_FLAT 0       /* stretch_frame, stretch_video_frames: rank over the whole frame, row-major */
#define ELVIS_STRETCH_ROWS 1       /* stretch_frame_row_only: rank inside the block row */

/* dst[n, y, x] = src block src_of[n, y, x] (a flat index into the sby x sbx source grid of the same frame), a zero
 * block where src_of < 0 or beyond the source grid.  src u8 [n, hs, ws, c] with hs >= sby*block_size and
 * ws >= sbx*block_size (rows and columns past the grid are never read: the crop of utils.py:707); dst u8
 * [n, dby*block_size, dbx*block_size, c]; src_of int32 [n, dby, dbx].  mask_out (may be NULL): u8
 * [n, dby*block_size, dbx*block_size], 255 on the pixels of a zero block, 0 elsewhere - the inpainter's mask of
 * elvis.py:4560-4575 in the same launch.  Any block_size >= 1, c in {1, 3}; a sby x sbx = 0 source gives all holes. */
int elvis_block_gather_u8(const uint8_t* src, const int32_t* src_of, uint8_t* dst, uint8_t* mask_out, int n, int hs,
                          int ws, int c, int block_size, int sby, int sbx, int dby, int dbx, elvis_stream_t stream);

/* apply_selective_removal (elvis.py:1387-1427), selection step: per block row, column i is removed iff fewer than k
 * columns j have s_j > s_i, or s_j == s_i and j < i - the k highest scores.  TIE RULE: among equal scores the lower
 * column goes first; the reference's np.argsort(-row) is not a stable sort, so its ties are not defined.
 * scores f64 [n, by, bx]; mask int8 [n, by, bx] (1 = removed); src_of int32 [n, by, bx - k]: the kept columns of
 * every row in order, as flat indices into the by x bx grid (the map of the shrink).  0 <= k <= bx; src_of may be
 * NULL when k == bx. */
int elvis_shrink_select_topk(const double* scores, int8_t* mask, int32_t* src_of, int n, int by, int bx, int k,
                             elvis_stream_t stream);

/* Host only (no device work): the shrunk grid *sby x *sbx of the pass rule below and the number of removals of each
 * pass (the first min(max_passes, return value) entries of pass_counts; pass_counts may be NULL with max_passes 0).
 * Returns the number of passes (>= 0) or ELVIS_E_INVALID.  A function of (by, bx, target, mode) alone. */
int elvis_shrink_passes_plan(int by, int bx, int target, int mode, int* sby, int* sbx, int* pass_counts, int max_passes);

/* shrink_frame_row_only (utils.py:692-736), shrink_frame_position_map (:763-836) and shrink_frame_removal_indices
 * (:862-948), selection step.  Until `target` = int(by * bx * shrink_amount) blocks are gone: a row pass removes from
 * every row (in order) its current argmin - first index on ties, as np.argmin - and shifts the row left; with
 * ELVIS_SHRINK_ROWS_COLS a column pass follows (argmin of every column, shift up), then a row pass, ...
 * PARTIAL PASSES: a pass that reaches the target midway stops there.  ELVIS_SHRINK_ROWS still drops the last column
 * (rows the pass did not reach lose their last block without a mask entry) and never goes below one column;
 * ELVIS_SHRINK_ROWS_COLS keeps the dimension, so the shrunk grid ends with stale duplicates of the shifted lines.
 * scores f64 [n, by, bx]; mask u8 [n, by, bx] (1 = removed); src_of int32 [n, sby, sbx]: the position map of the
 * shrunk grid as flat indices (y * bx + x) into the by x bx grid; removal_idx (may be NULL) int32 [n, target]: the
 * argmins in removal order (split per pass with elvis_shrink_passes_plan); ws_scores f64 / ws_pos int32
 * [n, by, bx]: scratch.  sby, sbx must be what elvis_shrink_passes_plan gives. */
int elvis_shrink_select_passes(const double* scores, uint8_t* mask, int32_t* src_of, int32_t* removal_idx,
                               double* ws_scores, int32_t* ws_pos, int n, int by, int bx, int target, int mode, int sby,
                               int sbx, elvis_stream_t stream);

/* The index map of a stretch whose side data is a mask (u8 [n, by, bx], non-zero = removed): src_of int32
 * [n, by, bx] = the rank of a kept block among the kept blocks - of the frame in row-major order
 * (ELVIS_STRETCH_FLAT: stretch_frame elvis.py:1436-1455, stretch_video_frames presley.py:787-827), or of its row,
 * plus row * sbx (ELVIS_STRETCH_ROWS: stretch_frame_row_only utils.py:739-759) - and -1 for a removed block or a
 * rank outside the sby x sbx shrunk grid (the bounds checks of the Presley and row-only forms).  stretch_frame
 * itself raises when the kept count differs from sby * sbx: a precondition here, checked by the Python layer. */
int elvis_stretch_index(const uint8_t* mask, int32_t* src_of, int n, int by, int bx, int sby, int sbx, int mode,
                        elvis_stream_t stream);

/* ------------------------------------------------------------------ ELVIS v1 inpaint
 * The step after the stretch: cv2.inpaint(stretched_frame, mask, inpaintRadius=3, flags=cv2.INPAINT_TELEA) in the
 * reference (elvis.py:4601-4606; Presley's inpaint_with_opencv, presley.py:838-850).  This is a BUILD-DEFINED
 * inpainter, "wavefront Telea": Telea's estimator and weights (radius 3) on a fill order a GPU can run - waves by the
 * exact Euclidean distance to the nearest known pixel, every pixel of a wave computed from known pixels and earlier
 * waves only.  It does not claim parity with cv2; DESIGN.md 7 is the contract, tests/_inpaint_ref.py states it in numpy
 * and the kernels equal that bit for bit.
 *
 * Two calls per clip with one small download between them (the caller synchronises, no entry point does):
 *   1. elvis_inpaint_prepare fills the workspace (elvis_inpaint_workspace_bytes bytes, 256-byte aligned).  Its first
 *      h + w + 2 int32 are the number of hole pixels of every wave (entry 0 is 0) over the whole clip.
 *   2. the caller copies those counts to the host (after the stream has finished the prepare) and passes the first
 *      K + 1 of them, K = the last wave with pixels, to elvis_inpaint_fill: one launch per non-empty wave, one thread
 *      per hole pixel.  A clip without holes needs no call (num_counts = 1 launches nothing).
 * n * h * w < 2^31, h and w at most 32767. */

/* Host only: bytes of the workspace of an [n, h, w] clip; 0 for a shape the entry points reject. */
size_t elvis_inpaint_workspace_bytes(int n, int h, int w);

/* mask u8, non-zero = hole (as for cv2.inpaint): [n, h, w] with block_size 0, or [n, h / block_size, w / block_size]
 * expanded over whole blocks with block_size > 0 (pixels past the last whole block are known).  Launches
 * inpaint_rows_kernel, inpaint_columns_kernel (the exact distance transform, T and the wave of every pixel, the
 * histogram), inpaint_scan_kernel and inpaint_scatter_kernel (the per-wave pixel lists). */
int elvis_inpaint_prepare(const uint8_t* mask, int block_size, void* workspace, int n, int h, int w, elvis_stream_t stream);

/* Fills the holes of frames u8 [n, h, w, c] (c in {1, 3}) IN PLACE from the workspace of the same clip.  The bytes
 * under the holes are never read, known pixels are never written; frames without a hole or without a known pixel
 * stay as they are.  wave_counts_host: HOST int32 [num_counts], the first num_counts entries of the workspace. */
int elvis_inpaint_fill(uint8_t* frames, const void* workspace, int n, int h, int w, int c, const int32_t* wave_counts_host,
                       int num_counts, elvis_stream_t stream);

/* ------------------------------------------------------------------ ELVIS v1 temporal fill (tfill.hip)
 * The reference's v1 results come from trained video inpainters (inpaint_with_propainter / inpaint_with_e2fgvi,
 * elvis.py:1458, 1693; utils.py:1395-1425; presley.py:854-885), which take a removed block's content from frames where
 * the same scene point was not removed.  This is a BUILD-DEFINED restatement of the part of those methods that needs no
 * training, in integers: for every block (size B, grid anchored at (0, 0)) of frame t that holds a hole pixel, the
 * window of the block and a margin G is matched against the frames t-1, t+1, t-2, ... t+R over the (2S+1)^2
 * displacements - mean absolute difference over the pixels known in both, exact comparison, ties to the earlier
 * displacement in raster order, at least half of the window's known pixels compared, at most M a channel - and the
 * best displacement's known pixels are copied under the hole.  "Known" is always the input mask and sources are always
 * input bytes, so the result does not depend on any order.  It claims no parity with ProPainter or E2FGVI; DESIGN.md 7
 * is the contract, tests/_tfill_ref.py states it in numpy and the kernel equals that bit for bit.  Holes it cannot fill
 * are reported in `left`, the mask for elvis_inpaint_prepare. */

/* Host only: 1 where elvis_tfill takes the shape and the parameters, 0 otherwise: n, h, w >= 1, c in {1, 3},
 * h, w <= 32767, n * h * w * c < 2^31, B in 1..32, G in 0..16, R in 0..8, S in 0..7, M in 0..255. */
int elvis_tfill_limits_ok(int n, int h, int w, int c, int B, int G, int R, int S, int M);

/* frames u8 [n, h, w, c]; masks u8, non-zero = hole: [n, h, w] with block_mask_size 0, or [n, h / block_mask_size,
 * w / block_mask_size] expanded over whole blocks as for elvis_inpaint_prepare.  out u8 [n, h, w, c]: the frames with
 * the filled pixels (every byte is written; known pixels and pixels under remaining holes get the input's bytes).
 * left u8 [n, h, w]: 255 where a hole stayed unfilled, 0 elsewhere.  out and left may alias neither each other nor an
 * input.  Everything outside the limits is refused before the launch of tfill_kernel<c>. */
int elvis_tfill(const uint8_t* frames, const uint8_t* masks, int block_mask_size, uint8_t* out, uint8_t* left, int n,
                int h, int w, int c, int B, int G, int R, int S, int M, elvis_stream_t stream);

/* ------------------------------------------------------------------ foreground masks (segment.hip)
 * The reference takes its foreground masks from UFO, a trained video salient-object network (presley.py:203
 * `segment_frames(frames, device=device)`; elvis.py:1187 reads its mask files).  Neither UFO's architecture nor its weights
 * are available to this build, so this is a BUILD-DEFINED, training-free segmenter behind that call surface and it claims
 * no parity with UFO.  On the 1/4-resolution grid (Ry = h / 4, Rx = w / 4, P = Ry * Rx; Y, U, V of i420.h summed over
 * 4 x 4 pixels): the global shift in [-R, R]^2 against the previous frame (the first frame: the next) by 64-bit SAD over
 * the common window, ties to the least (dy*dy + dx*dx, dy, dx); the motion residual (3 x 3 min, 3 x 3 sum) and the least
 * colour distance to the means of the four border strips, each scaled to 0..255 by max(its maximum, its floor); their
 * weighted mean, a 5 x 5 mean, Otsu's threshold in float64 (none where the peak is below min_peak); close, open and
 * `dilation` dilations; 2 of 3 over t - 1, t, t + 1; all ones where the share is 0 or above max_share; x 4 nearest.
 * tests/_segment_ref.py states every stage in numpy and the kernels equal it bit for bit.
 *
 * The extended clip is before (n_before in 0..2 frames) + frames (n) + after (n_after in 0..1), m frames of [h, w, c] u8,
 * c in {1, 3} (bgr: the channel order of c == 3).  Frame e > 0 of it is paired with e - 1, frame 0 with frame 1; with two
 * frames before, the first is a partner only.  m <= 4096, 4 <= h, w <= 16384, Ry and Rx >= 2 * radius + 1, radius in
 * 0..16, dilation in 0..4, weights in 1..1024, floors >= 1, min_peak in 0..255, share_num = max_share * 10000 in 1..10000.
 *
 * The workspace (device, 8-byte aligned, caller-owned) holds every intermediate, each section at the next multiple of
 * 256 bytes, in this order, with D = 2 * radius + 1:
 *   red u16 [m][3][P] | sad u64 [m][D*D] | maxima i32 [m][2] | hist u32 [m][256] | count u32 [m] | shift i32 [m][2] |
 *   means i32 [m][4][3] | M u16 [m][P] | S u16 [m][P] | Mn u8 [m][P] | Sn u8 [m][P] | F u8 [m][P] | thr i32 [m] |
 *   pre u8 [m][P] (the mask before the vote) | voted u8 [m][P] (the first n frames)
 * elvis_segment_workspace_bytes returns their total, 0 for a shape the entry point refuses. */
size_t elvis_segment_workspace_bytes(int m, int h, int w, int radius);

/* masks u8 [n, h, w] of 0 / 1.  Ten launches (eight for a clip of one frame, which has no motion term) and one memset
 * on `stream`, nothing read back; the last launch is seg_upsample_kernel.  The inputs are not written. */
int elvis_segment_foreground_u8(const uint8_t* frames, const uint8_t* before, int n_before, const uint8_t* after, int n_after,
                                uint8_t* masks, void* workspace, long long workspace_bytes, int n, int h, int w, int c, int bgr,
                                int radius, int motion_weight, int spatial_weight, int motion_floor, int spatial_floor,
                                int min_peak, int dilation, int share_num, int temporal_vote, elvis_stream_t stream);

/* ------------------------------------------------------------------ block complexity (complexity.hip)
 * The first server-side stage: the per-block spatial (SC) and temporal (TC) complexity maps that the reference takes
 * from EVCA - elvis.py:968-1224 runs it as a subprocess and reads evca_SC_blocks.csv / evca_TC_blocks.csv,
 * presley.py:202 calls analyze_frames(frames, EVCAConfig(block_size=...)) and reads .SC and .TC.  EVCA is available
 * neither to the reference tree nor to this build, so this is a BUILD-DEFINED analyser behind that call surface: a
 * DCT-energy block complexity in the published VCA form.  The contract below is stated in numpy float64 in
 * tests/_complexity_ref.py and the kernel agrees with it to 1e-9 * max(1, |value|); it does not claim EVCA's pixels.
 *
 *   frames  u8 [n, h, w, c], c in {1, 3}; block B in {8, 16, 32}; By = h / B, Bx = w / B (floored).  Rows and columns
 *           past the last whole block belong to no block and are never read (elvis.py:1163-1164).
 *   prev    NULL, or u8 [h, w, c]: the frame before frames[0].
 *   luma    c == 1: the byte.  c == 3: the Y of elvis_rgb_to_i420_u8 above (the same device function), order 0 = RGB,
 *           1 = BGR.
 *   dct     f64 [B, B], built by the host: dct[k][m] = s_k cos(pi (2m + 1) k / 2B), s_0 = sqrt(1 / B), s_k = sqrt(2 / B).
 *   weight  f64 [B, B], built by the host: weight[i][j] = exp(|(i j / B^2)^2 - 1|), weight[0][0] = 0 (no DC term).
 *   SC      of a block X (B x B luma, integers): X' = X - X[0][0]; Cf = D X' D^T in float64;
 *           SC = (sum_ij weight[i][j] |Cf[i][j]|) / B^2.  A flat block gives exactly 0.0.
 *   TC      of frame f against its predecessor p (frames[f - 1]; prev for f = 0): E = X_f - X_p in integers,
 *           E' = E - E[0][0], TC = (sum weight |D E' D^T|) / B^2.  A block whose luma did not change gives exactly 0.0;
 *           without a predecessor TC[0] is 0.0 everywhere.
 *   sc, tc  f64 [n, By, Bx], dense.  Nothing else is written.  No atomics and a fixed summation order: the same input
 *           gives the same bytes, whatever n it is analysed with.
 * ELVIS_E_INVALID: a block other than 8, 16, 32; c other than 1, 3; order other than 0, 1; h < block or w < block; a
 * null frames / dct / weight / sc / tc.  n == 0 is a no-op. */
int elvis_block_complexity_f64(const uint8_t* frames, const uint8_t* prev, const double* dct, const double* weight,
                               double* sc, double* tc, int n, int h, int w, int c, int order, int block,
                               elvis_stream_t stream);

/* ------------------------------------------------------------------ LPIPS, AlexNet (lpips.hip)
 * The perceptual distance of the evaluation report, which the reference takes from lpips.LPIPS(net='alex') for every
 * sampled frame (elvis.py:437-447, 3163-3195, 3887-3893; presley.py:329-357).  The package and its weights are available
 * neither to the reference tree nor to this build, so this is a BUILD-DEFINED restatement behind that call surface,
 * stated in torch float64 in tests/_lpips_ref.py.  It does not claim parity with the lpips package.
 *
 *   stem      x = ((byte / 127.5 - 1) - shift_c) / scale_c in RGB order, shift (-0.030, -0.088, -0.188), scale (0.458,
 *             0.448, 0.450); the byte of a pixel whose mask is 0 is 0 (a masked pixel is affine(0), not 0); the conv's
 *             zero padding is 0 after the affine.  conv 3 -> 64, 11x11, stride 4, pad 2, ReLU      -> tap 0
 *   max-pool  3x3 stride 2, no padding, floor
 *   conv      64 -> 192, 5x5, pad 2, ReLU                                                          -> tap 1
 *   max-pool  the same; then conv 192 -> 384, 384 -> 256, 256 -> 256, 3x3, pad 1, ReLU (elvis_conv2d) -> taps 2, 3, 4
 *   distance  per tap and pixel xh = x / (sqrt(sum_c x^2) + 1e-10), yh likewise, v = sum_c w_c (xh_c - yh_c)^2 in fp32
 *             in a fixed order; the tap's value is the mean of v over its pixels, summed and divided in float64; the
 *             score is the sum of the five tap values in tap order.
 * fp32 with fp32 accumulation throughout.  Activations are NHWC fp32 [n, h, w, pitch], 16-byte aligned, the pitch a
 * multiple of 8.  No atomics: a frame's result does not depend on n or on how a clip is cut into calls.  Every entry
 * point returns ELVIS_E_INVALID before any launch for a null pointer, a bad order, a rect outside the frame or under
 * 31 x 31, and a pitch that is not a multiple of 8 (or smaller than the channel count); n == 0 is a no-op. */

/* elvis.py:3163-3195 (calculate_lpips_per_frame: the BGR -> RGB flip, / 127.5 - 1, and the net's scaling layer and first
 * conv).  frames u8 [n, h, w, 3], order 0 = RGB, 1 = BGR; mask u8 [n, h, w] or null (0: the pixel's three bytes are
 * taken as 0, elvis.py:615-624); the network sees rows y0 .. y1 - 1, columns x0 .. x1 - 1 of the masked frame (the
 * reference's roi_slice crop, elvis.py:3853-3854) - no byte outside the rect is read.  weight f32 [363][64] with row
 * (ky 11 + kx) 3 + c, c in RGB order; bias f32 [64]; out f32 [n, ho, wo, out_pitch], ho = (y1 - y0 - 7) / 4 + 1. */
int elvis_lpips_stem_u8(const uint8_t* frames, const uint8_t* mask, const float* weight, const float* bias, float* out,
                        int n, int h, int w, int y0, int y1, int x0, int x1, int order, int out_pitch,
                        elvis_stream_t stream);
/* elvis.py:3163-3195 (the net's second conv).  x f32 [n, h, w, in_pitch], 64 channels; weight f32 [1600][192] with row
 * (ky 5 + kx) 64 + c; bias f32 [192]; out f32 [n, h, w, out_pitch]: relu(conv 5x5 pad 2 + bias). */
int elvis_lpips_conv5_f32(const float* x, const float* weight, const float* bias, float* out, int n, int h, int w,
                          int in_pitch, int out_pitch, elvis_stream_t stream);
/* elvis.py:3163-3195 (the net's max-pools).  x f32 [n, h, w, in_pitch] -> out f32 [n, (h - 3) / 2 + 1, (w - 3) / 2 + 1,
 * out_pitch], the first c channels (c a multiple of 4; h, w >= 3). */
int elvis_lpips_maxpool_f32(const float* x, float* out, int n, int h, int w, int c, int in_pitch, int out_pitch,
                            elvis_stream_t stream);
/* elvis.py:3163-3195: bytes of the workspace elvis_lpips_distance_f64 needs for n feature maps of h x w pixels (one
 * float64 partial sum per 64 pixels); 0 for a bad shape. */
size_t elvis_lpips_distance_workspace_bytes(int n, int h, int w);
/* elvis.py:3163-3195 (the net's normalize_tensor, squared difference, 1x1 weighting and spatial average of one tap).
 * x, y f32 [n, h, w, pitch] with c <= 384 channels; weight f32 [c]; out f64 [n]: the tap's value, added to out where
 * accumulate is 1 and stored where it is 0.  Two launches: partial sums per workgroup, then their sum in index order. */
int elvis_lpips_distance_f64(const float* x, const float* y, const float* weight, void* workspace, double* out, int n,
                             int h, int w, int c, int pitch, int accumulate, elvis_stream_t stream);

/* ------------------------------------------------------------------ VMAF (vmaf.hip)
 * The third per-frame metric of the evaluation report.  The reference writes both clips to disk as I420 and starts the
 * vmaf binary in a subprocess (elvis.py:3197-3356, presley.py:262-326); neither libvmaf nor its model file is available
 * to this build, so this is a BUILD-DEFINED restatement of the published float feature extractors - VIF on four
 * scales, ADM2 on four scales, motion2 - and of the nu-SVR over them.  The contract is stated in numpy float64 in
 * tests/_vmaf_ref.py (and in words in DESIGN.md 7); the kernels agree with it to 1e-9 * max(1, |value|).  It does not
 * claim libvmaf's numbers.  All arithmetic is float64 on luma less 128, every per-pixel quantity in one stated order
 * (a filter is ((f0 x0 + f1 x1) + f2 x2) + ..., vertical pass first, mirror border without repeating the edge), no FMA
 * contraction, no atomics, fixed summation orders: the same input gives the same bytes, whatever n it is given with.
 *
 * elvis_vmaf_luma_u8: frames u8 [n, h, w, 3] (order 0 rgb, 1 bgr) -> out u8 [n, y1 - y0, x1 - x0], the Y of
 *   elvis_rgb_to_i420_u8 over the rectangle [y0, y1) x [x0, x1), any h and w.  masks NULL, or u8 [n, h, w]: where
 *   (mask != 0) == invert the pixel's three bytes count as 0 (elvis.py:615-624).  n == 0 is a no-op. */
int elvis_vmaf_luma_u8(const uint8_t* frames, const uint8_t* masks, uint8_t* out, int n, int h, int w, int order,
                       int invert, int y0, int y1, int x0, int x1, elvis_stream_t stream);
/* Bytes of the workspace elvis_vmaf_features_f64 needs for n frame pairs of h x w: the pyramids of four frames at a
 * time and every frame's tile partials; 0 for a bad shape (h or w under 64 included). */
size_t elvis_vmaf_workspace_bytes(int n, int h, int w);
/* ref, dis u8 [n, h, w] luma, h, w >= 64 -> out f64 [n, 6] = adm2, motion2, vif_scale0..3.  prev NULL, or u8 [h, w]:
 * the reference frame before ref[0] (without it motion of frame 0 is 0); next NULL, or u8 [h, w]: the one after
 * ref[n - 1] (without it motion2 of the last frame is its motion) - with both, a clip cut into calls gives the bytes
 * of one call.  tables f64 [56]: the filters and constants, built on the host (elvis_amd/vmaf.py vmaf_tables):
 * the normalised Gaussians of 17, 9, 5 and 3 taps, the 5-tap motion blur, the db2 low and high pass, cos^2(1 degree)
 * and per scale 1 / Q for the h, v bands and for the d band.  workspace: elvis_vmaf_workspace_bytes(n, h, w) bytes,
 * 8-byte aligned, written before it is read.  ELVIS_E_INVALID: h or w under 64, n < 0 or n >= 65535, a null ref / dis
 * / tables / workspace / out.  n == 0 is a no-op. */
int elvis_vmaf_features_f64(const uint8_t* ref, const uint8_t* dis, const uint8_t* prev, const uint8_t* next,
                            const double* tables, double* workspace, double* out, int n, int h, int w,
                            elvis_stream_t stream);
/* feats f64 [n, 6] -> out f64 [n], the score.  model f64 [21 + 7 nsv]: slopes[7], intercepts[7], rho, gamma, the clip's
 * two ends, the transform's p0, p1, p2, then the support vectors [nsv, 6] and their coefficients [nsv].
 * x_i = slopes[i + 1] f_i + intercepts[i + 1]; p = sum_j coef_j exp(-gamma |sv_j - x|^2) - rho;
 * s = (p - intercepts[0]) / slopes[0]; flags bit 0: s = p0 + p1 s + p2 s^2, bit 1: no less than the s it came from;
 * bit 2: clipped.  One wave per frame, a fixed summation order. */
int elvis_vmaf_predict_f64(const double* feats, const double* model, double* out, int n, int nsv, int flags,
                           elvis_stream_t stream);

/* ------------------------------------------------------------------ FVMD (fvmd.hip)
 * The sixth quality number of the evaluation report.  The reference hands two clips to the `fvmd` package
 * (track_keypoints, calc_hist, calculate_fd_given_vectors: elvis.py:3476-3505, inside calculate_fvmd,
 * elvis.py:3358-3597).  BUILD-DEFINED: the package is available neither to the reference tree nor to this build; its
 * tracker (PIPs++, a network), its calc_hist and its VideoDataset semantics cannot be read.  This is a restatement of
 * the published form - tracks -> velocity / acceleration -> cell orientation histograms -> Frechet distance - with a
 * pyramidal Lucas-Kanade (KLT) tracker in the network's place.  It does NOT claim parity with the `fvmd` package and its
 * values are not comparable with published FVMD numbers.  It is pinned against its own numpy float64 statement,
 * tests/_fvmd_ref.py (1e-9 * max(1, |value|) per stage), and - for the control flow of calculate_fvmd only - against
 * the reference's own code (tests/golden/fvmd.npz).
 *
 * THE CONTRACT.  All arithmetic is float64, no FMA, every reduction in a fixed order, no float atomics; nothing branches
 * on data except the singular test below.
 *   input      8-bit luma [F, h, w], h, w >= 64, taken as float64 unscaled (a masked pixel is luma 16).
 *   segments   sliding windows of S frames (10 <= S <= 16, the reference's clip_seq_len, elvis.py:3452) starting every
 *              segment_step frames: B = (F - S) / segment_step + 1; each is tracked on its own from a fresh grid.
 *              segment_step is this build's reading of VideoDataset(..., stride=1).
 *   keypoints  20 x 20, x_j = ((j + 0.5) w) / 20 - 0.5, y_i = ((i + 0.5) h) / 20 - 0.5; index i * 20 + j.
 *   pyramid    3 levels; level l + 1 = level l filtered with [1,4,6,4,1] / 16, vertical pass first, taps ascending
 *              (((c0 x0 + c1 x1) + c2 x2) + ...), mirror border without repeating the edge, kept at even indices: size
 *              (n + 1) / 2.
 *   frame step t -> t + 1, per point, levels 2, 1, 0: d = 0 at level 2 and is doubled on the way down; p = position /
 *              2^level; window = the 225 integer offsets |ox|, |oy| <= 7, offset o = (oy + 7) 15 + (ox + 7).  A sample is
 *              bilinear, (1 - ay) ((1 - ax) v00 + ax v01) + ay ((1 - ax) v10 + ax v11), its coordinate clamped to
 *              [0, n - 1] first.  T(o) = I_t(p + o); gx(o) = (I_t(p + o + (1,0)) - I_t(p + o - (1,0))) / 2, gy likewise;
 *              G = sum [gx gx, gx gy; gx gy, gy gy] once per level.  Then exactly 8 iterations, no early exit:
 *              b = sum (T(o) - I_{t+1}((p + o) + d)) (gx, gy); d += G^-1 b by the closed form
 *              ((gyy bx - gxy by) / det, (gxx by - gxy bx) / det).  THE ONE DATA BRANCH: with lambda_min(G) =
 *              ((gxx + gyy) - sqrt((gxx - gyy)^2 + 4 gxy^2)) / 2, a level with lambda_min / 225 < 1e-3 adds no update.
 *              After level 0 the position is p + d clamped to the frame; a point is never dropped.  A sum over the
 *              window is: lane L of 64 adds offsets L, L + 64, L + 128, L + 192 (< 225) in that order, then the
 *              butterfly v += v[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.  Exact consequences: a black (masked) region has
 *              G = 0 and does not move; a static clip has d = 0.
 *   fields     v_t = p_{t+1} - p_t (S - 1 of them), a_t = v_{t+1} - v_t (S - 2), in input pixels.
 *   histograms 4 x 4 cells of 5 x 5 points, 8 bins centred at k pi / 4: for a vector of magnitude m,
 *              u = atan2(y, x) / (pi / 4) (+ 8 where negative), k = floor(u), f = u - k; (1 - f) m goes to bin k mod 8,
 *              f m to bin (k + 1) mod 8 - a soft vote, continuous across a pure horizontal pan where vy is +-1e-17.
 *              A cell's bin is summed over its points in point order.  Row of a segment: velocity fields, then
 *              acceleration fields, each [cell][bin], unnormalised: d = (2 S - 3) 128.
 *   distance   rows A [n, d] (reference) and Bm [m, d] (decoded), each centred by its own column means, n, m >= 2:
 *              FD = |mu_A - mu_B|^2 + |A|_F^2 / (n - 1) + |Bm|_F^2 / (m - 1) - 2 |A Bm^T|_* / sqrt((n - 1)(m - 1)),
 *              |.|_* the sum of singular values.  In exact arithmetic this is tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) with
 *              np.cov covariances: the non-zero eigenvalues of S1 S2 are those of (A Bm^T)(A Bm^T)^T / ((n-1)(m-1)).
 *              The form needs no d x d matrix and no square root of a singular product (n, m << d = 3712 here).
 * n == 0 / no segment is a no-op; ELVIS_E_INVALID before any launch for a bad shape or a null pointer. */

/* elvis.py:3476-3505 (what track_keypoints first does with a clip).  Bytes of the pyramid of `frames` planes of h x w:
 * levels 1 and 2 as float64 (level 0 is the luma itself); 0 for a bad shape (h or w under 64, frames > 65535). */
size_t elvis_fvmd_pyramid_bytes(int frames, int h, int w);
/* elvis.py:3476-3505.  luma u8 [frames, h, w] -> pyramid: level 1 f64 [frames, h1, w1], then level 2 f64
 * [frames, h2, w2], h1 = (h + 1) / 2, h2 = (h1 + 1) / 2 (fvmd_pyr_down_kernel, a lane per output pixel). */
int elvis_fvmd_pyramid_f64(const uint8_t* luma, double* pyramid, int frames, int h, int w, elvis_stream_t stream);
/* elvis.py:3476-3505 (track_keypoints).  luma and its pyramid -> tracks f64 [B, seq_len, 400, 2] = (x, y), B =
 * (frames - seq_len) / segment_step + 1 (nothing is written when frames < seq_len).  One wave per (segment, point),
 * template and gradients in registers across a level's 8 iterations (fvmd_track_kernel).  10 <= seq_len <= 16. */
int elvis_fvmd_track_f64(const uint8_t* luma, const double* pyramid, double* tracks, int frames, int h, int w, int seq_len,
                         int segment_step, elvis_stream_t stream);
/* elvis.py:3476-3505 (calc_hist on velocities and accelerations, concatenated).  tracks f64 [segments, seq_len, 400, 2]
 * -> rows f64 [segments, (2 seq_len - 3) 128] (fvmd_hist_kernel, a workgroup per (segment, field)). */
int elvis_fvmd_features_f64(const double* tracks, double* rows, int segments, int seq_len, elvis_stream_t stream);
/* elvis.py:3476-3505 (calculate_fd_given_vectors).  Bytes of elvis_fvmd_gram_f64's workspace: (2 d + n + m) doubles;
 * 0 for a bad shape (n or m under 2 or over 1024). */
size_t elvis_fvmd_gram_workspace_bytes(int n, int m, int d);
/* elvis.py:3476-3505 (calculate_fd_given_vectors).  a f64 [n, d], b f64 [m, d] -> gram f64 [n, m] = the centred
 * A Bm^T (k ascending), scalars f64 [3] = |mu_A - mu_B|^2, |A|_F^2, |Bm|_F^2.  2 <= n, m <= 1024. */
int elvis_fvmd_gram_f64(const double* a, const double* b, double* workspace, double* gram, double* scalars, int n, int m,
                        int d, elvis_stream_t stream);
/* elvis.py:3476-3505 (the matrix square root inside calculate_fd_given_vectors, here a nuclear norm).  vectors f64
 * [k, len], k, len <= 1024, OVERWRITTEN -> sv f64 [k], unsorted: the singular values of the matrix (those past
 * min(k, len) are 0 to rounding).  One-sided (Hestenes) Jacobi on the k vectors: round-robin pairing, 16 sweeps, a
 * rotation skipped where |x.y| <= 1e-15 |x| |y|.  k * len <= 16384: one workgroup, the matrix in LDS
 * (fvmd_jacobi_lds_kernel); above: one launch per pairing round, a workgroup per pair (fvmd_jacobi_round_kernel).  No
 * kernel waits on another workgroup.  Give it the orientation with k <= len. */
int elvis_fvmd_singular_values_f64(double* vectors, double* sv, int k, int len, elvis_stream_t stream);
/* elvis.py:3476-3505 (calculate_fd_given_vectors' last line).  sv f64 [k], scalars f64 [3] of elvis_fvmd_gram_f64 ->
 * out f64 [1] = ((scalars[0] + scalars[1] / (n - 1)) + scalars[2] / (m - 1)) - 2 (sum sv) / sqrt((n - 1)(m - 1)). */
int elvis_fvmd_finish_f64(const double* sv, const double* scalars, double* out, int k, int n, int m, elvis_stream_t stream);

/* ------------------------------------------------------------------ PNG writer (png.hip)
 * Lossless PNG files written by the device in place of the cv2.imwrite(...png) that ends every client-side entry point
 * of the reference (elvis.py:131-135, 4566-4579).  Decodable by any PNG reader; the bytes are this build's own, not
 * cv2's or PIL's.  tests/_png_ref.py states the stream and the kernels equal it bit for bit.
 *
 *   frames   u8 [n, h, w, c] dense, c in {1, 3}; order 0 = RGB (or gray), 1 = BGR (swapped in the loads); 8-bit colour
 *            type 2 or 0, no interlace.  A row of the filtered stream is its type byte and w * c filtered bytes.
 *   filters  0 None, 1 Sub, 2 Up, 3 Average floor((a + b) / 2), 4 Paeth (p = a + b - c, the nearest of a, b, c, ties in
 *            that order), bpp = c, on the raw neighbours; left of the row and above row 0 is 0.  filter -1 picks per row
 *            the type with the least sum of min(v, 256 - v), a tie going to the lower type; 0..4 forces a type.
 *   stream   zlib header 78 01.  A segment is segment_rows rows (the last may be shorter), one dynamic-Huffman block of
 *            literals only (HLIT 257, HDIST 0 with one distance code of length 0, HCLEN 19: a flat 4-bit code-length
 *            code for 0..15, 1106 header bits), BFINAL on the last; every other segment ends with an empty stored block
 *            and so on a byte boundary.  All segments of a frame share one literal code.  Each segment is one IDAT
 *            chunk; the first also holds the zlib header, the last the big-endian Adler-32 of the filtered stream.
 * Two calls per clip with one download between them (the caller synchronises, no entry point does):
 *   1. elvis_png_stats writes types u8 [n, h] and stats u32 [n, segments, 260]: the 256-bin histogram of the segment's
 *      filtered bytes (type bytes included), then its Adler partial A = sum d_i, B = sum (len - i) d_i (both mod
 *      65521), its length and a 0.
 *   2. the host builds every frame's code (lengths <= 15, complete), sums the bit lengths, lays the files out and calls
 *      elvis_png_pack with chunks i64 [n * segments, 2] = (byte offset of the chunk in out, length of its data) and
 *      frame_tab u32 [n, 304] = 257 entries (bit-reversed code << 4 | length), the Adler-32 trailer, the 35 dwords of
 *      the block header with BFINAL 0, padding.  It writes every chunk whole - length, "IDAT", data, CRC-32
 *      (png_pack_kernel, png_crc_kernel) - and nothing outside the chunks: the 33 bytes in front of a frame's first
 *      chunk (signature, IHDR) and the 12 behind its last (IEND) are the host's.  No global atomics; the same input
 *      gives the same bytes.
 * ELVIS_E_INVALID before any launch: c outside {1, 3}, h or w under 1, a bad order or filter, segment_rows under 1,
 * n * h * (w * c + 1) >= 2^31, a null pointer, out not 4-byte aligned.  n == 0 is a no-op. */
int elvis_png_stats(const uint8_t* frames, uint8_t* types, uint32_t* stats, int n, int h, int w, int c, int order, int filter,
                    int segment_rows, elvis_stream_t stream);
int elvis_png_pack(const uint8_t* frames, const uint8_t* types, const int64_t* chunks, const uint32_t* frame_tab, uint8_t* out,
                   int64_t out_bytes, int n, int h, int w, int c, int order, int segment_rows, elvis_stream_t stream);
/* The same two phases for the run-length stream (png_stats_rle_kernel, png_pack_rle_kernel; csrc/png_rle.h has the token
 * rule, tests/_png_rle_ref.py states the stream): masks and flat frames, whose filtered bytes are nearly all 0, cost a
 * match per 258 bytes instead of a bit per byte.  Frames, filters, filter choice, segments, IDAT chunking, the 78 01
 * header, the empty stored block between segments, Adler-32 and CRC-32 are exactly as above; only the contents of a
 * segment's dynamic-Huffman block differ:
 *   tokens   a row's type byte is one literal.  The row's w * c filtered bytes are cut into spans of 4096 bytes, each
 *            tokenised on its own.  A run is a maximal sequence of equal bytes inside a span; a run of length L and value
 *            v is the literal v, then with R = L - 1: R / 258 matches of length 258 and, with r = R % 258, one match of
 *            length r if r >= 3, else r literals v.  Every match has distance 1; none reaches across a span, a row, a
 *            type byte or a segment.
 *   symbols  286 literal/length symbols (0..255, EOB 256, 257..285 by RFC 1951's table; 258 is symbol 285 without extra
 *            bits), extra bits behind the code LSB first; one distance symbol (code 0) of length 1, so every match ends
 *            with one distance bit, 0.
 *   header   HLIT field 29, HDIST field 0, HCLEN 15; the flat 4-bit code-length code carries the 286 lengths and the
 *            distance length 1: 3 + 5 + 5 + 4 + 57 + 287 * 4 = 1222 bits, 39 dwords.
 *   1. elvis_png_stats_rle writes types u8 [n, h] and stats u32 [n, segments, 290]: the 286-bin histogram of the
 *      segment's tokens (type bytes included, EOB not), then the Adler partial, the length and a 0 as above.
 *   2. the host builds one literal/length code per frame (EOB count = segments); a segment is 1222 + sum hist[s] *
 *      (len[s] + extra[s]) + sum hist[257..285] bits plus EOB.  elvis_png_pack_rle takes chunks as above and frame_tab u32
 *      [n, 328] = 286 entries (bit-reversed code << 4 | length), the Adler-32 trailer, the 39 header dwords with BFINAL
 *      0, padding.  Same clipping, same masks, no global atomics, the same errors before any launch. */
int elvis_png_stats_rle(const uint8_t* frames, uint8_t* types, uint32_t* stats, int n, int h, int w, int c, int order, int filter,
                        int segment_rows, elvis_stream_t stream);
int elvis_png_pack_rle(const uint8_t* frames, const uint8_t* types, const int64_t* chunks, const uint32_t* frame_tab, uint8_t* out,
                       int64_t out_bytes, int n, int h, int w, int c, int order, int segment_rows, elvis_stream_t stream);

/* ------------------------------------------------------------------ PNG reader (png_read.hip, inflate.h)
 * PNG files decoded by the device in place of the cv2.imread that starts every client-side entry point of the reference
 * (elvis.py:123-128).  8-bit, non-interlaced, colour type 0, 2 or 6.  The host reads the signature, the chunk headers
 * and IHDR, uploads the files as they are and tells where the chunks lie; it passes over no stream byte and no pixel.
 * Three calls per clip and one download of the status words at the end (the caller synchronises, no entry point does):
 *   1. elvis_png_gather: chunks i64 [nchunks, 3] = (offset of the chunk's type field in files, length of its data,
 *      offset in streams where the data go, or -1 for a chunk that is not IDAT).  Copies the IDAT payloads into the
 *      frames' zlib streams and checks EVERY chunk's CRC-32: crc_status u32 [nchunks] = 0 or 11.  A chunk whose span
 *      lies outside files gets crc_status 11 and is not read; a payload whose destination lies outside streams is not
 *      copied and leaves no status of its own (the inflater then reports what it finds in the stream).
 *   2. elvis_png_inflate: stream i is streams[in_spans[i][0] .. + in_spans[i][1]), decoded into out[out_spans[i][0] ..
 *      + out_spans[i][1]) (offsets multiples of 4); any zlib stream (RFC 1950 / 1951).  One wave per stream.
 *      status u32 [n, 4] = code, bytes produced, bytes consumed, Adler-32 of the bytes produced.  Codes: 0 ok,
 *      1 input exhausted, 2 bad zlib header, 3 bad block type, 4 stored LEN/NLEN mismatch, 5 bad code-length set,
 *      6 invalid literal/length or distance symbol, 7 distance too far back, 8 output longer than its span,
 *      9 output shorter, 10 Adler-32 mismatch (11 chunk CRC and 12 filter type are the other two calls').  The first
 *      defect in stream order wins; nothing is written outside the span.
 *   3. elvis_png_unfilter: filtered = n streams of h rows of 1 + w * bpp bytes, `stride` bytes apart (bpp 1, 3 or 4),
 *      reconstructed per the PNG specification into frames u8 [n, h, w, channels]; channels 3 (gray replicated, alpha
 *      dropped; order 0 = RGB, 1 = BGR, swapped in the stores) or 1 (bpp 1 only).  `filtered` is a workspace: some
 *      of its rows are overwritten.  status u32 [n, 2] = (0 or 12, the first row whose filter type is above 4).
 * The same input gives the same bytes, alone or in a batch; no global atomics.
 * ELVIS_E_INVALID before any launch: a negative count or size, a buffer of 2^31 bytes or more, bpp outside {1, 3, 4},
 * channels outside {1, 3} or 1 with bpp above 1, a bad order, h or w under 1, n * h * (w * bpp + 1) >= 2^31, a stride
 * under h * (w * bpp + 1), a null pointer, out not 4-byte aligned.  n == 0 (nchunks == 0) is a no-op. */
int elvis_png_gather(const uint8_t* files, int64_t files_bytes, const int64_t* chunks, int nchunks, uint8_t* streams,
                     int64_t streams_bytes, uint32_t* crc_status, elvis_stream_t stream);
int elvis_png_inflate(const uint8_t* streams, int64_t streams_bytes, const int64_t* in_spans, uint8_t* out, int64_t out_bytes,
                      const int64_t* out_spans, uint32_t* status, int n, elvis_stream_t stream);
int elvis_png_unfilter(uint8_t* filtered, int64_t stride, uint8_t* frames, uint32_t* status, int n, int h, int w, int bpp,
                       int channels, int order, elvis_stream_t stream);

/* ------------------------------------------------------------------ JPEG reader (jpeg_read.hip, jpeg_decode.h)
 * Baseline JPEG files decoded by the device: every frame loader of the reference takes .jpg / .jpeg beside .png
 * (elvis.py:147, 193, 238, 549, 1495, 1724, 3033, 4785, 4811).  SOF0 or 8-bit SOF1, Huffman coded, one interleaved
 * scan, gray or YCbCr with luma sampling 1x1, 2x1 or 2x2.  The host walks the markers, uploads the files as they are and
 * tells where the entropy-coded segments lie (a file is cut at its RSTn markers); it decodes no compressed byte and
 * touches no pixel.  The pixels are those of libjpeg-turbo with default settings (slow integer IDCT, fancy upsampling),
 * bit for bit; tests/_jpeg_ref.py states them.  Three calls per clip and one download of the status words at the end
 * (the caller synchronises, no entry point does):
 *   fd       i32 [n, 32], the frame descriptors: 0 components (1 | 3), 1 hmax, 2 vmax, 3 MCUs per row, 4 MCU rows,
 *            5 blocks of the frame, 6..7 zero; per component c at 8 + 8 c: h, v, first block, first plane byte (64 * first
 *            block), plane pitch (8 * MCUs per row * h), DC table, AC table, quantisation table (0..3 each).  A single
 *            component counts as 1x1.  A component's blocks are a row-major grid of whole MCUs; frame f's blocks start
 *            at block f * stride_blocks of coef, its planes at byte f * stride_blocks * 64 of planes.  A descriptor
 *            that does not fit stride_blocks is not followed: its segments get status 5, its frame is left unwritten.
 *   1. elvis_jpeg_entropy: segs i32 [nseg, 5] = (byte offset in files, byte length, first MCU, MCU count, frame), the
 *      bytes between the markers with fill FFs trimmed; huff u8 [n, 8, 272] = 16 counts and up to 256 values of the DC
 *      tables 0..3 and the AC tables 0..3; qt u16 [n, 4, 64] in natural order.  Builds the code tables into `tables`
 *      (n * 8 * ELVIS_JPEG_TABLE_BYTES bytes of work space) and decodes every segment, a lane each (ITU-T T.81 F.2.2; FF 00 is
 *      one FF, the DC predictors start at 0): coef i16 [n, stride_blocks, 64], dequantised, natural order, stored as
 *      decoded into blocks that the CALLER HAS ZEROED.  status u32 [nseg, 2] = (code, MCUs done).  Codes: 0 ok, 1 no
 *      code of up to 16 bits matches, 2 a coefficient index past 63, 3 the bits run out before the segment's MCUs are
 *      done, 4 a dequantised coefficient outside [-32768, 32767], 5 bad descriptor or span.  The first defect ends a
 *      segment; bits left over at its end are ignored.  Nothing is read outside a segment's span or written outside
 *      its frame's blocks.
 *   2. elvis_jpeg_idct: libjpeg's jidctint.c (CONST_BITS 13, PASS1_BITS 2; columns descaled by 11 bits, rows by 18,
 *      the range limit's wrap at 10 bits) in 64-bit integers: coef -> planes u8 [n, stride_blocks * 64].
 *   3. elvis_jpeg_colour: planes -> frames u8 [n, h, w, channels].  Chroma of a 2x1 / 2x2 frame by libjpeg's fancy
 *      upsampling over the ceil(w / 2) x ceil(h / vmax) samples that count, neighbours replicated at the edges (plain
 *      replication where that width is at most 2); R = Y + ((91881 Cr + 32768) >> 16), B = Y + ((116130 Cb + 32768) >>
 *      16), G = Y + ((-22554 Cb - 46802 Cr + 32768) >> 16) with Cb, Cr less 128, clamped.  channels 3 (gray replicated;
 *      order 0 = RGB, 1 = BGR, swapped in the stores) or 1 (the luma plane).
 * The same input gives the same bytes, alone or in a batch; no global atomics.
 * ELVIS_E_INVALID before any launch: a negative count, n above 65535, files_bytes of 2^31 or more, stride_blocks outside
 * [1, 2^25), h or w outside [1, 65535], channels outside {1, 3}, a bad order, a null pointer, coef not 16-byte or planes
 * not 8-byte aligned.  n == 0 (nseg == 0) is a no-op. */
#define ELVIS_JPEG_TABLE_BYTES 1312
int elvis_jpeg_entropy(const uint8_t* files, int64_t files_bytes, const int32_t* segs, int nseg, const int32_t* fd, int n,
                       const uint8_t* huff, const uint16_t* qt, void* tables, int16_t* coef, int64_t stride_blocks,
                       uint32_t* status, elvis_stream_t stream);
int elvis_jpeg_idct(const int16_t* coef, int64_t stride_blocks, const int32_t* fd, int n, uint8_t* planes, elvis_stream_t stream);
int elvis_jpeg_colour(const uint8_t* planes, int64_t stride_blocks, const int32_t* fd, uint8_t* frames, int n, int h, int w,
                      int channels, int order, elvis_stream_t stream);

/* ------------------------------------------------------------------ JPEG writer (jpeg_write.hip, jpeg_encode.h)
 * Baseline JPEG files written by the device in place of cv2.imwrite(path, frame) with a .jpg / .jpeg suffix
 * (save_frame, elvis.py:131-135; save_frames(..., pattern=), elvis.py:160-175): libjpeg's forward path, so that against a
 * libjpeg-turbo at the same quality and sampling without optimised tables the quantisation tables and the entropy-coded
 * bytes are equal bit for bit; tests/_jpeg_write_ref.py states them.  frames u8 [n, h, w, channels], channels 1 (gray,
 * one component, sampling ignored) or 3 (order 0 = RGB, 1 = BGR; sampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 of Y, Cb,
 * Cr).  One interleaved scan, no restart interval (the restart forms are below), the Annex K Huffman tables.  The host plans the layout between the
 * calls from two small downloads - a frame's bit count, then its byte count - writes the headers and downloads the
 * finished scans; pixels and coefficients never visit it (the caller synchronises, no entry point does):
 *   blocks   elvis_jpeg_frame_blocks: the blocks of a frame in MCU scan order (gray: ceil(w/8) * ceil(h/8); colour:
 *            hmax * vmax luma blocks, Cb, Cr per MCU, dummy blocks included), 0 for a shape that is refused.
 *   1. elvis_jpeg_fdct: one launch from pixels to coef i16 [n, blocks, 64], quantised, zig-zag order, MCU scan order.
 *      jccolor.c: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11058 R - 21710 G + 32768 B + (128 << 16) + 32767)
 *      >> 16, Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.  jcprepct.c / jcsample.c: the last column is
 *      repeated to whole blocks, an odd 4:2:0 frame's last row once, then h2v1 (a + b + bias) >> 1 with bias 0, 1, 0, 1 ...
 *      or h2v2 (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2 ... along the output row, then the plane's last row is
 *      repeated to whole blocks.  jfdctint.c on samples less 128 (CONST_BITS 13, PASS1_BITS 2, rows then columns, descales
 *      round half up, int32).  Quantiser: sign(c) * ((|c| + (q8 >> 1)) / q8) with q8 = table << 3 and the tables of
 *      jpeg_set_quality(quality, force_baseline = TRUE) of Annex K.  A dummy block (jccoefct.c) has AC 0 and the DC of the
 *      block before it in its MCU.  No pixel outside the frame is read.
 *   2. elvis_jpeg_bits: ehuff u32 [2, 272] = per table class (0 luma, 1 chroma) 16 DC entries by category and 256 AC
 *      entries by symbol, (code << 5) | length, 0 where the table has no such symbol.  bits u32 [n, blocks + 1]: the bit
 *      offset of every block's code in its frame's stream (T.81 F.1.2: DC differences per component in scan order, ZRL,
 *      EOB unless coefficient 63 is set) and, in element `blocks`, the frame's bit count.  The prefix sum takes
 *      ELVIS_JPEG_SCAN_CHUNK values a step.
 *   3. elvis_jpeg_pack: word_off i64 [n + 1], the caller's layout: frame f's stream before stuffing is words
 *      [word_off[f], word_off[f + 1]) of `words` (total_words of them), at least ceil(ceil(bit count / 8) / 4), bytes
 *      most significant first in a word.  The call clears the words, every block writes its code at its own bit offset
 *      (shared words by vector atomic OR), the last block adds the 1-fill.  ffc u32 [n, chunks + 1]: the FF bytes before
 *      every chunk of ELVIS_JPEG_STUFF_CHUNK stream bytes and, in element `chunks`, of the frame (chunks >= the chunks of
 *      the longest frame).  sizes u32 [n]: stream bytes + FF bytes + 2.
 *   4. elvis_jpeg_stuff: out_off i64 [n + 1], the caller's layout of `out` from sizes: frame f's finished scan - FF
 *      followed by 00, the filled last byte, FF D9 - is written to out[out_off[f] .. out_off[f + 1]).
 * A frame whose span of words or of out does not lie inside the buffer is not written.  The same input gives the same
 * bytes, alone or in a batch, whatever the buffers held.
 * ELVIS_E_INVALID before any launch: channels outside {1, 3}, a bad order or sampling, quality outside [1, 100], n
 * outside [0, 65535], h or w outside [1, 65535], more than 2^20 blocks a frame, chunks under 1, a negative size, a null
 * pointer, a misaligned buffer (coef 16, the offset tables 8, the others 4 bytes).  n == 0 is a no-op.
 *
 * Restart intervals (T.81 B.2.4.4, E.1.4; libjpeg's restart_interval, jchuff.c emit_restart): elvis_jpeg_bits_rst, _pack_rst
 * and _stuff_rst are calls 2 - 4 with restart_mcus in [0, 65535], the MCUs of an interval; elvis_jpeg_fdct is the same for
 * both forms.  A frame of M MCUs is segs = ceil(M / restart_mcus) segments (elvis_jpeg_segments; 1 for restart_mcus = 0 or
 * >= M, 0 for arguments that are refused), segment s holding MCUs [s * restart_mcus, min((s + 1) * restart_mcus, M)),
 * segb = restart_mcus * blocks per MCU blocks in all but the last (segb = blocks when segs = 1).  A segment starts on a
 * byte boundary with the DC predictor of every component at 0 (a dummy block still repeats the block before it in its
 * own MCU), ends in the 1-fill to the byte boundary, which is stuffed like any other byte, and is followed by FF D0+(s &
 * 7), which is not stuffed, or, behind a frame's last segment, by FF D9.  Everything that is per frame above is per
 * segment q = f * segs + s here, nseg = n * segs of them:
 *   bits u32 [nseg, segb + 1]: the bit offset of the segment's block i in the segment's stream, the segment's bit
 *      count in element segb; the elements past the blocks of a frame's last segment hold that count as well.
 *   word_off i64 [nseg + 1]: every segment has its own span of words, so that no two segments share a word; ffc u32
 *      [nseg, chunks + 1] (chunks >= the chunks of the longest segment); sizes u32 [nseg]: stream bytes + FF bytes + 2.
 *   out_off i64 [nseg + 1]: a frame's finished scan is its segments back to back, out[out_off[f * segs] .. out_off[(f +
 *      1) * segs]), each with its marker, the last with EOI.
 * restart_mcus = 0 is calls 2 - 4 themselves: the same code, the same layouts, the same bytes.  The file's DRI segment
 * is the caller's.  ELVIS_E_INVALID before any launch for what the calls above refuse, restart_mcus outside [0, 65535]
 * and n * segs above ELVIS_JPEG_MAX_SEGMENTS (encode the clip in parts).
 *
 * Per-block rate allocation (elvis_jpeg_fdct_roi): call 1 with a map of coarsening levels, in the place of the ROI files
 * the reference hands its encoders (create_kvazaar_roi_file, utils.py:1026-1053; encode_with_roi's x265 qpfile,
 * elvis.py:2013-2118).  levels u8 [n, by, bx] on a grid of block_size x block_size luma pixels, a level 0 .. 48 (above:
 * 48) in HEVC QP units: the step doubles every 6, scale16(L) = round(16 * 2^(L / 6)), a table of 49 constants.  A dead
 * zone, not a coarser step: for an AC coefficient c (the FDCT's output, scaled by 8) and its table entry Q, a = |c|, d =
 * scale16(L) * (Q << 3), the result is 0 when 16 * a + (d >> 1) < d - the quantiser of the step coarsened by L would round
 * it to 0 - and the quantiser of call 1 otherwise; DC is never touched, and level 0 is call 1 for every input.  The
 * file keeps the tables of its header and stays baseline JPEG.  The level of a DCT block is the minimum over the cells
 * its footprint touches, then min(., 48): the footprint is 8 x 8 luma pixels for a luma or gray block and 8 hmax x 8
 * vmax for a chroma block, both ends clamped to the frame; a cell index is min(p / block_size, bx - 1) and min(p /
 * block_size, by - 1).  by is max(1, h / block_size) or ceil(h / block_size), bx likewise: the reference's floored grids
 * and full grids.  A dummy block keeps its DC only, as in call 1.  levels = NULL with by = bx = block_size = 0 is call 1
 * itself.  Calls 2 - 4 and their restart forms follow unchanged.  ELVIS_E_INVALID before any launch for what call 1
 * refuses, a block_size that is not a positive multiple of 8, a by or bx that is neither of its two values, and a null
 * map with a non-zero by, bx or block_size.
 *
 * Per-frame optimised Huffman tables (libjpeg's optimize_coding: jchuff.c encode_mcu_gather, jpeg_gen_optimal_table; T.81
 * K.2).  Between call 1 and call 2:
 *   elvis_jpeg_tally: hist u32 [n, 2, 272] in the layout of ehuff - per frame and table class the DC difference
 *      categories in entries 0 .. 11 and the AC symbols (run << 4) | category, ZRL F0 and EOB 00 in entries 16 + symbol -
 *      counted over exactly the blocks the scan codes: dummy blocks included, the DC predictors reset at every restart
 *      interval (restart_mcus as in the restart forms, 0: none), coefficients as call 1 left them.  The call zeroes hist
 *      itself; it is the symbol walk of call 2 over another sink, one LDS histogram a workgroup.
 *   elvis_jpeg_optimal_tables: HOST ONLY, no device is touched: hist, downloaded, to the tables of every frame.  Per
 *      table class t (0, and 1 for channels = 3; a gray clip builds tables 0 only and the rest is zeroed) and kind k (0 DC
 *      from entries 0 .. 15, 1 AC from entries 16 .. 271): counts u8 [n, 2, 2, 16], the codes of each length 1 .. 16;
 *      symbols u8 [n, 2, 2, 256], the symbols in code order; nsym i32 [n, 2, 2], how many; ehuff u32 [n, 2, 272], the
 *      words calls 2 and 3 look up.  The rule is jpeg_gen_optimal_table's: a reserved symbol 256 of frequency 1, so that
 *      no real code is all ones; the two entries of smallest non-zero frequency are merged, ties to the largest index,
 *      until one is left; lengths are counted up to 32 and, from 32 down to 17, shortened by bits[i] -= 2, bits[i - 1] +=
 *      1, bits[j + 1] += 2, bits[j] -= 1 for the first j <= i - 2 with bits[j] != 0; the reserved symbol leaves the
 *      longest length; symbols are listed by the length the merge gave them, by value within a length.  ELVIS_E_INVALID
 *      for a count above 2^26 (blocks a frame times 64), a table without a symbol, a code past 32 bits before limiting.
 *   elvis_jpeg_bits_ftab, elvis_jpeg_pack_ftab: elvis_jpeg_bits_rst and elvis_jpeg_pack_rst with ehuff u32 [n, 2, 272], a
 *      table set per frame; call 4 is unchanged.  The DHT segments of every file are the caller's. */
#define ELVIS_JPEG_SCAN_CHUNK 256
#define ELVIS_JPEG_STUFF_CHUNK 1024
#define ELVIS_JPEG_MAX_SEGMENTS 16777216
int elvis_jpeg_frame_blocks(int h, int w, int channels, int sampling);
int elvis_jpeg_fdct(const uint8_t* frames, int16_t* coef, int n, int h, int w, int channels, int order, int quality, int sampling,
                    elvis_stream_t stream);
int elvis_jpeg_fdct_roi(const uint8_t* frames, int16_t* coef, int n, int h, int w, int channels, int order, int quality, int sampling,
                        const uint8_t* levels, int by, int bx, int block_size, elvis_stream_t stream);
int elvis_jpeg_bits(const int16_t* coef, const uint32_t* ehuff, uint32_t* bits, int n, int h, int w, int channels, int sampling,
                    elvis_stream_t stream);
int elvis_jpeg_pack(const int16_t* coef, const uint32_t* ehuff, const uint32_t* bits, const int64_t* word_off, uint32_t* words,
                    int64_t total_words, uint32_t* ffc, int chunks, uint32_t* sizes, int n, int h, int w, int channels, int sampling,
                    elvis_stream_t stream);
int elvis_jpeg_stuff(const uint32_t* bits, const int64_t* word_off, const uint32_t* words, int64_t total_words, const uint32_t* ffc,
                     int chunks, const int64_t* out_off, uint8_t* out, int64_t out_bytes, int n, int h, int w, int channels, int sampling,
                     elvis_stream_t stream);
int elvis_jpeg_segments(int h, int w, int channels, int sampling, int restart_mcus);
int elvis_jpeg_bits_rst(const int16_t* coef, const uint32_t* ehuff, uint32_t* bits, int n, int h, int w, int channels, int sampling,
                        int restart_mcus, elvis_stream_t stream);
int elvis_jpeg_pack_rst(const int16_t* coef, const uint32_t* ehuff, const uint32_t* bits, const int64_t* word_off, uint32_t* words,
                        int64_t total_words, uint32_t* ffc, int chunks, uint32_t* sizes, int n, int h, int w, int channels, int sampling,
                        int restart_mcus, elvis_stream_t stream);
int elvis_jpeg_stuff_rst(const uint32_t* bits, const int64_t* word_off, const uint32_t* words, int64_t total_words, const uint32_t* ffc,
                         int chunks, const int64_t* out_off, uint8_t* out, int64_t out_bytes, int n, int h, int w, int channels,
                         int sampling, int restart_mcus, elvis_stream_t stream);
int elvis_jpeg_tally(const int16_t* coef, uint32_t* hist, int n, int h, int w, int channels, int sampling, int restart_mcus,
                     elvis_stream_t stream);
int elvis_jpeg_optimal_tables(const uint32_t* hist, int n, int channels, uint8_t* counts, uint8_t* symbols, int32_t* nsym, uint32_t* ehuff);
int elvis_jpeg_bits_ftab(const int16_t* coef, const uint32_t* ehuff, uint32_t* bits, int n, int h, int w, int channels, int sampling,
                         int restart_mcus, elvis_stream_t stream);
int elvis_jpeg_pack_ftab(const int16_t* coef, const uint32_t* ehuff, const uint32_t* bits, const int64_t* word_off, uint32_t* words,
                         int64_t total_words, uint32_t* ffc, int chunks, uint32_t* sizes, int n, int h, int w, int channels, int sampling,
                         int restart_mcus, elvis_stream_t stream);

/* ------------------------------------------------------------------ Real-ESRGAN / RRDBNet (rrdb.hip)
 * The network behind RealESRGANer.enhance (elvis.py:2515): RRDBNet(3, 3, 64, num_block, 32, scale) on f16 NHWC tensors.
 * Channel counts are the padded ones the kernel runs: cin in {32, 64, 96, 128, 160, 192}, cout in {32, 64}. */

/* Bytes of the packed f16 weights of one conv (9 * cin * cout * 2); 0 for an unsupported cin or cout.  elvis.py:2515 */
size_t elvis_rrdb_packed_weight_bytes(int cin, int cout);

/* Host function, no GPU: fp32 OIHW [cout_real][cin_real][3][3] -> packed f16 [cin/32][tap = ky*3+kx][cout][32]
 * (round to nearest even), element [kc][tap][co][k] = w[co][32 kc + k][ky][kx]; input channels past cin_real and output
 * channels past cout_real are zero (conv_first: 3 or 12 real inputs in 32; conv_last: 3 real outputs in 32).
 * elvis.py:2515 */
int elvis_rrdb_pack_weights(const float* w_oihw_host, int cin_real, int cout_real, int cin, int cout, void* packed_host);

/* 3x3 / stride 1 / pad 1 conv of a dense block (elvis.py:2515), f16 in, fp32 accumulate on v_mfma_f32_16x16x32_f16.
 * x: f16 [n,h,w,x_pitch], channels [0, cin) are read.  upsample != 0: the conv sees the nearest-2x image (pixel (y, x)
 * reads (y >> 1, x >> 1)), ho = 2h, wo = 2w; otherwise ho = h, wo = w.  w_packed: elvis_rrdb_pack_weights' layout on
 * the device; bias: fp32 [cout].  out: f16 [n,ho,wo,out_pitch], channels [out_coff, out_coff + cout) are written and no
 * other byte.  Epilogue in fp32: v = z + bias; lrelu != 0: v = v > 0 ? v : 0.2f * v; y = s0 * v + s1 * r1 + r2 with r1, r2
 * f16 [n,ho,wo,r*_pitch] read at channels [0, cout), each optional (NULL); y is stored as f16, round to nearest even.
 * out_u8 != 0 (conv_last; cout = 32, out_coff = 0): out is u8 [n,ho,wo,3], byte c = rint(clamp(y_c, 0, 1) * 255) (half
 * to even) from the fp32 y of the three real channels, written at 2 - c with swap_rb.
 * Aliasing: out may be x itself (same pointer and pitch, no upsample) when out_coff >= cin - the in-place concat of a
 * dense block; r1 and r2 may alias x; a residual may be out itself (same pointer and pitch) when out_coff == 0 (each
 * element is read, then written, by one lane) or out_coff >= cout.  Any other overlap of out with x or a residual is
 * ELVIS_E_INVALID, as are an unsupported cin / cout, a pitch or offset that is no multiple of 8 (residuals: 4) or too
 * small, out_u8 with cout != 32, a null or misaligned pointer (x, weights, bias 16 bytes; out, residuals 8).  Offsets
 * are 64-bit.  n, h or w == 0 does nothing and succeeds.  elvis_last_launch: "rrdb_conv3x3_kernel<32>" or "<64>". */
int elvis_rrdb_conv3x3(const void* x, int x_pitch, const void* w_packed, const float* bias, void* out, int out_pitch,
                       int out_coff, const void* r1, int r1_pitch, const void* r2, int r2_pitch, int n, int h, int w,
                       int cin, int cout, int upsample, int lrelu, float s0, float s1, int out_u8, int swap_rb,
                       elvis_stream_t stream);

/* The network's input stage (what RealESRGANer.pre_process and RRDBNet.forward do before conv_first, elvis.py:2515):
 * src u8 [n,h,w,3] -> dst f16 [n,ceil(h/s),ceil(w/s),32], values f16(v / 255.0f), channel order reversed with swap_rb.
 * s = 1: channels 0..2.  s = 2: pixel-unshuffle, input (c, 2y+sy, 2x+sx) at channel 4c + 2sy + sx
 * (torch.nn.functional.pixel_unshuffle's order); an odd h or w is first extended by one reflected row or column
 * (index h reads h - 2, F.pad(..., 'reflect')) and must then be at least 3.  Channels past 3*s*s are zero. */
int elvis_rrdb_input_u8(const uint8_t* src, void* dst, int n, int h, int w, int s, int swap_rb, elvis_stream_t stream);

/* ------------------------------------------------------------------ Real-ESRGAN / SRVGGNetCompact (srvgg.hip)
 * The network of `realesr-animevideov3` and `realesr-general-x4v3` (elvis.py:2431-2441), run by RealESRGANer.enhance
 * (elvis.py:2515): SRVGGNetCompact(3, 3, 64, num_conv, upscale=4, 'prelu') on f16 NHWC tensors.  The first layer reads
 * the 32-channel buffer elvis_rrdb_input_u8 writes with s = 1. */

/* Bytes of the packed f16 weights of one conv (9 * cin * cout * 2); 0 unless cin is 32 or 64 and cout 48 or 64.
 * elvis.py:2431-2441 / 2515 */
size_t elvis_srvgg_packed_weight_bytes(int cin, int cout);

/* Host function, no GPU: fp32 OIHW [cout_real][cin_real][3][3] -> packed f16 [cin/32][tap = ky*3+kx][cout][32]
 * (round to nearest even), element [kc][tap][co][k] = w[co][32 kc + k][ky][kx]; input channels past cin_real and output
 * channels past cout_real are zero (the first layer: 3 real inputs in 32).  elvis_rrdb_pack_weights' layout with the
 * tail's cout = 48 admitted.  elvis.py:2431-2441 / 2515 */
int elvis_srvgg_pack_weights(const float* w_oihw_host, int cin_real, int cout_real, int cin, int cout, void* packed_host);

/* One body layer (elvis.py:2431-2441 / 2515): 3x3 / stride 1 / pad 1 conv to 64 channels and a per-channel PReLU, f16
 * in, fp32 accumulate on v_mfma_f32_16x16x32_f16.  x: f16 [n,h,w,x_pitch], channels [0, cin) are read, cin 32 or 64.
 * w_packed: elvis_srvgg_pack_weights' layout (cout = 64) on the device; bias, slope: fp32 [64].  out: f16
 * [n,h,w,out_pitch], channels [0, 64) are written and no other byte.  Epilogue in fp32: z = sum + bias;
 * y = z > 0 ? z : slope[c] * z, stored as f16, round to nearest even.  out may not overlap x.  ELVIS_E_INVALID, before
 * any launch: an unsupported cin, a pitch that is no multiple of 8 or too small, a null or misaligned pointer (x,
 * weights, bias, slope 16 bytes; out 8), an out that overlaps x.  Offsets are 64-bit.  n, h or w == 0 does nothing and
 * succeeds.  elvis_last_launch: "srvgg_conv3x3_kernel<64,prelu>". */
int elvis_srvgg_conv3x3(const void* x, int x_pitch, const void* w_packed, const float* bias, const float* slope, void* out,
                        int out_pitch, int n, int h, int w, int cin, elvis_stream_t stream);

/* The last conv with everything after it (elvis.py:2431-2441 / 2515): 3x3 conv 64 -> 48, pixel shuffle by 4 (channel
 * 16c + 4dy + dx is colour c at (4y + dy, 4x + dx), torch's order), plus the nearest-4x base, then `enhance`'s
 * quantisation.  x: f16 [n,h,w,x_pitch], channels [0, 64) read; w_packed: elvis_srvgg_pack_weights' layout with
 * cin = 64, cout = 48; bias: fp32 [48]; base: f16 [n,h,w,base_pitch], channels 0..2 of pixel (y, x) are added to its
 * 16 output pixels.  y = (sum + bias) + base in fp32.  out_u8 != 0: out is u8 [n,4h,4w,3], byte
 * c = rint(clamp(y_c, 0, 1) * 255) (half to even); otherwise out is f16 [n,4h,4w,3], y before the clamp.  swap_rb != 0
 * reverses the channel order on the way out (either mode).  The 48-channel tensor is never stored.  ELVIS_E_INVALID,
 * before any launch: x_pitch no multiple of 8 or under 64, base_pitch under 3, a null or misaligned pointer (x, weights,
 * bias 16 bytes; base 2; out 4 for u8, 8 for f16), an out that overlaps x or base.  n, h or w == 0 does nothing and
 * succeeds.  elvis_last_launch: "srvgg_conv3x3_kernel<48,shuffle_u8>" or "<48,shuffle_f16>". */
int elvis_srvgg_tail(const void* x, int x_pitch, const void* w_packed, const float* bias, const void* base, int base_pitch,
                     void* out, int n, int h, int w, int out_u8, int swap_rb, elvis_stream_t stream);

/* ------------------------------------------------------------------ RealESRGANer.enhance around the network
 * csrc/sr_enhance.hip.  Tables come in a host copy (`*_h`, validated before the launch) and a device copy (read by
 * the kernel, which clamps whatever it reads from it into range). */

/* cv2.resize(src, (wd, hd), interpolation=cv2.INTER_LANCZOS4) of 8-bit frames: the resize to `outscale` inside
 * RealESRGANer.enhance (elvis.py:2515, presley.py:1308) and the resize back to (w, h) after it (utils.py:1466,
 * presley.py:1309).  src u8 [n,hs,ws,c], dst u8 [n,hd,wd,c], c in 1..4, any ratio.  Per destination column d:
 * xfirst[d] (the first of eight source columns, before the BORDER_REPLICATE clamp to [0, ws-1]) and xtaps[d][8] int16
 * (rint(coef * 2048)); rows likewise.  dst = saturate((sum_ky sum_kx p * tx * ty + 2^21) >> 22), exact in int32 when
 * the caller's tap sums keep 255 * (Px*Py + Nx*Ny) + 2^21 below 2^31.  One launch; a workgroup owns a th x tw
 * destination tile and keeps its source footprint and the int32 intermediate in at most 64 KiB of LDS.
 * ELVIS_E_INVALID: a null pointer, a non-positive size, c outside 1..4, a first index outside [-4, size-4] or a
 * decreasing table, tap tables not 16-byte aligned, or a tile whose footprint exceeds the LDS limit.
 * elvis_last_launch: "resize_lanczos4_u8_kernel<c>". */
int elvis_resize_lanczos4_u8(const uint8_t* src, uint8_t* dst, int n, int hs, int ws, int hd, int wd, int c,
                             const int32_t* xfirst_h, const int32_t* yfirst_h, const int32_t* xfirst,
                             const int16_t* xtaps, const int32_t* yfirst, const int16_t* ytaps, int th, int tw,
                             elvis_stream_t stream);
/* Host only: the bytes of LDS a workgroup of elvis_resize_lanczos4_u8 needs for th x tw destination tiles of these
 * tables (the same validation; ELVIS_E_INVALID = -1 on a bad argument). */
int elvis_resize_lanczos4_lds_bytes(const int32_t* xfirst_h, const int32_t* yfirst_h, int hs, int ws, int hd, int wd,
                                    int c, int th, int tw);

/* The padded input boxes of RealESRGANer.tile_process (the `input_tile` slice), all of one shape:
 * dst[t, y, x] = src[frame_t, rowmap[y0_t + y], colmap[x0_t + x]] with desc int32 [T][3] = (frame, y0, x0).  rowmap
 * int32 [Hp] and colmap int32 [Wp] map the padded image to the frame: the F.pad(..., (0, pre_pad, 0, pre_pad),
 * 'reflect') of pre_process, then for an x2 network its reflect pad to an even size.  src u8 [n,H,W,3], dst u8
 * [T,th,tw,3].  ELVIS_E_INVALID: a null pointer, a non-positive size, a map entry outside the frame, a tile outside
 * the padded image or naming a frame outside [0, n).  elvis_last_launch: "sr_gather_tiles_u8_kernel". */
int elvis_sr_gather_tiles_u8(const uint8_t* src, uint8_t* dst, int n, int H, int W, int T, int th, int tw,
                             const int32_t* desc_h, const int32_t* desc, const int32_t* rowmap_h, const int32_t* rowmap,
                             int Hp, const int32_t* colmap_h, const int32_t* colmap, int Wp, elvis_stream_t stream);

/* The paste of tile_process (`self.output[...] = output_tile[...]`) and the crop of post_process: tiles u8
 * [T,tth,ttw,3] (the network's output per tile), desc int32 [T][7] = (frame, crop y, crop x inside the tile,
 * destination y, x, crop height, width); dst u8 [n,OH,OW,3] receives each crop, clipped at OH x OW (the pre_pad and
 * mod-pad removal).  ELVIS_E_INVALID: a null pointer, a non-positive size, a crop outside its tile, a negative
 * destination, a frame outside [0, n).  elvis_last_launch: "sr_paste_tiles_u8_kernel". */
int elvis_sr_paste_tiles_u8(const uint8_t* tiles, uint8_t* dst, int T, int tth, int ttw, int n, int OH, int OW,
                            const int32_t* desc_h, const int32_t* desc, elvis_stream_t stream);

/* ------------------------------------------------------------------ clip intake (csrc/resize.hip) */

/* cv2.resize(frame, (wd, hd), interpolation=cv2.INTER_AREA) of every frame of a clip: the resize to the working size
 * that Presley applies to each decoded frame before anything else reads it (presley.py:186).  src u8 [n,hs,ws,c], dst u8
 * [n,hd,wd,c], c in {1, 3, 4}, hd <= hs and wd <= ws, any ratio >= 1 on each axis, one launch.  Per axis the table of
 * cv::computeResizeAreaTab in three arrays: start int32 [dst + 1] (the entries of destination d are start[d] ..
 * start[d + 1]), first int32 [dst] (the source index of d's first entry; its entries are consecutive source indices)
 * and w float32 [start[dst]].  start and first come in a host copy (`*_h`, validated before the launch) and a device
 * copy (read by the kernel); w on the device only.
 *   hs == fy * hd and ws == fx * wd: the integer box sum s; dst = s at 1x1, (s + 2) >> 2 at 2x2, otherwise
 *     rint(float(s) * float(1.0 / (fx * fy))), half to even; w is not read.
 *   otherwise cv::ResizeArea_<uchar, float>, on both axes: buf = sum_x S[sy][sx] * xw, sum = sum_y yw * buf, float32
 *     from 0 in table order, every product and every sum rounded on its own; dst = clip(rint(sum), 0, 255).
 * A workgroup owns th x tw destination pixels (th * tw * c <= 1024) and streams the source rows it needs through LDS,
 * rows_per_chunk rows of row_stride bytes at a time (row_stride a multiple of 4 and at least the widest tile's source
 * segment + 3; rows_per_chunk * row_stride <= 64 KiB); row_stride == 0 reads the source in place, for segments no LDS
 * holds.  The tiling does not change a byte.  ELVIS_E_INVALID, before any launch: a null pointer, a non-positive
 * size, another c, a destination larger than the source on either axis (cv2 switches to its area-mode bilinear
 * there; not built), a table that leaves the source, steps back or, at whole ratios, is not the box, a tile or a chunk
 * beyond the limits above. */
int elvis_resize_area_u8(const uint8_t* src, uint8_t* dst, int n, int hs, int ws, int hd, int wd, int c,
                         const int32_t* xstart_h, const int32_t* xfirst_h, const int32_t* ystart_h, const int32_t* yfirst_h,
                         const int32_t* xstart, const int32_t* xfirst, const float* xw, const int32_t* ystart,
                         const int32_t* yfirst, const float* yw, int th, int tw, int rows_per_chunk, int row_stride,
                         elvis_stream_t stream);

/* cv2.resize(mask, (wd, hd), interpolation=cv2.INTER_NEAREST) (presley.py:427, 846, 867, 884; elvis.py:206, 564, 4578):
 * dst[f, dy, dx] = src[f, floor(dy * hs / hd), floor(dx * ws / wd)] in integers, up or down.  src u8 [n,hs,ws,c], dst u8
 * [n,hd,wd,c], c in {1, 3, 4}. */
int elvis_resize_nearest_u8(const uint8_t* src, uint8_t* dst, int n, int hs, int ws, int hd, int wd, int c,
                            elvis_stream_t stream);

/* ------------------------------------------------------------------ DCT slot (LaplacianVCAR-style) */

/* DCNv2 modulated deformable 3x3 convolution (stride 1, pad 1, dilation 1), NHWC.
 * offset_mask[n,h,w,om_pitch]: channels [0, 18*G) offsets ((g*9+k)*2 + {dy,dx}), [18*G, 27*G) masks
 * (g*9+k); `mask_sigmoid` applies the sigmoid to the mask channels on load.  weight: [cout][cin][9]
 * in the tensor dtype, bias f32[cout] or NULL, act 0 / 3 (ReLU).  Out-of-image bilinear corners
 * contribute zero.  The reference only names this op (README.md:14-16, an absent CUDA build). */
int elvis_dcnv2(const void* x, const void* offset_mask, const void* weight, const float* bias, void* out,
                int dtype, int n, int h, int w, int cin, int x_pitch, int deformable_groups, int om_pitch,
                int mask_sigmoid, int cout, int out_pitch, int act, elvis_stream_t stream);

/* frames u8 [nf,h,w,3] -> planes [(f*3+c), h, w, pitch] for f in [f0, f0+nsel): channel t holds
 * colour c of frame clamp(f + t - radius) / 255 (the temporal window of the DCN restorer). */
int elvis_temporal_stack(const uint8_t* frames, void* out, int dtype, int nf, int f0, int nsel, int h, int w,
                         int radius, int pitch, elvis_stream_t stream);

/* out_u8[f,h,w,c] = round(clip(frames[f0+f][c]/255 + residual[(f*3+c),h,w,0], 0, 1) * 255). */
int elvis_plane_merge(const uint8_t* frames, const void* residual, uint8_t* out, int dtype, int f0, int nsel,
                      int h, int w, int pitch, elvis_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ELVIS_AMD_H */
