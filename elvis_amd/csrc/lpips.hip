// LPIPS (AlexNet) of the evaluation report: the perceptual distance the reference takes from `lpips.LPIPS(net='alex')`
// for every sampled frame (elvis.py:437-447, 3163-3195, 3887-3893; presley.py:329-357).  The package and its weights are
// available neither to the reference tree nor to this build, so this is a BUILD-DEFINED restatement behind that call
// surface - five convolutions, two max-pools, a channel-normalised squared difference and five 1x1 weightings - stated
// as a contract in include/elvis_amd.h and DESIGN.md 7 and in torch float64 in tests/_lpips_ref.py.  It does not claim
// parity with the lpips package.
//
// This file holds the stem (11x11 stride 4 on the u8 clip), the 5x5 conv, the max-pool and the distance; the three 3x3
// layers run through elvis_conv2d.  fp32 with fp32 accumulation, float64 only for the sum over pixels.  No atomics, a
// fixed summation order everywhere: a frame's score does not depend on n or on how a clip is cut into calls.
#include "common.h"
#include "lpips_index.h"

#define LPIPS_STEM_THREADS 256
#define LPIPS_STEM_LDS_PITCH (LPIPS_STEM_COLS * 3)      // 213 floats: odd, so rows fall on different banks
#define LPIPS_C5_THREADS 256
#define LPIPS_C5_CIN 64
#define LPIPS_C5_COUT 192
#define LPIPS_C5_TY 4                                   // output tile: 4 rows x 16 pixels x 192 channels
#define LPIPS_C5_TX 16
#define LPIPS_C5_ROWS (LPIPS_C5_TY + 4)
#define LPIPS_C5_COLS (LPIPS_C5_TX + 4)
#define LPIPS_C5_LDS_PITCH 68                           // floats per staged pixel: 16 lanes x 4 channel groups hit 64 distinct banks
#define LPIPS_POOL_THREADS 256

static inline bool lpips_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------------ stem
// One workgroup computes a 4 x 16 tile of output pixels, all 64 channels.  It stages the 23 x 71 x 3 input footprint in
// LDS as floats, in RGB order, with the affine applied on load:
//     t = byte / 127.5 - 1,   x = (t - shift_c) / scale_c            (IEEE fp32 divisions)
// where the byte of a pixel whose mask is 0 is 0 (so a masked pixel is affine(0), not 0) and an element outside the rect
// is the conv's padding: 0 AFTER the affine.  Lane p of wave g then forms channels 16 g .. 16 g + 15 of pixel p:
//     acc = 0;  for ky, kx, c in that order: acc = fmaf(x[ky][kx][c], w[(ky 11 + kx) 3 + c][co], acc);  relu(acc + bias)
// 363 products per output, one chain.  The weights of a wave are the same for all its lanes and come through the
// scalar cache.
__constant__ float lpips_shift[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float lpips_scale[3] = {0.458f, 0.448f, 0.450f};

template <int ORDER>
__global__ __launch_bounds__(LPIPS_STEM_THREADS) void lpips_stem_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ mask,
                                                                        const float* __restrict__ weight, const float* __restrict__ bias,
                                                                        float* __restrict__ out, int h, int w, int y0, int y1, int x0, int x1,
                                                                        int ho, int wo, int tiles_y, int tiles_x, int out_pitch) {
    __shared__ float tile[LPIPS_STEM_ROWS * LPIPS_STEM_LDS_PITCH];
    const int t = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, f = blockIdx.x / (tiles_x * tiles_y);
    const int oy0 = ty * LPIPS_STEM_TY, ox0 = tx * LPIPS_STEM_TX;

    for (int i = t; i < LPIPS_STEM_ROWS * LPIPS_STEM_COLS; i += LPIPS_STEM_THREADS) {
        const int r = i / LPIPS_STEM_COLS, cc = i % LPIPS_STEM_COLS;
        const long long pix = lpips_stem_src_pixel(f, h, w, y0, y1, x0, x1, oy0, ox0, r, cc);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = 0.0f;
            if (pix >= 0) {
                const float b = (float)lpips_stem_byte(frames, mask, pix, c, ORDER);
                v = ((b / 127.5f - 1.0f) - lpips_shift[c]) / lpips_scale[c];
            }
            tile[r * LPIPS_STEM_LDS_PITCH + cc * 3 + c] = v;
        }
    }
    __syncthreads();

    const int p = t & 63, g = __builtin_amdgcn_readfirstlane(t >> 6);
    const int py = p / LPIPS_STEM_TX, px = p % LPIPS_STEM_TX;
    const float* wg = weight + g * 16;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
    for (int ky = 0; ky < LPIPS_STEM_KS; ++ky) {
        const float* row = tile + (py * LPIPS_STEM_STRIDE + ky) * LPIPS_STEM_LDS_PITCH + px * LPIPS_STEM_STRIDE * 3;
        const float* wk = wg + ky * (LPIPS_STEM_KS * 3) * LPIPS_STEM_COUT;
#pragma unroll 3
        for (int q = 0; q < LPIPS_STEM_KS * 3; ++q) {                     // q = kx 3 + c
            const float x = row[q];
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = fmaf(x, wk[q * LPIPS_STEM_COUT + j], acc[j]);
        }
    }
    const int oy = oy0 + py, ox = ox0 + px;
    if (oy < ho && ox < wo) {
        float* o = out + lpips_stem_out_offset(f, ho, wo, oy, ox, out_pitch) + g * 16;
#pragma unroll
        for (int j = 0; j < 16; j += 4) {
            float4 v;
            v.x = fmaxf(acc[j] + bias[g * 16 + j], 0.0f);
            v.y = fmaxf(acc[j + 1] + bias[g * 16 + j + 1], 0.0f);
            v.z = fmaxf(acc[j + 2] + bias[g * 16 + j + 2], 0.0f);
            v.w = fmaxf(acc[j + 3] + bias[g * 16 + j + 3], 0.0f);
            *reinterpret_cast<float4*>(o + j) = v;
        }
    }
}

template <int ORDER>
static int lpips_stem_launch(const uint8_t* frames, const uint8_t* mask, const float* weight, const float* bias, float* out, int n, int h,
                             int w, int y0, int y1, int x0, int x1, int out_pitch, hipStream_t stream) {
    const int ho = lpips_stem_size(y1 - y0), wo = lpips_stem_size(x1 - x0);
    const int tiles_y = cdiv(ho, LPIPS_STEM_TY), tiles_x = cdiv(wo, LPIPS_STEM_TX);
    ELVIS_REQUIRE((long long)n * tiles_y * tiles_x <= 0x7fffffffLL, "elvis_lpips_stem_u8: n=%d rect %dx%d is more than one launch holds", n,
                  y1 - y0, x1 - x0);
    hipLaunchKernelGGL((lpips_stem_kernel<ORDER>), dim3(n * tiles_y * tiles_x), dim3(LPIPS_STEM_THREADS), 0, stream, frames, mask, weight,
                       bias, out, h, w, y0, y1, x0, x1, ho, wo, tiles_y, tiles_x, out_pitch);
    ELVIS_CHECK_LAUNCH("elvis_lpips_stem_u8");
    static const ElvisKernelName name("lpips_stem_kernel<%d>", ORDER);
    elvis_note_launch(name.s);
    return ELVIS_OK;
}

extern "C" int elvis_lpips_stem_u8(const uint8_t* frames, const uint8_t* mask, const float* weight, const float* bias, float* out, int n,
                                   int h, int w, int y0, int y1, int x0, int x1, int order, int out_pitch, elvis_stream_t stream) {
    ELVIS_REQUIRE(order == 0 || order == 1, "elvis_lpips_stem_u8: order must be 0 (rgb) or 1 (bgr), got %d", order);
    ELVIS_REQUIRE(n >= 0 && h > 0 && w > 0, "elvis_lpips_stem_u8: bad shape n=%d h=%d w=%d", n, h, w);
    ELVIS_REQUIRE(lpips_rect_ok(h, w, y0, y1, x0, x1), "elvis_lpips_stem_u8: rect (%d, %d, %d, %d) must lie inside the %d x %d frame and be at least %d x %d",
                  y0, y1, x0, x1, h, w, LPIPS_MIN_SIDE, LPIPS_MIN_SIDE);
    ELVIS_REQUIRE(out_pitch >= LPIPS_STEM_COUT && out_pitch % 8 == 0, "elvis_lpips_stem_u8: pitch %d must be a multiple of 8, at least %d", out_pitch,
                  LPIPS_STEM_COUT);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(frames && weight && bias && out, "elvis_lpips_stem_u8: null pointer");
    ELVIS_REQUIRE(lpips_aligned16(out), "elvis_lpips_stem_u8: out must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (order) return lpips_stem_launch<1>(frames, mask, weight, bias, out, n, h, w, y0, y1, x0, x1, out_pitch, s);
    return lpips_stem_launch<0>(frames, mask, weight, bias, out, n, h, w, y0, y1, x0, x1, out_pitch, s);
}

// ------------------------------------------------------------------------------------------------ 5x5 conv, 64 -> 192
// An implicit GEMM over K = 25 taps x 64 channels = 1600 on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32), with the
// channels as the rows of the result: A[co][k] = weight[k][co] (packed [1600][192], k = (ky 5 + kx) 64 + c, read from
// global memory - every workgroup reads the same 1.2 MB, which stays in L2), B[k][pixel] from the input tile staged in
// LDS with its two-pixel halo (zeros outside the image).  A workgroup takes 4 rows x 16 pixels x 192 channels; wave g takes
// channels 48 g .. 48 g + 47 as 3 x 4 tiles of 16 channels x 16 pixels (one row of the tile each).
// Summation order: the MFMA is a k-ordered fmaf chain, so each output is
//     acc = 0;  for k = 0 .. 1599 in order: acc = fmaf(w[k][co], x[k], acc);  relu(acc + bias)
// 1600 products per output, one chain.
__global__ __launch_bounds__(LPIPS_C5_THREADS) void lpips_conv5_kernel(const float* __restrict__ x, const float* __restrict__ weight,
                                                                       const float* __restrict__ bias, float* __restrict__ out, int h, int w,
                                                                       int tiles_y, int tiles_x, int in_pitch, int out_pitch) {
    __shared__ __attribute__((aligned(16))) float xt[LPIPS_C5_ROWS * LPIPS_C5_COLS * LPIPS_C5_LDS_PITCH];
    const int t = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, f = blockIdx.x / (tiles_x * tiles_y);
    const int oy0 = ty * LPIPS_C5_TY, ox0 = tx * LPIPS_C5_TX;

    for (int i = t; i < LPIPS_C5_ROWS * LPIPS_C5_COLS * (LPIPS_C5_CIN / 4); i += LPIPS_C5_THREADS) {
        const int pix = i / (LPIPS_C5_CIN / 4), q = i % (LPIPS_C5_CIN / 4);
        const int iy = oy0 - 2 + pix / LPIPS_C5_COLS, ix = ox0 - 2 + pix % LPIPS_C5_COLS;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (iy >= 0 && iy < h && ix >= 0 && ix < w)
            v = *reinterpret_cast<const float4*>(x + (((long long)f * h + iy) * w + ix) * in_pitch + q * 4);
        *reinterpret_cast<float4*>(xt + pix * LPIPS_C5_LDS_PITCH + q * 4) = v;
    }
    __syncthreads();

    const int lane = t & 63, g = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l16 = lane & 15, kq = lane >> 4;
    const int n0 = g * 48;
    float4v acc[3][LPIPS_C5_TY];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int m = 0; m < LPIPS_C5_TY; ++m) acc[j][m] = float4v{0.0f, 0.0f, 0.0f, 0.0f};

    for (int tap = 0; tap < 25; ++tap) {
        const int ky = tap / 5, kx = tap % 5;
        const float* wk = weight + (long long)(tap * LPIPS_C5_CIN + kq) * LPIPS_C5_COUT + n0 + l16;
        const float* xk = xt + (ky * LPIPS_C5_COLS + kx + l16) * LPIPS_C5_LDS_PITCH + kq;
#pragma unroll 4
        for (int cs = 0; cs < LPIPS_C5_CIN / 4; ++cs) {                   // channels 4 cs + kq
            float a[3], b[LPIPS_C5_TY];
#pragma unroll
            for (int j = 0; j < 3; ++j) a[j] = wk[cs * 4 * LPIPS_C5_COUT + j * 16];
#pragma unroll
            for (int m = 0; m < LPIPS_C5_TY; ++m) b[m] = xk[m * LPIPS_C5_COLS * LPIPS_C5_LDS_PITCH + cs * 4];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int m = 0; m < LPIPS_C5_TY; ++m) acc[j][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[m], acc[j][m], 0, 0, 0);
        }
    }
    // result tile (j, m): register r of lane (l16, kq) is channel n0 + 16 j + 4 kq + r of pixel (oy0 + m, ox0 + l16)
    const int ox = ox0 + l16;
#pragma unroll
    for (int m = 0; m < LPIPS_C5_TY; ++m) {
        const int oy = oy0 + m;
        if (oy >= h || ox >= w) continue;
        float* o = out + (((long long)f * h + oy) * w + ox) * out_pitch;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int co = n0 + j * 16 + kq * 4;
            const float4 bv = *reinterpret_cast<const float4*>(bias + co);
            float4 v;
            v.x = fmaxf(acc[j][m][0] + bv.x, 0.0f);
            v.y = fmaxf(acc[j][m][1] + bv.y, 0.0f);
            v.z = fmaxf(acc[j][m][2] + bv.z, 0.0f);
            v.w = fmaxf(acc[j][m][3] + bv.w, 0.0f);
            *reinterpret_cast<float4*>(o + co) = v;
        }
    }
}

extern "C" int elvis_lpips_conv5_f32(const float* x, const float* weight, const float* bias, float* out, int n, int h, int w, int in_pitch,
                                     int out_pitch, elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 0 && h > 0 && w > 0, "elvis_lpips_conv5_f32: bad shape n=%d h=%d w=%d", n, h, w);
    ELVIS_REQUIRE(in_pitch >= LPIPS_C5_CIN && in_pitch % 8 == 0 && out_pitch >= LPIPS_C5_COUT && out_pitch % 8 == 0,
                  "elvis_lpips_conv5_f32: pitches %d and %d must be multiples of 8, at least %d and %d", in_pitch, out_pitch, LPIPS_C5_CIN,
                  LPIPS_C5_COUT);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(x && weight && bias && out, "elvis_lpips_conv5_f32: null pointer");
    ELVIS_REQUIRE(lpips_aligned16(x) && lpips_aligned16(bias) && lpips_aligned16(out), "elvis_lpips_conv5_f32: x, bias and out must be 16-byte aligned");
    const int tiles_y = cdiv(h, LPIPS_C5_TY), tiles_x = cdiv(w, LPIPS_C5_TX);
    ELVIS_REQUIRE((long long)n * tiles_y * tiles_x <= 0x7fffffffLL, "elvis_lpips_conv5_f32: n=%d h=%d w=%d is more than one launch holds", n, h, w);
    hipLaunchKernelGGL(lpips_conv5_kernel, dim3(n * tiles_y * tiles_x), dim3(LPIPS_C5_THREADS), 0, (hipStream_t)stream, x, weight, bias, out,
                       h, w, tiles_y, tiles_x, in_pitch, out_pitch);
    ELVIS_CHECK_LAUNCH("elvis_lpips_conv5_f32");
    elvis_note_launch("lpips_conv5_kernel");
    return ELVIS_OK;
}

// ------------------------------------------------------------------------------------------------ max-pool 3x3 stride 2
// No padding, floor: output (y, x) is the maximum over input rows 2 y .. 2 y + 2 and columns 2 x .. 2 x + 2.  One lane per
// four channels of an output pixel.
__global__ __launch_bounds__(LPIPS_POOL_THREADS) void lpips_maxpool_kernel(const float* __restrict__ x, float* __restrict__ out, long long total,
                                                                           int h, int w, int ho, int wo, int c4, int in_pitch, int out_pitch) {
    const long long i = (long long)blockIdx.x * LPIPS_POOL_THREADS + threadIdx.x;
    if (i >= total) return;
    const int q = (int)(i % c4);
    const long long pix = i / c4;
    const int ox = (int)(pix % wo), oy = (int)((pix / wo) % ho);
    const long long f = pix / ((long long)wo * ho);
    const float* src = x + ((f * h + 2 * oy) * w + 2 * ox) * in_pitch + q * 4;
    float4 m = *reinterpret_cast<const float4*>(src);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float4 v = *reinterpret_cast<const float4*>(src + ((long long)dy * w + dx) * in_pitch);
            m.x = fmaxf(m.x, v.x);
            m.y = fmaxf(m.y, v.y);
            m.z = fmaxf(m.z, v.z);
            m.w = fmaxf(m.w, v.w);
        }
    *reinterpret_cast<float4*>(out + pix * out_pitch + q * 4) = m;
}

extern "C" int elvis_lpips_maxpool_f32(const float* x, float* out, int n, int h, int w, int c, int in_pitch, int out_pitch,
                                       elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 0 && h >= 3 && w >= 3, "elvis_lpips_maxpool_f32: bad shape n=%d h=%d w=%d (a 3 x 3 window)", n, h, w);
    ELVIS_REQUIRE(c > 0 && c % 4 == 0, "elvis_lpips_maxpool_f32: channels must come in fours, got %d", c);
    ELVIS_REQUIRE(in_pitch >= c && in_pitch % 8 == 0 && out_pitch >= c && out_pitch % 8 == 0,
                  "elvis_lpips_maxpool_f32: pitches %d and %d must be multiples of 8, at least %d", in_pitch, out_pitch, c);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(x && out, "elvis_lpips_maxpool_f32: null pointer");
    ELVIS_REQUIRE(lpips_aligned16(x) && lpips_aligned16(out), "elvis_lpips_maxpool_f32: x and out must be 16-byte aligned");
    const int ho = lpips_pool_size(h), wo = lpips_pool_size(w);
    const long long total = (long long)n * ho * wo * (c / 4);
    ELVIS_REQUIRE(cdiv(total, LPIPS_POOL_THREADS) <= 0x7fffffffLL, "elvis_lpips_maxpool_f32: n=%d h=%d w=%d is more than one launch holds", n, h, w);
    hipLaunchKernelGGL(lpips_maxpool_kernel, dim3(cdiv(total, LPIPS_POOL_THREADS)), dim3(LPIPS_POOL_THREADS), 0, (hipStream_t)stream, x, out,
                       total, h, w, ho, wo, c / 4, in_pitch, out_pitch);
    ELVIS_CHECK_LAUNCH("elvis_lpips_maxpool_f32");
    elvis_note_launch("lpips_maxpool_kernel");
    return ELVIS_OK;
}

// ------------------------------------------------------------------------------------------------ distance of one tap
// One wave per pixel; lane l holds channels l, l + 64, ... (C <= 384: at most six) of both feature vectors, read once.
//     sx = sum_c x^2, sy = sum_c y^2        per lane an fmaf chain over its channels in rising order, then the xor
//                                           butterfly over the wave (32, 16, .. 1): every lane gets the same total
//     xh = x / (sqrtf(sx) + 1e-10f), yh = y / (sqrtf(sy) + 1e-10f)
//     v  = sum_c w_c (xh - yh)^2            fmaf(w_c, d d, v) per lane in rising order, then the same butterfly
// A wave adds the v of its 16 pixels in float64, in pixel order; lane 0 of the workgroup adds the four waves in wave
// order and writes one partial sum to the workspace.  lpips_finish_kernel adds a frame's partials in index order and
// divides by the pixel count, in float64.
__global__ __launch_bounds__(LPIPS_DIST_THREADS) void lpips_distance_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                            const float* __restrict__ weight, double* __restrict__ partial,
                                                                            long long hw, int blocks, int c, int pitch) {
    __shared__ double red[LPIPS_DIST_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int block = blockIdx.x % blocks, f = blockIdx.x / blocks;
    float wr[LPIPS_DIST_MAX_C / 64];
#pragma unroll
    for (int j = 0; j < LPIPS_DIST_MAX_C / 64; ++j) wr[j] = lane + 64 * j < c ? weight[lane + 64 * j] : 0.0f;
    double total = 0.0;
    for (int i = 0; i < LPIPS_DIST_PIXELS / 4; ++i) {
        const long long p = lpips_dist_pixel(hw, block, wave, i);
        if (p < 0) break;                                                 // wave-uniform
        const long long at = lpips_feature_offset(f, hw, p, pitch, 0);
        float xv[LPIPS_DIST_MAX_C / 64], yv[LPIPS_DIST_MAX_C / 64];
        float sx = 0.0f, sy = 0.0f;
#pragma unroll
        for (int j = 0; j < LPIPS_DIST_MAX_C / 64; ++j) {
            const bool in = lane + 64 * j < c;
            xv[j] = in ? x[at + lane + 64 * j] : 0.0f;
            yv[j] = in ? y[at + lane + 64 * j] : 0.0f;
            sx = fmaf(xv[j], xv[j], sx);
            sy = fmaf(yv[j], yv[j], sy);
        }
        const float nx = sqrtf(wave_sum(sx)) + 1e-10f, ny = sqrtf(wave_sum(sy)) + 1e-10f;
        float v = 0.0f;
#pragma unroll
        for (int j = 0; j < LPIPS_DIST_MAX_C / 64; ++j) {
            const float d = xv[j] / nx - yv[j] / ny;
            v = fmaf(wr[j], d * d, v);
        }
        total += (double)wave_sum(v);
    }
    if (lane == 0) red[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) partial[(long long)f * blocks + block] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void lpips_finish_kernel(const double* __restrict__ partial, double* __restrict__ out, int n, long long hw, int blocks, int accumulate) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += partial[(long long)f * blocks + b];
    s /= (double)hw;
    out[f] = accumulate ? out[f] + s : s;
}

static int lpips_distance_shape(const char* who, int n, int h, int w) {
    ELVIS_REQUIRE(n >= 0 && h > 0 && w > 0, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    ELVIS_REQUIRE((long long)n * lpips_dist_blocks((long long)h * w) <= 0x7fffffffLL, "%s: n=%d h=%d w=%d is more than one launch holds", who, n, h, w);
    return ELVIS_OK;
}

extern "C" size_t elvis_lpips_distance_workspace_bytes(int n, int h, int w) {
    if (lpips_distance_shape("elvis_lpips_distance_workspace_bytes", n, h, w) != ELVIS_OK) return 0;
    return (size_t)n * lpips_dist_blocks((long long)h * w) * sizeof(double);
}

extern "C" int elvis_lpips_distance_f64(const float* x, const float* y, const float* weight, void* workspace, double* out, int n, int h,
                                        int w, int c, int pitch, int accumulate, elvis_stream_t stream) {
    int rc = lpips_distance_shape("elvis_lpips_distance_f64", n, h, w);
    if (rc) return rc;
    ELVIS_REQUIRE(c > 0 && c <= LPIPS_DIST_MAX_C, "elvis_lpips_distance_f64: 1 to %d channels, got %d", LPIPS_DIST_MAX_C, c);
    ELVIS_REQUIRE(pitch >= c && pitch % 8 == 0, "elvis_lpips_distance_f64: pitch %d must be a multiple of 8, at least %d", pitch, c);
    ELVIS_REQUIRE(accumulate == 0 || accumulate == 1, "elvis_lpips_distance_f64: accumulate must be 0 or 1, got %d", accumulate);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(x && y && weight && workspace && out, "elvis_lpips_distance_f64: null pointer");
    const long long hw = (long long)h * w;
    const int blocks = lpips_dist_blocks(hw);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lpips_distance_kernel, dim3(n * blocks), dim3(LPIPS_DIST_THREADS), 0, s, x, y, weight, (double*)workspace, hw, blocks, c, pitch);
    ELVIS_CHECK_LAUNCH("elvis_lpips_distance_f64");
    elvis_note_launch("lpips_distance_kernel");
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(cdiv(n, 64)), dim3(64), 0, s, (const double*)workspace, out, n, hw, blocks, accumulate);
    ELVIS_CHECK_LAUNCH("elvis_lpips_distance_f64");
    elvis_note_launch("lpips_finish_kernel");
    return ELVIS_OK;
}
