// Classical per-block restorers on the device: the OpenCV baselines ELVIS and Presley compare every neural slot
// against.
//   elvis_classical_lanczos_u8  - restore_downsample_opencv_lanczos (elvis.py:2773-2820): every b x b block of
//                                 level L > 0 is INTER_AREA-downscaled to s = max(1, b >> L) and resized back to
//                                 b x b with INTER_LANCZOS4
//   elvis_classical_unsharp_u8  - restore_blur_opencv_unsharp_mask (elvis.py:2822-2866) and the utils.py forms
//                                 (utils.py:1253-1392): GaussianBlur(sigma = L, ksize 6L+1, BORDER_REFLECT_101 at the
//                                 tile's edges), then addWeighted(tile, 1 + L/2, blurred, -L/2, 0); the tile is the
//                                 block, or the block grown by `halo` pixels and clipped at the frame
//   elvis_temporal_blend_u8     - utils.py:1308-1312: out[f] = uint8(tb * out[f-1] + (1 - tb) * cur[f]) in float64
// OpenCV is absent from the build and GPU environments, so its 8-bit fixed-point rules are restated (DESIGN.md 7,
// "parity unpinned"); what is pinned is bit-exactness against the numpy restatement in tests/_classical_ref.py.
// The tap tables are built once on the host (elvis_amd/classical.py) so that the kernels are pure integer work.
#include "block_u8.h"

namespace {

constexpr int kMaxHalo = 32;
constexpr int kLanczosPhases = 32;   // taps[(log2(f) - 1)][d][8] for d < kLanczosPhases

// One wave per block (the level is uniform per workgroup).  LDS: the block (u8), the INTER_AREA result (int), the
// horizontal Lanczos pass (int), this factor's taps (int).  Every loop strides the lanes over (pixel, channel).
__global__ __launch_bounds__(64) void classical_lanczos_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ levels,
                                                               uint8_t* __restrict__ dst, int h, int w, int c, int b, int lb,
                                                               int by, int bx, const int16_t* __restrict__ taps) {
    extern __shared__ int lds[];
    const BlockAddr at(h, w, c, b, by, bx);
    const long long rs = at.rs, base = at.base;
    const int lv = clampi(levels[at.blk], 0, 16);
    if (lv == 0) {
        copy_block(src, dst, base, rs, b, c);
        return;
    }
    const int lf = lv < lb ? lv : lb;           // log2 of the integer scale b / s
    const int fac = 1 << lf;
    const int s = b >> lf;                      // max(1, b >> L)
    const int rowlen = b * c;
    int* tap = lds;                             // [b][8]
    int* small = tap + b * 8;                   // [s][s][c]
    int* hp = small + s * s * c;                // [s][b][c]
    uint8_t* blkp = (uint8_t*)(hp + s * b * c); // [b][b][c]
    for (int e = threadIdx.x; e < b * 8; e += ELVIS_WAVE) tap[e] = taps[(lf - 1) * kLanczosPhases * 8 + e];
    stage_block(src, blkp, base, rs, b, rowlen);
    __syncthreads();
    // INTER_AREA at the integer scale fac
    const float inv = 1.0f / (float)(fac * fac);
    for (int e = threadIdx.x; e < s * s * c; e += ELVIS_WAVE) {
        const int ch = e % c;
        const int sx = (e / c) % s;
        const int sy = e / (c * s);
        small[e] = (int)area_box(blkp, rowlen, c, sy, sx, ch, fac, inv);
    }
    __syncthreads();
    // horizontal INTER_LANCZOS4 pass: s rows x b columns, source columns clamped (BORDER_REPLICATE).
    // Source column of destination d: floor((d + 0.5) / fac - 0.5) = floor((2d + 1 - fac) / (2 fac)), exact.
    for (int e = threadIdx.x; e < s * rowlen; e += ELVIS_WAVE) {
        const int ch = e % c;
        const int d = (e / c) % b;
        const int r = e / rowlen;
        const int num = 2 * d + 1 - fac;
        const int x0 = (num >= 0 ? num / (2 * fac) : -((2 * fac - 1 - num) / (2 * fac))) - 3;
        const int* a = tap + d * 8;
        const int* row = small + r * s * c + ch;
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += row[clampi(x0 + k, 0, s - 1) * c] * a[k];
        hp[e] = acc;
    }
    __syncthreads();
    // vertical pass, then (v + 2^21) >> 22 saturated to u8 (FixedPtCast<int, uchar, 22>); int32 cannot overflow
    // (bound proven over every phase pair in tests/test_classical_host.py)
    for (int e = threadIdx.x; e < b * rowlen; e += ELVIS_WAVE) {
        const int y = e / rowlen;
        const int xc = e - y * rowlen;
        const int num = 2 * y + 1 - fac;
        const int y0 = (num >= 0 ? num / (2 * fac) : -((2 * fac - 1 - num) / (2 * fac))) - 3;
        const int* be = tap + y * 8;
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += hp[clampi(y0 + k, 0, s - 1) * rowlen + xc] * be[k];
        dst[base + y * rs + xc] = (uint8_t)clampi((acc + (1 << 21)) >> 22, 0, 255);
    }
}

// One wave per block.  LDS: the tile (u8 [th][tw][c]) and the horizontal pass over the block's b centre columns
// (u16 [th][b][c], 8.8 fixed point: u8 x tap summed, at most 255 * 256).  The vertical pass accumulates in u32
// (16.16) and rounds once.  Taps: taps[tap_offsets[L] + k], k < 6L + 1, read with wave-uniform indices.
__global__ __launch_bounds__(64) void classical_unsharp_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ levels,
                                                               uint8_t* __restrict__ dst, int h, int w, int c, int b, int by,
                                                               int bx, int halo, const int16_t* __restrict__ taps,
                                                               const int32_t* __restrict__ tap_offsets, int max_level) {
    extern __shared__ int lds[];
    const BlockAddr at(h, w, c, b, by, bx);
    const long long rs = at.rs;
    const long long fbase = (long long)at.f * h * rs;
    const int y0 = at.byi * b, x0 = at.bxi * b;
    const int lv = clampi(levels[at.blk], 0, max_level);
    if (lv == 0) {
        copy_block(src, dst, fbase + (long long)y0 * rs + (long long)x0 * c, rs, b, c);
        return;
    }
    // tiler._extract_tile_with_halo: grown by `halo` where the frame allows
    const int top = y0 < halo ? y0 : halo, left = x0 < halo ? x0 : halo;
    const int ty0 = y0 - top, tx0 = x0 - left;
    const int th = (y0 + b + halo < h ? y0 + b + halo : h) - ty0;
    const int tw = (x0 + b + halo < w ? x0 + b + halo : w) - tx0;
    const int trow = tw * c, hrow = b * c;
    uint16_t* hp = (uint16_t*)lds;                  // [th][b][c]
    uint8_t* tile = (uint8_t*)(hp + ((th * hrow + 1) & ~1));
    const long long tbase = fbase + (long long)ty0 * rs + (long long)tx0 * c;
    stage_block(src, tile, tbase, rs, th, trow);
    __syncthreads();
    const int n = 6 * lv + 1, rad = 3 * lv;
    const int16_t* k0 = taps + tap_offsets[lv];
    for (int e = threadIdx.x; e < th * hrow; e += ELVIS_WAVE) {
        const int ch = e % c;
        const int p = left + (e / c) % b - rad;
        const uint8_t* row = tile + (e / hrow) * trow + ch;
        uint32_t acc = 0;
        for (int k = 0; k < n; ++k) acc += (uint32_t)row[reflect101(p + k, tw) * c] * (uint32_t)k0[k];
        hp[e] = (uint16_t)acc;
    }
    __syncthreads();
    const long long obase = fbase + (long long)y0 * rs + (long long)x0 * c;
    for (int e = threadIdx.x; e < b * hrow; e += ELVIS_WAVE) {
        const int i = e / hrow;
        const int jc = e - i * hrow;
        const int p = top + i - rad;
        uint32_t acc = 0;
        for (int k = 0; k < n; ++k) acc += (uint32_t)hp[reflect101(p + k, th) * hrow + jc] * (uint32_t)k0[k];
        const int blur = (int)((acc + 0x8000u) >> 16);
        const int x = tile[(top + i) * trow + left * c + jc];
        // addWeighted(x, 1 + L/2, blur, -L/2, 0) on u8: exact in float32, so round_half_even(((2 + L) x - L blur) / 2)
        const int v2 = (2 + lv) * x - lv * blur;
        int q = v2 >> 1;                            // floor(v2 / 2)
        q += (v2 & 1) & (q & 1);                    // a tie goes to the even neighbour
        dst[obase + (long long)i * rs + jc] = (uint8_t)clampi(q, 0, 255);
    }
}

// One thread per u8 element, walking the frames in order (frame f - 1's blended output feeds frame f).
__global__ __launch_bounds__(256) void temporal_blend_kernel(const uint8_t* cur, uint8_t* out, int nframes, long long pixels,
                                                             double tb, double one_minus_tb) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    uint8_t prev = cur[i];
    out[i] = prev;
    for (int f = 1; f < nframes; ++f) {
        const long long o = (long long)f * pixels + i;
        const double v = __dadd_rn(__dmul_rn(tb, (double)prev), __dmul_rn(one_minus_tb, (double)cur[o]));
        const int q = (int)v;                       // numpy astype(uint8) of a value in [0, 256): truncation
        prev = (uint8_t)clampi(q, 0, 255);
        out[o] = prev;
    }
}

}  // namespace

extern "C" int elvis_classical_lanczos_u8(const uint8_t* src, const int32_t* levels, uint8_t* dst, int n, int h, int w, int c,
                                          int block, int by, int bx, const int16_t* taps, elvis_stream_t stream) {
    int rc = check_block_maps(src && levels && dst && taps, n, h, w, c, block, by, bx, true, "elvis_classical_lanczos_u8");
    if (rc) return rc;
    const int lb = __builtin_ctz((unsigned)block);
    const int s_max = block / 2;
    const size_t shmem = sizeof(int) * (block * 8 + s_max * s_max * c + s_max * block * c) + (size_t)block * block * c;
    hipLaunchKernelGGL(classical_lanczos_kernel, dim3((unsigned)(n * by * bx)), dim3(ELVIS_WAVE), shmem, (hipStream_t)stream, src,
                       levels, dst, h, w, c, block, lb, by, bx, taps);
    ELVIS_CHECK_LAUNCH("elvis_classical_lanczos_u8");
    return ELVIS_OK;
}

extern "C" int elvis_classical_unsharp_u8(const uint8_t* src, const int32_t* levels, uint8_t* dst, int n, int h, int w, int c,
                                          int block, int by, int bx, int halo, const int16_t* taps, const int32_t* tap_offsets,
                                          int max_level, elvis_stream_t stream) {
    int rc = check_block_maps(src && levels && dst && taps, n, h, w, c, block, by, bx, true, "elvis_classical_unsharp_u8");
    if (rc) return rc;
    ELVIS_REQUIRE(tap_offsets, "elvis_classical_unsharp_u8: null pointer");
    ELVIS_REQUIRE(halo >= 0 && halo <= kMaxHalo, "elvis_classical_unsharp_u8: halo %d outside [0, %d]", halo, kMaxHalo);
    ELVIS_REQUIRE(max_level >= 1 && max_level <= ELVIS_CLASSICAL_MAX_LEVEL,
                  "elvis_classical_unsharp_u8: max_level %d outside [1, %d]", max_level, ELVIS_CLASSICAL_MAX_LEVEL);
    const int th = block + 2 * halo < h ? block + 2 * halo : h;
    const int tw = block + 2 * halo < w ? block + 2 * halo : w;
    const size_t shmem = sizeof(uint16_t) * (size_t)((th * block * c + 1) & ~1) + (size_t)th * tw * c;   // <= 60 KiB
    hipLaunchKernelGGL(classical_unsharp_kernel, dim3((unsigned)(n * by * bx)), dim3(ELVIS_WAVE), shmem, (hipStream_t)stream, src,
                       levels, dst, h, w, c, block, by, bx, halo, taps, tap_offsets, max_level);
    ELVIS_CHECK_LAUNCH("elvis_classical_unsharp_u8");
    return ELVIS_OK;
}

extern "C" int elvis_temporal_blend_u8(const uint8_t* cur, uint8_t* out, int nframes, long long pixels, double tb,
                                       double one_minus_tb, elvis_stream_t stream) {
    ELVIS_REQUIRE(cur && out, "elvis_temporal_blend_u8: null pointer");
    ELVIS_REQUIRE(nframes > 0 && pixels > 0, "elvis_temporal_blend_u8: bad shape");
    ELVIS_REQUIRE(tb >= 0.0 && tb <= 1.0 && one_minus_tb >= 0.0 && one_minus_tb <= 1.0,
                  "elvis_temporal_blend_u8: blend weights %g, %g outside [0, 1]", tb, one_minus_tb);
    const long long blocks = (pixels + 255) / 256;
    ELVIS_REQUIRE(blocks < (1LL << 31), "elvis_temporal_blend_u8: too many pixels");
    hipLaunchKernelGGL(temporal_blend_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, cur, out, nframes,
                       pixels, tb, one_minus_tb);
    ELVIS_CHECK_LAUNCH("elvis_temporal_blend_u8");
    return ELVIS_OK;
}
