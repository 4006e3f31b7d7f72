// What the per-block u8 kernels of classical.hip, degrade.hip and presley_degrade.hip share, each defined once: the block
// address, the LDS staging and copy loops, BORDER_REFLECT_101, OpenCV's integer-ratio INTER_AREA and INTER_LINEAR rules on
// u8, the block-size and channel limits, and the host-side check of the block-map arguments.
#pragma once
#include "common.h"

constexpr int kMaxBlock = 32;
constexpr int kMaxChannels = 4;

static __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static __device__ __forceinline__ int reflect101(int i, int n) {   // BORDER_REFLECT_101: -1 -> 1, n -> n-2, until inside (n == 1: 0)
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// The block of a one-wave-per-block kernel: blockIdx.x -> frame f, block row byi, block column bxi; rs is the row stride
// of the [n][h][w][c] frames and base the offset of the block's first element
struct BlockAddr {
    int blk, bxi, byi, f;
    long long rs, base;
    __device__ __forceinline__ BlockAddr(int h, int w, int c, int b, int by, int bx) {
        blk = blockIdx.x;
        bxi = blk % bx;
        byi = (blk / bx) % by;
        f = blk / (bx * by);
        rs = (long long)w * c;
        base = ((long long)f * h + (long long)byi * b) * rs + (long long)bxi * b * c;
    }
};

// rows x rowlen elements at src[base + y * rs + x], the wave's lanes strided over them: into a dense LDS tile ...
static __device__ __forceinline__ void stage_block(const uint8_t* src, uint8_t* tile, long long base, long long rs, int rows,
                                                   int rowlen) {
    for (int e = threadIdx.x; e < rows * rowlen; e += ELVIS_WAVE) {
        const int y = e / rowlen;
        tile[e] = src[base + y * rs + (e - y * rowlen)];
    }
}

// ... or straight to the same place of dst (a block that is kept as it is)
static __device__ __forceinline__ void copy_block(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long base,
                                                  long long rs, int b, int c) {
    const int rowlen = b * c;
    for (int e = threadIdx.x; e < b * rowlen; e += ELVIS_WAVE) {
        const int y = e / rowlen;
        const long long o = base + y * rs + (e - y * rowlen);
        dst[o] = src[o];
    }
}

// cv2.resize(INTER_AREA) on u8 at the integer ratio fac (cv::resizeAreaFast_): the box sum of fac x fac samples becomes
// (sum + 2) >> 2 at fac 2, otherwise round-half-even(sum * inv) with inv = 1.0f / (fac * fac), saturated
static __device__ __forceinline__ uint32_t area_round(uint32_t sum, int fac, float inv) {
    const uint32_t v = fac == 2 ? (sum + 2) >> 2 : (uint32_t)__float2int_rn(__fmul_rn((float)sum, inv));
    return v > 255 ? 255 : v;
}

// the same, for the result (sy, sx, ch) of a [.][rowlen / c][c] u8 tile in LDS
static __device__ __forceinline__ uint32_t area_box(const uint8_t* tile, int rowlen, int c, int sy, int sx, int ch, int fac,
                                                    float inv) {
    uint32_t sum = 0;
    for (int dy = 0; dy < fac; ++dy) {
        const uint8_t* row = tile + (sy * fac + dy) * rowlen + sx * fac * c + ch;
        for (int dx = 0; dx < fac; ++dx) sum += row[dx * c];
    }
    return area_round(sum, fac, inv);
}

// cv2.resize(INTER_LINEAR) source index and 11-bit weights of destination index d (s source samples, b results)
static __device__ __forceinline__ void linear_coef(int d, int s, int b, int& i0, int& a0, int& a1) {
    float f = (float)(((double)d + 0.5) * ((double)s / (double)b) - 0.5);   // double arithmetic, one rounding to float
    int i = (int)floorf(f);
    f = __fsub_rn(f, (float)i);
    if (i < 0) { i = 0; f = 0.f; }
    if (i >= s - 1) { i = s - 1; f = 0.f; }
    i0 = i;
    a0 = __float2int_rn(__fmul_rn(__fsub_rn(1.0f, f), 2048.0f));
    a1 = __float2int_rn(__fmul_rn(f, 2048.0f));
}

// cv2.resize(INTER_LINEAR) on u8, one destination pixel from its four source samples: horizontal pass in 11-bit fixed
// point (a0, a1), vertical pass (b0*(S0>>4)>>16 + b1*(S1>>4)>>16 + 2)>>2 (b0, b1), saturated
static __device__ __forceinline__ int linear_mix(int s00, int s01, int s10, int s11, int a0, int a1, int b0, int b1) {
    const int r0 = s00 * a0 + s01 * a1;
    const int r1 = s10 * a0 + s11 * a1;
    return clampi((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2, 0, 255);
}

// Host: the arguments of a kernel that takes [n][h][w][c] u8 frames and an [n][by][bx] map of the whole blocks (pixels past
// the last whole block are left alone).  `pointers` is the conjunction of the caller's pointers; `pow2` also asks for a
// power-of-two block.
static inline int check_block_maps(bool pointers, int n, int h, int w, int c, int b, int by, int bx, bool pow2, const char* what) {
    ELVIS_REQUIRE(pointers, "%s: null pointer", what);
    ELVIS_REQUIRE(n > 0 && h > 0 && w > 0, "%s: bad shape", what);
    ELVIS_REQUIRE(c >= 1 && c <= kMaxChannels, "%s: %d channels (1..%d supported)", what, c, kMaxChannels);
    if (pow2)
        ELVIS_REQUIRE(b >= 2 && b <= kMaxBlock && (b & (b - 1)) == 0, "%s: block_size %d must be a power of two in [2, %d]", what,
                      b, kMaxBlock);
    else
        ELVIS_REQUIRE(b >= 2 && b <= kMaxBlock, "%s: block_size %d outside [2, %d]", what, b, kMaxBlock);
    ELVIS_REQUIRE(by > 0 && bx > 0 && by == h / b && bx == w / b, "%s: the map must be %dx%d for a %dx%d image and block_size %d",
                  what, h / b, w / b, h, w, b);
    ELVIS_REQUIRE((long long)n * by * bx < (1LL << 31), "%s: too many blocks", what);
    return ELVIS_OK;
}
