// Decoder hand-off: planar I420 frames, what a video decoder emits, to packed 8-bit RGB (or BGR) - the way back from
// handoff.hip, cv2.cvtColor(planes, COLOR_YUV2RGB_I420) per frame.  Integer arithmetic only (OpenCV 4.x
// YUV420p2RGB8Invoker, 20-bit fixed point, i420.h); memory-bound: 6 bytes read and 12 written per 2x2 pixels, no LDS, no
// atomics.  Two kernels: strips of 8 pixels with a byte path for every width and alignment, strips of 16 where all is on
// 16 bytes.
#include "common.h"
#include "i420.h"

// One 2x2 quad: four lumas, one (u, v) pair replicated over them - not interpolated, as in OpenCV.
template <bool BGR>
__device__ __forceinline__ void i420_quad(int ya, int yb, int yc, int yd, int u, int v, uint8_t* o0, uint8_t* o1) {
    u -= 128;
    v -= 128;
    const int t[4] = {i420_luma_term(ya), i420_luma_term(yb), i420_luma_term(yc), i420_luma_term(yd)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint8_t* o = (k < 2 ? o0 : o1) + 3 * (k & 1);
        o[BGR ? 2 : 0] = i420_to_r(t[k], u, v);
        o[1] = i420_to_g(t[k], u, v);
        o[BGR ? 0 : 2] = i420_to_b(t[k], u, v);
    }
}

// The mirror image of rgb_to_i420_kernel: one lane per strip of 2 rows x 8 pixels; consecutive lanes take consecutive
// strips of a row pair, then the next row pair, then the next frame, so a wave's loads and stores are contiguous.  WIDE
// (w % 4 == 0, src and dst 4-byte aligned) makes every row and every full strip start on a dword: a full strip is 2
// dwords of Y per row and 4 bytes each of U and V in, 6 dwords per row out.  U and V rows start on a dword only where
// w % 8 == 0 (a chroma row is w / 2 bytes), so their 4 bytes come in as one dword when the address allows it and as
// bytes otherwise.  The last strip of a width that is no multiple of 8, and every strip without WIDE, goes quad by quad
// in bytes; a strip never touches a byte past its own `cnt` pixels.
template <bool BGR>
__global__ __launch_bounds__(256) void i420_to_rgb_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          long long items, int h, int w, int strips, int wide) {
    const int h2 = h / 2, w2 = w / 2;
    const long long frame_in = (long long)h2 * 3 * w;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < items) {
        const int s = (int)(i % strips);
        const long long t = i / strips;
        const int rp = (int)(t % h2);
        const long long f = t / h2;
        const int x = s * 8;
        const int cnt = min(8, w - x);                                  // even: w is
        const uint8_t* y0 = src + f * frame_in + (long long)(2 * rp) * w + x;
        const uint8_t* y1 = y0 + w;
        const uint8_t* pu = src + f * frame_in + (long long)h * w + (long long)rp * w2 + x / 2;
        const uint8_t* pv = pu + (long long)h2 * w2;
        uint8_t* p0 = dst + ((f * h + 2 * rp) * w + x) * 3;
        uint8_t* p1 = p0 + (long long)w * 3;
        if (wide && cnt == 8) {
            union { uint32_t d[2]; uint8_t b[8]; } a0, a1;
            union { uint32_t d; uint8_t b[4]; } au, av;
            union { uint32_t d[6]; uint8_t b[24]; } o0, o1;
            const uint32_t* q0 = reinterpret_cast<const uint32_t*>(y0);
            const uint32_t* q1 = reinterpret_cast<const uint32_t*>(y1);
            a0.d[0] = q0[0]; a0.d[1] = q0[1];
            a1.d[0] = q1[0]; a1.d[1] = q1[1];
            if (((uintptr_t)pu & 3) == 0) {
                au.d = *reinterpret_cast<const uint32_t*>(pu);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) au.b[k] = pu[k];
            }
            if (((uintptr_t)pv & 3) == 0) {
                av.d = *reinterpret_cast<const uint32_t*>(pv);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) av.b[k] = pv[k];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                i420_quad<BGR>(a0.b[2 * q], a0.b[2 * q + 1], a1.b[2 * q], a1.b[2 * q + 1], au.b[q], av.b[q], o0.b + 6 * q, o1.b + 6 * q);
            uint32_t* s0 = reinterpret_cast<uint32_t*>(p0);
            uint32_t* s1 = reinterpret_cast<uint32_t*>(p1);
#pragma unroll
            for (int k = 0; k < 6; ++k) { s0[k] = o0.d[k]; s1[k] = o1.d[k]; }
        } else {
            for (int p = 0; p < cnt; p += 2)
                i420_quad<BGR>(y0[p], y0[p + 1], y1[p], y1[p + 1], pu[p / 2], pv[p / 2], p0 + 3 * p, p1 + 3 * p);
        }
    }
}

// The same conversion where w % 16 == 0 and both pointers are 16-byte aligned: a lane takes two strips, 2 rows x 16
// pixels.  Every row, plane and frame then starts on 16 bytes (a chroma row on 8) and every strip is whole, so there is
// no tail: 16 bytes of Y per row and 8 bytes each of U and V in, three 16-byte stores per row out.
template <bool BGR>
__global__ __launch_bounds__(256) void i420_to_rgb_x16_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              long long items, int h, int w) {
    const int h2 = h / 2, w2 = w / 2, strips = w / 16;
    const long long frame_in = (long long)h2 * 3 * w;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < items) {
        const int s = (int)(i % strips);
        const long long t = i / strips;
        const int rp = (int)(t % h2);
        const long long f = t / h2;
        const int x = s * 16;
        const uint8_t* y0 = src + f * frame_in + (long long)(2 * rp) * w + x;
        const uint8_t* pu = src + f * frame_in + (long long)h * w + (long long)rp * w2 + x / 2;
        const uint8_t* pv = pu + (long long)h2 * w2;
        uint8_t* p0 = dst + ((f * h + 2 * rp) * w + x) * 3;
        union { uint4 q; uint8_t b[16]; } a0, a1;
        union { uint2 q; uint8_t b[8]; } au, av;
        union { uint4 q[3]; uint8_t b[48]; } o0, o1;
        a0.q = *reinterpret_cast<const uint4*>(y0);
        a1.q = *reinterpret_cast<const uint4*>(y0 + w);
        au.q = *reinterpret_cast<const uint2*>(pu);
        av.q = *reinterpret_cast<const uint2*>(pv);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            i420_quad<BGR>(a0.b[2 * q], a0.b[2 * q + 1], a1.b[2 * q], a1.b[2 * q + 1], au.b[q], av.b[q], o0.b + 6 * q, o1.b + 6 * q);
        uint4* s0 = reinterpret_cast<uint4*>(p0);
        uint4* s1 = reinterpret_cast<uint4*>(p0 + (long long)w * 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) { s0[k] = o0.q[k]; s1[k] = o1.q[k]; }
    }
}

extern "C" int elvis_i420_to_rgb_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int bgr, elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 0 && h >= 0 && w >= 0, "elvis_i420_to_rgb_u8: bad shape n=%d h=%d w=%d", n, h, w);
    ELVIS_REQUIRE(h % 2 == 0 && w % 2 == 0, "elvis_i420_to_rgb_u8: I420 needs an even height and width, got h=%d w=%d", h, w);
    if (n == 0 || h == 0 || w == 0) return ELVIS_OK;
    ELVIS_REQUIRE(src && dst, "elvis_i420_to_rgb_u8: null pointer");
    if (w % 16 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 16 == 0) {
        const long long items = (long long)n * (h / 2) * (w / 16);
        const long long blocks = (items + 255) / 256;
        ELVIS_REQUIRE(blocks <= 0x7fffffffLL, "elvis_i420_to_rgb_u8: n=%d h=%d w=%d is more than one launch holds", n, h, w);
        if (bgr) {
            hipLaunchKernelGGL(i420_to_rgb_x16_kernel<true>, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, src, dst, items, h, w);
            ELVIS_CHECK_LAUNCH("elvis_i420_to_rgb_u8");
            elvis_note_launch("i420_to_rgb_x16_kernel<bgr>");
        } else {
            hipLaunchKernelGGL(i420_to_rgb_x16_kernel<false>, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, src, dst, items, h, w);
            ELVIS_CHECK_LAUNCH("elvis_i420_to_rgb_u8");
            elvis_note_launch("i420_to_rgb_x16_kernel<rgb>");
        }
        return ELVIS_OK;
    }
    const int strips = (w + 7) / 8;
    const long long items = (long long)n * (h / 2) * strips;
    const long long blocks = (items + 255) / 256;
    ELVIS_REQUIRE(blocks <= 0x7fffffffLL, "elvis_i420_to_rgb_u8: n=%d h=%d w=%d is more than one launch holds", n, h, w);
    const int grid = (int)blocks;
    const int wide = w % 4 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 4 == 0;
    if (bgr) {
        hipLaunchKernelGGL(i420_to_rgb_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, dst, items, h, w, strips, wide);
        ELVIS_CHECK_LAUNCH("elvis_i420_to_rgb_u8");
        elvis_note_launch("i420_to_rgb_kernel<bgr>");
    } else {
        hipLaunchKernelGGL(i420_to_rgb_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, dst, items, h, w, strips, wide);
        ELVIS_CHECK_LAUNCH("elvis_i420_to_rgb_u8");
        elvis_note_launch("i420_to_rgb_kernel<rgb>");
    }
    return ELVIS_OK;
}
