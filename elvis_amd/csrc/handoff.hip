// Encoder hand-off: packed 8-bit RGB (or BGR) frames to planar I420, what the reference does per frame on the host with
// cv2.cvtColor(frame, COLOR_RGB2YUV_I420) before it feeds Kvazaar, SVT-AV1 and VMAF (utils.py:453-462, presley.py:217-223,
// presley.py:590-599).  Integer arithmetic only (OpenCV 4.x RGB8toYUV420pInvoker, 20-bit fixed point); memory-bound:
// 6 bytes read and 3 written per 2x1 pixels, no LDS, no atomics.
#include "common.h"
#include "i420.h"

// One lane per strip of 2 rows x 8 pixels; consecutive lanes take consecutive strips of a row pair, then the next row
// pair, then the next frame, so a wave's loads and stores are contiguous.  WIDE (w % 4 == 0, src and dst 4-byte aligned)
// makes every row and every full strip start on a dword: a full strip is 6 dwords per row in, 2 dwords of Y per row and
// 4 bytes each of U and V out.  U and V rows start on a dword only where w % 8 == 0 (a chroma row is w / 2 bytes), so
// their 4 bytes go out as one dword when the address allows it and as bytes otherwise.  The last strip of a width that
// is no multiple of 8, and every strip without WIDE, goes quad by quad in bytes; a strip never touches a byte past its
// own `cnt` pixels.  U and V come from the pixel at the even row and even column of a quad: OpenCV does not average.
template <bool BGR>
__global__ __launch_bounds__(256) void rgb_to_i420_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          long long items, int h, int w, int strips, int wide) {
    const int h2 = h / 2, w2 = w / 2;
    const long long frame_out = (long long)h2 * 3 * w;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < items) {
        const int s = (int)(i % strips);
        const long long t = i / strips;
        const int rp = (int)(t % h2);
        const long long f = t / h2;
        const int x = s * 8;
        const int cnt = min(8, w - x);                                  // even: w is
        const uint8_t* p0 = src + ((f * h + 2 * rp) * w + x) * 3;
        const uint8_t* p1 = p0 + (long long)w * 3;
        uint8_t* y0 = dst + f * frame_out + (long long)(2 * rp) * w + x;
        uint8_t* y1 = y0 + w;
        uint8_t* pu = dst + f * frame_out + (long long)h * w + (long long)rp * w2 + x / 2;
        uint8_t* pv = pu + (long long)h2 * w2;
        if (wide && cnt == 8) {
            union { uint32_t d[6]; uint8_t b[24]; } a0, a1;
            union { uint32_t d[2]; uint8_t b[8]; } o0, o1;
            union { uint32_t d; uint8_t b[4]; } ou, ov;
            const uint32_t* q0 = reinterpret_cast<const uint32_t*>(p0);
            const uint32_t* q1 = reinterpret_cast<const uint32_t*>(p1);
#pragma unroll
            for (int k = 0; k < 6; ++k) { a0.d[k] = q0[k]; a1.d[k] = q1[k]; }
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int r0 = a0.b[3 * p + (BGR ? 2 : 0)], g0 = a0.b[3 * p + 1], b0 = a0.b[3 * p + (BGR ? 0 : 2)];
                const int r1 = a1.b[3 * p + (BGR ? 2 : 0)], g1 = a1.b[3 * p + 1], b1 = a1.b[3 * p + (BGR ? 0 : 2)];
                o0.b[p] = i420_y(r0, g0, b0);
                o1.b[p] = i420_y(r1, g1, b1);
                if ((p & 1) == 0) {
                    ou.b[p / 2] = i420_u(r0, g0, b0);
                    ov.b[p / 2] = i420_v(r0, g0, b0);
                }
            }
            uint32_t* s0 = reinterpret_cast<uint32_t*>(y0);
            uint32_t* s1 = reinterpret_cast<uint32_t*>(y1);
            s0[0] = o0.d[0]; s0[1] = o0.d[1];
            s1[0] = o1.d[0]; s1[1] = o1.d[1];
            if (((uintptr_t)pu & 3) == 0) {
                *reinterpret_cast<uint32_t*>(pu) = ou.d;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) pu[k] = ou.b[k];
            }
            if (((uintptr_t)pv & 3) == 0) {
                *reinterpret_cast<uint32_t*>(pv) = ov.d;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) pv[k] = ov.b[k];
            }
        } else {
            for (int p = 0; p < cnt; p += 2) {
                const int r00 = p0[3 * p + (BGR ? 2 : 0)], g00 = p0[3 * p + 1], b00 = p0[3 * p + (BGR ? 0 : 2)];
                const int r01 = p0[3 * p + 3 + (BGR ? 2 : 0)], g01 = p0[3 * p + 4], b01 = p0[3 * p + 3 + (BGR ? 0 : 2)];
                const int r10 = p1[3 * p + (BGR ? 2 : 0)], g10 = p1[3 * p + 1], b10 = p1[3 * p + (BGR ? 0 : 2)];
                const int r11 = p1[3 * p + 3 + (BGR ? 2 : 0)], g11 = p1[3 * p + 4], b11 = p1[3 * p + 3 + (BGR ? 0 : 2)];
                y0[p] = i420_y(r00, g00, b00);
                y0[p + 1] = i420_y(r01, g01, b01);
                y1[p] = i420_y(r10, g10, b10);
                y1[p + 1] = i420_y(r11, g11, b11);
                pu[p / 2] = i420_u(r00, g00, b00);
                pv[p / 2] = i420_v(r00, g00, b00);
            }
        }
    }
}

extern "C" int elvis_rgb_to_i420_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int bgr, elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 0 && h >= 0 && w >= 0, "elvis_rgb_to_i420_u8: bad shape n=%d h=%d w=%d", n, h, w);
    ELVIS_REQUIRE(h % 2 == 0 && w % 2 == 0, "elvis_rgb_to_i420_u8: I420 needs an even height and width, got h=%d w=%d", h, w);
    if (n == 0 || h == 0 || w == 0) return ELVIS_OK;
    ELVIS_REQUIRE(src && dst, "elvis_rgb_to_i420_u8: null pointer");
    const int strips = (w + 7) / 8;
    const long long items = (long long)n * (h / 2) * strips;
    const long long blocks = (items + 255) / 256;
    ELVIS_REQUIRE(blocks <= 0x7fffffffLL, "elvis_rgb_to_i420_u8: n=%d h=%d w=%d is more than one launch holds", n, h, w);
    const int grid = (int)blocks;
    const int wide = w % 4 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 4 == 0;
    if (bgr) {
        hipLaunchKernelGGL(rgb_to_i420_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, dst, items, h, w, strips, wide);
        ELVIS_CHECK_LAUNCH("elvis_rgb_to_i420_u8");
        elvis_note_launch("rgb_to_i420_kernel<bgr>");
    } else {
        hipLaunchKernelGGL(rgb_to_i420_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, dst, items, h, w, strips, wide);
        ELVIS_CHECK_LAUNCH("elvis_rgb_to_i420_u8");
        elvis_note_launch("rgb_to_i420_kernel<rgb>");
    }
    return ELVIS_OK;
}
