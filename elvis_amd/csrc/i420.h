// The 20-bit fixed-point RGB -> Y'CbCr of OpenCV 4.x's RGB8toYUV420pInvoker, one statement for every kernel that needs it:
// the I420 hand-off (handoff.hip) and the luma the block-complexity analyser reads (complexity.hip).
#pragma once
#include <stdint.h>

#define I420_SHIFT 20
#define I420_HALF (1 << (I420_SHIFT - 1))

// 900726 * 255 + (1 << 19) + (16 << 20) = 247 510 922 and 460324 * 255 + (1 << 19) + (128 << 20) = 252 124 636 are the
// largest sums, 128 << 20 less 460323 * 255 the smallest: int32 holds them all, every sum is positive and every result
// lies in [16, 240] - saturate_cast has nothing to do.
__device__ __forceinline__ uint8_t i420_y(int r, int g, int b) {
    return (uint8_t)((269484 * r + 528482 * g + 102760 * b + I420_HALF + (16 << I420_SHIFT)) >> I420_SHIFT);
}
__device__ __forceinline__ uint8_t i420_u(int r, int g, int b) {
    return (uint8_t)((-155188 * r - 305135 * g + 460324 * b + I420_HALF + (128 << I420_SHIFT)) >> I420_SHIFT);
}
__device__ __forceinline__ uint8_t i420_v(int r, int g, int b) {
    return (uint8_t)((460324 * r - 385875 * g - 74448 * b + I420_HALF + (128 << I420_SHIFT)) >> I420_SHIFT);
}
