// The 20-bit fixed-point RGB -> Y'CbCr of OpenCV 4.x's RGB8toYUV420pInvoker, one statement for every kernel that needs it:
// the I420 hand-off (handoff.hip) and the luma the block-complexity analyser reads (complexity.hip) - and its inverse,
// OpenCV 4.x's YUV420p2RGB8Invoker, for the decoder hand-off (i420_in.hip).
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

// The way back.  yy = max(0, Y - 16) * 1220542 is at most 239 * 1220542 = 291 709 538; with u, v in [-128, 127] the
// largest sum is yy + (1 << 19) + 2116026 * 127 = 560 969 128 (B) and the smallest (1 << 19) - 852492 * 127 - 409993 * 127
// = -159 811 307 (G): int32 holds them all.  sat8(sum >> 20) with an arithmetic shift - a negative sum floors, then
// saturates to 0 - is written as clamp-then-shift: the sum clamped to [0, 2^28 - 1], then shifted, which is the same value
// for every int.  In the shift-then-clamp form hipcc (ROCm 7) pairs two channels into one v_ashr_pk_u8_i32 and ORs the
// result into a dword as if its upper half were zero; on the MI355X it is not, and bytes 2 and 3 of every packed dword
// came out ORed with stray bits (the dword strips of tests/test_gpu_i420_in.py caught it; the byte path never packs).
__device__ __forceinline__ int i420_luma_term(int y) { return max(0, y - 16) * 1220542 + I420_HALF; }
__device__ __forceinline__ uint8_t i420_sat8_shift(int sum) {
    return (uint8_t)((unsigned)min((256 << I420_SHIFT) - 1, max(0, sum)) >> I420_SHIFT);
}
// u and v are the chroma bytes less 128
__device__ __forceinline__ uint8_t i420_to_r(int yy, int u, int v) { return i420_sat8_shift(yy + 1673527 * v); }
__device__ __forceinline__ uint8_t i420_to_g(int yy, int u, int v) { return i420_sat8_shift(yy - 852492 * v - 409993 * u); }
__device__ __forceinline__ uint8_t i420_to_b(int yy, int u, int v) { return i420_sat8_shift(yy + 2116026 * u); }
