// Device helpers shared by the per-block u8 kernels of degrade.hip and presley_degrade.hip: OpenCV's INTER_LINEAR rule on
// u8 (one definition for elvis.py's and Presley's downscale-and-back degraders) and BORDER_REFLECT_101.
#pragma once
#include "common.h"

static __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static __device__ __forceinline__ int reflect101(int i, int n) {   // BORDER_REFLECT_101: -1 -> 1, n -> n-2 (n == 1: 0)
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
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
