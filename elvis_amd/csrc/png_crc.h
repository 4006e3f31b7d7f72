// The chunk CRC-32 of the PNG writer (csrc/png.hip) and reader (csrc/png_read.hip): one copy.  A workgroup of kPngThreads
// threads takes one run of bytes; every lane runs the byte-table CRC over a slice and the slices are combined with
// x^(8 len) mod P.
#pragma once
#include "common.h"

namespace {

constexpr int kPngThreads = 256;
constexpr int kPngWaves = kPngThreads / ELVIS_WAVE;
constexpr uint32_t kCrcPoly = 0xEDB88320u;

struct PngX2n {
    uint32_t v[32];   // x^(2^k) mod P, reflected
};

__host__ __device__ __forceinline__ uint32_t png_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}

// fills the byte table tab[256] (LDS); the caller synchronises before png_crc_workgroup
__device__ __forceinline__ void png_crc_table(uint32_t* tab) {
    uint32_t e = (uint32_t)threadIdx.x;
#pragma unroll
    for (int k = 0; k < 8; ++k) e = (e >> 1) ^ ((e & 1u) ? kCrcPoly : 0u);
    tab[threadIdx.x] = e;
}

// CRC-32 of p[0, len), valid in thread 0.  Lane t runs the byte-table CRC over slice t (the first from the register
// 0xFFFFFFFF, the others from 0); a slice's register times x^(8 * bytes behind it) mod P is its share of the final
// register, and the shares XOR together.  wred[kPngWaves] is LDS.
__device__ __forceinline__ uint32_t png_crc_workgroup(const uint8_t* p, long long len, const PngX2n& x2n, const uint32_t* tab, uint32_t* wred) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m = (len + kPngThreads - 1) / kPngThreads;
    const long long s0 = min(len, (long long)tid * m), s1 = min(len, s0 + m);
    uint32_t s = tid == 0 ? 0xFFFFFFFFu : 0u;
    for (long long i = s0; i < s1; ++i) s = tab[(s ^ p[i]) & 255u] ^ (s >> 8);
    if (s0 < s1) {
        unsigned long long behind = (unsigned long long)(len - s1);
        uint32_t xp = 0x80000000u;   // x^0
        for (int k = 3; behind; behind >>= 1, ++k)
            if (behind & 1ull) xp = png_mulmod(x2n.v[k & 31], xp);
        s = png_mulmod(xp, s);
    } else {
        s = 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s ^= __shfl_xor(s, o, 64);
    if (lane == 0) wred[wave] = s;
    __syncthreads();
    uint32_t crc = 0xFFFFFFFFu;
    for (int w = 0; w < kPngWaves; ++w) crc ^= wred[w];
    return crc;
}

inline PngX2n png_x2n_table() {
    PngX2n t;
    uint32_t p = 0x40000000u;   // x^1
    for (int k = 0; k < 32; ++k) {
        t.v[k] = p;
        p = png_mulmod(p, p);
    }
    return t;
}

}  // namespace
