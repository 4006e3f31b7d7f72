// The 3x3 MFMA conv tile of the Real-ESRGAN networks, shared by rrdb.hip (RRDBNet) and srvgg.hip (SRVGGNetCompact), and
// the host-side weight packing that feeds it.  Included by those two units only; everything here is static or inline.
//
// 3x3 / stride 1 / pad 1, f16 in, fp32 accumulate on v_mfma_f32_16x16x32_f16.  256 threads take an 8 x 32 pixel tile
// times all COUT (32, 48 or 64); wave v owns rows 2v, 2v+1.  The weights are the A operand (rows = cout) and the pixels
// the B operand (columns), so a lane ends with 4 consecutive output channels of one pixel per accumulator.  Per
// 32-channel K chunk the 10 x 34 halo (21.8 KB) and the chunk's nine taps (18 / 27 / 36 KB) are staged in LDS once; the
// next chunk's global loads are issued before the MFMAs of the current one and land in LDS after them.
//
// LDS images: rows of 64 bytes (one pixel or one (tap, cout) x 32 channels), four 16-byte slots; slot c of row p is
// stored at slot c ^ (2 * ((p >> 2) & 1)).  A ds_read_b128 is served in four groups of 16 lanes ({0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same + 32); a fragment read has lane l at row base + l % 16, slot l / 16, and with this
// XOR the 16 lanes of every group fall on 16 different slots of the 256-byte bank row for every base (checked by
// enumeration; c ^ ((p >> 2) & 3) and the plain image are both 2-way).  A weight fragment starts on a row that is a
// multiple of 16, for COUT = 48 too: tap * 48 + 16 nt.
#pragma once
#include "common.h"
#include <string.h>

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int SR_TY = 8, SR_TX = 32, SR_KC = 32;
constexpr int SR_HY = SR_TY + 2, SR_HX = SR_TX + 2;
constexpr int SR_HALO_UNITS = SR_HY * SR_HX * 4;             // 16-byte units of one chunk's halo
constexpr int SR_HALO_ITERS = (SR_HALO_UNITS + 255) / 256;   // 6
constexpr int SR_HALO_BYTES = SR_HY * SR_HX * 64;
// bytes of the workgroup's LDS block: the halo image, then one chunk's weights
template <int COUT> constexpr int SR_LDS_BYTES = SR_HALO_BYTES + 9 * COUT * 64;

__device__ __forceinline__ int sr_swz(int row, int c) { return row * 64 + ((c ^ ((row >> 1) & 2)) << 4); }

// The tile body, from the halo table to the end of the K loop: fills `acc` with the conv (no bias) of the workgroup's
// tile (blockIdx.x, blockIdx.y) of image blockIdx.z.  `x` is [n,h,w,x_pitch] with nkc * 32 channels read, `wp` the
// packed weights (sr_pack_weights), `lds` the workgroup's block of SR_LDS_BYTES<COUT>.  The conv runs over the ho x wo
// grid whose pixel (y, x) is input pixel (y >> ups, x >> ups): ups = 0 with ho = h, wo = w, or a nearest-2x upsample
// folded into the halo fetch.
//
// Fragment map, the contract of the epilogues: register j of (t, nt) is pixel (row 2*wave + t/2, column 16*(t%2) +
// lane%16), channel 16*nt + 4*(lane/16) + j.
template <int COUT>
__device__ __forceinline__ void sr_conv3x3_tile(const half_t* x, int x_pitch, const half_t* wp, int h, int w, int ho, int wo,
                                                int ups, int nkc, unsigned char* lds, float4v (&acc)[4][COUT / 16]) {
    constexpr int W_UNITS = 9 * COUT * 4;                    // 16-byte units of one chunk's weights
    constexpr int W_ITERS = (W_UNITS + 255) / 256;
    constexpr int NT = COUT / 16;
    unsigned char* lds_w = lds + SR_HALO_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * SR_TX, ty0 = blockIdx.y * SR_TY, img = blockIdx.z;

    // the halo units this thread stages: source element offset (channel 0 of the chunk), or -1 for the zero border
    long long hsrc[SR_HALO_ITERS];
    int hdst[SR_HALO_ITERS];
#pragma unroll
    for (int i = 0; i < SR_HALO_ITERS; ++i) {
        const int u = tid + i * 256;
        hsrc[i] = -1;
        hdst[i] = -1;
        if (u < SR_HALO_UNITS) {
            const int pix = u >> 2, c = u & 3;
            const int hy = pix / SR_HX, hx = pix - hy * SR_HX;
            const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
            hdst[i] = sr_swz(pix, c);
            if (gy >= 0 && gy < ho && gx >= 0 && gx < wo) {
                const int sy = gy >> ups, sx = gx >> ups;
                hsrc[i] = (((long long)img * h + sy) * w + sx) * x_pitch + c * 8;
            }
        }
    }

    u32x4 hreg[SR_HALO_ITERS], wreg[W_ITERS];
    auto fetch = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < SR_HALO_ITERS; ++i) {
            hreg[i] = u32x4{0u, 0u, 0u, 0u};
            if (hsrc[i] >= 0) hreg[i] = *reinterpret_cast<const u32x4*>(x + hsrc[i] + kc * SR_KC);
        }
        const u32x4* wsrc = reinterpret_cast<const u32x4*>(wp) + (long long)kc * W_UNITS;
#pragma unroll
        for (int i = 0; i < W_ITERS; ++i) {
            const int u = tid + i * 256;
            if (W_UNITS % 256 == 0 || u < W_UNITS) wreg[i] = wsrc[u];
        }
    };
    auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < SR_HALO_ITERS; ++i)
            if (hdst[i] >= 0) *reinterpret_cast<u32x4*>(lds + hdst[i]) = hreg[i];
#pragma unroll
        for (int i = 0; i < W_ITERS; ++i) {
            const int u = tid + i * 256;
            if (W_UNITS % 256 == 0 || u < W_UNITS) *reinterpret_cast<u32x4*>(lds_w + sr_swz(u >> 2, u & 3)) = wreg[i];
        }
    };

#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[t][nt] = float4v{0.f, 0.f, 0.f, 0.f};

    const int l15 = lane & 15, lg = lane >> 4;
    // weight rows of a fragment start on a multiple of 16, so the swizzle term depends on the lane alone
    const int a_lane = l15 * 64 + ((lg ^ ((l15 >> 1) & 2)) << 4);

    fetch(0);
    for (int kc = 0; kc < nkc; ++kc) {
        __syncthreads();                       // the previous chunk's fragment reads are done
        stage();
        __syncthreads();
        if (kc + 1 < nkc) fetch(kc + 1);       // in flight under the MFMAs below
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap - dy * 3;
            half8 fa[NT], fb[4];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                fa[nt] = *reinterpret_cast<const half8*>(lds_w + (tap * COUT + nt * 16) * 64 + a_lane);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int p = (wave * 2 + (t >> 1) + dy) * SR_HX + (t & 1) * 16 + l15 + dx;
                fb[t] = *reinterpret_cast<const half8*>(lds + sr_swz(p, lg));
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[nt], fb[t], acc[t][nt], 0, 0, 0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

// fp32 -> f16, round to nearest even, on the host (no device code, no compiler-specific host half type)
static inline uint16_t sr_f32_to_f16(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    const uint32_t mag = x & 0x7fffffffu;
    if (mag >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (mag > 0x7f800000u ? 0x200u : 0u));   // inf, nan
    if (mag >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                                       // rounds to inf
    if (mag < 0x33000001u) return (uint16_t)sign;                                                    // <= 2^-25: zero
    const int e = (int)(mag >> 23) - 127;
    uint32_t man = (mag & 0x7fffffu) | 0x800000u;
    int shift;
    uint32_t base;
    if (e < -14) {            // subnormal: value = man * 2^(e-23), unit 2^-24
        shift = -1 - e;       // 13 + (-14 - e)
        base = 0;
    } else {
        shift = 13;
        base = (uint32_t)(e + 15) << 10;
        man &= 0x7fffffu;
    }
    uint32_t q = man >> shift;
    const uint32_t rem = man & ((1u << shift) - 1u), mid = 1u << (shift - 1);
    if (rem > mid || (rem == mid && (q & 1u))) ++q;
    return (uint16_t)(sign | (base + q));   // a mantissa carry moves into the exponent, as it should
}

// do the byte ranges [p, p + bytes) and [q, q + qbytes) meet
static inline bool sr_ranges_meet(const void* p, long long bytes, const void* q, long long qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)qbytes && b < a + (uintptr_t)bytes;
}

// w[cout_real][cin_real][3][3] fp32 -> packed[kc][tap][co][ci % 32] f16, kc = ci / 32, tap = ky * 3 + kx, the channels
// past the real ones zero.  The callers have checked the arguments.
static inline void sr_pack_weights(const float* w, int cin_real, int cout_real, int cin, int cout, uint16_t* packed) {
    for (int kc = 0; kc < cin / SR_KC; ++kc)
        for (int tap = 0; tap < 9; ++tap)
            for (int co = 0; co < cout; ++co)
                for (int k = 0; k < SR_KC; ++k) {
                    const int ci = kc * SR_KC + k;
                    float v = 0.f;
                    if (ci < cin_real && co < cout_real) v = w[((size_t)co * cin_real + ci) * 9 + tap];
                    packed[(((size_t)kc * 9 + tap) * cout + co) * SR_KC + k] = sr_f32_to_f16(v);
                }
}
