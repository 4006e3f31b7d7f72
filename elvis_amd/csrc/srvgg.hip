// Real-ESRGAN's SRVGGNetCompact (the network behind `realesr-animevideov3` and `realesr-general-x4v3`, elvis.py:2431-2441,
// run by RealESRGANer.enhance, elvis.py:2515) on f16 NHWC tensors: the 64-channel 3x3 conv with a per-channel PReLU and
// the tail conv whose epilogue is the pixel shuffle, the nearest-4x base and the byte quantisation.  A translation unit
// of its own; nothing here touches rrdb.hip or conv*.hip.
//
// The design, and why.  Both kernels are one template, `srvgg_conv3x3_kernel<COUT, TAIL>`: 256 threads take an 8 x 32
// pixel tile times all COUT (64, or the tail's 48) on v_mfma_f32_16x16x32_f16; wave v owns rows 2v, 2v+1.  The weights
// are the A operand (rows = cout) and the pixels the B operand (columns), so a lane ends with 4 consecutive output
// channels of one pixel per accumulator.  That is what both epilogues want: the layer stores 8 bytes of f16 per
// accumulator with the four PReLU slopes in one 16-byte load; in the tail channel 16c + 4dy + dx of accumulator c is
// (colour c, dy = lane / 16, dx = register), so a lane holds all three colours of the four horizontally adjacent
// output pixels (4y + dy, 4x .. 4x + 3): 12 contiguous bytes, three 4-byte stores, and the 48-channel tensor never
// exists.  K runs in 32-channel chunks (one for the first layer's padded input, two elsewhere): per chunk the 10 x 34
// halo (21.8 KB) and the chunk's nine taps (36 KB, tail 27 KB) are staged in LDS once; the next chunk's global loads
// are issued before the MFMAs of the current one and land in LDS after them.  58 KB (tail 49 KB) of LDS: two
// workgroups per CU, so one workgroup's staging runs under the other's MFMAs.
//
// This is the tile, the LDS image and the swizzle of rrdb_conv3x3_kernel (rrdb.hip), kept on purpose: its fragment
// map and bank behaviour are measured and its edge matrix is known, and what this network needs that it lacks is all
// in the epilogue and in the 48-row weight image.  The plan the 72 KB weight set invites - the whole layer's weights
// resident in LDS, a persistent workgroup walking tiles and staging halos only - needs 72 + 43.5 KB for a two-chunk
// halo, one workgroup of four waves per CU, and then has nothing to run under its own halo loads unless the halo is
// double-buffered as well (159 KB, the whole LDS); it is not built here and nothing is claimed for it.  DESIGN.md 7.1
// has the measured times of this kernel.
//
// LDS images: rows of 64 bytes (one pixel or one (tap, cout) x 32 channels), four 16-byte slots; slot c of row p is
// stored at slot c ^ (2 * ((p >> 2) & 1)), as in rrdb.hip (conflict-free for the ds_read_b128 fragment reads of both
// operands; a weight fragment starts on a row that is a multiple of 16, for COUT = 48 too: tap * 48 + 16 nt).
#include "common.h"
#include <string.h>

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int SV_TY = 8, SV_TX = 32, SV_KC = 32;
constexpr int SV_HY = SV_TY + 2, SV_HX = SV_TX + 2;
constexpr int SV_HALO_UNITS = SV_HY * SV_HX * 4;             // 16-byte units of one chunk's halo
constexpr int SV_HALO_ITERS = (SV_HALO_UNITS + 255) / 256;   // 6
constexpr int SV_HALO_BYTES = SV_HY * SV_HX * 64;

__device__ __forceinline__ int sv_swz(int row, int c) { return row * 64 + ((c ^ ((row >> 1) & 2)) << 4); }

struct SrvggArgs {
    const half_t* x;
    const half_t* wp;
    const float* bias;
    const float* slope;
    const half_t* base;
    void* out;
    int x_pitch, out_pitch, base_pitch;
    int h, w, nkc, out_u8, swap_rb;
};

template <int COUT, bool TAIL>
__global__ __launch_bounds__(256) void srvgg_conv3x3_kernel(SrvggArgs a) {
    constexpr int W_UNITS = 9 * COUT * 4;                    // 16-byte units of one chunk's weights
    constexpr int W_ITERS = (W_UNITS + 255) / 256;
    constexpr int NT = COUT / 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[SV_HALO_BYTES + W_UNITS * 16];
    unsigned char* lds_w = lds + SV_HALO_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * SV_TX, ty0 = blockIdx.y * SV_TY, img = blockIdx.z;

    // the halo units this thread stages: source element offset (channel 0 of the chunk), or -1 for the zero border
    long long hsrc[SV_HALO_ITERS];
    int hdst[SV_HALO_ITERS];
#pragma unroll
    for (int i = 0; i < SV_HALO_ITERS; ++i) {
        const int u = tid + i * 256;
        hsrc[i] = -1;
        hdst[i] = -1;
        if (u < SV_HALO_UNITS) {
            const int pix = u >> 2, c = u & 3;
            const int hy = pix / SV_HX, hx = pix - hy * SV_HX;
            const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
            hdst[i] = sv_swz(pix, c);
            if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w)
                hsrc[i] = (((long long)img * a.h + gy) * a.w + gx) * a.x_pitch + c * 8;
        }
    }

    u32x4 hreg[SV_HALO_ITERS], wreg[W_ITERS];
    auto fetch = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < SV_HALO_ITERS; ++i) {
            hreg[i] = u32x4{0u, 0u, 0u, 0u};
            if (hsrc[i] >= 0) hreg[i] = *reinterpret_cast<const u32x4*>(a.x + hsrc[i] + kc * SV_KC);
        }
        const u32x4* wsrc = reinterpret_cast<const u32x4*>(a.wp) + (long long)kc * W_UNITS;
#pragma unroll
        for (int i = 0; i < W_ITERS; ++i) {
            const int u = tid + i * 256;
            if (W_UNITS % 256 == 0 || u < W_UNITS) wreg[i] = wsrc[u];
        }
    };
    auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < SV_HALO_ITERS; ++i)
            if (hdst[i] >= 0) *reinterpret_cast<u32x4*>(lds + hdst[i]) = hreg[i];
#pragma unroll
        for (int i = 0; i < W_ITERS; ++i) {
            const int u = tid + i * 256;
            if (W_UNITS % 256 == 0 || u < W_UNITS) *reinterpret_cast<u32x4*>(lds_w + sv_swz(u >> 2, u & 3)) = wreg[i];
        }
    };

    float4v acc[4][NT];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[t][nt] = float4v{0.f, 0.f, 0.f, 0.f};

    const int l15 = lane & 15, lg = lane >> 4;
    // weight rows of a fragment start on a multiple of 16, so the swizzle term depends on the lane alone
    const int a_lane = l15 * 64 + ((lg ^ ((l15 >> 1) & 2)) << 4);

    fetch(0);
    for (int kc = 0; kc < a.nkc; ++kc) {
        __syncthreads();                       // the previous chunk's fragment reads are done
        stage();
        __syncthreads();
        if (kc + 1 < a.nkc) fetch(kc + 1);     // in flight under the MFMAs below
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap - dy * 3;
            half8 fa[NT], fb[4];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                fa[nt] = *reinterpret_cast<const half8*>(lds_w + (tap * COUT + nt * 16) * 64 + a_lane);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int p = (wave * 2 + (t >> 1) + dy) * SV_HX + (t & 1) * 16 + l15 + dx;
                fb[t] = *reinterpret_cast<const half8*>(lds + sv_swz(p, lg));
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[nt], fb[t], acc[t][nt], 0, 0, 0);
        }
    }

    // epilogue: accumulator register j of (t, nt) is pixel (row 2*wave + t/2, column 16*(t%2) + lane%16), output
    // channel 16*nt + 4*(lane/16) + j
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int oy = ty0 + wave * 2 + (t >> 1), ox = tx0 + (t & 1) * 16 + l15;
        if (oy >= a.h || ox >= a.w) continue;
        const long long pix = ((long long)img * a.h + oy) * a.w + ox;
        if constexpr (!TAIL) {
            half_t* o = reinterpret_cast<half_t*>(a.out) + pix * a.out_pitch;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int co = nt * 16 + lg * 4;
                const float4v bv = *reinterpret_cast<const float4v*>(a.bias + co);
                const float4v sv = *reinterpret_cast<const float4v*>(a.slope + co);
                half4 r;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float z = acc[t][nt][j] + bv[j];
                    r[j] = (half_t)(z > 0.f ? z : sv[j] * z);
                }
                *reinterpret_cast<half4*>(o + co) = r;
            }
        } else {
            // pixel shuffle by 4: channel 16c + 4dy + dx is colour c at (4y + dy, 4x + dx); here c = nt, dy = lg, dx = j,
            // so this lane owns output row 4 oy + lg, columns 4 ox .. 4 ox + 3, all three colours
            float v[3][4], y[12];
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) {
                const float4v bv = *reinterpret_cast<const float4v*>(a.bias + nt * 16 + lg * 4);
                const float b0 = (float)a.base[pix * a.base_pitch + nt];    // nearest 4x of the stored input pixel
#pragma unroll
                for (int j = 0; j < 4; ++j) v[nt][j] = (acc[t][nt][j] + bv[j]) + b0;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {                                    // y: [dx][colour], the order in memory
                y[j * 3 + 0] = a.swap_rb ? v[2][j] : v[0][j];
                y[j * 3 + 1] = v[1][j];
                y[j * 3 + 2] = a.swap_rb ? v[0][j] : v[2][j];
            }
            const long long opix = (((long long)img * 4 * a.h + 4 * oy + lg) * 4 * a.w + 4 * ox);
            if (a.out_u8) {
                uint32_t q[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    uint32_t v = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const float f = fminf(fmaxf(y[k * 4 + b], 0.f), 1.f) * 255.f;
                        v |= (uint32_t)__float2int_rn(f) << (8 * b);          // half to even, as numpy's round
                    }
                    q[k] = v;
                }
                uint32_t* o = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(a.out) + opix * 3);
                o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
            } else {
                half4* o = reinterpret_cast<half4*>(reinterpret_cast<half_t*>(a.out) + opix * 3);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    half4 r;
#pragma unroll
                    for (int b = 0; b < 4; ++b) r[b] = (half_t)y[k * 4 + b];
                    o[k] = r;
                }
            }
        }
    }
}

// fp32 -> f16, round to nearest even, on the host (no device code, no compiler-specific host half type)
uint16_t sv_f32_to_f16(float f) {
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
        shift = -1 - e;
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
bool sv_ranges_meet(const void* p, long long bytes, const void* q, long long qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)qbytes && b < a + (uintptr_t)bytes;
}

}  // namespace

/* elvis.py:2431-2441 / 2515 */
extern "C" size_t elvis_srvgg_packed_weight_bytes(int cin, int cout) {
    if ((cin != 32 && cin != 64) || (cout != 48 && cout != 64)) return 0;
    return (size_t)9 * cin * cout * 2;
}

/* elvis.py:2431-2441 / 2515 */
extern "C" int elvis_srvgg_pack_weights(const float* w_oihw_host, int cin_real, int cout_real, int cin, int cout, void* packed_host) {
    ELVIS_REQUIRE(cin == 32 || cin == 64, "elvis_srvgg_pack_weights: cin=%d is not 32 or 64", cin);
    ELVIS_REQUIRE(cout == 48 || cout == 64, "elvis_srvgg_pack_weights: cout=%d is not 48 or 64", cout);
    ELVIS_REQUIRE(cin_real >= 1 && cin_real <= cin && cout_real >= 1 && cout_real <= cout,
                  "elvis_srvgg_pack_weights: real channels %d -> %d do not fit the padded %d -> %d", cin_real, cout_real, cin, cout);
    ELVIS_REQUIRE(w_oihw_host && packed_host, "elvis_srvgg_pack_weights: null pointer");
    uint16_t* p = static_cast<uint16_t*>(packed_host);
    // packed[kc][tap][co][ci % 32], kc = ci / 32, tap = ky * 3 + kx
    for (int kc = 0; kc < cin / SV_KC; ++kc)
        for (int tap = 0; tap < 9; ++tap)
            for (int co = 0; co < cout; ++co)
                for (int k = 0; k < SV_KC; ++k) {
                    const int ci = kc * SV_KC + k;
                    float v = 0.f;
                    if (ci < cin_real && co < cout_real) v = w_oihw_host[((size_t)co * cin_real + ci) * 9 + tap];
                    p[(((size_t)kc * 9 + tap) * cout + co) * SV_KC + k] = sv_f32_to_f16(v);
                }
    return ELVIS_OK;
}

/* elvis.py:2431-2441 / 2515 */
extern "C" int elvis_srvgg_conv3x3(const void* x, int x_pitch, const void* w_packed, const float* bias, const float* slope, void* out,
                                   int out_pitch, int n, int h, int w, int cin, elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 0 && h >= 0 && w >= 0, "elvis_srvgg_conv3x3: bad shape n=%d h=%d w=%d", n, h, w);
    ELVIS_REQUIRE(cin == 32 || cin == 64, "elvis_srvgg_conv3x3: cin=%d is not 32 or 64", cin);
    ELVIS_REQUIRE(x_pitch >= cin && x_pitch % 8 == 0, "elvis_srvgg_conv3x3: x_pitch=%d must be a multiple of 8 and at least cin=%d", x_pitch, cin);
    ELVIS_REQUIRE(out_pitch >= 64 && out_pitch % 8 == 0, "elvis_srvgg_conv3x3: out_pitch=%d must be a multiple of 8 and at least 64", out_pitch);
    ELVIS_REQUIRE(h <= (1 << 29) && w <= (1 << 29), "elvis_srvgg_conv3x3: h=%d w=%d too large", h, w);
    if (n == 0 || h == 0 || w == 0) return ELVIS_OK;
    ELVIS_REQUIRE(x && w_packed && bias && slope && out, "elvis_srvgg_conv3x3: null pointer");
    ELVIS_REQUIRE(((uintptr_t)x | (uintptr_t)w_packed | (uintptr_t)bias | (uintptr_t)slope) % 16 == 0 && (uintptr_t)out % 8 == 0,
                  "elvis_srvgg_conv3x3: x, weights, bias and slopes are 16-byte aligned, out 8");
    const long long px = (long long)n * h * w;
    ELVIS_REQUIRE(!sv_ranges_meet(x, px * x_pitch * 2, out, px * out_pitch * 2),
                  "elvis_srvgg_conv3x3: out overlaps x (a tile reads its neighbours' pixels: the layers ping-pong two buffers)");
    const int tiles_x = cdiv(w, SV_TX), tiles_y = cdiv(h, SV_TY);
    ELVIS_REQUIRE(n <= 65535 && tiles_y <= 65535, "elvis_srvgg_conv3x3: n=%d h=%d is more than one launch holds", n, h);
    SrvggArgs a;
    a.x = static_cast<const half_t*>(x);
    a.wp = static_cast<const half_t*>(w_packed);
    a.bias = bias;
    a.slope = slope;
    a.base = nullptr;
    a.out = out;
    a.x_pitch = x_pitch; a.out_pitch = out_pitch; a.base_pitch = 0;
    a.h = h; a.w = w; a.nkc = cin / SV_KC; a.out_u8 = 0; a.swap_rb = 0;
    hipLaunchKernelGGL((srvgg_conv3x3_kernel<64, false>), dim3(tiles_x, tiles_y, n), dim3(256), 0, (hipStream_t)stream, a);
    ELVIS_CHECK_LAUNCH("elvis_srvgg_conv3x3");
    elvis_note_launch("srvgg_conv3x3_kernel<64,prelu>");
    return ELVIS_OK;
}

/* elvis.py:2431-2441 / 2515 */
extern "C" int elvis_srvgg_tail(const void* x, int x_pitch, const void* w_packed, const float* bias, const void* base, int base_pitch,
                                void* out, int n, int h, int w, int out_u8, int swap_rb, elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 0 && h >= 0 && w >= 0, "elvis_srvgg_tail: bad shape n=%d h=%d w=%d", n, h, w);
    ELVIS_REQUIRE(x_pitch >= 64 && x_pitch % 8 == 0, "elvis_srvgg_tail: x_pitch=%d must be a multiple of 8 and at least 64", x_pitch);
    ELVIS_REQUIRE(base_pitch >= 3, "elvis_srvgg_tail: base_pitch=%d must be at least 3", base_pitch);
    ELVIS_REQUIRE(h <= (1 << 27) && w <= (1 << 27), "elvis_srvgg_tail: h=%d w=%d too large", h, w);
    if (n == 0 || h == 0 || w == 0) return ELVIS_OK;
    ELVIS_REQUIRE(x && w_packed && bias && base && out, "elvis_srvgg_tail: null pointer");
    ELVIS_REQUIRE(((uintptr_t)x | (uintptr_t)w_packed | (uintptr_t)bias) % 16 == 0 && (uintptr_t)base % 2 == 0 &&
                  (uintptr_t)out % (out_u8 ? 4 : 8) == 0,
                  "elvis_srvgg_tail: x, weights and bias are 16-byte aligned, base 2, out 4 (u8) or 8 (f16)");
    const long long px = (long long)n * h * w;
    const long long out_bytes = px * 16 * 3 * (out_u8 ? 1 : 2);
    ELVIS_REQUIRE(!sv_ranges_meet(x, px * x_pitch * 2, out, out_bytes), "elvis_srvgg_tail: out overlaps x");
    ELVIS_REQUIRE(!sv_ranges_meet(base, px * base_pitch * 2, out, out_bytes), "elvis_srvgg_tail: out overlaps base");
    const int tiles_x = cdiv(w, SV_TX), tiles_y = cdiv(h, SV_TY);
    ELVIS_REQUIRE(n <= 65535 && tiles_y <= 65535, "elvis_srvgg_tail: n=%d h=%d is more than one launch holds", n, h);
    SrvggArgs a;
    a.x = static_cast<const half_t*>(x);
    a.wp = static_cast<const half_t*>(w_packed);
    a.bias = bias;
    a.slope = nullptr;
    a.base = static_cast<const half_t*>(base);
    a.out = out;
    a.x_pitch = x_pitch; a.out_pitch = 3; a.base_pitch = base_pitch;
    a.h = h; a.w = w; a.nkc = 2; a.out_u8 = out_u8 ? 1 : 0; a.swap_rb = swap_rb ? 1 : 0;
    hipLaunchKernelGGL((srvgg_conv3x3_kernel<48, true>), dim3(tiles_x, tiles_y, n), dim3(256), 0, (hipStream_t)stream, a);
    ELVIS_CHECK_LAUNCH("elvis_srvgg_tail");
    elvis_note_launch(out_u8 ? "srvgg_conv3x3_kernel<48,shuffle_u8>" : "srvgg_conv3x3_kernel<48,shuffle_f16>");
    return ELVIS_OK;
}
