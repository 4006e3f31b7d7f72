// Real-ESRGAN's SRVGGNetCompact (the network behind `realesr-animevideov3` and `realesr-general-x4v3`, elvis.py:2431-2441,
// run by RealESRGANer.enhance, elvis.py:2515) on f16 NHWC tensors: the 64-channel 3x3 conv with a per-channel PReLU and
// the tail conv whose epilogue is the pixel shuffle, the nearest-4x base and the byte quantisation.  A translation unit
// of its own; nothing here touches rrdb.hip or conv*.hip.
//
// The design, and why.  Both kernels are one template, `srvgg_conv3x3_kernel<COUT, TAIL>`, on the 3x3 MFMA tile of
// sr_conv3x3.h (its LDS images, swizzle and fragment map are stated there) with COUT = 64, or the tail's 48.  A lane
// ends with 4 consecutive output channels of one pixel per accumulator.  That is what both epilogues want: the layer
// stores 8 bytes of f16 per accumulator with the four PReLU slopes in one 16-byte load; in the tail channel
// 16c + 4dy + dx of accumulator c is (colour c, dy = lane / 16, dx = register), so a lane holds all three colours of
// the four horizontally adjacent output pixels (4y + dy, 4x .. 4x + 3): 12 contiguous bytes, three 4-byte stores, and
// the 48-channel tensor never exists.  K runs in 32-channel chunks (one for the first layer's padded input, two
// elsewhere).  58 KB (tail 49 KB) of LDS: two workgroups per CU, so one workgroup's staging runs under the other's MFMAs.
//
// The plan the 72 KB weight set invites - the whole layer's weights resident in LDS, a persistent workgroup walking
// tiles and staging halos only - needs 72 + 43.5 KB for a two-chunk halo, one workgroup of four waves per CU, and then
// has nothing to run under its own halo loads unless the halo is double-buffered as well (159 KB, the whole LDS); it is
// not built here and nothing is claimed for it.  DESIGN.md 7.1 has the measured times of this kernel.
#include "sr_conv3x3.h"

namespace {

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
    constexpr int NT = COUT / 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[SR_LDS_BYTES<COUT>];
    float4v acc[4][NT];
    sr_conv3x3_tile<COUT>(a.x, a.x_pitch, a.wp, a.h, a.w, a.h, a.w, 0, a.nkc, lds, acc);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
    const int tx0 = blockIdx.x * SR_TX, ty0 = blockIdx.y * SR_TY, img = blockIdx.z;
    // epilogue, on the fragment map of sr_conv3x3_tile
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
    sr_pack_weights(w_oihw_host, cin_real, cout_real, cin, cout, static_cast<uint16_t*>(packed_host));
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
    ELVIS_REQUIRE(!sr_ranges_meet(x, px * x_pitch * 2, out, px * out_pitch * 2),
                  "elvis_srvgg_conv3x3: out overlaps x (a tile reads its neighbours' pixels: the layers ping-pong two buffers)");
    const int tiles_x = cdiv(w, SR_TX), tiles_y = cdiv(h, SR_TY);
    ELVIS_REQUIRE(n <= 65535 && tiles_y <= 65535, "elvis_srvgg_conv3x3: n=%d h=%d is more than one launch holds", n, h);
    SrvggArgs a;
    a.x = static_cast<const half_t*>(x);
    a.wp = static_cast<const half_t*>(w_packed);
    a.bias = bias;
    a.slope = slope;
    a.base = nullptr;
    a.out = out;
    a.x_pitch = x_pitch; a.out_pitch = out_pitch; a.base_pitch = 0;
    a.h = h; a.w = w; a.nkc = cin / SR_KC; a.out_u8 = 0; a.swap_rb = 0;
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
    ELVIS_REQUIRE(!sr_ranges_meet(x, px * x_pitch * 2, out, out_bytes), "elvis_srvgg_tail: out overlaps x");
    ELVIS_REQUIRE(!sr_ranges_meet(base, px * base_pitch * 2, out, out_bytes), "elvis_srvgg_tail: out overlaps base");
    const int tiles_x = cdiv(w, SR_TX), tiles_y = cdiv(h, SR_TY);
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
