// Real-ESRGAN's RRDBNet (the network RealESRGANer.enhance runs, elvis.py:2515) on f16 NHWC tensors: the dense-block
// 3x3 conv and the uint8 input stage.  A translation unit of its own; nothing here touches conv*.hip.
//
// elvis_rrdb_conv3x3: the 3x3 MFMA tile of sr_conv3x3.h (its LDS images, swizzle and fragment map are stated there) with
// 32 or 64 output channels written at a channel offset of a wider buffer, so that a dense block appends x1..x4 to its
// own input and no concat ever runs; a lane ends with 4 consecutive output channels of one pixel per accumulator: one
// 8-byte store.  40 / 58 KB of LDS and 172 / 232 registers per lane: two workgroups per CU.
#include "sr_conv3x3.h"

namespace {

struct RrdbArgs {
    const half_t* x;
    const half_t* wp;
    const float* bias;
    void* out;
    const half_t* r1;
    const half_t* r2;
    int x_pitch, out_pitch, out_coff, r1_pitch, r2_pitch;
    int h, w, ho, wo, nkc, ups, lrelu, out_u8, swap_rb;
    float s0, s1;
};

template <int COUT>
__global__ __launch_bounds__(256) void rrdb_conv3x3_kernel(RrdbArgs a) {
    constexpr int NT = COUT / 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[SR_LDS_BYTES<COUT>];
    float4v acc[4][NT];
    sr_conv3x3_tile<COUT>(a.x, a.x_pitch, a.wp, a.h, a.w, a.ho, a.wo, a.ups, a.nkc, lds, acc);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
    const int tx0 = blockIdx.x * SR_TX, ty0 = blockIdx.y * SR_TY, img = blockIdx.z;
    // epilogue, on the fragment map of sr_conv3x3_tile
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int oy = ty0 + wave * 2 + (t >> 1), ox = tx0 + (t & 1) * 16 + l15;
        if (oy >= a.ho || ox >= a.wo) continue;
        const long long pix = ((long long)img * a.ho + oy) * a.wo + ox;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int co = nt * 16 + lg * 4;
            const float4v bv = *reinterpret_cast<const float4v*>(a.bias + co);
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v = acc[t][nt][j] + bv[j];
                if (a.lrelu) v = v > 0.f ? v : 0.2f * v;
                y[j] = a.s0 * v;
            }
            if (a.r1) {
                const half4 r = *reinterpret_cast<const half4*>(a.r1 + pix * a.r1_pitch + co);
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = y[j] + a.s1 * (float)r[j];
            }
            if (a.r2) {
                const half4 r = *reinterpret_cast<const half4*>(a.r2 + pix * a.r2_pitch + co);
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = y[j] + (float)r[j];
            }
            if (a.out_u8) {
                if (co == 0) {                                   // the three real channels: one lane group, nt == 0
                    uint8_t* o = reinterpret_cast<uint8_t*>(a.out) + pix * 3;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float q = fminf(fmaxf(y[j], 0.f), 1.f) * 255.f;
                        o[a.swap_rb ? 2 - j : j] = (uint8_t)__float2int_rn(q);   // half to even, as numpy's round
                    }
                }
            } else {
                half4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (half_t)y[j];
                *reinterpret_cast<half4*>(reinterpret_cast<half_t*>(a.out) + pix * a.out_pitch + a.out_coff + co) = o;
            }
        }
    }
}

// [n,h,w,3] u8 -> f16 [n,ceil(h/s),ceil(w/s),32]: one thread per output pixel, four 16-byte stores
__global__ __launch_bounds__(256) void rrdb_input_u8_kernel(const uint8_t* __restrict__ src, half_t* __restrict__ dst,
                                                            long long pixels, int h, int w, int ho, int wo, int s, int swap_rb) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    const int x = (int)(i % wo);
    const long long t = i / wo;
    const int y = (int)(t % ho);
    const long long f = t / ho;
    union { uint4 q[4]; half_t v[32]; } o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o.q[k] = make_uint4(0, 0, 0, 0);
    const uint8_t* frame = src + f * h * w * 3;
    if (s == 1) {
        const uint8_t* p = frame + ((long long)y * w + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o.v[c] = (half_t)((float)p[swap_rb ? 2 - c : c] / 255.0f);
    } else {
#pragma unroll
        for (int sy = 0; sy < 2; ++sy) {
            int iy = 2 * y + sy;
            if (iy >= h) iy = h - 2;                             // reflect: index h reads h - 2
#pragma unroll
            for (int sx = 0; sx < 2; ++sx) {
                int ix = 2 * x + sx;
                if (ix >= w) ix = w - 2;
                const uint8_t* p = frame + ((long long)iy * w + ix) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) o.v[4 * c + 2 * sy + sx] = (half_t)((float)p[swap_rb ? 2 - c : c] / 255.0f);
            }
        }
    }
    uint4* d = reinterpret_cast<uint4*>(dst + i * 32);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = o.q[k];
}

bool rr_cin_ok(int c) { return c == 32 || c == 64 || c == 96 || c == 128 || c == 160 || c == 192; }

}  // namespace

extern "C" size_t elvis_rrdb_packed_weight_bytes(int cin, int cout) {
    if (!rr_cin_ok(cin) || (cout != 32 && cout != 64)) return 0;
    return (size_t)9 * cin * cout * 2;
}

extern "C" int elvis_rrdb_pack_weights(const float* w_oihw_host, int cin_real, int cout_real, int cin, int cout, void* packed_host) {
    ELVIS_REQUIRE(rr_cin_ok(cin), "elvis_rrdb_pack_weights: cin=%d is not one of 32, 64, 96, 128, 160, 192", cin);
    ELVIS_REQUIRE(cout == 32 || cout == 64, "elvis_rrdb_pack_weights: cout=%d is not 32 or 64", cout);
    ELVIS_REQUIRE(cin_real >= 1 && cin_real <= cin && cout_real >= 1 && cout_real <= cout,
                  "elvis_rrdb_pack_weights: real channels %d -> %d do not fit the padded %d -> %d", cin_real, cout_real, cin, cout);
    ELVIS_REQUIRE(w_oihw_host && packed_host, "elvis_rrdb_pack_weights: null pointer");
    sr_pack_weights(w_oihw_host, cin_real, cout_real, cin, cout, static_cast<uint16_t*>(packed_host));
    return ELVIS_OK;
}

extern "C" int elvis_rrdb_conv3x3(const void* x, int x_pitch, const void* w_packed, const float* bias, void* out, int out_pitch,
                                  int out_coff, const void* r1, int r1_pitch, const void* r2, int r2_pitch, int n, int h, int w,
                                  int cin, int cout, int upsample, int lrelu, float s0, float s1, int out_u8, int swap_rb,
                                  elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 0 && h >= 0 && w >= 0, "elvis_rrdb_conv3x3: bad shape n=%d h=%d w=%d", n, h, w);
    ELVIS_REQUIRE(rr_cin_ok(cin), "elvis_rrdb_conv3x3: cin=%d is not one of 32, 64, 96, 128, 160, 192", cin);
    ELVIS_REQUIRE(cout == 32 || cout == 64, "elvis_rrdb_conv3x3: cout=%d is not 32 or 64", cout);
    ELVIS_REQUIRE(x_pitch >= cin && x_pitch % 8 == 0, "elvis_rrdb_conv3x3: x_pitch=%d must be a multiple of 8 and at least cin=%d", x_pitch, cin);
    ELVIS_REQUIRE(h <= (1 << 29) && w <= (1 << 29), "elvis_rrdb_conv3x3: h=%d w=%d too large", h, w);
    const int ups = upsample ? 1 : 0;
    const int ho = h << ups, wo = w << ups;
    if (out_u8) {
        ELVIS_REQUIRE(cout == 32, "elvis_rrdb_conv3x3: out_u8 takes cout=32 (3 real channels), got cout=%d", cout);
        ELVIS_REQUIRE(out_coff == 0, "elvis_rrdb_conv3x3: out_u8 takes out_coff=0, got %d", out_coff);
    } else {
        ELVIS_REQUIRE(out_coff >= 0 && out_coff % 8 == 0 && out_pitch % 8 == 0 && out_coff + cout <= out_pitch,
                      "elvis_rrdb_conv3x3: channels [%d, %d) do not fit out_pitch=%d (offset and pitch are multiples of 8)",
                      out_coff, out_coff + cout, out_pitch);
    }
    ELVIS_REQUIRE(!r1 || (r1_pitch >= cout && r1_pitch % 4 == 0), "elvis_rrdb_conv3x3: r1_pitch=%d must be a multiple of 4 and at least cout=%d", r1_pitch, cout);
    ELVIS_REQUIRE(!r2 || (r2_pitch >= cout && r2_pitch % 4 == 0), "elvis_rrdb_conv3x3: r2_pitch=%d must be a multiple of 4 and at least cout=%d", r2_pitch, cout);
    if (n == 0 || h == 0 || w == 0) return ELVIS_OK;
    ELVIS_REQUIRE(x && w_packed && bias && out, "elvis_rrdb_conv3x3: null pointer");
    ELVIS_REQUIRE(((uintptr_t)x | (uintptr_t)w_packed | (uintptr_t)bias) % 16 == 0 && (uintptr_t)out % (out_u8 ? 1 : 8) == 0 &&
                  ((uintptr_t)r1 | (uintptr_t)r2) % 8 == 0, "elvis_rrdb_conv3x3: x, weights and bias are 16-byte aligned, out and residuals 8");
    const long long in_px = (long long)n * h * w, out_px = (long long)n * ho * wo;
    const long long x_bytes = in_px * x_pitch * 2, out_bytes = out_u8 ? out_px * 3 : out_px * out_pitch * 2;
    // aliasing: out may be x itself when the written channels lie past the read ones; any other overlap is refused
    if (sr_ranges_meet(x, x_bytes, out, out_bytes)) {
        ELVIS_REQUIRE(x == out && !out_u8 && !ups && out_pitch == x_pitch && out_coff >= cin,
                      "elvis_rrdb_conv3x3: out overlaps x: channels [%d, %d) written, [0, %d) read (out may alias x only at the same "
                      "pointer and pitch, without upsample, on disjoint channels)", out_coff, out_coff + cout, cin);
    }
    const void* rs[2] = {r1, r2};
    const int rp[2] = {r1_pitch, r2_pitch};
    for (int k = 0; k < 2; ++k) {
        if (!rs[k] || !sr_ranges_meet(rs[k], out_px * rp[k] * 2, out, out_bytes)) continue;
        // a residual inside out's allocation: element for element (read, then written, by one lane), or on other channels
        ELVIS_REQUIRE(rs[k] == out && !out_u8 && rp[k] == out_pitch && (out_coff == 0 || out_coff >= cout),
                      "elvis_rrdb_conv3x3: r%d overlaps out: channels [0, %d) read, [%d, %d) written", k + 1, cout, out_coff, out_coff + cout);
    }
    const int tiles_x = cdiv(wo, SR_TX), tiles_y = cdiv(ho, SR_TY);
    ELVIS_REQUIRE(n <= 65535 && tiles_y <= 65535, "elvis_rrdb_conv3x3: n=%d ho=%d is more than one launch holds", n, ho);
    RrdbArgs a;
    a.x = static_cast<const half_t*>(x);
    a.wp = static_cast<const half_t*>(w_packed);
    a.bias = bias;
    a.out = out;
    a.r1 = static_cast<const half_t*>(r1);
    a.r2 = static_cast<const half_t*>(r2);
    a.x_pitch = x_pitch; a.out_pitch = out_pitch; a.out_coff = out_coff; a.r1_pitch = r1_pitch; a.r2_pitch = r2_pitch;
    a.h = h; a.w = w; a.ho = ho; a.wo = wo; a.nkc = cin / SR_KC; a.ups = ups; a.lrelu = lrelu ? 1 : 0;
    a.out_u8 = out_u8 ? 1 : 0; a.swap_rb = swap_rb ? 1 : 0;
    a.s0 = s0; a.s1 = s1;
    const dim3 grid(tiles_x, tiles_y, n);
    if (cout == 64) {
        hipLaunchKernelGGL(rrdb_conv3x3_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, a);
        ELVIS_CHECK_LAUNCH("elvis_rrdb_conv3x3");
        elvis_note_launch("rrdb_conv3x3_kernel<64>");
    } else {
        hipLaunchKernelGGL(rrdb_conv3x3_kernel<32>, grid, dim3(256), 0, (hipStream_t)stream, a);
        ELVIS_CHECK_LAUNCH("elvis_rrdb_conv3x3");
        elvis_note_launch("rrdb_conv3x3_kernel<32>");
    }
    return ELVIS_OK;
}

extern "C" int elvis_rrdb_input_u8(const uint8_t* src, void* dst, int n, int h, int w, int s, int swap_rb, elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 0 && h >= 0 && w >= 0, "elvis_rrdb_input_u8: bad shape n=%d h=%d w=%d", n, h, w);
    ELVIS_REQUIRE(s == 1 || s == 2, "elvis_rrdb_input_u8: s=%d is not 1 or 2", s);
    if (n == 0 || h == 0 || w == 0) return ELVIS_OK;
    ELVIS_REQUIRE(s == 1 || ((h % 2 == 0 || h >= 3) && (w % 2 == 0 || w >= 3)),
                  "elvis_rrdb_input_u8: an odd h=%d or w=%d under 3 has no reflected row or column", h, w);
    ELVIS_REQUIRE(src && dst, "elvis_rrdb_input_u8: null pointer");
    ELVIS_REQUIRE((uintptr_t)dst % 16 == 0, "elvis_rrdb_input_u8: dst is 16-byte aligned");
    const int ho = (h + s - 1) / s, wo = (w + s - 1) / s;
    const long long pixels = (long long)n * ho * wo;
    const long long blocks = (pixels + 255) / 256;
    ELVIS_REQUIRE(blocks <= 0x7fffffffLL, "elvis_rrdb_input_u8: n=%d h=%d w=%d is more than one launch holds", n, h, w);
    hipLaunchKernelGGL(rrdb_input_u8_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, src,
                       static_cast<half_t*>(dst), pixels, h, w, ho, wo, s, swap_rb ? 1 : 0);
    ELVIS_CHECK_LAUNCH("elvis_rrdb_input_u8");
    elvis_note_launch(s == 2 ? "rrdb_input_u8_kernel<unshuffle2>" : "rrdb_input_u8_kernel<1>");
    return ELVIS_OK;
}
