// Block complexity: the spatial (SC) and temporal (TC) complexity maps the server side starts from, which the reference
// gets from EVCA (elvis.py:968-1224 reads its block CSVs, presley.py:202 calls analyze_frames).  EVCA is not available to
// this build, so this is a BUILD-DEFINED analyser in the published VCA form - a weighted sum of the absolute DCT
// coefficients of a luma block (SC) and of its difference to the previous frame (TC) - stated as a contract in
// include/elvis_amd.h and DESIGN.md 7 and in numpy float64 in tests/_complexity_ref.py.  It does not claim EVCA's pixels.
//
// All arithmetic is float64 on integer luma; the DCT basis and the weights come from the host, so no device cos / exp
// takes part.  No atomics, a fixed reduction order: two runs give the same bytes.
#include "common.h"
#include "i420.h"

#define CX_THREADS 256
#define CX_TILE 1024   // luma pixels of one strip of blocks: B rows x CX_TILE / B columns, CX_TILE / (B * B) blocks
#define CX_COEFFS 4    // coefficients per lane, pass and map: CX_TILE / CX_THREADS

// Four luma bytes (pixels x .. x + 3 of one row) as one dword, lowest byte first.  `p` points at the first byte of pixel
// x; the 4 * C bytes are read as dwords where the address allows it and as bytes otherwise, never a byte beyond them.
template <int C, int ORDER>
__device__ __forceinline__ uint32_t cx_luma4(const uint8_t* __restrict__ p) {
    union { uint32_t d[C]; uint8_t b[4 * C]; } v;
    if (((uintptr_t)p & 3) == 0) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int k = 0; k < C; ++k) v.d[k] = q[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4 * C; ++k) v.b[k] = p[k];
    }
    if constexpr (C == 1) {
        return v.d[0];
    } else {
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = v.b[3 * k + (ORDER ? 2 : 0)], g = v.b[3 * k + 1], b = v.b[3 * k + (ORDER ? 0 : 2)];
            out |= (uint32_t)i420_y(r, g, b) << (8 * k);
        }
        return out;
    }
}

// One workgroup takes one strip of G = TW / B neighbouring blocks of one block row (TW = CX_TILE / B luma columns) and
// walks the clip frame by frame, so every byte of the clip is read from HBM and converted to luma once: the luma strip
// of frame f stays in LDS as the predecessor of frame f + 1 (two strips, used in turn).  The predecessor of frame 0 is
// `prev`, or frame 0 itself where there is none - the difference is then 0 and TC[0] comes out as exactly 0.0 by the
// same arithmetic.
//
// Per frame, SC and TC together from the two staged strips:
//   pass 1  T[k][x]  = sum_y D[k][y] * X'[y][x]        lane (x, kg) holds k = 4 kg .. 4 kg + 3 for its column x
//   pass 2  Cf[k][l] = sum_m T[k][g B + m] * D[l][m]    lane (g B + l, kg) holds the same four k for its (block g, l)
//   sum     w[k][l] * |Cf[k][l]| over the lane's four k, then over the B lanes of a block by xor-shuffles, then over
//           the B / 4 lane groups through LDS in index order; / B^2.
// X' = X - X[0][0] and the difference D' = (X - P) - (X[0][0] - P[0][0]) are formed in integers from the luma bytes as
// pass 1 reads them.  LDS: lanes of a wave read consecutive bytes (pass 1), one T value per block (pass 2, a
// broadcast) and D[l][m] down a column - D is kept at a pitch of B + 1 doubles, which puts the B lanes of a block on
// distinct bank pairs for B = 8, 16 and 32.  Columns of the strip past the last whole block are staged as zeros and
// never written out.
template <int B, int C, int ORDER>
__global__ __launch_bounds__(CX_THREADS) void block_complexity_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ prev,
                                                                      const double* __restrict__ dct, const double* __restrict__ weight,
                                                                      double* __restrict__ sc, double* __restrict__ tc, int n, int h, int w,
                                                                      int by, int bx, int strips) {
    constexpr int TW = CX_TILE / B, G = TW / B, KG = CX_THREADS / TW, DP = B + 1;
    static_assert(B / KG == CX_COEFFS && TW % 4 == 0, "one lane holds CX_COEFFS coefficients");
    __shared__ uint32_t lum[2][CX_TILE / 4];
    __shared__ double ta[CX_TILE], td[CX_TILE];
    __shared__ double dl[B * DP];
    __shared__ double red[2][KG][G];

    const int t = threadIdx.x;
    const int strip = blockIdx.x % strips, brow = blockIdx.x / strips;
    const int x0 = strip * TW;
    const int valid = min(TW, bx * B - x0);                               // a multiple of B, at least B
    const int j = t % TW, kg = t / TW, k0 = kg * CX_COEFFS;
    const int g = j / B, l = j % B;
    const int lrow = t / (TW / 4), lx = (t % (TW / 4)) * 4;               // the four pixels this lane stages
    const long long frame_bytes = (long long)h * w * C;
    const long long lofs = ((long long)(brow * B + lrow) * w + x0 + lx) * C;

    for (int i = t; i < B * B; i += CX_THREADS) dl[(i / B) * DP + i % B] = dct[i];
    double wr[CX_COEFFS];
#pragma unroll
    for (int r = 0; r < CX_COEFFS; ++r) wr[r] = weight[(k0 + r) * B + l];
    lum[1][t] = lx < valid ? cx_luma4<C, ORDER>((prev ? prev : frames) + lofs) : 0u;

    for (int f = 0; f < n; ++f) {
        lum[f & 1][t] = lx < valid ? cx_luma4<C, ORDER>(frames + f * frame_bytes + lofs) : 0u;
        __syncthreads();
        const uint8_t* cur = reinterpret_cast<const uint8_t*>(lum[f & 1]);
        const uint8_t* prv = reinterpret_cast<const uint8_t*>(lum[(f & 1) ^ 1]);
        const int cur00 = cur[g * B], dif00 = cur00 - (int)prv[g * B];
        double a[CX_COEFFS], d[CX_COEFFS];
#pragma unroll
        for (int r = 0; r < CX_COEFFS; ++r) a[r] = d[r] = 0.0;
#pragma unroll 8
        for (int y = 0; y < B; ++y) {
            const int xv = cur[y * TW + j], pv = prv[y * TW + j];
            const double xa = (double)(xv - cur00), xd = (double)((xv - pv) - dif00);
#pragma unroll
            for (int r = 0; r < CX_COEFFS; ++r) {
                const double c = dl[(k0 + r) * DP + y];
                a[r] = fma(c, xa, a[r]);
                d[r] = fma(c, xd, d[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < CX_COEFFS; ++r) {
            ta[(k0 + r) * TW + j] = a[r];
            td[(k0 + r) * TW + j] = d[r];
            a[r] = d[r] = 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int m = 0; m < B; ++m) {
            const double c = dl[l * DP + m];
#pragma unroll
            for (int r = 0; r < CX_COEFFS; ++r) {
                a[r] = fma(ta[(k0 + r) * TW + g * B + m], c, a[r]);
                d[r] = fma(td[(k0 + r) * TW + g * B + m], c, d[r]);
            }
        }
        double s = 0.0, u = 0.0;
#pragma unroll
        for (int r = 0; r < CX_COEFFS; ++r) {
            s += wr[r] * fabs(a[r]);
            u += wr[r] * fabs(d[r]);
        }
#pragma unroll
        for (int o = B / 2; o > 0; o >>= 1) {                             // the B lanes of a block are B neighbours of one wave
            s += __shfl_xor(s, o, ELVIS_WAVE);
            u += __shfl_xor(u, o, ELVIS_WAVE);
        }
        if (l == 0) {
            red[0][kg][g] = s;
            red[1][kg][g] = u;
        }
        __syncthreads();                                                  // also: every lane is done with ta / td and with `prv`
        if (t < 2 * G && (t % G) * B < valid) {
            const int map = t / G, gg = t % G;
            double total = red[map][0][gg];
#pragma unroll
            for (int q = 1; q < KG; ++q) total += red[map][q][gg];
            (map ? tc : sc)[((long long)f * by + brow) * bx + x0 / B + gg] = total / (double)(B * B);
        }
    }
}

template <int B, int C, int ORDER>
static int cx_launch(const uint8_t* frames, const uint8_t* prev, const double* dct, const double* weight, double* sc, double* tc, int n,
                     int h, int w, hipStream_t stream) {
    constexpr int TW = CX_TILE / B;
    const int by = h / B, bx = w / B;
    const int strips = cdiv((long long)bx * B, TW);
    ELVIS_REQUIRE((long long)strips * by <= 0x7fffffffLL, "elvis_block_complexity_f64: h=%d w=%d is more than one launch holds", h, w);
    hipLaunchKernelGGL((block_complexity_kernel<B, C, ORDER>), dim3(strips * by), dim3(CX_THREADS), 0, stream, frames, prev, dct, weight, sc,
                       tc, n, h, w, by, bx, strips);
    ELVIS_CHECK_LAUNCH("elvis_block_complexity_f64");
    static const ElvisKernelName name("block_complexity_kernel<%d,%d,%d>", B, C, ORDER);
    elvis_note_launch(name.s);
    return ELVIS_OK;
}

template <int B>
static int cx_dispatch(const uint8_t* frames, const uint8_t* prev, const double* dct, const double* weight, double* sc, double* tc, int n,
                       int h, int w, int c, int order, hipStream_t stream) {
    if (c == 1) return cx_launch<B, 1, 0>(frames, prev, dct, weight, sc, tc, n, h, w, stream);
    if (order) return cx_launch<B, 3, 1>(frames, prev, dct, weight, sc, tc, n, h, w, stream);
    return cx_launch<B, 3, 0>(frames, prev, dct, weight, sc, tc, n, h, w, stream);
}

extern "C" int elvis_block_complexity_f64(const uint8_t* frames, const uint8_t* prev, const double* dct, const double* weight, double* sc,
                                          double* tc, int n, int h, int w, int c, int order, int block, elvis_stream_t stream) {
    ELVIS_REQUIRE(block == 8 || block == 16 || block == 32, "elvis_block_complexity_f64: block must be 8, 16 or 32, got %d", block);
    ELVIS_REQUIRE(c == 1 || c == 3, "elvis_block_complexity_f64: 1 or 3 channels, got %d", c);
    ELVIS_REQUIRE(order == 0 || order == 1, "elvis_block_complexity_f64: order must be 0 (rgb) or 1 (bgr), got %d", order);
    ELVIS_REQUIRE(n >= 0 && h >= block && w >= block, "elvis_block_complexity_f64: bad shape n=%d h=%d w=%d for blocks of %d", n, h, w, block);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(frames && dct && weight && sc && tc, "elvis_block_complexity_f64: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (block == 8) return cx_dispatch<8>(frames, prev, dct, weight, sc, tc, n, h, w, c, order, s);
    if (block == 16) return cx_dispatch<16>(frames, prev, dct, weight, sc, tc, n, h, w, c, order, s);
    return cx_dispatch<32>(frames, prev, dct, weight, sc, tc, n, h, w, c, order, s);
}
