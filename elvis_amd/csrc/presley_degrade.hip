// Presley's adaptive degraders on the device, in OpenCV's 8-bit arithmetic: what produces the frames the classical
// restorers (classical.hip) are fed.
//   elvis_degrade_scale_u8       - downscale_block / degrade_adaptive_downsample (presley.py:978-983, utils.py:1153-1161):
//                                  INTER_AREA to max(1, b // scale), at any ratio, then INTER_LINEAR back to b
//   elvis_degrade_gaussian_fx_u8 - blur_block / degrade_adaptive_blur (presley.py:986-990, utils.py:1203-1210):
//                                  `rounds` x GaussianBlur 5x5, sigma 1, in cv2's CV_8U fixed point
// One wave per block, the block staged in LDS, lanes strided over (pixel, channel), as in classical.hip; any block size in
// [2, 32], 1..4 channels; pixels past the last whole block are never written.  OpenCV is absent from the build and GPU
// environments, so its rules are restated from OpenCV 4.x ("parity unpinned"); what is pinned is
// bit-exactness against the numpy restatement in tests/_presley_degrade_ref.py.  Evaluation order of every float
// expression is fixed (explicit round-to-nearest intrinsics; the library is built with -ffp-contract=off).
#include "block_u8.h"

namespace {

__device__ __forceinline__ int pixel_of(int xc, int c) {   // xc / c for xc < 2^15, c in 1..4 (uniform), no integer divide
    return c == 1 ? xc : (c == 2 ? xc >> 1 : (c == 4 ? xc >> 2 : (int)(((unsigned)xc * 43691u) >> 17)));
}

// LDS of degrade_scale_kernel in bytes, sized by the largest target hb = b / 2 (the host's launch and the kernel's
// carve-up both go through these offsets)
struct ScaleLds {
    int coef, e_src, e_w, e_start, buf, small, blk, bytes;
    __host__ __device__ ScaleLds(int b, int c) {
        const int hb = b / 2;
        coef = 0;                                  // int   [b][3]     linear_coef of every destination index
        e_src = coef + 4 * 3 * b;                  // int   [2b]       this d's area table: source index,
        e_w = e_src + 4 * 2 * b;                   // float [2b]       weight,
        e_start = e_w + 4 * 2 * b;                 // int   [hb + 2]   first entry of destination i (and the end)
        buf = e_start + 4 * (hb + 2);              // float [b][d][c]  horizontal area pass
        small = buf + 4 * b * hb * c;              // u8    [d][d][c]  the INTER_AREA result
        blk = small + ((hb * hb * c + 3) & ~3);    // u8    [b][b][c]  the block
        bytes = blk + ((b * b * c + 3) & ~3);
    }
};

// One wave per block (the scale is uniform per workgroup).  INTER_AREA from b to d = max(1, b / scale): at an integer
// ratio block_u8.h's area_box; otherwise cv::ResizeArea_<uchar, float> - per source row
// buf[dx] = sum_k float(S[sx_k]) * alpha_k, per destination row sum[dx] = sum_j beta_j * buf_j[dx], float32 from 0
// in table order, every product rounded before it is added, then saturate_cast<uchar> (round-half-even).  Every output
// is its own ordered sum; the lanes are strided over outputs and never split a sum.  Then INTER_LINEAR back to b.
__global__ __launch_bounds__(64) void degrade_scale_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ scales,
                                                           uint8_t* __restrict__ dst, int h, int w, int c, int b, int by, int bx,
                                                           const int32_t* __restrict__ tab_starts,
                                                           const int32_t* __restrict__ tab_src,
                                                           const float* __restrict__ tab_w, int tab_len) {
    extern __shared__ int lds[];
    const BlockAddr at(h, w, c, b, by, bx);
    const long long rs = at.rs, base = at.base;
    const int sc = scales[at.blk];
    if (sc <= 1) {                                  // 0 = keep; 1 resizes to the same size twice: the identity
        copy_block(src, dst, base, rs, b, c);
        return;
    }
    const int hb = b / 2;
    const int d = b / sc > 1 ? b / sc : 1;          // <= hb
    const int rowlen = b * c, drow = d * c;
    const ScaleLds L(b, c);
    char* l8 = (char*)lds;
    int* coef = (int*)(l8 + L.coef);
    int* e_src = (int*)(l8 + L.e_src);
    float* e_w = (float*)(l8 + L.e_w);
    int* e_start = (int*)(l8 + L.e_start);
    float* buf = (float*)(l8 + L.buf);
    uint8_t* small = (uint8_t*)(l8 + L.small);
    uint8_t* blkp = (uint8_t*)(l8 + L.blk);
    const bool whole = b % d == 0;
    stage_block(src, blkp, base, rs, b, rowlen);
    for (int e = threadIdx.x; e < b; e += ELVIS_WAVE) linear_coef(e, d, b, coef[3 * e], coef[3 * e + 1], coef[3 * e + 2]);
    if (!whole) {
        // this d's table, read with a wave-uniform base; every index is clamped so that a bad table cannot leave the LDS
        const int32_t* st = tab_starts + d * (hb + 2);
        const int e0 = clampi(st[0], 0, tab_len);
        const int cap = e0 + 2 * b < tab_len ? e0 + 2 * b : tab_len;
        const int e1 = clampi(st[d], e0, cap);
        for (int e = threadIdx.x; e <= d; e += ELVIS_WAVE) e_start[e] = clampi(st[e], e0, e1) - e0;
        for (int e = threadIdx.x; e < e1 - e0; e += ELVIS_WAVE) {
            e_src[e] = clampi(tab_src[e0 + e], 0, b - 1);
            e_w[e] = tab_w[e0 + e];
        }
    }
    __syncthreads();
    if (whole) {
        const int fac = b / d;
        const float inv = 1.0f / (float)(fac * fac);
        for (int e = threadIdx.x; e < d * drow; e += ELVIS_WAVE) {
            const int sy = e / drow;
            const int xc = e - sy * drow;
            const int sx = pixel_of(xc, c);
            const int ch = xc - sx * c;
            small[e] = (uint8_t)area_box(blkp, rowlen, c, sy, sx, ch, fac, inv);
        }
    } else {
        for (int e = threadIdx.x; e < b * drow; e += ELVIS_WAVE) {
            const int r = e / drow;
            const int xc = e - r * drow;
            const int dx = pixel_of(xc, c);
            const uint8_t* row = blkp + r * rowlen + (xc - dx * c);
            float acc = 0.f;
            for (int k = e_start[dx]; k < e_start[dx + 1]; ++k) acc = __fadd_rn(acc, __fmul_rn((float)row[e_src[k] * c], e_w[k]));
            buf[e] = acc;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < d * drow; e += ELVIS_WAVE) {
            const int dy = e / drow;
            const float* col = buf + (e - dy * drow);
            float acc = 0.f;
            for (int k = e_start[dy]; k < e_start[dy + 1]; ++k) acc = __fadd_rn(acc, __fmul_rn(e_w[k], col[e_src[k] * drow]));
            small[e] = (uint8_t)clampi(__float2int_rn(acc), 0, 255);
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < b * rowlen; e += ELVIS_WAVE) {
        const int y = e / rowlen;
        const int xc = e - y * rowlen;
        const int x = pixel_of(xc, c);
        const int ch = xc - x * c;
        const int y0 = coef[3 * y], x0 = coef[3 * x];
        const int y1 = y0 + 1 < d ? y0 + 1 : y0, x1 = x0 + 1 < d ? x0 + 1 : x0;
        const uint8_t* s0 = small + y0 * drow + ch;
        const uint8_t* s1 = small + y1 * drow + ch;
        dst[base + y * rs + xc] = (uint8_t)linear_mix(s0[x0 * c], s0[x1 * c], s1[x0 * c], s1[x1 * c], coef[3 * x + 1],
                                                      coef[3 * x + 2], coef[3 * y + 1], coef[3 * y + 2]);
    }
}

// One wave per block (`rounds` is uniform per workgroup).  One pass of cv2.GaussianBlur(5x5, sigma 1) on CV_8U:
// horizontal u8 x tap summed in u16 (at most 255 * 256: ufixedpoint16's saturating adds never fire), vertical
// u16 x tap summed in u32, one rounding (acc + 0x8000) >> 16.  The passes ping-pong between two LDS tiles, cur (u8) and
// hp (u16); the block touches HBM at its first load and its last store only.
// LDS banks: both tiles are dense, rows of b*c elements with no padding.  In either pass lane l takes element
// e = l + 64 i, so at every tap the 64 lanes read 64 consecutive elements of a row-major tile (64 B of cur, 128 B of
// hp: at most 32 consecutive dwords, lanes sharing a dword are served by one broadcast).  The vertical pass walks its five
// rows one tap after the other, never two rows in one instruction, so the odd row stride of c = 3 (b*c bytes) does
// not decide which banks meet; padding the rows would only break the contiguous run.  Conflicts can arise only where one
// instruction covers several rows of a small block and the reflected border folds them onto each other (tiles of a few
// hundred bytes); not measured with counters.
__global__ __launch_bounds__(64) void degrade_gaussian_fx_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ rounds,
                                                                 uint8_t* __restrict__ dst, int h, int w, int c, int b, int by,
                                                                 int bx, int t0, int t1, int t2) {
    extern __shared__ int lds[];
    const BlockAddr at(h, w, c, b, by, bx);
    const long long rs = at.rs, base = at.base;
    const int r = clampi(rounds[at.blk], 0, ELVIS_DEGRADE_MAX_ROUNDS);
    if (r == 0) {
        copy_block(src, dst, base, rs, b, c);
        return;
    }
    const int rowlen = b * c, count = b * rowlen;
    uint16_t* hp = (uint16_t*)lds;                          // [b][b][c]
    uint8_t* cur = (uint8_t*)(hp + ((count + 1) & ~1));     // [b][b][c]
    stage_block(src, cur, base, rs, b, rowlen);
    __syncthreads();
    const int y_first = threadIdx.x / rowlen, xc_first = threadIdx.x - y_first * rowlen;
    for (int it = 0; it < r; ++it) {
        for (int e = threadIdx.x, y = y_first, xc = xc_first; e < count; e += ELVIS_WAVE) {
            const int x = pixel_of(xc, c);
            const uint8_t* row = cur + y * rowlen + (xc - x * c);
            const uint32_t acc = (uint32_t)t2 * row[x * c]
                + (uint32_t)t1 * ((uint32_t)row[reflect101(x - 1, b) * c] + row[reflect101(x + 1, b) * c])
                + (uint32_t)t0 * ((uint32_t)row[reflect101(x - 2, b) * c] + row[reflect101(x + 2, b) * c]);
            hp[e] = (uint16_t)acc;
            for (xc += ELVIS_WAVE; xc >= rowlen; xc -= rowlen) ++y;
        }
        __syncthreads();
        for (int e = threadIdx.x, y = y_first, xc = xc_first; e < count; e += ELVIS_WAVE) {
            const uint16_t* col = hp + xc;
            const uint32_t acc = (uint32_t)t2 * col[y * rowlen]
                + (uint32_t)t1 * ((uint32_t)col[reflect101(y - 1, b) * rowlen] + col[reflect101(y + 1, b) * rowlen])
                + (uint32_t)t0 * ((uint32_t)col[reflect101(y - 2, b) * rowlen] + col[reflect101(y + 2, b) * rowlen]);
            cur[e] = (uint8_t)((acc + 0x8000u) >> 16);
            for (xc += ELVIS_WAVE; xc >= rowlen; xc -= rowlen) ++y;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < count; e += ELVIS_WAVE) {
        const int y = e / rowlen;
        dst[base + y * rs + (e - y * rowlen)] = cur[e];
    }
}

}  // namespace

extern "C" int elvis_degrade_scale_u8(const uint8_t* src, const int32_t* scales, uint8_t* dst, int n, int h, int w, int c,
                                      int block, int by, int bx, const int32_t* tab_starts, const int32_t* tab_src,
                                      const float* tab_w, int tab_len, elvis_stream_t stream) {
    int rc = check_block_maps(src && scales && dst, n, h, w, c, block, by, bx, false, "elvis_degrade_scale_u8");
    if (rc) return rc;
    ELVIS_REQUIRE(tab_starts && tab_src && tab_w && tab_len > 0, "elvis_degrade_scale_u8: area tables missing");
    hipLaunchKernelGGL(degrade_scale_kernel, dim3((unsigned)(n * by * bx)), dim3(ELVIS_WAVE), (size_t)ScaleLds(block, c).bytes,
                       (hipStream_t)stream, src, scales, dst, h, w, c, block, by, bx, tab_starts, tab_src, tab_w, tab_len);
    ELVIS_CHECK_LAUNCH("elvis_degrade_scale_u8");
    elvis_note_launch("degrade_scale_kernel");
    return ELVIS_OK;
}

extern "C" int elvis_degrade_gaussian_fx_u8(const uint8_t* src, const int32_t* rounds, uint8_t* dst, int n, int h, int w, int c,
                                            int block, int by, int bx, int tap0, int tap1, int tap2, elvis_stream_t stream) {
    int rc = check_block_maps(src && rounds && dst, n, h, w, c, block, by, bx, false, "elvis_degrade_gaussian_fx_u8");
    if (rc) return rc;
    // 8.8 fixed point: the taps sum to one, which is what keeps the horizontal pass inside u16
    ELVIS_REQUIRE(tap0 >= 0 && tap1 >= 0 && tap2 >= 0 && 2 * (tap0 + tap1) + tap2 == 256,
                  "elvis_degrade_gaussian_fx_u8: taps %d %d %d %d %d are not 8.8 fixed point summing to 256", tap0, tap1, tap2,
                  tap1, tap0);
    const int count = block * block * c;
    const size_t shmem = sizeof(uint16_t) * (size_t)((count + 1) & ~1) + (size_t)count;   // <= 12 KiB
    hipLaunchKernelGGL(degrade_gaussian_fx_kernel, dim3((unsigned)(n * by * bx)), dim3(ELVIS_WAVE), shmem, (hipStream_t)stream,
                       src, rounds, dst, h, w, c, block, by, bx, tap0, tap1, tap2);
    ELVIS_CHECK_LAUNCH("elvis_degrade_gaussian_fx_u8");
    elvis_note_launch("degrade_gaussian_fx_kernel");
    return ELVIS_OK;
}
