// Baseline JPEG decoding on the device (include/elvis_amd.h "JPEG reader"): the host walks the markers and
// uploads the file bytes as they are with a table of the entropy-coded segments, the Huffman tables as (counts, values)
// and the quantisation tables (elvis_amd/jpeg.py); the compressed bytes and the pixels are only ever touched here.
// tests/_jpeg_ref.py states the decoder in Python and numpy; PIL on libjpeg-turbo is the second oracle.
//
//   jpeg_tables_kernel   a lane per (frame, table): jpeg_decode.h's jpeg_build_table, the 9-bit first-level lookup and
//                        the counts and values of the canonical walk for longer codes.
//   jpeg_entropy_kernel  a lane per entropy-coded segment, all frames of a clip in one launch: a file without restart
//                        markers is one serial stream and takes one lane, not one wave; a file with them is as many
//                        lanes as it has intervals.  jpeg_decode.h's jpeg_decode_segment, whose text the host check
//                        tools/jpeg_decode_check.cpp walks too: dequantised int16 coefficients in natural order, stored
//                        as they are decoded into blocks that were zero, and two status words a segment.
//   jpeg_idct_kernel     a lane per block: libjpeg's slow integer IDCT (jidctint.c) in 64-bit integers, which are exact
//                        for any coefficient the entropy kernel lets through; the 8 x 8 samples go to the component's
//                        plane as eight 8-byte stores.
//   jpeg_colour_kernel   a lane per pixel: libjpeg's fancy h2v1 / h2v2 chroma upsampling read straight from the planes
//                        (neighbours replicated at the edges; plain replication where the chroma plane is at most two
//                        samples wide, as libjpeg chooses), its fixed-point YCbCr -> RGB, the channel order and the
//                        gray replication in the stores.
//
// No kernel waits on another wave's progress, there are no global atomics, and every global access is clipped to the
// segment's, the frame's or the component's own range of its buffer: a malformed file gives a status word, never an
// access elsewhere.
#include "common.h"
#include "jpeg_decode.h"

namespace {

constexpr int kEntropyThreads = 64;   // one wave: a lane per segment
constexpr int kIdctThreads = 256;
constexpr int kColourX = 64, kColourY = 4;

__global__ __launch_bounds__(kEntropyThreads) void jpeg_tables_kernel(const uint8_t* __restrict__ huff, JpegTable* __restrict__ tables,
                                                                      int ntables) {
    const int t = blockIdx.x * kEntropyThreads + threadIdx.x;
    if (t < ntables) jpeg_build_table(tables + t, huff + (size_t)t * JPG_HUFF_BYTES);
}

__global__ __launch_bounds__(kEntropyThreads) void jpeg_entropy_kernel(const uint8_t* __restrict__ files, long long files_bytes,
                                                                       const int32_t* __restrict__ segs, int nseg,
                                                                       const int32_t* __restrict__ fd, int n,
                                                                       const JpegTable* __restrict__ tables,
                                                                       const uint16_t* __restrict__ qt, int16_t* __restrict__ coef,
                                                                       long long stride_blocks, uint32_t* __restrict__ status) {
    const int s = blockIdx.x * kEntropyThreads + threadIdx.x;
    if (s >= nseg) return;
    const int32_t* sd = segs + (size_t)JPG_SEG_WORDS * s;
    const long long off = sd[0], len = sd[1];
    const int f = sd[4];
    uint32_t* st = status + 2 * (size_t)s;
    // a segment that is not inside the upload, or whose frame's descriptor does not fit the buffers, touches nothing
    if (f < 0 || f >= n || off < 0 || len < 0 || off > files_bytes - len || !jpeg_fd_ok(fd + (size_t)JPG_FD_WORDS * f, stride_blocks)) {
        st[0] = JPG_E_DESC;
        st[1] = 0;
        return;
    }
    jpeg_decode_segment(files + off, (uint32_t)len, fd + (size_t)JPG_FD_WORDS * f, tables + (size_t)JPG_TABLES * f, qt + (size_t)256 * f,
                        sd[2], sd[3], coef + (size_t)f * stride_blocks * 64, stride_blocks, st);
}

// One 8-point pass of jidctint.c (CONST_BITS 13), descaled by `shift` bits with rounding.
__device__ __forceinline__ void idct_pass(const long long (&v)[8], long long (&o)[8], int shift) {
    long long z1 = (v[2] + v[6]) * 4433;
    const long long t2 = z1 - v[6] * 15137, t3 = z1 + v[2] * 6270;
    const long long t0 = (v[0] + v[4]) * 8192, t1 = (v[0] - v[4]) * 8192;
    const long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    long long a0 = v[7], a1 = v[5], a2 = v[3], a3 = v[1];
    z1 = a0 + a3;
    long long z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const long long z5 = (z3 + z4) * 9633;
    a0 *= 2446;
    a1 *= 16819;
    a2 *= 25172;
    a3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 += z1 + z3;
    a1 += z2 + z4;
    a2 += z2 + z3;
    a3 += z1 + z4;
    const long long half = 1ll << (shift - 1);
    o[0] = (t10 + a3 + half) >> shift;
    o[7] = (t10 - a3 + half) >> shift;
    o[1] = (t11 + a2 + half) >> shift;
    o[6] = (t11 - a2 + half) >> shift;
    o[2] = (t12 + a1 + half) >> shift;
    o[5] = (t12 - a1 + half) >> shift;
    o[3] = (t13 + a0 + half) >> shift;
    o[4] = (t13 - a0 + half) >> shift;
}

// coef i16 [n][stride_blocks][64] -> planes u8 [n][stride_blocks * 64]; grid (blocks of a frame / kIdctThreads, n).
__global__ __launch_bounds__(kIdctThreads) void jpeg_idct_kernel(const int16_t* __restrict__ coef, long long stride_blocks,
                                                                 const int32_t* __restrict__ fd, uint8_t* __restrict__ planes) {
    const size_t f = blockIdx.y;
    const int32_t* d = fd + JPG_FD_WORDS * f;
    if (!jpeg_fd_ok(d, stride_blocks)) return;   // uniform
    const long long b = (long long)blockIdx.x * kIdctThreads + threadIdx.x;
    if (b >= d[5]) return;                       // the last workgroup is ragged
    int c = 0;
    if (d[0] == 3 && b >= JPG_FD_COMP(d, 1)[2]) c = b >= JPG_FD_COMP(d, 2)[2] ? 2 : 1;
    const int32_t* cd = JPG_FD_COMP(d, c);
    const long long local = b - cd[2], pitch = cd[4], cols = pitch >> 3;
    const long long by = local / cols, bx = local - by * cols;
    const int4* src = reinterpret_cast<const int4*>(coef + (f * (size_t)stride_blocks + (size_t)b) * 64);
    int in[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int4 q = src[r];
        const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            in[r * 8 + 2 * k] = (int)(int16_t)(w[k] & 0xffff);
            in[r * 8 + 2 * k + 1] = w[k] >> 16;
        }
    }
    int ws[64];
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        long long v[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = in[i * 8 + col];
        idct_pass(v, o, 11);
#pragma unroll
        for (int i = 0; i < 8; ++i) ws[i * 8 + col] = (int)o[i];   // |.| < 2^22 for |coefficient| <= 2^15
    }
    uint8_t* plane = planes + f * (size_t)stride_blocks * 64 + (size_t)cd[3] + (size_t)(by * 8) * pitch + (size_t)bx * 8;
#pragma unroll
    for (int row = 0; row < 8; ++row) {
        long long v[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ws[row * 8 + i];
        idct_pass(v, o, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            // libjpeg's range-limit table: the descaled value wraps at 10 bits around the level shift, then clamps
            const int x = (int)(((o[i] + 512) & 1023) - 512) + 128;
            const uint32_t sample = (uint32_t)min(255, max(0, x));
            if (i < 4) lo |= sample << (8 * i);
            else hi |= sample << (8 * (i - 4));
        }
        *reinterpret_cast<uint2*>(plane + (size_t)row * pitch) = make_uint2(lo, hi);
    }
}

// The chroma sample of pixel (x, y) from plane p of cw x ch samples that count.
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, long long pitch, int x, int y, int hmax, int vmax, int cw, int ch) {
    if (hmax == 1) return p[(long long)y * pitch + x];
    const int i = x >> 1, odd = x & 1;
    if (cw <= 2) return p[(long long)(vmax == 2 ? y >> 1 : y) * pitch + i];
    const int nb = odd ? min(i + 1, cw - 1) : max(i - 1, 0);
    if (vmax == 1) {
        const uint8_t* row = p + (long long)y * pitch;
        return (3 * row[i] + row[nb] + (odd ? 2 : 1)) >> 2;
    }
    const int j = y >> 1, jn = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
    const uint8_t* near = p + (long long)j * pitch;
    const uint8_t* far = p + (long long)jn * pitch;
    const int here = 3 * near[i] + far[i], beside = 3 * near[nb] + far[nb];
    return (3 * here + beside + (odd ? 7 : 8)) >> 4;
}

// planes u8 [n][stride_blocks * 64] -> frames u8 [n, h, w, CH]; grid (w / 64, h / 4, n).
template <int CH>
__global__ __launch_bounds__(kColourX* kColourY) void jpeg_colour_kernel(const uint8_t* __restrict__ planes, long long stride_blocks,
                                                                         const int32_t* __restrict__ fd, uint8_t* __restrict__ frames,
                                                                         int h, int w, int bgr) {
    const size_t f = blockIdx.z;
    const int32_t* d = fd + JPG_FD_WORDS * f;
    if (!jpeg_fd_ok(d, stride_blocks)) return;   // uniform
    const int x = blockIdx.x * kColourX + threadIdx.x, y = blockIdx.y * kColourY + threadIdx.y;
    const int hmax = d[1], vmax = d[2];
    // the planes cover the picture: whole MCUs of 8 hmax x 8 vmax pixels
    if (x >= w || y >= h || (long long)d[3] * 8 * hmax < w || (long long)d[4] * 8 * vmax < h) return;
    const uint8_t* base = planes + f * (size_t)stride_blocks * 64;
    const int lum = base[(size_t)JPG_FD_COMP(d, 0)[3] + (size_t)y * JPG_FD_COMP(d, 0)[4] + x];
    uint8_t* out = frames + ((f * (size_t)h + y) * w + x) * CH;
    if (d[0] == 1 || CH == 1) {
#pragma unroll
        for (int k = 0; k < CH; ++k) out[k] = (uint8_t)lum;
        return;
    }
    const int cw = (w + hmax - 1) / hmax, ch = (h + vmax - 1) / vmax;
    const int cb = chroma_at(base + JPG_FD_COMP(d, 1)[3], JPG_FD_COMP(d, 1)[4], x, y, hmax, vmax, cw, ch) - 128;
    const int cr = chroma_at(base + JPG_FD_COMP(d, 2)[3], JPG_FD_COMP(d, 2)[4], x, y, hmax, vmax, cw, ch) - 128;
    const int r = lum + ((91881 * cr + 32768) >> 16);
    const int g = lum + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    const int bl = lum + ((116130 * cb + 32768) >> 16);
    out[bgr ? 2 : 0] = (uint8_t)min(255, max(0, r));
    out[1] = (uint8_t)min(255, max(0, g));
    out[bgr ? 0 : 2] = (uint8_t)min(255, max(0, bl));
}

}  // namespace

extern "C" int elvis_jpeg_entropy(const uint8_t* files, int64_t files_bytes, const int32_t* segs, int nseg, const int32_t* fd, int n,
                                  const uint8_t* huff, const uint16_t* qt, void* tables, int16_t* coef, int64_t stride_blocks,
                                  uint32_t* status, elvis_stream_t stream) {
    static_assert(sizeof(JpegTable) == ELVIS_JPEG_TABLE_BYTES, "ELVIS_JPEG_TABLE_BYTES is sizeof(JpegTable)");
    ELVIS_REQUIRE(nseg >= 0 && n >= 0 && n <= 65535, "elvis_jpeg_entropy: nseg must not be negative and n in [0, 65535] (nseg=%d n=%d)", nseg, n);
    ELVIS_REQUIRE(files_bytes >= 0 && files_bytes < 0x80000000LL, "elvis_jpeg_entropy: files_bytes must be in [0, 2^31)");
    ELVIS_REQUIRE(stride_blocks >= 1 && stride_blocks < 0x80000000LL / 64, "elvis_jpeg_entropy: stride_blocks must be in [1, 2^25)");
    if (nseg == 0 || n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(files && segs && fd && huff && qt && tables && coef && status, "elvis_jpeg_entropy: null pointer");
    ELVIS_REQUIRE(((uintptr_t)tables & 1) == 0 && ((uintptr_t)qt & 1) == 0 && ((uintptr_t)coef & 15) == 0,
                  "elvis_jpeg_entropy: tables and qt must be 2-byte aligned, coef 16-byte aligned");
    const int ntables = n * JPG_TABLES;
    hipLaunchKernelGGL(jpeg_tables_kernel, dim3((unsigned)cdiv(ntables, kEntropyThreads)), dim3(kEntropyThreads), 0, (hipStream_t)stream, huff,
                       (JpegTable*)tables, ntables);
    ELVIS_CHECK_LAUNCH("elvis_jpeg_entropy");
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)cdiv(nseg, kEntropyThreads)), dim3(kEntropyThreads), 0, (hipStream_t)stream, files,
                       (long long)files_bytes, segs, nseg, fd, n, (const JpegTable*)tables, qt, coef, (long long)stride_blocks, status);
    ELVIS_CHECK_LAUNCH("elvis_jpeg_entropy");
    elvis_note_launch("jpeg_entropy_kernel");
    return ELVIS_OK;
}

extern "C" int elvis_jpeg_idct(const int16_t* coef, int64_t stride_blocks, const int32_t* fd, int n, uint8_t* planes, elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 0 && n <= 65535, "elvis_jpeg_idct: n must be in [0, 65535], got %d", n);
    ELVIS_REQUIRE(stride_blocks >= 1 && stride_blocks < 0x80000000LL / 64, "elvis_jpeg_idct: stride_blocks must be in [1, 2^25)");
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(coef && fd && planes, "elvis_jpeg_idct: null pointer");
    ELVIS_REQUIRE(((uintptr_t)coef & 15) == 0 && ((uintptr_t)planes & 7) == 0, "elvis_jpeg_idct: coef must be 16-byte aligned, planes 8-byte aligned");
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)cdiv(stride_blocks, kIdctThreads), (unsigned)n), dim3(kIdctThreads), 0, (hipStream_t)stream,
                       coef, (long long)stride_blocks, fd, planes);
    ELVIS_CHECK_LAUNCH("elvis_jpeg_idct");
    elvis_note_launch("jpeg_idct_kernel");
    return ELVIS_OK;
}

extern "C" int elvis_jpeg_colour(const uint8_t* planes, int64_t stride_blocks, const int32_t* fd, uint8_t* frames, int n, int h, int w,
                                 int channels, int order, elvis_stream_t stream) {
    ELVIS_REQUIRE(channels == 1 || channels == 3, "elvis_jpeg_colour: channels must be 1 or 3, got %d", channels);
    ELVIS_REQUIRE(order == 0 || order == 1, "elvis_jpeg_colour: order must be 0 (rgb) or 1 (bgr), got %d", order);
    ELVIS_REQUIRE(n >= 0 && n <= 65535 && h >= 1 && w >= 1 && h <= 65535 && w <= 65535, "elvis_jpeg_colour: bad shape n=%d h=%d w=%d", n, h, w);
    ELVIS_REQUIRE(stride_blocks >= 1 && stride_blocks < 0x80000000LL / 64, "elvis_jpeg_colour: stride_blocks must be in [1, 2^25)");
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(planes && fd && frames, "elvis_jpeg_colour: null pointer");
    const dim3 grid((unsigned)cdiv(w, kColourX), (unsigned)cdiv(h, kColourY), (unsigned)n), block(kColourX, kColourY);
    if (channels == 1) hipLaunchKernelGGL((jpeg_colour_kernel<1>), grid, block, 0, (hipStream_t)stream, planes, (long long)stride_blocks, fd, frames, h, w, order);
    else hipLaunchKernelGGL((jpeg_colour_kernel<3>), grid, block, 0, (hipStream_t)stream, planes, (long long)stride_blocks, fd, frames, h, w, order);
    ELVIS_CHECK_LAUNCH("elvis_jpeg_colour");
    elvis_note_launch("jpeg_colour_kernel");
    return ELVIS_OK;
}
