// Lossless PNG decoding on the device (include/elvis_amd.h "PNG reader"): the host reads the signature, the
// chunk headers and IHDR and uploads the file bytes as they are with a table of chunk spans (elvis_amd/png.py); the
// stream and the pixels are only ever touched here.  tests/_png_read_ref.py states the decoder in Python; zlib and PIL
// are the oracles.
//
//   png_gather_kernel    a workgroup per (chunk, slice): the payloads of a frame's IDAT chunks are copied behind one
//                        another into the frame's zlib stream.
//   png_crc_check_kernel a workgroup per chunk, of any type: the CRC-32 of type and data (png_crc.h, the writer's
//                        routine) against the four bytes stored behind them.
//   png_inflate_kernel   one workgroup of one wave per stream: inflate.h's inflate_run, whose text the host check
//                        tools/png_inflate_check.cpp walks too.  Decoder state is wave-uniform, the code tables and the
//                        32 KB window are in LDS, the lanes share table fills, copies, flushes and the Adler-32.
//   png_unfilter_kernel  a workgroup per frame; bands of 64 rows in order, one row per lane of wave 0, lane l one pixel
//                        behind lane l - 1: "above" is the neighbour lane's previous result (one cross-lane shift a
//                        step), "above-left" the lane's own previous "above".  Tiles of the skewed band are staged
//                        through LDS by all four waves; the channel swap, the gray replication and the dropped alpha
//                        happen in the stores.  A band's last row is written back, raw, over its filtered bytes: the
//                        next band's lane 0 stages its "above" row from there, behind the workgroup barrier.
//
// No kernel waits on another wave's progress, there are no global atomics, and every global access is clipped to the
// frame's or chunk's own range of its buffer: a malformed file gives a status word, never an access elsewhere.
#include "common.h"
#include "inflate.h"
#include "png_crc.h"

namespace {

constexpr int kGatherSlices = 8;      // workgroups that share the copy of one chunk
constexpr int kUnfTile = 128;         // pixels of a tile, per row
constexpr int kUnfRows = 64;          // rows of a band: one per lane
constexpr int kUnfPitch = kUnfTile * 4 + 4;   // bytes; 129 dwords, so the lanes of a step hit different banks

// chunks i64 [nchunks, 3]: offset of the chunk's type field in `files`, length of its data, where the data go in
// `streams` (below 0: not an IDAT chunk)
__global__ __launch_bounds__(kPngThreads) void png_gather_kernel(const uint8_t* __restrict__ files, long long files_bytes,
                                                                 const long long* __restrict__ chunks, uint8_t* __restrict__ streams,
                                                                 long long streams_bytes) {
    const long long off = chunks[3 * (size_t)blockIdx.x], len = chunks[3 * (size_t)blockIdx.x + 1], dst = chunks[3 * (size_t)blockIdx.x + 2];
    if (dst < 0 || off < 0 || len <= 0 || len > 0x7fffffffLL || off > files_bytes - 4 - len || dst > streams_bytes - len) return;   // uniform
    const long long per = (len + kGatherSlices - 1) / kGatherSlices;
    const long long s0 = min(len, (long long)blockIdx.y * per), s1 = min(len, s0 + per);
    const uint8_t* src = files + off + 4;
    for (long long i = s0 + threadIdx.x; i < s1; i += kPngThreads) streams[dst + i] = src[i];
}

__global__ __launch_bounds__(kPngThreads) void png_crc_check_kernel(const uint8_t* __restrict__ files, long long files_bytes,
                                                                    const long long* __restrict__ chunks, uint32_t* __restrict__ crc_status,
                                                                    PngX2n x2n) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t wred[kPngWaves];
    png_crc_table(tab);
    __syncthreads();
    const long long off = chunks[3 * (size_t)blockIdx.x], len = chunks[3 * (size_t)blockIdx.x + 1];
    if (off < 0 || len < 0 || len > 0x7fffffffLL || off > files_bytes - 8 - len) {   // uniform
        if (threadIdx.x == 0) crc_status[blockIdx.x] = PNG_E_CRC;
        return;
    }
    const uint32_t crc = png_crc_workgroup(files + off, len + 4, x2n, tab, wred);
    if (threadIdx.x == 0) {
        const uint8_t* q = files + off + 4 + len;
        const uint32_t stored = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | (uint32_t)q[3];
        crc_status[blockIdx.x] = stored == crc ? 0u : (uint32_t)PNG_E_CRC;
    }
}

__global__ __launch_bounds__(INF_LANE_COUNT) void png_inflate_kernel(const uint8_t* __restrict__ streams, long long streams_bytes,
                                                                     const long long* __restrict__ in_spans, uint8_t* __restrict__ out,
                                                                     long long out_bytes, const long long* __restrict__ out_spans,
                                                                     uint32_t* __restrict__ status) {
    __shared__ InfShared S;
    const size_t f = blockIdx.x;
    const long long ioff = in_spans[2 * f], ilen = in_spans[2 * f + 1], ooff = out_spans[2 * f], cap = out_spans[2 * f + 1];
    uint32_t* st4 = status + 4 * f;
    // a span that is not inside its buffer touches nothing (uniform)
    const bool in_ok = ioff >= 0 && ilen >= 0 && ilen < 0x7fffffffLL && ioff <= streams_bytes - ilen;
    const bool out_ok = ooff >= 0 && (ooff & 3) == 0 && cap >= 0 && cap < 0x7fffffffLL && ooff <= out_bytes - cap;
    if (!in_ok || !out_ok) {
        if (threadIdx.x == 0) {
            st4[0] = in_ok ? INF_E_LONG : INF_E_INPUT;
            st4[1] = st4[2] = 0;
            st4[3] = 1;
        }
        return;
    }
    inflate_run(&S, streams + ioff, (uint32_t)ilen, out + ooff, (uint32_t)cap, st4);
}

__device__ __forceinline__ int unf_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// filtered: n streams of h rows of 1 + w * BPP bytes, `stride` bytes apart; a band's last row is overwritten with its raw
// bytes.  frames u8 [n, h, w, CH].  status u32 [n, 2]: 0 or PNG_E_FILTER, the first row whose type is above 4 (such a
// row is taken as type 0).
template <int BPP, int CH>
__global__ __launch_bounds__(kPngThreads) void png_unfilter_kernel(uint8_t* filtered, long long stride, uint8_t* __restrict__ frames,
                                                                   uint32_t* __restrict__ status, int h, int w, int bgr) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[kUnfRows][kUnfPitch];
    __shared__ __attribute__((aligned(16))) uint8_t above[kUnfTile * 4];
    constexpr int TB = kUnfTile * BPP;   // bytes of a row's tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t f = blockIdx.x;
    uint8_t* filt = filtered + f * (size_t)stride;
    uint8_t* frame = frames + f * (size_t)h * w * CH;
    const long long rowlen = (long long)w * BPP + 1;
    const int swap = bgr ? 2 : 0;   // channel k of a BGR pixel is byte 2 - k of the file's
    int bad_row = h;   // wave 0: the first row with a type above 4
    for (int r0 = 0; r0 < h; r0 += kUnfRows) {
        const int rows = min(kUnfRows, h - r0);
        int ft = 0;
        if (wave == 0 && lane < rows) {
            ft = filt[(long long)(r0 + lane) * rowlen];
            if (ft > 4) {
                bad_row = min(bad_row, r0 + lane);
                ft = 0;
            }
        }
        uint32_t left = 0, up_prev = 0, result = 0;   // the pixel to the left, the one above it, this lane's last result
        for (int x0 = 0; x0 < w + rows - 1; x0 += kUnfTile) {
            // stage: row l holds pixels x0 - l .. x0 - l + kUnfTile - 1 of row r0 + l
            for (int idx = tid; idx < rows * TB; idx += kPngThreads) {
                const int l = idx / TB, i = idx % TB, x = x0 - l + i / BPP;
                if (x >= 0 && x < w) tile[l][i] = filt[(long long)(r0 + l) * rowlen + 1 + (long long)(x0 - l) * BPP + i];
            }
            for (int i = tid; i < TB; i += kPngThreads) {
                const int x = x0 + i / BPP;
                above[i] = (r0 > 0 && x < w) ? filt[(long long)(r0 - 1) * rowlen + 1 + (long long)x0 * BPP + i] : (uint8_t)0;
            }
            __syncthreads();
            if (wave == 0) {
                for (int s = 0; s < kUnfTile; ++s) {
                    const int x = x0 - lane + s;
                    uint32_t up = __shfl_up(result, 1, 64);
                    if (lane == 0) {
                        up = 0;
#pragma unroll
                        for (int k = 0; k < BPP; ++k) up |= (uint32_t)above[s * BPP + k] << (8 * k);
                    }
                    if (lane < rows && x >= 0 && x < w) {
                        uint32_t raw = 0;
#pragma unroll
                        for (int k = 0; k < BPP; ++k) {
                            const int v = tile[lane][s * BPP + k];
                            const int a = (left >> (8 * k)) & 255, b = (up >> (8 * k)) & 255, c = (up_prev >> (8 * k)) & 255;
                            int pred = 0;
                            if (ft == 1) pred = a;
                            else if (ft == 2) pred = b;
                            else if (ft == 3) pred = (a + b) >> 1;
                            else if (ft == 4) pred = unf_paeth(a, b, c);
                            const int o = (v + pred) & 255;
                            tile[lane][s * BPP + k] = (uint8_t)o;
                            raw |= (uint32_t)o << (8 * k);
                        }
                        left = raw;
                        result = raw;
                    }
                    up_prev = up;
                }
            }
            __syncthreads();
            for (int idx = tid; idx < rows * kUnfTile * CH; idx += kPngThreads) {
                const int l = idx / (kUnfTile * CH), o = idx % (kUnfTile * CH), px = o / CH, k = o % CH, x = x0 - l + px;
                if (x >= 0 && x < w) {
                    const int sc = BPP == 1 ? 0 : k + swap * (1 - k);   // arithmetic, as png.hip's staging: no branch on the flag here
                    frame[((size_t)(r0 + l) * w + x) * CH + k] = tile[l][px * BPP + sc];
                }
            }
            if (rows == kUnfRows && r0 + kUnfRows < h) {
                const int l = kUnfRows - 1;
                for (int i = tid; i < TB; i += kPngThreads) {
                    const int x = x0 - l + i / BPP;
                    if (x >= 0 && x < w) filt[(long long)(r0 + l) * rowlen + 1 + (long long)(x0 - l) * BPP + i] = tile[l][i];
                }
            }
            __syncthreads();
        }
    }
    if (wave == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bad_row = min(bad_row, __shfl_xor(bad_row, o, 64));
        if (lane == 0) {
            status[2 * f] = bad_row < h ? (uint32_t)PNG_E_FILTER : 0u;
            status[2 * f + 1] = bad_row < h ? (uint32_t)bad_row : 0u;
        }
    }
}

}  // namespace

extern "C" int elvis_png_gather(const uint8_t* files, int64_t files_bytes, const int64_t* chunks, int nchunks, uint8_t* streams,
                                int64_t streams_bytes, uint32_t* crc_status, elvis_stream_t stream) {
    ELVIS_REQUIRE(nchunks >= 0, "elvis_png_gather: nchunks must not be negative, got %d", nchunks);
    ELVIS_REQUIRE(files_bytes >= 0 && files_bytes < 0x80000000LL && streams_bytes >= 0 && streams_bytes < 0x80000000LL,
                  "elvis_png_gather: files_bytes and streams_bytes must be in [0, 2^31)");
    if (nchunks == 0) return ELVIS_OK;
    ELVIS_REQUIRE(files && chunks && streams && crc_status, "elvis_png_gather: null pointer");
    static const PngX2n x2n = png_x2n_table();
    hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)nchunks, kGatherSlices), dim3(kPngThreads), 0, (hipStream_t)stream, files,
                       (long long)files_bytes, (const long long*)chunks, streams, (long long)streams_bytes);
    ELVIS_CHECK_LAUNCH("elvis_png_gather");
    hipLaunchKernelGGL(png_crc_check_kernel, dim3((unsigned)nchunks), dim3(kPngThreads), 0, (hipStream_t)stream, files, (long long)files_bytes,
                       (const long long*)chunks, crc_status, x2n);
    ELVIS_CHECK_LAUNCH("elvis_png_gather");
    elvis_note_launch("png_crc_check_kernel");
    return ELVIS_OK;
}

extern "C" int elvis_png_inflate(const uint8_t* streams, int64_t streams_bytes, const int64_t* in_spans, uint8_t* out, int64_t out_bytes,
                                 const int64_t* out_spans, uint32_t* status, int n, elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 0, "elvis_png_inflate: n must not be negative, got %d", n);
    ELVIS_REQUIRE(streams_bytes >= 0 && streams_bytes < 0x80000000LL && out_bytes >= 0 && out_bytes < 0x80000000LL,
                  "elvis_png_inflate: streams_bytes and out_bytes must be in [0, 2^31)");
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(streams && in_spans && out && out_spans && status, "elvis_png_inflate: null pointer");
    ELVIS_REQUIRE(((uintptr_t)out & 3) == 0, "elvis_png_inflate: out must be 4-byte aligned");
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)n), dim3(INF_LANE_COUNT), 0, (hipStream_t)stream, streams, (long long)streams_bytes,
                       (const long long*)in_spans, out, (long long)out_bytes, (const long long*)out_spans, status);
    ELVIS_CHECK_LAUNCH("elvis_png_inflate");
    elvis_note_launch("png_inflate_kernel");
    return ELVIS_OK;
}

extern "C" int elvis_png_unfilter(uint8_t* filtered, int64_t stride, uint8_t* frames, uint32_t* status, int n, int h, int w, int bpp,
                                  int channels, int order, elvis_stream_t stream) {
    ELVIS_REQUIRE(bpp == 1 || bpp == 3 || bpp == 4, "elvis_png_unfilter: bpp must be 1, 3 or 4, got %d", bpp);
    ELVIS_REQUIRE(channels == 3 || (channels == 1 && bpp == 1), "elvis_png_unfilter: channels must be 3, or 1 for bpp 1 (channels=%d bpp=%d)",
                  channels, bpp);
    ELVIS_REQUIRE(order == 0 || order == 1, "elvis_png_unfilter: order must be 0 (rgb) or 1 (bgr), got %d", order);
    ELVIS_REQUIRE(n >= 0 && h >= 1 && w >= 1, "elvis_png_unfilter: bad shape n=%d h=%d w=%d", n, h, w);
    const long long need = (long long)h * ((long long)w * bpp + 1);
    ELVIS_REQUIRE((long long)w * bpp + 1 < 0x80000000LL && need < 0x80000000LL && (long long)n * need < 0x80000000LL,
                  "elvis_png_unfilter: n * h * (w * bpp + 1) must be under 2^31 (n=%d h=%d w=%d bpp=%d)", n, h, w, bpp);
    ELVIS_REQUIRE(stride >= need && (n == 0 || stride < 0x80000000LL / n), "elvis_png_unfilter: stride %lld must be at least h * (w * bpp + 1) = %lld and n * stride under 2^31",
                  (long long)stride, need);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(filtered && frames && status, "elvis_png_unfilter: null pointer");
    const dim3 grid((unsigned)n), block(kPngThreads);
    hipStream_t s = (hipStream_t)stream;
    if (bpp == 1 && channels == 1) hipLaunchKernelGGL((png_unfilter_kernel<1, 1>), grid, block, 0, s, filtered, (long long)stride, frames, status, h, w, order);
    else if (bpp == 1) hipLaunchKernelGGL((png_unfilter_kernel<1, 3>), grid, block, 0, s, filtered, (long long)stride, frames, status, h, w, order);
    else if (bpp == 3) hipLaunchKernelGGL((png_unfilter_kernel<3, 3>), grid, block, 0, s, filtered, (long long)stride, frames, status, h, w, order);
    else hipLaunchKernelGGL((png_unfilter_kernel<4, 3>), grid, block, 0, s, filtered, (long long)stride, frames, status, h, w, order);
    ELVIS_CHECK_LAUNCH("elvis_png_unfilter");
    elvis_note_launch("png_unfilter_kernel");
    return ELVIS_OK;
}
