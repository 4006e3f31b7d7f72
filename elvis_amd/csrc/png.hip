// Lossless PNG encoding on the device (include/elvis_amd.h "PNG writer"): row filters and the filter choice,
// symbol statistics, Huffman bit packing, Adler-32 partials and the chunk CRC-32s.  The host only plans the layout between
// the two phases (elvis_amd/png.py); tests/_png_ref.py states the stream in numpy and Python ints, and the files written
// here equal that statement bit for bit.
//
//   png_stats_kernel   phase 1: a workgroup per (frame, segment).  Rows are staged in LDS (the current row and the raw row
//                      above it, tiles of kPngTile bytes with a bpp-byte halo on the left), the five filter costs are
//                      reduced per row, the chosen type is written, and the filtered bytes (type bytes included) go into
//                      a 256-bin LDS histogram and the segment's Adler partial.
//   png_pack_kernel    phase 2: a workgroup per (frame, segment) owns the segment's IDAT chunk.  It re-filters the rows
//                      from the input (no filtered stream is ever stored), looks the codes up in an LDS table, gets every
//                      symbol's bit offset from a workgroup scan of the code lengths and ORs the bits into an LDS bit buffer
//                      that mirrors the dword grid of the output; whole dwords go out with dword stores, the bytes of a
//                      dword that the chunk shares with its neighbour with byte stores.  No global atomics.
//   png_crc_kernel     phase 2: a workgroup per chunk; every lane takes a slice, the slices are combined with x^(8 len) mod P.
//
//   png_stats_rle_kernel, png_pack_rle_kernel   the same two phases for the run-length stream (deflate "rle": literals and
//                      distance-1 matches, csrc/png_rle.h has the token rule).  One body each, png_stats_body<kRle> and
//                      png_pack_body<kRle>, serves both streams: staging, filter choice, Adler partials, the bit buffer, the
//                      lane scan, the clipped stores and the CRC kernel are the literal path's own.  What differs is what a
//                      lane's 16 consecutive positions of a tile emit (png_rle_lane: run heads, a workgroup scan for every
//                      position's offset in its run and the run's end, then rle_token_at) and the table sizes.
//
// Every global store of phase 2 is clipped to the chunk's own byte range and to the output buffer, and every code length
// is read through a 4-bit mask, so tables that disagree with the plan give a wrong file, never a write elsewhere.
#include "common.h"
#include "png_crc.h"
#include "png_rle.h"

namespace {

constexpr int kPngTile = 4096;                          // row bytes staged at a time
constexpr int kPngPerThread = kPngTile / kPngThreads;   // consecutive symbols a lane packs
constexpr int kPngHalo = 4;                             // >= bpp; keeps the staged row dword aligned
constexpr int kPngRowBuf = kPngTile + kPngHalo;
constexpr int kPngBitWords = 4096;                      // the LDS bit buffer, dwords
constexpr int kPngMaxLen = 15;
// before a tile the buffer holds at most kPngFlushAt bits; a row's type code and a full tile add at most 15 + 15 * kPngTile,
// and the segment's tail (EOB, the empty stored block or the Adler trailer) fits in the 128 bits kept free.  The run-length
// stream keeps the bound: a literal is one position and at most 15 bits, a match is at most 15 + 5 + 1 = 21 bits and stands
// for at least 3 positions (7 bits a position), a covered position emits nothing - a tile of `len` bytes adds at most 15 * len
constexpr int kPngFlushAt = kPngBitWords * 32 - (kPngMaxLen * kPngTile + kPngMaxLen) - 128;
constexpr int kPngHeaderBits = 1106;                    // 3 + 5 + 5 + 4 + 19 * 3 + 258 * 4
constexpr int kPngHeaderWords = 35;
constexpr int kPngStatsStride = 260;                    // 256 bins, Adler A, Adler B, length, 0
constexpr int kPngFrameTab = 304;                       // 257 code entries, the Adler trailer, 35 header words, padding
constexpr int kPngTabAdler = 257;
constexpr int kPngTabHeader = 258;
constexpr uint32_t kAdlerMod = 65521u;
// the run-length stream: 286 symbols, and a header of 3 + 5 + 5 + 4 + 19 * 3 + 287 * 4 bits
constexpr int kPngRleHeaderBits = 1222;
constexpr int kPngRleHeaderWords = 39;
constexpr int kPngRleStatsStride = 290;                 // 286 bins, Adler A, Adler B, length, 0
constexpr int kPngRleFrameTab = 328;                    // 286 code entries, the Adler trailer, 39 header words, padding
constexpr int kPngRleTabAdler = 286;
constexpr int kPngRleTabHeader = 287;
static_assert(RLE_SPAN == kPngTile, "a span of the run-length stream is the staging tile");
static_assert(kPngTile == kPngThreads * kPngPerThread && kPngPerThread <= 32, "a lane's positions are one mask of run heads");

__device__ __forceinline__ int png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int png_filter(int ft, int x, int a, int b, int c) {
    int pred = 0;
    if (ft == 1) pred = a;
    else if (ft == 2) pred = b;
    else if (ft == 3) pred = (a + b) >> 1;
    else if (ft == 4) pred = png_paeth(a, b, c);
    return (x - pred) & 255;
}

__device__ __forceinline__ uint32_t png_cost(int v) { return (uint32_t)(v < 128 ? v : 256 - v); }

// buf[kPngHalo + i] = byte t0 + i of row `row` in PNG channel order, i in [-kPngHalo, len); bytes left of the row and rows
// above the frame are 0
__device__ __forceinline__ void png_stage(uint8_t* buf, const uint8_t* frame, int row, int t0, int len, int rowbytes, int swap) {
    for (int i = (int)threadIdx.x - kPngHalo; i < len; i += kPngThreads) {
        const int j = t0 + i;
        uint8_t v = 0;
        if (row >= 0 && j >= 0) {
            // swap is 0 or 2: byte j of a BGR row is byte j + 2, j, j - 2 of the pixel.  Arithmetic on purpose - a branch
            // on the (uniform) flag inside this divergent loop was compiled to a test of a stale lane mask
            const int src = j + swap * (1 - j % 3);
            v = frame[(size_t)row * rowbytes + src];
        }
        buf[kPngHalo + i] = v;
    }
}

// Stages tile `tile` of row r.  A row of one tile keeps the row above in the other buffer from the row before (the
// caller staged row r0 - 1 once); wider rows stage both buffers per tile.  Returns the buffer of the current row.
__device__ __forceinline__ int png_stage_pair(uint8_t (*rows)[kPngRowBuf], int cur, bool& staged, const uint8_t* frame, int r, int t0,
                                              int len, int rowbytes, int swap, int ntiles) {
    if (ntiles > 1) {
        __syncthreads();
        png_stage(rows[1], frame, r - 1, t0, len, rowbytes, swap);
        png_stage(rows[0], frame, r, t0, len, rowbytes, swap);
        __syncthreads();
        return 0;
    }
    if (!staged) {
        png_stage(rows[cur], frame, r, t0, len, rowbytes, swap);
        staged = true;
        __syncthreads();
    }
    return cur;
}

// The tokens of a lane's kPngPerThread consecutive positions of the staged tile [0, len), which is one span of the
// run-length stream: emit(k, v, token) for position tid * kPngPerThread + k < len, v its filtered byte.  A position is a run
// head where it is the span's first or differs from the byte before it; a forward max-scan of the heads over the
// workgroup gives every position the head of its run, a backward min-scan the run's end (`len` behind the last run), and
// rle_token_at (png_rle.h) turns offset and run length into the token.  Nothing is read outside the tile and nothing is
// carried from tile to tile.  Every thread of the workgroup calls it (one barrier); wred is free again after the caller's
// next barrier.
template <class Emit>
__device__ __forceinline__ void png_rle_lane(const uint8_t* pc, const uint8_t* pp, int ft, int c, int len, int (*wred)[kPngWaves],
                                             Emit&& emit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = tid * kPngPerThread;
    int v[kPngPerThread];
    uint32_t heads = 0;
    int prev = -1;
    if (base > 0 && base < len) prev = png_filter(ft, pc[base - 1], pc[base - 1 - c], pp[base - 1], pp[base - 1 - c]);
#pragma unroll
    for (int k = 0; k < kPngPerThread; ++k) {
        const int i = base + k;
        v[k] = -2;
        if (i < len) {
            v[k] = png_filter(ft, pc[i], pc[i - c], pp[i], pp[i - c]);
            if (v[k] != prev) heads |= 1u << k;
        }
        prev = v[k];
    }
    // the last head at or before the lane's positions, the first head behind them
    int last = heads ? base + 31 - __clz((int)heads) : -1;
    int first = heads ? base + __ffs((int)heads) - 1 : len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(last, o, 64), b = __shfl_down(first, o, 64);
        if (lane >= o) last = max(last, a);
        if (lane + o < 64) first = min(first, b);
    }
    if (lane == 63) wred[0][wave] = last;
    if (lane == 0) wred[1][wave] = first;
    int head = __shfl_up(last, 1, 64), next = __shfl_down(first, 1, 64);
    if (lane == 0) head = -1;
    if (lane == 63) next = len;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kPngWaves; ++w) {
        if (w < wave) head = max(head, wred[0][w]);
        if (w > wave) next = min(next, wred[1][w]);
    }
    int end[kPngPerThread];
#pragma unroll
    for (int k = kPngPerThread - 1; k >= 0; --k) {
        end[k] = next;
        if ((heads >> k) & 1u) next = base + k;
    }
#pragma unroll
    for (int k = 0; k < kPngPerThread; ++k) {
        const int i = base + k;
        if ((heads >> k) & 1u) head = i;
        if (i < len) emit(k, v[k], rle_token_at(i - head, end[k] - head, v[k]));
    }
}

template <bool kRle>
__device__ __forceinline__ void png_stats_body(const uint8_t* __restrict__ frames, uint8_t* __restrict__ types,
                                               uint32_t* __restrict__ stats, int h, int rowbytes, int c, int swap, int filter,
                                               int seg_rows, int nseg) {
    constexpr int kBins = kRle ? RLE_SYMBOLS : 256;
    __shared__ __attribute__((aligned(16))) uint8_t rows[2][kPngRowBuf];
    __shared__ uint32_t hist[kBins];
    __shared__ unsigned long long red[5][kPngWaves];
    __shared__ int wred[2][kPngWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.x % nseg, f = blockIdx.x / nseg;
    const uint8_t* frame = frames + (size_t)f * h * rowbytes;
    const int r0 = seg * seg_rows, r1 = min(h, r0 + seg_rows);
    const uint32_t seglen = (uint32_t)(r1 - r0) * (uint32_t)(rowbytes + 1);
    const int ntiles = (rowbytes + kPngTile - 1) / kPngTile;
    for (int i = tid; i < kBins; i += kPngThreads) hist[i] = 0;
    int cur = 0;
    if (ntiles == 1) png_stage(rows[1], frame, r0 - 1, 0, rowbytes, rowbytes, swap);
    __syncthreads();
    unsigned long long sa = 0, sb = 0;   // Adler partial: sum d, sum (weight mod 65521) * d
    int runv = 0;
    uint32_t runc = 0;                   // equal bytes in a row cost one LDS atomic
    for (int r = r0; r < r1; ++r) {
        bool staged = false;
        int ft = filter;
        if (filter < 0) {
            uint32_t cost[5] = {0, 0, 0, 0, 0};
            for (int tile = 0; tile < ntiles; ++tile) {
                const int t0 = tile * kPngTile, len = min(kPngTile, rowbytes - t0);
                const int cb = png_stage_pair(rows, cur, staged, frame, r, t0, len, rowbytes, swap, ntiles);
                const uint8_t* pc = rows[cb] + kPngHalo;
                const uint8_t* pp = rows[cb ^ 1] + kPngHalo;
                for (int i = tid; i < len; i += kPngThreads) {
                    const int x = pc[i], a = pc[i - c], b = pp[i], d = pp[i - c];
                    cost[0] += png_cost(x);
                    cost[1] += png_cost((x - a) & 255);
                    cost[2] += png_cost((x - b) & 255);
                    cost[3] += png_cost((x - ((a + b) >> 1)) & 255);
                    cost[4] += png_cost((x - png_paeth(a, b, d)) & 255);
                }
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                unsigned long long v = cost[k];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0) red[k][wave] = v;
            }
            __syncthreads();
            unsigned long long best = 0;
            ft = 0;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                unsigned long long v = 0;
#pragma unroll
                for (int w = 0; w < kPngWaves; ++w) v += red[k][w];
                if (k == 0 || v < best) {   // a tie keeps the lower type
                    best = v;
                    ft = k;
                }
            }
        }
        const uint32_t rowoff = (uint32_t)(r - r0) * (uint32_t)(rowbytes + 1);
        if (tid == 0) {
            types[(size_t)f * h + r] = (uint8_t)ft;
            atomicAdd(&hist[ft], 1u);
            sa += (unsigned)ft;
            sb += (unsigned long long)((seglen - rowoff) % kAdlerMod) * (unsigned)ft;
        }
        for (int tile = 0; tile < ntiles; ++tile) {
            const int t0 = tile * kPngTile, len = min(kPngTile, rowbytes - t0);
            const int cb = png_stage_pair(rows, cur, staged, frame, r, t0, len, rowbytes, swap, ntiles);
            const uint8_t* pc = rows[cb] + kPngHalo;
            const uint8_t* pp = rows[cb ^ 1] + kPngHalo;
            if constexpr (kRle) {
                // the histogram counts tokens, the Adler partial bytes; equal symbols in a row (the literals of short runs,
                // the 258s of a long one) still cost one LDS atomic
                png_rle_lane(pc, pp, ft, c, len, wred, [&](int k, int v, const RleToken& t) {
                    if (t.kind != RLE_NOTHING) {
                        if (t.symbol == runv) {
                            ++runc;
                        } else {
                            if (runc) atomicAdd(&hist[runv], runc);
                            runv = t.symbol;
                            runc = 1;
                        }
                    }
                    const uint32_t pos = rowoff + 1u + (uint32_t)(t0 + tid * kPngPerThread + k);
                    sa += (unsigned)v;
                    sb += (unsigned long long)((seglen - pos) % kAdlerMod) * (unsigned)v;
                });
            } else {
                for (int i = tid; i < len; i += kPngThreads) {
                    const int v = png_filter(ft, pc[i], pc[i - c], pp[i], pp[i - c]);
                    if (v == runv) {
                        ++runc;
                    } else {
                        if (runc) atomicAdd(&hist[runv], runc);
                        runv = v;
                        runc = 1;
                    }
                    const uint32_t pos = rowoff + 1u + (uint32_t)(t0 + i);
                    sa += (unsigned)v;
                    sb += (unsigned long long)((seglen - pos) % kAdlerMod) * (unsigned)v;
                }
            }
        }
        __syncthreads();   // the row above of the next row is this row's buffer; red[] is free again
        cur ^= 1;
    }
    if (runc) atomicAdd(&hist[runv], runc);
    uint32_t a = (uint32_t)(sa % kAdlerMod), b = (uint32_t)(sb % kAdlerMod);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if (lane == 0) {
        red[0][wave] = a;
        red[1][wave] = b;
    }
    __syncthreads();
    uint32_t* dst = stats + (size_t)blockIdx.x * (kRle ? kPngRleStatsStride : kPngStatsStride);
    for (int i = tid; i < kBins; i += kPngThreads) dst[i] = hist[i];
    if (tid == 0) {
        unsigned long long ta = 0, tb = 0;
        for (int w = 0; w < kPngWaves; ++w) {
            ta += red[0][w];
            tb += red[1][w];
        }
        dst[kBins] = (uint32_t)(ta % kAdlerMod);
        dst[kBins + 1] = (uint32_t)(tb % kAdlerMod);
        dst[kBins + 2] = seglen;
        dst[kBins + 3] = 0;
    }
}

__global__ __launch_bounds__(kPngThreads) void png_stats_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ types,
                                                                uint32_t* __restrict__ stats, int h, int rowbytes, int c, int swap,
                                                                int filter, int seg_rows, int nseg) {
    png_stats_body<false>(frames, types, stats, h, rowbytes, c, swap, filter, seg_rows, nseg);
}

__global__ __launch_bounds__(kPngThreads) void png_stats_rle_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ types,
                                                                    uint32_t* __restrict__ stats, int h, int rowbytes, int c, int swap,
                                                                    int filter, int seg_rows, int nseg) {
    png_stats_body<true>(frames, types, stats, h, rowbytes, c, swap, filter, seg_rows, nseg);
}

// Thread 0 ORs `n` bits (n <= 32, v < 2^n) into the zeroed buffer at bit `pos`; every thread advances its copy of `pos`.
__device__ __forceinline__ void png_put(uint32_t* bits, int& pos, uint32_t v, int n) {
    if (threadIdx.x == 0 && n > 0) {
        const int w = pos >> 5, s = pos & 31;
        bits[w] |= v << s;
        if (s + n > 32) bits[w + 1] |= v >> (32 - s);
    }
    pos += n;
}

// Stores dwords [0, nwords) of the bit buffer at byte gword * 4 of `out`: a dword store where the dword lies inside
// [lo, hi), byte stores for the bytes of an edge dword that do.
__device__ __forceinline__ void png_store_words(const uint32_t* bits, int nwords, long long gword, uint8_t* out, long long lo, long long hi) {
    for (int d = threadIdx.x; d < nwords; d += kPngThreads) {
        const long long g = (gword + d) * 4;
        const uint32_t v = bits[d];
        if (g >= lo && g + 4 <= hi) {
            *reinterpret_cast<uint32_t*>(out + g) = v;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (g + b >= lo && g + b < hi) out[g + b] = (uint8_t)(v >> (8 * b));
        }
    }
}

// A lane keeps the bits of each of its positions as (bits << kShift) | count: a literal is a code of at most 15 bits (count
// in 4 bits), a token of the run-length stream at most a 15-bit code, 5 extra bits and the distance bit (21 bits, count in 5).
template <bool kRle>
__device__ __forceinline__ void png_pack_body(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ types,
                                              const long long* __restrict__ chunks, const uint32_t* __restrict__ frame_tab,
                                              uint8_t* __restrict__ out, long long out_bytes, int h, int rowbytes, int c, int swap,
                                              int seg_rows, int nseg) {
    constexpr int kSymbols = kRle ? RLE_SYMBOLS : 257;
    constexpr int kFrameTab = kRle ? kPngRleFrameTab : kPngFrameTab;
    constexpr int kTabAdler = kRle ? kPngRleTabAdler : kPngTabAdler;
    constexpr int kTabHeader = kRle ? kPngRleTabHeader : kPngTabHeader;
    constexpr int kHeaderBits = kRle ? kPngRleHeaderBits : kPngHeaderBits;
    constexpr int kHeaderWords = kRle ? kPngRleHeaderWords : kPngHeaderWords;
    constexpr int kShift = kRle ? 5 : 4;
    constexpr uint32_t kCount = (1u << kShift) - 1u;
    __shared__ __attribute__((aligned(16))) uint8_t rows[2][kPngRowBuf];
    __shared__ uint32_t bits[kPngBitWords];
    __shared__ uint32_t code[kSymbols];
    __shared__ int wsum[kPngWaves];
    __shared__ int wred[2][kPngWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.x % nseg, f = blockIdx.x / nseg;
    const uint8_t* frame = frames + (size_t)f * h * rowbytes;
    const uint32_t* tab = frame_tab + (size_t)f * kFrameTab;
    const int r0 = seg * seg_rows, r1 = min(h, r0 + seg_rows);
    const bool first = seg == 0, last = seg == nseg - 1;
    const int ntiles = (rowbytes + kPngTile - 1) / kPngTile;
    const long long cbeg = chunks[2 * (size_t)blockIdx.x], datalen = chunks[2 * (size_t)blockIdx.x + 1];
    if (cbeg < 0 || datalen < 0 || datalen > 0xffffffffLL) return;   // uniform
    const long long lo = cbeg, hi = min(cbeg + 8 + datalen, out_bytes);

    for (int i = tid; i < kPngBitWords; i += kPngThreads) bits[i] = 0;
    for (int i = tid; i < kSymbols; i += kPngThreads) code[i] = tab[i];
    int cur = 0;
    if (ntiles == 1) png_stage(rows[1], frame, r0 - 1, 0, rowbytes, rowbytes, swap);
    __syncthreads();

    long long gword = cbeg >> 2;          // the dword of `out` that bits[0] mirrors
    int pos = (int)(cbeg & 3) * 8;        // bits in the buffer, the bytes before the chunk included (they stay 0)
    const uint32_t dl = (uint32_t)datalen;
    png_put(bits, pos, dl >> 24, 8);
    png_put(bits, pos, (dl >> 16) & 255, 8);
    png_put(bits, pos, (dl >> 8) & 255, 8);
    png_put(bits, pos, dl & 255, 8);
    png_put(bits, pos, 'I', 8);
    png_put(bits, pos, 'D', 8);
    png_put(bits, pos, 'A', 8);
    png_put(bits, pos, 'T', 8);
    if (first) {
        png_put(bits, pos, 0x78, 8);
        png_put(bits, pos, 0x01, 8);
    }
    for (int k = 0; k < kHeaderWords; ++k) {
        const int nb = min(32, kHeaderBits - 32 * k);
        uint32_t v = tab[kTabHeader + k];
        if (k == 0) v = (v & ~1u) | (last ? 1u : 0u);          // BFINAL
        if (nb < 32) v &= (1u << nb) - 1u;
        png_put(bits, pos, v, nb);
    }

    for (int r = r0; r < r1; ++r) {
        bool staged = false;
        const int ft = min((int)types[(size_t)f * h + r], 4);
        __syncthreads();                                        // code[] is loaded; the serial puts do not race the lanes' ORs
        png_put(bits, pos, code[ft] >> 4, (int)(code[ft] & 15u));
        for (int tile = 0; tile < ntiles; ++tile) {
            const int t0 = tile * kPngTile, len = min(kPngTile, rowbytes - t0);
            const int cb = png_stage_pair(rows, cur, staged, frame, r, t0, len, rowbytes, swap, ntiles);
            const uint8_t* pc = rows[cb] + kPngHalo;
            const uint8_t* pp = rows[cb ^ 1] + kPngHalo;
            uint32_t ent[kPngPerThread];
            int mylen = 0;
            if constexpr (kRle) {
#pragma unroll
                for (int k = 0; k < kPngPerThread; ++k) ent[k] = 0;
                png_rle_lane(pc, pp, ft, c, len, wred, [&](int k, int, const RleToken& t) {
                    if (t.kind == RLE_NOTHING) return;
                    const uint32_t e = code[t.symbol];          // 0..285 by the rule, whatever the span holds
                    const int cl = (int)(e & 15u);
                    // the code, a match's extra bits behind it, and above them its distance bit, 0
                    const uint32_t b = ((e >> 4) & ((1u << cl) - 1u)) | ((uint32_t)t.extra << cl);
                    const int nb = cl + (t.kind == RLE_MATCH ? t.nextra + 1 : 0);
                    ent[k] = (b << kShift) | (uint32_t)nb;
                    mylen += nb;
                });
            } else {
#pragma unroll
                for (int k = 0; k < kPngPerThread; ++k) {
                    const int i = tid * kPngPerThread + k;
                    uint32_t e = 0;
                    if (i < len) e = code[png_filter(ft, pc[i], pc[i - c], pp[i], pp[i - c])];
                    ent[k] = e;
                    mylen += (int)(e & kCount);
                }
            }
            int incl = mylen;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();                                    // also orders thread 0's type code before the ORs below
            int woff = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kPngWaves; ++w) {
                if (w < wave) woff += wsum[w];
                total += wsum[w];
            }
            const int bp = pos + woff + incl - mylen;
            int w = bp >> 5, na = bp & 31;
            unsigned long long acc = 0;
#pragma unroll
            for (int k = 0; k < kPngPerThread; ++k) {
                const uint32_t e = ent[k];
                acc |= (unsigned long long)(e >> kShift) << na;   // na < 32 and at most 21 bits: no bit is lost
                na += (int)(e & kCount);
                if (na >= 32) {
                    atomicOr(&bits[w++], (uint32_t)acc);
                    acc >>= 32;
                    na -= 32;
                }
            }
            if (acc) atomicOr(&bits[w], (uint32_t)acc);
            pos += total;
            __syncthreads();
            if (pos > kPngFlushAt) {                            // uniform
                const int nfull = pos >> 5;
                png_store_words(bits, nfull, gword, out, lo, hi);
                const uint32_t carry = bits[nfull];
                __syncthreads();
                for (int i = tid; i <= nfull; i += kPngThreads) bits[i] = i == 0 ? carry : 0u;
                gword += nfull;
                pos &= 31;
                __syncthreads();
            }
        }
        if (ntiles == 1) __syncthreads();                       // the row above of the next row is this row's buffer
        cur ^= 1;
    }
    __syncthreads();
    png_put(bits, pos, code[256] >> 4, (int)(code[256] & 15u));  // EOB
    if (!last) png_put(bits, pos, 0, 3);                        // an empty stored block: 000, pad, 00 00 FF FF
    pos = (pos + 7) & ~7;
    if (!last) {
        png_put(bits, pos, 0xFFFF0000u, 32);
    } else {
        const uint32_t ad = tab[kTabAdler];
        png_put(bits, pos, ad >> 24, 8);
        png_put(bits, pos, (ad >> 16) & 255, 8);
        png_put(bits, pos, (ad >> 8) & 255, 8);
        png_put(bits, pos, ad & 255, 8);
    }
    __syncthreads();
    png_store_words(bits, (pos + 31) >> 5, gword, out, lo, hi);
}

__global__ __launch_bounds__(kPngThreads) void png_pack_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ types,
                                                               const long long* __restrict__ chunks, const uint32_t* __restrict__ frame_tab,
                                                               uint8_t* __restrict__ out, long long out_bytes, int h, int rowbytes, int c,
                                                               int swap, int seg_rows, int nseg) {
    png_pack_body<false>(frames, types, chunks, frame_tab, out, out_bytes, h, rowbytes, c, swap, seg_rows, nseg);
}

__global__ __launch_bounds__(kPngThreads) void png_pack_rle_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ types,
                                                                   const long long* __restrict__ chunks,
                                                                   const uint32_t* __restrict__ frame_tab, uint8_t* __restrict__ out,
                                                                   long long out_bytes, int h, int rowbytes, int c, int swap,
                                                                   int seg_rows, int nseg) {
    png_pack_body<true>(frames, types, chunks, frame_tab, out, out_bytes, h, rowbytes, c, swap, seg_rows, nseg);
}

// CRC-32 of a chunk's type and data, written big-endian behind them (png_crc.h has the slices and their combination).
__global__ __launch_bounds__(kPngThreads) void png_crc_kernel(const long long* __restrict__ chunks, uint8_t* __restrict__ out,
                                                              long long out_bytes, PngX2n x2n) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t wred[kPngWaves];
    png_crc_table(tab);
    __syncthreads();
    const long long cbeg = chunks[2 * (size_t)blockIdx.x], datalen = chunks[2 * (size_t)blockIdx.x + 1];
    if (cbeg < 0 || datalen < 0 || datalen > 0xffffffffLL) return;   // uniform
    const long long start = cbeg + 4, len = datalen + 4;
    if (start + len + 4 > out_bytes) return;
    const uint32_t crc = png_crc_workgroup(out + start, len, x2n, tab, wred);
    if (threadIdx.x == 0) {
        uint8_t* q = out + start + len;
        q[0] = (uint8_t)(crc >> 24);
        q[1] = (uint8_t)(crc >> 16);
        q[2] = (uint8_t)(crc >> 8);
        q[3] = (uint8_t)crc;
    }
}

int png_check_shape(const char* who, int n, int h, int w, int c, int order, int segment_rows, long long* segments) {
    ELVIS_REQUIRE(c == 1 || c == 3, "%s: 1 or 3 channels, got %d", who, c);
    ELVIS_REQUIRE(order == 0 || order == 1, "%s: order must be 0 (rgb) or 1 (bgr), got %d", who, order);
    ELVIS_REQUIRE(n >= 0 && h >= 1 && w >= 1, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    ELVIS_REQUIRE(segment_rows >= 1, "%s: segment_rows must be at least 1, got %d", who, segment_rows);
    ELVIS_REQUIRE((long long)w * c + 1 < 0x80000000LL && (long long)n * h < 0x80000000LL &&
                      (long long)n * h * ((long long)w * c + 1) < 0x80000000LL,
                  "%s: n * h * (w * c + 1) must be under 2^31 (n=%d h=%d w=%d c=%d)", who, n, h, w, c);
    *segments = (long long)n * ((h + segment_rows - 1) / segment_rows);
    return ELVIS_OK;
}

int png_stats_launch(const char* who, bool rle, const uint8_t* frames, uint8_t* types, uint32_t* stats, int n, int h, int w, int c,
                     int order, int filter, int segment_rows, elvis_stream_t stream) {
    long long segments = 0;
    if (int rc = png_check_shape(who, n, h, w, c, order, segment_rows, &segments)) return rc;
    ELVIS_REQUIRE(filter >= -1 && filter <= 4, "%s: filter must be -1 (adaptive) or 0..4, got %d", who, filter);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(frames && types && stats, "%s: null pointer", who);
    const int nseg = (h + segment_rows - 1) / segment_rows;
    hipLaunchKernelGGL(rle ? png_stats_rle_kernel : png_stats_kernel, dim3((unsigned)segments), dim3(kPngThreads), 0, (hipStream_t)stream,
                       frames, types, stats, h, w * c, c, (c == 3 && order == 1) ? 2 : 0, filter, segment_rows, nseg);
    ELVIS_CHECK_LAUNCH(who);
    elvis_note_launch(rle ? "png_stats_rle_kernel" : "png_stats_kernel");
    return ELVIS_OK;
}

int png_pack_launch(const char* who, bool rle, const uint8_t* frames, const uint8_t* types, const int64_t* chunks, const uint32_t* frame_tab,
                    uint8_t* out, int64_t out_bytes, int n, int h, int w, int c, int order, int segment_rows, elvis_stream_t stream) {
    long long segments = 0;
    if (int rc = png_check_shape(who, n, h, w, c, order, segment_rows, &segments)) return rc;
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(frames && types && chunks && frame_tab && out, "%s: null pointer", who);
    ELVIS_REQUIRE(out_bytes > 0 && ((uintptr_t)out & 3) == 0, "%s: out must be 4-byte aligned and out_bytes positive", who);
    const int nseg = (h + segment_rows - 1) / segment_rows;
    static const PngX2n x2n = png_x2n_table();
    hipLaunchKernelGGL(rle ? png_pack_rle_kernel : png_pack_kernel, dim3((unsigned)segments), dim3(kPngThreads), 0, (hipStream_t)stream,
                       frames, types, (const long long*)chunks, frame_tab, out, (long long)out_bytes, h, w * c, c,
                       (c == 3 && order == 1) ? 2 : 0, segment_rows, nseg);
    ELVIS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(png_crc_kernel, dim3((unsigned)segments), dim3(kPngThreads), 0, (hipStream_t)stream, (const long long*)chunks, out,
                       (long long)out_bytes, x2n);
    ELVIS_CHECK_LAUNCH(who);
    elvis_note_launch("png_crc_kernel");
    return ELVIS_OK;
}

}  // namespace

extern "C" int elvis_png_stats(const uint8_t* frames, uint8_t* types, uint32_t* stats, int n, int h, int w, int c, int order, int filter,
                               int segment_rows, elvis_stream_t stream) {
    return png_stats_launch("elvis_png_stats", false, frames, types, stats, n, h, w, c, order, filter, segment_rows, stream);
}

extern "C" int elvis_png_pack(const uint8_t* frames, const uint8_t* types, const int64_t* chunks, const uint32_t* frame_tab, uint8_t* out,
                              int64_t out_bytes, int n, int h, int w, int c, int order, int segment_rows, elvis_stream_t stream) {
    return png_pack_launch("elvis_png_pack", false, frames, types, chunks, frame_tab, out, out_bytes, n, h, w, c, order, segment_rows, stream);
}

extern "C" int elvis_png_stats_rle(const uint8_t* frames, uint8_t* types, uint32_t* stats, int n, int h, int w, int c, int order,
                                   int filter, int segment_rows, elvis_stream_t stream) {
    return png_stats_launch("elvis_png_stats_rle", true, frames, types, stats, n, h, w, c, order, filter, segment_rows, stream);
}

extern "C" int elvis_png_pack_rle(const uint8_t* frames, const uint8_t* types, const int64_t* chunks, const uint32_t* frame_tab,
                                  uint8_t* out, int64_t out_bytes, int n, int h, int w, int c, int order, int segment_rows,
                                  elvis_stream_t stream) {
    return png_pack_launch("elvis_png_pack_rle", true, frames, types, chunks, frame_tab, out, out_bytes, n, h, w, c, order, segment_rows,
                           stream);
}
