// Baseline JPEG encoding on the device (include/elvis_amd.h "JPEG writer"): a resident clip goes in, the
// finished entropy-coded scans come out; pixels and coefficients never visit the host, which writes the headers only
// (elvis_amd/jpeg_write.py).  csrc/jpeg_encode.h holds the rule per sample and per block, tests/_jpeg_write_ref.py states
// it in numpy, and a libjpeg-turbo PIL with optimize=False is the second oracle: same tables, same scan bytes.
//
//   jpeg_fdct_kernel     32 blocks a workgroup, 8 lanes a block.  A lane fetches one row of its block - colour
//                        conversion, edge replication and downsampling in the fetch, every pixel read clamped to the
//                        frame - and runs the row pass; the block is transposed through LDS (row pitch 9 dwords: the
//                        32 lanes of a half wave hit 32 banks in both directions); the lane runs the column pass of
//                        its column, quantises, and the zig-zag order is made by a second trip through LDS, so that a
//                        lane stores 16 contiguous bytes.  Blocks are in MCU scan order; a dummy block is transformed as
//                        the block whose DC it repeats and keeps the DC only.  int32 throughout.
//                        With a map of ROI levels (elvis_jpeg_fdct_roi) an AC coefficient that the block's coarsened
//                        step would round to zero is zeroed (jpeg_quantise_roi): one branch, uniform over the launch.
//   jpeg_bits_kernel     a lane per block: the bit length of its code from the DC difference and the AC symbols.
//                        In its tally mode (elvis_jpeg_tally) the same walk counts the symbols instead: an LDS histogram
//                        a workgroup, its non-zero entries added to the frame's with vector atomics.  The host makes
//                        a frame's own Huffman tables of it (jpeg_gen_optimal_table, csrc/jpeg_encode.h), and the
//                        _ftab entry points hand bits and pack a table set per frame (a run-time stride).
//   jpeg_scan_kernel     a workgroup per segment: exclusive prefix sum in place, kScanChunk values a step with a carry;
//                        the total goes behind the last value.  Used for the block bit offsets and the FF counts.
//   jpeg_clear_kernel    zeroes the stream words the pack kernel ORs into: no result depends on what the buffer held.
//   jpeg_pack_kernel     a lane per block: the same symbol walk, writing at the block's bit offset.  Words a block covers
//                        whole are stored, the two it may share with its neighbours are ORed (vector atomics).  The
//                        frame's last block adds the 1-fill to the byte boundary.
//   jpeg_ff_kernel       FF bytes per chunk of kStuffChunk stream bytes.
//   jpeg_sizes_kernel    per frame: stream bytes + FF bytes + 2 (EOI).
//   jpeg_stuff_kernel    every stream byte to its place in the output, a 00 behind every FF, EOI at the end.
//
// Restart intervals (elvis_jpeg_*_rst): a segment is what a frame is without them - a run of blocks that starts on a byte
// boundary with zeroed DC predictors and ends in a 1-fill - so everything behind the transform works per segment q = f *
// segs + s instead of per frame: bits is [n * segs, segb + 1] (a frame's last segment is filled up with zero lengths),
// word_off / ffc / sizes / out_off have a row or an element per segment, and the stuffing pass ends a segment with RSTm,
// m = s mod 8, or, behind a frame's last, EOI.  Without an interval segs = 1, segb = blocks: the layouts of above.
// Segments lie on grid.y, and on grid.z once there are more than 65535 of them.
//
// No kernel waits on another wave's progress.  Every global write is checked against its segment's own span.
#include <algorithm>
#include "common.h"
#include "jpeg_encode.h"

namespace {

constexpr int kFdctBlocks = 32, kFdctThreads = kFdctBlocks * 8;
constexpr int kBlockThreads = 256;     // bits and pack: a lane per block
constexpr int kScanChunk = 256;        // values of one step of the prefix sum
constexpr int kStuffChunk = 1024;      // stream bytes of one workgroup of the stuffing pass: a dword a lane
static_assert(kScanChunk == ELVIS_JPEG_SCAN_CHUNK && kStuffChunk == ELVIS_JPEG_STUFF_CHUNK, "the header names the chunks");

// frames u8 [n, h, w, channels] -> coef i16 [n, blocks, 64]; grid (blocks / 32, n).  levels: null, or the ROI map u8 [n, By,
// Bx] on a grid of B x B luma pixels, frame f's at levels + f * map_stride: the 8 lanes of a block read its level and an
// AC coefficient goes through jpeg_quantise_roi.  The branch is the same for every lane of the launch.
__global__ __launch_bounds__(kFdctThreads) void jpeg_fdct_kernel(const uint8_t* __restrict__ frames, JpegEncGeom g, int quality,
                                                                 int16_t* __restrict__ coef, const uint8_t* __restrict__ levels, int By, int Bx,
                                                                 int B, long long map_stride) {
    __shared__ int ws[kFdctBlocks][72];
    __shared__ __attribute__((aligned(16))) int16_t zz[kFdctBlocks][64];
    __shared__ uint16_t qt[128];
    const int tid = threadIdx.x, blk = tid >> 3, lane = tid & 7;
    const int b = blockIdx.x * kFdctBlocks + blk;
    const bool live = b < g.blocks;     // the last workgroup is ragged; every lane still reaches the barriers
    const size_t f = blockIdx.y;
    const uint8_t* frame = frames + f * (size_t)g.h * g.w * g.channels;
    if (tid < 128) qt[tid] = (uint16_t)jpeg_quant_value(quality, tid >> 6, tid & 63);
    JpegEncPlace p = {0, 0, 0, 0};
    if (live) {
        p = jpeg_enc_place(g, b);
        int d[8], o[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) d[x] = jpeg_enc_sample(frame, g, p.c, p.by * 8 + lane, p.bx * 8 + x) - 128;
        jpeg_fdct_pass<true>(d, o);
#pragma unroll
        for (int x = 0; x < 8; ++x) ws[blk][lane * 9 + x] = o[x];
    }
    __syncthreads();
    if (live) {
        int d[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = ws[blk][i * 9 + lane];
        jpeg_fdct_pass<false>(d, o);
        const uint16_t* table = qt + (p.c ? 64 : 0);
        if (levels == nullptr) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int nat = i * 8 + lane;
                const int q = jpeg_quantise(o[i], table[nat]);
                zz[blk][jpeg_zigzag_of(nat)] = (int16_t)((p.dummy && nat) ? 0 : q);
            }
        } else {
            const int scale16 = jpeg_roi_scale16(jpeg_roi_block_level(g, p, levels + f * (size_t)map_stride, By, Bx, B));
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int nat = i * 8 + lane;
                const int q = nat ? jpeg_quantise_roi(o[i], table[nat], scale16) : jpeg_quantise(o[i], table[nat]);
                zz[blk][jpeg_zigzag_of(nat)] = (int16_t)((p.dummy && nat) ? 0 : q);
            }
        }
    }
    __syncthreads();
    if (live) *reinterpret_cast<int4*>(coef + (f * (size_t)g.blocks + (size_t)b) * 64 + lane * 8) = *reinterpret_cast<const int4*>(&zz[blk][lane * 8]);
}

// The segment a workgroup works on: grid.y, continued on grid.z.  The same for every lane of a workgroup.
__device__ __forceinline__ size_t segment_index() { return (size_t)blockIdx.z * gridDim.y + blockIdx.y; }

// The tables of both classes into LDS; every lane of the workgroup calls it.
__device__ __forceinline__ void stage_tables(uint32_t* tab, const uint32_t* __restrict__ ehuff) {
    for (int i = threadIdx.x; i < 2 * JPGE_HUFF_WORDS; i += kBlockThreads) tab[i] = ehuff[i];
    __syncthreads();
}

// A block's coefficients as eight 16-byte loads.
__device__ __forceinline__ void load_block(const int16_t* __restrict__ src, int16_t (&zz)[64]) {
    const int4* s = reinterpret_cast<const int4*>(src);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int4 q = s[r];
        const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            zz[r * 8 + 2 * k] = (int16_t)(w[k] & 0xffff);
            zz[r * 8 + 2 * k + 1] = (int16_t)(w[k] >> 16);
        }
    }
}

// coef -> bits u32 [nseg, segb + 1]: element i of a segment is the bit length of its block i (the scan makes offsets of
// them), 0 past the blocks of a frame's last segment.  grid (segb / 256, segments).  Frame f's tables are ehuff + f *
// table_stride (0: one set for the clip).
// With `hist` (u32 [n, 2, JPGE_HUFF_WORDS], zeroed by an earlier launch) the launch tallies instead: nothing is looked up
// and no bit length written; the workgroup - it lies inside one segment, so inside one frame - counts its blocks' symbols
// in LDS and adds the entries that are not zero to its frame's histogram (vector atomics).  The branch is the same for
// every lane of the launch.
__global__ __launch_bounds__(kBlockThreads) void jpeg_bits_kernel(const int16_t* __restrict__ coef, JpegEncGeom g,
                                                                  const uint32_t* __restrict__ ehuff, long long table_stride,
                                                                  uint32_t* __restrict__ bits, int nseg, uint32_t* __restrict__ hist) {
    __shared__ uint32_t tab[2 * JPGE_HUFF_WORDS];
    const size_t q = segment_index();
    if (q >= (size_t)nseg) return;      // the whole workgroup
    const size_t f = q / (size_t)g.segs;
    const int i = blockIdx.x * kBlockThreads + threadIdx.x;
    const int b = (int)(q - f * (size_t)g.segs) * g.segb + i;
    if (hist != nullptr) {
        for (int k = threadIdx.x; k < 2 * JPGE_HUFF_WORDS; k += kBlockThreads) tab[k] = 0u;
        __syncthreads();
        if (i < g.segb && b < g.blocks) {
            const int16_t* base = coef + f * (size_t)g.blocks * 64;
            int16_t zz[64];
            load_block(base + (size_t)b * 64, zz);
            const int pb = jpeg_enc_pred_block(g, b);
            const int pred = pb >= 0 ? base[(size_t)pb * 64] : 0;
            JpegSymbolTally tally{tab + JPGE_HUFF_WORDS * jpeg_enc_table_class(g, b)};
            jpeg_encode_block(zz, pred, tab, tally);
        }
        __syncthreads();
        for (int k = threadIdx.x; k < 2 * JPGE_HUFF_WORDS; k += kBlockThreads) {
            const uint32_t v = tab[k];
            if (v) atomicAdd(hist + f * (size_t)(2 * JPGE_HUFF_WORDS) + k, v);
        }
        return;
    }
    stage_tables(tab, ehuff + f * (size_t)table_stride);
    if (i >= g.segb) return;
    if (b >= g.blocks) {
        bits[q * ((size_t)g.segb + 1) + i] = 0u;
        return;
    }
    const int16_t* base = coef + f * (size_t)g.blocks * 64;
    int16_t zz[64];
    load_block(base + (size_t)b * 64, zz);
    const int pb = jpeg_enc_pred_block(g, b);
    const int pred = pb >= 0 ? base[(size_t)pb * 64] : 0;
    JpegBitCounter count;
    jpeg_encode_block(zz, pred, tab + JPGE_HUFF_WORDS * jpeg_enc_table_class(g, b), count);
    bits[q * ((size_t)g.segb + 1) + i] = count.bits;
}

// Inclusive scan over the workgroup's kScanChunk lanes; `total` is the sum.  lds: 4 words.
__device__ __forceinline__ uint32_t workgroup_scan(uint32_t v, uint32_t* lds, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    __syncthreads();                 // the last use of lds is over
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < kScanChunk / 64; ++k) {
        const uint32_t t = lds[k];
        if (k < wave) before += t;
        total += t;
    }
    return v + before;
}

// vals u32 [rows, count + 1]: the first `count` values of a row (a segment) become their exclusive prefix sums, element
// `count` the total.  grid rows.
__global__ __launch_bounds__(kScanChunk) void jpeg_scan_kernel(uint32_t* __restrict__ vals, int count) {
    __shared__ uint32_t lds[kScanChunk / 64];
    uint32_t* p = vals + (size_t)blockIdx.x * ((size_t)count + 1);
    uint32_t carry = 0;
    for (int base = 0; base < count; base += kScanChunk) {
        const int i = base + (int)threadIdx.x;
        const uint32_t v = i < count ? p[i] : 0u;
        uint32_t total;
        const uint32_t incl = workgroup_scan(v, lds, total);
        if (i < count) p[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) p[count] = carry;
}

__global__ __launch_bounds__(256) void jpeg_clear_kernel(uint32_t* __restrict__ words, long long total_words) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total_words; i += (long long)gridDim.x * 256) words[i] = 0u;
}

// Whether segment f's span of the stream, words word_off[f] .. word_off[f + 1], lies inside the buffer.
__device__ __forceinline__ bool span_ok(const long long* __restrict__ off, size_t f, long long total) {
    return off[f] >= 0 && off[f] <= off[f + 1] && off[f + 1] <= total && off[f + 1] - off[f] < 0x40000000LL;
}

// coef, bits (offsets) -> segment q's unstuffed stream in words[word_off[q] ..]; grid (segb / 256, segments).  Frame f's
// tables are ehuff + f * table_stride (0: one set for the clip).
__global__ __launch_bounds__(kBlockThreads) void jpeg_pack_kernel(const int16_t* __restrict__ coef, JpegEncGeom g,
                                                                  const uint32_t* __restrict__ ehuff, long long table_stride,
                                                                  const uint32_t* __restrict__ bits, const long long* __restrict__ word_off,
                                                                  uint32_t* __restrict__ words, long long total_words, int nseg) {
    __shared__ uint32_t tab[2 * JPGE_HUFF_WORDS];
    const size_t q = segment_index();
    if (q >= (size_t)nseg) return;      // the whole workgroup
    const size_t f = q / (size_t)g.segs;
    stage_tables(tab, ehuff + f * (size_t)table_stride);
    const int i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= g.segb) return;
    const int b = (int)(q - f * (size_t)g.segs) * g.segb + i;
    if (b >= g.blocks || !span_ok(word_off, q, total_words)) return;
    const int16_t* base = coef + f * (size_t)g.blocks * 64;
    int16_t zz[64];
    load_block(base + (size_t)b * 64, zz);
    const int pb = jpeg_enc_pred_block(g, b);
    const int pred = pb >= 0 ? base[(size_t)pb * 64] : 0;
    JpegBitWriter out(words + word_off[q], (uint32_t)(word_off[q + 1] - word_off[q]), bits[q * ((size_t)g.segb + 1) + i]);
    jpeg_encode_block(zz, pred, tab + JPGE_HUFF_WORDS * jpeg_enc_table_class(g, b), out);
    if (i == g.segb - 1 || b == g.blocks - 1) {
        const int pad = (8 - (out.n & 7)) & 7;      // the segment's final fill: 1 bits to the byte boundary
        out.put((1u << pad) - 1u, pad);
    }
    out.flush();
}

__device__ __forceinline__ uint32_t stream_bytes(const uint32_t* __restrict__ bits, size_t f, int blocks) {
    return (bits[f * ((size_t)blocks + 1) + blocks] + 7u) >> 3;
}

// The lane's dword of the stream and how many of its bytes count; the bytes are in the dword most significant first.
__device__ __forceinline__ int lane_bytes(const uint32_t* __restrict__ words, const long long* __restrict__ word_off, size_t f,
                                          long long total_words, uint32_t nbytes, uint32_t& word) {
    const uint32_t j0 = (blockIdx.x * (uint32_t)kStuffChunk) + threadIdx.x * 4u;
    word = 0;
    if (j0 >= nbytes || !span_ok(word_off, f, total_words) || (long long)(j0 >> 2) >= word_off[f + 1] - word_off[f]) return 0;
    word = words[word_off[f] + (j0 >> 2)];
    return (int)min(4u, nbytes - j0);
}

__device__ __forceinline__ uint32_t count_ff(uint32_t word, int valid) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += (k < valid && ((word >> (24 - 8 * k)) & 0xffu) == 0xffu) ? 1u : 0u;
    return c;
}

// ffc u32 [nseg, chunks + 1]: FF bytes of every chunk of kStuffChunk stream bytes of a segment (`blocks`: the blocks of
// a row of bits); grid (chunks, segments).
__global__ __launch_bounds__(kScanChunk) void jpeg_ff_kernel(const uint32_t* __restrict__ bits, int blocks, const long long* __restrict__ word_off,
                                                             const uint32_t* __restrict__ words, long long total_words,
                                                             uint32_t* __restrict__ ffc, int chunks, int nseg) {
    __shared__ uint32_t lds[kScanChunk / 64];
    const size_t f = segment_index();
    if (f >= (size_t)nseg) return;      // the whole workgroup
    uint32_t word, total;
    const int valid = lane_bytes(words, word_off, f, total_words, stream_bytes(bits, f, blocks), word);
    workgroup_scan(count_ff(word, valid), lds, total);
    if (threadIdx.x == 0) ffc[f * ((size_t)chunks + 1) + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void jpeg_sizes_kernel(const uint32_t* __restrict__ bits, int blocks, const uint32_t* __restrict__ ffc,
                                                         int chunks, uint32_t* __restrict__ sizes, int n) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < n) sizes[f] = stream_bytes(bits, f, blocks) + ffc[(size_t)f * ((size_t)chunks + 1) + chunks] + 2u;
}

// The stream bytes of segment f to out[out_off[f] ..], a 00 behind every FF, then what ends the segment: FF and RSTm
// (m = s mod 8 for a frame's segment s) or, behind the last of its `segs`, EOI; grid (chunks, segments).
__global__ __launch_bounds__(kScanChunk) void jpeg_stuff_kernel(const uint32_t* __restrict__ bits, int blocks, const long long* __restrict__ word_off,
                                                                const uint32_t* __restrict__ words, long long total_words,
                                                                const uint32_t* __restrict__ ffc, int chunks,
                                                                const long long* __restrict__ out_off, uint8_t* __restrict__ out,
                                                                long long out_bytes, JpegEncGeom g, int nseg) {
    __shared__ uint32_t lds[kScanChunk / 64];
    const size_t f = segment_index();
    if (f >= (size_t)nseg) return;      // the whole workgroup
    const uint32_t nbytes = stream_bytes(bits, f, blocks);
    uint32_t word, total;
    const int valid = lane_bytes(words, word_off, f, total_words, nbytes, word);
    const uint32_t mine = count_ff(word, valid);
    const uint32_t before = workgroup_scan(mine, lds, total) - mine;
    if (!span_ok(out_off, f, out_bytes)) return;
    const long long first = out_off[f], end = out_off[f + 1];
    const uint32_t* fc = ffc + f * ((size_t)chunks + 1);
    long long at = first + (long long)blockIdx.x * kStuffChunk + threadIdx.x * 4 + fc[blockIdx.x] + before;
    for (int k = 0; k < valid; ++k) {
        const uint32_t byte = (word >> (24 - 8 * k)) & 0xffu;
        if (at < end) out[at] = (uint8_t)byte;
        ++at;
        if (byte == 0xffu) {
            if (at < end) out[at] = 0;
            ++at;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const long long eoi = first + nbytes + fc[chunks];
        if (eoi >= first && eoi + 2 <= end) {
            out[eoi] = 0xff;
            out[eoi + 1] = (uint8_t)jpeg_enc_seg_marker(g, (int)(f % (size_t)g.segs));
        }
    }
}

// The argument checks every entry point shares; the geometry comes out.
int check_shape(const char* who, int n, int h, int w, int channels, int sampling, JpegEncGeom& g) {
    ELVIS_REQUIRE(channels == 1 || channels == 3, "%s: channels must be 1 or 3, got %d", who, channels);
    ELVIS_REQUIRE(sampling >= JPGE_SAMPLING_444 && sampling <= JPGE_SAMPLING_420, "%s: sampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), got %d", who,
                  sampling);
    ELVIS_REQUIRE(n >= 0 && n <= 65535 && h >= 1 && w >= 1 && h <= 65535 && w <= 65535, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    ELVIS_REQUIRE(((long long)((w + 7) / 8 + 1) * ((h + 7) / 8 + 1)) * 3 <= JPGE_MAX_BLOCKS, "%s: a %d x %d frame has more than 2^20 blocks", who, h, w);
    g = jpeg_enc_geometry(h, w, channels, 0, sampling);
    return ELVIS_OK;
}

// The interval of the restart forms: the geometry gets its segments, `nseg` the segments of the clip.
int check_restart(const char* who, int n, int restart_mcus, JpegEncGeom& g, int& nseg) {
    ELVIS_REQUIRE(restart_mcus >= 0 && restart_mcus <= 65535, "%s: restart_mcus must be in [0, 65535], got %d", who, restart_mcus);
    g = jpeg_enc_restart(g, restart_mcus);
    ELVIS_REQUIRE((long long)n * g.segs <= ELVIS_JPEG_MAX_SEGMENTS, "%s: %d frames of %d restart intervals are more than %d segments", who, n, g.segs,
                  ELVIS_JPEG_MAX_SEGMENTS);
    nseg = n * g.segs;
    return ELVIS_OK;
}

// Segments on grid.y and, past 65535 of them, on grid.z: every kernel drops the segments at and past nseg.
dim3 segment_grid(int x, int nseg) {
    const int gy = std::min(nseg, 65535);
    return dim3((unsigned)x, (unsigned)gy, (unsigned)cdiv(nseg, gy));
}

// The three calls behind the transform; the entry points without an interval are their restart_mcus = 0.
int bits_call(const char* who, const int16_t* coef, const uint32_t* ehuff, uint32_t* bits, int n, int h, int w, int channels, int sampling,
              int restart_mcus, elvis_stream_t stream, long long table_stride = 0) {
    JpegEncGeom g;
    int nseg = 0;
    if (int rc = check_shape(who, n, h, w, channels, sampling, g)) return rc;
    if (int rc = check_restart(who, n, restart_mcus, g, nseg)) return rc;
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(coef && ehuff && bits, "%s: null pointer", who);
    ELVIS_REQUIRE(((uintptr_t)coef & 15) == 0 && ((uintptr_t)bits & 3) == 0 && ((uintptr_t)ehuff & 3) == 0,
                  "%s: coef must be 16-byte aligned, ehuff and bits 4-byte aligned", who);
    hipLaunchKernelGGL(jpeg_bits_kernel, segment_grid(cdiv(g.segb, kBlockThreads), nseg), dim3(kBlockThreads), 0, (hipStream_t)stream, coef, g, ehuff,
                       table_stride, bits, nseg, (uint32_t*)nullptr);
    ELVIS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)nseg), dim3(kScanChunk), 0, (hipStream_t)stream, bits, g.segb);
    ELVIS_CHECK_LAUNCH(who);
    elvis_note_launch("jpeg_bits_kernel");
    return ELVIS_OK;
}

int pack_call(const char* who, const int16_t* coef, const uint32_t* ehuff, const uint32_t* bits, const int64_t* word_off, uint32_t* words,
              int64_t total_words, uint32_t* ffc, int chunks, uint32_t* sizes, int n, int h, int w, int channels, int sampling, int restart_mcus,
              elvis_stream_t stream, long long table_stride = 0) {
    JpegEncGeom g;
    int nseg = 0;
    if (int rc = check_shape(who, n, h, w, channels, sampling, g)) return rc;
    if (int rc = check_restart(who, n, restart_mcus, g, nseg)) return rc;
    ELVIS_REQUIRE(total_words >= 0 && total_words < (1LL << 38), "%s: total_words must be in [0, 2^38)", who);
    ELVIS_REQUIRE(chunks >= 1 && chunks <= 65535 * 32, "%s: chunks must be in [1, 2^21), got %d", who, chunks);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(coef && ehuff && bits && word_off && words && ffc && sizes, "%s: null pointer", who);
    ELVIS_REQUIRE(((uintptr_t)coef & 15) == 0 && (((uintptr_t)bits | (uintptr_t)ehuff | (uintptr_t)words | (uintptr_t)ffc | (uintptr_t)sizes) & 3) == 0 &&
                      ((uintptr_t)word_off & 7) == 0,
                  "%s: coef must be 16-byte, word_off 8-byte, the other buffers 4-byte aligned", who);
    hipLaunchKernelGGL(jpeg_clear_kernel, dim3((unsigned)std::max(1, std::min(4096, cdiv(total_words, 256)))), dim3(256), 0, (hipStream_t)stream, words,
                       (long long)total_words);
    ELVIS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(jpeg_pack_kernel, segment_grid(cdiv(g.segb, kBlockThreads), nseg), dim3(kBlockThreads), 0, (hipStream_t)stream, coef, g, ehuff,
                       table_stride, bits, (const long long*)word_off, words, (long long)total_words, nseg);
    ELVIS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(jpeg_ff_kernel, segment_grid(chunks, nseg), dim3(kScanChunk), 0, (hipStream_t)stream, bits, g.segb, (const long long*)word_off,
                       (const uint32_t*)words, (long long)total_words, ffc, chunks, nseg);
    ELVIS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)nseg), dim3(kScanChunk), 0, (hipStream_t)stream, ffc, chunks);
    ELVIS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(jpeg_sizes_kernel, dim3((unsigned)cdiv(nseg, 256)), dim3(256), 0, (hipStream_t)stream, bits, g.segb, (const uint32_t*)ffc, chunks,
                       sizes, nseg);
    ELVIS_CHECK_LAUNCH(who);
    elvis_note_launch("jpeg_pack_kernel");
    return ELVIS_OK;
}

// The tally: the histograms are zeroed by the library, then jpeg_bits_kernel runs in its tally mode over the grid of the
// bit count.
int tally_call(const char* who, const int16_t* coef, uint32_t* hist, int n, int h, int w, int channels, int sampling, int restart_mcus,
               elvis_stream_t stream) {
    JpegEncGeom g;
    int nseg = 0;
    if (int rc = check_shape(who, n, h, w, channels, sampling, g)) return rc;
    if (int rc = check_restart(who, n, restart_mcus, g, nseg)) return rc;
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(coef && hist, "%s: null pointer", who);
    ELVIS_REQUIRE(((uintptr_t)coef & 15) == 0 && ((uintptr_t)hist & 3) == 0, "%s: coef must be 16-byte aligned, hist 4-byte aligned", who);
    const long long hist_words = (long long)n * 2 * JPGE_HUFF_WORDS;
    hipLaunchKernelGGL(jpeg_clear_kernel, dim3((unsigned)std::max(1, std::min(4096, cdiv(hist_words, 256)))), dim3(256), 0, (hipStream_t)stream, hist,
                       hist_words);
    ELVIS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(jpeg_bits_kernel, segment_grid(cdiv(g.segb, kBlockThreads), nseg), dim3(kBlockThreads), 0, (hipStream_t)stream, coef, g,
                       (const uint32_t*)nullptr, 0LL, (uint32_t*)nullptr, nseg, hist);
    ELVIS_CHECK_LAUNCH(who);
    elvis_note_launch("jpeg_bits_kernel");
    return ELVIS_OK;
}

int stuff_call(const char* who, const uint32_t* bits, const int64_t* word_off, const uint32_t* words, int64_t total_words, const uint32_t* ffc, int chunks,
               const int64_t* out_off, uint8_t* out, int64_t out_bytes, int n, int h, int w, int channels, int sampling, int restart_mcus,
               elvis_stream_t stream) {
    JpegEncGeom g;
    int nseg = 0;
    if (int rc = check_shape(who, n, h, w, channels, sampling, g)) return rc;
    if (int rc = check_restart(who, n, restart_mcus, g, nseg)) return rc;
    ELVIS_REQUIRE(total_words >= 0 && total_words < (1LL << 38), "%s: total_words must be in [0, 2^38)", who);
    ELVIS_REQUIRE(out_bytes >= 0 && out_bytes < (1LL << 40), "%s: out_bytes must be in [0, 2^40)", who);
    ELVIS_REQUIRE(chunks >= 1 && chunks <= 65535 * 32, "%s: chunks must be in [1, 2^21), got %d", who, chunks);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(bits && word_off && words && ffc && out_off && out, "%s: null pointer", who);
    ELVIS_REQUIRE((((uintptr_t)bits | (uintptr_t)words | (uintptr_t)ffc) & 3) == 0 && (((uintptr_t)word_off | (uintptr_t)out_off) & 7) == 0,
                  "%s: word_off and out_off must be 8-byte, bits, words and ffc 4-byte aligned", who);
    hipLaunchKernelGGL(jpeg_stuff_kernel, segment_grid(chunks, nseg), dim3(kScanChunk), 0, (hipStream_t)stream, bits, g.segb, (const long long*)word_off,
                       words, (long long)total_words, ffc, chunks, (const long long*)out_off, out, (long long)out_bytes, g, nseg);
    ELVIS_CHECK_LAUNCH(who);
    elvis_note_launch("jpeg_stuff_kernel");
    return ELVIS_OK;
}

// The transform: without a map (levels null, by = bx = block_size = 0) the path of elvis_jpeg_fdct.  With one, the grid
// must be one of the two a frame has - floored, max(1, h / B) x max(1, w / B), or full, ceil(h / B) x ceil(w / B) - in
// each axis on its own, so that no cell index the kernel clamps to lies outside the map.
int fdct_call(const char* who, const uint8_t* frames, int16_t* coef, int n, int h, int w, int channels, int order, int quality, int sampling,
              const uint8_t* levels, int by, int bx, int block_size, elvis_stream_t stream) {
    JpegEncGeom g;
    if (int rc = check_shape(who, n, h, w, channels, sampling, g)) return rc;
    ELVIS_REQUIRE(order == 0 || order == 1, "%s: order must be 0 (rgb) or 1 (bgr), got %d", who, order);
    ELVIS_REQUIRE(quality >= 1 && quality <= 100, "%s: quality must be in [1, 100], got %d", who, quality);
    if (levels == nullptr) {
        ELVIS_REQUIRE(by == 0 && bx == 0 && block_size == 0, "%s: null map with by=%d bx=%d block_size=%d (all 0 without a map)", who, by, bx, block_size);
    } else {
        ELVIS_REQUIRE(block_size >= 8 && block_size % 8 == 0, "%s: block_size must be a positive multiple of 8, got %d", who, block_size);
        ELVIS_REQUIRE(by == std::max(1, h / block_size) || by == cdiv(h, block_size),
                      "%s: a map of %d rows is not the grid of a frame of %d rows in blocks of %d (%d or %d)", who, by, h, block_size,
                      std::max(1, h / block_size), cdiv(h, block_size));
        ELVIS_REQUIRE(bx == std::max(1, w / block_size) || bx == cdiv(w, block_size),
                      "%s: a map of %d columns is not the grid of a frame of %d columns in blocks of %d (%d or %d)", who, bx, w, block_size,
                      std::max(1, w / block_size), cdiv(w, block_size));
    }
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(frames && coef, "%s: null pointer", who);
    ELVIS_REQUIRE(((uintptr_t)coef & 15) == 0, "%s: coef must be 16-byte aligned", who);
    g.bgr = order;
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((unsigned)cdiv(g.blocks, kFdctBlocks), (unsigned)n), dim3(kFdctThreads), 0, (hipStream_t)stream, frames, g,
                       quality, coef, levels, by, bx, block_size, (long long)by * bx);
    ELVIS_CHECK_LAUNCH(who);
    elvis_note_launch("jpeg_fdct_kernel");
    return ELVIS_OK;
}

}  // namespace

extern "C" int elvis_jpeg_frame_blocks(int h, int w, int channels, int sampling) {
    JpegEncGeom g;
    if (check_shape("elvis_jpeg_frame_blocks", 0, h, w, channels, sampling, g) != ELVIS_OK) return 0;
    return g.blocks;
}

extern "C" int elvis_jpeg_fdct(const uint8_t* frames, int16_t* coef, int n, int h, int w, int channels, int order, int quality, int sampling,
                               elvis_stream_t stream) {
    return fdct_call("elvis_jpeg_fdct", frames, coef, n, h, w, channels, order, quality, sampling, nullptr, 0, 0, 0, stream);
}

extern "C" int elvis_jpeg_fdct_roi(const uint8_t* frames, int16_t* coef, int n, int h, int w, int channels, int order, int quality, int sampling,
                                   const uint8_t* levels, int by, int bx, int block_size, elvis_stream_t stream) {
    return fdct_call("elvis_jpeg_fdct_roi", frames, coef, n, h, w, channels, order, quality, sampling, levels, by, bx, block_size, stream);
}

extern "C" int elvis_jpeg_segments(int h, int w, int channels, int sampling, int restart_mcus) {
    JpegEncGeom g;
    int nseg = 0;
    if (check_shape("elvis_jpeg_segments", 0, h, w, channels, sampling, g) != ELVIS_OK) return 0;
    if (check_restart("elvis_jpeg_segments", 0, restart_mcus, g, nseg) != ELVIS_OK) return 0;
    return g.segs;
}

extern "C" int elvis_jpeg_bits(const int16_t* coef, const uint32_t* ehuff, uint32_t* bits, int n, int h, int w, int channels, int sampling,
                               elvis_stream_t stream) {
    return bits_call("elvis_jpeg_bits", coef, ehuff, bits, n, h, w, channels, sampling, 0, stream);
}

extern "C" int elvis_jpeg_bits_rst(const int16_t* coef, const uint32_t* ehuff, uint32_t* bits, int n, int h, int w, int channels, int sampling,
                                   int restart_mcus, elvis_stream_t stream) {
    return bits_call("elvis_jpeg_bits_rst", coef, ehuff, bits, n, h, w, channels, sampling, restart_mcus, stream);
}

extern "C" int elvis_jpeg_pack(const int16_t* coef, const uint32_t* ehuff, const uint32_t* bits, const int64_t* word_off, uint32_t* words,
                               int64_t total_words, uint32_t* ffc, int chunks, uint32_t* sizes, int n, int h, int w, int channels, int sampling,
                               elvis_stream_t stream) {
    return pack_call("elvis_jpeg_pack", coef, ehuff, bits, word_off, words, total_words, ffc, chunks, sizes, n, h, w, channels, sampling, 0, stream);
}

extern "C" int elvis_jpeg_pack_rst(const int16_t* coef, const uint32_t* ehuff, const uint32_t* bits, const int64_t* word_off, uint32_t* words,
                                   int64_t total_words, uint32_t* ffc, int chunks, uint32_t* sizes, int n, int h, int w, int channels, int sampling,
                                   int restart_mcus, elvis_stream_t stream) {
    return pack_call("elvis_jpeg_pack_rst", coef, ehuff, bits, word_off, words, total_words, ffc, chunks, sizes, n, h, w, channels, sampling, restart_mcus,
                     stream);
}

extern "C" int elvis_jpeg_stuff(const uint32_t* bits, const int64_t* word_off, const uint32_t* words, int64_t total_words, const uint32_t* ffc,
                                int chunks, const int64_t* out_off, uint8_t* out, int64_t out_bytes, int n, int h, int w, int channels,
                                int sampling, elvis_stream_t stream) {
    return stuff_call("elvis_jpeg_stuff", bits, word_off, words, total_words, ffc, chunks, out_off, out, out_bytes, n, h, w, channels, sampling, 0, stream);
}

extern "C" int elvis_jpeg_stuff_rst(const uint32_t* bits, const int64_t* word_off, const uint32_t* words, int64_t total_words, const uint32_t* ffc,
                                    int chunks, const int64_t* out_off, uint8_t* out, int64_t out_bytes, int n, int h, int w, int channels,
                                    int sampling, int restart_mcus, elvis_stream_t stream) {
    return stuff_call("elvis_jpeg_stuff_rst", bits, word_off, words, total_words, ffc, chunks, out_off, out, out_bytes, n, h, w, channels, sampling,
                      restart_mcus, stream);
}

// ----------------------------------------------------------------------------- per-frame optimised tables
extern "C" int elvis_jpeg_tally(const int16_t* coef, uint32_t* hist, int n, int h, int w, int channels, int sampling, int restart_mcus,
                                elvis_stream_t stream) {
    return tally_call("elvis_jpeg_tally", coef, hist, n, h, w, channels, sampling, restart_mcus, stream);
}

extern "C" int elvis_jpeg_bits_ftab(const int16_t* coef, const uint32_t* ehuff, uint32_t* bits, int n, int h, int w, int channels, int sampling,
                                    int restart_mcus, elvis_stream_t stream) {
    return bits_call("elvis_jpeg_bits_ftab", coef, ehuff, bits, n, h, w, channels, sampling, restart_mcus, stream, 2 * JPGE_HUFF_WORDS);
}

extern "C" int elvis_jpeg_pack_ftab(const int16_t* coef, const uint32_t* ehuff, const uint32_t* bits, const int64_t* word_off, uint32_t* words,
                                    int64_t total_words, uint32_t* ffc, int chunks, uint32_t* sizes, int n, int h, int w, int channels, int sampling,
                                    int restart_mcus, elvis_stream_t stream) {
    return pack_call("elvis_jpeg_pack_ftab", coef, ehuff, bits, word_off, words, total_words, ffc, chunks, sizes, n, h, w, channels, sampling, restart_mcus,
                     stream, 2 * JPGE_HUFF_WORDS);
}

// Host only: jpeg_gen_optimal_table of jchuff.c per frame and table (csrc/jpeg_encode.h).  No device is touched.
extern "C" int elvis_jpeg_optimal_tables(const uint32_t* hist, int n, int channels, uint8_t* counts, uint8_t* symbols, int32_t* nsym, uint32_t* ehuff) {
    const char* who = "elvis_jpeg_optimal_tables";
    ELVIS_REQUIRE(channels == 1 || channels == 3, "%s: channels must be 1 or 3, got %d", who, channels);
    ELVIS_REQUIRE(n >= 0 && n <= 65535, "%s: n must be in [0, 65535], got %d", who, n);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(hist && counts && symbols && nsym && ehuff, "%s: null pointer", who);
    for (int f = 0; f < n; ++f) {
        const uint32_t* hf = hist + (size_t)f * 2 * JPGE_HUFF_WORDS;
        for (int k = 0; k < 2 * JPGE_HUFF_WORDS; ++k)
            ELVIS_REQUIRE(hf[k] <= (uint32_t)JPGE_MAX_BLOCKS * 64u, "%s: frame %d counts %u at entry %d, above 2^26", who, f, hf[k], k);
        int nsym4[4];
        const int bad = jpeg_frame_optimal_tables(hf, channels == 3 ? 2 : 1, counts + (size_t)f * 64, symbols + (size_t)f * 1024, nsym4,
                                                  ehuff + (size_t)f * 2 * JPGE_HUFF_WORDS);
        for (int k = 0; k < 4; ++k) nsym[(size_t)f * 4 + k] = nsym4[k];
        ELVIS_REQUIRE(bad == 0, "%s: frame %d has no symbol for its %s table %d (or a code longer than 32 bits before limiting)", who, f,
                      (bad - 1) & 1 ? "AC" : "DC", (bad - 1) >> 1);
    }
    return ELVIS_OK;
}
