// The baseline JPEG entropy decoder of csrc/jpeg_read.hip, host and device: the frame descriptor's check, the code
// tables' build from (counts, values), the bit reader and the decode of one entropy-coded segment (ITU-T T.81 F.2.2),
// written once.  On the device a lane decodes a segment; on the host the same text is plain C++, so that
// tools/jpeg_decode_check.cpp walks the very code of the kernels over exact-size buffers under the address and
// undefined-behaviour sanitizers.  tests/_jpeg_ref.py states what it computes.
//
// Rules kept by every loop here: an iteration consumes at least one input bit, or finishes a block, or ends; input
// bytes are capped by the segment's length (bits past its end are never invented: JPG_E_BITS); every table index goes
// through a mask; every store goes to a block of the segment's own MCUs, inside the frame's span of the buffer.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPG_HD __host__ __device__ __forceinline__
#else
#define JPG_HD static inline
#endif

// Status codes of a segment; the first defect ends it.
#define JPG_OK 0
#define JPG_E_CODE 1      // no code of up to 16 bits matches
#define JPG_E_INDEX 2     // a coefficient index past 63
#define JPG_E_BITS 3      // the bits run out before the segment's MCUs are done
#define JPG_E_RANGE 4     // a dequantised coefficient outside [-32768, 32767]
#define JPG_E_DESC 5      // the segment or its frame descriptor does not fit its buffers (nothing is touched)

#define JPG_FAST_BITS 9
#define JPG_FD_WORDS 32
#define JPG_SEG_WORDS 5
#define JPG_HUFF_BYTES 272          // 16 counts, 256 values
#define JPG_TABLES 8                // per frame: DC tables 0..3, AC tables 0..3

// The frame descriptor, int32 [32]: 0 components (1 | 3), 1 hmax, 2 vmax, 3 MCUs per row, 4 MCU rows, 5 blocks of the
// frame, 6..7 zero; per component c at 8 + 8 c: h, v, first block, first plane byte, plane pitch, DC table, AC table,
// quantisation table.  A component's blocks are a row-major grid of (MCU rows * v) x (MCUs per row * h); its plane is
// that grid in samples, 64 bytes a block.
#define JPG_FD_COMP(fd, c) ((fd) + 8 + 8 * (c))

struct JpegTable {
    uint16_t fast[1 << JPG_FAST_BITS];   // (symbol << 4) | code length for codes of up to 9 bits, by the next 9 bits; 0 = none
    uint16_t count[16];                  // codes of each length 1..16
    uint8_t values[256];                 // symbols in canonical order
};

// zig-zag position -> natural index without a table in memory: eight positions to a 64-bit constant, six bits each
JPG_HD int jpeg_natural(int k) {
    const uint64_t packed[8] = {
        0ull | 1ull << 6 | 8ull << 12 | 16ull << 18 | 9ull << 24 | 2ull << 30 | 3ull << 36 | 10ull << 42,
        17ull | 24ull << 6 | 32ull << 12 | 25ull << 18 | 18ull << 24 | 11ull << 30 | 4ull << 36 | 5ull << 42,
        12ull | 19ull << 6 | 26ull << 12 | 33ull << 18 | 40ull << 24 | 48ull << 30 | 41ull << 36 | 34ull << 42,
        27ull | 20ull << 6 | 13ull << 12 | 6ull << 18 | 7ull << 24 | 14ull << 30 | 21ull << 36 | 28ull << 42,
        35ull | 42ull << 6 | 49ull << 12 | 56ull << 18 | 57ull << 24 | 50ull << 30 | 43ull << 36 | 36ull << 42,
        29ull | 22ull << 6 | 15ull << 12 | 23ull << 18 | 30ull << 24 | 37ull << 30 | 44ull << 36 | 51ull << 42,
        58ull | 59ull << 6 | 52ull << 12 | 45ull << 18 | 38ull << 24 | 31ull << 30 | 39ull << 36 | 46ull << 42,
        53ull | 60ull << 6 | 61ull << 12 | 54ull << 18 | 47ull << 24 | 55ull << 30 | 62ull << 36 | 63ull << 42};
    k &= 63;
    const int g = k >> 3;
    // a chain of selects, not an indexed load: the constants stay in registers
    uint64_t w = packed[0];
    w = g == 1 ? packed[1] : w;
    w = g == 2 ? packed[2] : w;
    w = g == 3 ? packed[3] : w;
    w = g == 4 ? packed[4] : w;
    w = g == 5 ? packed[5] : w;
    w = g == 6 ? packed[6] : w;
    w = g == 7 ? packed[7] : w;
    return (int)((w >> (6 * (k & 7))) & 63);
}

// Whether a frame descriptor fits buffers of `stride_blocks` coefficient blocks (and 64 plane bytes a block) a frame.
JPG_HD bool jpeg_fd_ok(const int32_t* fd, long long stride_blocks) {
    const int ncomp = fd[0], hmax = fd[1], vmax = fd[2];
    const long long mcux = fd[3], mcuy = fd[4];
    if (!(ncomp == 1 || ncomp == 3) || hmax < 1 || hmax > 2 || vmax < 1 || vmax > hmax) return false;   // 1x1, 2x1, 2x2
    if (mcux < 1 || mcuy < 1 || mcux > 65535 || mcuy > 65535 || stride_blocks < 1 || stride_blocks >= (1ll << 31) / 64) return false;
    long long at = 0;
    for (int c = 0; c < ncomp; ++c) {
        const int32_t* cd = JPG_FD_COMP(fd, c);
        const long long h = cd[0], v = cd[1];
        if (h != (c == 0 ? hmax : 1) || v != (c == 0 ? vmax : 1)) return false;
        if (cd[2] != at || cd[3] != at * 64 || cd[4] != mcux * h * 8) return false;
        if (cd[5] < 0 || cd[5] > 3 || cd[6] < 0 || cd[6] > 3 || cd[7] < 0 || cd[7] > 3) return false;
        at += mcux * h * mcuy * v;
        if (at > stride_blocks) return false;
    }
    return fd[5] == at;
}

// One table from 16 counts and up to 256 values; `spec` is JPG_HUFF_BYTES bytes.  Counts that over-subscribe the code
// space or sum past 256 are cut off where they do (the host refuses such a file; here they must only be harmless).
JPG_HD void jpeg_build_table(JpegTable* t, const uint8_t* spec) {
    for (int i = 0; i < (1 << JPG_FAST_BITS); ++i) t->fast[i] = 0;
    for (int i = 0; i < 256; ++i) t->values[i] = spec[16 + i];
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        int n = spec[len - 1];
        if (n > 256 - k) n = 256 - k;
        if (n > (1 << len) - code) n = (1 << len) - code;
        if (n < 0) n = 0;
        t->count[len - 1] = (uint16_t)n;
        if (len <= JPG_FAST_BITS) {
            for (int j = 0; j < n; ++j) {
                const int first = (code + j) << (JPG_FAST_BITS - len);
                for (int e = 0; e < (1 << (JPG_FAST_BITS - len)); ++e)
                    t->fast[(first + e) & ((1 << JPG_FAST_BITS) - 1)] = (uint16_t)((int)spec[16 + ((k + j) & 255)] << 4 | len);
            }
        }
        code = (code + n) << 1;
        k += n;
    }
}

struct JpegBits {
    const uint8_t* src;
    uint32_t len, pos;     // bytes of the segment, bytes taken
    uint64_t hold;         // the next bits, the first at bit 63
    int nbits;
};

// Tops the hold up to at least 57 bits while the segment has bytes.  FF 00 is one FF; an FF in front of anything else,
// or at the very end, ends the data.  A byte a load: a variant that loaded the next 8 bytes at once into a register
// and took them from there was measured slower on an MI355X and is not kept.
JPG_HD void jpeg_fill(JpegBits& b) {
    while (b.nbits <= 56 && b.pos < b.len) {
        const uint32_t v = b.src[b.pos];
        if (v == 0xFF) {
            if (b.pos + 1 < b.len && b.src[b.pos + 1] == 0) {
                b.pos += 2;
            } else {
                b.len = b.pos;
                break;
            }
        } else {
            b.pos += 1;
        }
        b.hold |= (uint64_t)v << (56 - b.nbits);
        b.nbits += 8;
    }
}

// One Huffman symbol, or -JPG_E_BITS / -JPG_E_CODE.  After jpeg_fill the hold has at least 57 bits unless the segment is at its end.
JPG_HD int jpeg_symbol(JpegBits& b, const JpegTable* t) {
    const uint32_t peek = (uint32_t)(b.hold >> 48);   // 16 bits, zeros behind the last real one
    const uint32_t e = t->fast[(peek >> (16 - JPG_FAST_BITS)) & ((1 << JPG_FAST_BITS) - 1)];
    if (e) {
        const int len = (int)(e & 15);
        if (len > b.nbits) return -JPG_E_BITS;
        b.hold <<= len;
        b.nbits -= len;
        return (int)(e >> 4);
    }
    // the canonical walk, one bit a step: `first` is the first code of the length, `index` its place among the values
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 16; ++len) {
        if (len > b.nbits) return -JPG_E_BITS;
        code |= (int)((peek >> (16 - len)) & 1);
        const int n = t->count[len - 1];
        if (code - n < first) {
            b.hold <<= len;
            b.nbits -= len;
            return t->values[(index + (code - first)) & 255];
        }
        index += n;
        first = (first + n) << 1;
        code <<= 1;
    }
    return -JPG_E_CODE;
}

// The value of category t (1..15) from the next t bits; the caller has checked that they are there.
JPG_HD int jpeg_receive_extend(JpegBits& b, int t) {
    const int v = (int)(b.hold >> (64 - t));
    b.hold <<= t;
    b.nbits -= t;
    return v >= (1 << (t - 1)) ? v : v - (1 << t) + 1;
}

// One segment: MCUs [first, first + count) of the frame `fd` (checked by jpeg_fd_ok) from src[0, len), dequantised int16
// coefficients in natural order into `coef`, the frame's `stride_blocks` blocks (zero before the call).  tables: the
// frame's JPG_TABLES tables; qt: its four quantisation tables, uint16 [4][64] in natural order.  status[0] = code,
// status[1] = MCUs done.
JPG_HD void jpeg_decode_segment(const uint8_t* src, uint32_t len, const int32_t* fd, const JpegTable* tables, const uint16_t* qt,
                                int first, int count, int16_t* coef, long long stride_blocks, uint32_t* status) {
    const int ncomp = fd[0], mcux = fd[3];
    const long long total = (long long)fd[3] * fd[4];
    int code = JPG_OK, done = 0;
    if (first < 0 || count < 0 || (long long)first + count > total) {
        status[0] = JPG_E_DESC;
        status[1] = 0;
        return;
    }
    JpegBits b;
    b.src = src;
    b.len = len;
    b.pos = 0;
    b.hold = 0;
    b.nbits = 0;
    long long pred0 = 0, pred1 = 0, pred2 = 0;
    for (int m = first; m < first + count && code == JPG_OK; ++m) {
        const int my = m / mcux, mx = m - my * mcux;
        for (int c = 0; c < ncomp && code == JPG_OK; ++c) {
            const int32_t* cd = JPG_FD_COMP(fd, c);
            const int h = cd[0], v = cd[1];
            const JpegTable* dc = tables + (cd[5] & 3);
            const JpegTable* ac = tables + 4 + (cd[6] & 3);
            const uint16_t* q = qt + 64 * (cd[7] & 3);
            for (int sub = 0; sub < h * v && code == JPG_OK; ++sub) {
                const int vy = sub / h, hx = sub - vy * h;
                const long long blk = (long long)cd[2] + (long long)(my * v + vy) * ((long long)mcux * h) + (mx * h + hx);
                const bool inside = blk >= 0 && blk < stride_blocks;   // always, for a descriptor that jpeg_fd_ok passed
                int16_t* out = coef + (inside ? blk : 0) * 64;
                // DC
                jpeg_fill(b);
                int s = jpeg_symbol(b, dc);
                if (s < 0) {
                    code = -s;
                    break;
                }
                const int t = s & 15;
                int diff = 0;
                if (t) {
                    jpeg_fill(b);
                    if (t > b.nbits) {
                        code = JPG_E_BITS;
                        break;
                    }
                    diff = jpeg_receive_extend(b, t);
                }
                long long pred = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
                pred += diff;
                if (c == 0) pred0 = pred;
                else if (c == 1) pred1 = pred;
                else pred2 = pred;
                const long long dcv = pred * (long long)q[0];
                if (dcv < -32768 || dcv > 32767) {
                    code = JPG_E_RANGE;
                    break;
                }
                if (inside) out[0] = (int16_t)dcv;
                // AC
                int k = 1;
                while (k <= 63) {
                    jpeg_fill(b);
                    s = jpeg_symbol(b, ac);
                    if (s < 0) {
                        code = -s;
                        break;
                    }
                    const int r = s >> 4, size = s & 15;
                    if (size == 0) {
                        if (r != 15) break;   // end of block
                        k += 16;
                        continue;
                    }
                    k += r;
                    if (k > 63) {
                        code = JPG_E_INDEX;
                        break;
                    }
                    jpeg_fill(b);
                    if (size > b.nbits) {
                        code = JPG_E_BITS;
                        break;
                    }
                    const int nat = jpeg_natural(k);
                    const int val = jpeg_receive_extend(b, size) * (int)q[nat];   // |.| < 2^15 * 2^16
                    if (val < -32768 || val > 32767) {
                        code = JPG_E_RANGE;
                        break;
                    }
                    if (inside) out[nat] = (int16_t)val;
                    ++k;
                }
            }
        }
        if (code == JPG_OK) ++done;
    }
    status[0] = (uint32_t)code;
    status[1] = (uint32_t)done;
}
