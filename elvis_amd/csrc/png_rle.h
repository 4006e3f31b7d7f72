// The token rule of the PNG writer's run-length deflate (csrc/png.hip png_stats_rle_kernel / png_pack_rle_kernel, DESIGN.md
// 7, include/elvis_amd.h "PNG writer"), host and device, written once: which position of a span emits a literal, which a
// match and which nothing, and the symbol, extra value and extra count of a match length.  The kernels call rle_token_at
// with the run offsets they get from a workgroup scan; tools/png_rle_check.cpp walks rle_span_token, which finds the same
// offsets by looking left and right in the span, over exact-size buffers under the address and undefined-behaviour
// sanitizers and compares the tokens with the statement's (tests/_png_rle_ref.py).
//
// The rule.  A row's filtered bytes are cut into spans of RLE_SPAN bytes, each tokenised on its own.  A run is a maximal
// sequence of equal bytes inside a span.  A run of length L and value v is: the literal v; with R = L - 1, R / 258
// matches of length 258; with r = R % 258 one match of length r if r >= 3, else r literals v.  Every match has distance 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RLE_HD __host__ __device__ __forceinline__
#else
#define RLE_HD static inline
#endif

#define RLE_SPAN 4096          // bytes tokenised on their own: the pack kernel's staging tile
#define RLE_MIN_MATCH 3
#define RLE_MAX_MATCH 258
#define RLE_SYMBOLS 286        // literals 0..255, EOB 256, lengths 257..285
#define RLE_NOTHING 0
#define RLE_LITERAL 1
#define RLE_MATCH 2

struct RleToken {
    int kind;     // RLE_NOTHING (the position is covered by a match), RLE_LITERAL or RLE_MATCH
    int symbol;   // the byte value of a literal, 257..285 of a match
    int extra;    // a match's extra value, sent LSB first behind its code
    int nextra;   // and how many bits of it, 0..5
};

// RFC 1951 3.2.5: the length symbols 257..285, their base lengths and extra bit counts.  rle_length_symbol below is the
// same table in arithmetic (the kernels index no table); the host check compares the two on every length.
static const uint16_t kRleLengthBase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                            31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t kRleLengthExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};

// The symbol of match length `len` in [3, 258] with its extra value and count.  258 is symbol 285 without extra bits,
// not 284 with 31.  A length outside the range is clamped into it, so that no caller can get a symbol outside 257..285.
RLE_HD int rle_length_symbol(int len, int* extra, int* nextra) {
    len = len < RLE_MIN_MATCH ? RLE_MIN_MATCH : (len > RLE_MAX_MATCH ? RLE_MAX_MATCH : len);
    const int l = len - 3;
    int e = 0;
    if (l >= 8 && len != RLE_MAX_MATCH) e = 29 - __builtin_clz((unsigned)l);   // floor(log2 l) - 2, 1..5
    *nextra = e;
    *extra = l & ((1 << e) - 1);
    if (len == RLE_MAX_MATCH) {
        *extra = 0;
        return 285;
    }
    return e == 0 ? 257 + l : 261 + 4 * e + ((l >> e) & 3);
}

// What the position `off` bytes into a run of `runlen` bytes of value `v` emits (0 <= off < runlen).
RLE_HD RleToken rle_token_at(int off, int runlen, int v) {
    RleToken t = {RLE_LITERAL, v, 0, 0};
    if (off <= 0) return t;                                  // the run's head
    const int q = off - 1, rest = runlen - 1;                // the q-th of the `rest` bytes behind the head
    const int in_chunk = q % RLE_MAX_MATCH;
    const int chunk = rest - (q - in_chunk) < RLE_MAX_MATCH ? rest - (q - in_chunk) : RLE_MAX_MATCH;
    if (chunk < RLE_MIN_MATCH) return t;                     // a remainder of 1 or 2: literals
    t.kind = RLE_NOTHING;
    t.symbol = 0;
    if (in_chunk == 0) {
        t.kind = RLE_MATCH;
        t.symbol = rle_length_symbol(chunk, &t.extra, &t.nextra);
    }
    return t;
}

// The same from the span's bytes alone: span[0 .. n) is one span (n <= RLE_SPAN), i a position in it.  Reads no byte
// outside [0, n).
RLE_HD RleToken rle_span_token(const uint8_t* span, int n, int i) {
    const int v = span[i];
    int head = i, end = i + 1;
    while (head > 0 && span[head - 1] == v) --head;
    while (end < n && span[end] == v) ++end;
    return rle_token_at(i - head, end - head, v);
}

// Bits a token takes under a code of `len` bits for its symbol: a match adds its extra bits and the one distance bit.
RLE_HD int rle_token_bits(const RleToken& t, int len) {
    return t.kind == RLE_NOTHING ? 0 : (t.kind == RLE_MATCH ? len + t.nextra + 1 : len);
}
