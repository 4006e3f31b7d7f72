// The zlib / deflate decoder of csrc/png_read.hip, host and device: the bit reader, the code-length validation and table
// build, the token decode, the bounds rules and the per-lane copy arithmetic, written once.  One wave of 64 lanes decodes
// one stream.  All decoder state (InfState) is wave-uniform; the lanes share the work that has no serial dependence: the
// input window's fill, the first-level tables' fill, a match's or a stored block's copy, the window's flush and its
// Adler-32 partial.  On the device a lane section (INF_LANES) is the lane's own pass and INF_SYNC is a workgroup barrier;
// on the host the same text runs the lanes as a loop and the barrier is empty, so that a plain C++ program can walk the
// very code of the kernel over exact-size buffers under the address and undefined-behaviour sanitizers
// (tools/png_inflate_check.cpp).
//
// Rules kept by every loop here: an iteration consumes at least one input bit, or produces at least one output byte, or
// ends; input bits are capped by in_len (reads past the end give zero bits and INF_E_INPUT), output bytes by cap.  Every
// table index goes through a mask, a back-reference is checked against the bytes produced before it is followed, and
// every store to `dst` is clipped to [0, cap).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define INF_HD __host__ __device__ __forceinline__
#else
#define INF_HD static inline
#endif

// Status codes, shared with the PNG layer (the last two are set by the CRC and unfilter kernels).
#define INF_OK 0
#define INF_E_INPUT 1     // input exhausted
#define INF_E_HEADER 2    // zlib header: CM, CINFO, FCHECK, FDICT
#define INF_E_BTYPE 3     // block type 3
#define INF_E_STORED 4    // stored LEN / NLEN mismatch
#define INF_E_LENS 5      // bad code-length set
#define INF_E_SYMBOL 6    // invalid literal/length or distance symbol
#define INF_E_DIST 7      // distance too far back
#define INF_E_LONG 8      // output longer than cap
#define INF_E_SHORT 9     // output shorter than cap
#define INF_E_ADLER 10    // Adler-32 mismatch
#define PNG_E_CRC 11      // chunk CRC mismatch
#define PNG_E_FILTER 12   // filter type above 4

#define INF_LANE_COUNT 64
#define INF_WINDOW 32768            // the LDS ring: deflate's window
#define INF_WINDOW_MASK (INF_WINDOW - 1)
#define INF_IN_WORDS 1024           // the input window, dwords
#define INF_FLUSH_AT 16384          // unflushed bytes at which the ring is flushed; + 258 + 4096 stays under the ring
#define INF_STORED_STEP 4096        // a stored block is copied in pieces of this many bytes
#define INF_LIT_BITS 10
#define INF_DIST_BITS 9
#define INF_CL_BITS 7
#define INF_ADLER_MOD 65521u

#if defined(__HIP_DEVICE_COMPILE__)
#define INF_LANES(l) for (int l = (int)threadIdx.x, l##_once = 1; l##_once; l##_once = 0)
#define INF_SYNC() __syncthreads()
#define INF_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define INF_LANEVAR(type, name) type name
#define INF_LV(name, l) name
#define INF_ONE if (threadIdx.x == 0)
#else
#define INF_LANES(l) for (int l = 0; l < INF_LANE_COUNT; ++l)
#define INF_SYNC() ((void)0)
#define INF_UNI(x) ((uint32_t)(x))
#define INF_LANEVAR(type, name) type name[INF_LANE_COUNT]
#define INF_LV(name, l) name[l]
#define INF_ONE
#endif

struct InfShared {
    uint32_t in[INF_IN_WORDS + 1];          // stream bytes [wbase, wbase + 4 * INF_IN_WORDS + 4), zeros past the stream's end
    uint32_t ring[INF_WINDOW / 4];          // output byte p is byte p & INF_WINDOW_MASK
    uint16_t lit_fast[1 << INF_LIT_BITS];   // (symbol << 4) | code length, indexed by the next bits; 0 = a longer code
    uint16_t dist_fast[1 << INF_DIST_BITS];
    uint16_t cl_fast[1 << INF_CL_BITS];
    uint16_t lit_count[16], dist_count[16], cl_count[16];   // codes of each length
    uint16_t lit_sym[512], dist_sym[32], cl_sym[32];        // symbols in canonical order
    uint16_t code[512];                     // a symbol's canonical code while its table is built
    uint16_t next[16], offs[16];
    uint8_t lens[512];                      // code lengths: literal/length, then distance
    uint8_t cl_lens[32];
    int rc;
};

struct InfState {
    const uint8_t* src;
    uint32_t in_len, in_pos, wbase;   // bytes; in_pos counts the bytes taken into `hold`
    uint64_t hold;
    int nbits;
    uint8_t* dst;
    uint32_t cap, produced, flushed;  // flushed is a multiple of 4 until the last flush
    uint32_t a, b;                    // Adler-32 of dst[0, flushed)
    int fixed_built;
    int status;
};

INF_HD uint32_t inf_ring_byte(const InfShared* S, uint32_t p) {
    return (S->ring[(p & INF_WINDOW_MASK) >> 2] >> (8 * (p & 3))) & 255u;
}
// byte stores into the ring go through a byte view: lanes store neighbouring bytes of a dword together
INF_HD void inf_ring_store(InfShared* S, uint32_t p, uint32_t v) { ((uint8_t*)S->ring)[p & INF_WINDOW_MASK] = (uint8_t)v; }

// ----------------------------------------------------------------------------- the bit reader
INF_HD void inf_window(InfShared* S, InfState& st) {
    st.wbase = st.in_pos & ~3u;
    INF_SYNC();
    INF_LANES(l) {
        for (int i = l; i < INF_IN_WORDS + 1; i += INF_LANE_COUNT) {
            const uint64_t p = (uint64_t)st.wbase + 4u * (uint32_t)i;
            uint32_t w = 0;
            for (int k = 0; k < 4; ++k)
                if (p + k < st.in_len) w |= (uint32_t)st.src[p + k] << (8 * k);
            S->in[i] = w;
        }
    }
    INF_SYNC();
}

// adds 32 bits to `hold`; the caller has nbits <= 32
INF_HD void inf_refill(InfShared* S, InfState& st) {
    if (st.in_pos - st.wbase > 4u * INF_IN_WORDS - 4u) inf_window(S, st);   // unsigned: also in_pos < wbase
    const uint32_t o = st.in_pos - st.wbase, i = (o >> 2) & (INF_IN_WORDS - 1), s = (o & 3u) * 8u;
    const uint32_t lo = S->in[i], hi = S->in[i + 1];
    const uint32_t v = INF_UNI(s ? (lo >> s) | (hi << (32u - s)) : lo);
    st.hold |= (uint64_t)v << st.nbits;
    st.nbits += 32;
    st.in_pos += 4;
}

// the next n bits, n in [0, 16]
INF_HD uint32_t inf_bits(InfShared* S, InfState& st, int n) {
    if (st.nbits < n) inf_refill(S, st);
    const uint32_t v = (uint32_t)st.hold & ((1u << n) - 1u);
    st.hold >>= n;
    st.nbits -= n;
    return v;
}

INF_HD uint64_t inf_bit_pos(const InfState& st) { return (uint64_t)st.in_pos * 8u - (uint64_t)st.nbits; }
// bits were taken from beyond the stream's end
INF_HD int inf_over(const InfState& st) { return inf_bit_pos(st) > (uint64_t)st.in_len * 8u; }

// gives the whole bytes held in `hold` back and leaves the reader on a byte boundary
INF_HD void inf_byte_align(InfState& st) {
    st.in_pos -= (uint32_t)(st.nbits >> 3);
    st.hold = 0;
    st.nbits = 0;
}

// ----------------------------------------------------------------------------- code tables
INF_HD uint32_t inf_reverse(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) {
        r = (r << 1) | (code & 1u);
        code >>= 1;
    }
    return r;
}

// Validates the code lengths lens[0, n) (n <= 512, each <= 15) and builds the code's tables.  Over-subscribed sets are
// refused; incomplete ones too, but for a distance code with no code at all or with a single code of length 1.
// Returns 0 or INF_E_LENS, the same in every lane.
INF_HD int inf_build(InfShared* S, const uint8_t* lens, int n, uint16_t* fast, int fbits, uint16_t* count, uint16_t* syms, int smask,
                     int is_dist) {
    INF_SYNC();
    INF_LANES(l) {
        for (int i = l; i < (1 << fbits); i += INF_LANE_COUNT) fast[i] = 0;
    }
    INF_ONE {
        for (int len = 0; len < 16; ++len) count[len] = 0;
        for (int i = 0; i < n; ++i) count[lens[i] & 15] = (uint16_t)(count[lens[i] & 15] + 1);
        const int total = n - count[0];
        count[0] = 0;
        int left = 1, rc = 0;
        for (int len = 1; len < 16; ++len) {
            left = (left << 1) - (int)count[len];
            if (left < 0) {
                rc = INF_E_LENS;
                break;
            }
        }
        if (left > 0 && !(is_dist && (total == 0 || (total == 1 && count[1] == 1)))) rc = INF_E_LENS;
        if (!rc) {
            uint32_t code = 0, off = 0;
            S->next[0] = 0;
            S->offs[0] = 0;
            for (int len = 1; len < 16; ++len) {
                code = (code + count[len - 1]) << 1;
                off += count[len - 1];
                S->next[len] = (uint16_t)code;
                S->offs[len] = (uint16_t)off;
            }
            for (int i = 0; i < n; ++i) {
                const int len = lens[i] & 15;
                if (len) {
                    S->code[i & 511] = S->next[len];
                    S->next[len] = (uint16_t)(S->next[len] + 1);
                    syms[S->offs[len] & smask] = (uint16_t)i;
                    S->offs[len] = (uint16_t)(S->offs[len] + 1);
                }
            }
        }
        S->rc = rc;
    }
    INF_SYNC();
    const int rc = (int)INF_UNI(S->rc);
    if (rc) return rc;
    INF_LANES(l) {
        for (int i = l; i < n; i += INF_LANE_COUNT) {
            const int len = lens[i] & 15;
            if (len && len <= fbits) {
                const uint32_t e = ((uint32_t)i << 4) | (uint32_t)len;
                for (uint32_t k = inf_reverse(S->code[i & 511], len); k < (1u << fbits); k += 1u << len)
                    fast[k & ((1u << fbits) - 1u)] = (uint16_t)e;
            }
        }
    }
    INF_SYNC();
    return 0;
}

// The next symbol of a code, or -1 where the next bits are no code of it (nothing is consumed then).
INF_HD int inf_decode(InfShared* S, InfState& st, const uint16_t* fast, int fbits, const uint16_t* count, const uint16_t* syms, int smask) {
    if (st.nbits < 15) inf_refill(S, st);
    const uint32_t e = INF_UNI(fast[(uint32_t)st.hold & ((1u << fbits) - 1u)]);
    if (e & 15u) {
        st.hold >>= (e & 15u);
        st.nbits -= (int)(e & 15u);
        return (int)(e >> 4);
    }
    uint32_t bits = (uint32_t)st.hold;
    int code = 0, first = 0, index = 0;
    for (int len = 1; len < 16; ++len) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int c = (int)INF_UNI(count[len]);
        if (code - c < first) {
            const uint32_t sym = INF_UNI(syms[(index + (code - first)) & smask]);
            st.hold >>= len;
            st.nbits -= len;
            return (int)sym;
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// a failed decode: the stream ended inside the code, or the bits are no code
INF_HD int inf_decode_error(const InfState& st) {
    return (uint64_t)st.in_len * 8u < inf_bit_pos(st) + 15u ? INF_E_INPUT : INF_E_SYMBOL;
}

// ----------------------------------------------------------------------------- output
// Stores ring bytes [flushed, upto) to dst (clipped to cap) and takes them into the Adler-32; upto is a multiple of 4
// unless it is the stream's end.
INF_HD void inf_flush(InfShared* S, InfState& st, uint32_t upto) {
    INF_SYNC();
    const uint32_t from = st.flushed, len = upto - from;
    INF_LANEVAR(uint32_t, sa);
    INF_LANEVAR(uint32_t, sb);
    INF_LANES(l) {
        uint32_t a = 0, b = 0;
        for (uint32_t p = from + 4u * (uint32_t)l; p < upto; p += 4u * INF_LANE_COUNT) {
            const uint32_t w = S->ring[(p & INF_WINDOW_MASK) >> 2];
            if (p + 4u <= upto && p + 4u <= st.cap) {
                *(uint32_t*)(st.dst + p) = w;
            } else {
                for (uint32_t k = 0; k < 4; ++k)
                    if (p + k < upto && p + k < st.cap) st.dst[p + k] = (uint8_t)(w >> (8 * k));
            }
            for (uint32_t k = 0; k < 4; ++k) {
                if (p + k < upto) {
                    const uint32_t d = (w >> (8 * k)) & 255u;
                    a += d;
                    b += (upto - (p + k)) * d;   // at most 21 000 bytes a flush, 330 a lane: below 2^32
                }
            }
        }
        INF_LV(sa, l) = a % INF_ADLER_MOD;
        INF_LV(sb, l) = b % INF_ADLER_MOD;
    }
    uint32_t ta = 0, tb = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    ta = sa;
    tb = sb;
    for (int o = 32; o > 0; o >>= 1) {
        ta += __shfl_xor(ta, o, 64);
        tb += __shfl_xor(tb, o, 64);
    }
    ta = INF_UNI(ta);
    tb = INF_UNI(tb);
#else
    for (int l = 0; l < INF_LANE_COUNT; ++l) {
        ta += sa[l];
        tb += sb[l];
    }
#endif
    st.b = (uint32_t)(((uint64_t)st.b + (uint64_t)(len % INF_ADLER_MOD) * st.a + tb) % INF_ADLER_MOD);
    st.a = (st.a + ta) % INF_ADLER_MOD;
    st.flushed = upto;
    INF_SYNC();
}

INF_HD void inf_flush_if_due(InfShared* S, InfState& st) {
    if (st.produced - st.flushed >= INF_FLUSH_AT) inf_flush(S, st, st.produced & ~3u);
}

// Copies `len` (<= 258) bytes from `dist` back; the caller has checked 1 <= dist <= min(produced, 32768) and
// produced + len <= cap.  Byte j comes from produced - dist + j % dist, which lies before the match; all lanes of a
// step load before any stores, because with dist near the ring's size a step's sources and destinations share slots.
INF_HD void inf_copy_match(InfShared* S, InfState& st, uint32_t len, uint32_t dist) {
    INF_SYNC();
    for (uint32_t j0 = 0; j0 < len; j0 += INF_LANE_COUNT) {
        INF_LANEVAR(uint32_t, v);
        INF_LANES(l) {
            const uint32_t j = j0 + (uint32_t)l;
            INF_LV(v, l) = j < len ? inf_ring_byte(S, st.produced - dist + j % dist) : 0u;
        }
        INF_LANES(l) {
            const uint32_t j = j0 + (uint32_t)l;
            if (j < len) inf_ring_store(S, st.produced + j, INF_LV(v, l));
        }
    }
    INF_SYNC();
    st.produced += len;
}

// ----------------------------------------------------------------------------- blocks
INF_HD void inf_stored(InfShared* S, InfState& st) {
    st.hold >>= st.nbits & 7;
    st.nbits &= ~7;
    const uint32_t len = inf_bits(S, st, 16), nlen = inf_bits(S, st, 16);
    if (inf_over(st)) {
        st.status = INF_E_INPUT;
        return;
    }
    if ((len ^ 0xffffu) != nlen) {
        st.status = INF_E_STORED;
        return;
    }
    inf_byte_align(st);
    // both ends are checked for the whole block before a byte of it is copied
    if (len > st.in_len - st.in_pos) {
        st.status = INF_E_INPUT;
        return;
    }
    if (len > st.cap - st.produced) {
        st.status = INF_E_LONG;
        return;
    }
    uint32_t left = len;
    while (left) {
        inf_flush_if_due(S, st);
        const uint32_t step = left < INF_STORED_STEP ? left : INF_STORED_STEP;
        INF_SYNC();
        INF_LANES(l) {
            for (uint32_t j = (uint32_t)l; j < step; j += INF_LANE_COUNT) inf_ring_store(S, st.produced + j, st.src[st.in_pos + j]);
        }
        INF_SYNC();
        st.produced += step;
        st.in_pos += step;
        left -= step;
    }
}

INF_HD void inf_fixed_tables(InfShared* S, InfState& st) {
    if (st.fixed_built) return;
    INF_SYNC();
    INF_LANES(l) {
        for (int i = l; i < 320; i += INF_LANE_COUNT) S->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    }
    inf_build(S, S->lens, 288, S->lit_fast, INF_LIT_BITS, S->lit_count, S->lit_sym, 511, 0);
    inf_build(S, S->lens + 288, 32, S->dist_fast, INF_DIST_BITS, S->dist_count, S->dist_sym, 31, 1);
    st.fixed_built = 1;
}

INF_HD void inf_dynamic_tables(InfShared* S, InfState& st) {
    st.fixed_built = 0;
    const int nlen = (int)inf_bits(S, st, 5) + 257, ndist = (int)inf_bits(S, st, 5) + 1, ncode = (int)inf_bits(S, st, 4) + 4;
    if (inf_over(st)) {
        st.status = INF_E_INPUT;
        return;
    }
    if (nlen > 286 || ndist > 30) {
        st.status = INF_E_LENS;
        return;
    }
    INF_SYNC();
    for (int i = 0; i < 19; ++i) {
        // the order of RFC 1951 3.2.7, packed five bits a symbol
        const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                                  10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
        const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
        const int s = (int)((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31u);
        const uint32_t v = i < ncode ? inf_bits(S, st, 3) : 0u;
        INF_ONE { S->cl_lens[s & 31] = (uint8_t)v; }
    }
    if (inf_over(st)) {
        st.status = INF_E_INPUT;
        return;
    }
    if (inf_build(S, S->cl_lens, 19, S->cl_fast, INF_CL_BITS, S->cl_count, S->cl_sym, 31, 0)) {
        st.status = INF_E_LENS;
        return;
    }
    int idx = 0, prev = 0;
    while (idx < nlen + ndist) {
        const int sym = inf_decode(S, st, S->cl_fast, INF_CL_BITS, S->cl_count, S->cl_sym, 31);
        if (sym < 0 || sym > 18) {
            st.status = sym < 0 && inf_decode_error(st) == INF_E_INPUT ? INF_E_INPUT : INF_E_LENS;
            return;
        }
        int rep = 1, val = sym;
        if (sym == 16) {
            rep = 3 + (int)inf_bits(S, st, 2);
            val = prev;
        } else if (sym == 17) {
            rep = 3 + (int)inf_bits(S, st, 3);
            val = 0;
        } else if (sym == 18) {
            rep = 11 + (int)inf_bits(S, st, 7);
            val = 0;
        }
        if (inf_over(st)) {
            st.status = INF_E_INPUT;
            return;
        }
        if ((sym == 16 && idx == 0) || idx + rep > nlen + ndist) {
            st.status = INF_E_LENS;
            return;
        }
        INF_ONE {
            for (int k = 0; k < rep; ++k) S->lens[(idx + k) & 511] = (uint8_t)val;
        }
        idx += rep;
        prev = val;
    }
    INF_SYNC();
    if (INF_UNI(S->lens[256]) == 0 || inf_build(S, S->lens, nlen, S->lit_fast, INF_LIT_BITS, S->lit_count, S->lit_sym, 511, 0) ||
        inf_build(S, S->lens + nlen, ndist, S->dist_fast, INF_DIST_BITS, S->dist_count, S->dist_sym, 31, 1))
        st.status = INF_E_LENS;
}

INF_HD void inf_tokens(InfShared* S, InfState& st) {
    for (;;) {
        inf_flush_if_due(S, st);
        int sym = inf_decode(S, st, S->lit_fast, INF_LIT_BITS, S->lit_count, S->lit_sym, 511);
        if (sym < 0) {
            st.status = inf_decode_error(st);
            return;
        }
        if (inf_over(st)) {
            st.status = INF_E_INPUT;
            return;
        }
        if (sym < 256) {
            if (st.produced >= st.cap) {
                st.status = INF_E_LONG;
                return;
            }
            INF_ONE { inf_ring_store(S, st.produced, (uint32_t)sym); }
            st.produced += 1;
            continue;
        }
        if (sym == 256) return;
        sym -= 257;
        if (sym >= 29) {
            st.status = INF_E_SYMBOL;
            return;
        }
        uint32_t len = 258;
        if (sym < 8) {
            len = 3u + (uint32_t)sym;
        } else if (sym < 28) {
            const int extra = (sym >> 2) - 1;
            len = 3u + ((4u + ((uint32_t)sym & 3u)) << extra) + inf_bits(S, st, extra);
        }
        const int dsym = inf_decode(S, st, S->dist_fast, INF_DIST_BITS, S->dist_count, S->dist_sym, 31);
        if (dsym < 0) {
            st.status = inf_decode_error(st);
            return;
        }
        if (inf_over(st)) {
            st.status = INF_E_INPUT;
            return;
        }
        if (dsym >= 30) {
            st.status = INF_E_SYMBOL;
            return;
        }
        uint32_t dist = 1u + (uint32_t)dsym;
        if (dsym >= 4) {
            const int extra = (dsym >> 1) - 1;
            dist = 1u + ((2u + ((uint32_t)dsym & 1u)) << extra) + inf_bits(S, st, extra);
            if (inf_over(st)) {
                st.status = INF_E_INPUT;
                return;
            }
        }
        if (dist > st.produced) {
            st.status = INF_E_DIST;
            return;
        }
        if (len > st.cap - st.produced) {
            st.status = INF_E_LONG;
            return;
        }
        inf_copy_match(S, st, len, dist);
    }
}

// Decodes the zlib stream src[0, in_len) into dst[0, cap) and returns the status; out4 = status, bytes produced, bytes
// consumed, Adler-32 of the bytes produced.  in_len and cap are below 2^31 and dst is 4-byte aligned.
INF_HD void inflate_run(InfShared* S, const uint8_t* src, uint32_t in_len, uint8_t* dst, uint32_t cap, uint32_t* out4) {
    InfState st;
    st.src = src;
    st.in_len = in_len;
    st.in_pos = 0;
    st.hold = 0;
    st.nbits = 0;
    st.dst = dst;
    st.cap = cap;
    st.produced = 0;
    st.flushed = 0;
    st.a = 1;
    st.b = 0;
    st.fixed_built = 0;
    st.status = INF_OK;
    inf_window(S, st);
    const uint32_t cmf = inf_bits(S, st, 8), flg = inf_bits(S, st, 8);
    if (inf_over(st)) st.status = INF_E_INPUT;
    else if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) st.status = INF_E_HEADER;
    int final = 0;
    while (!st.status && !final) {
        final = (int)inf_bits(S, st, 1);
        const uint32_t type = inf_bits(S, st, 2);
        if (inf_over(st)) st.status = INF_E_INPUT;
        else if (type == 3) st.status = INF_E_BTYPE;
        else if (type == 0) inf_stored(S, st);
        else {
            if (type == 1) inf_fixed_tables(S, st);
            else inf_dynamic_tables(S, st);
            if (!st.status) inf_tokens(S, st);
        }
    }
    inf_flush(S, st, st.produced);
    const uint32_t adler = (st.b << 16) | st.a;
    if (!st.status && st.produced < st.cap) st.status = INF_E_SHORT;
    if (!st.status) {
        st.hold >>= st.nbits & 7;
        st.nbits &= ~7;
        uint32_t stored = 0;
        for (int k = 0; k < 4; ++k) stored = (stored << 8) | inf_bits(S, st, 8);
        if (inf_over(st)) st.status = INF_E_INPUT;
        else if (stored != adler) st.status = INF_E_ADLER;
    }
    // bytes consumed: whole bytes the decoder has taken bits from, never more than the stream has
    uint64_t used = (inf_bit_pos(st) + 7u) >> 3;
    if (used > st.in_len) used = st.in_len;
    INF_ONE {
        out4[0] = (uint32_t)st.status;
        out4[1] = st.produced;
        out4[2] = (uint32_t)used;
        out4[3] = adler;
    }
}
