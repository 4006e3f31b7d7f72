// The baseline JPEG encoder of csrc/jpeg_write.hip, host and device: the geometry of a frame's blocks in MCU scan order,
// the sample a component has at a plane position (colour conversion, edge replication and downsampling in libjpeg's
// order), the two passes of jfdctint.c, the quantiser, the quantisation tables of jpeg_set_quality, and the symbol rule
// of one block (ITU-T T.81 F.1.2) over a sink that counts bits, writes them at a bit offset or tallies the symbols, and
// the optimal-table rule of jchuff.c for the host - written once.  On the device a lane takes a row, a column or a
// block; on the host the same text is plain C++, so that tools/jpeg_encode_check.cpp walks the very code of the kernels
// over exact-size buffers under the address and undefined-behaviour sanitizers.  tests/_jpeg_write_ref.py states what it
// computes, tests/_jpeg_opt_ref.py the tally and the tables.
//
// Rules kept here: every pixel read goes through a clamp to the frame; every table index goes through a mask; every
// stream word written is checked against the word count of its own segment (a frame, or one restart interval of it); a
// block's code is at most 1658 bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPGE_HD __host__ __device__ __forceinline__
#define JPGE_HDM __host__ __device__ __forceinline__   // on a member function
#else
#define JPGE_HD static inline
#define JPGE_HDM inline
#endif

// Words of the stream that two blocks share are ORed into (they were cleared by an earlier launch); a vector atomic on
// the device, where neighbouring blocks are other lanes, a plain OR on the host, where they are earlier iterations.
#if defined(__HIP_DEVICE_COMPILE__)
#define JPGE_OR(p, v) atomicOr((p), (v))
#else
#define JPGE_OR(p, v) (*(p) |= (v))
#endif

#define JPGE_SAMPLING_444 0
#define JPGE_SAMPLING_422 1
#define JPGE_SAMPLING_420 2
#define JPGE_HUFF_WORDS 272            // per table class (0 luma, 1 chroma): 16 DC entries by category, 256 AC entries by symbol
#define JPGE_MAX_BLOCK_BITS 2048       // bound used for the size checks: DC 9 + 11, 63 AC symbols of at most 16 + 10
#define JPGE_MAX_BLOCKS (1 << 20)      // blocks of a frame: its bit offsets stay below 2^31

// A clip's geometry: every frame has it.  A gray frame is one component whose MCU is one block (wib x hib of them, no
// dummy blocks); a colour frame's MCU is hmax * vmax luma blocks, then Cb, then Cr.
struct JpegEncGeom {
    int h, w, channels, bgr;
    int hmax, vmax;        // luma sampling factors (1, 1 for gray)
    int mcux, mcuy;        // MCUs per row, MCU rows
    int wib, hib;          // luma blocks that count: ceil(w / 8), ceil(h / 8)
    int bpm;               // blocks per MCU
    int blocks;            // blocks of a frame: mcux * mcuy * bpm
    // Restart intervals (T.81 B.2.4.4, E.1.4; libjpeg's restart_interval).  An interval is a segment of the scan that
    // starts on a byte boundary with every DC predictor at 0 and ends in a 1-fill: without an interval the frame is one.
    int restart_mcus;      // MCUs of an interval, 0: none
    int segs;              // intervals of a frame: ceil(mcux * mcuy / restart_mcus), 1 without an interval
    int segb;              // blocks of every interval but a frame's last, which may hold fewer: restart_mcus * bpm
};

JPGE_HD JpegEncGeom jpeg_enc_geometry(int h, int w, int channels, int bgr, int sampling) {
    JpegEncGeom g;
    g.h = h;
    g.w = w;
    g.channels = channels;
    g.bgr = bgr;
    g.hmax = channels == 3 && sampling != JPGE_SAMPLING_444 ? 2 : 1;
    g.vmax = channels == 3 && sampling == JPGE_SAMPLING_420 ? 2 : 1;
    g.mcux = (w + 8 * g.hmax - 1) / (8 * g.hmax);
    g.mcuy = (h + 8 * g.vmax - 1) / (8 * g.vmax);
    g.wib = (w + 7) / 8;
    g.hib = (h + 7) / 8;
    g.bpm = channels == 3 ? g.hmax * g.vmax + 2 : 1;
    g.blocks = g.mcux * g.mcuy * g.bpm;
    g.restart_mcus = 0;
    g.segs = 1;
    g.segb = g.blocks;
    return g;
}

// The geometry with a restart interval of `restart_mcus` MCUs (0 .. 65535, 0: none).  An interval that holds the whole
// scan leaves one segment: the file gets its DRI segment and no marker.
JPGE_HD JpegEncGeom jpeg_enc_restart(JpegEncGeom g, int restart_mcus) {
    const int mcus = g.mcux * g.mcuy;
    g.restart_mcus = restart_mcus > 0 ? restart_mcus : 0;
    if (g.restart_mcus > 0 && g.restart_mcus < mcus) {
        g.segs = (mcus + g.restart_mcus - 1) / g.restart_mcus;
        g.segb = g.restart_mcus * g.bpm;
    } else {
        g.segs = 1;
        g.segb = g.blocks;
    }
    return g;
}

// Blocks of interval s of a frame, 0 <= s < g.segs.
JPGE_HD int jpeg_enc_seg_blocks(const JpegEncGeom& g, int s) {
    const int left = g.blocks - s * g.segb;
    return left < g.segb ? left : g.segb;
}

// The second byte of what ends interval s: RSTm, m = s mod 8, in front of the next interval, EOI behind a frame's last.
JPGE_HD int jpeg_enc_seg_marker(const JpegEncGeom& g, int s) { return s == g.segs - 1 ? 0xd9 : 0xd0 + (s & 7); }

// Where block b of a frame lies: component, block row and column in the component's grid.  A dummy block - one that only
// completes an MCU, past the luma blocks that count - is placed at the block whose DC it repeats: the one before it in
// the MCU's own order, followed back until a real one (block 0 of an MCU is always real).
struct JpegEncPlace {
    int c, by, bx, dummy;
};

JPGE_HD JpegEncPlace jpeg_enc_place(const JpegEncGeom& g, int b) {
    JpegEncPlace p;
    p.dummy = 0;
    if (g.channels == 1) {
        p.c = 0;
        p.by = b / g.mcux;
        p.bx = b - p.by * g.mcux;
        return p;
    }
    const int m = b / g.bpm, my = m / g.mcux, mx = m - my * g.mcux, ny = g.hmax * g.vmax;
    int k = b - m * g.bpm;
    if (k >= ny) {
        p.c = 1 + (k - ny);
        p.by = my;
        p.bx = mx;
        return p;
    }
    p.c = 0;
    for (;;) {
        const int vy = k / g.hmax, hx = k - vy * g.hmax;
        p.by = my * g.vmax + vy;
        p.bx = mx * g.hmax + hx;
        if (k == 0 || (p.by < g.hib && p.bx < g.wib)) return p;
        p.dummy = 1;
        --k;
    }
}

// The block before b among its component's blocks in scan order, whose DC is b's prediction; -1 for a component's first
// of the frame and of every restart interval (a dummy block still repeats the block before it in its own MCU).
JPGE_HD int jpeg_enc_pred_block(const JpegEncGeom& g, int b) {
    const int m = b / g.bpm, k = b - m * g.bpm, ny = g.hmax * g.vmax;
    const bool first = m == 0 || (g.restart_mcus > 0 && m % g.restart_mcus == 0);     // the MCU opens a segment
    if (g.channels == 1) return first ? -1 : b - 1;
    if (k < ny) {
        if (k > 0) return b - 1;
        return first ? -1 : (m - 1) * g.bpm + ny - 1;
    }
    return first ? -1 : b - g.bpm;
}

JPGE_HD int jpeg_enc_table_class(const JpegEncGeom& g, int b) { return g.channels == 3 && b % g.bpm >= g.hmax * g.vmax ? 1 : 0; }

// jccolor.c: 16-bit fixed point, F(x) = int(x * 65536 + 0.5).
JPGE_HD int jpeg_enc_ycc(int r, int gr, int bl, int c) {
    if (c == 0) return (19595 * r + 38470 * gr + 7471 * bl + 32768) >> 16;
    if (c == 1) return (-11058 * r - 21710 * gr + 32768 * bl + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * gr - 5329 * bl + (128 << 16) + 32767) >> 16;
}

// Component c of the pixel (y, x), both clamped to the frame: the replication of the last column and the last row.
JPGE_HD int jpeg_enc_full(const uint8_t* frame, const JpegEncGeom& g, int c, int y, int x) {
    y = y < 0 ? 0 : (y > g.h - 1 ? g.h - 1 : y);
    x = x < 0 ? 0 : (x > g.w - 1 ? g.w - 1 : x);
    const uint8_t* p = frame + ((size_t)y * g.w + x) * g.channels;
    if (g.channels == 1) return p[0];
    return jpeg_enc_ycc(p[g.bgr ? 2 : 0], p[1], p[g.bgr ? 0 : 2], c);
}

// The sample of component c at (py, px) of its own plane of whole blocks.  jcprepct.c / jcsample.c: the columns are
// widened first, 4:2:0 repeats an odd frame's last row once, then the downsample (h2v1: bias 0, 1, 0, 1 ...; h2v2: 1, 2,
// 1, 2 ... along the output row), then the plane is lengthened by its last row - so a chroma row past ceil(h / 2) is the
// last downsampled row, not the downsample of repeated rows.
JPGE_HD int jpeg_enc_sample(const uint8_t* frame, const JpegEncGeom& g, int c, int py, int px) {
    if (c == 0 || (g.hmax == 1 && g.vmax == 1)) return jpeg_enc_full(frame, g, c, py, px);
    if (g.vmax == 1) return (jpeg_enc_full(frame, g, c, py, 2 * px) + jpeg_enc_full(frame, g, c, py, 2 * px + 1) + (px & 1)) >> 1;
    const int ch = (g.h + 1) >> 1;
    py = py > ch - 1 ? ch - 1 : py;
    return (jpeg_enc_full(frame, g, c, 2 * py, 2 * px) + jpeg_enc_full(frame, g, c, 2 * py, 2 * px + 1) +
            jpeg_enc_full(frame, g, c, 2 * py + 1, 2 * px) + jpeg_enc_full(frame, g, c, 2 * py + 1, 2 * px + 1) + 1 + (px & 1)) >> 2;
}

// One 8-point pass of jfdctint.c (CONST_BITS 13, PASS1_BITS 2) in int32; the constants are those of the IDCT in
// csrc/jpeg_read.hip.  FIRST: the row pass, outputs scaled up by 4; else the column pass, which takes that scale out
// again.  Descales round half up.  |d| <= 128 in the first pass and <= 2^13 in the second keep every product in int32.
template <bool FIRST>
JPGE_HD void jpeg_fdct_pass(const int (&d)[8], int (&o)[8]) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int s = FIRST ? 11 : 15, half = 1 << (s - 1);
    if (FIRST) {
        o[0] = (t10 + t11) * 4;
        o[4] = (t10 - t11) * 4;
    } else {
        o[0] = (t10 + t11 + 2) >> 2;
        o[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    o[2] = (z1 + t13 * 6270 + half) >> s;
    o[6] = (z1 - t12 * 15137 + half) >> s;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o[7] = (a4 + z1 + z3 + half) >> s;
    o[5] = (a5 + z2 + z4 + half) >> s;
    o[3] = (a6 + z2 + z3 + half) >> s;
    o[1] = (a7 + z1 + z4 + half) >> s;
}

// The quantiser: the coefficient carries the FDCT's factor 8, so the divisor is table << 3; round half away from zero.
JPGE_HD int jpeg_quantise(int coef, int table) {
    const int q8 = table << 3, a = coef < 0 ? -coef : coef, q = (a + (q8 >> 1)) / q8;
    return coef < 0 ? -q : q;
}

// ----------------------------------------------------------------------------- per-block rate allocation (ROI)
// A map of coarsening levels, uint8 [By, Bx] on a grid of B x B luma pixels, in HEVC QP units: the quantiser step doubles
// every 6 levels.  A coefficient that the quantiser of the file's own table coarsened by the block's level would round to
// zero is zeroed; every other one keeps the file's own quantiser, and DC is never touched - a dead zone, not a coarser
// step, so the file stays a baseline JPEG with the tables of its header.  Integers only.
#define JPGE_ROI_MAX_LEVEL 48

// round(16 * 2^(level / 6)) for level 0 .. 48; a level above 48 counts as 48.
JPGE_HD int jpeg_roi_scale16(int level) {
    const uint16_t scale[JPGE_ROI_MAX_LEVEL + 1] = {16,  18,  20,  23,  25,  29,  32,  36,  40,   45,   51,   57,   64,   72,   81,   91,  102,
                                                    114, 128, 144, 161, 181, 203, 228, 256, 287,  323,  362,  406,  456,  512,  575,  645, 724,
                                                    813, 912, 1024, 1149, 1290, 1448, 1625, 1825, 2048, 2299, 2580, 2896, 3251, 3649, 4096};
    return scale[level < 0 ? 0 : (level > JPGE_ROI_MAX_LEVEL ? JPGE_ROI_MAX_LEVEL : level)];
}

// The level of the block at `p`: the minimum over the cells its footprint touches - a luma or gray block covers 8 x 8
// luma pixels, a chroma block 8 * hmax x 8 * vmax; both ends of the footprint are clamped to the frame, a cell index to
// the grid (which may be the floored one, h / B x w / B).  B is a multiple of 8, so the footprint touches at most 2 x 2
// cells, its corners: at most 4 bytes are read, every index clamped.
JPGE_HD int jpeg_roi_block_level(const JpegEncGeom& g, const JpegEncPlace& p, const uint8_t* levels, int By, int Bx, int B) {
    const int fx = p.c ? g.hmax : 1, fy = p.c ? g.vmax : 1;
    int x0 = p.bx * 8 * fx, x1 = x0 + 8 * fx - 1, y0 = p.by * 8 * fy, y1 = y0 + 8 * fy - 1;
    x0 = x0 > g.w - 1 ? g.w - 1 : x0;
    x1 = x1 > g.w - 1 ? g.w - 1 : x1;
    y0 = y0 > g.h - 1 ? g.h - 1 : y0;
    y1 = y1 > g.h - 1 ? g.h - 1 : y1;
    int cx0 = x0 / B, cx1 = x1 / B, cy0 = y0 / B, cy1 = y1 / B;
    cx0 = cx0 > Bx - 1 ? Bx - 1 : cx0;
    cx1 = cx1 > Bx - 1 ? Bx - 1 : cx1;
    cy0 = cy0 > By - 1 ? By - 1 : cy0;
    cy1 = cy1 > By - 1 ? By - 1 : cy1;
    const int a = levels[(size_t)cy0 * Bx + cx0], b = levels[(size_t)cy0 * Bx + cx1];
    const int c = levels[(size_t)cy1 * Bx + cx0], d = levels[(size_t)cy1 * Bx + cx1];
    const int top = a < b ? a : b, bottom = c < d ? c : d, level = top < bottom ? top : bottom;
    return level > JPGE_ROI_MAX_LEVEL ? JPGE_ROI_MAX_LEVEL : level;
}

// The quantiser of an AC coefficient of a block whose level has the scale `scale16`: 0 where the step scale16 / 16 times
// the table's would round to 0, else jpeg_quantise.  scale16 = 16 is jpeg_quantise for every input (d = 16 * q8 and q8 is
// a multiple of 8, so the test is "the quotient is 0").  16 * a <= 2^19 and d <= 4096 * 255 * 8 < 2^23: int32.
JPGE_HD int jpeg_quantise_roi(int coef, int table, int scale16) {
    const int a = coef < 0 ? -coef : coef, d = scale16 * (table << 3);
    return 16 * a + (d >> 1) < d ? 0 : jpeg_quantise(coef, table);
}

// natural index -> zig-zag position
JPGE_HD int jpeg_zigzag_of(int natural) {
    const uint8_t pos[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                             10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return pos[natural & 63];
}

// Entry i (natural order) of the quantisation table `which` (0 luma, 1 chroma): jpeg_set_quality(quality, force_baseline =
// TRUE) of the Annex K tables, (base * scale + 50) / 100 clamped to 1..255, scale = 5000 / quality below 50 and 200 - 2 *
// quality from there.
JPGE_HD int jpeg_quant_value(int quality, int which, int i) {
    const uint8_t base[2][64] = {
        {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
        {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    quality = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = (base[which & 1][i & 63] * scale + 50) / 100;
    return v < 1 ? 1 : (v > 255 ? 255 : v);
}

// ----------------------------------------------------------------------------- the symbol rule of a block
// A sink takes a block's symbols as indices into its table class's JPGE_HUFF_WORDS entries (`symbol`) and the magnitude
// bits behind them (`put`).  A sink that counts:
struct JpegBitCounter {
    uint32_t bits = 0;
    JPGE_HDM void put(uint32_t, int len) { bits += (uint32_t)len; }
    JPGE_HDM void symbol(const uint32_t* tab, int index) { bits += tab[index] & 31u; }
};

// A sink that writes at a bit offset into a frame's stream of 32-bit words, the first bit of the stream in bit 31 of
// word 0.  A word the block covers whole is stored; the word it shares with the block before it and the one it shares
// with the block after it are ORed into.  Nothing is written at or past `nwords`.
struct JpegBitWriter {
    uint32_t* words;
    uint32_t nwords, at;       // the word the accumulator goes to next
    uint64_t acc = 0;
    int n;                     // bits in the accumulator, the leading `lead` of them not this block's
    bool shared;               // the next word to go out is shared with the block before
    JPGE_HDM JpegBitWriter(uint32_t* w, uint32_t count, uint32_t bit_offset)
        : words(w), nwords(count), at(bit_offset >> 5), n((int)(bit_offset & 31)), shared((bit_offset & 31) != 0) {}
    JPGE_HDM void put(uint32_t code, int len) {
        acc = (acc << len) | (code & ((1u << len) - 1u));   // len <= 16
        n += len;
        if (n >= 32) {
            const uint32_t word = (uint32_t)(acc >> (n - 32));
            if (at < nwords) {
                if (shared) JPGE_OR(words + at, word);
                else words[at] = word;
            }
            shared = false;
            ++at;
            n -= 32;
            acc &= (1ull << n) - 1ull;
        }
    }
    JPGE_HDM void symbol(const uint32_t* tab, int index) {
        const uint32_t e = tab[index];
        put(e >> 5, (int)(e & 31));
    }
    JPGE_HDM void flush() {
        if (n > 0 && at < nwords) JPGE_OR(words + at, (uint32_t)(acc << (32 - n)));
    }
};

// A sink that tallies: entry `index` of the histogram the block is handed in the table's place goes up by one, the
// magnitude bits count for nothing.  On the device the histogram is the workgroup's, in LDS, and its blocks are other
// lanes (a vector atomic); on the host they are earlier iterations.
#if defined(__HIP_DEVICE_COMPILE__)
#define JPGE_INC(p) atomicAdd((p), 1u)
#else
#define JPGE_INC(p) (++*(p))
#endif
struct JpegSymbolTally {
    uint32_t* hist;            // JPGE_HUFF_WORDS entries of the block's table class
    JPGE_HDM void put(uint32_t, int) {}
    JPGE_HDM void symbol(const uint32_t*, int index) { JPGE_INC(hist + index); }
};

JPGE_HD int jpeg_category(int v) {
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// One block's symbols (T.81 F.1.2): the DC difference's category and bits, then per non-zero AC coefficient ZRLs for
// runs above 15, the (run, category) symbol and the bits; EOB unless coefficient 63 is not zero.  zz: the block in zig-zag
// order; tab: JPGE_HUFF_WORDS entries of the block's table class, (code << 5) | length, length 0 for a symbol the table
// does not have (nothing goes out for it).  A symbol's index is its category (DC) or 16 + its value (AC).
template <class Sink>
JPGE_HD void jpeg_encode_block(const int16_t* zz, int pred, const uint32_t* tab, Sink& sink) {
    int v = (int)zz[0] - pred, cat = jpeg_category(v);
    sink.symbol(tab, cat & 15);
    if (cat) sink.put((uint32_t)(v < 0 ? v + (1 << cat) - 1 : v), cat);
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        v = zz[k];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            sink.symbol(tab, 16 + 0xF0);
            run -= 16;
        }
        cat = jpeg_category(v);
        sink.symbol(tab, 16 + (((run << 4) | cat) & 255));
        sink.put((uint32_t)(v < 0 ? v + (1 << cat) - 1 : v), cat & 15);
        run = 0;
    }
    if (run) sink.symbol(tab, 16);
}

// ----------------------------------------------------------------------------- optimal tables (host planning work)
// jpeg_gen_optimal_table of libjpeg's jchuff.c (T.81 K.2) in plain C++: from the counts of a table's symbols to the
// DHT contents - the codes of each length 1..16 and the symbols in code order.  freq: `nsym` counts by symbol value (16
// for a DC table, 256 for an AC one), each below 2^26.  A reserved symbol 256 of frequency 1 keeps every real code from
// being all ones.  The two least frequent entries are merged until one is left, ties to the largest index; lengths
// above 16 are shortened by the rule of K.2 (figure K.3); the reserved symbol leaves the longest length; the symbols are
// listed by the length the merge gave them, by value within a length.  Returns the number of symbols, 0 for a histogram
// without one or for one whose longest code would pass 32 bits before limiting (libjpeg's JERR_HUFF_CLEN_OVERFLOW):
// nothing is written then.  `prelimit`, when not null, receives the longest length before limiting.
#define JPGE_OPT_MAX_CLEN 32
inline int jpeg_gen_optimal_table(const uint32_t* freq_in, int nsym, uint8_t* counts16, uint8_t* symbols, int* prelimit) {
    int64_t freq[257];
    int codesize[257], others[257], bits[JPGE_OPT_MAX_CLEN + 1];
    nsym = nsym < 0 ? 0 : (nsym > 256 ? 256 : nsym);
    bool any = false;
    for (int i = 0; i < 257; ++i) {
        freq[i] = i < nsym ? (int64_t)freq_in[i] : 0;
        any = any || freq[i] != 0;
        codesize[i] = 0;
        others[i] = -1;
    }
    if (!any) return 0;
    freq[256] = 1;
    int live[257], m = 0;       // the entries whose frequency is not zero, in ascending order: only they are searched
    for (int i = 0; i <= 256; ++i)
        if (freq[i]) live[m++] = i;
    for (;;) {
        int p1 = -1, p2 = -1;
        int64_t v = INT64_MAX;
        for (int k = 0; k < m; ++k) {
            if (freq[live[k]] <= v) {
                v = freq[live[k]];
                p1 = k;
            }
        }
        v = INT64_MAX;
        for (int k = 0; k < m; ++k) {
            if (freq[live[k]] <= v && k != p1) {
                v = freq[live[k]];
                p2 = k;
            }
        }
        if (p2 < 0) break;
        int c1 = live[p1], c2 = live[p2];
        freq[c1] += freq[c2];
        freq[c2] = 0;
        --m;
        for (int k = p2; k < m; ++k) live[k] = live[k + 1];
        ++codesize[c1];
        while (others[c1] >= 0) {
            c1 = others[c1];
            ++codesize[c1];
        }
        others[c1] = c2;
        ++codesize[c2];
        while (others[c2] >= 0) {
            c2 = others[c2];
            ++codesize[c2];
        }
    }
    for (int i = 0; i <= JPGE_OPT_MAX_CLEN; ++i) bits[i] = 0;
    int longest = 0;
    for (int i = 0; i <= 256; ++i) {
        if (codesize[i] > JPGE_OPT_MAX_CLEN) return 0;
        if (codesize[i]) ++bits[codesize[i]];
        longest = codesize[i] > longest ? codesize[i] : longest;
    }
    if (prelimit) *prelimit = longest;
    for (int i = JPGE_OPT_MAX_CLEN; i > 16; --i) {
        while (bits[i] > 0) {
            int j = i - 2;
            while (j > 0 && bits[j] == 0) --j;
            if (j == 0) return 0;       // cannot happen for a complete code; the walk stays inside the array
            bits[i] -= 2;
            bits[i - 1] += 1;
            bits[j + 1] += 2;
            bits[j] -= 1;
        }
    }
    int top = 16;
    while (top > 0 && bits[top] == 0) --top;
    if (top == 0) return 0;
    --bits[top];
    int p = 0;
    for (int len = 1; len <= JPGE_OPT_MAX_CLEN; ++len)
        for (int j = 0; j < 256; ++j)
            if (codesize[j] == len) symbols[p++] = (uint8_t)j;
    for (int len = 1; len <= 16; ++len) counts16[len - 1] = (uint8_t)bits[len];
    return p;
}

// The words the kernels look up, (code << 5) | length by symbol value, from a table's DHT contents (T.81 C.2): `tab`
// gets `entries` words (16 for DC, 256 for AC), 0 for a symbol the table does not have.  False where the counts and
// `nsym` do not agree, a code does not fit its length or a symbol has no entry.
inline bool jpeg_code_words(const uint8_t* counts16, const uint8_t* symbols, int nsym, uint32_t* tab, int entries) {
    for (int i = 0; i < entries; ++i) tab[i] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int c = 0; c < counts16[len - 1]; ++c) {
            if (k >= nsym || symbols[k] >= entries || code >= (1u << len)) return false;
            tab[symbols[k++]] = (code << 5) | (uint32_t)len;
            ++code;
        }
        code <<= 1;
    }
    return k == nsym;
}

// A frame's tables from its histograms.  hist: u32 [2, JPGE_HUFF_WORDS] in the layout of the code tables; classes: 1
// for a gray frame (class 1 is left alone: its outputs are zeroed), 2 for colour.  counts u8 [2, 2, 16] and symbols u8
// [2, 2, 256] by class and kind (0 DC, 1 AC), nsym int [2, 2], ehuff u32 [2, JPGE_HUFF_WORDS].  Returns 0, or 1 + the
// index 2 * class + kind of the first table that has no symbol.
inline int jpeg_frame_optimal_tables(const uint32_t* hist, int classes, uint8_t* counts, uint8_t* symbols, int* nsym, uint32_t* ehuff) {
    for (int i = 0; i < 2 * 2 * 16; ++i) counts[i] = 0;
    for (int i = 0; i < 2 * 2 * 256; ++i) symbols[i] = 0;
    for (int i = 0; i < 2 * JPGE_HUFF_WORDS; ++i) ehuff[i] = 0;
    for (int i = 0; i < 4; ++i) nsym[i] = 0;
    for (int t = 0; t < classes && t < 2; ++t) {
        for (int kind = 0; kind < 2; ++kind) {
            const int at = 2 * t + kind, entries = kind ? 256 : 16;
            const uint32_t* freq = hist + t * JPGE_HUFF_WORDS + (kind ? 16 : 0);
            nsym[at] = jpeg_gen_optimal_table(freq, entries, counts + at * 16, symbols + at * 256, nullptr);
            if (nsym[at] == 0) return 1 + at;
            if (!jpeg_code_words(counts + at * 16, symbols + at * 256, nsym[at], ehuff + t * JPGE_HUFF_WORDS + (kind ? 16 : 0), entries)) return 1 + at;
        }
    }
    return 0;
}
