// Host check of the restart intervals of csrc/jpeg_encode.h, the text the kernels of csrc/jpeg_write.hip run: every case
// of the restart corpus (python tests/_jpeg_restart_ref.py dump FILE) is walked the way the kernels walk it behind the
// transform - per (segment, block of the segment): the bit length with the predictor jpeg_enc_pred_block gives, zero
// lengths past the blocks of the last segment, the prefix sum of a segment's row; every segment's words planned from its
// own bit count, so that no two segments share a word; every block written at its own bit offset into words that were
// cleared, the segments and their blocks in an order that is not the stream's; the FF counts per chunk, the sizes, and
// the stuffing with RSTm or EOI behind every segment - over buffers of exactly the size the kernels get, and compared with
// the statement's coefficients and its bytes from SOS to the end of the file.  Meant to be built with the address and
// undefined-behaviour sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_restart_check.cpp -o check
//   ./check FILE
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../elvis_amd/csrc/jpeg_encode.h"

namespace {

constexpr uint32_t kStuffChunk = 1024;      // ELVIS_JPEG_STUFF_CHUNK

struct Reader {
    FILE* f;
    uint32_t u32() {
        uint32_t v = 0;
        if (fread(&v, 4, 1, f) != 1) {
            fprintf(stderr, "short read\n");
            exit(2);
        }
        return v;
    }
    std::vector<uint8_t> blob() {
        std::vector<uint8_t> b(u32());
        if (!b.empty() && fread(b.data(), 1, b.size(), f) != b.size()) {
            fprintf(stderr, "short read\n");
            exit(2);
        }
        return b;
    }
};

// The segments in an order that is not the stream's: the odd ones downwards, then the even ones.
std::vector<int> shuffled(int count) {
    std::vector<int> order;
    for (int pass = 0; pass < 2; ++pass)
        for (int s = count - 1 - pass; s >= 0; s -= 2) order.push_back(s);
    return order;
}

bool run_case(const std::string& name, int h, int w, int channels, int order, int quality, int sampling, int restart_mcus,
              const std::vector<uint8_t>& pixels, const std::vector<uint8_t>& ehuff_bytes, const std::vector<uint8_t>& want_coef,
              const std::vector<uint8_t>& want_scan) {
    const JpegEncGeom g = jpeg_enc_restart(jpeg_enc_geometry(h, w, channels, order, sampling), restart_mcus);
    if (pixels.size() != (size_t)h * w * channels || ehuff_bytes.size() != 2 * JPGE_HUFF_WORDS * 4 || want_coef.size() != (size_t)g.blocks * 128) {
        fprintf(stderr, "%s: bad case sizes (blocks %d)\n", name.c_str(), g.blocks);
        return false;
    }
    const int mcus = g.mcux * g.mcuy;
    if (g.segs < 1 || g.segb < 1 || (long long)(g.segs - 1) * g.segb >= g.blocks || (long long)g.segs * g.segb < g.blocks ||
        (g.segs > 1 && (g.segb != restart_mcus * g.bpm || g.segs != (mcus + restart_mcus - 1) / restart_mcus))) {
        fprintf(stderr, "%s: %d segments of %d blocks do not tile %d blocks\n", name.c_str(), g.segs, g.segb, g.blocks);
        return false;
    }
    std::vector<uint32_t> ehuff(2 * JPGE_HUFF_WORDS);
    memcpy(ehuff.data(), ehuff_bytes.data(), ehuff_bytes.size());
    uint16_t qt[2][64];
    for (int i = 0; i < 128; ++i) qt[i >> 6][i & 63] = (uint16_t)jpeg_quant_value(quality, i >> 6, i & 63);
    // the transform kernel: the same with and without an interval
    std::vector<int16_t> coef((size_t)g.blocks * 64);
    for (int b = 0; b < g.blocks; ++b) {
        const JpegEncPlace p = jpeg_enc_place(g, b);
        int ws[72];
        for (int lane = 0; lane < 8; ++lane) {
            int d[8], o[8];
            for (int x = 0; x < 8; ++x) d[x] = jpeg_enc_sample(pixels.data(), g, p.c, p.by * 8 + lane, p.bx * 8 + x) - 128;
            jpeg_fdct_pass<true>(d, o);
            for (int x = 0; x < 8; ++x) ws[lane * 9 + x] = o[x];
        }
        for (int lane = 0; lane < 8; ++lane) {
            int d[8], o[8];
            for (int i = 0; i < 8; ++i) d[i] = ws[i * 9 + lane];
            jpeg_fdct_pass<false>(d, o);
            for (int i = 0; i < 8; ++i) {
                const int nat = i * 8 + lane, q = jpeg_quantise(o[i], qt[p.c ? 1 : 0][nat]);
                coef[(size_t)b * 64 + jpeg_zigzag_of(nat)] = (int16_t)((p.dummy && nat) ? 0 : q);
            }
        }
    }
    if (memcmp(coef.data(), want_coef.data(), want_coef.size()) != 0) {
        fprintf(stderr, "%s: the coefficients are not the statement's\n", name.c_str());
        return false;
    }
    const std::vector<int> seg_order = shuffled(g.segs);
    const size_t row = (size_t)g.segb + 1;
    // the bit-length kernel, a lane per (segment, block of the segment), and the prefix sum of every row
    std::vector<uint32_t> bits((size_t)g.segs * row);
    for (int s : seg_order) {
        if (jpeg_enc_seg_blocks(g, s) < 1) {
            fprintf(stderr, "%s: segment %d is empty\n", name.c_str(), s);
            return false;
        }
        for (int i = g.segb - 1; i >= 0; --i) {
            const int b = s * g.segb + i;
            if (b >= g.blocks) {
                bits[s * row + i] = 0u;
                continue;
            }
            const int pb = jpeg_enc_pred_block(g, b);
            if (pb >= b || (pb >= 0 && pb < s * g.segb)) {
                fprintf(stderr, "%s: block %d of segment %d is predicted from block %d\n", name.c_str(), b, s, pb);
                return false;
            }
            JpegBitCounter count;
            jpeg_encode_block(coef.data() + (size_t)b * 64, pb >= 0 ? coef[(size_t)pb * 64] : 0, ehuff.data() + JPGE_HUFF_WORDS * jpeg_enc_table_class(g, b),
                              count);
            if (count.bits > JPGE_MAX_BLOCK_BITS) {
                fprintf(stderr, "%s: block %d has %u bits\n", name.c_str(), b, count.bits);
                return false;
            }
            bits[s * row + i] = count.bits;
        }
        uint32_t at = 0;
        for (int i = 0; i < g.segb; ++i) {
            const uint32_t v = bits[s * row + i];
            bits[s * row + i] = at;
            at += v;
        }
        bits[s * row + g.segb] = at;
    }
    // the host's plan: a span of whole words for every segment
    std::vector<long long> word_off((size_t)g.segs + 1, 0);
    uint32_t longest = 0;
    for (int s = 0; s < g.segs; ++s) {
        const uint32_t nbytes = (bits[s * row + g.segb] + 7) >> 3;
        word_off[s + 1] = word_off[s] + (nbytes + 3) / 4;
        longest = nbytes > longest ? nbytes : longest;
    }
    const int chunks = (int)((longest + kStuffChunk - 1) / kStuffChunk) > 1 ? (int)((longest + kStuffChunk - 1) / kStuffChunk) : 1;
    // the clear and the pack kernel over exactly those words
    std::vector<uint32_t> words((size_t)word_off[g.segs], 0u);
    for (int s : seg_order) {
        for (int pass = 0; pass < 2; ++pass) {
            for (int i = g.segb - 1 - pass; i >= 0; i -= 2) {
                const int b = s * g.segb + i;
                if (b >= g.blocks) continue;
                const int pb = jpeg_enc_pred_block(g, b);
                JpegBitWriter out(words.data() + word_off[s], (uint32_t)(word_off[s + 1] - word_off[s]), bits[s * row + i]);
                jpeg_encode_block(coef.data() + (size_t)b * 64, pb >= 0 ? coef[(size_t)pb * 64] : 0,
                                  ehuff.data() + JPGE_HUFF_WORDS * jpeg_enc_table_class(g, b), out);
                if (i == g.segb - 1 || b == g.blocks - 1) {
                    const int pad = (8 - (out.n & 7)) & 7;
                    out.put((1u << pad) - 1u, pad);
                }
                out.flush();
            }
        }
    }
    // the FF counts per chunk, their prefix sums, and the sizes
    std::vector<uint32_t> ffc((size_t)g.segs * (chunks + 1)), sizes((size_t)g.segs);
    for (int s : seg_order) {
        const uint32_t nbytes = (bits[s * row + g.segb] + 7) >> 3;
        uint32_t at = 0;
        for (int c = 0; c < chunks; ++c) {
            uint32_t count = 0;
            for (uint32_t j = c * kStuffChunk; j < (c + 1) * kStuffChunk && j < nbytes; ++j)
                count += ((words[(size_t)word_off[s] + (j >> 2)] >> (24 - 8 * (j & 3))) & 0xffu) == 0xffu;
            ffc[(size_t)s * (chunks + 1) + c] = at;
            at += count;
        }
        ffc[(size_t)s * (chunks + 1) + chunks] = at;
        sizes[s] = nbytes + at + 2u;
    }
    std::vector<long long> out_off((size_t)g.segs + 1, 0);
    for (int s = 0; s < g.segs; ++s) out_off[s + 1] = out_off[s] + sizes[s];
    // the stuffing pass, a chunk at a time, into exactly the bytes the sizes add up to
    std::vector<uint8_t> scan((size_t)out_off[g.segs], 0xa5);
    for (int s : seg_order) {
        const uint32_t nbytes = (bits[s * row + g.segb] + 7) >> 3;
        const long long first = out_off[s], end = out_off[s + 1];
        for (int c = chunks - 1; c >= 0; --c) {
            long long at = first + (long long)c * kStuffChunk + ffc[(size_t)s * (chunks + 1) + c];
            for (uint32_t j = c * kStuffChunk; j < (c + 1) * kStuffChunk && j < nbytes; ++j) {
                const uint8_t byte = (uint8_t)(words[(size_t)word_off[s] + (j >> 2)] >> (24 - 8 * (j & 3)));
                if (at < end) scan[at] = byte;
                ++at;
                if (byte == 0xff) {
                    if (at < end) scan[at] = 0;
                    ++at;
                }
            }
        }
        const long long mark = first + nbytes + ffc[(size_t)s * (chunks + 1) + chunks];
        if (mark < first || mark + 2 > end) {
            fprintf(stderr, "%s: segment %d has no room for its marker\n", name.c_str(), s);
            return false;
        }
        scan[mark] = 0xff;
        scan[mark + 1] = (uint8_t)jpeg_enc_seg_marker(g, s);
    }
    if (scan != want_scan) {
        fprintf(stderr, "%s: the scan has %zu bytes, the statement's %zu, or they differ\n", name.c_str(), scan.size(), want_scan.size());
        return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s FILE   (python tests/_jpeg_restart_ref.py dump FILE)\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    Reader r{f};
    const uint32_t n = r.u32();
    uint32_t bad = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const std::vector<uint8_t> name = r.blob();
        int v[7];
        for (int& x : v) x = (int)r.u32();
        const std::vector<uint8_t> pixels = r.blob(), ehuff = r.blob(), coef = r.blob(), scan = r.blob();
        if (!run_case(std::string(name.begin(), name.end()), v[0], v[1], v[2], v[3], v[4], v[5], v[6], pixels, ehuff, coef, scan)) ++bad;
    }
    fclose(f);
    printf("%u cases, %u failed\n", n, bad);
    return bad ? 1 : 0;
}
