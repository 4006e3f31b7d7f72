// Host check of the per-frame optimised Huffman tables of csrc/jpeg_encode.h, the text jpeg_bits_kernel (bit count and
// tally mode) and jpeg_pack_kernel of csrc/jpeg_write.hip run: every case of the corpus (python tests/_jpeg_opt_ref.py dump
// FILE) is walked the way the kernels walk it, over buffers of exactly the size the kernels get -
//   the tally: per segment and workgroup of 256 blocks a histogram of 2 * 272 words (the LDS one) through
//     JpegSymbolTally, its non-zero entries added to the frame's 2 * 272 words; compared with the statement's counts;
//   the table builder: jpeg_frame_optimal_tables over that histogram into exact-size outputs; counts, symbols, how many
//     and the code words compared with the statement's; jpeg_gen_optimal_table on an empty histogram, on one symbol, on two,
//     and on Fibonacci counts up to a length of 32 before limiting;
//   the bit count and the pack with the frame's own words, the FF counts and the stuffing pass as tools/
//     jpeg_restart_check.cpp has them; the scan compared with the statement's.
// Meant to be built with the address and undefined-behaviour sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_opt_check.cpp -o check
//   ./check FILE
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../elvis_amd/csrc/jpeg_encode.h"

namespace {

constexpr uint32_t kStuffChunk = 1024;
constexpr int kBlockThreads = 256;

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

// The Kraft sum of a table's counts in units of 2^-16: a prefix code has at most 65536, and one that keeps the all-ones
// code free has less.
long kraft16(const uint8_t* counts16) {
    long sum = 0;
    for (int len = 1; len <= 16; ++len) sum += (long)counts16[len - 1] << (16 - len);
    return sum;
}

bool builder_edges() {
    // exact-size outputs: an AC table of n symbols writes n symbol bytes and 16 counts
    uint32_t freq[256];
    for (uint32_t& v : freq) v = 0;
    std::vector<uint8_t> counts(16, 0xa5), none;
    int prelimit = -1;
    if (jpeg_gen_optimal_table(freq, 256, counts.data(), none.data(), &prelimit) != 0 || counts[0] != 0xa5) {
        fprintf(stderr, "an empty histogram is not refused\n");
        return false;
    }
    freq[0x21] = 7;
    std::vector<uint8_t> one(1);
    if (jpeg_gen_optimal_table(freq, 256, counts.data(), one.data(), &prelimit) != 1 || one[0] != 0x21 || counts[0] != 1 || prelimit != 1) {
        fprintf(stderr, "one symbol does not get the code 0\n");
        return false;
    }
    freq[0xf0] = 7;
    std::vector<uint8_t> two(2);
    if (jpeg_gen_optimal_table(freq, 256, counts.data(), two.data(), &prelimit) != 2 || two[0] != 0x21 || two[1] != 0xf0 || counts[0] != 1 ||
        counts[1] != 1 || prelimit != 2) {
        fprintf(stderr, "two symbols do not get the codes 0 and 10\n");
        return false;
    }
    // Fibonacci counts: with the reserved symbol the longest code before limiting has as many bits as there are symbols
    for (int n = 3; n <= 33; ++n) {
        for (uint32_t& v : freq) v = 0;
        uint32_t a = 1, b = 2;
        for (int k = 0; k < n; ++k) {
            freq[(k * 255) / (n - 1)] = a;
            const uint32_t next = a + b;
            a = b;
            b = next;
        }
        std::vector<uint8_t> syms((size_t)n);
        prelimit = -1;
        const int got = jpeg_gen_optimal_table(freq, 256, counts.data(), syms.data(), &prelimit);
        if (n == 33) {
            if (got != 0) {
                fprintf(stderr, "a code of 33 bits before limiting is not refused\n");
                return false;
            }
            continue;
        }
        int total = 0;
        for (int len = 0; len < 16; ++len) total += counts[len];
        uint32_t words[256];
        if (got != n || prelimit != n || total != n || kraft16(counts.data()) >= 65536 || !jpeg_code_words(counts.data(), syms.data(), n, words, 256)) {
            fprintf(stderr, "%d Fibonacci counts: %d symbols, %d bits before limiting, %d codes, Kraft %ld\n", n, got, prelimit, total, kraft16(counts.data()));
            return false;
        }
    }
    return true;
}

bool run_case(const std::string& name, int h, int w, int channels, int sampling, int restart_mcus, const std::vector<uint8_t>& coef_bytes,
              const std::vector<uint8_t>& want_hist, const std::vector<uint8_t>& want_counts, const std::vector<uint8_t>& want_symbols,
              const std::vector<uint8_t>& want_nsym, const std::vector<uint8_t>& want_words, const std::vector<uint8_t>& want_scan) {
    const JpegEncGeom g = jpeg_enc_restart(jpeg_enc_geometry(h, w, channels, 0, sampling), restart_mcus);
    if (coef_bytes.size() != (size_t)g.blocks * 128 || want_hist.size() != 2 * JPGE_HUFF_WORDS * 4 || want_counts.size() != 64 ||
        want_symbols.size() != 1024 || want_nsym.size() != 16 || want_words.size() != 2 * JPGE_HUFF_WORDS * 4) {
        fprintf(stderr, "%s: bad case sizes (blocks %d)\n", name.c_str(), g.blocks);
        return false;
    }
    std::vector<int16_t> coef((size_t)g.blocks * 64);
    memcpy(coef.data(), coef_bytes.data(), coef_bytes.size());
    const size_t row = (size_t)g.segb + 1;
    // the tally mode: a workgroup's histogram, then its non-zero entries into the frame's
    std::vector<uint32_t> hist(2 * JPGE_HUFF_WORDS, 0u);
    for (int s = g.segs - 1; s >= 0; --s) {
        for (int first = 0; first < g.segb; first += kBlockThreads) {
            std::vector<uint32_t> lds(2 * JPGE_HUFF_WORDS, 0u);
            for (int i = first; i < first + kBlockThreads; ++i) {
                const int b = s * g.segb + i;
                if (i >= g.segb || b >= g.blocks) continue;
                const int pb = jpeg_enc_pred_block(g, b);
                JpegSymbolTally tally{lds.data() + JPGE_HUFF_WORDS * jpeg_enc_table_class(g, b)};
                jpeg_encode_block(coef.data() + (size_t)b * 64, pb >= 0 ? coef[(size_t)pb * 64] : 0, lds.data(), tally);
            }
            for (int k = 0; k < 2 * JPGE_HUFF_WORDS; ++k)
                if (lds[k]) hist[k] += lds[k];
        }
    }
    if (memcmp(hist.data(), want_hist.data(), want_hist.size()) != 0) {
        fprintf(stderr, "%s: the histograms are not the statement's\n", name.c_str());
        return false;
    }
    // the table builder
    std::vector<uint8_t> counts(64, 0xa5), symbols(1024, 0xa5);
    std::vector<int> nsym(4, -1);
    std::vector<uint32_t> ehuff(2 * JPGE_HUFF_WORDS, 0xa5a5a5a5u);
    if (jpeg_frame_optimal_tables(hist.data(), channels == 3 ? 2 : 1, counts.data(), symbols.data(), nsym.data(), ehuff.data()) != 0) {
        fprintf(stderr, "%s: the builder refuses the histograms\n", name.c_str());
        return false;
    }
    if (memcmp(counts.data(), want_counts.data(), 64) != 0 || memcmp(symbols.data(), want_symbols.data(), 1024) != 0 ||
        memcmp(nsym.data(), want_nsym.data(), 16) != 0 || memcmp(ehuff.data(), want_words.data(), want_words.size()) != 0) {
        fprintf(stderr, "%s: the tables are not the statement's\n", name.c_str());
        return false;
    }
    for (int t = 0; t < (channels == 3 ? 4 : 2); ++t) {
        if (kraft16(counts.data() + t * 16) >= 65536) {
            fprintf(stderr, "%s: table %d is no prefix code with a free all-ones code\n", name.c_str(), t);
            return false;
        }
    }
    // the bit-length kernel with the frame's own words, and the prefix sum of every row
    std::vector<uint32_t> bits((size_t)g.segs * row);
    for (int s = 0; s < g.segs; ++s) {
        for (int i = g.segb - 1; i >= 0; --i) {
            const int b = s * g.segb + i;
            if (b >= g.blocks) {
                bits[s * row + i] = 0u;
                continue;
            }
            const int pb = jpeg_enc_pred_block(g, b);
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
    for (int s = g.segs - 1; s >= 0; --s) {
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
    // the FF counts, the sizes and the stuffing pass into exactly the bytes the sizes add up to
    std::vector<uint32_t> ffc((size_t)g.segs * (chunks + 1)), sizes((size_t)g.segs);
    for (int s = 0; s < g.segs; ++s) {
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
    std::vector<uint8_t> scan((size_t)out_off[g.segs], 0xa5);
    for (int s = 0; s < g.segs; ++s) {
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
        fprintf(stderr, "usage: %s FILE   (python tests/_jpeg_opt_ref.py dump FILE)\n", argv[0]);
        return 2;
    }
    if (!builder_edges()) return 1;
    printf("builder edges ok\n");
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
        int v[5];
        for (int& x : v) x = (int)r.u32();
        const std::vector<uint8_t> coef = r.blob(), hist = r.blob(), counts = r.blob(), symbols = r.blob(), nsym = r.blob(), words = r.blob(), scan = r.blob();
        if (!run_case(std::string(name.begin(), name.end()), v[0], v[1], v[2], v[3], v[4], coef, hist, counts, symbols, nsym, words, scan)) ++bad;
    }
    fclose(f);
    printf("%u cases, %u failed\n", n, bad);
    return bad ? 1 : 0;
}
