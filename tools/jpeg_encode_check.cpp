// Host check of csrc/jpeg_encode.h, the text the kernels of csrc/jpeg_write.hip run: every case of the writer's corpus
// (python tests/_jpeg_write_ref.py dump FILE) is walked the way the kernels walk it - a row pass per (block, row), the
// transpose, a column pass per (block, column), the quantiser and the zig-zag; a bit count per block and the prefix sum;
// every block written at its own bit offset into words that were cleared; the stuffing - over buffers of exactly the
// size the kernels get, and compared with the statement's coefficients and scan.  Meant to be built with the address and
// undefined-behaviour sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_encode_check.cpp -o check
//   ./check FILE
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../elvis_amd/csrc/jpeg_encode.h"

namespace {

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

bool run_case(const std::string& name, int h, int w, int channels, int order, int quality, int sampling, const std::vector<uint8_t>& pixels,
              const std::vector<uint8_t>& ehuff_bytes, const std::vector<uint8_t>& want_coef, const std::vector<uint8_t>& want_scan) {
    JpegEncGeom g = jpeg_enc_geometry(h, w, channels, order, sampling);
    if (pixels.size() != (size_t)h * w * channels || ehuff_bytes.size() != 2 * JPGE_HUFF_WORDS * 4 || want_coef.size() != (size_t)g.blocks * 128) {
        fprintf(stderr, "%s: bad case sizes (blocks %d)\n", name.c_str(), g.blocks);
        return false;
    }
    std::vector<uint32_t> ehuff(2 * JPGE_HUFF_WORDS);
    memcpy(ehuff.data(), ehuff_bytes.data(), ehuff_bytes.size());
    uint16_t qt[2][64];
    for (int i = 0; i < 128; ++i) qt[i >> 6][i & 63] = (uint16_t)jpeg_quant_value(quality, i >> 6, i & 63);
    // the transform kernel
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
        for (size_t i = 0; i < coef.size(); ++i) {
            int16_t want;
            memcpy(&want, want_coef.data() + 2 * i, 2);
            if (want != coef[i]) {
                fprintf(stderr, "%s: block %zu coefficient %zu is %d, the statement says %d\n", name.c_str(), i / 64, i % 64, coef[i], want);
                break;
            }
        }
        return false;
    }
    // the bit-length kernel and the prefix sum
    std::vector<uint32_t> bits((size_t)g.blocks + 1);
    uint32_t at = 0;
    for (int b = 0; b < g.blocks; ++b) {
        const int pb = jpeg_enc_pred_block(g, b);
        JpegBitCounter count;
        jpeg_encode_block(coef.data() + (size_t)b * 64, pb >= 0 ? coef[(size_t)pb * 64] : 0, ehuff.data() + JPGE_HUFF_WORDS * jpeg_enc_table_class(g, b),
                          count);
        if (count.bits > JPGE_MAX_BLOCK_BITS) {
            fprintf(stderr, "%s: block %d has %u bits\n", name.c_str(), b, count.bits);
            return false;
        }
        bits[b] = at;
        at += count.bits;
    }
    bits[g.blocks] = at;
    // the pack kernel, over exactly the words the host plans for the frame; the blocks in an order that is not the stream's
    const uint32_t nbytes = (at + 7) >> 3;
    std::vector<uint32_t> words((nbytes + 3) / 4, 0u);
    for (int pass = 0; pass < 2; ++pass) {
        for (int b = g.blocks - 1 - pass; b >= 0; b -= 2) {
            const int pb = jpeg_enc_pred_block(g, b);
            JpegBitWriter out(words.data(), (uint32_t)words.size(), bits[b]);
            jpeg_encode_block(coef.data() + (size_t)b * 64, pb >= 0 ? coef[(size_t)pb * 64] : 0,
                              ehuff.data() + JPGE_HUFF_WORDS * jpeg_enc_table_class(g, b), out);
            if (b == g.blocks - 1) {
                const int pad = (8 - (out.n & 7)) & 7;
                out.put((1u << pad) - 1u, pad);
            }
            out.flush();
        }
    }
    // the stuffing pass
    std::vector<uint8_t> scan;
    for (uint32_t j = 0; j < nbytes; ++j) {
        const uint8_t byte = (uint8_t)(words[j >> 2] >> (24 - 8 * (j & 3)));
        scan.push_back(byte);
        if (byte == 0xff) scan.push_back(0);
    }
    scan.push_back(0xff);
    scan.push_back(0xd9);
    if (scan != want_scan) {
        fprintf(stderr, "%s: the scan has %zu bytes, the statement's %zu, or they differ\n", name.c_str(), scan.size(), want_scan.size());
        return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s FILE   (python tests/_jpeg_write_ref.py dump FILE)\n", argv[0]);
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
        int v[6];
        for (int& x : v) x = (int)r.u32();
        const std::vector<uint8_t> pixels = r.blob(), ehuff = r.blob(), coef = r.blob(), scan = r.blob();
        if (!run_case(std::string(name.begin(), name.end()), v[0], v[1], v[2], v[3], v[4], v[5], pixels, ehuff, coef, scan)) ++bad;
    }
    fclose(f);
    printf("%u cases, %u failed\n", n, bad);
    return bad ? 1 : 0;
}
