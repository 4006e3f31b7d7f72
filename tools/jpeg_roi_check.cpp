// Host check of the per-block rate allocation of csrc/jpeg_encode.h, the text jpeg_fdct_kernel of csrc/jpeg_write.hip runs
// with a map of ROI levels: every case of the ROI corpus (python tests/_jpeg_roi_ref.py dump FILE) is walked the way the
// kernel walks it - per block the place, the level from jpeg_roi_block_level over a map of exactly by * bx bytes, the two
// passes of the transform, jpeg_quantise for DC and jpeg_quantise_roi for AC, the dummy blocks' zeros - over buffers of
// exactly the size the kernel gets, and the coefficients are compared with the statement's.  Level 0 is checked against
// jpeg_quantise for every coefficient met, and the table of jpeg_roi_scale16 against round(16 * 2^(L / 6)) in exact
// integers.  Meant to be built with the address and undefined-behaviour sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_roi_check.cpp -o check
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

// v = round(16 * 2^(level / 6)), half up: (2 v - 1)^6 <= 32^6 * 2^level < (2 v + 1)^6, in 128-bit integers.
bool is_scale16(int level, long long v) {
    auto pow6 = [](unsigned __int128 x) { return x * x * x * x * x * x; };
    const unsigned __int128 rhs = pow6(32) << level;
    return pow6((unsigned __int128)(2 * v - 1)) <= rhs && rhs < pow6((unsigned __int128)(2 * v + 1));
}

bool run_case(const std::string& name, int h, int w, int channels, int order, int quality, int sampling, int B, int By, int Bx,
              const std::vector<uint8_t>& pixels, const std::vector<uint8_t>& levels, const std::vector<uint8_t>& want_coef) {
    const JpegEncGeom g = jpeg_enc_geometry(h, w, channels, order, sampling);
    if (pixels.size() != (size_t)h * w * channels || levels.size() != (size_t)By * Bx || want_coef.size() != (size_t)g.blocks * 128 || B < 8 || B % 8 ||
        (By != (h / B > 1 ? h / B : 1) && By != (h + B - 1) / B) || (Bx != (w / B > 1 ? w / B : 1) && Bx != (w + B - 1) / B)) {
        fprintf(stderr, "%s: bad case sizes (blocks %d, grid %d x %d of %d)\n", name.c_str(), g.blocks, By, Bx, B);
        return false;
    }
    uint16_t qt[2][64];
    for (int i = 0; i < 128; ++i) qt[i >> 6][i & 63] = (uint16_t)jpeg_quant_value(quality, i >> 6, i & 63);
    std::vector<int16_t> coef((size_t)g.blocks * 64);
    for (int b = 0; b < g.blocks; ++b) {
        const JpegEncPlace p = jpeg_enc_place(g, b);
        const int level = jpeg_roi_block_level(g, p, levels.data(), By, Bx, B);
        if (level < 0 || level > JPGE_ROI_MAX_LEVEL) {
            fprintf(stderr, "%s: block %d has level %d\n", name.c_str(), b, level);
            return false;
        }
        const int scale16 = jpeg_roi_scale16(level);
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
                const int nat = i * 8 + lane, table = qt[p.c ? 1 : 0][nat];
                const int q = nat ? jpeg_quantise_roi(o[i], table, scale16) : jpeg_quantise(o[i], table);
                if (jpeg_quantise_roi(o[i], table, 16) != jpeg_quantise(o[i], table)) {
                    fprintf(stderr, "%s: level 0 is not the plain quantiser for %d / %d\n", name.c_str(), o[i], table);
                    return false;
                }
                coef[(size_t)b * 64 + jpeg_zigzag_of(nat)] = (int16_t)((p.dummy && nat) ? 0 : q);
            }
        }
    }
    if (memcmp(coef.data(), want_coef.data(), want_coef.size()) != 0) {
        fprintf(stderr, "%s: the coefficients are not the statement's\n", name.c_str());
        return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s FILE   (python tests/_jpeg_roi_ref.py dump FILE)\n", argv[0]);
        return 2;
    }
    for (int level = 0; level <= JPGE_ROI_MAX_LEVEL; ++level) {
        if (!is_scale16(level, jpeg_roi_scale16(level))) {
            fprintf(stderr, "scale16(%d) = %d is not round(16 * 2^(%d / 6))\n", level, jpeg_roi_scale16(level), level);
            return 1;
        }
    }
    if (jpeg_roi_scale16(-1) != 16 || jpeg_roi_scale16(JPGE_ROI_MAX_LEVEL + 1) != 4096 || jpeg_roi_scale16(255) != 4096) {
        fprintf(stderr, "scale16 does not clamp its level\n");
        return 1;
    }
    printf("scale16 table ok\n");
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
        int v[9];
        for (int& x : v) x = (int)r.u32();
        const std::vector<uint8_t> pixels = r.blob(), levels = r.blob(), coef = r.blob();
        if (!run_case(std::string(name.begin(), name.end()), v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], pixels, levels, coef)) ++bad;
    }
    fclose(f);
    printf("%u cases, %u failed\n", n, bad);
    return bad ? 1 : 0;
}
