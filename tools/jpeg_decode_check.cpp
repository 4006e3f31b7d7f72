// The decoder of csrc/jpeg_read.hip's jpeg_tables_kernel and jpeg_entropy_kernel (csrc/jpeg_decode.h, the very functions
// the kernels call) walked on the host over every file of the test corpus - the well-formed ones and the malformed
// ones that only the device can tell - with buffers of exactly the size the entry points are handed: the file's own
// bytes, its segment table, frame descriptor, Huffman and quantisation tables in, `stride_blocks` coefficient blocks and
// two status words a segment out.  For every case the coefficients and the status words are compared with the
// statement's (tests/_jpeg_ref.py).  Meant to be built with the address and undefined-behaviour sanitizers and run as it
// is:
//
//     python tests/_jpeg_ref.py dump corpus.bin
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_decode_check.cpp -o jpeg_decode_check
//     ./jpeg_decode_check corpus.bin
//
// A read outside the file, a store outside the coefficient buffer, or an index outside a table stops it.  The malformed
// cases go to a GPU only after they have passed here.  Every case is also run with its segments cut short at every
// length up to 24 bytes and with a descriptor that does not fit: whatever the bytes, nothing outside the buffers is
// touched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../elvis_amd/csrc/jpeg_decode.h"

static bool read_u32(FILE* f, uint32_t* v) {
    unsigned char b[4];
    if (std::fread(b, 1, 4, f) != 4) return false;
    *v = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
    return true;
}

// an exactly sized heap copy, so that the sanitizer sees every byte past its end
template <typename T>
static T* read_blob(FILE* f, size_t* count) {
    uint32_t bytes = 0;
    if (!read_u32(f, &bytes)) std::exit(2);
    T* p = (T*)std::malloc(bytes ? bytes : 1);
    if (bytes && std::fread(p, 1, bytes, f) != bytes) std::exit(2);
    *count = bytes / sizeof(T);
    return p;
}

// what jpeg_entropy_kernel does for segment s
static void run_segment(const uint8_t* file, size_t file_bytes, const int32_t* segs, size_t s, const int32_t* fd, const JpegTable* tables,
                        const uint16_t* qt, int16_t* coef, long long stride_blocks, uint32_t* st, long long len_override = -1) {
    const int32_t* sd = segs + JPG_SEG_WORDS * s;
    const long long off = sd[0], len = len_override >= 0 ? len_override : sd[1];
    if (sd[4] != 0 || off < 0 || len < 0 || off > (long long)file_bytes - len || !jpeg_fd_ok(fd, stride_blocks)) {
        st[0] = JPG_E_DESC;
        st[1] = 0;
        return;
    }
    jpeg_decode_segment(file + off, (uint32_t)len, fd, tables, qt, sd[2], sd[3], coef, stride_blocks, st);
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: jpeg_decode_check CORPUS (written by python tests/_jpeg_ref.py dump CORPUS)\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "jpeg_decode_check: cannot open %s\n", argv[1]);
        return 2;
    }
    uint32_t count = 0;
    if (!read_u32(f, &count)) return 2;
    int failures = 0, malformed = 0;
    size_t segments = 0;
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t name_len = 0;
        if (!read_u32(f, &name_len)) return 2;
        std::string name(name_len, ' ');
        if (std::fread(&name[0], 1, name_len, f) != name_len) return 2;
        size_t file_bytes, seg_words, fd_words, huff_bytes, qt_words, status_words, coef_words;
        uint8_t* file = read_blob<uint8_t>(f, &file_bytes);
        int32_t* segs = read_blob<int32_t>(f, &seg_words);
        int32_t* fd = read_blob<int32_t>(f, &fd_words);
        uint8_t* huff = read_blob<uint8_t>(f, &huff_bytes);
        uint16_t* qt = read_blob<uint16_t>(f, &qt_words);
        uint32_t* want_status = read_blob<uint32_t>(f, &status_words);
        int16_t* want_coef = read_blob<int16_t>(f, &coef_words);
        const size_t nseg = seg_words / JPG_SEG_WORDS;
        const long long stride_blocks = (long long)(coef_words / 64);
        if (fd_words != JPG_FD_WORDS || huff_bytes != JPG_TABLES * JPG_HUFF_BYTES || qt_words != 256 || status_words != 2 * nseg) return 2;
        JpegTable* tables = (JpegTable*)std::malloc(JPG_TABLES * sizeof(JpegTable));
        std::memset(tables, 0xEE, JPG_TABLES * sizeof(JpegTable));   // nothing relies on zeroed tables
        for (int t = 0; t < JPG_TABLES; ++t) jpeg_build_table(tables + t, huff + t * JPG_HUFF_BYTES);
        int16_t* coef = (int16_t*)std::calloc(coef_words ? coef_words : 1, sizeof(int16_t));
        std::vector<uint32_t> got(2 * nseg, 99);
        bool bad_case = false;
        for (size_t s = 0; s < nseg; ++s) {
            run_segment(file, file_bytes, segs, s, fd, tables, qt, coef, stride_blocks, &got[2 * s]);
            bad_case = bad_case || want_status[2 * s] != 0;
        }
        const bool ok = std::memcmp(got.data(), want_status, 2 * nseg * sizeof(uint32_t)) == 0 &&
                        std::memcmp(coef, want_coef, coef_words * sizeof(int16_t)) == 0;
        if (!ok) {
            ++failures;
            std::fprintf(stderr, "MISMATCH %s:", name.c_str());
            for (size_t s = 0; s < nseg; ++s)
                if (got[2 * s] != want_status[2 * s] || got[2 * s + 1] != want_status[2 * s + 1])
                    std::fprintf(stderr, " segment %zu (%u, %u) want (%u, %u)", s, got[2 * s], got[2 * s + 1], want_status[2 * s], want_status[2 * s + 1]);
            std::fprintf(stderr, "\n");
        }
        malformed += bad_case;
        segments += nseg;
        // every segment cut short: a status, or a clean end where the padding hid the cut, and no access outside
        uint32_t st[2];
        for (size_t s = 0; s < nseg; ++s)
            for (long long len = 0; len < 24 && len < segs[JPG_SEG_WORDS * s + 1]; ++len)
                run_segment(file, file_bytes, segs, s, fd, tables, qt, coef, stride_blocks, st, len);
        // a descriptor that claims more blocks than the buffer holds is not followed
        if (nseg) {
            run_segment(file, file_bytes, segs, 0, fd, tables, qt, coef, stride_blocks - 1 > 0 && fd[5] == stride_blocks ? stride_blocks - 1 : 0, st);
            if (st[0] != JPG_E_DESC) {
                ++failures;
                std::fprintf(stderr, "MISMATCH %s: a descriptor that does not fit was followed\n", name.c_str());
            }
        }
        std::free(file);
        std::free(segs);
        std::free(fd);
        std::free(huff);
        std::free(qt);
        std::free(want_status);
        std::free(want_coef);
        std::free(tables);
        std::free(coef);
    }
    std::fclose(f);
    std::printf("%u files (%d malformed), %zu segments: %d mismatches\n", count, malformed, segments, failures);
    return failures ? 1 : 0;
}
