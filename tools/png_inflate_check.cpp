// The decoder of csrc/png_read.hip's png_inflate_kernel (csrc/inflate.h, the very functions the kernel calls) walked on
// the host, the 64 lanes as a loop, over every stream of the test corpus - the well-formed ones and the malformed ones -
// with buffers of exactly the size the entry points are handed: the stream's own bytes in, `cap` bytes out.  For every
// case the bytes produced, the status, the counts and the Adler-32 are compared with the statement's
// (tests/_png_read_ref.py).  Meant to be built with the address and undefined-behaviour sanitizers and run as it is:
//
//     python tests/_png_read_ref.py dump corpus.bin
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/png_inflate_check.cpp -o png_inflate_check
//     ./png_inflate_check corpus.bin
//
// A read outside the stream, a store outside the output, or an index outside a table stops it.  The malformed cases go
// to a GPU only after they have passed here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../elvis_amd/csrc/inflate.h"

static bool read_u32(FILE* f, uint32_t* v) {
    unsigned char b[4];
    if (std::fread(b, 1, 4, f) != 4) return false;
    *v = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: png_inflate_check CORPUS (written by python tests/_png_read_ref.py dump CORPUS)\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "png_inflate_check: cannot open %s\n", argv[1]);
        return 2;
    }
    uint32_t count = 0;
    if (!read_u32(f, &count)) return 2;
    InfShared* S = (InfShared*)std::malloc(sizeof(InfShared));
    int failures = 0, malformed = 0;
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t name_len = 0, in_len = 0, head[5];
        if (!read_u32(f, &name_len)) return 2;
        std::string name(name_len, ' ');
        if (std::fread(&name[0], 1, name_len, f) != name_len || !read_u32(f, &in_len)) return 2;
        uint8_t* in = (uint8_t*)std::malloc(in_len ? in_len : 1);
        if (std::fread(in, 1, in_len, f) != in_len) return 2;
        for (int i = 0; i < 5; ++i)
            if (!read_u32(f, &head[i])) return 2;
        const uint32_t cap = head[0], status = head[1], produced = head[2], consumed = head[3], adler = head[4];
        std::vector<uint8_t> want(produced);
        if (produced && std::fread(want.data(), 1, produced, f) != produced) return 2;
        uint8_t* out = (uint8_t*)std::malloc(cap ? cap : 1);
        std::memset(out, 0xA5, cap ? cap : 1);
        std::memset(S, 0xEE, sizeof(InfShared));   // nothing relies on zeroed tables
        uint32_t got[4] = {99, 0, 0, 0};
        inflate_run(S, in, in_len, out, cap, got);
        bool ok = got[0] == status && got[1] == produced && got[3] == adler && got[2] == consumed && produced <= cap &&
                  (produced == 0 || std::memcmp(out, want.data(), produced) == 0);
        for (uint32_t i = produced; ok && i < cap; ++i) ok = out[i] == 0xA5;   // nothing behind the bytes produced
        if (!ok) {
            std::fprintf(stderr, "png_inflate_check: %s: status %u (want %u), produced %u (%u), consumed %u (%u), adler %08x (%08x)\n",
                         name.c_str(), got[0], status, got[1], produced, got[2], consumed, got[3], adler);
            ++failures;
        }
        malformed += status != 0;
        std::free(in);
        std::free(out);
    }
    std::free(S);
    std::fclose(f);
    std::printf("png_inflate_check: %u streams (%d malformed), %d failure(s)\n", count, malformed, failures);
    return failures ? 1 : 0;
}
