// The host code of csrc/srvgg.hip - elvis_srvgg_pack_weights and the argument checks of elvis_srvgg_conv3x3 and
// elvis_srvgg_tail - called from a program of its own with buffers of exactly the sizes the contract names, meant to be
// built with the address and undefined-behaviour sanitizers on the host side and run as it is, without a GPU:
//
//     hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/srvgg_host_check.cpp elvis_amd/csrc/srvgg.hip elvis_amd/csrc/api.hip \
//         -o srvgg_host_check && ./srvgg_host_check
//
// Packing: every supported (cin, cout) with full and ragged real channel counts, into a heap block of exactly
// elvis_srvgg_packed_weight_bytes; each element is compared with a conversion written here (a write past the block or a
// read past the fp32 tensor stops the run).  Argument checks: every refusal must come back as -1 before any launch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/elvis_amd.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

// f16 bits -> float, exact
static float f16_value(uint16_t h) {
    const int s = h >> 15, e = (h >> 10) & 31, m = h & 1023;
    float v;
    if (e == 0) v = std::ldexp((float)m, -24);
    else if (e == 31) v = m ? NAN : INFINITY;
    else v = std::ldexp((float)(m + 1024), e - 25);
    return s ? -v : v;
}

// is `h` a nearest f16 of `f` (ties: the even one)
static bool is_rne16(float f, uint16_t h) {
    const float v = f16_value(h);
    if (std::isnan(f)) return std::isnan(v);
    if (std::isinf(v)) return std::fabs(f) >= 65520.0f && (v > 0) == (f > 0);
    if (std::signbit(v) != std::signbit(f)) return false;
    const uint16_t mag = h & 0x7fff;
    const float up = f16_value((uint16_t)(mag + 1)), dn = mag ? f16_value((uint16_t)(mag - 1)) : -f16_value(1);
    const double a = std::fabs((double)f), c = std::fabs((double)v);
    const double hi = (mag + 1 == 0x7c00) ? 65520.0 : 0.5 * (c + up), lo = 0.5 * (c + dn);
    if (a > hi || a < lo) return false;
    if ((a == hi || a == lo) && (mag & 1)) return false;
    return true;
}

int main() {
    const int cins[] = {32, 64}, couts[] = {48, 64};
    uint32_t seed = 54321u;
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed; };
    for (int cin : cins)
        for (int cout : couts)
            for (int ragged = 0; ragged < 2; ++ragged) {
                const int cin_real = ragged ? (cin == 32 ? 3 : cin - 5) : cin, cout_real = ragged ? cout - 1 : cout;
                const size_t nw = (size_t)cout_real * cin_real * 9;
                std::vector<float> w(nw);
                for (size_t i = 0; i < nw; ++i) {
                    const uint32_t r = next();
                    switch (r % 11) {
                        case 0: w[i] = std::ldexp(1.0f, -25); break;                  // tie at the smallest subnormal
                        case 1: w[i] = -std::ldexp(3.0f, -25); break;                 // tie between subnormals
                        case 2: w[i] = 65519.9f; break;
                        case 3: w[i] = 65520.0f; break;                               // rounds to infinity
                        case 4: w[i] = 1.0f + std::ldexp(1.0f, -11); break;           // tie, even below
                        case 5: w[i] = 1.0f + std::ldexp(3.0f, -11); break;           // tie, even above
                        case 6: w[i] = -0.0f; break;
                        default: w[i] = ((int)(r >> 8) % 20001 - 10000) * 1e-4f * std::ldexp(1.0f, (int)(r % 7) - 8);
                    }
                }
                const size_t bytes = elvis_srvgg_packed_weight_bytes(cin, cout);
                EXPECT(bytes == (size_t)9 * cin * cout * 2);
                uint16_t* packed = (uint16_t*)std::malloc(bytes);
                std::memset(packed, 0xff, bytes);
                EXPECT(elvis_srvgg_pack_weights(w.data(), cin_real, cout_real, cin, cout, packed) == 0);
                for (int kc = 0; kc < cin / 32; ++kc)
                    for (int tap = 0; tap < 9; ++tap)
                        for (int co = 0; co < cout; ++co)
                            for (int k = 0; k < 32; ++k) {
                                const int ci = kc * 32 + k;
                                const uint16_t got = packed[(((size_t)kc * 9 + tap) * cout + co) * 32 + k];
                                if (ci < cin_real && co < cout_real) EXPECT(is_rne16(w[((size_t)co * cin_real + ci) * 9 + tap], got));
                                else EXPECT(got == 0);
                            }
                std::free(packed);
            }
    EXPECT(elvis_srvgg_packed_weight_bytes(96, 64) == 0);
    EXPECT(elvis_srvgg_packed_weight_bytes(64, 32) == 0);
    float one = 1.0f;
    uint16_t small[4];
    EXPECT(elvis_srvgg_pack_weights(&one, 1, 1, 48, 64, small) == -1);
    EXPECT(elvis_srvgg_pack_weights(&one, 1, 1, 32, 32, small) == -1);
    EXPECT(elvis_srvgg_pack_weights(&one, 0, 1, 32, 48, small) == -1);
    EXPECT(elvis_srvgg_pack_weights(&one, 1, 49, 32, 48, small) == -1);
    EXPECT(elvis_srvgg_pack_weights(&one, 33, 1, 32, 48, small) == -1);
    EXPECT(elvis_srvgg_pack_weights(nullptr, 1, 1, 32, 48, small) == -1);
    EXPECT(elvis_srvgg_pack_weights(&one, 1, 1, 32, 48, nullptr) == -1);

    // the argument checks: addresses that are never dereferenced, every call refused before a launch
    void* const X = (void*)(uintptr_t)0x10000;
    void* const O = (void*)(uintptr_t)0x4000000;
    const void* const W = (const void*)(uintptr_t)0x20000;
    const float* const B = (const float*)(uintptr_t)0x30000;
    const float* const A = (const float*)(uintptr_t)0x31000;
    const void* const BASE = (const void*)(uintptr_t)0x40000;
    auto conv = [&](const void* x, int xp, const float* slope, void* out, int op, int n, int h, int w, int cin) {
        return elvis_srvgg_conv3x3(x, xp, W, B, slope, out, op, n, h, w, cin, nullptr);
    };
    EXPECT(conv(X, 64, A, O, 64, 1, 4, 4, 48) == -1);
    EXPECT(conv(X, 64, A, O, 64, 1, 4, 4, 96) == -1);
    EXPECT(conv(X, 56, A, O, 64, 1, 4, 4, 64) == -1);
    EXPECT(conv(X, 68, A, O, 64, 1, 4, 4, 64) == -1);
    EXPECT(conv(X, 64, A, O, 56, 1, 4, 4, 64) == -1);
    EXPECT(conv(X, 64, A, O, 68, 1, 4, 4, 64) == -1);
    EXPECT(conv(X, 64, A, O, 64, -1, 4, 4, 64) == -1);
    EXPECT(conv(X, 64, A, O, 64, 1, (1 << 29) + 1, 4, 64) == -1);
    EXPECT(conv(nullptr, 64, A, O, 64, 1, 4, 4, 64) == -1);
    EXPECT(conv(X, 64, nullptr, O, 64, 1, 4, 4, 64) == -1);
    EXPECT(conv(X, 64, A, nullptr, 64, 1, 4, 4, 64) == -1);
    EXPECT(conv((char*)X + 8, 64, A, O, 64, 1, 4, 4, 64) == -1);
    EXPECT(conv(X, 64, A + 1, O, 64, 1, 4, 4, 64) == -1);
    EXPECT(conv(X, 64, A, (char*)O + 4, 64, 1, 4, 4, 64) == -1);
    EXPECT(conv(X, 64, A, X, 64, 1, 4, 4, 64) == -1);                                  // in place
    EXPECT(conv(X, 64, A, (char*)X + 16 * 128 - 8, 64, 1, 4, 4, 64) == -1);           // the last 8 bytes of x
    EXPECT(conv((char*)O + 16 * 128 - 16, 64, A, O, 64, 1, 4, 4, 64) == -1);          // the last 16 bytes of out
    EXPECT(conv(X, 64, A, (void*)(uintptr_t)0x10000000000ull, 64, 70000, 4, 4, 64) == -1);
    EXPECT(conv(X, 64, A, (void*)(uintptr_t)0x10000000000ull, 64, 1, 8 * 65536, 1, 64) == -1);
    EXPECT(conv(nullptr, 64, nullptr, nullptr, 64, 0, 4, 4, 64) == 0);
    EXPECT(conv(nullptr, 64, nullptr, nullptr, 64, 1, 0, 4, 32) == 0);
    EXPECT(std::strncmp(elvis_last_error(), "elvis_srvgg_conv3x3", 19) == 0);

    auto tail = [&](const void* x, int xp, const void* base, int bp, void* out, int n, int h, int w, int u8) {
        return elvis_srvgg_tail(x, xp, W, B, base, bp, out, n, h, w, u8, 1, nullptr);
    };
    EXPECT(tail(X, 56, BASE, 32, O, 1, 4, 4, 1) == -1);
    EXPECT(tail(X, 68, BASE, 32, O, 1, 4, 4, 1) == -1);
    EXPECT(tail(X, 64, BASE, 2, O, 1, 4, 4, 1) == -1);
    EXPECT(tail(X, 64, BASE, 32, O, 1, -4, 4, 1) == -1);
    EXPECT(tail(X, 64, BASE, 32, O, 1, 4, (1 << 27) + 1, 1) == -1);
    EXPECT(tail(nullptr, 64, BASE, 32, O, 1, 4, 4, 1) == -1);
    EXPECT(tail(X, 64, nullptr, 32, O, 1, 4, 4, 1) == -1);
    EXPECT(tail(X, 64, BASE, 32, nullptr, 1, 4, 4, 1) == -1);
    EXPECT(tail((char*)X + 8, 64, BASE, 32, O, 1, 4, 4, 1) == -1);
    EXPECT(tail(X, 64, (char*)BASE + 1, 32, O, 1, 4, 4, 1) == -1);
    EXPECT(tail(X, 64, BASE, 32, (char*)O + 2, 1, 4, 4, 1) == -1);
    EXPECT(tail(X, 64, BASE, 32, (char*)O + 4, 1, 4, 4, 0) == -1);                     // f16 out: 8 bytes
    EXPECT(tail(X, 64, BASE, 32, (char*)X + 16, 1, 4, 4, 1) == -1);                    // out inside x
    EXPECT(tail(X, 64, BASE, 3, (char*)BASE + 16 * 6 - 4, 1, 4, 4, 1) == -1);          // the last 4 bytes of a pitch-3 base
    EXPECT(tail(X, 64, (char*)O + 16 * 48 - 2, 3, O, 1, 4, 4, 1) == -1);               // base on the last bytes of a u8 out
    EXPECT(tail(X, 64, (char*)O + 16 * 96 - 2, 3, O, 1, 4, 4, 0) == -1);               // ... of an f16 out
    EXPECT(tail(X, 64, BASE, 32, (void*)(uintptr_t)0x10000000000ull, 70000, 4, 4, 1) == -1);
    EXPECT(tail(nullptr, 64, nullptr, 32, nullptr, 0, 4, 4, 1) == 0);
    EXPECT(tail(nullptr, 64, nullptr, 32, nullptr, 1, 4, 0, 0) == 0);
    EXPECT(std::strncmp(elvis_last_error(), "elvis_srvgg_tail", 16) == 0);
    std::printf("srvgg_host_check: %s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
