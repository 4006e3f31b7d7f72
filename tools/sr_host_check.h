// The common half of rrdb_host_check.cpp and srvgg_host_check.cpp: the failure counter, an f16 conversion written
// independently of the library's, and the packing check over a list of padded channel counts.
#pragma once
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
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
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

// Every (cin, cout) of the lists, with full and with ragged real channel counts (`ragged_cout` gives the latter's
// cout_real), packed into a heap block of exactly `packed_bytes(cin, cout)` and compared element by element.  The
// weights are adversarial for the rounding: ties, subnormals, the overflow threshold, signed zero.
template <size_t NI, size_t NO>
static void check_packing(size_t (*packed_bytes)(int, int), int (*pack)(const float*, int, int, int, int, void*),
                          const int (&cins)[NI], const int (&couts)[NO], int (*ragged_cout)(int), uint32_t seed) {
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed; };
    for (int cin : cins)
        for (int cout : couts)
            for (int ragged = 0; ragged < 2; ++ragged) {
                const int cin_real = ragged ? (cin == 32 ? 3 : cin - 5) : cin, cout_real = ragged ? ragged_cout(cout) : cout;
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
                const size_t bytes = packed_bytes(cin, cout);
                EXPECT(bytes == (size_t)9 * cin * cout * 2);
                uint16_t* packed = (uint16_t*)std::malloc(bytes);
                std::memset(packed, 0xff, bytes);
                EXPECT(pack(w.data(), cin_real, cout_real, cin, cout, packed) == 0);
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
}
