// The host code of csrc/srvgg.hip - elvis_srvgg_pack_weights and the argument checks of elvis_srvgg_conv3x3 and
// elvis_srvgg_tail - called from a program of its own with buffers of exactly the sizes the contract names, meant to be
// built with the address and undefined-behaviour sanitizers on the host side and run as it is, without a GPU:
//
//     hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/srvgg_host_check.cpp elvis_amd/csrc/srvgg.hip elvis_amd/csrc/api.hip \
//         -o srvgg_host_check && ./srvgg_host_check
//
// Packing: every supported (cin, cout) with full and ragged real channel counts, into a heap block of exactly
// elvis_srvgg_packed_weight_bytes; each element is compared with sr_host_check.h's own conversion (a write past the
// block or a read past the fp32 tensor stops the run).  Argument checks: every refusal must come back as -1 before any
// launch.
#include "sr_host_check.h"

int main() {
    const int cins[] = {32, 64}, couts[] = {48, 64};
    check_packing(elvis_srvgg_packed_weight_bytes, elvis_srvgg_pack_weights, cins, couts,
                  [](int cout) { return cout - 1; }, 54321u);
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
