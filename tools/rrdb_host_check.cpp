// The host code of csrc/rrdb.hip - elvis_rrdb_pack_weights and the argument checks of elvis_rrdb_conv3x3 and
// elvis_rrdb_input_u8 - called from a program of its own with buffers of exactly the sizes the contract names, meant
// to be built with the address and undefined-behaviour sanitizers on the host side and run as it is, without a GPU:
//
//     hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/rrdb_host_check.cpp elvis_amd/csrc/rrdb.hip elvis_amd/csrc/api.hip \
//         -o rrdb_host_check && ./rrdb_host_check
//
// Packing: every supported (cin, cout) with ragged real channel counts, into a heap block of exactly
// elvis_rrdb_packed_weight_bytes; each element is compared with sr_host_check.h's own conversion (a write past the
// block or a read past the fp32 tensor stops the run).  Argument checks: every refusal must come back as -1 before any
// launch.
#include "sr_host_check.h"

int main() {
    const int cins[] = {32, 64, 96, 128, 160, 192}, couts[] = {32, 64};
    check_packing(elvis_rrdb_packed_weight_bytes, elvis_rrdb_pack_weights, cins, couts,
                  [](int cout) { return cout == 32 ? 3 : cout - 1; }, 12345u);
    EXPECT(elvis_rrdb_packed_weight_bytes(48, 32) == 0);
    float one = 1.0f;
    uint16_t small[4];
    EXPECT(elvis_rrdb_pack_weights(&one, 1, 1, 48, 32, small) == -1);
    EXPECT(elvis_rrdb_pack_weights(&one, 1, 1, 32, 48, small) == -1);
    EXPECT(elvis_rrdb_pack_weights(&one, 0, 1, 32, 32, small) == -1);
    EXPECT(elvis_rrdb_pack_weights(&one, 1, 33, 32, 32, small) == -1);
    EXPECT(elvis_rrdb_pack_weights(nullptr, 1, 1, 32, 32, small) == -1);

    // the argument checks: addresses that are never dereferenced, every call refused before a launch
    void* const X = (void*)(uintptr_t)0x10000;
    void* const O = (void*)(uintptr_t)0x4000000;
    const void* const W = (const void*)(uintptr_t)0x20000;
    const float* const B = (const float*)(uintptr_t)0x30000;
    auto conv = [&](const void* x, int xp, void* out, int op, int coff, const void* r1, int r1p, const void* r2, int r2p, int n,
                    int h, int w, int cin, int cout, int ups, int u8) {
        return elvis_rrdb_conv3x3(x, xp, W, B, out, op, coff, r1, r1p, r2, r2p, n, h, w, cin, cout, ups, 1, 0.2f, 1.0f, u8, 0, nullptr);
    };
    EXPECT(conv(X, 64, O, 64, 0, nullptr, 0, nullptr, 0, 1, 4, 4, 48, 32, 0, 0) == -1);
    EXPECT(conv(X, 64, O, 64, 0, nullptr, 0, nullptr, 0, 1, 4, 4, 64, 48, 0, 0) == -1);
    EXPECT(conv(X, 56, O, 64, 0, nullptr, 0, nullptr, 0, 1, 4, 4, 64, 32, 0, 0) == -1);
    EXPECT(conv(X, 64, O, 64, 40, nullptr, 0, nullptr, 0, 1, 4, 4, 64, 32, 0, 0) == -1);
    EXPECT(conv(X, 64, O, 64, 0, nullptr, 0, nullptr, 0, 1, 4, 4, 64, 64, 0, 1) == -1);
    EXPECT(conv(X, 96, X, 96, 32, nullptr, 0, nullptr, 0, 1, 4, 4, 64, 32, 0, 0) == -1);
    EXPECT(conv(X, 96, X, 96, 64, nullptr, 0, nullptr, 0, 1, 4, 4, 64, 32, 1, 0) == -1);
    EXPECT(conv(X, 64, O, 64, 0, O, 96, nullptr, 0, 1, 4, 4, 64, 32, 0, 0) == -1);
    EXPECT(conv(X, 64, O, 64, 0, nullptr, 0, (char*)O + 8, 64, 1, 4, 4, 64, 32, 0, 0) == -1);
    EXPECT(conv(nullptr, 64, O, 64, 0, nullptr, 0, nullptr, 0, 1, 4, 4, 64, 32, 0, 0) == -1);
    EXPECT(conv(X, 64, O, 64, 0, nullptr, 0, nullptr, 0, -1, 4, 4, 64, 32, 0, 0) == -1);
    EXPECT(conv(X, 64, O, 64, 0, nullptr, 0, nullptr, 0, 70000, 4, 4, 64, 32, 0, 0) == -1);
    EXPECT(conv(X, 64, O, 64, 0, nullptr, 0, nullptr, 0, 1, 1 << 30, 4, 64, 32, 1, 0) == -1);
    EXPECT(conv(nullptr, 64, nullptr, 64, 0, nullptr, 0, nullptr, 0, 0, 4, 4, 64, 32, 0, 0) == 0);
    EXPECT(std::strncmp(elvis_last_error(), "elvis_rrdb_conv3x3", 18) == 0);
    EXPECT(elvis_rrdb_input_u8((const uint8_t*)X, O, 1, 4, 4, 3, 0, nullptr) == -1);
    EXPECT(elvis_rrdb_input_u8((const uint8_t*)X, O, 1, 1, 4, 2, 0, nullptr) == -1);
    EXPECT(elvis_rrdb_input_u8(nullptr, O, 1, 4, 4, 2, 0, nullptr) == -1);
    EXPECT(elvis_rrdb_input_u8((const uint8_t*)X, (char*)O + 4, 1, 4, 4, 1, 0, nullptr) == -1);
    EXPECT(elvis_rrdb_input_u8(nullptr, nullptr, 0, 4, 4, 1, 0, nullptr) == 0);
    std::printf("rrdb_host_check: %s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
