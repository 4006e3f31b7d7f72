// The host code of csrc/tfill.hip - elvis_tfill_limits_ok and the argument checks of elvis_tfill - called from a program
// of its own, meant to be built with the address and undefined-behaviour sanitizers on the host side and run as it is,
// without a GPU:
//
//     hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all tools/tfill_host_check.cpp elvis_amd/csrc/tfill.hip elvis_amd/csrc/api.hip \
//         -o tfill_host_check && ./tfill_host_check
//
// Every refusal must come back as -1 before any launch: the addresses below are never dereferenced.  The limits are
// walked at, one below and one above every bound, and at the sizes where an index would pass 2^31.
#include "sr_host_check.h"

int main() {
    // elvis_tfill_limits_ok(n, h, w, c, B, G, R, S, M)
    EXPECT(elvis_tfill_limits_ok(1, 1, 1, 1, 1, 0, 0, 0, 0) == 1);
    EXPECT(elvis_tfill_limits_ok(5, 1080, 1920, 3, 16, 8, 2, 7, 6) == 1);
    EXPECT(elvis_tfill_limits_ok(5, 1080, 1920, 3, 32, 16, 8, 7, 255) == 1);
    const int lo[9] = {1, 1, 1, 1, 1, 0, 0, 0, 0}, hi[9] = {0, 0, 0, 3, 32, 16, 8, 7, 255};
    for (int k = 0; k < 9; ++k) {
        int a[9] = {2, 40, 48, 3, 16, 8, 2, 7, 6};
        a[k] = lo[k] - 1;
        EXPECT(elvis_tfill_limits_ok(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]) == 0);
        a[k] = lo[k];
        EXPECT(elvis_tfill_limits_ok(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]) == 1);
        if (hi[k]) {
            a[k] = hi[k];
            EXPECT(elvis_tfill_limits_ok(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]) == 1);
            a[k] = hi[k] + 1;
            EXPECT(elvis_tfill_limits_ok(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]) == 0);
        }
        a[k] = INT32_MIN;
        EXPECT(elvis_tfill_limits_ok(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]) == 0);
        a[k] = INT32_MAX;
        EXPECT(elvis_tfill_limits_ok(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]) == 0);
    }
    EXPECT(elvis_tfill_limits_ok(1, 1, 1, 2, 16, 8, 2, 7, 6) == 0);                      // c = 2
    EXPECT(elvis_tfill_limits_ok(1, 32767, 32767, 3, 16, 8, 2, 7, 6) == 0);              // 3 * 1 073 676 289 >= 2^31
    EXPECT(elvis_tfill_limits_ok(2, 32767, 32767, 1, 16, 8, 2, 7, 6) == 1);              // 2 147 352 578 < 2^31
    EXPECT(elvis_tfill_limits_ok(3, 32767, 32767, 1, 16, 8, 2, 7, 6) == 0);
    EXPECT(elvis_tfill_limits_ok(1, 32768, 8, 1, 16, 8, 2, 7, 6) == 0);                  // h, w <= 32767
    EXPECT(elvis_tfill_limits_ok(1, 8, 32768, 1, 16, 8, 2, 7, 6) == 0);
    EXPECT(elvis_tfill_limits_ok(INT32_MAX, INT32_MAX, INT32_MAX, 3, 1, 0, 0, 0, 0) == 0);
    EXPECT(elvis_tfill_limits_ok(INT32_MAX, 1, 1, 1, 1, 0, 0, 0, 0) == 1);               // 2^31 - 1 blocks of one pixel
    EXPECT(elvis_tfill_limits_ok(INT32_MAX, 1, 1, 3, 1, 0, 0, 0, 0) == 0);

    // elvis_tfill: a 2 x 40 x 48 x 3 clip at addresses that are never read
    const size_t npix = 2 * 40 * 48;
    const uint8_t* const F = (const uint8_t*)(uintptr_t)0x100000;
    const uint8_t* const K = (const uint8_t*)(uintptr_t)0x200000;
    uint8_t* const O = (uint8_t*)(uintptr_t)0x300000;
    uint8_t* const L = (uint8_t*)(uintptr_t)0x400000;
    auto fill = [&](const uint8_t* f, const uint8_t* k, int bm, uint8_t* o, uint8_t* l, int n, int h, int w, int c, int B, int G,
                    int R, int S, int M) { return elvis_tfill(f, k, bm, o, l, n, h, w, c, B, G, R, S, M, nullptr); };
    EXPECT(fill(nullptr, K, 0, O, L, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, nullptr, 0, O, L, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, nullptr, L, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, nullptr, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(std::strstr(elvis_last_error(), "null") != nullptr);
    EXPECT(fill(F, K, 0, O, L, 2, 40, 48, 2, 16, 8, 2, 7, 6) == -1);
    EXPECT(std::strstr(elvis_last_error(), "channels") != nullptr);
    EXPECT(fill(F, K, 0, O, L, 2, 40, 48, 4, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 0, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 2, 0, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 2, 40, -1, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 3, 32767, 32767, 1, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 2, 40, 48, 3, 0, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 2, 40, 48, 3, 33, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 2, 40, 48, 3, 16, -1, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 2, 40, 48, 3, 16, 17, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 2, 40, 48, 3, 16, 8, -1, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 2, 40, 48, 3, 16, 8, 9, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 2, 40, 48, 3, 16, 8, 2, -1, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 2, 40, 48, 3, 16, 8, 2, 8, 6) == -1);
    EXPECT(fill(F, K, 0, O, L, 2, 40, 48, 3, 16, 8, 2, 7, -1) == -1);
    EXPECT(fill(F, K, 0, O, L, 2, 40, 48, 3, 16, 8, 2, 7, 256) == -1);
    EXPECT(std::strstr(elvis_last_error(), "limits") != nullptr);
    EXPECT(fill(F, K, -1, O, L, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(std::strstr(elvis_last_error(), "block_mask_size") != nullptr);
    // aliasing: out on frames, one byte into them, ending on their first byte; left on each of the others
    EXPECT(fill(F, K, 0, (uint8_t*)F, L, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(std::strstr(elvis_last_error(), "alias") != nullptr);
    EXPECT(fill(F, K, 0, (uint8_t*)F + 3 * npix - 1, L, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, (uint8_t*)F - 3 * npix + 1, L, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, (uint8_t*)F + 5, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, (uint8_t*)K, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, O, O + 3 * npix - 1, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(fill(F, K, 0, (uint8_t*)K + npix - 1, L, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    // block masks: [2, 5, 6] of 8 - left on their last byte
    EXPECT(fill(F, K, 8, O, (uint8_t*)K + 59, 2, 40, 48, 3, 16, 8, 2, 7, 6) == -1);
    EXPECT(std::strncmp(elvis_last_error(), "elvis_tfill", 11) == 0);
    std::printf("tfill_host_check: %s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
