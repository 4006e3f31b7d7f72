// The index arithmetic of csrc/lpips.hip's stem and distance kernels (csrc/lpips_index.h, the functions the kernels
// call) walked on the host over the case matrix of tests/_lpips_ref.py, with buffers of exactly the size the entry points
// are handed: every byte the stem stages is read, every float the distance kernel loads is read, every output is written.
// Meant to be built with the address and undefined-behaviour sanitizers and run as it is:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/lpips_index_check.cpp -o lpips_index_check
//     ./lpips_index_check
//
// It also checks what the sanitizers cannot see: no staged pixel lies outside the rect, every output element is
// written exactly once, every pixel of a feature map is taken by exactly one lane group.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../elvis_amd/csrc/lpips_index.h"

struct StemCase { int n, h, w, y0, y1, x0, x1, masked, bgr; };

static int fail(const char* what, int a, int b) {
    std::fprintf(stderr, "lpips_index_check: %s (%d, %d)\n", what, a, b);
    return 1;
}

static int check_stem(const StemCase& c) {
    const size_t pixels = (size_t)c.n * c.h * c.w;
    uint8_t* frames = (uint8_t*)std::malloc(pixels * 3);
    uint8_t* mask = c.masked ? (uint8_t*)std::malloc(pixels) : nullptr;
    for (size_t i = 0; i < pixels * 3; ++i) frames[i] = (uint8_t)(i * 7 + 3);
    if (mask) for (size_t i = 0; i < pixels; ++i) mask[i] = (uint8_t)((i * 5) % 3 ? 255 : 0);
    if (!lpips_rect_ok(c.h, c.w, c.y0, c.y1, c.x0, c.x1)) return fail("case rect refused", c.h, c.w);
    const int ho = lpips_stem_size(c.y1 - c.y0), wo = lpips_stem_size(c.x1 - c.x0), pitch = LPIPS_STEM_COUT;
    const size_t out_floats = (size_t)c.n * ho * wo * pitch;
    float* out = (float*)std::malloc(out_floats * sizeof(float));
    std::vector<int> written(out_floats, 0);
    const int tiles_y = (ho + LPIPS_STEM_TY - 1) / LPIPS_STEM_TY, tiles_x = (wo + LPIPS_STEM_TX - 1) / LPIPS_STEM_TX;
    long long sum = 0;
    for (int f = 0; f < c.n; ++f)
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx) {
                const int oy0 = ty * LPIPS_STEM_TY, ox0 = tx * LPIPS_STEM_TX;
                for (int i = 0; i < LPIPS_STEM_ROWS * LPIPS_STEM_COLS; ++i) {          // the staging loop, every thread's share
                    const int r = i / LPIPS_STEM_COLS, cc = i % LPIPS_STEM_COLS;
                    const long long pix = lpips_stem_src_pixel(f, c.h, c.w, c.y0, c.y1, c.x0, c.x1, oy0, ox0, r, cc);
                    if (pix < 0) continue;
                    const int y = (int)((pix / c.w) % c.h), x = (int)(pix % c.w);
                    if (pix / ((long long)c.w * c.h) != f || y < c.y0 || y >= c.y1 || x < c.x0 || x >= c.x1) return fail("staged pixel outside the rect", y, x);
                    for (int ch = 0; ch < 3; ++ch) sum += lpips_stem_byte(frames, mask, pix, ch, c.bgr);
                }
                for (int p = 0; p < LPIPS_STEM_TY * LPIPS_STEM_TX; ++p) {              // lanes of a wave; g: the four waves
                    const int oy = oy0 + p / LPIPS_STEM_TX, ox = ox0 + p % LPIPS_STEM_TX;
                    if (oy >= ho || ox >= wo) continue;
                    // the farthest element the lane reads from the staged footprint
                    const int r = (p / LPIPS_STEM_TX) * LPIPS_STEM_STRIDE + LPIPS_STEM_KS - 1, cc = (p % LPIPS_STEM_TX) * LPIPS_STEM_STRIDE + LPIPS_STEM_KS - 1;
                    if (r >= LPIPS_STEM_ROWS || cc >= LPIPS_STEM_COLS) return fail("lane reads past the footprint", r, cc);
                    for (int g = 0; g < 4; ++g)
                        for (int j = 0; j < 16; ++j) {
                            const long long at = lpips_stem_out_offset(f, ho, wo, oy, ox, pitch) + g * 16 + j;
                            out[at] = (float)sum;
                            ++written[at];
                        }
                }
            }
    for (size_t i = 0; i < out_floats; ++i)
        if (written[i] != 1) return fail("an output element written other than once", (int)i, written[i]);
    std::free(frames);
    std::free(mask);
    std::free(out);
    return 0;
}

static int check_distance(int n, int h, int w, int c, int pitch) {
    const long long hw = (long long)h * w;
    const size_t floats = (size_t)n * hw * pitch;
    float* x = (float*)std::malloc(floats * sizeof(float));
    float* y = (float*)std::malloc(floats * sizeof(float));
    for (size_t i = 0; i < floats; ++i) x[i] = y[i] = (float)(i % 13);
    const int blocks = lpips_dist_blocks(hw);
    double* partial = (double*)std::malloc((size_t)n * blocks * sizeof(double));   // elvis_lpips_distance_workspace_bytes
    double* out = (double*)std::malloc((size_t)n * sizeof(double));
    std::vector<int> taken((size_t)n * hw, 0);
    for (int f = 0; f < n; ++f)
        for (int block = 0; block < blocks; ++block) {
            double total = 0.0;
            for (int wave = 0; wave < LPIPS_DIST_THREADS / 64; ++wave)
                for (int i = 0; i < LPIPS_DIST_PIXELS / 4; ++i) {
                    const long long p = lpips_dist_pixel(hw, block, wave, i);
                    if (p < 0) break;
                    ++taken[(size_t)f * hw + p];
                    const long long at = lpips_feature_offset(f, hw, p, pitch, 0);
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < LPIPS_DIST_MAX_C / 64; ++j)
                            if (lane + 64 * j < c) total += x[at + lane + 64 * j] - y[at + lane + 64 * j];
                }
            partial[(long long)f * blocks + block] = total;
        }
    for (int f = 0; f < n; ++f) {
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += partial[(long long)f * blocks + b];
        out[f] = s / (double)hw;
    }
    for (size_t i = 0; i < taken.size(); ++i)
        if (taken[i] != 1) return fail("a pixel taken other than once", (int)i, taken[i]);
    if (out[0] != 0.0) return fail("x - y did not cancel", 0, 0);
    std::free(x);
    std::free(y);
    std::free(partial);
    std::free(out);
    return 0;
}

int main() {
    // tests/_lpips_ref.py CASES (shape, rect, mask, order), and the rect at every corner of its frame
    const StemCase stem[] = {
        {1, 31, 31, 0, 31, 0, 31, 0, 1}, {1, 32, 35, 0, 32, 0, 35, 0, 1}, {1, 33, 38, 0, 33, 0, 38, 0, 1}, {1, 67, 95, 0, 67, 0, 95, 0, 1},
        {1, 47, 64, 0, 47, 0, 64, 0, 1}, {1, 32, 35, 0, 32, 0, 35, 0, 0}, {2, 70, 90, 5, 64, 9, 82, 1, 1}, {3, 33, 38, 0, 33, 0, 38, 0, 1},
        {2, 70, 90, 0, 31, 0, 31, 1, 0}, {2, 70, 90, 39, 70, 59, 90, 1, 1}, {2, 70, 90, 39, 70, 0, 31, 0, 1}, {2, 70, 90, 0, 31, 59, 90, 1, 0},
        {1, 48, 64, 3, 48, 1, 64, 1, 1},
    };
    int checked = 0;
    for (const StemCase& c : stem) {
        if (check_stem(c)) return 1;
        ++checked;
    }
    // the five taps of those cases: (pixels, channels); 1 x 1 maps, a ragged last workgroup, more than one workgroup
    const int maps[][2] = {{7, 7}, {7, 8}, {8, 9}, {16, 23}, {11, 15}, {14, 18}, {3, 3}, {1, 1}, {1, 2}, {6, 8}, {5, 27}, {8, 8}, {5, 13}};
    const int chans[][2] = {{64, 64}, {192, 192}, {384, 384}, {256, 256}, {40, 48}};
    for (const auto& m : maps)
        for (const auto& ch : chans)
            for (int n = 1; n <= 3; n += 2) {
                if (check_distance(n, m[0], m[1], ch[0], ch[1])) return 1;
                ++checked;
            }
    std::printf("lpips_index_check: %d cases clean\n", checked);
    return 0;
}
