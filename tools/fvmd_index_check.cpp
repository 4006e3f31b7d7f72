// The index arithmetic of csrc/fvmd.hip (csrc/fvmd_index.h, the functions the kernels call) walked on the host with
// buffers of exactly the size the entry points are handed: every pixel the pyramid filter reads, every keypoint slot and
// track element the tracker writes, every cell point the histogram reads, every pair of every Jacobi round.
// Meant to be built with the address and undefined-behaviour sanitizers and run as it is:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/fvmd_index_check.cpp -o fvmd_index_check
//     ./fvmd_index_check
//
// It also checks what the sanitizers cannot see: the slot map and the cell map are permutations of the 400 points with a
// cell's 25 points in 25 neighbouring slots, every track element is written once, the pairs of a round are disjoint and
// every two vectors meet exactly once per sweep.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../elvis_amd/csrc/fvmd_index.h"

static int fail(const char* what, int a, int b) {
    std::fprintf(stderr, "fvmd_index_check: %s (%d, %d)\n", what, a, b);
    return 1;
}

static int check_pyramid(int h, int w) {
    long long sum = 0;
    int ih = h, iw = w;
    for (int level = 1; level < FVMD_LEVELS; ++level) {
        const int ho = fvmd_level_size(h, level), wo = fvmd_level_size(w, level);
        if (ho != (ih + 1) / 2 || wo != (iw + 1) / 2) return fail("level size", ho, wo);
        unsigned char* in = (unsigned char*)std::malloc((size_t)ih * iw);
        for (int i = 0; i < ih * iw; ++i) in[i] = (unsigned char)(i * 7 + 1);
        for (int oy = 0; oy < ho; ++oy)
            for (int ox = 0; ox < wo; ++ox)
                for (int ky = 0; ky < 5; ++ky)
                    for (int kx = 0; kx < 5; ++kx) sum += in[(size_t)fvmd_reflect(2 * oy + ky - 2, ih) * iw + fvmd_reflect(2 * ox + kx - 2, iw)];
        std::free(in);
        ih = ho, iw = wo;
    }
    return sum < 0;
}

static int check_points() {
    std::vector<int> seen(FVMD_POINTS, 0), cell_seen(FVMD_POINTS, 0);
    for (int q = 0; q < FVMD_POINTS; ++q) {
        const int pt = fvmd_point_of_slot(q);
        if (pt < 0 || pt >= FVMD_POINTS) return fail("slot maps outside the grid", q, pt);
        seen[pt]++;
        if (pt != fvmd_cell_point(q / 25, q % 25)) return fail("a cell's points are not its 25 neighbouring slots", q, pt);
    }
    for (int c = 0; c < FVMD_CELLS * FVMD_CELLS; ++c)
        for (int a = 0; a < FVMD_CELL_SIDE * FVMD_CELL_SIDE; ++a) {
            const int pt = fvmd_cell_point(c, a);
            if (pt < 0 || pt >= FVMD_POINTS) return fail("cell point outside the grid", c, a);
            cell_seen[pt]++;
            const int i = pt / FVMD_GRID, j = pt % FVMD_GRID;
            if (i / FVMD_CELL_SIDE != c / FVMD_CELLS || j / FVMD_CELL_SIDE != c % FVMD_CELLS) return fail("cell point in another cell", c, a);
        }
    for (int pt = 0; pt < FVMD_POINTS; ++pt)
        if (seen[pt] != 1 || cell_seen[pt] != 1) return fail("a point is not taken exactly once", pt, seen[pt]);
    return 0;
}

static int check_tracks(int frames, int seq_len, int step) {
    const int segments = fvmd_segments(frames, seq_len, step);
    if (segments <= 0) return frames >= seq_len ? fail("no segment", frames, seq_len) : 0;
    std::vector<int> written((size_t)segments * seq_len * FVMD_POINTS * 2, 0);
    std::vector<unsigned char> clip(frames, 1);
    for (int seg = 0; seg < segments; ++seg)
        for (int q = 0; q < FVMD_POINTS; ++q) {
            size_t out = ((size_t)seg * seq_len * FVMD_POINTS + fvmd_point_of_slot(q)) * 2;
            written[out]++, written[out + 1]++;
            for (int t = 0; t + 1 < seq_len; ++t) {
                const long long f = (long long)seg * step + t;
                if (clip.at((size_t)f) + clip.at((size_t)f + 1) != 2) return fail("frame outside the clip", seg, t);
                out += FVMD_POINTS * 2;
                written.at(out)++, written.at(out + 1)++;
            }
        }
    for (size_t i = 0; i < written.size(); ++i)
        if (written[i] != 1) return fail("a track element is not written exactly once", (int)i, written[i]);
    return 0;
}

static int check_pairs(int k) {
    const int K = (k + 1) & ~1;
    std::vector<int> met((size_t)K * K, 0);
    for (int r = 0; r < K - 1; ++r) {
        std::vector<int> used(K, 0);
        for (int p = 0; p < K / 2; ++p) {
            int i = -1, j = -1;
            fvmd_pair(r, p, K, &i, &j);
            if (i < 0 || j < 0 || i >= K || j >= K || i == j) return fail("bad pair", i, j);
            used[i]++, used[j]++;
            met[(size_t)i * K + j]++, met[(size_t)j * K + i]++;
        }
        for (int v = 0; v < K; ++v)
            if (used[v] != 1) return fail("a vector is not in exactly one pair of a round", r, v);
    }
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j)
            if (i != j && met[(size_t)i * K + j] != 1) return fail("two vectors do not meet exactly once per sweep", i, j);
    return 0;
}

int main() {
    int bad = 0;
    const int sizes[][2] = {{64, 64}, {67, 81}, {64, 65}, {65, 64}, {66, 70}, {71, 93}, {270, 480}, {1080, 1920}};
    for (const auto& s : sizes) bad += check_pyramid(s[0], s[1]);
    bad += check_points();
    const int clips[][3] = {{9, 10, 1}, {10, 10, 1}, {11, 10, 1}, {12, 10, 2}, {18, 16, 2}, {20, 16, 2}, {24, 16, 1}, {25, 16, 3}, {300, 16, 1}};
    for (const auto& c : clips) bad += check_tracks(c[0], c[1], c[2]);
    for (int k = 1; k <= 40; ++k) bad += check_pairs(k);
    const int more[] = {127, 128, 129, 130, 511, 512, 1023, 1024};
    for (int k : more) bad += check_pairs(k);
    if (bad) return 1;
    std::puts("fvmd_index_check: ok");
    return 0;
}
