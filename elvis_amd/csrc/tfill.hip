// Temporal fill of the ELVIS v1 holes: a removed block's content is taken from neighbouring frames where
// the same scene point was not removed.  The reference runs trained video inpainters in this slot (ProPainter, E2FGVI:
// elvis.py:1458, 1693; utils.py:1395-1425; presley.py:854-885).  This is a BUILD-DEFINED restatement of the one part of
// those methods that needs no training - find where a block's surroundings are in a neighbouring frame and copy the
// pixels the hole hides - in integers, and it claims no parity with either network.  tests/_tfill_ref.py states it in
// numpy; this file equals that bit for bit.
//   elvis_tfill_limits_ok - host only: 1 for a shape and parameters the entry point takes
//   elvis_tfill           - one launch of tfill_kernel<C> over all (frame, block) pairs
// "Known" is always the INPUT mask and source bytes are always INPUT bytes: nothing a fill writes is read by another
// fill, so the workgroups are independent and the launch order does not matter.  Every byte of `out` and `left` is
// written exactly once, by the thread that owns the pixel.
#include <limits.h>
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlock = 32, kMaxMargin = 16, kMaxRadius = 8, kMaxSearch = 7;
constexpr int kMinContext = 64;
constexpr int kWin = kMaxBlock + 2 * kMaxMargin;     // 64: the target window's side at most, and its LDS pitch
constexpr int kReg = kWin + 2 * kMaxSearch;          // 78: the search region's side at most
constexpr int kRegPitch = 79;                        // 79 % 32 = 15: the 15 dx of one dy and the next dy's share no bank
constexpr int kOwned = kMaxBlock * kMaxBlock / kThreads;   // block pixels a thread owns at most

// The mask is [n, h, w] (block == 0) or [n, h / block, w / block] expanded over whole blocks (pixels past the last
// whole block are known).  Non-zero = hole.
struct MaskView {
    const uint8_t* m;
    int block, by, bx;
};
__device__ __forceinline__ bool is_hole(const MaskView& mv, int f, int y, int x, int h, int w) {
    if (mv.block == 0) return mv.m[((long long)f * h + y) * w + x] != 0;
    const int yb = y / mv.block, xb = x / mv.block;
    return yb < mv.by && xb < mv.bx && mv.m[((long long)f * mv.by + yb) * mv.bx + xb] != 0;
}

struct Params {
    int n, h, w;
    int B, G, R, S, M;
    int nby, nbx;
};

// A pixel in LDS: its bytes in the low three (C = 1: one), 1 in the fourth where it may be compared - a known pixel of
// the target, a known pixel inside the frame of a source.
template <int C>
__device__ __forceinline__ uint32_t load_pixel(const uint8_t* __restrict__ frames, long long pix, bool flag) {
    const uint8_t* p = frames + pix * C;
    uint32_t v = p[0];
    if (C == 3) v |= ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    return v | ((uint32_t)flag << 24);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the sum of v over the workgroup, in every thread; red: 4 ints of LDS (a barrier on either side of their use)
__device__ __forceinline__ int block_sum(int v, int* red) {
    v = wave_sum_i(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// A candidate: cnt == 0 means none.  a beats b iff a's mean difference is smaller - exactly, cost_a * cnt_b <
// cost_b * cnt_a in 64 bits (up to 4096 * 765 * 4096) - or equal with the earlier raster index.
struct Cand {
    uint32_t cost, cnt, idx;
};
__device__ __forceinline__ bool beats(const Cand& a, const Cand& b) {
    if (a.cnt == 0) return false;
    if (b.cnt == 0) return true;
    const uint64_t l = (uint64_t)a.cost * b.cnt, r = (uint64_t)b.cost * a.cnt;
    return l < r || (l == r && a.idx < b.idx);
}

// One workgroup per (frame t, block): the block's hole pixels are filled from the frames t-1, t+1, t-2, ... t+R.
// Thread i owns displacement i of the (2S+1)^2 and the block pixels i, i + 256, ...
template <int C>
__global__ __launch_bounds__(kThreads) void tfill_kernel(const uint8_t* __restrict__ frames, MaskView mv, uint8_t* __restrict__ out,
                                                         uint8_t* __restrict__ left, Params p) {
    __shared__ uint32_t tw[kWin * kWin];             // the target window
    __shared__ uint32_t sw[kReg * kRegPitch];        // a source's search region
    __shared__ int red[4];
    __shared__ Cand wbest[4];

    const int tid = threadIdx.x, lane = tid & 63;
    const int h = p.h, w = p.w, B = p.B, S = p.S;
    int g = blockIdx.x;
    const int bxi = g % p.nbx;
    g /= p.nbx;
    const int byi = g % p.nby, t = g / p.nby;
    const int by = byi * B, bx = bxi * B;
    const int bh = min(B, h - by), bw = min(B, w - bx);

    // the pixels this thread owns: state 0 = known, 1 = hole (unfilled), 2 = filled (`fill` holds the bytes)
    int state[kOwned];
    uint32_t fill[kOwned];
    int holes = 0;
#pragma unroll
    for (int k = 0; k < kOwned; ++k) {
        const int i = tid + k * kThreads, ly = i / B, lx = i - ly * B;
        state[k] = -1;                                // not a pixel of the block
        fill[k] = 0;
        if (i < B * B && ly < bh && lx < bw) {
            state[k] = is_hole(mv, t, by + ly, bx + lx, h, w) ? 1 : 0;
            holes += state[k];
        }
    }
    // A block without holes: its pixels are copied and the workgroup leaves before any barrier.  Every wave decides
    // for the whole block (a wave sees only a quarter of it in its own pixels), so the exit is workgroup-uniform.
    bool any = false;
    for (int i = lane; i < bh * bw; i += 64) {
        const int ly = i / bw, lx = i - ly * bw;
        any |= is_hole(mv, t, by + ly, bx + lx, h, w);
    }
    const bool block_has_hole = __ballot(any) != 0;

    int remaining = 0;
    if (block_has_hole) {
        const int y0 = max(0, by - p.G), y1 = min(h, by + B + p.G), x0 = max(0, bx - p.G), x1 = min(w, bx + B + p.G);
        const int wh = y1 - y0, ww = x1 - x0;         // <= kWin
        int known = 0;
        for (int i = tid; i < wh * ww; i += kThreads) {
            const int ly = i / ww, lx = i - ly * ww;
            const bool k = !is_hole(mv, t, y0 + ly, x0 + lx, h, w);
            tw[ly * kWin + lx] = load_pixel<C>(frames, ((long long)t * h + y0 + ly) * w + x0 + lx, k);
            known += k;
        }
        const int nk = block_sum(known, red);          // its barriers also publish tw
        remaining = block_sum(holes, red);
        if (nk >= kMinContext) {
            const int D = 2 * S + 1;
            const int rh = wh + 2 * S, rw = ww + 2 * S;   // <= kReg
            const int dy = tid / D, dx = tid - dy * D;    // the displacement is (dy - S, dx - S); it exists iff tid < D * D
            for (int k = 1; k <= p.R && remaining > 0; ++k)
                for (int sign = -1; sign <= 1 && remaining > 0; sign += 2) {
                    const int s = t + sign * k;
                    if (s < 0 || s >= p.n) continue;      // uniform
                    for (int i = tid; i < rh * rw; i += kThreads) {
                        const int ly = i / rw, lx = i - ly * rw;
                        const int y = y0 - S + ly, x = x0 - S + lx;
                        uint32_t v = 0;                   // outside the frame: in no P(d), the source of no fill
                        if (y >= 0 && y < h && x >= 0 && x < w)
                            v = load_pixel<C>(frames, ((long long)s * h + y) * w + x, !is_hole(mv, s, y, x, h, w));
                        sw[ly * kRegPitch + lx] = v;
                    }
                    __syncthreads();
                    Cand mine = {0u, 0u, (uint32_t)tid};
                    if (tid < D * D) {
                        uint32_t cost = 0, cnt = 0;
                        for (int py = 0; py < wh; ++py) {
                            const uint32_t* trow = tw + py * kWin;
                            const uint32_t* srow = sw + (py + dy) * kRegPitch + dx;
#pragma unroll 4
                            for (int px = 0; px < ww; ++px) {
                                const uint32_t a = trow[px], b = srow[px];
                                const uint32_t both = (a & b) >> 24;          // 1 iff p is in P(d)
                                cnt += both;
                                cost = __builtin_amdgcn_sad_u8(a, both ? b : a, cost);   // outside P(d): equal, adds nothing
                            }
                        }
                        // valid: 2 * cnt >= nk (so cnt >= 32); accepted: cost <= M * cnt * C
                        if (2 * (int)cnt >= nk && cost <= (uint32_t)p.M * cnt * C) {
                            mine.cost = cost;
                            mine.cnt = cnt;
                        }
                    }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        Cand other = {(uint32_t)__shfl_xor((int)mine.cost, o, 64), (uint32_t)__shfl_xor((int)mine.cnt, o, 64),
                                      (uint32_t)__shfl_xor((int)mine.idx, o, 64)};
                        if (beats(other, mine)) mine = other;
                    }
                    if (lane == 0) wbest[tid >> 6] = mine;
                    __syncthreads();
                    Cand best = wbest[0];
#pragma unroll
                    for (int i = 1; i < 4; ++i) {
                        const Cand other = wbest[i];
                        if (beats(other, best)) best = other;
                    }
                    int filled_now = 0;
                    if (best.cnt != 0) {
                        const int bdy = (int)best.idx / D, bdx = (int)best.idx - bdy * D;
#pragma unroll
                        for (int k2 = 0; k2 < kOwned; ++k2)
                            if (state[k2] == 1) {
                                const int i = tid + k2 * kThreads, ly = i / B, lx = i - ly * B;
                                const uint32_t v = sw[(by - y0 + ly + bdy) * kRegPitch + (bx - x0 + lx + bdx)];
                                if (v >> 24) {
                                    state[k2] = 2;
                                    fill[k2] = v;
                                    ++filled_now;
                                }
                            }
                    }
                    remaining -= block_sum(filled_now, red);   // its barriers: sw and wbest are free again
                }
        }
    }

    // every pixel of the block is written once: the input's bytes where nothing arrived, 255 in `left` on those holes
#pragma unroll
    for (int k = 0; k < kOwned; ++k)
        if (state[k] >= 0) {
            const int i = tid + k * kThreads, ly = i / B, lx = i - ly * B;
            const long long pix = ((long long)t * h + by + ly) * w + bx + lx;
            uint32_t v = fill[k];
            if (state[k] != 2) v = load_pixel<C>(frames, pix, false);
            out[pix * C] = (uint8_t)v;
            if (C == 3) {
                out[pix * C + 1] = (uint8_t)(v >> 8);
                out[pix * C + 2] = (uint8_t)(v >> 16);
            }
            left[pix] = state[k] == 1 ? 255 : 0;
        }
}

bool limits_ok(int n, int h, int w, int c, int B, int G, int R, int S, int M) {
    if (n < 1 || h < 1 || w < 1 || h > 32767 || w > 32767 || (c != 1 && c != 3)) return false;   // H, W as the inpaint step
    if (B < 1 || B > kMaxBlock || G < 0 || G > kMaxMargin || R < 0 || R > kMaxRadius || S < 0 || S > kMaxSearch || M < 0 || M > 255)
        return false;
    if ((long long)n * h * w * c >= (1LL << 31)) return false;
    const long long blocks = (long long)n * ((h + B - 1) / B) * ((w + B - 1) / B);
    return blocks < (1LL << 31);
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" int elvis_tfill_limits_ok(int n, int h, int w, int c, int B, int G, int R, int S, int M) {
    return limits_ok(n, h, w, c, B, G, R, S, M) ? 1 : 0;
}

extern "C" int elvis_tfill(const uint8_t* frames, const uint8_t* masks, int block_mask_size, uint8_t* out, uint8_t* left, int n,
                           int h, int w, int c, int B, int G, int R, int S, int M, elvis_stream_t stream) {
    ELVIS_REQUIRE(frames && masks && out && left, "elvis_tfill: null pointer");
    ELVIS_REQUIRE(c == 1 || c == 3, "elvis_tfill: %d channels (1 or 3 supported)", c);
    ELVIS_REQUIRE(limits_ok(n, h, w, c, B, G, R, S, M),
                  "elvis_tfill: beyond the limits (n=%d h=%d w=%d with h, w <= 32767 and n*h*w*c < 2^31; block %d in 1..%d, margin %d in 0..%d, "
                  "radius %d in 0..%d, search %d in 0..%d, max_mad %d in 0..255)",
                  n, h, w, B, kMaxBlock, G, kMaxMargin, R, kMaxRadius, S, kMaxSearch, M);
    ELVIS_REQUIRE(block_mask_size >= 0, "elvis_tfill: block_mask_size %d must be 0 (a mask per pixel) or positive", block_mask_size);
    const size_t npix = (size_t)n * h * w;
    const size_t mask_bytes = block_mask_size ? (size_t)n * (h / block_mask_size) * (w / block_mask_size) : npix;
    ELVIS_REQUIRE(!overlap(out, npix * c, frames, npix * c), "elvis_tfill: out may not alias frames (sources stay input bytes)");
    ELVIS_REQUIRE(!overlap(left, npix, frames, npix * c) && !overlap(left, npix, out, npix * c) &&
                      !(mask_bytes && overlap(left, npix, masks, mask_bytes)),
                  "elvis_tfill: left may not alias frames, masks or out");
    ELVIS_REQUIRE(!(mask_bytes && overlap(out, npix * c, masks, mask_bytes)), "elvis_tfill: out may not alias masks");
    Params p = {n, h, w, B, G, R, S, M, (h + B - 1) / B, (w + B - 1) / B};
    MaskView mv = {masks, block_mask_size, block_mask_size ? h / block_mask_size : 0, block_mask_size ? w / block_mask_size : 0};
    const dim3 grid((unsigned)((long long)n * p.nby * p.nbx));
    if (c == 3)
        hipLaunchKernelGGL(tfill_kernel<3>, grid, dim3(kThreads), 0, (hipStream_t)stream, frames, mv, out, left, p);
    else
        hipLaunchKernelGGL(tfill_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, frames, mv, out, left, p);
    ELVIS_CHECK_LAUNCH("elvis_tfill");
    elvis_note_launch(c == 3 ? "tfill_kernel<3>" : "tfill_kernel<1>");
    return ELVIS_OK;
}
