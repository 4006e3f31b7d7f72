// Foreground masks in UFO's slot: segment_frames of presley.py:203, the mask files of elvis.py:1187.
// UFO is a trained video salient-object network; neither its architecture nor its weights are available to this build.
// This is a BUILD-DEFINED, training-free segmenter behind that call surface - global motion compensation, a motion
// residual, a colour distance to the frame's border, Otsu, a little morphology and a temporal vote - in integers with
// one float64 threshold search, and it claims no parity with UFO.  tests/_segment_ref.py states it in numpy; this file
// equals every stage of that bit for bit.  Every stage is an image kernel over the 1/4-resolution grid (Ry = h / 4,
// Rx = w / 4, P = Ry * Rx) of the extended clip of m = n_before + n + n_after frames:
//   seg_reduce_kernel<C>   Y, U, V (i420.h) summed over 4 x 4 pixels                          -> red
//   seg_strips_kernel      the mean colour of the four border strips                          -> means
//   seg_sad_kernel         the SAD of every shift in [-R, R]^2 over the common window         -> sad  (64-bit atomics)
//   seg_pick_kernel        the least (sad, dy*dy + dx*dx, dy, dx)                             -> shift
//   seg_terms_kernel       motion residual M (3 x 3 min, 3 x 3 sum), spatial term S, maxima   -> mraw, sraw, maxima
//   seg_fuse_kernel        Mn, Sn, their weighted mean, the 5 x 5 mean F, F's histogram       -> mn, sn, f, hist
//   seg_threshold_kernel   Otsu in float64, one wave a frame; 255 where max(F) < min_peak     -> thr
//   seg_morph_kernel       F > thr, close, open, `dilation` dilations on an LDS tile          -> pre
//   seg_vote_kernel        2 of 3 over t - 1, t, t + 1 for the n frames, the foreground count -> voted, count
//   seg_upsample_kernel    the fallback to ones, x 4 nearest                                  -> masks
// Nothing is read back to the host.  The frame bytes are read by seg_reduce_kernel alone, byte by byte: a row of 3 w
// bytes is in general not 4-byte aligned.
#include <limits.h>
#include "common.h"
#include "i420.h"

namespace {

constexpr int kQ = 4;
constexpr int kThreads = 256;
constexpr int kMaxRadius = 16, kMaxDilation = 4, kMaxWeight = 1024, kMaxSide = 16384, kMaxFrames = 4096;
constexpr int kShareDen = 10000;
constexpr int kSadTileY = 16, kSadTileX = 64;            // a tile of the common window
constexpr int kSadThreads = 320;                         // 5 waves: the 289 shifts of R = 8 in one pass
constexpr int kSadPitch = kSadTileX + 2 * kMaxRadius + 1;    // 97: odd, the rows of the partner tile share no bank
constexpr int kTile = 16;                                // seg_terms_kernel and seg_fuse_kernel: 16 x 16 pixels a workgroup
constexpr int kResSide = kTile + 2, kFuseSide = kTile + 4;   // with the halo of the 3 x 3 and the 5 x 5 sum
constexpr int kMorphTile = 32;
constexpr int kMorphSide = kMorphTile + 2 * (4 + kMaxDilation);   // 48
constexpr int kAlign = 256;

// The workspace: byte offsets of every section, each a multiple of 256.  sad .. count are zeroed by every call.
struct Layout {
    size_t red;      // u16 [m][3][P]   the reduced Y, U, V planes
    size_t sad;      // u64 [m][D * D]  D = 2 R + 1, entry (dy + R) * D + dx + R
    size_t maxima;   // i32 [m][2]      max(M), max(S)
    size_t hist;     // u32 [m][256]    the histogram of F
    size_t count;    // u32 [m]         foreground pixels after the vote (the first n entries)
    size_t shift;    // i32 [m][2]      dy, dx
    size_t means;    // i32 [m][4][3]   top, bottom, left, right strip; Y, U, V
    size_t mraw;     // u16 [m][P]      M (at most 9 * 3840)
    size_t sraw;     // u16 [m][P]      S (at most 3 * 3840)
    size_t mn;       // u8  [m][P]
    size_t sn;       // u8  [m][P]
    size_t f;        // u8  [m][P]
    size_t thr;      // i32 [m]
    size_t pre;      // u8  [m][P]      the cleaned mask before the vote
    size_t voted;    // u8  [m][P]      after the vote (the first n frames)
    size_t total;
};
inline size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }
Layout make_layout(int m, size_t P, int R) {
    const size_t M = (size_t)m, D2 = (size_t)(2 * R + 1) * (2 * R + 1);
    Layout l;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = align_up(at + bytes); return o; };
    l.red = take(M * 3 * P * 2);
    l.sad = take(M * D2 * 8);
    l.maxima = take(M * 2 * 4);
    l.hist = take(M * 256 * 4);
    l.count = take(M * 4);
    l.shift = take(M * 2 * 4);
    l.means = take(M * 12 * 4);
    l.mraw = take(M * P * 2);
    l.sraw = take(M * P * 2);
    l.mn = take(M * P);
    l.sn = take(M * P);
    l.f = take(M * P);
    l.thr = take(M * 4);
    l.pre = take(M * P);
    l.voted = take(M * P);
    l.total = at;
    return l;
}

bool shape_ok(int m, int h, int w, int R) {
    if (m < 1 || m > kMaxFrames || h < kQ || w < kQ || h > kMaxSide || w > kMaxSide || R < 0 || R > kMaxRadius) return false;
    return h / kQ >= 2 * R + 1 && w / kQ >= 2 * R + 1;
}

// the extended clip: before, frames, after - three buffers, one frame index
struct Clip {
    const uint8_t *before, *frames, *after;
    int nb, n;
    long long frame_bytes;
};
__device__ __forceinline__ const uint8_t* frame_ptr(const Clip& c, int e) {
    if (e < c.nb) return c.before + e * c.frame_bytes;
    if (e < c.nb + c.n) return c.frames + (e - c.nb) * c.frame_bytes;
    return c.after + (e - c.nb - c.n) * c.frame_bytes;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(hi, max(lo, v)); }
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------ 1. reduce
// One thread a reduced pixel: 16 pixels, C bytes each, read as bytes.  grid (ceil(P / 256), m).
template <int C>
__global__ __launch_bounds__(kThreads) void seg_reduce_kernel(Clip clip, uint16_t* __restrict__ red, int w, int ry, int rx, int bgr) {
    const int P = ry * rx, p = blockIdx.x * kThreads + threadIdx.x, e = blockIdx.y;
    if (p >= P) return;
    const int y = p / rx, x = p - y * rx;
    const uint8_t* f = frame_ptr(clip, e);
    int sy = 0, su = 0, sv = 0;
#pragma unroll
    for (int j = 0; j < kQ; ++j) {
        const uint8_t* row = f + ((long long)(y * kQ + j) * w + x * kQ) * C;
#pragma unroll
        for (int i = 0; i < kQ; ++i) {
            if (C == 1) {
                sy += row[i];
                su += 128;
                sv += 128;
            } else {
                const int c0 = row[i * 3], g = row[i * 3 + 1], c2 = row[i * 3 + 2];
                const int r = bgr ? c2 : c0, b = bgr ? c0 : c2;
                sy += i420_y(r, g, b);
                su += i420_u(r, g, b);
                sv += i420_v(r, g, b);
            }
        }
    }
    uint16_t* o = red + (size_t)e * 3 * P;
    o[p] = (uint16_t)sy;
    o[P + p] = (uint16_t)su;
    o[2 * (size_t)P + p] = (uint16_t)sv;
}

// ------------------------------------------------------------------ 4a. the border strips
// grid (4, m): strip 0 / 1 the top / bottom bw rows, 2 / 3 the left / right bw columns, full length.  A two-pass sum
// (thread, wave, workgroup) in 64 bits; the mean is sum / count, floored.
__global__ __launch_bounds__(kThreads) void seg_strips_kernel(const uint16_t* __restrict__ red, int* __restrict__ means, int ry, int rx) {
    __shared__ long long part[3][kThreads / 64];
    const int s = blockIdx.x, e = blockIdx.y, P = ry * rx;
    const int bw = max(1, min(ry, rx) / 16);
    const int count = bw * (s < 2 ? rx : ry);
    const uint16_t* r = red + (size_t)e * 3 * P;
    long long sum[3] = {0, 0, 0};
    for (int i = threadIdx.x; i < count; i += kThreads) {
        int y, x;
        if (s < 2) {
            y = i / rx;
            x = i - y * rx;
            if (s == 1) y += ry - bw;
        } else {
            y = i / bw;
            x = i - y * bw;
            if (s == 3) x += rx - bw;
        }
        const int p = y * rx + x;
#pragma unroll
        for (int k = 0; k < 3; ++k) sum[k] += r[(size_t)k * P + p];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long v = wave_sum_ll(sum[k]);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const long long v = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        means[(e * 4 + s) * 3 + threadIdx.x] = (int)(v / count);
    }
}

// ------------------------------------------------------------------ 2. global motion
// grid (tiles of the window, m).  The window is y in [R, ry - R), x in [R, rx - R); a workgroup takes a 16 x 64 tile of
// it, holds the tile of the frame and the (16 + 2R) x (64 + 2R) tile of the partner in LDS, and thread i sums shift i
// (and i + 320, ...) over the tile: the frame's pixel is one address for the whole wave (a broadcast), the partner's
// consecutive addresses for consecutive dx.  A tile's sum is at most 1024 * 3840; the table is 64-bit.
__global__ __launch_bounds__(kSadThreads) void seg_sad_kernel(const uint16_t* __restrict__ red, unsigned long long* __restrict__ sad,
                                                              int ry, int rx, int R, int tiles_x) {
    __shared__ int cs[kSadTileY * kSadTileX];
    __shared__ int os[(kSadTileY + 2 * kMaxRadius) * kSadPitch];
    const int e = blockIdx.y, partner = e > 0 ? e - 1 : 1, P = ry * rx;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kSadTileY, x0 = tx * kSadTileX;          // the partner tile's corner; the frame's is (y0 + R, x0 + R)
    const int th = min(kSadTileY, ry - 2 * R - y0), tw = min(kSadTileX, rx - 2 * R - x0);
    const uint16_t* cy = red + (size_t)e * 3 * P;
    const uint16_t* oy = red + (size_t)partner * 3 * P;
    for (int i = threadIdx.x; i < th * tw; i += kSadThreads) {
        const int py = i / tw, px = i - py * tw;
        cs[py * kSadTileX + px] = cy[(y0 + R + py) * rx + x0 + R + px];
    }
    const int oh = th + 2 * R, ow = tw + 2 * R;                  // y0 + oh <= ry, x0 + ow <= rx
    for (int i = threadIdx.x; i < oh * ow; i += kSadThreads) {
        const int py = i / ow, px = i - py * ow;
        os[py * kSadPitch + px] = oy[(y0 + py) * rx + x0 + px];
    }
    __syncthreads();
    const int D = 2 * R + 1;
    for (int cand = threadIdx.x; cand < D * D; cand += kSadThreads) {
        const int dyi = cand / D, dxi = cand - dyi * D;
        int acc = 0;
        for (int py = 0; py < th; ++py) {
            const int* crow = cs + py * kSadTileX;
            const int* orow = os + (py + dyi) * kSadPitch + dxi;
#pragma unroll 4
            for (int px = 0; px < tw; ++px) acc += abs(crow[px] - orow[px]);
        }
        atomicAdd(&sad[(size_t)e * D * D + cand], (unsigned long long)acc);
    }
}

// grid m, one wave: the least (sad, dy*dy + dx*dx, dy, dx).  key = d2 << 12 | (dy + R) << 6 | (dx + R) orders the last
// three (dy + R, dx + R <= 32, d2 <= 512).
__global__ __launch_bounds__(64) void seg_pick_kernel(const unsigned long long* __restrict__ sad, int* __restrict__ shift, int R) {
    const int e = blockIdx.x, D = 2 * R + 1, lane = threadIdx.x;
    unsigned long long best = ~0ull;
    unsigned key = ~0u;
    for (int cand = lane; cand < D * D; cand += 64) {
        const int dyi = cand / D, dxi = cand - dyi * D, dy = dyi - R, dx = dxi - R;
        const unsigned long long s = sad[(size_t)e * D * D + cand];
        const unsigned k = ((unsigned)(dy * dy + dx * dx) << 12) | ((unsigned)dyi << 6) | (unsigned)dxi;
        if (s < best || (s == best && k < key)) {
            best = s;
            key = k;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long s = __shfl_xor(best, o, 64);
        const unsigned k = __shfl_xor(key, o, 64);
        if (s < best || (s == best && k < key)) {
            best = s;
            key = k;
        }
    }
    if (lane == 0) {
        shift[e * 2] = (int)((key >> 6) & 63) - R;
        shift[e * 2 + 1] = (int)(key & 63) - R;
    }
}

// ------------------------------------------------------------------ 3, 4b. motion residual and spatial term
// grid (tiles of 16 x 16, m).  res on the tile and a halo of one (coordinates clamped: the edge replication of the
// 3 x 3 sum), then M from LDS; S from the pixel's colour and the four means.  The maxima: wave, then one atomicMax.
__global__ __launch_bounds__(kThreads) void seg_terms_kernel(const uint16_t* __restrict__ red, const int* __restrict__ shift,
                                                             const int* __restrict__ means, uint16_t* __restrict__ mraw,
                                                             uint16_t* __restrict__ sraw, int* __restrict__ maxima, int ry, int rx,
                                                             int tiles_x, int has_motion) {
    __shared__ int res[kResSide * kResSide];
    const int e = blockIdx.y, P = ry * rx;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int ty0 = ty * kTile, tx0 = tx * kTile;
    const uint16_t* cy = red + (size_t)e * 3 * P;
    if (has_motion) {
        const uint16_t* oy = red + (size_t)(e > 0 ? e - 1 : 1) * 3 * P;
        const int dy = shift[e * 2], dx = shift[e * 2 + 1];
        for (int i = threadIdx.x; i < kResSide * kResSide; i += kThreads) {
            const int ly = i / kResSide, lx = i - ly * kResSide;
            const int gy = clampi(ty0 - 1 + ly, 0, ry - 1), gx = clampi(tx0 - 1 + lx, 0, rx - 1);
            const int sy = gy + dy, sx = gx + dx;
            int r = 0;
            if (sy >= 0 && sy < ry && sx >= 0 && sx < rx) {
                const int c = cy[gy * rx + gx];
                r = INT_MAX;
#pragma unroll
                for (int a = -1; a <= 1; ++a)
#pragma unroll
                    for (int b = -1; b <= 1; ++b)
                        r = min(r, abs(c - (int)oy[clampi(sy + a, 0, ry - 1) * rx + clampi(sx + b, 0, rx - 1)]));
            }
            res[i] = r;
        }
    }
    __syncthreads();
    const int ly = threadIdx.x / kTile, lx = threadIdx.x - ly * kTile;
    const int y = ty0 + ly, x = tx0 + lx;
    int M = 0, S = 0;
    if (y < ry && x < rx) {
        if (has_motion) {
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) M += res[(ly + a) * kResSide + lx + b];
        }
        const int p = y * rx + x;
        const int Y = cy[p], U = cy[(size_t)P + p], V = cy[2 * (size_t)P + p];
        const int* mean = means + e * 12;
        S = INT_MAX;
#pragma unroll
        for (int s = 0; s < 4; ++s) S = min(S, abs(Y - mean[s * 3]) + abs(U - mean[s * 3 + 1]) + abs(V - mean[s * 3 + 2]));
        mraw[(size_t)e * P + p] = (uint16_t)M;
        sraw[(size_t)e * P + p] = (uint16_t)S;
    }
    const int wm = wave_max_i(M), ws = wave_max_i(S);
    if ((threadIdx.x & 63) == 0) {
        if (wm > 0) atomicMax(&maxima[e * 2], wm);
        if (ws > 0) atomicMax(&maxima[e * 2 + 1], ws);
    }
}

// ------------------------------------------------------------------ 5. normalise, fuse, 5 x 5 mean, histogram
struct FuseParams {
    int wm, ws, motion_floor, spatial_floor, has_motion;
};
// grid (tiles of 16 x 16, m).  The fused value on the tile and a halo of two (clamped), then the 5 x 5 sum / 25 from
// LDS.  The histogram is summed in LDS and added to the frame's with one atomic a used bin.
__global__ __launch_bounds__(kThreads) void seg_fuse_kernel(const uint16_t* __restrict__ mraw, const uint16_t* __restrict__ sraw,
                                                            const int* __restrict__ maxima, uint8_t* __restrict__ mn_out,
                                                            uint8_t* __restrict__ sn_out, uint8_t* __restrict__ f_out,
                                                            unsigned* __restrict__ hist, int ry, int rx, int tiles_x, FuseParams fp) {
    __shared__ int f0[kFuseSide * kFuseSide];
    __shared__ unsigned lh[256];
    const int e = blockIdx.y, P = ry * rx;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int ty0 = ty * kTile, tx0 = tx * kTile;
    lh[threadIdx.x] = 0;
    const int max_m = max(maxima[e * 2], fp.motion_floor), max_s = max(maxima[e * 2 + 1], fp.spatial_floor);
    for (int i = threadIdx.x; i < kFuseSide * kFuseSide; i += kThreads) {
        const int ly = i / kFuseSide, lx = i - ly * kFuseSide;
        const int uy = ty0 - 2 + ly, ux = tx0 - 2 + lx;
        const int gy = clampi(uy, 0, ry - 1), gx = clampi(ux, 0, rx - 1);
        const size_t p = (size_t)e * P + gy * rx + gx;
        const int mn = fp.has_motion ? min(255, (int)mraw[p] * 255 / max_m) : 0;
        const int sn = min(255, (int)sraw[p] * 255 / max_s);
        f0[i] = fp.has_motion ? (fp.wm * mn + fp.ws * sn) / (fp.wm + fp.ws) : sn;
        if (ly >= 2 && ly < 2 + kTile && lx >= 2 && lx < 2 + kTile && uy < ry && ux < rx) {      // the tile's own pixels
            mn_out[p] = (uint8_t)mn;
            sn_out[p] = (uint8_t)sn;
        }
    }
    __syncthreads();
    const int ly = threadIdx.x / kTile, lx = threadIdx.x - ly * kTile;
    const int y = ty0 + ly, x = tx0 + lx;
    if (y < ry && x < rx) {
        int sum = 0;
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = 0; b < 5; ++b) sum += f0[(ly + a) * kFuseSide + lx + b];
        const int F = sum / 25;
        f_out[(size_t)e * P + y * rx + x] = (uint8_t)F;
        atomicAdd(&lh[F], 1u);
    }
    __syncthreads();
    const unsigned v = lh[threadIdx.x];
    if (v) atomicAdd(&hist[e * 256 + threadIdx.x], v);
}

// ------------------------------------------------------------------ 6. Otsu
// grid m, one wave; lane l has the bins 4l .. 4l + 3.  The prefix sums are integers (exact, whatever the order); the
// products, the square and the quotient are float64 in the statement's order, uncontracted.  The first strictly
// largest v wins: the larger v, then the smaller t.  255 where no candidate splits the histogram or max(F) < min_peak.
__global__ __launch_bounds__(64) void seg_threshold_kernel(const unsigned* __restrict__ hist, int* __restrict__ thr, int min_peak) {
    const int e = blockIdx.x, lane = threadIdx.x;
    long long h[4], w = 0, s = 0;
    int top = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        h[k] = hist[e * 256 + lane * 4 + k];
        w += h[k];
        s += h[k] * (lane * 4 + k);
        if (h[k]) top = lane * 4 + k;
    }
    const long long N = wave_sum_ll(w), tot = wave_sum_ll(s);
    top = wave_max_i(top);
    long long w0 = w, s0 = s;                          // inclusive scan over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long pw = __shfl_up(w0, o, 64), ps = __shfl_up(s0, o, 64);
        if (lane >= o) {
            w0 += pw;
            s0 += ps;
        }
    }
    w0 -= w;                                           // exclusive
    s0 -= s;
    double best_v = -1.0;
    int best_t = 255;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int t = lane * 4 + k;
        w0 += h[k];
        s0 += h[k] * t;
        const long long w1 = N - w0;
        if (t < 255 && w0 != 0 && w1 != 0) {
            const double d = (double)tot * (double)w0 - (double)s0 * (double)N;
            const double v = d * d / ((double)w0 * (double)w1);
            if (v > best_v) {
                best_v = v;
                best_t = t;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v = __shfl_xor(best_v, o, 64);
        const int t = __shfl_xor(best_t, o, 64);
        if (v > best_v || (v == best_v && t < best_t)) {
            best_v = v;
            best_t = t;
        }
    }
    if (lane == 0) thr[e] = top < min_peak ? 255 : best_t;
}

// ------------------------------------------------------------------ 7. clean
// grid (tiles of 32 x 32, m).  The binary mask on the tile and a halo of 4 + dilation, then dilate, erode, erode,
// dilate and `dilation` dilations between two LDS planes; every pass writes the positions inside the frame whose
// margin is one less, and reads its neighbours at coordinates clamped to the frame - the edge replication of that
// pass (a clamped neighbour is never farther from the tile than the unclamped one, so it was written by the pass
// before).
__global__ __launch_bounds__(kThreads) void seg_morph_kernel(const uint8_t* __restrict__ f, const int* __restrict__ thr,
                                                             uint8_t* __restrict__ pre, int ry, int rx, int tiles_x, int dilation) {
    __shared__ uint8_t plane[2][kMorphSide * kMorphSide];
    const int e = blockIdx.y, P = ry * rx;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int halo = 4 + dilation;
    const int oy = ty * kMorphTile - halo, ox = tx * kMorphTile - halo;      // the frame coordinates of plane (0, 0)
    const int side = kMorphTile + 2 * halo;
    const int t = thr[e];
    for (int i = threadIdx.x; i < side * side; i += kThreads) {
        const int ly = i / side, lx = i - ly * side;
        const int gy = oy + ly, gx = ox + lx;
        uint8_t v = 0;
        if (gy >= 0 && gy < ry && gx >= 0 && gx < rx) v = f[(size_t)e * P + gy * rx + gx] > t;
        plane[0][ly * kMorphSide + lx] = v;
    }
    __syncthreads();
    int cur = 0;
    for (int pass = 0; pass < halo; ++pass) {
        const bool dilate = pass != 1 && pass != 2;
        const int lo = pass + 1, span = side - 2 * lo;
        const uint8_t* src = plane[cur];
        uint8_t* dst = plane[cur ^ 1];
        for (int i = threadIdx.x; i < span * span; i += kThreads) {
            const int ly = lo + i / span, lx = lo + i % span;
            const int gy = oy + ly, gx = ox + lx;
            if (gy < 0 || gy >= ry || gx < 0 || gx >= rx) continue;
            int acc = dilate ? 0 : 1;
#pragma unroll
            for (int a = -1; a <= 1; ++a)
#pragma unroll
                for (int b = -1; b <= 1; ++b) {
                    const int v = src[(clampi(gy + a, 0, ry - 1) - oy) * kMorphSide + clampi(gx + b, 0, rx - 1) - ox];
                    acc = dilate ? (acc | v) : (acc & v);
                }
            dst[ly * kMorphSide + lx] = (uint8_t)acc;
        }
        __syncthreads();
        cur ^= 1;
    }
    const uint8_t* src = plane[cur];
    for (int i = threadIdx.x; i < kMorphTile * kMorphTile; i += kThreads) {
        const int ly = i / kMorphTile, lx = i - ly * kMorphTile;
        const int gy = ty * kMorphTile + ly, gx = tx * kMorphTile + lx;
        if (gy < ry && gx < rx) pre[(size_t)e * P + gy * rx + gx] = src[(ly + halo) * kMorphSide + lx + halo];
    }
}

// ------------------------------------------------------------------ 8. vote
// grid (ceil(P / 256), n).  Frame i of the call is frame nb + i of the extended clip.
__global__ __launch_bounds__(kThreads) void seg_vote_kernel(const uint8_t* __restrict__ pre, uint8_t* __restrict__ voted,
                                                            unsigned* __restrict__ count, int P, int nb, int m, int vote) {
    const int p = blockIdx.x * kThreads + threadIdx.x, i = blockIdx.y, e = nb + i;
    int v = 0;
    if (p < P) {
        v = pre[(size_t)e * P + p];
        if (vote && e - 1 >= 0 && e + 1 < m) v = (v + pre[(size_t)(e - 1) * P + p] + pre[(size_t)(e + 1) * P + p]) >= 2;
        voted[(size_t)i * P + p] = (uint8_t)v;
    }
    const unsigned c = (unsigned)__popcll(__ballot(v != 0));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&count[i], c);
}

// ------------------------------------------------------------------ 9, 10. fallback and upsample
// grid (ceil(h w / 256), n), one byte a thread.  A frame whose share is 0 or above share_num / 10000 is all ones.
__global__ __launch_bounds__(kThreads) void seg_upsample_kernel(const uint8_t* __restrict__ voted, const unsigned* __restrict__ count,
                                                                uint8_t* __restrict__ masks, int h, int w, int ry, int rx, int share_num) {
    const int i = blockIdx.y, P = ry * rx;
    const long long q = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (q >= (long long)h * w) return;
    const int y = (int)(q / w), x = (int)(q - (long long)y * w);
    const unsigned long long c = count[i];
    const bool ones = c == 0 || c * kShareDen > (unsigned long long)share_num * (unsigned long long)P;
    const uint8_t v = voted[(size_t)i * P + min(y / kQ, ry - 1) * rx + min(x / kQ, rx - 1)];
    masks[(long long)i * h * w + q] = ones ? (uint8_t)1 : v;
}

}  // namespace

extern "C" size_t elvis_segment_workspace_bytes(int m, int h, int w, int radius) {
    if (!shape_ok(m, h, w, radius)) return 0;
    return make_layout(m, (size_t)(h / kQ) * (w / kQ), radius).total;
}

extern "C" int elvis_segment_foreground_u8(const uint8_t* frames, const uint8_t* before, int n_before, const uint8_t* after, int n_after,
                                           uint8_t* masks, void* workspace, long long workspace_bytes, int n, int h, int w, int c, int bgr,
                                           int radius, int motion_weight, int spatial_weight, int motion_floor, int spatial_floor,
                                           int min_peak, int dilation, int share_num, int temporal_vote, elvis_stream_t stream) {
    ELVIS_REQUIRE(frames && masks && workspace, "elvis_segment_foreground_u8: null pointer");
    ELVIS_REQUIRE(c == 1 || c == 3, "elvis_segment_foreground_u8: %d channels (1 or 3 supported)", c);
    ELVIS_REQUIRE(n >= 1 && n_before >= 0 && n_before <= 2 && n_after >= 0 && n_after <= 1,
                  "elvis_segment_foreground_u8: n=%d frames (>= 1) with %d before (0..2) and %d after (0..1)", n, n_before, n_after);
    ELVIS_REQUIRE((n_before == 0 || before) && (n_after == 0 || after), "elvis_segment_foreground_u8: null halo frames");
    ELVIS_REQUIRE(radius >= 0 && radius <= kMaxRadius, "elvis_segment_foreground_u8: radius %d outside 0..%d", radius, kMaxRadius);
    const int m = n_before + n + n_after;
    ELVIS_REQUIRE(shape_ok(m, h, w, radius),
                  "elvis_segment_foreground_u8: beyond the limits (%d frames <= %d, h=%d w=%d in 4..%d, and the reduced %d x %d frame "
                  "must be at least 2 * radius + 1 = %d on each side)",
                  m, kMaxFrames, h, w, kMaxSide, h / kQ, w / kQ, 2 * radius + 1);
    ELVIS_REQUIRE(dilation >= 0 && dilation <= kMaxDilation, "elvis_segment_foreground_u8: dilation %d outside 0..%d", dilation, kMaxDilation);
    ELVIS_REQUIRE(motion_weight >= 1 && motion_weight <= kMaxWeight && spatial_weight >= 1 && spatial_weight <= kMaxWeight,
                  "elvis_segment_foreground_u8: weights %d, %d outside 1..%d", motion_weight, spatial_weight, kMaxWeight);
    ELVIS_REQUIRE(motion_floor >= 1 && spatial_floor >= 1, "elvis_segment_foreground_u8: floors %d, %d must be positive", motion_floor,
                  spatial_floor);
    ELVIS_REQUIRE(min_peak >= 0 && min_peak <= 255, "elvis_segment_foreground_u8: min_peak %d outside 0..255", min_peak);
    ELVIS_REQUIRE(share_num >= 1 && share_num <= kShareDen, "elvis_segment_foreground_u8: max_share %d / %d outside (0, 1]", share_num,
                  kShareDen);
    const int ry = h / kQ, rx = w / kQ, P = ry * rx;
    const Layout l = make_layout(m, (size_t)P, radius);
    ELVIS_REQUIRE(workspace_bytes >= 0 && (size_t)workspace_bytes >= l.total,
                  "elvis_segment_foreground_u8: workspace of %lld bytes, %zu needed (elvis_segment_workspace_bytes)", workspace_bytes, l.total);
    ELVIS_REQUIRE((uintptr_t)workspace % 8 == 0, "elvis_segment_foreground_u8: workspace must be 8-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    uint16_t* red = (uint16_t*)(ws + l.red);
    unsigned long long* sad = (unsigned long long*)(ws + l.sad);
    int* maxima = (int*)(ws + l.maxima);
    unsigned* hist = (unsigned*)(ws + l.hist);
    unsigned* count = (unsigned*)(ws + l.count);
    int* shift = (int*)(ws + l.shift);
    int* means = (int*)(ws + l.means);
    uint16_t* mraw = (uint16_t*)(ws + l.mraw);
    uint16_t* sraw = (uint16_t*)(ws + l.sraw);
    int* thr = (int*)(ws + l.thr);
    const int has_motion = m > 1;

    // sad, maxima, hist, count and the shifts (read as (0, 0) by a one-frame clip's details) start at zero
    hipError_t err = hipMemsetAsync(ws + l.sad, 0, l.means - l.sad, st);
    if (err != hipSuccess) {
        elvis_set_error("elvis_segment_foreground_u8: hipMemsetAsync failed: %s", hipGetErrorString(err));
        return ELVIS_E_RUNTIME;
    }
    const Clip clip = {before, frames, after, n_before, n, (long long)h * w * c};
    const dim3 per_pixel((unsigned)cdiv(P, kThreads), (unsigned)m);
    if (c == 3)
        hipLaunchKernelGGL(seg_reduce_kernel<3>, per_pixel, dim3(kThreads), 0, st, clip, red, w, ry, rx, bgr ? 1 : 0);
    else
        hipLaunchKernelGGL(seg_reduce_kernel<1>, per_pixel, dim3(kThreads), 0, st, clip, red, w, ry, rx, 0);
    ELVIS_CHECK_LAUNCH("elvis_segment_foreground_u8 (reduce)");
    hipLaunchKernelGGL(seg_strips_kernel, dim3(4, (unsigned)m), dim3(kThreads), 0, st, red, means, ry, rx);
    ELVIS_CHECK_LAUNCH("elvis_segment_foreground_u8 (strips)");
    if (has_motion) {
        const int sty = cdiv(ry - 2 * radius, kSadTileY), stx = cdiv(rx - 2 * radius, kSadTileX);
        hipLaunchKernelGGL(seg_sad_kernel, dim3((unsigned)(sty * stx), (unsigned)m), dim3(kSadThreads), 0, st, red, sad, ry, rx, radius, stx);
        ELVIS_CHECK_LAUNCH("elvis_segment_foreground_u8 (sad)");
        hipLaunchKernelGGL(seg_pick_kernel, dim3((unsigned)m), dim3(64), 0, st, sad, shift, radius);
        ELVIS_CHECK_LAUNCH("elvis_segment_foreground_u8 (pick)");
    }
    const int tiles_y = cdiv(ry, kTile), tiles_x = cdiv(rx, kTile);
    const dim3 tiles((unsigned)(tiles_y * tiles_x), (unsigned)m);
    hipLaunchKernelGGL(seg_terms_kernel, tiles, dim3(kThreads), 0, st, red, shift, means, mraw, sraw, maxima, ry, rx, tiles_x, has_motion);
    ELVIS_CHECK_LAUNCH("elvis_segment_foreground_u8 (terms)");
    const FuseParams fp = {motion_weight, spatial_weight, motion_floor, spatial_floor, has_motion};
    hipLaunchKernelGGL(seg_fuse_kernel, tiles, dim3(kThreads), 0, st, mraw, sraw, maxima, ws + l.mn, ws + l.sn, ws + l.f, hist, ry, rx,
                       tiles_x, fp);
    ELVIS_CHECK_LAUNCH("elvis_segment_foreground_u8 (fuse)");
    hipLaunchKernelGGL(seg_threshold_kernel, dim3((unsigned)m), dim3(64), 0, st, hist, thr, min_peak);
    ELVIS_CHECK_LAUNCH("elvis_segment_foreground_u8 (threshold)");
    const int mty = cdiv(ry, kMorphTile), mtx = cdiv(rx, kMorphTile);
    hipLaunchKernelGGL(seg_morph_kernel, dim3((unsigned)(mty * mtx), (unsigned)m), dim3(kThreads), 0, st, ws + l.f, thr, ws + l.pre, ry, rx,
                       mtx, dilation);
    ELVIS_CHECK_LAUNCH("elvis_segment_foreground_u8 (morph)");
    hipLaunchKernelGGL(seg_vote_kernel, dim3((unsigned)cdiv(P, kThreads), (unsigned)n), dim3(kThreads), 0, st, ws + l.pre, ws + l.voted, count,
                       P, n_before, m, temporal_vote ? 1 : 0);
    ELVIS_CHECK_LAUNCH("elvis_segment_foreground_u8 (vote)");
    hipLaunchKernelGGL(seg_upsample_kernel, dim3((unsigned)cdiv((long long)h * w, kThreads), (unsigned)n), dim3(kThreads), 0, st,
                       ws + l.voted, count, masks, h, w, ry, rx, share_num);
    ELVIS_CHECK_LAUNCH("elvis_segment_foreground_u8 (upsample)");
    elvis_note_launch("seg_upsample_kernel");
    return ELVIS_OK;
}
