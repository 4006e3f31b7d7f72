// FVMD of the evaluation report on the device: keypoint tracks, velocity / acceleration orientation histograms and the
// Frechet distance between two clips' feature rows.  The reference leans on the `fvmd` package (track_keypoints,
// calc_hist, calculate_fd_given_vectors: elvis.py:3476-3505); the package is available neither to the reference tree nor
// to this build, and its tracker is a network (PIPs++).  BUILD-DEFINED: a restatement of the published form - tracks ->
// velocity / acceleration -> cell orientation histograms -> Frechet distance - with a pyramidal Lucas-Kanade tracker in
// the network's place.  It does NOT claim parity with the `fvmd` package; its values are not comparable with published
// FVMD numbers.  The contract is stated in include/elvis_amd.h and DESIGN.md 7 and in numpy float64 in
// tests/_fvmd_ref.py.
//
// All arithmetic is float64, every expression in the one order the contract states, the library is built without FMA
// contraction and no fma is used; every reduction has a fixed order (lane partials in ascending index, then a butterfly
// or a tree) and there are no float atomics.  The tracker's one data branch is the singular test of a level; every
// sampling coordinate is clamped into the plane before it becomes an index, so no index depends on the data being sane.
// No kernel waits on another workgroup: the Jacobi sweeps run in one workgroup, or as one launch per pairing round.
#include "common.h"
#include "fvmd_index.h"

#define FVMD_THREADS 256
#define FVMD_WAVES (FVMD_THREADS / ELVIS_WAVE)
#define FVMD_PER_LANE 4              // ceil(225 / 64) window pixels a lane holds
#define FVMD_ITERS 8
#define FVMD_MIN_EIG 1e-3
#define FVMD_SWEEPS 16
#define FVMD_ROT_TOL 1e-15
#define FVMD_TILE 16
#define FVMD_QUARTER_PI 0.78539816339744830962

// every lane gets the wave's sum, by the butterfly 32, 16, 8, 4, 2, 1 (the two halves of the double are moved)
__device__ __forceinline__ double fvmd_wave_sum(double v) {
#pragma unroll
    for (int o = ELVIS_WAVE / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o, ELVIS_WAVE);
    return v;
}

// sum of the workgroup's 256 values in a fixed tree; `red` is 256 doubles of LDS
__device__ __forceinline__ double fvmd_tree_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int o = FVMD_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) red[t] = red[t] + red[t + o];
        __syncthreads();
    }
    const double total = red[0];
    __syncthreads();
    return total;
}

template <bool U8>
__device__ __forceinline__ double fvmd_load(const void* p, long long i) {
    if constexpr (U8) return (double)reinterpret_cast<const uint8_t*>(p)[i];
    else return reinterpret_cast<const double*>(p)[i];
}

// ----------------------------------------------------------------------------------------------------------- pyramid
// out[i][j] = ([1,4,6,4,1] / 16 applied vertically, then horizontally)(in)[2i][2j], every frame of the clip.  A lane takes
// one output pixel: the vertical pass of its five columns, then the horizontal pass over them, taps ascending.
template <bool U8>
__global__ __launch_bounds__(FVMD_THREADS) void fvmd_pyr_down_kernel(const void* __restrict__ in, double* __restrict__ out, int h, int w, int ho,
                                                                     int wo) {
    const long long i = (long long)blockIdx.x * FVMD_THREADS + threadIdx.x;
    if (i >= (long long)ho * wo) return;
    const int oy = (int)(i / wo), ox = (int)(i % wo);
    const long long base = (long long)blockIdx.y * h * w;
    const double c[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    int rows[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) rows[k] = fvmd_reflect(2 * oy + k - 2, h);
    double acc = 0.0;
#pragma unroll
    for (int kx = 0; kx < 5; ++kx) {
        const int x = fvmd_reflect(2 * ox + kx - 2, w);
        double col = c[0] * fvmd_load<U8>(in, base + (long long)rows[0] * w + x);
#pragma unroll
        for (int ky = 1; ky < 5; ++ky) col = col + c[ky] * fvmd_load<U8>(in, base + (long long)rows[ky] * w + x);
        acc = kx == 0 ? c[0] * col : acc + c[kx] * col;
    }
    out[(long long)blockIdx.y * ho * wo + i] = acc;
}

// ----------------------------------------------------------------------------------------------------------- tracker
// bilinear sample at (x, y), each coordinate clamped to [0, n - 1] first: every index lies inside the plane
template <bool U8>
__device__ __forceinline__ double fvmd_sample(const void* img, int h, int w, double x, double y) {
    x = fmin(fmax(x, 0.0), (double)(w - 1));
    y = fmin(fmax(y, 0.0), (double)(h - 1));
    const double fx0 = floor(x), fy0 = floor(y);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const double ax = x - fx0, ay = y - fy0;
    const double v00 = fvmd_load<U8>(img, (long long)y0 * w + x0), v01 = fvmd_load<U8>(img, (long long)y0 * w + x1);
    const double v10 = fvmd_load<U8>(img, (long long)y1 * w + x0), v11 = fvmd_load<U8>(img, (long long)y1 * w + x1);
    const double top = (1.0 - ax) * v00 + ax * v01;
    const double bot = (1.0 - ax) * v10 + ax * v11;
    return (1.0 - ay) * top + ay * bot;
}

// One pyramid level of one frame step: the template and its gradients over the 15 x 15 window around (px, py) of `cur`
// are held in registers, G is formed once, then 8 updates of (dx, dy) against `nxt`.  Every lane ends with the same d.
template <bool U8>
__device__ __forceinline__ void fvmd_level(const void* cur, const void* nxt, int h, int w, double px, double py, double& dx, double& dy,
                                           int lane) {
    double tpl[FVMD_PER_LANE], gx[FVMD_PER_LANE], gy[FVMD_PER_LANE], wx[FVMD_PER_LANE], wy[FVMD_PER_LANE];
    double sxx = 0.0, sxy = 0.0, syy = 0.0;
#pragma unroll
    for (int q = 0; q < FVMD_PER_LANE; ++q) {
        const int o = lane + ELVIS_WAVE * q;
        const bool on = o < FVMD_WIN_PIXELS;
        const int oo = on ? o : 0;
        wx[q] = px + (double)(oo % FVMD_WIN - FVMD_RADIUS);
        wy[q] = py + (double)(oo / FVMD_WIN - FVMD_RADIUS);
        const double t = fvmd_sample<U8>(cur, h, w, wx[q], wy[q]);
        const double ex = (fvmd_sample<U8>(cur, h, w, wx[q] + 1.0, wy[q]) - fvmd_sample<U8>(cur, h, w, wx[q] - 1.0, wy[q])) * 0.5;
        const double ey = (fvmd_sample<U8>(cur, h, w, wx[q], wy[q] + 1.0) - fvmd_sample<U8>(cur, h, w, wx[q], wy[q] - 1.0)) * 0.5;
        tpl[q] = on ? t : 0.0;
        gx[q] = on ? ex : 0.0;
        gy[q] = on ? ey : 0.0;
        sxx = sxx + gx[q] * gx[q];
        sxy = sxy + gx[q] * gy[q];
        syy = syy + gy[q] * gy[q];
    }
    sxx = fvmd_wave_sum(sxx), sxy = fvmd_wave_sum(sxy), syy = fvmd_wave_sum(syy);
    const double diff = sxx - syy;
    const double lam = 0.5 * ((sxx + syy) - sqrt(diff * diff + 4.0 * (sxy * sxy)));
    if (lam / (double)FVMD_WIN_PIXELS < FVMD_MIN_EIG) return;          // THE data branch: a singular level adds no update
    const double det = sxx * syy - sxy * sxy;
    for (int it = 0; it < FVMD_ITERS; ++it) {
        double bx = 0.0, by = 0.0;
#pragma unroll
        for (int q = 0; q < FVMD_PER_LANE; ++q) {
            const double r = tpl[q] - fvmd_sample<U8>(nxt, h, w, wx[q] + dx, wy[q] + dy);
            bx = bx + r * gx[q];
            by = by + r * gy[q];
        }
        bx = fvmd_wave_sum(bx), by = fvmd_wave_sum(by);
        dx = dx + (syy * bx - sxy * by) / det;
        dy = dy + (sxx * by - sxy * bx) / det;
    }
}

// One wave per (segment, keypoint); the wave walks its segment's S - 1 frame steps and writes tracks [B, S, 400, 2]
// (x, y).  Neighbouring waves are neighbouring points of one histogram cell (fvmd_point_of_slot).
__global__ __launch_bounds__(FVMD_THREADS) void fvmd_track_kernel(const uint8_t* __restrict__ luma, const double* __restrict__ lvl1,
                                                                  const double* __restrict__ lvl2, double* __restrict__ tracks, int h, int w,
                                                                  int seq_len, int step) {
    const int lane = threadIdx.x & (ELVIS_WAVE - 1);
    const int slot = blockIdx.x * FVMD_WAVES + (threadIdx.x >> 6);     // grid.x * 4 == 400 exactly
    const int seg = blockIdx.y;
    const int pt = fvmd_point_of_slot(slot);
    const int h1 = fvmd_level_size(h, 1), w1 = fvmd_level_size(w, 1), h2 = fvmd_level_size(h, 2), w2 = fvmd_level_size(w, 2);
    const long long n0 = (long long)h * w, n1 = (long long)h1 * w1, n2 = (long long)h2 * w2;
    double x = (((double)(pt % FVMD_GRID) + 0.5) * (double)w) / (double)FVMD_GRID - 0.5;
    double y = (((double)(pt / FVMD_GRID) + 0.5) * (double)h) / (double)FVMD_GRID - 0.5;
    double* out = tracks + ((long long)seg * seq_len * FVMD_POINTS + pt) * 2;
    if (lane == 0) out[0] = x, out[1] = y;
    for (int t = 0; t + 1 < seq_len; ++t) {
        const long long f = (long long)seg * step + t;
        double dx = 0.0, dy = 0.0;
        fvmd_level<false>(lvl2 + f * n2, lvl2 + (f + 1) * n2, h2, w2, x * 0.25, y * 0.25, dx, dy, lane);
        dx = 2.0 * dx, dy = 2.0 * dy;
        fvmd_level<false>(lvl1 + f * n1, lvl1 + (f + 1) * n1, h1, w1, x * 0.5, y * 0.5, dx, dy, lane);
        dx = 2.0 * dx, dy = 2.0 * dy;
        fvmd_level<true>(luma + f * n0, luma + (f + 1) * n0, h, w, x, y, dx, dy, lane);
        x = fmin(fmax(x + dx, 0.0), (double)(w - 1));
        y = fmin(fmax(y + dy, 0.0), (double)(h - 1));
        out += FVMD_POINTS * 2;
        if (lane == 0) out[0] = x, out[1] = y;
    }
}

// ----------------------------------------------------------------------------------------------------------- histograms
// A workgroup takes one (segment, field): the soft votes of the 400 vectors go to LDS, then lane (cell, bin) sums its
// cell's 25 points in point order.  Fields 0 .. S-2 are velocities, S-1 .. 2S-4 accelerations.
__global__ __launch_bounds__(FVMD_THREADS) void fvmd_hist_kernel(const double* __restrict__ tracks, double* __restrict__ rows, int seq_len) {
    __shared__ int bin_of[FVMD_POINTS];
    __shared__ double vote0[FVMD_POINTS], vote1[FVMD_POINTS];
    const int field = blockIdx.x, seg = blockIdx.y, nv = seq_len - 1;
    const double* tr = tracks + (long long)seg * seq_len * FVMD_POINTS * 2;
    const int stride = FVMD_POINTS * 2;
    for (int pt = threadIdx.x; pt < FVMD_POINTS; pt += FVMD_THREADS) {
        double vx, vy;
        if (field < nv) {
            const double* p = tr + (long long)field * stride + pt * 2;
            vx = p[stride] - p[0], vy = p[stride + 1] - p[1];
        } else {
            const double* p = tr + (long long)(field - nv) * stride + pt * 2;
            vx = (p[2 * stride] - p[stride]) - (p[stride] - p[0]);
            vy = (p[2 * stride + 1] - p[stride + 1]) - (p[stride + 1] - p[1]);
        }
        const double m = sqrt(vx * vx + vy * vy);
        double u = atan2(vy, vx) / FVMD_QUARTER_PI;
        if (u < 0.0) u = u + 8.0;
        const double k = floor(u), f = u - k;
        bin_of[pt] = (int)k & (FVMD_BINS - 1);
        vote0[pt] = (1.0 - f) * m;
        vote1[pt] = f * m;
    }
    __syncthreads();
    if (threadIdx.x < FVMD_FIELD_VALUES) {
        const int cell = threadIdx.x >> 3, bin = threadIdx.x & (FVMD_BINS - 1);
        double acc = 0.0;
        for (int a = 0; a < FVMD_CELL_SIDE * FVMD_CELL_SIDE; ++a) {
            const int pt = fvmd_cell_point(cell, a), k = bin_of[pt];
            acc = (acc + (k == bin ? vote0[pt] : 0.0)) + (((k + 1) & (FVMD_BINS - 1)) == bin ? vote1[pt] : 0.0);
        }
        const long long d = (long long)(2 * seq_len - 3) * FVMD_FIELD_VALUES;
        rows[(long long)seg * d + (long long)field * FVMD_FIELD_VALUES + threadIdx.x] = acc;
    }
}

// ----------------------------------------------------------------------------------------------------------- Gram
// column means of both row sets, rows summed in order: mean[which * d + col]
__global__ __launch_bounds__(FVMD_THREADS) void fvmd_mean_kernel(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ mean,
                                                                 int n, int m, int d) {
    const int col = blockIdx.x * FVMD_THREADS + threadIdx.x;
    if (col >= d) return;
    const double* src = blockIdx.y ? b : a;
    const int rows = blockIdx.y ? m : n;
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s = s + src[(long long)r * d + col];
    mean[(long long)blockIdx.y * d + col] = s / (double)rows;
}

// gram[i][j] = sum_k (a[i][k] - mean_a[k]) (b[j][k] - mean_b[k]), k ascending; 16 x 16 outputs per workgroup, the two
// centred panels of 16 columns at a time through LDS
__global__ __launch_bounds__(FVMD_THREADS) void fvmd_gram_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                                 const double* __restrict__ mean, double* __restrict__ gram, int n, int m, int d) {
    __shared__ double as[FVMD_TILE][FVMD_TILE + 1], bs[FVMD_TILE][FVMD_TILE + 1];
    const int ty = threadIdx.x / FVMD_TILE, tx = threadIdx.x % FVMD_TILE;
    const int i0 = blockIdx.y * FVMD_TILE, j0 = blockIdx.x * FVMD_TILE;
    double acc = 0.0;
    for (int k0 = 0; k0 < d; k0 += FVMD_TILE) {
        const int k = k0 + tx;
        as[ty][tx] = (i0 + ty < n && k < d) ? a[(long long)(i0 + ty) * d + k] - mean[k] : 0.0;
        bs[ty][tx] = (j0 + ty < m && k < d) ? b[(long long)(j0 + ty) * d + k] - mean[(long long)d + k] : 0.0;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < FVMD_TILE; ++kk) acc = acc + as[ty][kk] * bs[tx][kk];
        __syncthreads();
    }
    if (i0 + ty < n && j0 + tx < m) gram[(long long)(i0 + ty) * m + j0 + tx] = acc;
}

// squared norm of one centred row per workgroup: partial[r], r < n the rows of a, then those of b
__global__ __launch_bounds__(FVMD_THREADS) void fvmd_row_norm_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                                     const double* __restrict__ mean, double* __restrict__ partial, int n, int d) {
    __shared__ double red[FVMD_THREADS];
    const int r = blockIdx.x;
    const double* src = r < n ? a + (long long)r * d : b + (long long)(r - n) * d;
    const double* mu = r < n ? mean : mean + d;
    double s = 0.0;
    for (int k = threadIdx.x; k < d; k += FVMD_THREADS) {
        const double v = src[k] - mu[k];
        s = s + v * v;
    }
    s = fvmd_tree_sum(s, red);
    if (threadIdx.x == 0) partial[r] = s;
}

// scalars[0..2] = |mean_a - mean_b|^2, |A|_F^2, |Bm|_F^2 (both centred)
__global__ __launch_bounds__(FVMD_THREADS) void fvmd_scalars_kernel(const double* __restrict__ mean, const double* __restrict__ partial,
                                                                    double* __restrict__ scalars, int n, int m, int d) {
    __shared__ double red[FVMD_THREADS];
    double dm = 0.0, fa = 0.0, fb = 0.0;
    for (int k = threadIdx.x; k < d; k += FVMD_THREADS) {
        const double v = mean[k] - mean[(long long)d + k];
        dm = dm + v * v;
    }
    for (int r = threadIdx.x; r < n; r += FVMD_THREADS) fa = fa + partial[r];
    for (int r = threadIdx.x; r < m; r += FVMD_THREADS) fb = fb + partial[n + r];
    dm = fvmd_tree_sum(dm, red), fa = fvmd_tree_sum(fa, red), fb = fvmd_tree_sum(fb, red);
    if (threadIdx.x == 0) scalars[0] = dm, scalars[1] = fa, scalars[2] = fb;
}

// ----------------------------------------------------------------------------------------------------------- Jacobi
// The plane rotation of one-sided (Hestenes) Jacobi for a pair with squared norms al, be and inner product ga; false
// (skip) when |ga| <= 1e-15 sqrt(al be), which covers zero vectors.
__device__ __forceinline__ bool fvmd_rotation(double al, double be, double ga, double& c, double& s) {
    if (!(fabs(ga) > FVMD_ROT_TOL * sqrt(al * be))) return false;
    const double zeta = (be - al) / (2.0 * ga);
    const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    c = 1.0 / sqrt(1.0 + t * t);
    s = c * t;
    return true;
}

// k vectors of `len` doubles, all in LDS: FVMD_SWEEPS sweeps of K - 1 pairing rounds, a wave per pair, a workgroup barrier
// between rounds (pairs of one round are disjoint).  sv[v] = |vector v| after the sweeps.
__global__ __launch_bounds__(FVMD_THREADS) void fvmd_jacobi_lds_kernel(const double* __restrict__ vectors, double* __restrict__ sv, int k, int len) {
    extern __shared__ double mat[];
    const int lane = threadIdx.x & (ELVIS_WAVE - 1), wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < k * len; e += FVMD_THREADS) mat[e] = vectors[e];
    __syncthreads();
    const int K = (k + 1) & ~1;
    for (int sweep = 0; sweep < FVMD_SWEEPS; ++sweep) {
        for (int r = 0; r < K - 1; ++r) {
            for (int p = wave; p < K / 2; p += FVMD_WAVES) {
                int i, j;
                fvmd_pair(r, p, K, &i, &j);
                if (i >= k || j >= k) continue;
                double* x = mat + i * len;
                double* y = mat + j * len;
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int e = lane; e < len; e += ELVIS_WAVE) {
                    const double xv = x[e], yv = y[e];
                    al = al + xv * xv, be = be + yv * yv, ga = ga + xv * yv;
                }
                al = fvmd_wave_sum(al), be = fvmd_wave_sum(be), ga = fvmd_wave_sum(ga);
                double c, s;
                if (fvmd_rotation(al, be, ga, c, s)) {
                    for (int e = lane; e < len; e += ELVIS_WAVE) {
                        const double xv = x[e], yv = y[e];
                        x[e] = c * xv - s * yv;
                        y[e] = s * xv + c * yv;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int v = wave; v < k; v += FVMD_WAVES) {
        double al = 0.0;
        for (int e = lane; e < len; e += ELVIS_WAVE) al = al + mat[v * len + e] * mat[v * len + e];
        al = fvmd_wave_sum(al);
        if (lane == 0) sv[v] = sqrt(al);
    }
}

// one pairing round in global memory: a workgroup per pair, in place
__global__ __launch_bounds__(FVMD_THREADS) void fvmd_jacobi_round_kernel(double* __restrict__ vectors, int k, int len, int K, int r) {
    __shared__ double red[FVMD_THREADS];
    int i, j;
    fvmd_pair(r, blockIdx.x, K, &i, &j);
    if (i >= k || j >= k) return;                                          // the whole workgroup leaves: no barrier is skipped by a part of it
    double* x = vectors + (long long)i * len;
    double* y = vectors + (long long)j * len;
    double al = 0.0, be = 0.0, ga = 0.0;
    for (int e = threadIdx.x; e < len; e += FVMD_THREADS) {
        const double xv = x[e], yv = y[e];
        al = al + xv * xv, be = be + yv * yv, ga = ga + xv * yv;
    }
    al = fvmd_tree_sum(al, red), be = fvmd_tree_sum(be, red), ga = fvmd_tree_sum(ga, red);
    double c, s;
    if (!fvmd_rotation(al, be, ga, c, s)) return;
    for (int e = threadIdx.x; e < len; e += FVMD_THREADS) {
        const double xv = x[e], yv = y[e];
        x[e] = c * xv - s * yv;
        y[e] = s * xv + c * yv;
    }
}

__global__ __launch_bounds__(FVMD_THREADS) void fvmd_norm_kernel(const double* __restrict__ vectors, double* __restrict__ sv, int len) {
    __shared__ double red[FVMD_THREADS];
    const double* x = vectors + (long long)blockIdx.x * len;
    double al = 0.0;
    for (int e = threadIdx.x; e < len; e += FVMD_THREADS) al = al + x[e] * x[e];
    al = fvmd_tree_sum(al, red);
    if (threadIdx.x == 0) sv[blockIdx.x] = sqrt(al);
}

// out[0] = ((|dmu|^2 + |A|^2 / (n - 1)) + |Bm|^2 / (m - 1)) - 2 (sum of singular values) / sqrt((n - 1)(m - 1))
__global__ __launch_bounds__(FVMD_THREADS) void fvmd_finish_kernel(const double* __restrict__ sv, const double* __restrict__ scalars,
                                                                   double* __restrict__ out, int k, int n, int m) {
    __shared__ double red[FVMD_THREADS];
    double s = 0.0;
    for (int v = threadIdx.x; v < k; v += FVMD_THREADS) s = s + sv[v];
    s = fvmd_tree_sum(s, red);
    if (threadIdx.x == 0) {
        const double na = (double)(n - 1), nb = (double)(m - 1);
        out[0] = ((scalars[0] + scalars[1] / na) + scalars[2] / nb) - (2.0 * s) / sqrt(na * nb);
    }
}

// ----------------------------------------------------------------------------------------------------------- host
static bool fvmd_clip_ok(int frames, int h, int w) {
    return frames >= 0 && frames <= 65535 && h >= FVMD_MIN_SIDE && w >= FVMD_MIN_SIDE && (long long)h * w <= 0x3fffffffLL;
}

extern "C" size_t elvis_fvmd_pyramid_bytes(int frames, int h, int w) {
    if (!fvmd_clip_ok(frames, h, w) || frames == 0) return 0;
    const long long n1 = (long long)fvmd_level_size(h, 1) * fvmd_level_size(w, 1), n2 = (long long)fvmd_level_size(h, 2) * fvmd_level_size(w, 2);
    return (size_t)frames * (size_t)(n1 + n2) * sizeof(double);
}

extern "C" int elvis_fvmd_pyramid_f64(const uint8_t* luma, double* pyramid, int frames, int h, int w, elvis_stream_t stream) {
    ELVIS_REQUIRE(fvmd_clip_ok(frames, h, w), "elvis_fvmd_pyramid_f64: bad shape frames=%d h=%d w=%d (planes of at least %d x %d)", frames, h, w,
                  FVMD_MIN_SIDE, FVMD_MIN_SIDE);
    if (frames == 0) return ELVIS_OK;
    ELVIS_REQUIRE(luma && pyramid, "elvis_fvmd_pyramid_f64: null pointer");
    const int h1 = fvmd_level_size(h, 1), w1 = fvmd_level_size(w, 1), h2 = fvmd_level_size(h, 2), w2 = fvmd_level_size(w, 2);
    double* lvl1 = pyramid;
    double* lvl2 = pyramid + (long long)frames * h1 * w1;
    hipLaunchKernelGGL(fvmd_pyr_down_kernel<true>, dim3(cdiv((long long)h1 * w1, FVMD_THREADS), frames), dim3(FVMD_THREADS), 0, (hipStream_t)stream,
                       (const void*)luma, lvl1, h, w, h1, w1);
    ELVIS_CHECK_LAUNCH("elvis_fvmd_pyramid_f64(level 1)");
    hipLaunchKernelGGL(fvmd_pyr_down_kernel<false>, dim3(cdiv((long long)h2 * w2, FVMD_THREADS), frames), dim3(FVMD_THREADS), 0,
                       (hipStream_t)stream, (const void*)lvl1, lvl2, h1, w1, h2, w2);
    ELVIS_CHECK_LAUNCH("elvis_fvmd_pyramid_f64(level 2)");
    elvis_note_launch("fvmd_pyr_down_kernel");
    return ELVIS_OK;
}

extern "C" int elvis_fvmd_track_f64(const uint8_t* luma, const double* pyramid, double* tracks, int frames, int h, int w, int seq_len,
                                    int segment_step, elvis_stream_t stream) {
    ELVIS_REQUIRE(fvmd_clip_ok(frames, h, w), "elvis_fvmd_track_f64: bad shape frames=%d h=%d w=%d (planes of at least %d x %d)", frames, h, w,
                  FVMD_MIN_SIDE, FVMD_MIN_SIDE);
    ELVIS_REQUIRE(seq_len >= FVMD_MIN_SEQ && seq_len <= FVMD_MAX_SEQ, "elvis_fvmd_track_f64: seq_len %d outside [%d, %d]", seq_len, FVMD_MIN_SEQ,
                  FVMD_MAX_SEQ);
    ELVIS_REQUIRE(segment_step >= 1, "elvis_fvmd_track_f64: segment_step %d under 1", segment_step);
    const int segments = fvmd_segments(frames, seq_len, segment_step);
    if (segments == 0) return ELVIS_OK;
    ELVIS_REQUIRE(luma && pyramid && tracks, "elvis_fvmd_track_f64: null pointer");
    const double* lvl2 = pyramid + (long long)frames * fvmd_level_size(h, 1) * fvmd_level_size(w, 1);
    hipLaunchKernelGGL(fvmd_track_kernel, dim3(FVMD_POINTS / FVMD_WAVES, segments), dim3(FVMD_THREADS), 0, (hipStream_t)stream, luma, pyramid, lvl2,
                       tracks, h, w, seq_len, segment_step);
    ELVIS_CHECK_LAUNCH("elvis_fvmd_track_f64");
    elvis_note_launch("fvmd_track_kernel");
    return ELVIS_OK;
}

extern "C" int elvis_fvmd_features_f64(const double* tracks, double* rows, int segments, int seq_len, elvis_stream_t stream) {
    ELVIS_REQUIRE(segments >= 0 && segments <= 65535, "elvis_fvmd_features_f64: bad segment count %d", segments);
    ELVIS_REQUIRE(seq_len >= FVMD_MIN_SEQ && seq_len <= FVMD_MAX_SEQ, "elvis_fvmd_features_f64: seq_len %d outside [%d, %d]", seq_len,
                  FVMD_MIN_SEQ, FVMD_MAX_SEQ);
    if (segments == 0) return ELVIS_OK;
    ELVIS_REQUIRE(tracks && rows, "elvis_fvmd_features_f64: null pointer");
    hipLaunchKernelGGL(fvmd_hist_kernel, dim3(2 * seq_len - 3, segments), dim3(FVMD_THREADS), 0, (hipStream_t)stream, tracks, rows, seq_len);
    ELVIS_CHECK_LAUNCH("elvis_fvmd_features_f64");
    elvis_note_launch("fvmd_hist_kernel");
    return ELVIS_OK;
}

static bool fvmd_rows_ok(int n, int m, int d) { return n >= 2 && m >= 2 && n <= FVMD_MAX_ROWS && m <= FVMD_MAX_ROWS && d >= 1 && d <= (1 << 20); }

extern "C" size_t elvis_fvmd_gram_workspace_bytes(int n, int m, int d) {
    return fvmd_rows_ok(n, m, d) ? (size_t)(2LL * d + n + m) * sizeof(double) : 0;
}

extern "C" int elvis_fvmd_gram_f64(const double* a, const double* b, double* workspace, double* gram, double* scalars, int n, int m, int d,
                                   elvis_stream_t stream) {
    ELVIS_REQUIRE(fvmd_rows_ok(n, m, d), "elvis_fvmd_gram_f64: bad shape n=%d m=%d d=%d (2 <= n, m <= %d rows)", n, m, d, FVMD_MAX_ROWS);
    ELVIS_REQUIRE(a && b && workspace && gram && scalars, "elvis_fvmd_gram_f64: null pointer");
    hipStream_t s = (hipStream_t)stream;
    double* mean = workspace;
    double* partial = workspace + 2LL * d;
    hipLaunchKernelGGL(fvmd_mean_kernel, dim3(cdiv(d, FVMD_THREADS), 2), dim3(FVMD_THREADS), 0, s, a, b, mean, n, m, d);
    ELVIS_CHECK_LAUNCH("elvis_fvmd_gram_f64(mean)");
    hipLaunchKernelGGL(fvmd_gram_kernel, dim3(cdiv(m, FVMD_TILE), cdiv(n, FVMD_TILE)), dim3(FVMD_THREADS), 0, s, a, b, (const double*)mean, gram, n,
                       m, d);
    ELVIS_CHECK_LAUNCH("elvis_fvmd_gram_f64(gram)");
    hipLaunchKernelGGL(fvmd_row_norm_kernel, dim3(n + m), dim3(FVMD_THREADS), 0, s, a, b, (const double*)mean, partial, n, d);
    ELVIS_CHECK_LAUNCH("elvis_fvmd_gram_f64(row norms)");
    hipLaunchKernelGGL(fvmd_scalars_kernel, dim3(1), dim3(FVMD_THREADS), 0, s, (const double*)mean, (const double*)partial, scalars, n, m, d);
    ELVIS_CHECK_LAUNCH("elvis_fvmd_gram_f64(scalars)");
    elvis_note_launch("fvmd_gram_kernel");
    return ELVIS_OK;
}

extern "C" int elvis_fvmd_singular_values_f64(double* vectors, double* sv, int k, int len, elvis_stream_t stream) {
    ELVIS_REQUIRE(k >= 1 && len >= 1 && k <= FVMD_MAX_ROWS && len <= FVMD_MAX_ROWS, "elvis_fvmd_singular_values_f64: bad shape k=%d len=%d (at most %d)",
                  k, len, FVMD_MAX_ROWS);
    ELVIS_REQUIRE(vectors && sv, "elvis_fvmd_singular_values_f64: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if ((long long)k * len <= FVMD_LDS_DOUBLES) {
        static ElvisLdsOptIn opt_in;
        const int rc = elvis_lds_opt_in((const void*)fvmd_jacobi_lds_kernel, opt_in, elvis_device_slot(), "elvis_fvmd_singular_values_f64: LDS opt-in");
        if (rc != ELVIS_OK) return rc;
        hipLaunchKernelGGL(fvmd_jacobi_lds_kernel, dim3(1), dim3(FVMD_THREADS), (size_t)k * len * sizeof(double), s, (const double*)vectors, sv, k,
                           len);
        ELVIS_CHECK_LAUNCH("elvis_fvmd_singular_values_f64(lds)");
        elvis_note_launch("fvmd_jacobi_lds_kernel");
        return ELVIS_OK;
    }
    const int K = (k + 1) & ~1;
    for (int sweep = 0; sweep < FVMD_SWEEPS; ++sweep)
        for (int r = 0; r < K - 1; ++r) hipLaunchKernelGGL(fvmd_jacobi_round_kernel, dim3(K / 2), dim3(FVMD_THREADS), 0, s, vectors, k, len, K, r);
    ELVIS_CHECK_LAUNCH("elvis_fvmd_singular_values_f64(rounds)");
    hipLaunchKernelGGL(fvmd_norm_kernel, dim3(k), dim3(FVMD_THREADS), 0, s, (const double*)vectors, sv, len);
    ELVIS_CHECK_LAUNCH("elvis_fvmd_singular_values_f64(norms)");
    elvis_note_launch("fvmd_jacobi_round_kernel");
    return ELVIS_OK;
}

extern "C" int elvis_fvmd_finish_f64(const double* sv, const double* scalars, double* out, int k, int n, int m, elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 2 && m >= 2 && n <= FVMD_MAX_ROWS && m <= FVMD_MAX_ROWS && k >= 1 && k <= FVMD_MAX_ROWS,
                  "elvis_fvmd_finish_f64: bad shape k=%d n=%d m=%d", k, n, m);
    ELVIS_REQUIRE(sv && scalars && out, "elvis_fvmd_finish_f64: null pointer");
    hipLaunchKernelGGL(fvmd_finish_kernel, dim3(1), dim3(FVMD_THREADS), 0, (hipStream_t)stream, sv, scalars, out, k, n, m);
    ELVIS_CHECK_LAUNCH("elvis_fvmd_finish_f64");
    elvis_note_launch("fvmd_finish_kernel");
    return ELVIS_OK;
}
