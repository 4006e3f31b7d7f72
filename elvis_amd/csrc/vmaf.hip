// VMAF of the evaluation report on the device: the VIF (4 scales), ADM2 (4 scales) and motion2 features of a pair of
// 8-bit luma clips and the nu-SVR score over them.  The reference writes both clips to disk and starts the vmaf binary
// in a subprocess (elvis.py:3197-3356, presley.py:262-326); neither libvmaf nor its model file is available to this
// build, so this is a BUILD-DEFINED restatement of the published float feature extractors, stated as a contract in
// include/elvis_amd.h and DESIGN.md 7 and in numpy float64 in tests/_vmaf_ref.py.  It does not claim libvmaf's numbers.
//
// All arithmetic is float64 on luma less 128.  Every per-pixel quantity is evaluated in the one order the contract
// states - a filter is ((f0 x0 + f1 x1) + f2 x2) + ... in ascending tap order, the vertical pass first - and the library
// is built without FMA contraction, so every branch falls as it does in the numpy statement; only log2, cbrt, exp and
// the order of the big sums differ.  The filters and constants come from the host (`tables`, VT_* below), so no device
// exp / cos takes part in them.  No atomics; every reduction has a fixed order: two runs give the same bytes, and a
// frame's features do not depend on how many frames a call is given.
#include "common.h"
#include "i420.h"

#define VMAF_THREADS 256
#define VMAF_SCALES 4
#define VMAF_MIN_SIDE 64
#define VMAF_PASS_FRAMES 4       // frames whose pyramids are resident at once; the workspace is sized for that many
#define VMAF_TH 16               // the tile of the filter kernels (VIF statistic, motion): 16 rows x 32 columns
#define VMAF_TW 32
#define VMAF_AT 16               // the tile of the ADM pooling kernel: 16 x 16, one pixel per lane

// the host's table of float64 constants (elvis_amd/vmaf.py `vmaf_tables`)
enum { VT_G17 = 0, VT_G9 = 17, VT_G5 = 26, VT_G3 = 31, VT_BLUR = 34, VT_LO = 39, VT_HI = 43, VT_COS2 = 47, VT_CSF = 48, VT_COUNT = 56 };

// model array of elvis_vmaf_predict_f64
enum { VM_SLOPES = 0, VM_INTERCEPTS = 7, VM_RHO = 14, VM_GAMMA = 15, VM_CLIP = 16, VM_TRANSFORM = 18, VM_SV = 21 };

struct VmafPlan {
    int h, w, n, has_next;
    int vh[VMAF_SCALES], vw[VMAF_SCALES], vtiles[VMAF_SCALES];       // VIF plane sizes and statistic tiles per scale
    int ah[VMAF_SCALES], aw[VMAF_SCALES], atiles[VMAF_SCALES];       // ADM band sizes and pooling tiles per scale
    int left[VMAF_SCALES], top[VMAF_SCALES];                         // the central window of a band: [top, ah - top) x [left, aw - left)
    int mtiles;
    long long voff[VMAF_SCALES], aoff[VMAF_SCALES], per_frame;       // doubles: a frame's partials
    long long plane_off[VMAF_SCALES], band_off[VMAF_SCALES];         // doubles: the pass buffers (plane_off[0] unused)
    long long motion_off, partial_off, total;                        // doubles: the workspace
};

static bool vmaf_plan(int n, int h, int w, int has_next, VmafPlan& p) {
    if (n <= 0 || h < VMAF_MIN_SIDE || w < VMAF_MIN_SIDE || n > 65535 - 1) return false;
    if ((long long)h * w > 0x3fffffffLL) return false;
    p.h = h, p.w = w, p.n = n, p.has_next = has_next;
    const long long pass = n < VMAF_PASS_FRAMES ? n : VMAF_PASS_FRAMES;
    long long at = 0, part = 0;
    int ih = h, iw = w;
    for (int s = 0; s < VMAF_SCALES; ++s) {
        p.vh[s] = s ? p.vh[s - 1] / 2 : h;
        p.vw[s] = s ? p.vw[s - 1] / 2 : w;
        p.vtiles[s] = cdiv(p.vh[s], VMAF_TH) * cdiv(p.vw[s], VMAF_TW);
        p.voff[s] = part;
        part += 2LL * p.vtiles[s];
        p.plane_off[s] = at;
        if (s) at += pass * 2 * p.vh[s] * p.vw[s];
    }
    for (int s = 0; s < VMAF_SCALES; ++s) {
        p.ah[s] = (ih + 1) / 2;
        p.aw[s] = (iw + 1) / 2;
        ih = p.ah[s], iw = p.aw[s];
        p.atiles[s] = cdiv(p.ah[s], VMAF_AT) * cdiv(p.aw[s], VMAF_AT);
        p.aoff[s] = part;
        part += 6LL * p.atiles[s];
        p.band_off[s] = at;
        at += pass * 8 * p.ah[s] * p.aw[s];
        const int l = (int)(p.aw[s] * 0.1 - 0.5), t = (int)(p.ah[s] * 0.1 - 0.5);
        p.left[s] = l > 0 ? l : 0;
        p.top[s] = t > 0 ? t : 0;
    }
    p.per_frame = part;
    p.mtiles = cdiv(h, VMAF_TH) * cdiv(w, VMAF_TW);
    p.motion_off = at;
    at += (long long)(n + 1) * p.mtiles;
    p.partial_off = at;
    at += (long long)n * p.per_frame;
    p.total = at;
    return true;
}

// mirror without repeating the edge, one fold at each end; |i| < n and i <= 2n - 2 wherever a value is used
__device__ __forceinline__ int vmaf_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}
// the same, held inside the plane: the halo of a ragged tile reaches past one fold, and what it reads there is not used
__device__ __forceinline__ int vmaf_reflect_in(int i, int n) { return min(max(vmaf_reflect(i, n), 0), n - 1); }

template <bool U8>
__device__ __forceinline__ double vmaf_load(const void* p, long long i) {
    if constexpr (U8) return (double)((int)reinterpret_cast<const uint8_t*>(p)[i] - 128);
    else return reinterpret_cast<const double*>(p)[i];
}

// sum of the workgroup's 256 values in a fixed tree; `red` is 256 doubles of LDS
__device__ __forceinline__ double vmaf_tree_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int o = VMAF_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    const double total = red[0];
    __syncthreads();
    return total;
}

// ----------------------------------------------------------------------------------------------------------- luma
// RGB / BGR [n,h,w,3] -> the luma the encoder is handed (i420_y), of the rectangle [y0, y1) x [x0, x1); where a mask is
// given and says so, the pixel's three bytes count as 0 (elvis.py:615-624), which is luma 16.
__global__ __launch_bounds__(VMAF_THREADS) void vmaf_luma_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ masks,
                                                                 uint8_t* __restrict__ out, int h, int w, int order, int invert, int y0,
                                                                 int x0, int rh, int rw) {
    const long long i = (long long)blockIdx.x * VMAF_THREADS + threadIdx.x;
    if (i >= (long long)rh * rw) return;
    const int f = blockIdx.y, y = y0 + (int)(i / rw), x = x0 + (int)(i % rw);
    const long long px = ((long long)f * h + y) * w + x;
    int r = frames[px * 3 + (order ? 2 : 0)], g = frames[px * 3 + 1], b = frames[px * 3 + (order ? 0 : 2)];
    if (masks && ((masks[px] != 0) == (invert != 0))) r = g = b = 0;
    out[(long long)f * rh * rw + i] = i420_y(r, g, b);
}

// ----------------------------------------------------------------------------------------------------------- VIF
// Filter and decimate: out[i][j] = G_N(plane)[2i][2j], both planes of every frame of the pass.  A lane takes one output
// pixel: the vertical pass of its N columns, then the horizontal pass over them - the separable filter's own order.
// N = 9 reads the 8-bit planes (scale 1), N = 5 and 3 the float64 planes of the scale before.
template <int N>
__global__ __launch_bounds__(VMAF_THREADS) void vmaf_vif_down_kernel(const void* __restrict__ ref, const void* __restrict__ dis,
                                                                     long long in_stride, const double* __restrict__ filter,
                                                                     double* __restrict__ out, int h, int w, int ho, int wo) {
    constexpr bool U8 = N == 9;
    constexpr int R = N / 2;
    const long long i = (long long)blockIdx.x * VMAF_THREADS + threadIdx.x;
    if (i >= (long long)ho * wo) return;
    const int f = blockIdx.y, plane = blockIdx.z, oy = (int)(i / wo), ox = (int)(i % wo);
    const void* src = plane ? dis : ref;
    const long long base = (long long)f * in_stride;
    double fl[N];
#pragma unroll
    for (int k = 0; k < N; ++k) fl[k] = filter[k];
    int rows[N];
#pragma unroll
    for (int k = 0; k < N; ++k) rows[k] = vmaf_reflect(2 * oy - R + k, h);
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int col = vmaf_reflect(2 * ox - R + c, w);
        double v = fl[0] * vmaf_load<U8>(src, base + (long long)rows[0] * w + col);
#pragma unroll
        for (int k = 1; k < N; ++k) v = v + fl[k] * vmaf_load<U8>(src, base + (long long)rows[k] * w + col);
        acc = c ? acc + fl[c] * v : fl[0] * v;
    }
    out[((long long)f * 2 + plane) * ho * wo + i] = acc;
}

// The statistic of one scale.  A workgroup takes a 16 x 32 tile: the two planes with their halo go to LDS, the vertical
// pass of the five moment planes (x, y, x x, y y, x y) goes to LDS, the horizontal pass and the statistic follow per
// pixel, and ONE (num, den) pair leaves per tile - each lane adds its two pixels in index order, then the fixed tree.
// LDS for N = 17: 2 x 32 x 48 + 5 x 16 x 48 + 256 doubles = 57 KiB, two workgroups per CU.
template <int N>
__global__ __launch_bounds__(VMAF_THREADS) void vmaf_vif_stat_kernel(const void* __restrict__ ref, const void* __restrict__ dis,
                                                                     long long in_stride, const double* __restrict__ filter,
                                                                     double* __restrict__ partial, long long partial_stride, int h, int w,
                                                                     int tiles_x) {
    constexpr bool U8 = N == 17;
    constexpr int R = N / 2, IH = VMAF_TH + N - 1, IW = VMAF_TW + N - 1;
    __shared__ double sx[IH * IW], sy[IH * IW];
    __shared__ double sv[5][VMAF_TH * IW];
    __shared__ double red[VMAF_THREADS];
    __shared__ double sf[N];
    const int t = threadIdx.x, f = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * VMAF_TH, tx0 = (blockIdx.x % tiles_x) * VMAF_TW;
    const long long base = (long long)f * in_stride;
    if (t < N) sf[t] = filter[t];
    for (int i = t; i < IH * IW; i += VMAF_THREADS) {
        const int gy = vmaf_reflect_in(ty0 - R + i / IW, h), gx = vmaf_reflect_in(tx0 - R + i % IW, w);
        sx[i] = vmaf_load<U8>(ref, base + (long long)gy * w + gx);
        sy[i] = vmaf_load<U8>(dis, base + (long long)gy * w + gx);
    }
    __syncthreads();
    for (int i = t; i < VMAF_TH * IW; i += VMAF_THREADS) {
        const int ly = i / IW, lx = i % IW;
        double a[5];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double x = sx[(ly + k) * IW + lx], y = sy[(ly + k) * IW + lx], c = sf[k];
            const double m[5] = {x, y, x * x, y * y, x * y};
#pragma unroll
            for (int q = 0; q < 5; ++q) a[q] = k ? a[q] + c * m[q] : c * m[q];
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) sv[q][i] = a[q];
    }
    __syncthreads();
    const double eps = 1e-10, nsq = 2.0;
    double num = 0.0, den = 0.0;
    for (int p = t; p < VMAF_TH * VMAF_TW; p += VMAF_THREADS) {
        const int oy = p / VMAF_TW, ox = p % VMAF_TW;
        if (ty0 + oy >= h || tx0 + ox >= w) continue;
        double a[5];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double c = sf[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const double v = sv[q][oy * IW + ox + k];
                a[q] = k ? a[q] + c * v : c * v;
            }
        }
        const double mu1 = a[0], mu2 = a[1];
        double s1 = fmax(a[2] - mu1 * mu1, 0.0);
        const double s2 = fmax(a[3] - mu2 * mu2, 0.0);
        const double s12 = a[4] - mu1 * mu2;
        double g = s12 / (s1 + eps);
        double sw = s2 - g * s12;
        if (s1 < eps) g = 0.0, sw = s2, s1 = 0.0;
        if (s2 < eps) g = 0.0, sw = 0.0;
        if (g < 0.0) sw = s2, g = 0.0;
        sw = fmax(sw, eps);
        g = fmin(g, 100.0);
        if (s1 >= nsq) {
            num += log2(1.0 + ((g * g) * s1) / (sw + nsq));
            den += log2(1.0 + s1 / nsq);
        } else {
            num += 1.0 - (s2 * 4.0) / 65025.0;
            den += 1.0;
        }
    }
    num = vmaf_tree_sum(num, red);
    den = vmaf_tree_sum(den, red);
    if (t == 0) {
        double* out = partial + (long long)f * partial_stride + 2LL * blockIdx.x;
        out[0] = num;
        out[1] = den;
    }
}

// ----------------------------------------------------------------------------------------------------------- ADM
// One db2 analysis step on both planes of every frame of the pass: out[i] = sum_k f[k] x[2i + k - 1], vertical then
// horizontal, four bands each - 0 a = (lo, lo), 1 h = (hi, lo), 2 v = (lo, hi), 3 d = (hi, hi), (vertical, horizontal).
// A lane takes one output pixel of all four bands from its 4 x 4 inputs.  Scale 0 reads the 8-bit planes, the others
// the `a` bands of the scale before.
template <bool U8>
__global__ __launch_bounds__(VMAF_THREADS) void vmaf_dwt_kernel(const void* __restrict__ ref, const void* __restrict__ dis, long long in_stride,
                                                                const double* __restrict__ tables, double* __restrict__ bands, int h, int w,
                                                                int bh, int bw) {
    const long long i = (long long)blockIdx.x * VMAF_THREADS + threadIdx.x;
    if (i >= (long long)bh * bw) return;
    const int f = blockIdx.y, plane = blockIdx.z, oy = (int)(i / bw), ox = (int)(i % bw);
    const void* src = plane ? dis : ref;
    const long long base = (long long)f * in_stride;
    double lo[4], hi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) lo[k] = tables[VT_LO + k], hi[k] = tables[VT_HI + k];
    int rows[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) rows[k] = vmaf_reflect(2 * oy + k - 1, h);
    double vl[4], vh[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int col = vmaf_reflect(2 * ox + c - 1, w);
        double x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = vmaf_load<U8>(src, base + (long long)rows[k] * w + col);
        vl[c] = ((lo[0] * x[0] + lo[1] * x[1]) + lo[2] * x[2]) + lo[3] * x[3];
        vh[c] = ((hi[0] * x[0] + hi[1] * x[1]) + hi[2] * x[2]) + hi[3] * x[3];
    }
    double* out = bands + ((long long)f * 2 + plane) * 4 * bh * bw + i;
    const long long size = (long long)bh * bw;
    out[0] = ((lo[0] * vl[0] + lo[1] * vl[1]) + lo[2] * vl[2]) + lo[3] * vl[3];
    out[size] = ((lo[0] * vh[0] + lo[1] * vh[1]) + lo[2] * vh[2]) + lo[3] * vh[3];
    out[2 * size] = ((hi[0] * vl[0] + hi[1] * vl[1]) + hi[2] * vl[2]) + hi[3] * vl[3];
    out[3 * size] = ((hi[0] * vh[0] + hi[1] * vh[1]) + hi[2] * vh[2]) + hi[3] * vh[3];
}

// the decoupling of one pixel: o, t are the reference's and the distorted plane's (h, v, d); r the restored, a the
// additive part
__device__ __forceinline__ void vmaf_decouple(const double* o, const double* t, double cos2, double* r, double* a) {
    const double dp = o[0] * t[0] + o[1] * t[1];
    const double om = o[0] * o[0] + o[1] * o[1], tm = t[0] * t[0] + t[1] * t[1];
    const bool flag = dp >= 0.0 && dp * dp >= (cos2 * om) * tm;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const double k = fmin(fmax(t[b] / (o[b] + 1e-30), 0.0), 1.0);
        r[b] = flag ? t[b] : k * o[b];
        a[b] = t[b] - r[b];
    }
}

// Decouple, contrast sensitivity, the 3 x 3 masking threshold and the cubes of one scale.  A workgroup takes a 16 x 16
// tile, one pixel per lane; |csf a| of the three bands goes to an LDS tile with a one-pixel, edge-clamped halo.  Six
// partials leave per tile: the restored cubes of h, v, d, then the reference's.
__global__ __launch_bounds__(VMAF_THREADS) void vmaf_adm_pool_kernel(const double* __restrict__ bands, const double* __restrict__ tables,
                                                                     double* __restrict__ partial, long long partial_stride, int scale, int bh,
                                                                     int bw, int tiles_x, int left, int top) {
    constexpr int LW = VMAF_AT + 2;
    __shared__ double sa[3][LW * LW];
    __shared__ double red[VMAF_THREADS];
    const int t = threadIdx.x, f = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * VMAF_AT, tx0 = (blockIdx.x % tiles_x) * VMAF_AT;
    const long long size = (long long)bh * bw;
    const double* ob = bands + (long long)f * 8 * size;       // reference a, h, v, d, then the distorted plane's
    const double* tb = ob + 4 * size;
    const double cos2 = tables[VT_COS2];
    const double rf[3] = {tables[VT_CSF + 2 * scale], tables[VT_CSF + 2 * scale], tables[VT_CSF + 2 * scale + 1]};
    for (int i = t; i < LW * LW; i += VMAF_THREADS) {
        const int gy = min(max(ty0 - 1 + i / LW, 0), bh - 1), gx = min(max(tx0 - 1 + i % LW, 0), bw - 1);
        const long long at = (long long)gy * bw + gx;
        double o[3], d[3], r[3], a[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) o[b] = ob[(b + 1) * size + at], d[b] = tb[(b + 1) * size + at];
        vmaf_decouple(o, d, cos2, r, a);
#pragma unroll
        for (int b = 0; b < 3; ++b) sa[b][i] = fabs(rf[b] * a[b]);
    }
    __syncthreads();
    const int ly = t / VMAF_AT, lx = t % VMAF_AT, y = ty0 + ly, x = tx0 + lx;
    double cube[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (y >= top && y < bh - top && x >= left && x < bw - left) {
        const long long at = (long long)y * bw + x;
        double o[3], d[3], r[3], a[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) o[b] = ob[(b + 1) * size + at], d[b] = tb[(b + 1) * size + at];
        vmaf_decouple(o, d, cos2, r, a);
        double thr = 0.0;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            double s = 0.0;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) s = s + sa[b][(ly + dy) * LW + lx + dx];
            s = s + sa[b][(ly + 1) * LW + lx + 1];
            thr = thr + s;
        }
        thr = thr / 30.0;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double v = fmax(fabs(rf[b] * r[b]) - thr, 0.0), u = fabs(rf[b] * o[b]);
            cube[b] = (v * v) * v;
            cube[3 + b] = (u * u) * u;
        }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double total = vmaf_tree_sum(cube[q], red);
        if (t == 0) partial[(long long)f * partial_stride + 6LL * blockIdx.x + q] = total;
    }
}

// ----------------------------------------------------------------------------------------------------------- motion
// sum |B(cur) - B(prv)| over a 16 x 32 tile, B the 5-tap blur: both tiles with their halo in LDS, the vertical pass of
// both in LDS, then the horizontal pass and the difference per pixel; one partial per tile.  Frame f of the launch is
// ref[f] against ref[f - 1]; frame 0 against `prev` (without one its partials are 0) and frame n, where the launch has
// one, `next` against ref[n - 1].
__global__ __launch_bounds__(VMAF_THREADS) void vmaf_motion_kernel(const uint8_t* __restrict__ ref, const uint8_t* __restrict__ prev,
                                                                   const uint8_t* __restrict__ next, const double* __restrict__ tables,
                                                                   double* __restrict__ partial, int n, int h, int w, int tiles_x) {
    constexpr int N = 5, R = 2, IH = VMAF_TH + N - 1, IW = VMAF_TW + N - 1;
    __shared__ double sc[IH * IW], sp[IH * IW];
    __shared__ double vc[VMAF_TH * IW], vp[VMAF_TH * IW];
    __shared__ double red[VMAF_THREADS];
    const int t = threadIdx.x, f = blockIdx.y;
    const long long size = (long long)h * w;
    const uint8_t* cur = f < n ? ref + f * size : next;
    const uint8_t* prv = f == 0 ? prev : ref + (f - 1) * size;
    double* out = partial + (long long)f * gridDim.x + blockIdx.x;
    if (prv == nullptr) {                                        // uniform over the workgroup
        if (t == 0) *out = 0.0;
        return;
    }
    const int ty0 = (blockIdx.x / tiles_x) * VMAF_TH, tx0 = (blockIdx.x % tiles_x) * VMAF_TW;
    double fl[N];
#pragma unroll
    for (int k = 0; k < N; ++k) fl[k] = tables[VT_BLUR + k];
    for (int i = t; i < IH * IW; i += VMAF_THREADS) {
        const int gy = vmaf_reflect_in(ty0 - R + i / IW, h), gx = vmaf_reflect_in(tx0 - R + i % IW, w);
        sc[i] = vmaf_load<true>(cur, (long long)gy * w + gx);
        sp[i] = vmaf_load<true>(prv, (long long)gy * w + gx);
    }
    __syncthreads();
    for (int i = t; i < VMAF_TH * IW; i += VMAF_THREADS) {
        const int ly = i / IW, lx = i % IW;
        double a = fl[0] * sc[ly * IW + lx], b = fl[0] * sp[ly * IW + lx];
#pragma unroll
        for (int k = 1; k < N; ++k) {
            a = a + fl[k] * sc[(ly + k) * IW + lx];
            b = b + fl[k] * sp[(ly + k) * IW + lx];
        }
        vc[i] = a, vp[i] = b;
    }
    __syncthreads();
    double sum = 0.0;
    for (int p = t; p < VMAF_TH * VMAF_TW; p += VMAF_THREADS) {
        const int oy = p / VMAF_TW, ox = p % VMAF_TW;
        if (ty0 + oy >= h || tx0 + ox >= w) continue;
        double a = fl[0] * vc[oy * IW + ox], b = fl[0] * vp[oy * IW + ox];
#pragma unroll
        for (int k = 1; k < N; ++k) {
            a = a + fl[k] * vc[oy * IW + ox + k];
            b = b + fl[k] * vp[oy * IW + ox + k];
        }
        sum += fabs(a - b);
    }
    sum = vmaf_tree_sum(sum, red);
    if (t == 0) *out = sum;
}

// ----------------------------------------------------------------------------------------------------------- finish
// sum of `count` partials `stride` apart: lane t adds partials t, t + 256, ... in that order, then the fixed tree
__device__ __forceinline__ double vmaf_partial_sum(const double* p, int count, int stride, double* red) {
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += VMAF_THREADS) s += p[(long long)i * stride];
    return vmaf_tree_sum(s, red);
}

// One workgroup per frame: the tile partials to the six features adm2, motion2, vif_scale0..3.
__global__ __launch_bounds__(VMAF_THREADS) void vmaf_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, VmafPlan p) {
    __shared__ double red[VMAF_THREADS];
    const int f = blockIdx.x;
    const double* part = ws + p.partial_off + (long long)f * p.per_frame;
    double feat[6];
    double anum = 0.0, aden = 0.0;
    for (int s = 0; s < VMAF_SCALES; ++s) {
        const double area = (double)(p.aw[s] - 2 * p.left[s]) * (double)(p.ah[s] - 2 * p.top[s]);
        const double floor_term = cbrt(area / 32.0);
        for (int q = 0; q < 6; ++q) {
            const double total = vmaf_partial_sum(part + p.aoff[s] + q, p.atiles[s], 6, red);
            (q < 3 ? anum : aden) += cbrt(total) + floor_term;
        }
    }
    feat[0] = anum / aden;
    const double pixels = (double)p.h * (double)p.w;
    const double m0 = vmaf_partial_sum(ws + p.motion_off + (long long)f * p.mtiles, p.mtiles, 1, red) / pixels;
    feat[1] = m0;
    if (f + 1 < p.n + p.has_next) {
        const double m1 = vmaf_partial_sum(ws + p.motion_off + (long long)(f + 1) * p.mtiles, p.mtiles, 1, red) / pixels;
        feat[1] = fmin(m0, m1);
    }
    for (int s = 0; s < VMAF_SCALES; ++s) {
        const double num = vmaf_partial_sum(part + p.voff[s], p.vtiles[s], 2, red);
        const double den = vmaf_partial_sum(part + p.voff[s] + 1, p.vtiles[s], 2, red);
        feat[2 + s] = den == 0.0 ? 1.0 : num / den;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) out[(long long)f * 6 + q] = feat[q];
    }
}

// ----------------------------------------------------------------------------------------------------------- score
// One wave per frame: lane l takes support vectors l, l + 64, ... in that order, the 64 sums meet in a fixed butterfly,
// lane 0 finishes the score.
__global__ __launch_bounds__(VMAF_THREADS) void vmaf_predict_kernel(const double* __restrict__ feats, const double* __restrict__ model,
                                                                    double* __restrict__ out, int n, int nsv, int flags) {
    const int lane = threadIdx.x % ELVIS_WAVE, f = blockIdx.x * (VMAF_THREADS / ELVIS_WAVE) + threadIdx.x / ELVIS_WAVE;
    if (f >= n) return;                                          // whole waves leave; no barrier follows
    double x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = model[VM_SLOPES + 1 + i] * feats[(long long)f * 6 + i] + model[VM_INTERCEPTS + 1 + i];
    const double gamma = model[VM_GAMMA];
    const double* sv = model + VM_SV;
    const double* coef = sv + 6LL * nsv;
    double acc = 0.0;
    for (int j = lane; j < nsv; j += ELVIS_WAVE) {
        double d2 = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double d = sv[6LL * j + i] - x[i];
            d2 = d2 + d * d;
        }
        acc += coef[j] * exp(-(gamma * d2));
    }
#pragma unroll
    for (int o = ELVIS_WAVE / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, ELVIS_WAVE);
    if (lane == 0) {
        double s = ((acc - model[VM_RHO]) - model[VM_INTERCEPTS]) / model[VM_SLOPES];
        if (flags & 1) {
            const double tr = (model[VM_TRANSFORM] + model[VM_TRANSFORM + 1] * s) + (model[VM_TRANSFORM + 2] * s) * s;
            s = (flags & 2) ? fmax(tr, s) : tr;
        }
        if (flags & 4) s = fmin(fmax(s, model[VM_CLIP]), model[VM_CLIP + 1]);
        out[f] = s;
    }
}

// ----------------------------------------------------------------------------------------------------------- host
extern "C" int elvis_vmaf_luma_u8(const uint8_t* frames, const uint8_t* masks, uint8_t* out, int n, int h, int w, int order, int invert,
                                  int y0, int y1, int x0, int x1, elvis_stream_t stream) {
    ELVIS_REQUIRE(order == 0 || order == 1, "elvis_vmaf_luma_u8: order must be 0 (rgb) or 1 (bgr), got %d", order);
    ELVIS_REQUIRE(n >= 0 && n <= 65535 && h > 0 && w > 0 && (long long)h * w <= 0x3fffffffLL, "elvis_vmaf_luma_u8: bad shape n=%d h=%d w=%d",
                  n, h, w);
    ELVIS_REQUIRE(y0 >= 0 && x0 >= 0 && y1 <= h && x1 <= w && y0 < y1 && x0 < x1,
                  "elvis_vmaf_luma_u8: rectangle [%d, %d) x [%d, %d) does not lie inside the %d x %d frame", y0, y1, x0, x1, h, w);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(frames && out, "elvis_vmaf_luma_u8: null pointer");
    const int rh = y1 - y0, rw = x1 - x0;
    hipLaunchKernelGGL(vmaf_luma_kernel, dim3(cdiv((long long)rh * rw, VMAF_THREADS), n), dim3(VMAF_THREADS), 0, (hipStream_t)stream, frames,
                       masks, out, h, w, order, invert ? 1 : 0, y0, x0, rh, rw);
    ELVIS_CHECK_LAUNCH("elvis_vmaf_luma_u8");
    elvis_note_launch("vmaf_luma_kernel");
    return ELVIS_OK;
}

extern "C" size_t elvis_vmaf_workspace_bytes(int n, int h, int w) {
    VmafPlan p;
    return vmaf_plan(n, h, w, 1, p) ? (size_t)p.total * sizeof(double) : 0;
}

template <int N>
static int vmaf_vif_scale(const VmafPlan& p, int s, int k, const void* ref, const void* dis, long long in_stride, const double* filter,
                          double* partial, hipStream_t stream) {
    hipLaunchKernelGGL(vmaf_vif_stat_kernel<N>, dim3(p.vtiles[s], k), dim3(VMAF_THREADS), 0, stream, ref, dis, in_stride, filter, partial,
                       p.per_frame, p.vh[s], p.vw[s], cdiv(p.vw[s], VMAF_TW));
    ELVIS_CHECK_LAUNCH("elvis_vmaf_features_f64(vif)");
    return ELVIS_OK;
}

template <int N>
static int vmaf_vif_down(const VmafPlan& p, int s, int k, const void* ref, const void* dis, long long in_stride, const double* filter,
                         double* out, hipStream_t stream) {
    hipLaunchKernelGGL(vmaf_vif_down_kernel<N>, dim3(cdiv((long long)p.vh[s] * p.vw[s], VMAF_THREADS), k, 2), dim3(VMAF_THREADS), 0, stream,
                       ref, dis, in_stride, filter, out, p.vh[s - 1], p.vw[s - 1], p.vh[s], p.vw[s]);
    ELVIS_CHECK_LAUNCH("elvis_vmaf_features_f64(down)");
    return ELVIS_OK;
}

extern "C" int elvis_vmaf_features_f64(const uint8_t* ref, const uint8_t* dis, const uint8_t* prev, const uint8_t* next,
                                       const double* tables, double* workspace, double* out, int n, int h, int w, elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 0 && n < 65535, "elvis_vmaf_features_f64: bad frame count n=%d", n);
    ELVIS_REQUIRE(h >= VMAF_MIN_SIDE && w >= VMAF_MIN_SIDE, "elvis_vmaf_features_f64: a %d x %d plane is smaller than %d x %d", h, w,
                  VMAF_MIN_SIDE, VMAF_MIN_SIDE);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(ref && dis && tables && workspace && out, "elvis_vmaf_features_f64: null pointer");
    VmafPlan p;
    ELVIS_REQUIRE(vmaf_plan(n, h, w, next ? 1 : 0, p), "elvis_vmaf_features_f64: n=%d h=%d w=%d is more than one call holds", n, h, w);
    hipStream_t s = (hipStream_t)stream;
    const long long size = (long long)h * w;
    int rc;
    for (int f0 = 0; f0 < n; f0 += VMAF_PASS_FRAMES) {
        const int k = n - f0 < VMAF_PASS_FRAMES ? n - f0 : VMAF_PASS_FRAMES;
        const uint8_t *r0 = ref + f0 * size, *d0 = dis + f0 * size;
        double* part = workspace + p.partial_off + (long long)f0 * p.per_frame;
        // VIF: the statistic of scale 0 from the bytes, then decimate and take the statistic, three times
        if ((rc = vmaf_vif_scale<17>(p, 0, k, r0, d0, size, tables + VT_G17, part + p.voff[0], s))) return rc;
        double* pl[VMAF_SCALES];
        long long ps[VMAF_SCALES];
        for (int q = 1; q < VMAF_SCALES; ++q) pl[q] = workspace + p.plane_off[q], ps[q] = (long long)p.vh[q] * p.vw[q];
        if ((rc = vmaf_vif_down<9>(p, 1, k, r0, d0, size, tables + VT_G9, pl[1], s))) return rc;
        if ((rc = vmaf_vif_scale<9>(p, 1, k, pl[1], pl[1] + ps[1], 2 * ps[1], tables + VT_G9, part + p.voff[1], s))) return rc;
        if ((rc = vmaf_vif_down<5>(p, 2, k, pl[1], pl[1] + ps[1], 2 * ps[1], tables + VT_G5, pl[2], s))) return rc;
        if ((rc = vmaf_vif_scale<5>(p, 2, k, pl[2], pl[2] + ps[2], 2 * ps[2], tables + VT_G5, part + p.voff[2], s))) return rc;
        if ((rc = vmaf_vif_down<3>(p, 3, k, pl[2], pl[2] + ps[2], 2 * ps[2], tables + VT_G3, pl[3], s))) return rc;
        if ((rc = vmaf_vif_scale<3>(p, 3, k, pl[3], pl[3] + ps[3], 2 * ps[3], tables + VT_G3, part + p.voff[3], s))) return rc;
        // ADM: one wavelet step and one pooling per scale
        int ih = h, iw = w;
        for (int q = 0; q < VMAF_SCALES; ++q) {
            double* bands = workspace + p.band_off[q];
            const long long bsize = (long long)p.ah[q] * p.aw[q];
            const dim3 grid(cdiv(bsize, VMAF_THREADS), k, 2);
            if (q == 0) {
                hipLaunchKernelGGL(vmaf_dwt_kernel<true>, grid, dim3(VMAF_THREADS), 0, s, (const void*)r0, (const void*)d0, size, tables, bands,
                                   ih, iw, p.ah[q], p.aw[q]);
            } else {
                const double* before = workspace + p.band_off[q - 1];
                const long long in_size = (long long)ih * iw;
                hipLaunchKernelGGL(vmaf_dwt_kernel<false>, grid, dim3(VMAF_THREADS), 0, s, (const void*)before,
                                   (const void*)(before + 4 * in_size), 8 * in_size, tables, bands, ih, iw, p.ah[q], p.aw[q]);
            }
            ELVIS_CHECK_LAUNCH("elvis_vmaf_features_f64(dwt)");
            hipLaunchKernelGGL(vmaf_adm_pool_kernel, dim3(p.atiles[q], k), dim3(VMAF_THREADS), 0, s, (const double*)bands, tables,
                               part + p.aoff[q], p.per_frame, q, p.ah[q], p.aw[q], cdiv(p.aw[q], VMAF_AT), p.left[q], p.top[q]);
            ELVIS_CHECK_LAUNCH("elvis_vmaf_features_f64(adm)");
            ih = p.ah[q], iw = p.aw[q];
        }
    }
    hipLaunchKernelGGL(vmaf_motion_kernel, dim3(p.mtiles, n + p.has_next), dim3(VMAF_THREADS), 0, s, ref, prev, next, tables,
                       workspace + p.motion_off, n, h, w, cdiv(w, VMAF_TW));
    ELVIS_CHECK_LAUNCH("elvis_vmaf_features_f64(motion)");
    hipLaunchKernelGGL(vmaf_finish_kernel, dim3(n), dim3(VMAF_THREADS), 0, s, (const double*)workspace, out, p);
    ELVIS_CHECK_LAUNCH("elvis_vmaf_features_f64(finish)");
    elvis_note_launch("vmaf_finish_kernel");
    return ELVIS_OK;
}

extern "C" int elvis_vmaf_predict_f64(const double* feats, const double* model, double* out, int n, int nsv, int flags,
                                      elvis_stream_t stream) {
    ELVIS_REQUIRE(n >= 0 && nsv >= 1 && nsv <= (1 << 20), "elvis_vmaf_predict_f64: bad shape n=%d support vectors=%d", n, nsv);
    ELVIS_REQUIRE(flags >= 0 && flags < 8, "elvis_vmaf_predict_f64: bad flags %d", flags);
    if (n == 0) return ELVIS_OK;
    ELVIS_REQUIRE(feats && model && out, "elvis_vmaf_predict_f64: null pointer");
    hipLaunchKernelGGL(vmaf_predict_kernel, dim3(cdiv(n, VMAF_THREADS / ELVIS_WAVE)), dim3(VMAF_THREADS), 0, (hipStream_t)stream, feats, model,
                       out, n, nsv, flags);
    ELVIS_CHECK_LAUNCH("elvis_vmaf_predict_f64");
    elvis_note_launch("vmaf_predict_kernel");
    return ELVIS_OK;
}
