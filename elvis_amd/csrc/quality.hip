// Quality report on the device: mask bounding boxes, mask application, and the windowed SSIM mean of the two
// evaluators the reference runs per sampled frame - skimage's Gaussian SSIM on masked luma (elvis.py:674-721) and
// pytorch_msssim's valid-window SSIM per channel (presley.py:248-259).  float64 throughout, no fused contraction,
// no float atomics: a frame's result is a fixed-order sum and does not depend on the batch it rides in.
#include "common.h"

// ---------------------------------------------------------------------------------------
// elvis_mask_bbox_u8: one workgroup per frame scans the mask as a flat byte array (8 bytes per load where the frame's
// plane is 8-byte aligned), keeps integer min/max per thread and reduces them in LDS.
#define BBOX_THREADS 1024

__global__ __launch_bounds__(BBOX_THREADS) void mask_bbox_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ out,
                                                                 int h, int w) {
    const int f = blockIdx.x;
    const long long plane = (long long)h * w;
    const uint8_t* pm = mask + (long long)f * plane;
    int y0 = h, y1 = 0, x0 = w, x1 = 0;
    const bool wide = ((uintptr_t)pm & 7) == 0;
    const long long words = wide ? plane / 8 : 0;
    for (long long i = threadIdx.x; i < words; i += BBOX_THREADS) {
        const unsigned long long v = *reinterpret_cast<const unsigned long long*>(pm + i * 8);
        if (v == 0) continue;
        int y = (int)((i * 8) / w), x = (int)((i * 8) - (long long)y * w);
        for (int k = 0; k < 8; ++k) {
            if ((v >> (8 * k)) & 0xFFull) {
                y0 = min(y0, y); y1 = max(y1, y + 1); x0 = min(x0, x); x1 = max(x1, x + 1);
            }
            if (++x == w) { x = 0; ++y; }
        }
    }
    for (long long i = words * 8 + threadIdx.x; i < plane; i += BBOX_THREADS) {
        if (pm[i]) {
            const int y = (int)(i / w), x = (int)(i - (long long)y * w);
            y0 = min(y0, y); y1 = max(y1, y + 1); x0 = min(x0, x); x1 = max(x1, x + 1);
        }
    }
    __shared__ int red[4][BBOX_THREADS];
    red[0][threadIdx.x] = y0; red[1][threadIdx.x] = y1; red[2][threadIdx.x] = x0; red[3][threadIdx.x] = x1;
    __syncthreads();
    for (int s = BBOX_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] = min(red[0][threadIdx.x], red[0][threadIdx.x + s]);
            red[1][threadIdx.x] = max(red[1][threadIdx.x], red[1][threadIdx.x + s]);
            red[2][threadIdx.x] = min(red[2][threadIdx.x], red[2][threadIdx.x + s]);
            red[3][threadIdx.x] = max(red[3][threadIdx.x], red[3][threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool empty = red[1][0] == 0;
        out[f * 4 + 0] = empty ? 0 : red[0][0];
        out[f * 4 + 1] = red[1][0];
        out[f * 4 + 2] = empty ? 0 : red[2][0];
        out[f * 4 + 3] = red[3][0];
    }
}

extern "C" int elvis_mask_bbox_u8(const uint8_t* mask, int32_t* bbox_out, int n, int h, int w, elvis_stream_t stream) {
    ELVIS_REQUIRE(mask && bbox_out, "elvis_mask_bbox_u8: null pointer");
    ELVIS_REQUIRE(n > 0 && h > 0 && w > 0, "elvis_mask_bbox_u8: bad shape n=%d h=%d w=%d", n, h, w);
    hipLaunchKernelGGL(mask_bbox_kernel, dim3(n), dim3(BBOX_THREADS), 0, (hipStream_t)stream, mask, bbox_out, h, w);
    ELVIS_CHECK_LAUNCH("elvis_mask_bbox_u8");
    elvis_note_launch("mask_bbox_kernel");
    return ELVIS_OK;
}

// ---------------------------------------------------------------------------------------
// elvis_apply_mask_u8: out = (mask != 0) != invert ? frame : 0.  C = 1, 3 or 4 on 16-byte aligned tensors: a thread
// takes 16 pixels - one 16-byte mask load, C 16-byte frame loads and stores; the tail and every other case go byte
// by byte (C == 0 names that instantiation).
template <int C>
__global__ __launch_bounds__(256) void apply_mask_u8_kernel(const uint8_t* __restrict__ frame, const uint8_t* __restrict__ mask,
                                                            uint8_t* __restrict__ out, long long pixels, int c, int invert) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long done = 0;
    if (C > 0) {
        const long long groups = pixels / 16;
        for (long long g = t0; g < groups; g += stride) {
            union { uint4 v; uint8_t b[16]; } m;
            union { uint4 v[C > 0 ? C : 1]; uint8_t b[16 * (C > 0 ? C : 1)]; } px;
            m.v = *reinterpret_cast<const uint4*>(mask + g * 16);
#pragma unroll
            for (int k = 0; k < C; ++k) px.v[k] = *reinterpret_cast<const uint4*>(frame + (g * 16) * C + 16 * k);
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const bool keep = (m.b[p] != 0) != (invert != 0);
#pragma unroll
                for (int k = 0; k < C; ++k) px.b[p * C + k] = keep ? px.b[p * C + k] : (uint8_t)0;
            }
#pragma unroll
            for (int k = 0; k < C; ++k) *reinterpret_cast<uint4*>(out + (g * 16) * C + 16 * k) = px.v[k];
        }
        done = groups * 16;
    }
    for (long long p = done + t0; p < pixels; p += stride) {
        const bool keep = (mask[p] != 0) != (invert != 0);
        for (int k = 0; k < c; ++k) out[p * c + k] = keep ? frame[p * c + k] : (uint8_t)0;
    }
}

extern "C" int elvis_apply_mask_u8(const uint8_t* frames, const uint8_t* mask, uint8_t* out, int n, int h, int w, int c,
                                   int invert, elvis_stream_t stream) {
    ELVIS_REQUIRE(frames && mask && out, "elvis_apply_mask_u8: null pointer");
    ELVIS_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0, "elvis_apply_mask_u8: bad shape n=%d h=%d w=%d c=%d", n, h, w, c);
    const long long pixels = (long long)n * h * w;
    const bool aligned = ((uintptr_t)frames | (uintptr_t)mask | (uintptr_t)out) % 16 == 0;
    int grid = cdiv(cdiv(pixels, 16), 256);
    if (grid > 16384) grid = 16384;
    const int vc = aligned && (c == 1 || c == 3 || c == 4) ? c : 0;
#define ELVIS_APPLY_MASK(C)                                                                                            \
    hipLaunchKernelGGL(apply_mask_u8_kernel<C>, dim3(grid), dim3(256), 0, (hipStream_t)stream, frames, mask, out, pixels, \
                       c, invert);                                                                                     \
    ELVIS_CHECK_LAUNCH("elvis_apply_mask_u8");                                                                         \
    elvis_note_launch("apply_mask_u8_kernel<" #C ">")
    if (vc == 1) { ELVIS_APPLY_MASK(1); }
    else if (vc == 3) { ELVIS_APPLY_MASK(3); }
    else if (vc == 4) { ELVIS_APPLY_MASK(4); }
    else { ELVIS_APPLY_MASK(0); }
#undef ELVIS_APPLY_MASK
    return ELVIS_OK;
}

// ---------------------------------------------------------------------------------------
// elvis_ssim_mean_f64.
//
// Geometry of one frame.  The work area is the frame's rectangle (clipped to the frame) or the whole frame, lh x lw.
// The SSIM map that is averaged starts at (my, mx) of the work area and is mh x mw:
//   REFLECT  taps reach 5 pixels either side of an output and reflect at the work area's edge (d c b a | a b c d,
//            repeatedly); the map is the work area shrunk by pad on every side (skimage's crop(S, pad))
//   VALID    taps reach 10 pixels right of / below an output, the map is 10 shorter than the work area; a dimension
//            shorter than 11 is not smoothed (its window is a single 1 at tap 0 - the other ten taps multiply in-range
//            pixels by an exact 0.0, which leaves the sum bit-for-bit the pixel)
// pad < 0 (ELVIS_SSIM_PAD_AUTO) takes pad and cov_norm per frame from the work area by the rule of elvis.py:702-711:
// win = 7, or for a smallest side in 3..6 the largest odd number not above it; pad = (win - 1) / 2,
// cov_norm = win^2 / (win^2 - 1).  A frame with no map to average (empty rectangle, a side under 3 in the automatic
// rule, pad eating the whole area) is `degenerate`: its tiles add nothing and the result is 1.0, which is what
// elvis.py:685-686 and :704-706 return.
#define SSIM_TH 16
#define SSIM_TW 32
#define SSIM_ROWS (SSIM_TH + 10)
#define SSIM_COLS (SSIM_TW + 10)
#define SSIM_THREADS 256
#define SSIM_RAW_PITCH 176    // bytes: 42 pixels x 4 channels + 3 bytes of alignment shift, rounded to 16
#define SSIM_MASK_PITCH 48    // bytes: 42 + 3, rounded to 16
#define SSIM_MAX_C 4

struct SsimArea {
    int y0, x0, lh, lw;   // work area in the frame
    int my, mx, mh, mw;   // averaged map inside the work area
    double cov_norm;
    bool degenerate;
};

template <int BORDER>
__device__ __forceinline__ SsimArea ssim_area(const int32_t* __restrict__ rects, int f, int h, int w, int pad, double cov_norm) {
    SsimArea g;
    int y0 = 0, y1 = h, x0 = 0, x1 = w;
    if (rects) {
        y0 = max(0, rects[f * 4 + 0]); y1 = min(h, rects[f * 4 + 1]);
        x0 = max(0, rects[f * 4 + 2]); x1 = min(w, rects[f * 4 + 3]);
    }
    g.y0 = y0; g.x0 = x0; g.lh = y1 - y0; g.lw = x1 - x0;
    g.cov_norm = cov_norm;
    g.degenerate = g.lh <= 0 || g.lw <= 0;
    if (pad < 0) {
        const int side = min(g.lh, g.lw);
        int win = 7;
        if (side < 3) g.degenerate = true;
        else if (side < 7) win = (side & 1) ? side : max(3, side - 1);
        pad = (win - 1) / 2;
        g.cov_norm = (double)(win * win) / (double)(win * win - 1);
    }
    const int sh = BORDER == ELVIS_SSIM_VALID && g.lh >= 11 ? g.lh - 10 : g.lh;
    const int sw = BORDER == ELVIS_SSIM_VALID && g.lw >= 11 ? g.lw - 10 : g.lw;
    g.my = pad; g.mx = pad; g.mh = sh - 2 * pad; g.mw = sw - 2 * pad;
    if (g.mh <= 0 || g.mw <= 0) g.degenerate = true;
    return g;
}

// scipy.ndimage's `reflect` (half-sample symmetric), for any integer p
__device__ __forceinline__ int reflect_idx(int p, int len) {
    const int per = 2 * len;
    int m = p % per;
    if (m < 0) m += per;
    return m < len ? m : per - 1 - m;
}

// First byte of staged row r: pixel (reflected row iy0 + r, column ix0) of the work area.  Only meaningful as a whole
// row when columns ix0 .. ix0 + SSIM_COLS - 1 lie inside the work area (the `wide` case).
__device__ __forceinline__ const uint8_t* ssim_row_ptr(const uint8_t* plane, int w, int bpp, const SsimArea& g, int iy0, int ix0, int r) {
    const int gy = g.y0 + reflect_idx(iy0 + r, g.lh);
    return plane + ((long long)gy * w + g.x0 + ix0) * bpp;
}

// Stage SSIM_ROWS x SSIM_COLS pixels of bpp bytes into LDS.  wide: every row is one contiguous run in memory, fetched
// as aligned 4-byte words (the run starts `ptr & 3` bytes into its first word; a word that would cross the tensor's
// end is fetched by bytes).  Otherwise each pixel is fetched through the reflected column index and the run starts at
// byte 0 of the LDS row.
__device__ __forceinline__ void ssim_stage(const uint8_t* plane, const uint8_t* tensor_end, int w, int bpp, const SsimArea& g,
                                           int iy0, int ix0, bool wide, uint8_t* lds, int pitch) {
    if (wide) {
        const int ndw_max = (3 + SSIM_COLS * bpp + 3) / 4;
        for (int i = threadIdx.x; i < SSIM_ROWS * ndw_max; i += SSIM_THREADS) {
            const int r = i / ndw_max, d = i - r * ndw_max;
            const uint8_t* p = ssim_row_ptr(plane, w, bpp, g, iy0, ix0, r);
            const int sh = (int)((uintptr_t)p & 3);
            if (d * 4 >= sh + SSIM_COLS * bpp) continue;
            const uint8_t* q = p - sh + d * 4;
            uint32_t v = 0;
            if (q + 4 <= tensor_end) v = *reinterpret_cast<const uint32_t*>(q);
            else
                for (int k = 0; k < 4; ++k)
                    if (q + k < tensor_end) v |= (uint32_t)q[k] << (8 * k);
            *reinterpret_cast<uint32_t*>(lds + r * pitch + d * 4) = v;
        }
    } else {
        for (int i = threadIdx.x; i < SSIM_ROWS * SSIM_COLS; i += SSIM_THREADS) {
            const int r = i / SSIM_COLS, j = i - r * SSIM_COLS;
            const int gy = g.y0 + reflect_idx(iy0 + r, g.lh), gx = g.x0 + reflect_idx(ix0 + j, g.lw);
            const uint8_t* p = plane + ((long long)gy * w + gx) * bpp;
            for (int k = 0; k < bpp; ++k) lds[r * pitch + j * bpp + k] = p[k];
        }
    }
}

struct SsimParams {
    const uint8_t* a;
    const uint8_t* b;
    const uint8_t* mask;
    const int32_t* rects;
    const double* win11;
    double* partial;
    int n, h, w, c, tiles_x, tiles, pad, aligned;
    double C1, C2, cov_norm, scale;
};

template <int SOURCE, int BORDER>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_tile_kernel(SsimParams P) {
    // one LDS array: the five moment planes after the row pass; the raw bytes alias them (dead once converted)
    __shared__ __attribute__((aligned(16))) double lds_f64[2 * SSIM_ROWS * SSIM_COLS + 5 * SSIM_ROWS * SSIM_TW];
    double (*xs)[SSIM_COLS] = reinterpret_cast<double (*)[SSIM_COLS]>(lds_f64);
    double (*ys)[SSIM_COLS] = reinterpret_cast<double (*)[SSIM_COLS]>(lds_f64 + SSIM_ROWS * SSIM_COLS);
    double (*hp)[SSIM_ROWS][SSIM_TW] = reinterpret_cast<double (*)[SSIM_ROWS][SSIM_TW]>(lds_f64 + 2 * SSIM_ROWS * SSIM_COLS);
    uint8_t* raw_a = reinterpret_cast<uint8_t*>(&hp[0][0][0]);
    uint8_t* raw_b = raw_a + SSIM_ROWS * SSIM_RAW_PITCH;
    uint8_t* raw_m = raw_b + SSIM_ROWS * SSIM_RAW_PITCH;
    static_assert(2 * SSIM_ROWS * SSIM_RAW_PITCH + SSIM_ROWS * SSIM_MASK_PITCH <= 5 * SSIM_ROWS * SSIM_TW * 8, "raw bytes must fit the planes");
    static_assert(SSIM_RAW_PITCH >= ((3 + SSIM_COLS * SSIM_MAX_C + 3) / 4) * 4 && SSIM_MASK_PITCH >= ((3 + SSIM_COLS + 3) / 4) * 4, "LDS row pitch");

    const int tile = blockIdx.x, ch = blockIdx.y, f = blockIdx.z;
    const int cout = SOURCE == ELVIS_SSIM_LUMA ? 1 : P.c;
    double* dst = P.partial + ((long long)f * cout + ch) * P.tiles + tile;
    const SsimArea g = ssim_area<BORDER>(P.rects, f, P.h, P.w, P.pad, P.cov_norm);
    const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
    const int oy0 = ty * SSIM_TH, ox0 = tx * SSIM_TW;            // the tile's first output, in map coordinates
    if (g.degenerate || oy0 >= g.mh || ox0 >= g.mw) {            // uniform over the workgroup
        if (threadIdx.x == 0) *dst = 0.0;
        return;
    }
    const int toff = BORDER == ELVIS_SSIM_REFLECT ? -5 : 0;
    const int iy0 = g.my + oy0 + toff, ix0 = g.mx + ox0 + toff;  // first staged pixel, in work-area coordinates
    const bool wide = P.aligned && ix0 >= 0 && ix0 + SSIM_COLS <= g.lw;

    const long long plane_px = (long long)P.h * P.w;
    const uint8_t* pa = P.a + (long long)f * plane_px * P.c;
    const uint8_t* pb = P.b + (long long)f * plane_px * P.c;
    const uint8_t* pm = P.mask ? P.mask + (long long)f * plane_px : nullptr;
    ssim_stage(pa, P.a + (long long)P.n * plane_px * P.c, P.w, P.c, g, iy0, ix0, wide, raw_a, SSIM_RAW_PITCH);
    ssim_stage(pb, P.b + (long long)P.n * plane_px * P.c, P.w, P.c, g, iy0, ix0, wide, raw_b, SSIM_RAW_PITCH);
    if (pm) ssim_stage(pm, P.mask + (long long)P.n * plane_px, P.w, 1, g, iy0, ix0, wide, raw_m, SSIM_MASK_PITCH);
    __syncthreads();

    // bytes -> float64 samples: luma by OpenCV's 8-bit BGR2YCrCb rule, or one channel / scale; zero outside the mask
    for (int i = threadIdx.x; i < SSIM_ROWS * SSIM_COLS; i += SSIM_THREADS) {
        const int r = i / SSIM_COLS, j = i - r * SSIM_COLS;
        int sa = 0, sb = 0, sm = 0;
        if (wide) {
            sa = (int)((uintptr_t)ssim_row_ptr(pa, P.w, P.c, g, iy0, ix0, r) & 3);
            sb = (int)((uintptr_t)ssim_row_ptr(pb, P.w, P.c, g, iy0, ix0, r) & 3);
            if (pm) sm = (int)((uintptr_t)ssim_row_ptr(pm, P.w, 1, g, iy0, ix0, r) & 3);
        }
        const uint8_t* qa = raw_a + r * SSIM_RAW_PITCH + sa + j * P.c;
        const uint8_t* qb = raw_b + r * SSIM_RAW_PITCH + sb + j * P.c;
        double va, vb;
        if (SOURCE == ELVIS_SSIM_LUMA) {
            va = (double)((1868 * qa[0] + 9617 * qa[1] + 4899 * qa[2] + 8192) >> 14);
            vb = (double)((1868 * qb[0] + 9617 * qb[1] + 4899 * qb[2] + 8192) >> 14);
        } else {
            va = (double)qa[ch] / P.scale;
            vb = (double)qb[ch] / P.scale;
        }
        if (pm && raw_m[r * SSIM_MASK_PITCH + sm + j] == 0) va = vb = 0.0;
        xs[r][j] = va;
        ys[r][j] = vb;
    }
    double wy[11], wx[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) {
        const double wk = P.win11[k];
        wy[k] = BORDER == ELVIS_SSIM_VALID && g.lh < 11 ? (k == 0 ? 1.0 : 0.0) : wk;
        wx[k] = BORDER == ELVIS_SSIM_VALID && g.lw < 11 ? (k == 0 ? 1.0 : 0.0) : wk;
    }
    __syncthreads();   // samples written; the raw bytes under hp are dead

    // row pass: five moment planes, SSIM_ROWS x SSIM_TW
    for (int i = threadIdx.x; i < SSIM_ROWS * SSIM_TW; i += SSIM_THREADS) {
        const int r = i / SSIM_TW, ox = i - r * SSIM_TW;
        double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const double x = xs[r][ox + k], y = ys[r][ox + k];
            ux += wx[k] * x; uy += wx[k] * y; uxx += wx[k] * (x * x); uyy += wx[k] * (y * y); uxy += wx[k] * (x * y);
        }
        hp[0][r][ox] = ux; hp[1][r][ox] = uy; hp[2][r][ox] = uxx; hp[3][r][ox] = uyy; hp[4][r][ox] = uxy;
    }
    __syncthreads();

    // column pass, S per output, fixed-order sum over the tile
    double acc = 0.0;
    for (int i = threadIdx.x; i < SSIM_TH * SSIM_TW; i += SSIM_THREADS) {
        const int ly = i / SSIM_TW, lx = i - ly * SSIM_TW;
        if (oy0 + ly >= g.mh || ox0 + lx >= g.mw) continue;
        double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            ux += wy[k] * hp[0][ly + k][lx]; uy += wy[k] * hp[1][ly + k][lx];
            uxx += wy[k] * hp[2][ly + k][lx]; uyy += wy[k] * hp[3][ly + k][lx]; uxy += wy[k] * hp[4][ly + k][lx];
        }
        const double vx = g.cov_norm * (uxx - ux * ux), vy = g.cov_norm * (uyy - uy * uy), vxy = g.cov_norm * (uxy - ux * uy);
        const double num = (2.0 * ux * uy + P.C1) * (2.0 * vxy + P.C2);
        const double den = (ux * ux + uy * uy + P.C1) * (vx + vy + P.C2);
        acc += num / den;
    }
    double* red = &xs[0][0];   // samples are dead after the row pass (barrier above)
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = SSIM_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *dst = red[0];
}

// out[f, ch] = (sum of the frame's tile partials, in a fixed order) / map size; 1.0 for a degenerate frame
template <int BORDER>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_finish_kernel(const double* __restrict__ partial, const int32_t* __restrict__ rects,
                                                                   double* __restrict__ out, int h, int w, int cout, int tiles,
                                                                   int pad) {
    __shared__ double red[SSIM_THREADS];
    const int fc = blockIdx.x, f = fc / cout;
    const SsimArea g = ssim_area<BORDER>(rects, f, h, w, pad, 1.0);
    const double* p = partial + (long long)fc * tiles;
    double acc = 0.0;
    for (int i = threadIdx.x; i < tiles; i += SSIM_THREADS) acc += p[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = SSIM_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[fc] = g.degenerate ? 1.0 : red[0] / ((double)g.mh * (double)g.mw);
}

static inline int ssim_tiles(int h, int w) { return cdiv(h, SSIM_TH) * cdiv(w, SSIM_TW); }

extern "C" size_t elvis_ssim_workspace_bytes(int n, int h, int w, int c) {
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return 0;
    return (size_t)n * (size_t)c * (size_t)ssim_tiles(h, w) * sizeof(double);
}

template <int SOURCE, int BORDER>
static int ssim_launch(const SsimParams& P, double* out, hipStream_t stream, const char* tile_name) {
    const int cout = SOURCE == ELVIS_SSIM_LUMA ? 1 : P.c;
    hipLaunchKernelGGL((ssim_tile_kernel<SOURCE, BORDER>), dim3(P.tiles, cout, P.n), dim3(SSIM_THREADS), 0, stream, P);
    ELVIS_CHECK_LAUNCH("elvis_ssim_mean_f64");
    hipLaunchKernelGGL(ssim_finish_kernel<BORDER>, dim3(P.n * cout), dim3(SSIM_THREADS), 0, stream, P.partial, P.rects, out, P.h,
                       P.w, cout, P.tiles, P.pad);
    ELVIS_CHECK_LAUNCH("elvis_ssim_mean_f64(finish)");
    elvis_note_launch(tile_name);
    return ELVIS_OK;
}

extern "C" int elvis_ssim_mean_f64(const uint8_t* a, const uint8_t* b, const uint8_t* mask, const int32_t* rects,
                                   const double* win11, double* workspace, double* out, int n, int h, int w, int c, int source,
                                   int border, double C1, double C2, double cov_norm, int pad, double scale,
                                   elvis_stream_t stream) {
    ELVIS_REQUIRE(a && b && win11 && workspace && out, "elvis_ssim_mean_f64: null pointer");
    ELVIS_REQUIRE(n > 0 && n <= 65535 && h > 0 && w > 0 && c > 0 && c <= SSIM_MAX_C, "elvis_ssim_mean_f64: bad shape n=%d h=%d w=%d c=%d",
                  n, h, w, c);
    ELVIS_REQUIRE(source == ELVIS_SSIM_LUMA || source == ELVIS_SSIM_CHANNELS, "elvis_ssim_mean_f64: unknown source %d", source);
    ELVIS_REQUIRE(border == ELVIS_SSIM_REFLECT || border == ELVIS_SSIM_VALID, "elvis_ssim_mean_f64: unknown border %d", border);
    ELVIS_REQUIRE(source != ELVIS_SSIM_LUMA || c == 3, "elvis_ssim_mean_f64: the luma form needs 3-channel BGR frames, got %d channels", c);
    ELVIS_REQUIRE(pad >= 0 || pad == ELVIS_SSIM_PAD_AUTO, "elvis_ssim_mean_f64: bad pad %d", pad);
    ELVIS_REQUIRE(scale > 0.0 && cov_norm > 0.0, "elvis_ssim_mean_f64: scale and cov_norm must be positive");
    SsimParams P;
    P.a = a; P.b = b; P.mask = mask; P.rects = rects; P.win11 = win11; P.partial = workspace;
    P.n = n; P.h = h; P.w = w; P.c = c; P.tiles_x = cdiv(w, SSIM_TW); P.tiles = ssim_tiles(h, w); P.pad = pad;
    P.aligned = ((uintptr_t)a | (uintptr_t)b | (uintptr_t)mask) % 4 == 0;
    P.C1 = C1; P.C2 = C2; P.cov_norm = cov_norm; P.scale = scale;
    hipStream_t s = (hipStream_t)stream;
    if (source == ELVIS_SSIM_LUMA)
        return border == ELVIS_SSIM_REFLECT ? ssim_launch<ELVIS_SSIM_LUMA, ELVIS_SSIM_REFLECT>(P, out, s, "ssim_tile_kernel<luma,reflect>")
                                            : ssim_launch<ELVIS_SSIM_LUMA, ELVIS_SSIM_VALID>(P, out, s, "ssim_tile_kernel<luma,valid>");
    return border == ELVIS_SSIM_REFLECT ? ssim_launch<ELVIS_SSIM_CHANNELS, ELVIS_SSIM_REFLECT>(P, out, s, "ssim_tile_kernel<channels,reflect>")
                                        : ssim_launch<ELVIS_SSIM_CHANNELS, ELVIS_SSIM_VALID>(P, out, s, "ssim_tile_kernel<channels,valid>");
}
