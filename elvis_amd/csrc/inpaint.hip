// The ELVIS v1 inpaint step on the device: the holes a stretch leaves are filled with Telea's estimator.  The
// reference calls cv2.inpaint(stretched_frame, mask, inpaintRadius=3, flags=cv2.INPAINT_TELEA) (elvis.py:4601-4606,
// Presley's inpaint_with_opencv presley.py:838-850).  OpenCV's Telea is a fast-marching method: one heap orders the
// pixels and every fill reads fills made just before it.  This is a BUILD-DEFINED inpainter ("wavefront Telea",
// DESIGN.md 7): Telea's weights on a fill order a GPU can run.  It does not claim parity with cv2.
//   elvis_inpaint_workspace_bytes - host only: the size of the workspace of a clip
//   elvis_inpaint_prepare         - the exact squared Euclidean distance D2 of every hole pixel to the nearest known
//                                   pixel of its frame, T = sqrt(D2) (1 - sqrt(distance to the hole) on the known side),
//                                   wave = ceil(sqrt(D2)) in integers, and per wave the list of its pixels
//                                   (histogram, scan, scatter)
//   elvis_inpaint_fill            - one launch per wave over the whole clip, one thread per listed pixel, in place:
//                                   a wave reads known pixels and earlier waves only (Jacobi), so the result does
//                                   not depend on the order inside a wave
// Every float operation is an IEEE float32 operation in the order DESIGN.md 7 writes it (no contraction).  Square
// roots are sqrtf, which hipcc rounds correctly by default; HIP's __fsqrt_rn is the native v_sqrt_f32 (1 ulp) and
// gave another T where D2 = 82 - found by the `bins_256` case of tests/_inpaint_ref.py.
#include <limits.h>
#include "common.h"

namespace {

constexpr int kRadius = 3;
constexpr int kNoDist = 0xFFFF;      // row distance of a pixel whose row has no known pixel
constexpr int kLocalBins = 64;       // waves counted in LDS before they reach the global histogram

// ------------------------------------------------------------------------------------------------ workspace
// [ hist int32[bins] | offs int32[bins + 1] | cursor int32[bins] | T f32[npix] | wave u16[npix] | list int32[npix] ]
// bins = h + w + 2 (a wave is at most ceil(hypot(h - 1, w - 1)) <= h + w).  The row distances (u16[npix]) live in the
// list's bytes: they are dead when the scatter starts.  Every part starts on a 256-byte boundary.
struct Workspace {
    int32_t *hist, *offs, *cursor;
    float* T;
    uint16_t* wave;
    int32_t* list;
    uint16_t* rowdist;
    size_t bytes;
};

size_t round256(size_t v) { return (v + 255) / 256 * 256; }

Workspace carve(void* base, long long npix, int bins) {
    Workspace ws;
    char* p = (char*)base;
    size_t o = 0;
    ws.hist = (int32_t*)(p + o);
    ws.offs = ws.hist + bins;
    ws.cursor = ws.offs + bins + 1;
    o = round256(sizeof(int32_t) * (3 * (size_t)bins + 1));
    ws.T = (float*)(p + o);
    o += round256(sizeof(float) * (size_t)npix);
    ws.wave = (uint16_t*)(p + o);
    o += round256(sizeof(uint16_t) * (size_t)npix);
    ws.list = (int32_t*)(p + o);
    ws.rowdist = (uint16_t*)(p + o);
    o += round256(sizeof(int32_t) * (size_t)npix);
    ws.bytes = o;
    return ws;
}

// h, w <= 32767: h * h + w * w fits an int, a row distance and a wave fit 16 bits below kNoDist
bool shape_ok(int n, int h, int w) {
    return n > 0 && h > 0 && w > 0 && h <= 32767 && w <= 32767 && (long long)n * h * w < (1LL << 31);
}

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

// ------------------------------------------------------------------------------------------------ prepare
// One workgroup per frame row: the distance of every pixel to the nearest known pixel of its row (0 on a known
// pixel, kNoDist where the row has none).  A thread owns a run of consecutive pixels; the nearest known pixel before
// and after the run comes from the other threads' first / last known pixel.  Workgroup 0 also clears the histogram.
__global__ __launch_bounds__(256) void inpaint_rows_kernel(MaskView mv, uint16_t* __restrict__ rowdist, int32_t* __restrict__ hist,
                                                           int bins, int h, int w) {
    __shared__ int first_known[256], last_known[256];
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < bins; i += blockDim.x) hist[i] = 0;
    const long long row = blockIdx.x;                         // f * h + y
    const int f = (int)(row / h), y = (int)(row - (long long)f * h);
    const int chunk = (w + 255) / 256;
    const int lo = min(w, (int)threadIdx.x * chunk), hi = min(w, lo + chunk);
    int fk = INT_MAX, lk = -1;
    for (int x = lo; x < hi; ++x)
        if (!is_hole(mv, f, y, x, h, w)) {
            if (fk == INT_MAX) fk = x;
            lk = x;
        }
    first_known[threadIdx.x] = fk;
    last_known[threadIdx.x] = lk;
    __syncthreads();
    int left = -1, right = INT_MAX;
    for (int t = (int)threadIdx.x - 1; t >= 0 && left < 0; --t) left = last_known[t];
    for (int t = (int)threadIdx.x + 1; t < 256 && right == INT_MAX; ++t) right = first_known[t];
    uint16_t* g = rowdist + row * w;
    int cur = left;
    for (int x = lo; x < hi; ++x) {
        if (!is_hole(mv, f, y, x, h, w)) cur = x;
        g[x] = (uint16_t)(cur < 0 ? kNoDist : x - cur);
    }
    cur = right;
    for (int x = hi - 1; x >= lo; --x) {
        if (!is_hole(mv, f, y, x, h, w)) cur = x;
        const int d = cur == INT_MAX ? kNoDist : cur - x;
        if (d < (int)g[x]) g[x] = (uint16_t)d;
    }
}

// One thread per pixel.  Hole: D2 = min over the rows y' of (y - y')^2 + rowdist(y', x)^2, searched outward from y and
// stopped where dy^2 alone reaches the best value so far - exact.  Known: T = 1 - sqrt(d2h) with d2h the squared
// distance to the nearest hole among |dx|, |dy| <= 3 (0 where there is none; such a T is never read).
__global__ __launch_bounds__(256) void inpaint_columns_kernel(MaskView mv, const uint16_t* __restrict__ rowdist,
                                                              float* __restrict__ T, uint16_t* __restrict__ wave,
                                                              int32_t* __restrict__ hist, int bins, int h, int w, long long npix) {
    __shared__ int local_hist[kLocalBins];
    if (threadIdx.x < kLocalBins) local_hist[threadIdx.x] = 0;
    __syncthreads();
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < npix) {
        const long long row = idx / w;
        const int x = (int)(idx - row * w);
        const int f = (int)(row / h), y = (int)(row - (long long)f * h);
        float t = 0.0f;
        int k = 0;
        if (!is_hole(mv, f, y, x, h, w)) {
            int d2h = INT_MAX;
            for (int dy = -kRadius; dy <= kRadius; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= h) continue;
                for (int dx = -kRadius; dx <= kRadius; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= w || dy * dy + dx * dx >= d2h) continue;
                    if (is_hole(mv, f, yy, xx, h, w)) d2h = dy * dy + dx * dx;
                }
            }
            if (d2h != INT_MAX) t = __fsub_rn(1.0f, sqrtf((float)d2h));
        } else {
            const uint16_t* col = rowdist + (long long)f * h * w + x;
            const int g0 = col[(long long)y * w];
            int best = g0 == kNoDist ? INT_MAX : g0 * g0;
            for (int dy = 1; dy * dy < best; ++dy) {
                const bool up = y - dy >= 0, down = y + dy < h;
                if (!up && !down) break;
                if (up) {
                    const int g = col[(long long)(y - dy) * w];
                    if (g != kNoDist) best = min(best, dy * dy + g * g);
                }
                if (down) {
                    const int g = col[(long long)(y + dy) * w];
                    if (g != kNoDist) best = min(best, dy * dy + g * g);
                }
            }
            if (best != INT_MAX) {                            // else: a frame without a known pixel stays as it is
                k = (int)sqrtf((float)best);
                while ((long long)k * k < best) ++k;          // the smallest k with k * k >= D2, in integers
                while (k > 1 && (long long)(k - 1) * (k - 1) >= best) --k;
                t = sqrtf((float)best);
                if (k < kLocalBins) atomicAdd(&local_hist[k], 1);
                else if (k < bins) atomicAdd(&hist[k], 1);
            }
        }
        T[idx] = t;
        wave[idx] = (uint16_t)k;
    }
    __syncthreads();
    if (threadIdx.x < kLocalBins && threadIdx.x < bins && local_hist[threadIdx.x]) atomicAdd(&hist[threadIdx.x], local_hist[threadIdx.x]);
}

// One workgroup: offs = the exclusive scan of the histogram (offs[bins] = the number of listed pixels), cursor = offs.
__global__ __launch_bounds__(256) void inpaint_scan_kernel(const int32_t* __restrict__ hist, int32_t* __restrict__ offs,
                                                           int32_t* __restrict__ cursor, int bins) {
    __shared__ int sums[256];
    const int chunk = (bins + 255) / 256;
    const int lo = min(bins, (int)threadIdx.x * chunk), hi = min(bins, lo + chunk);
    int cnt = 0;
    for (int i = lo; i < hi; ++i) cnt += hist[i];
    sums[threadIdx.x] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int v = sums[t];
            sums[t] = run;
            run += v;
        }
        offs[bins] = run;
    }
    __syncthreads();
    int run = sums[threadIdx.x];
    for (int i = lo; i < hi; ++i) {
        offs[i] = run;
        cursor[i] = run;
        run += hist[i];
    }
}

// One thread per pixel: a hole pixel goes into the list of its wave.  A workgroup reserves one range per wave (LDS
// counts, one global atomic per wave and workgroup), so the entries of 256 neighbouring pixels stay together.  The
// order inside a wave's list comes from atomics and is NOT deterministic; the output does not depend on it, because
// a fill never reads a pixel of its own wave.
__global__ __launch_bounds__(256) void inpaint_scatter_kernel(const uint16_t* __restrict__ wave, int32_t* __restrict__ cursor,
                                                              int32_t* __restrict__ list, int bins, long long npix) {
    __shared__ int local_count[kLocalBins], local_base[kLocalBins];
    if (threadIdx.x < kLocalBins) local_count[threadIdx.x] = 0;
    __syncthreads();
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int k = idx < npix ? wave[idx] : 0;
    int rank = 0;
    if (k > 0 && k < kLocalBins) rank = atomicAdd(&local_count[k], 1);
    __syncthreads();
    if (threadIdx.x < kLocalBins && threadIdx.x < bins && local_count[threadIdx.x])
        local_base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], local_count[threadIdx.x]);
    __syncthreads();
    if (k <= 0 || k >= bins) return;
    const int pos = k < kLocalBins ? local_base[k] + rank : atomicAdd(&cursor[k], 1);
    if (pos >= 0 && pos < npix) list[pos] = (int32_t)idx;
}

// ------------------------------------------------------------------------------------------------ fill
struct DstTable {
    float v[2 * kRadius + 1][2 * kRadius + 1];                // 1 / (d2 * sqrtf(d2)), built on the host
};

// the availability of the 9 x 9 pixels around p: the disc of radius 3 and the 4-neighbours of its pixels
struct Avail {
    uint64_t lo, hi;
    __device__ __forceinline__ void set(int bit) {
        if (bit < 64) lo |= 1ull << bit;
        else hi |= 1ull << (bit - 64);
    }
    __device__ __forceinline__ bool get(int dy, int dx) const {
        const int bit = (dy + kRadius + 1) * 9 + dx + kRadius + 1;
        return bit < 64 ? (lo >> bit) & 1 : (hi >> (bit - 64)) & 1;
    }
};

// the image gradient at q along one axis from the neighbours that are available (the factor 2 is Telea's)
__device__ __forceinline__ float grad_i(bool ap, bool am, float vp, float vq, float vm) {
    if (ap && am) return __fmul_rn(__fsub_rn(vp, vm), 2.0f);
    if (ap) return __fsub_rn(vp, vq);
    if (am) return __fsub_rn(vq, vm);
    return 0.0f;
}

// One thread per listed pixel of wave k, the channels in that thread.  In place: it reads pixels of waves < k and
// writes a pixel of wave k.
template <int C>
__global__ __launch_bounds__(256) void inpaint_fill_kernel(uint8_t* frames, const float* __restrict__ T,
                                                           const uint16_t* __restrict__ wave, const int32_t* __restrict__ list,
                                                           DstTable dst, int first, int count, int k, int h, int w, long long npix) {
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= count) return;
    const long long idx = list[first + item];
    if (idx < 0 || idx >= npix) return;
    const long long row = idx / w;
    const int x = (int)(idx - row * w);
    const int y = (int)(row % h);
    if (wave[idx] != k) return;

    Avail av = {0, 0};
#pragma unroll
    for (int dy = -kRadius - 1; dy <= kRadius + 1; ++dy)
#pragma unroll
        for (int dx = -kRadius - 1; dx <= kRadius + 1; ++dx) {
            if (dy * dy + dx * dx > (kRadius + 1) * (kRadius + 1)) continue;      // no disc pixel is next to these
            const int yy = y + dy, xx = x + dx;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w && wave[idx + (long long)dy * w + dx] < k)
                av.set((dy + kRadius + 1) * 9 + dx + kRadius + 1);
        }

    const float tp = T[idx];
    const float gtx = __fmul_rn(__fsub_rn(T[idx + (x + 1 < w ? 1 : 0)], T[idx - (x > 0 ? 1 : 0)]), 0.5f);
    const float gty = __fmul_rn(__fsub_rn(T[idx + (y + 1 < h ? w : 0)], T[idx - (y > 0 ? w : 0)]), 0.5f);
    float ia[C], jx[C], jy[C], s = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) ia[c] = jx[c] = jy[c] = 0.0f;

#pragma unroll
    for (int dy = -kRadius; dy <= kRadius; ++dy)
#pragma unroll
        for (int dx = -kRadius; dx <= kRadius; ++dx) {
            if (dy * dy + dx * dx == 0 || dy * dy + dx * dx > kRadius * kRadius) continue;
            if (!av.get(dy, dx)) continue;
            const long long q = idx + (long long)dy * w + dx;
            const float rx = (float)-dx, ry = (float)-dy;
            const float lev = __fdiv_rn(1.0f, __fadd_rn(1.0f, fabsf(__fsub_rn(T[q], tp))));
            float dir = __fadd_rn(__fmul_rn(rx, gtx), __fmul_rn(ry, gty));
            if (fabsf(dir) <= 0.01f) dir = 1e-6f;
            const float wgt = fabsf(__fmul_rn(__fmul_rn(dst.v[dy + kRadius][dx + kRadius], lev), dir));
            const bool axp = av.get(dy, dx + 1), axm = av.get(dy, dx - 1), ayp = av.get(dy + 1, dx), aym = av.get(dy - 1, dx);
            const uint8_t* pq = frames + q * C;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float vq = (float)pq[c];
                const float vxp = axp ? (float)pq[C + c] : 0.0f, vxm = axm ? (float)pq[c - C] : 0.0f;
                const float vyp = ayp ? (float)pq[(long long)w * C + c] : 0.0f, vym = aym ? (float)pq[c - (long long)w * C] : 0.0f;
                ia[c] = __fadd_rn(ia[c], __fmul_rn(wgt, vq));
                jx[c] = __fsub_rn(jx[c], __fmul_rn(__fmul_rn(wgt, grad_i(axp, axm, vxp, vq, vxm)), rx));
                jy[c] = __fsub_rn(jy[c], __fmul_rn(__fmul_rn(wgt, grad_i(ayp, aym, vyp, vq, vym)), ry));
            }
            s = __fadd_rn(s, wgt);
        }

    uint8_t res[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float norm = __fadd_rn(sqrtf(__fadd_rn(__fmul_rn(jx[c], jx[c]), __fmul_rn(jy[c], jy[c]))), 1e-20f);
        const float v = __fadd_rn(__fdiv_rn(ia[c], s), __fdiv_rn(__fadd_rn(jx[c], jy[c]), norm));
        res[c] = (uint8_t)fminf(fmaxf(rintf(v), 0.0f), 255.0f);                   // half to even, saturated
    }
    // s > 0 always; should it not be, v is NaN and the byte is 0 rather than anything out of bounds
#pragma unroll
    for (int c = 0; c < C; ++c) frames[idx * C + c] = res[c];
}

DstTable make_dst_table() {
    DstTable t;
    for (int dy = -kRadius; dy <= kRadius; ++dy)
        for (int dx = -kRadius; dx <= kRadius; ++dx) {
            const float d2 = (float)(dy * dy + dx * dx);
            t.v[dy + kRadius][dx + kRadius] = d2 > 0.0f ? 1.0f / (d2 * sqrtf(d2)) : 0.0f;
        }
    return t;
}

}  // namespace

extern "C" size_t elvis_inpaint_workspace_bytes(int n, int h, int w) {
    if (!shape_ok(n, h, w)) return 0;
    return carve(nullptr, (long long)n * h * w, h + w + 2).bytes;
}

extern "C" int elvis_inpaint_prepare(const uint8_t* mask, int block_size, void* workspace, int n, int h, int w,
                                     elvis_stream_t stream) {
    ELVIS_REQUIRE(mask && workspace, "elvis_inpaint_prepare: null pointer");
    ELVIS_REQUIRE(shape_ok(n, h, w), "elvis_inpaint_prepare: bad shape n=%d h=%d w=%d", n, h, w);
    ELVIS_REQUIRE(block_size >= 0, "elvis_inpaint_prepare: block_size %d must be 0 (a mask per pixel) or positive", block_size);
    ELVIS_REQUIRE((uintptr_t)workspace % 256 == 0, "elvis_inpaint_prepare: the workspace must be 256-byte aligned");
    const long long npix = (long long)n * h * w;
    const int bins = h + w + 2;
    const Workspace ws = carve(workspace, npix, bins);
    MaskView mv = {mask, block_size, block_size ? h / block_size : 0, block_size ? w / block_size : 0};
    hipStream_t st = (hipStream_t)stream;
    const unsigned pixel_grid = (unsigned)((npix + 255) / 256);
    hipLaunchKernelGGL(inpaint_rows_kernel, dim3((unsigned)(n * h)), dim3(256), 0, st, mv, ws.rowdist, ws.hist, bins, h, w);
    ELVIS_CHECK_LAUNCH("elvis_inpaint_prepare");
    hipLaunchKernelGGL(inpaint_columns_kernel, dim3(pixel_grid), dim3(256), 0, st, mv, ws.rowdist, ws.T, ws.wave, ws.hist, bins, h, w, npix);
    ELVIS_CHECK_LAUNCH("elvis_inpaint_prepare");
    hipLaunchKernelGGL(inpaint_scan_kernel, dim3(1), dim3(256), 0, st, ws.hist, ws.offs, ws.cursor, bins);
    ELVIS_CHECK_LAUNCH("elvis_inpaint_prepare");
    hipLaunchKernelGGL(inpaint_scatter_kernel, dim3(pixel_grid), dim3(256), 0, st, ws.wave, ws.cursor, ws.list, bins, npix);
    ELVIS_CHECK_LAUNCH("elvis_inpaint_prepare");
    elvis_note_launch("inpaint_scatter_kernel");
    return ELVIS_OK;
}

extern "C" int elvis_inpaint_fill(uint8_t* frames, const void* workspace, int n, int h, int w, int c,
                                  const int32_t* wave_counts_host, int num_counts, elvis_stream_t stream) {
    ELVIS_REQUIRE(frames && workspace && wave_counts_host, "elvis_inpaint_fill: null pointer");
    ELVIS_REQUIRE(shape_ok(n, h, w), "elvis_inpaint_fill: bad shape n=%d h=%d w=%d", n, h, w);
    ELVIS_REQUIRE(c == 1 || c == 3, "elvis_inpaint_fill: %d channels (1 or 3 supported)", c);
    ELVIS_REQUIRE((uintptr_t)workspace % 256 == 0, "elvis_inpaint_fill: the workspace must be 256-byte aligned");
    const long long npix = (long long)n * h * w;
    const int bins = h + w + 2;
    ELVIS_REQUIRE(num_counts >= 1 && num_counts <= bins, "elvis_inpaint_fill: %d wave counts outside [1, %d]", num_counts, bins);
    long long total = 0;
    for (int k = 0; k < num_counts; ++k) {
        ELVIS_REQUIRE(wave_counts_host[k] >= 0, "elvis_inpaint_fill: negative count of wave %d", k);
        total += wave_counts_host[k];
    }
    ELVIS_REQUIRE(wave_counts_host[0] == 0 && total <= npix, "elvis_inpaint_fill: the wave counts are not those of this clip");
    const Workspace ws = carve(const_cast<void*>(workspace), npix, bins);
    static const DstTable dst = make_dst_table();
    int first = 0;
    for (int k = 1; k < num_counts; ++k) {
        const int count = wave_counts_host[k];
        if (count > 0) {
            const dim3 grid((unsigned)((count + 255) / 256));
            if (c == 3)
                hipLaunchKernelGGL(inpaint_fill_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, frames, ws.T, ws.wave, ws.list, dst,
                                   first, count, k, h, w, npix);
            else
                hipLaunchKernelGGL(inpaint_fill_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, frames, ws.T, ws.wave, ws.list, dst,
                                   first, count, k, h, w, npix);
            ELVIS_CHECK_LAUNCH("elvis_inpaint_fill");
            elvis_note_launch(c == 3 ? "inpaint_fill_kernel<3>" : "inpaint_fill_kernel<1>");
        }
        first += count;
    }
    return ELVIS_OK;
}
