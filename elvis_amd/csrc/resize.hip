// Clip intake on the device: what resizes a decoded clip to the working size before any other stage reads it.
//   elvis_resize_area_u8    - cv2.resize(frame, (width, height), interpolation=cv2.INTER_AREA) of every frame of a clip
//                             (presley.py:186), down or equal on both axes, in one launch
//   elvis_resize_nearest_u8 - cv2.resize(mask, (w, h), interpolation=cv2.INTER_NEAREST) (presley.py:427, 846, 867, 884,
//                             elvis.py:206, 564, 4578): destination d reads source floor(d * src / dst), up or down
// OpenCV is absent from the build and GPU environments, so its rules are restated from OpenCV 4.x ("parity
// unpinned"); what is pinned is bit-exactness against the numpy statement in tests/_resize_ref.py.
//
// INTER_AREA.  Each axis has a table (degrade.area_table, = cv::computeResizeAreaTab): destination d covers the
// consecutive source indices first[d] .. first[d] + (start[d + 1] - start[d]) - 1 with the float32 weights
// w[start[d] ..].  Both ratios whole: the integer box sum, (sum + 2) >> 2 at 2x2, otherwise
// rint(float(sum) * float(1.0 / area)), half to even (cv::resizeAreaFast_); the weights are not read.  Otherwise
// cv::ResizeArea_<uchar, float>: buf = sum over the x entries of S * alpha, sum = sum over the y entries of beta * buf,
// float32 from 0 in table order, every product rounded before it is added (explicit round-to-nearest intrinsics; the
// library is built with -ffp-contract=off), then rint and the clip to [0, 255].
//
// One workgroup of 256 threads owns a tile of th x tw destination pixels of one frame, at most kAreaValues values, up to
// four per thread in registers.  A destination value is its own ordered sum and depends on no other, so the tiling
// cannot change the bytes.  The source rows the tile needs are streamed through LDS, rows_per_chunk at a time, in
// ascending order - the order of the y table - so a thread takes the entries of its values as their rows come by; no
// loop has a bound other than the table's.  A row is staged with dword loads where the dword lies whole inside the
// row's segment and byte by byte at its two ends: nothing outside the segment is read.  Neighbouring tiles re-read the
// one source row or column a fractional boundary shares.  Where one destination pixel's segment of a source row does
// not fit the LDS (tens of thousands of source columns per destination column) the same loops read the source in
// place (row_stride 0).
// LDS banks: lanes take consecutive destination values, so at every table entry a wave reads bytes that lie
// fx * c (fractional: about that) apart per pixel and one apart per channel: at the ratios of a working size (1.5 to
// 3) a wave's 64 byte reads fall into 24 to 48 consecutive dwords, lanes sharing a dword are one broadcast.  Not measured
// with counters.
#include "common.h"

namespace {

constexpr int kAreaThreads = 256;
constexpr int kAreaPerThread = 4;
constexpr int kAreaValues = kAreaThreads * kAreaPerThread;   // destination values (pixel x channel) of a tile, at most
constexpr int kAreaLdsLimit = 64 * 1024;                     // dynamic LDS without the opt-in

struct AxisTab {
    const int32_t* start;   // [dst + 1] first table entry of destination d (and the end)
    const int32_t* first;   // [dst]     source index of that entry; the entries of d are consecutive source indices
    const float* w;         // [start[dst]]
};

__device__ __forceinline__ int last_source(const AxisTab& t, int d) { return t.first[d] + (t.start[d + 1] - t.start[d]) - 1; }

template <bool WHOLE, bool DIRECT>
__global__ __launch_bounds__(kAreaThreads) void resize_area_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int hs,
                                                                   int ws, int hd, int wd, int c, AxisTab xt, AxisTab yt, int th,
                                                                   int tw, int tiles_y, int tiles_x, int rows_per_chunk,
                                                                   int row_stride, int two_by_two, float inv) {
    extern __shared__ int lds[];
    uint8_t* tile = (uint8_t*)lds;
    const int t = blockIdx.x;
    const int txi = t % tiles_x;
    const int tyi = (t / tiles_x) % tiles_y;
    const int f = t / (tiles_x * tiles_y);
    const int ty0 = tyi * th, tx0 = txi * tw;
    const int ty1 = ty0 + th < hd ? ty0 + th : hd, tx1 = tx0 + tw < wd ? tx0 + tw : wd;
    const int sx_lo = xt.first[tx0], sx_hi = last_source(xt, tx1 - 1);
    const int sy_lo = yt.first[ty0], sy_hi = last_source(yt, ty1 - 1);
    const int seg = (sx_hi - sx_lo + 1) * c;                      // bytes of a source row this tile reads
    const long long rs = (long long)ws * c;
    const uint8_t* fsrc = src + (long long)f * hs * rs + (long long)sx_lo * c;   // row sy of the segment: fsrc + sy * rs
    const int rowvals = (tx1 - tx0) * c;
    const int nvals = (ty1 - ty0) * rowvals;

    // this thread's destination values: where their y entries stand, their x entries, their running sums
    int ky[kAreaPerThread], ky_end[kAreaPerThread], sy_next[kAreaPerThread], xa[kAreaPerThread], xn[kAreaPerThread], coff[kAreaPerThread];
    float fsum[kAreaPerThread];
    unsigned long long isum[kAreaPerThread];
#pragma unroll
    for (int v = 0; v < kAreaPerThread; ++v) {
        const int e = threadIdx.x + v * kAreaThreads;
        ky[v] = ky_end[v] = sy_next[v] = xa[v] = xn[v] = coff[v] = 0;
        fsum[v] = 0.f;
        isum[v] = 0;
        if (e < nvals) {
            const int ly = e / rowvals;
            const int xc = e - ly * rowvals;
            const int lx = xc / c;
            const int dy = ty0 + ly, dx = tx0 + lx;
            ky[v] = yt.start[dy];
            ky_end[v] = yt.start[dy + 1];
            sy_next[v] = yt.first[dy];
            xa[v] = xt.start[dx];
            xn[v] = xt.start[dx + 1] - xa[v];
            coff[v] = (xt.first[dx] - sx_lo) * c + (xc - lx * c);
        }
    }

    const int step = DIRECT ? sy_hi - sy_lo + 1 : rows_per_chunk;
    for (int r0 = sy_lo; r0 <= sy_hi; r0 += step) {
        const int r1 = r0 + step < sy_hi + 1 ? r0 + step : sy_hi + 1;
        if (!DIRECT) {
            // one wave per row; LDS dword j of a row holds the global dword of the same alignment
            for (int r = r0 + (int)(threadIdx.x >> 6); r < r1; r += kAreaThreads / ELVIS_WAVE) {
                const uint8_t* g = fsrc + (long long)r * rs;
                const int pad = (int)((uintptr_t)g & 3);
                uint8_t* lrow = tile + (size_t)(r - r0) * row_stride;
                const int ndw = (pad + seg + 3) >> 2;
                for (int j = threadIdx.x & 63; j < ndw; j += ELVIS_WAVE) {
                    const int lo = 4 * j - pad;                    // the segment byte this dword starts at
                    if (lo >= 0 && lo + 4 <= seg) {
                        *(uint32_t*)(lrow + 4 * j) = *(const uint32_t*)(g + lo);
                    } else {
                        for (int b = 0; b < 4; ++b)
                            if (lo + b >= 0 && lo + b < seg) lrow[4 * j + b] = g[lo + b];
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int v = 0; v < kAreaPerThread; ++v) {
            while (ky[v] < ky_end[v] && sy_next[v] < r1) {
                const uint8_t* g = fsrc + (long long)sy_next[v] * rs;
                const uint8_t* row = DIRECT ? g + coff[v] : tile + (size_t)(sy_next[v] - r0) * row_stride + ((uintptr_t)g & 3) + coff[v];
                if (WHOLE) {
                    for (int j = 0; j < xn[v]; ++j) isum[v] += row[j * c];
                } else {
                    float buf = 0.f;
                    for (int j = 0; j < xn[v]; ++j) buf = __fadd_rn(buf, __fmul_rn((float)row[j * c], xt.w[xa[v] + j]));
                    fsum[v] = __fadd_rn(fsum[v], __fmul_rn(yt.w[ky[v]], buf));
                }
                ++ky[v];
                ++sy_next[v];
            }
        }
        if (!DIRECT) __syncthreads();
    }

    uint8_t* fdst = dst + ((long long)f * hd * wd + (long long)tx0) * c;
#pragma unroll
    for (int v = 0; v < kAreaPerThread; ++v) {
        const int e = threadIdx.x + v * kAreaThreads;
        if (e >= nvals) continue;
        const int ly = e / rowvals;
        int r;
        if (WHOLE) {
            const unsigned long long s = isum[v];
            r = two_by_two ? (int)((s + 2) >> 2) : __float2int_rn(__fmul_rn((float)s, inv));   // 1x1: inv is 1, the copy
        } else {
            r = __float2int_rn(fsum[v]);
        }
        fdst[(long long)(ty0 + ly) * wd * c + (e - ly * rowvals)] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
    }
}

// One workgroup per destination row of a frame, lanes strided over its pixel x channel values
__global__ __launch_bounds__(256) void resize_nearest_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int hs, int ws,
                                                             int hd, int wd, int c) {
    const long long row = blockIdx.x;                              // f * hd + dy
    const long long f = row / hd;
    const int dy = (int)(row - f * hd);
    const int sy = (int)((long long)dy * hs / hd);
    const uint8_t* srow = src + (f * hs + sy) * (long long)ws * c;
    uint8_t* drow = dst + row * (long long)wd * c;
    for (long long xc = threadIdx.x; xc < (long long)wd * c; xc += blockDim.x) {
        const long long dx = xc / c;
        drow[xc] = srow[dx * ws / wd * c + (xc - dx * c)];
    }
}

// Host: one axis of the tables as the kernel reads it - every destination has entries, they stay inside the source and
// never step back; at a whole ratio f destination d is exactly the f sources from d * f.  Returns the ratio's message or 0.
const char* check_axis(const int32_t* start, const int32_t* first, int src_n, int dst_n, bool whole) {
    if (start[0] != 0) return "the table does not start at entry 0";
    const int fac = src_n / dst_n;
    int last_before = -1, first_before = 0;
    for (int d = 0; d < dst_n; ++d) {
        const long long cnt = (long long)start[d + 1] - start[d];
        if (cnt < 1 || cnt > src_n) return "a destination index without table entries";
        if (first[d] < first_before || (long long)first[d] + cnt > src_n) return "table entries outside the source";
        const int last = first[d] + (int)cnt - 1;
        if (last < last_before) return "table entries that step back";
        if (whole && (cnt != fac || first[d] != d * fac)) return "a whole ratio whose table is not the box";
        first_before = first[d];
        last_before = last;
    }
    return nullptr;
}

// the most source indices a tile of `span` destination indices reads
int tile_reach(const int32_t* start, const int32_t* first, int dst_n, int span) {
    int reach = 0;
    for (int d0 = 0; d0 < dst_n; d0 += span) {
        const int d1 = (d0 + span < dst_n ? d0 + span : dst_n) - 1;
        const int r = first[d1] + (start[d1 + 1] - start[d1]) - first[d0];
        reach = r > reach ? r : reach;
    }
    return reach;
}

}  // namespace

extern "C" int elvis_resize_area_u8(const uint8_t* src, uint8_t* dst, int n, int hs, int ws, int hd, int wd, int c,
                                    const int32_t* xstart_h, const int32_t* xfirst_h, const int32_t* ystart_h,
                                    const int32_t* yfirst_h, const int32_t* xstart, const int32_t* xfirst, const float* xw,
                                    const int32_t* ystart, const int32_t* yfirst, const float* yw, int th, int tw,
                                    int rows_per_chunk, int row_stride, elvis_stream_t stream) {
    const char* who = "elvis_resize_area_u8";
    ELVIS_REQUIRE(src && dst && xstart_h && xfirst_h && ystart_h && yfirst_h && xstart && xfirst && xw && ystart && yfirst && yw,
                  "%s: null pointer", who);
    ELVIS_REQUIRE(n > 0 && hs > 0 && ws > 0 && hd > 0 && wd > 0, "%s: bad shape", who);
    ELVIS_REQUIRE(c == 1 || c == 3 || c == 4, "%s: %d channels (1, 3 or 4 supported)", who, c);
    ELVIS_REQUIRE(hd <= hs, "%s: the destination height %d is larger than the source height %d (upscaling is not INTER_AREA's box rule)", who, hd, hs);
    ELVIS_REQUIRE(wd <= ws, "%s: the destination width %d is larger than the source width %d (upscaling is not INTER_AREA's box rule)", who, wd, ws);
    ELVIS_REQUIRE((long long)ws * c < (1LL << 31) && (long long)wd * c < (1LL << 31), "%s: a row of 2^31 bytes or more", who);
    const bool whole = hs % hd == 0 && ws % wd == 0;
    const char* bad = check_axis(xstart_h, xfirst_h, ws, wd, whole);
    ELVIS_REQUIRE(!bad, "%s: x table: %s", who, bad);
    bad = check_axis(ystart_h, yfirst_h, hs, hd, whole);
    ELVIS_REQUIRE(!bad, "%s: y table: %s", who, bad);
    ELVIS_REQUIRE(th >= 1 && tw >= 1 && (long long)th * tw * c <= kAreaValues, "%s: a %dx%d tile of %d channels holds more than %d values",
                  who, th, tw, c, kAreaValues);
    const bool direct = row_stride == 0;
    size_t shmem = 0;
    if (!direct) {
        const long long seg = (long long)tile_reach(xstart_h, xfirst_h, wd, tw) * c;
        ELVIS_REQUIRE(row_stride % 4 == 0 && row_stride >= seg + 3, "%s: row_stride %d does not hold a %lld-byte segment at any alignment",
                      who, row_stride, seg);
        ELVIS_REQUIRE(rows_per_chunk >= 1 && (long long)rows_per_chunk * row_stride <= kAreaLdsLimit,
                      "%s: %d rows of %d bytes do not fit %d bytes of LDS", who, rows_per_chunk, row_stride, kAreaLdsLimit);
        shmem = (size_t)rows_per_chunk * row_stride;
    }
    const int tiles_y = cdiv(hd, th), tiles_x = cdiv(wd, tw);
    ELVIS_REQUIRE((long long)n * tiles_y * tiles_x < (1LL << 31), "%s: too many tiles", who);
    const dim3 grid((unsigned)(n * tiles_y * tiles_x)), block(kAreaThreads);
    const AxisTab xt{xstart, xfirst, xw}, yt{ystart, yfirst, yw};
    const int fy = hs / hd, fx = ws / wd;
    const float inv = (float)(1.0 / ((double)fx * (double)fy));
    const int two = whole && fx == 2 && fy == 2;
#define ELVIS_AREA_LAUNCH(W, D)                                                                                                    \
    hipLaunchKernelGGL((resize_area_kernel<W, D>), grid, block, shmem, (hipStream_t)stream, src, dst, hs, ws, hd, wd, c, xt, yt, th, \
                       tw, tiles_y, tiles_x, rows_per_chunk, row_stride, two, inv)
    if (whole && direct) ELVIS_AREA_LAUNCH(true, true);
    else if (whole) ELVIS_AREA_LAUNCH(true, false);
    else if (direct) ELVIS_AREA_LAUNCH(false, true);
    else ELVIS_AREA_LAUNCH(false, false);
#undef ELVIS_AREA_LAUNCH
    ELVIS_CHECK_LAUNCH(who);
    elvis_note_launch(whole ? (direct ? "resize_area_kernel<whole,direct>" : "resize_area_kernel<whole,lds>")
                            : (direct ? "resize_area_kernel<frac,direct>" : "resize_area_kernel<frac,lds>"));
    return ELVIS_OK;
}

extern "C" int elvis_resize_nearest_u8(const uint8_t* src, uint8_t* dst, int n, int hs, int ws, int hd, int wd, int c,
                                       elvis_stream_t stream) {
    const char* who = "elvis_resize_nearest_u8";
    ELVIS_REQUIRE(src && dst, "%s: null pointer", who);
    ELVIS_REQUIRE(n > 0 && hs > 0 && ws > 0 && hd > 0 && wd > 0, "%s: bad shape", who);
    ELVIS_REQUIRE(c == 1 || c == 3 || c == 4, "%s: %d channels (1, 3 or 4 supported)", who, c);
    ELVIS_REQUIRE((long long)n * hd < (1LL << 31), "%s: too many rows", who);
    hipLaunchKernelGGL(resize_nearest_kernel, dim3((unsigned)(n * hd)), dim3(256), 0, (hipStream_t)stream, src, dst, hs, ws, hd, wd, c);
    ELVIS_CHECK_LAUNCH(who);
    elvis_note_launch("resize_nearest_kernel");
    return ELVIS_OK;
}
