// ELVIS v1 block removal on the device: the server removes the least important blocks of a frame ("shrink"), the
// client puts the kept blocks back where they came from ("stretch") and hands the frame plus a hole mask to an
// inpainter.  Every shrink and every stretch of the reference is ONE block gather driven by an index map:
//   elvis_block_gather_u8       - dst[n, by, bx] = src[n, src_of[n, by, bx]], a zero block where src_of < 0, and
//                                 optionally the full-resolution 0/255 hole mask in the same launch
//   elvis_shrink_select_topk    - apply_selective_removal (elvis.py:1387-1427): per block row the k highest scores go
//   elvis_shrink_select_passes  - shrink_frame_row_only / _position_map / _removal_indices (utils.py:692-948):
//                                 alternating passes that remove each row's (column's) current argmin and shift
//   elvis_stretch_index         - the rank of the kept blocks, flat (stretch_frame elvis.py:1436-1455,
//                                 stretch_video_frames presley.py:787-827) or per row (stretch_frame_row_only
//                                 utils.py:739-759): the index map of a stretch whose side data is a mask
//   elvis_shrink_passes_plan    - host only: the shrunk grid and the per-pass removal counts, a function of
//                                 (by, bx, target, mode) alone, so every output is allocated before the launch
// Scores are float64 and are only ever compared (no arithmetic, no down-cast): ties are exactly the reference's.
#include <limits.h>
#include "common.h"

namespace {

constexpr int kModeRows = 0;      // ELVIS_SHRINK_ROWS
constexpr int kModeRowsCols = 1;  // ELVIS_SHRINK_ROWS_COLS
constexpr int kRankFlat = 0;      // ELVIS_STRETCH_FLAT
constexpr int kRankRows = 1;      // ELVIS_STRETCH_ROWS

// ------------------------------------------------------------------------------------------------ gather
__device__ __forceinline__ void move_bytes(uint8_t* __restrict__ d, const uint8_t* __restrict__ s, int vw, bool zero,
                                           uint32_t fill) {
    switch (vw) {
        case 16: {
            uint4 v = make_uint4(fill, fill, fill, fill);
            if (!zero) v = *reinterpret_cast<const uint4*>(s);
            *reinterpret_cast<uint4*>(d) = v;
            break;
        }
        case 8: {
            uint2 v = make_uint2(fill, fill);
            if (!zero) v = *reinterpret_cast<const uint2*>(s);
            *reinterpret_cast<uint2*>(d) = v;
            break;
        }
        case 4: {
            uint32_t v = fill;
            if (!zero) v = *reinterpret_cast<const uint32_t*>(s);
            *reinterpret_cast<uint32_t*>(d) = v;
            break;
        }
        default: *d = zero ? (uint8_t)fill : *s;
    }
}

// One work item = one vector of `vf` bytes of a destination frame row (items [0, nvec_f)) or of `vm` bytes of a
// full-resolution mask row (items [nvec_f, nvec_f + nvec_m)).  A block's row segment (block * c bytes in a frame,
// block bytes in the mask) is a whole number of vectors, so a vector lies in one block: one map look-up, one load,
// one store.  vf = vm = 1 is the per-byte form for segments and pitches that allow nothing wider.
__global__ __launch_bounds__(256) void block_gather_u8_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ src_of,
                                                              uint8_t* __restrict__ dst, uint8_t* __restrict__ mask, int hs,
                                                              int ws, int c, int block, int sby, int sbx, int dby, int dbx,
                                                              int vf, int vm, long long nvec_f, long long nvec_m) {
    const int hd = dby * block;
    const int nsrc = sby * sbx;
    const long long src_row = (long long)ws * c;
    for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x; item < nvec_f + nvec_m;
         item += (long long)gridDim.x * blockDim.x) {
        const bool is_mask = item >= nvec_f;
        const long long v = is_mask ? item - nvec_f : item;
        const int seg = is_mask ? block : block * c;          // bytes of one block in a row of this plane
        const int vw = is_mask ? vm : vf;
        const int vec_per_row = dbx * seg / vw;
        const long long row = v / vec_per_row;                // = f * hd + y
        const int o = (int)(v - row * vec_per_row) * vw;      // byte offset inside the row
        const int f = (int)(row / hd), y = (int)(row - (long long)f * hd);
        const int byi = y / block, iy = y - byi * block;
        const int bxi = o / seg, io = o - bxi * seg;
        const int s = src_of[((long long)f * dby + byi) * dbx + bxi];
        const bool hole = s < 0 || s >= nsrc;                 // an index outside the source grid is never read
        uint8_t* d = (is_mask ? mask : dst) + row * ((long long)dbx * seg) + o;
        if (is_mask) {
            move_bytes(d, nullptr, vw, true, hole ? 0xFFFFFFFFu : 0u);
        } else {
            const int sy = hole ? 0 : s / sbx, sx = hole ? 0 : s - sy * sbx;
            const uint8_t* p = src + ((long long)f * hs + (long long)sy * block + iy) * src_row + (long long)sx * seg + io;
            move_bytes(d, p, vw, hole, 0u);
        }
    }
}

int widest_vector(long long seg, long long pitch, uintptr_t bits) {
    for (int v = 16; v > 1; v >>= 1)
        if (v >= 4 && seg % v == 0 && pitch % v == 0 && bits % v == 0) return v;
    return 1;
}

// ------------------------------------------------------------------------------------------------ top-k rule
// One workgroup per block row.  Column i is removed iff fewer than k columns j beat it (s_j > s_i, or s_j == s_i
// and j < i): the k highest scores, the lower column first among equals.  The kept columns keep their order.
__global__ __launch_bounds__(256) void shrink_select_topk_kernel(const double* __restrict__ scores, int8_t* mask,
                                                                 int32_t* __restrict__ src_of, int by, int bx, int k) {
    const long long row = blockIdx.x;                         // f * by + r
    const int r = (int)(row % by);
    const double* s = scores + row * bx;
    int8_t* m = mask + row * bx;
    for (int i = threadIdx.x; i < bx; i += blockDim.x) {
        const double si = s[i];
        int beat = 0;
        for (int j = 0; j < bx; ++j) {
            const double sj = s[j];
            beat += (sj > si || (sj == si && j < i)) ? 1 : 0;
        }
        m[i] = beat < k ? 1 : 0;
    }
    __syncthreads();
    const int sbx = bx - k;
    for (int i = threadIdx.x; i < bx; i += blockDim.x) {
        if (m[i]) continue;
        int pos = 0;
        for (int j = 0; j < i; ++j) pos += m[j] ? 0 : 1;
        src_of[row * sbx + pos] = r * bx + i;
    }
}

// ------------------------------------------------------------------------------------------------ pass rule
// First index of the minimum of `len` doubles at stride `stride`, by one wave (every lane gets the result).
__device__ __forceinline__ int wave_argmin_first(const volatile double* p, int len, int stride, int lane) {
    double bv = 0.0;
    int bi = INT_MAX;
    for (int i = lane; i < len; i += ELVIS_WAVE) {
        const double v = p[(long long)i * stride];
        if (bi == INT_MAX || v < bv) { bv = v; bi = i; }      // ascending i: an equal value keeps the earlier index
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, ELVIS_WAVE);
        const int oi = __shfl_xor(bi, o, ELVIS_WAVE);
        if (oi != INT_MAX && (bi == INT_MAX || ov < bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    return bi;
}

// Elements idx+1 .. len-1 of a strided line move down by one, scores and positions together.  One wave, 64 elements
// per step in ascending order: a step's loads (wave-wide) complete before its stores, and the element the next step
// overwrites first was loaded by this step's last lane.  The pointers are volatile so that the compiler keeps that order.
__device__ __forceinline__ void wave_shift_down(volatile double* sc, volatile int32_t* pos, int idx, int len, int stride, int lane) {
    for (int p = idx + lane; p < len - 1; p += ELVIS_WAVE) {
        const double v = sc[(long long)(p + 1) * stride];
        const int32_t q = pos[(long long)(p + 1) * stride];
        sc[(long long)p * stride] = v;
        pos[(long long)p * stride] = q;
    }
}

// One workgroup per frame, one wave per row (column) inside a pass.  The working copy of the scores and the position
// map live in a caller-provided workspace (2 x by x bx entries per frame, L2-resident: 389 KB per 1080p / block 8
// frame does not fit the 160 KB of LDS, and one code path for every grid keeps the partial-pass rule in one place).
__global__ __launch_bounds__(1024) void shrink_select_passes_kernel(const double* __restrict__ scores, uint8_t* mask,
                                                                    int32_t* __restrict__ src_of, int32_t* __restrict__ removal_idx,
                                                                    double* ws_scores, int32_t* ws_pos, int by, int bx,
                                                                    int target, int mode, int sby, int sbx) {
    const int f = blockIdx.x;
    const long long cells = (long long)by * bx;
    volatile double* sc = ws_scores + f * cells;
    volatile int32_t* pos = ws_pos + f * cells;
    uint8_t* m = mask + f * cells;
    int32_t* ridx = removal_idx ? removal_idx + (long long)f * target : nullptr;
    for (long long e = threadIdx.x; e < cells; e += blockDim.x) {
        sc[e] = scores[f * cells + e];
        pos[e] = (int32_t)e;
        m[e] = 0;
    }
    __syncthreads();
    const int lane = threadIdx.x & (ELVIS_WAVE - 1), wave = threadIdx.x / ELVIS_WAVE, nwaves = blockDim.x / ELVIS_WAVE;
    int cur_by = by, cur_bx = bx, removed = 0;
    while (removed < target && cur_by > 0 && cur_bx > 0 && (mode == kModeRowsCols || cur_bx > 1)) {
        // row pass: the first `cnt` rows lose their argmin; the width shrinks after a whole pass - and, in the
        // rows-only form, after a partial one too (rows the pass did not reach lose their last block unmasked)
        int cnt = min(cur_by, target - removed);
        for (int r = wave; r < cnt; r += nwaves) {
            const int idx = wave_argmin_first(sc + (long long)r * bx, cur_bx, 1, lane);
            if (lane == 0) {
                m[pos[(long long)r * bx + idx]] = 1;
                if (ridx) ridx[removed + r] = idx;
            }
            wave_shift_down(sc + (long long)r * bx, pos + (long long)r * bx, idx, cur_bx, 1, lane);
        }
        removed += cnt;
        if (mode == kModeRows || cnt == cur_by) --cur_bx;
        __syncthreads();
        if (mode != kModeRowsCols || removed >= target || cur_bx <= 0) continue;
        // column pass: the first `cnt` columns lose their argmin and shift up; the height shrinks after a whole pass only
        cnt = min(cur_bx, target - removed);
        for (int col = wave; col < cnt; col += nwaves) {
            const int idx = wave_argmin_first(sc + col, cur_by, bx, lane);
            if (lane == 0) {
                m[pos[(long long)idx * bx + col]] = 1;
                if (ridx) ridx[removed + col] = idx;
            }
            wave_shift_down(sc + col, pos + col, idx, cur_by, bx, lane);
        }
        removed += cnt;
        if (cnt == cur_bx) --cur_by;
        __syncthreads();
    }
    // the position map of the shrunk grid (after a partial pass it still holds the stale last entries of the lines
    // that were shifted, as the reference's does)
    for (int e = threadIdx.x; e < sby * sbx; e += blockDim.x) {
        const int y = e / sbx, x = e - y * sbx;
        src_of[(long long)f * sby * sbx + e] = pos[(long long)y * bx + x];
    }
}

// the host-side mirror of the loop above: grid after the passes and the removals of each pass
int passes_plan(int by, int bx, int target, int mode, int* sby, int* sbx, int* counts, int max_passes) {
    int cur_by = by, cur_bx = bx, removed = 0, np = 0;
    while (removed < target && cur_by > 0 && cur_bx > 0 && (mode == kModeRowsCols || cur_bx > 1)) {
        int cnt = cur_by < target - removed ? cur_by : target - removed;
        if (counts && np < max_passes) counts[np] = cnt;
        ++np;
        removed += cnt;
        if (mode == kModeRows || cnt == cur_by) --cur_bx;
        if (mode != kModeRowsCols || removed >= target || cur_bx <= 0) continue;
        cnt = cur_bx < target - removed ? cur_bx : target - removed;
        if (counts && np < max_passes) counts[np] = cnt;
        ++np;
        removed += cnt;
        if (cnt == cur_bx) --cur_by;
    }
    *sby = cur_by;
    *sbx = cur_bx;
    return np;
}

// ------------------------------------------------------------------------------------------------ ranks of the kept blocks
// One workgroup per segment (a frame in the flat form, a block row in the per-row form): an exclusive scan of the
// kept flags.  src_of = offset + rank for a kept block whose rank is inside the shrunk grid, -1 otherwise.
__global__ __launch_bounds__(256) void stretch_index_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ src_of, int by,
                                                            int bx, int sby, int sbx, int mode) {
    __shared__ int sums[256];
    const long long seg = blockIdx.x;
    int len, off, limit;
    if (mode == kRankFlat) {
        len = by * bx;
        off = 0;
        limit = sby * sbx;
    } else {
        const int r = (int)(seg % by);
        len = bx;
        off = r * sbx;
        limit = r < sby ? sbx : 0;
    }
    const uint8_t* m = mask + seg * len;
    int32_t* out = src_of + seg * len;
    const int chunk = (len + 255) / 256;
    const int lo = min(len, (int)threadIdx.x * chunk), hi = min(len, lo + chunk);
    int cnt = 0;
    for (int i = lo; i < hi; ++i) cnt += m[i] ? 0 : 1;
    sums[threadIdx.x] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int v = sums[t];
            sums[t] = run;
            run += v;
        }
    }
    __syncthreads();
    int rank = sums[threadIdx.x];
    for (int i = lo; i < hi; ++i) {
        int v = -1;
        if (!m[i]) {
            if (rank < limit) v = off + rank;
            ++rank;
        }
        out[i] = v;
    }
}

}  // namespace

extern "C" int elvis_block_gather_u8(const uint8_t* src, const int32_t* src_of, uint8_t* dst, uint8_t* mask_out, int n, int hs,
                                     int ws, int c, int block, int sby, int sbx, int dby, int dbx, elvis_stream_t stream) {
    ELVIS_REQUIRE(src_of && dst, "elvis_block_gather_u8: null pointer");
    ELVIS_REQUIRE(block >= 1, "elvis_block_gather_u8: block_size %d must be at least 1", block);
    ELVIS_REQUIRE(c == 1 || c == 3, "elvis_block_gather_u8: %d channels (1 or 3 supported)", c);
    ELVIS_REQUIRE(n > 0 && dby > 0 && dbx > 0 && sby >= 0 && sbx >= 0 && hs >= 0 && ws >= 0,
                  "elvis_block_gather_u8: bad shape n=%d source grid %dx%d destination grid %dx%d", n, sby, sbx, dby, dbx);
    ELVIS_REQUIRE((long long)sby * block <= hs && (long long)sbx * block <= ws,
                  "elvis_block_gather_u8: a source grid of %dx%d blocks of %d does not fit a %dx%d frame", sby, sbx, block, hs, ws);
    ELVIS_REQUIRE(src || sby == 0 || sbx == 0, "elvis_block_gather_u8: null pointer");
    ELVIS_REQUIRE((long long)n * dby * dbx < (1LL << 31) && (long long)sby * sbx < (1LL << 31) &&
                      (long long)dby * block < (1LL << 31) && (long long)dbx * block * c < (1LL << 31),
                  "elvis_block_gather_u8: too many blocks");
    const long long seg = (long long)block * c;
    const int vf = widest_vector(seg, (long long)ws * c, (uintptr_t)src | (uintptr_t)dst);
    const int vm = mask_out ? widest_vector(block, 0, (uintptr_t)mask_out) : 1;
    const long long rows = (long long)n * dby * block;
    const long long nvec_f = rows * (dbx * seg / vf);
    const long long nvec_m = mask_out ? rows * ((long long)dbx * block / vm) : 0;
    long long grid = (nvec_f + nvec_m + 255) / 256;
    if (grid > 256 * 32) grid = 256 * 32;
    hipLaunchKernelGGL(block_gather_u8_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, src, src_of, dst, mask_out,
                       hs, ws, c, block, sby, sbx, dby, dbx, vf, vm, nvec_f, nvec_m);
    ELVIS_CHECK_LAUNCH("elvis_block_gather_u8");
    elvis_note_launch(vf == 16 ? "block_gather_u8_kernel<16>" : vf == 8 ? "block_gather_u8_kernel<8>"
                      : vf == 4 ? "block_gather_u8_kernel<4>" : "block_gather_u8_kernel<1>");
    return ELVIS_OK;
}

extern "C" int elvis_shrink_select_topk(const double* scores, int8_t* mask, int32_t* src_of, int n, int by, int bx, int k,
                                        elvis_stream_t stream) {
    ELVIS_REQUIRE(scores && mask, "elvis_shrink_select_topk: null pointer");
    ELVIS_REQUIRE(n > 0 && by > 0 && bx > 0, "elvis_shrink_select_topk: bad shape n=%d by=%d bx=%d", n, by, bx);
    ELVIS_REQUIRE(k >= 0 && k <= bx, "elvis_shrink_select_topk: k = %d outside [0, %d]", k, bx);
    ELVIS_REQUIRE(src_of || k == bx, "elvis_shrink_select_topk: null pointer");
    ELVIS_REQUIRE((long long)n * by * bx < (1LL << 31), "elvis_shrink_select_topk: too many blocks");
    hipLaunchKernelGGL(shrink_select_topk_kernel, dim3((unsigned)(n * by)), dim3(256), 0, (hipStream_t)stream, scores, mask, src_of,
                       by, bx, k);
    ELVIS_CHECK_LAUNCH("elvis_shrink_select_topk");
    return ELVIS_OK;
}

extern "C" int elvis_shrink_passes_plan(int by, int bx, int target, int mode, int* sby, int* sbx, int* pass_counts,
                                        int max_passes) {
    ELVIS_REQUIRE(sby && sbx, "elvis_shrink_passes_plan: null pointer");
    ELVIS_REQUIRE(by > 0 && bx > 0 && (long long)by * bx < (1LL << 31), "elvis_shrink_passes_plan: bad grid %dx%d", by, bx);
    ELVIS_REQUIRE(mode == kModeRows || mode == kModeRowsCols, "elvis_shrink_passes_plan: unknown mode %d", mode);
    ELVIS_REQUIRE(target >= 0 && target <= by * bx, "elvis_shrink_passes_plan: target %d outside [0, %d]", target, by * bx);
    ELVIS_REQUIRE(max_passes >= 0 && (pass_counts || max_passes == 0), "elvis_shrink_passes_plan: null pointer");
    return passes_plan(by, bx, target, mode, sby, sbx, pass_counts, max_passes);
}

extern "C" int elvis_shrink_select_passes(const double* scores, uint8_t* mask, int32_t* src_of, int32_t* removal_idx,
                                          double* ws_scores, int32_t* ws_pos, int n, int by, int bx, int target, int mode,
                                          int sby, int sbx, elvis_stream_t stream) {
    ELVIS_REQUIRE(scores && mask && ws_scores && ws_pos, "elvis_shrink_select_passes: null pointer");
    ELVIS_REQUIRE(n > 0 && by > 0 && bx > 0 && (long long)n * by * bx < (1LL << 31),
                  "elvis_shrink_select_passes: bad shape n=%d by=%d bx=%d", n, by, bx);
    ELVIS_REQUIRE(mode == kModeRows || mode == kModeRowsCols, "elvis_shrink_select_passes: unknown mode %d", mode);
    ELVIS_REQUIRE(target >= 0 && target <= by * bx, "elvis_shrink_select_passes: target %d outside [0, %d]", target, by * bx);
    ELVIS_REQUIRE((long long)n * target < (1LL << 31), "elvis_shrink_select_passes: too many removals");
    int want_by = 0, want_bx = 0;
    passes_plan(by, bx, target, mode, &want_by, &want_bx, nullptr, 0);
    ELVIS_REQUIRE(sby == want_by && sbx == want_bx,
                  "elvis_shrink_select_passes: the shrunk grid of a %dx%d grid with %d removals is %dx%d, not %dx%d", by, bx, target,
                  want_by, want_bx, sby, sbx);
    ELVIS_REQUIRE(src_of || sby == 0 || sbx == 0, "elvis_shrink_select_passes: null pointer");
    hipLaunchKernelGGL(shrink_select_passes_kernel, dim3((unsigned)n), dim3(1024), 0, (hipStream_t)stream, scores, mask, src_of,
                       removal_idx, ws_scores, ws_pos, by, bx, target, mode, sby, sbx);
    ELVIS_CHECK_LAUNCH("elvis_shrink_select_passes");
    return ELVIS_OK;
}

extern "C" int elvis_stretch_index(const uint8_t* mask, int32_t* src_of, int n, int by, int bx, int sby, int sbx, int mode,
                                   elvis_stream_t stream) {
    ELVIS_REQUIRE(mask && src_of, "elvis_stretch_index: null pointer");
    ELVIS_REQUIRE(n > 0 && by > 0 && bx > 0 && sby >= 0 && sbx >= 0, "elvis_stretch_index: bad shape n=%d by=%d bx=%d", n, by, bx);
    ELVIS_REQUIRE(mode == kRankFlat || mode == kRankRows, "elvis_stretch_index: unknown mode %d", mode);
    ELVIS_REQUIRE((long long)n * by * bx < (1LL << 31) && (long long)sby * sbx < (1LL << 31), "elvis_stretch_index: too many blocks");
    const unsigned grid = (unsigned)(mode == kRankFlat ? n : n * by);
    hipLaunchKernelGGL(stretch_index_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, mask, src_of, by, bx, sby, sbx, mode);
    ELVIS_CHECK_LAUNCH("elvis_stretch_index");
    return ELVIS_OK;
}
