// What `RealESRGANer.enhance` does around the network (elvis.py:2482-2519, utils.py:1428-1470, presley.py:1279-1314):
//   elvis_resize_lanczos4_u8   - cv2.resize(src, (wd, hd), interpolation=INTER_LANCZOS4) of 8-bit frames at any ratio, the
//                                resize to `outscale` inside `enhance` and the resize back to (w, h) after it
//   elvis_sr_gather_tiles_u8   - the padded input boxes of `tile_process`, read through two index maps that realise
//                                `pre_process` (reflect pre_pad, then the reflect pad to an even size of an x2 network)
//   elvis_sr_paste_tiles_u8    - the output crops of `tile_process` written into the frame, clipped at s*H x s*W, which is
//                                the pad removal of `post_process`
//   elvis_resize_lanczos4_lds_bytes - host only: the LDS one workgroup of the resize needs for a destination tile
//
// The resize is cv2's fixed-point rule, the one classical.py states for the per-block upscale: per destination index a
// first source index and eight int16 taps (rint(coef * 2048)), source indices clamped to the frame (BORDER_REPLICATE),
// no rounding between the passes, (sum + 2^21) >> 22 saturated at the end.  The host builds the tables; the kernel only
// multiplies.  One launch: a workgroup of 256 threads owns a th x tw destination tile,
//   1. loads the tile's source footprint (rows [first_y(top), first_y(bottom) + 7], columns likewise, clipped to the
//      frame) into LDS with aligned 4-byte loads: a row's bytes keep their global phase (address mod 4) in LDS, so a
//      loaded dword is stored as it is,
//   2. horizontal pass: int32 mid[row][x * c + ch] = sum_k xt[k] * src[row][clamp(first_x + k)], kept in LDS,
//   3. vertical pass: sum_k yt[k] * mid[clamp(first_y + k)][j], rounded, saturated, stored.
// LDS BUDGET: 64 KiB per workgroup (the default dynamic limit, no opt-in), of 160 KiB per CU: two workgroups are always
// resident.  The host picks the largest tile of 16x64, 16x32, 8x32, 8x16, 4x16 whose footprint fits; the entry point
// recomputes the footprint from the host copy of the first-index tables and refuses a launch that does not fit.
// BANKS: the mid row is tw * c int32, a multiple of 32 dwords for every tile of 32 or 64 columns.  Both passes address it
// with consecutive lanes on consecutive dwords (j = x * c + ch), and when a wave spans two rows each 32-lane half stays
// inside one row, so ds_read_b32 / ds_write_b32 (32 banks, conflicts per 32-lane half) are conflict-free at any row
// stride.  The byte reads of the horizontal pass hit one dword per c lanes (broadcast) and move by at most 4 * c bytes
// per pixel in a 4:1 downscale: at most 2-way.
// int32: the largest partial sum is 255 * (Px * Py + Nx * Ny) + 2^21 (P, N: sums of a phase's positive and negative
// taps); the host (enhance.py) computes it from the tables it built and refuses 2^31 or more.
#include "common.h"

namespace {

constexpr int kLdsBudget = 64 * 1024;

__host__ __device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct ResizeLds {
    int fh, fw, sstride, mstride, off_yt, off_xf, off_yf, off_src, off_mid, bytes;
};

// the LDS image of one workgroup: x taps, y taps, x firsts, y firsts, source bytes, int32 intermediate
ResizeLds resize_lds(int fh, int fw, int c, int th, int tw) {
    ResizeLds l;
    l.fh = fh;
    l.fw = fw;
    l.sstride = (fw * c + 3 + 3) & ~3;      // up to 3 bytes of phase in front
    l.mstride = tw * c;
    l.off_yt = tw * 16;
    l.off_xf = l.off_yt + th * 16;
    l.off_yf = l.off_xf + tw * 4;
    l.off_src = l.off_yf + th * 4;
    l.off_mid = l.off_src + fh * l.sstride;
    l.bytes = l.off_mid + fh * l.mstride * 4;
    return l;
}

// the widest clipped source span [first[d0], first[d1] + 7] over the tiles of `t` destination indices
int footprint(const int32_t* first, int n_src, int n_dst, int t) {
    int worst = 0;
    for (int d0 = 0; d0 < n_dst; d0 += t) {
        const int d1 = (d0 + t < n_dst ? d0 + t : n_dst) - 1;
        const int a = clampi(first[d0], 0, n_src - 1), b = clampi(first[d1] + 7, 0, n_src - 1);
        if (b - a + 1 > worst) worst = b - a + 1;
    }
    return worst;
}

// 0 when the table is a resize table of n_src -> n_dst: every first index in [-4, n_src - 4], never decreasing
int bad_first_table(const int32_t* first, int n_src, int n_dst) {
    for (int d = 0; d < n_dst; ++d) {
        if (first[d] < -4 || first[d] > n_src - 4) return d + 1;
        if (d && first[d] < first[d - 1]) return d + 1;
    }
    return 0;
}

template <int C>
__global__ __launch_bounds__(256) void resize_lanczos4_u8_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int32_t* __restrict__ xfirst,
    const int16_t* __restrict__ xtaps, const int32_t* __restrict__ yfirst, const int16_t* __restrict__ ytaps, int hs, int ws,
    int hd, int wd, int th, int tw, ResizeLds l, long long total_bytes, int aligned) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    int4* s_xt = reinterpret_cast<int4*>(lds);
    int4* s_yt = reinterpret_cast<int4*>(lds + l.off_yt);
    int32_t* s_xf = reinterpret_cast<int32_t*>(lds + l.off_xf);
    int32_t* s_yf = reinterpret_cast<int32_t*>(lds + l.off_yf);
    uint8_t* s_src = lds + l.off_src;
    int32_t* s_mid = reinterpret_cast<int32_t*>(lds + l.off_mid);

    const int f = blockIdx.z, dy0 = blockIdx.y * th, dx0 = blockIdx.x * tw;
    const int tile_h = min(th, hd - dy0), tile_w = min(tw, wd - dx0);
    const int tid = threadIdx.x;
    // the footprint, clipped to the frame and (against tables that disagree with the host's) to the LDS image
    const int cy0 = clampi(yfirst[dy0], 0, hs - 1), cx0 = clampi(xfirst[dx0], 0, ws - 1);
    const int rows = min(clampi(yfirst[dy0 + tile_h - 1] + 7, cy0, hs - 1) - cy0 + 1, l.fh);
    const int cols = min(clampi(xfirst[dx0 + tile_w - 1] + 7, cx0, ws - 1) - cx0 + 1, l.fw);
    const int cy1 = cy0 + rows - 1, cx1 = cx0 + cols - 1;

    for (int i = tid; i < tile_w; i += 256) {
        s_xt[i] = *reinterpret_cast<const int4*>(xtaps + 8 * (long long)(dx0 + i));
        s_xf[i] = xfirst[dx0 + i];
    }
    for (int i = tid; i < tile_h; i += 256) {
        s_yt[i] = *reinterpret_cast<const int4*>(ytaps + 8 * (long long)(dy0 + i));
        s_yf[i] = yfirst[dy0 + i];
    }
    // 1. source rows, as aligned dwords that keep their phase
    const int ndw_max = l.sstride >> 2;
    const int len = cols * C;
    for (int item = tid; item < rows * ndw_max; item += 256) {
        const int r = item / ndw_max, j = item - r * ndw_max;
        const long long g0 = (((long long)f * hs + cy0 + r) * ws + cx0) * C;
        const int phase = (int)(g0 & 3);
        if (4 * j >= phase + len) continue;
        const long long a = g0 - phase + 4 * j;
        uint32_t v = 0;
        if (aligned && a + 4 <= total_bytes) {
            v = *reinterpret_cast<const uint32_t*>(src + a);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (a + b < total_bytes) v |= (uint32_t)src[a + b] << (8 * b);
        }
        reinterpret_cast<uint32_t*>(s_src)[r * ndw_max + j] = v;
    }
    __syncthreads();
    // 2. horizontal pass
    const int wj = tile_w * C;
    // item = r * wj + j walks in steps of 256: (r, j) advance by (256 / wj, 256 % wj) with a carry, no division per item
    const int step_r = 256 / wj, step_j = 256 - step_r * wj;
    int r = tid / wj, j = tid - r * wj;
    for (; r < rows; r += step_r, j += step_j) {
        if (j >= wj) {
            j -= wj;
            if (++r >= rows) break;
        }
        const int x = j / C, ch = j - x * C;
        const int phase = (int)(((((unsigned)f * (unsigned)hs + (unsigned)(cy0 + r)) * (unsigned)ws + (unsigned)cx0) * (unsigned)C) & 3u);
        const uint8_t* row = s_src + r * l.sstride + phase + ch;
        const int4 tv = s_xt[x];
        const int first = s_xf[x];
        const int t[8] = {(int16_t)(tv.x & 0xffff), tv.x >> 16, (int16_t)(tv.y & 0xffff), tv.y >> 16,
                          (int16_t)(tv.z & 0xffff), tv.z >> 16, (int16_t)(tv.w & 0xffff), tv.w >> 16};
        int sum = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) sum += t[k] * (int)row[(clampi(first + k, cx0, cx1) - cx0) * C];
        s_mid[r * l.mstride + j] = sum;
    }
    __syncthreads();
    // 3. vertical pass, rounding, saturation
    int dy = tid / wj;
    j = tid - dy * wj;
    for (; dy < tile_h; dy += step_r, j += step_j) {
        if (j >= wj) {
            j -= wj;
            if (++dy >= tile_h) break;
        }
        const int4 tv = s_yt[dy];
        const int first = s_yf[dy];
        const int t[8] = {(int16_t)(tv.x & 0xffff), tv.x >> 16, (int16_t)(tv.y & 0xffff), tv.y >> 16,
                          (int16_t)(tv.z & 0xffff), tv.z >> 16, (int16_t)(tv.w & 0xffff), tv.w >> 16};
        int sum = 1 << 21;
#pragma unroll
        for (int k = 0; k < 8; ++k) sum += t[k] * s_mid[(clampi(first + k, cy0, cy1) - cy0) * l.mstride + j];
        dst[(((long long)f * hd + dy0 + dy) * wd + dx0) * C + j] = (uint8_t)clampi(sum >> 22, 0, 255);
    }
}

// dst[t, y, x] = src[frame_t, rowmap[y0_t + y], colmap[x0_t + x]]; the kernel only indexes
__global__ __launch_bounds__(256) void sr_gather_tiles_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                 const int32_t* __restrict__ desc, const int32_t* __restrict__ rowmap,
                                                                 const int32_t* __restrict__ colmap, int n, int H, int W, int th,
                                                                 int tw, int Hp, int Wp, long long total) {
    const int per = th * tw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(i / per), rem = (int)(i - (long long)t * per);
        const int y = rem / tw, x = rem - y * tw;
        const int fr = clampi(desc[3 * t], 0, n - 1);
        const int sy = clampi(rowmap[clampi(desc[3 * t + 1] + y, 0, Hp - 1)], 0, H - 1);
        const int sx = clampi(colmap[clampi(desc[3 * t + 2] + x, 0, Wp - 1)], 0, W - 1);
        const uint8_t* p = src + (((long long)fr * H + sy) * W + sx) * 3;
        uint8_t* d = dst + i * 3;
        d[0] = p[0];
        d[1] = p[1];
        d[2] = p[2];
    }
}

// desc[t] = (frame, crop y, crop x inside the tile, destination y, x, crop height, width); blockIdx.x is the tile
__global__ __launch_bounds__(256) void sr_paste_tiles_u8_kernel(const uint8_t* __restrict__ tiles, uint8_t* __restrict__ dst,
                                                                const int32_t* __restrict__ desc, int tth, int ttw, int n, int OH,
                                                                int OW) {
    const int t = blockIdx.x;
    const int32_t* e = desc + 7 * (long long)t;
    const int fr = clampi(e[0], 0, n - 1);
    const int cy = clampi(e[1], 0, tth), cx = clampi(e[2], 0, ttw), oy = max(e[3], 0), ox = max(e[4], 0);
    const int ch = min(min(e[5], tth - cy), OH - oy), cw = min(min(e[6], ttw - cx), OW - ox);   // beyond s*H, s*W: dropped
    if (ch <= 0 || cw <= 0) return;
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < ch * cw; i += gridDim.y * blockDim.x) {
        const int y = i / cw, x = i - y * cw;
        const uint8_t* p = tiles + (((long long)t * tth + cy + y) * ttw + cx + x) * 3;
        uint8_t* d = dst + (((long long)fr * OH + oy + y) * OW + ox + x) * 3;
        d[0] = p[0];
        d[1] = p[1];
        d[2] = p[2];
    }
}

int check_resize_tables(const char* who, const int32_t* xfirst_h, const int32_t* yfirst_h, int hs, int ws, int hd, int wd, int c,
                        int th, int tw, ResizeLds* out) {
    ELVIS_REQUIRE(xfirst_h && yfirst_h, "%s: null pointer", who);
    ELVIS_REQUIRE(hs > 0 && ws > 0 && hd > 0 && wd > 0, "%s: bad shape %dx%d -> %dx%d", who, hs, ws, hd, wd);
    ELVIS_REQUIRE(c >= 1 && c <= 4, "%s: %d channels (1 to 4 supported)", who, c);
    ELVIS_REQUIRE(th >= 1 && tw >= 1 && th <= 64 && tw <= 256, "%s: destination tile %dx%d outside [1, 64] x [1, 256]", who, th, tw);
    int bad = bad_first_table(yfirst_h, hs, hd);
    ELVIS_REQUIRE(!bad, "%s: row table entry %d = %d outside [-4, %d] or decreasing", who, bad - 1, yfirst_h[bad - 1], hs - 4);
    bad = bad_first_table(xfirst_h, ws, wd);
    ELVIS_REQUIRE(!bad, "%s: column table entry %d = %d outside [-4, %d] or decreasing", who, bad - 1, xfirst_h[bad - 1], ws - 4);
    *out = resize_lds(footprint(yfirst_h, hs, hd, th), footprint(xfirst_h, ws, wd, tw), c, th, tw);
    return ELVIS_OK;
}

}  // namespace

extern "C" int elvis_resize_lanczos4_lds_bytes(const int32_t* xfirst_h, const int32_t* yfirst_h, int hs, int ws, int hd, int wd,
                                               int c, int th, int tw) {
    ResizeLds l;
    const int rc = check_resize_tables("elvis_resize_lanczos4_lds_bytes", xfirst_h, yfirst_h, hs, ws, hd, wd, c, th, tw, &l);
    return rc != ELVIS_OK ? rc : l.bytes;
}

extern "C" int elvis_resize_lanczos4_u8(const uint8_t* src, uint8_t* dst, int n, int hs, int ws, int hd, int wd, int c,
                                        const int32_t* xfirst_h, const int32_t* yfirst_h, const int32_t* xfirst,
                                        const int16_t* xtaps, const int32_t* yfirst, const int16_t* ytaps, int th, int tw,
                                        elvis_stream_t stream) {
    const char* who = "elvis_resize_lanczos4_u8";
    ELVIS_REQUIRE(src && dst && xfirst && xtaps && yfirst && ytaps, "%s: null pointer", who);
    ELVIS_REQUIRE(n > 0, "%s: bad frame count %d", who, n);
    ResizeLds l;
    const int rc = check_resize_tables(who, xfirst_h, yfirst_h, hs, ws, hd, wd, c, th, tw, &l);
    if (rc != ELVIS_OK) return rc;
    ELVIS_REQUIRE(l.bytes <= kLdsBudget, "%s: a %dx%d tile of %dx%d -> %dx%d needs %d bytes of LDS, the limit is %d", who, th, tw, hs,
                  ws, hd, wd, l.bytes, kLdsBudget);
    ELVIS_REQUIRE(((uintptr_t)xtaps & 15) == 0 && ((uintptr_t)ytaps & 15) == 0, "%s: tap tables must be 16-byte aligned", who);
    const int gx = cdiv(wd, tw), gy = cdiv(hd, th);
    ELVIS_REQUIRE(n <= 65535 && gy <= 65535, "%s: grid %d x %d x %d too large", who, gx, gy, n);
    ELVIS_REQUIRE((long long)hd * wd * c < (1LL << 31) && (long long)hs * ws * c < (1LL << 31), "%s: frame too large", who);
    const long long total = (long long)n * hs * ws * c;
    const int aligned = ((uintptr_t)src & 3) == 0;
    const dim3 grid(gx, gy, n);
#define LAUNCH(C)                                                                                                              \
    hipLaunchKernelGGL(resize_lanczos4_u8_kernel<C>, grid, dim3(256), (size_t)l.bytes, (hipStream_t)stream, src, dst, xfirst, xtaps, \
                       yfirst, ytaps, hs, ws, hd, wd, th, tw, l, total, aligned)
    switch (c) {
        case 1: LAUNCH(1); elvis_note_launch("resize_lanczos4_u8_kernel<1>"); break;
        case 2: LAUNCH(2); elvis_note_launch("resize_lanczos4_u8_kernel<2>"); break;
        case 3: LAUNCH(3); elvis_note_launch("resize_lanczos4_u8_kernel<3>"); break;
        default: LAUNCH(4); elvis_note_launch("resize_lanczos4_u8_kernel<4>"); break;
    }
#undef LAUNCH
    ELVIS_CHECK_LAUNCH(who);
    return ELVIS_OK;
}

extern "C" int elvis_sr_gather_tiles_u8(const uint8_t* src, uint8_t* dst, int n, int H, int W, int T, int th, int tw,
                                        const int32_t* desc_h, const int32_t* desc, const int32_t* rowmap_h, const int32_t* rowmap,
                                        int Hp, const int32_t* colmap_h, const int32_t* colmap, int Wp, elvis_stream_t stream) {
    const char* who = "elvis_sr_gather_tiles_u8";
    ELVIS_REQUIRE(src && dst && desc_h && desc && rowmap_h && rowmap && colmap_h && colmap, "%s: null pointer", who);
    ELVIS_REQUIRE(n > 0 && H > 0 && W > 0 && T > 0 && th > 0 && tw > 0 && Hp > 0 && Wp > 0,
                  "%s: bad shape n=%d %dx%d, %d tiles of %dx%d, padded %dx%d", who, n, H, W, T, th, tw, Hp, Wp);
    ELVIS_REQUIRE(th <= Hp && tw <= Wp, "%s: a %dx%d tile does not fit the padded %dx%d image", who, th, tw, Hp, Wp);
    ELVIS_REQUIRE((long long)th * tw < (1LL << 31) && (long long)H * W * 3 < (1LL << 31), "%s: frame too large", who);
    for (int i = 0; i < Hp; ++i)
        ELVIS_REQUIRE(rowmap_h[i] >= 0 && rowmap_h[i] < H, "%s: row map entry %d = %d outside [0, %d)", who, i, rowmap_h[i], H);
    for (int i = 0; i < Wp; ++i)
        ELVIS_REQUIRE(colmap_h[i] >= 0 && colmap_h[i] < W, "%s: column map entry %d = %d outside [0, %d)", who, i, colmap_h[i], W);
    for (int t = 0; t < T; ++t) {
        const int32_t* e = desc_h + 3 * (long long)t;
        ELVIS_REQUIRE(e[0] >= 0 && e[0] < n && e[1] >= 0 && e[1] <= Hp - th && e[2] >= 0 && e[2] <= Wp - tw,
                      "%s: tile %d (frame %d, origin %d, %d) outside %d frames of padded %dx%d", who, t, e[0], e[1], e[2], n, Hp, Wp);
    }
    const long long total = (long long)T * th * tw;
    long long grid = (total + 255) / 256;
    if (grid > 256 * 64) grid = 256 * 64;
    hipLaunchKernelGGL(sr_gather_tiles_u8_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, src, dst, desc, rowmap,
                       colmap, n, H, W, th, tw, Hp, Wp, total);
    ELVIS_CHECK_LAUNCH(who);
    elvis_note_launch("sr_gather_tiles_u8_kernel");
    return ELVIS_OK;
}

extern "C" int elvis_sr_paste_tiles_u8(const uint8_t* tiles, uint8_t* dst, int T, int tth, int ttw, int n, int OH, int OW,
                                       const int32_t* desc_h, const int32_t* desc, elvis_stream_t stream) {
    const char* who = "elvis_sr_paste_tiles_u8";
    ELVIS_REQUIRE(tiles && dst && desc_h && desc, "%s: null pointer", who);
    ELVIS_REQUIRE(T > 0 && tth > 0 && ttw > 0 && n > 0 && OH > 0 && OW > 0, "%s: bad shape %d tiles of %dx%d into n=%d %dx%d", who, T,
                  tth, ttw, n, OH, OW);
    ELVIS_REQUIRE((long long)tth * ttw < (1LL << 30) && (long long)OH * OW * 3 < (1LL << 31), "%s: frame too large", who);
    int most = 1;
    for (int t = 0; t < T; ++t) {
        const int32_t* e = desc_h + 7 * (long long)t;
        ELVIS_REQUIRE(e[0] >= 0 && e[0] < n, "%s: tile %d names frame %d of %d", who, t, e[0], n);
        ELVIS_REQUIRE(e[5] > 0 && e[6] > 0 && e[1] >= 0 && e[2] >= 0 && e[1] <= tth - e[5] && e[2] <= ttw - e[6],
                      "%s: tile %d: a %dx%d crop at (%d, %d) is outside the %dx%d tile", who, t, e[5], e[6], e[1], e[2], tth, ttw);
        // a destination at or beyond OH, OW is a tile that lies in the padding: nothing of it is written
        ELVIS_REQUIRE(e[3] >= 0 && e[4] >= 0, "%s: tile %d: negative destination (%d, %d)", who, t, e[3], e[4]);
        if (e[5] * e[6] > most) most = e[5] * e[6];
    }
    int gy = cdiv(most, 256 * 4);
    if (gy > 1024) gy = 1024;
    hipLaunchKernelGGL(sr_paste_tiles_u8_kernel, dim3((unsigned)T, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, tiles, dst, desc,
                       tth, ttw, n, OH, OW);
    ELVIS_CHECK_LAUNCH(who);
    elvis_note_launch("sr_paste_tiles_u8_kernel");
    return ELVIS_OK;
}
