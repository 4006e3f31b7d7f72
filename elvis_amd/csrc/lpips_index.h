// Index arithmetic of csrc/lpips.hip, host and device: the geometry of the AlexNet trunk, which byte of a clip a staged
// element of the stem's footprint is, and which pixel a lane group of the distance kernel takes.  Kept apart from the
// kernels so that a host program can walk the same arithmetic over exact-size buffers (tools/lpips_index_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LPIPS_HD __host__ __device__ __forceinline__
#else
#define LPIPS_HD static inline
#endif

#define LPIPS_MIN_SIDE 31          // the smallest rect that leaves a 1 x 1 last feature map
#define LPIPS_STEM_KS 11
#define LPIPS_STEM_STRIDE 4
#define LPIPS_STEM_PAD 2
#define LPIPS_STEM_K (LPIPS_STEM_KS * LPIPS_STEM_KS * 3)   // 363 products per output
#define LPIPS_STEM_COUT 64
#define LPIPS_STEM_TY 4            // output tile of one workgroup: 4 x 16 pixels x 64 channels
#define LPIPS_STEM_TX 16
#define LPIPS_STEM_ROWS ((LPIPS_STEM_TY - 1) * LPIPS_STEM_STRIDE + LPIPS_STEM_KS)   // 23 rows of input ...
#define LPIPS_STEM_COLS ((LPIPS_STEM_TX - 1) * LPIPS_STEM_STRIDE + LPIPS_STEM_KS)   // ... by 71 columns
#define LPIPS_DIST_THREADS 256
#define LPIPS_DIST_PIXELS 64       // pixels of one workgroup of the distance kernel: 16 per wave, one after the other
#define LPIPS_DIST_MAX_C 384

LPIPS_HD int lpips_stem_size(int s) { return (s + 2 * LPIPS_STEM_PAD - LPIPS_STEM_KS) / LPIPS_STEM_STRIDE + 1; }
LPIPS_HD int lpips_pool_size(int s) { return (s - 3) / 2 + 1; }
LPIPS_HD int lpips_rect_ok(int h, int w, int y0, int y1, int x0, int x1) {
    return y0 >= 0 && x0 >= 0 && y1 <= h && x1 <= w && y1 - y0 >= LPIPS_MIN_SIDE && x1 - x0 >= LPIPS_MIN_SIDE;
}

// Element (r, cc) of the footprint staged for the output tile that starts at (oy0, ox0): the pixel index into frame f
// of an [n, h, w] clip, or -1 where the element is the conv's zero padding (outside the rect).
LPIPS_HD long long lpips_stem_src_pixel(int f, int h, int w, int y0, int y1, int x0, int x1, int oy0, int ox0, int r, int cc) {
    const int iy = oy0 * LPIPS_STEM_STRIDE - LPIPS_STEM_PAD + r, ix = ox0 * LPIPS_STEM_STRIDE - LPIPS_STEM_PAD + cc;
    if (iy < 0 || iy >= y1 - y0 || ix < 0 || ix >= x1 - x0) return -1;
    return ((long long)f * h + y0 + iy) * w + x0 + ix;
}

// The byte the network sees for channel `ch` (0 = R, 1 = G, 2 = B) of pixel `pix`: the frame's byte - rows are 3 w bytes
// and a rect starts anywhere, so bytes are loaded one by one - or 0 where the mask is 0.
LPIPS_HD int lpips_stem_byte(const uint8_t* frames, const uint8_t* mask, long long pix, int ch, int bgr) {
    if (mask && mask[pix] == 0) return 0;
    return frames[pix * 3 + (bgr ? 2 - ch : ch)];
}

// Float offset of channel 0 of output pixel (oy, ox) of frame f in the stem's [n, ho, wo, pitch] output.
LPIPS_HD long long lpips_stem_out_offset(int f, int ho, int wo, int oy, int ox, int pitch) { return (((long long)f * ho + oy) * wo + ox) * pitch; }

LPIPS_HD int lpips_dist_blocks(long long hw) { return (int)((hw + LPIPS_DIST_PIXELS - 1) / LPIPS_DIST_PIXELS); }
// Pixel i (0 .. 15) of wave `wave` of workgroup `block` of a frame, or -1 past the frame's last pixel.
LPIPS_HD long long lpips_dist_pixel(long long hw, int block, int wave, int i) {
    const long long p = (long long)block * LPIPS_DIST_PIXELS + wave * (LPIPS_DIST_PIXELS / 4) + i;
    return p < hw ? p : -1;
}
// Float offset of channel c of pixel p of frame f in an [n, hw, pitch] feature tensor.
LPIPS_HD long long lpips_feature_offset(int f, long long hw, long long p, int pitch, int c) { return ((long long)f * hw + p) * pitch + c; }
