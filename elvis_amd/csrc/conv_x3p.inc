// Planar form of the error-compensated f16 convolution (ELVIS_F32X3) for 3x3 / stride 1 / pad 1 layers and their 2x2
// relatives (sub-pixel upsample parities, space-to-depth stride 2): fp32 tensors,
// THREE f16 MFMAs per 32 input channels instead of the interleaved form's four (conv_kernels.inc mma_tile_x).
//
//   v = hi + lo,  hi = f16(v), lo = f16(v - hi)           (~22 significant bits; |v| < 65504, see elvis_amd.h)
//   w*x ~= w_hi*x_hi + w_hi*x_lo + w_lo*x_hi              (the dropped lo*lo term is 2^-22 relative)
//
// Activations are split ONCE per element while a K chunk of 32 channels is staged into LDS, into two planes of the
// f16 kernels' LDS image ([halo pixel][32 halfs] rows of 64 bytes, XOR-swizzled: lds_row_off): a hi plane and a lo
// plane.  Weights are packed at load time the same way, [tap][K chunk][cout tile][plane][TCO][32 halfs], so a (tap,
// chunk) slice of a cout tile is one contiguous block that LDS-DMA copies linearly.  Every fragment read then feeds a
// full-K v_mfma_f32_16x16x32_f16 - no operand is derived in registers and none multiplies zeros (the interleaved form
// spends 8 VALU per weight fragment and wastes half the K slots of its second MFMA).  Per tap and wave: 8 A fragments
// + 2 B fragments per pixel sub-tile feed 12 MFMAs each - a third of the f16 kernel's LDS reads per MFMA.
//
// 512 threads (8 waves, two per SIMD), one workgroup per CU: tile TY x 32 pixels x TCO output channels
// (128 x 12 rows: 64 co x 96 px per wave, 96 accumulator registers; 64 x 16 rows: 64 co x 64 px per wave).
// LDS: one halo buffer (2 planes) + a 2-slot ring of kernel ROWS (3 taps) of weights, filled by LDS-DMA one row
// ahead: 60.9 + 98.3 KB (TCO 128) / 78.3 + 49.2 KB (TCO 64).  The next chunk's halo is register-staged: loaded
// during the chunk's first row step, converted (fused GroupNorm-affine + SiLU in fast fp32 math: v_exp_f32 / v_rcp_f32,
// ~2 ulp - the compensated mode's own error is 2^-22; then the hi/lo split, 2 VALU per element) and written between
// the chunk's last barrier and the next.  Bias / residual seed the accumulators; epilogue, GroupNorm partial
// statistics and the tile walk are those of the halo kernels (conv_kernels.inc).
#pragma once
#include "conv_kernels.inc"

namespace {

// hi/lo split of two fp32 values into packed halfs: 4 VALU per pair
__device__ __forceinline__ void x3p_split2(float v0, float v1, unsigned& hi, unsigned& lo) {
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    const half2v h = {(half_t)v0, (half_t)v1};
    const half2v l = {(half_t)(v0 - (float)h[0]), (half_t)(v1 - (float)h[1])};
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}
// GroupNorm-affine + SiLU, fast form: the table holds a' = -log2(e) a, b' = -log2(e) b
__device__ __forceinline__ float x3p_prologue(float x, float a, float b) {
    const float K = -1.4426950408889634f;
    const float u = fmaf(x, a, b);                       // -log2(e) t
    const float d = fmaf(__builtin_amdgcn_exp2f(u), K, K);   // K (1 + e^-t)
    return u * __builtin_amdgcn_rcpf(d);                 // t / (1 + e^-t)
}

// KS = 3: 3x3 / stride 1 / pad 1.  KS = 2: one parity of the sub-pixel form of "nearest 2x + 3x3" (output pixel
// (2y + a, 2x + b), padding 1 - a / 1 - b) or the space-to-depth form of "pad (0,1,0,1) + 3x3 / stride 2" (K chunk kc
// reads phase kc / nkc_c of the full-resolution input) - the geometries of conv3x3_halo_body's KS = 2.
template <int TCO, int TY, int KS, bool PRO, bool ACT>
__global__ __launch_bounds__(512, 2) void conv3x3_x3p_kernel(ConvArgs p) {
    constexpr int NT = 512, TX = 32, HX = TX + KS - 1, HY = TY + KS - 1, HP = HX * HY;
    constexpr int PLANE = HP * 64, HALO_BYTES = 2 * PLANE;                 // hi plane, then lo plane
    constexpr int W_PLANE = TCO * 64, W_TAP = 2 * W_PLANE, W_ROW = KS * W_TAP;
    static_assert(KS == 3 || (KS == 2 && !PRO), "kernel size");
    constexpr int HCH = HP * 4, H_PER = (HCH + NT - 1) / NT;               // staging units (pixel, 8-channel group) per thread
    constexpr int W_PER = (TCO * 8) / NT;                                  // 16-byte DMA pieces per thread per tap
    constexpr int NW_CO = TCO / 64, NW_PX = 8 / NW_CO, ROWS = TY / NW_PX, WPX = ROWS * 2, WCO = 4;
    static_assert(TCO == 64 || TCO == 128, "cout tile");
    static_assert(ROWS * NW_PX == TY && (TCO * 8) % NT == 0, "tile shape");
    static_assert(HALO_BYTES + 2 * W_ROW + 256 <= 160 * 1024, "LDS");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const halo = smem;
    char* const wring = smem + HALO_BYTES;

    // ---- tile decode (as conv3x3_halo_body: XCD-contiguous bands, cout tiles of a pixel tile adjacent, column strips)
    const unsigned nblk = (unsigned)p.n_co_tiles * (unsigned)p.tiles_x * (unsigned)p.tiles_y * (unsigned)p.n;
    unsigned bid = blockIdx.x;
    {
        const unsigned q = nblk >> 3, r = nblk & 7u;
        const unsigned xcd = bid & 7u, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    int co_tile = 0;
    unsigned t = bid;
    if (p.n_co_tiles > 1) {
        t = bid / (unsigned)p.n_co_tiles;
        co_tile = (int)(bid - t * (unsigned)p.n_co_tiles);
    }
    int tx, ty, nimg;
    if (p.strip > 0) {
        const unsigned per_img = (unsigned)p.tiles_x * (unsigned)p.tiles_y;
        const unsigned ni = t / per_img;
        unsigned r = t - ni * per_img;
        const unsigned full = (unsigned)p.strip_full, strip_tiles = (unsigned)p.strip * (unsigned)p.tiles_y;
        unsigned s = r / strip_tiles;
        unsigned sw = (unsigned)p.strip;
        if (s >= full) { s = full; sw = (unsigned)p.tiles_x - full * (unsigned)p.strip; }
        r -= s * strip_tiles;
        const unsigned y = r / sw;
        nimg = (int)ni;
        ty = (int)y;
        tx = (int)(s * (unsigned)p.strip + (r - y * sw));
    } else {
        const unsigned row = t / (unsigned)p.tiles_x;
        tx = (int)(t - row * (unsigned)p.tiles_x);
        const unsigned ni = row / (unsigned)p.tiles_y;
        ty = (int)(row - ni * (unsigned)p.tiles_y);
        nimg = (int)ni;
    }
    const int oy0 = ty * TY, ox0 = tx * TX, co0 = co_tile * TCO;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w_co = wave / NW_PX, w_px = wave % NW_PX;
    const int lq = lane >> 4, lr = lane & 15;

    // ---- halo staging plan: unit = tid + NT*i -> (halo pixel, 8-channel group q4 = tid & 3); branch-free
    const int pad_y = KS == 2 ? p.pad2y : 1, pad_x = KS == 2 ? p.pad2x : 1;
    int h_src[H_PER];
    unsigned h_ok = 0;
#pragma unroll
    for (int i = 0; i < H_PER; ++i) {
        const int chunk = tid + i * NT;
        const int pix = chunk >> 2;
        const int hy = pix / HX, hx = pix - hy * HX;
        const int gy = oy0 + hy - pad_y, gx = ox0 + hx - pad_x;
        const bool ok = chunk < HCH && gy >= 0 && gy < p.h && gx >= 0 && gx < p.w_in;
        h_src[i] = ok ? ((nimg * p.h + gy) * p.istr * p.w_in + gx) * p.istr : 0;   // istr 2: pixel (2 gy, 2 gx) of the full-res input
        h_ok |= (ok ? 1u : 0u) << i;
    }
    const int q4 = tid & 3;
    const int nkc = p.nkc, nrows = nkc * KS;
    const int ctot = p.cin + p.cin2;

    // channel offset of this thread's group in K chunk kc (and, in the space-to-depth form, the phase's pixel offset)
    auto chunk_c0 = [&](int kc, int& pixoff) -> int {
        pixoff = 0;
        if (KS == 2 && p.s2d) {
            const int ph = kc / p.nkc_c;
            pixoff = (ph >> 1) * p.wfull + (ph & 1);
            return (kc - ph * p.nkc_c) * 32 + q4 * 8;
        }
        return (kc >= p.nkc1 ? kc - p.nkc1 : kc) * 32 + q4 * 8;
    };
    uint4 hx0[H_PER], hx1[H_PER];        // the unit's 8 fp32 channels, raw
    // PRO: the GroupNorm affine of a K chunk's 32 channels goes through a 64-float LDS table (a' then b', pre-scaled by
    // -log2 e; zero past the logical channel count: silu(0) = 0 keeps the padding exact).  Every wave loads the entry of
    // its lane (uniform vmcnt bookkeeping), wave 0 publishes it one row step later.
    float* const ptab = reinterpret_cast<float*>(smem + HALO_BYTES + 2 * W_ROW);
    float tv = 0.f;
    auto table_load = [&](int kc) {
        const bool second = kc >= p.nkc1;
        const int cl = (second ? kc - p.nkc1 : kc) * 32 + (lane & 31);
        const bool in = cl < (second ? p.cin2 : p.cin);
        const long long g = (long long)nimg * ctot + (second ? p.cin : 0) + (in ? cl : 0);
        const float raw = (lane < 32 ? p.pa : p.pb)[g];
        tv = in ? -1.4426950408889634f * raw : 0.f;
    };
    auto table_store = [&]() { if (wave == 0) ptab[lane] = tv; };
    auto halo_load = [&](int kc, bool live = true) {   // live = false: the tail's loads all read the first 32 bytes (no traffic)
        const bool second = kc >= p.nkc1;
        const char* xsrc = (const char*)(second ? p.x2 : p.x);
        const int pitch = second ? p.cin2_pitch : p.cin_pitch;
        int pixoff;
        const int c0 = chunk_c0(kc, pixoff);
        const int c0c = c0 < pitch ? c0 : 0;       // pitch % 8 == 0: a group is wholly inside the row or wholly outside
        const long long lv = live ? 4 : 0;
#pragma unroll
        for (int i = 0; i < H_PER; ++i) {
            const char* src = xsrc + ((long long)(h_src[i] + pixoff) * pitch + c0c) * lv;
            hx0[i] = *reinterpret_cast<const uint4*>(src);
            hx1[i] = *reinterpret_cast<const uint4*>(src + 16);
        }
        if constexpr (PRO) table_load(kc);
    };
    // conversion of the staged chunk IN its registers (hx0 -> hi halfs, hx1 -> lo halfs): pure VALU, interleaved with the
    // MFMAs of the chunk's last row step; halo_write then only stores
    auto halo_convert = [&](int kc, int i0, int i1) {
        const bool second = kc >= p.nkc1;
        const int pitch = second ? p.cin2_pitch : p.cin_pitch;
        int pixoff_;
        const int c0 = chunk_c0(kc, pixoff_);
        const bool ch_ok = c0 < pitch;
        float a[8], b[8];
        if constexpr (PRO) {
#pragma unroll
            for (int e = 0; e < 8; e += 4) {
                const float4v a4 = *reinterpret_cast<const float4v*>(ptab + q4 * 8 + e);
                const float4v b4 = *reinterpret_cast<const float4v*>(ptab + 32 + q4 * 8 + e);
#pragma unroll
                for (int k = 0; k < 4; ++k) { a[e + k] = a4[k]; b[e + k] = b4[k]; }
            }
        }
#pragma unroll
        for (int i = i0; i < i1; ++i) {
            float v[8];
            const float4v f0 = __builtin_bit_cast(float4v, hx0[i]), f1 = __builtin_bit_cast(float4v, hx1[i]);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = f0[e]; v[4 + e] = f1[e]; }
            if constexpr (PRO) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = x3p_prologue(v[e], a[e], b[e]);
            }
            uint4 hi, lo;
            x3p_split2(v[0], v[1], hi.x, lo.x);
            x3p_split2(v[2], v[3], hi.y, lo.y);
            x3p_split2(v[4], v[5], hi.z, lo.z);
            x3p_split2(v[6], v[7], hi.w, lo.w);
            const bool keep = ch_ok && ((h_ok >> i) & 1u);
            hi.x = keep ? hi.x : 0u; hi.y = keep ? hi.y : 0u; hi.z = keep ? hi.z : 0u; hi.w = keep ? hi.w : 0u;
            lo.x = keep ? lo.x : 0u; lo.y = keep ? lo.y : 0u; lo.z = keep ? lo.z : 0u; lo.w = keep ? lo.w : 0u;
            hx0[i] = hi;
            hx1[i] = lo;
        }
    };
    auto halo_write = [&]() {
#pragma unroll
        for (int i = 0; i < H_PER; ++i) {
            const int chunk = tid + i * NT;
            if ((i + 1) * NT <= HCH || chunk < HCH) {
                const int off = lds_row_off(chunk >> 2, chunk & 3);
                *reinterpret_cast<uint4*>(halo + off) = hx0[i];
                *reinterpret_cast<uint4*>(halo + PLANE + off) = hx1[i];
            }
        }
    };

    // ---- weights: global -> LDS by LDS-DMA, one kernel row (3 taps x 2 planes) per slot.  The DMA writes lane-linear,
    // so the row swizzle is applied to the per-lane SOURCE offset (an involution: the reads apply it again).
    int wl_off[W_PER];
#pragma unroll
    for (int i = 0; i < W_PER; ++i) {
        const int c = tid + i * NT, plane = c / (TCO * 4), cc = c - plane * (TCO * 4);
        wl_off[i] = plane * W_PLANE + lds_row_off(cc >> 2, cc & 3);
    }
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_ptr_t)smem);
    auto w_glds = [&](int r, int slot) {
        r = r < nrows ? r : nrows - 1;   // the row after the last re-loads it into the idle slot (never read)
        const int kc = r / KS, dy = r - kc * KS;
#pragma unroll
        for (int t2 = 0; t2 < KS; ++t2) {
            const char* wsrc = (const char*)p.w + ((long long)((dy * KS + t2) * nkc + kc) * p.n_co_tiles + co_tile) * W_TAP;
#pragma unroll
            for (int i = 0; i < W_PER; ++i) {
                unsigned keep;
                const unsigned dst = lds_base + (unsigned)(HALO_BYTES + slot * W_ROW + t2 * W_TAP + (i * NT + wave_u * 64) * 16);
                const char* src = wsrc + wl_off[i];
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
            }
        }
    };

    // ---- start-up: first halo chunk and weight row in flight before bias / residual
    halo_load(0);
    w_glds(0, 0);

    float4v acc[WCO][WPX];
    bool co_ok[WCO];
    float bv[WCO][4];
#pragma unroll
    for (int i = 0; i < WCO; ++i) {
        const int co = co0 + w_co * 64 + lq * 16 + i * 4;     // cout % 4 == 0 (host): whole 4-channel groups
        co_ok[i] = co < p.cout;
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[i][r] = 0.f;
        if (p.bias) {
            const float4v b4 = *reinterpret_cast<const float4v*>(p.bias + (co_ok[i] ? co : 0));
#pragma unroll
            for (int r = 0; r < 4; ++r) bv[i][r] = b4[r];
        }
    }
    auto pixel = [&](int j, bool& pix_ok) -> long long {
        const int oy = oy0 + w_px * ROWS + (j >> 1), ox = ox0 + (j & 1) * 16 + lr;
        if constexpr (KS == 2) {   // tile coordinates are those of the kernel's input image (low-res / phase image)
            pix_ok = oy < p.h && ox < p.w_in;
            return pix_ok ? ((long long)nimg * p.ho + p.ostr * oy + p.par_a) * p.wo + p.ostr * ox + p.par_b : 0;
        }
        pix_ok = oy < p.ho && ox < p.wo;
        return pix_ok ? ((long long)nimg * p.ho + oy) * p.wo + ox : 0;
    };
    // y = conv + bias + residual (no epilogue activation): the accumulators start from the residual, whose latency hides under
    // the start-up.  ONE branch around the whole block of loads (clamped addresses): a branch per load makes hipcc wait
    // vmcnt(0) after each - 24 serialized memory round trips per tile.
    const bool seed_res = !ACT && p.res != nullptr;
    if (seed_res) {
#pragma unroll
        for (int j = 0; j < WPX; ++j) {
            bool pix_ok;
            const long long m = pixel(j, pix_ok);
#pragma unroll
            for (int i = 0; i < WCO; ++i) {
                const int co = co0 + w_co * 64 + lq * 16 + i * 4;
                acc[i][j] = *reinterpret_cast<const float4v*>((const float*)p.res + m * p.res_pitch + (co_ok[i] ? co : 0));
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < WPX; ++j)
#pragma unroll
            for (int i = 0; i < WCO; ++i) acc[i][j] = (float4v){0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (PRO) {
        table_store();
        __syncthreads();
    }
    halo_convert(0, 0, H_PER);
    halo_write();
    if constexpr (!ACT) {   // + bias (after the first chunk's conversion work: the residual has landed by now)
#pragma unroll
        for (int j = 0; j < WPX; ++j)
#pragma unroll
            for (int i = 0; i < WCO; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] += bv[i][r];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // B-fragment addressing with zero per-read VALU (conv_kernels.inc): eight per-lane bases + compile-time offsets
    const int pp0 = (w_px * ROWS) * HX + lr;
    int bb[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int carry = ((pp0 & 3) + r) >> 2;
            const int bit = ((pp0 >> 2) & 1) ^ carry ^ e;
            bb[r][e] = pp0 * 64 + ((lq ^ (bit << 1)) << 4);
        }
    const int a_off = w_co * WCO * 1024 + lds_row_off(lr, lq);
    constexpr int YOUNG0 = 2 * H_PER + (PRO ? 1 : 0);   // loads issued after the weight DMA in row step 0

#define ELVIS_X3P_ROW(DY)                                                                                   \
    {                                                                                                       \
        const int rslot = (r0 + DY) & 1;                                                                    \
        /* chunk kcn's table entry (loaded in row step 0, read after row step 2's barrier): published BEFORE this   \
           row's weight DMA is issued - hipcc waits vmcnt(0) for the entry, which must not include that DMA */      \
        if (PRO && DY == 1) table_store();                                                                  \
        w_glds(r0 + DY + 1, rslot ^ 1);                                                                     \
        if (DY == 0) halo_load(kcn, kc + 1 < nkc);                                                          \
        const char* wsb = wring + rslot * W_ROW + a_off;                                                    \
        _Pragma("unroll") for (int dx = 0; dx < KS; ++dx) {                                                 \
            /* software pipeline: the B fragments of pixel sub-tile j+1 are in flight while the 12 MFMAs of     \
               sub-tile j issue (order pinned by sched_group_barrier; hipcc counts the lgkmcnt waits) */        \
            half8 fh[WCO], fl[WCO], xh[2], xl[2];                                                           \
            /* without the prologue the staged next chunk is converted in its registers during the chunk's LAST    \
               row step, a share of the units per tap (VALU only, spread between the MFMAs below) */              \
            if (!PRO && DY == KS - 1) halo_convert(kcn, dx * H_PER / KS, (dx + 1) * H_PER / KS);            \
            _Pragma("unroll") for (int i = 0; i < WCO; ++i) {                                               \
                fh[i] = lds_frag<half8>(wsb + dx * W_TAP + i * 1024);                                       \
                fl[i] = lds_frag<half8>(wsb + dx * W_TAP + W_PLANE + i * 1024);                             \
            }                                                                                               \
            {                                                                                               \
                const int C = DY * HX + dx;                                                                 \
                const char* bp = smem + bb[C & 3][(C >> 2) & 1] + C * 64;                                   \
                xh[0] = lds_frag<half8>(bp);                                                                \
                xl[0] = lds_frag<half8>(bp + PLANE);                                                        \
            }                                                                                               \
            _Pragma("unroll") for (int j = 0; j < WPX; ++j) {                                               \
                if (j + 1 < WPX) {                                                                          \
                    const int C = (((j + 1) >> 1) + DY) * HX + ((j + 1) & 1) * 16 + dx;                     \
                    const char* bp = smem + bb[C & 3][(C >> 2) & 1] + C * 64;                               \
                    xh[(j + 1) & 1] = lds_frag<half8>(bp);                                                  \
                    xl[(j + 1) & 1] = lds_frag<half8>(bp + PLANE);                                          \
                }                                                                                           \
                _Pragma("unroll") for (int i = 0; i < WCO; ++i) {                                           \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fl[i], xh[j & 1], acc[i][j], 0, 0, 0); \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh[i], xl[j & 1], acc[i][j], 0, 0, 0); \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh[i], xh[j & 1], acc[i][j], 0, 0, 0); \
                }                                                                                           \
            }                                                                                               \
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * WCO + 2, 0);                                    \
            _Pragma("unroll") for (int j = 0; j < WPX; ++j) {                                               \
                if (j + 1 < WPX) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                         \
                if (!PRO && DY == KS - 1) {                                                                 \
                    _Pragma("unroll") for (int g = 0; g < 3 * WCO; ++g) {                                   \
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                  \
                        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                                  \
                    }                                                                                       \
                } else {                                                                                    \
                    __builtin_amdgcn_sched_group_barrier(0x008, 3 * WCO, 0);                                \
                }                                                                                           \
            }                                                                                               \
        }                                                                                                   \
        /* retire this row's weight DMA; in row step 0 the younger halo / table loads stay in flight */      \
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(DY == 0 ? YOUNG0 : 0) : "memory");                        \
        __syncthreads();                                                                                    \
    }
    for (int kc = 0; kc < nkc; ++kc) {
        const int r0 = kc * KS;
        const int kcn = kc + 1 < nkc ? kc + 1 : kc;
        ELVIS_X3P_ROW(0)
        ELVIS_X3P_ROW(1)
        if constexpr (KS == 3) ELVIS_X3P_ROW(2)
        // every wave is past its last read of this chunk's halo: overwrite the buffer with the staged next chunk
        if (kc + 1 < nkc) {
            // (with the prologue the conversion stays one block here: interleaved into the row step it pushes the
            //  kernel past 256 registers - 58 spilled)
            if constexpr (PRO) halo_convert(kcn, 0, H_PER);
            halo_write();
        }
        __syncthreads();
    }
#undef ELVIS_X3P_ROW

    // ---- epilogue: (bias, activation, residual when ACT), fp32 NHWC stores, GroupNorm partial sums of the stored values
    float st[WCO][4], sq[WCO][4];
#pragma unroll
    for (int i = 0; i < WCO; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[i][r] = sq[i][r] = 0.f;
    const float* const rbase = p.res ? (const float*)p.res : (const float*)p.out;   // (ACT) always a readable address
    const long long rpitch = p.res ? p.res_pitch : p.cout_pitch;
#pragma unroll
    for (int j = 0; j < WPX; ++j) {
        bool pix_ok;
        const long long m = pixel(j, pix_ok);
#pragma unroll
        for (int i = 0; i < WCO; ++i) {
            const int co = co0 + w_co * 64 + lq * 16 + i * 4;
            const bool ok = pix_ok && co_ok[i];
            float4v v = acc[i][j];
            if constexpr (ACT) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float f = v[r] + bv[i][r];
                    if (p.act == 1) f = gelu_erf_f(f);
                    else if (p.act == 2) f = f / (1.0f + expf(-f));
                    else f = fmaxf(f, 0.0f);
                    v[r] = f;
                }
                // residual: unconditional load from a valid address + selects (no branch around the load, see the start-up)
                const float4v rv = *reinterpret_cast<const float4v*>(rbase + m * rpitch + (co_ok[i] ? co : 0));
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += p.res ? rv[r] : 0.f;
            }
            if (!co_ok[i]) v = (float4v){0.f, 0.f, 0.f, 0.f};                     // pad channels are written too, as zeros
            if (pix_ok && co < p.cout_pitch) *reinterpret_cast<float4v*>((float*)p.out + m * p.cout_pitch + co) = v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float f = ok ? v[r] : 0.f;
                st[i][r] += f;
                sq[i][r] = fmaf(f, f, sq[i][r]);
            }
        }
    }
    if (p.stats) {
        // (as conv3x3_halo_body: every lane writes its 32 partial sums, one thread per (channel, statistic) adds the
        //  tile's NW_PX * 16 pixel-lane partials in a fixed order; rows padded to an odd length)
        constexpr int PXP = NW_PX * 16 + 1;
        static_assert(TCO * 2 * PXP * 4 <= HALO_BYTES + 2 * W_ROW, "statistics columns fit the kernel's LDS");
        float* red = reinterpret_cast<float*>(smem);   // all LDS reads are done (last barrier of the loop)
        const int pcol = w_px * 16 + lr;
#pragma unroll
        for (int i = 0; i < WCO; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cl = w_co * 64 + lq * 16 + i * 4 + r;
                red[(cl * 2 + 0) * PXP + pcol] = st[i][r];
                red[(cl * 2 + 1) * PXP + pcol] = sq[i][r];
            }
        __syncthreads();
        if (tid < TCO * 2 && co0 + (tid >> 1) < p.cout) {
            const float* row = red + tid * PXP;
            float a = 0.f;
#pragma unroll
            for (int q = 0; q < NW_PX * 16; ++q) a += row[q];
            const long long tile = ((long long)nimg * p.tiles_y + ty) * p.tiles_x + tx;
            p.stats[(tile * p.cout + co0) * 2 + tid] = a;
        }
    }
}

// packed weights of the planar form: OIHW f32 -> [tap][kc][cout tile][plane][TCO][32] halfs, rows permuted inside each
// wave's 64-channel group like every other packing (pack_weights_kernel): a lane owns 16 contiguous output channels
__global__ void pack_weights_x3p_kernel(const float* __restrict__ w, half_t* __restrict__ out, int cout, int ctot, int nkc,
                                        int n_co_tiles, int tco, int taps, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i & 31);
    long long t = i >> 5;
    const int rt = (int)(t % tco); t /= tco;
    const int plane = (int)(t & 1); t >>= 1;
    const int ct = (int)(t % n_co_tiles); t /= n_co_tiles;
    const int kc = (int)(t % nkc);
    const int tap = (int)(t / nkc);
    const int row = ct * tco + rt;
    const int rho = row % 64, fi = rho / 16, q = (rho % 16) / 4, rr = rho % 4;
    const int co = (row / 64) * 64 + q * 16 + fi * 4 + rr;
    const int ci = kc * 32 + k;
    float v = 0.f;
    if (co < cout && ci < ctot) v = w[((long long)co * ctot + ci) * taps + tap];
    const half_t h = (half_t)v;
    out[i] = plane ? (half_t)(v - (float)h) : h;
}

template <int TCO, int KS, bool PRO, bool ACT> int launch_x3p_a(const ConvArgs& a, hipStream_t stream, ConvPick* query) {
    constexpr int TY = x3p_tile_rows(TCO);
    static const ElvisKernelName name("conv3x3_x3p_kernel<%d,%d,%d,%s,%s>", TCO, TY, KS, tf(PRO), tf(ACT));
    if (query) return query->set(name.s, TY);
    constexpr size_t lds = 2 * halo_tile_bytes(TY, KS) + 2 * KS * 2 * (size_t)TCO * 64 + (PRO ? 256 : 0);
    static ElvisLdsOptIn opt_in;
    if (int rc = elvis_lds_opt_in((const void*)conv3x3_x3p_kernel<TCO, TY, KS, PRO, ACT>, opt_in, elvis_device_slot(),
                                  "conv3x3_x3p: cannot reserve %zu bytes of LDS", lds))
        return rc;
    const long long nblk = (long long)a.n_co_tiles * a.tiles_x * a.tiles_y * a.n;
    ELVIS_REQUIRE(nblk < 0x7fffffffLL, "conv: grid too large");
    hipLaunchKernelGGL((conv3x3_x3p_kernel<TCO, TY, KS, PRO, ACT>), dim3((unsigned)nblk), dim3(512), lds, stream, a);
    ELVIS_CHECK_LAUNCH("elvis_conv2d(x3p)");
    elvis_note_launch(name.s);
    return ELVIS_OK;
}
template <int TCO> int launch_x3p(const ConvArgs& a, hipStream_t stream, ConvPick* query) {
    if (a.ksize == 2) return a.act != 0 ? launch_x3p_a<TCO, 2, false, true>(a, stream, query) : launch_x3p_a<TCO, 2, false, false>(a, stream, query);
    if (a.act != 0) return a.prologue ? launch_x3p_a<TCO, 3, true, true>(a, stream, query) : launch_x3p_a<TCO, 3, false, true>(a, stream, query);
    return a.prologue ? launch_x3p_a<TCO, 3, true, false>(a, stream, query) : launch_x3p_a<TCO, 3, false, false>(a, stream, query);
}

}  // namespace
