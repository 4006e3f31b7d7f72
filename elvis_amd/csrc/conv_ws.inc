// Weight-stationary 3x3 convolution for NARROW layers at large resolutions (f16, 3x3 / stride 1 / pad 1, at most 64 input
// channels, output tiles of 16 / 32 / 64 channels, bias + optional ReLU) - the DCT slot's 64 -> 64 quality convs, its
// 32-channel offset convs, 32 -> 189 offset / mask conv and 64 -> 1 output conv at 1080p.
//
// Those layers are HBM-bound (64 -> 64: 190 FLOP per byte against a machine balance of ~400), and the halo-tile kernels serve
// them badly: a workgroup per 8 x 32 tile re-streams the layer's whole weight set from L2 (73.7 KB for 64 -> 64 - more than
// the 43.5 KB input halo and the 32 KB output tile together) and has nothing in flight while it waits for its first halo
// (0.9 of the ~2.7 TB/s they reach is the best of three workgroups per CU, each mostly in start-up or epilogue).  Here
//
//   * ONE 512-thread workgroup per CU is PERSISTENT: the cout tile's weights (all taps, all K chunks) go to LDS once;
//   * waves 0-3 and 4-7 each own one 8 x 32 pixel tile of a PAIR of adjacent tiles, with a halo buffer each (whole K: every
//     input channel of the (8+2) x (32+2) window), in the halo kernels' swizzled 64-byte-row image;
//   * the NEXT pair's halos are register-staged: requested right after the current pair's halos have been written to LDS, in
//     flight during all 18 (tap, chunk) MFMA steps and the output stores, written behind the pair's last barrier - so every
//     wave always has 6 * NKC 16-byte loads outstanding and HBM latency never meets an idle CU;
//   * an XCD walks a contiguous band of tile pairs, one tile row per step, so the halo rows two tile rows share are L2 hits.
//
// LDS: weights NKC * 9 * TCO * 64 B + two halos of NKC * 340 * 64 B: 160 768 B for 64 -> 64 (of 163 840).
// Packed weights, fragment layouts, the row permutation that gives a lane contiguous output channels: conv_kernels.inc.
#pragma once
#include "conv_kernels.inc"
#include <atomic>

namespace {

template <int NKC, int TCO, bool STAG>
__global__ __launch_bounds__(512, 1) void conv3x3_ws_kernel(ConvArgs p, int ntiles, int nworkers) {
    constexpr int TY = 8, TX = 32, HX = TX + 2, HY = TY + 2, HP = HX * HY;
    constexpr int WCO = TCO / 16, WPX = 4, ROWS = 2;
    constexpr int PLANE = HP * 64, HALO_BYTES = NKC * PLANE;
    constexpr int W_SLICE = TCO * 64, W_BYTES = NKC * 9 * W_SLICE;
    constexpr int HCH = HP * 4, H_PER = (HCH + 255) / 256;                 // (pixel, 16-byte channel slice) units per thread and chunk
    static_assert(TCO == 16 || TCO == 32 || TCO == 64, "cout tile");
    static_assert(W_BYTES + 2 * HALO_BYTES <= 160 * 1024, "LDS");
    typedef half8 frag_t;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const wlds = smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half_id = wave >> 2, w_px = wave & 3, th = tid & 255;
    char* const halo = smem + W_BYTES + half_id * HALO_BYTES;
    const int lq = lane >> 4, lr = lane & 15;

    const int n_co = p.n_co_tiles;
    const int co_tile = (int)(blockIdx.x % (unsigned)n_co), worker = (int)(blockIdx.x / (unsigned)n_co);
    const int co0 = co_tile * TCO;

    // ---- the cout tile's weights: [tap][chunk][co_pad rows][64 B] in global memory, one [tap * NKC + chunk] slice of TCO
    //      swizzled rows each in LDS
    for (int c = tid; c < NKC * 9 * TCO * 4; c += 512) {
        const int s = c / (TCO * 4), rq = c - s * (TCO * 4);
        const int row = rq >> 2, q = rq & 3;
        const uint4 v = *reinterpret_cast<const uint4*>((const char*)p.w + ((long long)s * p.co_pad + co0 + row) * 64 + q * 16);
        *reinterpret_cast<uint4*>(wlds + s * W_SLICE + lds_row_off(row, q)) = v;
    }
    // bias of the lane's 4 * WCO channels (fragment i, register r: channel lq * 4 * WCO + 4 i + r); zero past cout, where the
    // packed weight rows are zero too - pad channels come out as exact zeros and are stored like any other
    float bv[WCO][4];
#pragma unroll
    for (int i = 0; i < WCO; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + lq * 4 * WCO + i * 4 + r;
            bv[i][r] = (p.bias && co < p.cout) ? p.bias[co] : 0.f;
        }

    // ---- halo staging plan: unit u = th + 256 i -> halo pixel u >> 2 (same 16-byte slice q for every i)
    const int q4 = th & 3;
    int h_yx[H_PER];
#pragma unroll
    for (int i = 0; i < H_PER; ++i) {
        const int pix = (th + 256 * i) >> 2;
        const int hy = pix / HX, hx = pix - hy * HX;
        h_yx[i] = (th + 256 * i) < HCH ? (hy << 8) | hx : -1;
    }
    const int tiles_x = p.tiles_x, tiles_y = p.tiles_y;
    const int npairs = (ntiles + 1) >> 1;
    // XCD-aware walk of the pairs: worker b runs on XCD b % 8 (round-robin dispatch); XCD x owns the contiguous band of pairs
    // [x * band, (x + 1) * band) and its workers take consecutive pairs of it per step: one tile row per step at 1080p
    // (fewer than 8 workers - not on an MI355X - : one band, plain round-robin)
    const bool banded = nworkers >= 8;
    const int wx = banded ? (worker & 7) : 0, wi = banded ? (worker >> 3) : worker;
    const int per_xcd = banded ? ((nworkers + 7 - wx) >> 3) : nworkers;   // workers that share this band
    const int band = banded ? ((npairs + 7) >> 3) : npairs;
    auto pair_of = [&](int k) -> int {   // k-th pair of this worker, or -1
        const int local = k * per_xcd + wi;
        const int pr = wx * band + local;
        return (local < band && pr < npairs) ? pr : -1;
    };
    struct TilePos { int nimg, oy0, ox0; bool ok; };
    auto tile_pos = [&](int pr) -> TilePos {
        const int t = 2 * pr + half_id;
        TilePos tp;
        tp.ok = pr >= 0 && t < ntiles;
        const int tc = tp.ok ? t : 0;
        const int row = tc / tiles_x;
        tp.ox0 = (tc - row * tiles_x) * TX;
        tp.nimg = row / tiles_y;
        tp.oy0 = (row - tp.nimg * tiles_y) * TY;
        return tp;
    };
    uint4 hreg[NKC][H_PER];
    unsigned hmask = 0;   // bit kc * H_PER + i: the unit lies inside the image and the channel pitch (applied when the registers are
                          // WRITTEN to LDS - a select right behind the load would wait for it and serialize the prefetch)
    auto halo_load = [&](const TilePos& tp) {
        hmask = 0;
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
            const bool second = kc >= p.nkc1;
            const char* xsrc = (const char*)(second ? p.x2 : p.x);
            const int pitch = second ? p.cin2_pitch : p.cin_pitch;
            const int c0 = (second ? kc - p.nkc1 : kc) * 32 + q4 * 8;
            const bool ch_ok = c0 < pitch;
#pragma unroll
            for (int i = 0; i < H_PER; ++i) {
                const int hy = h_yx[i] >> 8, hx = h_yx[i] & 255;
                const int gy = tp.oy0 + hy - 1, gx = tp.ox0 + hx - 1;
                const bool ok = tp.ok && ch_ok && h_yx[i] >= 0 && gy >= 0 && gy < p.h && gx >= 0 && gx < p.w_in;
                const long long e = ok ? ((long long)(tp.nimg * p.h + gy) * p.w_in + gx) * pitch + c0 : 0;   // branch-free: masked units read element 0
                hreg[kc][i] = *reinterpret_cast<const uint4*>(xsrc + e * 2);
                hmask |= (ok ? 1u : 0u) << (kc * H_PER + i);
            }
        }
    };
    auto halo_store = [&]() {
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc)
#pragma unroll
            for (int i = 0; i < H_PER; ++i) {
                const int u = th + 256 * i;
                const bool keep = (hmask >> (kc * H_PER + i)) & 1u;
                uint4 v = hreg[kc][i];
                v.x = keep ? v.x : 0u; v.y = keep ? v.y : 0u; v.z = keep ? v.z : 0u; v.w = keep ? v.w : 0u;
                if ((i + 1) * 256 <= HCH || u < HCH)
                    *reinterpret_cast<uint4*>(halo + kc * PLANE + lds_row_off(u >> 2, u & 3)) = v;
            }
    };

    const int lane_off = lds_row_off(lr, lq);
    // ---- the two halves run HALF AN ITERATION APART (waves w and w + 4 share a SIMD): while one half is in its output
    // stores, its next halo's address arithmetic and the first MFMA steps, the other is in the middle of its MFMAs.  In
    // lockstep all eight waves stored at once (store issue, not bandwidth, paces a burst of 16-byte stores from every wave of
    // a CU) and the matrix pipe idled meanwhile.  s_barrier is workgroup-wide, so every step carries two barriers: in a P0 step
    // they bracket the half's own halo write, in a P1 step they are the other half's.
    //   P0: [barrier] registers -> halo [barrier] request the next halo; first half of the (chunk, tap) steps
    //   P1: [barrier] [barrier] second half of the steps; epilogue
    // half 0 runs P0 on even steps, half 1 on odd steps; 2 * iterations + 1 steps in all.
    // STAG = false: both halves in step (P1 then needs no barriers).  Measured per instantiation (tools/experiments/README.md): the stagger
    // pays where the MFMA share is largest (two K chunks x 64 channels: 1.03 -> 0.86 ms on the 64 -> 64 convs) and costs
    // 10 - 20 % on the single-chunk and narrow tiles, whose phases are too short for four barriers per tile.
    constexpr int STEPS = 9 * NKC, S0 = (STEPS + 1) / 2;
    int k = 0;
    int pr = pair_of(0), prn = -1;
    int iters = 0;
    {
        const int lim0 = npairs - wx * band, lim = lim0 < band ? lim0 : band;
        iters = lim > wi ? (lim - wi + per_xcd - 1) / per_xcd : 0;
    }
    TilePos cur = tile_pos(pr), nxt = cur;
    if (pr >= 0) halo_load(cur);
    float4v acc[WCO][WPX];
    bool busy = false;   // this half is between its P0 and its P1
    // B-fragment addressing with no per-read arithmetic (as conv3x3_halo_body): a lane reads halo pixel x + C (x its pixel at
    // tap (0, 0) of the wave's first sub-tile, C a compile-time offset) at (x + C) * 64 + ((lq ^ (swz(x + C) << 1)) << 4),
    // swz(v) = (v >> 2) & 1 = swz(x) ^ ((C >> 2) & 1) ^ carry(x & 3, C & 3): eight per-lane bases + immediates
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
    auto mma_steps = [&](int s0, int s1) {
#pragma unroll
        for (int s = s0; s < s1; ++s) {
            const int kc = s / 9, tap = s - kc * 9;
            const int dy = tap / 3, dx = tap - dy * 3;
            frag_t fa[WCO];
#pragma unroll
            for (int i = 0; i < WCO; ++i) fa[i] = lds_frag<frag_t>(wlds + (tap * NKC + kc) * W_SLICE + i * 1024 + lane_off);
#pragma unroll
            for (int j = 0; j < WPX; ++j) {
                const int C = ((j >> 1) + dy) * HX + (j & 1) * 16 + dx;
                const frag_t fb = lds_frag<frag_t>(halo + kc * PLANE + bb[C & 3][(C >> 2) & 1] + C * 64);
#pragma unroll
                for (int i = 0; i < WCO; ++i) mma_tile(acc[i][j], fa[i], fb);
            }
        }
    };
    for (int step = 0; step < 2 * iters + (STAG ? 1 : 0); ++step) {
        if (((step + (STAG ? half_id : 0)) & 1) == 0) {
            __syncthreads();          // this half is past its reads of the previous tile's halo (first time: the weights are written)
            if (pr >= 0) halo_store();
            __syncthreads();
            if (pr >= 0) {
                prn = pair_of(++k);
                nxt = tile_pos(prn);
                if (prn >= 0) halo_load(nxt);   // in flight until this half's next P0
#pragma unroll
                for (int i = 0; i < WCO; ++i)
#pragma unroll
                    for (int j = 0; j < WPX; ++j) acc[i][j] = (float4v){bv[i][0], bv[i][1], bv[i][2], bv[i][3]};
                mma_steps(0, S0);
                busy = true;
            }
        } else {
            if constexpr (STAG) {
                __syncthreads();
                __syncthreads();
            }
            if (busy) {
                mma_steps(S0, STEPS);
                // ---- epilogue: ReLU, f16, the lane's 4 * WCO contiguous channels of each of its four pixels
                if (cur.ok) {
#pragma unroll
                    for (int j = 0; j < WPX; ++j) {
                        const int oy = cur.oy0 + w_px * ROWS + (j >> 1), ox = cur.ox0 + (j & 1) * 16 + lr;
                        if (oy >= p.ho || ox >= p.wo) continue;
                        half_t o[4 * WCO];
#pragma unroll
                        for (int i = 0; i < WCO; ++i)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                float v = acc[i][j][r];
                                if (p.act == 3) v = fmaxf(v, 0.f);
                                o[i * 4 + r] = (half_t)v;
                            }
                        const int cl = co0 + lq * 4 * WCO;
                        half_t* op = (half_t*)p.out + ((long long)(cur.nimg * p.ho + oy) * p.wo + ox) * p.cout_pitch + cl;
                        if constexpr (WCO == 1) {
                            if (cl < p.cout_pitch) *reinterpret_cast<uint2*>(op) = *reinterpret_cast<const uint2*>(o);
                        } else {
#pragma unroll
                            for (int v8 = 0; v8 < WCO / 2; ++v8)
                                if (cl + 8 * v8 < p.cout_pitch) *reinterpret_cast<uint4*>(op + 8 * v8) = *reinterpret_cast<const uint4*>(o + 8 * v8);
                        }
                    }
                }
                pr = prn;
                cur = nxt;
                busy = false;
            }
        }
    }
}

// Which convs run here: narrow f16 3x3 layers on large images, nothing fused but bias and ReLU.
inline bool ws_shape_ok(const elvis_conv_desc* d) {
    if (d->dtype != ELVIS_F16 || d->ksize != 3 || d->stride != 1 || d->pad_before != 1 || d->upsample || d->prologue) return false;
    if (d->ho != d->h || d->wo != d->w || (d->act != 0 && d->act != 3)) return false;
    if (choose_tile(d->cout).tco > 64) return false;
    if (conv_nkc32(d) > 2 || (d->cin_pitch & 7) || (d->cin2 > 0 && (d->cin2_pitch & 7)) || (d->cout_pitch & 7)) return false;
    return (long long)d->ho * d->wo >= 128 * 1024;   // per image (never per batch: the kernel choice must not depend on n)
}

// the halves run half an iteration apart where measured faster: two K chunks x a 64-channel tile
constexpr bool ws_stagger(int nkc, int tco) { return nkc == 2 && tco == 64; }
constexpr int WS_TY = 8;   // the host sizes the grid for 8 x HALO_TX pixel tiles, the TY x TX of the kernel

template <int NKC, int TCO> int launch_ws(const ConvArgs& a, hipStream_t stream, ConvPick* query) {
    constexpr bool STAG = ws_stagger(NKC, TCO);
    static const ElvisKernelName name("conv3x3_ws_kernel<%d,%d,%s>", NKC, TCO, tf(STAG));
    if (query) return query->set(name.s, WS_TY);
    constexpr size_t lds = (size_t)NKC * 9 * TCO * 64 + 2 * (size_t)NKC * 340 * 64;
    static ElvisLdsOptIn opt_in;
    static std::atomic<int> ncu[64];   // compute units per device: every thread that asks first stores the same value
    const int dev = elvis_device_slot();
    if (int rc = elvis_lds_opt_in((const void*)conv3x3_ws_kernel<NKC, TCO, STAG>, opt_in, dev, "conv3x3_ws: device setup failed")) return rc;
    int n_cu = ncu[dev].load(std::memory_order_relaxed);
    if (n_cu == 0) {
        hipError_t e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess || n_cu <= 0) {
            elvis_set_error("conv3x3_ws: device setup failed: %s", hipGetErrorString(e));
            return ELVIS_E_RUNTIME;
        }
        ncu[dev].store(n_cu, std::memory_order_relaxed);
    }
    const long long ntiles = (long long)a.n * a.tiles_y * a.tiles_x;
    ELVIS_REQUIRE(ntiles < 0x3fffffffLL, "conv: grid too large");
    int nworkers = n_cu / a.n_co_tiles;
    const long long npairs = (ntiles + 1) / 2;
    if (nworkers > npairs) nworkers = (int)npairs;
    ELVIS_REQUIRE(nworkers >= 1, "conv3x3_ws: more cout tiles than compute units");
    hipLaunchKernelGGL((conv3x3_ws_kernel<NKC, TCO, STAG>), dim3((unsigned)(nworkers * a.n_co_tiles)), dim3(512), lds, stream, a, (int)ntiles, nworkers);
    ELVIS_CHECK_LAUNCH("elvis_conv2d(ws)");
    elvis_note_launch(name.s);
    return ELVIS_OK;
}

inline int dispatch_ws(const ConvArgs& a, int tco, hipStream_t stream, ConvPick* query) {
    if (a.nkc == 1) {
        if (tco == 64) return launch_ws<1, 64>(a, stream, query);
        if (tco == 32) return launch_ws<1, 32>(a, stream, query);
        return launch_ws<1, 16>(a, stream, query);
    }
    if (tco == 64) return launch_ws<2, 64>(a, stream, query);
    if (tco == 32) return launch_ws<2, 32>(a, stream, query);
    return launch_ws<2, 16>(a, stream, query);
}

}  // namespace
