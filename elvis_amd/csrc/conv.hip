// C ABI of the conv kernels (elvis_conv2d and friends) + the f16 instantiations; the fp32 / compensated-f16
// instantiations live in conv_f32.hip.  Kernels, leaf launchers and the descriptor predicates: conv_kernels.inc.
//
// One path from a call to its kernel: conv_path() picks the family from the descriptor and the call's two flags,
// conv_plan() builds the kernels' argument block, conv_walk() goes down the launch tree to a leaf launcher.  elvis_conv2d
// walks it to launch; the name query and elvis_conv_stats_tiles walk the same tree with a ConvPick, which the leaf answers
// with its own name and tile height instead of launching.  Nothing here names a kernel or knows a tile height: to change
// one edit halo_tile_rows() and the constants beside it (conv_kernels.inc).
#include "conv_kernels.inc"
#include "conv_ws.inc"
#include <string.h>

// conv_f32.hip: halo != 0 -> launch_x3p<tco> / launch_halo<float, tco>, else dispatch<float>(id); query: a ConvPick* or null
__attribute__((visibility("hidden"))) int elvis_conv_launch_f32_(const void* conv_args, int halo, int tco, int id, hipStream_t stream, void* query);
// conv_f32.hip: the planar compensated form's weight packing (conv_x3p.inc)
__attribute__((visibility("hidden"))) int elvis_conv_pack_x3p_(const float* w_oihw, void* packed, int cout, int ctot, int nkc, int n_co_tiles,
                                                              int tco, int taps, hipStream_t stream);

// elvis_conv_debug_set("no_halo", 1) sends every conv to the generic implicit-GEMM kernel (tests compare the halo
// kernels with it); 0 or -1 restores the default dispatch.
#include <atomic>
static std::atomic<int> g_no_halo{0};
static bool no_halo() { return g_no_halo.load(std::memory_order_relaxed) > 0; }
extern "C" int elvis_conv_debug_set(const char* key, int value) {
    ELVIS_REQUIRE(key, "elvis_conv_debug_set: null key");
    if (!strcmp(key, "no_halo")) { g_no_halo.store(value, std::memory_order_relaxed); return ELVIS_OK; }
    ELVIS_REQUIRE(false, "elvis_conv_debug_set: unknown key '%s'", key);
}

static void conv_geom(const elvis_conv_desc* d, int* nkc1, int* nkc, int* co_pad) {
    int kc = kc_of(d);
    *nkc1 = (d->cin + kc - 1) / kc;
    *nkc = *nkc1 + (d->cin2 > 0 ? (d->cin2 + kc - 1) / kc : 0);
    TileCfg t = choose_tile(d->cout);
    *co_pad = ((d->cout + t.tco - 1) / t.tco) * t.tco;
}

extern "C" size_t elvis_conv_packed_weight_bytes(const elvis_conv_desc* d) {
    if (!d || d->cin <= 0 || d->cout <= 0) return 0;
    int nkc1, nkc, co_pad;
    conv_geom(d, &nkc1, &nkc, &co_pad);
    return (size_t)d->ksize * d->ksize * nkc * co_pad * (x3_planar_fmt(d) ? 128 : 64);   // planar: a hi and a lo row per 32 channels
}

extern "C" int elvis_conv_pack_weights(const elvis_conv_desc* d, const float* w_oihw, void* packed,
                                       elvis_stream_t stream) {
    int rc = validate(d);
    if (rc) return rc;
    ELVIS_REQUIRE(w_oihw && packed, "elvis_conv_pack_weights: null pointer");
    int nkc1, nkc, co_pad;
    conv_geom(d, &nkc1, &nkc, &co_pad);
    if (x3_planar_fmt(d)) {
        const int tco = choose_tile(d->cout).tco;
        return elvis_conv_pack_x3p_(w_oihw, packed, d->cout, d->cin + d->cin2, nkc, co_pad / tco, tco, d->ksize * d->ksize, (hipStream_t)stream);
    }
    int KC = kc_elems(d->dtype);
    // with two inputs the packed K axis is [cin padded to nkc1*KC | cin2]; cin % KC == 0 is
    // enforced in that case so the source channel index is simply ci.
    long long total = (long long)d->ksize * d->ksize * nkc * co_pad * KC;
    int grid = (int)((total + 255) / 256);
    int ctot = d->cin + d->cin2;
    const int tco_ = choose_tile(d->cout).tco, wco = tco_ >= 64 ? 4 : tco_ / 16;   // 16-row fragments per wave (all kernels agree)
    if (d->dtype == ELVIS_F16)
        hipLaunchKernelGGL(pack_weights_kernel<half_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w_oihw,
                           (half_t*)packed, d->cout, ctot, d->ksize, nkc, co_pad, KC, total, wco);
    else
        hipLaunchKernelGGL(pack_weights_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w_oihw,
                           (float*)packed, d->cout, ctot, d->ksize, nkc, co_pad, KC, total, wco, d->dtype == ELVIS_F32X3 ? 1 : 0);
    ELVIS_CHECK_LAUNCH("elvis_conv_pack_weights");
    return ELVIS_OK;
}

// Does a descriptor with dtype ELVIS_F32X3 run on a compensated-f16 kernel?  (Its weights are packed as (hi, lo)
// half pairs, which only those kernels read: a host keeps the ELVIS_F32 packing for everything else.)
static bool x3_eligible(const elvis_conv_desc* d) {
    if (!(d->dtype == ELVIS_F32X3 && halo_eligible(d) && !no_halo() && choose_tile(d->cout).tco >= 64)) return false;
    // a layer packed in the planar format runs on the planar kernel only (plain 3x3 / stride 1 / pad 1 geometry)
    return !x3_planar_fmt(d) || x3_planar_run(d);
}
extern "C" int elvis_conv_x3_eligible(const elvis_conv_desc* d) {
    if (!d || validate(d)) return 0;
    return x3_eligible(d) ? 1 : 0;
}

// The one rule that picks a conv's kernel family.  A call with a residual or a statistics buffer never runs on the
// weight-stationary kernel (it fuses neither): such a call of a ws-eligible shape lands on the halo kernel.
enum class ConvPath { WS, HALO, IGEMM };
static ConvPath conv_path(const elvis_conv_desc* d, bool has_residual, bool has_stats) {
    if (no_halo()) return ConvPath::IGEMM;
    if (ws_shape_ok(d) && !has_residual && !has_stats) return ConvPath::WS;   // narrow layer, large image: persistent weight-stationary kernel
    return halo_eligible(d) ? ConvPath::HALO : ConvPath::IGEMM;
}

// Down the launch tree to the leaf.  query == nullptr: the leaf launches on `stream`; else it fills *query, no HIP call.
static int conv_walk(const elvis_conv_desc* d, ConvPath path, const ConvArgs& a, hipStream_t stream, ConvPick* query) {
    const TileCfg t = choose_tile(d->cout);
    const bool f16 = d->dtype == ELVIS_F16;
    if (path == ConvPath::WS) return dispatch_ws(a, t.tco, stream, query);
    if (path == ConvPath::IGEMM) return f16 ? dispatch<half_t>(a, t.id, stream, query) : elvis_conv_launch_f32_(&a, 0, t.tco, t.id, stream, query);
    if (!f16) return elvis_conv_launch_f32_(&a, 1, t.tco, t.id, stream, query);
    switch (t.tco) {
        case 128: return launch_halo<half_t, 128>(a, stream, query);
        case 64: return launch_halo<half_t, 64>(a, stream, query);
        case 32: return launch_halo<half_t, 32>(a, stream, query);
        default: return launch_halo<half_t, 16>(a, stream, query);
    }
}

// The argument block as far as it follows from the descriptor and the path (the caller adds pointers and residual
// pitch), and the leaf the call resolves to: the pixel-tile grid is sized from the tile height that leaf reports.
static int conv_plan(const elvis_conv_desc* d, ConvPath path, ConvArgs& a, ConvPick& pick) {
    a.n = d->n; a.h = d->h; a.w_in = d->w;
    a.cin = d->cin; a.cin_pitch = d->cin_pitch; a.cin2 = d->cin2; a.cin2_pitch = d->cin2_pitch;
    a.cout = d->cout; a.cout_pitch = d->cout_pitch;
    a.ksize = d->ksize; a.stride = d->stride; a.pad = d->pad_before; a.upsample = d->upsample;
    a.ho = d->ho; a.wo = d->wo; a.act = d->act; a.prologue = d->prologue;
    conv_geom(d, &a.nkc1, &a.nkc, &a.co_pad);
    TileCfg t = choose_tile(d->cout);
    a.M = (long long)d->n * d->ho * d->wo;
    a.n_co_tiles = a.co_pad / t.tco;
    a.n_px_tiles = (a.M + t.tpx - 1) / t.tpx;
    const bool s2d = d->ksize == 2 && d->subpixel == ELVIS_CONV_S2D;
    const bool subpix = d->ksize == 2 && !s2d;
    a.sub = d->ksize == 2;
    a.par_a = subpix ? (d->subpixel - 1) >> 1 : 0;
    a.par_b = subpix ? (d->subpixel - 1) & 1 : 0;
    a.ostr = subpix ? 2 : 1;
    a.pad2y = subpix ? 1 - a.par_a : (s2d ? d->pad_before : 0);   // space-to-depth: pad (0,1,0,1) form 0, pad 1 form 1
    a.pad2x = subpix ? 1 - a.par_b : (s2d ? d->pad_before : 0);
    a.s2d = s2d ? 1 : 0;
    a.istr = s2d ? 2 : 1;
    a.nkc_c = s2d ? d->cin / 4 / kc_of(d) : 0x3fffffff;
    a.wfull = d->w;
    if (s2d) {   // the kernel sees the phase image: ho x wo pixels of 4C channels
        a.h = d->ho;
        a.w_in = d->wo;
    }
    a.x3 = d->dtype == ELVIS_F32X3 ? (x3_planar_run(d) ? 2 : 1) : 0;
    a.two = (halo_two(d) || halo_g1(d)) ? 1 : 0;
    a.tall = (halo_two(d) && halo_tall(d)) ? 1 : 0;
    int rc = conv_walk(d, path, a, nullptr, &pick);
    if (rc) return rc;
    a.tiles_x = ((subpix ? d->w : d->wo) + HALO_TX - 1) / HALO_TX;   // a sub-pixel parity launch covers the low-resolution grid
    a.tiles_y = pick.ty > 0 ? ((subpix ? d->h : d->ho) + pick.ty - 1) / pick.ty : 0;
    a.strip = HALO_STRIP < a.tiles_x ? HALO_STRIP : 0;
    a.strip_full = a.strip > 0 ? a.tiles_x / a.strip : 0;
    return ELVIS_OK;
}

extern "C" int elvis_conv_stats_tiles(const elvis_conv_desc* d) {
    if (!d || !halo_eligible(d)) return 0;
    ConvArgs a{};
    ConvPick pick{};
    if (conv_plan(d, ConvPath::HALO, a, pick)) return 0;   // statistics are fused by the halo family only
    return d->n * a.tiles_y * a.tiles_x;   // per parity launch for the sub-pixel form
}

extern "C" int elvis_conv_kernel_name_for_call(const elvis_conv_desc* d, int has_residual, int has_stats, char* buf, size_t n) {
    int rc = validate(d);
    if (rc) return rc;
    ELVIS_REQUIRE(buf && n > 0, "elvis_conv_kernel_name: null buffer");
    ConvArgs a{};
    ConvPick pick{};
    rc = conv_plan(d, conv_path(d, has_residual != 0, has_stats != 0), a, pick);
    if (rc) return rc;
    snprintf(buf, n, "%s", pick.name);
    return ELVIS_OK;
}

extern "C" int elvis_conv_kernel_name(const elvis_conv_desc* d, char* buf, size_t n) {
    return elvis_conv_kernel_name_for_call(d, 0, 0, buf, n);   // a call without residual and statistics
}

extern "C" int elvis_conv2d(const elvis_conv_desc* d, const void* x, const void* x2, const void* w_packed,
                            const float* bias, const void* residual, int residual_pitch, const float* pa,
                            const float* pb, void* out, float* stats, elvis_stream_t stream) {
    int rc = validate(d);
    if (rc) return rc;
    ELVIS_REQUIRE(x && w_packed && out, "elvis_conv2d: null pointer");
    ELVIS_REQUIRE(d->cin2 == 0 || x2, "elvis_conv2d: cin2 > 0 but x2 is null");
    ELVIS_REQUIRE(!d->prologue || (pa && pb), "elvis_conv2d: prologue requested without pa/pb");
    ELVIS_REQUIRE(d->dtype != ELVIS_F32X3 || x3_eligible(d),
                  "elvis_conv2d: this shape has no compensated-f16 kernel (elvis_conv_x3_eligible): run it as ELVIS_F32");
    ELVIS_REQUIRE(!residual || residual_pitch >= d->cout, "elvis_conv2d: bad residual pitch");
    ELVIS_REQUIRE(((uintptr_t)x | (uintptr_t)(x2 ? x2 : x) | (uintptr_t)w_packed | (uintptr_t)out) % 16 == 0,
                  "elvis_conv2d: pointers must be 16-byte aligned");
    const ConvPath path = conv_path(d, residual != nullptr, stats != nullptr);
    ELVIS_REQUIRE(path != ConvPath::IGEMM || !stats, "elvis_conv2d: fused statistics need a 3x3/stride-1 conv with cout >= 64 (query elvis_conv_stats_tiles)");
    ELVIS_REQUIRE(path == ConvPath::IGEMM || (long long)d->n * d->h * d->w < 0x7fffffffLL, "conv: input too large for 32-bit pixel indices");
    ConvArgs a{};
    ConvPick pick{};
    rc = conv_plan(d, path, a, pick);
    if (rc) return rc;
    a.x = x; a.x2 = x2; a.w = w_packed; a.bias = bias; a.res = residual; a.pa = pa; a.pb = pb; a.out = out;
    a.res_pitch = residual_pitch; a.stats = stats;
    return conv_walk(d, path, a, (hipStream_t)stream, nullptr);
}
