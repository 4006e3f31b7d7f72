// GroupNorm, one-buffer case: a conv's per-tile partial sums -> the per-(n, channel) affine (pa, pb) in ONE launch.
//
// The two-launch path (norm.hip: gn_partials_reduce[4]_kernel, then gn_affine_kernel) stays for concatenated inputs and for
// inputs whose sums come from gn_channel_sums_kernel.  This kernel restates both steps with the same operations in the
// same order, so pa / pb are bit-identical:
//   * per channel and statistic, 256 virtual lanes; lane v adds the tiles t = v, v + 256, ... in ascending order, in fp64,
//     starting from 0 (gn_partials_reduce_kernel's thread loop);
//   * the binary tree  lane[v] += lane[v + o], o = 128 ... 1  (its LDS loop);
//   * the group's sum over its cpg channels in ascending channel order, from 0, then gn_affine_kernel's arithmetic.
// What changes is who holds a virtual lane.  A workgroup spans CB >= 16 channels (whole groups), F = 2 CB floats of every
// partials row, and thread (f, r) - float f of the span, row lane r < RL - owns the virtual lanes v = r + RL k, k < 256 / RL,
// as 256 / RL fp64 registers.  A wave then reads whole contiguous spans of 2 CB floats (128 bytes at CB = 16) of RL rows per
// load instead of 32 bytes of each of 64 rows.  The tree's levels o >= RL pair two lanes of ONE thread (v + o = r + RL (k +
// o / RL)); only the last log2(RL) levels cross threads, through LDS, with the same pairing.
#include "common.h"

namespace {

constexpr int GNF_MAX_F = 64;   // floats of a row a workgroup spans: cpg <= 32

template <int RL>
__global__ __launch_bounds__(256) void gn_partials_affine_kernel(const float* __restrict__ partials, int tiles_per_image,
                                                                 int c, int cb, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta,
                                                                 const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, float* __restrict__ pa,
                                                                 float* __restrict__ pb, int hw, int groups, float eps) {
    constexpr int K = 256 / RL;
    __shared__ double red[RL][GNF_MAX_F];
    __shared__ double tot[GNF_MAX_F];
    const int n = blockIdx.y, ch0 = blockIdx.x * cb, tid = threadIdx.x;
    const int span = (c - ch0 < cb ? c - ch0 : cb) * 2;   // floats of a row this workgroup reads (the last one may be short)
    const int F = cb * 2;
    const int r = tid / F, f = tid - r * F;
    const bool active = r < RL && f < span;
    if (active) {
        double acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0;
        // Lane v's tiles in ascending order, as the old loop.  The loads of a sweep over 256 rows (two sweeps where the
        // registers allow) are all issued before the first add, and the ragged last sweep clamps its row and selects the
        // result instead of branching around the load: a branch per load makes the compiler wait for each one in turn.
        const float* base = partials + ((long long)n * tiles_per_image * c + ch0) * 2 + f + (long long)r * c * 2;
        const long long kstride = (long long)RL * c * 2, sweep = 256LL * c * 2;
        int t0 = 0;
        if constexpr (K <= 32) {
            for (; t0 + 512 <= tiles_per_image; t0 += 512) {
                float v0[K], v1[K];
                const float* b = base + (long long)t0 * c * 2;
#pragma unroll
                for (int k = 0; k < K; ++k) v0[k] = b[k * kstride];
#pragma unroll
                for (int k = 0; k < K; ++k) v1[k] = b[sweep + k * kstride];
                __builtin_amdgcn_sched_barrier(0);   // keep every load ahead of the adds: the scheduler would interleave them
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] += (double)v0[k];
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] += (double)v1[k];
            }
        }
        for (; t0 + 256 <= tiles_per_image; t0 += 256) {
            float v[K];
            const float* b = base + (long long)t0 * c * 2;
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = b[k * kstride];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] += (double)v[k];
        }
        if (t0 < tiles_per_image) {
            float v[K];
            const float* b = base + (long long)t0 * c * 2;
            const int left = tiles_per_image - t0 - r;   // rows r + RL k < left exist; row t0 itself always does
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const long long off = RL * k < left ? k * kstride : -(long long)r * c * 2;
                v[k] = b[off];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = RL * k < left ? acc[k] + (double)v[k] : acc[k];
        }
        // tree levels o = 128 ... RL: lane v = r + RL k meets v + o = r + RL (k + o / RL)
#pragma unroll
        for (int o = K / 2; o > 0; o >>= 1) {
#pragma unroll
            for (int k = 0; k < o; ++k) acc[k] += acc[k + o];
        }
        red[r][f] = acc[0];
    }
    __syncthreads();
    // levels o = RL / 2 ... 1: lane r meets r + o
    for (int o = RL / 2; o > 0; o >>= 1) {
        if (active && r < o) red[r][f] += red[r + o][f];
        __syncthreads();
    }
    if (tid < span) tot[tid] = red[0][tid];
    __syncthreads();
    if (tid * 2 < span) {
        // gn_affine_kernel, line for line, on the sums this workgroup holds
        const int ch = ch0 + tid;
        const int i = n * c + ch;
        const int cpg = c / groups;
        const int g = ch / cpg;
        double s = 0, ss = 0;
        for (int k = 0; k < cpg; ++k) {
            s += tot[(g * cpg + k - ch0) * 2 + 0];
            ss += tot[(g * cpg + k - ch0) * 2 + 1];
        }
        double cnt = (double)hw * cpg;
        double mean = s / cnt;
        double var = ss / cnt - mean * mean;
        if (var < 0) var = 0;
        float rstd = (float)(1.0 / sqrt(var + (double)eps));
        float ga = gamma ? gamma[ch] : 1.f, be = beta ? beta[ch] : 0.f;
        float a = rstd * ga;
        float b = be - (float)mean * a;
        if (scale) {
            float sc = 1.f + scale[ch];
            a *= sc;
            b = b * sc + (shift ? shift[ch] : 0.f);
        } else if (shift) {
            b += shift[ch];
        }
        pa[i] = a;
        pb[i] = b;
    }
}

}  // namespace

// Channels a workgroup spans for c / groups = cpg: the smallest multiple of cpg that is >= 16 (whole groups, and at least
// one 128-byte line of a partials row); 0 when a group is wider than the kernel's span.
extern "C" int elvis_gn_partials_affine_span(int c, int groups) {
    if (c <= 0 || groups <= 0 || c % groups) return 0;
    const int cpg = c / groups;
    if (cpg * 2 > GNF_MAX_F) return 0;
    return (16 + cpg - 1) / cpg * cpg;
}

extern "C" int elvis_gn_partials_affine(const float* partials, int tiles_per_image, const float* gamma, const float* beta,
                                        const float* scale, const float* shift, float* pa, float* pb, int n, int hw, int c,
                                        int groups, float eps, elvis_stream_t stream) {
    ELVIS_REQUIRE(partials && pa && pb, "elvis_gn_partials_affine: null pointer");
    ELVIS_REQUIRE(tiles_per_image > 0 && n > 0 && hw > 0 && c > 0 && groups > 0 && c % groups == 0,
                  "elvis_gn_partials_affine: c=%d not divisible by groups=%d", c, groups);
    const int cb = elvis_gn_partials_affine_span(c, groups);
    ELVIS_REQUIRE(cb > 0, "elvis_gn_partials_affine: %d channels per group (at most %d)", c / groups, GNF_MAX_F / 2);
    const dim3 grid((c + cb - 1) / cb, n);
    if (cb * 2 <= 32) {
        hipLaunchKernelGGL(gn_partials_affine_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, partials, tiles_per_image, c,
                           cb, gamma, beta, scale, shift, pa, pb, hw, groups, eps);
        ELVIS_CHECK_LAUNCH("elvis_gn_partials_affine");
        elvis_note_launch("gn_partials_affine_kernel<8>");
    } else {
        hipLaunchKernelGGL(gn_partials_affine_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, partials, tiles_per_image, c,
                           cb, gamma, beta, scale, shift, pa, pb, hw, groups, eps);
        ELVIS_CHECK_LAUNCH("elvis_gn_partials_affine");
        elvis_note_launch("gn_partials_affine_kernel<4>");
    }
    return ELVIS_OK;
}
