// Exact nearest-code search through a uniform grid over the codebook (c == 3).
//
// The codebook is a weight: elvis_vq_index_build runs once per loaded model and lays the codes out by grid cell (CSR: cell
// c holds entries [start[c], start[c + 1]), code ids ascending inside a cell, every entry the code's three coordinates and
// its id).  elvis_vq_nearest_indexed gives, value for value, what elvis_vq_nearest's scan of all codes gives:
//
//   * a candidate's distance is the scan's expression, ((dx dx) + dy dy) + dz dz with one IEEE rounding per operation
//     (__fsub_rn, __fmul_rn, __fadd_rn), so every code has the same rounded distance d^ in both kernels;
//   * the scan returns the first minimum: the least (d^, id) in lexicographic order among the codes with d^ < 3.0e38.  That
//     is a total order, so any visiting order that keeps the lexicographic minimum returns it too - as long as no code that
//     could be that minimum is left out;
//   * one lane works one pixel p.  It searches its own cell, then the Chebyshev shells of cells around it.  After shell r it
//     has seen every code of the cube of cells [ci - r, ci + r]^3.  A code q it has not seen lies in a cell beyond one of the
//     cube's faces, say beyond the plane x = e on axis x: cells are assigned from the very edge values the kernel reads
//     (edge[i] <= q_x <= edge[i + 1] for a code of cell i, exactly), so |p_x - q_x| >= |p_x - e| in real numbers.  Rounding
//     to nearest is monotone, hence |fl(p_x - q_x)| >= |fl(p_x - e)|, fl(dx dx) >= fl(g g) with g = fl(p_x - e), and adding
//     the two other (non-negative) squares, each sum rounded, never takes the value below its first operand: d^(q) >=
//     fl(g g).  The least of fl(g g) over the faces that still have cells beyond them is therefore a lower bound of every
//     unseen d^ with NO allowance for the three roundings of the distance; the kernel still lowers it by the factor
//     (1 - 1e-5), about 170 ulp, far more than the 3 half-ulps those roundings could ever move a sum - slack that costs a
//     few extra shells at most.  The search stops when that lowered bound is > the best d^ so far (strictly: an unseen code
//     that ties the best with a smaller id must still be visited);
//   * pixels outside the codebook's bounding box take the nearest border cell; their gaps to the faces that matter only
//     grow.  Clustered or duplicate codes make cells long, not wrong.
//
// Non-finite latents are outside the contract of both entries (the scan leaves its sentinel index); here they end the
// search early and write code 0's coordinates with the sentinel index, without reading out of bounds.
#include <math.h>
#include <string.h>
#include <cmath>
#include <algorithm>
#include <vector>
#include "common.h"

namespace {

constexpr int VQG_MAX = 16;                    // cells per axis, at most
constexpr int VQG_HEADER_WORDS = 64;           // [0] G, [1] n_embed, [4 .. 4 + 3 * 17) the edges of the three axes
constexpr int VQG_SENTINEL = 0x7fffffff;

inline int vq_grid_cells(int n_embed) {
    int g = (int)lround(cbrt((double)n_embed / 2.0));   // about two codes a cell: 16^3 cells for 8192 codes
    return g < 1 ? 1 : (g > VQG_MAX ? VQG_MAX : g);
}
__host__ __device__ inline size_t vq_grid_entry_word(int g) { return (size_t)(VQG_HEADER_WORDS + g * g * g + 1 + 3) / 4 * 4; }

// cell of coordinate x on an axis with edges e[0 .. G]: the number of inner edges e[1 .. G - 1] that are <= x
__host__ __device__ inline int vq_grid_cell(const float* e, int g, float x) {
    int i = 0;
    for (int j = 1; j < g; ++j) i += x >= e[j] ? 1 : 0;
    return i;
}

template <typename T>
__global__ __launch_bounds__(256) void vq_grid_nearest_kernel(const T* __restrict__ z, T* __restrict__ zq,
                                                              int32_t* __restrict__ idx_out, long long pixels, int pitch_in,
                                                              int pitch_out, const int* __restrict__ index) {
    __shared__ float edge[3][VQG_MAX + 1];
    if (threadIdx.x < 3 * (VQG_MAX + 1))
        (&edge[0][0])[threadIdx.x] = reinterpret_cast<const float*>(index)[4 + threadIdx.x];
    __syncthreads();
    const long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (px >= pixels) return;
    const int G = index[0];
    const int* __restrict__ start = index + VQG_HEADER_WORDS;
    const float4* __restrict__ ent = reinterpret_cast<const float4*>(index + vq_grid_entry_word(G));
    float p[3];
    int ci[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        p[d] = to_f(z[px * pitch_in + d]);
        ci[d] = vq_grid_cell(edge[d], G, p[d]);
    }
    float best = 3.0e38f;
    int best_i = VQG_SENTINEL, best_e = 0;
    auto scan = [&](int e0, int e1) {
        for (int e = e0; e < e1; ++e) {
            const float4 q = ent[e];
            const float dx = __fsub_rn(p[0], q.x), dy = __fsub_rn(p[1], q.y), dz = __fsub_rn(p[2], q.z);
            const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            const int id = __float_as_int(q.w);
            // the scan's `d < best`, and among equal distances the smaller id (never against the sentinel: the scan takes
            // no code at d >= 3.0e38)
            if (d < best || (d == best && id < best_i && best_i != VQG_SENTINEL)) {
                best = d;
                best_i = id;
                best_e = e;
            }
        }
    };
    for (int r = 0; r < G; ++r) {
        const int i0 = max(ci[0] - r, 0), i1 = min(ci[0] + r, G - 1);
        const int j0 = max(ci[1] - r, 0), j1 = min(ci[1] + r, G - 1);
        const int k0 = max(ci[2] - r, 0), k1 = min(ci[2] + r, G - 1);
        for (int i = i0; i <= i1; ++i) {
            for (int j = j0; j <= j1; ++j) {
                const int row = (i * G + j) * G;
                if (abs(i - ci[0]) < r && abs(j - ci[1]) < r) {
                    // inside the shell's hull on both other axes: only the two end cells of the row are new
                    const int ka = ci[2] - r, kb = ci[2] + r;
                    if (ka >= 0) scan(start[row + ka], start[row + ka + 1]);
                    if (kb < G) scan(start[row + kb], start[row + kb + 1]);
                } else {
                    scan(start[row + k0], start[row + k1 + 1]);   // cells k0 .. k1 of a row are adjacent in the CSR
                }
            }
        }
        // the least rounded squared gap to a face of the searched cube that still has cells beyond it
        float lb = INFINITY;
        bool open = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int a = ci[d] - r, b = ci[d] + r + 1;
            if (a >= 1) {
                const float g = fmaxf(__fsub_rn(p[d], edge[d][a]), 0.f);
                lb = fminf(lb, __fmul_rn(g, g));
                open = true;
            }
            if (b <= G - 1) {
                const float g = fmaxf(__fsub_rn(edge[d][b], p[d]), 0.f);
                lb = fminf(lb, __fmul_rn(g, g));
                open = true;
            }
        }
        if (!open || __fmul_rn(lb, 0.99999f) > best) break;
    }
    if (idx_out) idx_out[px] = best_i;
    const float4 q = ent[best_e];
    T* o = zq + px * pitch_out;
    o[0] = from_f<T>(q.x);
    o[1] = from_f<T>(q.y);
    o[2] = from_f<T>(q.z);
    for (int k = 3; k < pitch_out; ++k) o[k] = from_f<T>(0.f);
}

}  // namespace

extern "C" size_t elvis_vq_index_bytes(int n_embed, int c) {
    if (n_embed <= 0 || c != 3) return 0;
    return (vq_grid_entry_word(vq_grid_cells(n_embed)) + (size_t)n_embed * 4) * 4;
}

extern "C" int elvis_vq_index_build(const float* codebook, int n_embed, int c, void* workspace, elvis_stream_t stream) {
    ELVIS_REQUIRE(codebook && workspace && n_embed > 0, "elvis_vq_index_build: bad argument");
    ELVIS_REQUIRE(c == 3, "elvis_vq_index_build: the grid is three-dimensional (c = %d)", c);
    ELVIS_REQUIRE((uintptr_t)workspace % 16 == 0, "elvis_vq_index_build: workspace must be 16-byte aligned");
    std::vector<float> cb((size_t)n_embed * 3);
    if (hipMemcpyAsync(cb.data(), codebook, cb.size() * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
        elvis_set_error("elvis_vq_index_build: reading the codebook failed");
        return ELVIS_E_RUNTIME;
    }
    for (float v : cb) ELVIS_REQUIRE(std::isfinite(v), "elvis_vq_index_build: the codebook holds a non-finite value");
    const int G = vq_grid_cells(n_embed);
    const size_t words = elvis_vq_index_bytes(n_embed, c) / 4;
    std::vector<int32_t> img(words, 0);
    img[0] = G;
    img[1] = n_embed;
    float* edges = reinterpret_cast<float*>(img.data()) + 4;
    for (int d = 0; d < 3; ++d) {
        float lo = cb[d], hi = cb[d];
        for (int k = 1; k < n_embed; ++k) {
            lo = std::min(lo, cb[(size_t)k * 3 + d]);
            hi = std::max(hi, cb[(size_t)k * 3 + d]);
        }
        float* e = edges + d * (VQG_MAX + 1);
        for (int i = 0; i <= VQG_MAX; ++i) {
            // uniform edges, non-decreasing; e[0] = lo and e[G ..] = hi exactly, so every code lies in [e[i], e[i + 1]] of its cell
            float v = i >= G ? hi : (float)((double)lo + ((double)hi - (double)lo) * i / G);
            if (i > 0 && v < e[i - 1]) v = e[i - 1];
            e[i] = std::min(v, hi);
        }
        e[0] = lo;
    }
    std::vector<int> cell(n_embed);
    int32_t* start = img.data() + VQG_HEADER_WORDS;
    for (int k = 0; k < n_embed; ++k) {
        int id = 0;
        for (int d = 0; d < 3; ++d) id = id * G + vq_grid_cell(edges + d * (VQG_MAX + 1), G, cb[(size_t)k * 3 + d]);
        cell[k] = id;
        ++start[id + 1];
    }
    const int ncell = G * G * G;
    for (int i = 0; i < ncell; ++i) start[i + 1] += start[i];
    std::vector<int> fill(start, start + ncell);
    float* ent = reinterpret_cast<float*>(img.data() + vq_grid_entry_word(G));
    for (int k = 0; k < n_embed; ++k) {        // ascending k: ids ascend inside a cell
        float* q = ent + (size_t)fill[cell[k]]++ * 4;
        q[0] = cb[(size_t)k * 3 + 0];
        q[1] = cb[(size_t)k * 3 + 1];
        q[2] = cb[(size_t)k * 3 + 2];
        memcpy(q + 3, &k, 4);
    }
    // on the caller's stream, and waited for: the host image dies at return
    if (hipMemcpyAsync(workspace, img.data(), words * 4, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
        elvis_set_error("elvis_vq_index_build: writing the index failed");
        return ELVIS_E_RUNTIME;
    }
    return ELVIS_OK;
}

extern "C" int elvis_vq_nearest_indexed(const void* z, void* zq, int32_t* idx_out, int dtype, long long pixels, int c,
                                        int pitch_in, int pitch_out, const float* codebook, int n_embed, const void* index,
                                        elvis_stream_t stream) {
    ELVIS_REQUIRE(z && zq && codebook && index && pixels > 0 && n_embed > 0, "elvis_vq_nearest_indexed: bad argument");
    ELVIS_REQUIRE(c == 3 && pitch_in >= c && pitch_out >= c, "elvis_vq_nearest_indexed: the index serves c = 3 (got %d)", c);
    ELVIS_REQUIRE((uintptr_t)index % 16 == 0, "elvis_vq_nearest_indexed: index must be 16-byte aligned");
    ELVIS_REQUIRE(pixels <= 0x7fffffffLL * 256, "elvis_vq_nearest_indexed: too many pixels");
    const unsigned grid = (unsigned)((pixels + 255) / 256);
    if (dtype == ELVIS_F16)
        hipLaunchKernelGGL(vq_grid_nearest_kernel<half_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const half_t*)z,
                           (half_t*)zq, idx_out, pixels, pitch_in, pitch_out, (const int*)index);
    else if (dtype == ELVIS_F32)
        hipLaunchKernelGGL(vq_grid_nearest_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)z,
                           (float*)zq, idx_out, pixels, pitch_in, pitch_out, (const int*)index);
    else
        ELVIS_REQUIRE(false, "elvis_vq_nearest_indexed: bad dtype");
    ELVIS_CHECK_LAUNCH("elvis_vq_nearest_indexed");
    elvis_note_launch(dtype == ELVIS_F16 ? "vq_grid_nearest_kernel<half>" : "vq_grid_nearest_kernel<float>");
    return ELVIS_OK;
}
