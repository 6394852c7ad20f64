// layout.hip -- polygon rasteriser behind litho_rasterize_edges: the device side of the layout import
// (lithographysimulator_amd/layout.py; SURVEY.md section 8(f) row 4 -- the reference has no counterpart, README.md:20-22
// lists GDSII import as an unbuilt goal, so there is no parity target; the checker is a CPU restatement in the test tree, bit for bit).
//
// A pixel is 1 when its centre lies inside the union of the polygons: non-zero winding number, all polygons
// counter-clockwise (the host side orients them), half-open on edges.  Two kernels, integer arithmetic after the
// crossing abscissa (so the result does not depend on the order the atomics land in):
//   k_raster_edges   one thread per edge: for every pixel row whose centre ordinate yc lies in [ymin, ymax) of the edge,
//                    the crossing x = x0 + (yc - y0) (x1 - x0) / (y1 - y0) (fp64, no contraction: Makefile) gives
//                    k = #columns whose centre is left of it; the centres left of an upward edge gain +1, of a downward
//                    edge -1:  delta[row][0] += dir, delta[row][k] -= dir  (int32 atomics, [pn][pn + 1]).
//   k_raster_fill    one workgroup per row: prefix sum of delta = winding number of every centre; geometry = (w != 0).
// litho_rasterize_coverage (further down) applies the same rule to s x s sub-centres per pixel: k_cov_edges, k_cov_fill.
#include "engine_common.hpp"
#include "../../include/litho_abbe.h"

#include <cmath>
#include <cstdint>

namespace litho {

__global__ __launch_bounds__(256) void k_raster_edges(const double* __restrict__ edges, int ne, int pn, double ox, double oy,
                                                      double ps, int* __restrict__ delta)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const double x0 = edges[4 * e], y0 = edges[4 * e + 1], x1 = edges[4 * e + 2], y1 = edges[4 * e + 3];
    // a non-finite coordinate (NaN or +-inf: inf * 0 and inf - inf below would be NaN and the cast to int undefined) or a
    // horizontal edge: no crossing
    if (!(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1)) || y0 == y1) return;
    const int dir = y1 > y0 ? 1 : -1;
    const double ymin = y0 < y1 ? y0 : y1, ymax = y0 < y1 ? y1 : y0;
    // candidate rows: one spare on both sides, the exact test below decides
    double rlo = floor((ymin - oy) / ps - 0.5) - 1.0, rhi = ceil((ymax - oy) / ps - 0.5) + 1.0;
    if (rlo < 0.0) rlo = 0.0;
    if (rhi > (double)(pn - 1)) rhi = (double)(pn - 1);
    if (!(rlo <= rhi)) return;
    const double slope_num = x1 - x0, slope_den = y1 - y0;
    for (int r = (int)rlo; r <= (int)rhi; ++r) {
        const double yc = oy + ((double)r + 0.5) * ps;
        if (!(ymin <= yc && yc < ymax)) continue;
        const double xc = x0 + ((yc - y0) * slope_num) / slope_den;
        double t = ceil((xc - ox) / ps - 0.5);                 // columns c with ox + (c + 0.5) ps < xc
        if (t < 0.0) t = 0.0;
        if (t > (double)pn) t = (double)pn;
        const int k = (int)t;
        if (k == 0) continue;                                  // nothing lies left of the crossing
        int* row = delta + (size_t)r * (pn + 1);
        atomicAdd(row, dir);
        atomicAdd(row + k, -dir);
    }
}

// (a kernel, not hipMemsetAsync: memset nodes of a captured HIP graph are not replayed correctly on this stack, see abbe_engine.hip)
__global__ __launch_bounds__(256) void k_raster_clear(int* __restrict__ delta, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) delta[i] = 0;
}

__global__ __launch_bounds__(256) void k_raster_fill(const int* __restrict__ delta, int pn, int16_t* __restrict__ geo)
{
    __shared__ int part[256];
    const int r = blockIdx.x, t = threadIdx.x;
    const int per = (pn + 255) / 256;                          // consecutive columns per thread
    const int c0 = t * per, c1 = min(pn, c0 + per);
    const int* row = delta + (size_t)r * (pn + 1);
    int s = 0;
    for (int c = c0; c < c1; ++c) s += row[c];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {                  // inclusive scan of the 256 partial sums
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int w = t ? part[t - 1] : 0;
    for (int c = c0; c < c1; ++c) {
        w += row[c];
        geo[(size_t)r * pn + c] = w != 0 ? 1 : 0;
    }
}

// ---- Area coverage (litho_rasterize_coverage): the same inside rule on the s x s sub-centres of every pixel, sub-grid pitch
// q = pixel / s; coverage = (inside sub-centres) / s^2.  The sub-grid delta array [pn s][pn s + 1] is 1 GiB at 2048^2, s = 8,
// so it is evaluated in BANDS of whole pixel rows, as many as the caller's workspace holds: clear -> edges clipped to the
// band's sub-rows -> fill and reduce.  Every sub-row is computed from its own deltas alone: the band height cannot show.
constexpr int COV_CHUNK = 128;                                 // sub-rows one k_cov_edges thread walks at most

// k_raster_edges' arithmetic at pitch q (W = pn s sub-columns), one thread per (edge, chunk of COV_CHUNK sub-rows of the band
// [sub_lo, sub_hi)): at s = 16 a tall edge crosses 32768 sub-rows, which is not one thread's work.  delta holds the band only.
__global__ __launch_bounds__(256) void k_cov_edges(const double* __restrict__ edges, int ne, int W, double ox, double oy, double q,
                                                   int sub_lo, int sub_hi, int* __restrict__ delta)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const int c_lo = sub_lo + (int)blockIdx.y * COV_CHUNK;
    const int c_hi = min(sub_hi, c_lo + COV_CHUNK) - 1;       // inclusive; grid.y covers the band, so c_lo <= c_hi
    const double x0 = edges[4 * e], y0 = edges[4 * e + 1], x1 = edges[4 * e + 2], y1 = edges[4 * e + 3];
    if (!(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1)) || y0 == y1) return;
    const int dir = y1 > y0 ? 1 : -1;
    const double ymin = y0 < y1 ? y0 : y1, ymax = y0 < y1 ? y1 : y0;
    // candidate sub-rows: one spare on both sides, clipped to this thread's chunk; the exact test below decides
    double rlo = floor((ymin - oy) / q - 0.5) - 1.0, rhi = ceil((ymax - oy) / q - 0.5) + 1.0;
    if (rlo < (double)c_lo) rlo = (double)c_lo;
    if (rhi > (double)c_hi) rhi = (double)c_hi;
    if (!(rlo <= rhi)) return;
    const double slope_num = x1 - x0, slope_den = y1 - y0;
    for (int r = (int)rlo; r <= (int)rhi; ++r) {
        const double yc = oy + ((double)r + 0.5) * q;
        if (!(ymin <= yc && yc < ymax)) continue;
        const double xc = x0 + ((yc - y0) * slope_num) / slope_den;
        double t = ceil((xc - ox) / q - 0.5);                  // sub-columns C with ox + (C + 0.5) q < xc
        if (t < 0.0) t = 0.0;
        if (t > (double)W) t = (double)W;
        const int k = (int)t;
        if (k == 0) continue;
        int* row = delta + (size_t)(r - sub_lo) * ((size_t)W + 1);
        atomicAdd(row, dir);
        atomicAdd(row + k, -dir);
    }
}

// One WAVE per pixel row of the band (four rows per workgroup, no workgroup barrier anywhere), one lane per pixel, 64 pixels
// a step.  Per sub-row of the step: 64 S deltas arrive in S coalesced loads, go through the wave's LDS tile (one pad word per
// 32: both the lane-contiguous store and the S-strided read are conflict-free) so that every lane holds the S deltas of ITS
// pixel; a shuffle scan of the lanes' totals plus the winding carried along the sub-row (kept in lane r of `carry` for
// sub-row r) gives the winding of every sub-centre, and the lane counts the non-zero ones.  No atomics: a pixel's count is
// one lane's register.  The loads of RG sub-rows (<= 64 registers) are issued before the first is consumed.
template <int S>
__global__ __launch_bounds__(256) void k_cov_fill(const int* __restrict__ delta, int pn, int band_rows, float* __restrict__ cov)
{
    constexpr int RG = S * S <= 64 ? S : 64 / S;
    __shared__ int tile[4][66 * S];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int prow = (int)blockIdx.x * 4 + wave;
    if (prow >= band_rows) return;                             // wave-uniform
    const int W = pn * S;
    const size_t stride = (size_t)W + 1;
    const int* base = delta + (size_t)prow * S * stride;
    int* t = tile[wave];
    int carry = 0;
    for (int p0 = 0; p0 < pn; p0 += 64) {
        const int col0 = p0 * S;
        int cnt = 0;
#pragma unroll 1
        for (int g = 0; g < S; g += RG) {
            int v[RG][S];
            const int* rp = base + (size_t)g * stride + col0 + lane;
            if (col0 + 64 * S <= W) {                          // wave-uniform: every step but a ragged last one
#pragma unroll
                for (int rr = 0; rr < RG; ++rr)
#pragma unroll
                    for (int j = 0; j < S; ++j) v[rr][j] = rp[(size_t)rr * stride + j * 64];
            } else {                                           // past the row's W sub-columns: pixels >= pn, never written
#pragma unroll
                for (int rr = 0; rr < RG; ++rr)
#pragma unroll
                    for (int j = 0; j < S; ++j) v[rr][j] = col0 + j * 64 + lane < W ? rp[(size_t)rr * stride + j * 64] : 0;
            }
#pragma unroll
            for (int rr = 0; rr < RG; ++rr) {
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    const int i = j * 64 + lane;
                    t[i + (i >> 5)] = v[rr][j];
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // the wave's LDS accesses execute in order
                __builtin_amdgcn_wave_barrier();
                int x[S], tot = 0;
#pragma unroll
                for (int c = 0; c < S; ++c) {
                    const int i = lane * S + c;
                    x[c] = t[i + (i >> 5)];
                    tot += x[c];
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                int incl = tot;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int u = __shfl_up(incl, off);
                    if (lane >= off) incl += u;
                }
                int w = __shfl(carry, g + rr) + incl - tot;    // winding left of this lane's first sub-centre
#pragma unroll
                for (int c = 0; c < S; ++c) {
                    w += x[c];
                    cnt += w != 0 ? 1 : 0;
                }
                const int rowtot = __shfl(incl, 63);
                if (lane == g + rr) carry += rowtot;
            }
        }
        if (p0 + lane < pn) cov[(size_t)prow * pn + p0 + lane] = (float)cnt * (1.0f / (float)(S * S));
    }
}

template <int S>
static void launch_cov_fill(hipStream_t st, const int* delta, int pn, int rows, float* cov)
{
    hipLaunchKernelGGL(k_cov_fill<S>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, delta, pn, rows, cov);
}

static bool cov_supersampling(int s) { return s == 1 || s == 2 || s == 4 || s == 8 || s == 16; }

}  // namespace litho

extern "C" {

size_t litho_rasterize_work_bytes(int pn)
{
    if (pn < 1) return 0;
    return (size_t)pn * (size_t)(pn + 1) * sizeof(int);
}

int litho_rasterize_edges(const double* edges, int64_t n_edges, int pn, double x0, double y0, double pixel, void* work,
                          size_t work_bytes, int16_t* geometry, void* stream)
{
    using namespace litho;
    if (pn < 1 || pn > 32768 || n_edges < 0 || n_edges > 0x7FFFFFFF || !(pixel > 0.0) || !(x0 == x0) || !(y0 == y0) || !geometry ||
        !work || (n_edges > 0 && !edges))
        return LITHO_E_ARG;
    if (work_bytes < litho_rasterize_work_bytes(pn)) return LITHO_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t nwork = (size_t)pn * (size_t)(pn + 1);
    hipLaunchKernelGGL(k_raster_clear, dim3((unsigned)((nwork + 255) / 256 < 4096 ? (nwork + 255) / 256 : 4096)), dim3(256), 0, st, (int*)work, nwork);
    HIP_TRY(hipGetLastError());
    if (n_edges > 0) {
        hipLaunchKernelGGL(k_raster_edges, dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, st, edges, (int)n_edges, pn, x0, y0,
                           pixel, (int*)work);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_raster_fill, dim3(pn), dim3(256), 0, st, (const int*)work, pn, geometry);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

size_t litho_rasterize_coverage_work_bytes(int pn, int s, int band_rows)
{
    if (!litho::cov_supersampling(s) || pn < 1 || (int64_t)pn * s > 32768 || band_rows < 1) return 0;
    return (size_t)band_rows * (size_t)s * ((size_t)pn * s + 1) * sizeof(int);
}

int litho_rasterize_coverage(const double* edges, int64_t n_edges, int pn, double x0, double y0, double pixel, int s, void* work,
                             size_t work_bytes, float* coverage, void* stream)
{
    using namespace litho;
    if (!cov_supersampling(s) || pn < 1 || (int64_t)pn * s > 32768 || n_edges < 0 || n_edges > 0x7FFFFFFF || !(pixel > 0.0) ||
        !(x0 == x0) || !(y0 == y0) || !coverage || !work || (n_edges > 0 && !edges))
        return LITHO_E_ARG;
    const int W = pn * s;
    const size_t fit = work_bytes / litho_rasterize_coverage_work_bytes(pn, s, 1);
    if (fit < 1) return LITHO_E_WORKSPACE;
    const int band = fit < (size_t)pn ? (int)fit : pn;         // pixel rows per band
    const double q = pixel / (double)s;
    hipStream_t st = (hipStream_t)stream;
    for (int r0 = 0; r0 < pn; r0 += band) {
        const int rows = pn - r0 < band ? pn - r0 : band, nsub = rows * s;
        const size_t nwork = (size_t)nsub * ((size_t)W + 1);
        hipLaunchKernelGGL(k_raster_clear, dim3((unsigned)((nwork + 255) / 256 < 4096 ? (nwork + 255) / 256 : 4096)), dim3(256), 0, st, (int*)work, nwork);
        HIP_TRY(hipGetLastError());
        if (n_edges > 0) {
            hipLaunchKernelGGL(k_cov_edges, dim3((unsigned)((n_edges + 255) / 256), (unsigned)((nsub + COV_CHUNK - 1) / COV_CHUNK)), dim3(256), 0,
                               st, edges, (int)n_edges, W, x0, y0, q, r0 * s, r0 * s + nsub, (int*)work);
            HIP_TRY(hipGetLastError());
        }
        float* out = coverage + (size_t)r0 * pn;
        switch (s) {
        case 1: launch_cov_fill<1>(st, (const int*)work, pn, rows, out); break;
        case 2: launch_cov_fill<2>(st, (const int*)work, pn, rows, out); break;
        case 4: launch_cov_fill<4>(st, (const int*)work, pn, rows, out); break;
        case 8: launch_cov_fill<8>(st, (const int*)work, pn, rows, out); break;
        default: launch_cov_fill<16>(st, (const int*)work, pn, rows, out); break;
        }
        HIP_TRY(hipGetLastError());
    }
    return LITHO_OK;
}

}  // extern "C"
