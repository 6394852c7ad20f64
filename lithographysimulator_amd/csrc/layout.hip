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
// litho_rasterize_coverage_tiles does that for all windows of a tiled layout in one launch, the deltas of one sub-row in LDS: k_cov_tiles.
#include "engine_common.hpp"
#include "../../include/litho_abbe.h"

#include <cmath>
#include <cstdint>
#include <type_traits>

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

// ---- The crossing arithmetic of the coverage rasterisers, ONE text for k_cov_edges and k_cov_tiles: k_raster_edges' at pitch q
// (W = pn s sub-columns).  cov_edge_load: the edge and its candidate sub-rows [rlo, rhi] -- one spare on both sides, clipped to
// [c_lo, c_hi]; the exact test in cov_edge_cross decides.  false: the edge cannot add to those sub-rows (a non-finite coordinate
// -- NaN or +-inf: inf * 0 and inf - inf would be NaN and the cast to int undefined --, a horizontal edge, an empty clip).
struct CovEdge {
    double x0, y0, slope_num, slope_den, ymin, ymax, rlo, rhi;
    int dir;
};

__device__ __forceinline__ bool cov_edge_load(const double* __restrict__ edge, double oy, double q, int c_lo, int c_hi, CovEdge& E)
{
    const double x0 = edge[0], y0 = edge[1], x1 = edge[2], y1 = edge[3];
    if (!(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1)) || y0 == y1) return false;
    E.dir = y1 > y0 ? 1 : -1;
    E.ymin = y0 < y1 ? y0 : y1;
    E.ymax = y0 < y1 ? y1 : y0;
    double rlo = floor((E.ymin - oy) / q - 0.5) - 1.0, rhi = ceil((E.ymax - oy) / q - 0.5) + 1.0;
    if (rlo < (double)c_lo) rlo = (double)c_lo;
    if (rhi > (double)c_hi) rhi = (double)c_hi;
    if (!(rlo <= rhi)) return false;
    E.rlo = rlo;
    E.rhi = rhi;
    E.x0 = x0;
    E.y0 = y0;
    E.slope_num = x1 - x0;
    E.slope_den = y1 - y0;
    return true;
}

// k = the number of sub-columns C of sub-row r with ox + (C + 0.5) q left of the edge's crossing, clamped to [0, W]; 0 as well
// where the sub-row's ordinate misses [ymin, ymax).  The caller adds dir at column 0 and -dir at column k when k > 0.
__device__ __forceinline__ int cov_edge_cross(const CovEdge& E, int r, double ox, double oy, double q, int W)
{
    const double yc = oy + ((double)r + 0.5) * q;
    if (!(E.ymin <= yc && yc < E.ymax)) return 0;
    const double xc = E.x0 + ((yc - E.y0) * E.slope_num) / E.slope_den;
    double t = ceil((xc - ox) / q - 0.5);                      // sub-columns C with ox + (C + 0.5) q < xc
    if (t < 0.0) t = 0.0;
    if (t > (double)W) t = (double)W;
    return (int)t;
}

// One thread per (edge, chunk of COV_CHUNK sub-rows of the band [sub_lo, sub_hi)): at s = 16 a tall edge crosses 32768 sub-rows,
// which is not one thread's work.  delta holds the band only.
__global__ __launch_bounds__(256) void k_cov_edges(const double* __restrict__ edges, int ne, int W, double ox, double oy, double q,
                                                   int sub_lo, int sub_hi, int* __restrict__ delta)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const int c_lo = sub_lo + (int)blockIdx.y * COV_CHUNK;
    const int c_hi = min(sub_hi, c_lo + COV_CHUNK) - 1;       // inclusive; grid.y covers the band, so c_lo <= c_hi
    CovEdge E;
    if (!cov_edge_load(edges + 4 * (size_t)e, oy, q, c_lo, c_hi, E)) return;
    for (int r = (int)E.rlo; r <= (int)E.rhi; ++r) {
        const int k = cov_edge_cross(E, r, ox, oy, q, W);
        if (k == 0) continue;
        int* row = delta + (size_t)(r - sub_lo) * ((size_t)W + 1);
        atomicAdd(row, E.dir);
        atomicAdd(row + k, -E.dir);
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

// ---- All windows of a chunk in one launch (litho_rasterize_coverage_tiles): one workgroup per (tile, pixel row), the winding
// deltas of ONE sub-row in LDS -- no global delta array, no clear pass, no global atomics.  Dynamic LDS, in this order:
//   line  int32 [W + W / 32 + 1]   deltas of the current sub-row, one pad word per 32 (k_cov_fill's layout: the S-strided reads
//                                  of the scan are conflict-free); the sink at sub-column W is never stored
//   list  int32 [COV_LIST]         the numbers of the tile's edges whose candidate sub-rows meet this pixel row, compacted once
//   misc  int32 [16]               [0] the list's length, [8 + 4 (parity) + wave] the waves' totals of a scan step
//   cnt   CovCount<S> [pn]         inside sub-centres per pixel over the sub-rows done so far (S > 1; S = 1 writes at once)
// Per sub-row: the threads walk the list (or, when it overflowed, the tile's whole index range) and add +-1 with LDS integer
// atomics -- the order cannot show; barrier; steps of 256 pixels, one pixel per thread: the thread reads the S deltas of its
// pixel and stores zeros in their place (the line is clear again for the next sub-row), a shuffle scan per wave and the waves'
// totals through `misc` (one barrier per step, two parities) give the winding left of the pixel.  A pixel belongs to the same
// thread in every sub-row, so `cnt` needs no barrier of its own.
constexpr int COV_LIST = 1024;
constexpr int COV_TILES_LDS_MAX = 160 * 1024;
template <int S>
using CovCount = typename std::conditional<(S * S < 256), uint8_t, uint16_t>::type;

__host__ __device__ constexpr int cov_line_words(int W) { return W + (W >> 5) + 1; }

template <int S>
static size_t cov_tiles_lds(int pn)
{
    const size_t words = (size_t)cov_line_words(pn * S) + COV_LIST + 16;
    return words * sizeof(int) + (S > 1 ? (((size_t)pn * sizeof(CovCount<S>) + 3) & ~(size_t)3) : 0);
}

template <int S>
__global__ __launch_bounds__(256) void k_cov_tiles(const double* __restrict__ edges, long long n_edges,
                                                   const long long* __restrict__ tile_offsets, const int* __restrict__ tile_edges,
                                                   long long n_index, const double* __restrict__ windows, int tile0, int pn, double q,
                                                   float* __restrict__ coverage)
{
    extern __shared__ __attribute__((aligned(16))) int cov_lds[];
    const int W = pn * S;
    int* line = cov_lds;
    int* list = line + cov_line_words(W);
    int* misc = list + COV_LIST;
    CovCount<S>* cnt = (CovCount<S>*)(misc + 16);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tile = tile0 + (int)blockIdx.y, prow = (int)blockIdx.x;
    float* out = coverage + ((size_t)tile * pn + prow) * pn;
    const double ox = windows[2 * (size_t)tile], oy = windows[2 * (size_t)tile + 1];
    if (!(isfinite(ox) && isfinite(oy))) {                     // workgroup-uniform
        for (int p = t; p < pn; p += 256) out[p] = 0.0f;
        return;
    }
    long long lo = tile_offsets[tile], hi = tile_offsets[tile + 1];
    lo = lo < 0 ? 0 : (lo > n_index ? n_index : lo);
    hi = hi < lo ? lo : (hi > n_index ? n_index : hi);
    const long long span = hi - lo;
    const int sub0 = prow * S;
    for (int i = t; i < cov_line_words(W); i += 256) line[i] = 0;
    if (S > 1)
        for (int p = t; p < pn; p += 256) cnt[p] = 0;
    if (t == 0) misc[0] = 0;
    __syncthreads();
    // the edges that can meet this pixel row, once; more than COV_LIST of them: every sub-row walks the whole range instead
    for (long long i = t; i < span; i += 256) {
        const long long e = tile_edges[lo + i];
        CovEdge E;
        if (e < 0 || e >= n_edges || !cov_edge_load(edges + 4 * (size_t)e, oy, q, sub0, sub0 + S - 1, E)) continue;
        const int at = atomicAdd(&misc[0], 1);
        if (at < COV_LIST) list[at] = (int)e;
    }
    __syncthreads();
    const int found = misc[0];
    const bool listed = found <= COV_LIST;
    const long long walk = listed ? (long long)found : span;
    int parity = 0;
    for (int j = 0; j < S; ++j) {
        const int r = sub0 + j;
        int first = 0;                                         // this thread's share of column 0
        for (long long i = t; i < walk; i += 256) {
            const long long e = listed ? (long long)list[i] : (long long)tile_edges[lo + i];
            CovEdge E;
            if (e < 0 || e >= n_edges || !cov_edge_load(edges + 4 * (size_t)e, oy, q, r, r, E)) continue;
            const int k = cov_edge_cross(E, r, ox, oy, q, W);
            if (k == 0) continue;
            first += E.dir;
            if (k < W) atomicAdd(&line[k + (k >> 5)], -E.dir);
        }
        if (first != 0) atomicAdd(&line[0], first);
        __syncthreads();
        int carry = 0;                                         // winding left of the step's first sub-centre
        for (int p0 = 0; p0 < pn; p0 += 256) {
            const int p = p0 + t;
            int x[S], tot = 0;
#pragma unroll
            for (int c = 0; c < S; ++c) {
                const int i = p * S + c;
                x[c] = p < pn ? line[i + (i >> 5)] : 0;
                tot += x[c];
            }
            if (p < pn) {
#pragma unroll
                for (int c = 0; c < S; ++c) {
                    const int i = p * S + c;
                    line[i + (i >> 5)] = 0;
                }
            }
            int incl = tot;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int u = __shfl_up(incl, off);
                if (lane >= off) incl += u;
            }
            int* wt = misc + 8 + 4 * parity;
            if (lane == 63) wt[wave] = incl;
            __syncthreads();
            int w = carry + incl - tot;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int u = wt[v];
                if (v < wave) w += u;
                carry += u;
            }
            parity ^= 1;
            int inside = 0;
#pragma unroll
            for (int c = 0; c < S; ++c) {
                w += x[c];
                inside += w != 0 ? 1 : 0;
            }
            if (p < pn) {
                if (S == 1) out[p] = (float)inside;
                else if (j == S - 1) out[p] = (float)((int)cnt[p] + inside) * (1.0f / (float)(S * S));
                else cnt[p] = (CovCount<S>)((int)cnt[p] + inside);
            }
        }
    }
}

template <int S>
static hipError_t launch_cov_tiles(hipStream_t st, const double* edges, int64_t n_edges, const int64_t* offsets, const int32_t* index,
                                   int64_t n_index, const double* windows, int tiles, int pn, double q, float* cov)
{
    const size_t lds = cov_tiles_lds<S>(pn);
    if (lds > 64 * 1024) {                                     // once per device: the most a workgroup may declare
        static unsigned lds_done = 0;
        const hipError_t e = lds_opt_in(lds_done, (const void*)k_cov_tiles<S>, COV_TILES_LDS_MAX);
        if (e != hipSuccess) return e;
    }
    for (int t0 = 0; t0 < tiles; t0 += 65535) {                // grid.y
        const int n = tiles - t0 < 65535 ? tiles - t0 : 65535;
        hipLaunchKernelGGL(k_cov_tiles<S>, dim3((unsigned)pn, (unsigned)n), dim3(256), lds, st, edges, (long long)n_edges,
                           (const long long*)offsets, index, (long long)n_index, windows, t0, pn, q, cov);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

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

int litho_rasterize_coverage_tiles(const double* edges, int64_t n_edges, const int64_t* tile_offsets, const int32_t* tile_edges,
                                   int64_t n_index, const double* windows, int tiles, int pn, double pixel, int s, float* coverage,
                                   void* stream)
{
    using namespace litho;
    if (!cov_supersampling(s) || pn < 1 || (int64_t)pn * s > 32768 || tiles < 1 || n_edges < 0 || n_edges > 0x7FFFFFFF || n_index < 0 ||
        !(pixel > 0.0) || !(pixel <= 1.7976931348623157e308) || !coverage || !tile_offsets || !windows || (n_edges > 0 && !edges) ||
        (n_index > 0 && !tile_edges))
        return LITHO_E_ARG;
    const double q = pixel / (double)s;
    hipStream_t st = (hipStream_t)stream;
    switch (s) {
    case 1: HIP_TRY(launch_cov_tiles<1>(st, edges, n_edges, tile_offsets, tile_edges, n_index, windows, tiles, pn, q, coverage)); break;
    case 2: HIP_TRY(launch_cov_tiles<2>(st, edges, n_edges, tile_offsets, tile_edges, n_index, windows, tiles, pn, q, coverage)); break;
    case 4: HIP_TRY(launch_cov_tiles<4>(st, edges, n_edges, tile_offsets, tile_edges, n_index, windows, tiles, pn, q, coverage)); break;
    case 8: HIP_TRY(launch_cov_tiles<8>(st, edges, n_edges, tile_offsets, tile_edges, n_index, windows, tiles, pn, q, coverage)); break;
    default: HIP_TRY(launch_cov_tiles<16>(st, edges, n_edges, tile_offsets, tile_edges, n_index, windows, tiles, pn, q, coverage)); break;
    }
    return LITHO_OK;
}

}  // extern "C"
