// tiling.hip -- the kernels of tiled imaging (include/litho_abbe.h, "Tiled imaging of large layouts"): the cores
// of a batch of window images copied into one stitched image, and the seam measure -- how much two neighbouring windows disagree
// on the two pixel lines either side of the boundary between their cores; and, for the tiled inverse-lithography loop, a global
// transmission cut into windows with halos, the cut's adjoint (the window gradients summed back, overlap-add) and the stitch's
// adjoint.  All are bandwidth work on contiguous lines; the window images themselves come from litho_socs_image_batch and the
// window gradients from litho_socs_vjp_batch (socs_grad.hip).
// No reference counterpart; checked bit for bit against numpy slicing (tests/tiling_oracle.py, tests/tiled_ilt_oracle.py).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/litho_abbe.h"
#include "engine_common.hpp"

namespace litho {

static constexpr int STITCH_WAVES = 4;                         // core rows per workgroup, one wave each

// Row R of the flat list [count][planes][core]: core row i of plane p of tile t goes to image row place[t].row + i, columns
// place[t].col + j for the lanes' j = lane, lane + 64, ...  Rows and columns outside [0, n) are skipped; the index arithmetic is
// 64-bit, so any int32 placement is safe.
__global__ __launch_bounds__(64 * STITCH_WAVES) void k_tiles_stitch(const float* __restrict__ tiles, long long rows, int planes, int nt,
                                                                    const int32_t* __restrict__ place, int j0, int core,
                                                                    float* __restrict__ image, int n)
{
    const long long R = (long long)blockIdx.x * STITCH_WAVES + (threadIdx.x >> 6);
    if (R >= rows) return;
    const int lane = threadIdx.x & 63;
    const int i = (int)(R % core);
    const long long tp = R / core;                             // t planes + p
    const int p = (int)(tp % planes);
    const long long t = tp / planes;
    const long long gr = (long long)place[2 * t] + i, gc0 = (long long)place[2 * t + 1];
    if (gr < 0 || gr >= n) return;
    const float* src = tiles + ((size_t)tp * nt + (size_t)(j0 + i)) * nt + j0;
    float* dst = image + ((size_t)p * n + (size_t)gr) * n;
    for (int j = lane; j < core; j += 64) {
        const long long gc = gc0 + j;
        if (gc >= 0 && gc < n) dst[gc] = src[j];
    }
}

// One wave per (tile, plane, side): side 0 the right neighbour (the line runs down the core's rows, the two samples of a row are
// adjacent), side 1 the lower neighbour (the line runs along the core's columns: contiguous).  Each lane takes the maximum over
// the line positions lane, lane + 64, ..., then the xor butterfly; fmaxf is commutative and associative on the non-NaN values, so
// every lane ends with the same bits.
__global__ __launch_bounds__(64) void k_tiles_seam(const float* __restrict__ tiles, int count, int planes, int nt,
                                                   const int32_t* __restrict__ neighbours, int j0, int core, float* __restrict__ out)
{
    const long long w = blockIdx.x;                            // (t planes + p) 2 + side
    const int side = (int)(w & 1);
    const long long tp = w >> 1;
    const int p = (int)(tp % planes);
    const long long t = tp / planes;
    const int nb = neighbours[2 * t + side];
    if (nb < 0 || nb >= count) {
        if (threadIdx.x == 0) out[w] = __int_as_float(0x7fc00000);
        return;
    }
    const size_t plane = (size_t)nt * nt;
    const float* a = tiles + (size_t)tp * plane;
    const float* b = tiles + ((size_t)nb * planes + p) * plane;
    // a's sample (ra, ca) and b's (rb, cb) show the same place; d = 0, 1 steps across the boundary, k along it
    const int far = j0 + core - 1, near = j0 - 1;
    float m = 0.f;
    for (int k = threadIdx.x; k < core; k += 64) {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const size_t ia = side == 0 ? (size_t)(j0 + k) * nt + (far + d) : (size_t)(far + d) * nt + (j0 + k);
            const size_t ib = side == 0 ? (size_t)(j0 + k) * nt + (near + d) : (size_t)(near + d) * nt + (j0 + k);
            m = fmaxf(m, fabsf(a[ia] - b[ib]));
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o /= 2) m = fmaxf(m, __shfl_xor(m, o));
    if (threadIdx.x == 0) out[w] = m;
}

// ---- The tiled inverse-lithography loop's three: a global plane cut into windows, its adjoint, and the stitch's adjoint. ----

// Row R of the flat list [count][pn]: window row r of tile t is plane row place[t].row - halo + r from column place[t].col - halo
// on, `fill` where that leaves the plane.  One wave per row, lanes stride the columns; 64-bit index arithmetic.
__global__ __launch_bounds__(64 * STITCH_WAVES) void k_tiles_cut(const float2* __restrict__ plane, int rows, int cols,
                                                                 const int32_t* __restrict__ place, long long lines, int pn, int halo,
                                                                 float2 fill, float2* __restrict__ windows)
{
    const long long R = (long long)blockIdx.x * STITCH_WAVES + (threadIdx.x >> 6);
    if (R >= lines) return;
    const int lane = threadIdx.x & 63;
    const long long t = R / pn;
    const long long gr = (long long)place[2 * t] - halo + (R - t * pn), gc0 = (long long)place[2 * t + 1] - halo;
    const bool row_in = gr >= 0 && gr < rows;
    const float2* src = plane + (size_t)(row_in ? gr : 0) * cols;
    float2* dst = windows + (size_t)R * pn;
    for (int c = lane; c < pn; c += 64) {
        const long long gc = gc0 + c;
        dst[c] = (row_in && gc >= 0 && gc < cols) ? src[gc] : fill;
    }
}

// The cut's adjoint as a gather: the thread of plane pixel (gr, gc) adds windows[t][gr - row_t + halo][gc - col_t + halo] of every
// tile t whose window holds the pixel, t ascending, into one running fp32 sum per component that starts from zero.  The order is
// the tile list's and nothing else: no atomics, and the launch geometry does not enter.  Every thread reads the same place entry
// at a time (one cached broadcast); the window reads of a wave are contiguous.
__global__ __launch_bounds__(256) void k_tiles_overlap_add(const float2* __restrict__ windows, int count, int pn, int halo,
                                                           const int32_t* __restrict__ place, float2* __restrict__ plane, int rows,
                                                           int cols)
{
    const long long cell = (long long)blockIdx.x * 256 + threadIdx.x;
    if (cell >= (long long)rows * cols) return;
    const long long gr = cell / cols, gc = cell - gr * cols;
    float2 acc = make_float2(0.f, 0.f);
    for (int t = 0; t < count; ++t) {
        const long long r = gr - place[2 * t] + halo, c = gc - place[2 * t + 1] + halo;
        if (r < 0 || r >= pn || c < 0 || c >= pn) continue;
        const float2 w = windows[((size_t)t * pn + (size_t)r) * pn + (size_t)c];
        acc.x += w.x;
        acc.y += w.y;
    }
    plane[cell] = acc;
}

// The stitch's adjoint.  Row R of the flat list [count][planes][nt]: row r of plane p of tile t is image row place[t].row + r - j0
// from column place[t].col - j0 on inside the core [j0, j0 + core)^2 and where the image has such a pixel, zero everywhere else
// (what the stitch skips has no gradient).  Every element of tiles is written.
__global__ __launch_bounds__(64 * STITCH_WAVES) void k_tiles_unstitch(const float* __restrict__ image, int n,
                                                                      const int32_t* __restrict__ place, long long lines, int planes,
                                                                      int nt, int j0, int core, float* __restrict__ tiles)
{
    const long long R = (long long)blockIdx.x * STITCH_WAVES + (threadIdx.x >> 6);
    if (R >= lines) return;
    const int lane = threadIdx.x & 63;
    const int r = (int)(R % nt);
    const long long tp = R / nt;
    const int p = (int)(tp % planes);
    const long long t = tp / planes;
    const long long gr = (long long)place[2 * t] + r - j0, gc0 = (long long)place[2 * t + 1] - j0;
    const bool row_in = r >= j0 && r < j0 + core && gr >= 0 && gr < n;
    const float* src = image + ((size_t)p * n + (size_t)(row_in ? gr : 0)) * n;
    float* dst = tiles + (size_t)R * nt;
    for (int c = lane; c < nt; c += 64) {
        const long long gc = gc0 + c;
        dst[c] = (row_in && c >= j0 && c < j0 + core && gc >= 0 && gc < n) ? src[gc] : 0.f;
    }
}

}  // namespace litho

extern "C" {

int litho_tiles_stitch(const float* tiles, int count, int planes, int nt, const int32_t* place, int j0, int core, float* image, int n,
                       void* stream)
{
    using namespace litho;
    if (!tiles || !place || !image || count < 1 || planes < 1 || nt < 1 || core < 1 || n < 1 || j0 < 0 || j0 > nt - core)
        return LITHO_E_ARG;
    const long long rows = (long long)count * planes;          // count, planes <= INT_MAX: below 2^62
    if (rows > INT_MAX || rows * core > INT_MAX) return LITHO_E_ARG;
    const long long lines = rows * core;
    const unsigned blocks = (unsigned)((lines + STITCH_WAVES - 1) / STITCH_WAVES);
    hipLaunchKernelGGL(k_tiles_stitch, dim3(blocks), dim3(64 * STITCH_WAVES), 0, (hipStream_t)stream, tiles, lines, planes, nt, place,
                       j0, core, image, n);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_tiles_seam(const float* tiles, int count, int planes, int nt, const int32_t* neighbours, int j0, int core, float* out,
                     void* stream)
{
    using namespace litho;
    if (!tiles || !neighbours || !out || count < 1 || planes < 1 || nt < 1 || core < 1 || j0 < 1 || j0 >= nt - core) return LITHO_E_ARG;
    const long long waves = (long long)count * planes;
    if (waves > INT_MAX / 2) return LITHO_E_ARG;
    hipLaunchKernelGGL(k_tiles_seam, dim3((unsigned)(2 * waves)), dim3(64), 0, (hipStream_t)stream, tiles, count, planes, nt, neighbours,
                       j0, core, out);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_tiles_cut(const void* plane, int rows, int cols, const int32_t* place, int count, int pn, int halo, float fill_re,
                    float fill_im, void* windows, void* stream)
{
    using namespace litho;
    if (!plane || !place || !windows || count < 1 || rows < 1 || cols < 1 || pn < 1 || halo < 0 || 2LL * halo >= pn) return LITHO_E_ARG;
    if (pn - 2 * halo > rows || pn - 2 * halo > cols) return LITHO_E_ARG;       // a core larger than the plane
    const long long lines = (long long)count * pn;
    if (lines > INT_MAX) return LITHO_E_ARG;
    const unsigned blocks = (unsigned)((lines + STITCH_WAVES - 1) / STITCH_WAVES);
    hipLaunchKernelGGL(k_tiles_cut, dim3(blocks), dim3(64 * STITCH_WAVES), 0, (hipStream_t)stream, (const float2*)plane, rows, cols,
                       place, lines, pn, halo, make_float2(fill_re, fill_im), (float2*)windows);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_tiles_overlap_add(const void* windows, int count, int pn, int halo, const int32_t* place, void* plane, int rows, int cols,
                            void* stream)
{
    using namespace litho;
    if (!windows || !place || !plane || count < 1 || rows < 1 || cols < 1 || pn < 1 || halo < 0 || 2LL * halo >= pn) return LITHO_E_ARG;
    if (pn - 2 * halo > rows || pn - 2 * halo > cols) return LITHO_E_ARG;
    const long long cells = (long long)rows * cols;
    if ((long long)count * pn > INT_MAX || (cells + 255) / 256 > INT_MAX) return LITHO_E_ARG;
    hipLaunchKernelGGL(k_tiles_overlap_add, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float2*)windows, count, pn, halo, place, (float2*)plane, rows, cols);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_tiles_unstitch(const float* image, int n, const int32_t* place, int count, int planes, int nt, int j0, int core, float* tiles,
                         void* stream)
{
    using namespace litho;
    if (!image || !place || !tiles || count < 1 || planes < 1 || nt < 1 || core < 1 || n < 1 || j0 < 0 || j0 > nt - core || core > n)
        return LITHO_E_ARG;
    const long long rows = (long long)count * planes;
    if (rows > INT_MAX || rows * nt > INT_MAX) return LITHO_E_ARG;
    const long long lines = rows * nt;
    const unsigned blocks = (unsigned)((lines + STITCH_WAVES - 1) / STITCH_WAVES);
    hipLaunchKernelGGL(k_tiles_unstitch, dim3(blocks), dim3(64 * STITCH_WAVES), 0, (hipStream_t)stream, image, n, place, lines, planes, nt,
                       j0, core, tiles);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

}  // extern "C"
