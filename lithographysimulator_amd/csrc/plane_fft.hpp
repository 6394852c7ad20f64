// plane_fft.hpp -- what the plane transforms of socs.hip and socs_grad.hip share: the twiddle table, the line geometry, the
// in-place tiled transpose and the dispatch on the line size.  The row kernels themselves stay with their units.
//
// The library is built without relocatable device code, so a translation unit cannot name another's __device__ symbols: the
// table and the two kernels here have internal linkage, and each unit that includes this header keeps its own copy of them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "fft_core.hpp"

namespace litho {

static constexpr int FFT_MAX_N = 4096;
// exp(+2 pi i k / 4096), k = 0 .. 4095: the twiddle table of every size (a transform of n points reads it with stride 4096 / n).
// One copy per unit and device, rewritten with the same bits by every call on its own stream (as the engine refills its table
// per call).
static __device__ float2 g_twiddles[FFT_MAX_N];

static __global__ __launch_bounds__(256) void k_fill_twiddles()
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= FFT_MAX_N) return;
    double s, c;
    sincospi(2.0 * (double)k / (double)FFT_MAX_N, &s, &c);
    g_twiddles[k] = make_float2((float)c, (float)s);
}

static hipError_t fill_twiddles(hipStream_t st)
{
    hipLaunchKernelGGL(k_fill_twiddles, dim3(FFT_MAX_N / 256), dim3(256), 0, st);
    return hipGetLastError();
}

// How a row kernel lays lines of 2^LOG2N samples onto a workgroup.
template <int LOG2N>
struct LineShape {
    using F = LineFFT<LOG2N, +1>;
    static constexpr int L = (F::T >= 64) ? 1 : 64 / F::T;      // lines per workgroup: at least one full wave
    static constexpr int THREADS = F::T * L;
    static constexpr size_t LDS_EXCH = (size_t)L * F::LDS_LINE;
    static constexpr size_t LDS_BYTES = sizeof(float2) * (LDS_EXCH + F::LDS_TW);
    static dim3 grid(long long lines) { return dim3((unsigned)((lines + L - 1) / L)); }
};

// In-place transpose of `batch` n x n complex matrices (grid.z): the workgroup of tile (bi, bj), bi <= bj, swaps it with
// tile (bj, bi) through LDS.  32 x 32 tiles, rows padded by one sample; 256 threads move 8 tile rows per step.
static constexpr int TR_TILE = 32;
static __global__ __launch_bounds__(256) void k_transpose_inplace(float2* __restrict__ data, int n)
{
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    __shared__ float2 a[TR_TILE][TR_TILE + 1], b[TR_TILE][TR_TILE + 1];
    float2* m = data + (size_t)blockIdx.z * n * n;
    const int tx = threadIdx.x % TR_TILE, ty = threadIdx.x / TR_TILE;
    for (int r = ty; r < TR_TILE; r += 256 / TR_TILE) {
        const int ra = bi * TR_TILE + r, ca = bj * TR_TILE + tx;        // tile (bi, bj)
        const int rb = bj * TR_TILE + r, cb = bi * TR_TILE + tx;        // tile (bj, bi)
        if (ra < n && ca < n) a[r][tx] = m[(size_t)ra * n + ca];
        if (rb < n && cb < n) b[r][tx] = m[(size_t)rb * n + cb];
    }
    __syncthreads();
    for (int r = ty; r < TR_TILE; r += 256 / TR_TILE) {
        const int ra = bi * TR_TILE + r, ca = bj * TR_TILE + tx;
        const int rb = bj * TR_TILE + r, cb = bi * TR_TILE + tx;
        if (ra < n && ca < n) m[(size_t)ra * n + ca] = b[tx][r];        // (ra, ca) <- (ca, ra), which lies in tile (bj, bi)
        if (bi != bj && rb < n && cb < n) m[(size_t)rb * n + cb] = a[tx][r];
    }
}

static hipError_t transpose(float2* data, int batch, int n, hipStream_t st)
{
    const unsigned tiles = (unsigned)((n + TR_TILE - 1) / TR_TILE);
    for (int b0 = 0; b0 < batch; b0 += 65535) {                    // grid.z holds at most 65535 matrices
        const int nb = batch - b0 < 65535 ? batch - b0 : 65535;
        hipLaunchKernelGGL(k_transpose_inplace, dim3(tiles, tiles, (unsigned)nb), dim3(256), 0, st, data + (size_t)b0 * n * n, n);
    }
    return hipGetLastError();
}

inline int log2_exact(int n)
{
    int l = 0;
    while ((1 << l) < n) ++l;
    return (1 << l) == n ? l : -1;
}

inline bool fft_size_ok(int n) { return n >= 16 && n <= FFT_MAX_N && log2_exact(n) > 0; }

// f(std::integral_constant<int, l2>{}) for the line sizes the row kernels are built for, 2^4 ... 2^12.
template <class F>
hipError_t for_log2(int l2, F&& f)
{
    switch (l2) {
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 9: return f(std::integral_constant<int, 9>{});
    case 10: return f(std::integral_constant<int, 10>{});
    case 11: return f(std::integral_constant<int, 11>{});
    case 12: return f(std::integral_constant<int, 12>{});
    default: return hipErrorInvalidValue;
    }
}

// Y is X, or `bytes` from each do not overlap: what an entry that copies X to Y and then works in place on Y can take.
inline bool same_or_disjoint(const void* X, const void* Y, size_t bytes)
{
    const uintptr_t x0 = (uintptr_t)X, y0 = (uintptr_t)Y;
    return x0 == y0 || x0 >= y0 + bytes || y0 >= x0 + bytes;
}

// two complex samples in one 16-byte access (complex64 arrays promise 8-byte alignment only)
typedef float float4c __attribute__((ext_vector_type(4), aligned(8)));

}  // namespace litho
