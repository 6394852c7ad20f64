// resist_volume.hpp -- what the units of the resist chain share (peb.hip, develop.hip, develop_grad.hip): the limits of a volume
// [B, D, n, n], the 16-byte packs of the pointwise kernels and their launch, the host predicates of the entry points, the gains,
// Mack's rate law (host set-up, device forward and backward), the entry points' aliasing rule (Span, writes_clear), and the
// geometry and the host loop of the tiled fixed-point solvers.
//
// The library is built without relocatable device code, so a translation unit cannot name another's __device__ symbols:
// everything here is static or inline, and each unit that includes this header keeps its own copy.  The units are built with
// -ffp-contract=off (Makefile): the device functions below are fixed sequences of single operations, and their lines are the
// ones the float64 oracles of tests/ restate.
#pragma once
#include "engine_common.hpp"
#include "../../include/litho_abbe.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>

namespace litho {

static constexpr int VOL_DMAX = 32, VOL_GAINS = 64;                        // planes through the resist, gains per call
static constexpr int VOL_TILE = 16, VOL_HALO = VOL_TILE + 2;               // a workgroup's lateral tile, and with its one-cell halo
static constexpr int VOL_INNER = 8, VOL_CHECK = 4, VOL_MAXIT = 65536;      // solver rounds per launch, launches per host check, cap

struct VolGains {
    float g[VOL_GAINS];
};
struct VolSurface {
    double f[VOL_DMAX];                                  // the surface-inhibition factor of plane d, from the host
};

// ---- packs: VEC consecutive x of a row, one 16-byte access when VEC = 4
template <int VEC>
struct Pack {
    float v[VEC];
};
template <int VEC>
__device__ __forceinline__ Pack<VEC> load_pack(const float* p)
{
    Pack<VEC> r;
    if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int VEC>
__device__ __forceinline__ Pack<VEC> fill_pack(float x)
{
    Pack<VEC> r;
    for (int v = 0; v < VEC; ++v) r.v[v] = x;
    return r;
}
template <int VEC>
__device__ __forceinline__ void store_pack(float* p, const Pack<VEC>& r)
{
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else *p = r.v[0];
}

// index -1 - k <-> k and n + k <-> n - 1 - k, repeated as needed
__host__ __device__ __forceinline__ int mirror_index(int i, int n)
{
    int m = i % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

// ---- host predicates of the entry points
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + b_bytes && pb < pa + a_bytes;
}
// The aliasing rule of every entry point: what a call writes (outputs, workspace, sum outputs) overlaps nothing else the call
// touches; what it only reads may alias.  True when no span of `writes` overlaps another of them or one of `reads`; a null span is
// an optional buffer that was not given.
struct Span { const void* p; size_t bytes; };
static bool writes_clear(std::initializer_list<Span> writes, std::initializer_list<Span> reads)
{
    for (const Span* w = writes.begin(); w != writes.end(); ++w) {
        if (!w->p) continue;
        for (const Span* o = w + 1; o != writes.end(); ++o)
            if (o->p && overlap(w->p, w->bytes, o->p, o->bytes)) return false;
        for (const Span& r : reads)
            if (r.p && overlap(w->p, w->bytes, r.p, r.bytes)) return false;
    }
    return true;
}
static bool finite_pos(double v) { return v > 0.0 && !std::isinf(v); }
static bool finite_nonneg(double v) { return v >= 0.0 && !std::isinf(v); }
static unsigned plane_blocks(int n, int vec) { return (unsigned)(((long long)n * n / vec + 255) / 256); }
static bool volume_ok(int B, int D, int n) { return B >= 1 && D >= 1 && D <= VOL_DMAX && n >= 1 && n <= 16384 && (long long)B * D <= 65535; }
static size_t flag_bytes(int max_iterations) { return ((size_t)max_iterations * sizeof(int) + 255) & ~(size_t)255; }

// The packed kernel k<4> when `wide` (n a multiple of 4 and every pointer 16-byte aligned: the caller's test), else its scalar
// twin k<1>; grid.x covers the n^2 / VEC packs of a plane, grid.y the planes.
#define LAUNCH_PACKED(k, wide, n, planes, st, ...)                                                                       \
    do {                                                                                                                 \
        if (wide) hipLaunchKernelGGL(k<4>, dim3(plane_blocks(n, 4), (unsigned)(planes)), dim3(256), 0, st, __VA_ARGS__); \
        else hipLaunchKernelGGL(k<1>, dim3(plane_blocks(n, 1), (unsigned)(planes)), dim3(256), 0, st, __VA_ARGS__);      \
    } while (0)

// The gains of a call as its kernel takes them.  False when there are none, more than VOL_GAINS or a NaN among them, or when the
// volumes x gains x D planes of the gained volume exceed what grid.y holds.
static bool make_gains(const float* gains_host, int n_gains, int volumes, int D, VolGains& gains)
{
    if (!gains_host || n_gains < 1 || n_gains > VOL_GAINS || (long long)volumes * n_gains * D > 65535) return false;
    memset(&gains, 0, sizeof(gains));
    for (int i = 0; i < n_gains; ++i) {
        if (!(gains_host[i] == gains_host[i])) return false;
        gains.g[i] = gains_host[i];
    }
    return true;
}

// ---- Mack's rate law: with b = 1 - m the dissolved fraction, X = b^q, r = (rmax (a + 1) X / (a + X) + rmin) f, a = (q + 1) /
// (q - 1) (1 - m_th)^q and f the surface-inhibition factor of the plane, 1 - (1 - r0) exp(-z / delta) at z = thickness (d + 1/2) / D.
struct MackLaw {
    double rmax_a1, rmin, q, a;                          // the kernels take these four as scalars
    VolSurface surface;
};
// false when a parameter is outside its domain (litho_develop_rate's, include/litho_abbe.h)
static bool make_mack(double r_max, double r_min, double q, double m_th, double surface_rate, double surface_depth_nm, double thickness_nm,
                      int D, MackLaw& law)
{
    if (!finite_pos(r_max) || !finite_pos(r_min) || !(q > 1.0) || std::isinf(q) || !(m_th >= 0.0) || !(m_th < 1.0) ||
        !(surface_rate > 0.0) || !(surface_rate <= 1.0) || !finite_pos(surface_depth_nm) || !finite_pos(thickness_nm))
        return false;
    law.a = (q + 1.0) / (q - 1.0) * std::pow(1.0 - m_th, q);
    law.rmax_a1 = r_max * (law.a + 1.0);
    law.rmin = r_min;
    law.q = q;
    for (int d = 0; d < VOL_DMAX; ++d) {
        const double z = thickness_nm * (d + 0.5) / D;
        law.surface.f[d] = 1.0 - (1.0 - surface_rate) * std::exp(-z / surface_depth_nm);
    }
    return true;
}
// slowness = fp32(1 / r), rounded once.  b < 0 (a negative dose-intensity product) or NaN: pow is finite there for an integer q,
// so the NaN is written explicitly
__device__ __forceinline__ float mack_slowness(double b, double rmax_a1, double rmin, double q, double a, double f)
{
    const double x = pow(b, q);
    const double r = (rmax_a1 * x / (a + x) + rmin) * f;
    return (b >= 0.0) ? (float)(1.0 / r) : __builtin_nanf("");
}
// ds/dx of s = 1 / r for b = b(x) with db/dx = db: -s^2 f R a / (a + X)^2 q b^(q - 1) db, R = rmax (a + 1).  For b >= 0 only (the
// caller skips a wall).
__device__ __forceinline__ double mack_slowness_dx(double b, double db, double rmax_a1, double rmin, double q, double a, double f)
{
    const double X = pow(b, q);
    const double r = (rmax_a1 * X / (a + X) + rmin) * f;
    const double s = 1.0 / r;
    const double dX = q * pow(b, q - 1.0) * db;
    return -(s * s) * f * (rmax_a1 * a / ((a + X) * (a + X))) * dX;
}

// The derivatives of s = 1 / r with respect to the rate law's own numbers, for b >= 0 (the caller skips a wall), R = rmax (a + 1):
//   d[0] ds/dR     = -s^2 f X / (a + X)                        at fixed a
//   d[1] ds/drmin  = -s^2 f
//   d[2] ds/dq     = -s^2 f R a / (a + X)^2 X ln b             at fixed a; 0 at b = 0
//   d[3] ds/da     = -s^2 f (R / (a + 1)) X (X - 1) / (a + X)^2  at fixed rmax = R / (a + 1), R following a
//   d[4] ds/df     = -s / f
__device__ __forceinline__ void mack_slowness_dparams(double b, double rmax_a1, double rmin, double q, double a, double f, double (&d)[5])
{
    const double X = pow(b, q), aX = a + X;
    const double r = (rmax_a1 * X / aX + rmin) * f;
    const double s = 1.0 / r, ssf = (s * s) * f;
    d[0] = -ssf * (X / aX);
    d[1] = -ssf;
    d[2] = (b > 0.0) ? -ssf * (rmax_a1 * a / (aX * aX)) * (X * log(b)) : 0.0;
    d[3] = -ssf * (rmax_a1 / (a + 1.0)) * (X * (X - 1.0) / (aX * aX));
    d[4] = -(s / f);
}

// ---- sums without atomics (the parameter reductions of peb.hip and develop_grad.hip).  vol_block_sum: the N doubles of each
// thread of a 256-thread workgroup added in one fixed tree -- within a wave of 64 by shuffles from the upper half onto the lower
// (32, 16, .. 1), then the four waves in ascending order through LDS by thread 0, whose t[] holds the sums on return.  Every
// thread of the workgroup must call it.
template <int N>
__device__ __forceinline__ void vol_block_sum(double (&t)[N], double (*lds)[N])
{
    for (int j = 0; j < N; ++j)
        for (int off = 32; off >= 1; off >>= 1) t[j] = t[j] + __shfl_down(t[j], off, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int j = 0; j < N; ++j) lds[wave][j] = t[j];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int j = 0; j < N; ++j) t[j] = ((lds[0][j] + lds[1][j]) + lds[2][j]) + lds[3][j];
}
// out[g][N] = the sum of the `count` consecutive slots [N] of group g = blockIdx.x: thread i adds the slots i, i + 256, ... in
// ascending order, then the tree of vol_block_sum.  The order is fixed by `count` alone.
template <int N>
__global__ __launch_bounds__(256) void k_vol_total(const double* __restrict__ partials, long long count, double* __restrict__ out)
{
    __shared__ double lds[4][N];
    double t[N];
    for (int j = 0; j < N; ++j) t[j] = 0.0;
    const double* mine = partials + (size_t)blockIdx.x * (size_t)count * N;
    for (long long i = threadIdx.x; i < count; i += 256)
        for (int j = 0; j < N; ++j) t[j] = t[j] + mine[i * N + j];
    vol_block_sum<N>(t, lds);
    if (threadIdx.x == 0)
        for (int j = 0; j < N; ++j) out[(size_t)blockIdx.x * N + j] = t[j];
}

// ---- the geometry of the front solvers (litho_develop_time and its two derivatives) as they round it: the fp32 spacings and the
// weights 1 / spacing^2.  False when one of them leaves fp32's range.
struct FrontGeometry { float h, hz, wxy, wz; };
static bool front_geometry(double pixel_nm, double thickness_nm, int D, FrontGeometry& g)
{
    g.h = (float)pixel_nm; g.hz = (float)(thickness_nm / D);
    g.wxy = 1.f / (g.h * g.h); g.wz = 1.f / (g.hz * g.hz);
    return g.h > 0.f && g.hz > 0.f && !std::isinf(g.wxy) && !std::isinf(g.wz) && g.wxy > 0.f && g.wz > 0.f;
}

// ---- the host loop of the tiled solvers (k_develop_time, k_develop_time_vjp).  enqueue(it) puts launch it = 0, 1, ... on `st`;
// launch `it` stores 1 into flags[it] when it changed a cell.  The flag words are zeroed up front; the launches go out in groups
// of VOL_CHECK, each group followed by one copy-back of its flag words and one synchronise.  Returns the number of launches up
// to and including the first one that changed nothing (its output equals its input), 0 when none of max_iterations did, or
// LITHO_E_HIP.
template <class F>
static int iterate_until_unchanged(int* flags, int max_iterations, hipStream_t st, F enqueue)
{
    HIP_TRY(hipMemsetAsync(flags, 0, flag_bytes(max_iterations), st));
    for (int done = 0; done < max_iterations;) {
        const int group = max_iterations - done < VOL_CHECK ? max_iterations - done : VOL_CHECK;
        for (int j = 0; j < group; ++j) enqueue(done + j);
        HIP_TRY(hipGetLastError());
        int seen[VOL_CHECK] = {1, 1, 1, 1};
        HIP_TRY(hipMemcpyAsync(seen, flags + done, (size_t)group * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int j = 0; j < group; ++j)
            if (seen[j] == 0) return done + j + 1;
        done += group;
    }
    return 0;
}

}  // namespace litho
