// metrology.hip -- edge placement error on layout edges behind litho_measure_epe (no reference counterpart; the definition
// is in include/litho_abbe.h, the checker its CPU restatement tests/epe_oracle.py).  Built with -ffp-contract=off
// (Makefile): every sample is a fixed sequence of fp32 operations that a NumPy float32 restatement reproduces bit for bit.
//
// One 64-lane wave per (site, plane), lanes as samples along the site's normal, the gains in a loop inside.  The outward
// half (samples k = 0 .. K, K <= 64) is read first: lane l holds sample l and gets sample l + 1 from its neighbour
// (__shfl_down; lane 63 reads sample 64 itself).  __ballot + a bit scan give the first crossing going outward, kp.  A
// crossing on the inward half wins only when it is nearer, |2k + 1| < 2 kp + 1, so only the lanes l < kp of the inward half
// (sample -1 - l, its neighbour from lane l - 1, lane 0's from the outward half) read the image at all: a site on a
// printed edge costs a handful of gathers, not 129.  No LDS, no barrier, no atomics.  A lane gathers four floats from two
// image rows; consecutive sites of a polygon edge touch neighbouring lines -- accepted, as k_measure_cd's column gauge is.
// A sample outside the grid (or not finite) is never turned into an address.
#include "cd_search.hpp"
#include "engine_common.hpp"
#include "../../include/litho_abbe.h"

#include <cmath>
#include <cstdint>
#include <cstring>

namespace litho {

static constexpr int EPE_GAINS = 64, EPE_WAVES = 4;      // four sites per 256-thread workgroup
struct EpeGains {
    float g[EPE_GAINS];                                  // rides in the kernel arguments
};

// sample k of a site: position, validity, bilinear value (the form of bilinear_at); an invalid sample reads nothing
__device__ __forceinline__ float epe_sample(const float* __restrict__ img, int n, float x, float y, float nx, float ny, int k,
                                            bool& valid)
{
    const float top = (float)(n - 1);
    const float t = (float)k * 0.5f;
    const float px = x + t * nx, py = y + t * ny;
    valid = n >= 2 && px >= 0.f && px <= top && py >= 0.f && py <= top;       // NaN and inf fail the comparisons
    if (!valid) return 0.f;
    const int ix = min((int)floorf(px), n - 2), iy = min((int)floorf(py), n - 2);
    const float fx = px - (float)ix, fy = py - (float)iy;
    const float* q = img + (size_t)iy * n + ix;
    const float a = q[0], b = q[1], c = q[n], d = q[n + 1];
    return (1.f - fy) * ((1.f - fx) * a + fx * b) + fy * ((1.f - fx) * c + fx * d);
}

// The search of one site on one plane by one wave, shared by the primal and its tangent: for every gain, exactly one lane calls
// emit(gi, found, k, a, b) -- the lane of the chosen interval k with its ends a = u_k and b = u_{k+1}, or lane 0 with found = false.
template <class Emit>
__device__ __forceinline__ void epe_search(const float* __restrict__ img, int n, float x, float y, float nx, float ny,
                                           const EpeGains& gains, int n_gains, float T, bool ex, int K, int lane, Emit&& emit)
{
    auto sample = [&](int k, bool& valid) -> float { return epe_sample(img, n, x, y, nx, ny, k, valid); };
    // outward half: lane = sample k = lane (0 .. K), interval k = lane (0 .. K - 1)
    bool okP = false, ok64 = false;
    float vP = 0.f, v64 = 0.f;
    if (lane <= K) vP = sample(lane, okP);
    if (lane == 63 && K == 64) v64 = sample(64, ok64);
    float vP1 = __shfl_down(vP, 1);
    bool okP1 = __shfl_down((int)okP, 1) != 0;
    if (lane == 63) { vP1 = v64; okP1 = ok64; }
    const bool pairP = lane < K && okP && okP1;
    // how far the inward half can matter: the farthest first outward crossing over the gains (K where a gain has none)
    int need = 0;
    for (int gi = 0; gi < n_gains; ++gi) {
        const float gain = gains.g[gi];
        const unsigned long long m = __ballot(pairP && ((vP * gain >= T) == ex) && ((vP1 * gain >= T) != ex));
        need = max(need, m ? __ffsll((long long)m) - 1 : K);
    }
    // inward half: lane = interval k = -1 - lane, its sample k is the lane's own, sample k + 1 the previous lane's
    bool okN = false;
    float vN = 0.f;
    if (lane < need) vN = sample(-1 - lane, okN);
    float vN1 = __shfl_up(vN, 1);
    bool okN1 = __shfl_up((int)okN, 1) != 0;
    const float v0 = __shfl(vP, 0);
    const bool ok0 = __shfl((int)okP, 0) != 0;
    if (lane == 0) { vN1 = v0; okN1 = ok0; }
    const bool pairN = lane < need && okN && okN1;
    for (int gi = 0; gi < n_gains; ++gi) {
        const float gain = gains.g[gi];
        const float aP = vP * gain, bP = vP1 * gain, aN = vN * gain, bN = vN1 * gain;
        const unsigned long long mP = __ballot(pairP && ((aP >= T) == ex) && ((bP >= T) != ex));
        const unsigned long long mN = __ballot(pairN && ((aN >= T) == ex) && ((bN >= T) != ex));
        const int kp = mP ? __ffsll((long long)mP) - 1 : -1;                    // interval kp, |2k + 1| = 2 kp + 1
        const int ln = mN ? __ffsll((long long)mN) - 1 : -1;                    // interval -1 - ln, |2k + 1| = 2 ln + 1
        const bool takeP = kp >= 0 && (ln < 0 || kp <= ln);                     // a tie goes to k >= 0
        const bool takeN = !takeP && ln >= 0;
        if (takeP ? lane == kp : (takeN ? lane == ln : lane == 0))
            emit(gi, takeP || takeN, takeP ? kp : -1 - ln, takeP ? aP : aN, takeP ? bP : bN);
    }
}

__global__ __launch_bounds__(64 * EPE_WAVES) void k_measure_epe(const float* __restrict__ image, int planes, int n,
                                                                const float* __restrict__ sites, long long S,
                                                                const EpeGains gains, int n_gains, float T, int exposed, int K,
                                                                float ps, float* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * EPE_WAVES + (threadIdx.x >> 6);
    const int p = blockIdx.y;
    if (s >= S) return;                                  // wave-uniform
    const float x = sites[4 * s], y = sites[4 * s + 1], nx = sites[4 * s + 2], ny = sites[4 * s + 3];
    const float nan = __builtin_nanf("");
    epe_search(image + (size_t)p * n * n, n, x, y, nx, ny, gains, n_gains, T, exposed != 0, K, lane,
               [&](int gi, bool found, int k, float a, float b) {
                   float* o = out + (((size_t)gi * planes + p) * (size_t)S + (size_t)s) * 3;
                   float epe = nan, ils = nan, tk = nan;
                   if (found) {
                       tk = (float)k * 0.5f;
                       const float ts = tk + 0.5f * ((T - a) / (b - a));
                       epe = ts * ps;
                       ils = fabsf(b - a) / ((0.5f * ps) * T);
                   }
                   o[0] = epe; o[1] = ils; o[2] = tk;
               });
}

// The tangent of k_measure_epe: the same search on the primal image, then on the lane that owns the chosen interval
//   d epe = ps h [ -du_k (u_{k+1} - u_k) - (T - u_k)(du_{k+1} - du_k) ] / (u_{k+1} - u_k)^2,   du = gain . bilinear(dImage) at the
// same two points, direction by direction; NaN where the primal is NaN.  dImage [P][planes][n][n], out [P][n_gains][planes][S].
__global__ __launch_bounds__(64 * EPE_WAVES) void k_measure_epe_jvp(const float* __restrict__ image, const float* __restrict__ dImage,
                                                                    int P, int planes, int n, const float* __restrict__ sites,
                                                                    long long S, const EpeGains gains, int n_gains, float T,
                                                                    int exposed, int K, float ps, float* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * EPE_WAVES + (threadIdx.x >> 6);
    const int p = blockIdx.y;
    if (s >= S) return;                                  // wave-uniform
    const float x = sites[4 * s], y = sites[4 * s + 1], nx = sites[4 * s + 2], ny = sites[4 * s + 3];
    const float nan = __builtin_nanf("");
    const size_t cells = (size_t)n * n;
    epe_search(image + (size_t)p * cells, n, x, y, nx, ny, gains, n_gains, T, exposed != 0, K, lane,
               [&](int gi, bool found, int k, float a, float b) {
                   const float gain = gains.g[gi];
                   for (int d = 0; d < P; ++d) {
                       float v = nan;
                       if (found) {
                           const float* dimg = dImage + ((size_t)d * planes + p) * cells;
                           bool ok;                      // both samples are valid: the primal read them at the same points
                           const float da = epe_sample(dimg, n, x, y, nx, ny, k, ok) * gain;
                           const float db = epe_sample(dimg, n, x, y, nx, ny, k + 1, ok) * gain;
                           const float w = b - a;
                           v = (ps * 0.5f) * ((-da * w - (T - a) * (db - da)) / (w * w));
                       }
                       out[(((size_t)d * n_gains + gi) * planes + p) * (size_t)S + (size_t)s] = v;
                   }
               });
}

// The tangent of k_measure_cd (optics.hip), on the run that cd_run (cd_search.hpp) finds for the primal: one wave per (gauge,
// plane), lane d < P takes direction d.  x = i + (T - a) / (b - a) between samples i, i + 1 has
//   dx = [ -da (b - a) - (T - a)(db - da) ] / (b - a)^2;  a border edge does not move.  out [P][n_gains][planes][G][3] =
// (dcd_nm, dx_lo, dx_hi); not inside: (0, NaN, NaN); a gauge outside the grid: three NaN -- the primal's pattern.
__global__ __launch_bounds__(64) void k_measure_cd_jvp(const float* __restrict__ image, const float* __restrict__ dImage, int P,
                                                       int planes, int n, const int32_t* __restrict__ gauges, int G,
                                                       const EpeGains gains, int n_gains, float T, int exposed, float ps,
                                                       float* __restrict__ out)
{
    const int g = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    const int row = gauges[3 * g], col = gauges[3 * g + 1], axis = gauges[3 * g + 2];
    const bool ok = row >= 0 && row < n && col >= 0 && col < n && (axis == 0 || axis == 1);   // else: never touch the images
    const size_t stride = axis == 0 ? 1 : (size_t)n;
    const size_t start = axis == 0 ? (size_t)row * n : (size_t)col;
    const float* line = image + (size_t)p * n * n + start;
    const int c = axis == 0 ? col : row;
    const bool ex = exposed != 0;
    const float nan = __builtin_nanf("");
    for (int gi = 0; gi < n_gains; ++gi) {
        const float gain = gains.g[gi];
        auto u = [&](int i) { return line[(size_t)i * stride] * gain; };
        float dcd = nan, dlo = nan, dhi = nan;
        if (ok && ((u(c) >= T) == ex)) {
            int lo, hi;
            cd_run(u, c, n, lane, T, ex, lo, hi);
            if (lane < P) {
                const float* dline = dImage + ((size_t)lane * planes + p) * n * n + start;
                auto du = [&](int i) { return dline[(size_t)i * stride] * gain; };
                auto dx = [&](int i) {
                    const float a = u(i), b = u(i + 1), da = du(i), db = du(i + 1), w = b - a;
                    return (-da * w - (T - a) * (db - da)) / (w * w);
                };
                dlo = lo > 0 ? dx(lo - 1) : 0.f;
                dhi = hi < n - 1 ? dx(hi) : 0.f;
                dcd = (dhi - dlo) * ps;
            }
        } else if (ok) {
            dcd = 0.f;
        }
        if (lane < P) {
            float* o = out + ((((size_t)lane * n_gains + gi) * planes + p) * G + g) * 3;
            o[0] = dcd; o[1] = dlo; o[2] = dhi;
        }
    }
}

}  // namespace litho

extern "C" {

int litho_measure_epe(const float* image, int planes, int n, const float* sites, int64_t n_sites, const float* gains_host,
                      int n_gains, float threshold, int exposed, float range_px, float pixel_size, float* out, void* stream)
{
    using namespace litho;
    if (!image || !sites || !gains_host || !out || planes < 1 || planes > 65535 || n < 1 || n_sites < 1) return LITHO_E_ARG;
    if (n_gains < 1 || n_gains > EPE_GAINS || !(range_px > 0.f) || !(range_px <= 32.f) || !(pixel_size > 0.f) ||
        std::isinf(pixel_size))
        return LITHO_E_ARG;
    const int64_t blocks = (n_sites + EPE_WAVES - 1) / EPE_WAVES;
    if (blocks > 2147483647LL) return LITHO_E_ARG;
    EpeGains gains;
    memset(&gains, 0, sizeof(gains));
    for (int i = 0; i < n_gains; ++i) {
        if (!(gains_host[i] == gains_host[i])) return LITHO_E_ARG;
        gains.g[i] = gains_host[i];
    }
    const int K = (int)std::ceil((double)range_px * 2.0);                        // range_px / h, h = 0.5: 1 .. 64
    hipLaunchKernelGGL(k_measure_epe, dim3((unsigned)blocks, planes), dim3(64 * EPE_WAVES), 0, (hipStream_t)stream, image, planes,
                       n, sites, (long long)n_sites, gains, n_gains, threshold, exposed, K, pixel_size, out);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_measure_epe_jvp(const float* image, const float* dImage, int P, int planes, int n, const float* sites, int64_t n_sites,
                          const float* gains_host, int n_gains, float threshold, int exposed, float range_px, float pixel_size,
                          float* out, void* stream)
{
    using namespace litho;
    if (!image || !dImage || !sites || !gains_host || !out || P < 1 || P > LITHO_SOCS_JVP_MAX_DIRECTIONS || planes < 1 ||
        planes > 65535 || n < 1 || n_sites < 1)
        return LITHO_E_ARG;
    if (n_gains < 1 || n_gains > EPE_GAINS || !(range_px > 0.f) || !(range_px <= 32.f) || !(pixel_size > 0.f) ||
        std::isinf(pixel_size))
        return LITHO_E_ARG;
    const int64_t blocks = (n_sites + EPE_WAVES - 1) / EPE_WAVES;
    if (blocks > 2147483647LL) return LITHO_E_ARG;
    EpeGains gains;
    memset(&gains, 0, sizeof(gains));
    for (int i = 0; i < n_gains; ++i) {
        if (!(gains_host[i] == gains_host[i])) return LITHO_E_ARG;
        gains.g[i] = gains_host[i];
    }
    const int K = (int)std::ceil((double)range_px * 2.0);
    hipLaunchKernelGGL(k_measure_epe_jvp, dim3((unsigned)blocks, planes), dim3(64 * EPE_WAVES), 0, (hipStream_t)stream, image, dImage,
                       P, planes, n, sites, (long long)n_sites, gains, n_gains, threshold, exposed, K, pixel_size, out);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_measure_cd_jvp(const float* image, const float* dImage, int P, int planes, int n, const int32_t* gauges, int n_gauges,
                         const float* gains_host, int n_gains, double threshold, int exposed, double pixel_size, float* out,
                         void* stream)
{
    using namespace litho;
    if (!image || !dImage || !gauges || !gains_host || !out || P < 1 || P > LITHO_SOCS_JVP_MAX_DIRECTIONS || planes < 1 ||
        planes > 65535 || n < 1 || n_gauges < 1)
        return LITHO_E_ARG;
    if (n_gains < 1 || n_gains > EPE_GAINS || !(threshold == threshold) || !(pixel_size > 0.0) || std::isinf(pixel_size))
        return LITHO_E_ARG;
    EpeGains gains;
    memset(&gains, 0, sizeof(gains));
    for (int i = 0; i < n_gains; ++i) {
        if (!(gains_host[i] == gains_host[i])) return LITHO_E_ARG;
        gains.g[i] = gains_host[i];
    }
    hipLaunchKernelGGL(k_measure_cd_jvp, dim3(n_gauges, planes), dim3(64), 0, (hipStream_t)stream, image, dImage, P, planes, n, gauges,
                       n_gauges, gains, n_gains, (float)threshold, exposed, (float)pixel_size, out);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

}  // extern "C"
