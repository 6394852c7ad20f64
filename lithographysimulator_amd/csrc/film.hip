// film.hip -- vector imaging into a resist film stack: the six pupil planes at depths inside one layer of a thin-film stack.
//
// litho_vector_pupils (socs.hip) images into one homogeneous medium.  Here the wafer side is a stack: the incident medium of
// real index n0, L finite layers (n, k, thickness), a semi-infinite substrate; one layer, the resist, is sampled at D depths.
// Only the six planes Q_cj change -- the vector TCC, its factorisation and every consumer take them as they are
// (include/litho_abbe.h).  No reference counterpart; checked against tests/film_oracle.py.
//
// Per pupil cell, s = NA^2 sigma^2 is the conserved squared transverse index; in a medium of complex index nn = n - i k the
// normal component is w = sqrt(nn^2 - s) with Im w <= 0 (the engine's waves advance into the wafer as exp(-i kappa z),
// kappa = 2 pi w / lambda, so an absorbing or evanescent wave decays with depth).  Two scalar problems share one recursion,
//   u(z) = a exp(-i kappa z) + b exp(+i kappa z),   v = eta (a exp(-i kappa z) - b exp(+i kappa z)),   u, v continuous,
// s-polarisation with u = E_s, eta = w, a0 = 1, and p-polarisation with u = H_s, eta = w / nn^2, a0 = n0.
//
// Evaluation, one thread per cell: with Gamma the ratio upward / downward at the TOP of the medium below (0 in the substrate),
//   D_m = eta_m (1 + Gamma) + eta_m+1 (1 - Gamma),   rho_m = (eta_m (1 + Gamma) - eta_m+1 (1 - Gamma)) / D_m
// is the ratio at the BOTTOM of medium m, the downward amplitude crosses the interface as a_m+1 = (a_m e_m) 2 eta_m / D_m, and
// Gamma_m = rho_m e_m^2 with e_m = exp(-i kappa_m d_m), |e_m| <= 1.  The media are walked once, from the substrate up; the
// transfer factors of the media above the resist are multiplied up on the way (a product, so its order is free), which leaves
// no per-thread array.  In the resist the upward wave is referenced to the layer's bottom, b exp(+i kappa z) =
// c exp(+i kappa (z - d)) with c = rho a e: no exponential with a positive real exponent is ever formed, and every cell inside
// alpha^2 + beta^2 < 1 gives finite planes whatever the thicknesses and absorptions.  (w = 0 exactly in a layer -- grazing
// propagation in it -- divides by zero in the p-problem; that single point is not pinned.)
//
// The stack travels by value as a kernel argument: the layer loop indexes it uniformly, so the reads are scalar loads of the
// kernel-argument segment.  Double precision per cell as k_vector_pupils, each output component rounded to fp32 once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/litho_abbe.h"
#include "engine_common.hpp"

namespace litho {

static constexpr int FILM_MAX_LAYERS = 16;
static constexpr int FILM_DEPTHS = 16;          // depths per launch; a longer list takes ceil(D / 16) launches per plane
static constexpr int FILM_T = 6;

struct FilmTable {
    int media;                                  // L + 2: incident medium, the layers, substrate
    int resist;                                 // index into the media, 1 ... L
    int depths;                                 // of this launch, 1 ... FILM_DEPTHS
    int pad;
    double e_re[FILM_MAX_LAYERS + 2];           // nn^2 = (n - i k)^2 per medium
    double e_im[FILM_MAX_LAYERS + 2];
    double halfwaves[FILM_MAX_LAYERS + 2];      // 2 d / lambda per layer (unused at both ends): kappa d = pi w halfwaves
    double z_top[FILM_DEPTHS];                  // 2 z / lambda, z below the top of the resist
    double z_bottom[FILM_DEPTHS];               // 2 (d_resist - z) / lambda
};

struct cplx {
    double re, im;
};
__device__ __forceinline__ cplx operator+(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cplx operator-(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx operator*(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cplx operator*(double f, cplx a) { return {f * a.re, f * a.im}; }
__device__ __forceinline__ cplx operator/(cplx a, cplx b)
{
    const double q = 1.0 / (b.re * b.re + b.im * b.im);
    return {(a.re * b.re + a.im * b.im) * q, (a.im * b.re - a.re * b.im) * q};
}

// sqrt(x + i y) for y <= 0 on the branch Im <= 0 (Re > 0 when Im = 0, -i sqrt(-x) for a negative real argument)
__device__ __forceinline__ cplx film_sqrt(double x, double y)
{
    if (y == 0.0) return x >= 0.0 ? cplx{sqrt(x), 0.0} : cplx{0.0, -sqrt(-x)};
    const double m = hypot(x, y);
    if (x >= 0.0) {
        const double re = sqrt(0.5 * (m + x));
        return {re, y / (2.0 * re)};
    }
    const double im = -sqrt(0.5 * (m - x));
    return {y / (2.0 * im), im};
}

// exp(-i pi w h) for Im w <= 0, h >= 0: modulus exp(pi Im w h) <= 1
__device__ __forceinline__ cplx film_decay(cplx w, double h)
{
    double sn, cs;
    sincospi(w.re * h, &sn, &cs);
    const double mod = exp(M_PI * w.im * h);
    return {mod * cs, -mod * sn};
}

// One thread per cell of one pupil plane: the two recursions once, then the depths of this launch.  out points at this
// plane's first depth of the launch; consecutive depths are 6 cells apart.
__global__ __launch_bounds__(256) void k_film_pupils(const float2* __restrict__ pupil, int pn, double NA, double index,
                                                     int radiometric, double waves /* index z_focus / wavelength */,
                                                     const FilmTable tab, float2* __restrict__ out)
{
    const size_t cells = (size_t)pn * pn;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const int r = (int)(i / pn), c = (int)(i - (size_t)r * pn);
    const double a = NA * ((double)(c - pn / 2) * 4.0 / (double)pn) / index;
    const double b = NA * ((double)(r - pn / 2) * 4.0 / (double)pn) / index;
    const double s0 = a * a + b * b;
    if (!(s0 < 1.0)) {                                             // evanescent in the incident medium: every plane is 0
        for (int d = 0; d < tab.depths; ++d)
#pragma unroll
            for (int t = 0; t < FILM_T; ++t) out[((size_t)d * FILM_T + t) * cells + i] = make_float2(0.f, 0.f);
        return;
    }
    const double s = index * index * s0;
    const int top = tab.media - 1;
    // from the substrate up
    cplx w_below = film_sqrt(tab.e_re[top] - s, tab.e_im[top]);
    cplx p_below = w_below / cplx{tab.e_re[top], tab.e_im[top]};
    cplx gam_s = {0.0, 0.0}, gam_p = {0.0, 0.0};                   // Gamma at the top of the medium below
    cplx tau_s = {1.0, 0.0}, tau_p = {1.0, 0.0};                   // a_resist / a0
    cplx rho_s = {0.0, 0.0}, rho_p = {0.0, 0.0}, w_res = {0.0, 0.0}, e_res = {0.0, 0.0};
    for (int m = top - 1; m >= 0; --m) {
        const cplx w = film_sqrt(tab.e_re[m] - s, tab.e_im[m]);
        const cplx p = w / cplx{tab.e_re[m], tab.e_im[m]};
        const cplx one = {1.0, 0.0};
        const cplx us = w * (one + gam_s), ds = w_below * (one - gam_s);
        const cplx up = p * (one + gam_p), dp = p_below * (one - gam_p);
        const cplx rs = (us - ds) / (us + ds), rp = (up - dp) / (up + dp);
        cplx e = one;
        if (m > 0) e = film_decay(w, tab.halfwaves[m]);
        if (m < tab.resist) {
            tau_s = tau_s * (e * ((2.0 * w) / (us + ds)));
            tau_p = tau_p * (e * ((2.0 * p) / (up + dp)));
        }
        if (m == tab.resist) {
            rho_s = rs;
            rho_p = rp;
            w_res = w;
            e_res = e;
        }
        gam_s = rs * (e * e);
        gam_p = rp * (e * e);
        w_below = w;
        p_below = p;
    }
    // amplitudes in the resist: a downward at its top, c upward at its bottom
    const cplx a_s = tau_s, c_s = rho_s * (a_s * e_res);
    const cplx a_p = index * tau_p, c_p = rho_p * (a_p * e_res);
    const cplx inv_e = cplx{1.0, 0.0} / cplx{tab.e_re[tab.resist], tab.e_im[tab.resist]};
    const cplx eta_p = w_res * inv_e;
    const double root_s = sqrt(s);
    // the pupil value with gamma^(-1/2) and the defocus phase of the incident medium, as k_vector_pupils
    const double g = sqrt(1.0 - s0), dd = 1.0 / (1.0 + g);
    const double f = radiometric ? 1.0 / sqrt(g) : 1.0;
    double sn, cs;
    sincospi(2.0 * waves * (s0 * dd), &sn, &cs);
    const float2 pv = pupil[i];
    const cplx P = {f * ((double)pv.x * cs - (double)pv.y * sn), f * ((double)pv.x * sn + (double)pv.y * cs)};
    const bool centre = s0 == 0.0;
    const double rn = centre ? 0.0 : 1.0 / sqrt(s0);
    const double rx = a * rn, ry = b * rn;
    for (int d = 0; d < tab.depths; ++d) {
        const cplx down = film_decay(w_res, tab.z_top[d]), upw = film_decay(w_res, tab.z_bottom[d]);
        const cplx Es = a_s * down + c_s * upw;
        const cplx H = a_p * down + c_p * upw;
        const cplx Erad = centre ? Es : eta_p * (a_p * down - c_p * upw);
        const cplx Ez = (-root_s) * (inv_e * H);
        const cplx diff = Erad - Es;
        const cplx m[FILM_T] = {Es + (rx * rx) * diff, (rx * ry) * diff, (rx * ry) * diff, Es + (ry * ry) * diff, rx * Ez, ry * Ez};
#pragma unroll
        for (int t = 0; t < FILM_T; ++t) {
            const cplx q = P * m[t];
            out[((size_t)d * FILM_T + t) * cells + i] = make_float2((float)q.re, (float)q.im);
        }
    }
}

static bool film_finite(double v) { return v > -1e300 && v < 1e300; }

}  // namespace litho

extern "C" {

int litho_film_pupils(const void* pupil, int planes, int pn, double NA, double index, int radiometric, const double* layers, int L,
                      double substrate_n, double substrate_k, int resist, const double* depths_nm, int D,
                      const double* defocus_nm_host, double wavelength, void* out, void* stream)
{
    using namespace litho;
    if (!pupil || !out || !layers || !depths_nm || planes < 1 || pn < 16 || pn > 16384 || (pn & 1)) return LITHO_E_ARG;
    if (L < 1 || L > FILM_MAX_LAYERS || resist < 0 || resist >= L || D < 1 || (int64_t)planes * D > 65535) return LITHO_E_ARG;
    if (!(NA > 0.0) || !(index > 0.0) || !(NA < index) || !(index < 1e6)) return LITHO_E_ARG;
    if (!(wavelength > 0.0) || !(wavelength < 1e300)) return LITHO_E_ARG;
    for (int l = 0; l < L; ++l) {
        const double n = layers[3 * l], k = layers[3 * l + 1], d = layers[3 * l + 2];
        if (!(n > 0.0 && n < 1e6) || !(k >= 0.0 && k < 1e6) || !(d > 0.0) || !film_finite(d)) return LITHO_E_ARG;
    }
    if (!(substrate_n > 0.0 && substrate_n < 1e6) || !(substrate_k >= 0.0 && substrate_k < 1e6)) return LITHO_E_ARG;
    const double d_resist = layers[3 * resist + 2];
    for (int d = 0; d < D; ++d)
        if (!(depths_nm[d] >= 0.0 && depths_nm[d] <= d_resist)) return LITHO_E_ARG;
    if (defocus_nm_host)
        for (int p = 0; p < planes; ++p)
            if (!film_finite(defocus_nm_host[p])) return LITHO_E_ARG;

    FilmTable tab = {};
    tab.media = L + 2;
    tab.resist = resist + 1;
    tab.e_re[0] = index * index;
    tab.e_re[L + 1] = substrate_n * substrate_n - substrate_k * substrate_k;
    tab.e_im[L + 1] = -2.0 * substrate_n * substrate_k;
    for (int l = 0; l < L; ++l) {
        const double n = layers[3 * l], k = layers[3 * l + 1];
        tab.e_re[l + 1] = n * n - k * k;
        tab.e_im[l + 1] = -2.0 * n * k;
        tab.halfwaves[l + 1] = 2.0 * layers[3 * l + 2] / wavelength;
    }
    const size_t cells = (size_t)pn * pn;
    const dim3 grid((unsigned)((cells + 255) / 256));
    for (int d0 = 0; d0 < D; d0 += FILM_DEPTHS) {
        tab.depths = D - d0 < FILM_DEPTHS ? D - d0 : FILM_DEPTHS;
        for (int d = 0; d < tab.depths; ++d) {
            tab.z_top[d] = 2.0 * depths_nm[d0 + d] / wavelength;
            tab.z_bottom[d] = 2.0 * (d_resist - depths_nm[d0 + d]) / wavelength;
        }
        for (int p = 0; p < planes; ++p) {                          // one launch per plane: its defocus travels as an argument
            const double waves = defocus_nm_host ? index * defocus_nm_host[p] / wavelength : 0.0;
            hipLaunchKernelGGL(k_film_pupils, grid, dim3(256), 0, (hipStream_t)stream, (const float2*)pupil + (size_t)p * cells, pn,
                               NA, index, radiometric ? 1 : 0, waves, tab,
                               (float2*)out + ((size_t)p * D + d0) * FILM_T * cells);
        }
    }
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

}  // extern "C"
