// develop.hip -- resist development behind litho_latent_diffuse, litho_develop_rate, litho_develop_time and litho_developed_depth
// (no reference counterpart; the definitions are in include/litho_abbe.h, the checker is their float64 restatement
// tests/develop_oracle.py).  Built with -ffp-contract=off (Makefile): every fp32 result is a fixed sequence of single operations.
//
// Volumes are fp32 [B, D, n, n], D <= 32 planes through the resist, x fastest.  The limits, the packs, the host predicates, the
// gains, Mack's rate law and the solver's host loop are resist_volume.hpp's, shared with peb.hip and develop_grad.hip.  Four kernels:
//   k_latent_diffuse   one pass of the separable Gaussian along x, y (zero outside the grid) or z (mirrored layer faces); a gather
//                      per output element, lanes along x, so every load of a wave is one contiguous run of a row
//   k_develop_rate     Dill C exposure and Mack's rate in double per cell, the gains in a loop inside, slowness 1 / r out
//   k_develop_time     the development front: a tiled fast-iterative solver of |grad T| = s (below)
//   k_developed_depth  one thread per column walks down to the first plane that is not developed
// The pointwise kernels move four consecutive x per thread (16-byte accesses) when n is a multiple of 4 and the pointers are
// 16-byte aligned, one otherwise.
//
// k_develop_time.  A workgroup owns a 16 x 16 lateral tile with all D planes: T of tile + one-cell halo and s of the tile live in
// LDS, D (18 . 18 + 16 . 16) floats = 72.5 KiB at D = 32.  It relaxes the tile VOL_INNER rounds; a round is two phases, the columns
// with (row + col) even, a barrier, the odd ones, a barrier.  In a phase 128 threads own one column each and sweep it down and
// up (Gauss-Seidel along z, where the front mostly runs); the four lateral neighbours of a column have the other colour and are
// not written in that phase, so there is no race and the result does not depend on scheduling.  Halo cells are read-only, cells
// outside the grid hold +inf.  Launches ping-pong T between two global buffers: no workgroup reads what another writes.  A cell
// "changed" when it took a strictly smaller value (new < old: false for a NaN); a thread that changed one stores 1 into the
// launch's own flag word with a plain store.  The host reads the flag words every VOL_CHECK launches and stops at the first
// launch that changed nothing: its output equals its input, so both buffers hold the fixed point.  Values only ever decrease and
// every loop has a trip count fixed by D: a launch cannot hang, and the launch count is capped by the caller.
#include "resist_volume.hpp"

namespace litho {

static constexpr int DEV_RMAX = 32;
static constexpr int DEV_TCELLS = VOL_HALO * VOL_HALO, DEV_SCELLS = VOL_TILE * VOL_TILE;

struct DevTaps {
    float g[DEV_RMAX + 1];                               // g[|k|], normalised over k = -R .. R; rides in the kernel arguments
};

// ---- 1. one pass of the latent-image diffusion.  axis 0: along x, 1: along y (zero outside), 2: along z (mirror).  grid.x covers
// the n^2 / VEC packs of a plane, grid.y the B D planes.  Symmetric taps are paired, acc = g[0] c; acc += g[k] (c[-k] + c[k]),
// ascending k -- the order of k_postprocess_diffused.
template <int VEC>
__global__ __launch_bounds__(256) void k_latent_diffuse(const float* __restrict__ in, float* __restrict__ out, int D, int n, int axis,
                                                        const DevTaps taps, int R)
{
    const long long plane_elems = (long long)n * n;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e >= plane_elems) return;
    const int p = blockIdx.y, row = (int)(e / n), col = (int)(e % n);
    const int d = p % D;
    const float* vol = in + (size_t)(p - d) * plane_elems;                  // plane 0 of this volume
    const float* here = in + (size_t)p * plane_elems + e;
    // the neighbour at signed offset k along the axis: zeros where the grid ends, never an address outside the volume
    auto at = [&](int k) -> Pack<VEC> {
        Pack<VEC> z;
        for (int v = 0; v < VEC; ++v) z.v[v] = 0.f;
        if (axis == 0) {
            const int c = col + k;
            return (c >= 0 && c < n) ? load_pack<VEC>(here + k) : z;      // VEC == 1 on this axis
        }
        if (axis == 1) {
            const int r = row + k;
            return (r >= 0 && r < n) ? load_pack<VEC>(here + (long long)k * n) : z;
        }
        return load_pack<VEC>(vol + (size_t)mirror_index(d + k, D) * plane_elems + e);
    };
    Pack<VEC> c = load_pack<VEC>(here), acc;
    for (int v = 0; v < VEC; ++v) acc.v[v] = taps.g[0] * c.v[v];
    for (int k = 1; k <= R; ++k) {
        const Pack<VEC> lo = at(-k), hi = at(k);
        for (int v = 0; v < VEC; ++v) acc.v[v] = acc.v[v] + taps.g[k] * (lo.v[v] + hi.v[v]);
    }
    store_pack<VEC>(out + (size_t)p * plane_elems + e, acc);
}

// ---- 2. Dill C exposure and Mack's rate: m = exp(-(C g) I), then mack_slowness of 1 - m with the surface factor of the plane
// (resist_volume.hpp): NaN where 1 - m is negative or NaN.  Double per cell, rounded once.  grid.y: the F D planes of the image.
template <int VEC>
__global__ __launch_bounds__(256) void k_develop_rate(const float* __restrict__ image, float* __restrict__ out, int planes, int D, int n,
                                                      const VolGains gains, int n_gains, double C, double rmax_a1, double rmin, double q,
                                                      double a, const VolSurface surface)
{
    const long long plane_elems = (long long)n * n;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e >= plane_elems) return;
    const int p = blockIdx.y;
    const double f = surface.f[p % D];
    const Pack<VEC> I = load_pack<VEC>(image + (size_t)p * plane_elems + e);
    for (int gi = 0; gi < n_gains; ++gi) {
        const double Cg = C * (double)gains.g[gi];
        Pack<VEC> s;
        for (int v = 0; v < VEC; ++v) {
            const double m = exp(-(Cg * (double)I.v[v]));
            s.v[v] = mack_slowness(1.0 - m, rmax_a1, rmin, q, a, f);
        }
        store_pack<VEC>(out + ((size_t)gi * planes + p) * plane_elems + e, s);
    }
}

// ---- 3. the development front
// The first-order Godunov update of one cell from (a, h, w = 1 / h^2) on the three axes, in the shifted form u = T - a_min.
__device__ __forceinline__ float godunov(float a0, float h0, float w0, float a1, float h1, float w1, float a2, float h2, float w2,
                                         float s)
{
    float t;
#define DEV_SWAP(i, j)                                                                          \
    if (a##i > a##j) {                                                                          \
        t = a##i; a##i = a##j; a##j = t; t = h##i; h##i = h##j; h##j = t; t = w##i; w##i = w##j; w##j = t; \
    }
    DEV_SWAP(0, 1)
    DEV_SWAP(1, 2)
    DEV_SWAP(0, 1)
#undef DEV_SWAP
    if (!(a0 < INFINITY)) return INFINITY;               // no neighbour has been reached yet
    float u = h0 * s;
    const float d1 = a1 - a0;                            // +inf where that axis has no finite neighbour
    if (u <= d1) return a0 + u;
    // Bq^2 - A Cq in the equivalent form A s^2 - sum_{i<j} w_i w_j (delta_i - delta_j)^2: the literal form subtracts two numbers
    // of size (w delta)^2 to get one of size w s^2 and loses log2 of their ratio in bits once hz << h
    const float ss = s * s;
    float A = w0 + w1;
    u = (w1 * d1 + sqrtf(fmaxf(A * ss - (w0 * w1) * (d1 * d1), 0.f))) / A;
    const float d2 = a2 - a0;
    if (u <= d2) return a0 + u;
    const float d21 = d2 - d1;
    A = A + w2;
    const float cross = ((w0 * w1) * (d1 * d1) + (w0 * w2) * (d2 * d2)) + (w1 * w2) * (d21 * d21);
    u = ((w1 * d1 + w2 * d2) + sqrtf(fmaxf(A * ss - cross, 0.f))) / A;
    return a0 + u;
}

// One cell of the LDS tile (q points at it, plane d): T <- min(T, G(T)); true when it took a strictly smaller value.
__device__ __forceinline__ bool relax_cell(float* q, float s, int d, int D, float h, float hz, float wxy, float wz)
{
    if (!(s > 0.f && s < INFINITY)) return false;        // a wall keeps +inf
    const float ax = fminf(q[-1], q[1]), ay = fminf(q[-VOL_HALO], q[VOL_HALO]);
    const float below = d + 1 < D ? q[DEV_TCELLS] : INFINITY;
    float az = 0.f, hd = 0.5f * hz, wd = 4.f * wz;       // plane 0: the resist top, T = 0, half a step above
    if (d > 0) {
        az = fminf(q[-DEV_TCELLS], below);
        hd = hz;
        wd = wz;
    }
    const float v = godunov(ax, h, wxy, ay, h, wxy, az, hd, wd, s);
    if (v < *q) {
        *q = v;
        return true;
    }
    return false;
}

__global__ __launch_bounds__(256) void k_develop_time(const float* __restrict__ slow, const float* __restrict__ Tin,
                                                      float* __restrict__ Tout, int D, int n, float h, float hz, float wxy, float wz,
                                                      int* __restrict__ flag)
{
    extern __shared__ __attribute__((aligned(16))) float dev_lds[];
    float* Tl = dev_lds;                                 // [D][18][18]  tile + halo
    float* sl = dev_lds + D * DEV_TCELLS;                // [D][16][16]  tile
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * VOL_TILE, y0 = blockIdx.y * VOL_TILE;
    const size_t plane_elems = (size_t)n * n;
    const size_t vol = (size_t)blockIdx.z * D * plane_elems;
    const float inf = INFINITY, nan = __builtin_nanf("");
    for (int i = tid; i < D * DEV_TCELLS; i += 256) {
        const int d = i / DEV_TCELLS, r = i - d * DEV_TCELLS, ly = r / VOL_HALO, lx = r - ly * VOL_HALO;
        const int gy = y0 + ly - 1, gx = x0 + lx - 1;
        Tl[i] = (gy >= 0 && gy < n && gx >= 0 && gx < n) ? Tin[vol + (size_t)d * plane_elems + (size_t)gy * n + gx] : inf;
    }
    for (int i = tid; i < D * DEV_SCELLS; i += 256) {
        const int d = i / DEV_SCELLS, r = i - d * DEV_SCELLS, ly = r / VOL_TILE, lx = r - ly * VOL_TILE;
        const int gy = y0 + ly, gx = x0 + lx;
        sl[i] = (gy < n && gx < n) ? slow[vol + (size_t)d * plane_elems + (size_t)gy * n + gx] : nan;   // outside the grid: a wall
    }
    __syncthreads();
    // compute threads: 128, row = tid / 8, the columns of this phase's colour in that row
    const int row = (tid >> 3) & (VOL_TILE - 1), pair = tid & 7;
    bool changed = false;
    for (int round = 0; round < VOL_INNER; ++round) {
        for (int colour = 0; colour < 2; ++colour) {
            if (tid < 128) {
                const int col = 2 * pair + ((row + colour) & 1);
                float* Tc = Tl + (row + 1) * VOL_HALO + (col + 1);
                const float* sc = sl + row * VOL_TILE + col;
                for (int d = 0; d < D; ++d) changed |= relax_cell(Tc + d * DEV_TCELLS, sc[d * DEV_SCELLS], d, D, h, hz, wxy, wz);
                for (int d = D - 2; d >= 0; --d) changed |= relax_cell(Tc + d * DEV_TCELLS, sc[d * DEV_SCELLS], d, D, h, hz, wxy, wz);
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < D * DEV_SCELLS; i += 256) {
        const int d = i / DEV_SCELLS, r = i - d * DEV_SCELLS, ly = r / VOL_TILE, lx = r - ly * VOL_TILE;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy < n && gx < n) Tout[vol + (size_t)d * plane_elems + (size_t)gy * n + gx] = Tl[d * DEV_TCELLS + (ly + 1) * VOL_HALO + lx + 1];
    }
    if (changed) *flag = 1;
}

// ---- 4. developed depth: the first crossing of T = t going down a column, fp32
template <int VEC>
__global__ __launch_bounds__(256) void k_developed_depth(const float* __restrict__ T, float* __restrict__ out, int D, int n, float t,
                                                         float hz, float thickness)
{
    const long long plane_elems = (long long)n * n;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e >= plane_elems) return;
    const float* col = T + (size_t)blockIdx.y * D * plane_elems + e;
    Pack<VEC> z, prev;
    bool done[VEC];
    for (int v = 0; v < VEC; ++v) {
        z.v[v] = thickness;                              // every plane developed: cleared
        prev.v[v] = 0.f;
        done[v] = false;
    }
    for (int d = 0; d < D; ++d) {
        const Pack<VEC> cur = load_pack<VEC>(col + (size_t)d * plane_elems);
        for (int v = 0; v < VEC; ++v) {
            if (!done[v] && !(cur.v[v] <= t)) {
                done[v] = true;
                z.v[v] = d == 0 ? (0.5f * hz) * (t / cur.v[v])
                                : ((float)(d - 1) + 0.5f) * hz + hz * ((t - prev.v[v]) / (cur.v[v] - prev.v[v]));
            }
            prev.v[v] = cur.v[v];
        }
    }
    store_pack<VEC>(out + (size_t)blockIdx.y * plane_elems + e, z);
}

// taps of litho_postprocess_resist_diffused; false when R = ceil(4 sigma) > 32 or sigma is negative or not finite
static bool make_taps(double sigma_px, DevTaps& taps, int& R)
{
    memset(&taps, 0, sizeof(taps));
    R = 0;
    if (!(sigma_px >= 0.0) || !(sigma_px <= (double)DEV_RMAX / 4.0)) return false;
    if (sigma_px == 0.0) return true;
    R = (int)std::ceil(4.0 * sigma_px);
    if (R < 1 || R > DEV_RMAX) return false;
    double g[DEV_RMAX + 1], sum = 0.0;
    for (int k = 0; k <= R; ++k) {
        g[k] = std::exp(-(double)k * k / (2.0 * sigma_px * sigma_px));
        sum += k ? 2.0 * g[k] : g[k];
    }
    for (int k = 0; k <= R; ++k) taps.g[k] = (float)(g[k] / sum);
    return true;
}

}  // namespace litho

extern "C" {

int litho_latent_diffuse(const float* image, int B, int D, int n, double sigma_xy_px, double sigma_z_px, float* out, void* work,
                         size_t work_bytes, void* stream)
{
    using namespace litho;
    if (!image || !out || !volume_ok(B, D, n)) return LITHO_E_ARG;
    DevTaps txy, tz;
    int Rxy = 0, Rz = 0;
    if (!make_taps(sigma_xy_px, txy, Rxy) || !make_taps(sigma_z_px, tz, Rz)) return LITHO_E_ARG;
    const size_t bytes = (size_t)B * D * n * n * sizeof(float);
    if (!writes_clear({{out, bytes}}, {{image, bytes}})) return LITHO_E_ARG;
    const int passes = (Rxy ? 2 : 0) + (Rz ? 1 : 0);
    if (passes >= 2) {
        if (!work) return LITHO_E_ARG;
        if (work_bytes < bytes) return LITHO_E_WORKSPACE;
        if (!writes_clear({{work, bytes}, {out, bytes}}, {{image, bytes}})) return LITHO_E_ARG;   // a pass would read what it writes
    }
    hipStream_t st = (hipStream_t)stream;
    if (passes == 0) {                                   // the identity, bit for bit
        HIP_TRY(hipMemcpyAsync(out, image, bytes, hipMemcpyDeviceToDevice, st));
        return LITHO_OK;
    }
    const bool wide = (n & 3) == 0 && aligned16(image) && aligned16(out) && (passes < 2 || aligned16(work));
    // the last pass lands in `out`, the passes before it alternate between `work` and `out`
    const float* src = image;
    int left = passes;
    auto pass = [&](int axis, const DevTaps& taps, int R) {
        float* dst = (left & 1) ? out : (float*)work;
        LAUNCH_PACKED(k_latent_diffuse, wide && axis != 0, n, B * D, st, src, dst, D, n, axis, taps, R);
        src = dst;
        --left;
    };
    if (Rxy) {
        pass(0, txy, Rxy);
        pass(1, txy, Rxy);
    }
    if (Rz) pass(2, tz, Rz);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_develop_rate(const float* image, int volumes, int D, int n, const float* gains_host, int n_gains, double C, double r_max,
                       double r_min, double q, double m_th, double surface_rate, double surface_depth_nm, double thickness_nm,
                       float* slowness, void* stream)
{
    using namespace litho;
    VolGains gains;
    MackLaw law;
    if (!image || !slowness || !volume_ok(volumes, D, n) || !make_gains(gains_host, n_gains, volumes, D, gains) || !finite_pos(C) ||
        !make_mack(r_max, r_min, q, m_th, surface_rate, surface_depth_nm, thickness_nm, D, law))
        return LITHO_E_ARG;
    const int planes = volumes * D;
    const bool wide = (n & 3) == 0 && aligned16(image) && aligned16(slowness);
    LAUNCH_PACKED(k_develop_rate, wide, n, planes, (hipStream_t)stream, image, slowness, planes, D, n, gains, n_gains, C, law.rmax_a1,
                  law.rmin, law.q, law.a, law.surface);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

size_t litho_develop_work_bytes(int B, int D, int n, int max_iterations)
{
    using namespace litho;
    if (!volume_ok(B, D, n) || max_iterations < 1 || max_iterations > VOL_MAXIT) return 0;
    return flag_bytes(max_iterations) + (size_t)B * D * n * n * sizeof(float);
}

int litho_develop_time(const float* slowness, int B, int D, int n, double thickness_nm, double pixel_nm, int max_iterations,
                       float* T, void* work, size_t work_bytes, int* launches_host, void* stream)
{
    using namespace litho;
    if (launches_host) *launches_host = 0;
    if (!slowness || !T || !work || !launches_host || !volume_ok(B, D, n)) return LITHO_E_ARG;
    if (max_iterations < 1 || max_iterations > VOL_MAXIT || !finite_pos(thickness_nm) || !finite_pos(pixel_nm)) return LITHO_E_ARG;
    const size_t vol_bytes = (size_t)B * D * n * n * sizeof(float), need = litho_develop_work_bytes(B, D, n, max_iterations);
    if (!aligned16(work) || !writes_clear({{T, vol_bytes}}, {{slowness, vol_bytes}})) return LITHO_E_ARG;
    if (work_bytes < need) return LITHO_E_WORKSPACE;
    if (!writes_clear({{work, need}, {T, vol_bytes}}, {{slowness, vol_bytes}})) return LITHO_E_ARG;   // the second T buffer lives there
    FrontGeometry geo;
    if (!front_geometry(pixel_nm, thickness_nm, D, geo)) return LITHO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    int* flags = (int*)work;
    float* buf[2] = {T, (float*)((char*)work + flag_bytes(max_iterations))};
    const size_t cells = (size_t)B * D * n * n;
    const size_t lds = (size_t)D * (DEV_TCELLS + DEV_SCELLS) * sizeof(float);
    if (lds > 64 * 1024) {                               // once per device: the worst case, D = 32
        static unsigned lds_done = 0;
        HIP_TRY(lds_opt_in(lds_done, (const void*)k_develop_time, (size_t)VOL_DMAX * (DEV_TCELLS + DEV_SCELLS) * sizeof(float)));
    }
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)T, 0x7f800000, cells, st));                    // +inf everywhere
    const unsigned tiles = (unsigned)((n + VOL_TILE - 1) / VOL_TILE);
    const dim3 grid(tiles, tiles, (unsigned)B);
    // launch `it` reads buf[it & 1] and writes the other
    const int launches = iterate_until_unchanged(flags, max_iterations, st, [&](int it) {
        hipLaunchKernelGGL(k_develop_time, grid, dim3(256), lds, st, slowness, (const float*)buf[it & 1], buf[(it + 1) & 1], D, n, geo.h, geo.hz,
                           geo.wxy, geo.wz, flags + it);
    });
    if (launches < 0) return launches;
    *launches_host = launches ? launches : max_iterations;
    return launches ? LITHO_OK : LITHO_E_NOCONV;
}

int litho_developed_depth(const float* T, int B, int D, int n, double thickness_nm, double develop_time_s, float* depth, void* stream)
{
    using namespace litho;
    if (!T || !depth || !volume_ok(B, D, n) || !finite_pos(thickness_nm) || !(develop_time_s >= 0.0) || std::isinf(develop_time_s))
        return LITHO_E_ARG;
    const float thickness = (float)thickness_nm, hz = (float)(thickness_nm / D);
    if (!(hz > 0.f) || std::isinf(thickness)) return LITHO_E_ARG;
    const bool wide = (n & 3) == 0 && aligned16(T) && aligned16(depth);
    LAUNCH_PACKED(k_developed_depth, wide, n, B, (hipStream_t)stream, T, depth, D, n, (float)develop_time_s, hz, thickness);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

}  // extern "C"
