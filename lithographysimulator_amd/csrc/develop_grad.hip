// develop_grad.hip -- gradients through resist development, behind litho_develop_time_vjp and litho_develop_rate_vjp (no
// reference counterpart; the definitions are in include/litho_abbe.h, "Gradients through development"; the checker is their
// float64 restatement tests/develop_grad_oracle.py).  Built with -ffp-contract=off (Makefile): every fp32 result is a fixed
// sequence of single operations.
//
// The arrival time T of develop.hip is the fixed point T_i = G_i(T_N(i), s_i) of the Godunov update.  For a reached cell that is
// no wall, sum_j w_j (T_i - a_j)^2 = s_i^2 over the axes the update used, and with P_i = sum_j w_j (T_i - a_j)
//   dT_i / da_j = alpha_ij = w_j (T_i - a_j) / P_i   (non-negative, summing to 1),     dT_i / ds_i = sigma_i = s_i / P_i.
// For a cotangent g = dl/dT the adjoint variable solves lambda_i = g_i + sum_j alpha_ji lambda_j over the neighbours j whose
// update took i as the upwind cell of its axis, and dl/ds_i = lambda_i sigma_i.  Four kernels:
//   k_develop_links     per cell, in double, rounded once: the branch of the update, its three link weights and sigma
//   k_develop_time_vjp  the tiled gather iteration for lambda (below)
//   k_develop_scale     grad_s = lambda sigma, exactly 0 where the cell has no gradient
//   k_develop_rate_vjp  the rate law of k_develop_rate / k_peb_rate backwards, double per cell, the gains summed inside
// and behind litho_develop_rate_vjp_params k_develop_rate_params, the rate law's six parameter sums per gained plane (section 5);
// behind litho_develop_rate_jvp and litho_develop_time_jvp k_develop_rate_jvp and k_develop_time_jvp, forward mode (section 6).  The
// three rate kernels share rate_cell and rate_derivatives, the two solver entries front_derivative (section 7), the two host
// chains of the rate law rate_chain (section 8).
// The pointwise kernels move four consecutive x per thread (16-byte accesses) when n is a multiple of 4 and the pointers are
// 16-byte aligned, one otherwise.  The limits, the packs, the host predicates, the gains, the rate law (mack_slowness_dx, next to
// the forward's mack_slowness), the solvers' geometry and host loop are resist_volume.hpp's, shared with develop.hip and peb.hip.
//
// Links.  Four fp32 per cell, (lx, ly, lz, sigma).  |l| is alpha on that axis; the sign carries the direction: positive when the
// upwind cell is the lower-index neighbour (a tie of the two neighbours goes there), negative when it is the higher-index one.
// A weight is 0 when the axis was not used, when the upwind "cell" is the resist top (plane 0's z axis) and when the upwind
// cell's stored T is not strictly below the cell's own stored T: the links then point strictly down in T, the dependency graph
// is acyclic and the iteration below is nilpotent.  sigma = 0 marks a cell with no gradient (a wall, or T = +inf): all of its
// weights are 0, nothing gathers from it and it gathers from nothing.
//
// k_develop_time_vjp.  The decomposition of k_develop_time: a workgroup owns a 16 x 16 lateral tile with all D planes.  In LDS:
// lambda, lx and ly of tile + one-cell halo as [D][18][18] (of a halo cell only lambda and the one link that points into the
// tile are loaded and read; the corners are never touched) and lz of the tile as [D][16][16]: D (3 . 324 + 256) floats = 4912 B
// per plane, 38.4 KiB at D = 8 (four workgroups per CU), 76.8 KiB at D = 16 (two), 153.5 KiB at D = 32 (one).  The cotangent g
// is read from global memory by the thread that owns the column: keeping it in LDS as well (5936 B per plane, possible up to
// D = 27) costs a workgroup per CU at D = 8 and at D = 16 and was slower in a same-box A/B at 2048^2, 2.80 against 2.31 ms per
// launch at D = 8 and 16.3 against 9.0 at D = 16 (LABNOTES).  A round is two phases, the columns with (row + col) even, a barrier, the odd ones,
// a barrier; in a phase 128 threads own one column each and sweep it up and then down (Gauss-Seidel along z: the front mostly
// ran downwards, so lambda flows upwards).  A cell's update is a pure gather,
//   lambda_i = g_i (+) w lambda_j  over x-, x+, y-, y+, z-, z+ in this order, a term only where the neighbour's link points at i,
// each term one fp32 multiplication and one addition.  The lateral neighbours of a column have the other colour and are not
// written in that phase; halo cells are read-only: no race, no atomics.  Launches ping-pong lambda between two global buffers,
// so no workgroup reads what another writes.  A cell "changed" when the new value's bit pattern differs from the old one (never
// `!=`, which does not settle on a NaN); a thread that changed one stores 1 into the launch's own flag word with a plain store.
// The host reads the flag words every VOL_CHECK launches and stops at the first launch that changed nothing.  Every loop has a
// trip count fixed by D; the launch count is capped by the caller.
//
// Determinism.  Each cell's final value is the fixed expression above on the final values of cells with strictly larger T.  By
// induction from the sinks of the graph the bits depend on neither the tile schedule, nor the batch, nor the start value, nor
// the launch at which the iteration stops.
#include "resist_volume.hpp"

namespace litho {

static constexpr int DG_HCELLS = VOL_HALO * VOL_HALO, DG_TCELLS = VOL_TILE * VOL_TILE;
static constexpr size_t DG_PLANE_BYTES = (size_t)(3 * DG_HCELLS + DG_TCELLS) * sizeof(float);
static_assert((size_t)VOL_DMAX * DG_PLANE_BYTES <= 160 * 1024, "the tile of the deepest volume must fit a gfx950 workgroup's LDS");

// ---- 1. the links of one cell.  s, Ti: the cell's slowness and stored T; (xm, xp), (ym, yp), (zm, zp): the stored T of the two
// neighbours per axis, +inf where there is none; top: plane 0, whose z axis is the resist top (a = 0 at hz / 2).  The branch and
// T_i are recomputed from these as godunov (develop.hip) decides -- sorted axes, u <= d1, u <= d2 -- in double.
__device__ __forceinline__ float4 link_cell(float s, float Ti, float xm, float xp, float ym, float yp, float zm, float zp, bool top,
                                            double h, double hz)
{
    const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!(s > 0.f && s < INFINITY) || !(Ti < INFINITY)) return none;      // a wall, or never reached
    const bool xlo = xm <= xp, ylo = ym <= yp, zlo = zm <= zp;            // a tie goes to the lower-index neighbour
    const float ux = xlo ? xm : xp, uy = ylo ? ym : yp, uz = zlo ? zm : zp;
    double a0 = ux, a1 = uy, a2 = top ? 0.0 : (double)uz;
    double h0 = h, h1 = h, h2 = top ? 0.5 * hz : hz;
    int k0 = 0, k1 = 1, k2 = 2;
    double t;
    int ti;
#define DG_SWAP(i, j)                                                                          \
    if (a##i > a##j) {                                                                         \
        t = a##i; a##i = a##j; a##j = t; t = h##i; h##i = h##j; h##j = t; ti = k##i; k##i = k##j; k##j = ti; \
    }
    DG_SWAP(0, 1)
    DG_SWAP(1, 2)
    DG_SWAP(0, 1)
#undef DG_SWAP
    if (!(a0 < (double)INFINITY)) return none;
    const double w0 = 1.0 / (h0 * h0), w1 = 1.0 / (h1 * h1), w2 = 1.0 / (h2 * h2);
    const double sd = s, ss = sd * sd;
    double u = h0 * sd, p0, p1 = 0.0, p2 = 0.0;
    const double d1 = a1 - a0;                           // +inf where that axis has no finite neighbour
    if (!(u <= d1)) {
        double A = w0 + w1;
        u = (w1 * d1 + sqrt(fmax(A * ss - (w0 * w1) * (d1 * d1), 0.0))) / A;
        const double d2 = a2 - a0;
        if (!(u <= d2)) {
            const double d21 = d2 - d1;
            A = A + w2;
            const double cross = ((w0 * w1) * (d1 * d1) + (w0 * w2) * (d2 * d2)) + (w1 * w2) * (d21 * d21);
            u = ((w1 * d1 + w2 * d2) + sqrt(fmax(A * ss - cross, 0.0))) / A;
            p2 = w2 * (u - d2);
        }
        p1 = w1 * (u - d1);
    }
    p0 = w0 * u;
    const double P = (p0 + p1) + p2;
    if (!(P > 0.0)) return none;                         // cannot happen for a positive finite s; never divide by 0
    const double al0 = p0 / P, al1 = p1 / P, al2 = p2 / P;
    const double ax = k0 == 0 ? al0 : (k1 == 0 ? al1 : al2);
    const double ay = k0 == 1 ? al0 : (k1 == 1 ? al1 : al2);
    const double az = k0 == 2 ? al0 : (k1 == 2 ? al1 : al2);
    float4 out;
    // strict upwind: a link counts only where the upwind cell's stored T is below the cell's own
    out.x = (ux < Ti) ? (float)(xlo ? ax : -ax) : 0.f;
    out.y = (uy < Ti) ? (float)(ylo ? ay : -ay) : 0.f;
    out.z = (!top && uz < Ti) ? (float)(zlo ? az : -az) : 0.f;
    out.w = (float)(sd / P);
    return out;
}

// grid.x covers the n^2 / VEC packs of a plane, grid.y the B D planes
template <int VEC>
__global__ __launch_bounds__(256) void k_develop_links(const float* __restrict__ slow, const float* __restrict__ T,
                                                       float4* __restrict__ links, int D, int n, double h, double hz)
{
    const long long plane_elems = (long long)n * n;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e >= plane_elems) return;
    const int p = blockIdx.y, d = p % D;
    const int row = (int)(e / n), col = (int)(e % n);
    const size_t at = (size_t)p * plane_elems + e;
    const float inf = INFINITY;
    const Pack<VEC> s = load_pack<VEC>(slow + at), c = load_pack<VEC>(T + at);
    const Pack<VEC> ym = row > 0 ? load_pack<VEC>(T + at - n) : fill_pack<VEC>(inf);
    const Pack<VEC> yp = row + 1 < n ? load_pack<VEC>(T + at + n) : fill_pack<VEC>(inf);
    const Pack<VEC> zm = d > 0 ? load_pack<VEC>(T + at - plane_elems) : fill_pack<VEC>(inf);
    const Pack<VEC> zp = d + 1 < D ? load_pack<VEC>(T + at + plane_elems) : fill_pack<VEC>(inf);
    const float left = col > 0 ? T[at - 1] : inf, right = col + VEC < n ? T[at + VEC] : inf;
    for (int v = 0; v < VEC; ++v) {
        const float xm = v > 0 ? c.v[v - 1] : left, xp = v + 1 < VEC ? c.v[v + 1] : right;
        links[at + v] = link_cell(s.v[v], c.v[v], xm, xp, ym.v[v], yp.v[v], zm.v[v], zp.v[v], d == 0, h, hz);
    }
}

// ---- 2. the gather iteration
__device__ __forceinline__ unsigned bits_of(float x) { return __float_as_uint(x); }

// One cell: lam/lx/ly point at it in the [18][18] planes, lz in the [16][16] planes; true when its bits changed.
__device__ __forceinline__ bool gather_cell(float* lam, const float* lx, const float* ly, const float* lz, float g, int d, int D)
{
    float acc = g, w;
    w = lx[-1];
    if (w < 0.f) acc = acc + (-w) * lam[-1];
    w = lx[1];
    if (w > 0.f) acc = acc + w * lam[1];
    w = ly[-VOL_HALO];
    if (w < 0.f) acc = acc + (-w) * lam[-VOL_HALO];
    w = ly[VOL_HALO];
    if (w > 0.f) acc = acc + w * lam[VOL_HALO];
    if (d > 0) {
        w = lz[-DG_TCELLS];
        if (w < 0.f) acc = acc + (-w) * lam[-DG_HCELLS];
    }
    if (d + 1 < D) {
        w = lz[DG_TCELLS];
        if (w > 0.f) acc = acc + w * lam[DG_HCELLS];
    }
    const bool changed = bits_of(acc) != bits_of(*lam);
    *lam = acc;
    return changed;
}

__global__ __launch_bounds__(256) void k_develop_time_vjp(const float* __restrict__ links, const float* __restrict__ g,
                                                          const float* __restrict__ lin, float* __restrict__ lout, int D, int n,
                                                          int* __restrict__ flag)
{
    extern __shared__ __attribute__((aligned(16))) float dg_lds[];
    float* lam = dg_lds;                                 // [D][18][18]  tile + halo
    float* lx = lam + D * DG_HCELLS;                     // [D][18][18]
    float* ly = lx + D * DG_HCELLS;                      // [D][18][18]
    float* lz = ly + D * DG_HCELLS;                      // [D][16][16]  tile
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * VOL_TILE, y0 = blockIdx.y * VOL_TILE;
    const size_t plane_elems = (size_t)n * n;
    const size_t vol = (size_t)blockIdx.z * D * plane_elems;
    // the tile: all three links and lambda; a tile cell outside the grid has no links and lambda 0
    for (int i = tid; i < D * DG_TCELLS; i += 256) {
        const int d = i / DG_TCELLS, r = i - d * DG_TCELLS, ty = r / VOL_TILE, tx = r - ty * VOL_TILE;
        const int gy = y0 + ty, gx = x0 + tx;
        const int q = d * DG_HCELLS + (ty + 1) * VOL_HALO + tx + 1;
        float4 L = make_float4(0.f, 0.f, 0.f, 0.f);
        float l0 = 0.f;
        if (gy < n && gx < n) {
            const size_t cell = vol + (size_t)d * plane_elems + (size_t)gy * n + gx;
            L = *reinterpret_cast<const float4*>(links + 4 * cell);
            l0 = lin[cell];
        }
        lam[q] = l0;
        lx[q] = L.x;
        ly[q] = L.y;
        lz[i] = L.z;
    }
    // the 64 edge cells of the halo per plane: lambda and the one link that can point into the tile
    for (int i = tid; i < D * 4 * VOL_TILE; i += 256) {
        const int d = i / (4 * VOL_TILE), r = i - d * (4 * VOL_TILE), side = r / VOL_TILE, k = r - side * VOL_TILE;
        int hy, hx;                                      // position in the [18][18] plane
        if (side == 0) { hy = k + 1; hx = 0; }
        else if (side == 1) { hy = k + 1; hx = VOL_HALO - 1; }
        else if (side == 2) { hy = 0; hx = k + 1; }
        else { hy = VOL_HALO - 1; hx = k + 1; }
        const int gy = y0 + hy - 1, gx = x0 + hx - 1;
        float l0 = 0.f, w = 0.f;
        if (gy >= 0 && gy < n && gx >= 0 && gx < n) {
            const size_t cell = vol + (size_t)d * plane_elems + (size_t)gy * n + gx;
            l0 = lin[cell];
            w = links[4 * cell + (side < 2 ? 0 : 1)];
        }
        const int q = d * DG_HCELLS + hy * VOL_HALO + hx;
        lam[q] = l0;
        if (side < 2) lx[q] = w;
        else ly[q] = w;
    }
    __syncthreads();
    // compute threads: 128, row = tid / 8, the columns of this phase's colour in that row
    const int row = (tid >> 3) & (VOL_TILE - 1), pair = tid & 7;
    bool changed = false;
    for (int round = 0; round < VOL_INNER; ++round) {
        for (int colour = 0; colour < 2; ++colour) {
            const int col = 2 * pair + ((row + colour) & 1);
            if (tid < 128 && y0 + row < n && x0 + col < n) {
                const int q = (row + 1) * VOL_HALO + (col + 1), t = row * VOL_TILE + col;
                const float* gc = g + vol + (size_t)(y0 + row) * n + (x0 + col);     // the column's cotangent, from global memory
                for (int d = D - 1; d >= 0; --d)
                    changed |= gather_cell(lam + d * DG_HCELLS + q, lx + d * DG_HCELLS + q, ly + d * DG_HCELLS + q,
                                           lz + d * DG_TCELLS + t, gc[d * plane_elems], d, D);
                for (int d = 1; d < D; ++d)
                    changed |= gather_cell(lam + d * DG_HCELLS + q, lx + d * DG_HCELLS + q, ly + d * DG_HCELLS + q,
                                           lz + d * DG_TCELLS + t, gc[d * plane_elems], d, D);
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < D * DG_TCELLS; i += 256) {
        const int d = i / DG_TCELLS, r = i - d * DG_TCELLS, ty = r / VOL_TILE, tx = r - ty * VOL_TILE;
        const int gy = y0 + ty, gx = x0 + tx;
        if (gy < n && gx < n)
            lout[vol + (size_t)d * plane_elems + (size_t)gy * n + gx] = lam[d * DG_HCELLS + (ty + 1) * VOL_HALO + tx + 1];
    }
    if (changed) *flag = 1;
}

// ---- 3. grad_s = lambda sigma; a cell with no gradient (sigma = 0) gets exactly 0 whatever its cotangent held
template <int VEC>
__global__ __launch_bounds__(256) void k_develop_scale(const float* __restrict__ lambda, const float* __restrict__ links,
                                                       float* __restrict__ out, int n)
{
    const long long plane_elems = (long long)n * n;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e >= plane_elems) return;
    const size_t at = (size_t)blockIdx.y * plane_elems + e;
    const Pack<VEC> l = load_pack<VEC>(lambda + at);
    Pack<VEC> r;
    for (int v = 0; v < VEC; ++v) {
        const float sigma = links[4 * (at + v) + 3];
        r.v[v] = sigma > 0.f ? l.v[v] * sigma : 0.f;
    }
    store_pack<VEC>(out + at, r);
}

// ---- 4. the rate law backwards.  A cell of the rate law under the gain g: m = exp(-(kappa g) x) and b = 1 - m, the dissolved
// fraction; a wall where b is negative or NaN.
struct RateCell { double m, b; bool wall; };
__device__ __forceinline__ RateCell rate_cell(double kg, double x)
{
    const double m = exp(-(kg * x)), b = 1.0 - m;
    return RateCell{m, b, !(b >= 0.0)};
}
// The six derivatives of the slowness of a cell that is no wall: d[0] = ds/dkappa (mack_slowness_dx with db/dkappa = (g x) m) and
// d[1 .. 5] = mack_slowness_dparams' five (resist_volume.hpp), what the parameter sums and the tangent both take.
__device__ __forceinline__ void rate_derivatives(const RateCell& c, double g, double x, double rmax_a1, double rmin, double q, double a, double f,
                                                 double (&d)[6])
{
    double five[5];
    mack_slowness_dparams(c.b, rmax_a1, rmin, q, a, f, five);
    d[0] = mack_slowness_dx(c.b, (g * x) * c.m, rmax_a1, rmin, q, a, f);
    for (int j = 0; j < 5; ++j) d[1 + j] = five[j];
}

// k_develop_rate_vjp: db/dx = (kappa g) m, ds/dx from mack_slowness_dx, summed over the gains.  A wall contributes 0.
template <int VEC>
__global__ __launch_bounds__(256) void k_develop_rate_vjp(const float* __restrict__ x, const float* __restrict__ grad_s,
                                                          float* __restrict__ grad_x, int planes, int D, int n, const VolGains gains,
                                                          int n_gains, double kappa, double rmax_a1, double rmin, double q, double a,
                                                          const VolSurface surface)
{
    const long long plane_elems = (long long)n * n;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e >= plane_elems) return;
    const int p = blockIdx.y;
    const double f = surface.f[p % D];
    const size_t at = (size_t)p * plane_elems + e;
    const Pack<VEC> xv = load_pack<VEC>(x + at);
    double acc[VEC];
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0;
    for (int gi = 0; gi < n_gains; ++gi) {
        const double kg = kappa * (double)gains.g[gi];
        const Pack<VEC> gs = load_pack<VEC>(grad_s + ((size_t)gi * planes + p) * plane_elems + e);
        for (int v = 0; v < VEC; ++v) {
            const RateCell c = rate_cell(kg, (double)xv.v[v]);
            if (c.wall) continue;
            acc[v] += (double)gs.v[v] * mack_slowness_dx(c.b, kg * c.m, rmax_a1, rmin, q, a, f);
        }
    }
    Pack<VEC> out;
    for (int v = 0; v < VEC; ++v) out.v[v] = (float)acc[v];
    store_pack<VEC>(grad_x + at, out);
}

// ---- 5. the rate law's parameter sums (litho_develop_rate_vjp_params): per cell of a gained plane the six products of the
// cotangent with rate_derivatives' six, in double; a wall contributes 0.  A workgroup adds its terms in vol_block_sum's fixed tree and writes them to its own slot
// partials[gained plane][workgroup][6]; k_vol_total adds the slots of a gained plane.  grid.y: the n_gains x planes gained planes.
__global__ __launch_bounds__(256) void k_develop_rate_params(const float* __restrict__ x, const float* __restrict__ grad_s,
                                                             double* __restrict__ partials, int planes, int D, int n,
                                                             const VolGains gains, double kappa, double rmax_a1, double rmin, double q,
                                                             double a, const VolSurface surface)
{
    __shared__ double lds[4][6];
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const long long plane_elems = (long long)n * n;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int gp = blockIdx.y, gi = gp / planes, p = gp - gi * planes;
    if (e < plane_elems) {
        const double f = surface.f[p % D], g = (double)gains.g[gi], kg = kappa * g;
        const double xv = x[(size_t)p * plane_elems + e], gs = grad_s[(size_t)gp * plane_elems + e];
        const RateCell c = rate_cell(kg, xv);
        if (!c.wall) {
            double d[6];
            rate_derivatives(c, g, xv, rmax_a1, rmin, q, a, f, d);
            for (int j = 0; j < 6; ++j) t[j] = gs * d[j];
        }
    }
    vol_block_sum<6>(t, lds);
    if (threadIdx.x == 0) {
        double* slot = partials + ((size_t)gp * gridDim.x + blockIdx.x) * 6;
        for (int j = 0; j < 6; ++j) slot[j] = t[j];
    }
}

// ---- 6. forward mode (litho_develop_rate_jvp, litho_develop_time_jvp; include/litho_abbe.h's "Forward mode (tangents) of the
// resist chain").
//
// The rate law's tangent: ds = ds/dx (kappa g) m dx_p + sum_j d_j dphi[p][plane][j], j = 0 .. 5 in this order, d_0 the line of
// rate_derivatives' d[0] and d_1 .. d_5 its other five; double per cell, rounded once; a wall gives exactly 0.
// grid.y: the planes of x; the directions and the gains in loops inside.  dx == nullptr: dx = 0.
template <int VEC>
__global__ __launch_bounds__(256) void k_develop_rate_jvp(const float* __restrict__ x, const float* __restrict__ dx,
                                                          const double* __restrict__ dphi, float* __restrict__ out, int planes, int D,
                                                          int n, const VolGains gains, int n_gains, int P, double kappa, double rmax_a1,
                                                          double rmin, double q, double a, const VolSurface surface)
{
    const long long plane_elems = (long long)n * n;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e >= plane_elems) return;
    const int p = blockIdx.y, d = p % D;
    const double f = surface.f[d];
    const Pack<VEC> xv = load_pack<VEC>(x + (size_t)p * plane_elems + e);
    for (int gi = 0; gi < n_gains; ++gi) {
        const double g = (double)gains.g[gi], kg = kappa * g;
        RateCell c[VEC];
        double dj[VEC][6];
        for (int v = 0; v < VEC; ++v) {
            c[v] = rate_cell(kg, (double)xv.v[v]);
            if (!c[v].wall) rate_derivatives(c[v], g, (double)xv.v[v], rmax_a1, rmin, q, a, f, dj[v]);
        }
        for (int k = 0; k < P; ++k) {
            const Pack<VEC> dxv = dx ? load_pack<VEC>(dx + ((size_t)k * planes + p) * plane_elems + e) : fill_pack<VEC>(0.f);
            const double* phi = dphi + ((size_t)k * D + d) * 6;
            Pack<VEC> r;
            for (int v = 0; v < VEC; ++v) {
                if (c[v].wall) {
                    r.v[v] = 0.f;
                    continue;
                }
                double acc = mack_slowness_dx(c[v].b, (kg * c[v].m) * (double)dxv.v[v], rmax_a1, rmin, q, a, f);
                for (int j = 0; j < 6; ++j) acc = acc + dj[v][j] * phi[j];
                r.v[v] = (float)acc;
            }
            store_pack<VEC>(out + (((size_t)k * n_gains + gi) * planes + p) * plane_elems + e, r);
        }
    }
}

// The front's tangent, the transpose of k_develop_time_vjp on the same tiling: a cell gathers along its OWN links from its upwind
// cells, so only tau needs the one-cell halo in LDS and the links of the tile alone are kept: tau [D][18][18] and lx, ly, lz
// [D][16][16], D (324 + 768) floats = 4368 D bytes, 136.5 KiB at D = 32.  The source sigma ds of a cell is read from global memory
// by the thread that owns the column (as the adjoint reads its cotangent).  grid.z: the P B volumes, direction-major; the links
// belong to volume blockIdx.z % B.  A column is swept down and then up: the tangent flows the way the front ran.
static constexpr size_t DT_PLANE_BYTES = (size_t)(DG_HCELLS + 3 * DG_TCELLS) * sizeof(float);
static_assert((size_t)VOL_DMAX * DT_PLANE_BYTES <= 160 * 1024, "the tile of the deepest volume must fit a gfx950 workgroup's LDS");

// One cell: tau points at it in the [18][18] planes, (lx, ly, lz) are its own links; true when its bits changed.
__device__ __forceinline__ bool tangent_cell(float* tau, float lx, float ly, float lz, float src, int d, int D)
{
    float acc = src;
    if (lx > 0.f) acc = acc + lx * tau[-1];
    else if (lx < 0.f) acc = acc + (-lx) * tau[1];
    if (ly > 0.f) acc = acc + ly * tau[-VOL_HALO];
    else if (ly < 0.f) acc = acc + (-ly) * tau[VOL_HALO];
    if (lz > 0.f && d > 0) acc = acc + lz * tau[-DG_HCELLS];
    else if (lz < 0.f && d + 1 < D) acc = acc + (-lz) * tau[DG_HCELLS];
    const bool changed = bits_of(acc) != bits_of(*tau);
    *tau = acc;
    return changed;
}

__global__ __launch_bounds__(256) void k_develop_time_jvp(const float* __restrict__ links, const float* __restrict__ ds,
                                                          const float* __restrict__ tin, float* __restrict__ tout, int B, int D, int n,
                                                          int* __restrict__ flag)
{
    extern __shared__ __attribute__((aligned(16))) float dt_lds[];
    float* tau = dt_lds;                                 // [D][18][18]  tile + halo
    float* lx = tau + D * DG_HCELLS;                     // [D][16][16]  tile
    float* ly = lx + D * DG_TCELLS;
    float* lz = ly + D * DG_TCELLS;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * VOL_TILE, y0 = blockIdx.y * VOL_TILE;
    const size_t plane_elems = (size_t)n * n;
    const size_t vol = (size_t)blockIdx.z * D * plane_elems;                 // in the direction-major tangent volumes
    const size_t lvol = (size_t)(blockIdx.z % B) * D * plane_elems;          // in the links
    // the tile: its links and tau; a tile cell outside the grid has no links and tau 0
    for (int i = tid; i < D * DG_TCELLS; i += 256) {
        const int d = i / DG_TCELLS, r = i - d * DG_TCELLS, ty = r / VOL_TILE, tx = r - ty * VOL_TILE;
        const int gy = y0 + ty, gx = x0 + tx;
        float4 L = make_float4(0.f, 0.f, 0.f, 0.f);
        float t0 = 0.f;
        if (gy < n && gx < n) {
            const size_t cell = (size_t)d * plane_elems + (size_t)gy * n + gx;
            L = *reinterpret_cast<const float4*>(links + 4 * (lvol + cell));
            t0 = tin[vol + cell];
        }
        tau[d * DG_HCELLS + (ty + 1) * VOL_HALO + tx + 1] = t0;
        lx[i] = L.x;
        ly[i] = L.y;
        lz[i] = L.z;
    }
    // the 64 edge cells of the halo per plane: tau alone
    for (int i = tid; i < D * 4 * VOL_TILE; i += 256) {
        const int d = i / (4 * VOL_TILE), r = i - d * (4 * VOL_TILE), side = r / VOL_TILE, k = r - side * VOL_TILE;
        int hy, hx;                                      // position in the [18][18] plane
        if (side == 0) { hy = k + 1; hx = 0; }
        else if (side == 1) { hy = k + 1; hx = VOL_HALO - 1; }
        else if (side == 2) { hy = 0; hx = k + 1; }
        else { hy = VOL_HALO - 1; hx = k + 1; }
        const int gy = y0 + hy - 1, gx = x0 + hx - 1;
        float t0 = 0.f;
        if (gy >= 0 && gy < n && gx >= 0 && gx < n) t0 = tin[vol + (size_t)d * plane_elems + (size_t)gy * n + gx];
        tau[d * DG_HCELLS + hy * VOL_HALO + hx] = t0;
    }
    __syncthreads();
    // compute threads: 128, row = tid / 8, the columns of this phase's colour in that row
    const int row = (tid >> 3) & (VOL_TILE - 1), pair = tid & 7;
    bool changed = false;
    for (int round = 0; round < VOL_INNER; ++round) {
        for (int colour = 0; colour < 2; ++colour) {
            const int col = 2 * pair + ((row + colour) & 1);
            if (tid < 128 && y0 + row < n && x0 + col < n) {
                const int q = (row + 1) * VOL_HALO + (col + 1), t = row * VOL_TILE + col;
                const size_t column = (size_t)(y0 + row) * n + (x0 + col);
                const float* sc = ds + vol + column;                         // the column's ds and sigma, from global memory
                const float* gc = links + 4 * (lvol + column) + 3;
                auto cell = [&](int d) {
                    const float sigma = gc[4 * d * plane_elems];
                    const float src = sigma > 0.f ? sigma * sc[d * plane_elems] : 0.f;
                    const int l = d * DG_TCELLS + t;
                    return tangent_cell(tau + d * DG_HCELLS + q, lx[l], ly[l], lz[l], src, d, D);
                };
                for (int d = 0; d < D; ++d) changed |= cell(d);
                for (int d = D - 2; d >= 0; --d) changed |= cell(d);
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < D * DG_TCELLS; i += 256) {
        const int d = i / DG_TCELLS, r = i - d * DG_TCELLS, ty = r / VOL_TILE, tx = r - ty * VOL_TILE;
        const int gy = y0 + ty, gx = x0 + tx;
        if (gy < n && gx < n)
            tout[vol + (size_t)d * plane_elems + (size_t)gy * n + gx] = tau[d * DG_HCELLS + (ty + 1) * VOL_HALO + tx + 1];
    }
    if (changed) *flag = 1;
}

// ---- 7. what litho_develop_time_vjp (P = 1) and litho_develop_time_jvp share: the checks in their order (the output over an
// input is reported before the workspace's size), the workspace (flags | links | one buffer of P volumes), the LDS opt-in of
// `kernel` (lds_done: the caller's once-per-device word, one per kernel), the links, the iteration of launch(...) on a grid P B
// deep and the launch count.  `source`: the cotangent, or the P directions of the slowness; `out`: P volumes, the second buffer of
// the ping-pong.  scale: k_develop_scale from the workspace's buffer into `out` closes the call.
template <class Launch>
static int front_derivative(const float* slowness, const float* T, const float* source, int B, int D, int n, int P, double thickness_nm,
                            double pixel_nm, int max_iterations, float* out, void* work, size_t work_bytes, int* launches_host, void* stream,
                            bool wide, const void* kernel, unsigned& lds_done, size_t lds_plane_bytes, bool scale, Launch launch)
{
    if (launches_host) *launches_host = 0;
    if (!slowness || !T || !source || !out || !work || !launches_host || !volume_ok(B, D, n)) return LITHO_E_ARG;
    if (P < 1 || P > LITHO_TANGENT_MAX || (long long)P * B * D > 65535) return LITHO_E_ARG;
    if (max_iterations < 1 || max_iterations > VOL_MAXIT || !finite_pos(thickness_nm) || !finite_pos(pixel_nm)) return LITHO_E_ARG;
    const size_t cells = (size_t)B * D * n * n, vol_bytes = cells * sizeof(float), tan_bytes = vol_bytes * P;
    const size_t need = flag_bytes(max_iterations) + 4 * vol_bytes + tan_bytes;
    if (!aligned16(work)) return LITHO_E_ARG;
    if (!writes_clear({{out, tan_bytes}}, {{slowness, vol_bytes}, {T, vol_bytes}, {source, tan_bytes}})) return LITHO_E_ARG;
    if (work_bytes < need) return LITHO_E_WORKSPACE;
    if (!writes_clear({{work, need}, {out, tan_bytes}}, {{slowness, vol_bytes}, {T, vol_bytes}, {source, tan_bytes}})) return LITHO_E_ARG;
    FrontGeometry geo;
    if (!front_geometry(pixel_nm, thickness_nm, D, geo)) return LITHO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    int* flags = (int*)work;
    float* links = (float*)((char*)work + flag_bytes(max_iterations));
    float* buf[2] = {links + 4 * cells, out};
    const size_t lds = (size_t)D * lds_plane_bytes;
    if (lds > 64 * 1024) HIP_TRY(lds_opt_in(lds_done, kernel, (size_t)VOL_DMAX * lds_plane_bytes));     // once per device: the worst case, D = 32
    HIP_TRY(hipMemsetAsync(buf[0], 0, tan_bytes, st));
    LAUNCH_PACKED(k_develop_links, wide, n, B * D, st, slowness, T, (float4*)links, D, n, (double)geo.h, (double)geo.hz);
    HIP_TRY(hipGetLastError());
    const unsigned tiles = (unsigned)((n + VOL_TILE - 1) / VOL_TILE);
    const dim3 grid(tiles, tiles, (unsigned)(P * B));
    // launch `it` reads buf[it & 1] and writes the other
    const int launches = iterate_until_unchanged(flags, max_iterations, st, [&](int it) {
        launch(grid, lds, st, (const float*)links, (const float*)buf[it & 1], buf[(it + 1) & 1], flags + it);
    });
    if (launches < 0) return launches;
    *launches_host = launches ? launches : max_iterations;
    if (!launches) return LITHO_E_NOCONV;
    if (scale) {                                         // both buffers hold the fixed point: read the workspace's, write the output
        LAUNCH_PACKED(k_develop_scale, wide, n, B * D, st, (const float*)buf[0], (const float*)links, out, n);
        HIP_TRY(hipGetLastError());
    }
    return LITHO_OK;
}

// ---- 8. the coefficients of the chain from the rate law's seven physical numbers to the kernels' six slots, whose two products
// are litho_develop_rate_param_chain and _param_tangent: a and its two derivatives, and per plane ez = df_d/dr0 and ddelta =
// df_d/d delta of f_d = 1 - (1 - r0) exp(-z_d / delta).  False when D or a parameter is outside its domain (make_mack's).
struct RateChain { double a, da_dq, da_dm, ez[VOL_DMAX], ddelta[VOL_DMAX]; };
static bool rate_chain(double r_max, double r_min, double q, double m_th, double surface_rate, double surface_depth_nm, double thickness_nm, int D,
                       RateChain& c)
{
    MackLaw law;
    if (D < 1 || D > VOL_DMAX || !make_mack(r_max, r_min, q, m_th, surface_rate, surface_depth_nm, thickness_nm, D, law)) return false;
    c.a = law.a;
    c.da_dq = c.a * (1.0 / (q + 1.0) - 1.0 / (q - 1.0) + std::log(1.0 - m_th));
    c.da_dm = -q * c.a / (1.0 - m_th);
    for (int d = 0; d < D; ++d) {
        const double z = thickness_nm * (d + 0.5) / D, ez = std::exp(-z / surface_depth_nm);
        c.ez[d] = ez;
        c.ddelta[d] = -(1.0 - surface_rate) * ez * z / (surface_depth_nm * surface_depth_nm);
    }
    return true;
}

}  // namespace litho

extern "C" {

size_t litho_develop_vjp_work_bytes(int B, int D, int n, int max_iterations)
{
    using namespace litho;
    if (!volume_ok(B, D, n) || max_iterations < 1 || max_iterations > VOL_MAXIT) return 0;
    return flag_bytes(max_iterations) + 5 * (size_t)B * D * n * n * sizeof(float);     // flags, links (4), lambda (1)
}

int litho_develop_time_vjp(const float* slowness, const float* T, const float* grad_T, int B, int D, int n, double thickness_nm,
                           double pixel_nm, int max_iterations, float* grad_slowness, void* work, size_t work_bytes,
                           int* launches_host, void* stream)
{
    using namespace litho;
    static unsigned lds_done = 0;
    const bool wide = (n & 3) == 0 && aligned16(slowness) && aligned16(T) && aligned16(grad_slowness);
    return front_derivative(slowness, T, grad_T, B, D, n, 1, thickness_nm, pixel_nm, max_iterations, grad_slowness, work, work_bytes,
                            launches_host, stream, wide, (const void*)k_develop_time_vjp, lds_done, DG_PLANE_BYTES, true,
                            [&](dim3 grid, size_t lds, hipStream_t st, const float* links, const float* in, float* out, int* flag) {
                                hipLaunchKernelGGL(k_develop_time_vjp, grid, dim3(256), lds, st, links, grad_T, in, out, D, n, flag);
                            });
}

int litho_develop_rate_vjp(const float* x, int volumes, int D, int n, const float* gains_host, int n_gains, double kappa, double r_max,
                           double r_min, double q, double m_th, double surface_rate, double surface_depth_nm, double thickness_nm,
                           const float* grad_slowness, float* grad_x, void* stream)
{
    using namespace litho;
    VolGains gains;
    MackLaw law;
    if (!x || !grad_slowness || !grad_x || !volume_ok(volumes, D, n) || !make_gains(gains_host, n_gains, volumes, D, gains) ||
        !finite_pos(kappa) || !make_mack(r_max, r_min, q, m_th, surface_rate, surface_depth_nm, thickness_nm, D, law))
        return LITHO_E_ARG;
    const size_t x_bytes = (size_t)volumes * D * n * n * sizeof(float);
    if (!writes_clear({{grad_x, x_bytes}}, {{x, x_bytes}, {grad_slowness, x_bytes * n_gains}})) return LITHO_E_ARG;
    const int planes = volumes * D;
    const bool wide = (n & 3) == 0 && aligned16(x) && aligned16(grad_slowness) && aligned16(grad_x);
    LAUNCH_PACKED(k_develop_rate_vjp, wide, n, planes, (hipStream_t)stream, x, grad_slowness, grad_x, planes, D, n, gains, n_gains, kappa,
                  law.rmax_a1, law.rmin, law.q, law.a, law.surface);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

size_t litho_develop_rate_params_work_bytes(int volumes, int D, int n, int n_gains)
{
    using namespace litho;
    if (!volume_ok(volumes, D, n) || n_gains < 1 || n_gains > VOL_GAINS || (long long)volumes * n_gains * D > 65535) return 0;
    return (size_t)n_gains * volumes * D * plane_blocks(n, 1) * 6 * sizeof(double);
}

int litho_develop_rate_vjp_params(const float* x, int volumes, int D, int n, const float* gains_host, int n_gains, double kappa, double r_max,
                                  double r_min, double q, double m_th, double surface_rate, double surface_depth_nm, double thickness_nm,
                                  const float* grad_slowness, double* plane_sums, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    VolGains gains;
    MackLaw law;
    if (!x || !grad_slowness || !plane_sums || !work || !volume_ok(volumes, D, n) || !make_gains(gains_host, n_gains, volumes, D, gains) ||
        !finite_pos(kappa) || !make_mack(r_max, r_min, q, m_th, surface_rate, surface_depth_nm, thickness_nm, D, law))
        return LITHO_E_ARG;
    if (!aligned16(work) || !aligned16(plane_sums)) return LITHO_E_ARG;
    const size_t need = litho_develop_rate_params_work_bytes(volumes, D, n, n_gains);
    if (work_bytes < need) return LITHO_E_WORKSPACE;
    const int planes = volumes * D;
    const size_t x_bytes = (size_t)planes * n * n * sizeof(float), out_bytes = (size_t)n_gains * planes * 6 * sizeof(double);
    if (!writes_clear({{plane_sums, out_bytes}, {work, need}}, {{x, x_bytes}, {grad_slowness, x_bytes * n_gains}})) return LITHO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = plane_blocks(n, 1);
    hipLaunchKernelGGL(k_develop_rate_params, dim3(blocks, (unsigned)(n_gains * planes)), dim3(256), 0, st, x, grad_slowness, (double*)work,
                       planes, D, n, gains, kappa, law.rmax_a1, law.rmin, law.q, law.a, law.surface);
    hipLaunchKernelGGL(k_vol_total<6>, dim3((unsigned)(n_gains * planes)), dim3(256), 0, st, (const double*)work, (long long)blocks, plane_sums);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_develop_rate_param_chain(double r_max, double r_min, double q, double m_th, double surface_rate, double surface_depth_nm,
                                   double thickness_nm, int D, int groups, const double* plane_sums, double* grad_param)
{
    using namespace litho;
    RateChain c;
    if (!plane_sums || !grad_param || groups < 1 || !rate_chain(r_max, r_min, q, m_th, surface_rate, surface_depth_nm, thickness_nm, D, c))
        return LITHO_E_ARG;
    const double a = c.a;
    for (int g = 0; g < groups; ++g) {
        double sum[4] = {0.0, 0.0, 0.0, 0.0}, s_a = 0.0, s_r0 = 0.0, s_delta = 0.0;       // kappa, R, rmin, q at fixed a
        for (int d = 0; d < D; ++d) {                    // the planes in ascending order
            const double* t = plane_sums + ((size_t)g * D + d) * 6;
            for (int j = 0; j < 4; ++j) sum[j] += t[j];
            s_a += t[4];
            s_r0 += t[5] * c.ez[d];                      // f = 1 - (1 - r0) exp(-z / delta)
            s_delta += t[5] * c.ddelta[d];
        }
        double* out = grad_param + (size_t)g * 7;
        out[0] = sum[0];
        out[1] = sum[1] * (a + 1.0);                     // R = rmax (a + 1); the a slot already follows R through a
        out[2] = sum[2];
        out[3] = sum[3] + s_a * c.da_dq;
        out[4] = s_a * c.da_dm;
        out[5] = s_r0;
        out[6] = s_delta;
    }
    return LITHO_OK;
}

int litho_develop_rate_jvp(const float* x, int volumes, int D, int n, const float* gains_host, int n_gains, double kappa, double r_max,
                           double r_min, double q, double m_th, double surface_rate, double surface_depth_nm, double thickness_nm, int P,
                           const float* dx, const double* dphi, float* dslowness, void* stream)
{
    using namespace litho;
    VolGains gains;
    MackLaw law;
    if (!x || !dphi || !dslowness || P < 1 || P > LITHO_TANGENT_MAX || !volume_ok(volumes, D, n) ||
        !make_gains(gains_host, n_gains, volumes, D, gains) || (long long)P * n_gains * volumes * D > 65535 || !finite_pos(kappa) ||
        !make_mack(r_max, r_min, q, m_th, surface_rate, surface_depth_nm, thickness_nm, D, law))
        return LITHO_E_ARG;
    if (!aligned16(dphi)) return LITHO_E_ARG;
    const size_t x_bytes = (size_t)volumes * D * n * n * sizeof(float), out_bytes = x_bytes * n_gains * P;
    const size_t phi_bytes = (size_t)P * D * 6 * sizeof(double);
    if (!writes_clear({{dslowness, out_bytes}}, {{x, x_bytes}, {dphi, phi_bytes}, {dx, x_bytes * P}})) return LITHO_E_ARG;
    const int planes = volumes * D;
    const bool wide = (n & 3) == 0 && aligned16(x) && aligned16(dx) && aligned16(dslowness);
    LAUNCH_PACKED(k_develop_rate_jvp, wide, n, planes, (hipStream_t)stream, x, dx, dphi, dslowness, planes, D, n, gains, n_gains, P, kappa,
                  law.rmax_a1, law.rmin, law.q, law.a, law.surface);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_develop_rate_param_tangent(double r_max, double r_min, double q, double m_th, double surface_rate, double surface_depth_nm,
                                     double thickness_nm, int D, const double* dparam, double* dphi)
{
    using namespace litho;
    RateChain c;
    if (!dparam || !dphi || !rate_chain(r_max, r_min, q, m_th, surface_rate, surface_depth_nm, thickness_nm, D, c)) return LITHO_E_ARG;
    for (int d = 0; d < D; ++d) {
        double* out = dphi + (size_t)d * 6;
        out[0] = dparam[0];
        out[1] = (c.a + 1.0) * dparam[1];
        out[2] = dparam[2];
        out[3] = dparam[3];
        out[4] = c.da_dq * dparam[3] + c.da_dm * dparam[4];
        out[5] = c.ez[d] * dparam[5] + c.ddelta[d] * dparam[6];
    }
    return LITHO_OK;
}

size_t litho_develop_jvp_work_bytes(int B, int D, int n, int P, int max_iterations)
{
    using namespace litho;
    if (!volume_ok(B, D, n) || P < 1 || P > LITHO_TANGENT_MAX || (long long)P * B * D > 65535 || max_iterations < 1 ||
        max_iterations > VOL_MAXIT)
        return 0;
    return flag_bytes(max_iterations) + (4 + (size_t)P) * B * D * n * n * sizeof(float);     // flags, links (4), tau (P)
}

int litho_develop_time_jvp(const float* slowness, const float* T, const float* dslowness, int B, int D, int n, int P, double thickness_nm,
                           double pixel_nm, int max_iterations, float* dT, void* work, size_t work_bytes, int* launches_host, void* stream)
{
    using namespace litho;
    static unsigned lds_done = 0;
    const bool wide = (n & 3) == 0 && aligned16(slowness) && aligned16(T);
    return front_derivative(slowness, T, dslowness, B, D, n, P, thickness_nm, pixel_nm, max_iterations, dT, work, work_bytes, launches_host,
                            stream, wide, (const void*)k_develop_time_jvp, lds_done, DT_PLANE_BYTES, false,
                            [&](dim3 grid, size_t lds, hipStream_t st, const float* links, const float* in, float* out, int* flag) {
                                hipLaunchKernelGGL(k_develop_time_jvp, grid, dim3(256), lds, st, links, dslowness, in, out, B, D, n, flag);
                            });
}

}  // extern "C"
