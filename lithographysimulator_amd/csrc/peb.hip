// peb.hip -- the post-exposure bake of a chemically amplified resist behind litho_peb_expose, litho_peb_bake and litho_peb_rate
// (no reference counterpart; the definitions are in include/litho_abbe.h, the checker is their float64 restatement
// tests/peb_oracle.py).  Built with -ffp-contract=off (Makefile): every fp32 result is a fixed sequence of single operations.
//
// Volumes are fp32 [B, D, n, n], D <= 32 planes through the resist, x fastest.  The forward kernels:
//   k_peb_expose   acid h0 = 1 - exp(-(C g) I) in double per cell, the gains in a loop inside
//   k_peb_direct   one bake step per launch: a thread per cell, the six neighbours of both species from global memory
//   k_peb_fused    s >= 2 bake steps per launch (temporal blocking, below)
//   k_peb_rate     inhibitor m = exp(-kAmp a), Mack's rate and the surface factor in double per cell, slowness 1 / r out
// and behind litho_peb_bake_vjp and litho_peb_expose_vjp, the bake and the exposure backwards (section 2b):
//   k_peb_taped       one bake step per launch through peb_step, without a, storing the step's (hd, qd) when a tape is given
//   k_peb_adjoint     one backward step per launch: a thread per cell gathers (u, v) at the cell and its six neighbours
//   k_peb_expose_vjp  gI = sum_g (C g) exp(-(C g) I) gh0[g] in double per cell
// and behind litho_peb_bake_vjp_params and litho_peb_expose_vjp_params, the sums for the resist's parameters (section 2c):
//   k_peb_adjoint_params  k_peb_adjoint plus the six step-parameter terms of the cell, added per workgroup into its own slot
//   k_peb_expose_params   gh0 (g I) exp(-(C g) I) per cell, added per workgroup into its own slot
//   k_vol_total           (resist_volume.hpp) the slots of a volume added in a fixed order
// and behind litho_peb_expose_jvp and litho_peb_bake_jvp, forward mode (section 2d): k_peb_expose_jvp, and k_peb_jvp, one bake step
// with its P tangents.  Each piece of arithmetic exists once: peb_laplacians and peb_diffuse (the diffusion line of the step, of
// its transpose and of its tangent), peb_step (every forward kernel calls it with the same inputs in the same order, so the bits
// of a bake depend neither on how its steps are cut into launches nor on the entry that runs them), peb_react_partials (the
// reaction's derivatives, adjoint and tangent), peb_start (the opening of k_peb_taped and k_peb_jvp) and peb_step_adjoint (one
// backward cell, both adjoint kernels); the kernels that take one cell per thread get it and its six clamped neighbour offsets
// from peb_cell.  On the host PebBake and bake_checked are the one description and the one set of checks of the five entries that
// take a bake, and step_jacobian the coefficients whose two products are param_chain and param_tangent.  expose and rate move
// four consecutive x per thread (16-byte accesses) when n is a multiple of 4 and the pointers are 16-byte aligned, one otherwise.
// The limits, the packs, the host predicates (the aliasing rule writes_clear among them), the gains and Mack's rate law are
// resist_volume.hpp's, shared with develop.hip and develop_grad.hip.
//
// k_peb_fused.  A workgroup owns a 16 x 16 lateral tile with all D planes.  It loads h and q of the tile and an s-cell lateral
// halo into LDS, W = 16 + 2 s cells on a side; a cell beyond the grid is read from its mirror image (mirror_index, folding as
// often as needed when n < s), so the LDS window is a piece of the mirror-extended lattice and a ghost cell takes exactly the
// update of the cell it mirrors (the update pairs W + E and S + N).  Step j = 1 .. s updates the cells [j, W - j)^2 x D from
// one LDS copy into the other (Jacobi; a barrier; the copies swap): the region that is still exact shrinks by one cell per
// step and after s steps is the tile.  The amplification integral a is kept for the tile's own cells only, in LDS.  LDS:
// D (4 W^2 + 256) floats.  Launches ping-pong h and q between the outputs and the caller's workspace; a is updated in place
// by the one thread that owns the cell.  No workgroup reads what another writes in the same launch; no atomics.
#include "resist_volume.hpp"

namespace litho {

static constexpr int PEB_SMAX = 4, PEB_MAXSTEPS = 65536;  // bake steps per launch, per bake
static constexpr size_t PEB_LDS_MAX = 160 * 1024;         // what one workgroup can have on gfx950
// The automatic choice of steps per launch takes the largest s <= PEB_SMAX whose LDS fits this budget, else the direct kernel.
// It started at 64 KiB (two workgroups per CU of 160 KiB) and the first timing (scripts/peb_time.py, LABNOTES: 2048^2, S = 32)
// set it to 0: the direct kernel runs at 87 - 91 % of the HBM rate, 0.22 ms per step at D = 8 against 0.46 / 0.39 / 0.35 for the
// untuned fused kernel at s = 2 / 3 / 4 (D = 16: 0.43 against 1.60 / 1.38 / 1.27), which moves fewer bytes but is bound by its
// index arithmetic and LDS traffic.  Until the fused kernel wins somewhere, the automatic choice is the direct kernel.
static constexpr size_t PEB_LDS_BUDGET = 0;

// what one bake step needs, fp32 as the kernels use it; rides in the kernel arguments
struct PebStep {
    float lxy_h, lz_h, lxy_q, lz_q;                       // lambda = D_s dt / spacing^2 per species and direction
    float beta, fl, half_dt;                              // kQuench dt, exp(-kLoss dt), dt / 2
    int diffuse_h, diffuse_q, instant;                    // sigma > 0 per species; kQuench dt = +inf
};
struct PebNb {
    float w, e, s, n, u, d;
};

// A thread's cell in the kernels that take one cell per thread (grid.x covers the n^2 cells of a plane, grid.y the B D planes):
// its index in the batch and the offsets to its six neighbours.  A neighbour outside the grid is the cell's mirror image: the
// cell itself, offset 0.
struct PebCell {
    size_t at;
    long long w, e, s, n, u, d;
};
__device__ __forceinline__ bool peb_cell(int D, int n, PebCell& c)          // false: this thread has no cell
{
    const long long plane_elems = (long long)n * n;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= plane_elems) return false;
    const int p = blockIdx.y, d = p % D, row = (int)(e / n), col = (int)(e - (long long)row * n);
    c.at = (size_t)p * plane_elems + e;
    c.w = col > 0 ? -1 : 0;
    c.e = col + 1 < n ? 1 : 0;
    c.s = row > 0 ? -(long long)n : 0;
    c.n = row + 1 < n ? n : 0;
    c.u = d > 0 ? -plane_elems : 0;
    c.d = d + 1 < D ? plane_elems : 0;
    return true;
}
// the six neighbours of the cell that `here` points at
__device__ __forceinline__ PebNb peb_around(const float* here, const PebCell& c)
{
    return PebNb{here[c.w], here[c.e], here[c.s], here[c.n], here[c.u], here[c.d]};
}

// ---- 1. exposure: h0 = 1 - exp(-(C g) I), NaN where that is negative or NaN (litho_develop_rate's convention).  Double per
// cell, rounded once.  grid.y: the F D planes of the image.
template <int VEC>
__global__ __launch_bounds__(256) void k_peb_expose(const float* __restrict__ image, float* __restrict__ out, int planes, int n,
                                                    const VolGains gains, int n_gains, double C)
{
    const long long plane_elems = (long long)n * n;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e >= plane_elems) return;
    const int p = blockIdx.y;
    const Pack<VEC> I = load_pack<VEC>(image + (size_t)p * plane_elems + e);
    for (int gi = 0; gi < n_gains; ++gi) {
        const double Cg = C * (double)gains.g[gi];
        Pack<VEC> h;
        for (int v = 0; v < VEC; ++v) {
            const double h0 = 1.0 - exp(-(Cg * (double)I.v[v]));
            h.v[v] = (h0 >= 0.0) ? (float)h0 : __builtin_nanf("");
        }
        store_pack<VEC>(out + ((size_t)gi * planes + p) * plane_elems + e, h);
    }
}

// ---- 2. one bake step of one cell.  The two Laplacians of a value x with the neighbours b, lateral and vertical, in T = float,
// or in double from the widened fp32 operands (the parameter terms of k_peb_adjoint_params); and the diffusion update of one
// value with them: the forward's line, its transpose on (u, v) and its tangent.
template <class T>
struct PebLap { T xy, z; };
template <class T>
__device__ __forceinline__ PebLap<T> peb_laplacians(const PebNb& b, T x)
{
    return PebLap<T>{(((T)b.w + (T)b.e) + ((T)b.s + (T)b.n)) - (T)4 * x, ((T)b.u + (T)b.d) - (T)2 * x};
}
__device__ __forceinline__ float peb_diffuse(float x, const PebNb& b, float lxy, float lz)
{
    const PebLap<float> L = peb_laplacians(b, x);
    return x + lxy * L.xy + lz * L.z;
}
// h, q: the cell at the start of the step; nb_h(), nb_q(): its six neighbours at the start of the step, fetched only for a
// species that diffuses.  Diffusion (Jacobi, no flux), neutralisation, acid loss, and the trapezoid of the amplification
// integral, in this order; every line is include/litho_abbe.h's.  hd, qd: the two species after the diffusion line, what the
// reaction saw -- the tape of the backward sweep (k_peb_taped), a dead store elsewhere.
template <class FH, class FQ>
__device__ __forceinline__ void peb_step(const PebStep& P, float h, float q, FH nb_h, FQ nb_q, float& h_new, float& q_new, float& a,
                                         float& hd, float& qd)
{
    hd = P.diffuse_h ? peb_diffuse(h, nb_h(), P.lxy_h, P.lz_h) : h;
    qd = P.diffuse_q ? peb_diffuse(q, nb_q(), P.lxy_q, P.lz_q) : q;
    const float R = P.instant ? ((hd < qd) ? hd : qd) : P.beta * hd * qd / (1.f + P.beta * (hd + qd));
    h_new = (hd - R) * P.fl;
    q_new = qd - R;
    a = a + P.half_dt * (h + h_new);
}
// The start of a forward step of one cell in k_peb_taped and k_peb_jvp (k_peb_direct keeps its own lines: its machine code is the
// measured one): the cell, whether this is the first step (q_in == nullptr: q = q0 everywhere), h and q at the start of the step
// and the six neighbours of each species that diffuses -- zeros for one that does not, which nothing reads.
struct PebStart { PebCell c; bool first; float h, q; PebNb bh, bq; };
__device__ __forceinline__ bool peb_start(const PebStep& P, const float* h_in, const float* q_in, float q0, int D, int n, PebStart& s)
{
    if (!peb_cell(D, n, s.c)) return false;              // this thread has no cell
    const PebNb zero = PebNb{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    s.first = q_in == nullptr;
    s.h = h_in[s.c.at];
    s.q = s.first ? q0 : q_in[s.c.at];
    s.bh = P.diffuse_h ? peb_around(h_in + s.c.at, s.c) : zero;
    s.bq = P.diffuse_q ? (s.first ? PebNb{q0, q0, q0, q0, q0, q0} : peb_around(q_in + s.c.at, s.c)) : zero;
    return true;
}

// grid.x covers the n^2 cells of a plane, grid.y the B D planes.  q_in == nullptr: the first step, q = q0 everywhere and a = 0.
__global__ __launch_bounds__(256) void k_peb_direct(const float* __restrict__ h_in, const float* __restrict__ q_in, float q0,
                                                    float* __restrict__ h_out, float* __restrict__ q_out, float* __restrict__ a_io,
                                                    int D, int n, const PebStep P)
{
    PebCell c;
    if (!peb_cell(D, n, c)) return;
    const size_t at = c.at;
    const bool first = q_in == nullptr;
    const float h = h_in[at], q = first ? q0 : q_in[at];
    float a = first ? 0.f : a_io[at], h_new, q_new, hd, qd;
    peb_step(P, h, q, [&] { return peb_around(h_in + at, c); },
             [&] { return first ? PebNb{q0, q0, q0, q0, q0, q0} : peb_around(q_in + at, c); }, h_new, q_new, a, hd, qd);
    h_out[at] = h_new;
    q_out[at] = q_new;
    a_io[at] = a;
}

// grid: (tiles, tiles, B).  Dynamic LDS: D (4 W^2 + 256) floats, W = 16 + 2 s.
__global__ __launch_bounds__(256) void k_peb_fused(const float* __restrict__ h_in, const float* __restrict__ q_in, float q0,
                                                   float* __restrict__ h_out, float* __restrict__ q_out, float* __restrict__ a_io,
                                                   int D, int n, int s, const PebStep P)
{
    extern __shared__ __attribute__((aligned(16))) float peb_lds[];
    const int W = VOL_TILE + 2 * s, WW = W * W, cells = D * WW;
    float* hc = peb_lds;                                  // [D][W][W]  the current copy of h, tile + halo
    float* hn = hc + cells;                               //            the next one
    float* qc = hn + cells;
    float* qn = qc + cells;
    float* al = qn + cells;                               // [D][16][16] a of the tile
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * VOL_TILE, y0 = blockIdx.y * VOL_TILE;
    const size_t plane_elems = (size_t)n * n;
    const size_t vol = (size_t)blockIdx.z * D * plane_elems;
    const bool first = q_in == nullptr;
    for (int i = tid; i < cells; i += 256) {
        const int d = i / WW, r = i - d * WW, ly = r / W, lx = r - ly * W;
        const size_t g = vol + (size_t)d * plane_elems + (size_t)mirror_index(y0 - s + ly, n) * n + mirror_index(x0 - s + lx, n);
        hc[i] = h_in[g];
        qc[i] = first ? q0 : q_in[g];
    }
    // thread tid owns the column (tid / 16, tid % 16) of the tile when a is loaded and when the results are stored
    const int oy = tid >> 4, ox = tid & 15;
    const bool inside = y0 + oy < n && x0 + ox < n;
    const size_t own = vol + (size_t)(y0 + oy) * n + (x0 + ox);
    for (int d = 0; d < D; ++d) al[d * 256 + tid] = (first || !inside) ? 0.f : a_io[own + (size_t)d * plane_elems];
    __syncthreads();
    for (int j = 1; j <= s; ++j) {
        const int w = W - 2 * j, ww = w * w, todo = D * ww;
        for (int i = tid; i < todo; i += 256) {
            const int d = i / ww, r = i - d * ww, ry = r / w, ly = j + ry, lx = j + (r - ry * w);
            const int c = (d * W + ly) * W + lx;
            const int up = d > 0 ? -WW : 0, dn = d + 1 < D ? WW : 0;
            auto around = [&](const float* b) -> PebNb { return PebNb{b[c - 1], b[c + 1], b[c - W], b[c + W], b[c + up], b[c + dn]}; };
            const int ty = ly - s, tx = lx - s;
            const bool mine = ty >= 0 && ty < VOL_TILE && tx >= 0 && tx < VOL_TILE;
            const int ai = d * 256 + ty * VOL_TILE + tx;
            float h_new, q_new, hd, qd, a = mine ? al[ai] : 0.f;          // a halo cell's a is not kept
            peb_step(P, hc[c], qc[c], [&] { return around(hc); }, [&] { return around(qc); }, h_new, q_new, a, hd, qd);
            hn[c] = h_new;
            qn[c] = q_new;
            if (mine) al[ai] = a;
        }
        __syncthreads();
        float* t = hc; hc = hn; hn = t;
        t = qc; qc = qn; qn = t;
    }
    if (!inside) return;
    for (int d = 0; d < D; ++d) {
        const int c = (d * W + oy + s) * W + ox + s;
        const size_t g = own + (size_t)d * plane_elems;
        h_out[g] = hc[c];
        q_out[g] = qc[c];
        a_io[g] = al[d * 256 + tid];
    }
}

// ---- 2b. the backward sweep of the bake (litho_peb_bake_vjp; the definitions are include/litho_abbe.h's "Gradients through the
// bake").  k_peb_taped is k_peb_direct without the amplification integral (nothing in the adjoint needs a): one step through
// peb_step, the step's (hd, qd) to the tape when one is given, the new state when one is wanted.  q_in == nullptr: q = q0.
__global__ __launch_bounds__(256) void k_peb_taped(const float* __restrict__ h_in, const float* __restrict__ q_in, float q0,
                                                   float* __restrict__ h_out, float* __restrict__ q_out, float* __restrict__ hd_out,
                                                   float* __restrict__ qd_out, int D, int n, const PebStep P)
{
    PebStart s;
    if (!peb_start(P, h_in, q_in, q0, D, n, s)) return;
    const size_t at = s.c.at;
    float a = 0.f, h_new, q_new, hd, qd;
    peb_step(P, s.h, s.q, [&] { return s.bh; }, [&] { return s.bq; }, h_new, q_new, a, hd, qd);
    if (h_out) {
        h_out[at] = h_new;
        q_out[at] = q_new;
    }
    if (hd_out) {
        hd_out[at] = hd;
        qd_out[at] = qd;
    }
}

// The reaction's partials at the (hd, qd) the reaction saw, fp32: R itself, Rh = dR/dhd, Rq = dR/dqd and Rb = dR/dbeta.  With
// instantaneous neutralisation R = min(hd, qd) and the partials take the forward's own comparison; no beta in it.
struct PebReact { float Rh, Rq, Rb, R; };
__device__ __forceinline__ PebReact peb_react_partials(const PebStep& P, float hd, float qd)
{
    if (P.instant) return (hd < qd) ? PebReact{1.f, 0.f, 0.f, hd} : PebReact{0.f, 1.f, 0.f, qd};
    const float Dn = 1.f + P.beta * (hd + qd), DD = Dn * Dn;
    return PebReact{P.beta * qd * (1.f + P.beta * qd) / DD, P.beta * hd * (1.f + P.beta * hd) / DD, hd * qd / DD, P.beta * hd * qd / Dn};
}
// The pointwise half of the backward step: (u, v) of one cell from hp = hbar + half_dt abar, qbar and the step's (hd, qd).
struct PebUV {
    float u, v;
};
__device__ __forceinline__ PebUV peb_react_adjoint(const PebStep& P, float hp, float qb, float hd, float qd)
{
    const PebReact r = peb_react_partials(P, hd, qd);
    const float fhp = P.fl * hp;
    return PebUV{fhp * (1.f - r.Rh) - qb * r.Rh, qb * (1.f - r.Rq) - fhp * r.Rq};
}
// One backward step of one cell: (hb, qb) = (hbar, qbar) before the step, and with them the cell's own fp32 hp and (u, v), which
// the parameter terms take.  hb_in, qb_in, abar: the cotangents after the step, nullptr = zero; hd, qd: the step's tape.  (u, v)
// at the six neighbours (the cell itself beyond a face) are asked for only when a species diffuses.  A_s is symmetric, so the
// transposed stencil is the forward's line on u and v: a gather.
struct PebBack { float hb, qb, hp; PebUV c; };
__device__ __forceinline__ PebBack peb_step_adjoint(const PebStep& P, const PebCell& cell, const float* hb_in, const float* qb_in,
                                                    const float* abar, const float* hd, const float* qd)
{
    auto hp_at = [&](size_t c) { return (hb_in ? hb_in[c] : 0.f) + P.half_dt * (abar ? abar[c] : 0.f); };
    auto uv = [&](long long off) -> PebUV {
        const size_t c = (size_t)((long long)cell.at + off);
        return peb_react_adjoint(P, hp_at(c), qb_in ? qb_in[c] : 0.f, hd[c], qd[c]);
    };
    PebBack r;
    r.hp = hp_at(cell.at);
    r.c = uv(0);
    float hu = r.c.u, qv = r.c.v;
    if (P.diffuse_h || P.diffuse_q) {
        const PebUV w = uv(cell.w), e = uv(cell.e), s = uv(cell.s), n = uv(cell.n), up = uv(cell.u), dn = uv(cell.d);
        if (P.diffuse_h) hu = peb_diffuse(r.c.u, PebNb{w.u, e.u, s.u, n.u, up.u, dn.u}, P.lxy_h, P.lz_h);
        if (P.diffuse_q) qv = peb_diffuse(r.c.v, PebNb{w.v, e.v, s.v, n.v, up.v, dn.v}, P.lxy_q, P.lz_q);
    }
    r.hb = hu + P.half_dt * (abar ? abar[cell.at] : 0.f);
    r.qb = qv;
    return r;
}

// grid as k_peb_direct.
__global__ __launch_bounds__(256) void k_peb_adjoint(const float* __restrict__ hb_in, const float* __restrict__ qb_in,
                                                     const float* __restrict__ abar, const float* __restrict__ hd,
                                                     const float* __restrict__ qd, float* __restrict__ hb_out, float* __restrict__ qb_out,
                                                     int D, int n, const PebStep P)
{
    PebCell cell;
    if (!peb_cell(D, n, cell)) return;
    const PebBack r = peb_step_adjoint(P, cell, hb_in, qb_in, abar, hd, qd);
    hb_out[cell.at] = r.hb;
    qb_out[cell.at] = r.qb;
}

// ---- 2c. the step-parameter sums of the backward sweep (litho_peb_bake_vjp_params; include/litho_abbe.h's "Gradients with respect
// to the bake's parameters").  The workgroup's fixed-order sum and the closing kernel are resist_volume.hpp's (vol_block_sum,
// k_vol_total).
// k_peb_adjoint with the step's six parameter terms: the same function gives (hbar_k, qbar_k), so their bits are k_peb_adjoint's.
// h, q: the state at the start of the step (q == nullptr: the first step, q uniform, its Laplacians 0).  The terms are formed in
// double from the fp32 operands; thread 0 adds the workgroup's six sums into the workgroup's own slot
// partials[blockIdx.y][blockIdx.x][6] -- the backward steps are successive launches on one stream, so a slot's additions come in
// the order k = S-1 .. 0.  A thread without a cell contributes zeros and still takes part in the sum.
__global__ __launch_bounds__(256) void k_peb_adjoint_params(const float* __restrict__ hb_in, const float* __restrict__ qb_in,
                                                            const float* __restrict__ abar, const float* __restrict__ h,
                                                            const float* __restrict__ q, const float* __restrict__ hd,
                                                            const float* __restrict__ qd, float* __restrict__ hb_out,
                                                            float* __restrict__ qb_out, double* __restrict__ partials, int D, int n,
                                                            const PebStep P)
{
    __shared__ double lds[4][6];
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    PebCell cell;
    if (peb_cell(D, n, cell)) {
        const size_t at = cell.at;
        const PebBack r = peb_step_adjoint(P, cell, hb_in, qb_in, abar, hd, qd);
        hb_out[at] = r.hb;
        qb_out[at] = r.qb;
        const double hp = r.hp, qbk = qb_in ? qb_in[at] : 0.f, hdc = hd[at], qdc = qd[at], fl = P.fl;
        auto laplacians = [&](const float* x, double w, int j) {
            const PebLap<double> L = peb_laplacians(peb_around(x + at, cell), (double)x[at]);
            t[j] = w * L.xy;
            t[j + 1] = w * L.z;
        };
        if (P.diffuse_h) laplacians(h, (double)r.c.u, 0);
        if (P.diffuse_q && q) laplacians(q, (double)r.c.v, 2);
        double R;
        if (P.instant) {
            R = (hdc < qdc) ? hdc : qdc;                  // the forward's own comparison; no beta in it
        } else {
            const double beta = P.beta, Dn = 1.0 + beta * (hdc + qdc);
            R = beta * hdc * qdc / Dn;
            t[4] = -(fl * hp + qbk) * (hdc * qdc) / (Dn * Dn);
        }
        t[5] = hp * (hdc - R);
    }
    vol_block_sum<6>(t, lds);
    if (threadIdx.x == 0) {
        double* slot = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 6;
        for (int j = 0; j < 6; ++j) slot[j] = slot[j] + t[j];
    }
}

// The exposure's VJP: gI = sum_g (C g) exp(-(C g) I) gh0[g], the gains in ascending order, double per cell, rounded once.
template <int VEC>
__global__ __launch_bounds__(256) void k_peb_expose_vjp(const float* __restrict__ image, const float* __restrict__ grad_acid,
                                                        float* __restrict__ grad_image, int planes, int n, const VolGains gains,
                                                        int n_gains, double C)
{
    const long long plane_elems = (long long)n * n;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e >= plane_elems) return;
    const int p = blockIdx.y;
    const Pack<VEC> I = load_pack<VEC>(image + (size_t)p * plane_elems + e);
    double sum[VEC];
    for (int v = 0; v < VEC; ++v) sum[v] = 0.0;
    for (int gi = 0; gi < n_gains; ++gi) {
        const double Cg = C * (double)gains.g[gi];
        const Pack<VEC> g = load_pack<VEC>(grad_acid + ((size_t)gi * planes + p) * plane_elems + e);
        for (int v = 0; v < VEC; ++v) sum[v] = sum[v] + Cg * exp(-(Cg * (double)I.v[v])) * (double)g.v[v];
    }
    Pack<VEC> out;
    for (int v = 0; v < VEC; ++v) out.v[v] = (float)sum[v];
    store_pack<VEC>(grad_image + (size_t)p * plane_elems + e, out);
}

// The exposure's parameter sum (litho_peb_expose_vjp_params): per cell of a gained plane gh0 (g I) exp(-(C g) I), the derivative of
// h0 with respect to C times its cotangent, in double; a cell whose acid is NaN (1 - exp negative or NaN) contributes 0.  The
// workgroup's sum goes to its own slot partials[gained plane][workgroup]; grid.y: the n_gains x planes gained planes.
__global__ __launch_bounds__(256) void k_peb_expose_params(const float* __restrict__ image, const float* __restrict__ grad_acid,
                                                           double* __restrict__ partials, int planes, int n, const VolGains gains, double C)
{
    __shared__ double lds[4][1];
    double t[1] = {0.0};
    const long long plane_elems = (long long)n * n;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int gp = blockIdx.y, gi = gp / planes, p = gp - gi * planes;
    if (e < plane_elems) {
        const double g = (double)gains.g[gi], Cg = C * g, I = image[(size_t)p * plane_elems + e];
        const double ex = exp(-(Cg * I));
        if (1.0 - ex >= 0.0) t[0] = (double)grad_acid[(size_t)gp * plane_elems + e] * ((g * I) * ex);
    }
    vol_block_sum<1>(t, lds);
    if (threadIdx.x == 0) partials[(size_t)gp * gridDim.x + blockIdx.x] = t[0];
}

// ---- 2d. forward mode (litho_peb_expose_jvp, litho_peb_bake_jvp; include/litho_abbe.h's "Forward mode (tangents) of the resist
// chain").  P directions ride in one launch: the kernel arguments carry their host numbers, the volumes are direction-major.
static constexpr int TAN_MAX = LITHO_TANGENT_MAX;
struct TanScalars {
    double v[TAN_MAX];                                    // dC per direction
};
struct PebTanStep {
    float d[TAN_MAX][6];                                  // d(lxy_h, lz_h, lxy_q, lz_q, beta, fl) per direction, rounded once
    float dq0[TAN_MAX];                                   // the uniform dq_0 per direction
};

// The exposure's tangent: dh0 = exp(-(C g) I) ((g I) dC_p + (C g) dI_p) in double per cell, rounded once; exactly 0 where the acid
// is NaN.  grid.y: the planes of the image; the directions and the gains in loops inside.  dimage == nullptr: dI = 0.
template <int VEC>
__global__ __launch_bounds__(256) void k_peb_expose_jvp(const float* __restrict__ image, const float* __restrict__ dimage,
                                                        float* __restrict__ out, int planes, int n, const VolGains gains, int n_gains,
                                                        double C, int P, const TanScalars dC)
{
    const long long plane_elems = (long long)n * n;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e >= plane_elems) return;
    const int p = blockIdx.y;
    const Pack<VEC> I = load_pack<VEC>(image + (size_t)p * plane_elems + e);
    for (int k = 0; k < P; ++k) {
        const Pack<VEC> dI = dimage ? load_pack<VEC>(dimage + ((size_t)k * planes + p) * plane_elems + e) : fill_pack<VEC>(0.f);
        for (int gi = 0; gi < n_gains; ++gi) {
            const double g = (double)gains.g[gi], Cg = C * g;
            Pack<VEC> r;
            for (int v = 0; v < VEC; ++v) {
                const double Iv = (double)I.v[v], ex = exp(-(Cg * Iv));
                const double t = ex * ((g * Iv) * dC.v[k] + Cg * (double)dI.v[v]);
                r.v[v] = (1.0 - ex >= 0.0) ? (float)t : 0.f;
            }
            store_pack<VEC>(out + (((size_t)k * n_gains + gi) * planes + p) * plane_elems + e, r);
        }
    }
}

// One bake step with its P tangents: grid as k_peb_direct, a thread per cell.  The primal goes through peb_step with
// k_peb_direct's operands, so (h, q, a) are its bits; the cell's seven-point loads, its two Laplacians per species and R_h, R_q,
// Dn of the reaction are formed once and reused by every direction.  q_in == nullptr: the first step, q = q0, dq = dq0[p], a = da
// = 0, and dh = 0 when dh_in is nullptr too.  Tangent volumes are [P][V], V the cells of the batch.
__global__ __launch_bounds__(256) void k_peb_jvp(const float* __restrict__ h_in, const float* __restrict__ q_in, float q0,
                                                 float* __restrict__ h_out, float* __restrict__ q_out, float* __restrict__ a_io,
                                                 const float* __restrict__ dh_in, const float* __restrict__ dq_in,
                                                 float* __restrict__ dh_out, float* __restrict__ dq_out, float* __restrict__ da_io,
                                                 size_t V, int D, int n, int P, const PebStep S, const PebTanStep T)
{
    PebStart s;
    if (!peb_start(S, h_in, q_in, q0, D, n, s)) return;
    const PebCell& c = s.c;
    const size_t at = c.at;
    const bool first = s.first;
    float a = first ? 0.f : a_io[at], h_new, q_new, hd, qd;
    peb_step(S, s.h, s.q, [&] { return s.bh; }, [&] { return s.bq; }, h_new, q_new, a, hd, qd);
    h_out[at] = h_new;
    q_out[at] = q_new;
    a_io[at] = a;
    // what every direction shares
    const PebLap<float> lap_h = peb_laplacians(s.bh, s.h), lap_q = peb_laplacians(s.bq, s.q);
    const PebReact r = peb_react_partials(S, hd, qd);
    const float hR = hd - r.R;
    const PebNb zero = PebNb{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < P; ++p) {
        const size_t tp = (size_t)p * V + at;
        const float dh = dh_in ? dh_in[tp] : 0.f, dq = first ? T.dq0[p] : dq_in[tp];
        float dhd = dh, dqd = dq;
        if (S.diffuse_h)
            dhd = peb_diffuse(dh, dh_in ? peb_around(dh_in + tp, c) : zero, S.lxy_h, S.lz_h) + T.d[p][0] * lap_h.xy + T.d[p][1] * lap_h.z;
        if (S.diffuse_q)
            dqd = peb_diffuse(dq, first ? PebNb{dq, dq, dq, dq, dq, dq} : peb_around(dq_in + tp, c), S.lxy_q, S.lz_q) + T.d[p][2] * lap_q.xy +
                  T.d[p][3] * lap_q.z;
        const float dR = S.instant ? ((hd < qd) ? dhd : dqd) : (r.Rh * dhd + r.Rq * dqd) + r.Rb * T.d[p][4];
        const float dh_new = (dhd - dR) * S.fl + hR * T.d[p][5];
        dh_out[tp] = dh_new;
        dq_out[tp] = dqd - dR;
        da_io[tp] = (first ? 0.f : da_io[tp]) + S.half_dt * (dh + dh_new);
    }
}

// ---- 3. rate: m = exp(-kAmp a), then mack_slowness of 1 - m with the surface factor of the plane (resist_volume.hpp, the
// function k_develop_rate calls): NaN where 1 - m is negative or NaN.  grid.y: the B D planes.
template <int VEC>
__global__ __launch_bounds__(256) void k_peb_rate(const float* __restrict__ dose, float* __restrict__ slowness, float* __restrict__ inhibitor,
                                                  int D, int n, double k_amp, double rmax_a1, double rmin, double q, double a_m,
                                                  const VolSurface surface)
{
    const long long plane_elems = (long long)n * n;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e >= plane_elems) return;
    const int p = blockIdx.y;
    const double f = surface.f[p % D];
    const size_t at = (size_t)p * plane_elems + e;
    const Pack<VEC> a = load_pack<VEC>(dose + at);
    Pack<VEC> s, mi;
    for (int v = 0; v < VEC; ++v) {
        const double m = exp(-(k_amp * (double)a.v[v]));
        s.v[v] = mack_slowness(1.0 - m, rmax_a1, rmin, q, a_m, f);
        mi.v[v] = (float)m;
    }
    store_pack<VEC>(slowness + at, s);
    if (inhibitor) store_pack<VEC>(inhibitor + at, mi);
}

static size_t lds_bytes(int D, int s)
{
    const size_t W = VOL_TILE + 2 * s;
    return (size_t)D * (4 * W * W + VOL_TILE * VOL_TILE) * sizeof(float);
}

// lambda_xy = sigma^2 / (2 S pixel^2), lambda_z = (v sigma)^2 / (2 S hz^2): D_s dt / spacing^2 with sigma = sqrt(2 D_s bakeTime)
static void lambdas(double sigma, double vscale, double pixel, double hz, int S, double& lxy, double& lz)
{
    const double sz = vscale * sigma;
    lxy = sigma * sigma / (2.0 * S * (pixel * pixel));
    lz = sz * sz / (2.0 * S * (hz * hz));
}
static bool stable(double sigma, double vscale, double pixel, double hz, int S)
{
    double lxy, lz;
    lambdas(sigma, vscale, pixel, hz, S, lxy, lz);
    return 4.0 * lxy + 2.0 * lz <= 1.0;
}
// the smallest S with 4 lambda_xy + 2 lambda_z <= 1 for both species; 0 when the arguments are bad or it exceeds the cap
static int min_steps(double sigma_h, double sigma_q, double vscale, double thickness, int D, double pixel)
{
    if (!finite_nonneg(sigma_h) || !finite_nonneg(sigma_q) || !finite_nonneg(vscale) || !finite_pos(thickness) || !finite_pos(pixel) ||
        D < 1 || D > VOL_DMAX)
        return 0;
    const double hz = thickness / D;
    const double sigma = sigma_h > sigma_q ? sigma_h : sigma_q;       // both lambdas grow with sigma: the larger one decides
    const double need = sigma * sigma * (2.0 / (pixel * pixel) + (vscale * vscale) / (hz * hz));
    if (!(need <= (double)PEB_MAXSTEPS + 1.0)) return 0;              // too many, infinite or NaN
    int S = (int)need - 1;                                            // the closed form, then settled with the test the kernels' lambdas pass
    if (S < 1) S = 1;
    while (S <= PEB_MAXSTEPS && !stable(sigma, vscale, pixel, hz, S)) ++S;
    return S <= PEB_MAXSTEPS ? S : 0;
}

// The bake's physical description as the entry points take it; quencher0 where the entry has one.
struct PebBake {
    double thickness_nm, pixel_nm, quencher0, k_quench, k_loss, sigma_acid_nm, sigma_quencher_nm, vertical_scale, bake_time_s;
    int D, steps;
};
// the step's parameters as the kernels take them: formed in double, rounded to fp32 once
static PebStep step_of(const PebBake& b)
{
    const double hz = b.thickness_nm / b.D, dt = b.bake_time_s / b.steps;
    double lxy_h, lz_h, lxy_q, lz_q;
    lambdas(b.sigma_acid_nm, b.vertical_scale, b.pixel_nm, hz, b.steps, lxy_h, lz_h);
    lambdas(b.sigma_quencher_nm, b.vertical_scale, b.pixel_nm, hz, b.steps, lxy_q, lz_q);
    PebStep P;
    P.lxy_h = (float)lxy_h; P.lz_h = (float)lz_h; P.lxy_q = (float)lxy_q; P.lz_q = (float)lz_q;
    P.beta = (float)(b.k_quench * dt);
    P.fl = (float)std::exp(-b.k_loss * dt);
    P.half_dt = (float)(0.5 * dt);
    P.diffuse_h = b.sigma_acid_nm > 0.0;
    P.diffuse_q = b.sigma_quencher_nm > 0.0;
    P.instant = std::isinf(P.beta);                       // kQuench = +inf, or kQuench dt beyond fp32
    return P;
}
// The domains of a bake's description: false is LITHO_E_ARG.  with_q0: the entry takes the quencher loading.  Yields what the
// kernels run with; fits: q0 and dt / 2 lie inside fp32's range, which the entries report last, after workspace and aliasing.
struct PebRun { PebStep P; float q0; bool fits; };
static bool bake_checked(const PebBake& b, bool with_q0, PebRun& r)
{
    if ((with_q0 && !finite_nonneg(b.quencher0)) || !(b.k_quench >= 0.0) || !finite_nonneg(b.k_loss) || !finite_pos(b.bake_time_s)) return false;
    const int least = min_steps(b.sigma_acid_nm, b.sigma_quencher_nm, b.vertical_scale, b.thickness_nm, b.D, b.pixel_nm);
    if (least == 0 || b.steps < least || b.steps > PEB_MAXSTEPS) return false;
    r.P = step_of(b);
    r.q0 = with_q0 ? (float)b.quencher0 : 0.f;
    r.fits = !std::isinf(r.q0) && !std::isinf(r.P.half_dt);
    return true;
}
static bool vjp_shape_ok(int B, int D, int n, int steps, int c) { return volume_ok(B, D, n) && steps >= 1 && steps <= PEB_MAXSTEPS && c >= 1 && c <= steps; }
// the workspace of litho_peb_bake_vjp in volumes: the checkpoints (h, q) at c, 2 c, ... < S, one segment's tape (hd, qd) of c steps,
// the ping-pong of the re-run's (h, q) and the ping-pong of (hbar, qbar)
static size_t vjp_volumes(int steps, int c) { return 2 * (size_t)((steps + c - 1) / c - 1) + 2 * (size_t)c + 8; }
// the workspace of litho_peb_bake_vjp_params: its tape keeps four volumes per step -- (hd, qd) and the state (h, q) after the
// step, which is the next step's state at its start -- and behind the volumes, on a 16-byte boundary, one slot of six doubles per
// workgroup of a backward launch
static size_t vjp_params_volumes(int steps, int c) { return 2 * (size_t)((steps + c - 1) / c - 1) + 4 * (size_t)c + 8; }
static size_t vjp_params_slots(int B, int D, int n) { return (size_t)B * D * plane_blocks(n, 1); }
static size_t vjp_params_tape_bytes(int B, int D, int n, int steps, int c)
{
    return (vjp_params_volumes(steps, c) * ((size_t)B * D * n * n * sizeof(float)) + 15) & ~(size_t)15;
}

// litho_peb_bake_vjp (grad_step == nullptr) and litho_peb_bake_vjp_params behind one set of checks and one sweep.  The forward
// launches and the arithmetic of the backward steps are the same in both, so grad_acid_in and grad_quencher_in have the same bits.
static int bake_vjp_run(const float* acid_in, int B, int n, const PebBake& bake, int checkpoint_every, const float* grad_acid,
                        const float* grad_quencher, const float* grad_acid_dose, float* grad_acid_in, float* grad_quencher_in, double* grad_step,
                        bool params, void* work, size_t work_bytes, void* stream)
{
    const int D = bake.D, steps = bake.steps, c = checkpoint_every;
    PebRun run;
    if (!acid_in || !grad_acid_in || !work || (params && !grad_step) || !volume_ok(B, D, n)) return LITHO_E_ARG;
    if (!grad_acid && !grad_quencher && !grad_acid_dose) return LITHO_E_ARG;
    if (!bake_checked(bake, true, run) || c < 1 || c > steps) return LITHO_E_ARG;
    const size_t V = (size_t)B * D * n * n, vol_bytes = V * sizeof(float);
    const size_t slots = params ? vjp_params_slots(B, D, n) : 0, tape_bytes = params ? vjp_params_tape_bytes(B, D, n, steps, c) : 0;
    const size_t need = params ? tape_bytes + slots * 6 * sizeof(double) : vjp_volumes(steps, c) * vol_bytes;
    const size_t step_bytes = (size_t)B * 6 * sizeof(double);
    if (!aligned16(work) || (params && !aligned16(grad_step))) return LITHO_E_ARG;
    if (work_bytes < need) return LITHO_E_WORKSPACE;
    if (!writes_clear({{grad_acid_in, vol_bytes}, {grad_quencher_in, vol_bytes}, {work, need}, {grad_step, step_bytes}},
                      {{acid_in, vol_bytes}, {grad_acid, vol_bytes}, {grad_quencher, vol_bytes}, {grad_acid_dose, vol_bytes}}))
        return LITHO_E_ARG;
    if (!run.fits) return LITHO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int nc = (steps + c - 1) / c;                   // segments; checkpoint j = (h, q) at step j c, j = 1 .. nc - 1, kept in work
    const size_t per = params ? 4 : 2;                    // tape volumes per step
    float* base = (float*)work;
    auto ck_h = [&](int j) { return base + (size_t)(2 * (j - 1)) * V; };
    auto ck_q = [&](int j) { return base + (size_t)(2 * (j - 1) + 1) * V; };
    float* tape = base + (size_t)(2 * (nc - 1)) * V;      // step i of the segment: hd at tape + per i V, qd one volume on; with
                                                          // params the state after the step in the two volumes behind them
    float* state = tape + (per * c) * V;                  // (h, q) x 2
    float* bar = state + 4 * V;                           // (hbar, qbar) x 2
    double* partials = params ? (double*)((char*)work + tape_bytes) : nullptr;
    if (params) HIP_TRY(hipMemsetAsync(partials, 0, slots * 6 * sizeof(double), st));
    const dim3 grid(plane_blocks(n, 1), (unsigned)(B * D)), block(256);
    // the forward sweep to the last checkpoint: step k writes checkpoint (k + 1) / c when k + 1 is a multiple of c
    const float *src_h = acid_in, *src_q = nullptr;
    for (int k = 0; k < (nc - 1) * c; ++k) {
        const bool keep = (k + 1) % c == 0;
        float* to_h = keep ? ck_h((k + 1) / c) : state + (size_t)(2 * (k & 1)) * V;
        float* to_q = keep ? ck_q((k + 1) / c) : to_h + V;
        hipLaunchKernelGGL(k_peb_taped, grid, block, 0, st, src_h, src_q, run.q0, to_h, to_q, (float*)nullptr, (float*)nullptr, D, n,
                           run.P);
        src_h = to_h;
        src_q = to_q;
    }
    // the segments last to first: the taped steps from the checkpoint, then their backward steps
    const float *hb = grad_acid, *qb = grad_quencher;
    int flip = 0;
    for (int j = nc - 1; j >= 0; --j) {
        const int k0 = j * c, k1 = (k0 + c < steps) ? k0 + c : steps;
        const float *seg_h = j ? ck_h(j) : acid_in, *seg_q = j ? ck_q(j) : nullptr;
        src_h = seg_h;
        src_q = seg_q;
        for (int k = k0; k < k1; ++k) {
            const bool last = k + 1 == k1;                // its new state is the next checkpoint, or of no use
            float* t = tape + (per * (k - k0)) * V;
            float* to_h = last ? nullptr : (params ? t + 2 * V : state + (size_t)(2 * ((k - k0) & 1)) * V);
            float* to_q = last ? nullptr : to_h + V;
            hipLaunchKernelGGL(k_peb_taped, grid, block, 0, st, src_h, src_q, run.q0, to_h, to_q, t, t + V, D, n, run.P);
            src_h = to_h;
            src_q = to_q;
        }
        for (int k = k1 - 1; k >= k0; --k) {
            float* to_h = k == 0 ? grad_acid_in : bar + (size_t)(2 * flip) * V;
            float* to_q = (k == 0 && grad_quencher_in) ? grad_quencher_in : bar + (size_t)(2 * flip + 1) * V;
            const float* t = tape + (per * (k - k0)) * V;
            if (params) {
                const float* at_h = k == k0 ? seg_h : t - 2 * V;           // the state at the start of step k
                const float* at_q = k == k0 ? seg_q : t - V;
                hipLaunchKernelGGL(k_peb_adjoint_params, grid, block, 0, st, hb, qb, grad_acid_dose, at_h, at_q, t, t + V, to_h, to_q,
                                   partials, D, n, run.P);
            } else {
                hipLaunchKernelGGL(k_peb_adjoint, grid, block, 0, st, hb, qb, grad_acid_dose, t, t + V, to_h, to_q, D, n, run.P);
            }
            hb = to_h;
            qb = to_q;
            flip ^= 1;
        }
    }
    if (params)
        hipLaunchKernelGGL(k_vol_total<6>, dim3((unsigned)B), block, 0, st, (const double*)partials,
                           (long long)D * (long long)plane_blocks(n, 1), grad_step);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

// d(step parameters) / d(physical parameters) of step_of's formulas at a fixed step count, in double: lxy = sigma^2 / (2 S pixel^2),
// lz = (v sigma)^2 / (2 S hz^2), beta = k_quench dt, fl = exp(-k_loss dt).  Written so that a zero length or scale gives 0, not 0 / 0.
// param_chain (physical gradient [5] from step gradient [6]) and param_tangent (its transpose) are the Jacobian's two products.
struct PebJacobian { double dxy_h, dz_h, dv_h, dxy_q, dz_q, dv_q, dt, dfl; bool instant; };
static PebJacobian step_jacobian(const PebBake& b)
{
    const double hz = b.thickness_nm / b.D, S = b.steps, dt = b.bake_time_s / b.steps, sh = b.sigma_acid_nm, sq = b.sigma_quencher_nm;
    const double pp = S * (b.pixel_nm * b.pixel_nm), zz = S * (hz * hz), vs = b.vertical_scale, vv = vs * vs / zz;
    return PebJacobian{sh / pp, vv * sh, vs * sh * sh / zz, sq / pp, vv * sq, vs * sq * sq / zz, dt, -dt * std::exp(-b.k_loss * dt),
                       std::isinf(b.k_quench)};
}
static void param_chain(const PebJacobian& J, const double* g, double* out)
{
    out[0] = J.instant ? 0.0 : g[4] * J.dt;
    out[1] = g[5] * J.dfl;
    out[2] = g[0] * J.dxy_h + g[1] * J.dz_h;
    out[3] = g[2] * J.dxy_q + g[3] * J.dz_q;
    out[4] = g[1] * J.dv_h + g[3] * J.dv_q;
}
static void param_tangent(const PebJacobian& J, const double* dp, double* out)
{
    out[0] = J.dxy_h * dp[2];
    out[1] = J.dz_h * dp[2] + J.dv_h * dp[4];
    out[2] = J.dxy_q * dp[3];
    out[3] = J.dz_q * dp[3] + J.dv_q * dp[4];
    out[4] = J.instant ? 0.0 : J.dt * dp[0];
    out[5] = J.dfl * dp[1];
}

}  // namespace litho

extern "C" {

int litho_peb_expose(const float* image, int volumes, int D, int n, const float* gains_host, int n_gains, double C, float* acid,
                     void* stream)
{
    using namespace litho;
    VolGains gains;
    if (!image || !acid || !volume_ok(volumes, D, n) || !make_gains(gains_host, n_gains, volumes, D, gains) || !finite_pos(C))
        return LITHO_E_ARG;
    const size_t in_bytes = (size_t)volumes * D * n * n * sizeof(float);
    if (!writes_clear({{acid, in_bytes * n_gains}}, {{image, in_bytes}})) return LITHO_E_ARG;
    const int planes = volumes * D;
    const bool wide = (n & 3) == 0 && aligned16(image) && aligned16(acid);
    LAUNCH_PACKED(k_peb_expose, wide, n, planes, (hipStream_t)stream, image, acid, planes, n, gains, n_gains, C);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_peb_min_steps(double sigma_acid_nm, double sigma_quencher_nm, double vertical_scale, double thickness_nm, int D,
                        double pixel_nm)
{
    return litho::min_steps(sigma_acid_nm, sigma_quencher_nm, vertical_scale, thickness_nm, D, pixel_nm);
}

size_t litho_peb_work_bytes(int B, int D, int n)
{
    using namespace litho;
    if (!volume_ok(B, D, n)) return 0;
    return 2 * (size_t)B * D * n * n * sizeof(float);
}

int litho_peb_steps_per_launch(int D)
{
    using namespace litho;
    if (D < 1 || D > VOL_DMAX) return 0;
    for (int s = PEB_SMAX; s >= 2; --s)
        if (lds_bytes(D, s) <= PEB_LDS_BUDGET) return s;
    return 1;
}

int litho_peb_bake(const float* acid_in, int B, int D, int n, double thickness_nm, double pixel_nm, double quencher0, double k_quench,
                   double k_loss, double sigma_acid_nm, double sigma_quencher_nm, double vertical_scale, double bake_time_s, int steps,
                   int steps_per_launch, float* acid, float* quencher, float* acid_dose, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    const PebBake bake = {thickness_nm, pixel_nm, quencher0, k_quench, k_loss, sigma_acid_nm, sigma_quencher_nm, vertical_scale, bake_time_s, D, steps};
    PebRun run;
    if (!acid_in || !acid || !quencher || !acid_dose || !work || !volume_ok(B, D, n) || !bake_checked(bake, true, run)) return LITHO_E_ARG;
    if (steps_per_launch < 0 || steps_per_launch > PEB_SMAX) return LITHO_E_ARG;
    const int s = steps_per_launch ? steps_per_launch : litho_peb_steps_per_launch(D);
    const size_t lds = s >= 2 ? lds_bytes(D, s) : 0;
    if (lds > PEB_LDS_MAX) return LITHO_E_ARG;
    const size_t vol_bytes = (size_t)B * D * n * n * sizeof(float), need = 2 * vol_bytes;
    if (!aligned16(work)) return LITHO_E_ARG;
    if (work_bytes < need) return LITHO_E_WORKSPACE;
    if (!writes_clear({{acid, vol_bytes}, {quencher, vol_bytes}, {acid_dose, vol_bytes}, {work, need}}, {{acid_in, vol_bytes}})) return LITHO_E_ARG;
    if (!run.fits) return LITHO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (lds > 64 * 1024) {                                // once per device; the automatic choice never gets here
        static unsigned lds_done = 0;
        HIP_TRY(lds_opt_in(lds_done, (const void*)k_peb_fused, PEB_LDS_MAX));
    }
    // launch k of L reads what launch k - 1 wrote; the last one writes the outputs, the ones before it alternate
    float* out_h[2] = {acid, (float*)work};
    float* out_q[2] = {quencher, (float*)work + (size_t)B * D * n * n};
    const int L = (steps + s - 1) / s;
    const unsigned tiles = (unsigned)((n + VOL_TILE - 1) / VOL_TILE);
    const float *src_h = acid_in, *src_q = nullptr;
    int left = steps;
    for (int k = 0; k < L; ++k) {
        const int now = left < s ? left : s, to = (L - 1 - k) & 1;
        if (now == 1)
            hipLaunchKernelGGL(k_peb_direct, dim3(plane_blocks(n, 1), (unsigned)(B * D)), dim3(256), 0, st, src_h, src_q, run.q0,
                               out_h[to], out_q[to], acid_dose, D, n, run.P);
        else
            hipLaunchKernelGGL(k_peb_fused, dim3(tiles, tiles, (unsigned)B), dim3(256), lds_bytes(D, now), st, src_h, src_q, run.q0,
                               out_h[to], out_q[to], acid_dose, D, n, now, run.P);
        src_h = out_h[to];
        src_q = out_q[to];
        left -= now;
    }
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

size_t litho_peb_vjp_work_bytes(int B, int D, int n, int steps, int checkpoint_every)
{
    using namespace litho;
    if (!vjp_shape_ok(B, D, n, steps, checkpoint_every)) return 0;
    return vjp_volumes(steps, checkpoint_every) * ((size_t)B * D * n * n * sizeof(float));
}

int litho_peb_bake_vjp(const float* acid_in, int B, int D, int n, double thickness_nm, double pixel_nm, double quencher0, double k_quench,
                       double k_loss, double sigma_acid_nm, double sigma_quencher_nm, double vertical_scale, double bake_time_s, int steps,
                       int checkpoint_every, const float* grad_acid, const float* grad_quencher, const float* grad_acid_dose,
                       float* grad_acid_in, float* grad_quencher_in, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    const PebBake bake = {thickness_nm, pixel_nm, quencher0, k_quench, k_loss, sigma_acid_nm, sigma_quencher_nm, vertical_scale, bake_time_s, D, steps};
    return bake_vjp_run(acid_in, B, n, bake, checkpoint_every, grad_acid, grad_quencher, grad_acid_dose, grad_acid_in, grad_quencher_in, nullptr,
                        false, work, work_bytes, stream);
}

size_t litho_peb_vjp_params_work_bytes(int B, int D, int n, int steps, int checkpoint_every)
{
    using namespace litho;
    if (!vjp_shape_ok(B, D, n, steps, checkpoint_every)) return 0;
    return vjp_params_tape_bytes(B, D, n, steps, checkpoint_every) + vjp_params_slots(B, D, n) * 6 * sizeof(double);
}

int litho_peb_bake_vjp_params(const float* acid_in, int B, int D, int n, double thickness_nm, double pixel_nm, double quencher0,
                              double k_quench, double k_loss, double sigma_acid_nm, double sigma_quencher_nm, double vertical_scale,
                              double bake_time_s, int steps, int checkpoint_every, const float* grad_acid, const float* grad_quencher,
                              const float* grad_acid_dose, float* grad_acid_in, float* grad_quencher_in, double* grad_step, void* work,
                              size_t work_bytes, void* stream)
{
    using namespace litho;
    const PebBake bake = {thickness_nm, pixel_nm, quencher0, k_quench, k_loss, sigma_acid_nm, sigma_quencher_nm, vertical_scale, bake_time_s, D, steps};
    return bake_vjp_run(acid_in, B, n, bake, checkpoint_every, grad_acid, grad_quencher, grad_acid_dose, grad_acid_in, grad_quencher_in, grad_step,
                        true, work, work_bytes, stream);
}

int litho_peb_param_chain(double thickness_nm, double pixel_nm, double k_quench, double k_loss, double sigma_acid_nm,
                          double sigma_quencher_nm, double vertical_scale, double bake_time_s, int D, int steps, const double* grad_step,
                          double* grad_param)
{
    using namespace litho;
    const PebBake bake = {thickness_nm, pixel_nm, 0.0, k_quench, k_loss, sigma_acid_nm, sigma_quencher_nm, vertical_scale, bake_time_s, D, steps};
    PebRun run;                                           // not looked at: no kernel runs
    if (!grad_step || !grad_param || !finite_pos(pixel_nm) || !bake_checked(bake, false, run)) return LITHO_E_ARG;
    param_chain(step_jacobian(bake), grad_step, grad_param);
    return LITHO_OK;
}

int litho_peb_expose_vjp(const float* image, int volumes, int D, int n, const float* gains_host, int n_gains, double C,
                         const float* grad_acid, float* grad_image, void* stream)
{
    using namespace litho;
    VolGains gains;
    if (!image || !grad_acid || !grad_image || !volume_ok(volumes, D, n) || !make_gains(gains_host, n_gains, volumes, D, gains) ||
        !finite_pos(C))
        return LITHO_E_ARG;
    const size_t in_bytes = (size_t)volumes * D * n * n * sizeof(float);
    if (!writes_clear({{grad_image, in_bytes}}, {{image, in_bytes}, {grad_acid, in_bytes * n_gains}})) return LITHO_E_ARG;
    const int planes = volumes * D;
    const bool wide = (n & 3) == 0 && aligned16(image) && aligned16(grad_acid) && aligned16(grad_image);
    LAUNCH_PACKED(k_peb_expose_vjp, wide, n, planes, (hipStream_t)stream, image, grad_acid, grad_image, planes, n, gains, n_gains, C);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

size_t litho_peb_expose_params_work_bytes(int volumes, int D, int n, int n_gains)
{
    using namespace litho;
    if (!volume_ok(volumes, D, n) || n_gains < 1 || n_gains > VOL_GAINS || (long long)volumes * n_gains * D > 65535) return 0;
    return (size_t)n_gains * volumes * D * plane_blocks(n, 1) * sizeof(double);
}

int litho_peb_expose_vjp_params(const float* image, int volumes, int D, int n, const float* gains_host, int n_gains, double C,
                                const float* grad_acid, double* grad_C, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    VolGains gains;
    if (!image || !grad_acid || !grad_C || !work || !volume_ok(volumes, D, n) || !make_gains(gains_host, n_gains, volumes, D, gains) ||
        !finite_pos(C))
        return LITHO_E_ARG;
    if (!aligned16(work) || !aligned16(grad_C)) return LITHO_E_ARG;
    const size_t need = litho_peb_expose_params_work_bytes(volumes, D, n, n_gains);
    if (work_bytes < need) return LITHO_E_WORKSPACE;
    const size_t in_bytes = (size_t)volumes * D * n * n * sizeof(float), out_bytes = (size_t)n_gains * volumes * sizeof(double);
    if (!writes_clear({{grad_C, out_bytes}, {work, need}}, {{image, in_bytes}, {grad_acid, in_bytes * n_gains}})) return LITHO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int planes = volumes * D;
    const unsigned blocks = plane_blocks(n, 1);
    hipLaunchKernelGGL(k_peb_expose_params, dim3(blocks, (unsigned)(n_gains * planes)), dim3(256), 0, st, image, grad_acid, (double*)work,
                       planes, n, gains, C);
    hipLaunchKernelGGL(k_vol_total<1>, dim3((unsigned)(n_gains * volumes)), dim3(256), 0, st, (const double*)work,
                       (long long)D * (long long)blocks, grad_C);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_peb_expose_jvp(const float* image, int volumes, int D, int n, const float* gains_host, int n_gains, double C, int P,
                         const double* dC_host, const float* dimage, float* dacid, void* stream)
{
    using namespace litho;
    VolGains gains;
    if (!image || !dacid || !dC_host || P < 1 || P > TAN_MAX || !volume_ok(volumes, D, n) ||
        !make_gains(gains_host, n_gains, volumes, D, gains) || !finite_pos(C) || (long long)P * n_gains * volumes * D > 65535)
        return LITHO_E_ARG;
    TanScalars dC;
    memset(&dC, 0, sizeof(dC));
    for (int p = 0; p < P; ++p) {
        if (!std::isfinite(dC_host[p])) return LITHO_E_ARG;
        dC.v[p] = dC_host[p];
    }
    const size_t in_bytes = (size_t)volumes * D * n * n * sizeof(float), out_bytes = in_bytes * n_gains * P;
    if (!writes_clear({{dacid, out_bytes}}, {{image, in_bytes}, {dimage, in_bytes * P}})) return LITHO_E_ARG;
    const int planes = volumes * D;
    const bool wide = (n & 3) == 0 && aligned16(image) && aligned16(dimage) && aligned16(dacid);
    LAUNCH_PACKED(k_peb_expose_jvp, wide, n, planes, (hipStream_t)stream, image, dimage, dacid, planes, n, gains, n_gains, C, P, dC);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

size_t litho_peb_jvp_work_bytes(int B, int D, int n, int P)
{
    using namespace litho;
    if (!volume_ok(B, D, n) || P < 1 || P > TAN_MAX || (long long)P * B * D > 65535) return 0;
    return (5 + 2 * (size_t)P) * ((size_t)B * D * n * n * sizeof(float));
}

int litho_peb_bake_jvp(const float* acid_in, int B, int D, int n, double thickness_nm, double pixel_nm, double quencher0, double k_quench,
                       double k_loss, double sigma_acid_nm, double sigma_quencher_nm, double vertical_scale, double bake_time_s, int steps,
                       int P, const float* dacid_in, const double* dquencher0_host, const double* dstep_host, float* acid, float* quencher,
                       float* acid_dose, float* dacid, float* dquencher, float* dacid_dose, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    const PebBake bake = {thickness_nm, pixel_nm, quencher0, k_quench, k_loss, sigma_acid_nm, sigma_quencher_nm, vertical_scale, bake_time_s, D, steps};
    PebRun run;
    if (!acid_in || !dquencher0_host || !dstep_host || !dacid || !dquencher || !dacid_dose || !work || !volume_ok(B, D, n)) return LITHO_E_ARG;
    if (P < 1 || P > TAN_MAX || (long long)P * B * D > 65535 || !bake_checked(bake, true, run)) return LITHO_E_ARG;
    PebTanStep T;
    memset(&T, 0, sizeof(T));
    for (int p = 0; p < P; ++p) {
        if (!std::isfinite(dquencher0_host[p])) return LITHO_E_ARG;
        T.dq0[p] = (float)dquencher0_host[p];
        for (int j = 0; j < 6; ++j) {
            if (!std::isfinite(dstep_host[p * 6 + j])) return LITHO_E_ARG;
            T.d[p][j] = (float)dstep_host[p * 6 + j];
        }
    }
    const size_t V = (size_t)B * D * n * n, vol_bytes = V * sizeof(float), need = (5 + 2 * (size_t)P) * vol_bytes;
    if (!aligned16(work)) return LITHO_E_ARG;
    if (work_bytes < need) return LITHO_E_WORKSPACE;
    const size_t tan_bytes = P * vol_bytes;
    if (!writes_clear({{acid, vol_bytes}, {quencher, vol_bytes}, {acid_dose, vol_bytes}, {dacid, tan_bytes}, {dquencher, tan_bytes},
                       {dacid_dose, tan_bytes}, {work, need}},
                      {{acid_in, vol_bytes}, {dacid_in, tan_bytes}}))
        return LITHO_E_ARG;
    if (!run.fits) return LITHO_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    // the primal pair ping-pongs between two sides of the workspace, a lives in its fifth volume; the last step writes the
    // outputs that were asked for.  The tangent pairs ping-pong between the outputs and the workspace, the last step to the
    // outputs; da is updated in place in its output.
    float* base = (float*)work;
    float* ph[2] = {base, base + 2 * V};
    float* pa = acid_dose ? acid_dose : base + 4 * V;
    float* th[2] = {dacid, base + 5 * V};
    float* tq[2] = {dquencher, base + (5 + (size_t)P) * V};
    const dim3 grid(plane_blocks(n, 1), (unsigned)(B * D)), block(256);
    const float *src_h = acid_in, *src_q = nullptr, *src_dh = dacid_in, *src_dq = nullptr;
    for (int k = 0; k < steps; ++k) {
        const int to = (steps - 1 - k) & 1;
        const bool last = k + 1 == steps;
        float* to_h = (last && acid) ? acid : ph[k & 1];
        float* to_q = (last && quencher) ? quencher : ph[k & 1] + V;
        hipLaunchKernelGGL(k_peb_jvp, grid, block, 0, st, src_h, src_q, run.q0, to_h, to_q, pa, src_dh, src_dq, th[to], tq[to], dacid_dose,
                           V, D, n, P, run.P, T);
        src_h = to_h;
        src_q = to_q;
        src_dh = th[to];
        src_dq = tq[to];
    }
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_peb_param_tangent(double thickness_nm, double pixel_nm, double k_quench, double k_loss, double sigma_acid_nm,
                            double sigma_quencher_nm, double vertical_scale, double bake_time_s, int D, int steps, const double* dparam,
                            double* dstep)
{
    using namespace litho;
    const PebBake bake = {thickness_nm, pixel_nm, 0.0, k_quench, k_loss, sigma_acid_nm, sigma_quencher_nm, vertical_scale, bake_time_s, D, steps};
    PebRun run;                                           // not looked at: no kernel runs
    if (!dparam || !dstep || !finite_pos(pixel_nm) || !bake_checked(bake, false, run)) return LITHO_E_ARG;
    param_tangent(step_jacobian(bake), dparam, dstep);
    return LITHO_OK;
}

int litho_peb_rate(const float* acid_dose, int B, int D, int n, double k_amp, double r_max, double r_min, double q, double m_th,
                   double surface_rate, double surface_depth_nm, double thickness_nm, float* slowness, float* inhibitor, void* stream)
{
    using namespace litho;
    MackLaw law;
    if (!acid_dose || !slowness || !volume_ok(B, D, n) || !finite_pos(k_amp) ||
        !make_mack(r_max, r_min, q, m_th, surface_rate, surface_depth_nm, thickness_nm, D, law))
        return LITHO_E_ARG;
    const size_t bytes = (size_t)B * D * n * n * sizeof(float);
    if (!writes_clear({{slowness, bytes}, {inhibitor, bytes}}, {{acid_dose, bytes}})) return LITHO_E_ARG;
    const bool wide = (n & 3) == 0 && aligned16(acid_dose) && aligned16(slowness) && aligned16(inhibitor);
    LAUNCH_PACKED(k_peb_rate, wide, n, B * D, (hipStream_t)stream, acid_dose, slowness, inhibitor, D, n, k_amp, law.rmax_a1, law.rmin, law.q,
                  law.a, law.surface);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

}  // extern "C"
