// socs_grad.hip -- mask gradients of Hopkins imaging: the K coherent fields of one mask spectrum and the adjoint (vector-Jacobian
// product) of I = sum_k |E_k|^2 with respect to the mask spectrum.
//
//   E_k = L(phi_k . M),   L(X) = F X F^T,   F[q][i] = exp(+2 pi i (i - c)(q - c) / N),  c = pn / 2,  q, i in [0, pn)
//   g   = 2 sum_p sum_k conj(phi_pk) . L^H(G_p . E_pk),   L^H(Y) = conj(F) Y conj(F)^T          (include/litho_abbe.h)
//
// L is the engine's chain at shift (0, 0) (imageformation.py:32-45: pad to N, centred inverse transform, centre pn x pn); the
// engine keeps |E|^2 only, so the fields are formed here, by a route that never holds an N^2 array and runs no line longer than
// pn.  Along one axis, with m = N / pn and q - c = m t + r, 0 <= r < m,
//   y[c + m t + r] = sum_i (x[i] w_N^((i - c) r)) w_pn^((i - c) t):
// m centred pn-point transforms of the pre-modulated line, the r-th one giving the outputs q = c + r (mod m).  The line is loaded
// once, kept in registers, and pn outputs are written; m = 1 is one centred transform.  L^H is the same code with the other sign.
//
// Layout as socs.hip: rows, tiled transpose, rows, tiled transpose -- every global access of a row pass is a contiguous line
// (thread t of a line owns samples t + T e, fft_core.hpp); the twiddle table, the line geometry, the transpose and the dispatch on
// the line size are plane_fft.hpp's, shared with socs.hip.  The elementwise products of both directions ride on the first row
// pass's load (phi . M on the way in, G . E on the way back), the reduction over the batch is one running fp32 sum per element
// in ascending item order: no atomics, so the result is deterministic and a chunked call gives the chunk-ordered sum.
// No reference counterpart; checked against tests/socs_grad_oracle.py.
//
// Source sensitivities (litho_source_sensitivity) are the same field code with two other ends: a source point is the coherent
// kernel roll(P, d_s), so the first row pass reads the one pupil plane rolled (LOAD_ROLLED) instead of a stored kernel, and the
// second row pass reduces G^T . |E|^2 over its line (STORE_REDUCE) instead of writing the field; a small kernel sums a point's
// line partials.  Every sum has one fixed order and nothing is atomic, so a point's number depends on that point alone.
// Checked against tests/source_grad_oracle.py.
//
// Pupil gradients (litho_pupil_vjp) join the two: the rolled load with the stored field (the field in natural layout), the
// adjoint transform of the mask-gradient path with the G of the item's plane, and a reducing pass that undoes each point's roll
// and sums the points in list order (k_pupil_reduce); litho_pupil_project pairs the result with a basis of wavefront maps in a
// two-stage reduction of fixed order.  Checked against tests/pupil_grad_oracle.py.
//
// The tangent of the image (litho_socs_jvp) is forward mode through the same fields: dI = 2 sum_k Re(conj(E_k) . L(phi_k . dM)).
// A direction's first row pass is the fields' own (the kernel times a plane on the load -- the plane is dM instead of M); its second
// row pass folds each output against the stored field as it comes out (STORE_FOLD), so a tangent field is never stored.
// Checked against tests/socs_tangent_oracle.py.
//
// The image of a batch of mask spectra (litho_socs_image_batch) is the same two row passes with two other ends: the first reads
// kernel plane and mask plane per item (LOAD_BATCH), the second adds |E|^2 over a group's K items into the running sums that
// STORE_FOLD keeps (STORE_SQUARE), so the K fields of a tile meet in LDS and no K-plane stack of intensities is written.
// Checked against tests/socs_oracle.py (kernel_image).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/litho_abbe.h"
#include "engine_common.hpp"
#include "plane_fft.hpp"

namespace litho {

// What the row pass multiplies into the line as it loads it.
enum : int { LOAD_PLAIN = 0, LOAD_TIMES_MASK = 1, LOAD_TIMES_GRAD = 2, LOAD_ROLLED = 3, LOAD_BATCH = 4 };
// What it does with the outputs: writes them, reduces mul_r . |y|^2 over the line to one number, folds them against a stored
// field into a running real sum over the K items of a group (the tangent of the image, litho_socs_jvp), or sums their squared
// moduli over the K items of a group (the image itself, litho_socs_image_batch).
enum : int { STORE_FIELD = 0, STORE_REDUCE = 1, STORE_FOLD = 2, STORE_SQUARE = 3 };

// `lines` lines of pn = 2^LOG2P samples, line l = row (l mod pn) of item (l / pn); each becomes its centred pruned transform
//   dst[q] = sum_i src[i] exp(SIGN 2 pi i (i - c)(q - c) / N),  q in [0, pn),  N = pn << log2m.
// LOAD_TIMES_MASK: src[i] is first multiplied by mul_c[row][i] (complex [pn][pn], the same for every item);
// LOAD_TIMES_GRAD: by mul_r[(item mod per_point) / per_group][row][i] (real; per_point = the batch for litho_socs_vjp, whose items
// are the planes themselves, groups K for the point-major chunks of litho_pupil_vjp).  dst may BE src: a line is in registers
// before any of its outputs is written (every write follows a barrier that the line's threads reach with their loads consumed; a 16-point line has one
// thread), and no workgroup touches another's lines.
// LOAD_ROLLED: item b is plane (b mod per_point) of source point (b / per_point); src holds the per_point planes once and
//   src[i] = plane[(row - dy) mod pn][(i - dx) mod pn] . mul_c[row][i],  (dy, dx) = shifts[point], read once per line.
// STORE_REDUCE: nothing is written to dst; partial[line] = sum_q mul_r[(item mod per_point) / per_group][row][q] |dst[q]|^2, each
// thread over the outputs it owns (r ascending, then e), then the line's threads in a fixed order: the xor butterfly of a wave's
// shuffles, every lane ending with the same bits, and for a line of several waves their sums through LDS, added in wave order.
// STORE_FOLD: `lines` counts the lines of the GROUPS, line l = row (l mod pn) of group (l / pn), and the workgroup walks the
//   per_group = K items of its group in ascending order: item g K + k's line is transformed and
//   partial[l][q] += 2 Re(conj(mul_c[g K + k][row][q]) . dst[q])
// (mul_c: the stored fields, one plane per item; nothing is written to dst).  The running sums of a line live in LDS, fp32, one
// per output q, touched by the one thread that owns q and by nobody else between the two barriers around the loop; they start
// from partial[l] when per_point != 0 (the accumulate flag of this mode) and from zero otherwise.  One sum per element in item
// order, no atomics.
// LOAD_BATCH: many mask spectra through one kernel set.  Item b is kernel plane (b mod per_point) under mask plane (b / per_point):
//   src[i] = src_planes[b mod per_point][row][i] . mul_c[b / per_point][row][i]
// (src holds the per_point = groups K kernel planes once, mul_c one plane per tile; dst is the item's own plane, never src).
// STORE_SQUARE: STORE_FOLD's walk and LDS layout with another term: item g K + k's line adds
//   partial[l][q] += fmaf(dst[q].re, dst[q].re, dst[q].im dst[q].im)
// -- the image of group l / pn, nothing read besides the line.  per_point != 0 is again the accumulate flag.
template <int LOG2P, int SIGN, int LOAD, int STORE = STORE_FIELD>
__global__ __launch_bounds__(LineShape<LOG2P>::THREADS) void k_centred_rows(const float2* src, float2* dst,
                                                                            const float2* __restrict__ mul_c,
                                                                            const float* __restrict__ mul_r, int per_group,
                                                                            long long lines, int log2m,
                                                                            const int32_t* __restrict__ shifts, int per_point,
                                                                            float* __restrict__ partial)
{
    using F = LineFFT<LOG2P, SIGN>;
    using LS = LineShape<LOG2P>;
    constexpr int PN = F::N, C = PN / 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2* smem = reinterpret_cast<float2*>(smem_raw);
    const int lt = threadIdx.x % F::T, lg = threadIdx.x / F::T;
    float2* lds = smem + (size_t)lg * F::LDS_LINE;
    typename F::Twiddles tw;
    F::load_twiddles(tw, g_twiddles, lt, smem + LS::LDS_EXCH, threadIdx.x, LS::THREADS, FFT_MAX_N / PN);
    const long long line = (long long)blockIdx.x * LS::L + lg;
    const bool active = line < lines;                       // every thread runs the transforms: they hold workgroup barriers
    float* sums_all = reinterpret_cast<float*>(smem + LS::LDS_EXCH + F::LDS_TW);   // STORE_FOLD: L lines of PN running sums
    float* sums = sums_all + (size_t)lg * PN;
    const long long fold_base = (long long)blockIdx.x * LS::L * PN, fold_end = lines * PN;
    if (STORE == STORE_FOLD) {
        for (int i = threadIdx.x; i < LS::L * PN; i += LS::THREADS)
            sums_all[i] = (per_point != 0 && fold_base + i < fold_end) ? partial[fold_base + i] : 0.f;
        __syncthreads();
    }
    if (STORE == STORE_SQUARE) {
        for (int i = threadIdx.x; i < LS::L * PN; i += LS::THREADS)
            sums_all[i] = (per_point != 0 && fold_base + i < fold_end) ? partial[fold_base + i] : 0.f;
        __syncthreads();
    }
    const int items = (STORE == STORE_FOLD || STORE == STORE_SQUARE) ? per_group : 1;
    for (int item_k = 0; item_k < items; ++item_k) {
        long long l = active ? line : 0;
        const int row = (int)(l & (PN - 1));
        if (STORE == STORE_FOLD) l = ((((l >> LOG2P) * per_group) + item_k) << LOG2P) + row;
        if (STORE == STORE_SQUARE) l = ((((l >> LOG2P) * per_group) + item_k) << LOG2P) + row;
        const float2* in = src + (size_t)l * PN;
        float2* out = dst + (size_t)l * PN;
        const float2* fold = mul_c + (size_t)l * PN;             // STORE_FOLD only
        const float2* tile_m = mul_c;                            // LOAD_BATCH only: the item's mask plane
        if (LOAD == LOAD_BATCH) {
            const long long item = l >> LOG2P, tile = item / per_point;
            in = src + ((size_t)(item - tile * per_point) * PN + row) * PN;
            tile_m = mul_c + (size_t)tile * PN * PN;
        }
        unsigned dx = 0;
        if (LOAD == LOAD_ROLLED) {
            const long long item = l >> LOG2P, point = item / per_point;
            const unsigned dy = (unsigned)shifts[2 * point];    // unsigned: the modular index of any integer, no overflow
            dx = (unsigned)shifts[2 * point + 1];
            in = src + ((size_t)(item - point * per_point) * PN + (((unsigned)row - dy) & (PN - 1))) * PN;
        }
        // transform index n = lt + T e stands for the sample at signed offset s = n (n < c) or n - pn from the centre: i = s + c
        float2 x0[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int n = lt + F::T * e;
            const int i = (n + C) & (PN - 1);
            float2 v = make_float2(0.f, 0.f);
            if (active) {
                v = LOAD == LOAD_ROLLED ? in[((unsigned)i - dx) & (PN - 1)] : in[i];
                if (LOAD == LOAD_TIMES_MASK || LOAD == LOAD_ROLLED) v = cmul(v, mul_c[(size_t)row * PN + i]);
                if (LOAD == LOAD_BATCH) v = cmul(v, tile_m[(size_t)row * PN + i]);
                if (LOAD == LOAD_TIMES_GRAD) {
                    const float g = mul_r[((size_t)((l >> LOG2P) % per_point / per_group) * PN + row) * PN + i];
                    v = make_float2(v.x * g, v.y * g);
                }
            }
            x0[e] = v;
        }
        const int m = 1 << log2m;
        const int nmask = (PN << log2m) - 1;                   // N - 1
        const int tshift = 12 - LOG2P - log2m;                 // table stride 4096 / N
        int flip = 0;
        float acc = 0.f;
        const float* gt = mul_r;
        if (STORE == STORE_REDUCE) gt = mul_r + ((size_t)((l >> LOG2P) % per_point / per_group) * PN + row) * PN;
        for (int r = 0; r < m; ++r) {
            if (m > PN && r >= C && r < m - C) continue;       // no q in [0, pn) is congruent to c + r (uniform over the workgroup)
            float2 x[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = lt + F::T * e;
                const int s = n < C ? n : n - PN;
                float2 w = g_twiddles[((s * r) & nmask) << tshift];
                if (SIGN < 0) w.y = -w.y;
                x[e] = r == 0 ? x0[e] : cmul(x0[e], w);
            }
            F::template run<1>(x, tw, lds, lt, flip);
            if (!active) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int u = lt + F::T * e;
                const int t = u < C ? u : u - PN;
                const int q = C + (t << log2m) + r;
                if (q >= 0 && q < PN) {
                    if (STORE == STORE_REDUCE) acc = fmaf(gt[q], fmaf(x[e].x, x[e].x, x[e].y * x[e].y), acc);
                    else if (STORE == STORE_FOLD) {
                        const float2 ev = fold[q];
                        sums[q] += 2.0f * fmaf(ev.x, x[e].x, ev.y * x[e].y);
                    } else if (STORE == STORE_SQUARE) sums[q] += fmaf(x[e].x, x[e].x, x[e].y * x[e].y);
                    else out[q] = x[e];
                }
            }
        }
        if (STORE == STORE_REDUCE) {
            constexpr int W = F::T < 64 ? F::T : 64;           // the line's lanes within one wave: an aligned group of W
#pragma unroll
            for (int o = W / 2; o >= 1; o /= 2) acc += __shfl_xor(acc, o);
            if (F::T > 64) {                                   // one line per workgroup, T / 64 waves
                float* red = reinterpret_cast<float*>(smem);   // the exchange buffer, free once every thread has left the transforms
                __syncthreads();
                if ((lt & 63) == 0) red[lt >> 6] = acc;
                __syncthreads();
                acc = red[0];
                for (int w = 1; w < F::T / 64; ++w) acc += red[w];
            }
            if (active && lt == 0) partial[l] = acc;
        }
    }
    if (STORE == STORE_FOLD) {
        __syncthreads();
        for (int i = threadIdx.x; i < LS::L * PN; i += LS::THREADS)
            if (fold_base + i < fold_end) partial[fold_base + i] = sums_all[i];
    }
    if (STORE == STORE_SQUARE) {
        __syncthreads();
        for (int i = threadIdx.x; i < LS::L * PN; i += LS::THREADS)
            if (fold_base + i < fold_end) partial[fold_base + i] = sums_all[i];
    }
}

// out[g][c][r] = in[g][r][c] for `gridDim.z` real n x n planes, through a 32 x 32 LDS tile: the copy of gradI whose lines the
// reducing row pass reads contiguously.
__global__ __launch_bounds__(256) void k_transpose_real(const float* __restrict__ in, float* __restrict__ out, int n)
{
    __shared__ float tile[TR_TILE][TR_TILE + 1];
    const size_t plane = (size_t)blockIdx.z * n * n;
    const int tx = threadIdx.x % TR_TILE, ty = threadIdx.x / TR_TILE;
    for (int r = ty; r < TR_TILE; r += 256 / TR_TILE) {
        const int ri = blockIdx.y * TR_TILE + r, ci = blockIdx.x * TR_TILE + tx;
        if (ri < n && ci < n) tile[r][tx] = in[plane + (size_t)ri * n + ci];
    }
    __syncthreads();
    for (int r = ty; r < TR_TILE; r += 256 / TR_TILE) {
        const int ro = blockIdx.x * TR_TILE + r, co = blockIdx.y * TR_TILE + tx;
        if (ro < n && co < n) out[plane + (size_t)ro * n + co] = tile[tx][r];
    }
}

// sens[p] = sum of the `n` line partials of point p: one wave per point, lane t over t, t + 64, ... ascending, then the xor
// butterfly.  n is a multiple of 16.
__global__ __launch_bounds__(64) void k_sum_partials(const float* __restrict__ partial, int n, float* __restrict__ sens)
{
    const float* p = partial + (size_t)blockIdx.x * n;
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) acc += p[i];
#pragma unroll
    for (int o = 32; o >= 1; o /= 2) acc += __shfl_xor(acc, o);
    if (threadIdx.x == 0) sens[blockIdx.x] = acc;
}

// grad[i] (+)= sum_b 2 conj(kernels[b][i]) adj[b][i], b ascending, one running fp32 sum per component.  Bandwidth-bound: two
// complex elements per thread in one 16-byte access (float4c, plane_fft.hpp); cells is even.
__global__ __launch_bounds__(256) void k_vjp_reduce(const float2* __restrict__ kernels, const float2* __restrict__ adj, int batch,
                                                    long long cells, float2* __restrict__ grad, int accumulate)
{
    const long long pairs = cells / 2;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pairs; p += (long long)gridDim.x * 256) {
        float4c acc = {0.f, 0.f, 0.f, 0.f};
        if (accumulate) acc = *reinterpret_cast<const float4c*>(grad + 2 * p);
        for (int b = 0; b < batch; ++b) {
            const float4c k = *reinterpret_cast<const float4c*>(kernels + (size_t)b * cells + 2 * p);
            const float4c a = *reinterpret_cast<const float4c*>(adj + (size_t)b * cells + 2 * p);
            float4c term;
            term.x = 2.0f * (k.x * a.x + k.y * a.y);
            term.y = 2.0f * (k.x * a.y - k.y * a.x);
            term.z = 2.0f * (k.z * a.z + k.w * a.w);
            term.w = 2.0f * (k.z * a.w - k.w * a.z);
            acc += term;
        }
        *reinterpret_cast<float4c*>(grad + 2 * p) = acc;
    }
}

// The reducing pass of litho_pupil_vjp.  adj holds the chunk's adjoints A[p][j] = L^H(G . E) in the mask frame, item p per_point + j;
//   grad[j][r][c] (+)= sum_p 2 w_p conj(M[r'][c']) A[p][j][r'][c'],   r' = (r + dy_p) mod pn,  c' = (c + dx_p) mod pn,
// p ascending: the roll undone per point, as unsigned modular indices (any integer shift, no overflow).  One thread per cell and
// plane keeps the running fp32 sum; each term is added as
//   re = fma(2 w, fma(M.re, A.re, M.im A.im), re),   im = fma(2 w, fma(M.re, A.im, -(M.im A.re)), im)
// (w = 1 without weights), so the additions into a cell are the list's, whatever chunk a point falls into: a chunk that starts
// from grad (`accumulate`) continues the same sequence, an fp32 store and load changing nothing.  A gather: the reads of one
// point are a rolled copy of the thread order, contiguous except at the wrap.  cells = pn^2 is a multiple of 256.
__global__ __launch_bounds__(256) void k_pupil_reduce(const float2* __restrict__ adj, const float2* __restrict__ M,
                                                      const int32_t* __restrict__ shifts, const float* __restrict__ weights, int points,
                                                      int per_point, int log2pn, float2* __restrict__ grad, int accumulate)
{
    const unsigned pn = 1u << log2pn, wrap = pn - 1;
    const size_t cells = (size_t)pn << log2pn;
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    const unsigned r = (unsigned)(cell >> log2pn), c = (unsigned)cell & wrap;
    for (int j = blockIdx.y; j < per_point; j += gridDim.y) {
        float2* g = grad + (size_t)j * cells + cell;
        float2 acc = accumulate ? *g : make_float2(0.f, 0.f);
        for (int p = 0; p < points; ++p) {
            const unsigned dy = (unsigned)shifts[2 * p], dx = (unsigned)shifts[2 * p + 1];
            const size_t at = ((size_t)((r + dy) & wrap) << log2pn) | ((c + dx) & wrap);
            const float2 a = adj[((size_t)p * per_point + j) * cells + at];
            const float2 m = M[at];
            const float tw = weights ? 2.0f * weights[p] : 2.0f;
            acc.x = fmaf(tw, fmaf(m.x, a.x, m.y * a.y), acc.x);
            acc.y = fmaf(tw, fmaf(m.x, a.y, -(m.y * a.x)), acc.y);
        }
        *g = acc;
    }
}

// litho_pupil_project, stage 1: workgroup (x, y) sums d . basis_j for the PROJ_JT terms j = y PROJ_JT ... over its grid-stride share
// of the planes' cells, d = 2 pi Im(grad conj(P)) = 2 pi (g.im P.re - g.re P.im).  grad and the pupils are read once per tile of
// PROJ_JT terms, two cells per thread and access; each thread adds its cells in ascending order, the lanes of a wave meet in the
// xor butterfly, the four waves through LDS in wave order.  partial[x][j]; nothing is atomic.
static constexpr int PROJ_JT = 16;
static constexpr int PROJ_MAX_BLOCKS = 1024;
typedef float float2u __attribute__((ext_vector_type(2), aligned(4)));     // two fp32 of a 4-byte aligned array in one access

__global__ __launch_bounds__(256) void k_project_partial(const float2* __restrict__ grad, const float2* __restrict__ pupils,
                                                         const float* __restrict__ basis, int J, long long cells, long long pairs,
                                                         float* __restrict__ partial)
{
    constexpr float TWO_PI = 6.28318530717958647692f;
    const int j0 = blockIdx.y * PROJ_JT;
    const int nj = J - j0 < PROJ_JT ? J - j0 : PROJ_JT;
    float acc[PROJ_JT];
#pragma unroll
    for (int t = 0; t < PROJ_JT; ++t) acc[t] = 0.f;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < pairs; q += (long long)gridDim.x * 256) {
        const long long e = 2 * q, cell = e & (cells - 1);                 // cells is a power of two: the basis is shared by the planes
        const float4c g = *reinterpret_cast<const float4c*>(grad + e);
        const float4c p = *reinterpret_cast<const float4c*>(pupils + e);
        const float d0 = TWO_PI * fmaf(g.y, p.x, -(g.x * p.y));
        const float d1 = TWO_PI * fmaf(g.w, p.z, -(g.z * p.w));
#pragma unroll
        for (int t = 0; t < PROJ_JT; ++t) {
            if (t < nj) {
                const float2u b = *reinterpret_cast<const float2u*>(basis + (size_t)(j0 + t) * cells + cell);
                acc[t] = fmaf(d1, b.y, fmaf(d0, b.x, acc[t]));
            }
        }
    }
    __shared__ float red[4][PROJ_JT];
#pragma unroll
    for (int t = 0; t < PROJ_JT; ++t) {
#pragma unroll
        for (int o = 32; o >= 1; o /= 2) acc[t] += __shfl_xor(acc[t], o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][t] = acc[t];
    }
    __syncthreads();
    if ((int)threadIdx.x < nj)
        partial[(size_t)blockIdx.x * J + j0 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// stage 2: out[j] = the sum of the `blocks` partials of term j: one wave per term, lane t over t, t + 64, ... ascending, then the
// xor butterfly.
__global__ __launch_bounds__(64) void k_project_final(const float* __restrict__ partial, int blocks, int J, float* __restrict__ out)
{
    float acc = 0.f;
    for (int b = threadIdx.x; b < blocks; b += 64) acc += partial[(size_t)b * J + blockIdx.x];
#pragma unroll
    for (int o = 32; o >= 1; o /= 2) acc += __shfl_xor(acc, o);
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

struct RowArgs {
    const float2* src;
    float2* dst;
    const float2* mul_c;
    const float* mul_r;
    int per_group;
    long long lines;
    int log2m;
    const int32_t* shifts = nullptr;                       // LOAD_ROLLED / STORE_REDUCE only
    int per_point = 1;
    float* partial = nullptr;
};

template <int LOAD, int STORE = STORE_FIELD>
static hipError_t centred_rows(const RowArgs& a, int pn, int sign, hipStream_t st)
{
    return for_log2(log2_exact(pn), [&](auto l2) {
        constexpr int LOG2P = decltype(l2)::value;
        using LS = LineShape<LOG2P>;
        // STORE_FOLD and STORE_SQUARE keep the running sums of their L lines behind the exchange buffers and the twiddle tables
        constexpr size_t LDS =
            LS::LDS_BYTES + ((STORE == STORE_FOLD || STORE == STORE_SQUARE) ? sizeof(float) * LS::L * (size_t(1) << LOG2P) : 0);
        static_assert(LDS <= 64 * 1024, "the row pass stays inside the default LDS allowance");
        if (sign > 0)
            hipLaunchKernelGGL((k_centred_rows<LOG2P, +1, LOAD, STORE>), LS::grid(a.lines), dim3(LS::THREADS), LDS, st, a.src,
                               a.dst, a.mul_c, a.mul_r, a.per_group, a.lines, a.log2m, a.shifts, a.per_point, a.partial);
        else
            hipLaunchKernelGGL((k_centred_rows<LOG2P, -1, LOAD, STORE>), LS::grid(a.lines), dim3(LS::THREADS), LDS, st, a.src,
                               a.dst, a.mul_c, a.mul_r, a.per_group, a.lines, a.log2m, a.shifts, a.per_point, a.partial);
        return hipGetLastError();
    });
}

// data <- L(first-pass product) for sign +1, L^H for sign -1: rows (with the product on the load), transpose, rows, transpose.
// The `batch` items are `per_point` planes per source point, point-major (LOAD_ROLLED reads shifts[point]; LOAD_TIMES_GRAD takes
// the plane's G); a plain batch of planes is one point of `batch` planes.
template <int LOAD>
static hipError_t centred2d(const float2* src, float2* data, const float2* mul_c, const float* mul_r, int per_group, int batch, int pn,
                            int log2m, int sign, hipStream_t st, int per_point, const int32_t* shifts = nullptr)
{
    const long long lines = (long long)batch * pn;
    hipError_t e = centred_rows<LOAD>(RowArgs{src, data, mul_c, mul_r, per_group, lines, log2m, shifts, per_point}, pn, sign, st);
    if (e != hipSuccess) return e;
    e = transpose(data, batch, pn, st);
    if (e != hipSuccess) return e;
    e = centred_rows<LOAD_PLAIN>(RowArgs{data, data, nullptr, nullptr, 1, lines, log2m}, pn, sign, st);
    if (e != hipSuccess) return e;
    return transpose(data, batch, pn, st);
}

// LITHO_OK, or the code of the first size rule broken (litho_fft2_c2c's domain for pn and for N, then N >= pn).
static int check_sizes(long long batch, int pn, int N)
{
    if (batch < 1 || !fft_size_ok(pn) || !fft_size_ok(N)) return LITHO_E_ARG;
    if (N < pn) return LITHO_E_NSMALL;
    if (batch * pn > INT_MAX) return LITHO_E_ARG;                   // one workgroup per line at the large sizes
    return LITHO_OK;
}

// The three parts of litho_source_sensitivity's workspace, in float2 / float / float elements.
struct SensWork {
    size_t fields, gt, partial;
    size_t bytes() const { return fields * sizeof(float2) + (gt + partial) * sizeof(float); }
};

static bool sens_work(int groups, int K, int batch, int pn, SensWork& w)
{
    if (groups < 1 || K < 1 || batch < 1 || !fft_size_ok(pn)) return false;
    const long long items = (long long)groups * K;
    if (items > INT_MAX || items * batch > INT_MAX || items * batch * pn > INT_MAX) return false;
    w.partial = (size_t)(items * batch * pn);
    w.fields = w.partial * pn;
    w.gt = (size_t)groups * pn * pn;
    return true;
}

// Workgroups of litho_pupil_project's first stage: a function of the sizes alone, so the order of every sum is too.  0 for a
// bad argument.
static int project_blocks(int planes, int J, int pn)
{
    if (planes < 1 || J < 1 || J > LITHO_PUPIL_PROJECT_MAX_TERMS || !fft_size_ok(pn)) return 0;
    const long long pairs = (long long)planes * pn * pn / 2;
    if ((long long)planes * pn > INT_MAX) return 0;
    const long long blocks = (pairs + 255) / 256;
    return (int)(blocks < PROJ_MAX_BLOCKS ? blocks : PROJ_MAX_BLOCKS);
}

}  // namespace litho

extern "C" {

int litho_socs_fields(const void* kernels, const void* maskFT, int batch, int pn, int N, void* fields, void* stream)
{
    using namespace litho;
    if (!kernels || !maskFT || !fields) return LITHO_E_ARG;
    const int rc = check_sizes(batch, pn, N);
    if (rc != LITHO_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(fill_twiddles(st));
    HIP_TRY(centred2d<LOAD_TIMES_MASK>((const float2*)kernels, (float2*)fields, (const float2*)maskFT, nullptr, 1, batch, pn,
                                       log2_exact(N) - log2_exact(pn), +1, st, batch));
    return LITHO_OK;
}

size_t litho_socs_vjp_work_bytes(int groups, int K, int pn)
{
    using namespace litho;
    if (groups < 1 || K < 1 || !fft_size_ok(pn) || (long long)groups * K * pn > INT_MAX) return 0;
    return (size_t)groups * K * pn * pn * sizeof(float2);
}

int litho_socs_vjp(const void* kernels, const void* maskFT, const float* gradI, int groups, int K, int pn, int N, void* grad,
                   int accumulate, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    if (!kernels || !maskFT || !gradI || !grad || !work || groups < 1 || K < 1) return LITHO_E_ARG;
    const long long batch = (long long)groups * K;
    const int rc = check_sizes(batch, pn, N);
    if (rc != LITHO_OK) return rc;
    if (work_bytes < litho_socs_vjp_work_bytes(groups, K, pn)) return LITHO_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float2* w = (float2*)work;
    const int log2m = log2_exact(N) - log2_exact(pn);
    HIP_TRY(fill_twiddles(st));
    // the fields of the batch, then L^H of G . E in place
    HIP_TRY(centred2d<LOAD_TIMES_MASK>((const float2*)kernels, w, (const float2*)maskFT, nullptr, 1, (int)batch, pn, log2m, +1, st,
                                       (int)batch));
    HIP_TRY(centred2d<LOAD_TIMES_GRAD>(w, w, nullptr, gradI, K, (int)batch, pn, log2m, -1, st, (int)batch));
    const long long cells = (long long)pn * pn, pairs = cells / 2;
    long long blocks = (pairs + 255) / 256;
    if (blocks > 65536) blocks = 65536;                            // grid-stride beyond that
    hipLaunchKernelGGL(k_vjp_reduce, dim3((unsigned)blocks), dim3(256), 0, st, (const float2*)kernels, (const float2*)w, (int)batch,
                       cells, (float2*)grad, accumulate ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

// The tangent of the image: dI[p][g] (+)= 2 sum_k Re(conj(E_gk) . L(kernels[gK+k] . dMaskFT[p])).  Workspace: the chunk's fields
// E^T (their final transpose left out: the fold meets them line for line in the transposed layout), one direction's stack between
// its two passes, and the real planes of one direction in the transposed layout -- nothing grows with P.
size_t litho_socs_jvp_work_bytes(int groups, int K, int P, int pn)
{
    using namespace litho;
    if (groups < 1 || groups > 65535 || K < 1 || P < 1 || P > LITHO_SOCS_JVP_MAX_DIRECTIONS || !fft_size_ok(pn) ||
        (long long)groups * K * pn > INT_MAX)
        return 0;
    const size_t cells = (size_t)pn * pn;
    return 2 * (size_t)groups * K * cells * sizeof(float2) + (size_t)groups * cells * sizeof(float);
}

int litho_socs_jvp(const void* kernels, const void* maskFT, const void* dMaskFT, int P, int groups, int K, int pn, int N, float* dI,
                   int accumulate, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    if (!kernels || !maskFT || !dMaskFT || !dI || !work || groups < 1 || groups > 65535 || K < 1 || P < 1 ||
        P > LITHO_SOCS_JVP_MAX_DIRECTIONS)
        return LITHO_E_ARG;
    const long long batch = (long long)groups * K;
    const int rc = check_sizes(batch, pn, N);
    if (rc != LITHO_OK) return rc;
    if (work_bytes < litho_socs_jvp_work_bytes(groups, K, P, pn)) return LITHO_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t cells = (size_t)pn * pn;
    float2* fields = (float2*)work;                                // E^T, item by item
    float2* tang = fields + (size_t)batch * cells;                 // one direction between its passes
    float* sums = (float*)(tang + (size_t)batch * cells);          // dI[p]^T, plane by plane
    const int log2m = log2_exact(N) - log2_exact(pn);
    const long long lines = batch * pn;
    const unsigned tiles = (unsigned)((pn + TR_TILE - 1) / TR_TILE);
    const dim3 tgrid(tiles, tiles, (unsigned)groups);
    HIP_TRY(fill_twiddles(st));
    // the fields of the chunk once per call: rows of phi . M, transpose, rows -- and no transpose back
    HIP_TRY(centred_rows<LOAD_TIMES_MASK>(RowArgs{(const float2*)kernels, fields, (const float2*)maskFT, nullptr, 1, lines, log2m}, pn,
                                          +1, st));
    HIP_TRY(transpose(fields, (int)batch, pn, st));
    HIP_TRY(centred_rows<LOAD_PLAIN>(RowArgs{fields, fields, nullptr, nullptr, 1, lines, log2m}, pn, +1, st));
    // direction by direction, each by the same launches: its bits do not depend on P or on its neighbours
    for (int p = 0; p < P; ++p) {
        float* out = dI + (size_t)p * groups * cells;
        HIP_TRY(centred_rows<LOAD_TIMES_MASK>(RowArgs{(const float2*)kernels, tang, (const float2*)dMaskFT + (size_t)p * cells, nullptr, 1,
                                                      lines, log2m}, pn, +1, st));
        HIP_TRY(transpose(tang, (int)batch, pn, st));
        if (accumulate) {
            hipLaunchKernelGGL(k_transpose_real, tgrid, dim3(256), 0, st, (const float*)out, sums, pn);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY((centred_rows<LOAD_PLAIN, STORE_FOLD>(RowArgs{tang, tang, fields, nullptr, K, (long long)groups * pn, log2m, nullptr,
                                                              accumulate ? 1 : 0, sums}, pn, +1, st)));
        hipLaunchKernelGGL(k_transpose_real, tgrid, dim3(256), 0, st, (const float*)sums, out, pn);
        HIP_TRY(hipGetLastError());
    }
    return LITHO_OK;
}

// The image of many mask spectra: out[b][g] (+)= sum_k |L(kernels[gK+k] . maskFTs[b])|^2.  Workspace: the fields of every (tile,
// plane, kernel) between their two row passes, and the images in the transposed layout, where the second pass sums them.
size_t litho_socs_image_batch_work_bytes(int tiles, int groups, int K, int pn)
{
    using namespace litho;
    if (tiles < 1 || groups < 1 || groups > 65535 || K < 1 || !fft_size_ok(pn)) return 0;
    const long long planes = (long long)tiles * groups;
    if (planes > INT_MAX || planes * K > INT_MAX || planes * K * pn > INT_MAX) return 0;
    const size_t cells = (size_t)pn * pn;
    return (size_t)planes * K * cells * sizeof(float2) + (size_t)planes * cells * sizeof(float);
}

int litho_socs_image_batch(const void* kernels, const void* maskFTs, int tiles, int groups, int K, int pn, int N, float* out,
                           int accumulate, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    if (!kernels || !maskFTs || !out || !work || tiles < 1 || groups < 1 || groups > 65535 || K < 1) return LITHO_E_ARG;
    const long long planes = (long long)tiles * groups;
    if (planes > INT_MAX || planes * K > INT_MAX) return LITHO_E_ARG;
    const long long batch = planes * K;
    const int rc = check_sizes(batch, pn, N);
    if (rc != LITHO_OK) return rc;
    if (work_bytes < litho_socs_image_batch_work_bytes(tiles, groups, K, pn)) return LITHO_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t cells = (size_t)pn * pn;
    float2* fields = (float2*)work;                                // item (b groups + g) K + k between its passes
    float* sums = (float*)(fields + (size_t)batch * cells);        // out[b][g]^T, plane by plane
    const int log2m = log2_exact(N) - log2_exact(pn);
    const unsigned tr = (unsigned)((pn + TR_TILE - 1) / TR_TILE);
    // the real transpose of `planes` planes, at most 65535 per launch (grid.z)
    auto transpose_real = [&](const float* from, float* to) {
        for (long long p0 = 0; p0 < planes; p0 += 65535) {
            const unsigned nb = (unsigned)(planes - p0 < 65535 ? planes - p0 : 65535);
            hipLaunchKernelGGL(k_transpose_real, dim3(tr, tr, nb), dim3(256), 0, st, from + (size_t)p0 * cells, to + (size_t)p0 * cells, pn);
        }
        return hipGetLastError();
    };
    HIP_TRY(fill_twiddles(st));
    // rows of phi . M for every (tile, plane, kernel), transpose, then the columns, squared and summed over k as they come out
    HIP_TRY(centred_rows<LOAD_BATCH>(RowArgs{(const float2*)kernels, fields, (const float2*)maskFTs, nullptr, 1, batch * pn, log2m, nullptr,
                                             groups * K}, pn, +1, st));
    HIP_TRY(transpose(fields, (int)batch, pn, st));
    if (accumulate) HIP_TRY(transpose_real(out, sums));
    HIP_TRY((centred_rows<LOAD_PLAIN, STORE_SQUARE>(RowArgs{fields, fields, nullptr, nullptr, K, planes * pn, log2m, nullptr,
                                                            accumulate ? 1 : 0, sums}, pn, +1, st)));
    HIP_TRY(transpose_real(sums, out));
    return LITHO_OK;
}

size_t litho_source_sensitivity_work_bytes(int groups, int K, int batch, int pn)
{
    litho::SensWork w;
    return litho::sens_work(groups, K, batch, pn, w) ? w.bytes() : 0;
}

int litho_source_sensitivity(const void* pupils, const void* maskFT, const float* gradI, int groups, int K, const int32_t* shifts,
                             int64_t count, int pn, int N, float* sens, int batch, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    if (!pupils || !maskFT || !gradI || !shifts || !sens || !work || groups < 1 || K < 1 || batch < 1 || count < 0) return LITHO_E_ARG;
    if (!fft_size_ok(pn) || !fft_size_ok(N)) return LITHO_E_ARG;
    if (N < pn) return LITHO_E_NSMALL;
    SensWork w;
    if (!sens_work(groups, K, batch, pn, w)) return LITHO_E_ARG;   // more than INT_MAX lines in a chunk
    if (work_bytes < w.bytes()) return LITHO_E_WORKSPACE;
    if (count == 0) return LITHO_OK;
    hipStream_t st = (hipStream_t)stream;
    float2* fields = (float2*)work;
    float* gt = (float*)(fields + w.fields);
    float* partial = gt + w.gt;
    const int log2m = log2_exact(N) - log2_exact(pn), per_point = groups * K;
    HIP_TRY(fill_twiddles(st));
    const unsigned tiles = (unsigned)((pn + TR_TILE - 1) / TR_TILE);
    hipLaunchKernelGGL(k_transpose_real, dim3(tiles, tiles, (unsigned)groups), dim3(256), 0, st, gradI, gt, pn);
    HIP_TRY(hipGetLastError());
    for (int64_t p0 = 0; p0 < count; p0 += batch) {
        const int nb = count - p0 < batch ? (int)(count - p0) : batch;
        const int items = nb * per_point;
        const long long lines = (long long)items * pn;
        // rows of roll(P, d) . M, transpose, then the columns, each reduced against its line of G^T as it comes out
        HIP_TRY(centred_rows<LOAD_ROLLED>(RowArgs{(const float2*)pupils, fields, (const float2*)maskFT, nullptr, 1, lines, log2m,
                                                  shifts + 2 * p0, per_point, nullptr}, pn, +1, st));
        HIP_TRY(transpose(fields, items, pn, st));
        HIP_TRY((centred_rows<LOAD_PLAIN, STORE_REDUCE>(RowArgs{fields, fields, nullptr, gt, K, lines, log2m, nullptr, per_point,
                                                                partial}, pn, +1, st)));
        hipLaunchKernelGGL(k_sum_partials, dim3((unsigned)nb), dim3(64), 0, st, (const float*)partial, per_point * pn, sens + p0);
        HIP_TRY(hipGetLastError());
    }
    return LITHO_OK;
}

size_t litho_pupil_vjp_work_bytes(int groups, int K, int batch, int pn)
{
    litho::SensWork w;
    return litho::sens_work(groups, K, batch, pn, w) ? w.fields * sizeof(float2) : 0;
}

int litho_pupil_vjp(const void* pupils, const void* maskFT, const float* gradI, int groups, int K, const int32_t* shifts,
                    const float* weights, int64_t count, int pn, int N, void* grad, int accumulate, int batch, void* work,
                    size_t work_bytes, void* stream)
{
    using namespace litho;
    if (!pupils || !maskFT || !gradI || !grad || !work || groups < 1 || K < 1 || batch < 1 || count < 0) return LITHO_E_ARG;
    if (!shifts && count > 0) return LITHO_E_ARG;                  // an empty list has no address
    if (!fft_size_ok(pn) || !fft_size_ok(N)) return LITHO_E_ARG;
    if (N < pn) return LITHO_E_NSMALL;
    SensWork w;
    if (!sens_work(groups, K, batch, pn, w)) return LITHO_E_ARG;   // more than INT_MAX lines in a chunk
    if (work_bytes < w.fields * sizeof(float2)) return LITHO_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int log2pn = log2_exact(pn), log2m = log2_exact(N) - log2pn, per_point = groups * K;
    const size_t cells = (size_t)pn * pn;
    if (count == 0) {
        if (!accumulate) HIP_TRY(hipMemsetAsync(grad, 0, (size_t)per_point * cells * sizeof(float2), st));
        return LITHO_OK;
    }
    float2* fields = (float2*)work;
    HIP_TRY(fill_twiddles(st));
    const dim3 rgrid((unsigned)(cells / 256), (unsigned)(per_point < 65535 ? per_point : 65535));
    for (int64_t p0 = 0; p0 < count; p0 += batch) {
        const int nb = count - p0 < batch ? (int)(count - p0) : batch;
        const int items = nb * per_point;
        // the fields of the chunk in natural layout, L^H of G . E in place, then the roll undone and the points summed
        HIP_TRY(centred2d<LOAD_ROLLED>((const float2*)pupils, fields, (const float2*)maskFT, nullptr, 1, items, pn, log2m, +1, st,
                                       per_point, shifts + 2 * p0));
        HIP_TRY(centred2d<LOAD_TIMES_GRAD>(fields, fields, nullptr, gradI, K, items, pn, log2m, -1, st, per_point));
        hipLaunchKernelGGL(k_pupil_reduce, rgrid, dim3(256), 0, st, (const float2*)fields, (const float2*)maskFT, shifts + 2 * p0,
                           weights ? weights + p0 : nullptr, nb, per_point, log2pn, (float2*)grad, (accumulate || p0 > 0) ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    return LITHO_OK;
}

size_t litho_pupil_project_work_bytes(int planes, int J, int pn)
{
    return (size_t)litho::project_blocks(planes, J, pn) * (size_t)(J > 0 ? J : 0) * sizeof(float);
}

int litho_pupil_project(const void* grad, const void* pupils, int planes, const float* basis, int J, int pn, float* out, void* work,
                        size_t work_bytes, void* stream)
{
    using namespace litho;
    if (!grad || !pupils || !basis || !out || !work) return LITHO_E_ARG;
    const int blocks = project_blocks(planes, J, pn);
    if (blocks == 0) return LITHO_E_ARG;
    if (work_bytes < (size_t)blocks * J * sizeof(float)) return LITHO_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long long cells = (long long)pn * pn;
    hipLaunchKernelGGL(k_project_partial, dim3((unsigned)blocks, (unsigned)((J + PROJ_JT - 1) / PROJ_JT)), dim3(256), 0, st,
                       (const float2*)grad, (const float2*)pupils, basis, J, cells, (long long)planes * cells / 2, (float*)work);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_project_final, dim3((unsigned)J), dim3(64), 0, st, (const float*)work, blocks, J, out);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

}  // extern "C"
