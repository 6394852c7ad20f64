// socs_grad.hip -- the coherent fields of Hopkins imaging and what is differentiated through them: mask, source and pupil
// gradients, the image tangent, the image of a batch of mask spectra.
//
//   E = L(X),   L(X) = F X F^T,   F[q][i] = exp(+2 pi i (i - c)(q - c) / N),  c = pn / 2,  q, i in [0, pn)
//   L^H(Y) = conj(F) Y conj(F)^T                                                       (include/litho_abbe.h)
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
// the line size are plane_fft.hpp's, shared with socs.hip.  There is one row kernel, k_centred_rows<size, sign, Load, Store>: what
// a pass multiplies into its lines on the way in and what it does with the outputs are its two ends, small structs that carry
// their own arguments (below).  Every entry is two_passes -- a first row pass with the entry's load into a stack of planes, the
// transpose, a second row pass with the entry's store -- plus, where it has one, a reduction kernel:
//
//   entry                      first pass: load, sign                   second pass: store      after it
//   litho_socs_fields          TimesPlane(kernels . maskFT)        +1   Field                   transposed back
//   litho_socs_vjp             TimesPlane(kernels . maskFT)        +1   Field                   transposed back
//                              TimesGroupReal(fields . gradI)      -1   Field                   transposed back, k_vjp_reduce
//   litho_socs_jvp             TimesPlane(kernels . maskFT)        +1   Field                   left transposed: E^T is kept
//     per direction p          TimesPlane(kernels . dMaskFT[p])    +1   GroupSums<FoldTerm>     the real planes transposed
//   litho_socs_image_batch     KernelTimesTile(kernels . maskFTs)  +1   GroupSums<SquareTerm>   the real planes transposed
//   litho_socs_vjp_batch       KernelTimesTile(kernels . maskFTs)  +1   Field                   left transposed: E^T is kept
//                              TimesGroupReal(fields^T . gradIs^T) -1   TileSums                nothing: the sums are the gradients
//     at pn 4096               as above                            -1   Field                   k_vjp_reduce per tile
//   litho_source_sensitivity   Rolled(roll(pupils, d) . maskFT)    +1   LineReduce              k_sum_partials
//   litho_pupil_vjp            Rolled(roll(pupils, d) . maskFT)    +1   Field                   transposed back
//                              TimesGroupReal(fields . gradI)      -1   Field                   transposed back, k_pupil_reduce
//   litho_pupil_project        no row pass: k_project_partial, k_project_final
//
// The first pass always stores its field lines (StoreField) and the second always loads them plain (LoadPlain).  The running
// sums of GroupSums and the G of LineReduce are real planes in the transposed layout, where the second pass meets them line for
// line (transpose_real).  Every reduction is one running fp32 sum per element in one fixed order: no atomics, so every result
// is deterministic, a chunked call gives the chunk-ordered sum, and a source point's numbers depend on that point alone.
// No reference counterpart; checked against tests/socs_grad_oracle.py, source_grad_oracle.py, pupil_grad_oracle.py,
// socs_tangent_oracle.py and socs_oracle.py (kernel_image).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <initializer_list>

#include "../../include/litho_abbe.h"
#include "engine_common.hpp"
#include "plane_fft.hpp"

namespace litho {

// ---- The ways in.  open(l, row, log2p) takes line l = row `row` of item l >> log2p and returns at(i), its sample i in [0, pn). ----

// The item's own line.
struct LoadPlain {
    const float2* src;                                      // [items][pn][pn]
    __device__ auto open(long long l, int, int log2p) const { return [in = src + ((size_t)l << log2p)](int i) { return in[i]; }; }
};

// src . plane: one complex plane, the same for every item (the kernels times a mask spectrum or a direction of it).
struct LoadTimesPlane {
    const float2* src;                                      // [items][pn][pn]
    const float2* plane;                                    // [pn][pn]
    __device__ auto open(long long l, int row, int log2p) const
    {
        const float2 *in = src + ((size_t)l << log2p), *mul = plane + ((size_t)row << log2p);
        return [=](int i) { return cmul(in[i], mul[i]); };
    }
};

// src . G[group]: the items are `planes` planes per source point, point-major, and plane j of a point belongs to group j / K
// (a plain stack of planes is one point).  G is real.
struct LoadTimesGroupReal {
    const float2* src;                                      // [points][planes][pn][pn]
    const float* G;                                         // [planes / K][pn][pn]
    int planes, K;
    __device__ auto open(long long l, int row, int log2p) const
    {
        const float2* in = src + ((size_t)l << log2p);
        const float* g = G + ((((size_t)((l >> log2p) % planes / K) << log2p) + row) << log2p);
        return [=](int i) { return make_float2(in[i].x * g[i], in[i].y * g[i]); };
    }
};

// roll(pupil plane, d) . mask: item b is plane (b mod planes) of source point (b / planes), and
//   at(i) = pupils[plane][(row - dy) mod pn][(i - dx) mod pn] . mask[row][i],  (dy, dx) = shifts[point], read once per line.
// The indices are unsigned: the modular index of any integer shift, no overflow.
struct LoadRolled {
    const float2* pupils;                                   // [planes][pn][pn], held once
    const float2* mask;                                     // [pn][pn]
    const int32_t* shifts;                                  // [points][2]
    int planes;
    __device__ auto open(long long l, int row, int log2p) const
    {
        const long long item = l >> log2p, point = item / planes;
        const unsigned dy = (unsigned)shifts[2 * point], dx = (unsigned)shifts[2 * point + 1], wrap = (1u << log2p) - 1;
        const float2* in = pupils + ((((size_t)(item - point * planes) << log2p) + (((unsigned)row - dy) & wrap)) << log2p);
        const float2* mul = mask + ((size_t)row << log2p);
        return [=](int i) { return cmul(in[((unsigned)i - dx) & wrap], mul[i]); };
    }
};

// Many mask spectra through one kernel set: item b is kernel plane (b mod kernels) under the mask plane of tile (b / kernels).
// The kernel planes are read by every tile's items, so the pass writes the item's own plane, never kernel_planes.
struct LoadKernelTimesTile {
    const float2* kernel_planes;                            // [kernels][pn][pn], held once
    const float2* tile_masks;                               // [tiles][pn][pn]
    int kernels;
    __device__ auto open(long long l, int row, int log2p) const
    {
        const long long item = l >> log2p, tile = item / kernels;
        const float2* in = kernel_planes + ((((size_t)(item - tile * kernels) << log2p) + row) << log2p);
        const float2* mul = tile_masks + ((((size_t)tile << log2p) + row) << log2p);
        return [=](int i) { return cmul(in[i], mul[i]); };
    }
};

// ---- The ways out.  The grid covers `lines` line slots, slot s = row (s mod pn) of unit s / pn, and a unit is walk(store)
// consecutive items, transformed one after another by the slot's threads.  store.open(l, row, log2p, lds_line) takes an item line
// and returns put(q, y), which is handed every output of the line; finish sees the line off (every thread of the workgroup calls
// it).  A store may keep lds_floats of LDS per workgroup behind the transform's own (lds_line: the slot's pn of them); begin and
// end run once per workgroup, on every thread, around the walk.  What a store answers unless it says otherwise: one item per
// slot, no LDS of its own, every line size, nothing to do when a line ends. ----
constexpr size_t lds_floats(const void*, int, int) { return 0; }
constexpr int max_log2(const void*) { return 12; }           // the largest line, 2^max_log2, a store's LDS leaves room for
template <class S> __host__ __device__ int walk(const S&) { return 1; }
template <class S> __device__ void begin(const S&, float*, long long, int, int, int) {}
template <class S> __device__ void end(const S&, float*, long long, int, int, int) {}
template <int T, class S, class Put> __device__ void finish(const S&, Put&, float2*, int, bool) {}

// dst[l][q] = y.  dst may BE the pass's src: a line is in registers before any of its outputs is written (every write follows a
// barrier that the line's threads reach with their loads consumed; a 16-point line has one thread), and no workgroup touches
// another's lines.
struct StoreField {
    float2* dst;                                            // [items][pn][pn]
    __device__ auto open(long long l, int, int log2p, float*) const { return [out = dst + ((size_t)l << log2p)](int q, float2 y) { out[q] = y; }; }
};

// partial[l] = sum_q Gt[group][row][q] |y[q]|^2 and nothing else is written (items and groups as LoadTimesGroupReal's).  Each
// thread sums the outputs it owns (r ascending, then e), then the line's threads meet in a fixed order: the xor butterfly of a
// wave's shuffles, every lane ending with the same bits, and for a line of several waves their sums through LDS, added in wave
// order.
struct StoreLineReduce {
    const float* Gt;                                        // [planes / K][pn][pn], transposed planes
    int planes, K;
    float* partial;                                         // [lines]
    struct Put {
        const float* gt;
        float* to;                                          // partial + l
        float acc;
        __device__ void operator()(int q, float2 y) { acc = fmaf(gt[q], fmaf(y.x, y.x, y.y * y.y), acc); }
    };
    __device__ Put open(long long l, int row, int log2p, float*) const
    {
        return {Gt + ((((size_t)((l >> log2p) % planes / K) << log2p) + row) << log2p), partial + l, 0.f};
    }
};
// T threads per line, this one thread lt of it; inactive lines come with acc = 0
template <int T>
__device__ void finish(const StoreLineReduce&, StoreLineReduce::Put& put, float2* smem, int lt, bool active)
{
    float& acc = put.acc;
    constexpr int W = T < 64 ? T : 64;                      // the line's lanes within one wave: an aligned group of W
#pragma unroll
    for (int o = W / 2; o >= 1; o /= 2) acc += __shfl_xor(acc, o);
    if (T > 64) {                                           // one line per workgroup, T / 64 waves
        float* red = reinterpret_cast<float*>(smem);        // the exchange buffer, free once every thread has left the transforms
        __syncthreads();
        if ((lt & 63) == 0) red[lt >> 6] = acc;
        __syncthreads();
        acc = red[0];
        for (int w = 1; w < T / 64; ++w) acc += red[w];
    }
    if (active && lt == 0) *put.to = acc;
}

// What one output adds to a group's running sum: its squared modulus (the image), or twice the real part of its product with
// the conjugate of a stored field (the image tangent; E holds one plane per item, in the layout of the outputs).
struct SquareTerm {
    __device__ auto open(long long, int) const { return [](int, float2 y) { return fmaf(y.x, y.x, y.y * y.y); }; }
};
struct FoldTerm {
    const float2* E;                                        // [groups K][pn][pn]
    __device__ auto open(long long l, int log2p) const
    {
        return [e = E + ((size_t)l << log2p)](int q, float2 y) { return 2.0f * fmaf(e[q].x, y.x, e[q].y * y.y); };
    }
};

// sums[s][q] (+)= sum_k term(y of item g K + k), g = s / pn: the slots are the lines of the GROUPS, and the workgroup walks the
// K items of its group in ascending order; nothing is written besides.  The running sums of the workgroup's lines live in LDS,
// fp32, one per output q, touched by the one thread that owns q and by nobody else between the barrier that ends begin and the
// one that opens end; they start from `sums` when accumulate != 0 and from zero otherwise.  One sum per element in item order,
// no atomics.
template <class Term>
struct StoreGroupSums {
    Term term;
    float* sums;                                            // [groups][pn][pn]
    int K, accumulate;
    __device__ auto open(long long l, int, int log2p, float* lds_line) const
    {
        return [add = term.open(l, log2p), lds_line](int q, float2 y) { lds_line[q] += add(q, y); };
    }
};
template <class Term> constexpr size_t lds_floats(const StoreGroupSums<Term>*, int L, int pn) { return (size_t)L * pn; }
template <class Term> __host__ __device__ int walk(const StoreGroupSums<Term>& s) { return s.K; }
// `cells` sums from the workgroup's first slot on, `threads` threads; the last workgroup's may run past the `slots` there are
template <class Term>
__device__ void begin(const StoreGroupSums<Term>& s, float* lds, long long slots, int cells, int threads, int log2p)
{
    const long long base = (long long)blockIdx.x * cells, limit = slots << log2p;
    for (int i = threadIdx.x; i < cells; i += threads) lds[i] = (s.accumulate != 0 && base + i < limit) ? s.sums[base + i] : 0.f;
    __syncthreads();
}
template <class Term>
__device__ void end(const StoreGroupSums<Term>& s, float* lds, long long slots, int cells, int threads, int log2p)
{
    const long long base = (long long)blockIdx.x * cells, limit = slots << log2p;
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += threads)
        if (base + i < limit) s.sums[base + i] = lds[i];
}

// The complex sibling of StoreGroupSums: grads[s][q] (+)= sum_j 2 conj(kernels[j][row][q]) . y of item t J + j, t = s / pn the TILE
// of slot s and row = s mod pn; the workgroup walks the J = groups K items of its tile in ascending order and the adjoint stack
// is not written.  Two running fp32 sums per output, the real parts of the workgroup's `cells` outputs in LDS ahead of the
// imaginary parts (two float planes: a wave's accesses are to consecutive words at m = 1 and m words apart otherwise, as
// StoreGroupSums'), touched by the one thread that owns q between the barrier that ends begin and the one that opens end.  The
// products are k_vjp_reduce's, so a sum that starts from grads (`accumulate`) continues one sequence of additions.  cells is
// LineShape's L pn, what begin and end are handed; the LDS (8 L pn bytes) fits beside the transform's up to pn 2048.
struct StoreTileSums {
    const float2* kernels;                                  // [J][pn][pn], held once
    float2* grads;                                          // [tiles][pn][pn]
    int J, accumulate, cells;
    __device__ auto open(long long l, int row, int log2p, float* lds_line) const
    {
        const float2* k = kernels + ((((size_t)((l >> log2p) % J) << log2p) + row) << log2p);
        return [k, re = lds_line, im = lds_line + cells](int q, float2 y) {
            re[q] += 2.0f * (k[q].x * y.x + k[q].y * y.y);
            im[q] += 2.0f * (k[q].x * y.y - k[q].y * y.x);
        };
    }
};
constexpr size_t lds_floats(const StoreTileSums*, int L, int pn) { return 2 * (size_t)L * pn; }
constexpr int max_log2(const StoreTileSums*) { return 11; }
__host__ __device__ inline int walk(const StoreTileSums& s) { return s.J; }
__device__ inline void begin(const StoreTileSums& s, float* lds, long long slots, int cells, int threads, int log2p)
{
    const long long base = (long long)blockIdx.x * cells, limit = slots << log2p;
    for (int i = threadIdx.x; i < cells; i += threads) {
        const float2 g = (s.accumulate != 0 && base + i < limit) ? s.grads[base + i] : make_float2(0.f, 0.f);
        lds[i] = g.x;
        lds[cells + i] = g.y;
    }
    __syncthreads();
}
__device__ inline void end(const StoreTileSums& s, float* lds, long long slots, int cells, int threads, int log2p)
{
    const long long base = (long long)blockIdx.x * cells, limit = slots << log2p;
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += threads)
        if (base + i < limit) s.grads[base + i] = make_float2(lds[i], lds[cells + i]);
}

// `lines` line slots of pn = 2^LOG2P samples; each item line x of a slot's unit becomes its centred pruned transform
//   y[q] = sum_i x[i] exp(SIGN 2 pi i (i - c)(q - c) / N),  q in [0, pn),  N = pn << log2m,
// x from `load`, y to `store`.
template <int LOG2P, int SIGN, class Load, class Store>
__global__ __launch_bounds__(LineShape<LOG2P>::THREADS) void k_centred_rows(const Load load, const Store store, long long lines,
                                                                            int log2m)
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
    const long long slot = (long long)blockIdx.x * LS::L + lg;
    const bool active = slot < lines;                       // every thread runs the transforms: they hold workgroup barriers
    float* store_lds = reinterpret_cast<float*>(smem + LS::LDS_EXCH + F::LDS_TW);   // behind the exchange buffers and the tables
    begin(store, store_lds, lines, LS::L * PN, LS::THREADS, LOG2P);
    const int items = walk(store);
    for (int k = 0; k < items; ++k) {
        const long long mine = active ? slot : 0;
        const int row = (int)(mine & (PN - 1));
        const long long l = ((((mine >> LOG2P) * items) + k) << LOG2P) + row;
        const auto at = load.open(l, row, LOG2P);
        auto put = store.open(l, row, LOG2P, store_lds + (size_t)lg * PN);
        // transform index n = lt + T e stands for the sample at signed offset s = n (n < c) or n - pn from the centre: i = s + c
        float2 x0[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int n = lt + F::T * e;
            x0[e] = active ? at((n + C) & (PN - 1)) : make_float2(0.f, 0.f);
        }
        const int m = 1 << log2m;
        const int nmask = (PN << log2m) - 1;                   // N - 1
        const int tshift = 12 - LOG2P - log2m;                 // table stride 4096 / N
        int flip = 0;
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
                if (q >= 0 && q < PN) put(q, x[e]);
            }
        }
        finish<F::T>(store, put, smem, lt, active);
    }
    end(store, store_lds, lines, LS::L * PN, LS::THREADS, LOG2P);
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

// One row pass over `lines` line slots of pn samples.  The sign is the call site's, so only the passes some entry runs exist.
template <int SIGN, class Load, class Store>
static hipError_t centred_rows(const Load& load, const Store& store, long long lines, int pn, int log2m, hipStream_t st)
{
    return for_log2(log2_exact(pn), [&](auto l2) {
        constexpr int LOG2P = decltype(l2)::value;
        if constexpr (LOG2P > max_log2((const Store*)nullptr)) {
            return hipErrorInvalidValue;                        // no such kernel: the entry takes another route at this size
        } else {
            using LS = LineShape<LOG2P>;
            constexpr size_t LDS = LS::LDS_BYTES + sizeof(float) * lds_floats((const Store*)nullptr, LS::L, 1 << LOG2P);
            static_assert(LDS <= 64 * 1024, "the row pass stays inside the default LDS allowance");
            hipLaunchKernelGGL((k_centred_rows<LOG2P, SIGN, Load, Store>), LS::grid(lines), dim3(LS::THREADS), LDS, st, load, store,
                               lines, log2m);
            return hipGetLastError();
        }
    });
}

// The real-plane transpose to[g] = from[g]^T of `planes` pn x pn planes, at most 65535 per launch (grid.z).
static hipError_t transpose_real(const float* from, float* to, long long planes, int pn, hipStream_t st)
{
    const unsigned tiles = (unsigned)((pn + TR_TILE - 1) / TR_TILE);
    const size_t cells = (size_t)pn * pn;
    for (long long p0 = 0; p0 < planes; p0 += 65535) {
        const unsigned nb = (unsigned)(planes - p0 < 65535 ? planes - p0 : 65535);
        hipLaunchKernelGGL(k_transpose_real, dim3(tiles, tiles, nb), dim3(256), 0, st, from + p0 * cells, to + p0 * cells, pn);
    }
    return hipGetLastError();
}

// What every entry is made of: rows of the `items` planes of `data` with `load` on the way in, transpose, rows again with
// `store` on the way out -- the planes are left transposed.  Running sums that start from real planes `start` get them in their
// own layout, `start_t`, ahead of the second pass (one plane per unit of the store).
template <int SIGN, class Load, class Store>
static hipError_t two_passes(const Load& load, float2* data, long long items, const Store& store, int pn, int log2m, hipStream_t st,
                             const float* start = nullptr, float* start_t = nullptr)
{
    const long long units = items / walk(store);
    hipError_t e = centred_rows<SIGN>(load, StoreField{data}, items * pn, pn, log2m, st);
    if (e == hipSuccess) e = transpose(data, (int)items, pn, st);
    if (e == hipSuccess && start) e = transpose_real(start, start_t, units, pn, st);
    return e != hipSuccess ? e : centred_rows<SIGN>(LoadPlain{data}, store, units * pn, pn, log2m, st);
}

// data <- L(the load's product) for sign +1, L^H for sign -1, in natural layout.
template <int SIGN, class Load>
static hipError_t centred2d(const Load& load, float2* data, long long items, int pn, int log2m, hipStream_t st)
{
    const hipError_t e = two_passes<SIGN>(load, data, items, StoreField{data}, pn, log2m, st);
    return e != hipSuccess ? e : transpose(data, (int)items, pn, st);
}

// ---- The size rules, once.  A stack of planes: whether its counts are in range (`counts`) and whether the row pass can number
// its lines (`fits`: pn a transform size and at most INT_MAX lines -- one workgroup per line at the large sizes).  Every entry's
// workspace layout is one, its *_work_bytes is the layout's bytes(), and admit turns it into the entry's return code. ----
struct Stack {
    bool counts, fits = false;
    int pn;
    long long items = 0;                                    // the product of the counts; 0 unless the stack fits
    Stack(std::initializer_list<int> n, int pn, bool counts_ok = true) : counts(counts_ok), pn(pn)
    {
        for (int c : n) counts = counts && c >= 1;
        if (!counts || !fft_size_ok(pn)) return;
        long long lines = pn;                               // counts in [1, INT_MAX]: no partial product leaves a long long
        for (int c : n)
            if ((lines *= c) > INT_MAX) return;
        fits = true;
        items = lines / pn;
    }
    size_t cells(long long planes) const { return fits ? (size_t)planes * pn * pn : 0; }
};

// The order in which every entry refuses: bad pointers and counts, sizes outside litho_fft2_c2c's domain (pn, then N), N < pn,
// too many lines, a workspace too small.
static int admit(bool pointers, const Stack& s, int pn, int N, size_t work_need = 0, size_t work_bytes = 0)
{
    if (!pointers || !s.counts || !fft_size_ok(pn) || !fft_size_ok(N)) return LITHO_E_ARG;
    if (N < pn) return LITHO_E_NSMALL;
    if (!s.fits) return LITHO_E_ARG;
    return work_bytes < work_need ? LITHO_E_WORKSPACE : LITHO_OK;
}

// litho_socs_vjp: the fields of the batch, turned into their adjoints in place.
struct VjpWork : Stack {
    VjpWork(int groups, int K, int pn) : Stack({groups, K}, pn) {}
    size_t bytes() const { return cells(items) * sizeof(float2); }
};

// litho_socs_jvp: the chunk's fields E^T (their final transpose left out: the fold meets them line for line in the transposed
// layout), one direction's stack between its two passes, and the real planes of one direction in the transposed layout --
// nothing grows with P.
struct JvpWork : Stack {
    int groups;
    JvpWork(int groups, int K, int P, int pn)
        : Stack({groups, K}, pn, groups <= 65535 && P >= 1 && P <= LITHO_SOCS_JVP_MAX_DIRECTIONS), groups(groups) {}
    size_t tangent() const { return cells(items); }         // float2 elements behind the fields
    size_t sums() const { return 2 * cells(items); }        // float2 elements ahead of the real planes
    size_t bytes() const { return sums() * sizeof(float2) + cells(groups) * sizeof(float); }
};

// litho_socs_image_batch: the fields of every (tile, plane, kernel) between their two row passes, and the images in the
// transposed layout, where the second pass sums them.  tiles groups K <= INT_MAX is a rule for the counts (refused ahead of N).
struct BatchWork : Stack {
    long long planes;                                       // tiles groups
    BatchWork(int tiles, int groups, int K, int pn)
        : Stack({tiles, groups, K}, pn, groups <= 65535 && (long long)tiles * groups <= INT_MAX / (K > 0 ? K : 1)),
          planes((long long)tiles * groups) {}
    size_t sums() const { return cells(items); }            // float2 elements ahead of the real planes
    size_t bytes() const { return sums() * sizeof(float2) + cells(planes) * sizeof(float); }
};

// litho_socs_vjp_batch: BatchWork's layout and count rules with other contents -- the fields E^T of every (tile, plane, kernel),
// turned into their adjoints in place, and behind them the planes of gradIs in the transposed layout.
struct VjpBatchWork : BatchWork {
    using BatchWork::BatchWork;
    size_t stack() const { return sums(); }                 // float2 elements ahead of G^T
    // L pn of the row pass at this size: the outputs one workgroup sums (StoreTileSums::cells)
    int line_cells() const
    {
        int c = 0;
        (void)for_log2(log2_exact(pn), [&](auto l2) {
            c = LineShape<decltype(l2)::value>::L << decltype(l2)::value;
            return hipSuccess;
        });
        return c;
    }
};

// litho_source_sensitivity: a chunk's fields, G^T, and one partial per line of the chunk.  litho_pupil_vjp: the fields alone.
struct SensWork : Stack {
    int groups;
    SensWork(int groups, int K, int batch, int pn) : Stack({groups, K, batch}, pn), groups(groups) {}
    size_t fields() const { return cells(items); }          // float2
    size_t gt() const { return cells(groups); }             // float
    size_t partial() const { return (size_t)items * pn; }   // float
    size_t field_bytes() const { return fields() * sizeof(float2); }
    size_t bytes() const { return field_bytes() + (gt() + partial()) * sizeof(float); }
};

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
    const int rc = admit(kernels && maskFT && fields, Stack({batch}, pn), pn, N);
    if (rc != LITHO_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(fill_twiddles(st));
    HIP_TRY(centred2d<+1>(LoadTimesPlane{(const float2*)kernels, (const float2*)maskFT}, (float2*)fields, batch, pn,
                          log2_exact(N) - log2_exact(pn), st));
    return LITHO_OK;
}

size_t litho_socs_vjp_work_bytes(int groups, int K, int pn) { return litho::VjpWork(groups, K, pn).bytes(); }

int litho_socs_vjp(const void* kernels, const void* maskFT, const float* gradI, int groups, int K, int pn, int N, void* grad,
                   int accumulate, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    const VjpWork w(groups, K, pn);
    const int rc = admit(kernels && maskFT && gradI && grad && work, w, pn, N, w.bytes(), work_bytes);
    if (rc != LITHO_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    float2* fields = (float2*)work;
    const int batch = (int)w.items, log2m = log2_exact(N) - log2_exact(pn);
    HIP_TRY(fill_twiddles(st));
    // the fields of the batch, then L^H of G . E in place
    HIP_TRY(centred2d<+1>(LoadTimesPlane{(const float2*)kernels, (const float2*)maskFT}, fields, batch, pn, log2m, st));
    HIP_TRY(centred2d<-1>(LoadTimesGroupReal{fields, gradI, batch, K}, fields, batch, pn, log2m, st));
    const long long cells = (long long)pn * pn, pairs = cells / 2;
    long long blocks = (pairs + 255) / 256;
    if (blocks > 65536) blocks = 65536;                            // grid-stride beyond that
    hipLaunchKernelGGL(k_vjp_reduce, dim3((unsigned)blocks), dim3(256), 0, st, (const float2*)kernels, (const float2*)fields, batch,
                       cells, (float2*)grad, accumulate ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

// The tangent of the image: dI[p][g] (+)= 2 sum_k Re(conj(E_gk) . L(kernels[gK+k] . dMaskFT[p])).
size_t litho_socs_jvp_work_bytes(int groups, int K, int P, int pn) { return litho::JvpWork(groups, K, P, pn).bytes(); }

int litho_socs_jvp(const void* kernels, const void* maskFT, const void* dMaskFT, int P, int groups, int K, int pn, int N, float* dI,
                   int accumulate, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    const JvpWork w(groups, K, P, pn);
    const int rc = admit(kernels && maskFT && dMaskFT && dI && work, w, pn, N, w.bytes(), work_bytes);
    if (rc != LITHO_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t cells = (size_t)pn * pn;
    float2* fields = (float2*)work;                                // E^T, item by item
    float2* tang = fields + w.tangent();                           // one direction between its passes
    float* sums = (float*)(fields + w.sums());                     // dI[p]^T, plane by plane
    const int log2m = log2_exact(N) - log2_exact(pn);
    HIP_TRY(fill_twiddles(st));
    // the fields of the chunk once per call, left transposed
    HIP_TRY(two_passes<+1>(LoadTimesPlane{(const float2*)kernels, (const float2*)maskFT}, fields, w.items, StoreField{fields}, pn,
                           log2m, st));
    // direction by direction, each by the same launches: its bits do not depend on P or on its neighbours.  Each output is
    // folded against the stored field as it comes out, so a tangent field is never stored.
    for (int p = 0; p < P; ++p) {
        float* out = dI + (size_t)p * groups * cells;
        HIP_TRY(two_passes<+1>(LoadTimesPlane{(const float2*)kernels, (const float2*)dMaskFT + (size_t)p * cells}, tang, w.items,
                               StoreGroupSums<FoldTerm>{{fields}, sums, K, accumulate ? 1 : 0}, pn, log2m, st, accumulate ? out : nullptr, sums));
        HIP_TRY(transpose_real(sums, out, groups, pn, st));
    }
    return LITHO_OK;
}

// The image of many mask spectra: out[b][g] (+)= sum_k |L(kernels[gK+k] . maskFTs[b])|^2.
size_t litho_socs_image_batch_work_bytes(int tiles, int groups, int K, int pn) { return litho::BatchWork(tiles, groups, K, pn).bytes(); }

int litho_socs_image_batch(const void* kernels, const void* maskFTs, int tiles, int groups, int K, int pn, int N, float* out,
                           int accumulate, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    const BatchWork w(tiles, groups, K, pn);
    const int rc = admit(kernels && maskFTs && out && work, w, pn, N, w.bytes(), work_bytes);
    if (rc != LITHO_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    float2* fields = (float2*)work;                                // item (b groups + g) K + k between its passes
    float* sums = (float*)(fields + w.sums());                     // out[b][g]^T, plane by plane
    HIP_TRY(fill_twiddles(st));
    // rows of phi . M for every (tile, plane, kernel), transpose, then the columns, squared and summed over k as they come out:
    // the K fields of a tile meet in LDS and no K-plane stack of intensities is written
    HIP_TRY(two_passes<+1>(LoadKernelTimesTile{(const float2*)kernels, (const float2*)maskFTs, groups * K}, fields, w.items,
                           StoreGroupSums<SquareTerm>{{}, sums, K, accumulate ? 1 : 0}, pn, log2_exact(N) - log2_exact(pn), st,
                           accumulate ? out : nullptr, sums));
    HIP_TRY(transpose_real(sums, out, w.planes, pn, st));
    return LITHO_OK;
}

// The mask gradients of many windows: grads[b] (+)= 2 sum_j conj(kernels[j]) . L^H(gradIs[b][j / K] . L(kernels[j] . maskFTs[b])),
// j < groups K ascending.  The fields are left transposed and the adjoint is taken of (G . E)^T, since L^H(Y)^T = L^H(Y^T): it
// comes out of its own transpose in natural layout, where it meets the kernels line for line.  Two routes by pn alone:
//   pn <= 2048  fused: the adjoint's second row pass ends in StoreTileSums, the sum over j held in LDS; the adjoint stack is not
//               stored after that pass and no reduction kernel runs;
//   pn == 4096  unfused (the sums would take 32 KiB of LDS beside 36 KiB of exchange buffer and the tables): the second pass
//               stores the adjoints (natural layout, after the pass pair's own transpose) and k_vjp_reduce sums them tile by
//               tile.
// Either way a tile's sum is one sequence of additions in j, started from grads[b] when accumulate != 0.
size_t litho_socs_vjp_batch_work_bytes(int tiles, int groups, int K, int pn) { return litho::VjpBatchWork(tiles, groups, K, pn).bytes(); }

int litho_socs_vjp_batch(const void* kernels, const void* maskFTs, const float* gradIs, int tiles, int groups, int K, int pn, int N,
                         void* grads, int accumulate, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    const VjpBatchWork w(tiles, groups, K, pn);
    const int rc = admit(kernels && maskFTs && gradIs && grads && work, w, pn, N, w.bytes(), work_bytes);
    if (rc != LITHO_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    float2* fields = (float2*)work;                                // item (b groups + g) K + k: E^T, then its adjoint
    float* gt = (float*)(fields + w.stack());                      // gradIs[b][g]^T, plane by plane
    const int log2m = log2_exact(N) - log2_exact(pn), J = groups * K;
    HIP_TRY(fill_twiddles(st));
    HIP_TRY(two_passes<+1>(LoadKernelTimesTile{(const float2*)kernels, (const float2*)maskFTs, J}, fields, w.items, StoreField{fields},
                           pn, log2m, st));
    HIP_TRY(transpose_real(gradIs, gt, w.planes, pn, st));
    const LoadTimesGroupReal load{fields, gt, (int)w.items, K};    // item i meets plane i / K
    if (pn <= 1 << max_log2((const StoreTileSums*)nullptr)) {
        const StoreTileSums sums{(const float2*)kernels, (float2*)grads, J, accumulate ? 1 : 0, w.line_cells()};
        HIP_TRY(two_passes<-1>(load, fields, w.items, sums, pn, log2m, st));
        return LITHO_OK;
    }
    HIP_TRY(two_passes<-1>(load, fields, w.items, StoreField{fields}, pn, log2m, st));    // natural layout: no transpose back
    const long long cells = (long long)pn * pn, pairs = cells / 2;
    long long blocks = (pairs + 255) / 256;
    if (blocks > 65536) blocks = 65536;                            // grid-stride beyond that
    for (int b = 0; b < tiles; ++b) {
        hipLaunchKernelGGL(k_vjp_reduce, dim3((unsigned)blocks), dim3(256), 0, st, (const float2*)kernels,
                           (const float2*)fields + (size_t)b * J * cells, J, cells, (float2*)grads + (size_t)b * cells,
                           accumulate ? 1 : 0);
    }
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

size_t litho_source_sensitivity_work_bytes(int groups, int K, int batch, int pn) { return litho::SensWork(groups, K, batch, pn).bytes(); }

int litho_source_sensitivity(const void* pupils, const void* maskFT, const float* gradI, int groups, int K, const int32_t* shifts,
                             int64_t count, int pn, int N, float* sens, int batch, void* work, size_t work_bytes, void* stream)
{
    using namespace litho;
    const SensWork w(groups, K, batch, pn);
    const int rc = admit(pupils && maskFT && gradI && shifts && sens && work && count >= 0, w, pn, N, w.bytes(), work_bytes);
    if (rc != LITHO_OK) return rc;
    if (count == 0) return LITHO_OK;
    hipStream_t st = (hipStream_t)stream;
    float2* fields = (float2*)work;
    float* gt = (float*)(fields + w.fields());
    float* partial = gt + w.gt();
    const int log2m = log2_exact(N) - log2_exact(pn), per_point = groups * K;
    HIP_TRY(fill_twiddles(st));
    HIP_TRY(transpose_real(gradI, gt, groups, pn, st));
    for (int64_t p0 = 0; p0 < count; p0 += batch) {
        const int nb = count - p0 < batch ? (int)(count - p0) : batch;
        // a source point is the coherent kernel roll(P, d): rows of roll(P, d) . M, transpose, then the columns, each reduced
        // against its line of G^T as it comes out; a point's line partials are summed last
        HIP_TRY(two_passes<+1>(LoadRolled{(const float2*)pupils, (const float2*)maskFT, shifts + 2 * p0, per_point}, fields,
                               (long long)nb * per_point, StoreLineReduce{gt, per_point, K, partial}, pn, log2m, st));
        hipLaunchKernelGGL(k_sum_partials, dim3((unsigned)nb), dim3(64), 0, st, (const float*)partial, per_point * pn, sens + p0);
        HIP_TRY(hipGetLastError());
    }
    return LITHO_OK;
}

size_t litho_pupil_vjp_work_bytes(int groups, int K, int batch, int pn) { return litho::SensWork(groups, K, batch, pn).field_bytes(); }

int litho_pupil_vjp(const void* pupils, const void* maskFT, const float* gradI, int groups, int K, const int32_t* shifts,
                    const float* weights, int64_t count, int pn, int N, void* grad, int accumulate, int batch, void* work,
                    size_t work_bytes, void* stream)
{
    using namespace litho;
    const SensWork w(groups, K, batch, pn);
    const bool pointers = pupils && maskFT && gradI && grad && work && (shifts || count == 0);   // an empty list has no address
    const int rc = admit(pointers && count >= 0, w, pn, N, w.field_bytes(), work_bytes);
    if (rc != LITHO_OK) return rc;
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
        // the fields of the chunk in natural layout, L^H of G . E in place, then the roll undone and the points summed in list order
        HIP_TRY(centred2d<+1>(LoadRolled{(const float2*)pupils, (const float2*)maskFT, shifts + 2 * p0, per_point}, fields, items, pn,
                              log2m, st));
        HIP_TRY(centred2d<-1>(LoadTimesGroupReal{fields, gradI, per_point, K}, fields, items, pn, log2m, st));
        hipLaunchKernelGGL(k_pupil_reduce, rgrid, dim3(256), 0, st, (const float2*)fields, (const float2*)maskFT, shifts + 2 * p0,
                           weights ? weights + p0 : nullptr, nb, per_point, log2pn, (float2*)grad, (accumulate || p0 > 0) ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    return LITHO_OK;
}

// The pupil gradient paired with a basis of wavefront maps, in a two-stage reduction of fixed order.
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
