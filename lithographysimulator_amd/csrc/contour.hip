// contour.hip -- printed contours as linked polygon vertices (marching squares) behind litho_contour_count / litho_contour_emit,
// and the dose-focus envelope behind litho_dose_focus_envelope.  No reference counterpart; the definition is in
// include/litho_abbe.h, the checker its CPU restatement tests/contour_oracle.py.  Built with -ffp-contract=off (Makefile):
// every vertex is a fixed sequence of fp32 operations that a NumPy float32 restatement follows operation for operation.
//
// The grid is extended by one ring of virtual samples that are never inside.  Extended row record R = r + 1 (R = 0 .. n) holds
// the H edges of row r (index e = c + 1 = 0 .. n, none at R = 0) and then the V edges between rows r and r + 1 (index c).
//
// k_contour_classify: one 64-lane wave per record and plane, lanes as columns, 64 per step, the gains in a loop inside -- a
//   row is read once as a record's upper and once as the next record's lower row for ALL doses.  __ballot of the inside
//   predicate gives the row's inside word I; the H crossings of the word are I ^ (I << 1 | carry), the V crossings
//   I_upper ^ I_lower: one 64-bit mask word per 64 edges, its exclusive prefix (__popcll, kept by lane `gain`) and the
//   record's two totals go to the workspace.
// k_contour_scan: one wave per image scans the 2 (n + 1) totals into the records' H and V bases and the vertex count.
// k_contour_emit: the same wave-per-record shape over the MASK words (a word without a crossing costs one load); every
//   crossed edge reads its two samples and the two other corners of the cell the contour enters, writes its vertex and the
//   index of the edge it leaves that cell through: base + word prefix + popc(mask & lanes below).
// No atomics, no LDS, no workgroup barrier.  Every address comes from (record, column, mask words); image VALUES decide
// only which of three neighbouring edges is named, never an address.
#include "engine_common.hpp"
#include "../../include/litho_abbe.h"

#include <cmath>
#include <cstdint>
#include <cstring>

namespace litho {

static constexpr int CT_GAINS = 64, CT_WAVES = 4;        // four records per 256-thread workgroup
struct ContourGains {
    float g[CT_GAINS];                                   // rides in the kernel arguments
};

// Where everything lives in the caller's workspace (bytes from its 8-byte aligned base); `images` = n_gains * planes.
struct ContourLayout {
    int W;                       // mask words per edge kind and record: ceil((n + 1) / 64)
    size_t rec;                  // words per image: (n + 1) * 2 W
    size_t mask, offs, pref, base, total, bytes;
};

static ContourLayout contour_layout(int n, int planes, int n_gains)
{
    ContourLayout l;
    const size_t images = (size_t)planes * (size_t)n_gains;
    l.W = (n + 1 + 63) / 64;
    l.rec = (size_t)(n + 1) * 2 * (size_t)l.W;
    l.mask = 0;                                                     // uint64 [images][n + 1][2 W]: H words, then V words
    l.offs = l.mask + images * l.rec * 8;                           // int64 [images + 1]: the caller's output offsets
    l.pref = l.offs + (images + 1) * 8;                             // int32 [images][n + 1][2 W]: exclusive prefix in its kind
    l.base = l.pref + images * l.rec * 4;                           // int32 [images][n + 1][2]: totals, then bases (H, V)
    l.total = l.base + images * (size_t)(n + 1) * 2 * 4;            // int32 [images]: vertices of the image
    l.bytes = (l.total + images * 4 + 7) & ~(size_t)7;
    return l;
}

__device__ __forceinline__ unsigned long long first_lane64(unsigned long long v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(64 * CT_WAVES) void k_contour_classify(const float* __restrict__ image, int planes, int n,
                                                                    const ContourGains gains, int n_gains, float T, int exposed,
                                                                    int W, unsigned long long* __restrict__ mask,
                                                                    int* __restrict__ pref, int* __restrict__ base)
{
    const int lane = threadIdx.x & 63;
    const int R = blockIdx.x * CT_WAVES + (threadIdx.x >> 6);
    const int p = blockIdx.y;
    if (R > n) return;                                   // wave-uniform
    const int r = R - 1;
    const bool ex = exposed != 0;
    const float* up = image + ((size_t)p * n + (size_t)(r < 0 ? 0 : r)) * n;             // row r (unused when r < 0)
    const float* dn = image + ((size_t)p * n + (size_t)(r + 1 < n ? r + 1 : n - 1)) * n; // row r + 1 (unused when r + 1 = n)
    const bool has_up = r >= 0, has_dn = r + 1 < n;
    const size_t rec = (size_t)(n + 1) * 2 * W;
    const size_t img = (size_t)lane * planes + p;        // lane `gain` keeps that gain's prefix and writes its words
    unsigned long long carry = 0;                        // bit `gain`: inside(last column of the previous step) in the upper row
    int cntH = 0, cntV = 0;
    for (int s = 0; s < W; ++s) {
        const int c = 64 * s + lane;
        const float a = (has_up && c < n) ? up[c] : 0.f;
        const float b = (has_dn && c < n) ? dn[c] : 0.f;
        unsigned long long myH = 0, myV = 0;
        for (int gi = 0; gi < n_gains; ++gi) {
            const float gain = gains.g[gi];
            const unsigned long long Iu = __ballot(has_up && c < n && ((a * gain >= T) == ex));
            const unsigned long long Id = __ballot(has_dn && c < n && ((b * gain >= T) == ex));
            const unsigned long long hx = Iu ^ ((Iu << 1) | ((carry >> gi) & 1ull));     // H edge e = c joins columns c - 1, c
            const unsigned long long vx = Iu ^ Id;
            carry = (carry & ~(1ull << gi)) | ((Iu >> 63) << gi);
            if (lane == gi) { myH = hx; myV = vx; }
        }
        if (lane < n_gains) {
            const size_t at = img * rec + (size_t)R * 2 * W + s;
            mask[at] = myH;      pref[at] = cntH;
            mask[at + W] = myV;  pref[at + W] = cntV;
            cntH += __popcll(myH);
            cntV += __popcll(myV);
        }
    }
    if (lane < n_gains) {
        int* t = base + (img * (size_t)(n + 1) + R) * 2;
        t[0] = cntH; t[1] = cntV;
    }
}

// one wave per image: exclusive scan of (H total, V total) of records 0 .. n, in place; counts[image] = the sum
__global__ __launch_bounds__(64) void k_contour_scan(int n, int* __restrict__ base, int* __restrict__ total,
                                                     long long* __restrict__ counts)
{
    const int lane = threadIdx.x;
    int* b = base + (size_t)blockIdx.x * (size_t)(n + 1) * 2;
    int run = 0;
    for (int R0 = 0; R0 <= n; R0 += 64) {
        const int R = R0 + lane;
        const int h = R <= n ? b[2 * R] : 0, v = R <= n ? b[2 * R + 1] : 0;
        int incl = h + v;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (R <= n) {
            b[2 * R] = run + incl - h - v;
            b[2 * R + 1] = run + incl - v;
        }
        run += __shfl(incl, 63);
    }
    if (lane == 0) {
        total[blockIdx.x] = run;
        counts[blockIdx.x] = run;
    }
}

struct CtAt {                    // a sample (row, column), or a cell by its top-left sample (rows r, r + 1, columns c, c + 1)
    int r, c;
};
struct CtEdge {                  // H(r, c) joins samples (r, c) and (r, c + 1); V(r, c) joins (r, c) and (r + 1, c)
    bool horizontal;
    int r, c;
};
__device__ __forceinline__ CtEdge H(int r, int c) { return CtEdge{true, r, c}; }
__device__ __forceinline__ CtEdge V(int r, int c) { return CtEdge{false, r, c}; }

struct ContourView {
    const float* img;            // one plane
    const unsigned long long* mask;
    const int* pref;
    const int* base;
    int n, W;
    float gain, T;
    bool ex;
    // a sample's value times the gain; a virtual sample is never inside
    __device__ __forceinline__ bool real(int r, int c) const { return r >= 0 && r < n && c >= 0 && c < n; }
    __device__ __forceinline__ float at(int r, int c) const { return img[(size_t)r * n + c] * gain; }
    __device__ __forceinline__ bool inside(int r, int c) const { return real(r, c) && ((at(r, c) >= T) == ex); }
    // index of a grid edge among the image's crossed edges
    // (clamped to the table: with the image the masks were made from the clamps never act)
    __device__ __forceinline__ int index(CtEdge e) const
    {
        const int R = min(max(e.r + 1, 0), n), k = min(max(e.horizontal ? e.c + 1 : e.c, 0), n);
        const size_t w = (size_t)R * 2 * W + (e.horizontal ? 0 : W) + (k >> 6);
        return base[2 * R + (e.horizontal ? 0 : 1)] + pref[w] + __popcll(mask[w] & ((1ull << (k & 63)) - 1ull));
    }
    // the edge a contour leaves `cell` through: it entered with the inside on its left, `left` / `right` are the corners ahead
    // on its left / right, and the three other edges of the cell are named by the turn that reaches them
    __device__ __forceinline__ int leave(CtAt left, CtAt right, CtAt cell, CtEdge left_turn, CtEdge straight, CtEdge right_turn) const
    {
        const bool L = inside(left.r, left.c), Q = inside(right.r, right.c);
        const int r0 = cell.r, c0 = cell.c;
        int turn;                                        // 0 left, 1 straight, 2 right
        if (L) turn = Q ? 2 : 1;
        else if (!Q) turn = 0;
        else if (r0 < 0 || c0 < 0 || r0 + 1 >= n || c0 + 1 >= n) turn = 0;      // cannot happen with the image the masks came from
        else {                                           // saddle: all four corners are real
            const float m = ((at(r0, c0) + at(r0, c0 + 1)) + (at(r0 + 1, c0) + at(r0 + 1, c0 + 1))) * 0.25f;
            turn = ((m >= T) == ex) ? 2 : 0;
        }
        return index(turn == 0 ? left_turn : (turn == 1 ? straight : right_turn));
    }
    __device__ __forceinline__ float cut(float a, float b) const
    {
        float t = (T - a) / (b - a);
        if (!(t >= 0.f && t <= 1.f)) t = 0.5f;
        return t;
    }
};

__global__ __launch_bounds__(64 * CT_WAVES) void k_contour_emit(const float* __restrict__ image, int planes, int n,
                                                                const ContourGains gains, int n_gains, float T, int exposed, int W,
                                                                const unsigned long long* __restrict__ mask,
                                                                const int* __restrict__ pref, const int* __restrict__ base,
                                                                const int* __restrict__ total, const long long* __restrict__ offs,
                                                                float* __restrict__ xy, int* __restrict__ next)
{
    const int lane = threadIdx.x & 63;
    const int R = blockIdx.x * CT_WAVES + (threadIdx.x >> 6);
    const int p = blockIdx.y;
    if (R > n) return;                                   // wave-uniform
    const int r = R - 1;
    const size_t rec = (size_t)(n + 1) * 2 * W;
    for (int gi = 0; gi < n_gains; ++gi) {
        const size_t img = (size_t)gi * planes + p;
        const long long o0 = offs[img];
        if (offs[img + 1] - o0 != (long long)total[img]) continue;   // outputs sized for another image: write nothing
        ContourView v;
        v.img = image + (size_t)p * n * n;
        v.mask = mask + img * rec;
        v.pref = pref + img * rec;
        v.base = base + img * (size_t)(n + 1) * 2;
        v.n = n; v.W = W; v.gain = gains.g[gi]; v.T = T; v.ex = exposed != 0;
        const size_t row = (size_t)R * 2 * W;
        for (int s = 0; s < W; ++s) {
            const unsigned long long mh = first_lane64(v.mask[row + s]), mv = first_lane64(v.mask[row + W + s]);
            if (!(mh | mv)) continue;                    // wave-uniform
            const unsigned long long below = (1ull << lane) - 1ull;
            if ((mh >> lane) & 1ull) {                   // H(r, c): samples (r, c) and (r, c + 1), r real
                const int c = 64 * s + lane - 1;
                const long long k = o0 + v.base[2 * R] + v.pref[row + s] + __popcll(mh & below);
                float x;
                int nx;
                const bool lo_in = v.inside(r, c);
                if (c < 0) x = 0.f;
                else if (c + 1 >= n) x = (float)(n - 1);
                else x = (float)c + v.cut(v.at(r, c), v.at(r, c + 1));
                if (lo_in)                               // heading towards row r + 1 through the cell above
                    nx = v.leave(CtAt{r + 1, c}, CtAt{r + 1, c + 1}, CtAt{r, c}, V(r, c), H(r + 1, c), V(r, c + 1));
                else                                     // heading towards row r - 1 through the cell below
                    nx = v.leave(CtAt{r - 1, c + 1}, CtAt{r - 1, c}, CtAt{r - 1, c}, V(r - 1, c + 1), H(r - 1, c), V(r - 1, c));
                xy[2 * k] = x; xy[2 * k + 1] = (float)r;
                next[k] = nx;
            }
            if ((mv >> lane) & 1ull) {                   // V(r, c): samples (r, c) and (r + 1, c), c real
                const int c = 64 * s + lane;
                const long long k = o0 + v.base[2 * R + 1] + v.pref[row + W + s] + __popcll(mv & below);
                float y;
                int nx;
                const bool lo_in = v.inside(r, c);
                if (r < 0) y = 0.f;
                else if (r + 1 >= n) y = (float)(n - 1);
                else y = (float)r + v.cut(v.at(r, c), v.at(r + 1, c));
                if (lo_in)                               // heading towards column c - 1
                    nx = v.leave(CtAt{r, c - 1}, CtAt{r + 1, c - 1}, CtAt{r, c - 1}, H(r, c - 1), V(r, c - 1), H(r + 1, c - 1));
                else                                     // heading towards column c + 1
                    nx = v.leave(CtAt{r + 1, c + 1}, CtAt{r, c + 1}, CtAt{r, c}, H(r + 1, c), V(r, c + 1), H(r, c));
                xy[2 * k] = (float)c; xy[2 * k + 1] = y;
                next[k] = nx;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_envelope(const float* __restrict__ image, int planes, long long cells,
                                                  const ContourGains gains, int n_gains, float* __restrict__ lo,
                                                  float* __restrict__ hi)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cells; i += (long long)gridDim.x * 256) {
        float mn = 0.f, mx = 0.f;
        for (int p = 0; p < planes; ++p) {
            const float u = image[(size_t)p * cells + i];
            for (int gi = 0; gi < n_gains; ++gi) {
                const float a = u * gains.g[gi];
                if (p == 0 && gi == 0) { mn = a; mx = a; }
                else { mn = fminf(mn, a); mx = fmaxf(mx, a); }
            }
        }
        lo[i] = mn;
        hi[i] = mx;
    }
}

static int contour_args(const void* image, int planes, int n, const float* gains_host, int n_gains, ContourGains& gains)
{
    if (!image || !gains_host || n < 1 || n > 16384 || planes < 1 || planes > 65535 || n_gains < 1 || n_gains > CT_GAINS)
        return LITHO_E_ARG;
    memset(&gains, 0, sizeof(gains));
    for (int i = 0; i < n_gains; ++i) {
        if (!(gains_host[i] == gains_host[i])) return LITHO_E_ARG;
        gains.g[i] = gains_host[i];
    }
    return LITHO_OK;
}

}  // namespace litho

extern "C" {

size_t litho_contour_work_bytes(int n, int planes, int n_gains)
{
    if (n < 1 || n > 16384 || planes < 1 || planes > 65535 || n_gains < 1 || n_gains > litho::CT_GAINS) return 0;
    return litho::contour_layout(n, planes, n_gains).bytes;
}

int litho_contour_count(const float* image, int planes, int n, const float* gains_host, int n_gains, float threshold, int exposed,
                        void* work, size_t work_bytes, int64_t* counts_dev, void* stream)
{
    using namespace litho;
    ContourGains gains;
    const int rc = contour_args(image, planes, n, gains_host, n_gains, gains);
    if (rc) return rc;
    if (!work || !counts_dev || ((uintptr_t)work & 7)) return LITHO_E_ARG;
    const ContourLayout l = contour_layout(n, planes, n_gains);
    if (work_bytes < l.bytes) return LITHO_E_WORKSPACE;
    char* w = (char*)work;
    hipLaunchKernelGGL(k_contour_classify, dim3((unsigned)((n + 1 + CT_WAVES - 1) / CT_WAVES), planes), dim3(64 * CT_WAVES), 0,
                       (hipStream_t)stream, image, planes, n, gains, n_gains, threshold, exposed, l.W,
                       (unsigned long long*)(w + l.mask), (int*)(w + l.pref), (int*)(w + l.base));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_contour_scan, dim3((unsigned)(planes * n_gains)), dim3(64), 0, (hipStream_t)stream, n, (int*)(w + l.base),
                       (int*)(w + l.total), (long long*)counts_dev);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_contour_emit(const float* image, int planes, int n, const float* gains_host, int n_gains, float threshold, int exposed,
                       void* work, size_t work_bytes, const int64_t* offsets_host, float* xy_out, int32_t* next_out, void* stream)
{
    using namespace litho;
    ContourGains gains;
    const int rc = contour_args(image, planes, n, gains_host, n_gains, gains);
    if (rc) return rc;
    if (!work || !offsets_host || ((uintptr_t)work & 7)) return LITHO_E_ARG;
    const int64_t images = (int64_t)planes * n_gains;
    if (offsets_host[0] != 0) return LITHO_E_ARG;
    for (int64_t i = 0; i < images; ++i) {
        const int64_t d = offsets_host[i + 1] - offsets_host[i];
        if (d < 0 || d > 2 * (int64_t)n * (n + 1)) return LITHO_E_ARG;
    }
    if (offsets_host[images] > 0 && (!xy_out || !next_out)) return LITHO_E_ARG;
    const ContourLayout l = contour_layout(n, planes, n_gains);
    if (work_bytes < l.bytes) return LITHO_E_WORKSPACE;
    if (offsets_host[images] == 0) return LITHO_OK;      // nothing crosses anywhere
    char* w = (char*)work;
    HIP_TRY(hipMemcpyAsync(w + l.offs, offsets_host, (size_t)(images + 1) * 8, hipMemcpyHostToDevice, (hipStream_t)stream));
    hipLaunchKernelGGL(k_contour_emit, dim3((unsigned)((n + 1 + CT_WAVES - 1) / CT_WAVES), planes), dim3(64 * CT_WAVES), 0,
                       (hipStream_t)stream, image, planes, n, gains, n_gains, threshold, exposed, l.W,
                       (const unsigned long long*)(w + l.mask), (const int*)(w + l.pref), (const int*)(w + l.base),
                       (const int*)(w + l.total), (const long long*)(w + l.offs), xy_out, next_out);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

int litho_dose_focus_envelope(const float* image, int planes, int n, const float* gains_host, int n_gains, float* lo_out,
                              float* hi_out, void* stream)
{
    using namespace litho;
    ContourGains gains;
    const int rc = contour_args(image, planes, n, gains_host, n_gains, gains);
    if (rc) return rc;
    if (!lo_out || !hi_out) return LITHO_E_ARG;
    const long long cells = (long long)n * n;
    const long long blocks = (cells + 255) / 256;
    hipLaunchKernelGGL(k_envelope, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, image, planes,
                       cells, gains, n_gains, lo_out, hi_out);
    HIP_TRY(hipGetLastError());
    return LITHO_OK;
}

}  // extern "C"
