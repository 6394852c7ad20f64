/*
 * litho_abbe.h -- C ABI of the MI355X (gfx950) Abbe aerial-image engine.
 *
 * Drop-in boundary for the hot path of quarterwave0/LithographySimulator.  The
 * reference is pure Python over torch and has no FFI of its own; these entry points
 * are what a binding for that path would call (ctypes stub: INTEGRATION.md), one per
 * reference callable.  Each comment names the reference interface it replaces.
 *
 * Conventions (all functions):
 *   - return 0 on success, a negative LITHO_E_* code otherwise; never throw, never abort;
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - complex64 arrays are interleaved (re, im) fp32, row-major, exactly torch's layout;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *     and the call returns without waiting for it, except where a comment says
 *     "reads back": those calls copy a few bytes to the host and wait for `stream`;
 *   - nothing is allocated on behalf of the caller: scratch comes from the caller's
 *     `workspace` (size from litho_abbe_workspace_bytes);
 *   - pn = mask pixelNumber (even, 2..16384), N = FFT size from
 *     Mask.calculateEpsilonN (power of two, pn <= N <= 16384).
 */
#ifndef LITHO_ABBE_H
#define LITHO_ABBE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LITHO_OK 0
#define LITHO_E_ARG (-1)        /* bad size / null pointer / unsupported (pn odd, N not 2^k) */
#define LITHO_E_NSMALL (-2)     /* N < pn: the reference fails here too           */
#define LITHO_E_WORKSPACE (-3)  /* workspace too small                                        */
#define LITHO_E_HIP (-4)        /* a HIP runtime call failed; see litho_last_error()           */
#define LITHO_E_INDEX (-5)      /* aberration vector of length 4 (pupil.py:91-92)   */
#define LITHO_E_NOCONV (-6)     /* litho_develop_time: the launch cap was reached before the fixed point */

/* Library version and the gfx target it was compiled for ("gfx950"). */
int litho_version(void);
const char *litho_target_arch(void);
/* Text of the last HIP error seen by this thread ("" if none). */
const char *litho_last_error(void);

/* ---- FFT sizing: Mask.calculateEpsilonN / _nearest2SqInt (mask.py:63-72). Host only. */
int litho_epsilon_n(double deltaK, double pixelSize, double wavelength,
                    double *epsilon_host, int *N_host);

/* ---- Source sampling: LightSource.generateAnnular (lightsource.py:34-50) and
 * generateQuasar (lightsource.py:52-73).  kind 0 = annular, 1 = quasar.  Writes the int64
 * 0/1 bitmap [pn,pn] the reference returns (fp16-exact sigma grid). */
int litho_source_bitmap(int kind, double sigma_in, double sigma_out, int pn,
                        double shift_x, double shift_y, int count, double rotation,
                        int64_t *bitmap, void *stream);

/* ---- imageformation.py:59 `(argwhere(lightsource) - pn//2).int()`: compacts any int64
 * bitmap [pn,pn] (non-zero = lit) into int32 [S,2] (dy,dx) in row-major order.
 * `shifts` must have room for pn*pn pairs (or `capacity` pairs; more lit pixels than
 * that is LITHO_E_ARG).  scratch: (pn+1) int32.  Reads back: *count_host = S.
 * Asynchronous form: count_host == NULL -- nothing is read back and the call does not wait; S stays on the
 * device in scratch[pn] (an int32) for litho_abbe_accumulate_counted. */
int litho_source_compact(const int64_t *bitmap, int pn, int32_t *shifts, int64_t capacity,
                         int32_t *scratch, int64_t *count_host, void *stream);

/* ---- The same compaction for a weighted source: a FLOAT32 map [pn,pn] whose values are intensity weights (lit = w > 0;
 * no reference counterpart, see litho_abbe_accumulate_weighted) into int32 [S,2] shifts plus fp32 [S] weights, same row-major
 * order, same scratch and the same asynchronous form (count_host == NULL: S stays in scratch[pn]).  `weights` has room for as
 * many entries as `shifts` has pairs.  A map of exact 0 / 1 values gives the shift list of litho_source_compact bit for bit. */
int litho_source_compact_weighted(const float *map, int pn, int32_t *shifts, float *weights, int64_t capacity,
                                  int32_t *scratch, int64_t *count_host, void *stream);

/* ---- Pupil: Pupil.generateWavefrontError / generatePupilFunction
 * (pupil.py:32-38, 46-111).  coeffs_f16_host: J fp16 bit patterns (uint16) in OSA/ANSI
 * order, as given by the caller, BEFORE the defocus rescale of coefficient 4; the
 * rescaled vector is written back to coeffs_f16_host (the reference mutates its
 * argument).  flags bit 0: skip that rescale (single-term generateZ,
 * pupil.py:46-77).  Outputs (either may be NULL): wavefront = fp16 W [pn,pn] as uint16
 * bit patterns, pupil = complex64 phi [pn,pn].  Asynchronous for J <= 32 (the term table
 * travels in the kernel arguments); longer vectors are staged through a transient device
 * buffer and the call waits for `stream`. */
int litho_pupil(uint16_t *coeffs_f16_host, int J, int pn, double NA, double wavelength, int flags,
                uint16_t *wavefront, void *pupil, void *stream);

/* ---- Through-focus pupil stack (the pupil export "batched over P defocus planes").  The reference has no
 * stack call: its counterpart is a Python loop `ab = aberrations.clone(); ab[4] = d_p; Pupil(pn, wavelength, NA, ab)
 * .generatePupilFunction()` per plane, i.e. pupil.py:88-100 + 102-111 run once per defocus value with the rescale of
 * pupil.py:91-92 applied to each d_p.  Here: ONE launch per 64 planes writes wavefront fp16 [planes,pn,pn] and / or pupil
 * complex64 [planes,pn,pn] in place; the sigma grid, r, theta and the J - 1 other Zernike terms are evaluated once per pixel,
 * the fp16 running sum is re-run per plane in the reference's order.  Bit-identical to `planes` litho_pupil calls.
 * coeffs_f16_host: J >= 5 fp16 bit patterns (coefficient 4 is ignored; J < 5: LITHO_E_INDEX, as `ab[4] = d` raises);
 * defocus_f16_host: `planes` fp16 bit patterns, the values of coefficient 4 BEFORE the rescale.  Nothing is written back
 * (the loop above works on clones).  Asynchronous for J <= 32; longer vectors run plane by plane through litho_pupil. */
int litho_pupil_stack(const uint16_t *coeffs_f16_host, int J, const uint16_t *defocus_f16_host, int planes, int pn,
                      double NA, double wavelength, uint16_t *wavefront, void *pupil, void *stream);

/* ---- generatePhi (pupil.py:102-111): pupil = exp(1j*2*pi*WE) for a complex64 wavefront
 * error WE [pn,pn], zero where the fp16 radius exceeds 1. */
int litho_pupil_phase(const void *wavefront_c64, int pn, void *pupil, void *stream);

/* ---- Workspace for the three calls below.  (For a mask size that runs embedded -- see litho_abbe_embedded_size -- this
 * includes the padded grid's regions and the padded copies; a smaller workspace of at least the size's own regions is
 * accepted and simply runs the problem un-embedded.) */
int litho_abbe_workspace_bytes(int pn, int N, size_t *bytes_host);

/* ---- Which grid a pn x pn problem RUNS at.  The specialised kernels (and the coarse grid) exist for pn = N and pn = N / 2;
 * every other even size -- a 1000^2 or 3000^2 mask; 10 nm pixels, where N = 4 pn -- is evaluated EMBEDDED: mask spectrum and
 * pupil centred in a zero-padded N / 2 (from 256 up) or N (from 1024 up) grid inside the workspace, the same shift list, the
 * centre pn x pn of the accumulated intensity added to `out`: the identical sum term by term, 1.7-3.6x faster than the
 * generic kernels.  The reference rolls the pupil modulo ITS grid (imageformation.py:63), so a source
 * list with a shift that wraps the pupil around the caller's grid is detected (from the plan read-back) and runs the general
 * path at the caller's size instead.  No reference counterpart: it runs any size through torch.fft (imageformation.py:32-45). */
int litho_abbe_embedded_size(int pn, int N, int *size_host);

/* ---- Abbe accumulation: the loop of abbeImage, imageformation.py:54-67.
 *   out[p][q] += sum_{s<S} | E_{p,s}[q] |^2,   E = calculateFFTAerial(roll(P_p, shift_s), M)
 * maskFT  complex64 [pn,pn]; pupil complex64 [planes,pn,pn] (planes >= 1: a through-focus
 * stack sharing maskFT and the source list); shifts int32 [S,2] = (dy,dx) =
 * (row - pn/2, col - pn/2); out fp32 [planes,pn,pn], accumulated into (the caller zeroes
 * it, and all-reduces it across GPUs when the source list is sharded).
 * Reads back 56 bytes once (pupil support box, its edge supports, shift extents, count) to plan the launch -- and 40 more,
 * once, when some but not all shifts of the list wrap the pupil around the grid (a shifted source: the list is then split on
 * the device into a part that keeps the fast paths and a part that needs the general one; options.split).
 * How the sum is evaluated is the library's business: for N = 2 pn, pn = 256 .. 4096 and a source list long
 * enough to repay it, the loop runs pn-point transforms on the grid q = 2 v and the fine image is reconstructed
 * once per call and plane; same result to rounding.  Environment, read once per call:
 * LITHO_ABBE_COARSE = 0 (never) / 1 (default: by source count) / 2 (whenever eligible); the other LITHO_ABBE_*
 * variables select kernel variants for parity tests and tuning. */
int litho_abbe_accumulate(const void *maskFT, const void *pupil, int planes,
                          const int32_t *shifts, int64_t S, int pn, int N, float *out,
                          void *workspace, size_t workspace_bytes, void *stream);

/* Same, with the source-point count left ON THE DEVICE by the asynchronous litho_source_compact:
 * count_dev = &scratch[pn] of that call, capacity = room in `shifts` (the count is clamped to it).  The count
 * comes back with the planning read-back, so compaction + accumulation + post-process of one image wait for the
 * stream exactly once.  *count_host (may be NULL) receives S. */
int litho_abbe_accumulate_counted(const void *maskFT, const void *pupil, int planes,
                                  const int32_t *shifts, const int32_t *count_dev, int64_t capacity,
                                  int pn, int N, float *out, void *workspace, size_t workspace_bytes,
                                  void *stream, int64_t *count_host);

/* ---- Plan reuse for sequences of images that share the pupil (stack) and the source list -- many masks through one
 * optical setting.  The two calls above read 56 bytes back to plan EVERY call (pupil support box, shift extents, count).
 * With a caller-held record the first call plans as usual and fills it; later calls with the same record issue no
 * planning launch and never wait for the stream (images can be queued back to back).  CONTRACT: the caller passes a
 * valid record only while `pupil`, `shifts` and the count are unchanged (set plan->valid = 0 after changing them); pn, N
 * and planes are checked.  count_dev may be NULL (then `capacity` is the number of source points, as in
 * litho_abbe_accumulate).  A source list that was SPLIT by the planning call (a shifted source: some shifts wrap the pupil
 * around the grid, see litho_abbe_accumulate) is split again by every planned call -- the record carries the two counts and
 * extents, the three small split kernels are re-run without a read-back -- so the non-wrapping points keep their fast path
 * (until round 5 a planned call ran the whole list on the general path).  litho_abbe_last_plan field [15]: 0 = planned
 * afresh, 1 = from the record, 2 = planned afresh and the list was split, 3 = split, from the record. */
typedef struct litho_abbe_plan {
    int32_t words[16];      /* the library's business (packed: plan words, source-point count, the grid size the run was planned
                             * for -- the call's own or the padded one of an embedded evaluation --, the outcome of the split;
                             * csrc/abbe_plan.hpp record_store).  A record another library version wrote is ignored (re-planned). */
    int32_t valid;          /* 0: empty, the call fills it; 1: use it */
    int32_t pn, N, planes;  /* what it was made for */
} litho_abbe_plan;
int litho_abbe_accumulate_planned(const void *maskFT, const void *pupil, int planes,
                                  const int32_t *shifts, const int32_t *count_dev, int64_t capacity,
                                  int pn, int N, float *out, void *workspace, size_t workspace_bytes,
                                  void *stream, litho_abbe_plan *plan, int64_t *count_host);

/* ---- The same call with the launch planner's options passed explicitly instead of through the process environment.
 * The reference has no counterpart (its loop has nothing to tune, imageformation.py:62-67); this is how tests, bench.py
 * and embedding applications select an evaluation path per CALL -- per thread, per stream -- without touching
 * LITHO_ABBE_* variables.  Every field: < 0 = not set (the LITHO_ABBE_<NAME> environment variable if present, else the
 * default); the meanings are those of DESIGN.md section 6.  `size` = sizeof(litho_abbe_options) as the caller compiled it
 * (fields beyond it count as not set, so the struct can grow).  plan, options, count_dev and count_host may each be NULL
 * (count_dev NULL: `capacity` is the number of source points). */
typedef struct litho_abbe_options {
    int32_t size;
    int32_t coarse;          /* 0 direct path, 1 coarse grid when the source list repays it (default), 2 whenever eligible */
    int32_t batch;           /* source points per launch pair (0 = automatic) */
    int32_t groups;          /* y-pass groups (partial-image slabs) per launch (0 = automatic) */
    int32_t xchunk;          /* source points per x-pass workgroup (0 = automatic) */
    int32_t tile;            /* T tile width in columns: 4, 8, 16 (0 = automatic) */
    int32_t plane_chunk;     /* planes of a stack in flight per launch pair (0 = automatic: 1) */
    int32_t w64, rect, w64_8192, xsplit, xrect, w64x, gcombine, rowpairs;   /* kernel families, DESIGN.md section 6 */
    int32_t force_generic, force_general;                                  /* runtime-predicated kernels / modular gather */
    int32_t poison;          /* 1: scratch starts the call as NaN bit patterns (tests) */
    int32_t embed;           /* 0: run mask sizes other than N and N / 2 on the generic kernels at their own size instead of
                              * embedded in the next such grid (litho_abbe_embedded_size; default 1) */
    int32_t split;           /* 0: a source list in which SOME shifts wrap the pupil around the grid (shifted, off-axis sources) runs
                              * the general path for every point instead of being split into a non-wrapping part (every fast
                              * path) and a wrapping one (general path) on the device (default 1: from 256 source points; 2: always) */
    int32_t coopdma;         /* 0: the 4096-point coarse-grid y-pass over 16-column tiles loads through registers (k_ypass_coop, round 3)
                              * instead of prefetching the next line by LDS-DMA (k_ypass_coop_dma, default 1) */
} litho_abbe_options;
int litho_abbe_accumulate_opts(const void *maskFT, const void *pupil, int planes, const int32_t *shifts,
                               const int32_t *count_dev, int64_t capacity, int pn, int N, float *out,
                               void *workspace, size_t workspace_bytes, void *stream, litho_abbe_plan *plan,
                               const litho_abbe_options *options, int64_t *count_host);

/* ---- Weighted (grey-level) sources: per-point intensity in the Abbe sum.
 *   out[p][q] += sum_{s<S} w_s | E_{p,s}[q] |^2
 * The reference treats the source as a bitmap -- `argwhere(lightsource)` keeps "non-zero = lit" (imageformation.py:59) and its
 * loop adds every |E_s|^2 with weight one (imageformation.py:62-67) -- so a measured pupil fill, a pixelated freeform source or
 * an apodised annulus cannot be expressed there; this entry goes beyond it.  The argument list of litho_abbe_accumulate_opts
 * plus `weights`: fp32 [S] (or [capacity] with count_dev), one INTENSITY weight per source point, in the order of `shifts`;
 * the square root is taken inside the library.  weights == NULL is exactly litho_abbe_accumulate_opts.  Every evaluation path
 * honours the weights (pruned box, coarse grid, embedded sizes, general mode, stacks, batches, plan reuse); of the launch
 * planner's options the two opt-in x-pass families (rowpairs, w64x) are ignored.  w_s = 0 is legal and adds nothing; a
 * negative, NaN or infinite weight is LITHO_E_ARG from the call that PLANS (found in the planning read-back, before anything
 * is accumulated); a call planned from a record does not look again -- the contract of litho_abbe_accumulate_planned extends
 * to `weights`.  One limit: a weighted list whose shifts wrap the pupil around the grid for SOME points is not split
 * (options.split): it runs whole on the general path (litho_abbe_last_plan [0] = 1, [15] != 2), correct and slower. */
int litho_abbe_accumulate_weighted(const void *maskFT, const void *pupil, int planes, const int32_t *shifts,
                                   const int32_t *count_dev, int64_t capacity, int pn, int N, float *out,
                                   void *workspace, size_t workspace_bytes, void *stream, litho_abbe_plan *plan,
                                   const litho_abbe_options *options, int64_t *count_host, const float *weights);

/* ---- Dry run of the launch planner: what litho_abbe_accumulate* WOULD do for a problem, without touching a device.
 * The reference has no counterpart (its loop has nothing to plan, imageformation.py:62-67); this exists so that the host
 * logic that replaced those six lines -- batching, kernel families, embedded evaluation of odd sizes, the split of a partly
 * wrapping source list, and above all WHERE in the caller's workspace every intermediate lives -- can be verified on a CPU
 * for every admissible size (tests/test_planner_cpu.py).  Inputs = what the call learns from its 56-byte read-back:
 * plan_words[14] (pupil support box rows lo/hi, columns lo/hi; shift extents dy lo/hi, dx lo/hi; source-point count;
 * rows lo/hi of non-zero samples on the natural box's column edges, columns lo/hi on its row edges (INT_MAX / INT_MIN =
 * none); corner flag), and -- needed only when the call would split the list -- split_words[10] (non-wrapping count,
 * wrapping count, dy lo/hi dx lo/hi of either part).  cus = compute units (<= 0: 256); workspace_bytes = what the caller
 * would pass (0: what litho_abbe_workspace_bytes reports).  Regions are byte ranges of the workspace.  Same code as the real
 * path (csrc/abbe_plan.hpp).  result->status = what the call would return before its first launch. */
typedef struct litho_abbe_region { int64_t offset, bytes; } litho_abbe_region;
typedef struct litho_abbe_dry_part {
    int32_t present;            /* 0: this part does not run */
    int32_t run_size;           /* grid it runs at: pn, or the padded size of an embedded evaluation */
    int32_t general, variant, coarse, natural_box, wave_y, xkind;   /* as litho_abbe_last_plan reports them */
    int32_t batch, planes_in_flight, groups, slabs, xchunk, tile;
    int64_t source_points;
    int64_t t_item_bytes;       /* one T item of the run's geometry */
    litho_abbe_region plan, twtab, twtab2, slab_region, slab_used, ic_used, chat_used, gam_used, T_region, T_used, recon_T_used,
                      embed_M, embed_P, embed_O;     /* (bytes 0 = not used by this part; twtab2 is also filled, in front of the
                                                      * planning read-back, when a run at the call's own size COULD take the coarse grid) */
} litho_abbe_dry_part;
typedef struct litho_abbe_dry_run {
    int32_t size;               /* sizeof(litho_abbe_dry_run) as the caller compiled it */
    int32_t status;             /* LITHO_OK, or the error the call would return */
    int32_t run_size, nowrap, split, reserved;
    int64_t workspace_bytes;    /* litho_abbe_workspace_bytes(pn, N) */
    litho_abbe_region list_a, list_b, split_counts;   /* the two lists of a split source list; the block counts (head of T, dead before the loops) */
    litho_abbe_dry_part part[2];   /* [0] the whole list, or the non-wrapping part of a split; [1] the wrapping part */
    litho_abbe_region plan_scratch;   /* the planning launch's partial extrema: 64 bytes per block, ceil(pn / 8) * planes box blocks +
                                       * ceil(S / 1024) extent blocks (1 .. 256; a counted call: S = its capacity), at the head of
                                       * the T region of the call's OWN size -- dead before the loops; for an embedded run that lies
                                       * inside the padded layout's slab region, whichever slabs the plan uses */
} litho_abbe_dry_run;
int litho_abbe_plan_dry_run(int pn, int N, int planes, const int32_t *plan_words, const int32_t *split_words,
                            const litho_abbe_options *options, int cus, size_t workspace_bytes, litho_abbe_dry_run *result);

/* ---- Single-point field: calculateFFTAerial(pf, maskFFFT, pixelNumber, N)
 * (imageformation.py:32-45).  field = complex64 [pn,pn].  Reads back the pupil's support box (56 bytes). */
int litho_abbe_field(const void *pf, const void *maskFT, int pn, int N, void *field,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---- Post-process: imageformation.py:69-77 (abs, bilinear resample by 1/epsilon,
 * zero pad; output size from litho_postprocess_size: 4096 -> 4094).
 * raw fp32 [planes,pn,pn] -> out fp32 [planes,n_out,n_out]. */
int litho_postprocess_size(int pn, double epsilon, int *n_out_host);
int litho_postprocess(const float *raw, int planes, int pn, double epsilon, float *out,
                      void *stream);

/* ---- The same pass with a constant-threshold resist model fused in (the reference lists "photoresist response
 * modeling, simple or otherwise" as an open goal, README.md:21; there is no reference code, so the definition is
 * this one): resist[p][y][x] = 1 where fp32(image * gain) >= fp32(threshold), else 0, on the post-processed
 * [planes,n_out,n_out] grid; gain = exposure dose (or dose / S for a normalised image).  out (the fp32 aerial image)
 * may be NULL when only the contour mask is wanted; resist uint8, required. */
int litho_postprocess_resist(const float *raw, int planes, int pn, double epsilon, double gain, double threshold,
                             float *out, uint8_t *resist, void *stream);

/* ---- Diffused aerial image (the simplest resist model in practical use: Gaussian acid diffusion of the image, then the
 * threshold), fused into the same pass.  The reference has NO counterpart (its README.md:21 lists resist modelling as an
 * open goal), so the definition is this one; checked against the CPU restatement tests/resist_oracle.py.  I = the image
 * litho_postprocess writes (zero border included), zero outside the grid; taps g[k] = exp(-k^2 / (2 sigma_px^2)),
 * k = -R..R, R = ceil(4 sigma_px), normalised to sum 1 in double and rounded to fp32; D = I convolved with g along the
 * rows and along the columns, fp32 accumulation; resist = 1 where fp32(D * gain) >= fp32(threshold).  sigma_px =
 * diffusion length / pixel pitch of the post-processed grid (the mask's pixelSize).  sigma_px = 0 is the identity, bit for
 * bit litho_postprocess_resist; R > 32 (sigma_px > 8), a negative or non-finite sigma_px: LITHO_E_ARG.  out (fp32 D) and
 * resist (uint8) may each be NULL, not both.  Asynchronous: one kernel, no allocation, no host wait. */
int litho_postprocess_resist_diffused(const float *raw, int planes, int pn, double epsilon, double gain, double threshold,
                                      double sigma_px, float *out, uint8_t *resist, void *stream);

/* ---- Sub-pixel critical-dimension metrology on cut lines (no reference counterpart; checked against
 * tests/resist_oracle.py).  image fp32 [planes,n,n] on the post-processed grid (aerial or diffused); gauges int32
 * [n_gauges][3] = (row, col, axis) on the device, axis 0: measure along the row through (row, col), 1: along the column;
 * gains_host: n_gains <= 64 host floats (doses, or dose / S).  out fp32 [n_gains][planes][n_gauges][5] =
 * (cd_nm, x_lo, x_hi, ils_lo, ils_hi).  Along the gauge's line v[0..n-1] with c the gauge's coordinate on it:
 * u[i] = fp32(v[i] * gain), inside(i) = (u[i] >= fp32(threshold)) == (exposed != 0) -- pixel for pixel the contour mask.
 * !inside(c): cd_nm = 0, the rest NaN.  Else [lo, hi] = the maximal run of inside samples through c,
 * x_lo = lo - 1 + (T - u[lo-1]) / (u[lo] - u[lo-1]) (lo = 0: -0.5), x_hi = hi + (T - u[hi]) / (u[hi+1] - u[hi])
 * (hi = n - 1: n - 0.5), in pixels; cd_nm = (x_hi - x_lo) * pixel_size; ils_* = |u[b] - u[a]| / (T * pixel_size) of the
 * crossing segment (image log-slope per nm), NaN at a border edge.  A gauge outside the grid (or axis not 0 / 1) writes
 * five NaN and reads nothing.  Asynchronous, no allocation, no host wait. */
int litho_measure_cd(const float *image, int planes, int n, const int32_t *gauges, int n_gauges, const float *gains_host,
                     int n_gains, double threshold, int exposed, double pixel_size, float *out, void *stream);

/* ---- Edge placement error on layout edges (no reference counterpart; checked against tests/epe_oracle.py).  image fp32
 * [planes,n,n] on the post-processed grid (aerial or diffused), on the device; sites fp32 [n_sites][4] = (x, y, nx, ny) on
 * the device; gains_host: n_gains <= 64 host floats (doses, or dose / S), as litho_measure_cd.  out fp32
 * [n_gains][planes][n_sites][3] = (epe_nm, ils_per_nm, t_k).  All arithmetic is fp32 in exactly this order:
 * Coordinates: image-grid pixel units, sample (row r, column c) sits at (x = c, y = r) -- the convention of
 * litho_measure_cd's x_lo.  (nx, ny) points OUT of the feature and is not normalised; t runs in pixels along it.
 * Samples: h = 0.5, K = ceil(range_px / h) <= 64; for k = -K .. K: t_k = (float)k * 0.5f, px = x + t_k * nx,
 * py = y + t_k * ny (one multiply and one add each).  A sample is VALID iff px and py are finite, 0 <= px <= n - 1 and
 * 0 <= py <= n - 1; an invalid sample carries no information and is never read.  i0 = min((int)floorf(px), n - 2),
 * fx = px - i0 (the same for y), v = (1 - fy) * ((1 - fx) * a + fx * b) + fy * ((1 - fx) * c + fx * d) with a, b the row
 * j0 samples at i0, i0 + 1 and c, d those of row j0 + 1; u_k = v * gain.  in(u) = ((u >= T) == (exposed != 0)), as in
 * litho_measure_cd.  Interval k (-K <= k < K) is a CROSSING when both ends are valid, in(u_k) holds and in(u_{k+1}) does not
 * (leaving the feature going outward); among the crossings the one with the smallest |2k + 1| is taken, on a tie the one
 * with k >= 0.  t* = t_k + h * ((T - u_k) / (u_{k+1} - u_k)); epe_nm = t* * pixel_size (positive: the printed feature
 * reaches beyond the target edge); ils_per_nm = |u_{k+1} - u_k| / ((h * pixel_size) * T); t_k pins the chosen interval.
 * Three NaN when no crossing lies in range, when the site is not finite, or when n < 2.  LITHO_E_ARG, nothing written: a
 * null pointer, n_sites < 1, planes < 1 (or > 65535), n < 1, n_gains outside 1..64, a NaN gain, range_px outside (0, 32] or
 * not finite, pixel_size <= 0 or not finite.  Asynchronous: one kernel, no allocation, no host wait. */
int litho_measure_epe(const float *image, int planes, int n, const float *sites, int64_t n_sites, const float *gains_host,
                      int n_gains, float threshold, int exposed, float range_px, float pixel_size, float *out, void *stream);

/* ---- Forward-mode metrology (csrc/metrology.hip; no reference counterpart, checked against tests/socs_tangent_oracle.py): the exact
 * derivatives of the two piecewise formulas above along P <= LITHO_SOCS_JVP_MAX_DIRECTIONS image directions, not a finite
 * difference.  dImage fp32 [P][planes][n][n] on the device; every other argument as in the primal.  Both kernels run the primal's
 * own search on `image` (one device function serves both), so they differentiate the interval or the run the primal chose.
 *
 * litho_measure_epe_jvp: out fp32 [P][n_gains][planes][n_sites] = d(epe_nm).  With du = gain * (the bilinear sample of dImage at the
 * same two points as u_k and u_{k+1}), h = 0.5 and w = u_{k+1} - u_k,
 *   d epe = (pixel_size * h) * ((-du_k * w - (T - u_k) * (du_{k+1} - du_k)) / (w * w)),
 * fp32 in this order; NaN wherever the primal is NaN.  LITHO_E_ARG as litho_measure_epe, and for P outside 1..16 or a null dImage.
 *
 * litho_measure_cd_jvp: out fp32 [P][n_gains][planes][n_gauges][3] = (dcd_nm, dx_lo, dx_hi).  A crossing x = i + (T - a) / (b - a)
 * between samples i and i + 1 moves by dx = (-da * w - (T - a) * (db - da)) / (w * w), w = b - a, da and db the gained samples of
 * dImage there; a border edge (x_lo = -0.5, x_hi = n - 0.5) has derivative 0; dcd_nm = (dx_hi - dx_lo) * pixel_size.  Where the
 * gauge's sample is not inside: (0, NaN, NaN); a gauge outside the grid: three NaN -- the primal's pattern.  LITHO_E_ARG as
 * litho_measure_cd, and for P outside 1..16 or a null dImage.  Both: asynchronous, one kernel, no allocation, no host wait. */
#define LITHO_SOCS_JVP_MAX_DIRECTIONS 16
int litho_measure_epe_jvp(const float *image, const float *dImage, int P, int planes, int n, const float *sites, int64_t n_sites,
                          const float *gains_host, int n_gains, float threshold, int exposed, float range_px, float pixel_size,
                          float *out, void *stream);
int litho_measure_cd_jvp(const float *image, const float *dImage, int P, int planes, int n, const int32_t *gauges, int n_gauges,
                         const float *gains_host, int n_gains, double threshold, int exposed, double pixel_size, float *out,
                         void *stream);

/* ---- Printed contours as polygons: a marching-squares tracer (no reference counterpart; checked against
 * tests/contour_oracle.py).  image fp32 [planes,n,n] on the device, sample (row r, column c) at (x = c, y = r) as in
 * litho_measure_epe; gains_host: n_gains <= 64 host floats.  One IMAGE is a (gain, plane) pair, numbered gain * planes + plane;
 * a = fl32(u * gain), one fp32 multiply; a sample is INSIDE iff (a >= T) == (exposed != 0), litho_measure_epe's predicate (NaN
 * compares false).  The grid is extended by one ring of virtual samples, rows and columns -1 and n, that are never inside: every
 * contour is a closed loop, and a feature that touches the border is closed along the border samples.
 * Vertices: exactly one on every CROSSED grid edge (one end inside, the other not).  H(r, c) joins (r, c) and (r, c + 1),
 * r in [0, n - 1], c in [-1, n - 1]; V(r, c) joins (r, c) and (r + 1, c), r in [-1, n - 1], c in [0, n - 1].  From the
 * lower-index sample a to the higher-index one b: t = (T - a) / (b - a) in fp32; if !(t >= 0 && t <= 1) then t = 0.5 (non-finite
 * data only); the vertex is (c + t, r) on H and (c, r + t) on V, one fp32 add of the exact integer and t; on an edge with a
 * virtual end it is the real sample's own position.
 * Numbering (the order of the outputs): for r = -1 .. n - 1 the crossed H edges of row r by ascending c (they exist for r >= 0),
 * then the crossed V edges between rows r and r + 1 by ascending c.
 * Linking: next[] is a permutation of one image's crossed edges, image-local int32.  Walking v -> next[v] the feature lies on
 * the LEFT in (x = column, y = row) axes: an outer boundary has positive shoelace area, a hole negative.  Every cell (between
 * extended rows i - 1, i and columns j - 1, j; i, j in [0, n]) has zero, one or two entry edges and as many exits.  A saddle
 * (two diagonal corners inside; all four are then real) is resolved by m = ((a_tl + a_tr) + (a_bl + a_br)) * 0.25f in that
 * fp32 order: (m >= T) == exposed joins the two inside corners, otherwise each is cut off on its own.
 * Polygons = the cycles of next, each from its lowest-numbered vertex, ordered by that number (litho_contour_link, host).
 * Vertex count per image <= 2 n (n + 1): int32 up to n = 16384.
 * Two calls and one read-back between them, the caller's: litho_contour_count classifies (one wave per extended row and plane,
 * the gains in a loop inside) and scans, leaving int64 counts_dev[image]; the caller reads them, forms offsets_host[images + 1]
 * (offsets[0] = 0, exclusive sums of the counts), sizes xy_out fp32 [total][2] and next_out int32 [total], and litho_contour_emit
 * with the SAME image, gains, T, exposed and work writes image i's vertices at offsets[i] .. offsets[i + 1].  An image whose
 * offsets do not match the count found is left unwritten.  work: litho_contour_work_bytes(n, planes, n_gains) device bytes, 8-byte
 * aligned, untouched between the two calls (0 for a bad argument).  LITHO_E_ARG before any launch: a null pointer, n < 1 (or
 * > 16384), planes outside 1..65535, n_gains outside 1..64, a NaN gain, offsets that decrease; LITHO_E_WORKSPACE: work_bytes
 * too small.  Image values are never turned into addresses.  Asynchronous, no allocation, no host wait: emit copies the offsets
 * to the device with an asynchronous copy on `stream`, so offsets_host must stay allocated and unchanged until `stream` has
 * passed that copy (until the stream is synchronised, or an event recorded after the call has completed); gains_host is read
 * before either call returns. */
size_t litho_contour_work_bytes(int n, int planes, int n_gains);
int litho_contour_count(const float *image, int planes, int n, const float *gains_host, int n_gains, float threshold,
                        int exposed, void *work, size_t work_bytes, int64_t *counts_dev /* int64 per image */, void *stream);
int litho_contour_emit(const float *image, int planes, int n, const float *gains_host, int n_gains, float threshold, int exposed,
                       void *work, size_t work_bytes, const int64_t *offsets_host /* images + 1 */, float *xy_out,
                       int32_t *next_out, void *stream);

/* ---- HOST: the cycles of a permutation next[0 .. V) in O(V).  order[V] receives the indices cycle by cycle, every cycle from its
 * lowest index, the cycles by ascending lowest index; starts[n_cycles + 1] (room for V + 1) the cycles' bounds in `order`.  An
 * index outside [0, V), or one reached twice (not a permutation): LITHO_E_ARG, nothing is read out of bounds.  No device. */
int litho_contour_link(const int32_t *next_host, int64_t V, int64_t *order_host, int64_t *starts_host, int64_t *n_cycles_host);

/* ---- Dose-focus envelope for process-variation bands: lo[r][c] = min, hi[r][c] = max over all (gain, plane) pairs of
 * fl32(image[plane][r][c] * gain), folded with fminf / fmaxf in the order plane-major, gain-minor (a NaN product is skipped
 * unless all are NaN).  image fp32 [planes,n,n], lo_out / hi_out fp32 [n,n], all on the device.  The contour of hi at T is the
 * union, that of lo the intersection, of the exposed features over all conditions.  Argument checks as litho_contour_count.
 * Asynchronous: one kernel, no allocation, no host wait. */
int litho_dose_focus_envelope(const float *image, int planes, int n, const float *gains_host, int n_gains, float *lo_out,
                              float *hi_out, void *stream);

/* ---- Hopkins imaging: SOCS kernels from the transmission cross coefficient (no reference counterpart -- the reference images by
 * the Abbe sum alone, imageformation.py:54-67; checked against tests/socs_oracle.py).  For a pupil P [n,n] and a source weight map
 * W [n,n] (d = (row - n/2, col - n/2), as `shifts`), T = sum_s w_s roll(P, d_s) roll(P, d_s)^H is Hermitian positive semidefinite,
 * and the weighted Abbe image is sum_k |field(phi_k)|^2 at shift (0,0) for any phi with sum_k phi_k phi_k^H = T.  T x needs no
 * source list: T x = ifft2(ph . fft2(Wsh . ifft2(conj(ph) . fft2(x)))), ph = fft2(P), Wsh = ifftshift(W), all transforms the plain
 * DFT below.  The factorisation itself (subspace iteration) is lithographysimulator_amd/socs.py; DESIGN.md section 10.
 *
 * litho_fft2_c2c: data complex64 [batch,n,n], in place: the standard 2-D DFT, out[u][v] = sum_jk in[j][k] exp(-/+ 2 pi i (j u + k v) / n)
 * (inverse != 0: the + sign), neither centred nor scaled -- forward then inverse returns n^2 x.  n a power of two, 16..4096;
 * anything else, batch < 1 or a null pointer: LITHO_E_ARG.  Asynchronous, no allocation, no host wait. */
int litho_fft2_c2c(void *data, int batch, int n, int inverse, void *stream);
/* litho_tcc_apply: Y[b] = T X[b], b < batch, by the formula above including the n^-4 of its two inverse transforms.  pupil_hat
 * complex64 [n,n] = litho_fft2_c2c of the pupil; weight_shifted fp32 [n,n]; X, Y complex64 [batch,n,n]; Y may BE X, and must not
 * overlap it otherwise (LITHO_E_ARG).  Sizes and errors as litho_fft2_c2c.  Asynchronous, no allocation, no host wait. */
int litho_tcc_apply(const void *pupil_hat, const float *weight_shifted, const void *X, void *Y, int batch, int n, void *stream);
/* litho_socs_fold: out[g][i] (+)= sum_{k<K} stack[g K + k][i], i < elems, g < groups: the K coherent images of every plane summed
 * in ascending k with one running fp32 sum per element (accumulate != 0: starting from out's value, otherwise overwriting it).
 * stack fp32 [groups K, elems], out fp32 [groups, elems], not overlapping.  groups 1..65535, K >= 1, elems >= 1, else LITHO_E_ARG.
 * Asynchronous: one kernel. */
int litho_socs_fold(const float *stack, int groups, int K, int64_t elems, float *out, int accumulate, void *stream);

/* ---- Vector (polarised, high-NA) Hopkins imaging (csrc/socs.hip; no reference counterpart, checked against tests/vector_oracle.py;
 * DESIGN.md section 10).  Pupil grid point (row i, column j) is sigma = ((j - pn/2) 4/pn, (i - pn/2) 4/pn), the reference's grid
 * (pupil.py:105-111).  Direction cosines in the image medium of refractive index `index`: alpha = NA sigma_x / index,
 * beta = NA sigma_y / index, gamma = sqrt(1 - alpha^2 - beta^2); NA < index; where alpha^2 + beta^2 >= 1 every factor is 0.
 * M_cj maps polarisation component j in {x, y} at the mask side (paraxial object side, thin mask) onto field component
 * c in {x, y, z} at the wafer:
 *   M_xx = 1 - alpha^2 / (1 + gamma)   M_xy = M_yx = -alpha beta / (1 + gamma)   M_yy = 1 - beta^2 / (1 + gamma)
 *   M_zx = -alpha                      M_zy = -beta
 * (columns orthonormal).  radiometric != 0: every factor times gamma^(-1/2), the aplanatic energy factor.  Defocus z in nm:
 * every factor times exp(+2 pi i index z (1 - gamma) / wavelength), the exact high-NA defocus phase (the sign of the rho^2 term
 * of the reference's coefficient 4; not its Zernike-normalised scale).  The six planes of a pupil P are Q_cj = P . M_cj, stored
 * as plane t = 2 c + j.
 *
 * Polarisation: a real symmetric 2 x 2 coherency per source point as three maps on the source grid, W_xx, W_yy, W_xy (the
 * intensity weight map times the coherency entry).  For source point s (weight w_s, shift d_s) and every pure state m of its
 * coherency (weight mu_m, unit vector e_m), a_smc = sqrt(w_s mu_m) roll(e_mx Q_cx + e_my Q_cy, d_s); the image is
 * I = sum_smc |L_N(a_smc . M)|^2 with the engine's chain L_N, and the vector transmission cross coefficient T = sum_smc a a^H,
 *   T x = sum_c sum_j Q_cj (*) ( sum_j' W_jj' . (Q_cj' (star) x) )              (circular on the n grid), in transforms
 *   u_cj' = ifft2(conj(q_cj') . fft2(x)),  v_cj = sum_j' ifftshift(W_jj') . u_cj',  T x = ifft2(sum_cj q_cj . fft2(v_cj)),
 * q = fft2(Q): 14 transforms per vector.  Hermitian positive semidefinite, rank <= 3 S for a rank-one coherency at every lit
 * point and <= 5 S otherwise (M_xy = M_yx); it factors into SOCS kernels as the scalar one does.
 *
 * litho_vector_pupils: out complex64 [planes,6,pn,pn] from pupil complex64 [planes,pn,pn], one kernel launch per plane; factors
 * and phase in double per cell, multiplied into the fp32 pupil value, each component rounded once.  defocus_nm_host: `planes`
 * values on the host (read before the call returns), or NULL for none; wavelength is read only with it.  pn even, 16..16384.
 * NA >= index, planes < 1, a null pupil or out, a non-finite defocus: LITHO_E_ARG.  Asynchronous, no allocation. */
int litho_vector_pupils(const void *pupil, int planes, int pn, double NA, double index, int radiometric, const double *defocus_nm_host,
                        double wavelength, void *out, void *stream);
/* litho_tcc_apply_vector: Y[b] = T X[b], b < batch, by the three steps above including the n^-4 of the inverse transforms.  q_hat
 * complex64 [6,n,n] = litho_fft2_c2c of the six planes (natural orientation; transposed once into the head of `work`);
 * w_shifted fp32 [3,n,n] = ifftshift of W_xx, W_yy, W_xy; X, Y complex64 [batch,n,n]; Y may BE X, and must not overlap it
 * otherwise (LITHO_E_ARG).  work: litho_tcc_apply_vector_work_bytes(batch, n) = 48 (batch + 1) n^2 device bytes, 8-byte aligned
 * (0 for a bad argument); less is LITHO_E_WORKSPACE.  n a power of two, 16..4096, batch 1..2^20.  No atomics, fixed summation
 * order: two calls give the same bits, and so does any split of the batch.  Asynchronous, no allocation, no host wait. */
size_t litho_tcc_apply_vector_work_bytes(int batch, int n);
int litho_tcc_apply_vector(const void *q_hat, const float *w_shifted, const void *X, void *Y, int batch, int n, void *work,
                           size_t work_bytes, void *stream);

/* ---- Resist film stack for vector imaging (csrc/film.hip; no reference counterpart, checked against tests/film_oracle.py;
 * DESIGN.md section 10).  A film stack changes only the six planes Q_cj; the vector TCC above and every consumer take them as
 * they are.  Conventions: the defocus phase exp(+2 pi i n z (1 - gamma) / lambda) above means that a wave advancing by z into
 * the wafer carries exp(-i kappa z), so an absorbing medium (n, k), k >= 0, enters as nn = n - i k.
 * Stack, top to bottom: the incident medium of real index n0 = `index` (NA < n0); L finite layers, 1 <= L <= 16, each
 * (n_l, k_l, thickness d_l > 0 nm); a semi-infinite substrate (n_s, k_s).  Layer `resist` (0-based) is sampled at depths z in nm
 * below its top, 0 <= z <= d_resist.
 * Per pupil cell, (alpha, beta) as above with index = n0, s = NA^2 (sigma_x^2 + sigma_y^2) = n0^2 (alpha^2 + beta^2); every plane
 * is exactly 0 where alpha^2 + beta^2 >= 1.  In each medium w = sqrt(nn^2 - s), the root with Im w <= 0 and Re w > 0 when
 * Im w = 0; kappa = 2 pi w / lambda.  Two independent scalar problems share one recursion: a primary quantity
 * u(z) = a exp(-i kappa z) + b exp(+i kappa z) with flux v = eta (a exp(-i kappa z) - b exp(+i kappa z)), u and v continuous at
 * every interface, b = 0 in the substrate.
 *   s-polarisation: u = E_s, eta = w, incident amplitude a0 = 1.
 *   p-polarisation: u = H_s, eta = w / nn^2, incident amplitude a0 = n0; in the sampled layer
 *     E_rad(z) = (w / nn^2) (a exp(-i kappa z) - b exp(+i kappa z)),   E_z(z) = -(sqrt(s) / nn^2) u(z).
 * With r = (alpha, beta) / sqrt(alpha^2 + beta^2) and t = (-r_y, r_x), the planes at depth z are
 *   Q_cj = P . f . [ t_c E_s t_j + (r_c E_rad + zhat_c E_z) r_j ],   c in {x, y, z}, j in {x, y}, plane 2 c + j;
 * at s = 0, E_s on the diagonal and 0 elsewhere (E_rad = E_s there).  f = gamma0^(-1/2) with `radiometric`, gamma0 in the
 * incident medium.  The pupil's own defocus (nm, in the incident medium: the phase litho_vector_pupils applies) rides on top and
 * places best focus relative to the top of the stack.  No global phase is removed: with every index equal to n0 and k = 0 the
 * planes equal litho_vector_pupils' at defocus z times exp(-2 pi i n0 z / lambda).
 * Evaluation: the reflection ratio is swept upward from the substrate, the transmitted amplitude downward, and the upward wave
 * of a layer is referenced to that layer's BOTTOM, so that no exponential with a positive real exponent is ever formed: every
 * cell with alpha^2 + beta^2 < 1 gives finite planes whatever the thicknesses and absorptions.  The single degenerate point
 * w = 0 exactly in a layer (grazing propagation in it) is NOT pinned.  Double precision per cell, each output component rounded
 * to fp32 once.  Not modelled: absorbed-energy weighting (n k |E|^2 is a constant factor inside one layer), development,
 * layers with a gradient in index.
 *
 * litho_film_pupils: out complex64 [planes, D, 6, pn, pn] from pupil complex64 [planes,pn,pn].  layers: L x {n, k, d_nm} on the
 * host, depths_nm: D values on the host, defocus_nm_host: `planes` values on the host or NULL (all read before the call
 * returns; the stack travels to the kernel by value).  One thread per cell runs the two recursions once and walks the depths;
 * one launch per plane and per 16 depths.  pn even, 16..16384.  LITHO_E_ARG, before any launch: a null pointer, planes < 1,
 * L or resist out of range, D < 1 or planes D > 65535, any non-finite value, k < 0, n <= 0, d <= 0, wavelength <= 0, a depth
 * outside [0, d_resist], NA >= index.  Asynchronous, no allocation, no host wait. */
int litho_film_pupils(const void *pupil, int planes, int pn, double NA, double index, int radiometric, const double *layers, int L,
                      double substrate_n, double substrate_k, int resist, const double *depths_nm, int D,
                      const double *defocus_nm_host, double wavelength, void *out, void *stream);

/* ---- Resist development (csrc/develop.hip; no reference counterpart, checked against tests/develop_oracle.py; DESIGN.md
 * section 10): latent-image diffusion, Mack's dissolution rate and the arrival time of the development front.
 * Grid: a volume is fp32 [D, n, n], 1 <= D <= 32 planes through ONE resist layer of `thickness` nm, plane d at depth
 * z_d = (d + 1/2) hz, hz = thickness / D (the depths of litho_film_pupils' midpoint sampling), lateral pitch h = the image's
 * pixel size in nm, x fastest.  A batch is [B, D, n, n], B D <= 65535, n any size 1..16384.
 *
 * 1. Latent-image diffusion.  A separable Gaussian on the intensity volume, along x, then y, then z.  Taps on each axis are
 * exactly litho_postprocess_resist_diffused's: g[k] = exp(-k^2 / (2 sigma_px^2)), R = ceil(4 sigma_px) <= 32, normalised over
 * -R..R in double, rounded to fp32; fp32 accumulation acc = g[0] c[0], then acc += g[k] (c[-k] + c[k]) in ascending k.  Laterally
 * the volume is zero outside the grid (sigma_px = sigma_nm / h); in z the layer faces are mirrored, no flux: index -1 - k reads
 * k and D + k reads D - 1 - k, repeated as often as needed (sigma_px = sigma_nm / hz) -- acid does not leave the layer.  sigma = 0
 * on an axis is the identity on that axis, bit for bit.
 *
 * 2. Rate: Dill C exposure and Mack's model, per cell in double, rounded to fp32 once:
 *   m = exp(-(C g) I), g the gain (dose);  x = (1 - m)^q;  a = (q + 1) / (q - 1) (1 - m_th)^q;
 *   r = r_max (a + 1) x / (a + x) + r_min   [nm / s],  times the surface-inhibition factor 1 - (1 - r0) exp(-z_d / delta)
 * (r0 = 1: the factor is exactly 1).  The kernel writes the slowness s = 1 / r.  Where 1 - m is negative or NaN (a negative
 * product g I, a NaN intensity) it writes NaN explicitly -- (1 - m)^q alone is finite there for an integer q -- and the solver
 * treats a NaN slowness as a wall.
 *
 * 3. Arrival time T in seconds: the first-order Godunov upwind solution of |grad T| = s with T = 0 on the resist top z = 0, which
 * lies hz / 2 above plane 0.  There is no neighbour beyond the lateral edges of the grid or below plane D - 1; a missing neighbour
 * counts as +inf.  A cell whose s is not finite and positive is a WALL: it keeps T = +inf and passes nothing on.  For a cell,
 * on each axis a_i = the smaller of the two neighbours and h_i the spacing, (h, h, hz); for plane 0 the z-axis value is 0 at spacing
 * hz / 2.  Sort the a_i ascending; with delta_i = a_i - a_1, w_i = 1 / h_i^2, solve for u = T - a_1 (the shifted form: the unshifted
 * discriminant cancels once T >> h s), all in fp32:
 *   one axis:    u = h_1 s; accepted if u <= delta_2;
 *   two axes:    A = w_1 + w_2, Bq = w_2 delta_2, Cq = w_2 delta_2^2 - s^2, u = (Bq + sqrt(max(Bq^2 - A Cq, 0))) / A; accepted if
 *                u <= delta_3;
 *   three axes:  the same with w_3, w_3 delta_3, w_3 delta_3^2 added;
 * the discriminant is evaluated in the algebraically equal form A s^2 - sum_{i<j} w_i w_j (delta_i - delta_j)^2 (delta_1 = 0), which
 * subtracts nothing of size (w delta)^2 and so keeps its bits when hz << h;
 * G = a_1 + u (+inf when a_1 is).  T is the fixed point of T <- min(T, G(T)) started from +inf.  s^2 must be finite in fp32.
 *
 * 4. Developed depth z* [B, n, n] in nm: the first crossing of T = t going down each column, fp32.  T_0 > t: z* = z_0 (t / T_0);
 * first d >= 1 with T_d > t: z* = z_{d-1} + hz ((t - T_{d-1}) / (T_d - T_{d-1})); every plane developed: z* = thickness (cleared).
 * The remaining resist height is thickness - z*.
 *
 * litho_latent_diffuse: image, out fp32 [B,D,n,n], not overlapping; one gather kernel per pass, up to three.  work: B D n^2
 * floats on the device, needed (non-NULL, else LITHO_E_ARG; smaller: LITHO_E_WORKSPACE) when two or three passes run, and then
 * overlapping neither image nor out (LITHO_E_ARG: a pass would read the buffer it writes).  A sigma
 * that is negative, not finite or gives R > 32: LITHO_E_ARG.  Asynchronous, no allocation, no host wait.
 * litho_develop_rate: image fp32 [volumes,D,n,n]; gains_host: n_gains <= 64 host floats, as litho_measure_cd; slowness fp32
 * [n_gains volumes, D, n, n], gain-major; n_gains volumes D <= 65535.  LITHO_E_ARG unless C > 0, r_max > 0, r_min > 0, q > 1,
 * 0 <= m_th < 1, 0 < surface_rate (r0) <= 1, surface_depth_nm (delta) > 0, thickness_nm > 0, all finite, no NaN gain.  One kernel,
 * asynchronous, no allocation, no host wait.
 * litho_develop_time: slowness, T fp32 [B,D,n,n], not overlapping each other or work (LITHO_E_ARG).  A tiled fast-iterative solver: a workgroup relaxes a 16 x 16 x D tile in
 * LDS for a fixed number of rounds (columns in two colours, no races, no atomics: two calls give the same bits, and a batch
 * equals its volumes solved one by one), launches ping-pong T between `T` and `work`, and a launch that lowers no cell ends the
 * loop.  READS BACK: every fourth launch the call copies the launches' change flags to the host and waits for `stream`; it
 * cannot be captured into a graph.  *launches_host = the number of launches up to and including the first that changed nothing.
 * After max_iterations launches (1..65536) without one: LITHO_E_NOCONV, *launches_host = max_iterations, and T holds an
 * unconverged upper bound that must not be used.  work: litho_develop_work_bytes(B, D, n, max_iterations) device bytes
 * (0 for a bad argument), 16-byte aligned; less is LITHO_E_WORKSPACE.  No allocation.
 * litho_developed_depth: T fp32 [B,D,n,n], depth fp32 [B,n,n]; develop_time_s >= 0 and finite.  One kernel, asynchronous.
 * All five: a null pointer, D outside 1..32, n outside 1..16384, B < 1 or B D > 65535: LITHO_E_ARG before any GPU call. */
int litho_latent_diffuse(const float *image, int B, int D, int n, double sigma_xy_px, double sigma_z_px, float *out, void *work,
                         size_t work_bytes, void *stream);
int litho_develop_rate(const float *image, int volumes, int D, int n, const float *gains_host, int n_gains, double C, double r_max,
                       double r_min, double q, double m_th, double surface_rate, double surface_depth_nm, double thickness_nm,
                       float *slowness, void *stream);
size_t litho_develop_work_bytes(int B, int D, int n, int max_iterations);
int litho_develop_time(const float *slowness, int B, int D, int n, double thickness_nm, double pixel_nm, int max_iterations,
                       float *T, void *work, size_t work_bytes, int *launches_host, void *stream);
int litho_developed_depth(const float *T, int B, int D, int n, double thickness_nm, double develop_time_s, float *depth,
                          void *stream);

/* ---- Post-exposure bake of a chemically amplified resist (csrc/peb.hip; no reference counterpart, checked against the float64
 * restatement tests/peb_oracle.py).  Acid h, base quencher q (both relative to the initial PAG) and the accumulated acid dose a
 * [s] on the grid of the development calls: fp32 [B, D, n, n], plane d at depth (d + 1/2) hz, hz = thickness / D, lateral pitch
 * `pixel`; lengths in nm, times in s.  A bake makes the slowness volume that litho_develop_time takes, in place of
 * litho_latent_diffuse and litho_develop_rate.
 *
 * 1. Exposure: h0 = 1 - exp(-(C g) I), g the gain (dose), per cell in double, rounded to fp32 once; NaN where that is negative
 * or NaN (a negative product g I, a NaN intensity), litho_develop_rate's convention.  q starts uniform at q0 >= 0, a at 0.
 *
 * 2. One bake step of length dt = bake_time / S, all in fp32, each line a fixed sequence of single operations:
 *   diffusion       x' = x + lxy (((W + E) + (S + N)) - 4 x) + lz ((U + Dn) - 2 x)  for x = h and x = q, both from the values at
 *                   the start of the step (Jacobi); W, E, S, N the lateral neighbours, U, Dn the planes above and below.  NO FLUX
 *                   through any of the six faces: a neighbour outside the grid is the cell's mirror image, index -1 <-> 0 (the
 *                   cell itself).  lxy = D_s dt / pixel^2 and lz = D_z dt / hz^2 per species, from the customary diffusion lengths
 *                   sigma = sqrt(2 D_s bake_time) and sigma_z = vertical_scale sigma: lxy = sigma^2 / (2 S pixel^2),
 *                   lz = sigma_z^2 / (2 S hz^2), formed in double and rounded to fp32.  A species with sigma = 0 skips this line
 *                   and is left untouched bit for bit.
 *   neutralisation  beta = fp32(k_quench dt); R = beta h' q' / (1 + beta (h' + q')) (left to right), or, when beta is +inf
 *                   (k_quench = +inf, instantaneous), R = (h' < q') ? h' : q' -- written like this so that a NaN behaves as in
 *                   numpy.where; h'' = h' - R, q'' = q' - R.  h - q is conserved; in exact arithmetic neither goes negative.
 *   acid loss       h''' = h'' fl, fl = fp32(exp(-k_loss dt)) from the host.
 *   amplification   a <- a + fp32(dt / 2) (h_at_the_start_of_the_step + h''')  (trapezoid).
 * (Unlike litho_latent_diffuse, which puts zeros outside the grid laterally, the bake mirrors: mass is then conserved exactly
 * and a bake does not drain acid out of the picture.)
 *
 * 3. After S steps: inhibitor m = exp(-k_amp a), Mack's rate r(m) of litho_develop_rate with x = (1 - m)^q, times the surface
 * factor of the plane; slowness 1 / r.  Double per cell, rounded once; NaN where 1 - m is negative or NaN, a wall to
 * litho_develop_time.  a = 0 gives m = 1 and r = r_min exactly.
 *
 * Steps.  litho_peb_min_steps: the smallest S with 4 lxy + 2 lz <= 1 (in double) for both species -- every diffusion update is
 * then a convex combination: a maximum principle holds and no concentration goes negative; 0 for a bad argument (a negative or
 * non-finite length or scale, thickness or pixel not positive and finite, D outside 1..32) or when that S exceeds the cap 65536.
 * The reaction is first order in dt: raise S for a stiff finite k_quench.
 *
 * litho_peb_expose: image fp32 [volumes,D,n,n]; gains_host: n_gains <= 64 host floats; acid fp32 [n_gains volumes, D, n, n],
 * gain-major, not overlapping image; n_gains volumes D <= 65535; C > 0 and finite, no NaN gain.  One kernel, asynchronous.
 * litho_peb_bake: acid_in (h0), acid, quencher, acid_dose fp32 [B,D,n,n] and work, litho_peb_work_bytes(B, D, n) = two volumes
 * of device bytes (0 for a bad argument), 16-byte aligned: none may overlap another (LITHO_E_ARG); less workspace is
 * LITHO_E_WORKSPACE.  quencher0, k_loss, the two diffusion lengths and vertical_scale >= 0 and finite, k_quench >= 0 (+inf
 * allowed; a finite k_quench whose beta overflows fp32 counts as +inf), bake_time_s > 0 and finite, steps from
 * litho_peb_min_steps(...) to 65536; anything else is LITHO_E_ARG.  Two kernels run the one step function: a direct kernel, one
 * step per launch with the neighbours from global memory, and a fused kernel that runs s = 2..4 steps per launch on a
 * 16 x 16 x D tile with an s-cell halo in LDS, D (4 (16 + 2 s)^2 + 256) floats.  steps_per_launch = 0: the largest s <= 4 whose
 * LDS fits the library's budget, else the direct kernel (litho_peb_steps_per_launch(D) tells which; 0 for a bad D) -- the
 * budget is 0 today, the direct kernel being the faster one wherever it was timed (LABNOTES), so 0 means the direct kernel;
 * 1: the direct kernel; 2..4: the fused kernel, LITHO_E_ARG if its LDS exceeds the 160 KiB of a workgroup (D = 32 always does).
 * The steps left over by steps mod s run as a shorter last launch.  The result does NOT depend on steps_per_launch, bit for
 * bit, two calls give the same bits, and a batch equals its volumes baked one at a time: no atomics, no workgroup reads what
 * another writes.  Launches ping-pong h and q between the outputs and work.  Asynchronous, no allocation, no host wait: it can
 * be captured into a graph (an explicit steps_per_launch whose LDS exceeds 64 KiB raises the fused kernel's dynamic-LDS limit
 * on its first call per device: make that call once before capturing).
 * litho_peb_rate: acid_dose, slowness and the optional inhibitor (NULL: not written) fp32 [B,D,n,n], not overlapping; k_amp > 0
 * and finite, Mack's parameters and the surface factor as litho_develop_rate checks them.  One kernel, asynchronous.
 * All: a null pointer, D outside 1..32, n outside 1..16384, B < 1 or B D > 65535: LITHO_E_ARG before any GPU call. */
int litho_peb_expose(const float *image, int volumes, int D, int n, const float *gains_host, int n_gains, double C, float *acid,
                     void *stream);
int litho_peb_min_steps(double sigma_acid_nm, double sigma_quencher_nm, double vertical_scale, double thickness_nm, int D,
                        double pixel_nm);
size_t litho_peb_work_bytes(int B, int D, int n);
int litho_peb_steps_per_launch(int D);
int litho_peb_bake(const float *acid_in, int B, int D, int n, double thickness_nm, double pixel_nm, double quencher0, double k_quench,
                   double k_loss, double sigma_acid_nm, double sigma_quencher_nm, double vertical_scale, double bake_time_s, int steps,
                   int steps_per_launch, float *acid, float *quencher, float *acid_dose, void *work, size_t work_bytes, void *stream);
int litho_peb_rate(const float *acid_dose, int B, int D, int n, double k_amp, double r_max, double r_min, double q, double m_th,
                   double surface_rate, double surface_depth_nm, double thickness_nm, float *slowness, float *inhibitor, void *stream);

/* ---- Gradients through the bake (csrc/peb.hip; checked against the float64 restatement tests/peb_grad_oracle.py, itself pinned to
 * central differences of tests/peb_oracle.py).  The discrete adjoint of the S bake steps above, for a real loss l on the bake's
 * outputs (h_S, q_S, a_S) with cotangents gh = dl/dh_S, gq = dl/dq_S, ga = dl/da_S (any may be absent = zero, not all).
 *
 * Forward step k = 0 .. S-1, (h_k, q_k, a_k) -> (h_k+1, q_k+1, a_k+1):  hd = A_h h_k, qd = A_q q_k with A_s the diffusion line
 * (A_s = I when sigma_s = 0);  R = beta hd qd / (1 + beta (hd + qd)), or (hd < qd) ? hd : qd when beta = +inf;
 * h_k+1 = (hd - R) fl;  q_k+1 = qd - R;  a_k+1 = a_k + half_dt (h_k + h_k+1).  With mirror faces A_s = I + lambda (graph
 * Laplacian of the grid) is symmetric: its transpose is the same stencil with the same face rule.
 *
 * Backward step.  abar = ga throughout.  hbar_S = gh, qbar_S = gq; for k = S-1 .. 0, with the step's own (hd, qd), all fp32, each
 * line a fixed sequence of single operations, per cell:
 *   hp  = hbar_k+1 + half_dt abar
 *   finite beta:    Dn = 1 + beta (hd + qd);  R_h = beta qd (1 + beta qd) / (Dn Dn);  R_q = beta hd (1 + beta hd) / (Dn Dn)
 *                   (each left to right: ((beta qd) (1 + beta qd)) / (Dn Dn))
 *   instantaneous:  R_h = (hd < qd) ? 1 : 0;  R_q = 1 - R_h                 (the forward's own comparison)
 *   f = fl hp;  u = f (1 - R_h) - qbar_k+1 R_h;  v = qbar_k+1 (1 - R_q) - f R_q
 *   hbar_k = A_h u + half_dt abar,  qbar_k = A_q v:  x + lxy (((W + E) + (S + N)) - 4 x) + lz ((U + Dn) - 2 x) on u and on v, the
 *   neighbours' u, v evaluated by the same lines at the neighbour cells (a gather; a cell at a face takes itself).
 * Results: dl/dh_0 = hbar_0 and qbar_0; the initial quencher is uniform, so dl/dquencher0 of a volume is the sum of its qbar_0.
 * u and v are convex combinations of (f, -qbar) and (-f, qbar) and A_s has non-negative rows that sum to 1, so
 * |hbar_0|, |qbar_0| <= G = max(|gh|_inf, |gq|_inf) + bake_time |ga|_inf.
 *
 * litho_peb_bake_vjp is stateless: it runs its own forward sweep from acid_in and keeps (h_k, q_k) at k = c, 2c, .. < S, c =
 * checkpoint_every in 1 .. S; the backward sweep takes the segments of c steps last to first, re-runs each from its checkpoint
 * through the one step function while taping (hd, qd), then runs its backward steps -- one launch per step, a thread per cell,
 * no atomics and no scatter: two calls give the same bits, the bits do not depend on c, and a batch equals its volumes one at a
 * time.  work: litho_peb_vjp_work_bytes(B, D, n, steps, c) = (2 (ceil(S / c) - 1) + 2 c + 8) volumes of B D n n floats (the
 * checkpoints, one segment's tape, the ping-pong of (h, q) and of (hbar, qbar)); 0 for a bad argument; 16-byte aligned, less is
 * LITHO_E_WORKSPACE.  The physical arguments are litho_peb_bake's, checked alike.  grad_acid, grad_quencher, grad_acid_dose
 * (gh, gq, ga; NULL = zero) and the outputs grad_acid_in (hbar_0) and grad_quencher_in (qbar_0, NULL: not returned) are fp32
 * [B,D,n,n].  LITHO_E_ARG: all three cotangents NULL, steps below litho_peb_min_steps(...) or above 65536, c outside 1 .. steps,
 * a bad volume, an output overlapping an input, the other output or work, an input overlapping work.  NaN in the acid propagates
 * by arithmetic and is not otherwise specified.  Asynchronous, no allocation, no host wait.
 *
 * litho_peb_expose_vjp: the exposure h0[g] = 1 - exp(-(C gain_g) I) backwards, grad_image = sum_g (C gain_g) exp(-(C gain_g) I)
 * grad_acid[g], the gains in ascending order, double per cell, rounded to fp32 once; image, grad_image fp32 [volumes,D,n,n],
 * grad_acid fp32 [n_gains volumes,D,n,n] gain-major, grad_image overlapping neither; otherwise litho_peb_expose's checks. */
size_t litho_peb_vjp_work_bytes(int B, int D, int n, int steps, int checkpoint_every);
int litho_peb_bake_vjp(const float *acid_in, int B, int D, int n, double thickness_nm, double pixel_nm, double quencher0, double k_quench,
                       double k_loss, double sigma_acid_nm, double sigma_quencher_nm, double vertical_scale, double bake_time_s, int steps,
                       int checkpoint_every, const float *grad_acid, const float *grad_quencher, const float *grad_acid_dose,
                       float *grad_acid_in, float *grad_quencher_in, void *work, size_t work_bytes, void *stream);
int litho_peb_expose_vjp(const float *image, int volumes, int D, int n, const float *gains_host, int n_gains, double C,
                         const float *grad_acid, float *grad_image, void *stream);

/* ---- Gradients with respect to the bake's parameters (csrc/peb.hip; checked against the float64 restatement
 * tests/resist_param_oracle.py, itself pinned to central differences of tests/peb_oracle.py).  The six numbers of a bake step are
 * theta = (lxy_h, lz_h, lxy_q, lz_q, beta, fl).  In the notation of the backward step above -- hp = hbar_k+1 + half_dt abar,
 * qb = qbar_k+1, (u, v) its result, (hd, qd) the step's tape -- and with (h_k, q_k) the state at the START of step k, the backward
 * step k contributes per cell
 *   slot 0  lxy_h   u (((W + E) + (S + N)) - 4 x)  on x = h_k      slot 2  lxy_q   v (((W + E) + (S + N)) - 4 x)  on x = q_k
 *   slot 1  lz_h    u ((U + Dn) - 2 x)             on x = h_k      slot 3  lz_q    v ((U + Dn) - 2 x)             on x = q_k
 *   slot 4  beta    -(fl hp + qb) hd qd / (1 + beta (hd + qd))^2
 *   slot 5  fl      hp (hd - R),  R = beta hd qd / (1 + beta (hd + qd)), or (hd < qd) ? hd : qd when beta = +inf
 * and grad_step[b][slot] is the sum of these over the steps k = S-1 .. 0 and the cells of volume b: dl/dtheta with half_dt held
 * fixed.  The neighbours follow the forward's face rule (the cell itself beyond a face).  The slots of a species that does not
 * diffuse are exactly 0; at step 0 q_k is uniform, so its two terms are 0; slot 4 is exactly 0 for an instantaneous step, whose
 * R = min(hd, qd) holds no beta.  Each term is formed in double from the fp32 operands (u, v, hp, qb, the tape and the state as
 * the fp32 sweep has them) and the sums are kept in double.
 *
 * litho_peb_bake_vjp_params: the arguments and checks of litho_peb_bake_vjp, and grad_step, device double [B][6], 16-byte aligned
 * and not NULL (LITHO_E_ARG), overlapping neither an input, nor an output, nor work (LITHO_E_ARG).  grad_acid_in and
 * grad_quencher_in are written as litho_peb_bake_vjp writes them, bit for bit: the same forward launches, the same two functions
 * in the backward step.  The tape of a segment keeps four volumes per step, (hd, qd) and the state after the step, which is the
 * next step's (h_k, q_k) -- the forward's own bits, no recomputation.  work: litho_peb_vjp_params_work_bytes(B, D, n, steps, c) =
 * (2 (ceil(S / c) - 1) + 4 c + 8) volumes of B D n n floats, rounded up to 16 bytes, then B D ceil(n n / 256) slots of six
 * doubles, one per workgroup of a backward launch; 0 for a bad argument; 16-byte aligned, less is LITHO_E_WORKSPACE.  No atomics:
 * a 256-thread workgroup adds its six terms in a fixed tree (within each wave of 64 the upper half onto the lower, 32, 16 .. 1,
 * then the four waves in ascending order) and one thread adds the result into the workgroup's own slot, zeroed at the start of
 * the call; the backward steps are successive launches on one stream, so a slot's additions come in the order k = S-1 .. 0
 * whatever c is.  A last kernel adds the D ceil(n n / 256) slots of volume b, which lie planes ascending, then workgroups
 * ascending: thread i of one workgroup takes the slots i, i + 256, .. in ascending order, then the same tree.  So grad_step has the
 * same bits in two calls, for every c, and for a volume alone or inside a batch.  Asynchronous, no allocation, no host wait.
 *
 * litho_peb_param_chain: host only, no GPU call.  grad_param[5] = d/d(k_quench, k_loss, sigma_acid, sigma_quencher,
 * vertical_scale) from grad_step[6] (host doubles) by the derivative of the step parameters' own formulas (section 2 of the bake)
 * at a FIXED step count S, which is an integer the caller holds fixed:  d lxy / d sigma = 2 lxy / sigma = sigma / (S pixel^2),
 * d lz / d sigma = 2 lz / sigma,  d lz / d vertical_scale = 2 lz / vertical_scale  (each 0 at a zero length or scale),
 * d beta / d k_quench = dt (the result is 0 for k_quench = +inf),  d fl / d k_loss = -dt fl.  This is the analytic derivative in
 * double, not the derivative of the fp32 rounding of the step parameters.  bake_time is a process setting and is not
 * differentiated; the quencher loading's gradient stays the sum of grad_quencher_in over a volume.  LITHO_E_ARG: a NULL pointer,
 * steps outside litho_peb_min_steps(...) .. 65536, k_quench negative or NaN, k_loss, bake_time or pixel outside their domains.
 *
 * litho_peb_expose_vjp_params: dl/dC of the exposure h0[g] = 1 - exp(-(C gain_g) I) for the cotangent grad_acid = dl/dh0:
 * grad_C[g][v] = sum over the cells of volume v of grad_acid[g] (gain_g I) exp(-(C gain_g) I), device double [n_gains][volumes],
 * 16-byte aligned, one number per gain and volume (the caller adds them).  Each term in double; a cell whose acid is NaN
 * (1 - exp negative or NaN) contributes 0 whatever its cotangent holds.  The sums as above: a workgroup's fixed tree into its own
 * slot, then the D ceil(n n / 256) slots of a gained volume, planes ascending, by one workgroup in a fixed order; no atomics,
 * the same bits in two calls and for a volume alone or in a batch.  The arguments and checks of litho_peb_expose_vjp; work:
 * litho_peb_expose_params_work_bytes(volumes, D, n, n_gains) = n_gains volumes D ceil(n n / 256) doubles (0 for a bad argument),
 * 16-byte aligned, less is LITHO_E_WORKSPACE; grad_C and work overlap nothing (LITHO_E_ARG).  Asynchronous. */
size_t litho_peb_expose_params_work_bytes(int volumes, int D, int n, int n_gains);
int litho_peb_expose_vjp_params(const float *image, int volumes, int D, int n, const float *gains_host, int n_gains, double C,
                                const float *grad_acid, double *grad_C, void *work, size_t work_bytes, void *stream);
size_t litho_peb_vjp_params_work_bytes(int B, int D, int n, int steps, int checkpoint_every);
int litho_peb_bake_vjp_params(const float *acid_in, int B, int D, int n, double thickness_nm, double pixel_nm, double quencher0,
                              double k_quench, double k_loss, double sigma_acid_nm, double sigma_quencher_nm, double vertical_scale,
                              double bake_time_s, int steps, int checkpoint_every, const float *grad_acid, const float *grad_quencher,
                              const float *grad_acid_dose, float *grad_acid_in, float *grad_quencher_in, double *grad_step, void *work,
                              size_t work_bytes, void *stream);
int litho_peb_param_chain(double thickness_nm, double pixel_nm, double k_quench, double k_loss, double sigma_acid_nm,
                          double sigma_quencher_nm, double vertical_scale, double bake_time_s, int D, int steps, const double *grad_step,
                          double *grad_param);

/* ---- Gradients through development (csrc/develop_grad.hip; checked against the float64 restatement
 * tests/develop_grad_oracle.py, itself pinned to central differences of tests/develop_oracle.py).  The arrival time T of
 * litho_develop_time is the fixed point T_i = G_i(T at i's neighbours, s_i) of the Godunov update of section 3 above.  For a
 * reached cell i that is no wall the update used k = 1, 2 or 3 axes; on a used axis j the upwind value is a_j, the smaller of the
 * two neighbours (plane 0's z axis: the resist top, a = 0 at spacing hz / 2, no upstream cell).  T_i satisfies
 * sum_j w_j (T_i - a_j)^2 = s_i^2, w_j = 1 / h_j^2; with P_i = sum_j w_j (T_i - a_j), implicit differentiation gives
 *   dT_i / da_j = alpha_ij = w_j (T_i - a_j) / P_i   (non-negative, summing to 1 over the used axes),
 *   dT_i / ds_i = sigma_i = s_i / P_i               (= h_1 in the one-axis branch).
 * For a real loss l with cotangent g = dl/dT the adjoint variable solves lambda_i = g_i + sum_j alpha_ji lambda_j, the sum over
 * those of i's six neighbours j whose update took i as the upwind cell of its axis, and dl/ds_i = lambda_i sigma_i.  The rules
 * that make this well defined:
 *   branch     k and the T_i in the coefficients are recomputed from the neighbours' STORED T and from s_i as the update decides
 *              (axes sorted by a, u <= delta_2, u <= delta_3), in double from the fp32 inputs with h = fp32(pixel),
 *              hz = fp32(thickness / D); alpha and sigma are rounded to fp32 once.  (The stored fp32 fixed point may differ from
 *              G_i(T) by an ulp.  The derivative is continuous across a branch switch -- alpha -> 0 for the axis that drops out --
 *              so a near-tie decided differently in fp32 and in double moves the result by rounding, not by a jump.)
 *   axis ties  a tie between the two neighbours of one axis goes to the LOWER-index neighbour: on the symmetry line of a
 *              symmetric pattern the result is a valid but one-sided subgradient.
 *   strict     a link counts only if the upwind cell's stored T is strictly below the stored T_i, otherwise it is dropped: the
 *              dependency graph is then acyclic (ordered by T) and the iteration below reaches its fixed point in finitely
 *              many sweeps.
 *   no gradient  a wall (s not finite and positive) or a cell with T = +inf gets gradient 0, and its cotangent is ignored
 *              whatever it holds, NaN and inf included.
 *
 * litho_develop_time_vjp: slowness, T, grad_T, grad_slowness fp32 [B,D,n,n]; T MUST be the converged output of
 * litho_develop_time for the same slowness and geometry (documented, not verifiable).  Three stages.  A pointwise kernel writes
 * four fp32 per cell into work, the signed link weights of the three axes (positive: the upwind cell is the lower-index
 * neighbour) and sigma.  Then the tiled gather iteration, the decomposition of litho_develop_time: a workgroup holds lambda and
 * the links of a 16 x 16 x D tile with a one-cell halo in LDS, D (3 . 18 . 18 + 16 . 16) floats = 4912 D bytes (153.5 KiB at D = 32;
 * every D from 1 to 32 works), the cotangent read from global memory by the thread that owns the column; columns in two colours, a Gauss-Seidel sweep up and down each column, 8 rounds per launch, lambda ping-ponged between
 * grad_slowness and work.  A cell's update is a pure gather, lambda_i = g_i + the terms of the neighbours whose link points at
 * i, added in the fixed order x-, x+, y-, y+, z-, z+, each one fp32 multiplication and one addition: no atomics, no scatter.  A
 * launch in which no cell's BIT PATTERN changed ends the loop; a closing pointwise kernel writes lambda sigma (0 where sigma is
 * 0).  Each cell's final value is that fixed expression on the final values of cells with strictly larger T, so the bits depend
 * on neither the tile schedule, nor the batch, nor the launch at which the loop stops: two calls give the same bits, and a batch
 * equals its volumes one at a time.  READS BACK every fourth launch like litho_develop_time and cannot be captured into a graph.
 * *launches_host = the gather launches up to and including the first that changed nothing; after max_iterations (1..65536)
 * without one: LITHO_E_NOCONV, *launches_host = max_iterations and grad_slowness holds nothing usable.  work:
 * litho_develop_vjp_work_bytes(B, D, n, max_iterations) device bytes (the flag words and five volumes; 0 for a bad argument),
 * 16-byte aligned; less is LITHO_E_WORKSPACE.  LITHO_E_ARG: a null pointer, a bad volume (as above), thickness or pixel not
 * positive and finite, grad_slowness overlapping an input, work overlapping anything.  No allocation.
 *
 * litho_develop_rate_vjp: the rate law backwards, for litho_develop_rate (kappa = C, x = the intensity, the doses as gains) and for
 * litho_peb_rate (kappa = k_amp, x = the acid dose, one gain of 1) alike.  With m = exp(-(kappa g) x), X = (1 - m)^q,
 * r = (R X / (a + X) + r_min) f, R = r_max (a + 1), f the surface factor of the plane, s = 1 / r:
 *   grad_x = sum over the gains of grad_slowness[gain] . (-s^2 f R a / (a + X)^2 . q (1 - m)^(q-1) . (kappa g) m),
 * double per cell, the gains in ascending order, rounded to fp32 once; a cell whose slowness is NaN (1 - m negative or NaN: a wall)
 * contributes 0 whatever its cotangent holds.  x, grad_x fp32 [volumes,D,n,n], grad_slowness fp32 [n_gains volumes,D,n,n]
 * gain-major, grad_x overlapping neither; the parameters as litho_develop_rate checks them.  One kernel, asynchronous. */
size_t litho_develop_vjp_work_bytes(int B, int D, int n, int max_iterations);
int litho_develop_time_vjp(const float *slowness, const float *T, const float *grad_T, int B, int D, int n, double thickness_nm,
                           double pixel_nm, int max_iterations, float *grad_slowness, void *work, size_t work_bytes,
                           int *launches_host, void *stream);
int litho_develop_rate_vjp(const float *x, int volumes, int D, int n, const float *gains_host, int n_gains, double kappa, double r_max,
                           double r_min, double q, double m_th, double surface_rate, double surface_depth_nm, double thickness_nm,
                           const float *grad_slowness, float *grad_x, void *stream);

/* ---- Gradients with respect to the rate law's parameters (csrc/develop_grad.hip; checked against tests/resist_param_oracle.py,
 * itself pinned to central differences of the rate oracles).  For litho_develop_rate (kappa = C, the doses as gains) and
 * litho_peb_rate (kappa = k_amp, one gain of 1) alike, in the notation of litho_develop_rate_vjp with b = 1 - m, X = b^q,
 * R = r_max (a + 1), a = (q + 1) / (q - 1) (1 - m_th)^q:
 *   slot 0  ds/dkappa = -s^2 f R a / (a + X)^2 q b^(q-1) (g x) m       (litho_develop_rate_vjp's line with db = (g x) m)
 *   slot 1  ds/dR     = -s^2 f X / (a + X)                              at fixed a
 *   slot 2  ds/dr_min = -s^2 f
 *   slot 3  ds/dq     = -s^2 f R a / (a + X)^2 X ln b                   at fixed a; 0 at b = 0
 *   slot 4  ds/da     = -s^2 f (R / (a + 1)) X (X - 1) / (a + X)^2      at fixed r_max, R following a
 *   slot 5  ds/df     = -s / f
 * litho_develop_rate_vjp_params: plane_sums[gained plane][slot] = the sum over the cells of the plane of grad_slowness times the
 * slot's derivative, device double [n_gains volumes D][6], gain-major like grad_slowness, 16-byte aligned; every term in double, a
 * wall (1 - m negative or NaN) contributes 0 whatever its cotangent holds.  Two kernels, no atomics: a 256-thread workgroup adds
 * its terms in a fixed tree (as litho_peb_bake_vjp_params) into its own slot of work, and one workgroup per gained plane adds the
 * plane's ceil(n n / 256) slots in a fixed order: the same bits in two calls and for a volume alone or in a batch.  The
 * arguments and checks of litho_develop_rate_vjp without grad_x; work: litho_develop_rate_params_work_bytes(volumes, D, n,
 * n_gains) = n_gains volumes D ceil(n n / 256) slots of six doubles (0 for a bad argument), 16-byte aligned, less is
 * LITHO_E_WORKSPACE; plane_sums and work overlap nothing (LITHO_E_ARG).  Asynchronous, no allocation, no host wait.
 *
 * litho_develop_rate_param_chain: host only, no GPU call.  From plane_sums (HOST doubles [groups][D][6], a group = one gained
 * volume) grad_param[group][7] = d/d(kappa, r_max, r_min, q, m_th, surface_rate, surface_depth), the planes added in ascending
 * order:  kappa: slot 0;  r_max: (a + 1) slot 1;  r_min: slot 2;  q: slot 3 + slot 4 da/dq,  da/dq = a (1 / (q + 1) - 1 / (q - 1)
 * + ln(1 - m_th));  m_th: slot 4 da/dm_th,  da/dm_th = -q a / (1 - m_th);  and with f_d = 1 - (1 - r0) exp(-z_d / delta),
 * z_d = thickness (d + 1/2) / D:  surface_rate: sum_d slot 5 exp(-z_d / delta);  surface_depth: sum_d slot 5 (-(1 - r0)
 * exp(-z_d / delta) z_d / delta^2).  LITHO_E_ARG: a NULL pointer, groups < 1, D outside 1..32, a parameter outside
 * litho_develop_rate's domain.  NOT built: the gradients of a MackResist's own Gaussian diffusion lengths. */
size_t litho_develop_rate_params_work_bytes(int volumes, int D, int n, int n_gains);
int litho_develop_rate_vjp_params(const float *x, int volumes, int D, int n, const float *gains_host, int n_gains, double kappa,
                                  double r_max, double r_min, double q, double m_th, double surface_rate, double surface_depth_nm,
                                  double thickness_nm, const float *grad_slowness, double *plane_sums, void *work, size_t work_bytes,
                                  void *stream);
int litho_develop_rate_param_chain(double r_max, double r_min, double q, double m_th, double surface_rate, double surface_depth_nm,
                                   double thickness_nm, int D, int groups, const double *plane_sums, double *grad_param);

/* ---- Forward mode (tangents) of the resist chain (csrc/peb.hip, csrc/develop_grad.hip; checked against the float64 restatement
 * tests/resist_tangent_oracle.py, itself pinned to central differences of the forward oracles and to the adjoint oracles by
 * <g, J v> = <J^T g, v>).  Each call is the tangent-linear twin of one adjoint call above and carries P directions,
 * 1 <= P <= LITHO_TANGENT_MAX; direction-major volumes are fp32 [P, B, D, n, n] and P B D <= 65535.  A direction alone has the
 * bits of that direction inside a batch of P, a volume alone the bits of that volume inside a batch of B, two calls the same
 * bits.  No atomics, no allocation.  The checks are those of the adjoint twin: LITHO_E_ARG before any GPU call, LITHO_E_WORKSPACE
 * for too little workspace; an output overlaps no input, no other output and no workspace (LITHO_E_ARG).
 *
 * litho_peb_expose_jvp: the tangent of litho_peb_expose for the directions (dC_p, dI_p), dC HOST doubles [P], dimage device fp32
 * [P, volumes, D, n, n] or NULL = 0:
 *   dacid[p][gain][cell] = exp(-(C g) I) ((g I) dC_p + (C g) dI_p),
 * in double per cell, rounded once; exactly 0 where the acid is NaN (1 - exp negative or NaN), whatever dimage holds there.
 * dacid fp32 [P, n_gains volumes, D, n, n], gain-major inside a direction like litho_peb_expose's acid.
 *
 * litho_peb_bake_jvp: the S bake steps of litho_peb_bake with their tangent, one step per launch, a thread per cell with the primal
 * and all P tangents.  The primal goes through the forward's own step function: acid, quencher, acid_dose (each fp32 [B,D,n,n] or
 * NULL = not written) are litho_peb_bake's bits.  Per direction p: dacid_in device fp32 [P,B,D,n,n] or NULL = 0 (dh_0), dquencher0
 * HOST doubles [P] (the uniform dq_0, the direction of the quencher loading) and dstep HOST doubles [P][6] = d(lxy_h, lz_h, lxy_q,
 * lz_q, beta, fl), the three rounded to fp32 once; half_dt is fixed (bake_time_s is a process setting).  With Lxy(x) = ((W + E) +
 * (S + N)) - 4 x and Lz(x) = (U + Dn) - 2 x under the forward's mirror rule, (h, q) the state at the start of the step, (hd, qd)
 * the step's species after diffusion and R its neutralisation, one tangent step in fp32, every line a fixed sequence of single
 * operations, added left to right:
 *   dhd = dh + lxy_h Lxy(dh) + lz_h Lz(dh) + dlxy_h Lxy(h) + dlz_h Lz(h)        (dhd = dh when the acid does not diffuse; dqd likewise)
 *   finite beta:    dR = (R_h dhd + R_q dqd) + (hd qd / (Dn Dn)) dbeta,   Dn = 1 + beta (hd + qd),
 *                   R_h = beta qd (1 + beta qd) / (Dn Dn),  R_q = beta hd (1 + beta hd) / (Dn Dn)   (the adjoint's expressions)
 *   instantaneous:  dR = hd < qd ? dhd : dqd                                     (the forward's own comparison)
 *   dh' = (dhd - dR) fl + (hd - R) dfl,      dq' = dqd - dR,      da' = da + half_dt (dh + dh').
 * Outputs dacid, dquencher, dacid_dose fp32 [P,B,D,n,n] = (dh_S, dq_S, da_S); a direction of zeros comes back exactly 0.  work:
 * litho_peb_jvp_work_bytes(B, D, n, P) = (5 + 2 P) volumes (the ping-pong of the primal pair with its a, and the second side of
 * the P tangent pairs, whose first side is the outputs; 0 for a bad argument), 16-byte aligned; nothing scales with the step count.
 * The other arguments and their domain are litho_peb_bake's.
 *
 * litho_peb_param_tangent: host only.  dstep[6] from dparam[5] = d(kQuench, kLoss, acidDiffusionLength, quencherDiffusionLength,
 * verticalScale): the transpose of litho_peb_param_chain at the same fixed step count, analytic in double; 0 for a zero length or
 * scale and for kQuench = +inf.
 *
 * litho_develop_rate_jvp: the tangent of litho_develop_rate (kappa = C) and litho_peb_rate (kappa = k_amp, one gain of 1):
 *   dslowness[p][gain][cell] = ds/dx (kappa g) m dx_p  +  sum_j d_j dphi[p][plane d][j],   j = 0 .. 5 in this order,
 * ds/dx litho_develop_rate_vjp's line and d_j the six slot derivatives of litho_develop_rate_vjp_params.  dx device fp32
 * [P, volumes, D, n, n] or NULL = 0; dphi device doubles [P][D][6], 16-byte aligned (slot 5, the surface factor, differs per plane).
 * Double per cell, rounded once; a wall (1 - m negative or NaN) gives exactly 0.  dslowness fp32 [P, n_gains volumes, D, n, n].
 *
 * litho_develop_rate_param_tangent: host only.  dphi[D][6] from dparam[7] = d(kappa, r_max, r_min, q, m_th, surface_rate,
 * surface_depth): the transpose of litho_develop_rate_param_chain.
 *
 * litho_develop_time_jvp: the tangent of the Godunov fixed point of litho_develop_time.  With the links (alpha on the three axes,
 * sigma) of litho_develop_time_vjp, computed once per volume and shared by the P directions,
 *   dT_i = sigma_i ds_i (+) |l_x| dT_up(x) (+) |l_y| dT_up(y) (+) |l_z| dT_up(z)     in this order,
 * each term one fp32 multiplication and one addition, the upwind neighbour of an axis the one the link's sign names, a zero link
 * adding nothing; where sigma_i = 0 (a wall, or T = +inf) dT_i = 0 exactly whatever ds_i holds.  A cell gathers along its own links
 * from cells with strictly smaller T, so by induction from the sources of the graph the bits depend on neither the schedule, nor
 * the batch, nor P, nor the launch at which the iteration stops.  The tiling, colours, rounds per launch, bitwise fixed point and
 * launch cap (LITHO_E_NOCONV) are litho_develop_time_vjp's; a column is swept down and then up.  dslowness, dT fp32 [P,B,D,n,n].
 * work: litho_develop_jvp_work_bytes(B, D, n, P, max_iterations) = the flag words, the links (4 volumes) and one side of the
 * ping-pong (P volumes), 16-byte aligned.  Waits for the device while it iterates, like its twin. */
#define LITHO_TANGENT_MAX 16
int litho_peb_expose_jvp(const float *image, int volumes, int D, int n, const float *gains_host, int n_gains, double C, int P,
                         const double *dC_host, const float *dimage, float *dacid, void *stream);
size_t litho_peb_jvp_work_bytes(int B, int D, int n, int P);
int litho_peb_bake_jvp(const float *acid_in, int B, int D, int n, double thickness_nm, double pixel_nm, double quencher0,
                       double k_quench, double k_loss, double sigma_acid_nm, double sigma_quencher_nm, double vertical_scale,
                       double bake_time_s, int steps, int P, const float *dacid_in, const double *dquencher0_host,
                       const double *dstep_host, float *acid, float *quencher, float *acid_dose, float *dacid, float *dquencher,
                       float *dacid_dose, void *work, size_t work_bytes, void *stream);
int litho_peb_param_tangent(double thickness_nm, double pixel_nm, double k_quench, double k_loss, double sigma_acid_nm,
                            double sigma_quencher_nm, double vertical_scale, double bake_time_s, int D, int steps,
                            const double *dparam, double *dstep);
int litho_develop_rate_jvp(const float *x, int volumes, int D, int n, const float *gains_host, int n_gains, double kappa, double r_max,
                           double r_min, double q, double m_th, double surface_rate, double surface_depth_nm, double thickness_nm,
                           int P, const float *dx, const double *dphi, float *dslowness, void *stream);
int litho_develop_rate_param_tangent(double r_max, double r_min, double q, double m_th, double surface_rate, double surface_depth_nm,
                                     double thickness_nm, int D, const double *dparam, double *dphi);
size_t litho_develop_jvp_work_bytes(int B, int D, int n, int P, int max_iterations);
int litho_develop_time_jvp(const float *slowness, const float *T, const float *dslowness, int B, int D, int n, int P,
                           double thickness_nm, double pixel_nm, int max_iterations, float *dT, void *work, size_t work_bytes,
                           int *launches_host, void *stream);

/* ---- Mask gradients of Hopkins imaging (csrc/socs_grad.hip; no reference counterpart, checked against tests/socs_grad_oracle.py).
 * With F[q][i] = exp(+2 pi i (i - c)(q - c) / N), c = pn / 2, q, i in [0, pn), the engine's chain at shift (0,0) is L(X) = F X F^T,
 * the coherent fields are E_k = L(phi_k . M) and I = sum_k |E_k|^2.  For a real loss l with G = dl/dI,
 *   g = dl/dRe M + i dl/dIm M = 2 sum_p sum_k conj(phi_pk) . L^H(G_p . E_pk),   L^H(Y) = conj(F) Y conj(F)^T,
 * torch's convention for the gradient of a complex leaf (dl = Re <g, dM>).  pn and N powers of two, 16..4096 (anything else, a
 * batch < 1 or a null pointer: LITHO_E_ARG), N >= pn (LITHO_E_NSMALL); every check is made before any launch.  All calls are
 * asynchronous, allocate nothing and wait for nothing.
 *
 * litho_socs_fields: fields[b] = L(kernels[b] . maskFT), b < batch; kernels, fields complex64 [batch,pn,pn], maskFT complex64 [pn,pn];
 * fields must not overlap kernels. */
int litho_socs_fields(const void *kernels, const void *maskFT, int batch, int pn, int N, void *fields, void *stream);
/* litho_socs_vjp: grad (+)= 2 sum_b conj(kernels[b]) . L^H(gradI[b / K] . L(kernels[b] . maskFT)), b < groups K ascending, one running
 * fp32 sum per component and no atomics: the result is deterministic, and calls on consecutive chunks of the kernels with
 * accumulate != 0 give the chunk-ordered sum (accumulate == 0 starts from zero).  kernels complex64 [groups K,pn,pn] with item
 * g K + k = kernel k of plane g, gradI fp32 [groups,pn,pn], grad complex64 [pn,pn].  work: litho_socs_vjp_work_bytes(groups, K, pn)
 * device bytes (the field stack; 0 for a bad argument), less is LITHO_E_WORKSPACE. */
size_t litho_socs_vjp_work_bytes(int groups, int K, int pn);
int litho_socs_vjp(const void *kernels, const void *maskFT, const float *gradI, int groups, int K, int pn, int N, void *grad,
                   int accumulate, void *work, size_t work_bytes, void *stream);
/* litho_socs_jvp: forward mode through the same fields.  The image is quadratic in the mask spectrum, so along a direction dM
 *   dI[p][g] (+)= 2 sum_{k < K} Re( conj(E_gk) . L(kernels[g K + k] . dMaskFT[p]) ),   E_gk = L(kernels[g K + k] . maskFT),
 * k ascending, one running fp32 sum per output element and no atomics; accumulate != 0 continues from dI, so calls on consecutive
 * chunks of the kernels give the chunk-ordered sum.  kernels complex64 [groups K,pn,pn] as for litho_socs_vjp, maskFT complex64
 * [pn,pn], dMaskFT complex64 [P,pn,pn], dI fp32 [P,groups,pn,pn]; 1 <= P <= LITHO_SOCS_JVP_MAX_DIRECTIONS, groups <= 65535.  The
 * directions run one after another through the same launches: direction p's bits depend neither on P nor on the other
 * directions, and two calls give the same bits.  A tangent field is folded against its primal field as it leaves the second row
 * pass and is never stored.  work: litho_socs_jvp_work_bytes(groups, K, P, pn) device bytes -- the chunk's field stack, one
 * direction's stack between its two passes and one direction's real planes; nothing grows with P (0 for a bad argument), less is
 * LITHO_E_WORKSPACE.  Domain and codes as litho_socs_vjp, and LITHO_E_ARG for P outside 1..16; every check precedes any launch. */
size_t litho_socs_jvp_work_bytes(int groups, int K, int P, int pn);
int litho_socs_jvp(const void *kernels, const void *maskFT, const void *dMaskFT, int P, int groups, int K, int pn, int N, float *dI,
                   int accumulate, void *work, size_t work_bytes, void *stream);
/* litho_socs_image_batch: the Hopkins image of MANY mask spectra through one kernel set in one call,
 *   out[b][g] (+)= sum_{k < K} | L(kernels[g K + k] . maskFTs[b]) |^2,   b < tiles, g < groups,
 * k ascending, each term added as fmaf(re, re, im im) to one running fp32 sum per output element that lives in LDS through the
 * second row pass: no K-plane stack is written and nothing is atomic.  accumulate != 0 starts the sums from out, so calls on
 * consecutive chunks of the kernels continue the same sequence of additions (bit for bit what one call on all of them gives);
 * accumulate == 0 starts from zero.  The bits of out[b] depend on maskFTs[b] and the kernels alone: not on tiles, on b, or on how
 * the caller cuts the spectra into calls.  kernels complex64 [groups K,pn,pn] as for litho_socs_vjp (groups = the planes of a
 * through-focus set), maskFTs complex64 [tiles,pn,pn], out fp32 [tiles,groups,pn,pn].  work: litho_socs_image_batch_work_bytes(tiles,
 * groups, K, pn) device bytes = tiles groups K pn^2 complex (the fields between the two row passes) + tiles groups pn^2 floats (the
 * image in the transposed layout); 0 for a bad argument, less is LITHO_E_WORKSPACE.  Domain and codes as litho_socs_vjp, and
 * LITHO_E_ARG for tiles < 1, groups > 65535 or tiles groups K pn > INT_MAX lines; every check precedes any launch. */
size_t litho_socs_image_batch_work_bytes(int tiles, int groups, int K, int pn);
int litho_socs_image_batch(const void *kernels, const void *maskFTs, int tiles, int groups, int K, int pn, int N, float *out,
                           int accumulate, void *work, size_t work_bytes, void *stream);
/* litho_socs_vjp_batch: the mask gradients of MANY windows through one kernel set in one call,
 *   grads[b] (+)= 2 sum_{j < groups K} conj(kernels[j]) . L^H( gradIs[b][j / K] . L(kernels[j] . maskFTs[b]) ),   b < tiles,
 * j ascending, each term added as litho_socs_vjp adds it to one running fp32 sum per component: no atomics.  accumulate != 0 starts
 * the sums from grads, so calls on consecutive chunks of the kernels continue the same sequence of additions (bit for bit what one
 * call on all of them gives); accumulate == 0 starts from zero.  The bits of grads[b] depend on maskFTs[b], gradIs[b] and the kernels
 * alone: not on tiles, on b, or on how the caller cuts the windows into calls.  kernels complex64 [groups K,pn,pn] as for
 * litho_socs_vjp, maskFTs complex64 [tiles,pn,pn], gradIs fp32 [tiles,groups,pn,pn] (the layout of litho_socs_image_batch's out),
 * grads complex64 [tiles,pn,pn].  Two routes by pn: up to 2048 the sum over j is held in LDS through the adjoint's last row pass
 * and the adjoint stack is never stored after it; at 4096, where those sums do not fit, the adjoints are stored and summed tile by
 * tile by litho_socs_vjp's reduction.  Their sums are the same sequence; their bits may differ from litho_socs_vjp's, whose
 * transforms run in the other order.  work: litho_socs_vjp_batch_work_bytes(tiles, groups, K, pn) device bytes = tiles groups K
 * pn^2 complex (the field stack, turned into the adjoints in place) + tiles groups pn^2 floats (gradIs in the transposed layout); 0
 * for a bad argument, less is LITHO_E_WORKSPACE.  Domain and codes as litho_socs_image_batch; every check precedes any launch. */
size_t litho_socs_vjp_batch_work_bytes(int tiles, int groups, int K, int pn);
int litho_socs_vjp_batch(const void *kernels, const void *maskFTs, const float *gradIs, int tiles, int groups, int K, int pn, int N,
                         void *grads, int accumulate, void *work, size_t work_bytes, void *stream);

/* ---- Tiled imaging of large layouts (csrc/tiling.hip; no reference counterpart, checked against numpy slicing in
 * tests/tiling_oracle.py).  A layout larger than one window is imaged as `count` windows of nt x nt pixels on one pixel lattice;
 * each window's image is trusted on its core, the `core` x `core` pixels that start at (j0, j0), and the cores are disjoint.
 *
 * litho_tiles_stitch: image[p][place[t][0] + i][place[t][1] + j] = tiles[t][p][j0 + i][j0 + j],  0 <= i, j < core, t < count,
 * p < planes; a pixel outside [0, n) is skipped (an edge tile is clipped) and nothing else of image is written -- the caller
 * zeroes it.  tiles fp32 [count,planes,nt,nt], place device int32 [count][2] = (row, col), any integers, image fp32 [planes,n,n].
 * A pure copy, one wave per core row.  LITHO_E_ARG: a null pointer, count, planes, nt, core or n < 1, j0 < 0, j0 + core > nt,
 * or count planes core > INT_MAX rows.
 *
 * litho_tiles_seam: how much two neighbouring windows disagree where their cores meet.  neighbours device int32 [count][2] =
 * (right, lower) tile of tile t, the tiles whose windows lie `core` columns / rows further; a value outside [0, count) means none.
 * With a = tiles[t][p] and b = tiles[right][p], b[r][c] shows what a[r][c + core] shows, and
 *   out[t][p][0] = max over i < core, d in {0, 1} of | a[j0 + i][j0 + core - 1 + d] - b[j0 + i][j0 - 1 + d] |
 * -- the two pixel columns either side of the common core boundary, on the core's rows; out[t][p][1] likewise for the lower
 * neighbour on the two rows either side, over the core's columns.  NaN (0x7fc00000) where there is no neighbour; a NaN difference
 * is ignored by the maximum (fmaxf).  One wave per (tile, plane, side), lanes stride the line, the maximum through the xor
 * butterfly: no atomics, one fixed order.  out fp32 [count,planes,2], every element written.  LITHO_E_ARG: as above, and
 * j0 < 1 or j0 + core >= nt (both windows must hold both lines: a halo of at least one pixel).
 * Both calls are asynchronous, allocate nothing and wait for nothing. */
int litho_tiles_stitch(const float *tiles, int count, int planes, int nt, const int32_t *place, int j0, int core, float *image, int n,
                       void *stream);
int litho_tiles_seam(const float *tiles, int count, int planes, int nt, const int32_t *neighbours, int j0, int core, float *out,
                     void *stream);
/* The tiled inverse-lithography loop keeps ONE complex transmission `plane` [rows,cols] on the raster lattice (the cores of the
 * plan: rows = ny core, cols = nx core, core = pn - 2 halo) and place[t] = (row, col) of core t's first pixel in it.
 *
 * litho_tiles_cut: windows[t][r][c] = plane[place[t][0] - halo + r][place[t][1] - halo + c], and (fill_re, fill_im) where that lies
 * outside the plane; plane complex64 [rows,cols], windows complex64 [count,pn,pn], every element written.
 * litho_tiles_overlap_add: the cut's adjoint as a gather, plane[R][C] = sum over the tiles t whose window holds (R, C), t ascending,
 * of windows[t][R - place[t][0] + halo][C - place[t][1] + halo]: one thread per plane pixel, one running fp32 sum per component
 * from zero, what falls outside the plane dropped, no atomics; the result does not depend on the launch geometry.  Every
 * element of plane is written.
 * litho_tiles_unstitch: the stitch's adjoint, tiles[t][p][j0 + i][j0 + j] = image[p][place[t][0] + i][place[t][1] + j] for
 * 0 <= i, j < core where the image has that pixel, and zero everywhere else; image fp32 [planes,n,n], tiles fp32
 * [count,planes,nt,nt], every element written.
 * LITHO_E_ARG, before any launch: a null pointer, count < 1, a size < 1, halo < 0 or 2 halo >= pn, a core larger than the plane
 * (cut, overlap-add) or than the image (unstitch), j0 < 0 or j0 + core > nt, more than INT_MAX rows.  Asynchronous. */
int litho_tiles_cut(const void *plane, int rows, int cols, const int32_t *place, int count, int pn, int halo, float fill_re,
                    float fill_im, void *windows, void *stream);
int litho_tiles_overlap_add(const void *windows, int count, int pn, int halo, const int32_t *place, void *plane, int rows, int cols,
                            void *stream);
int litho_tiles_unstitch(const float *image, int n, const int32_t *place, int count, int planes, int nt, int j0, int core, float *tiles,
                         void *stream);

/* ---- Source gradients of Abbe imaging (csrc/socs_grad.hip; no reference counterpart, checked against tests/source_grad_oracle.py).
 * The weighted Abbe sum I = sum_s w_s |E_s|^2 is linear in the weights, and source point s is the coherent kernel roll(P, d_s) of
 * the field code above: E_s = L(roll(P, d_s) . M), L as documented for litho_socs_fields.  For a real loss l with G = dl/dI,
 *   dl/dw_s = <G, |E_s|^2> = sum_q G[q] |E_s[q]|^2:
 * one number per source point, independent of the weights, and no adjoint transform -- one forward field and a reduction.
 *
 * litho_source_sensitivity:
 *   sens[s] = sum_{g < groups} sum_{k < K} sum_q gradI[g][q] . | L( roll(pupils[g K + k], (dy_s, dx_s)) . maskFT )[q] |^2,   s < count,
 * roll(P, (dy, dx))[r][c] = P[(r - dy) mod pn][(c - dx) mod pn] (torch.roll(P, (dy, dx), (0, 1)), the reference's
 * imageformation.py:63).  shifts: device int32 [count][2] = (dy, dx), what litho_source_compact writes; any integers, a wrapping
 * shift is the modular index.  pupils complex64 [groups K,pn,pn] with item g K + k = pupil k of plane g (K > 1: pupil stacks that
 * share one image plane, such as the effective pupils of vector imaging; the (groups, K) convention of litho_socs_vjp), maskFT
 * complex64 [pn,pn], gradI fp32 [groups,pn,pn], sens fp32 [count], overwritten.  The list is walked in chunks of `batch` points and
 * work holds one chunk: litho_source_sensitivity_work_bytes(groups, K, batch, pn) device bytes, 8-byte aligned (batch groups K field
 * planes, one partial per line of them, one transposed copy of gradI; 0 for a bad argument), less is LITHO_E_WORKSPACE.  No
 * atomics and one fixed order for every sum: sens[s] depends on point s alone -- its bits do not change with batch, count, the
 * point's place in the list or the other points.  Domain as litho_socs_fields: pn, N powers of two, 16..4096, else LITHO_E_ARG;
 * N < pn: LITHO_E_NSMALL; count < 0, batch, groups or K < 1, a null pointer, or batch groups K pn > INT_MAX lines: LITHO_E_ARG;
 * every check is made before any launch.  count == 0: LITHO_OK, nothing is launched.  Asynchronous, no allocation, no host wait. */
size_t litho_source_sensitivity_work_bytes(int groups, int K, int batch, int pn);
int litho_source_sensitivity(const void *pupils, const void *maskFT, const float *gradI, int groups, int K, const int32_t *shifts,
                             int64_t count, int pn, int N, float *sens, int batch, void *work, size_t work_bytes, void *stream);

/* ---- Pupil gradients of Abbe imaging (csrc/socs_grad.hip; no reference counterpart, checked against tests/pupil_grad_oracle.py).
 * Notation of the source-gradient block: L(X) = F X F^T, L^H(Y) = conj(F) Y conj(F)^T, roll(P, (dy, dx))[r][c] =
 * P[(r - dy) mod pn][(c - dx) mod pn], M the mask spectrum [pn,pn], pupils P_j, j < groups K, plane g = j / K with image I_g,
 * weights w_s.  Forward model:  E_{s,j} = L(roll(P_j, d_s) . M),   I_g = sum_s w_s sum_{k < K} |E_{s,g K + k}|^2.
 * For a real loss l with G_g = dl/dI_g, in torch's convention for a complex leaf (dl = Re <g, dP>),
 *   g_j[r][c] = dl/dRe P_j + i dl/dIm P_j = 2 sum_s w_s conj(M[r'][c']) A_{s,j}[r'][c'],
 *   r' = (r + dy_s) mod pn,  c' = (c + dx_s) mod pn,   A_{s,j} = L^H(G_{j / K} . E_{s,j}):
 * each point's adjoint is multiplied by conj(M) in the mask frame, rolled back by -d_s, and summed.  SOCS cannot give this (its
 * kernels are eigenvectors of a TCC that depends on the pupil), so it costs one forward and one adjoint field per source point.
 * Wavefront gradient, where P = a . exp(2 pi i W) with a real and independent of W:  dl/dW = 2 pi Im(g . conj(P)), real [pn,pn]
 * per pupil.  Coefficient gradient, for W_p = W0_p + sum_j c_j B_j with real basis maps B_j shared by all planes:
 *   dl/dc_j = sum_p sum_cells (dl/dW_p) . B_j.
 *
 * litho_pupil_vjp: grad (+)= g of the list.  pupils complex64 [groups K,pn,pn], maskFT complex64 [pn,pn], gradI fp32 [groups,pn,pn],
 * shifts device int32 [count][2] = (dy, dx) (any integers), weights device fp32 [count] or NULL = all 1, grad complex64
 * [groups K,pn,pn].  The list is walked in chunks of `batch` points, items of a chunk point-major (item = point groups K + j); a
 * chunk is: the fields (rolled load, rows, transpose, rows, transpose: natural layout), L^H of G . E in place, then one reducing
 * pass in which every cell of every plane keeps one running fp32 sum over the chunk's points in ascending order, each term
 *   re += fma(2 w, fma(M.re, A.re, M.im A.im), .),   im += fma(2 w, fma(M.re, A.im, -(M.im A.re)), .)   read at (r', c'),
 * starting from grad for every chunk after the first or when accumulate != 0, from 0 otherwise.  Nothing is atomic and the
 * additions into a cell are the list's order: grad's bits do not depend on `batch`, and a list split over two calls, the second with
 * accumulate != 0, gives the bits of one call (another ORDER of the list is another rounding).  work holds one chunk:
 * litho_pupil_vjp_work_bytes(groups, K, batch, pn) = batch groups K pn^2 complex64 (0 for a bad argument), nothing of size count
 * pn^2; less is LITHO_E_WORKSPACE.  Sizes and codes as litho_source_sensitivity: pn, N powers of two, 16..4096, else LITHO_E_ARG;
 * N < pn: LITHO_E_NSMALL; count < 0, batch, groups or K < 1, a null pointer other than weights (and than shifts when count == 0), or batch groups K pn >
 * INT_MAX lines: LITHO_E_ARG; every check is made before any launch.  count == 0: grad is zeroed when accumulate == 0 and left alone
 * otherwise.  Asynchronous, no allocation, no host wait. */
size_t litho_pupil_vjp_work_bytes(int groups, int K, int batch, int pn);
int litho_pupil_vjp(const void *pupils, const void *maskFT, const float *gradI, int groups, int K, const int32_t *shifts,
                    const float *weights, int64_t count, int pn, int N, void *grad, int accumulate, int batch, void *work,
                    size_t work_bytes, void *stream);
/* litho_pupil_project: out[j] = sum_{p < planes} sum_cells 2 pi Im(grad[p] . conj(pupils[p])) . basis[j], j < J: the coefficient
 * gradient.  grad, pupils complex64 [planes,pn,pn], basis fp32 [J,pn,pn], out fp32 [J], overwritten; 1 <= J <=
 * LITHO_PUPIL_PROJECT_MAX_TERMS, pn a power of two, 16..4096, planes >= 1 (else, or for a null pointer, LITHO_E_ARG).  Two stages
 * with one fixed order and no atomics: per workgroup and term a partial (threads over their cells in ascending order, a wave's
 * lanes in the xor butterfly of its shuffles, the waves in order), then per term the partials in a fixed order; the number of
 * workgroups depends on the sizes alone, so two calls give the same bits.  grad and pupils are read once per tile of 16 terms,
 * not once per term.  work: litho_pupil_project_work_bytes(planes, J, pn) device bytes (the partials; 0 for a bad argument), less
 * is LITHO_E_WORKSPACE.  Asynchronous, no allocation, no host wait. */
#define LITHO_PUPIL_PROJECT_MAX_TERMS 1024
size_t litho_pupil_project_work_bytes(int planes, int J, int pn);
int litho_pupil_project(const void *grad, const void *pupils, int planes, const float *basis, int J, int pn, float *out, void *work,
                        size_t work_bytes, void *stream);

/* ---- Layout rasteriser: the device side of the GDSII import (lithographysimulator_amd/layout.py).  SURVEY.md section
 * 8(f) row 4: the reference has NO counterpart (README.md:20-22 lists GDSII import among its unbuilt goals), it is the
 * caller side of Mask(geometry, pixelSize) (mask.py:5-30), so there is no parity target; checked bit for bit against
 * oracle/layout_oracle.py.  edges: fp64 [n_edges][4] = (x0, y0, x1, y1) of closed, counter-clockwise polygons, same
 * length unit as x0 / y0 / pixel.  geometry int16 [pn][pn]: pixel (r, c) = 1 when its centre
 * (x0 + (c + 0.5) pixel, y0 + (r + 0.5) pixel) has a non-zero winding number (half-open: a centre on a left / bottom
 * edge is inside, on a right / top edge outside), else 0.  work: litho_rasterize_work_bytes(pn) device bytes. */
size_t litho_rasterize_work_bytes(int pn);
int litho_rasterize_edges(const double *edges, int64_t n_edges, int pn, double x0, double y0, double pixel, void *work,
                          size_t work_bytes, int16_t *geometry, void *stream);

/* ---- Area coverage (anti-aliased raster): the same inside rule on s x s sub-centres per pixel, s in {1, 2, 4, 8, 16}.  Sub-grid
 * pitch q = pixel / (double)s (one fp64 division on the host); sub-centre (R, C) lies at (x0 + (C + 0.5) q, y0 + (R + 0.5) q),
 * R, C in [0, pn s), and is inside exactly when litho_rasterize_edges at (pn s, q) with the same x0, y0 sets pixel (R, C).
 * coverage fp32 [pn][pn] = (inside sub-centres of the pixel) / s^2, exact.  So coverage * s^2 equals the s x s block sums of that
 * binary raster bit for bit: overlapping polygons union, the order in which the integer atomics land cannot show.
 * The [pn s][pn s + 1] sub-grid work array (1 GiB at 2048^2, s = 8) is not required: the call works through BANDS of whole pixel
 * rows, as many as work_bytes holds (at most pn; litho_rasterize_coverage_work_bytes(pn, s, band_rows) = band_rows * s *
 * (pn s + 1) * 4 bytes, 0 for a bad argument), and the result does not depend on the band height.  Less than one pixel row of
 * workspace: LITHO_E_WORKSPACE.  s outside the set, pn < 1, pn * s > 32768, a null pointer, pixel <= 0 or a NaN origin:
 * LITHO_E_ARG, before any launch.  Non-finite and horizontal edges are skipped.  Asynchronous: three kernels per band, no
 * allocation, no host wait. */
size_t litho_rasterize_coverage_work_bytes(int pn, int s, int band_rows);
int litho_rasterize_coverage(const double *edges, int64_t n_edges, int pn, double x0, double y0, double pixel, int s, void *work,
                             size_t work_bytes, float *coverage, void *stream);

/* ---- The same coverage for all windows of a tiled layout in one call (tiling.py: rasterizeLayoutTiles).  coverage[t], t < tiles,
 * equals bit for bit what litho_rasterize_coverage writes for the edge list edges[tile_edges[i]], tile_offsets[t] <= i <
 * tile_offsets[t + 1], at origin (windows[t][0], windows[t][1]) with the same pixel and s: one inside rule, one q = pixel /
 * (double)s, one text for the sub-centre positions, the candidate-row test and the crossing abscissa.
 * A tile's list must hold WHOLE closed polygons: an edge to the right of the window adds winding to every sub-column of its
 * rows, and only the polygon's other edges cancel it.  So the caller culls per POLYGON (a polygon whose bounding box misses the
 * window may be left out), never per edge.
 * All arrays live on the device and are not inspected by the host; the kernel guards itself: an edge number outside
 * [0, n_edges) is skipped, offsets are clamped to [0, n_index] (a descending pair is an empty list), non-finite and horizontal
 * edges are skipped, a tile with a non-finite origin is written as zeros; nothing in them can make it read or write out of range.
 * s outside {1, 2, 4, 8, 16}, pn < 1, pn * s > 32768, tiles < 1, n_edges or n_index < 0, n_edges >= 2^31, pixel <= 0 or not
 * finite, or a null pointer (edges may be null when n_edges is 0, tile_edges when n_index is 0): LITHO_E_ARG, before any launch.
 * No workspace: one workgroup per (tile, pixel row) keeps the winding deltas of one sub-row, pn * s int32, in LDS (at most
 * 128 KiB of the 160 KiB a gfx950 workgroup may declare), adds the edges with LDS integer atomics -- the order cannot show --
 * and scans; no global delta array, no clear pass, no global atomics.  Asynchronous, no allocation, no host wait; ONE launch
 * whatever `tiles` is, up to 65535 tiles, and one more per further 65535. */
int litho_rasterize_coverage_tiles(const double *edges, int64_t n_edges,          /* device fp64 [n_edges][4], layout units  */
                                   const int64_t *tile_offsets,                   /* device [tiles + 1], ascending, into ... */
                                   const int32_t *tile_edges, int64_t n_index,    /* device [n_index] edge numbers           */
                                   const double *windows,                         /* device fp64 [tiles][2] = (x0, y0)       */
                                   int tiles, int pn, double pixel, int s,
                                   float *coverage /* [tiles][pn][pn] */, void *stream);

/* ---- Mask spectrum pre-step: Mask._ffFraunhofer (mask.py:74-90).  geometry int16
 * [pn,pn]; spectrum complex64 [pn,pn].  Uses the same workspace as the Abbe calls. */
int litho_mask_spectrum(const int16_t *geometry, int pn, double epsilon, int N, void *spectrum,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---- The same pre-step for a complex field transmission (phase-shift and grey masks).  The reference has no counterpart;
 * this is the definition: transmission complex64 [pn,pn] (a binary mask is the special case of values 0 and 1); the
 * spectrum is the chain of mask.py:74-90 applied to a complex image -- bilinear resize by epsilon of the real and of the
 * imaginary part, each in fp32 with torch's coordinate rule, pad or crop to N, centred forward DFT, centre pn x pn.  Every
 * step is linear: spectrum = S(Re t) + i S(Im t) with S = litho_mask_spectrum's chain; a transmission of zeros and ones
 * gives litho_mask_spectrum's result bit for bit.  One x-pass and one y-pass.  Same workspace, error codes and argument
 * checks as litho_mask_spectrum, made before anything touches a device: a null pointer, an odd pn or epsilon <= 0 ->
 * LITHO_E_ARG, N < pn -> LITHO_E_NSMALL.  Values are not inspected: a NaN in the transmission propagates into the
 * spectrum.  Asynchronous, no allocation, no host wait; safe inside a captured graph. */
int litho_mask_spectrum_complex(const void *transmission /* complex64 [pn,pn] */, int pn, double epsilon, int N,
                                void *spectrum, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Introspection for bench.py / tests: what the last litho_abbe_accumulate on this
 * thread planned.  fields: [0]=mode (0 pruned box, 1 general/wrapping), [1]=box row0,
 * [2]=box col0, [3]=box rows, [4]=box cols, [5]=points per batch, [6]=x-pass launches,
 * [7]=kernel variant (-1 generic, else log2(N/pn) of the pruned specialisation), [8]=planes in flight per
 * launch pair (through-focus stacks), [9]=y-pass groups per plane, [10]=source points per x-pass workgroup,
 * [11]=x-pass kernel family (1 plane-fused k_xpass_abbe, 2 k_xpass_split, 3 k_xpass_rect, 0 fall-backs),
 * [12]=1 when the coarse-grid path ran (pn-point transforms on the grid q = 2 v, fine image reconstructed once
 * per plane), [13]=1 when the y-pass ran a wave-level kernel (k_ypass_rect / k_ypass_wave / k_ypass_pair), [14]=1 when
 * the pupil's support box lies inside the natural support |k| <= pn/4, [15]=1 when the call planned from a caller-held
 * record (litho_abbe_accumulate_planned), 2 when the source list was split into a non-wrapping and a wrapping part (the other
 * fields then describe the part that ran last, the wrapping one if there is one; [6] counts both). */
int litho_abbe_last_plan(int64_t fields_host[16]);

/* Names of the x-pass and y-pass kernels the last litho_abbe_accumulate on this thread launched in its source-point
 * loop, spelt as rocprofv3 prints them without "void litho::" and the argument list (e.g. "k_ypass_rect<11, 8, true>").
 * Each buffer holds `capacity` bytes (96 is enough); empty strings before the first call. */
int litho_abbe_last_kernels(char *xpass_host, char *ypass_host, size_t capacity);

/* ---- Per-kernel timing for bench.py: when on, litho_abbe_accumulate brackets every x-pass
 * and y-pass launch with HIP events recorded on `stream` (the first 4096 launch pairs of a call)
 * and waits for the last one before returning.  fields: [0]=x-pass total ms, [1]=x-pass
 * batches (one batch = the x-pass launches of one launch pair), [2]=T items (source point x plane) they
 * covered, [3..5]=the same for the y-pass, [6]=1 when the y-pass ran the wave-per-line kernel
 * (k_ypass_wave) instead of k_ypass_acc, [7]=planes in flight per launch pair. */
int litho_abbe_set_profiling(int on);
int litho_abbe_last_profile(double fields_host[8]);

#ifdef __cplusplus
}
#endif
#endif /* LITHO_ABBE_H */
