/*
 * hmm_flagger_hip.h — C ABI of the MI355X (gfx950) E-step of HMM-Flagger.
 *
 * This is the drop-in boundary.  The reference has no FFI; the seam is the C
 * function pair a maintainer would re-point at this library (citations relative to
 * mobinasri/flagger, programs/submodules/hmm/):
 *
 *   void EM_runOneIterationForList(stList *emList, HMM *model, int threads);  hmm.h:109, hmm.c:739
 *   void EM_runForwardForList   (stList *emList, HMM *model, int threads);  hmm.h:113, hmm.c:790
 *   double *EM_getPosterior(EM *em, int pos);                               hmm.h:101, hmm.c:671
 *   int     EM_getMostProbableState(EM *em, int pos);                       hmm.h:103, hmm.c:687
 *
 * Plain pointers and sizes only.  Window arrays are uploaded once (hf_create); per iteration
 * only the parameter block goes up and the sufficient statistics + labels come back.
 * All functions return 0 on success or a negative HF_E_* code; where the reference calls
 * exit(EXIT_FAILURE) (hmm.c:412-415, 521-524; hmm_utils.c:782-786) the code says which check
 * fired and the caller maps it to the reference's message and exit status.
 */
#ifndef HMM_FLAGGER_HIP_H
#define HMM_FLAGGER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HF_NSTATES 4      /* Err, Dup, Hap, Col — hmm_flagger.c:173 */
#define HF_MAXCOMP 16     /* per-state mixture components (reference clamps K to 2..10) */
#define HF_MAXREGIONS 64  /* 6 region bits — ptBlock.c:294-304 */

enum { HF_MODEL_TRUNC_EXP_GAUSSIAN = 0, HF_MODEL_GAUSSIAN = 1, HF_MODEL_NEGATIVE_BINOMIAL = 2 };   /* hmm_utils.h:43-48 */
#define HF_NB_MAX_COVERAGE 250   /* MAX_COVERAGE_VALUE, hmm_utils.h:15: count data has bins 0..249, tables 0..250 */
enum { HF_MODE_FULL = 0,          /* EM_runOneIterationForList */
       HF_MODE_FORWARD_ONLY = 1   /* EM_runForwardForList */ };
enum { HF_ALGO_SCAN = 0,          /* in-chunk parallel prefix scan (default) */
       HF_ALGO_SEQ = 1            /* one wavefront per chunk, reference operation order */ };

enum {
    HF_OK = 0,
    HF_E_ARG = -1,        /* bad argument */
    HF_E_HIP = -2,        /* HIP runtime error (hf_last_error() has the text) */
    HF_E_SCALE = -3,      /* "scale (= ...) is very low!"      hmm.c:412-415, 521-524 */
    HF_E_NAN = -4,        /* "[Error] prob is NAN"             hmm_utils.c:782-786 */
    HF_E_REGION = -5,     /* a window's region index >= n_regions */
    HF_E_NOGPU = -6,      /* no HIP device: there is no CPU fallback */
    HF_E_RETRY = -7       /* hf_finish_exchange / hf_finish_gathered / hf_check only: the context changed its launch mode (a hand-off
                           * inside the one-launch segment kernel timed out) and the pass has to be run again: hf_estep, exchange,
                           * finish — with an exchange every rank gets this code together.  hf_finish and hf_em_iterate re-run the
                           * pass themselves. */
};

typedef struct hf_ctx hf_ctx;

/* The windowed coverage track, in the reference's packed-record fields (chunk.c:669-697):
 * one entry per window, chunks delimited by chunk_off; all arrays in HOST memory.  A chunk may hold no window.  Windows may lie in
 * front of the first chunk and behind the last one (0 <= chunk_off[0], chunk_off[n_chunks] <= n_windows, else HF_E_ARG): values exist
 * only for windows inside a chunk — the labels of hf_get_labels, hf_get_viterbi_labels and hf_get_sample_labels are -1 outside, and
 * every getter that takes a window range or jobs returns HF_E_ARG for one that touches a window outside every chunk. */
typedef struct hf_windows {
    int64_t n_windows;
    int32_t n_chunks;
    const int64_t *chunk_off;        /* [n_chunks+1] first window of each chunk */
    const uint16_t *cov;             /* CoverageInfo.coverage            ptBlock.h:79-92 */
    const uint16_t *mapq;            /* CoverageInfo.coverage_high_mapq */
    const uint16_t *clip;            /* CoverageInfo.coverage_high_clip */
    const uint64_t *annot;           /* annotation_flag, region index in bits 58..63 */
    const int32_t *chunk_s;          /* [n_chunks] Chunk.s (0-based)     chunk.h:16-23 */
    const int32_t *chunk_e;          /* [n_chunks] Chunk.e (0-based, inclusive) */
    const int32_t *chunk_ctg_len;    /* [n_chunks] Chunk.ctgLen */
    int32_t window_len;              /* Chunk.windowLen */
    int32_t mean_read_len;           /* header averageAlignmentLength    hmm_flagger.c:312 */
    int32_t adjust_contig_ends;      /* !--disableAdjustContigEnds       hmm_flagger.c:624 */
    double min_read_frac;            /* --minReadFractionAtEnds          hmm.c:305 */
    double max_high_mapq_ratio;      /* TransitionRequirements           hmm_utils.c:1950-1958 */
    double min_high_mapq_ratio;
    double min_highly_clipped_ratio;
} hf_windows;

/* One iteration's model (HMM struct, hmm.h:14-25), HOST memory, read during hf_estep only. */
typedef struct hf_params {
    int32_t model_type;              /* HF_MODEL_* */
    int32_t n_regions;
    int32_t ncomp[HF_NSTATES];       /* components per state */
    double alpha[4][4];              /* alpha[preState][state]           hmm.c:388 */
    const double *trans;             /* [n_regions][5][5] row 4 = Start, col 4 = End */
    const double *lambda;            /* [n_regions] Err trunc-exp rate   hmm_utils.h:393-397 */
    const double *trunc_point;       /* [n_regions] */
    const double *mean;              /* [n_regions][4][HF_MAXCOMP] */
    const double *var;               /* [n_regions][4][HF_MAXCOMP] */
    const double *weight;            /* [n_regions][4][HF_MAXCOMP] */
    /* HF_MODEL_NEGATIVE_BINOMIAL only (NULL otherwise); mean = theta, var = lambda of the NegativeBinomial struct.
     * Every quantity of that model depends on the coverage x alone (no alpha, no beta), so the caller tabulates it
     * with its own libm, K = the max_comps given to hf_create, NX = HF_NB_MAX_COVERAGE + 1:
     *   nb_E[r][s][x]        emission value, NegativeBinomial_getProb                      hmm_utils.c:480-485
     *   nb_P[r][s][c][x]     component probabilities (weights and 1e-40 floor applied)     hmm_utils.c:497-520
     *   nb_dig[r][s][c][x]   NegativeBinomial.digammaTable                                 hmm_utils.c:394-408
     *   nb_r, nb_beta[r][s][c]   r = -lambda/log(theta), beta = -theta/(1-theta) - 1/log(theta)   :458-461, 547 */
    const double *nb_E, *nb_P, *nb_dig, *nb_r, *nb_beta;
    /* <= 0: the nb_* tables are filled for every x; else the largest x for which they are (hfm_set_max_coverage): hf_estep
     * refuses a context whose windows exceed it.  The tables cost ~70 ns per (component, x) on the host every iteration. */
    int32_t nb_max_x;
} hf_params;

/* Layout of one statistics vector (doubles):
 *   [0]                                   log-likelihood (sum of log scale, hmm.c:428)
 *   per region r, base = 1 + r*hf_region_stride(K):
 *     base + ((s*3 + p)*2 + 0)*K + c      numeratorPerComp[c]   of state s, parameter p
 *     base + ((s*3 + p)*2 + 1)*K + c      denominatorPerComp[c]
 *         p = 0 mean (or trunc-exp lambda for Err), 1 var, 2 weight   hmm_utils.h:50-54,64-68
 *     base + 24*K + pre*4 + s             TransitionCountData.countMatrix[pre][s]
 * with K = max_comps given to hf_create. */
static inline int64_t hf_region_stride(int max_comps) { return 24 * (int64_t) max_comps + 16; }
static inline int64_t hf_stats_len(int n_regions, int max_comps) {
    return 1 + (int64_t) n_regions * hf_region_stride(max_comps);
}

const char *hf_version(void);
const char *hf_last_error(void);
int hf_device_count(void);
/* Optional: bring up the HIP runtime and the context of `device` ahead of hf_create (≈ 0.1 s), e.g. on another thread
 * while the input is being read.  Returns HF_E_NOGPU without a device. */
int hf_warmup(int device);

/* Upload the windows to `device` and build the device-resident window store. */
int hf_create(const hf_windows *w, int n_regions, int max_comps, int device, int algo, hf_ctx **out);
void hf_destroy(hf_ctx *ctx);

/* Launch one E-step pass over every chunk of this context on `stream` (a hipStream_t, NULL =
 * default stream); asynchronous.  Leaves one statistics vector PER CHUNK on the device.
 * Streams (DESIGN.md "Streams", tests/test_streams_gpu.py): `stream` may be any stream of the caller's on the context's device, a
 * non-blocking one included; everything the pass reads and writes is ordered on it.  The stream of the LAST hf_estep is the stream
 * every getter of the context runs on; it must outlive the context (hf_destroy first, then hipStreamDestroy). */
int hf_estep(hf_ctx *ctx, const hf_params *p, int mode, void *stream);

int32_t hf_n_chunks(const hf_ctx *ctx);
int64_t hf_n_windows(const hf_ctx *ctx);
int64_t hf_chunk_stats_len(const hf_ctx *ctx);        /* = hf_stats_len(n_regions, max_comps) */
double *hf_chunk_stats_dev(hf_ctx *ctx);              /* device [n_chunks][hf_chunk_stats_len] */
int8_t *hf_labels_dev(hf_ctx *ctx);                   /* device [n_windows] */
/* device-to-device copy of the per-chunk vectors into a caller-owned device buffer (e.g. the
 * send buffer of the multi-GPU all-gather); asynchronous on `stream`. */
int hf_copy_chunk_stats(hf_ctx *ctx, double *dst_dev, void *stream);

/* Sum `n_chunks` per-chunk vectors (the reference's reduction over the chunk list, hmm.c:759-763) into one
 * vector, in a fixed order that depends only on the position of a chunk in the list; src/dst are DEVICE
 * pointers; asynchronous on `stream`. */
int hf_reduce_chunks(hf_ctx *ctx, const double *chunk_stats_dev, int64_t n_chunks, double *out_dev, void *stream);
/* Same, with the vector of list position c taken from row row_index_dev[c] of `rows_dev` (multi-GPU: the
 * all-gathered buffer holds every rank's rows padded to a common count); identical result to the packed form. */
int hf_reduce_chunks_indexed(hf_ctx *ctx, const double *rows_dev, const int32_t *row_index_dev, int64_t n_chunks,
                             double *out_dev, void *stream);

/* Multi-GPU counterpart of hf_finish: `rows_dev` holds the per-chunk vectors of ALL ranks (all-gathered; row_index_dev[c]
 * = row of list position c, or NULL when packed), summed in the fixed order into `stats_host`; waits for the stream
 * and translates the device error flags of this rank's pass.  Every rank gets identical bits. */
int hf_finish_gathered(hf_ctx *ctx, const double *rows_dev, const int32_t *row_index_dev, int64_t n_chunks,
                       double *stats_host, void *stream);

/* The same with the error flags of EVERY rank: the gathered buffer holds `rows_per_rank` rows per rank and row
 * `flag_row` of each rank carries that rank's device flag word (hf_write_flag_row); the words are OR-ed into the result,
 * so all ranks return the same HF_E_* code and none is left waiting in the next collective (hmm.c:412-415 exits the whole
 * process; here the whole job stops).  rows_per_rank >= 2, 0 <= flag_row < rows_per_rank. */
int hf_finish_exchange(hf_ctx *ctx, const double *rows_dev, const int32_t *row_index_dev, int64_t n_rows, int n_ranks,
                       int rows_per_rank, int flag_row, double *stats_host, void *stream);
/* Let the pass write its per-chunk vectors straight into caller-owned device memory (>= n_chunks rows), e.g. this rank's
 * slot of an in-place all-gather buffer: no device-to-device copy per pass.  NULL: back to a buffer of the context. */
int hf_bind_chunk_stats(hf_ctx *ctx, double *rows_dev);
/* The same for the `ranks` exchange: a full pass in HF_STATS_ROWS mode (Gaussian / trunc-exp models) writes its total (V
 * doubles) straight to `total_dev` and its error-flag word to element 0 of `flag_row_dev`; hf_rank_total(total_dev) and
 * hf_write_flag_row(flag_row_dev) after such a pass then launch nothing.  Passes that do not produce a total of their own
 * (forward-only, negative_binomial, per-chunk statistics) are unaffected.  NULL, NULL: unbind. */
int hf_bind_rank_total(hf_ctx *ctx, double *total_dev, double *flag_row_dev);
/* This context's device error-flag word as element 0 of `row_dev` (device memory, one row of the exchange buffer);
 * asynchronous on `stream`, after the pass. */
int hf_write_flag_row(hf_ctx *ctx, double *row_dev, void *stream);

/* Single-GPU convenience: reduce this context's chunks, copy the vector to `stats_host`,
 * wait for the stream and translate the device error flags (HF_E_SCALE / HF_E_NAN / ...).  Blocks the host until `stream` (the
 * stream of the hf_estep it completes) has drained.  A pass whose flags report an error leaves nothing to get: every getter of the
 * pass's results returns HF_E_ARG until the next HF_MODE_FULL pass (hf_check likewise). */
/* (hf_finish waits for a value that hipStreamWriteValue32 writes behind the pass, or synchronises the stream: hf_estep.hip wait_total.) */
int hf_finish(hf_ctx *ctx, double *stats_host, void *stream);
/* Only wait + error flags (multi-GPU callers reduce the gathered vectors themselves).  HF_E_RETRY: a hand-off of the one-launch
 * segment kernel timed out; the context has switched to two launches and the caller repeats the pass from hf_estep.  Blocks the
 * host until `stream` has drained, as hf_finish does. */
int hf_check(hf_ctx *ctx, void *stream);

/* How a HF_MODE_FULL pass of HF_ALGO_SCAN produces the statistics:
 *   HF_STATS_CHUNKS  one estimator vector per chunk (EM_runOneIterationForList's per-chunk EM objects, hmm.c:739-763),
 *                    reduced over the chunk list in list order: hf_chunk_stats_dev / hf_copy_chunk_stats /
 *                    hf_reduce_chunks* / hf_finish_gathered work on these vectors, and the result does not depend on how
 *                    the chunk list is sharded over GPUs (bit for bit).
 *   HF_STATS_ROWS    the pair counts are summed per emission row first and the estimator updates run once per row
 *                    (flagger_amd/csrc/hf_rows.h); hf_finish returns the same vector up to the rounding of a different
 *                    summation order (fixed by the plan of hf_create: reproducible), ~2.5x less statistics time.  The
 *                    per-chunk vectors are NOT produced (only element 0, the chunk's log-likelihood).
 * Default: HF_STATS_ROWS where it applies — HF_ALGO_SCAN and a plan that is not
 * dominated by padding (it is when nearly every window has a private emission row: reads longer than the contigs) —
 * else HF_STATS_CHUNKS is used silently (hf_get_stats_mode tells); environment HF_STATS=chunks|rows
 * overrides the default at hf_create. */
enum { HF_STATS_CHUNKS = 0, HF_STATS_ROWS = 1 };
int hf_set_stats_mode(hf_ctx *ctx, int mode);
/* The statistics vector of THIS context's chunks after a pass, in either mode, into device memory (hf_chunk_stats_len
 * doubles): what ranks exchange when the per-chunk vectors are not needed — all-gather one vector per rank, then
 * hf_finish_gathered(rows = the gathered vectors, row_index = NULL, n = world size) sums them in rank order.  Asynchronous on
 * `stream`, after the pass. */
int hf_rank_total(hf_ctx *ctx, double *out_dev, void *stream);
int hf_get_stats_mode(const hf_ctx *ctx);          /* the mode the NEXT full pass will use */
/* Launches of the segment forward-backward in the NEXT pass: 1 = k_seg_fb alone (its segments hand their products over inside the
 * launch), 2 = k_seg_prod + k_seg_fb (hf_create's choice for a chunk with more segments than the device holds workgroups,
 * environment HF_SEG_LAUNCHES=2, or after a hand-off timed out), 0 = the context does not run the segment kernels (HF_ALGO_SEQ, empty). */
int hf_seg_launches(const hf_ctx *ctx);
/* Row blocks (of at most 8 = windows per lane) that a segment workgroup of the NEXT one-launch pass keeps in LDS across its three walks
 * instead of fetching them again: hf_create's choice — all 8 when every segment is still resident together with that much LDS each (up to
 * ~430 segments on 256 CUs: a 1/8 shard of BASELINE configs[2]), 0 otherwise (environment HF_SEG_CACHED_STEPS forces any number). */
int hf_seg_cached_steps(const hf_ctx *ctx);
/* Sub-passes of a full pass: a context whose pair records (64 bytes per window) would not fit the 256 MB Infinity Cache — more than ~2.8 M
 * windows on one GPU — cuts its chunk list into sub-passes of whole chunks (<= ~1.6 M windows each) and runs the segment kernel and the
 * per-group sums sub-pass by sub-pass through one record buffer; 1 for BASELINE configs[2] (environment HF_SUBPASSES forces a number).
 * hf_sub_pass_windows: the windows of sub-pass k (what ONE launch of the segment kernel processes: hf_set_profiling times the first). */
int hf_sub_passes(const hf_ctx *ctx);
int64_t hf_sub_pass_windows(const hf_ctx *ctx, int k);
/* Where hf_create's wall time went (what EM_construct + EM_renewParametersAndEstimatorsFromModel cost the reference per chunk and
 * iteration, hmm.c:253-298, paid once here): up to `max` phases in call order, ms[i] and a static name each; returns the number of
 * phases recorded.  The last entry is the total. */
int hf_create_phases(const hf_ctx *ctx, int max, double *ms, const char **names);

/* Results of the last HF_MODE_FULL pass (HF_E_ARG when the last pass was HF_MODE_FORWARD_ONLY: f and scales would be new,
 * b and the labels stale; HF_E_ARG also once hf_finish / hf_check — hf_finish_gathered / hf_finish_exchange, hf_batch_finish for the
 * model's status — have reported an error of the pass (HF_E_NAN, HF_E_SCALE, ...): its labels and vectors are what the NaN or the
 * underflow left; the same holds for every getter below that answers "under the model of the last HF_MODE_FULL pass" and for
 * hf_batch_get_labels / hf_batch_get_posterior of a model whose status was an error).  hf_get_posterior / hf_get_forward_backward: an EM pass of the default algorithm keeps no per-window scale (and,
 * in several sub-passes, only the last sub-pass's records) — the first call after a pass runs the segment kernel once more over the pass's
 * tables, with the scale array (~0.05 ms per 1.5 M windows; the array itself is allocated by that first call); same values as the pass.
 * No stream argument: the three run on the stream of the last hf_estep, behind the pass, and block the host until their result is
 * there — whatever else the caller has enqueued on that stream first is waited for too. */
int hf_get_labels(hf_ctx *ctx, int8_t *labels_host);                                   /* hmm.c:730-736 */
int hf_get_posterior(hf_ctx *ctx, int64_t first, int64_t n, double *post_host);        /* [n][4] hmm.c:671-685 */
int hf_get_forward_backward(hf_ctx *ctx, int64_t first, int64_t n, double *f_host, double *b_host,
                            double *scales_host);                                      /* EM.f/.b/.scales */
/* Exact interval probabilities (flagger_amd/csrc/hf_interval.h), under the model of the last HF_MODE_FULL pass like hf_get_posterior.
 * Job i is the window range first[i]..last[i] (global indices, inclusive, 0 <= first <= last < n_windows; it may span chunks) and the
 * state set S = state_mask[i] (bit s = state s: 0 Err, 1 Dup, 2 Hap, 3 Col; 1..15):
 *   log_p[i] = log P(s_t in S for every t in first..last | data)
 * Chunks are independent chains: the value is the sum, in chunk order, over the job's chunk-local parts [a, b] of log(N_S / N),
 *   N_S = sum_{p in S} sum_{q in S} f_a[p] M_S[p][q] b_b[q],   M_S = prod_{t=a+1..b} (A_t D_S) (the identity when a == b),
 *   D_S = diag(1_S), N = the same with all four states; f, b the pass's scaled forward and backward vectors (hf_get_forward_backward),
 *   A_t the row the pass multiplied by at window t.
 * -inf when no path of the interval stays in S; mask 15 gives exactly 0.0.  P(some window of the range in state k) is
 * -expm1(log_p) of the job with mask 15 & ~(1 << k).  A job's value depends only on (first, last, mask) and the pass, bitwise: not on
 * the other jobs of the call, their order or their number.  Synchronous on the pass's stream; the first call after an EM pass of the
 * default algorithm re-runs the segment kernel once, as hf_get_posterior's does.  Buffers of its own: nothing an EM pass, hf_viterbi
 * or hf_sample_paths reads is written.  HF_E_ARG: no full pass yet or the last pass forward-only, n < 0, a NULL array with n > 0, a
 * bad range, a mask of 0 or above 15. */
int hf_get_interval_log_probs(hf_ctx *ctx, int64_t n, const int64_t *first, const int64_t *last,
                              const uint8_t *state_mask, double *log_p_host);
/* Exact mean and variance of label totals (flagger_amd/csrc/hf_moments.h), under the model of the last HF_MODE_FULL pass like hf_get_posterior.
 * Job i is the window range first[i]..last[i] and the state set S = state_mask[i] as for hf_get_interval_log_probs, a region filter
 * region[i] (-1: every window, else only the windows whose annotation region index equals it; region == NULL: -1 for every job) and the
 * unit of the call: HF_COUNT_WINDOWS gives window t the weight w_t = 1, HF_COUNT_BASES its length in bases (window k of a chunk:
 * min(chunk_s + (k+1) window_len - 1, chunk_e) - (chunk_s + k window_len) + 1); w_t = 0 where the filter rejects the window.  With
 * N = sum_{t in range} w_t 1[s_t in S]:
 *   mean[i] = E[N | data] = sum_t w_t gamma_t(S),  gamma_t(S) = sum_{s in S} posterior_t[s] (hf_get_posterior's values; a fixed summation
 *             order, not a by-product of the variance)
 *   var[i]  = Var[N | data], exactly (all pairwise covariances of the chain), from the second-order jet of the chain's product with the
 *             weights centred by gamma_t; never negative, never NaN (a negative rounding residue is 0.0)
 * Chunks are independent chains: both values are the sums, in chunk order, of the values of the job's chunk-local parts.  Mask 15 gives
 * var exactly 0.0 and mean exactly the sum of the job's weights; a job whose filter leaves no window gives (0.0, 0.0).  A job's two values
 * depend only on (first, last, mask, region, unit) and the pass, bitwise: not on the other jobs of the call, their order or their number.
 * Synchronous on the pass's stream; the first call after an EM pass of the default algorithm re-runs the segment kernel once, as
 * hf_get_posterior's does.  Buffers of its own: nothing an EM pass, hf_viterbi, hf_sample_paths, hf_get_interval_log_probs or
 * hf_get_alpha_stats reads is written.  n = 0 is a successful no-op.  HF_E_ARG: the cases of hf_get_interval_log_probs, a region outside
 * -1..n_regions-1, an unknown unit.  hf_batch_* and hf_multi_* have no counterpart. */
enum { HF_COUNT_WINDOWS = 0, HF_COUNT_BASES = 1 };
int hf_get_count_moments(hf_ctx *ctx, int64_t n, const int64_t *first, const int64_t *last, const uint8_t *state_mask,
                         const int32_t *region /* NULL: all -1 */, int unit, double *mean_host, double *var_host);
/* Exact mean and variance of block counts (flagger_amd/csrc/hf_runs.h), under the model of the last HF_MODE_FULL pass like hf_get_posterior.
 * Job i is the window range first[i]..last[i] and the state set S = state_mask[i] as for hf_get_interval_log_probs.  For a chunk-local
 * part [a, b] of the job:
 *   R  = 1[s_a in S] + sum_{t=a+1..b} 1[s_{t-1} not in S, s_t in S]    (the runs of S that start inside the part)
 *   S0 = 1[s_a in S],  E0 = 1[s_b in S]
 * joined (NULL: all 0; joined[0] must be 0): joined[c] != 0 says that chunk c continues chunk c-1 on the same contig, so that a run of S
 * over the last window of c-1 and the first window of c is ONE run.  With the job's parts 1..m in chunk order, part j+1 is joined to
 * part j when it lies in the next chunk and that chunk has joined != 0; a chunk without windows has no part, so it ends a run of
 * joined chunks whatever its and its successor's entries say.  The job's count is
 *   B = sum_j R_j - sum_{joined j} E0_j S0_{j+1}
 * and, chunks being independent chains, with e_j = E[E0_j], s_j = E[S0_j], q_j = e_j s_{j+1}:
 *   mean[i] = sum_j E[R_j] - sum_{joined j} q_j
 *   var[i]  = sum_j Var(R_j) + sum_{joined j} [ q_j (1 - q_j) - 2 (s_{j+1} Cov(R_j, E0_j) + e_j Cov(R_{j+1}, S0_{j+1})) ]
 *             + 2 sum_{j, j+1 both joined} e_j s_{j+2} Cov(S0_{j+1}, E0_{j+1})
 * each sum in chunk order; never negative, never NaN (a negative rounding residue is 0.0).  The per-part values are exact: E[R] =
 * gamma_a(S) + the sum of the pair posteriors P(s_{t-1} not in S, s_t in S | data) in a fixed order, the variance and the covariances from
 * the second-order jet of the chain's product with the pair tilt 1[p not in S] 1[s in S] centred by that pair posterior.  Mask 15 gives
 * var exactly 0.0 and mean exactly the number of maximal joined groups of the job's parts.  A job's two values depend only on (first,
 * last, mask, joined) and the pass, bitwise: not on the other jobs of the call, their order or their number; without a join they are the
 * left-to-right sums of the parts' values.  Synchronous on the pass's stream; the first call after an EM pass of the default algorithm
 * re-runs the segment kernel once, as hf_get_posterior's does.  Buffers of its own: nothing an EM pass or another getter reads is
 * written.  n = 0 is a successful no-op.  HF_E_ARG: the cases of hf_get_interval_log_probs, joined[0] != 0.  hf_batch_* and hf_multi_*
 * have no counterpart. */
int hf_get_run_moments(hf_ctx *ctx, int64_t n, const int64_t *first, const int64_t *last, const uint8_t *state_mask,
                       const uint8_t *joined /* [n_chunks], NULL: none */, double *mean_host, double *var_host);
/* Exact path entropy and labelling log-probability (flagger_amd/csrc/hf_entropy.h), under the model of the last HF_MODE_FULL pass like
 * hf_get_posterior.  f, b are that pass's scaled forward and backward vectors (hf_get_forward_backward), A_t the row the pass multiplied
 * by at window t.  Given the data, the label path of a chunk is an inhomogeneous Markov chain whose transition at window t is the pair
 * posterior over its row marginal.  For a window t that is not the first of its chunk:
 *   x_t[p][s] = f_{t-1}[p] * A_t[p][s] * b_t[s]   (multiplied in that order)
 *   m_t[p]    = sum_s x_t[p][s]                   (summed in state order)
 *   Z_t       = sum_p m_t[p]
 *   cond_t    = - sum_p sum_s (x_t[p][s] / Z_t) log(x_t[p][s] / m_t[p])      (an entry with x = 0 contributes 0)
 * x <= m_p holds in floating point too (m_p is a sum of non-negatives that contains x): every term is >= 0, and neither a clamp nor a
 * difference of large numbers appears.  For any window:
 *   gamma_t[s] = f_t[s] b_t[s] / sum_s f_t[s] b_t[s]      (hf_get_posterior's value, the sum in state order)
 *   marg_t     = - sum_s gamma_t[s] log gamma_t[s]        (a zero contributes 0)
 * and cond_t := marg_t at the first window of a chunk.  Job i is the window range first[i]..last[i] (global indices, inclusive, 0 <= first
 * <= last < n_windows; it may span chunks).  Chunks are independent chains: a job's value is the sum, in chunk order, of the values of its
 * chunk-local parts [a, b]:
 *   entropy(part)     = marg_a + sum_{t=a+1..b} cond_t: the Shannon entropy of the joint posterior of (s_a..s_b), in nats (the chain
 *                       rule H(s_a..s_b) = H(s_a) + sum_t H(s_t | s_{t-1}) of a Markov chain; exp of it is the effective number of
 *                       plausible labellings of the range)
 *   log_prob(part; y) = log gamma_a[y_a] + sum_{t=a+1..b} log(x_t[y_{t-1}][y_t] / m_t[y_{t-1}]) = log P(s_a..s_b = y_a..y_b | data);
 *                       -inf as soon as one factor is 0 (a zero m makes that factor 0)
 *   hf_get_path_entropy     entropy_host[i] >= 0, never NaN
 *   hf_get_path_log_probs   log_p_host[i] <= 0 or -inf, never NaN, for the labelling labels_host[t] (0..3) of the windows of the job;
 *                           labels_host has n_windows entries, of which only those inside some job's range are read
 *   hf_get_entropy_profile  marg_host[i] = marg_t and cond_host[i] = cond_t for t = first + i, i < n (either array may be NULL): 0 <=
 *                           cond_t <= marg_t up to rounding, since conditioning cannot raise entropy; the sum of marg_t over a range is
 *                           what the per-window posteriors alone give, and it is never below the path entropy beyond rounding
 * A job's value depends only on (first, last), the labels inside the range and the pass, bitwise: not on the other jobs of the call, their
 * order or their number; a chunk-spanning job is bitwise the left-to-right sum of its parts asked as separate jobs.  Synchronous on the
 * pass's stream; the first call after an EM pass of the default algorithm re-runs the segment kernel once, as hf_get_posterior's does,
 * also in several sub-passes.  HF_ALGO_SCAN and HF_ALGO_SEQ, all three model types (nothing here depends on the emission).  Buffers of
 * their own: nothing an EM pass or another getter reads is written.  n = 0 is a successful no-op.  HF_E_ARG: the cases of
 * hf_get_interval_log_probs (no full pass yet or the last pass forward-only, n < 0, a NULL array with n > 0, a bad range), a label
 * outside 0..3 inside some job's range (labels outside every range are not looked at), the profile call with both output arrays NULL.
 * hf_batch_* and hf_multi_* have no counterpart. */
int hf_get_path_entropy(hf_ctx *ctx, int64_t n, const int64_t *first, const int64_t *last, double *entropy_host);
int hf_get_path_log_probs(hf_ctx *ctx, int64_t n, const int64_t *first, const int64_t *last,
                          const int8_t *labels_host /* [n_windows], read only inside the jobs' ranges */, double *log_p_host);
int hf_get_entropy_profile(hf_ctx *ctx, int64_t first, int64_t n, double *marg_host /* or NULL */, double *cond_host /* or NULL */);
/* Exact breakpoint posteriors (flagger_amd/csrc/hf_breakpoint.h), under the model of the last HF_MODE_FULL pass like
 * hf_get_interval_log_probs: given that a range switches once from a state set U to a state set V, the posterior over the switching
 * window (the change-point-location posterior of a constrained HMM).  f, b are that pass's scaled forward and backward vectors
 * (hf_get_forward_backward), A_t the row the pass multiplied by at window t.  Job i is the window range a = first[i] < b = last[i], both
 * in the SAME chunk, a left set U = left_mask[i] and a right set V = right_mask[i], each 1..15 (bit s = state s), U & V == 0.  For
 * k = a+1 .. b the event E_k is "s_t in U for a <= t < k and s_t in V for k <= t <= b": the events are disjoint and k is the first window
 * of the right side.  With D_S = diag(1_S):
 *   L_a = f_a o 1_U,  L_t = L_{t-1} (A_t D_U)       (row vectors, t = a+1 .. b-1)
 *   r_b = b_b,        r_{t-1} = (A_t D_V) r_t       (column vectors, t = b .. a+1)
 *   w_k = L_{k-1} . r_{k-1}                         (sum in state order)
 *   N   = f_a (A_{a+1} ... A_b) b_b                 (the unmasked chain, the same operations as the masked one: hf_get_interval_log_probs' N)
 *   P(E_k | data) = w_k / N,  W = sum_k w_k,  p_k = w_k / W
 * Every vector and matrix is renormalised by a power of two after every product, with integer exponent sums, and a weight is carried as
 * (mantissa in [1, 2), exponent) until the job's largest exponent emax is known: nothing underflows before that.  THE ORDER of the sums:
 * x_k = mantissa_k 2^(e_k - emax) is summed in blocks of 64 consecutive k (block m holds k = a+1+64m .. a+64m+64); inside a block by
 * an inclusive scan whose step off = 1, 2, 4 .. 32 adds, at place l >= off, the running value of place l - off on the left of the running
 * value of place l; the sum of the blocks before is added on the left of that, and becomes the value at the block's last place.  W is
 * the value at the last block's last place, p_k = x_k / W, and c_k is the same blocked scan over the p_k.  A job returns
 *   log_p_event  log W - log N = log P(exactly one switch U -> V inside [a, b] | data): <= 0 up to rounding, -inf when no k has weight
 *   quantile[j]  for probs[j] (0 < probs[j] < 1, n_probs in 0..8; quantile_host is [n][n_probs]): the smallest k with p_k > 0 and
 *                c_k >= probs[j]; if rounding leaves none, the largest k with p_k > 0
 *   mode, mode_p the smallest k of maximal p_k, and that p_k
 * and quantile = mode = -1, mode_p = 0.0 for a job without weight.  No NaN, except that a pass that left no weight (N not > 0) gives NaN
 * in log_p_event only, as hf_get_interval_log_probs does.  hf_get_breakpoint_profile returns p_k, k = first+1 .. last, of one job (zeros
 * for a job without weight) and its log_p_event: bitwise the values the batch call derives its quantiles and mode from.  A job's
 * outputs depend only on (first, last, U, V, probs) and the pass, bitwise: not on the other jobs of the call, their order, their number
 * or the device batch they fall in (HF_BP_BATCH_PIECES).  Synchronous on the pass's stream; the first call after an EM pass of the default
 * algorithm re-runs the segment kernel once, as hf_get_posterior's does, also in several sub-passes.  HF_ALGO_SCAN and HF_ALGO_SEQ, all
 * three model types.  Buffers of their own: nothing an EM pass or another getter reads is written.  n = 0 is a successful no-op.
 * HF_E_ARG: the cases of hf_get_interval_log_probs (no full pass yet or the last pass forward-only, n < 0, a NULL array with n > 0, a bad
 * range, a mask of 0 or above 15), first == last, first and last in different chunks, overlapping masks, n_probs outside 0..8, a
 * probability outside (0, 1), a NULL probs or quantile_host with n_probs > 0.  hf_batch_* and hf_multi_* have no counterpart. */
int hf_get_breakpoints(hf_ctx *ctx, int64_t n, const int64_t *first, const int64_t *last, const uint8_t *left_mask,
                       const uint8_t *right_mask, int n_probs, const double *probs, double *log_p_event_host /* [n] */,
                       int64_t *quantile_host /* [n][n_probs] */, int64_t *mode_host /* [n] */, double *mode_p_host /* [n] */);
int hf_get_breakpoint_profile(hf_ctx *ctx, int64_t first, int64_t last, uint8_t left_mask, uint8_t right_mask,
                              double *p_host /* [last - first], k = first+1 .. last */, double *log_p_event_host);
/* Exact long-run probabilities (flagger_amd/csrc/hf_longrun.h), under the model of the last HF_MODE_FULL pass like hf_get_posterior: how
 * probable is it that a range holds a block of a label set that is long enough to be reported.  f, b are that pass's scaled forward and
 * backward vectors (hf_get_forward_backward), A_t the row the pass multiplied by at window t.  Job i is the window range
 * first[i]..last[i] (global, inclusive, it may span chunks), a state set S = state_mask[i] (1..15), a length L = min_len[i] >= 1 in
 * windows, and the optional joined[n_chunks] of hf_get_run_moments with the same meaning and the same joined[0] == 0 rule.  The job's
 * parts are its chunk-local ranges [a, b]; part j+1 is joined to part j under the rule hf_get_run_moments states; a GROUP is a maximal
 * sequence of parts joined to each other, its label sequence the concatenation of its parts' windows.  HIT: the group's sequence contains
 * at least L consecutive windows whose state is in S (runs are clipped at the job's ends; the windows of a run may change state inside
 * S).  Chunks are independent chains given the data: the path distribution of a group is the product of its chunks' posterior path
 * distributions.
 *   log_p_none[i] = sum over the job's groups, in chunk order, of log P(no HIT in the group | data)
 *   log_p_some[i] = log(1 - exp(log_p_none[i]))        (log P(some group has a HIT))
 * The expanded chain of a group: one lane per state outside S, lanes (s, d) for s in S, d = 1..L-1 ("the current run of S has d
 * windows"), four absorbing HIT lanes, one per state; a step from (s, L-1), or with L == 1 from anything, into a state of S goes to that
 * state's HIT lane.
 *   lanes(S, L) = (4 - |S|) + |S| (L - 1) + 4 <= HF_LONGRUN_MAX_LANES
 * Window a of the first part starts the lanes with f_a[s]; a window inside a chunk multiplies by A_t; the step from the last window b of
 * a part to the first window a' of the next joined part multiplies by the rank-one row b_b[p] * f_a'[s] (the previous chunk's posterior
 * collapse times the next chunk's start: the counter runs on across the boundary); the last window of the group takes the dot product
 * with b_b.  N_none is the sum over the non-HIT lanes, N_hit over the HIT lanes, P(no HIT) = N_none / (N_none + N_hit).
 * THE ORDER of the operations.  Linear domain, value = x 2^E with separate integer exponent sums E_n (non-HIT lanes) and E_h (HIT lanes);
 * the inflow into HIT is multiplied by 2^(E_n - E_h).  Every sum of a step runs over the source states p = 0..3 in order; the non-HIT
 * total T[p] of a state of S is a sum over the wavefront in one fixed order (hf_longrun.h lr_wave_sum).  After every 8th step counted
 * from the group's first window, each class is scaled by a power of two that brings the largest of its per-state totals, taken before
 * that step, to exponent 300 (HIT lanes that were all zero take the non-HIT exponent, non-HIT lanes that are all zero the HIT exponent; otherwise E_n - E_h is
 * kept <= 600): a group's bits depend on
 * the job alone, and neither log N_none nor log N_hit underflows at any range length.  With d = (log N_hit - log N_none) + (E_h - E_n) ln 2,
 * per group:
 *   d < 0:   log P(no HIT) = -log1p(exp(d)),       log P(HIT) = d - log1p(exp(d))
 *   d >= 0:  log P(no HIT) = -d - log1p(exp(-d)),  log P(HIT) = -log1p(exp(-d))
 * so a tiny P(HIT) gives an accurate log P(HIT) and a log P(no HIT) that is -P(HIT) to rounding, and a tiny P(no HIT) stays finite down
 * to the range hf_get_interval_log_probs reaches.  A job: log_p_none is the left-to-right sum of its groups' values from 0.0;
 * log_p_some is -inf when no group has a HIT of positive weight, that group's log P(HIT) when exactly one has, else
 * log(-expm1(log_p_none)) above -ln 2 and log1p(-exp(log_p_none)) below.
 * Exact cases: N_hit == 0 gives log_p_none = 0.0 and log_p_some = -inf, so a group of fewer than L windows does; mask 15 with L <= the
 * group's length gives (-inf, 0.0); with L == 1 the job is "some window in S" and log_p_none equals hf_get_interval_log_probs of mask
 * 15 & ~S to rounding (mask 15: -inf).  No NaN, except where the pass itself left no weight (as hf_get_interval_log_probs).  A job's two
 * values depend only on (first, last, mask, L, joined) and the pass, bitwise: not on the other jobs of the call, their order, their
 * number or the device batch they fall in (HF_LR_BATCH_PARTS, HF_LR_BATCH_PIECES); without joins log_p_none is bitwise the left-to-right
 * sum of the parts asked as separate jobs.  Synchronous on the pass's stream; the first call after an EM pass of the default algorithm
 * re-runs the segment kernel once, as hf_get_posterior's does, also in several sub-passes.  HF_ALGO_SCAN and HF_ALGO_SEQ, all three model
 * types.  Buffers of its own: nothing an EM pass or another getter reads is written.  n = 0 is a successful no-op.  Either output array
 * may be NULL, not both.  HF_E_ARG: the cases of hf_get_interval_log_probs, min_len < 1, lanes(S, L) above the cap, joined[0] != 0, both
 * outputs NULL with n > 0; any bad job refuses the whole call.  hf_batch_* and hf_multi_* have no counterpart. */
#define HF_LONGRUN_MAX_LANES 64
int hf_get_long_run_log_probs(hf_ctx *ctx, int64_t n, const int64_t *first, const int64_t *last, const uint8_t *state_mask,
                              const int32_t *min_len, const uint8_t *joined /* [n_chunks], NULL: none */,
                              double *log_p_none_host, double *log_p_some_host /* either may be NULL, not both */);
/* The exact block-length spectrum (flagger_amd/csrc/hf_runlen.hip), under the model of the last HF_MODE_FULL pass like hf_get_posterior:
 * how many blocks of a label set of every length the posterior expects.  Job i is the window range first[i]..last[i] (global,
 * inclusive, it may span chunks) and a state set S = state_mask[i] (1..15); max_len = L, 1..HF_RUN_LENGTHS_MAX, is one for the call;
 * joined[n_chunks] is that of hf_get_run_moments with the same meaning and the same joined[0] == 0 rule.  Parts, joins and groups are
 * those of hf_get_long_run_log_probs.  A RUN is a maximal stretch of consecutive windows of a group's concatenated sequence whose state
 * is in S; it is clipped at the job's ends and the state may change inside S.
 *   spectrum[i][l-1] = E[number of runs of exactly l windows | data], l = 1..L
 *   spectrum[i][L]   = E[number of runs of more than L windows | data]
 * each summed over the job's groups in chunk order.  Chunks are independent chains given the data.
 * PER PART [a, b] (chunk-local), with f, b the pass's scaled vectors and A_t its rows; only ratios are formed, so no scale is needed:
 *   Q_u[p][q]  = A_u[p][q] b_u[q] / sum_q' A_u[p][q'] b_u[q'], a < u <= b   (the posterior chain; q' = 0..3 in order; a denominator of
 *                                                                           0 gives a zero row: no mass can reach it)
 *   sigma_a[s] = gamma_a(s);  sigma_t[s] = sum_{p not in S} f_{t-1}[p] A_t[p][s] b_t[s] / sum_{p,s} f_{t-1}[p] A_t[p][s] b_t[s], t > a
 * for s in S, zero outside (the pair posterior of a run start, summed over p in order, never formed as gamma - xi).  The run started at
 * t walks from v_1 = sigma_t; at age d it stands at window u = t + d - 1.  At u = b it is OPEN at b: sum v_d goes to Rc[d], or to W if
 * t = a.  Otherwise w = v_d Q_{u+1}; sum_{q not in S} w[q] closes a run of exactly d windows, into I[d] for t > a or Lc[d] for t = a
 * (left-touching), and v_{d+1} = w o 1_S.  A run still in S at age L + 1 adds sum v_{L+1} to bin "> L" of I or Lc and is dropped: it is
 * counted once, where it saturates.  A part yields I[1..L+1], Lc[1..L+1], Rc[1..L], W, s = gamma_a(S), e = gamma_b(S) and its length T.
 * A GROUP is stitched on the host left to right (flagger_amd/csrc/hf_runlen_stitch.h), from o[1..L] = 0, O = 0, N = 0, for every part:
 *   N += I;  N[l'] += o[l'] (1 - s);  for l = 1..L+1: N[l] += (1 - O) Lc[l] and N[min(l' + l, L + 1)] += o[l'] Lc[l], l' = 1..L;
 *   T <= L: the new o gets (1 - O) W at T and o[l'] W at l' + T (N[L + 1] where l' + T > L);  the new o[d] += Rc[d];  O = e
 * and N[l'] += o[l'] after the last part.
 * Exact cases: a job's values depend only on (first, last, mask, L, joined) and the pass, bitwise: not on the other jobs of the call,
 * their order, their number or the device batch (HF_RL_BATCH_PARTS, HF_RL_BATCH_PIECES); joined all zero is NULL; without a join a job
 * is bitwise the left-to-right sum of its parts asked as separate jobs; bin "> L" is exactly 0.0 when no group of the job has more than
 * L windows; every bin is >= 0 and never NaN, also on emission-floor stretches and where S has posterior 0 (every bin 0.0 then).
 * Synchronous on the pass's stream; the first call after an EM pass of the default algorithm re-runs the segment kernel once, as
 * hf_get_posterior's does, also in several sub-passes.  HF_ALGO_SCAN and HF_ALGO_SEQ, all three model types.  Buffers of its own:
 * nothing an EM pass or another getter reads is written.  n = 0 is a successful no-op.  HF_E_ARG: the cases of
 * hf_get_interval_log_probs, max_len outside 1..HF_RUN_LENGTHS_MAX, joined[0] != 0, a NULL output with n > 0; any bad job refuses the
 * whole call.  hf_batch_* and hf_multi_* have no counterpart. */
#define HF_RUN_LENGTHS_MAX 64
int hf_get_run_lengths(hf_ctx *ctx, int64_t n, const int64_t *first, const int64_t *last, const uint8_t *state_mask,
                       int32_t max_len /* L, 1..HF_RUN_LENGTHS_MAX, one for the call */,
                       const uint8_t *joined /* [n_chunks], NULL: none */, double *spectrum_host /* [n][L + 1] */);
/* The exact distribution of label totals (flagger_amd/csrc/hf_countdist.hip), under the model of the last HF_MODE_FULL pass like
 * hf_get_posterior: how probable it is that exactly k windows of a range carry a label of a set.  Job i is the window range
 * first[i]..last[i] (global, inclusive, it may span chunks; refusals and parts are those of hf_get_interval_log_probs) and a state set
 * S = state_mask[i] (1..15); max_count = K, 1..HF_COUNT_DIST_MAX, is one for the call.  N = sum_t 1[s_t in S] over the job's windows:
 *   dist[i][k]     = P(N = k | data), k = 0..K
 *   dist[i][K + 1] = P(N > K | data)
 * K + 2 <= 64 bins.  The unit is windows; there is no region filter and no `joined` argument: a total does not depend on how chunks
 * are joined.  (hf_get_count_moments gives the mean and variance of the same N without a bound on it.)
 * PER PART [a, b] (chunk-local), with f, b the pass's scaled vectors and A_t its rows; only ratios are formed, so no scale is needed:
 *   Q_u[p][q]  = A_u[p][q] b_u[q] / sum_q' A_u[p][q'] b_u[q'], a < u <= b   (hf_get_run_lengths' posterior chain; q' = 0..3 in order; a
 *                                                                           denominator of 0 gives a zero row: no mass can reach it)
 *   gamma_a[s] = f_a[s] b_a[s] / sum_s' f_a[s'] b_a[s']                     (s' in order; all 0.0 where the pass left no weight)
 * The walk carries v[s][k], k = 0..K and K + 1 for "more than K": v_a[s][1_S[s]] = gamma_a[s], every other entry 0.  Per window
 * u = a+1..b: w[q][k] = ((v[0][k] Q_u[0][q] + v[1][k] Q_u[1][q]) + v[2][k] Q_u[2][q]) + v[3][k] Q_u[3][q]; for q not in S v[q][k] = w[q][k];
 * for q in S v[q][k] = w[q][k-1] for 1 <= k <= K, v[q][0] = 0 and v[q][K+1] = w[q][K+1] + w[q][K].  The part's distribution is
 * ((v_b[0][k] + v_b[1][k]) + v_b[2][k]) + v_b[3][k].  Every bin is a sum of non-negative terms; "> K" is carried, never formed as 1 - sum.
 * ON THE DEVICE the walk runs piece by piece of the getters' 512-window grid: a piece yields its transfer M[p][q][k] (the walk above
 * from the unit vector "state p in front of the piece, no window counted", k = 0..K+1), and the part takes its pieces in order,
 *   k <= K:  c[p][q] = sum_{j=0..k} v[p][j] M[p][q][k-j]                            (one accumulator from 0.0, j ascending)
 *   "> K":   c[p][q] = sum_{j=0..K+1} v[p][j] r_j,  r_j = sum_{m=K+1-j..K+1} M[p][q][m]
 * where r_j is ONE running tail sum that takes M[p][q][K+1-j] at step j: it adds M downwards from the "> K" bin, r_0 = 0.0 + M[p][q][K+1],
 * and the outer sum is one accumulator from 0.0, j ascending (index K + 1 of v is its own "> K" bin, which meets the whole of M); then
 * v[q] = ((c[0][q] + c[1][q]) + c[2][q]) + c[3][q].  A part with a = b has no piece and is gamma_a alone.
 * A JOB is the truncated convolution of its parts' distributions in chunk order, on the host (flagger_amd/csrc/hf_countdist_stitch.h): the
 * first part as it is, every further part d folded in by the same two sums (acc for v[p], d for M[p][q]).  Chunks are independent
 * chains given the data.
 * Exact cases: a job's values depend only on (first, last, mask, K) and the pass, bitwise: not on the other jobs of the call, their
 * order, their number or the device batch (HF_CD_BATCH_PARTS, HF_CD_BATCH_PIECES); a job over several chunks is bitwise the host stitch
 * of its parts asked as separate jobs; for a job of T windows the bins k > T are exactly 0.0, so bin "> K" is exactly 0.0 when T <= K;
 * with mask 15 every bin but T (bin "> K" when T > K) is exactly 0.0; every bin is >= 0 and never NaN, also on emission-floor stretches
 * and where S has posterior 0 (bin 0 carries the mass then).
 * Synchronous on the pass's stream; the first call after an EM pass of the default algorithm re-runs the segment kernel once, as
 * hf_get_posterior's does, also in several sub-passes.  HF_ALGO_SCAN and HF_ALGO_SEQ, all three model types.  Buffers of its own:
 * nothing an EM pass, a decoder or another getter reads is written.  n = 0 is a successful no-op.  HF_E_ARG: the cases of
 * hf_get_interval_log_probs, max_count outside 1..HF_COUNT_DIST_MAX, a NULL output with n > 0; any bad job refuses the whole call.
 * hf_batch_* and hf_multi_* have no counterpart. */
#define HF_COUNT_DIST_MAX 62
int hf_get_count_distribution(hf_ctx *ctx, int64_t n, const int64_t *first, const int64_t *last, const uint8_t *state_mask,
                              int32_t max_count /* K, 1..HF_COUNT_DIST_MAX, one for the call */, double *dist_host /* [n][K + 2] */);
/* The alpha statistics (flagger_amd/csrc/hf_alpha.h): what an EM needs to fit the matrix alpha[pre][s] itself.  Models gaussian and
 * trunc_exp_gaussian.  For a pair of windows (t-1, t) of one chunk, t >= 1, with r the region of window t, x and x_prev the coverage of t
 * and t-1 as the pass sees them (8 bits), beta = beta_t:
 *   xi_t[p][s] = f_{t-1}[p] * A_t[p][s] * b_t[s] / 1e-4      (f, b: hf_get_forward_backward; A_t: the row the pass multiplied by)
 * and for a Gaussian state s (every state but Err under trunc_exp_gaussian), component c, a = alpha[p][s]:
 *   v_c = var_c beta,  d_c = x - ((1 - a) mu_c + a x_prev) beta,  u_c = beta (x_prev - mu_c),
 *   P_c = w_c / sqrt(2 PI v_c) exp(-d_c^2 / (2 v_c)), floored at 1e-40 as the emission does; g_c = P_c / sum_c P_c; phi_c = 0 if floored, else 1
 *   G[r][p][s] = sum_t xi_t[p][s] sum_c g_c phi_c d_c u_c / v_c        H[r][p][s] = sum_t xi_t[p][s] sum_c g_c phi_c u_c^2 / v_c  (>= 0)
 * over ALL pairs of every chunk whose window t lies in region r — the pair (0, 1) too, which the estimators of the statistics vector
 * skip.  A chunk of one window contributes nothing; Err under trunc_exp_gaussian has G = H = 0.
 * Summed over the regions, G is the exact derivative of the pass's log-likelihood (element 0 of the statistics vector) in alpha[p][s],
 * PROVIDED the End column of `trans` is the same for all four states: then sum_ps xi_t = 1 and xi_t is the pair posterior.  The host model
 * keeps it so (hf_model.cpp sets trans[r][s][End] = 1e-4 at creation and after every M-step, SQUAREM's prime model too).  alpha + G / H is
 * the maximiser of the expected complete-data log-likelihood in that entry with everything else fixed (hfm_estimate_alpha).
 *   hf_set_alpha_stats(ctx, 1)  full passes from now on may be asked for G and H.  The pass itself does not change — same launches, and
 *                       everything it returns is bit-identical to the switch off; the statistics are computed by the first
 *                       hf_get_alpha_stats after the pass (later calls on the same pass return the same bits).  HF_E_ARG on a context
 *                       that has run negative_binomial passes (that emission has no alpha).
 *   hf_alpha_stats_len  32 * n_regions
 *   hf_get_alpha_stats  out[r][0][p][s] = G, out[r][1][p][s] = H.  Synchronous on the pass's stream.  HF_ALGO_SCAN, in HF_STATS_ROWS and
 *                       HF_STATS_CHUNKS alike: the component terms are evaluated once per row of A of the pass, the pair counts xi come
 *                       per window from the pair records of all windows — so the first call after an EM pass of the default algorithm
 *                       re-runs the segment kernel once, as hf_get_posterior's does, also in several sub-passes — and the pair (0, 1)
 *                       of a chunk is a pair like any other.  HF_ALGO_SEQ: terms and counts per window from the pass's f, b and
 *                       emission rows (the on-device cross-check).  The first call of a context also builds the plan of the pairs
 *                       (sorted by region; one download of the window records and positions, one upload of 12 bytes per window).
 *                       The order of all additions is fixed by that plan: reproducible bit for bit.  HF_E_ARG: no full pass with the
 *                       switch on yet, the last pass forward-only or negative_binomial.
 * hf_batch_* and hf_multi_* do not produce them. */
int hf_set_alpha_stats(hf_ctx *ctx, int on);
int64_t hf_alpha_stats_len(const hf_ctx *ctx);
int hf_get_alpha_stats(hf_ctx *ctx, double *out_host);
/* Most-probable-path (Viterbi) decoding of every chunk (flagger_amd/csrc/hf_viterbi.h): with the parameters `p`, for a chunk of T windows
 *   s* = argmax over s_0..s_{T-1} of first[s_0] * prod_{t>=1} A_t[s_{t-1}][s_t] * end[s_{T-1}],
 *   first[s] = trans[r_0][4][s] * e_0[s],  A_t = the row a pass builds (transition x emission),  end[s] = trans[r_{T-1}][s][4];
 * ties go to the lowest state index (at every backpointer and at the final state).  The chunk's score is log of that maximum, the
 * run's score the sum over chunks in list order.  HF_E_SCALE when no path of a chunk has weight, HF_E_NAN on a NaN.
 * Decoding uses buffers of its own: the last pass's results (hf_get_labels / _posterior / _forward_backward) and the next hf_estep
 * are unaffected.  hf_viterbi is asynchronous on `stream`; hf_viterbi_finish waits, translates the error flags and returns the run's
 * score.  The getters answer for the last FINISHED run (HF_E_ARG before any).
 * `stream` need not be the stream of the last pass (a second stream of the caller's decodes while the first is busy); hf_viterbi_finish
 * takes the stream hf_viterbi ran on.  The getters have no stream argument: they copy a finished run's results, synchronously. */
int hf_viterbi(hf_ctx *ctx, const hf_params *p, void *stream);
int hf_viterbi_finish(hf_ctx *ctx, double *log_prob_host, void *stream);
int hf_get_viterbi_labels(hf_ctx *ctx, int8_t *labels_host);                          /* [n_windows], layout of hf_labels_dev */
int hf_get_viterbi_chunk_log_probs(hf_ctx *ctx, double *out_host);                    /* [n_chunks] */

/* Minimum-run-length Viterbi (flagger_amd/csrc/hf_minlen.h): the most probable path AMONG THE PATHS WHOSE RUNS MEET A MINIMUM LENGTH, the
 * exact form of minimum-duration decoding.  first[s], A_t[pre][s], end[s] and the weight of a path are exactly those of hf_viterbi.
 * min_len[4] holds windows per state (0 Err, 1 Dup, 2 Hap, 3 Col), 1 <= min_len[s] and sum_s min_len[s] <= HF_MINLEN_MAX_LANES.
 * A path of a chunk of T windows is ADMISSIBLE when every maximal run of equal state s has at least min_len[s] windows; a run that
 * contains the chunk's first or last window is exempt (a chunk is a cut of a contig, and the final BED merges runs across the chunks of
 * a contig), so a constant path is always admissible.  The decoder returns
 *   s* = argmax over admissible paths of first[s_0] * prod_{t>=1} A_t[s_{t-1}][s_t] * end[s_{T-1}].
 * It runs the expanded chain with lanes (s, d), d = 1..min_len[s]: "in state s, the current run has d windows so far", at
 * d = min_len[s] "at least that many" (the saturated lane):
 *   window 0:   delta[(s, min_len[s])] = first[s], every other lane has no weight (the exempt left end);
 *   lane (s,1): the maximum over predecessors p in increasing order of delta[(p, min_len[p])] * A_t[p][s], with p != s when
 *               min_len[s] > 1 (with min_len[s] == 1, p = s is the "stay", at its place); replacement needs strict >, so the lowest p
 *               wins a tie;
 *   lane (s,d), 1 < d < min_len[s]: delta[(s, d-1)] * A_t[s][s];
 *   lane (s,d), d = min_len[s] > 1: delta[(s, d-1)] * A_t[s][s], then delta[(s, d)] * A_t[s][s], strict >;
 *   end:        the maximum over all lanes, in order of s and then of d ascending, of delta[(s,d)] * end[s], strict > (the exempt
 *               right end).
 * With all four lengths 1 this is hf_viterbi's recurrence and tie rule.  The chain is carried IN LOGS (log of every row entry, -inf for
 * 0; a product above is a sum), so nothing underflows at any chunk length and a step is one add and one compare.
 * The chunk's score is the log of the maximum, the run's score the sum over chunks in list order; a chunk without windows scores 0;
 * windows outside every chunk get label -1.  HF_E_SCALE when no admissible path of a chunk has weight, HF_E_NAN on a NaN in a row or in
 * the end column.  HF_E_ARG: a NULL argument, a length below 1, a sum above HF_MINLEN_MAX_LANES, a getter before any finished run.
 * Streams: as hf_viterbi (any stream of the caller's; hf_viterbi_minlen_finish takes the same one).  Buffers of its own: the last pass's
 * results, hf_viterbi's results, the sampler's results and the next hf_estep are bitwise unaffected.  One code path serves HF_ALGO_SCAN
 * and HF_ALGO_SEQ contexts and all three model types: the outputs are bitwise the same on both kinds of context and across repeated
 * calls.  hf_batch_* and hf_multi_* have no counterpart. */
#define HF_MINLEN_MAX_LANES 64
int hf_viterbi_minlen(hf_ctx *ctx, const hf_params *p, const int32_t min_len[4], void *stream);   /* asynchronous, as hf_viterbi */
int hf_viterbi_minlen_finish(hf_ctx *ctx, double *log_prob_host, void *stream);
int hf_get_viterbi_minlen_labels(hf_ctx *ctx, int8_t *labels_host);                   /* [n_windows] */
int hf_get_viterbi_minlen_chunk_log_probs(hf_ctx *ctx, double *out_host);             /* [n_chunks] */

/* Minimum-run-length Viterbi over whole contigs (flagger_amd/csrc/hf_minlen.h): hf_viterbi_minlen with the rule applied to GROUPS
 * of joined chunks instead of chunks.  joined follows the rule hf_get_run_moments states: NULL means all 0; joined[0] must be 0;
 * joined[c] != 0 says that chunk c continues chunk c-1; a chunk without windows has no part, so it ends a group whatever its own entry
 * and its successor's entry say.  A GROUP is a maximal sequence of chunks joined to each other; chunk offsets are one array, so a group
 * is one contiguous window range, and its path is the concatenation of its chunks' paths.  Chunks are independent chains: the weight of
 * a group's path is the product of its chunks' weights, first * prod_t A_t * end per chunk, exactly as in hf_viterbi.
 * A group's path is ADMISSIBLE when every maximal run of equal state s IN THE GROUP'S LABEL SEQUENCE has at least min_len[s] windows;
 * only a run that contains the group's first or last window is exempt.  The decoder returns the admissible group path of the largest
 * weight.  The expanded chain, its lanes, the entry, in-between and saturated steps and every tie rule are those of hf_viterbi_minlen,
 * carried in logs, with
 *   window 0 and the end: the group's first window and the end at the group's last window take the place of the chunk's;
 *   the step into the first window t of a chunk c joined to c-1: an ordinary step with the row
 *               J_t[p][s] = log end_{c-1}[p] + log first_c[s],   end_{c-1}[p] = trans[r_{t-1}][p][4],
 *               formed first as one double (-inf when either term is -inf), then used like any log A_t[p][s].  The run counter runs on
 *               across the boundary: staying in s goes from (s, d) to (s, min(d+1, min_len[s])), a change of state needs the saturated
 *               lane of p and enters (s, 1), and p == s is excluded when min_len[s] > 1 as everywhere.
 * Restated: the joined decoder on (chunk list, joined) is hf_viterbi_minlen on the chunk list whose chunks are the groups, with the row
 * of every joined chunk-first window replaced by J_t and end taken from the group's last chunk.
 * Scores: a group's score is the log of its maximum, the run's score the sum over groups in list order.
 * hf_get_viterbi_minlen_chunk_log_probs returns the group's score in the entry of the group's first chunk and exactly 0.0 in the
 * entries of its other chunks, so that its list-order sum is the run's score; a chunk without windows scores 0.0; windows outside every
 * chunk get label -1.  HF_E_SCALE when no admissible path of a group has weight; HF_E_NAN on a NaN in a row or in an end column, the end
 * columns read at joined boundaries included; HF_E_ARG: the cases of hf_viterbi_minlen, and joined[0] != 0.
 * Exact cases: joined NULL or all zero gives the labels, chunk scores and run score of hf_viterbi_minlen bit for bit; all four lengths 1
 * gives the labels of hf_viterbi whatever joined says; the joined-admissible paths are a subset of the per-chunk-admissible ones, so a
 * group's score is never above the sum of its chunks' hf_viterbi_minlen scores, to rounding.
 * The call is asynchronous as hf_viterbi_minlen is and shares that decoder's state: hf_viterbi_minlen_finish,
 * hf_get_viterbi_minlen_labels and hf_get_viterbi_minlen_chunk_log_probs answer for the last finished run of either entry point.  Its
 * buffers are that decoder's own: the last pass, hf_viterbi, both samplers, hf_minlen_posterior and the next hf_estep are bitwise
 * unaffected.  One code path serves both kinds of context and all three model types.  hf_batch_* and hf_multi_* have no counterpart. */
int hf_viterbi_minlen_joined(hf_ctx *ctx, const hf_params *p, const int32_t min_len[4],
                             const uint8_t *joined /* [n_chunks], NULL: none */, void *stream);

/* Posteriors under minimum run lengths (flagger_amd/csrc/hf_minlen_post.h): the sum-product twin of hf_viterbi_minlen.  first[s],
 * A_t[p][s], end[s], min_len[4], admissibility (runs that contain a chunk's first or last window are exempt), the lanes (s, d),
 * d = 1..min_len[s], and the lane index sum_{q<s} min_len[q] + d - 1 are exactly those of hf_viterbi_minlen; so are 1 <= min_len[s] and
 * sum_s min_len[s] <= HF_MINLEN_MAX_LANES.  Chunks are independent chains.  With m_s = min_len[s], for a chunk of T windows:
 *   F_0[(s, m_s)] = first[s], 0 elsewhere
 *   F_t[(s, 1)]   = sum over p = 0..3 in order of F_{t-1}[(p, m_p)] * A_t[p][s], p == s left out when m_s > 1
 *   F_t[(s, d)]   = F_{t-1}[(s, d-1)] * A_t[s][s]                                               1 < d < m_s
 *   F_t[(s, m_s)] = F_{t-1}[(s, m_s - 1)] * A_t[s][s] + F_{t-1}[(s, m_s)] * A_t[s][s]            m_s > 1
 *   B_{T-1}[(s, d)] = end[s]
 *   B_{t-1}[(s, d)] = A_t[s][s] * B_t[(s, d+1)]                                                 d < m_s
 *   B_{t-1}[(s, m_s)] = [m_s > 1] A_t[s][s] * B_t[(s, m_s)] + sum over q = 0..3 in order of A_t[s][q] * B_t[(q, 1)], q == s only
 *                       when m_q == 1
 *   Z_adm = sum over lanes of F_{T-1}[lane] * end[s(lane)]
 *   Z     = the same recursion with all four lengths 1 (the plain 4-state forward)
 *   g_t[s] = sum over d of F_t[(s, d)] * B_t[(s, d)]
 *   post[t][s] = g_t[s] / (g_t[0] + g_t[1] + g_t[2] + g_t[3]) = P(s_t = s | data, path admissible)
 *   log_mass[c] = log Z_adm - log Z = log P(path of chunk c admissible | data)
 * THE ORDER OF EVERY SUM.  The sums over p and over q: ((t_0 + t_1) + t_2) + t_3, a term that is left out replaced by 0; in B the stay
 * term is added to the finished sum over q from the left.  The denominator of post: ((g_0 + g_1) + g_2) + g_3.  Z_adm, Z and every
 * g_t[s] are sums over the 64 lanes of a wavefront with 0 in the lanes that take no part (for g_t[s]: the lanes of the other states),
 * as ONE FIXED TREE: v += the value of lane ^ 1; v += that of lane ^ 2; v += that of the lane mirrored within its group of 8; v += that
 * of the lane mirrored within its row of 16; then ((row 0 + row 1) + row 2) + row 3.  Z comes from the same kernel and the same
 * operations as Z_adm, with the lengths (1, 1, 1, 1).
 * RESCALING.  Linear domain, value = x * 2^E with an integer exponent sum E.  A rescaling with the largest lane mx: e = ilogb(mx) - 300
 * (0 when mx is 0 or not finite), every lane is scaled by 2^-e and E += e.  It happens at the walk's first vector (F_0, or B_{T-1}),
 * with mx its largest lane, before that vector is stored or stepped; and after every 8th step of a walk, counted from the chunk's
 * first window (F) or its last window (B), with mx the largest lane BEFORE that step.  The largest lane is thus at exponent 300 at the
 * start of every period of eight steps, the first included, and meets at most nine rows before the next rescaling: emission floors
 * of 1e-40 keep it normal at either end of a chunk as well as inside it.  THE PRODUCTS IN g_t: with F_t[lane] = mf * 2^ef and
 * B_t[lane] = mb * 2^eb (frexp: mantissas in [1/2, 1)), a lane's term is (mf * mb) * 2^(ef + eb - e_t), e_t the largest ef + eb over the
 * lanes whose mf * mb is not 0: the two walks are each anywhere within their own period at a window, and the plain product of two
 * lanes could underflow although neither factor does.  The largest term of a window is in [1/4, 1).  log Z_adm = log(the wave sum) + E ln 2, likewise log Z.  post is a ratio within
 * one window, so it needs no exponent: any power-of-two scale of F_t and B_t cancels.
 * Exact cases.  All four lengths 1: log_mass is exactly 0.0 in every chunk, and post equals hf_get_posterior of a full pass with the
 * same parameters to rounding.  A chunk of one or two windows has mass 1 (log_mass within rounding of 0).  A chunk without windows has
 * log_mass 0.0 and log Z_adm 0.0.  Windows outside every chunk get label -1, and a posterior range that touches one is HF_E_ARG.
 * HF_E_SCALE: a chunk with Z_adm or Z not > 0 (or a window whose g_t sum to nothing).  HF_E_NAN: a NaN in a row or in the end column.
 * No NaN is returned otherwise.
 * HF_E_ARG: the argument cases of hf_viterbi_minlen; a getter before a finished run; the forward lanes (n_windows x sum(min_len) x 8
 * bytes) do not fit nine tenths of the free device memory (hf_last_error names the size).
 * hf_minlen_posterior_finish returns the sum of log_mass over the chunks in list order.  hf_get_minlen_posterior_labels: the first
 * largest entry of post (replacement needs strict >).
 * Streams: as hf_viterbi_minlen.  Buffers of its own: the results of the last pass, hf_viterbi, hf_viterbi_minlen and the sampler, and
 * the next hf_estep, are bitwise unaffected.  One code path serves HF_ALGO_SCAN and HF_ALGO_SEQ contexts and all three model types:
 * the outputs are bitwise the same on both kinds of context, across repeated calls and on any stream.  hf_batch_* and hf_multi_* have
 * no counterpart. */
int hf_minlen_posterior(hf_ctx *ctx, const hf_params *p, const int32_t min_len[4], void *stream);   /* asynchronous, as hf_viterbi_minlen */
int hf_minlen_posterior_finish(hf_ctx *ctx, double *log_mass_total_host, void *stream);
int hf_get_minlen_posterior(hf_ctx *ctx, int64_t first, int64_t n, double *post_host);              /* [n][4] */
int hf_get_minlen_posterior_labels(hf_ctx *ctx, int8_t *labels_host);                 /* [n_windows], -1 outside chunks */
int hf_get_minlen_chunk_log_mass(hf_ctx *ctx, double *log_mass_host, double *log_z_adm_host);       /* [n_chunks]; log_z_adm_host may be NULL */

/* The E-step under minimum run lengths (flagger_amd/csrc/hf_minlen_em.h): the expected sufficient statistics of EM_updateEstimators
 * under the posterior over ADMISSIBLE paths, in hf_finish's layout (hf_chunk_stats_len), for the unchanged M-step (hfm_estimate).  An
 * EM over it maximises sum over chunks of log Z_adm = log P(data, path admissible | theta) instead of log P(data | theta).
 * first[s], A_t[p][s], end[s], min_len[4], the lanes (s, d), the lane index, admissibility (runs touching a chunk's first or last
 * window are exempt), the recursions of F_t and B_t, every sum order inside them and the rescaling are exactly hf_minlen_posterior's;
 * F is the bits its forward kernel stores.  For a chunk of T windows and every pair (t-1, t), 1 <= t <= T-1, m_s = min_len[s]:
 *   p != s:           u_t[p][s] = F_{t-1}[(p, m_p)] * A_t[p][s] * B_t[(s, 1)]
 *   p == s, m_s == 1: u_t[s][s] = F_{t-1}[(s, 1)] * A_t[s][s] * B_t[(s, 1)]
 *   p == s, m_s > 1:  u_t[s][s] = sum over d = 2..m_s of c_d * A_t[s][s] * B_t[(s, d)],
 *                     c_d = F_{t-1}[(s, d-1)] for d < m_s, c_{m_s} = F_{t-1}[(s, m_s - 1)] + F_{t-1}[(s, m_s)]
 *   tot_t = sum over s ascending of ((u_t[0][s] + u_t[1][s]) + u_t[2][s]) + u_t[3][s], accumulated from the left
 *   xi_adm_t[p][s] = u_t[p][s] / tot_t = P(s_{t-1} = p, s_t = s | data, path admissible)
 * THE ORDER OF EVERY PRODUCT AND SUM.  A term x * a * y (x of F_{t-1}, or c_d; a of A_t; y of B_t) is formed from the three frexp
 * mantissas (in [1/2, 1), 0 for a zero) as (mx * ma) * my, with the exponent sum e = ex + ea + ey.  e_t is the largest e over the
 * window's terms that are not 0 (the 12 or more terms u_t[p][s] of a single product and the terms of every sum over d), and a term
 * enters as (mx * ma) * my * 2^max(e - e_t, -2000): F_{t-1} and B_t each sit anywhere in their own rescaling period, so the plain
 * product could underflow although no factor does; the largest term of a window is in [1/8, 1), and the power of two cancels in
 * xi_adm.  The sum over d is the fixed tree of hf_minlen_posterior's wave sums with 0 in the lanes that take no part.  tot_t as above.
 * Identities: sum_p xi_adm_t[p][s] = post[t][s] and sum_s xi_adm_t[p][s] = post[t-1][p] of hf_minlen_posterior, to rounding; with all
 * four lengths 1, xi_adm_t is the plain pass's xi_t = f_{t-1}[p] * A_t[p][s] * b_t[s] / 1e-4, to rounding.
 * STATISTICS.  Element 0 of a chunk's vector is that chunk's log Z_adm, bit for bit what hf_get_minlen_chunk_log_mass returns as
 * log_z_adm.  Every other element is the estimator arithmetic of the per-chunk statistics of hf_estep (transition counts, the trunc-exp
 * numerator and denominator, the one-component Gaussian states, the collapsed state's component loop with the component rows of THIS
 * call's tables), term for term, over the same pairs (w-1, w), w = 2..T-1 (the reference's skipped first pair included), with
 * xi_adm_w[p][s] in the place of count / terminationProb: xi_adm is normalised already, nothing is divided by the termination
 * probability.  The chunk vectors are summed in the order of hf_reduce_chunks.  A chunk of one or two windows has no such pair: statistics
 * of exactly zero behind element 0; a chunk without windows the vector of zeros.  WITH ALL FOUR LENGTHS 1 element 0 is log Z, which
 * holds the end column end[s]; the log-likelihood of hf_estep (the sum of the log scales) leaves it out, so the two differ by the
 * chunks' log sum_s f_{T-1}[s] end[s] while every other element agrees with hf_estep + hf_finish to rounding.
 * hf_estep_minlen is asynchronous on `stream`; hf_estep_minlen_finish waits for that stream, translates the flags and copies the
 * summed vector [hf_chunk_stats_len] to stats_host and, when log_z_host is not NULL, the sum over chunks in list order of log Z (the
 * plain chain's, from the same forward kernel) to *log_z_host.  HF_E_SCALE: a chunk whose Z_adm (or Z) or a window whose tot_t is not
 * > 0.  HF_E_NAN: a NaN in a row, in the end column, in a chunk's sum or in tot_t.
 * hf_get_minlen_pair_posterior: xi_adm of windows first .. first + n - 1 of the last FINISHED call, [n][16] with entry p * 4 + s;
 * the first window of a chunk holds zeros; a range that touches a window outside every chunk is HF_E_ARG.
 * hf_get_minlen_em_chunk_stats: the per-chunk vectors [n_chunks][hf_chunk_stats_len], log Z_adm [n_chunks] and log Z [n_chunks] of the
 * last finished call; each array may be NULL.
 * HF_E_ARG: a NULL argument, a length below 1, a sum above HF_MINLEN_MAX_LANES, a getter or a finish before its call; model_type
 * negative_binomial (its statistics are another path; hf_last_error says so); the forward lanes (n_windows x sum(min_len) x 8 bytes)
 * plus xi_adm (n_windows x 128 bytes) do not fit nine tenths of the free device memory (hf_last_error names the size).
 * The call has a parameter block, tables, rows, forward lanes, xi_adm, tile and chunk statistics of its own: the context's last full
 * pass and every getter of it, hf_viterbi*, both samplers, hf_minlen_posterior and the next hf_estep are bitwise unaffected.  One code
 * path serves HF_ALGO_SCAN and HF_ALGO_SEQ contexts: the outputs are bitwise the same on both kinds of context, across repeated calls
 * and on any stream.  hf_batch_* and hf_multi_* have no counterpart; hf_estep_minlen_joined below is the whole-contig form. */
int hf_estep_minlen(hf_ctx *ctx, const hf_params *p, const int32_t min_len[4], void *stream);
int hf_estep_minlen_finish(hf_ctx *ctx, double *stats_host, double *log_z_host /* may be NULL */, void *stream);
int hf_get_minlen_pair_posterior(hf_ctx *ctx, int64_t first, int64_t n, double *xi_host);          /* [n][16], p-major */
int hf_get_minlen_em_chunk_stats(hf_ctx *ctx, double *chunk_stats_host, double *log_z_adm_host, double *log_z_host);

/* The E-step under minimum run lengths over groups of joined chunks (flagger_amd/csrc/hf_minlen_em_joined.h): hf_estep_minlen with
 * hf_viterbi_minlen_joined's rule, under which only the runs at a GROUP's ends are exempt.  An EM over it maximises the sum over
 * groups of log Z_adm(group), the mass of the set the whole-contig decoders decode in.  It is asynchronous on `stream`, finished by
 * hf_estep_minlen_finish and read by hf_get_minlen_pair_posterior and hf_get_minlen_em_chunk_stats; it shares its state with
 * hf_estep_minlen as hf_minlen_posterior_joined shares hf_minlen_posterior's: a later call of either replaces the earlier one's results.
 * joined[c] != 0 joins chunk c to chunk c - 1; a chunk continues its predecessor when it is joined to it and both have windows.
 * DEFINITION.  The joined call on (chunk list, joined) is hf_estep_minlen's definition on the GROUP-AS-CHUNK list, in which a group's
 * first chunk holds the group's whole window range and its other chunks hold none, with the row of every joined chunk-first window t
 * (first window of chunk c, joined to c - 1) replaced by
 *   J_t[p][s] = end_{c-1}[p] * first_c[s]      end_{c-1}[p] = trans[region of window t-1][p][4], first_c[s] = first[s] of chunk c
 * formed as ONE DOUBLE first and then used as A_t[p][s] wherever the definition above reads A_t; `end` is taken at the group's last
 * window.  F is the bits the forward kernel of hf_minlen_posterior_joined stores; the backward recursion, its sum orders and its
 * rescaling (at the walk's first vector and after every 8th step, counted from the group's last window) are that call's.
 * PAIR POSTERIOR.  xi_adm_t is the formula above for every t >= 1 inside a group, with A_t := J_t at a joined chunk-first window (the
 * boundary pair), and zero at a group's first window.  Identities: sum_p xi_adm_t[p][s] = post[t][s] and sum_s xi_adm_t[p][s] =
 * post[t-1][p] of hf_minlen_posterior_joined, to rounding.  With all four lengths 1, J_t has rank 1 and a group factorises into its
 * chunks: xi_adm, the statistics and the sum of log Z_adm agree with hf_estep_minlen's to rounding, and at a joined chunk-first window
 * xi_adm_t[p][s] = post[t-1][p] * post[t][s].
 * STATISTICS.  The estimator arithmetic is hf_estep_minlen's, unchanged, over the track's own pairs (w-1, w), w = 2..T_c-1 of each
 * ORIGINAL chunk c, with the joined call's xi_adm as the counts: the reference's estimators never see a boundary pair, under this rule
 * as under the other.  log Z_adm and log Z of a group sit in the entry of the group's first chunk, its other chunks hold exactly 0.0;
 * element 0 of a chunk's statistics vector follows the same rule, so element 0 of the total is the sum over groups of log Z_adm and
 * *log_z_host of the finish the sum over groups of log Z.
 * joined == NULL or all zeros: every output is bitwise hf_estep_minlen's.
 * HF_E_ARG: what hf_estep_minlen refuses (hf_last_error names hf_estep_minlen_joined), and joined[0] != 0.  What the call leaves
 * untouched, the two kinds of context, repeated calls and streams: as hf_estep_minlen. */
int hf_estep_minlen_joined(hf_ctx *ctx, const hf_params *p, const int32_t min_len[4], const uint8_t *joined /* [n_chunks] or NULL */,
                           void *stream);

/* Admissible path sampling (flagger_amd/csrc/hf_minlen_sample.h): whole paths drawn from the posterior under minimum run lengths.
 * first[s], A_t[p][s], end[s], min_len[4], admissibility (runs that contain a chunk's first or last window are exempt), the lanes (s, d)
 * and the lane index are hf_viterbi_minlen's; F_t is hf_minlen_posterior's forward vector: the same recursion, sum orders and rescaling,
 * so the same bits.  A sample of a chunk is an admissible path drawn with probability weight(path) / Z_adm, the distribution whose
 * marginals hf_get_minlen_posterior returns.  It is drawn by backward sampling over the expanded chain.
 * UNIFORMS: hf_sample_paths': key_k, then u(k, i), i the global window index t for the draw of window t and i = n_windows + c for
 * chunk c's final lane.  A sample depends on (seed, absolute sample index, window, lengths) and nothing else.
 * THE DRAW RULE over a candidate list, hf_sample_paths': weights w_0..w_{n-1}; c_0 = w_0, c_i = c_{i-1} + w_i; x = u * c_{n-1}; the
 * smallest i with x < c_i, else the largest i with w_i > 0, else 0.
 *   the final lane of chunk c   the candidates are all sum(min_len) lanes in lane order, w_l = F_{T-1}[l] * end[s(l)]; the cumulative
 *                               sums run strictly left to right (a prefix, not the tree of the wave sums)
 *   the lane at t-1 given lane (s, d) at window t >= 1 of the chunk, m_s = min_len[s]:
 *     d = 1 (the entry lane; the only lane when m_s = 1)   four slots p = 0..3, w_p = F_{t-1}[(p, m_p)] * A_t[p][s], w_s replaced by 0
 *                                                          when m_s > 1; the result is (p, m_p)
 *     1 < d < m_s                                          (s, d-1), no draw
 *     d = m_s > 1                                          two slots, w_0 = F_{t-1}[(s, m_s - 1)] * A_t[s][s] ("arrived"),
 *                                                          w_1 = F_{t-1}[(s, m_s)] * A_t[s][s] ("stayed"): (s, m_s - 1) or (s, m_s)
 * SCALING BEFORE THE PRODUCTS.  The eight F_{t-1} values a window's draws read (the four saturated lanes (p, m_p) and the four lanes
 * (p, m_p - 1) below them, where m_p > 1) are first scaled by 2^-e, e = ilogb of the largest of the eight (0 when that is 0 or not
 * finite): the stored lanes can sit near 2e-270, and a floored row would push the products into the subnormals.  The final weights'
 * lanes are scaled the same way by the largest lane of F_{T-1}.  A power of two changes no comparison.
 * Exact cases.  With all four lengths 1 this is hf_sample_paths' rule word for word.  A chunk without windows draws nothing.  Windows
 * outside every chunk get label -1.
 * HF_E_SCALE: a chunk's Z_adm is not > 0.  HF_E_NAN: a NaN in a row or in the end column.  HF_E_ARG: the length cases of
 * hf_viterbi_minlen; n_samples < 1 or above hf_minlen_sample_capacity; first_sample < 0; k out of range; a getter before a finished call.
 * hf_minlen_sample_capacity: the samples per call at these lengths (at most 65535): the rows (128 bytes per window), the forward lanes
 * (8 * sum(min_len) bytes per window) and about 3 bytes per window and sample (the words for a multiple of 64 samples) within nine
 * tenths of the free device memory, what the sampler holds already counting as free; 0, with hf_last_error, when not one sample fits.
 * Streams: as hf_viterbi_minlen (hf_sample_minlen_finish takes the stream of the call).  Buffers of its own, the forward lanes
 * included: the results of the last pass, hf_viterbi, hf_viterbi_minlen, hf_sample_paths and hf_minlen_posterior, and the next
 * hf_estep, are bitwise unaffected.  One code path serves HF_ALGO_SCAN and HF_ALGO_SEQ contexts and all three model types: the samples
 * are bitwise the same on both kinds of context, across repeated calls, on any stream and however they are grouped into calls.
 * hf_batch_* and hf_multi_* have no counterpart. */
int hf_minlen_sample_capacity(const hf_ctx *ctx, const int32_t min_len[4]);   /* samples per call; <= 0 with hf_last_error when not even one fits */
int hf_sample_paths_minlen(hf_ctx *ctx, const hf_params *p, const int32_t min_len[4],
                           int64_t first_sample, int n_samples, uint64_t seed, void *stream);   /* asynchronous */
int hf_sample_minlen_finish(hf_ctx *ctx, void *stream);
int hf_get_minlen_sample_labels(hf_ctx *ctx, int k, int8_t *labels_host);      /* sample first_sample + k, [n_windows], -1 outside chunks */

/* The posterior and the sampler over whole contigs (flagger_amd/csrc/hf_minlen_post_joined.h): hf_minlen_posterior and
 * hf_sample_paths_minlen with the rule applied to GROUPS of joined chunks.  joined and the groups are exactly those of
 * hf_viterbi_minlen_joined: NULL means all 0; joined[0] != 0 is HF_E_ARG; a chunk without windows ends a group whatever the entries
 * say; a group is one contiguous window range.
 * NORMATIVE RESTATEMENT.  The joined call on (chunk list, joined) is the per-chunk call on a modified chunk list: in that list each
 * group's first chunk holds the group's whole window range and the group's other chunks hold no windows, and the row of every joined
 * chunk-first window t (first window of chunk c, joined to c-1) is replaced by
 *               J_t[p][s] = end_{c-1}[p] * first_c[s],   end_{c-1}[p] = trans[r_{t-1}][p][4],  first_c[s] = row pre = 0 of the
 *               chunk-first row,
 * formed first as one double, then used like any A_t[p][s]; end is taken at the group's last window.  Everything else follows:
 *   recursions and sums   the F and B recursions, every sum order and the tree of the wave sums are hf_minlen_posterior's.
 *   run counter           it runs on across the boundary: staying goes (s, d) -> (s, min(d+1, m_s)); a change needs the saturated lane of
 *                         p and enters (s, 1); p == s is excluded when m_s > 1.
 *   rescaling             at a walk's first vector and after every 8th step, counted from the GROUP's first window (F) or last window
 *                         (B).  No further rescaling is made at a joined boundary: J_t is the size of any row (a transition probability
 *                         times first[s]), so a period still passes at most nine rows.
 *   the products F_t B_t  the frexp form of hf_minlen_posterior.
 *   Z                     the plain 4-state chain over the same rows of the group, from the same kernel and operations.
 *   hf_get_minlen_chunk_log_mass   the group's log_mass and log Z_adm in the entry of the group's first chunk, exactly 0.0 in the
 *                         entries of its other chunks; the list-order sum of hf_minlen_posterior_finish is then the track's.
 *   sampler               the draw rule, candidate lists, scaling of the eight F_{t-1} values, word format and uniforms are
 *                         hf_sample_paths_minlen's.  The draw of window t uses uniform index t, the joined chunk-first windows
 *                         included, which draw with A_t := J_t.  The final lane of a group uses index n_windows + c, c the group's
 *                         FIRST chunk: a group's sample depends on (seed, absolute sample index, its own windows, lengths) and not on
 *                         how other contigs are joined.  The indices n_windows + c of the group's other chunks go unused.
 *   errors                HF_E_NAN also for a NaN in an end column read at a joined boundary; HF_E_SCALE per group; every other
 *                         refusal is the per-chunk entry point's (lengths, capacity, the forward lanes within nine tenths of the free
 *                         device memory).
 * Exact cases.  joined NULL or all zero gives hf_minlen_posterior / hf_sample_paths_minlen bit for bit: post, labels, both per-chunk
 * arrays, the total and every sample.  All four lengths 1, any joined: log_mass is exactly 0.0 in every entry, and post equals
 * hf_get_posterior of a full pass to rounding (the boundary row is of rank one).  A group's log_mass is never above the sum of its
 * chunks' per-chunk log_mass, to rounding; its log Z (log Z_adm - log_mass) equals the sum of its chunks' per-chunk log Z, to rounding.
 * Every sampled group path is admissible over the group, and a path of hf_viterbi_minlen_joined has non-zero probability.
 * Each call is asynchronous and shares its decoder's state with the per-chunk entry point: hf_minlen_posterior_finish and the
 * posterior's getters, hf_sample_minlen_finish and hf_get_minlen_sample_labels answer for the last finished run of either entry point,
 * and hf_minlen_sample_capacity holds for both.  The outputs are bitwise the same on both kinds of context, across repeated calls and on
 * any stream; the samples however they are grouped into calls.  hf_batch_* and hf_multi_* have no counterpart. */
int hf_minlen_posterior_joined(hf_ctx *ctx, const hf_params *p, const int32_t min_len[4],
                               const uint8_t *joined /* [n_chunks], NULL: none */, void *stream);
int hf_sample_paths_minlen_joined(hf_ctx *ctx, const hf_params *p, const int32_t min_len[4],
                                  const uint8_t *joined /* [n_chunks], NULL: none */,
                                  int64_t first_sample, int n_samples, uint64_t seed, void *stream);

/* Maximum-expected-accuracy decoding under minimum run lengths (flagger_amd/csrc/hf_mea.h): to posterior argmax what hf_viterbi_minlen
 * is to hf_viterbi.  Among the labellings whose runs meet the minimum lengths, the one with the largest expected gain under the
 * posterior of the last HF_MODE_FULL pass; with the identity gain, the largest expected number of correctly labelled windows.  A getter
 * of that pass, as hf_get_interval_log_probs is: no parameters, synchronous on the pass's stream.
 * Posterior and gains.  For a window t of a chunk, with f_t, b_t of the pass (hf_get_forward_backward):
 *   p_s        = f_t[s] * b_t[s]
 *   gamma_t(s) = p_s / (((p_0 + p_1) + p_2) + p_3)                 hf_get_posterior's value to rounding
 *   g_t(k)     = ((gamma_t(0) W[0][k] + gamma_t(1) W[1][k]) + gamma_t(2) W[2][k]) + gamma_t(3) W[3][k]
 * gain[s * 4 + k] = W[s][k] is the gain of calling k when the truth is s; NULL means the identity.  The expected gain of a labelling
 * is the sum over its windows of g_t(l_t).
 * Blocks.  joined and the groups are exactly those of hf_viterbi_minlen_joined (NULL: none joined; joined[0] != 0 is HF_E_ARG; a chunk
 * without windows ends a group).  A BLOCK is a chunk (joined NULL) or a group.
 * ADMISSIBLE: every maximal run of state s in the block's label sequence has at least min_len[s] windows; a run that contains the
 * block's first or last window is exempt.  The family's rule, lanes and limits: 1 <= min_len[s], sum <= HF_MINLEN_MAX_LANES.
 * SUPPORTED: the computed gamma_t(l_t) > 0 at every window, and A_t[l_{t-1}][l_t] > 0 at every window that is not the first of its
 * chunk (A_t: the row of the pass).  A step across a joined chunk boundary carries no condition of its own: the two chains are
 * independent, and the first condition at the two windows already implies end[p] > 0 and first[k] > 0.  In exact arithmetic, supported
 * means that every chunk's path has positive probability.
 * Result.  Per block, the admissible supported labelling with the largest expected gain: the walk of hf_viterbi_minlen in (max, +)
 * over gain rows in place of log rows and with an end column of zeros.  The rows:
 *   gk_t(k)   = g_t(k) if gamma_t(k) > 0, else -inf
 *   G_t[p][k] = gk_t(k)                                 at a chunk-first window (the four rows alike: the first window of a block and a
 *                                                       joined boundary are served by the same row)
 *   G_t[p][k] = gk_t(k) if A_t[p][k] > 0, else -inf     at every other window
 * Entry lanes, in-between lanes, saturated lanes, the exclusion of p == s, strict > with the lowest candidate winning, and the final
 * lane as the first largest in lane order are hf_viterbi_minlen's, word for word.  A block's score is its maximum;
 * block_gain_host[c] holds the score of chunk c, or with joined a group's score in the entry of its first chunk and 0.0 in the
 * others; *total_gain_host is their sum in list order.  A chunk without windows scores 0.0; windows outside every chunk get label -1.
 * HF_E_SCALE: a block has no admissible supported labelling.  HF_E_NAN: a NaN in a gain row.  HF_E_ARG: no full pass to answer for, the
 * length cases of hf_viterbi_minlen, joined[0] != 0, a NULL label array, a gain entry that is not finite or above 1e100 in magnitude.
 * Exact cases: lengths 1 with the identity give posterior argmax wherever the two largest posteriors differ by more than rounding;
 * a gain scaled by a power of two gives the same labels and scores scaled exactly.  Repeated calls return the same bits; HF_ALGO_SCAN
 * and HF_ALGO_SEQ contexts agree to rounding only (their f and b differ in the last bit).
 * Its buffers are its own (allocated by the first call): the last pass, every decoder's and sampler's results and the next hf_estep
 * are bitwise unaffected.  hf_batch_* and hf_multi_* have no counterpart. */
int hf_get_mea_labels(hf_ctx *ctx, const double *gain /* [16], NULL: identity */, const int32_t min_len[4],
                      const uint8_t *joined /* [n_chunks], NULL: none */, int8_t *labels_host /* [n_windows] */,
                      double *block_gain_host /* [n_chunks] or NULL */, double *total_gain_host /* or NULL */);

/* Posterior path sampling (forward filtering, backward sampling; flagger_amd/csrc/hf_sample.h): with the parameters `p` and the
 * quantities hf_viterbi uses, a sample of a chunk of T windows is a path s_0..s_{T-1} drawn with probability proportional to
 *   first[s_0] * prod_{t>=1} A_t[s_{t-1}][s_t] * end[s_{T-1}]
 * (the distribution whose marginals hf_get_posterior returns).  Uniforms are counter-based, so a sample depends only on
 * (seed, absolute sample index, window index): not on the algorithm, the segment plan or how samples are grouped into calls.
 * With splitmix64(x) the standard finaliser of x + 0x9E3779B97F4A7C15:
 *   key_k  = splitmix64(seed ^ splitmix64(k))           k = absolute sample index
 *   u(k,i) = (splitmix64(key_k + i) >> 11) * 2^-53      i = global window index t (the draw of window t),
 *                                                       i = n_windows + c (the final-state draw of chunk c)
 * Draw rule: window t >= 1 of a chunk, state s at t: w_p = alpha_{t-1}[p] * A_t[p][s] (alpha: the forward vector, any power-of-two
 * scale), c_0 = w_0, c_p = c_{p-1} + w_p, x = u * c_3; the state at t-1 is the smallest p with x < c_p, else the largest p with
 * w_p > 0, else 0.  The final state: the same rule with w_s = alpha_{T-1}[s] * end[s].
 * hf_sample_paths draws samples first_sample .. first_sample + n_samples - 1 asynchronously on `stream`; hf_sample_finish waits and
 * translates the flags (HF_E_NAN: a NaN in a row or the end column, HF_E_SCALE: a chunk's forward vector or final weights all 0).
 * HF_E_ARG: n_samples < 1 or above hf_sample_capacity (samples per call that fit nine tenths of the free device memory), k out of
 * range, a getter before any finished call.  The sampler's buffers are its own: the last pass's results, Viterbi's and the next
 * hf_estep are unaffected.  Streams: as hf_viterbi (any stream of the caller's; hf_sample_finish takes the same one). */
int hf_sample_capacity(const hf_ctx *ctx);
int hf_sample_paths(hf_ctx *ctx, const hf_params *p, int64_t first_sample, int n_samples, uint64_t seed, void *stream);
int hf_sample_finish(hf_ctx *ctx, void *stream);
int hf_get_sample_labels(hf_ctx *ctx, int k, int8_t *labels_host);                    /* sample first_sample + k, [n_windows] */

/* Many models on one context (flagger_amd/csrc/hf_batch.h): e.g. one EM per candidate alpha matrix over the same track, with the
 * windows loaded, uploaded and planned once.  A batch keeps the pass state of n_models models beside the context: every model has its
 * own parameter block, tables, rows of A, hand-off flags and epochs, pair records, sums, labels, error flags and result block, and shares
 * the context's windows, segment plan, row stream and statistics plan.  The context's own pass buffers are never written:
 * hf_estep / hf_get_* / hf_viterbi on `ctx` behave as without a batch, before, between and after batched passes.
 * Model m of a batch runs the kernels, the arithmetic and the order of hf_estep on `ctx` with the same hf_params, in the context's
 * statistics mode and launch mode: its statistics, log-likelihood and labels are the single path's bits.
 * The batch engine covers HF_ALGO_SCAN contexts of one sub-pass (hf_sub_passes == 1) and the trunc_exp_gaussian and gaussian models;
 * otherwise hf_batch_capacity returns 0 and hf_batch_create HF_E_ARG (hf_last_error says why).  hf_create takes no model type, so a
 * context is known to serve negative_binomial only once it has run such a pass: from then on capacity is 0 and hf_batch_create
 * refuses it; before that, hf_batch_estep refuses negative_binomial parameters (HF_E_ARG).  The context must outlive the batch.
 * Full passes of the default pass (one-launch segment kernel, statistics by emission row) run the segment kernel of all their
 * models in ONE launch (k_seg_fb_batch: blockIdx.y = model); the tables and the statistics run per model.
 *   hf_batch_capacity   models whose pass state fits nine tenths of the device's free memory and whose pinned host blocks fit an
 *                       eighth of the host's physical memory (at most HF_BATCH_MAX_MODELS)
 *   hf_batch_estep      one pass of each of the n_active models models[0..n_active-1] (distinct indices < n_models) with p[i] for
 *                       model models[i], enqueued on `stream` in that order; the other models keep the results of their last pass
 *   hf_batch_finish     waits for the models of the last hf_batch_estep: stats_host[i][hf_chunk_stats_len] and status[i] (HF_OK,
 *                       HF_E_SCALE, HF_E_NAN, ...) for models[i].  A model's own failure is its status only; the call returns HF_OK
 *                       unless the runtime or an argument failed.  A timed-out hand-off (HF_E_RETRY) re-runs that model's pass inside.
 *   hf_batch_get_labels / hf_batch_get_posterior: as hf_get_labels / hf_get_posterior, for the last finished pass of `model`
 * Streams: hf_batch_estep is asynchronous on `stream` (any stream of the caller's, as hf_estep), hf_batch_finish blocks until that
 * stream has drained; the two getters run on the stream of the model's last pass and block until their result is there. */
#define HF_BATCH_MAX_MODELS 1024
typedef struct hf_batch hf_batch;
int hf_batch_capacity(const hf_ctx *ctx);
int hf_batch_create(hf_ctx *ctx, int n_models, hf_batch **out);
void hf_batch_destroy(hf_batch *b);
int hf_batch_size(const hf_batch *b);
int hf_batch_shared_models(const hf_batch *b);   /* models of the last hf_batch_estep whose segment kernel ran in the shared launch */
/* Diagnostics (the test suite): *epoch = the hand-off epoch of model `model`'s pass (advanced once per launch of a segment kernel that
 * the model takes part in); ready_host[0 .. min(n, segments)) = the flag word of every chunk segment, in segment order: the epoch of
 * the last one-launch pass in which the segment published its product (segments of one-segment chunks publish nothing: 0).  Waits for
 * the model's last pass.  Returns the number of segments of the context, or a negative HF_E_*. */
int64_t hf_batch_handoff(hf_batch *b, int model, uint32_t *epoch, uint32_t *ready_host, int64_t n);
int hf_batch_estep(hf_batch *b, const hf_params *p, const int32_t *models, int n_active, int mode, void *stream);
int hf_batch_finish(hf_batch *b, double *stats_host, int32_t *status, void *stream);
int hf_batch_get_labels(hf_batch *b, int model, int8_t *labels_host);
int hf_batch_get_posterior(hf_batch *b, int model, int64_t first, int64_t n, double *post_host);

/* kernel time of the last hf_estep + reduce in milliseconds (HIP events on the stream used); recorded only while
 * hf_set_profiling's mask carries HF_PROF_PASS (two extra stream packets per pass) */
int hf_last_kernel_ms(hf_ctx *ctx, float *ms);

/* Per-kernel timing (bench.py's roofline leg): every kernel k whose bit is set in kernel_mask is bracketed
 * by a pair of HIP events on the launch stream; hf_kernel_times returns the duration of each selected kernel in
 * the LAST pass in milliseconds (0 for kernels not selected or not run).  Call after hf_finish/hf_check.
 * Each selected kernel adds two event packets to the stream, so select only what is being measured. */
#define HF_NKERNELS 16
/* indices 1..3 are reserved (round 1's tile kernels, retired in round 2: no name, never run; the later indices keep their values) */
enum { HF_K_TABLES = 0, HF_K_STATS_TILE = 4, HF_K_CHUNK_STATS, HF_K_REDUCE,
       HF_K_EMIT_ROWS, HF_K_FWD_SEQ, HF_K_BWD_SEQ, HF_K_PAIR_SUMS, HF_K_ROW_STATS, HF_K_ROWS_TOTAL, HF_K_SEG_PROD, HF_K_SEG_FB, HF_K_AROWS };
#define HF_PROF_PASS 0x80000000u   /* in kernel_mask: also bracket the whole pass (hf_last_kernel_ms) */
int hf_set_profiling(hf_ctx *ctx, unsigned kernel_mask);
/* Bracket the selected kernels only in every n-th pass (default 1: every pass): an event pair costs a few microseconds of
 * a 0.2 ms pass, so a timed loop can sample the dominant kernel's duration without carrying the cost in every step. */
int hf_set_profiling_stride(hf_ctx *ctx, int every_nth_pass);
int hf_kernel_times(hf_ctx *ctx, float ms[HF_NKERNELS]);
/* Sum of the durations (ms) and number of timed launches of every selected kernel over all passes finished by
 * hf_finish / hf_em_iterate since the last hf_set_profiling: one call after a timed loop instead of one per pass. */
int hf_kernel_time_sums(hf_ctx *ctx, double sum_ms[HF_NKERNELS], int64_t launches[HF_NKERNELS]);
const char *hf_kernel_name(int k);   /* "k_tables", "k_seg_fb", ... as they appear in a rocprofv3 kernel trace */

/* Self-test hook: fast[i] = a[i] / d[i] through the shared-denominator form the statistics kernel uses (hf_device.h
 * prediv / divp), exact[i] = the plain division, safe[i] = whether the kernel's guard would take the fast form.
 * fast must equal exact bit for bit wherever safe is set. */
int hf_selftest_division(int device, int64_t n, const double *a, const double *d, double *fast, double *exact, int32_t *safe);
/* Self-test hook: csrc/hf_exp.h — glibc's exp for double restated, fused where the host's FMA build fuses (the emission densities of the
 * reference call libm's: hmm_utils.c:782, 945) — for n arguments: dev_out[i] computed on the device, host_out[i] by the same function compiled
 * for the host, libm_out[i] = the host's libm exp.  All three must hold the same bits on a host whose libm runs its FMA variant.  (The
 * emission kernels themselves use the device library's exp unless built with -DHF_EXP_OCML=0: hf_device.h says why.) */
int hf_selftest_exp(int device, int64_t n, const double *x, double *dev_out, double *host_out, double *libm_out);

#ifdef __cplusplus
}
#endif
#endif
