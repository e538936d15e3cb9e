// hf_decoders.hip — the path decoders of the C ABI (include/hmm_flagger_hip.h), a translation unit of its own: Viterbi (hf_viterbi.h)
// and posterior path sampling (hf_sample.h) over the core they share (hf_decode.h), kernels and host side.  Each decoder has its own
// parameter block, rows, flags and outputs, so that the last pass's getters (which re-run the segment kernel over the pass's tables), the
// next pass and the other decoder see nothing of it.  The context and the host templates every decoder front uses come from hf_host.h;
// the minimum-run-length family (hf_minlen.hip) finishes its runs through dec_finish* and smp_* below and launches k_dec_rows_win
// through dec_launch_rows_win.
#include "hf_host.h"
#include "hf_viterbi.h"
#include "hf_sample.h"

static bool dec_scan(const Track& tr) { return tr.algo == HF_ALGO_SCAN; }
static size_t dec_nrow(const Track& tr) { return dec_scan(tr) ? (size_t) tr.n_slots : (size_t) tr.N; }   // rows and map bytes per path
static size_t dec_nseg(const Track& tr) { return dec_scan(tr) ? (size_t) tr.nseg : 0; }

// Every device array of a decoder, f(array, bytes) in turn: the ONE place that sizes them (dec_take allocates them, hf_sample_capacity
// counts them).  What dec_front fills and every decoder has (dec_front_arrays, hf_host.h; nrow rows); SCAN: the arrays of A and B, with
// their exponent sums when the decoder reports a score.
template <class D, class F> static void dec_arrays(const Track& tr, D& d, bool score, F&& f) {
    const size_t G = dec_nseg(tr);
    dec_front_arrays(tr, d, dec_nrow(tr), f);
    if (dec_scan(tr)) {
        f(d.d_P, G * 16 * 64 * 8); f(d.d_S, G * 16 * 8); f(d.d_vin, G * 4 * 8);
        if (score) { f(d.d_PE, G * 64 * 4); f(d.d_SE, G * 4); f(d.d_vinE, G * 8); }
    }
}
template <class F> static void vit_arrays(const Track& tr, Viterbi& v, F&& f) {
    const size_t G = dec_nseg(tr);
    dec_arrays(tr, v, true, f);
    f(v.d_bp, dec_nrow(tr)); f(v.d_label, (size_t) tr.N); f(v.d_chunk, (size_t) tr.C * 8); f(v.d_final, (size_t) tr.C);
    if (dec_scan(tr)) { f(v.d_lmap, G * 64); f(v.d_smap, G); f(v.d_sexit, G); }
}
// the per-sample part for k samples: keys, map bytes, labels; SCAN: final states, lane and segment maps, exit states
template <class S, class F> static void smp_arrays(const Track& tr, S& s, size_t k, F&& f) {
    const size_t G = dec_nseg(tr);
    f(s.d_keys, k * 8); f(s.d_maps, k * dec_nrow(tr)); f(s.d_label, k * (size_t) tr.N);
    if (dec_scan(tr)) { f(s.d_final, k * (size_t) tr.C); f(s.d_lmap, k * G * 64); f(s.d_smap, k * G); f(s.d_sexit, k * G); }
}

// the rows of every window in window order (HF_ALGO_SEQ, and every decoder of the minimum-run-length family), for the decoder d
void dec_launch_rows_win(const Track& tr, const Decoder& d, const double* nbE, hipStream_t st) {
    hipLaunchKernelGGL(k_dec_rows_win, dim3((unsigned) ((tr.N + 255) / 256)), dim3(256), 0, st, tr.N, tr.d_rec, tr.d_beta, d.d_params, nbE,
                       d.d_rows, d.d_flags);
}

// hf_viterbi and the sampler: the refusal of a scan context without a segment plan, dec_front, then on `st` the rows and, on the scan
// path, steps A and B in the semiring SR.
template <class SR, class Prep>
static int dec_begin(const Track& tr, Decoder& d, const hf_params* p, hipStream_t st, const char* who, Prep&& prepare) {
    HIPCHK(hipSetDevice(tr.device));
    const std::string w = who;
    if (tr.algo == HF_ALGO_SCAN && tr.N > 0 && tr.C > 0 && tr.nseg == 0)
        return set_err(HF_E_ARG, w + ": HF_ALGO_SCAN holds at most 2^30 windows per context");
    const double* nbE = nullptr;
    const int rc = dec_front(tr, d, p, st, w, prepare, nbE);
    if (rc || !dec_work(tr)) return rc;
    if (dec_scan(tr)) {
        const unsigned G = (unsigned) tr.nseg, CB = (unsigned) ((tr.C + 63) / 64);
        hipLaunchKernelGGL(k_dec_rows_seg, dim3(G), dim3(64), 0, st, tr.d_seg, tr.d_rec, tr.d_beta, d.d_params, nbE, d.d_rows, d.d_flags);
        hipLaunchKernelGGL(k_dec_prod<SR>, dim3(G), dim3(64), 0, st, tr.d_seg, d.d_rows, d.d_P, d.d_PE, d.d_S, d.d_SE);
        hipLaunchKernelGGL(k_dec_chain<SR>, dim3(CB), dim3(64), 0, st, tr.C, tr.d_chunk_seg0, d.d_S, d.d_SE, d.d_vin, d.d_vinE);
    } else
        dec_launch_rows_win(tr, d, nbE, st);
    return HF_OK;
}

// D on the scan path: K paths' exit states and labels from their maps
static void dec_back(const Track& tr, hipStream_t st, unsigned K, const uint8_t* maps, const uint8_t* lmap, const uint8_t* smap,
                     const int8_t* final_state, uint8_t* sexit, int8_t* label) {
    const unsigned G = (unsigned) tr.nseg, CB = (unsigned) ((tr.C + 63) / 64);
    hipLaunchKernelGGL(k_dec_exits, dim3(CB, K), dim3(64), 0, st, tr.C, (int) G, tr.d_chunk_seg0, smap, final_state, sexit);
    hipLaunchKernelGGL(k_dec_back, dim3(G, K), dim3(64), 0, st, tr.d_seg, maps, tr.n_slots, (int) G, tr.N, lmap, sexit, label);
}

// the wait for a decoder's run and its flag word
int dec_finish(const Track& tr, Decoder& d, void* stream) {
    HIPCHK(hipSetDevice(tr.device));
    HIPCHK(hipStreamSynchronize((hipStream_t) stream));
    d.launched = false;
    unsigned fl = 0;
    HIPCHK(hipMemcpy(&fl, d.d_flags, 4, hipMemcpyDeviceToHost));
    return fl ? flags_to_code(fl) : HF_OK;
}

// ---- the decoders that leave labels and `per` values per chunk (LabelDecoder) ----
// what the kernels do not write: the values of chunks without windows (0), the labels of windows outside every chunk (-1)
int dec_clear_outputs(const Track& tr, LabelDecoder& d, int per, hipStream_t st) {
    if (tr.C > 0) HIPCHK(hipMemsetAsync(d.d_chunk, 0, (size_t) tr.C * per * 8, st));
    if (!all_in_chunks(tr)) HIPCHK(hipMemsetAsync(d.d_label, 0xff, (size_t) tr.N, st));
    return HF_OK;
}

// dec_finish, then the chunk values to the host copy; the run counts as finished
int dec_finish_chunks(const Track& tr, LabelDecoder& d, int per, void* stream) {
    const int rc = dec_finish(tr, d, stream);
    if (rc) return rc;
    d.h_chunk.assign((size_t) tr.C * per, 0.0);
    if (tr.C > 0) HIPCHK(hipMemcpy(d.h_chunk.data(), d.d_chunk, (size_t) tr.C * per * 8, hipMemcpyDeviceToHost));
    d.done = true;
    return HF_OK;
}

// ... for a decoder with one score per chunk: their sum in chunk-list order
int dec_finish_scores(const Track& tr, LabelDecoder& d, double* log_prob_host, void* stream) {
    const int rc = dec_finish_chunks(tr, d, 1, stream);
    if (rc) return rc;
    double tot = 0.0;
    for (double x : d.h_chunk) tot += x;
    if (log_prob_host) *log_prob_host = tot;
    return HF_OK;
}

int dec_labels(const Track& tr, const LabelDecoder& d, int8_t* labels_host) {
    HIPCHK(hipSetDevice(tr.device));
    if (tr.N > 0) HIPCHK(hipMemcpy(labels_host, d.d_label, (size_t) tr.N, hipMemcpyDeviceToHost));
    return HF_OK;
}

// the first value of every chunk
int dec_chunk_values(const Track& tr, const LabelDecoder& d, double* out_host) {
    if (tr.C > 0) std::memcpy(out_host, d.h_chunk.data(), (size_t) tr.C * 8);
    return HF_OK;
}

int hf_viterbi(hf_ctx* ctx, const hf_params* p, void* stream) {
    if (!ctx || !p) return set_err(HF_E_ARG, "hf_viterbi: bad argument");
    const Track& tr = ctx->tr;
    Viterbi& v = ctx->vit;
    hipStream_t st = (hipStream_t) stream;
    int rc = dec_begin<MaxTimes>(tr, v, p, st, "hf_viterbi",
                                 [&] { return dec_alloc(tr, v, [&](auto&& f) { vit_arrays(tr, v, f); }); });
    if (rc || (rc = dec_clear_outputs(tr, v, 1, st))) return rc;
    if (dec_work(tr)) {
        if (dec_scan(tr)) {
            hipLaunchKernelGGL(k_vit_replay, dim3((unsigned) tr.nseg), dim3(64), 0, st, tr.d_seg, tr.d_rec, v.d_params, v.d_rows, v.d_P,
                               v.d_PE, v.d_vin, v.d_vinE, v.d_bp, v.d_lmap, v.d_smap, v.d_final, v.d_chunk, v.d_flags);
            dec_back(tr, st, 1, v.d_bp, v.d_lmap, v.d_smap, v.d_final, v.d_sexit, v.d_label);   // (the backpointers: one path's maps)
        } else {
            hipLaunchKernelGGL(k_vit_seq, dim3((unsigned) tr.C), dim3(64), 0, st, tr.d_off, tr.d_rec, v.d_params, v.d_rows, v.d_bp,
                               v.d_label, v.d_chunk, v.d_flags);
        }
    }
    HIPCHK(hipGetLastError());
    v.launched = true;
    return HF_OK;
}

int hf_viterbi_finish(hf_ctx* ctx, double* log_prob_host, void* stream) {
    if (!ctx || !ctx->vit.launched) return set_err(HF_E_ARG, "hf_viterbi_finish: no hf_viterbi to finish");
    return dec_finish_scores(ctx->tr, ctx->vit, log_prob_host, stream);
}

int hf_get_viterbi_labels(hf_ctx* ctx, int8_t* labels_host) {
    if (!ctx || !labels_host || !ctx->vit.done) return set_err(HF_E_ARG, "hf_get_viterbi_labels: no finished hf_viterbi");
    return dec_labels(ctx->tr, ctx->vit, labels_host);
}

int hf_get_viterbi_chunk_log_probs(hf_ctx* ctx, double* out_host) {
    if (!ctx || !out_host || !ctx->vit.done) return set_err(HF_E_ARG, "hf_get_viterbi_chunk_log_probs: no finished hf_viterbi");
    return dec_chunk_values(ctx->tr, ctx->vit, out_host);
}

int hf_sample_capacity(const hf_ctx* ctx) {
    if (!ctx) return set_err(HF_E_ARG, "hf_sample_capacity: bad argument");
    const Track& tr = ctx->tr; const Sampler& s = ctx->smp;
    HIPCHK(hipSetDevice(tr.device));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    size_t fixed = 0, per = 0;   // the fixed slab; the per-sample arrays of one sample
    dec_arrays(tr, s, false, [&](auto&, size_t bytes) { fixed += Slab::granule(bytes); });
    smp_arrays(tr, s, 1, [&](auto&, size_t bytes) { per += bytes; });
    // what the sampler holds already counts as free: a call reuses (or replaces) it
    const double held = (s.alloc ? (double) fixed : 0.0) + (double) s.cap * (double) per;
    const double budget = 0.9 * ((double) free_b + held) - (double) fixed;
    if (budget < (double) per) return 0;
    const double cap = std::floor(budget / (double) per);
    return cap > HF_SMP_MAX_PER_CALL ? HF_SMP_MAX_PER_CALL : (int) cap;
}

// ---- the per-sample part of a sampler (SampleSet; smp_grow: hf_host.h) ----
// the keys of samples first .. first + n - 1 (synchronous)
int smp_keys(SampleSet& s, int64_t first, int n, uint64_t seed) {
    s.h_keys.resize((size_t) n);
    for (int k = 0; k < n; k++) s.h_keys[(size_t) k] = hf_sample_key(seed, (uint64_t) (first + k));
    HIPCHK(hipMemcpy(s.d_keys, s.h_keys.data(), (size_t) n * 8, hipMemcpyHostToDevice));
    return HF_OK;
}

// dec_finish; the run counts as finished
int smp_finish(const Track& tr, Decoder& d, void* stream) {
    const int rc = dec_finish(tr, d, stream);
    if (rc) return rc;
    d.done = true;
    return HF_OK;
}

// the labels of sample k of the last call, for the getter `who`
int smp_labels(const Track& tr, const SampleSet& s, const char* who, int k, int8_t* labels_host) {
    if (k < 0 || k >= s.n) return set_err(HF_E_ARG, std::string(who) + ": k out of range");
    HIPCHK(hipSetDevice(tr.device));
    if (tr.N > 0) HIPCHK(hipMemcpy(labels_host, s.d_label + (int64_t) k * tr.N, (size_t) tr.N, hipMemcpyDeviceToHost));
    return HF_OK;
}

// the sampler's buffers for n samples and the keys of samples first .. first + n - 1
static int smp_prepare(hf_ctx* ctx, int64_t first, int n, uint64_t seed) {
    const Track& tr = ctx->tr; Sampler& s = ctx->smp;
    if (n > s.cap) {
        const int cap = hf_sample_capacity(ctx);
        if (cap < 0) return cap;
        if (n > cap) return set_err(HF_E_ARG, "hf_sample_paths: n_samples exceeds hf_sample_capacity (" + std::to_string(cap) + ")");
    }
    int rc = dec_alloc(tr, s, [&](auto&& f) { dec_arrays(tr, s, false, f); });
    if (rc || (rc = smp_grow(s, n, [&](auto&& f) { smp_arrays(tr, s, (size_t) n, f); }))) return rc;
    return smp_keys(s, first, n, seed);
}

int hf_sample_paths(hf_ctx* ctx, const hf_params* p, int64_t first_sample, int n_samples, uint64_t seed, void* stream) {
    if (!ctx || !p) return set_err(HF_E_ARG, "hf_sample_paths: bad argument");
    if (n_samples < 1) return set_err(HF_E_ARG, "hf_sample_paths: n_samples must be >= 1");
    if (first_sample < 0) return set_err(HF_E_ARG, "hf_sample_paths: first_sample must be >= 0");
    const Track& tr = ctx->tr;
    Sampler& s = ctx->smp;
    hipStream_t st = (hipStream_t) stream;
    const int rc = dec_begin<SumTimes>(tr, s, p, st, "hf_sample_paths", [&] { return smp_prepare(ctx, first_sample, n_samples, seed); });
    if (rc) return rc;
    if (!all_in_chunks(tr)) HIPCHK(hipMemsetAsync(s.d_label, 0xff, (size_t) n_samples * (size_t) tr.N, st));   // (windows outside every chunk: label -1)
    if (dec_work(tr)) {
        if (dec_scan(tr)) {
            const unsigned G = (unsigned) tr.nseg, K = (unsigned) n_samples;
            hipLaunchKernelGGL(k_smp_replay, dim3(G), dim3(64), 0, st, tr.d_seg, tr.d_rec, s.d_params, s.d_rows, s.d_P, s.d_vin, s.d_keys,
                               n_samples, tr.N, tr.C, tr.n_slots, s.d_maps, s.d_final, s.d_flags);
            hipLaunchKernelGGL(k_smp_maps, dim3(G, K), dim3(64), 0, st, tr.d_seg, s.d_maps, tr.n_slots, (int) G, s.d_lmap, s.d_smap);
            dec_back(tr, st, K, s.d_maps, s.d_lmap, s.d_smap, s.d_final, s.d_sexit, s.d_label);
        } else {
            hipLaunchKernelGGL(k_smp_seq, dim3((unsigned) tr.C), dim3(64), 0, st, tr.d_off, tr.d_rec, s.d_params, s.d_rows, s.d_keys,
                               n_samples, tr.N, tr.C, s.d_maps, s.d_label, s.d_flags);
        }
    }
    HIPCHK(hipGetLastError());
    s.n = n_samples;
    s.launched = true;
    return HF_OK;
}

int hf_sample_finish(hf_ctx* ctx, void* stream) {
    if (!ctx || !ctx->smp.launched) return set_err(HF_E_ARG, "hf_sample_finish: no hf_sample_paths to finish");
    return smp_finish(ctx->tr, ctx->smp, stream);
}

int hf_get_sample_labels(hf_ctx* ctx, int k, int8_t* labels_host) {
    if (!ctx || !labels_host || !ctx->smp.done) return set_err(HF_E_ARG, "hf_get_sample_labels: no finished hf_sample_paths");
    return smp_labels(ctx->tr, ctx->smp, "hf_get_sample_labels", k, labels_host);
}
