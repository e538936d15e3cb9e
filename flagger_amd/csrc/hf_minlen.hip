// hf_minlen.hip — the minimum-run-length family of the C ABI (include/hmm_flagger_hip.h), a translation unit of its own: Viterbi
// (hf_minlen.h, hf_minlen_joined.h), the posterior (hf_minlen_post.h), admissible path sampling (hf_minlen_sample.h), the two over groups
// of joined chunks (hf_minlen_post_joined.h), maximum-expected-accuracy decoding (hf_mea.h) and the E-step, per chunk and over groups
// (hf_minlen_em.h, hf_minlen_em_joined.h), kernels and host side.  The context and the decoders' shared host side come from hf_host.h; kernels of the other units (k_dec_rows_win, k_tables,
// k_chunk_stats, k_reduce) are launched through their owners' launchers.  THE ORDER OF THE KERNEL HEADERS BELOW IS PART OF THE BUILD
// (DESIGN.md 7k-m): each stands where it stood in the one-unit file relative to the others of this family, hf_minlen_joined.h last.
// Nothing outside this unit bears on its kernels' code.
#define HF_HELPERS_ONLY   // of hf_decode.h, hf_sample.h (kernels: hf_decoders.hip) and hf_scan.h, hf_chunks.h (kernels: hf_estep.hip)
#include "hf_host.h"
#include "hf_jobs.h"   // chunk_continues: the one statement of which chunks form a group

// ------------------------------------------------------------------------------------------
// minimum-run-length Viterbi (hf_minlen.h): a decoder of its own beside hf_viterbi, one code path for both kinds of context (rows in
// window order, one wavefront per chunk).  hf_viterbi_minlen_joined applies the rule to groups of joined chunks: the same decoder
// (ctx->mlv, its buffers, hf_viterbi_minlen_finish and the two getters) and the same host run (mlv_run, which cuts the groups of a
// call); its forward walk is a second body, k_mlvj_fwd, included last in this file.  With it comes hf_chain.h, the core it shares with the sections after it: wave primitives, lane geometry,
// row staging; and minlen_front, the front of every call of the family.
// ------------------------------------------------------------------------------------------
#include "hf_minlen.h"

static_assert(HF_MINLEN_MAX_LANES == 64, "one wavefront holds the expanded chain");

// every device array of the decoder, f(array, bytes) in turn (as vit_arrays)
template <class F> static void mlv_arrays(const Track& tr, MinLenViterbi& v, F&& f) {
    dec_front_arrays(tr, v, (size_t) tr.N, f);
    f(v.d_bp, (size_t) tr.N * 2); f(v.d_label, (size_t) tr.N); f(v.d_chunk, (size_t) tr.C * 8); f(v.d_final, (size_t) tr.C);
    f(v.d_goff, ((size_t) tr.C + 1) * 8); f(v.d_gchunk, (size_t) tr.C * 4);
}

// the four minimum lengths of a call to `who`: every one >= 1, at most HF_MINLEN_MAX_LANES lanes together
static int minlen_check(const std::string& who, const int32_t min_len[4], int64_t* lanes) {
    *lanes = 0;
    for (int s = 0; s < 4; s++) {
        if (min_len[s] < 1) return set_err(HF_E_ARG, who + ": every minimum length must be >= 1");
        *lanes += min_len[s];
    }
    if (*lanes > HF_MINLEN_MAX_LANES)
        return set_err(HF_E_ARG, who + ": the minimum lengths sum to " + std::to_string(*lanes) + ", above HF_MINLEN_MAX_LANES (64)");
    return HF_OK;
}

// what every entry point that takes `joined` refuses (joined null: every chunk a group of its own)
static int mlg_refuse(const hf_ctx* ctx, const uint8_t* joined, const std::string& w) {
    return joined && ctx->tr.C > 0 && joined[0] ? set_err(HF_E_ARG, w + ": joined[0] must be 0 (the first chunk continues nothing)") : (int) HF_OK;
}

// free device memory plus `held`: the bytes a decoder holds already count as free, a call reuses or replaces them
static int mem_avail(double held, double* avail) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    *avail = (double) free_b + held;
    return HF_OK;
}

// the refusal of a buffer of `bytes`, of which the decoder holds `held` (enough: nothing to refuse), above nine tenths of that:
// "<w>: <what> need <bytes> bytes (<formula>), above nine tenths of the free device memory"
static int mem_refuse(const std::string& w, const char* what, size_t bytes, size_t held, const char* formula) {
    if (bytes <= held) return HF_OK;
    double avail = 0.0;
    const int rc = mem_avail((double) held, &avail);
    if (rc) return rc;
    if ((double) bytes > 0.9 * avail)
        return set_err(HF_E_ARG, w + ": " + what + " need " + std::to_string(bytes) + " bytes (" + formula + "), above nine tenths of the free device memory");
    return HF_OK;
}

// windows first .. first + n - 1 of d_array, `per` doubles per window, for the getter `w` of a finished `run`
static int minlen_get_range(hf_ctx* ctx, const std::string& w, const char* run, bool done, const double* d_array, int per, int64_t first,
                            int64_t n, double* out_host) {
    if (!ctx || !out_host || !done) return set_err(HF_E_ARG, w + ": no finished " + run);
    const Track& tr = ctx->tr;
    if (first < 0 || n < 0 || first + n > tr.N) return set_err(HF_E_ARG, w + ": bad range");
    if (n > 0 && !in_chunks(tr, first, first + n - 1)) return set_err(HF_E_ARG, w + ": the range holds a window outside every chunk");
    HIPCHK(hipSetDevice(tr.device));
    if (n > 0) HIPCHK(hipMemcpy(out_host, d_array + first * per, (size_t) n * per * 8, hipMemcpyDeviceToHost));
    return HF_OK;
}

// The front of every call of the family, error messages naming the entry point `w`: the refusal of a null argument, minlen_check (it
// leaves the sum of the lengths in `lanes`), `refuse` (what else the entry point refuses before it touches the decoder), then dec_front
// on the context's decoder `dec` with prepare(track, decoder), which may use `lanes`.
template <class D, class Refuse, class Prep>
static int minlen_front(hf_ctx* ctx, D hf_ctx::* dec, const hf_params* p, const int32_t min_len[4], hipStream_t st, const std::string& w,
                        Refuse&& refuse, Prep&& prepare, int64_t& lanes, const double*& nbE) {
    if (!ctx || !p || !min_len) return set_err(HF_E_ARG, w + ": bad argument");
    int rc = minlen_check(w, min_len, &lanes);
    if (rc || (rc = refuse())) return rc;
    return dec_front(ctx->tr, ctx->*dec, p, st, w, [&] { return prepare(ctx->tr, ctx->*dec); }, nbE);
}

// hf_viterbi_minlen (!whole: a block of the walks is a chunk) and hf_viterbi_minlen_joined (whole: a group of joined chunks, cut here;
// joined null: every chunk a group of its own)
static int mlv_run(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], bool whole, const uint8_t* joined, hipStream_t st,
                   const std::string& w) {
    int64_t lanes = 0;
    const double* nbE = nullptr;
    int rc = minlen_front(ctx, &hf_ctx::mlv, p, min_len, st, w, [&] { return mlg_refuse(ctx, joined, w); },
                          [](const Track& tr, MinLenViterbi& v) { return dec_alloc(tr, v, [&](auto&& f) { mlv_arrays(tr, v, f); }); }, lanes, nbE);
    if (rc) return rc;
    const Track& tr = ctx->tr;
    MinLenViterbi& v = ctx->mlv;
    if ((rc = dec_clear_outputs(tr, v, 1, st))) return rc;
    if (dec_work(tr)) {
        const int l0 = (int) min_len[0], l1 = (int) min_len[1], l2 = (int) min_len[2], l3 = (int) min_len[3];
        const int64_t* d_boff = tr.d_off;               // the window ranges of the walks' blocks
        unsigned B = (unsigned) tr.C;
        if (whole) {
            // a chunk starts a group unless it is joined to its predecessor and both have windows (a chunk without windows has no part)
            const std::vector<int64_t>& off = tr.h_off;
            v.h_goff.clear(); v.h_gchunk.clear();
            for (int c = 0; c < tr.C; c++) {
                if (!chunk_continues(off.data(), tr.C, joined, c)) { v.h_gchunk.push_back(c); v.h_goff.push_back(off[(size_t) c]); }
            }
            v.h_goff.push_back(off[(size_t) tr.C]);
            const size_t G = v.h_gchunk.size();
            HIPCHK(hipMemcpyAsync(v.d_goff, v.h_goff.data(), (G + 1) * 8, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(v.d_gchunk, v.h_gchunk.data(), G * 4, hipMemcpyHostToDevice, st));
            d_boff = v.d_goff; B = (unsigned) G;
        }
        hipLaunchKernelGGL(k_mlv_rows, dim3((unsigned) ((tr.N + 255) / 256)), dim3(256), 0, st, tr.N, tr.d_rec, tr.d_beta, v.d_params, nbE,
                           v.d_rows, v.d_flags);
        if (whole)
            hipLaunchKernelGGL(k_mlvj_fwd, dim3(B), dim3(64), 0, st, d_boff, v.d_gchunk, tr.d_rec, v.d_params, v.d_rows, l0, l1, l2, l3, v.d_bp,
                               v.d_final, v.d_chunk, v.d_flags);
        else
            hipLaunchKernelGGL(k_mlv_fwd, dim3(B), dim3(64), 0, st, d_boff, tr.d_rec, v.d_params, v.d_rows, l0, l1, l2, l3, v.d_bp, v.d_final,
                               v.d_chunk, v.d_flags);
        hipLaunchKernelGGL(k_mlv_back, dim3(B), dim3(64), 0, st, d_boff, l0, l1, l2, l3, v.d_bp, v.d_final, v.d_label);
    }
    HIPCHK(hipGetLastError());
    v.launched = true;
    return HF_OK;
}

int hf_viterbi_minlen(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], void* stream) {
    return mlv_run(ctx, p, min_len, false, nullptr, (hipStream_t) stream, "hf_viterbi_minlen");
}

int hf_viterbi_minlen_joined(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], const uint8_t* joined, void* stream) {
    return mlv_run(ctx, p, min_len, true, joined, (hipStream_t) stream, "hf_viterbi_minlen_joined");
}

int hf_viterbi_minlen_finish(hf_ctx* ctx, double* log_prob_host, void* stream) {
    if (!ctx || !ctx->mlv.launched) return set_err(HF_E_ARG, "hf_viterbi_minlen_finish: no hf_viterbi_minlen to finish");
    return dec_finish_scores(ctx->tr, ctx->mlv, log_prob_host, stream);
}

int hf_get_viterbi_minlen_labels(hf_ctx* ctx, int8_t* labels_host) {
    if (!ctx || !labels_host || !ctx->mlv.done) return set_err(HF_E_ARG, "hf_get_viterbi_minlen_labels: no finished hf_viterbi_minlen");
    return dec_labels(ctx->tr, ctx->mlv, labels_host);
}

int hf_get_viterbi_minlen_chunk_log_probs(hf_ctx* ctx, double* out_host) {
    if (!ctx || !out_host || !ctx->mlv.done) return set_err(HF_E_ARG, "hf_get_viterbi_minlen_chunk_log_probs: no finished hf_viterbi_minlen");
    return dec_chunk_values(ctx->tr, ctx->mlv, out_host);
}


// ------------------------------------------------------------------------------------------
// posteriors under minimum run lengths (hf_minlen_post.h): the sum-product twin of hf_viterbi_minlen, a decoder of its own with one code
// path for both kinds of context.
// ------------------------------------------------------------------------------------------
#include "hf_minlen_post.h"

// every device array of the decoder but the forward lanes (their size depends on the lengths of a call: MinLenPosterior::fwd)
template <class F> static void mlp_arrays(const Track& tr, MinLenPosterior& v, F&& f) {
    dec_front_arrays(tr, v, (size_t) tr.N, f);
    f(v.d_post, (size_t) tr.N * 32); f(v.d_label, (size_t) tr.N); f(v.d_chunk, (size_t) tr.C * 16);
}

// hf_minlen_posterior and hf_minlen_posterior_joined (hf_minlen_post_joined.h, below): one front, the rows, then
// `walks(track, decoder, forward lanes)` launches the entry point's two walks; `refuse`: what it refuses beyond the family's front
template <class Refuse, class Walks>
static int mlp_run(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], hipStream_t st, const std::string& w, Refuse&& refuse,
                   Walks&& walks) {
    int64_t lanes = 0;
    const double* nbE = nullptr;
    int rc = minlen_front(ctx, &hf_ctx::mlp, p, min_len, st, w, refuse, [&](const Track& tr, MinLenPosterior& v) {
        const size_t f_bytes = (size_t) tr.N * (size_t) lanes * 8;
        int rc = mem_refuse(w, "the forward lanes", f_bytes, v.fwd.cap, "n_windows x sum of the lengths x 8");
        if (rc || (rc = dec_alloc(tr, v, [&](auto&& f) { mlp_arrays(tr, v, f); }))) return rc;
        return v.fwd.reserve(f_bytes, w);
    }, lanes, nbE);
    if (rc) return rc;
    const Track& tr = ctx->tr;
    MinLenPosterior& v = ctx->mlp;
    if ((rc = dec_clear_outputs(tr, v, 2, st))) return rc;
    if (dec_work(tr)) {
        dec_launch_rows_win(tr, v, nbE, st);
        if ((rc = walks(tr, v, reinterpret_cast<double*>(v.fwd.d_buf)))) return rc;
    }
    HIPCHK(hipGetLastError());
    v.launched = true;
    return HF_OK;
}

int hf_minlen_posterior(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], void* stream) {
    hipStream_t st = (hipStream_t) stream;
    return mlp_run(ctx, p, min_len, st, "hf_minlen_posterior", [] { return (int) HF_OK; }, [&](const Track& tr, MinLenPosterior& v, double* d_F) {
        hipLaunchKernelGGL(k_mlp_fwd, dim3((unsigned) tr.C, 2), dim3(64), 0, st, (int) tr.C, tr.d_off, tr.d_rec, v.d_params, v.d_rows,
                           (int) min_len[0], (int) min_len[1], (int) min_len[2], (int) min_len[3], d_F, v.d_chunk, v.d_flags);
        hipLaunchKernelGGL(k_mlp_bwd, dim3((unsigned) tr.C), dim3(64), 0, st, tr.d_off, tr.d_rec, v.d_params, v.d_rows, (int) min_len[0],
                           (int) min_len[1], (int) min_len[2], (int) min_len[3], d_F, v.d_post, v.d_label, v.d_flags);
        return (int) HF_OK;
    });
}

int hf_minlen_posterior_finish(hf_ctx* ctx, double* log_mass_total_host, void* stream) {
    if (!ctx || !ctx->mlp.launched) return set_err(HF_E_ARG, "hf_minlen_posterior_finish: no hf_minlen_posterior to finish");
    const Track& tr = ctx->tr;
    const int rc = dec_finish_chunks(tr, ctx->mlp, 2, stream);
    if (rc) return rc;
    const std::vector<double>& z = ctx->mlp.h_chunk;
    double tot = 0.0;
    for (int64_t c = 0; c < tr.C; c++) tot += z[(size_t) c] - z[(size_t) (tr.C + c)];   // chunk-list order
    if (log_mass_total_host) *log_mass_total_host = tot;
    return HF_OK;
}

int hf_get_minlen_posterior(hf_ctx* ctx, int64_t first, int64_t n, double* post_host) {
    return minlen_get_range(ctx, "hf_get_minlen_posterior", "hf_minlen_posterior", ctx && ctx->mlp.done, ctx ? ctx->mlp.d_post : nullptr, 4,
                            first, n, post_host);
}

int hf_get_minlen_posterior_labels(hf_ctx* ctx, int8_t* labels_host) {
    if (!ctx || !labels_host || !ctx->mlp.done) return set_err(HF_E_ARG, "hf_get_minlen_posterior_labels: no finished hf_minlen_posterior");
    return dec_labels(ctx->tr, ctx->mlp, labels_host);
}

int hf_get_minlen_chunk_log_mass(hf_ctx* ctx, double* log_mass_host, double* log_z_adm_host) {
    if (!ctx || !log_mass_host || !ctx->mlp.done) return set_err(HF_E_ARG, "hf_get_minlen_chunk_log_mass: no finished hf_minlen_posterior");
    const Track& tr = ctx->tr;
    const std::vector<double>& z = ctx->mlp.h_chunk;
    for (int64_t c = 0; c < tr.C; c++) log_mass_host[c] = z[(size_t) c] - z[(size_t) (tr.C + c)];
    return log_z_adm_host ? dec_chunk_values(tr, ctx->mlp, log_z_adm_host) : HF_OK;
}


// ------------------------------------------------------------------------------------------
// admissible path sampling (hf_minlen_sample.h): whole paths drawn from the posterior under minimum run lengths, a decoder of its own
// beside the three before it, one code path for both kinds of context.
// ------------------------------------------------------------------------------------------
#include "hf_minlen_sample.h"

static size_t mls_pad(size_t k) { return (k + HF_MLS_GROUP - 1) / HF_MLS_GROUP * HF_MLS_GROUP; }

// every device array of the fixed part but the forward lanes (MinLenSampler::fwd), and the per-sample part for k samples: the ONE place
// that sizes them (dec_take allocates them, hf_minlen_sample_capacity counts them)
template <class S, class F> static void mls_arrays(const Track& tr, S& v, F&& f) {
    dec_front_arrays(tr, v, (size_t) tr.N, f);
    f(v.d_chunk, (size_t) tr.C * 8);
}
template <class S, class F> static void mls_sample_arrays(const Track& tr, S& v, size_t k, F&& f) {
    const size_t kp = mls_pad(k);
    f(v.d_keys, k * 8); f(v.d_words, (size_t) tr.N * kp * 2); f(v.d_final, (size_t) tr.C * kp); f(v.d_label, k * (size_t) tr.N);
}
static double mls_sample_bytes(const Track& tr, const MinLenSampler& v, size_t k) {
    double b = 0.0;
    mls_sample_arrays(tr, v, k, [&](auto&, size_t bytes) { b += (double) Slab::granule(bytes); });
    return b;
}

// samples per call at `lanes` lanes: the fixed part and the forward lanes come off nine tenths of the free device memory first; what the
// sampler holds already counts as free
static int mls_capacity(const hf_ctx* ctx, int64_t lanes, const std::string& w) {
    const Track& tr = ctx->tr; const MinLenSampler& v = ctx->mls;
    HIPCHK(hipSetDevice(tr.device));
    double fixed = 0.0, avail = 0.0;
    mls_arrays(tr, v, [&](auto&, size_t bytes) { fixed += (double) Slab::granule(bytes); });
    const double f_bytes = (double) tr.N * (double) lanes * 8.0;
    const int rc = mem_avail((v.alloc ? fixed : 0.0) + (double) v.fwd.cap + (v.cap ? (double) v.samples.first : 0.0), &avail);   // (Slab::release keeps `first`)
    if (rc) return rc;
    const double budget = 0.9 * avail - fixed - f_bytes;
    if (budget < mls_sample_bytes(tr, v, 1)) {
        set_err(HF_E_ARG, w + ": the rows, the forward lanes (" + std::to_string((size_t) f_bytes) + " bytes) and one sample do not fit nine tenths of the free device memory");
        return 0;
    }
    int lo = 1, hi = HF_SMP_MAX_PER_CALL;               // the largest k whose arrays fit
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (mls_sample_bytes(tr, v, (size_t) mid) <= budget) lo = mid; else hi = mid - 1;
    }
    return lo;
}

int hf_minlen_sample_capacity(const hf_ctx* ctx, const int32_t min_len[4]) {
    const std::string w = "hf_minlen_sample_capacity";
    if (!ctx || !min_len) return set_err(HF_E_ARG, w + ": bad argument");
    int64_t lanes = 0;
    const int rc = minlen_check(w, min_len, &lanes);
    return rc ? rc : mls_capacity(ctx, lanes, w);
}

// hf_sample_paths_minlen and hf_sample_paths_minlen_joined (hf_minlen_post_joined.h, below): one front, the rows, then
// `walks(track, sampler, forward lanes, K, Kp)` launches the entry point's kernels; `refuse`: what it refuses beyond the common checks
template <class Refuse, class Walks>
static int mls_run(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], int64_t first_sample, int n_samples, uint64_t seed,
                   hipStream_t st, const std::string& w, Refuse&& refuse, Walks&& walks) {
    int64_t lanes = 0;
    const double* nbE = nullptr;
    int rc = minlen_front(ctx, &hf_ctx::mls, p, min_len, st, w, [&] {
        if (n_samples < 1) return set_err(HF_E_ARG, w + ": n_samples must be >= 1");
        if (first_sample < 0) return set_err(HF_E_ARG, w + ": first_sample must be >= 0");
        return (int) refuse();
    }, [&](const Track& tr, MinLenSampler& v) {
        const size_t f_bytes = (size_t) tr.N * (size_t) lanes * 8;
        if (n_samples > v.cap || f_bytes > v.fwd.cap) {
            const int cap = mls_capacity(ctx, lanes, w);
            if (cap < 0) return cap;
            if (n_samples > cap) return set_err(HF_E_ARG, w + ": n_samples exceeds hf_minlen_sample_capacity (" + std::to_string(cap) + ")");
        }
        int rc = dec_alloc(tr, v, [&](auto&& f) { mls_arrays(tr, v, f); });
        if (rc || (rc = v.fwd.reserve(f_bytes, w))) return rc;
        rc = smp_grow(v, n_samples, [&](auto&& f) { mls_sample_arrays(tr, v, (size_t) n_samples, f); });
        return rc ? rc : smp_keys(v, first_sample, n_samples, seed);
    }, lanes, nbE);
    if (rc) return rc;
    const Track& tr = ctx->tr;
    MinLenSampler& v = ctx->mls;
    if (!all_in_chunks(tr)) HIPCHK(hipMemsetAsync(v.d_label, 0xff, (size_t) n_samples * (size_t) tr.N, st));   // (windows outside every chunk: label -1)
    if (dec_work(tr)) {
        dec_launch_rows_win(tr, v, nbE, st);
        if ((rc = walks(tr, v, reinterpret_cast<double*>(v.fwd.d_buf), n_samples, (int) mls_pad((size_t) n_samples)))) return rc;
    }
    HIPCHK(hipGetLastError());
    v.n = n_samples;
    v.launched = true;
    return HF_OK;
}

int hf_sample_paths_minlen(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], int64_t first_sample, int n_samples, uint64_t seed,
                           void* stream) {
    hipStream_t st = (hipStream_t) stream;
    return mls_run(ctx, p, min_len, first_sample, n_samples, seed, st, "hf_sample_paths_minlen", [] { return (int) HF_OK; },
                   [&](const Track& tr, MinLenSampler& v, double* d_F, int K, int Kp) {
        const int l0 = (int) min_len[0], l1 = (int) min_len[1], l2 = (int) min_len[2], l3 = (int) min_len[3];
        const unsigned NB = (unsigned) ((tr.N + 255) / 256);
        hipLaunchKernelGGL(k_mlp_fwd, dim3((unsigned) tr.C, 1), dim3(64), 0, st, (int) tr.C, tr.d_off, tr.d_rec, v.d_params, v.d_rows, l0, l1,
                           l2, l3, d_F, v.d_chunk, v.d_flags);
        hipLaunchKernelGGL(k_mls_draw, dim3(NB), dim3(256), 0, st, tr.N, tr.d_rec, v.d_rows, l0, l1, l2, l3, d_F, v.d_keys, K, Kp, v.d_words);
        hipLaunchKernelGGL(k_mls_final, dim3((unsigned) tr.C), dim3(64), 0, st, tr.N, tr.d_off, tr.d_rec, v.d_params, l0, l1, l2, l3, d_F,
                           v.d_keys, K, Kp, v.d_final);
        hipLaunchKernelGGL(k_mls_back, dim3((unsigned) tr.C, (unsigned) (Kp / HF_MLS_GROUP)), dim3(64), 0, st, tr.N, tr.d_off, l0, l1, l2, l3,
                           v.d_words, v.d_final, K, Kp, v.d_label);
        return (int) HF_OK;
    });
}

int hf_sample_minlen_finish(hf_ctx* ctx, void* stream) {
    if (!ctx || !ctx->mls.launched) return set_err(HF_E_ARG, "hf_sample_minlen_finish: no hf_sample_paths_minlen to finish");
    return smp_finish(ctx->tr, ctx->mls, stream);
}

int hf_get_minlen_sample_labels(hf_ctx* ctx, int k, int8_t* labels_host) {
    if (!ctx || !labels_host || !ctx->mls.done) return set_err(HF_E_ARG, "hf_get_minlen_sample_labels: no finished hf_sample_paths_minlen");
    return smp_labels(ctx->tr, ctx->mls, "hf_get_minlen_sample_labels", k, labels_host);
}


// k_mea_rows, the one kernel of hf_get_mea_labels (its host side stands behind mlg_cut below), in its place of the family's order
#include "hf_mea.h"


// ------------------------------------------------------------------------------------------
// the posterior and the sampler over groups of joined chunks (hf_minlen_post_joined.h): hf_minlen_posterior_joined shares ctx->mlp, its
// finish and its getters with hf_minlen_posterior (mlp_run above), hf_sample_paths_minlen_joined shares ctx->mls with
// hf_sample_paths_minlen (mls_run above).  The kernels are second bodies launched over the group-as-chunk offsets.
// ------------------------------------------------------------------------------------------
#include "hf_minlen_post_joined.h"

// The groups of a call as a chunk list, hf_viterbi_minlen_joined's rule (a chunk continues its predecessor when it is joined to it and
// both have windows): h[0 .. C] the offsets in which a group's first chunk holds the group's window range and its other chunks none,
// h[C + 1 ..] the joined chunk-first windows.  Uploaded to `grp` on `st`; returns the number of those windows in *nb.
static int mlg_cut(const Track& tr, const uint8_t* joined, DevBuf& grp, std::vector<int64_t>& h, hipStream_t st, const std::string& w, int* nb) {
    const std::vector<int64_t>& off = tr.h_off;
    const size_t C = (size_t) tr.C;
    auto cont = [&](size_t c) { return chunk_continues(off.data(), (int64_t) C, joined, (int64_t) c); };
    h.assign(C + 1, 0);
    h[C] = off[C];
    int64_t gend = off[C];
    for (size_t c = C; c-- > 0;) {
        if (!cont(c + 1)) gend = off[c + 1];               // chunk c is the last of its group
        h[c] = cont(c) ? gend : off[c];
    }
    for (size_t c = 1; c < C; c++) if (cont(c)) h.push_back(off[c]);
    *nb = (int) (h.size() - (C + 1));
    const int rc = grp.reserve((2 * C + 1) * 8, w);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(grp.d_buf, h.data(), h.size() * 8, hipMemcpyHostToDevice, st));
    return HF_OK;
}

int hf_minlen_posterior_joined(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], const uint8_t* joined, void* stream) {
    const std::string w = "hf_minlen_posterior_joined";
    hipStream_t st = (hipStream_t) stream;
    return mlp_run(ctx, p, min_len, st, w, [&] { return mlg_refuse(ctx, joined, w); }, [&](const Track& tr, MinLenPosterior& v, double* d_F) {
        int nb = 0;
        const int rc = mlg_cut(tr, joined, v.grp, v.h_grp, st, w, &nb);
        if (rc) return rc;
        const int64_t* d_goff = reinterpret_cast<const int64_t*>(v.grp.d_buf);
        hipLaunchKernelGGL(k_mlpj_fwd, dim3((unsigned) tr.C, 2), dim3(64), 0, st, (int) tr.C, d_goff, tr.d_rec, v.d_params, v.d_rows,
                           (int) min_len[0], (int) min_len[1], (int) min_len[2], (int) min_len[3], d_F, v.d_chunk, v.d_flags);
        hipLaunchKernelGGL(k_mlpj_bwd, dim3((unsigned) tr.C), dim3(64), 0, st, d_goff, tr.d_rec, v.d_params, v.d_rows, (int) min_len[0],
                           (int) min_len[1], (int) min_len[2], (int) min_len[3], d_F, v.d_post, v.d_label, v.d_flags);
        return (int) HF_OK;
    });
}

int hf_sample_paths_minlen_joined(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], const uint8_t* joined, int64_t first_sample,
                                  int n_samples, uint64_t seed, void* stream) {
    const std::string w = "hf_sample_paths_minlen_joined";
    hipStream_t st = (hipStream_t) stream;
    return mls_run(ctx, p, min_len, first_sample, n_samples, seed, st, w, [&] { return mlg_refuse(ctx, joined, w); },
                   [&](const Track& tr, MinLenSampler& v, double* d_F, int K, int Kp) {
        int nb = 0;
        const int rc = mlg_cut(tr, joined, v.grp, v.h_grp, st, w, &nb);
        if (rc) return rc;
        const int64_t* d_goff = reinterpret_cast<const int64_t*>(v.grp.d_buf);
        const int l0 = (int) min_len[0], l1 = (int) min_len[1], l2 = (int) min_len[2], l3 = (int) min_len[3];
        const unsigned NB = (unsigned) ((tr.N + 255) / 256);
        hipLaunchKernelGGL(k_mlpj_fwd, dim3((unsigned) tr.C, 1), dim3(64), 0, st, (int) tr.C, d_goff, tr.d_rec, v.d_params, v.d_rows, l0, l1,
                           l2, l3, d_F, v.d_chunk, v.d_flags);
        hipLaunchKernelGGL(k_mls_draw, dim3(NB), dim3(256), 0, st, tr.N, tr.d_rec, v.d_rows, l0, l1, l2, l3, d_F, v.d_keys, K, Kp, v.d_words);
        if (nb > 0)
            hipLaunchKernelGGL(k_mlsj_bound, dim3((unsigned) nb), dim3(256), 0, st, d_goff + tr.C + 1, tr.d_rec, v.d_params, v.d_rows, l0, l1, l2,
                               l3, d_F, v.d_keys, K, Kp, v.d_words);
        hipLaunchKernelGGL(k_mls_final, dim3((unsigned) tr.C), dim3(64), 0, st, tr.N, d_goff, tr.d_rec, v.d_params, l0, l1, l2, l3, d_F,
                           v.d_keys, K, Kp, v.d_final);
        hipLaunchKernelGGL(k_mls_back, dim3((unsigned) tr.C, (unsigned) (Kp / HF_MLS_GROUP)), dim3(64), 0, st, tr.N, d_goff, l0, l1, l2, l3,
                           v.d_words, v.d_final, K, Kp, v.d_label);
        return (int) HF_OK;
    });
}


// ------------------------------------------------------------------------------------------
// maximum-expected-accuracy decoding under minimum run lengths (hf_mea.h): a getter of the last full pass, synchronous on the pass's
// stream as the range getters are.  k_mea_rows turns the pass's posterior into gain rows; k_mlv_fwd and k_mlv_back walk them as they
// are, over the chunk offsets or mlg_cut's group-as-chunk offsets, with the getter's unit-end parameter block.  Buffers of its own
// (ctx->mea): the last pass, every decoder's and sampler's results and the next hf_estep stay as they are.
// ------------------------------------------------------------------------------------------
// every device array of the getter, f(array, bytes) in turn (as mlv_arrays)
template <class F> static void mea_arrays(const Track& tr, MeaDecoder& m, F&& f) {
    f(m.d_rows, (size_t) tr.N * 128); f(m.d_bp, (size_t) tr.N * 2); f(m.d_label, (size_t) tr.N); f(m.d_score, (size_t) tr.C * 8);
    f(m.d_final, (size_t) tr.C); f(m.d_params, tr.params_bytes); f(m.d_flags, 4);
}

int hf_get_mea_labels(hf_ctx* ctx, const double* gain, const int32_t min_len[4], const uint8_t* joined, int8_t* labels_host,
                      double* block_gain_host, double* total_gain_host) {
    const std::string who = "hf_get_mea_labels";
    if (!ctx || !min_len) return set_err(HF_E_ARG, who + ": bad argument");
    if (!labels_host) return set_err(HF_E_ARG, who + ": NULL label array");
    int64_t lanes = 0;
    int rc = minlen_check(who, min_len, &lanes);
    if (rc || (rc = mlg_refuse(ctx, joined, who))) return rc;
    MeaGain W;
    for (int o = 0; o < 16; o++) {
        W.w[o] = gain ? gain[o] : ((o >> 2) == (o & 3) ? 1.0 : 0.0);
        if (!(std::fabs(W.w[o]) <= 1e100)) return set_err(HF_E_ARG, who + ": every gain must be finite and at most 1e100 in magnitude");
    }
    if (!ctx->pass.have_full)
        return set_err(HF_E_ARG, who + ": no HF_MODE_FULL pass to answer for (none yet, or the last pass was forward-only)");
    const Track& tr = ctx->tr;
    MeaDecoder& m = ctx->mea;
    PassView pv;
    rc = pass_view(ctx, who, dec_work(tr) ? 1 : 0, pv);
    if (rc) return rc;
    hipStream_t st = ctx->pass.last_stream;
    if (block_gain_host) for (int64_t c = 0; c < tr.C; c++) block_gain_host[c] = 0.0;
    if (total_gain_host) *total_gain_host = 0.0;
    if (!dec_work(tr)) {
        if (tr.N > 0) std::memset(labels_host, 0xff, (size_t) tr.N);
        return HF_OK;
    }
    if (!m.alloc) {
        if (dec_take(m.slab, [&](auto&& f) { mea_arrays(tr, m, f); })) { m.slab.release(); return set_err(HF_E_HIP, who + ": out of device memory"); }
        // the unit-end parameter block: all zero but trans[s][4] = 1.0 of every region (k_mlv_fwd reads nothing else of it)
        std::vector<double> img(tr.params_bytes / 8, 0.0);
        DevParams* hp = reinterpret_cast<DevParams*>(img.data());
        hp->n_regions = tr.R;
        for (int r = 0; r < tr.R; r++)
            for (int s = 0; s < 4; s++) hp->reg[r].trans[s][4] = 1.0;
        HIPCHK(hipMemcpy(m.d_params, img.data(), tr.params_bytes, hipMemcpyHostToDevice));
        m.alloc = true;
    }
    HIPCHK(hipMemsetAsync(m.d_flags, 0, 4, st));
    if (!all_in_chunks(tr)) HIPCHK(hipMemsetAsync(m.d_label, 0xff, (size_t) tr.N, st));   // (windows outside every chunk: label -1)
    const int64_t* d_boff = tr.d_off;                   // the window ranges of the walks' blocks: chunks, or groups as chunks
    if (joined) {
        int nb = 0;
        if ((rc = mlg_cut(tr, joined, m.grp, m.h_grp, st, who, &nb))) return rc;
        d_boff = reinterpret_cast<const int64_t*>(m.grp.d_buf);
    }
    const int l0 = (int) min_len[0], l1 = (int) min_len[1], l2 = (int) min_len[2], l3 = (int) min_len[3];
    by_algo(tr, [&](auto S) {
        constexpr bool SEQ = decltype(S)::value;
        hipLaunchKernelGGL(k_mea_rows<SEQ>, dim3((unsigned) ((tr.N + 255) / 256)), dim3(256), 0, st, tr.N, (int) tr.C, tr.d_off, pv, W, m.d_rows,
                           m.d_flags);
    });
    hipLaunchKernelGGL(k_mlv_fwd, dim3((unsigned) tr.C), dim3(64), 0, st, d_boff, tr.d_rec, m.d_params, m.d_rows, l0, l1, l2, l3, m.d_bp, m.d_final,
                       m.d_score, m.d_flags);
    hipLaunchKernelGGL(k_mlv_back, dim3((unsigned) tr.C), dim3(64), 0, st, d_boff, l0, l1, l2, l3, m.d_bp, m.d_final, m.d_label);
    HIPCHK(hipGetLastError());
    unsigned fl = 0;
    std::vector<double> score((size_t) tr.C);
    HIPCHK(hipMemcpyAsync(&fl, m.d_flags, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(score.data(), m.d_score, (size_t) tr.C * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(labels_host, m.d_label, (size_t) tr.N, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (fl & HF_FLAG_NAN) return set_err(HF_E_NAN, who + ": a NaN in a gain row");
    if (fl & HF_FLAG_SCALE) return set_err(HF_E_SCALE, who + ": a block has no admissible supported labelling");
    double tot = 0.0;
    for (int64_t c = 0; c < tr.C; c++) tot += score[(size_t) c];          // chunk-list order
    if (block_gain_host) std::memcpy(block_gain_host, score.data(), (size_t) tr.C * 8);
    if (total_gain_host) *total_gain_host = tot;
    return HF_OK;
}


// ------------------------------------------------------------------------------------------
// the E-step under minimum run lengths (hf_minlen_em.h): the expected sufficient statistics under the posterior over admissible paths,
// in hf_finish's layout.  The family's front (minlen_front) on a decoder of its own, k_tables into a pass state of its own, k_mlp_fwd as
// it is, k_mle_bwd, k_mle_tile, then k_chunk_stats and k_reduce as they are (the pass's kernels: through hf_estep.hip's launchers).  One
// code path for both kinds of context.
// ------------------------------------------------------------------------------------------
#include "hf_minlen_em.h"

template <class F> static void mle_arrays(const Track& tr, MinLenEM& v, F&& f) {
    dec_front_arrays(tr, v, (size_t) tr.N, f);
    f(v.d_chunk, (size_t) tr.C * 16); f(v.d_ll0, ((size_t) tr.C + 1) * 4);
}

template <int KT>
static int mle_launch_tile(const Track& tr, MinLenEM& v, hipStream_t st, int ncol) {
    Pass& ps = v.pass;
    const TileGeom g = tile_geom(tr, k_mle_tile<KT>, (size_t) (3 * ncol > 28 ? 3 * ncol : 28) * 65 * 8, false);
    if (!g.ok) return set_err(HF_E_ARG, "hf_estep_minlen: the accumulators of one wavefront do not fit the LDS of one workgroup");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mle_tile<KT>), dim3(g.blocks), dim3(g.threads), g.lds, st, tr.ntiles, tr.d_tile_desc, tr.d_rec,
                       row_src(ps), ps.d_params, v.d_xi, tr.d_regmask, ps.d_tile_stats);
    return HF_OK;
}

// hf_estep_minlen and hf_estep_minlen_joined (hf_minlen_em_joined.h, below): one front, this call's tables, the rows, then
// `walks(track, decoder, forward lanes)` launches the entry point's two walks; everything behind them (k_mle_tile, k_chunk_stats,
// k_reduce) is shared; `refuse`: what the entry point refuses beyond the negative_binomial model and the family's front
template <class Refuse, class Walks>
static int mle_run(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], hipStream_t st, const std::string& w, Refuse&& refuse,
                   Walks&& walks) {
    int64_t lanes = 0;
    const double* nbE = nullptr;
    int rc = minlen_front(ctx, &hf_ctx::mle, p, min_len, st, w, [&] {
        if (p->model_type == HF_MODEL_NEGATIVE_BINOMIAL)
            return set_err(HF_E_ARG, w + ": the negative_binomial model is not supported (its statistics are another path)");
        return (int) refuse();
    }, [&](const Track& tr, MinLenEM& v) {
        const size_t f_bytes = Slab::granule((size_t) tr.N * (size_t) lanes * 8), bytes = f_bytes + (size_t) tr.N * 128;
        int rc = mem_refuse(w, "the forward lanes and xi_adm", bytes, v.fwd.cap, "n_windows x (sum of the lengths x 8 + 128)");
        if (rc) return rc;
        const bool first = !v.alloc;
        if ((rc = dec_alloc(tr, v, [&](auto&& f) { mle_arrays(tr, v, f); }))) return rc;
        if (first) {   // one slot per chunk: k_chunk_stats' element 0 is the chunk's log Z_adm
            std::vector<int32_t> ll0((size_t) tr.C + 1);
            for (size_t c = 0; c < ll0.size(); c++) ll0[c] = (int32_t) c;
            HIPCHK(hipMemcpy(v.d_ll0, ll0.data(), ll0.size() * 4, hipMemcpyHostToDevice));
        }
        if (!v.pass_made) {
            v.pass_made = true;
            if ((rc = pass_create(tr, ctx->pass, &v.pass))) { v.drop_pass(); return rc; }
            HIPCHK(hipDeviceSynchronize());   // (pass_create clears its arrays on the null stream; `st` may not wait for that one)
        }
        if ((rc = v.fwd.reserve(bytes, w))) return rc;
        v.d_xi = reinterpret_cast<double*>(v.fwd.d_buf + f_bytes);
        return (int) HF_OK;
    }, lanes, nbE);
    if (rc) return rc;
    const Track& tr = ctx->tr;
    MinLenEM& v = ctx->mle;
    Pass& ps = v.pass;
    if (tr.C > 0) HIPCHK(hipMemsetAsync(v.d_chunk, 0, (size_t) tr.C * 16, st));
    if (tr.C > 0) {
        double* d_F = reinterpret_cast<double*>(v.fwd.d_buf);
        HIPCHK(hipMemcpyAsync(ps.d_params, v.h_params, tr.params_bytes, hipMemcpyHostToDevice, st));
        launch_tables(ps, v.d_flags, false, st);   // this call's tables; the kernel clears the flag word it is given, as dec_front has done
        if (dec_work(tr)) {
            dec_launch_rows_win(tr, v, nbE, st);
            if ((rc = walks(tr, v, d_F))) return rc;
        }
        const int kc = p->ncomp[3];
        if (tr.ntiles > 0) {
            rc = kc <= 4 ? mle_launch_tile<4>(tr, v, st, kc) : kc <= 8 ? mle_launch_tile<8>(tr, v, st, kc) : mle_launch_tile<16>(tr, v, st, kc);
            if (rc) return rc;
        }
        launch_chunk_stats(tr, st, kc, v.d_ll0, ps.d_tile_stats, v.d_chunk, ps.d_params, ps.d_chunk_stats_own, tr.ntiles > 0 ? 1 : 0);
        launch_reduce(tr, st, ps.d_chunk_stats_own, nullptr, tr.C, ps.d_total, v.d_flags);
    }
    HIPCHK(hipGetLastError());
    v.launched = true;
    return HF_OK;
}

int hf_estep_minlen(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], void* stream) {
    hipStream_t st = (hipStream_t) stream;
    return mle_run(ctx, p, min_len, st, "hf_estep_minlen", [] { return (int) HF_OK; }, [&](const Track& tr, MinLenEM& v, double* d_F) {
        const int l0 = (int) min_len[0], l1 = (int) min_len[1], l2 = (int) min_len[2], l3 = (int) min_len[3];
        hipLaunchKernelGGL(k_mlp_fwd, dim3((unsigned) tr.C, 2), dim3(64), 0, st, (int) tr.C, tr.d_off, tr.d_rec, v.d_params, v.d_rows, l0, l1, l2, l3,
                           d_F, v.d_chunk, v.d_flags);
        hipLaunchKernelGGL(k_mle_bwd, dim3((unsigned) tr.C), dim3(64), 0, st, tr.d_off, tr.d_rec, v.d_params, v.d_rows, l0, l1, l2, l3, d_F, v.d_xi,
                           v.d_flags);
        return (int) HF_OK;
    });
}

int hf_estep_minlen_finish(hf_ctx* ctx, double* stats_host, double* log_z_host, void* stream) {
    if (!ctx || !stats_host || !ctx->mle.launched) return set_err(HF_E_ARG, "hf_estep_minlen_finish: no hf_estep_minlen to finish");
    const Track& tr = ctx->tr;
    MinLenEM& v = ctx->mle;
    const int rc = dec_finish(tr, v, stream);
    if (rc) return rc;
    v.h_total.assign((size_t) tr.V, 0.0);
    v.h_chunk.assign((size_t) tr.C * 2, 0.0);
    if (tr.C > 0) {
        HIPCHK(hipMemcpy(v.h_total.data(), v.pass.d_total, (size_t) tr.V * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(v.h_chunk.data(), v.d_chunk, (size_t) tr.C * 16, hipMemcpyDeviceToHost));
    }
    std::memcpy(stats_host, v.h_total.data(), (size_t) tr.V * 8);
    if (log_z_host) {
        double z = 0.0;
        for (int64_t c = 0; c < tr.C; c++) z += v.h_chunk[(size_t) (tr.C + c)];   // chunk-list order
        *log_z_host = z;
    }
    v.done = true;
    return HF_OK;
}

int hf_get_minlen_pair_posterior(hf_ctx* ctx, int64_t first, int64_t n, double* xi_host) {
    return minlen_get_range(ctx, "hf_get_minlen_pair_posterior", "hf_estep_minlen", ctx && ctx->mle.done, ctx ? ctx->mle.d_xi : nullptr, 16,
                            first, n, xi_host);
}

int hf_get_minlen_em_chunk_stats(hf_ctx* ctx, double* chunk_stats_host, double* log_z_adm_host, double* log_z_host) {
    const std::string w = "hf_get_minlen_em_chunk_stats";
    if (!ctx || !ctx->mle.done) return set_err(HF_E_ARG, w + ": no finished hf_estep_minlen");
    const Track& tr = ctx->tr;
    const MinLenEM& v = ctx->mle;
    HIPCHK(hipSetDevice(tr.device));
    if (chunk_stats_host && tr.C > 0)
        HIPCHK(hipMemcpy(chunk_stats_host, v.pass.d_chunk_stats_own, (size_t) tr.C * (size_t) tr.V * 8, hipMemcpyDeviceToHost));
    if (log_z_adm_host && tr.C > 0) std::memcpy(log_z_adm_host, v.h_chunk.data(), (size_t) tr.C * 8);
    if (log_z_host && tr.C > 0) std::memcpy(log_z_host, v.h_chunk.data() + tr.C, (size_t) tr.C * 8);
    return HF_OK;
}

// hf_em_iterate with the constrained E-step: the model's log-likelihood becomes element 0, the sum of log Z_adm
int hf_em_iterate_minlen(hf_ctx* ctx, hfm_model* model, const int32_t min_len[4], int do_mstep, double tol, double* stats_host,
                         double* log_z_host, int* converged, void* stream) {
    if (!ctx || !model || !min_len || !stats_host) return set_err(HF_E_ARG, "hf_em_iterate_minlen: bad argument");
    hf_params p;
    hfm_params(model, &p);
    int rc = hf_estep_minlen(ctx, &p, min_len, stream);
    if (rc == HF_OK) rc = hf_estep_minlen_finish(ctx, stats_host, log_z_host, stream);
    if (rc != HF_OK) return rc;
    em_step_tail(model, stats_host, do_mstep != 0, tol, converged);
    return HF_OK;
}


// ------------------------------------------------------------------------------------------
// the E-step over groups of joined chunks (hf_minlen_em_joined.h): hf_estep_minlen_joined shares ctx->mle, its finish and its getters
// with hf_estep_minlen (mle_run above).  k_mlpj_fwd as it is and k_mlej_bwd, a second body of k_mle_bwd, over mlg_cut's group-as-chunk
// offsets; the statistics run over the track's own tile plan as before, so a group's log Z_adm and log Z sit in its first chunk's
// entries (and its element 0) and its other chunks hold 0.0 there.
// ------------------------------------------------------------------------------------------
#include "hf_minlen_em_joined.h"

int hf_estep_minlen_joined(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], const uint8_t* joined, void* stream) {
    const std::string w = "hf_estep_minlen_joined";
    hipStream_t st = (hipStream_t) stream;
    return mle_run(ctx, p, min_len, st, w, [&] { return mlg_refuse(ctx, joined, w); }, [&](const Track& tr, MinLenEM& v, double* d_F) {
        int nb = 0;
        const int rc = mlg_cut(tr, joined, v.grp, v.h_grp, st, w, &nb);
        if (rc) return rc;
        const int64_t* d_goff = reinterpret_cast<const int64_t*>(v.grp.d_buf);
        const int l0 = (int) min_len[0], l1 = (int) min_len[1], l2 = (int) min_len[2], l3 = (int) min_len[3];
        hipLaunchKernelGGL(k_mlpj_fwd, dim3((unsigned) tr.C, 2), dim3(64), 0, st, (int) tr.C, d_goff, tr.d_rec, v.d_params, v.d_rows, l0, l1, l2, l3,
                           d_F, v.d_chunk, v.d_flags);
        hipLaunchKernelGGL(k_mlej_bwd, dim3((unsigned) tr.C), dim3(64), 0, st, d_goff, tr.d_rec, v.d_params, v.d_rows, l0, l1, l2, l3, d_F, v.d_xi,
                           v.d_flags);
        return (int) HF_OK;
    });
}

// hf_em_iterate_minlen with the E-step over groups of joined chunks: element 0 is the sum over groups of log Z_adm
int hf_em_iterate_minlen_joined(hf_ctx* ctx, hfm_model* model, const int32_t min_len[4], const uint8_t* joined, int do_mstep, double tol,
                                double* stats_host, double* log_z_host, int* converged, void* stream) {
    if (!ctx || !model || !min_len || !stats_host) return set_err(HF_E_ARG, "hf_em_iterate_minlen_joined: bad argument");
    hf_params p;
    hfm_params(model, &p);
    int rc = hf_estep_minlen_joined(ctx, &p, min_len, joined, stream);
    if (rc == HF_OK) rc = hf_estep_minlen_finish(ctx, stats_host, log_z_host, stream);
    if (rc != HF_OK) return rc;
    em_step_tail(model, stats_host, do_mstep != 0, tol, converged);
    return HF_OK;
}


// k_mlvj_fwd, the forward walk of hf_viterbi_minlen_joined (mlv_run above launches it).  Last of the unit's kernel headers:
// hf_minlen_joined.h says why.
#include "hf_minlen_joined.h"
