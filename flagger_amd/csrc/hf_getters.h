// hf_getters.h — the range getters of the C ABI (include/hmm_flagger_hip.h), host side and kernels: values over window ranges under the
// model of the last full pass (hf_interval.h, hf_moments.h, hf_runs.h, hf_entropy.h, hf_breakpoint.h, hf_longrun.h) and the alpha
// statistics (hf_alpha.h).  Nothing of them runs inside a pass: they read what the pass left (on the scan path after the lazy re-run of
// the segment kernel, pass_all_records) and write buffers of their own.  hf_minlen.hip's hf_get_mea_labels takes its view of the pass
// from pass_view below.
// INCLUDED AT THE END OF hf_estep.hip, as hf_batch.h is, not a unit of its own: compiled without the pass kernels in the same module,
// k_alpha_pairs<*> and k_ent_piece<*> come out with other instructions around their __shfl_down (DESIGN.md 7k-m has the measurement).
//
// THE SCAFFOLD of every range getter, here and in hf_runlen.hip and hf_countdist.hip: rg_check refuses what every one of them refuses,
// pass_view says where the pass left its rows, f and b (hf_view.h), and hf_rg.h takes the jobs through the device batch by batch: the
// piece / chain getters (interval, count moments, run moments, entropy and labelling log-probability) through its rg_run, keeping their
// record builders, scratch sizes, two launches and fold; the breakpoint and long-run getters with a body of their own for rg_batches.
#pragma once
#include "hf_rg.h"
#include "hf_view.h"
#include "hf_interval.h"
#include "hf_moments.h"
#include "hf_runs.h"
#include "hf_entropy.h"

// (the caps of a device batch, HF_IV_BATCH_*, HF_MO_BATCH_*, HF_BP_BATCH_*: hf_estep.hip, in front of this file's include)
static_assert(HF_IV_PIECE == 512 && HF_MO_PIECE == 512 && HF_RN_PIECE == 512 && HF_EN_PIECE == 512, "one piece grid for every getter");

// What every range getter refuses, in this order: n < 0, `early` (a refusal of the getter's own that ranks here, or nullptr), NULL arrays,
// no full pass, `late` (the same), and job by job a bad range, a window outside every chunk, a state mask outside 1..15 (state_mask ==
// nullptr: the getter has none) and a region outside -1..n_regions-1 (region == nullptr: no filter).
// (declared in hf_host.h, with the defaults region = early = late = nullptr: the getters of hf_runlen.hip and hf_countdist.hip call it too)
int rg_check(const hf_ctx* ctx, const std::string& who, int64_t n, bool null_array, const int64_t* first, const int64_t* last,
             const uint8_t* state_mask, const int32_t* region, const char* early, const char* late) {
    const Track& tr = ctx->tr;
    if (n < 0) return set_err(HF_E_ARG, who + ": n < 0");
    if (early) return set_err(HF_E_ARG, who + ": " + early);
    if (n > 0 && null_array) return set_err(HF_E_ARG, who + ": NULL array");
    if (!ctx->pass.have_full)
        return set_err(HF_E_ARG, who + ": no HF_MODE_FULL pass to answer for (none yet, or the last pass was forward-only)");
    if (late) return set_err(HF_E_ARG, who + ": " + late);
    for (int64_t i = 0; i < n; i++) {
        if (first[i] < 0 || first[i] > last[i] || last[i] >= tr.N) return set_err(HF_E_ARG, who + ": bad range (job " + std::to_string(i) + ")");
        if (!in_chunks(tr, first[i], last[i])) return set_err(HF_E_ARG, who + ": a window outside every chunk (job " + std::to_string(i) + ")");
        if (state_mask && (state_mask[i] < 1 || state_mask[i] > 15))
            return set_err(HF_E_ARG, who + ": state_mask must be 1..15 (job " + std::to_string(i) + ")");
        if (region && (region[i] < -1 || region[i] >= tr.R))
            return set_err(HF_E_ARG, who + ": region must be -1..n_regions-1 (job " + std::to_string(i) + ")");
    }
    return HF_OK;
}

// where the last full pass left its rows, f and b (hf_view.h)
static PassView view_of(const hf_ctx* ctx) {
    const Track& tr = ctx->tr;
    const Pass& ps = ctx->pass;
    PassView pv{};
    pv.rec = tr.d_rec;
    if (tr.algo == HF_ALGO_SEQ) { pv.off = tr.d_off; pv.chunk_tile0 = tr.d_chunk_tile0; pv.F = ps.d_f; pv.B = ps.d_b; pv.E = ps.d_E; pv.Pm = ps.d_params; }
    else { pv.pos = tr.d_pos; pv.pos_f = tr.d_pos_f; pv.recs = ps.d_recs_all; pv.arow = tr.d_arow; pv.lutA = ps.d_lutA; }
    return pv;
}

// The state of the pass a getter answers for, after its own checks: the device, and for n > 0 (n == 0: nothing will be read, the getter
// returns) the pair records of the scan path and the view.
int pass_view(hf_ctx* ctx, const std::string& who, int64_t n, PassView& pv) {
    const Track& tr = ctx->tr;
    Pass& ps = ctx->pass;
    HIPCHK(hipSetDevice(tr.device));
    pv = PassView{};
    if (n == 0) return HF_OK;
    const bool seq = tr.algo == HF_ALGO_SEQ;
    if (!seq && (!ps.fb_recs || !tr.d_arow)) return set_err(HF_E_ARG, who + ": the last pass kept no pair records");
    if (!seq) {
        const int rc = pass_all_records(ps);
        if (rc) return rc;
    }
    pv = view_of(ctx);
    return HF_OK;
}

// exact interval probabilities (hf_interval.h): k_iv_piece multiplies the pieces, k_iv_chain every part's vectors through them, a job is
// the sum of its parts
int hf_get_interval_log_probs(hf_ctx* ctx, int64_t n, const int64_t* first, const int64_t* last, const uint8_t* state_mask, double* log_p_host) {
    const std::string who = "hf_get_interval_log_probs";
    if (!ctx) return set_err(HF_E_ARG, who + ": bad argument");
    int rc = rg_check(ctx, who, n, !first || !last || !state_mask || !log_p_host, first, last, state_mask);
    if (rc) return rc;
    PassView pv;
    rc = pass_view(ctx, who, n, pv);
    if (rc || n == 0) return rc;
    hipStream_t st = ctx->pass.last_stream;
    return rg_run<IvPiece, IvPart, HF_IV_PIECE>(ctx, who, ctx->iv, n, first, last, HF_IV_BATCH_PIECES, HF_IV_BATCH_PARTS, 32 * 8, 2 * 4, 1,
        [&](int64_t j, int c, int64_t a, int64_t b) { return IvPart{a, b, 0, 0, state_mask[j], c}; },
        [](const IvPart& pt, int64_t t, int len) { return IvPiece{t, len, pt.mask}; },
        [&](const RgBatch<IvPiece, IvPart>& bt) {
            int* d_pe = reinterpret_cast<int*>(bt.px);
            by_algo(ctx->tr, [&](auto S) {
                constexpr bool SEQ = decltype(S)::value;
                if (bt.np) hipLaunchKernelGGL(k_iv_piece<SEQ>, bt.piece_grid(), dim3(64), 0, st, bt.pieces, pv, bt.pm, d_pe);
                hipLaunchKernelGGL(k_iv_chain<SEQ>, bt.chain_grid(), dim3(64), 0, st, (int) bt.nq, bt.parts, bt.pm, d_pe, pv, bt.out);
            });
        },
        [&](int64_t j, const IvPart*, const double* val, int64_t k0, int64_t k1) {
            double s = 0.0;
            for (int64_t k = k0; k < k1; k++) s += val[k];
            log_p_host[j] = s;
        });
}


// ------------------------------------------------------------------------------------------
// the alpha statistics (hf_alpha.h) of the last full pass: like the interval getter, nothing of it runs inside a pass — hf_set_alpha_stats
// only marks the passes whose statistics may be asked for, and hf_get_alpha_stats computes them from what the pass left (on the scan path
// after the getters' lazy re-run of the segment kernel).
// ------------------------------------------------------------------------------------------
#include "hf_alpha.h"

// the plan: every pair (t-1, t) of every chunk, sorted by region of t, in blocks of one region
static int alpha_plan(hf_ctx* ctx) {
    const Track& tr = ctx->tr;
    AlphaStats& al = ctx->al;
    if (al.planned) return HF_OK;
    std::vector<uint32_t> rec((size_t) tr.N);
    if (tr.N > 0) HIPCHK(hipMemcpy(rec.data(), tr.d_rec, (size_t) tr.N * 4, hipMemcpyDeviceToHost));
    // the order of a region's pairs: HF_ALGO_SCAN by the position of window t's pair record (the plan keeps the records of one row of A
    // together: the record reads of a wavefront are contiguous and its rows few), HF_ALGO_SEQ by t
    std::vector<long long> ord_t; std::vector<int32_t> ord_c;
    ord_t.reserve((size_t) tr.N); ord_c.reserve((size_t) tr.N);
    bool by_pos = tr.algo == HF_ALGO_SCAN && tr.d_pos && tr.n_pos > 0;
    if (by_pos) {
        std::vector<int32_t> pos((size_t) tr.N);
        HIPCHK(hipMemcpy(pos.data(), tr.d_pos, (size_t) tr.N * 4, hipMemcpyDeviceToHost));
        std::vector<int64_t> inv_t((size_t) tr.n_pos, -1); std::vector<int32_t> inv_c((size_t) tr.n_pos, 0);
        for (int c = 0; c < tr.C && by_pos; c++)
            for (int64_t t = tr.h_off[(size_t) c] + 1; t < tr.h_off[(size_t) c + 1]; t++) {
                const int64_t q = pos[(size_t) t];
                if (q < 0 || q >= tr.n_pos || inv_t[(size_t) q] >= 0) { by_pos = false; break; }    // (not a plan this order understands: by t)
                inv_t[(size_t) q] = t; inv_c[(size_t) q] = c;
            }
        if (by_pos)
            for (int64_t q = 0; q < tr.n_pos; q++)
                if (inv_t[(size_t) q] >= 0) { ord_t.push_back(inv_t[(size_t) q]); ord_c.push_back(inv_c[(size_t) q]); }
    }
    if (!by_pos) {
        ord_t.clear(); ord_c.clear();
        for (int c = 0; c < tr.C; c++)
            for (int64_t t = tr.h_off[(size_t) c] + 1; t < tr.h_off[(size_t) c + 1]; t++) { ord_t.push_back(t); ord_c.push_back(c); }
    }
    std::vector<int64_t> cnt((size_t) tr.R + 1, 0);
    for (const long long t : ord_t) {
        const unsigned r = REC_REGION(rec[(size_t) t]);
        if (r < (unsigned) tr.R) cnt[r + 1]++;
    }
    for (int r = 0; r < tr.R; r++) cnt[(size_t) r + 1] += cnt[(size_t) r];
    const int64_t np = cnt[(size_t) tr.R];
    std::vector<long long> pair_t((size_t) np);
    std::vector<int32_t> pair_c((size_t) np);
    {
        std::vector<int64_t> fill(cnt.begin(), cnt.end() - 1);
        for (size_t i = 0; i < ord_t.size(); i++) {      // every region's pairs in that order
            const unsigned r = REC_REGION(rec[(size_t) ord_t[i]]);
            if (r >= (unsigned) tr.R) continue;
            const int64_t k = fill[r]++;
            pair_t[(size_t) k] = ord_t[i]; pair_c[(size_t) k] = ord_c[i];
        }
    }
    std::vector<AlBlock> blocks;
    std::vector<int32_t> rblk0((size_t) tr.R + 1, 0);
    for (int r = 0; r < tr.R; r++) {
        rblk0[(size_t) r] = (int32_t) blocks.size();
        for (int64_t p0 = cnt[(size_t) r]; p0 < cnt[(size_t) r + 1]; p0 += HF_AL_BLOCK)
            blocks.push_back(AlBlock{p0, (int) std::min<int64_t>(HF_AL_BLOCK, cnt[(size_t) r + 1] - p0), r});
    }
    rblk0[(size_t) tr.R] = (int32_t) blocks.size();
    const size_t nb = blocks.size();
    const size_t o_c = Slab::granule((size_t) np * 8), o_b = o_c + Slab::granule((size_t) np * 4), o_r = o_b + Slab::granule(nb * sizeof(AlBlock)),
                 o_p = o_r + Slab::granule(((size_t) tr.R + 1) * 4), o_o = o_p + Slab::granule(nb * 32 * 8), o_t = o_o + Slab::granule((size_t) tr.R * 32 * 8),
                 bytes = o_t + Slab::granule(tr.algo == HF_ALGO_SCAN ? (size_t) tr.tabwork.n_jobs * 32 * 8 : 0);
    al.release();      // (a buffer an earlier, failed attempt left)
    if (hipMalloc((void**) &al.d_buf, bytes) != hipSuccess) { (void) hipGetLastError(); al.d_buf = nullptr;
        return set_err(HF_E_HIP, "hf_get_alpha_stats: out of device memory"); }
    al.d_pair_t = reinterpret_cast<long long*>(al.d_buf); al.d_pair_c = reinterpret_cast<int32_t*>(al.d_buf + o_c);
    al.d_blocks = al.d_buf + o_b; al.d_rblk0 = reinterpret_cast<int32_t*>(al.d_buf + o_r);
    al.d_part = reinterpret_cast<double*>(al.d_buf + o_p); al.d_out = reinterpret_cast<double*>(al.d_buf + o_o);
    al.d_terms = reinterpret_cast<double*>(al.d_buf + o_t);
    if (np) {
        HIPCHK(hipMemcpy(al.d_pair_t, pair_t.data(), (size_t) np * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(al.d_pair_c, pair_c.data(), (size_t) np * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(al.d_blocks, blocks.data(), nb * sizeof(AlBlock), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(al.d_rblk0, rblk0.data(), ((size_t) tr.R + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());      // (the copies ran on the null stream, the kernels will run on the stream of the pass)
    al.n_pairs = np; al.n_blocks = (int) nb; al.planned = true;
    return HF_OK;
}

int hf_set_alpha_stats(hf_ctx* ctx, int on) {
    if (!ctx) return set_err(HF_E_ARG, "hf_set_alpha_stats: bad argument");
    if (on && ctx->pass.d_nbE)
        return set_err(HF_E_ARG, "hf_set_alpha_stats: the context has run negative_binomial passes, whose emission has no alpha");
    ctx->al.on = on != 0;
    if (!on) { ctx->al.pass = false; ctx->al.cached = false; }
    return HF_OK;
}

int64_t hf_alpha_stats_len(const hf_ctx* ctx) { return ctx ? 32 * (int64_t) ctx->tr.R : 0; }

int hf_get_alpha_stats(hf_ctx* ctx, double* out_host) {
    if (!ctx || !out_host) return set_err(HF_E_ARG, "hf_get_alpha_stats: bad argument");
    const Track& tr = ctx->tr;
    Pass& ps = ctx->pass;
    AlphaStats& al = ctx->al;
    if (!ps.have_full)
        return set_err(HF_E_ARG, "hf_get_alpha_stats: no HF_MODE_FULL pass to answer for (none yet, or the last pass was forward-only)");
    if (!al.pass) return set_err(HF_E_ARG, "hf_get_alpha_stats: the last pass ran without hf_set_alpha_stats(ctx, 1)");
    if (ps.last_p.model_type == HF_MODEL_NEGATIVE_BINOMIAL)
        return set_err(HF_E_ARG, "hf_get_alpha_stats: the negative_binomial emission has no alpha");
    const size_t len = (size_t) tr.R * 32;
    if (al.cached) { std::memcpy(out_host, al.last.data(), len * 8); return HF_OK; }
    HIPCHK(hipSetDevice(tr.device));
    const bool seq = tr.algo == HF_ALGO_SEQ;
    al.last.assign(len, 0.0);
    if (tr.C > 0 && tr.N > 0) {
        if (!seq && (!ps.fb_recs || !tr.d_arow)) return set_err(HF_E_ARG, "hf_get_alpha_stats: the last pass kept no pair records");
        if (!seq && tr.tabwork.n_jobs != tr.n_arows) return set_err(HF_E_ARG, "hf_get_alpha_stats: the job list of the context is not the list of its rows of A");
        if (!seq) {
            const int rc = pass_all_records(ps);
            if (rc) return rc;
        }
        const int rc = alpha_plan(ctx);
        if (rc) return rc;
        hipStream_t st = ps.last_stream;
        const AlBlock* blocks = reinterpret_cast<const AlBlock*>(al.d_blocks);
        if (al.n_blocks > 0) {
            if (!seq) {      // (the rows of A of a segment pass are the jobs of the track's list: enqueue_pass)
                const int nj = tr.tabwork.n_jobs;
                hipLaunchKernelGGL(k_alpha_terms, dim3((unsigned) ((nj + 255) / 256)), dim3(256), 0, st, nj, tr.d_jobs, ps.d_params, al.d_terms);
            }
            const PassView pv = view_of(ctx);
            by_algo(tr, [&](auto S) {
                hipLaunchKernelGGL(k_alpha_pairs<decltype(S)::value>, dim3((unsigned) al.n_blocks), dim3(HF_AL_THREADS), 0, st, blocks, al.d_pair_t,
                                   al.d_pair_c, tr.d_beta, seq ? nullptr : al.d_terms, pv, al.d_part);
            });
        }
        hipLaunchKernelGGL(k_alpha_sum, dim3((unsigned) tr.R), dim3(HF_AL_SUM_THREADS), 0, st, al.d_rblk0, al.d_part, al.d_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(al.last.data(), al.d_out, len * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    al.cached = true;
    std::memcpy(out_host, al.last.data(), len * 8);
    return HF_OK;
}


// exact mean and variance of label totals (hf_moments.h): k_mo_piece multiplies the pieces' jets, k_mo_chain carries every part's vectors
// through them, a job's mean and variance are the sums of its parts'
int hf_get_count_moments(hf_ctx* ctx, int64_t n, const int64_t* first, const int64_t* last, const uint8_t* state_mask, const int32_t* region,
                         int unit, double* mean_host, double* var_host) {
    const std::string who = "hf_get_count_moments";
    if (!ctx) return set_err(HF_E_ARG, who + ": bad argument");
    const Track& tr = ctx->tr;
    int rc = rg_check(ctx, who, n, !first || !last || !state_mask || !mean_host || !var_host, first, last, state_mask, region,
                      unit != HF_COUNT_WINDOWS && unit != HF_COUNT_BASES ? "unknown unit" : nullptr);
    if (rc) return rc;
    PassView pv;
    rc = pass_view(ctx, who, n, pv);
    if (rc || n == 0) return rc;
    hipStream_t st = ctx->pass.last_stream;
    const int W = unit == HF_COUNT_BASES ? tr.meta.window_len : 0;
    if (unit == HF_COUNT_BASES && W < 1) return set_err(HF_E_ARG, who + ": the context has no window length");
    return rg_run<MoPiece, MoPart, HF_MO_PIECE>(ctx, who, ctx->mo, n, first, last, HF_MO_BATCH_PIECES, HF_MO_BATCH_PARTS, 48 * 8, 8, 2,
        [&](int64_t j, int c, int64_t a, int64_t b) {
            return MoPart{a, b, 0, 0, state_mask[j], region ? region[j] : -1, c, (int) (a - tr.h_off[(size_t) c]), tr.h_cs[(size_t) c], tr.h_ce[(size_t) c]};
        },
        [](const MoPart& pt, int64_t t, int len) { return MoPiece{t, len, pt.mask, pt.region, pt.c, pt.ka + (int) (t - pt.a), pt.cs, pt.ce}; },
        [&](const RgBatch<MoPiece, MoPart>& bt) {
            by_algo(tr, [&](auto S) {
                constexpr bool SEQ = decltype(S)::value;
                if (bt.np) hipLaunchKernelGGL(k_mo_piece<SEQ>, bt.piece_grid(), dim3(64), 0, st, bt.pieces, W, pv, bt.pm, bt.px);
                hipLaunchKernelGGL(k_mo_chain<SEQ>, bt.chain_grid(), dim3(64), 0, st, (int) bt.nq, bt.parts, W, bt.pm, bt.px, pv, bt.out);
            });
        },
        [&](int64_t j, const MoPart*, const double* val, int64_t k0, int64_t k1) {
            double m = 0.0, v = 0.0;
            for (int64_t k = k0; k < k1; k++) { m += val[(size_t) k * 2]; v += val[(size_t) k * 2 + 1]; }
            mean_host[j] = m; var_host[j] = v;
        });
}


// exact mean and variance of block counts (hf_runs.h): k_run_piece multiplies the pieces' jets, k_run_chain carries every part's vectors
// through them and writes the part's seven numbers, the host stitches the parts of a job left to right (the joins between chunks:
// include/hmm_flagger_hip.h)
int hf_get_run_moments(hf_ctx* ctx, int64_t n, const int64_t* first, const int64_t* last, const uint8_t* state_mask, const uint8_t* joined,
                       double* mean_host, double* var_host) {
    const std::string who = "hf_get_run_moments";
    if (!ctx) return set_err(HF_E_ARG, who + ": bad argument");
    const Track& tr = ctx->tr;
    int rc = rg_check(ctx, who, n, !first || !last || !state_mask || !mean_host || !var_host, first, last, state_mask, nullptr, nullptr,
                      joined && tr.C > 0 && joined[0] ? "joined[0] must be 0 (the first chunk continues nothing)" : nullptr);
    if (rc) return rc;
    PassView pv;
    rc = pass_view(ctx, who, n, pv);
    if (rc || n == 0) return rc;
    hipStream_t st = ctx->pass.last_stream;
    return rg_run<RnPiece, RnPart, HF_RN_PIECE>(ctx, who, ctx->rn, n, first, last, HF_MO_BATCH_PIECES, HF_MO_BATCH_PARTS, 48 * 8, 8, HF_RN_OUT,
        [&](int64_t j, int c, int64_t a, int64_t b) { return RnPart{a, b, 0, 0, state_mask[j], c}; },
        [](const RnPart& pt, int64_t t, int len) { return RnPiece{t, len, pt.mask, pt.c}; },
        [&](const RgBatch<RnPiece, RnPart>& bt) {
            by_algo(tr, [&](auto S) {
                constexpr bool SEQ = decltype(S)::value;
                if (bt.np) hipLaunchKernelGGL(k_run_piece<SEQ>, bt.piece_grid(), dim3(64), 0, st, bt.pieces, pv, bt.pm, bt.px);
                hipLaunchKernelGGL(k_run_chain<SEQ>, bt.chain_grid(), dim3(64), 0, st, (int) bt.nq, bt.parts, bt.pm, bt.px, pv, bt.out);
            });
        },
        [&](int64_t j, const RnPart* parts, const double* val, int64_t k0, int64_t k1) {
            // the parts of a job in chunk order.  x = (E[R], Var(R), s, e, Cov(R, E0), Cov(R, S0), Cov(S0, E0)) of a part; part k is joined
            // to part k - 1 by the join rule of hf_jobs.h.  Three sums, each left to right:
            //   mean = sum E[R] - sum_joined q,  var = sum Var(R) + sum_joined [...] + 2 sum_{both joined} [...]   (q = e_{k-1} s_k)
            // so a job without a join is the plain sum of its parts.
            double m = 0.0, mq = 0.0, v = 0.0, vj = 0.0, vjj = 0.0;
            bool prev_join = false;
            for (int64_t k = k0; k < k1; k++) {
                const double* x = &val[(size_t) k * HF_RN_OUT];
                m += x[0]; v += x[1];
                const bool join = part_joined(parts, k, k0, joined);
                if (join) {
                    const double* y = x - HF_RN_OUT;      // the part before
                    const double q = y[3] * x[2];
                    mq += q;
                    vj += q * (1.0 - q) - 2.0 * (x[2] * y[4] + y[3] * x[5]);
                    if (prev_join) vjj += (y - HF_RN_OUT)[3] * x[2] * y[6];
                }
                prev_join = join;
            }
            double var = (v + vj) + 2.0 * vjj;
            if (!(var > 0.0)) var = 0.0;      // (a negative rounding residue)
            mean_host[j] = m - mq; var_host[j] = var;
        });
}


// exact path entropy and labelling log-probability (hf_entropy.h): k_ent_piece sums the pieces' local terms, k_ent_chain adds every part's
// first window and its piece sums, a job is the sum of its parts.
// labels == nullptr: the path entropy of every job; else the log-probability of the labelling inside every job's range
static int ent_jobs(hf_ctx* ctx, const std::string& who, int64_t n, const int64_t* first, const int64_t* last, const int8_t* labels, bool with_labels,
                    double* out_host) {
    if (!ctx) return set_err(HF_E_ARG, who + ": bad argument");
    const Track& tr = ctx->tr;
    int rc = rg_check(ctx, who, n, !first || !last || !out_host || (with_labels && !labels), first, last, nullptr);
    if (rc) return rc;
    // the labels of the call: the union of the ranges, and nothing outside it, is looked at; lo .. hi is the span of the union
    std::vector<int8_t> lab;
    int64_t lo = 0, hi = -1;
    if (with_labels && n > 0) {
        std::vector<std::pair<int64_t, int64_t>> rg((size_t) n);
        for (int64_t i = 0; i < n; i++) rg[(size_t) i] = {first[i], last[i]};
        std::sort(rg.begin(), rg.end());
        lo = rg.front().first;
        for (const auto& r : rg) hi = std::max(hi, r.second);
        lab.assign((size_t) (hi - lo + 1), 0);
        int64_t done = lo;                        // every window below `done` is checked and copied
        for (const auto& r : rg) {
            for (int64_t t = std::max(done, r.first); t <= r.second; t++) {
                if (labels[t] < 0 || labels[t] > 3) return set_err(HF_E_ARG, who + ": a label outside 0..3 (window " + std::to_string(t) + ")");
                lab[(size_t) (t - lo)] = labels[t];
            }
            done = std::max(done, r.second + 1);
        }
    }
    PassView pv;
    rc = pass_view(ctx, who, n, pv);
    if (rc || n == 0) return rc;
    hipStream_t st = ctx->pass.last_stream;
    if (with_labels) {
        rc = ctx->en_lab.reserve(lab.size(), who);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(ctx->en_lab.d_buf, lab.data(), lab.size(), hipMemcpyHostToDevice, st));
    }
    const int8_t* d_lab = reinterpret_cast<const int8_t*>(ctx->en_lab.d_buf);
    const long long lab0 = lo;
    return rg_run<EnPiece, EnPart, HF_EN_PIECE>(ctx, who, ctx->en, n, first, last, HF_MO_BATCH_PIECES, HF_MO_BATCH_PARTS, 8, 0, 1,
        [&](int64_t, int c, int64_t a, int64_t) { return EnPart{a, 0, 0, c, 0}; },
        [](const EnPart& pt, int64_t t, int len) { return EnPiece{t, len, pt.c}; },
        [&](const RgBatch<EnPiece, EnPart>& bt) {
            auto launch = [&](auto S, auto LB) {
                constexpr bool SEQ = decltype(S)::value, LAB = decltype(LB)::value;
                if (bt.np) hipLaunchKernelGGL((k_ent_piece<SEQ, LAB>), bt.piece_grid(), dim3(64), 0, st, bt.pieces, pv, d_lab, lab0, bt.pm);
                hipLaunchKernelGGL((k_ent_chain<SEQ, LAB>), bt.chain_grid(), dim3(64), 0, st, (int) bt.nq, bt.parts, bt.pm, pv, d_lab, lab0, bt.out);
            };
            by_algo(tr, [&](auto S) { if (with_labels) launch(S, std::true_type{}); else launch(S, std::false_type{}); });
        },
        [&](int64_t j, const EnPart*, const double* val, int64_t k0, int64_t k1) {
            double v = 0.0;
            for (int64_t k = k0; k < k1; k++) v += val[k];
            out_host[j] = v;
        });
}

int hf_get_path_entropy(hf_ctx* ctx, int64_t n, const int64_t* first, const int64_t* last, double* entropy_host) {
    return ent_jobs(ctx, "hf_get_path_entropy", n, first, last, nullptr, false, entropy_host);
}

int hf_get_path_log_probs(hf_ctx* ctx, int64_t n, const int64_t* first, const int64_t* last, const int8_t* labels_host, double* log_p_host) {
    return ent_jobs(ctx, "hf_get_path_log_probs", n, first, last, labels_host, true, log_p_host);
}

// windows per launch of k_ent_profile (16 bytes of results per window)
#define HF_EN_PROFILE_BATCH ((int64_t) 1 << 22)

int hf_get_entropy_profile(hf_ctx* ctx, int64_t first, int64_t n, double* marg_host, double* cond_host) {
    const std::string who = "hf_get_entropy_profile";
    if (!ctx) return set_err(HF_E_ARG, who + ": bad argument");
    const Track& tr = ctx->tr;
    if (!marg_host && !cond_host) return set_err(HF_E_ARG, who + ": both output arrays are NULL");
    if (first < 0 || n < 0 || first > tr.N || n > tr.N - first) return set_err(HF_E_ARG, who + ": bad range");
    if (n > 0 && !in_chunks(tr, first, first + n - 1)) return set_err(HF_E_ARG, who + ": the range holds a window outside every chunk");
    if (!ctx->pass.have_full)
        return set_err(HF_E_ARG, who + ": no HF_MODE_FULL pass to answer for (none yet, or the last pass was forward-only)");
    PassView pv;
    int rc = pass_view(ctx, who, n, pv);
    if (rc || n == 0) return rc;
    hipStream_t st = ctx->pass.last_stream;
    const int64_t nb = std::min<int64_t>(n, HF_EN_PROFILE_BATCH);
    const size_t o_cond = Slab::granule((size_t) nb * 8);
    rc = ctx->en.reserve(2 * o_cond, who);
    if (rc) return rc;
    double* d_marg = marg_host ? reinterpret_cast<double*>(ctx->en.d_buf) : nullptr;
    double* d_cond = cond_host ? reinterpret_cast<double*>(ctx->en.d_buf + o_cond) : nullptr;
    for (int64_t i0 = 0; i0 < n; i0 += nb) {
        const int64_t m = std::min<int64_t>(nb, n - i0);
        by_algo(tr, [&](auto S) {
            hipLaunchKernelGGL(k_ent_profile<decltype(S)::value>, dim3((unsigned) ((m + 255) / 256)), dim3(256), 0, st, (long long) (first + i0),
                               (long long) m, tr.d_off, tr.C, pv, d_marg, d_cond);
        });
        HIPCHK(hipGetLastError());
        if (marg_host) HIPCHK(hipMemcpyAsync(marg_host + i0, d_marg, (size_t) m * 8, hipMemcpyDeviceToHost, st));
        if (cond_host) HIPCHK(hipMemcpyAsync(cond_host + i0, d_cond, (size_t) m * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return HF_OK;
}


// ------------------------------------------------------------------------------------------
// exact breakpoint posteriors (hf_breakpoint.h): the first range getter with a value per window of a job.  It shares rg_check, pass_view
// and the batch loop (rg_batches) with the others; bp_run is rg_run's sibling for four launches and the per-window weight arrays of a batch.
// ------------------------------------------------------------------------------------------
#include "hf_breakpoint.h"

static_assert(HF_BP_PIECE == 512, "one piece grid for every getter");

// The jobs of a call, batch by batch, on the stream of the pass: k_bp_piece, k_bp_chain, k_bp_weights, k_bp_quant.  prof_host (a call of
// one job): its p_k.
static int bp_run(hf_ctx* ctx, const std::string& who, const PassView& pv, int64_t n, const int64_t* first, const int64_t* last,
                  const uint8_t* um, const uint8_t* vm, const BpProbs& pr, double* lpe_host, int64_t* quant_host, int64_t* mode_host,
                  double* mode_p_host, double* prof_host) {
    hipStream_t st = ctx->pass.last_stream;
    std::vector<double> vd;
    std::vector<long long> vi;
    constexpr size_t NI = HF_BP_MAX_PROBS + 1;
    long long nw = 0;      // windows with a weight so far in the batch being cut
    return rg_batches<BpPiece, BpPart, HF_BP_PIECE>(ctx, n, first, last, HF_BP_BATCH_PIECES, HF_BP_BATCH_PARTS,
        [&](int64_t j, int c, int64_t a, int64_t b) { BpPart pt{a, b, nw, 0, 0, um[j], vm[j], c, 0}; nw += b - a; return pt; },
        [](const BpPart& pt, int64_t t, int len) { return BpPiece{t, pt.w0 + (t - pt.a - 1), len, pt.um, pt.vm, 0}; },
        [&](const auto& jc, int64_t) -> int {
            const size_t np = jc.pieces.size(), nq = jc.parts.size(), nwb = (size_t) std::exchange(nw, 0LL);      // (the next cut starts a batch)
            BpPiece* d_pieces; BpPart* d_parts;
            double *d_pm, *d_lv, *d_rv, *d_nn, *d_wm, *d_prof = nullptr, *d_outd;
            int *d_pe, *d_we; long long *d_le, *d_re, *d_outi;
            const int rc = rg_take(ctx->bp, who, [&](auto f) {
                f(d_pieces, np * sizeof(BpPiece)); f(d_parts, nq * sizeof(BpPart)); f(d_pm, np * 48 * 8); f(d_pe, np * 4 * 4);
                f(d_lv, np * 4 * 8); f(d_le, np * 8); f(d_rv, np * 4 * 8); f(d_re, np * 8); f(d_nn, nq * 8);
                f(d_wm, nwb * 8); f(d_we, nwb * 4); if (prof_host) f(d_prof, nwb * 8);
                f(d_outd, nq * 2 * 8); f(d_outi, nq * NI * 8);
            });
            if (rc) return rc;
            HIPCHK(hipMemcpyAsync(d_pieces, jc.pieces.data(), np * sizeof(BpPiece), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_parts, jc.parts.data(), nq * sizeof(BpPart), hipMemcpyHostToDevice, st));
            by_algo(ctx->tr, [&](auto S) {
                constexpr bool SEQ = decltype(S)::value;
                hipLaunchKernelGGL(k_bp_piece<SEQ>, dim3((unsigned) np), dim3(64), 0, st, d_pieces, pv, d_pm, d_pe);
                hipLaunchKernelGGL(k_bp_chain<SEQ>, dim3((unsigned) ((nq + 63) / 64)), dim3(64), 0, st, (int) nq, d_parts, d_pm, d_pe, pv, d_lv, d_le,
                                   d_rv, d_re, d_nn);
                hipLaunchKernelGGL(k_bp_weights<SEQ>, dim3((unsigned) np), dim3(64), 0, st, d_pieces, pv, d_lv, d_le, d_rv, d_re, d_wm, d_we);
            });
            hipLaunchKernelGGL(k_bp_quant, dim3((unsigned) nq), dim3(64), 0, st, d_parts, d_wm, d_we, d_nn, pr, d_outd, d_outi, d_prof);
            HIPCHK(hipGetLastError());
            vd.resize(nq * 2);
            vi.resize(nq * NI);
            HIPCHK(hipMemcpyAsync(vd.data(), d_outd, nq * 2 * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(vi.data(), d_outi, nq * NI * 8, hipMemcpyDeviceToHost, st));
            if (prof_host) HIPCHK(hipMemcpyAsync(prof_host, d_prof, nwb * 8, hipMemcpyDeviceToHost, st));
            return HF_OK;
        },
        [&](const auto& jc, int64_t j, size_t i) {      // a job is one part
            const size_t k = (size_t) jc.job_p0[i];
            if (lpe_host) lpe_host[j] = vd[k * 2];
            if (mode_p_host) mode_p_host[j] = vd[k * 2 + 1];
            if (mode_host) mode_host[j] = vi[k * NI];
            for (int q = 0; q < pr.n; q++) quant_host[j * pr.n + q] = vi[k * NI + 1 + (size_t) q];
        });
}

// what the two calls refuse beyond rg_check (which has taken the ranges and the left masks), job by job
static int bp_check(const hf_ctx* ctx, const std::string& who, int64_t n, const int64_t* first, const int64_t* last, const uint8_t* um,
                    const uint8_t* vm) {
    const std::vector<int64_t>& off = ctx->tr.h_off;
    for (int64_t i = 0; i < n; i++) {
        const std::string job = " (job " + std::to_string(i) + ")";
        if (vm[i] < 1 || vm[i] > 15) return set_err(HF_E_ARG, who + ": right_mask must be 1..15" + job);
        if (um[i] & vm[i]) return set_err(HF_E_ARG, who + ": left_mask and right_mask overlap" + job);
        if (first[i] == last[i]) return set_err(HF_E_ARG, who + ": first == last, no window to switch at" + job);
        if (*(std::upper_bound(off.begin(), off.end(), first[i])) <= last[i])
            return set_err(HF_E_ARG, who + ": first and last lie in different chunks" + job);
    }
    return HF_OK;
}

int hf_get_breakpoints(hf_ctx* ctx, int64_t n, const int64_t* first, const int64_t* last, const uint8_t* left_mask, const uint8_t* right_mask,
                       int n_probs, const double* probs, double* log_p_event_host, int64_t* quantile_host, int64_t* mode_host,
                       double* mode_p_host) {
    const std::string who = "hf_get_breakpoints";
    if (!ctx) return set_err(HF_E_ARG, who + ": bad argument");
    const char* early = nullptr;
    BpProbs pr{};
    if (n_probs < 0 || n_probs > HF_BP_MAX_PROBS) early = "n_probs must be 0..8";
    else if (n_probs > 0 && (!probs || !quantile_host)) early = "NULL probs or quantile array with n_probs > 0";
    else {
        pr.n = n_probs;
        for (int q = 0; q < n_probs; q++) {
            if (!(probs[q] > 0.0 && probs[q] < 1.0)) early = "a probability outside (0, 1)";
            pr.q[q] = probs[q];
        }
    }
    int rc = rg_check(ctx, who, n, !first || !last || !left_mask || !right_mask || !log_p_event_host || !mode_host || !mode_p_host, first, last,
                      left_mask, nullptr, early);
    if (rc) return rc;
    if ((rc = bp_check(ctx, who, n, first, last, left_mask, right_mask))) return rc;
    PassView pv;
    rc = pass_view(ctx, who, n, pv);
    if (rc || n == 0) return rc;
    return bp_run(ctx, who, pv, n, first, last, left_mask, right_mask, pr, log_p_event_host, quantile_host, mode_host, mode_p_host, nullptr);
}

int hf_get_breakpoint_profile(hf_ctx* ctx, int64_t first, int64_t last, uint8_t left_mask, uint8_t right_mask, double* p_host,
                              double* log_p_event_host) {
    const std::string who = "hf_get_breakpoint_profile";
    if (!ctx) return set_err(HF_E_ARG, who + ": bad argument");
    int rc = rg_check(ctx, who, 1, !p_host || !log_p_event_host, &first, &last, &left_mask);
    if (rc) return rc;
    if ((rc = bp_check(ctx, who, 1, &first, &last, &left_mask, &right_mask))) return rc;
    PassView pv;
    rc = pass_view(ctx, who, 1, pv);
    if (rc) return rc;
    return bp_run(ctx, who, pv, 1, &first, &last, &left_mask, &right_mask, BpProbs{}, log_p_event_host, nullptr, nullptr, nullptr, p_host);
}


// ------------------------------------------------------------------------------------------
// exact long-run probabilities (hf_longrun.h): the job cutter's parts fall into groups of joined parts (hf_jobs.h group_parts), one
// wavefront of k_lr_chain walks a group's expanded chain, a job is folded from its groups on the host.
// ------------------------------------------------------------------------------------------
#include "hf_longrun.h"

static_assert(HF_LONGRUN_MAX_LANES == 64, "one wavefront holds the expanded chain");

// parts, and windows in pieces of 512 (the grid of the other getters), per device batch: a group is one workgroup and a window one step
// of it, so the caps bound a launch's run time, not its memory.  The environment variables of the same names lower them (rg_cap; tests).
#ifndef HF_LR_BATCH_PARTS
#define HF_LR_BATCH_PARTS (1 << 16)
#endif
#ifndef HF_LR_BATCH_PIECES
#define HF_LR_BATCH_PIECES (1 << 18)
#endif

// log(1 - exp(x)), x <= 0
static double lr_log1mexp(double x) { return x > -0.69314718055994530942 ? std::log(-std::expm1(x)) : std::log1p(-std::exp(x)); }

int hf_get_long_run_log_probs(hf_ctx* ctx, int64_t n, const int64_t* first, const int64_t* last, const uint8_t* state_mask, const int32_t* min_len,
                              const uint8_t* joined, double* log_p_none_host, double* log_p_some_host) {
    const std::string who = "hf_get_long_run_log_probs";
    if (!ctx) return set_err(HF_E_ARG, who + ": bad argument");
    const Track& tr = ctx->tr;
    int rc = rg_check(ctx, who, n, !first || !last || !state_mask || !min_len || (!log_p_none_host && !log_p_some_host), first, last, state_mask,
                      nullptr, nullptr, joined && tr.C > 0 && joined[0] ? "joined[0] must be 0 (the first chunk continues nothing)" : nullptr);
    if (rc) return rc;
    for (int64_t i = 0; i < n; i++) {
        if (min_len[i] < 1) return set_err(HF_E_ARG, who + ": min_len must be at least 1 (job " + std::to_string(i) + ")");
        if (long_run_lanes(state_mask[i], min_len[i]) > HF_LONGRUN_MAX_LANES)
            return set_err(HF_E_ARG, who + ": the expanded chain needs more than " + std::to_string(HF_LONGRUN_MAX_LANES) + " lanes (job " + std::to_string(i) + ")");
    }
    PassView pv;
    rc = pass_view(ctx, who, n, pv);
    if (rc || n == 0) return rc;
    hipStream_t st = ctx->pass.last_stream;
    std::vector<LrGroup> groups;
    std::vector<int64_t> job_g0;
    std::vector<double> val;
    return rg_batches<LrPiece, LrPart, 512>(ctx, n, first, last, rg_cap("HF_LR_BATCH_PIECES", HF_LR_BATCH_PIECES),
        rg_cap("HF_LR_BATCH_PARTS", HF_LR_BATCH_PARTS),
        [](int64_t, int c, int64_t a, int64_t b) { return LrPart{a, b, 0, 0, c, 0}; },
        [](const LrPart&, int64_t, int) { return LrPiece{0}; },
        [&](const auto& jc, int64_t j0) -> int {      // (no piece is uploaded: they count windows for the cap)
            group_parts(jc.parts, jc.job_p0, joined, groups, job_g0,
                [&](int64_t j, int64_t q0, int64_t q1) { return LrGroup{(int) q0, (int) q1, state_mask[j0 + j], min_len[j0 + j]}; });
            const size_t nq = jc.parts.size(), ng = groups.size();
            LrPart* d_parts; LrGroup* d_groups; double* d_out;
            const int rc = rg_take(ctx->lr, who, [&](auto f) { f(d_parts, nq * sizeof(LrPart)); f(d_groups, ng * sizeof(LrGroup)); f(d_out, ng * 2 * 8); });
            if (rc) return rc;
            HIPCHK(hipMemcpyAsync(d_parts, jc.parts.data(), nq * sizeof(LrPart), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_groups, groups.data(), ng * sizeof(LrGroup), hipMemcpyHostToDevice, st));
            by_algo(tr, [&](auto S) {
                constexpr bool SEQ = decltype(S)::value;
                hipLaunchKernelGGL(k_lr_chain<SEQ>, dim3((unsigned) ng), dim3(64), 0, st, d_groups, d_parts, pv, d_out);
            });
            HIPCHK(hipGetLastError());
            val.resize(ng * 2);
            HIPCHK(hipMemcpyAsync(val.data(), d_out, ng * 2 * 8, hipMemcpyDeviceToHost, st));
            return HF_OK;
        },
        [&](const auto&, int64_t j, size_t i) {
            // the groups of a job in chunk order: log_p_none is their left-to-right sum.  log_p_some: -inf when no group can hold a run,
            // the kernel's own value (accurate however small) when exactly one can, else log(1 - exp(log_p_none))
            double none = 0.0, some = -__builtin_inf();
            int hits = 0;
            for (int64_t g = job_g0[i]; g < job_g0[i + 1]; g++) {
                none += val[(size_t) g * 2];
                const double s = val[(size_t) g * 2 + 1];
                if (!(s == -__builtin_inf())) { hits++; some = s; }
            }
            if (hits > 1) some = lr_log1mexp(none);
            if (log_p_none_host) log_p_none_host[j] = none;
            if (log_p_some_host) log_p_some_host[j] = some;
        });
}
