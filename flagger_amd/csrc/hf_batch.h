// hf_batch.h — many models on one context (hf_batch_*, include/hmm_flagger_hip.h): every model of a batch is one more PASS over the
// context's TRACK (hf_host.h: Track, Pass).  The windows, the segment plan, the rows stream arow, the statistics plan and the job list of
// k_tables are the track's and are read by every model; everything a pass, hf_finish or a getter writes (parameter block, tables, lutA,
// hand-off flags and epochs, pair records, sums, labels, flags, totals, the pinned result block) is the model's Pass, made by pass_create as
// the context's own is.  A pass of model m is the ordinary enqueue_pass / pass_finish of its Pass: the same kernels, the same launch
// geometry, the same arithmetic in the same order as hf_estep on the context — so the results are the single path's bits, and a NaN or an
// underflow in one model raises that model's flag word only.  The context's own pass is never written by a batch.  Included once, at the
// end of hf_estep.hip (in front of hf_getters.h).

struct hf_batch {
    hf_ctx* ctx = nullptr;
    std::vector<std::unique_ptr<Pass>> m;     // one pass per model
    std::vector<int32_t> last;                // the models of the last hf_batch_estep, in its order (what hf_batch_finish waits for)
    SegFbModel* d_tab = nullptr;              // [models] every model's pointers for k_seg_fb_batch (device memory)
    int last_batched = 0;                     // models whose segment kernel ran in a shared launch in the last hf_batch_estep
};

// why `ctx` cannot carry a batch (nullptr: it can)
static const char* batch_refusal(const hf_ctx* ctx) {
    if (!ctx) return "no context";
    const Track& tr = ctx->tr;
    if (tr.algo != HF_ALGO_SCAN) return "the batch engine covers HF_ALGO_SCAN contexts only";
    if (!seg_pass(tr)) return "the context runs no segment kernels (no windows, or more than 2^30 of them)";
    if (tr.subs.size() != 1) return "the context runs sub-passes (hf_sub_passes > 1): the batch engine covers one sub-pass";
    if (ctx->pass.d_nbE || ctx->pass.pass_nb) return "negative_binomial has no alpha: the batch engine covers trunc_exp_gaussian and gaussian";
    return nullptr;
}

extern "C" {

int hf_batch_capacity(const hf_ctx* ctx) {
    if (batch_refusal(ctx)) return 0;
    const Track& tr = ctx->tr;
    if (hipSetDevice(tr.device) != hipSuccess) { (void) hipGetLastError(); return 0; }
    size_t fr = 0, total = 0;
    if (hipMemGetInfo(&fr, &total) != hipSuccess) { (void) hipGetLastError(); return 0; }
    const PassLayout L = pass_layout(tr);
    const size_t per = L.device_bytes() + ((size_t) 1 << 20);           // (+ a slab's worth of slack per model)
    size_t n = (fr / 10 * 9) / per;                                       // nine tenths of what is free
    // and the PINNED host memory a model takes: its result block, the label staging of its first hf_batch_get_labels and the row-statistics
    // partials that the host sums — at most an eighth of the host's physical memory for the whole batch
    const size_t pin = L.pin_block + ((size_t) tr.N + 16) + ((size_t) tr.n_rowwaves * stat_acc_len(16) + (size_t) tr.C + 65) * 8;
    const long pages = sysconf(_SC_PHYS_PAGES), psz = sysconf(_SC_PAGESIZE);
    if (pages > 0 && psz > 0) n = std::min(n, (size_t) pages * (size_t) psz / 8 / pin);
    return (int) std::min<size_t>(n, HF_BATCH_MAX_MODELS);
}

int hf_batch_create(hf_ctx* ctx, int n_models, hf_batch** out) {
    if (!out) return set_err(HF_E_ARG, "hf_batch_create: bad argument");
    *out = nullptr;
    if (const char* why = batch_refusal(ctx)) return set_err(HF_E_ARG, std::string("hf_batch_create: ") + why);
    if (n_models < 1 || n_models > HF_BATCH_MAX_MODELS) return set_err(HF_E_ARG, "hf_batch_create: n_models must be 1 .. HF_BATCH_MAX_MODELS");
    HIPCHK(hipSetDevice(ctx->tr.device));
    hf_batch* b = new hf_batch();
    b->ctx = ctx;
    for (int i = 0; i < n_models; i++) {   // a model's settings start from the context's pass; profiling and host trace off
        b->m.push_back(std::make_unique<Pass>());
        const int rc = pass_create(ctx->tr, ctx->pass, b->m.back().get());
        if (rc) { hf_batch_destroy(b); return rc; }
    }
    {   // the pointer table of k_seg_fb_batch: one row per model, written once
        std::vector<SegFbModel> tab((size_t) n_models);
        for (int i = 0; i < n_models; i++) {
            const Pass& s = *b->m[(size_t) i];
            SegFbModel& t = tab[(size_t) i];
            t.lutA = s.d_lutA; t.P = s.d_params; t.Qs = nullptr; t.Pseg = s.d_Pseg; t.ready = s.d_seg_ready;
            t.recs = s.d_recs; t.scale_s = nullptr; t.label = s.d_label; t.seg_ll = s.d_seg_ll; t.flags = s.d_flags;
        }
        if (hipMalloc((void**) &b->d_tab, tab.size() * sizeof(SegFbModel)) != hipSuccess ||
            hipMemcpy(b->d_tab, tab.data(), tab.size() * sizeof(SegFbModel), hipMemcpyHostToDevice) != hipSuccess) {
            const hipError_t e = hipGetLastError();
            hf_batch_destroy(b);
            return set_err(HF_E_HIP, std::string("hf_batch_create: ") + hipGetErrorString(e));
        }
    }
    HIPCHK(hipDeviceSynchronize());
    *out = b;
    return HF_OK;
}

void hf_batch_destroy(hf_batch* b) {
    if (!b) return;
    hipSetDevice(b->ctx->tr.device);
    if (b->d_tab) { hipDeviceSynchronize(); hipFree(b->d_tab); }
    for (auto& s : b->m) pass_destroy(*s);
    delete b;
}

int hf_batch_size(const hf_batch* b) { return b ? (int) b->m.size() : 0; }
int hf_batch_shared_models(const hf_batch* b) { return b ? b->last_batched : 0; }

// diagnostics (tests/test_batch_gpu.py): model `model`'s hand-off epoch and the flag words its segments have published so far
int64_t hf_batch_handoff(hf_batch* b, int model, uint32_t* epoch, uint32_t* ready_host, int64_t n) {
    if (!b || model < 0 || model >= (int) b->m.size() || n < 0 || (n > 0 && !ready_host)) return set_err(HF_E_ARG, "hf_batch_handoff: bad argument");
    Pass& s = *b->m[(size_t) model];
    const Track& tr = b->ctx->tr;
    HIPCHK(hipSetDevice(tr.device));
    HIPCHK(hipStreamSynchronize(s.last_stream));
    if (epoch) *epoch = s.seg_epoch;
    const int64_t k = std::min<int64_t>(n, tr.nseg);
    if (k > 0 && s.d_seg_ready) HIPCHK(hipMemcpy(ready_host, s.d_seg_ready, (size_t) k * 4, hipMemcpyDeviceToHost));
    return tr.nseg;
}

static int batch_models_ok(const hf_batch* b, const int32_t* models, int n_active, const char* who) {
    if (!b || (n_active > 0 && !models) || n_active < 0) return set_err(HF_E_ARG, std::string(who) + ": bad argument");
    for (int i = 0; i < n_active; i++) {
        if (models[i] < 0 || models[i] >= (int) b->m.size()) return set_err(HF_E_ARG, std::string(who) + ": model index out of range");
        for (int j = 0; j < i; j++)
            if (models[j] == models[i]) return set_err(HF_E_ARG, std::string(who) + ": a model is listed twice");
    }
    return HF_OK;
}

int hf_batch_estep(hf_batch* b, const hf_params* p, const int32_t* models, int n_active, int mode, void* stream) {
    int rc = batch_models_ok(b, models, n_active, "hf_batch_estep");
    if (rc) return rc;
    if (n_active > 0 && !p) return set_err(HF_E_ARG, "hf_batch_estep: bad argument");
    for (int i = 0; i < n_active; i++)
        if (p[i].model_type == HF_MODEL_NEGATIVE_BINOMIAL)
            return set_err(HF_E_ARG, "hf_batch_estep: negative_binomial has no alpha: the batch engine covers trunc_exp_gaussian and gaussian");
    hipStream_t st = (hipStream_t) stream;
    const Track& tr = b->ctx->tr;
    HIPCHK(hipSetDevice(tr.device));
    b->last.clear();
    b->last_batched = 0;
    // The shared launch covers full passes of models in one-launch mode with statistics by emission row and one sub-pass (the default
    // pass): tables per model, ONE k_seg_fb_batch over all of them, then per model k_pair_sums and k_row_stats.  A model that has fallen
    // back to two launches (a timed-out hand-off), a forward-only pass or the per-chunk statistics run the model's whole pass on its own.
    std::vector<int> joint;
    for (int i = 0; i < n_active; i++) {
        Pass& s = *b->m[(size_t) models[i]];
        rc = pack_params(tr, &p[i], s.h_params);
        if (rc) return rc;
        s.last_p = p[i]; s.last_mode = mode; s.last_stream = st;
        const bool shared = mode == HF_MODE_FULL && s.seg_fused && rows_pass(s) && tr.subs.size() == 1 && tr.C > 0 && tr.ntiles > 0;
        rc = enqueue_pass(s, &p[i], mode, st, false, shared ? PASS_PRE : PASS_ALL);
        if (rc) return rc;
        if (shared) joint.push_back(i);
    }
    if (!joint.empty()) {
        const auto& sb = tr.subs[0];
        const int g0 = sb.seg0, nblk = sb.seg1 - sb.seg0;
        const int nc = tr.seg_nc;
        const size_t lds = seg_lds_bytes(nc);
        if (nc > 0 && lds > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_seg_fb_batch<true, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess)
            HIPCHK(hipGetLastError());
        for (size_t j0 = 0; j0 < joint.size() && nblk > 0; j0 += HF_SEG_BATCH_MAX) {
            const size_t nj = std::min<size_t>(HF_SEG_BATCH_MAX, joint.size() - j0);
            SegFbBatch bt{};
            for (size_t j = 0; j < nj; j++) {
                const int i = joint[j0 + j];
                Pass& s = *b->m[(size_t) models[i]];
                const unsigned epoch = ++s.seg_epoch;
                bt.model[j] = models[i];
                bt.epoch[j] = epoch;
                bt.wait_epoch[j] = (s.seg_test_timeout && epoch == 1) ? 0xffffffffu : epoch;
            }
            const dim3 grid((unsigned) nblk, (unsigned) nj);
            if (nc > 0) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_seg_fb_batch<true, true, true>), grid, dim3(64), lds, st, tr.d_seg, tr.d_arow, b->d_tab, bt,
                                           tr.d_pos, (int32_t) g0, nc);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_seg_fb_batch<true, true, false>), grid, dim3(64), lds, st, tr.d_seg, tr.d_arow, b->d_tab, bt,
                                    tr.d_pos, (int32_t) g0, nc);
            HIPCHK(hipGetLastError());
        }
        for (int i : joint) {
            rc = enqueue_pass(*b->m[(size_t) models[i]], &p[i], mode, st, false, PASS_POST);
            if (rc) return rc;
        }
        b->last_batched = (int) joint.size();
    }
    for (int i = 0; i < n_active; i++) {
        b->m[(size_t) models[i]]->have_full = (mode == HF_MODE_FULL);
        b->last.push_back(models[i]);
    }
    return HF_OK;
}

int hf_batch_finish(hf_batch* b, double* stats_host, int32_t* status, void* stream) {
    if (!b || (!b->last.empty() && (!stats_host || !status))) return set_err(HF_E_ARG, "hf_batch_finish: bad argument");
    const int64_t V = b->ctx->tr.V;
    const std::vector<int32_t> act = b->last;
    b->last.clear();
    for (size_t i = 0; i < act.size(); i++) {
        // a model's own failure (HF_E_SCALE, HF_E_NAN, HF_E_REGION) goes to its status word and the batch goes on; a failure of the
        // runtime or of the arguments ends the call
        const int r = pass_finish(*b->m[(size_t) act[i]], stats_host + i * (size_t) V, stream);
        status[i] = r;
        if (r == HF_E_HIP || r == HF_E_ARG) return r;
    }
    return HF_OK;
}

int hf_batch_get_labels(hf_batch* b, int model, int8_t* labels_host) {
    if (!b || model < 0 || model >= (int) b->m.size()) return set_err(HF_E_ARG, "hf_batch_get_labels: bad argument");
    return pass_labels(*b->m[(size_t) model], labels_host);
}

int hf_batch_get_posterior(hf_batch* b, int model, int64_t first, int64_t n, double* post_host) {
    if (!b || model < 0 || model >= (int) b->m.size()) return set_err(HF_E_ARG, "hf_batch_get_posterior: bad argument");
    return pass_posterior(*b->m[(size_t) model], first, n, post_host);
}

int hf_em_iterate_batch(hf_batch* b, hfm_model** model_objs, const int32_t* active, int n_active, int mode, int do_mstep, double tol,
                        double* stats_host, int32_t* status, int* converged, void* stream) {
    if (!b || n_active < 0 || (n_active > 0 && (!model_objs || !active || !stats_host || !status)) ||
        (mode != HF_MODE_FULL && mode != HF_MODE_FORWARD_ONLY))
        return set_err(HF_E_ARG, "hf_em_iterate_batch: bad argument");
    std::vector<hf_params> ps((size_t) n_active);
    for (int i = 0; i < n_active; i++) {
        if (!model_objs[i]) return set_err(HF_E_ARG, "hf_em_iterate_batch: bad argument");
        hfm_params(model_objs[i], &ps[(size_t) i]);
    }
    int rc = hf_batch_estep(b, ps.data(), active, n_active, mode, stream);
    if (rc == HF_OK) rc = hf_batch_finish(b, stats_host, status, stream);
    if (rc != HF_OK) return rc;
    const size_t V = (size_t) b->ctx->tr.V;
    for (int i = 0; i < n_active; i++) {
        if (converged) converged[i] = 0;
        if (status[i] != HF_OK) continue;
        const double* st = stats_host + (size_t) i * V;
        hfm_set_loglikelihood(model_objs[i], st[0]);
        if (do_mstep && mode == HF_MODE_FULL) {
            const int cv = hfm_estimate(model_objs[i], st, tol);
            if (converged) converged[i] = cv;
        }
    }
    return HF_OK;
}

} // extern "C"
