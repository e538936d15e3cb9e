// hf_batch.h — many models on one context (hf_batch_*, include/hmm_flagger_hip.h): the pass state of every model of a batch is a
// SHADOW of the context.  A shadow is an hf_ctx whose model-independent members (the windows, the segment plan, the rows stream
// arow, the statistics plan, the job list of k_tables) point at the context's own device arrays, while everything a pass, hf_finish
// or a getter writes (parameter block, tables, lutA, hand-off flags and epochs, pair records, sums, labels, flags, totals, the pinned
// result block) is allocated for the shadow alone.  A pass of model m is the ordinary enqueue_pass / hf_finish of its shadow: the same
// kernels, the same launch geometry, the same arithmetic in the same order as hf_estep on the context — so the results are the
// single path's bits, and a NaN or an underflow in one model raises that model's flag word only.  The context itself is never
// written by a batch.  Included once, at the end of hf_estep.hip.

struct hf_batch {
    hf_ctx* ctx = nullptr;
    std::vector<hf_ctx*> m;                   // one shadow per model
    std::vector<int32_t> last;                // the models of the last hf_batch_estep, in its order (what hf_batch_finish waits for)
    SegFbModel* d_tab = nullptr;              // [models] every model's pointers for k_seg_fb_batch (device memory)
    int last_batched = 0;                     // models whose segment kernel ran in a shared launch in the last hf_batch_estep
};

// why `ctx` cannot carry a batch (nullptr: it can)
static const char* batch_refusal(const hf_ctx* ctx) {
    if (!ctx) return "no context";
    if (ctx->algo != HF_ALGO_SCAN) return "the batch engine covers HF_ALGO_SCAN contexts only";
    if (!seg_pass(ctx)) return "the context runs no segment kernels (no windows, or more than 2^30 of them)";
    if (ctx->subs.size() != 1) return "the context runs sub-passes (hf_sub_passes > 1): the batch engine covers one sub-pass";
    if (ctx->d_nbE || ctx->pass_nb) return "negative_binomial has no alpha: the batch engine covers trunc_exp_gaussian and gaussian";
    return nullptr;
}

// device bytes one shadow allocates (its slab), 256-byte granules as ctx_alloc rounds them
struct ShadowSizes {
    size_t label, chunk_stats, total, params, lutE, lutC, lutA, tile_ll, tile_stats, seg_ready, seg_ll, Pseg, recs, grp_sums, chunk_ll, rw_stats;
    size_t sum() const {
        auto g = [](size_t b) { b = b ? b : 8; return (b + 255) & ~(size_t) 255; };
        return g(label) + g(chunk_stats) + g(total) + g(4) + g(HF_DONE_BYTES) + g(8) + g(params) + g(lutE) + g(lutC) + (lutA ? g(lutA) : 0) +
               g(tile_ll) + g(tile_stats) + g(seg_ready) + g(seg_ll) + g(Pseg) + g(recs) + (grp_sums ? g(grp_sums) : 0) +
               (chunk_ll ? g(chunk_ll) : 0) + (rw_stats ? g(rw_stats) : 0);
    }
};
static ShadowSizes shadow_sizes(const hf_ctx* ctx) {
    ShadowSizes z{};
    const size_t C = (size_t) ctx->C, V = (size_t) ctx->V, nt = (size_t) ctx->ntiles, ns = (size_t) ctx->nseg;
    const size_t rows = (size_t) ctx->n_lut + (size_t) ctx->n_slow + 1;
    z.label = (size_t) ctx->N + 16; z.chunk_stats = C * V * 8; z.total = (V + 1) * 8; z.params = ctx->params_bytes;
    z.lutE = rows * 16 * 8; z.lutC = rows * 4 * (size_t) ctx->K * 8;
    z.lutA = ctx->d_lutA ? ((size_t) ctx->n_arows + 1) * 16 * 8 : 0;
    z.tile_ll = nt * 8; z.tile_stats = nt * (size_t) ctx->R * (16 + 9 + 2 + 3 * 16 + 1) * 8;
    z.seg_ready = ns * 4; z.seg_ll = ns * 8; z.Pseg = ns * 16 * 8;
    int64_t cap = 0;
    for (const auto& sb : ctx->subs) if (sb.p1 - sb.p0 > cap) cap = sb.p1 - sb.p0;
    z.recs = (size_t) (cap + 1) * 64;
    z.grp_sums = ctx->d_grp_sums ? (size_t) ((ctx->n_groups + 3) / 4 * 4) * 16 * 8 : 0;
    z.chunk_ll = ctx->d_chunk_ll ? C * 8 : 0;
    z.rw_stats = ctx->d_rw_stats ? (size_t) ctx->n_rowwaves * (16 + 9 + 2 + 3 * 16 + 1) * 8 : 0;
    return z;
}
// + what a shadow allocates later on its own: the pinned result block and, in rows mode, the pinned partials (host memory)
static size_t shadow_device_bytes(const hf_ctx* ctx) { return shadow_sizes(ctx).sum(); }

static void shadow_free(hf_ctx* s) {
    if (!s) return;
    hipSetDevice(s->device);
    // the lazily allocated arrays of a shadow (hf_get_forward_backward's, the two-launch lane products), then its slabs
    ctx_free(s, s->d_segQ); ctx_free(s, s->d_scale_s); ctx_free(s, s->d_slot_of);
    if (s->h_part) hipHostFree(s->h_part);
    if (s->h_label) pin_cache().release(reinterpret_cast<char*>(s->h_label));
    if (s->ev0) hipEventDestroy(s->ev0);
    if (s->ev1) hipEventDestroy(s->ev1);
    for (auto& sl : s->slabs) hipFree(sl.first);
    if (s->h_total) { hipDeviceSynchronize(); pin_cache().release(reinterpret_cast<char*>(s->h_total)); }
    delete s;
}

// a shadow of `ctx`: its model-independent members shared, its pass state its own (zeroed where hf_create zeroes it)
static int shadow_create(const hf_ctx* ctx, hf_ctx** out) {
    *out = nullptr;
    hf_ctx* s = new hf_ctx(*ctx);
    s->slabs.clear(); s->slab_cur = nullptr; s->slab_left = 0;
    s->vit = hf_ctx::Viterbi{};
    s->d_E = nullptr; s->d_f = nullptr; s->d_b = nullptr; s->d_scale = nullptr;
    s->d_nbE = s->d_nbP = s->d_nbDig = s->d_nbR = s->d_nbBeta = s->d_tile_hist = nullptr;
    for (int b = 0; b < 2; b++) { s->h_nb[b] = nullptr; s->nb_ev[b] = nullptr; s->nb_ev_used[b] = false; }
    s->d_slot_h = nullptr; s->d_H = nullptr;
    s->d_segQ = nullptr; s->d_scale_s = nullptr; s->d_slot_of = nullptr; s->d_recs_all = nullptr;
    s->h_part = nullptr; s->d_part_host = nullptr; s->part_cap = 0;
    s->h_label = nullptr; s->d_label_host = nullptr;
    s->h_total = nullptr; s->h_flags = nullptr; s->h_params = nullptr; s->d_total_host = nullptr;
    s->ev0 = s->ev1 = nullptr; s->ev_valid = false;
    for (int i = 0; i < 2 * HF_NKERNELS; i++) s->kev[i] = nullptr;
    for (int i = 0; i < HF_NKERNELS; i++) { s->ksum[i] = 0; s->kcount[i] = 0; s->klast[i] = 0; s->klast_ok[i] = false; s->kran[i] = false; }
    s->prof_mask = 0; s->prof_stride = 1; s->prof_pass = 0; s->prof_now = true;
    s->host_trace = false; s->ht_n = 0;
    s->d_rank_out = nullptr; s->d_rank_flag = nullptr; s->pass_bound = false;
    s->own_chunk_stats = true;
    s->d_seg_trace = nullptr;
    s->seg_epoch = 0; s->poll_seq = 0.0; s->stream_stamp = 0;
    s->have_full = false; s->fb_recs = false; s->recs_all = false; s->scales_all = false; s->pass_seg = false; s->pass_rows = false;
    s->launch_failed = false; s->last_stream = nullptr;
    // (everything below is null until allocated: shadow_free must not free the context's arrays)
    s->d_label = nullptr; s->d_chunk_stats = nullptr; s->d_total = nullptr; s->d_flags = nullptr; s->d_done = nullptr; s->d_cks = nullptr;
    s->d_params = nullptr; s->d_lutE = s->d_lutC = s->d_Es = s->d_Cs = nullptr; s->d_lutA = nullptr; s->d_tile_ll = nullptr; s->d_tile_stats = nullptr;
    s->d_seg_ready = nullptr; s->d_seg_ll = nullptr; s->d_Pseg = nullptr; s->d_recs = nullptr; s->d_grp_sums = nullptr; s->d_chunk_ll = nullptr;
    s->d_rw_stats = nullptr;
    const ShadowSizes z = shadow_sizes(ctx);
    s->slab_first = z.sum();
    bool ok = true;
    auto take = [&](size_t bytes) -> void* { void* p = ok ? ctx_alloc(s, bytes) : nullptr; if (!p) ok = false; return p; };
#define SALLOC(field, bytes) s->field = static_cast<decltype(s->field)>(take(bytes))
    SALLOC(d_label, z.label); SALLOC(d_chunk_stats, z.chunk_stats); SALLOC(d_total, z.total); SALLOC(d_flags, 4);
    SALLOC(d_done, HF_DONE_BYTES); SALLOC(d_cks, 8); SALLOC(d_params, z.params);
    SALLOC(d_lutE, z.lutE); SALLOC(d_lutC, z.lutC);
    if (z.lutA) SALLOC(d_lutA, z.lutA);
    SALLOC(d_tile_ll, z.tile_ll); SALLOC(d_tile_stats, z.tile_stats);
    SALLOC(d_seg_ready, z.seg_ready); SALLOC(d_seg_ll, z.seg_ll); SALLOC(d_Pseg, z.Pseg); SALLOC(d_recs, z.recs);
    if (z.grp_sums) SALLOC(d_grp_sums, z.grp_sums);
    if (z.chunk_ll) SALLOC(d_chunk_ll, z.chunk_ll);
    if (z.rw_stats) SALLOC(d_rw_stats, z.rw_stats);
#undef SALLOC
    if (!ok) { (void) hipGetLastError(); shadow_free(s); return set_err(HF_E_HIP, "hf_batch_create: out of device memory"); }
    s->d_Es = s->d_lutE + (size_t) ctx->n_lut * 16;
    s->d_Cs = s->d_lutC + (size_t) ctx->n_lut * 4 * (size_t) ctx->K;
    s->d_recs_all = s->d_recs;                                   // (one sub-pass: the pass buffer holds every window's records)
    s->tabwork.lutE = s->d_lutE; s->tabwork.lutC = s->d_lutC; s->tabwork.lutA = ctx->tabwork.lutA ? s->d_lutA : nullptr;
    {   // the pinned block: result vector (+ flag word, stamp, checksums) | flag word | parameter block, as hf_create lays it out
        const size_t tot_bytes = (((size_t) ctx->V + 2 + HF_MAXREGIONS) * 8 + 63) / 64 * 64;
        const size_t par_bytes = (ctx->params_bytes + 63) / 64 * 64;
        char* pin = pin_cache().acquire(tot_bytes + 64 + par_bytes);
        if (!pin) { shadow_free(s); return set_err(HF_E_HIP, "hf_batch_create: out of host memory"); }
        std::memset(pin, 0, tot_bytes + 64 + par_bytes);
        s->h_total = reinterpret_cast<double*>(pin);
        s->h_flags = reinterpret_cast<unsigned*>(pin + tot_bytes);
        s->h_params = reinterpret_cast<DevParams*>(pin + tot_bytes + 64);
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, s->h_total, 0) == hipSuccess) s->d_total_host = (double*) dp;
        else { (void) hipGetLastError(); s->d_total_host = nullptr; s->stream_stamp_ok = false; }
    }
    if (hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess) {
        (void) hipGetLastError(); shadow_free(s); return set_err(HF_E_HIP, "hf_batch_create: events");
    }
    // what hf_create zeroes; the identity row behind the rows of A (no kernel writes it) comes from the context
    bool z_ok = hipMemset(s->d_flags, 0, 4) == hipSuccess && hipMemset(s->d_done, 0, HF_DONE_BYTES) == hipSuccess &&
                hipMemset(s->d_cks, 0, 8) == hipSuccess && hipMemset(s->d_params, 0, z.params) == hipSuccess &&
                hipMemset(s->d_label, 0xff, (size_t) (ctx->N ? ctx->N : 1)) == hipSuccess &&
                hipMemset(s->d_seg_ready, 0, z.seg_ready ? z.seg_ready : 4) == hipSuccess;
    if (z_ok && z.lutA) z_ok = hipMemcpy(s->d_lutA, ctx->d_lutA, z.lutA, hipMemcpyDeviceToDevice) == hipSuccess;
    if (!z_ok) { const hipError_t e = hipGetLastError(); shadow_free(s); return set_err(HF_E_HIP, std::string("hf_batch_create: ") + hipGetErrorString(e)); }
    *out = s;
    return HF_OK;
}

extern "C" {

int hf_batch_capacity(const hf_ctx* ctx) {
    if (batch_refusal(ctx)) return 0;
    if (hipSetDevice(ctx->device) != hipSuccess) { (void) hipGetLastError(); return 0; }
    size_t fr = 0, total = 0;
    if (hipMemGetInfo(&fr, &total) != hipSuccess) { (void) hipGetLastError(); return 0; }
    const size_t per = shadow_device_bytes(ctx) + ((size_t) 1 << 20);   // (+ a slab's worth of slack per model)
    size_t n = (fr / 10 * 9) / per;                                       // nine tenths of what is free
    // and the PINNED host memory a model takes: its result block, the label staging of its first hf_batch_get_labels and the row-statistics
    // partials that the host sums — at most an eighth of the host's physical memory for the whole batch
    const size_t pin = (((size_t) ctx->V + 2 + HF_MAXREGIONS) * 8 + 64 + ctx->params_bytes + 192) + ((size_t) ctx->N + 16) +
                       ((size_t) ctx->n_rowwaves * (16 + 9 + 2 + 3 * 16 + 1) + (size_t) ctx->C + 65) * 8;
    const long pages = sysconf(_SC_PHYS_PAGES), psz = sysconf(_SC_PAGESIZE);
    if (pages > 0 && psz > 0) n = std::min(n, (size_t) pages * (size_t) psz / 8 / pin);
    return (int) std::min<size_t>(n, HF_BATCH_MAX_MODELS);
}

int hf_batch_create(hf_ctx* ctx, int n_models, hf_batch** out) {
    if (!out) return set_err(HF_E_ARG, "hf_batch_create: bad argument");
    *out = nullptr;
    if (const char* why = batch_refusal(ctx)) return set_err(HF_E_ARG, std::string("hf_batch_create: ") + why);
    if (n_models < 1 || n_models > HF_BATCH_MAX_MODELS) return set_err(HF_E_ARG, "hf_batch_create: n_models must be 1 .. HF_BATCH_MAX_MODELS");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());                    // (the context's uploads and k_setup: the shadows copy the identity row of A)
    hf_batch* b = new hf_batch();
    b->ctx = ctx;
    for (int i = 0; i < n_models; i++) {
        hf_ctx* s = nullptr;
        const int rc = shadow_create(ctx, &s);
        if (rc) { for (hf_ctx* t : b->m) shadow_free(t); delete b; return rc; }
        b->m.push_back(s);
    }
    {   // the pointer table of k_seg_fb_batch: one row per model, written once
        std::vector<SegFbModel> tab((size_t) n_models);
        for (int i = 0; i < n_models; i++) {
            const hf_ctx* s = b->m[(size_t) i];
            SegFbModel& t = tab[(size_t) i];
            t.lutA = s->d_lutA; t.P = s->d_params; t.Qs = nullptr; t.Pseg = s->d_Pseg; t.ready = s->d_seg_ready;
            t.recs = s->d_recs; t.scale_s = nullptr; t.label = s->d_label; t.seg_ll = s->d_seg_ll; t.flags = s->d_flags;
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
    if (b->d_tab) { hipSetDevice(b->ctx->device); hipDeviceSynchronize(); hipFree(b->d_tab); }
    for (hf_ctx* s : b->m) shadow_free(s);
    delete b;
}

int hf_batch_size(const hf_batch* b) { return b ? (int) b->m.size() : 0; }
int hf_batch_shared_models(const hf_batch* b) { return b ? b->last_batched : 0; }

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
    HIPCHK(hipSetDevice(b->ctx->device));
    b->last.clear();
    b->last_batched = 0;
    // The shared launch covers full passes of models in one-launch mode with statistics by emission row and one sub-pass (the default
    // pass): tables per model, ONE k_seg_fb_batch over all of them, then per model k_pair_sums and k_row_stats.  A model that has fallen
    // back to two launches (a timed-out hand-off), a forward-only pass or the per-chunk statistics run the model's whole pass on its own.
    std::vector<int> joint;
    for (int i = 0; i < n_active; i++) {
        hf_ctx* s = b->m[(size_t) models[i]];
        rc = pack_params(s, &p[i]);
        if (rc) return rc;
        s->last_p = p[i]; s->last_mode = mode; s->last_stream = st;
        const bool shared = mode == HF_MODE_FULL && s->seg_fused && rows_pass(s) && s->subs.size() == 1 && s->C > 0 && s->ntiles > 0;
        rc = enqueue_pass(s, &p[i], mode, st, false, shared ? PASS_PRE : PASS_ALL);
        if (rc) return rc;
        if (shared) joint.push_back(i);
    }
    if (!joint.empty()) {
        const hf_ctx* c0 = b->m[(size_t) models[joint[0]]];
        const int32_t* const sob = c0->d_seg_of_block;
        const auto& sb = c0->subs[0];
        const int g0 = sob ? sb.b0 : sb.seg0, nblk = sob ? sb.b1 - sb.b0 : sb.seg1 - sb.seg0;
        const int nc = c0->seg_nc;
        const size_t lds = seg_lds_bytes(nc);
        if (nc > 0 && lds > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_seg_fb_batch<true, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess)
            HIPCHK(hipGetLastError());
        for (size_t j0 = 0; j0 < joint.size() && nblk > 0; j0 += HF_SEG_BATCH_MAX) {
            const size_t nj = std::min<size_t>(HF_SEG_BATCH_MAX, joint.size() - j0);
            SegFbBatch bt{};
            for (size_t j = 0; j < nj; j++) {
                const int i = joint[j0 + j];
                hf_ctx* s = b->m[(size_t) models[i]];
                const unsigned epoch = ++s->seg_epoch;
                bt.model[j] = models[i];
                bt.epoch[j] = epoch;
                bt.wait_epoch[j] = (s->seg_test_timeout && epoch == 1) ? 0xffffffffu : epoch;
            }
            const dim3 grid((unsigned) nblk, (unsigned) nj);
            if (nc > 0) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_seg_fb_batch<true, true, true>), grid, dim3(64), lds, st, c0->d_seg, c0->d_arow, b->d_tab, bt,
                                           c0->d_pos, (int32_t) g0, nc, sob);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_seg_fb_batch<true, true, false>), grid, dim3(64), lds, st, c0->d_seg, c0->d_arow, b->d_tab, bt,
                                    c0->d_pos, (int32_t) g0, nc, sob);
            HIPCHK(hipGetLastError());
        }
        for (int i : joint) {
            rc = enqueue_pass(b->m[(size_t) models[i]], &p[i], mode, st, false, PASS_POST);
            if (rc) return rc;
        }
        b->last_batched = (int) joint.size();
    }
    for (int i = 0; i < n_active; i++) {
        hf_ctx* s = b->m[(size_t) models[i]];
        s->have_full = (mode == HF_MODE_FULL);
        b->last.push_back(models[i]);
    }
    return HF_OK;
}

int hf_batch_finish(hf_batch* b, double* stats_host, int32_t* status, void* stream) {
    if (!b || (!b->last.empty() && (!stats_host || !status))) return set_err(HF_E_ARG, "hf_batch_finish: bad argument");
    const int64_t V = b->ctx->V;
    const std::vector<int32_t> act = b->last;
    b->last.clear();
    for (size_t i = 0; i < act.size(); i++) {
        // a model's own failure (HF_E_SCALE, HF_E_NAN, HF_E_REGION) goes to its status word and the batch goes on; a failure of the
        // runtime or of the arguments ends the call
        const int r = hf_finish(b->m[(size_t) act[i]], stats_host + i * (size_t) V, stream);
        status[i] = r;
        if (r == HF_E_HIP || r == HF_E_ARG) return r;
    }
    return HF_OK;
}

int hf_batch_get_labels(hf_batch* b, int model, int8_t* labels_host) {
    if (!b || model < 0 || model >= (int) b->m.size()) return set_err(HF_E_ARG, "hf_batch_get_labels: bad argument");
    return hf_get_labels(b->m[(size_t) model], labels_host);
}

int hf_batch_get_posterior(hf_batch* b, int model, int64_t first, int64_t n, double* post_host) {
    if (!b || model < 0 || model >= (int) b->m.size()) return set_err(HF_E_ARG, "hf_batch_get_posterior: bad argument");
    return hf_get_posterior(b->m[(size_t) model], first, n, post_host);
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
    const size_t V = (size_t) b->ctx->V;
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
