// hf_estep.hip — MI355X (gfx950) E-step of HMM-Flagger: the host side of the C ABI (include/hmm_flagger_hip.h), the
// context, the one-time set-up kernels and the launch sequence of a pass; the kernels of a pass live in the headers below.
//
// Replaces EM_runOneIterationForList / EM_runForwardForList (programs/submodules/hmm/hmm.c:739,790).
// One pass (per EM iteration), HF_ALGO_SCAN:
//   hf_scan.h    k_tables      emission rows of this iteration (per occurring (region, x, x_prev) + per contig-end window)
//                              and the rows of A_t = T_t∘e_t           (hmm_utils.c:753-793, 941-947, 2278-2292)
//   hf_seg.h     k_seg_fb      one workgroup per chunk segment, ONE launch: lane products of A_t, scans, the segments' products
//                              handed over inside the launch, scaled forward + log-likelihood, scaled backward + posterior
//                              argmax, pair records   (k_seg_prod + k_seg_fb<., false>: the two-launch fall-back)
//                                                                        (hmm.c:333-434, 452-545, 671-692)
//   hf_rows.h    k_pair_sums / k_pair_sums_compact, k_row_stats (its last blocks sum the pass's total): xi sufficient statistics summed by emission row (default)
//                                                                        (hmm.c:563-650, hmm_utils.c:812-839, 1027-1034)
//   hf_chunks.h  k_stats_tile, k_chunk_stats, k_reduce: the same statistics as one vector per chunk, summed in chunk-list
//                order (hmm.c:759-763) — HF_STATS_CHUNKS, the per-chunk multi-GPU exchange, HF_ALGO_SEQ
//   hf_nb.h, hf_nb_rows.h   the negative_binomial model's tables and count data (per chunk / by emission row)
//   hf_seq.h     HF_ALGO_SEQ, an independent on-device check: k_emit_rows (direct evaluation of every window's row),
//                k_fwd_seq / k_bwd_seq (one wavefront per chunk, sequential recurrences)
// There is no CPU fallback: without a HIP device hf_create fails with HF_E_NOGPU.
//
// The library is five translation units over one host header (hf_host.h: the slab, the track, the pass and decoder states, the context,
// what crosses a unit boundary):
//   hf_estep.hip     this one: host pool and pinned cache, hf_create.h, the pass, hf_finish and the exchange entry points, the lazy getters
//                    of the pass (hf_get_labels / _posterior / _forward_backward), profiling, self-tests, hf_batch.h; at its end
//                    hf_getters.h: the range getters and the alpha statistics, host side and kernels (hf_view.h, hf_interval.h,
//                    hf_alpha.h, hf_moments.h, hf_runs.h, hf_entropy.h, hf_breakpoint.h, hf_longrun.h; rg_check, pass_view for every unit)
//   hf_decoders.hip  hf_decode.h, hf_viterbi.h, hf_sample.h: hf_viterbi*, hf_sample_*
//   hf_minlen.hip    the minimum-run-length family: hf_minlen*.h, hf_mea.h
//   hf_runlen.hip    the block-length spectrum hf_get_run_lengths (its host-only stitch: hf_runlen_stitch.h)
//   hf_countdist.hip the distribution of label totals hf_get_count_distribution (its host-only stitch: hf_countdist_stitch.h)
// Every kernel is compiled in exactly one of them; the other units reach this unit's kernels through launch_tables, launch_chunk_stats
// and launch_reduce.  The units with range getters share hf_rg.h (static templates: the batch loop over hf_jobs.h, scratch layout, caps).
#include "hf_host.h"

thread_local std::string g_err;

// hf_create's host loops over the windows are independent per chunk: run fn(first chunk, last chunk + 1, part) on up to
// HF_PARTS threads, the chunk list cut into parts of about equal window count (1.5 M windows: 6-8 ms per loop on one thread).
// The threads are a process-wide pool (hf_warmup starts it): spawning 16 threads per loop was measured at 1-2 ms a loop, as much
// as the loops themselves.  A caller that finds the pool busy (hf_multi's ranks create their contexts concurrently) spawns its own.
constexpr size_t HF_PARTS = 64;      // parts at most; host_threads() of them are used
namespace {
struct HostPool {
    std::mutex run_m, m;
    std::condition_variable cv;
    std::vector<std::thread> th;
    const std::function<void(size_t)>* job = nullptr;
    size_t gen = 0, parts = 0;
    std::atomic<size_t> next{0}, done{0}, active{0};
    bool stop = false;
    void start(size_t n) {
        std::lock_guard<std::mutex> g(m);
        while (th.size() < n) th.emplace_back([this] { worker(); });
    }
    void worker() {
        size_t seen = 0;
        for (;;) {
            const std::function<void(size_t)>* f;
            size_t P;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen; f = job; P = parts;
                if (!f) continue;                      // woke after the job was over
                active.fetch_add(1, std::memory_order_relaxed);   // under m: run() does not reuse the counters while a worker holds a job
            }
            for (size_t k; (k = next.fetch_add(1, std::memory_order_relaxed)) < P;) { (*f)(k); done.fetch_add(1, std::memory_order_release); }
            active.fetch_sub(1, std::memory_order_release);
        }
    }
    // f(k) for k = 0..P-1 on the caller and up to `workers` pool threads (parts are handed out one at a time: a thread that wakes late
    // takes fewer); false if another caller holds the pool
    bool run(size_t P, const std::function<void(size_t)>& f, size_t workers) {
        std::unique_lock<std::mutex> only(run_m, std::try_to_lock);
        if (!only.owns_lock()) return false;
        start(std::min(workers, P - 1));
        next.store(0); done.store(0);
        { std::lock_guard<std::mutex> g(m); job = &f; parts = P; gen++; }
        cv.notify_all();
        for (size_t k; (k = next.fetch_add(1, std::memory_order_relaxed)) < P;) { f(k); done.fetch_add(1, std::memory_order_release); }
        while (done.load(std::memory_order_acquire) < P) std::this_thread::yield();
        { std::lock_guard<std::mutex> g(m); job = nullptr; parts = 0; }   // a worker that wakes from here on leaves the counters alone
        while (active.load(std::memory_order_acquire) != 0) std::this_thread::yield();
        return true;
    }
    ~HostPool() {
        { std::lock_guard<std::mutex> g(m); stop = true; }
        cv.notify_all();
        for (auto& t : th) t.join();
    }
};
HostPool& host_pool() { static HostPool p; return p; }

// Pinned staging buffers of hf_create, kept for the life of the process (round 5): pinning costs ~0.2 ms per MB (1.2-1.3 ms of a 7 ms
// hf_create on BASELINE configs[2]) and un-pinning as much again on a helper thread.  A context takes the smallest free buffer that
// is large enough, or a new one (a free smaller one is given back first); hf_warmup pins a first set while the input loads.
struct PinCache {
    struct Slot { char* p = nullptr; size_t cap = 0; bool busy = false, pinned = false; };
    std::mutex m;
    std::vector<Slot> slots;
    char* try_acquire(size_t bytes) {                     // a cached buffer, or nullptr
        std::lock_guard<std::mutex> g(m);
        int best = -1;
        for (size_t i = 0; i < slots.size(); i++)
            if (!slots[i].busy && slots[i].cap >= bytes && (best < 0 || slots[i].cap < slots[(size_t) best].cap)) best = (int) i;
        if (best < 0) return nullptr;
        slots[(size_t) best].busy = true;
        return slots[(size_t) best].p;
    }
    char* acquire(size_t bytes) {                         // ... or a new one (pinned when possible; nullptr: out of host memory)
        if (char* p = try_acquire(bytes)) return p;
        Slot s;
        s.cap = bytes + bytes / 8 + 4096;
        {   // make room: one free buffer that was too small goes back
            std::lock_guard<std::mutex> g(m);
            for (size_t i = 0; i < slots.size(); i++)
                if (!slots[i].busy) { if (slots[i].pinned) (void) hipHostFree(slots[i].p); else std::free(slots[i].p); slots.erase(slots.begin() + (long) i); break; }
        }
        // Portable AND coherent: with a non-zero flag word and no Coherent / Mapped bit the runtime lets HIP_HOST_COHERENT decide, and
        // its default is non-coherent — the kernels' zero-copy writes into the result block (totals, partial vectors, labels) would then be visible
        // at the end of the kernel only.  Plain flags as the fall-back, pageable memory as the last one
        // (a context whose result block is not device-addressable completes its passes through a copy: create_device_store).
        if (hipHostMalloc((void**) &s.p, s.cap, hipHostMallocPortable | hipHostMallocCoherent) == hipSuccess) s.pinned = true;
        else if ((void) hipGetLastError(), hipHostMalloc((void**) &s.p, s.cap, hipHostMallocDefault) == hipSuccess) s.pinned = true;
        else { (void) hipGetLastError(); s.p = (char*) std::malloc(s.cap); }
        if (!s.p) return nullptr;
        s.busy = true;
        std::lock_guard<std::mutex> g(m);
        slots.push_back(s);
        return s.p;
    }
    void release(char* p) {
        if (!p) return;
        std::lock_guard<std::mutex> g(m);
        for (auto& s : slots) if (s.p == p) s.busy = false;
    }
};
PinCache& pin_cache() { static PinCache* c = new PinCache(); return *c; }   // (never destroyed: the process leaves without unwinding HIP)

// Validity masks of hmm_utils.c:2229-2254 by THRESHOLD per coverage value (every value below 256): the ratio v / (0.1 + cv) is monotone in v,
// so "Dup valid" = !(ratio > max_mapq) holds for v up to a largest value, "Col valid" = !(ratio < min_mapq) and "End valid" = !(ratio <
// min_clip) from a smallest value on — found with window_record's own divisions and comparisons, once per set of thresholds; the first pass
// of hf_create then needs three byte-sized table entries of its window's coverage (768 bytes: L1) instead of two divisions.
struct ValidityLut {
    double max_mapq = -1.0, min_mapq = -1.0, min_clip = -1.0;
    uint16_t dup_le[256], col_ge[256], end_ge[256];     // Dup valid iff mq <= dup_le[cv] (0xffff: never... see below); Col iff mq >= col_ge[cv]; End iff cp >= end_ge[cv]
    bool monotone = true;                               // (false: a NaN threshold or the like broke the monotone pattern — hf_create then takes window_record everywhere)
};
std::shared_ptr<const ValidityLut> validity_lut(double max_mapq, double min_mapq, double min_clip) {
    static std::mutex mu;
    static std::shared_ptr<const ValidityLut> cached;
    std::lock_guard<std::mutex> g(mu);
    if (cached && cached->max_mapq == max_mapq && cached->min_mapq == min_mapq && cached->min_clip == min_clip) return cached;
    auto L = std::make_shared<ValidityLut>();
    L->max_mapq = max_mapq; L->min_mapq = min_mapq; L->min_clip = min_clip;
    for (unsigned cv = 0; cv < 256; cv++) {
        int n_dup = 0, n_col = 0, n_end = 0;            // values v for which the bit is set; then check that they form a prefix / suffixes
        bool dup[256], col[256], end[256];
        for (unsigned v = 0; v < 256; v++) {
            const double ratio = (double) v / (0.1 + cv);                 // window_record's own expressions
            dup[v] = !(ratio > max_mapq); col[v] = !(ratio < min_mapq); end[v] = !(ratio < min_clip);
            n_dup += dup[v]; n_col += col[v]; n_end += end[v];
        }
        for (unsigned v = 0; v < 256; v++)
            if (dup[v] != ((int) v < n_dup) || col[v] != ((int) v >= 256 - n_col) || end[v] != ((int) v >= 256 - n_end)) L->monotone = false;
        L->dup_le[cv] = (uint16_t) (n_dup - 1 < 0 ? 0xffff : n_dup - 1);   // 0xffff: no value is valid (compared as signed below)
        L->col_ge[cv] = (uint16_t) (256 - n_col);                          // 256: no value
        L->end_ge[cv] = (uint16_t) (256 - n_end);
    }
    cached = L;
    return cached;
}
}
// threads of hf_create's passes over the windows: 16 (what rounds 2-4 used), fewer on a smaller host; HF_HOST_THREADS=n (<= 64) overrides
static size_t host_threads() {
    static const size_t n = [] {
        const unsigned hw = std::thread::hardware_concurrency();
        size_t t = std::min<size_t>(16, hw ? hw : 1);
        if (const char* e = std::getenv("HF_HOST_THREADS")) { const int v = std::atoi(e); if (v >= 1) t = std::min<size_t>((size_t) v, HF_PARTS); }
        return t;
    }();
    return n;
}
template <class Fn>
static void par_chunks(const int64_t* chunk_off, size_t C, Fn fn, size_t parts_per_thread = 4) {
    const unsigned hw = std::thread::hardware_concurrency();
    (void) hw;
    // Round 6: FOUR parts per thread, handed out dynamically (HostPool::run), instead of one static part each — on a box the driver leased
    // fresh, hf_create took 8.35 ms against 2.9-4.3 on others: a pass over the windows lasted as long as the thread that woke last.  Parts stay
    // consecutive chunk ranges in order (what the slow-window lists and the plan's per-part ranks rely on), and the cut depends on the chunk
    // list and the thread count only: the second and third pass of hf_create see the same parts.
    const size_t NT = C < 16 ? 1 : std::min<size_t>(host_threads(), C);
    if (NT <= 1) { fn((size_t) 0, C, (size_t) 0); return; }
    const size_t T = std::min<size_t>(std::min<size_t>(HF_PARTS, parts_per_thread * NT), C);
    std::vector<size_t> cut(T + 1, 0);
    const int64_t total = chunk_off[C] - chunk_off[0];
    size_t c = 0;
    for (size_t k = 1; k < T; k++) {
        const int64_t target = chunk_off[0] + total * (int64_t) k / (int64_t) T;
        while (c < C && chunk_off[c] < target) c++;
        cut[k] = c;
    }
    cut[T] = C;
    // HF_PARTS_TRACE=1 (profiles/tools): when every part started and ended, and on which thread — how late the pool's threads wake
    static const bool ptrace = std::getenv("HF_PARTS_TRACE") != nullptr;
    struct PartLog { double t0, t1; size_t tid; };
    std::vector<PartLog> plog(ptrace ? T : 0);
    const auto pstart = std::chrono::steady_clock::now();
    const std::function<void(size_t)> part = [&](size_t k) {
        if (!ptrace) { fn(cut[k], cut[k + 1], k); return; }
        const double a = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - pstart).count();
        fn(cut[k], cut[k + 1], k);
        plog[k] = {a, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - pstart).count(),
                   std::hash<std::thread::id>()(std::this_thread::get_id()) % 997};
    };
    struct PartDump {
        const std::vector<PartLog>& l; bool on;
        ~PartDump() {
            if (!on) return;
            std::fprintf(stderr, "[parts]");
            for (size_t k = 0; k < l.size(); k++) std::fprintf(stderr, " %zu:t%zu:%.0f-%.0f", k, l[k].tid, l[k].t0, l[k].t1);
            std::fprintf(stderr, " us\n");
        }
    } pdump{plog, ptrace};
    if (host_pool().run(T, part, NT - 1)) return;
    std::atomic<size_t> next{0};                       // the pool is busy (hf_multi's ranks create their contexts concurrently): threads of our own
    auto work = [&] { for (size_t k; (k = next.fetch_add(1, std::memory_order_relaxed)) < T;) part(k); };
    std::vector<std::thread> th;
    for (size_t k = 1; k < NT; k++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
}
// slot of a segment's x-th window: lane x / L holds it as its x % L-th (hf_seg.h)
static inline int32_t seg_slot(const SegDesc& d, int64_t x) { return d.slot0 + (int32_t) ((x % d.L) * 64 + x / d.L); }

// ------------------------------------------------------------------------------------------
// setup: packed records + contig-end factor beta (hmm.c:301-316), once per run
// ------------------------------------------------------------------------------------------
// packed != nullptr: the four per-window inputs as one word cov | mapq << 8 | clip << 16 | region << 24 (hf_create packs them on the
// host when every value fits a byte — window values are at most 250, chunk.c:393-441: a quarter of the bytes to upload)
// The packed record of one window (hf_device.h REC_*) and its beta: ONE function for the device (k_setup) and for the host
// (hf_create's plan reads the same bits without fetching them back; -ffp-contract=off on both sides, plain IEEE divisions and
// comparisons, so the two agree bit for bit -- HF_CREATE_VERIFY=1, set by the test suite, downloads the device's and compares).
__host__ __device__ static inline uint32_t window_record(unsigned cv, unsigned mq, unsigned cp, unsigned region, unsigned pre_region,
                                                         int64_t col, int s, int e, int ctg_len, int window_len, int mean_read_len,
                                                         int adjust, double min_frac, double max_mapq, double min_mapq,
                                                         double min_clip, double beta_star, double* beta_out) {
    // validity mask, hmm_utils.c:2229-2254
    const double ratio_m = (double) mq / (0.1 + cv);
    const double ratio_c = (double) cp / (0.1 + cv);
    unsigned vm = 0;
    if (!(ratio_m > max_mapq)) vm |= 1u;  // Dup valid
    if (!(ratio_m < min_mapq)) vm |= 2u;  // Col valid
    if (!(ratio_c < min_clip)) vm |= 4u;  // End/Msj column valid
    uint32_t r = (cv & 0xffu) | (region << 8) | (vm << 16);
    if (col == 0) r |= 1u << 19;
    else if (pre_region != region) r |= 1u << 20;
    // beta, hmm.c:301-316; min/max are the int functions of common.c:142-148
    double bt = 1.0;
    if (adjust) {
        const int icol = (int) col;
        const int a1 = (int) (s + (double) window_len * (icol + 0.5));
        const int a2 = (int) ((s + (double) window_len * icol + e) / 2);
        const int mid = a1 < a2 ? a1 : a2;
        const int L = mean_read_len;
        const int l1 = mid - L + 1, l2 = (int) (-(1 - min_frac) * L);
        const int l = l2 < l1 ? l1 : l2;
        const int u2 = (int) (ctg_len - min_frac * L);
        const int u = mid < u2 ? mid : u2;
        bt = (double) (u - l) / L;
        if (bt <= 0.25) bt = 0.25;
    }
    *beta_out = bt;
    if (col == 0 || bt != beta_star) r |= 1u << 21;   // private emission row (REC_SLOW)
    return r;
}

__global__ void k_setup(const int64_t* __restrict__ off, const uint32_t* __restrict__ packed, const uint16_t* __restrict__ cov,
                        const uint16_t* __restrict__ mapq, const uint16_t* __restrict__ clip,
                        const uint64_t* __restrict__ annot, const int32_t* __restrict__ cs,
                        const int32_t* __restrict__ ce, const int32_t* __restrict__ cl, int window_len,
                        int mean_read_len, int adjust, double min_frac, double max_mapq, double min_mapq,
                        double min_clip, int n_regions, double beta_star, uint32_t* __restrict__ rec,
                        double* __restrict__ beta, unsigned* __restrict__ flags) {
    const int c = blockIdx.y;
    const int64_t t0 = off[c], T = off[c + 1] - t0;
    const int64_t col = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= T) return;
    const int64_t t = t0 + col;
    const uint32_t pw = packed ? packed[t] : 0u;
    const unsigned cv = packed ? (pw & 0xffu) : cov[t];
    const unsigned mq = packed ? ((pw >> 8) & 0xffu) : mapq[t], cp = packed ? ((pw >> 16) & 0xffu) : clip[t];
    const unsigned region = packed ? (pw >> 24) : (unsigned) ((annot[t] & 0xFC00000000000000ULL) >> 58);
    if ((int) region >= n_regions) atomicOr(flags, HF_FLAG_REGION);
    unsigned pre_region = region;
    if (col > 0) pre_region = packed ? (packed[t - 1] >> 24) : (unsigned) ((annot[t - 1] & 0xFC00000000000000ULL) >> 58);
    double bt;
    rec[t] = window_record(cv, mq, cp, region, pre_region, col, cs[c], ce[c], cl[c], window_len, mean_read_len, adjust, min_frac,
                           max_mapq, min_mapq, min_clip, beta_star, &bt);
    beta[t] = bt;
}

__global__ void k_regmask(const int64_t* __restrict__ off, const uint32_t* __restrict__ rec,
                          uint64_t* __restrict__ regmask) {
    const int c = blockIdx.x;
    const int64_t t0 = off[c], T = off[c + 1] - t0;
    unsigned long long m = 0;
    for (int64_t i = threadIdx.x; i < T; i += blockDim.x) m |= 1ull << (REC_REGION(rec[t0 + i]) & 63u);
    for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor(m, o);
    __shared__ unsigned long long sm[16];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long a = 0;
        for (int w = 0; w < (int) (blockDim.x >> 6); w++) a |= sm[w];
        regmask[c] = a;
    }
}

// position of the record that holds every window's forward vector (the getters): the record of the NEXT window of its chunk, the chunk's
// spare record for the last one
__global__ void k_pos_f(const int64_t* __restrict__ off, const int32_t* __restrict__ pos, const int32_t* __restrict__ spare, int32_t* __restrict__ pos_f) {
    const int c = blockIdx.y;
    const int64_t t0 = off[c], T = off[c + 1] - t0;
    const int64_t col = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= T) return;
    pos_f[t0 + col] = col + 1 < T ? pos[t0 + col + 1] : spare[c];
}

#include "hf_scan.h"
#include "hf_seq.h"
#include "hf_nb.h"
#include "hf_chunks.h"
#include "hf_rows.h"
#include "hf_nb_rows.h"
#include "hf_seg.h"


// ------------------------------------------------------------------------------------------
// host side of the C ABI
// ------------------------------------------------------------------------------------------
// the event pair around a whole pass (hf_last_kernel_ms) costs two extra packets per step: only while profiling is on
static bool pass_events(const Pass& ps) {
    return (ps.prof_mask & HF_PROF_PASS) != 0 || ps.host_trace;
}

// small uploads of hf_create: through a pinned staging area when there is room (memcpy + ASYNCHRONOUS copy on the null stream: hf_create
// synchronises once, at its end) — a hipMalloc and a synchronous copy out of pageable memory per array were ~30 us each
struct UploadStage { char* p = nullptr; size_t cap = 0, used = 0; };
static int stage_upload(UploadStage* stg, void* dst, const void* src, size_t bytes) {
    const size_t need = (bytes + 63) & ~(size_t) 63;
    if (stg && stg->p && stg->used + need <= stg->cap) {
        std::memcpy(stg->p + stg->used, src, bytes);
        HIPCHK(hipMemcpyAsync(dst, stg->p + stg->used, bytes, hipMemcpyHostToDevice, nullptr));
        stg->used += need;
    } else HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
template <typename T>
static int dev_upload(Slab& slab, UploadStage& stg, T** dst, const T* src, size_t n) {
    *dst = static_cast<T*>(slab.alloc((n ? n : 1) * sizeof(T)));
    if (!*dst) return set_err(HF_E_HIP, "hf_create: out of device memory");
    return n ? stage_upload(&stg, *dst, src, n * sizeof(T)) : 0;
}

// event pair around one kernel launch, only for the kernels selected by hf_set_profiling
struct KTimer {
    Pass* c; hipStream_t st; int k; bool on;
    KTimer(Pass& c_, hipStream_t s_, int k_) : c(&c_), st(s_), k(k_), on(((c_.prof_mask >> k_) & 1u) && c_.prof_now) {
        if (on) hipEventRecord(c->kev[2 * k], st);
    }
    ~KTimer() { if (on) { hipEventRecord(c->kev[2 * k + 1], st); c->kran[k] = true; } }
};

// (TileGeom, tile_geom: hf_host.h)
#define TILE_GEOM_OR_FAIL(g) do { if (!(g).ok) { set_err(HF_E_ARG, "the per-region tables do not fit the LDS of one workgroup"); ps.launch_failed = true; return; } } while (0)

RowSrc row_src(const Pass& ps) {
    const Track& tr = *ps.tr;
    RowSrc S;
    S.lutE = ps.d_lutE; S.lutC = ps.d_lutC; S.Es = ps.d_Es; S.Cs = ps.d_Cs; S.M = tr.M; S.K = tr.K; S.n_lut = (int) tr.n_lut;
    return S;
}

// where the log-likelihood partials of the last forward pass are: per segment (hf_seg.h) or per tile (hf_scan.h)
static const int32_t* ll_off(const Pass& ps) { return ps.pass_seg ? ps.tr->d_chunk_seg0 : ps.tr->d_chunk_tile0; }
static const double* ll_part(const Pass& ps) { return ps.pass_seg ? ps.d_seg_ll : ps.d_tile_ll; }

// HF_ALGO_SCAN runs the segment kernels (hf_seg.h) whatever the statistics path
static bool seg_pass(const Track& tr) { return tr.algo == HF_ALGO_SCAN && tr.nseg > 0; }

// does a full pass of the Gaussian models take the statistics-by-row path?
static bool rows_pass(const Pass& ps) { return ps.stats_mode == HF_STATS_ROWS && ps.tr->rows_ready && ps.tr->algo == HF_ALGO_SCAN; }

// the groups' sums of f (x) b, times their row of A: padded plan (whole groups streamed) or compact plan (hf_create)
// the groups of ONE sub-pass (Track::SubPass): padded plan — whole groups streamed from the sub-pass's first position on; compact plan — the
// groups' own (global) positions.  recs_eff: the address position 0 would have (a pass buffer that holds one sub-pass starts p0 records later)
static void launch_pair_sums(Pass& ps, hipStream_t st, const Track::SubPass& sb, const double* recs_eff) {
    const Track& tr = *ps.tr;
    const int n = sb.g1 - sb.g0;
    if (n <= 0) return;
    if (tr.plan_compact)
        hipLaunchKernelGGL(k_pair_sums_compact, dim3((unsigned) ((n + 63) / 64)), dim3(256), 0, st, n, tr.d_grp_ar + sb.g0, tr.d_grp_off + sb.g0,
                           tr.d_grp_n + sb.g0, ps.d_lutA, recs_eff, ps.d_grp_sums + (size_t) sb.g0 * 16);
    else
        hipLaunchKernelGGL(k_pair_sums, dim3((unsigned) ((n + 15) / 16)), dim3(256), 0, st, n, tr.d_grp_ar + sb.g0, tr.d_grp_n + sb.g0,
                           ps.d_lutA, recs_eff + sb.p0 * 8, ps.d_grp_sums + (size_t) sb.g0 * 16);
}

// k_seg_fb over the segments [g0, g0 + n) (hf_seg.h); timed: by the dispatch's own start / stop timestamps (hipExtLaunchKernelGGL hands the two
// events to the launch: what rocprofv3 reports for the kernel, without the two marker packets of an event pair around it — those measured 3 us
// more than the kernel and cost the step ~15 us)
// sub >= 0: the segments of that sub-pass; < 0: all segments
static void launch_seg_fb(Pass& ps, hipStream_t st, bool full, double* recs_eff, int sub, unsigned epoch, unsigned wait_epoch, bool timed, bool with_scales = true) {
    const Track& tr = *ps.tr;
    const int g0 = sub >= 0 ? tr.subs[(size_t) sub].seg0 : 0, n = sub >= 0 ? tr.subs[(size_t) sub].seg1 - g0 : tr.nseg;
    if (n <= 0) return;
    const int nc = ps.seg_fused ? tr.seg_nc : 0;     // cached row blocks: one-launch mode only (the lane products are computed in the same kernel)
    const size_t lds = seg_lds_bytes(nc);
#define HF_SEG_FB_ARGS tr.d_seg, tr.d_arow, ps.d_lutA, ps.d_params, ps.d_segQ, ps.d_Pseg, ps.d_seg_ready, epoch, wait_epoch, tr.d_pos, recs_eff, \
                        with_scales ? ps.d_scale_s : (double*) nullptr, ps.d_label, ps.d_seg_ll, ps.d_flags, (int32_t) g0, nc
#define HF_SEG_FB_LAUNCH(B, F, CA) do { \
        if (timed) hipExtLaunchKernelGGL(HIP_KERNEL_NAME(k_seg_fb<B, F, CA>), dim3((unsigned) n), dim3(64), (uint32_t) lds, st, \
                                         ps.kev[2 * HF_K_SEG_FB], ps.kev[2 * HF_K_SEG_FB + 1], 0, HF_SEG_FB_ARGS); \
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_seg_fb<B, F, CA>), dim3((unsigned) n), dim3(64), lds, st, HF_SEG_FB_ARGS); } while (0)
    if (nc > 0) { if (full) HF_SEG_FB_LAUNCH(true, true, true); else HF_SEG_FB_LAUNCH(false, true, true); }
    else if (full) { if (ps.seg_fused) HF_SEG_FB_LAUNCH(true, true, false); else HF_SEG_FB_LAUNCH(true, false, false); }
    else { if (ps.seg_fused) HF_SEG_FB_LAUNCH(false, true, false); else HF_SEG_FB_LAUNCH(false, false, false); }
#undef HF_SEG_FB_LAUNCH
#undef HF_SEG_FB_ARGS
}

// the buffer that holds the records of ALL windows (one sub-pass: the pass buffer itself)
static int all_records_buffer(Pass& ps) {
    if (ps.d_recs_all) return HF_OK;
    int64_t n_pos = 0;
    for (const auto& sb : ps.tr->subs) if (sb.p1 > n_pos) n_pos = sb.p1;
    HIPCHK(hipMalloc((void**) &ps.d_recs_all, (size_t) (n_pos + 1) * 64));
    return HF_OK;
}

// ---- the launchers of this unit's kernels that hf_minlen.hip uses as well (hf_host.h) ----
// k_tables of the Gaussian models over ps's job list into ps's tables; the kernel clears `flags`.  The job list is the (key, class) list of
// the rows of A when the track has a segment plan (hf_seg.h), the key list otherwise, then the slow windows.
void launch_tables(const Pass& ps, unsigned* flags, bool kp, hipStream_t st) {
    const Track& tr = *ps.tr;
    const int jobs = (seg_pass(tr) ? tr.n_combo : tr.n_keys) + tr.n_slow;
#define HF_LAUNCH_TABLES(J, KA, KP) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tables<J, KA>), dim3((unsigned) ((jobs + J - 1) / J + (jobs == 0))), dim3(256), 0, st, \
                               ps.tabwork, ps.d_params, flags, KP, ps.d_params)
    if (kp) {     // the parameter block travels in the kernel arguments (pack_kparams): no copy was enqueued
        if (jobs < 64 * 1024) HF_LAUNCH_TABLES(HF_TABLE_JOBS_SMALL, true, ps.kparams); else HF_LAUNCH_TABLES(HF_TABLE_JOBS_LARGE, true, ps.kparams);
    } else {
        const NoKParams none{0};
        if (jobs < 64 * 1024) HF_LAUNCH_TABLES(HF_TABLE_JOBS_SMALL, false, none); else HF_LAUNCH_TABLES(HF_TABLE_JOBS_LARGE, false, none);
    }
#undef HF_LAUNCH_TABLES
}

// k_chunk_stats<KT>, KT the smallest of 4, 8, 16 that holds ncol collapsed-state components (as launch_stats is chosen)
void launch_chunk_stats(const Track& tr, hipStream_t st, int ncol, const int32_t* ll_off, const double* tile_stats, const double* ll_part,
                        const DevParams* params, double* chunk_stats, int full) {
#define HF_CHUNK_STATS(KT) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chunk_stats<KT>), dim3((unsigned) tr.C), dim3(128), 0, st, tr.d_chunk_tile0, ll_off, \
                                              tr.d_regmask, tile_stats, ll_part, params, chunk_stats, tr.V, tr.K, full)
    if (ncol <= 4) HF_CHUNK_STATS(4); else if (ncol <= 8) HF_CHUNK_STATS(8); else HF_CHUNK_STATS(16);
#undef HF_CHUNK_STATS
}

void launch_reduce(const Track& tr, hipStream_t st, const double* rows, const int32_t* row_index, int64_t n_rows, double* out,
                   const unsigned* flags, int n_ranks, int rows_per_rank, int flag_row) {
    hipLaunchKernelGGL(k_reduce, dim3((unsigned) (tr.V + 1)), dim3(64), 0, st, rows, row_index, n_rows, tr.V, out, flags, n_ranks, rows_per_rank,
                       flag_row);
}

template <int KT>
static void launch_stats(Pass& ps, hipStream_t st, int full, int ncol) {
    const Track& tr = *ps.tr;
    ps.pass_rows = false; ps.pass_host_total = false;
    if (full && rows_pass(ps)) {
        // statistics by emission row (hf_rows.h); the total of the pass comes out of k_row_stats' last blocks
        // (k_pair_sums ran behind every sub-pass's k_seg_fb: enqueue_pass)
        KTimer t(ps, st, HF_K_ROW_STATS);
        constexpr size_t NA = stat_acc_len(KT);
        // the wavefronts' sums: HF_RS_WPB wavefronts per block (a block stays inside one region: hf_create pads the regions to that multiple) — four
        // for a sparse plan, whose wavefronts take several batches of slots each: eight of those per block ran config 5 in 83 us instead of 51
        const int want_wpb = tr.rs_bpw > 1 ? 4 : HF_RS_WPB;
        TileGeom g = tile_geom(tr, k_row_stats<KT>, NA * 8, false, want_wpb);
        TILE_GEOM_OR_FAIL(g);
        if ((int) g.threads != 64 * want_wpb) { set_err(HF_E_ARG, "k_row_stats: the block's partial sums do not fit the LDS"); ps.launch_failed = true; return; }
        const int wpb = (int) g.threads / 64;
        const int n_rw_blocks = (tr.n_rowwaves + wpb - 1) / wpb, n_ll_blocks = (tr.C + wpb - 1) / wpb;
        // the launch's last block also sums the partials (rows_total): into d_total and straight into the pinned host block
        const bool bound = ps.d_rank_out != nullptr;    // multi-GPU `ranks` exchange: the total goes into the exchange buffer, not to the host
        ps.pass_bound = bound;
        // one GPU, nothing bound: the blocks' partial vectors go to pinned host memory and the HOST sums them (host_rows_total)
        bool host_total = !bound && ps.host_total_ok && ps.d_total_host != nullptr;
        if (host_total) {
            const size_t need = (size_t) n_rw_blocks * NA + (size_t) tr.C + 1;
            if (need > ps.part_cap) {
                if (ps.h_part) hipHostFree(ps.h_part);
                ps.h_part = nullptr; ps.d_part_host = nullptr; ps.part_cap = 0;
                void* dp = nullptr;
                if (hipHostMalloc((void**) &ps.h_part, (need + 64) * 8) == hipSuccess && hipHostGetDevicePointer(&dp, ps.h_part, 0) == hipSuccess) {
                    ps.d_part_host = (double*) dp; ps.part_cap = need + 64;
                } else { (void) hipGetLastError(); if (ps.h_part) hipHostFree(ps.h_part); ps.h_part = nullptr; ps.host_total_ok = false; host_total = false; }
            }
        }
        ps.pass_host_total = host_total; ps.pass_rw_blocks = n_rw_blocks;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_row_stats<KT>), dim3((unsigned) (n_rw_blocks + n_ll_blocks)), dim3(g.threads), g.lds, st,
                           tr.n_rowwaves, n_rw_blocks, tr.d_rw_region, tr.d_rowslots, ps.d_grp_sums, row_src(ps), ps.d_params,
                           ps.d_rw_stats, tr.C, ll_off(ps), ll_part(ps), ps.d_chunk_stats, tr.V, ps.d_chunk_ll,
                           tr.d_rw_off, tr.K, bound ? ps.d_rank_out : ps.d_total, bound ? (double*) nullptr : ps.d_total_host,
                           bound ? ps.d_rank_flag : (double*) nullptr, ps.d_flags, ps.d_done, tr.rs_bpw,
                           host_total ? ps.d_part_host : (double*) nullptr);
        ps.pass_wpb = wpb;
        ps.pass_rows = true;
        ps.pass_kc = ncol;
        return;
    }
    if (full) {
        KTimer t(ps, st, HF_K_STATS_TILE);
        const TileGeom g = tile_geom(tr, k_stats_tile<KT>, (size_t) (3 * ncol > 28 ? 3 * ncol : 28) * 65 * 8);
        TILE_GEOM_OR_FAIL(g);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stats_tile<KT>), dim3(g.blocks), dim3(g.threads), g.lds, st, tr.ntiles,
                           tr.d_tile_desc, tr.d_rec, row_src(ps), ps.d_params, ps.pass_seg ? ps.d_recs_all : ps.d_f, ps.d_b, tr.d_regmask,
                           ps.d_tile_stats, ps.pass_seg ? tr.d_pos : (const int32_t*) nullptr);
    }
    KTimer t(ps, st, HF_K_CHUNK_STATS);
    launch_chunk_stats(tr, st, ncol, ll_off(ps), ps.d_tile_stats, ll_part(ps), ps.d_params, ps.d_chunk_stats, full);
}

// the last kernel of a negative_binomial pass in HF_STATS_ROWS mode: total vector (+ flag word) into `out`
// (the Gaussian models' total is written by the last block of k_row_stats itself: hf_rows.h rows_total)
static int launch_nb_total(Pass& ps, hipStream_t st, double* out, bool with_flags = true) {
    const Track& tr = *ps.tr;
    KTimer t(ps, st, HF_K_ROWS_TOTAL);
    NbTables nt;
    nt.E = ps.d_nbE; nt.P = ps.d_nbP; nt.dig = ps.d_nbDig; nt.r = ps.d_nbR; nt.beta = ps.d_nbBeta;
    hipLaunchKernelGGL(k_nb_total, dim3((unsigned) tr.R), dim3(1024), 0, st, tr.d_rw_off, ps.pass_wpb, ps.d_rw_stats, ps.d_H,
                       ps.d_params, nt, ps.d_chunk_ll, (int64_t) tr.C, tr.V, tr.K, out,
                       with_flags ? ps.d_flags : (const unsigned*) nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}

__global__ void k_copy16(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// host getters (hf_get_forward_backward): f, b and the scale of windows first .. first + n, gathered from the pair records
__global__ void k_gather_fb(int64_t first, int64_t n, const int32_t* __restrict__ pos, const int32_t* __restrict__ pos_f,
                            const int32_t* __restrict__ slot_of, const double* __restrict__ recs, const double* __restrict__ scale_s,
                            double* __restrict__ f, double* __restrict__ b, double* __restrict__ sc) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t t = first + i;
    const double* __restrict__ rf = recs + (int64_t) pos_f[t] * 8;
    const double* __restrict__ rb = recs + (int64_t) pos[t] * 8 + 4;
#pragma unroll
    for (int s = 0; s < 4; s++) { f[i * 4 + s] = rf[s]; b[i * 4 + s] = rb[s]; }
    sc[i] = scale_s[slot_of[t]];
}

// Every per-pass device array of a track in bytes (0: the track has no use for it), and the pinned block: the ONE place that sizes a pass
// (pass_create allocates it, hf_batch_capacity counts it)
struct PassLayout {
    size_t label, chunk_stats, total, flags, done, params, lutE, lutC, lutA, tile_ll, tile_stats, seg_ready, seg_ll, Pseg, recs,
           grp_sums, chunk_ll, rw_stats, E, f, b, scale;
    size_t pin_total, pin_block;   // pinned: result vector (+ flag word) | flag word of hf_check | parameter block
    size_t device_bytes() const {
        size_t s = 0;
        for (size_t x : {label, chunk_stats, total, flags, done, params, lutE, lutC, lutA, tile_ll, tile_stats, seg_ready, seg_ll, Pseg,
                         recs, grp_sums, chunk_ll, rw_stats, E, f, b, scale})
            if (x) s += Slab::granule(x);
        return s;
    }
};
static PassLayout pass_layout(const Track& tr) {
    PassLayout L{};
    const size_t N = (size_t) tr.N, C = (size_t) tr.C, V = (size_t) tr.V, nt = (size_t) tr.ntiles, ns = (size_t) tr.nseg;
    const size_t rows = (size_t) tr.n_lut + (size_t) tr.n_slow + 1;   // emission rows: the keys, the slow windows, one row of padding
    auto some = [](size_t bytes) { return bytes ? bytes : 1; };      // (allocated even when empty)
    L.label = N + 16; L.chunk_stats = some(C * V * 8); L.total = (V + 1) * 8; L.flags = 4; L.done = HF_DONE_BYTES;
    L.params = tr.params_bytes; L.lutE = rows * 16 * 8; L.lutC = rows * 4 * (size_t) tr.K * 8;
    L.lutA = tr.d_arow ? ((size_t) tr.n_arows + 1) * 16 * 8 : 0;    // (+ the identity row)
    L.tile_ll = some(nt * 8); L.tile_stats = some(nt * (size_t) tr.R * stat_acc_len(16) * 8);
    if (ns) { L.seg_ready = ns * 4; L.seg_ll = ns * 8; L.Pseg = ns * 16 * 8; }
    int64_t cap = 0;                      // positions the pass buffer holds: the largest sub-pass (everything, with one)
    for (const auto& sb : tr.subs) cap = std::max<int64_t>(cap, sb.p1 - sb.p0);
    L.recs = tr.subs.empty() ? 0 : (size_t) (cap + 1) * 64;
    if (tr.rows_ready) {
        L.grp_sums = some((size_t) ((tr.n_groups + 3) / 4 * 4) * 16 * 8);   // (k_pair_sums: four groups per wavefront)
        L.chunk_ll = some(C * 8); L.rw_stats = some((size_t) tr.n_rowwaves * stat_acc_len(16) * 8);
    }
    if (tr.algo == HF_ALGO_SEQ) {         // the sequential cross-check: emission rows, window-order scales, f and b by tile (hf_device.h fb_slot)
        L.E = some(N * 16 * 8); L.scale = some(N * 8); L.f = L.b = some(nt * 64 * HF_SCAN_L * 4 * 8);
    }
    L.pin_total = ((V + 1) * 8 + 63) / 64 * 64;   // (what follows stays 64-byte aligned)
    L.pin_block = L.pin_total + 64 + (tr.params_bytes + 63) / 64 * 64;
    return L;
}

// does k_tables write the rows of A (the job list is the (key, class) list)?
static bool arow_jobs(const Track& tr) { return tr.nseg > 0 && tr.d_arow && tr.algo == HF_ALGO_SCAN; }

// The pass state of `tr` in *out: the settings copied from `settings` (the context's own pass may be both), the device arrays out of a slab of
// its own, the pinned block (from the process-wide cache: pinning even this small block was 0.1-0.2 ms of hf_create), the events; zeroed where a
// pass expects zeros, and the identity row behind the rows of A (hf_seg.h: what a lane multiplies by past its last window; no kernel writes it)
// written through `stg` when it has room — a synchronous copy in hf_create waited for the 6 MB of rows of A enqueued before it (0.25 ms).
// On failure the caller destroys *out.
int pass_create(const Track& tr, const Pass& settings, Pass* out, UploadStage* stg) {
    Pass& ps = *out;
    ps.tr = &tr;
    ps.stats_mode = settings.stats_mode; ps.seg_fused = settings.seg_fused; ps.seg_test_timeout = settings.seg_test_timeout;
    ps.kp_ok = settings.kp_ok; ps.host_total_ok = settings.host_total_ok; ps.stream_stamp_ok = settings.stream_stamp_ok;
    const PassLayout L = pass_layout(tr);
    ps.slab.first = L.device_bytes();
    bool ok = true;
    auto take = [&](auto*& p, size_t bytes) {
        if (bytes && ok) { p = static_cast<std::remove_reference_t<decltype(p)>>(ps.slab.alloc(bytes)); ok = p != nullptr; }
    };
    take(ps.d_label, L.label); take(ps.d_chunk_stats_own, L.chunk_stats); take(ps.d_total, L.total); take(ps.d_flags, L.flags);
    take(ps.d_done, L.done); take(ps.d_params, L.params); take(ps.d_lutE, L.lutE); take(ps.d_lutC, L.lutC);
    take(ps.d_lutA, L.lutA); take(ps.d_tile_ll, L.tile_ll); take(ps.d_tile_stats, L.tile_stats); take(ps.d_seg_ready, L.seg_ready);
    take(ps.d_seg_ll, L.seg_ll); take(ps.d_Pseg, L.Pseg); take(ps.d_recs, L.recs); take(ps.d_grp_sums, L.grp_sums);
    take(ps.d_chunk_ll, L.chunk_ll); take(ps.d_rw_stats, L.rw_stats);
    take(ps.d_E, L.E); take(ps.d_f, L.f); take(ps.d_b, L.b); take(ps.d_scale, L.scale);
    if (!ok) { (void) hipGetLastError(); return set_err(HF_E_HIP, "out of device memory for the pass state"); }
    ps.d_chunk_stats = ps.d_chunk_stats_own;
    ps.d_Es = ps.d_lutE + (size_t) tr.n_lut * 16;
    ps.d_Cs = ps.d_lutC + (size_t) tr.n_lut * 4 * (size_t) tr.K;
    if (tr.subs.size() == 1) ps.d_recs_all = ps.d_recs;      // (several sub-passes: the all-windows buffer on first use, all_records_buffer)
    ps.tabwork = tr.tabwork;
    ps.tabwork.lutE = ps.d_lutE; ps.tabwork.lutC = ps.d_lutC; ps.tabwork.lutA = arow_jobs(tr) ? ps.d_lutA : nullptr;
    char* pin = pin_cache().acquire(L.pin_block);
    if (!pin) return set_err(HF_E_HIP, "out of host memory for the pass state");
    std::memset(pin, 0, L.pin_block);                        // (a stale stamp word must not look like a future one)
    ps.h_total = reinterpret_cast<double*>(pin);
    ps.h_flags = reinterpret_cast<unsigned*>(pin + L.pin_total);
    ps.h_params = reinterpret_cast<DevParams*>(pin + L.pin_total + 64);
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, ps.h_total, 0) == hipSuccess) ps.d_total_host = (double*) dp;
    else {
        // (the cache falls back to pageable memory when pinning fails — a block the device cannot address: no zero-copy totals,
        // no stream stamp into it; passes then complete through a copy and hipStreamSynchronize)
        (void) hipGetLastError();
        ps.d_total_host = nullptr; ps.stream_stamp_ok = false;
    }
    HIPCHK(hipEventCreate(&ps.ev0)); HIPCHK(hipEventCreate(&ps.ev1));
    HIPCHK(hipMemsetAsync(ps.d_flags, 0, 4, nullptr));
    HIPCHK(hipMemsetAsync(ps.d_done, 0, HF_DONE_BYTES, nullptr));   // tickets of the in-launch hand-offs (hf_rows.h)
    HIPCHK(hipMemsetAsync(ps.d_params, 0, tr.params_bytes, nullptr));   // (the kernel-argument path writes the bytes in use only)
    HIPCHK(hipMemsetAsync(ps.d_label, 0xff, tr.N ? (size_t) tr.N : 1, nullptr));
    if (ps.d_seg_ready) HIPCHK(hipMemsetAsync(ps.d_seg_ready, 0, L.seg_ready, nullptr));
    if (ps.d_lutA) {
        double ident[16];
        for (int k = 0; k < 16; k++) ident[k] = (k % 5 == 0) ? 1.0 : 0.0;
        return stage_upload(stg, ps.d_lutA + (size_t) tr.n_arows * 16, ident, sizeof ident);
    }
    return HF_OK;
}

// everything pass_create and the pass's first uses allocated
void pass_destroy(Pass& ps) {
    for (void* p : {(void*) ps.d_segQ, (void*) ps.d_scale_s, (void*) ps.d_slot_of, (void*) ps.d_nbE, (void*) ps.d_tile_hist}) hipFree(p);
    if (ps.d_recs_all != ps.d_recs) hipFree(ps.d_recs_all);
    for (int b = 0; b < 2; b++) { if (ps.h_nb[b]) hipHostFree(ps.h_nb[b]); if (ps.nb_ev[b]) hipEventDestroy(ps.nb_ev[b]); }
    if (ps.h_part) hipHostFree(ps.h_part);
    if (ps.h_label) pin_cache().release(reinterpret_cast<char*>(ps.h_label));
    for (hipEvent_t e : {ps.ev0, ps.ev1}) if (e) hipEventDestroy(e);
    for (hipEvent_t e : ps.kev) if (e) hipEventDestroy(e);
    ps.slab.release();
    // the pinned block (h_flags and h_params live in it), back to the cache once nothing can write it any more
    if (ps.h_total) { hipDeviceSynchronize(); pin_cache().release(reinterpret_cast<char*>(ps.h_total)); }
}

void MinLenEM::drop_pass() { pass_destroy(pass); pass_made = false; }

#include "hf_create.h"

extern "C" {

const char* hf_version(void) { return "flagger_amd 0.1 (gfx950)"; }
const char* hf_last_error(void) { return g_err.c_str(); }

int hf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}


__global__ void k_selftest_div(int64_t n, const double* __restrict__ a, const double* __restrict__ d, double* __restrict__ fast,
                               double* __restrict__ exact, int32_t* __restrict__ safe);

int hf_warmup(int device) {
    if (hf_device_count() <= 0) return set_err(HF_E_NOGPU, "hf_warmup: no HIP device");
    {   // the host threads of hf_create's passes over the windows
        const unsigned hw = std::thread::hardware_concurrency();
        (void) hw;
        host_pool().start(host_threads() - 1);
    }
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipFree(nullptr));      // forces the context
    hipLaunchKernelGGL(k_selftest_div, dim3(1), dim3(64), 0, 0, (int64_t) 0, (const double*) nullptr, (const double*) nullptr,
                       (double*) nullptr, (double*) nullptr, (int32_t*) nullptr);   // loads this library's code object
    HIPCHK(hipDeviceSynchronize());
    {   // the first pinned allocation and the first copy in each direction cost several milliseconds each (queues, staging): pay them here
        void *d = nullptr, *h = nullptr;
        if (hipMalloc(&d, 8 << 20) == hipSuccess && hipHostMalloc(&h, 8 << 20) == hipSuccess) {   // (large: a 1 MiB copy takes another path)
            (void) hipMemcpy(d, h, 8 << 20, hipMemcpyHostToDevice);
            (void) hipMemcpy(h, d, 8 << 20, hipMemcpyDeviceToHost);
            (void) hipMemset(d, 0, 64);
        }
        if (h) hipHostFree(h);
        if (d) hipFree(d);
        (void) hipGetLastError();
    }
    {   // hf_create's pinned staging buffers (PinCache), for up to 2 M windows: pinning 32 MB takes ~6 ms — here, while the caller reads its input
        PinCache& pc = pin_cache();
        char* a = pc.acquire((size_t) 4 * (2u << 20));
        char* b = pc.acquire((size_t) 12 * (2u << 20));
        char* c = pc.acquire((size_t) 8 << 20);
        char* d = pc.acquire((size_t) 64 << 10);     // a context's result / parameter block
        pc.release(a); pc.release(b); pc.release(c); pc.release(d);
    }
    return HF_OK;
}

void hf_destroy(hf_ctx* ctx) {
#ifdef HF_KSTAMP
    if (ctx && std::getenv("HF_KSTAMP_FILE")) {
        unsigned long long h[64 * 4 + 1];
        hipSetDevice(ctx->tr.device); hipDeviceSynchronize();
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_kstamp), sizeof(h)) == hipSuccess)
            if (FILE* fp = std::fopen(std::getenv("HF_KSTAMP_FILE"), "ab")) { std::fwrite(h, 8, 64 * 4 + 1, fp); std::fclose(fp); }
    }
#endif
    if (!ctx) return;
    const Track& tr = ctx->tr;
    hipSetDevice(tr.device);
#ifdef HF_SEG_TRACE
    if (tr.d_seg_trace) {
        hipDeviceSynchronize();
        std::vector<unsigned long long> h((size_t) tr.nseg * HF_SEG_TRACE_N);
        hipMemcpy(h.data(), tr.d_seg_trace, h.size() * 8, hipMemcpyDeviceToHost);
        if (FILE* fp = std::fopen(std::getenv("HF_SEG_TRACE_FILE"), "wb")) { std::fwrite(h.data(), 8, h.size(), fp); std::fclose(fp); }
        unsigned long long* null_p = nullptr;
        hipMemcpyToSymbol(HIP_SYMBOL(g_seg_trace), &null_p, sizeof(void*));
    }
#endif
    const Pass& ps = ctx->pass;
    if (ps.host_trace && ps.ht_n)
        std::fprintf(stderr, "[hf host trace] %ld EM steps: parameter view (hfm_params: the negative-binomial tables) %.1f us, enqueue %.1f us, wait %.1f us, m-step %.1f us, gpu span (first launch .. reduction) %.1f us\n",
                     ps.ht_n, ps.ht[4] / ps.ht_n, ps.ht[0] / ps.ht_n, ps.ht[1] / ps.ht_n, ps.ht[2] / ps.ht_n, ps.ht[3] / ps.ht_n);
    pass_destroy(ctx->pass);
    ctx->vit.release();
    ctx->mlv.release();
    ctx->mlp.release();
    ctx->mls.release();
    ctx->smp.release();
    ctx->iv.release();
    ctx->al.release();
    ctx->mo.release();
    ctx->rn.release();
    ctx->en.release();
    ctx->en_lab.release();
    ctx->bp.release();
    ctx->lr.release();
    ctx->rl.release();
    ctx->cd.release();
    ctx->mea.release();
    ctx->mle.release();
    ctx->tr.slab.release();
    delete ctx;
}

// pack one iteration's model: conditional transition tables (hmm_utils.c:2278-2292) and the
// distinct alpha values of each column
extern "C++" int pack_params(const Track& tr, const hf_params* p, DevParams* dst) {
    if (p->n_regions != tr.R) return set_err(HF_E_ARG, "hf_estep: n_regions differs from hf_create");
    for (int s = 0; s < 4; s++)
        if (p->ncomp[s] < 1 || p->ncomp[s] > tr.K) return set_err(HF_E_ARG, "hf_estep: ncomp out of range");
    if (p->ncomp[1] != 1 || p->ncomp[2] != 1 || p->ncomp[0] != 1)
        return set_err(HF_E_ARG, "hf_estep: Err/Dup/Hap must have one component (hmm_flagger.c:180-182)");
    DevParams* h = dst;
    h->model_type = p->model_type; h->n_regions = p->n_regions;
    h->beta_star = tr.beta_star;
    for (int s = 0; s < 4; s++) h->ncomp[s] = p->ncomp[s];
    for (int pre = 0; pre < 4; pre++)
        for (int s = 0; s < 4; s++) h->alpha[pre * 4 + s] = p->alpha[pre][s];
    for (int s = 0; s < 4; s++) {
        int nu = 0;
        for (int pre = 0; pre < 4; pre++) {
            const double a = p->alpha[pre][s];
            int u = -1;
            for (int k = 0; k < nu; k++) if (h->ualpha[s][k] == a) { u = k; break; }
            if (u < 0) { u = nu; h->ualpha[s][nu++] = a; }
            h->umap[pre * 4 + s] = u;
        }
        for (int k = nu; k < 4; k++) h->ualpha[s][k] = 0.0;
        h->nuniq[s] = nu;
    }
    {   // k_tables' items: every (state, distinct alpha, component) of a row, Err as truncated exponential is one item
        int n = 0;
        for (int st = 0; st < 4; st++) {
            const bool te = st == 0 && p->model_type == HF_MODEL_TRUNC_EXP_GAUSSIAN;
            const int nu = te ? 1 : h->nuniq[st], nc = te ? 1 : p->ncomp[st];
            for (int u = 0; u < 4; u++) h->item_base[st * 4 + u] = u < nu ? n + u * nc : n;
            for (int u = 0; u < nu; u++)
                for (int c = 0; c < nc; c++) { h->item_s[n] = (uint8_t) st; h->item_u[n] = (uint8_t) u; h->item_c[n] = (uint8_t) c; n++; }
        }
        h->n_items = n;
    }
    for (int r = 0; r < tr.R; r++) {
        DevRegion* g = &h->reg[r];
        std::memcpy(g->trans, p->trans + (size_t) r * 25, sizeof(double) * 25);
        g->lambda = p->lambda ? p->lambda[r] : 1.0;
        g->trunc_point = p->trunc_point ? p->trunc_point[r] : 0.0;
        std::memcpy(g->mean, p->mean + (size_t) r * 4 * HF_MAXCOMP, sizeof(g->mean));
        std::memcpy(g->var, p->var + (size_t) r * 4 * HF_MAXCOMP, sizeof(g->var));
        std::memcpy(g->weight, p->weight + (size_t) r * 4 * HF_MAXCOMP, sizeof(g->weight));
        const double bs = tr.beta_star;
        for (int s = 0; s < 4; s++)
            for (int c = 0; c < p->ncomp[s]; c++) {             // (per EM step and region: the components in use, not HF_MAXCOMP)
                double var = g->var[s][c];
                var *= bs;
                g->gvar[s][c] = var;
                g->gnorm[s][c] = g->weight[s][c] / (std::sqrt(var * 2 * HF_PI));
                for (int u = 0; u < 4; u++) g->m1[s][u][c] = (1 - h->ualpha[s][u]) * g->mean[s][c];
            }
        g->te_lam = g->lambda / bs;
        g->te_den = 1 - std::exp(-g->te_lam * (bs * g->trunc_point));
        for (int vm = 0; vm < 8; vm++) {
            bool valid[5] = { true, (vm & 1) != 0, true, (vm & 2) != 0, (vm & 4) != 0 };
            for (int pre = 0; pre < 4; pre++) {
                double tot = 0.0;
                for (int s = 0; s < 5; s++) if (valid[s]) tot += g->trans[pre][s];
                for (int s = 0; s < 4; s++) g->tcond[vm][pre * 4 + s] = valid[s] ? g->trans[pre][s] / tot : 0.0;
            }
        }
    }
    return 0;
}


// the 8-byte words of the packed block that are in use, each with its place in the image (hf_device.h KParams); false: they do not fit
static bool pack_kparams(Pass& ps, const hf_params* p) {
    if (ps.tr->R != 1) return false;
    const DevParams* h = ps.h_params;
    KParams& kp = ps.kparams;
    const char* const base = reinterpret_cast<const char*>(h);
    int nw = 0;
    bool fits = true;
    auto add = [&](const void* first, size_t bytes) {
        const size_t o = (size_t) (reinterpret_cast<const char*>(first) - base);
        if (!fits || bytes == 0) return;
        if (o % 8 || bytes % 8 || nw + (int) (bytes / 8) > HF_KP_MAX_WORDS) { fits = false; return; }
        std::memcpy(kp.data + nw, first, bytes);
        for (size_t i = 0; i < bytes / 8; i++) kp.idx[nw + (int) i] = (uint16_t) (o / 8 + i);
        nw += (int) (bytes / 8);
    };
    const DevRegion* g = &h->reg[0];
    add(h, offsetof(DevParams, reg));                                                    // the header, the item list
    add(g->trans, sizeof g->trans + sizeof g->tcond + 2 * sizeof(double));               // trans, tcond, lambda, trunc_point: contiguous
    static_assert(offsetof(DevRegion, tcond) == sizeof(double) * 25 && offsetof(DevRegion, lambda) == sizeof(double) * (25 + 128) &&
                  offsetof(DevRegion, mean) == sizeof(double) * (25 + 128 + 2), "DevRegion starts with trans | tcond | lambda | trunc_point");
    for (int s = 0; s < HF_NSTATES; s++) {
        const size_t nc = (size_t) p->ncomp[s] * sizeof(double);
        add(g->mean[s], nc); add(g->var[s], nc); add(g->weight[s], nc); add(g->gvar[s], nc); add(g->gnorm[s], nc);
        for (int u = 0; u < 4; u++) add(g->m1[s][u], nc);
    }
    add(&g->te_lam, 2 * sizeof(double));
    if (!fits) return false;
    kp.n_words = nw; kp.pad = 0;
    return true;
}

// everything one pass enqueues on `st` after the parameters were packed into the pinned block
// retry: the pass again after HF_E_RETRY (hf_finish) — the caller's negative_binomial tables went up with the first attempt and
// may have been freed or rewritten since (hf_estep and hf_finish are separate calls): they are NOT read again
// phase (hf_batch.h): the parts of the pass to enqueue — PASS_PRE the parameter block and the tables, PASS_SEG the segment kernel, PASS_POST
// the statistics; a batch enqueues PRE and POST per model and the segment kernel of all models in one launch
enum { PASS_PRE = 1, PASS_SEG = 2, PASS_POST = 4, PASS_ALL = 7 };
static int enqueue_pass(Pass& ps, const hf_params* p, int mode, hipStream_t st, bool retry = false, int phase = PASS_ALL) {
    const Track& tr = *ps.tr;
    const bool ph_pre = (phase & PASS_PRE) != 0, ph_seg = (phase & PASS_SEG) != 0, ph_post = (phase & PASS_POST) != 0;
    // the parameter block: through the kernel arguments of k_tables when it fits them (one region, HF_ALGO_SCAN, Gaussian models:
    // hf_device.h KParams), a copy ahead of the pass otherwise
    if (ph_pre) {
        ps.kp_now = ps.kp_ok && tr.C > 0 && tr.algo == HF_ALGO_SCAN && p->model_type != HF_MODEL_NEGATIVE_BINOMIAL && pack_kparams(ps, p);
        if (!ps.kp_now) HIPCHK(hipMemcpyAsync(ps.d_params, ps.h_params, tr.params_bytes, hipMemcpyHostToDevice, st));
        for (int i = 0; i < HF_NKERNELS; i++) { ps.kran[i] = false; ps.klast_ok[i] = false; }
        ps.prof_now = ps.prof_stride <= 1 || (ps.prof_pass++ % ps.prof_stride) == 0;
    }
    ps.pass_rows = false; ps.pass_bound = false;
    ps.pass_seg = false;
    if (tr.C == 0 && ph_pre) HIPCHK(hipMemsetAsync(ps.d_flags, 0, 4, st));
    if (tr.C > 0) {
        const RowSrc S = row_src(ps);
        const bool full = mode == HF_MODE_FULL;
        const bool nbm = p->model_type == HF_MODEL_NEGATIVE_BINOMIAL;
        if (nbm) {   // the caller's per-x tables go up with the parameters
            if (!retry && (!p->nb_E || !p->nb_P || !p->nb_dig || !p->nb_r || !p->nb_beta))
                return set_err(HF_E_ARG, "hf_estep: negative_binomial needs hf_params.nb_E/nb_P/nb_dig/nb_r/nb_beta");
            if (p->nb_max_x > 0 && tr.M - 1 > p->nb_max_x)
                return set_err(HF_E_ARG, "hf_estep: the windows hold coverage values above hf_params.nb_max_x (hfm_set_max_coverage)");
            const size_t nE = (size_t) tr.R * 4 * HF_NB_NX * 8, nP = (size_t) tr.R * 4 * tr.K * HF_NB_NX * 8,
                         nR = (size_t) tr.R * 4 * tr.K * 8;
            // ONE device buffer and ONE copy per pass for the five tables (round 4; five copies out of pageable memory were ~50 us of a
            // 0.24 ms step): E | P | dig | r | beta, gathered into one of two pinned staging buffers (an event per buffer says when its
            // last copy has left it: a caller may enqueue the next pass before this one has run)
            const size_t nAll = nE + 2 * nP + 2 * nR;
            if (!ps.d_nbE) {
                // everything into locals first: the context is touched only when ALL of it exists (a failure half way used to leave
                // d_nbE set and a staging buffer null — the next pass skipped this block and copied through the null pointer)
                // the count data: tile_hist [ntiles][R][HF_NB_TILE_VEC] | slot_h [row slots][4] | H [R][4][256]
                const size_t nT = Slab::granule(((size_t) tr.ntiles * tr.R * HF_NB_TILE_VEC + 1) * 8),
                             nS = Slab::granule((size_t) tr.n_rowwaves * 16 * tr.rs_bpw * 4 * 8);
                double *dE = nullptr, *dH = nullptr; char* hb[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr};
                bool ok = hipMalloc((void**) &dE, nAll) == hipSuccess && hipMalloc((void**) &dH, nT + nS + (size_t) tr.R * 4 * 256 * 8) == hipSuccess;
                for (int b = 0; ok && b < 2; b++)
                    ok = hipHostMalloc((void**) &hb[b], nAll) == hipSuccess && hipEventCreateWithFlags(&ev[b], hipEventDisableTiming) == hipSuccess;
                if (!ok) {
                    const hipError_t e_ = hipGetLastError();
                    for (int b = 0; b < 2; b++) { if (hb[b]) hipHostFree(hb[b]); if (ev[b]) hipEventDestroy(ev[b]); }
                    hipFree(dE); hipFree(dH);
                    return set_err(HF_E_HIP, std::string("hf_estep: negative-binomial staging: ") + hipGetErrorString(e_));
                }
                char* base = reinterpret_cast<char*>(dE);
                ps.d_nbE = dE; ps.d_tile_hist = dH;
                ps.d_slot_h = reinterpret_cast<double*>(reinterpret_cast<char*>(dH) + nT); ps.d_H = reinterpret_cast<double*>(reinterpret_cast<char*>(dH) + nT + nS);
                ps.d_nbP = reinterpret_cast<double*>(base + nE); ps.d_nbDig = reinterpret_cast<double*>(base + nE + nP);
                ps.d_nbR = reinterpret_cast<double*>(base + nE + 2 * nP); ps.d_nbBeta = reinterpret_cast<double*>(base + nE + 2 * nP + nR);
                for (int b = 0; b < 2; b++) { ps.h_nb[b] = hb[b]; ps.nb_ev[b] = ev[b]; }
            }
            if (!retry) {
                const int b = (int) (ps.nb_turn++ & 1u);
                if (ps.nb_ev_used[b]) HIPCHK(hipEventSynchronize(ps.nb_ev[b]));
                char* h = ps.h_nb[b];
                std::memcpy(h, p->nb_E, nE); std::memcpy(h + nE, p->nb_P, nP); std::memcpy(h + nE + nP, p->nb_dig, nP);
                std::memcpy(h + nE + 2 * nP, p->nb_r, nR); std::memcpy(h + nE + 2 * nP + nR, p->nb_beta, nR);
                HIPCHK(hipMemcpyAsync(ps.d_nbE, h, nAll, hipMemcpyHostToDevice, st));
                HIPCHK(hipEventRecord(ps.nb_ev[b], st));
                ps.nb_ev_used[b] = true;
            }
        }
        if (ph_pre) {   // also clears the flag word: first kernel of every pass
            KTimer t(ps, st, HF_K_TABLES);
            if (nbm)
                hipLaunchKernelGGL(k_tables_nb, dim3((unsigned) ((tr.n_keys + tr.n_slow) / 256 + 1)), dim3(256), 0, st, tr.n_keys, tr.d_keys, tr.n_slow,
                                   tr.d_slow_w, tr.d_rec, tr.M, ps.d_nbE, ps.d_lutE, ps.d_Es, ps.d_flags);
            else
                launch_tables(ps, ps.d_flags, ps.kp_now, st);
        }
        if (tr.ntiles > 0) {
            if (tr.algo == HF_ALGO_SEQ) {
                {
                    KTimer t(ps, st, HF_K_EMIT_ROWS);
                    hipLaunchKernelGGL(k_emit_rows, dim3((unsigned) ((tr.N + 255) / 256)), dim3(256), 0, st, tr.N, tr.d_rec,
                                       tr.d_beta, ps.d_params, nbm ? ps.d_nbE : (const double*) nullptr, ps.d_E, ps.d_flags);
                }
                {
                    KTimer t(ps, st, HF_K_FWD_SEQ);
                    hipLaunchKernelGGL(k_fwd_seq, dim3((unsigned) tr.C), dim3(64), 0, st, tr.d_off, tr.d_chunk_tile0, tr.d_rec,
                                       ps.d_E, ps.d_params, ps.d_f, ps.d_scale, ps.d_tile_ll, ps.d_flags);
                }
                if (full) ps.fb_recs = false;
                if (full) {
                    KTimer t(ps, st, HF_K_BWD_SEQ);
                    hipLaunchKernelGGL(k_bwd_seq, dim3((unsigned) tr.C), dim3(64), 0, st, tr.d_off, tr.d_chunk_tile0, tr.d_rec,
                                       ps.d_E, ps.d_params, ps.d_f, ps.d_scale, ps.d_b, ps.d_label, ps.d_flags);
                }
            } else if (seg_pass(tr)) {
                // one workgroup per chunk segment does the whole forward-backward (hf_seg.h)
                const int nc = ps.seg_fused ? tr.seg_nc : 0;
                const size_t lds = seg_lds_bytes(nc);
                if (ps.host_trace && !ps.ht_n) {
                    int o1 = 0, o2 = 0;
                    hipOccupancyMaxActiveBlocksPerMultiprocessor(&o1, k_seg_prod, 64, seg_lds_bytes());
                    if (ps.seg_fused) hipOccupancyMaxActiveBlocksPerMultiprocessor(&o2, k_seg_fb<true, true>, 64, lds);
                    else hipOccupancyMaxActiveBlocksPerMultiprocessor(&o2, k_seg_fb<true, false>, 64, lds);
                    std::fprintf(stderr, "[hf host trace] segment kernels (%s): %d workgroups of 64 threads, %zu B of LDS; resident per CU: k_seg_prod %d, k_seg_fb %d\n",
                                 ps.seg_fused ? "one launch" : "two launches", tr.nseg, lds, o1, o2);
                }
                if (nbm && ph_pre) {   // k_tables_nb leaves the emission rows; the Gaussian k_tables writes the rows of A itself
                    KTimer t(ps, st, HF_K_AROWS);
                    hipLaunchKernelGGL(k_arows, dim3((unsigned) (((int64_t) tr.n_arows * 16 + 255) / 256)), dim3(256), 0, st, tr.n_arows,
                                       tr.d_arow_src, tr.d_arow_cls, ps.d_lutE, ps.d_params, ps.d_lutA);
                }
                if (!ps.seg_fused && ph_seg) {
                    if (!ps.d_segQ) HIPCHK(hipMalloc((void**) &ps.d_segQ, (size_t) tr.nseg * 64 * 16 * 8));   // lane products: two-launch mode only
                    KTimer t(ps, st, HF_K_SEG_PROD);
                    hipLaunchKernelGGL(k_seg_prod, dim3((unsigned) tr.nseg), dim3(64), seg_lds_bytes(), st, tr.d_seg, tr.d_arow, ps.d_lutA, ps.d_segQ, ps.d_Pseg);
                }
                const bool tfb = ((ps.prof_mask >> HF_K_SEG_FB) & 1u) && ps.prof_now;
                if (tfb) ps.kran[HF_K_SEG_FB] = true;
                const unsigned epoch = ph_seg ? ++ps.seg_epoch : ps.seg_epoch;
                // HF_SEG_TEST_TIMEOUT=1 (tests/test_estep_gpu.py): the first one-launch pass waits for flags nobody writes, so that
                // the time-out, HF_E_RETRY and the fall-back to two launches are exercised
                const unsigned wait_epoch = (ps.seg_test_timeout && epoch == 1) ? 0xffffffffu : epoch;
                // Sub-passes (Track::SubPass).  A full pass whose statistics go by emission row runs sub-pass by sub-pass through the pass
                // buffer: k_seg_fb writes a sub-pass's records, k_pair_sums reads them back while they are still in the Infinity Cache, the next
                // sub-pass overwrites them.  Any other pass (per-chunk statistics read the records by window afterwards; a forward-only pass writes
                // none) is ONE launch over all segments into the all-windows buffer.
                const bool want_rows = full && rows_pass(ps);
                ps.pass_pairs_done = false;
                if (want_rows) {
                    const bool alias = tr.subs.size() > 1;
                    bool first = true;
                    for (size_t si = 0; si < tr.subs.size(); si++) {
                        const auto& sb = tr.subs[si];
                        double* const recs_eff = alias ? ps.d_recs - sb.p0 * 8 : ps.d_recs;
                        if (ph_seg) launch_seg_fb(ps, st, true, recs_eff, (int) si, epoch, wait_epoch, tfb && first, false);   // (timed: the first sub-pass's launch, hf_sub_pass_windows; no scales)
                        first = false;
                        if (!ph_post) continue;
                        KTimer t(ps, st, HF_K_PAIR_SUMS);              // (event pairs around k_pair_sums: the last sub-pass's is what is read)
                        launch_pair_sums(ps, st, sb, recs_eff);
                    }
                    ps.pass_pairs_done = true;
                    ps.recs_all = !alias;
                    ps.scales_all = false;
                } else {
                    double* recs = ps.d_recs;
                    if (full && tr.subs.size() > 1) { const int rc_ = all_records_buffer(ps); if (rc_) return rc_; recs = ps.d_recs_all; }
                    if (ph_seg) launch_seg_fb(ps, st, full, recs, -1, epoch, wait_epoch, tfb, false);
                    if (full) { ps.recs_all = true; ps.scales_all = false; }
                }
                ps.pass_seg = true;
                if (full) ps.fb_recs = true;
            } else
                return set_err(HF_E_ARG, "hf_estep: HF_ALGO_SCAN holds at most 2^30 windows per context (shard the chunk list: hmm_flagger_multi.h)");
        }
        const int kc = p->ncomp[3];
        const int fl = full && tr.ntiles > 0;
        if (!ph_post) { HIPCHK(hipGetLastError()); return HF_OK; }
        ps.pass_nb = false;
        if (nbm && fl && rows_pass(ps)) {   // statistics by emission row, negative_binomial (hf_nb_rows.h)
            {   // (k_pair_sums ran behind every sub-pass's k_seg_fb, above)
                KTimer t(ps, st, HF_K_ROW_STATS);
                const int n_rw_blocks = (tr.n_rowwaves + 3) / 4, n_ll_blocks = (tr.C + 3) / 4;
                hipLaunchKernelGGL(k_row_stats_nb, dim3((unsigned) (n_rw_blocks + n_ll_blocks)), dim3(256), 0, st, tr.n_rowwaves, n_rw_blocks,
                                   tr.d_rowslots, ps.d_grp_sums, ps.d_slot_h, ps.d_rw_stats, tr.C, ll_off(ps), ll_part(ps),
                                   ps.d_chunk_stats, tr.V, ps.d_chunk_ll, tr.rs_bpw);
                const int n_bins = tr.R * 256;
                hipLaunchKernelGGL(k_nb_hist, dim3((unsigned) ((n_bins + 3) / 4)), dim3(256), 0, st, n_bins, tr.d_bin_off, tr.d_bin_list,
                                   ps.d_slot_h, ps.d_H);
            }
            ps.pass_rows = true; ps.pass_nb = true; ps.pass_wpb = 4;
        }
        else if (nbm) {
            if (fl) {
                KTimer t(ps, st, HF_K_STATS_TILE);
                const TileGeom g = tile_geom(tr, k_stats_tile_nb<HF_SCAN_L>, (size_t) HF_NB_WAVE_LDS * 8);
                if (!g.ok) return set_err(HF_E_ARG, "the per-region tables do not fit the LDS of one workgroup");
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stats_tile_nb<HF_SCAN_L>), dim3(g.blocks), dim3(g.threads), g.lds, st, tr.ntiles, tr.d_tile_desc,
                                   tr.d_rec, S, ps.d_params, ps.pass_seg ? ps.d_recs_all : ps.d_f, ps.d_b, tr.d_regmask, ps.d_tile_hist,
                                   ps.pass_seg ? tr.d_pos : (const int32_t*) nullptr);
            }
            NbTables nt;
            nt.E = ps.d_nbE; nt.P = ps.d_nbP; nt.dig = ps.d_nbDig; nt.r = ps.d_nbR; nt.beta = ps.d_nbBeta;
            KTimer t(ps, st, HF_K_CHUNK_STATS);
            hipLaunchKernelGGL(k_chunk_stats_nb, dim3((unsigned) tr.C), dim3(256), 0, st, tr.d_chunk_tile0, ll_off(ps), tr.d_regmask,
                               ps.d_tile_hist, ll_part(ps), ps.d_params, nt, ps.d_chunk_stats, tr.V, tr.K, fl);
        }
        else if (kc <= 4) launch_stats<4>(ps, st, fl, kc);
        else if (kc <= 8) launch_stats<8>(ps, st, fl, kc);
        else launch_stats<16>(ps, st, fl, kc);
        if (ps.launch_failed) { ps.launch_failed = false; return HF_E_ARG; }
    }
    HIPCHK(hipGetLastError());
    return HF_OK;
}

int hf_estep(hf_ctx* ctx, const hf_params* p, int mode, void* stream) {
    if (!ctx || !p || (mode != HF_MODE_FULL && mode != HF_MODE_FORWARD_ONLY)) return set_err(HF_E_ARG, "hf_estep: bad argument");
    Pass& ps = ctx->pass; const Track& tr = ctx->tr;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(hipSetDevice(tr.device));
    int rc = pack_params(tr, p, ps.h_params);
    if (rc) return rc;
    ps.last_p = *p; ps.last_mode = mode; ps.last_stream = st;
    ctx->al.pass = false; ctx->al.cached = false;
    if (pass_events(ps)) HIPCHK(hipEventRecord(ps.ev0, st));
    rc = enqueue_pass(ps, p, mode, st);
    if (rc) return rc;
    ctx->al.pass = ctx->al.on && mode == HF_MODE_FULL;
    if (pass_events(ps)) HIPCHK(hipEventRecord(ps.ev1, st));
    ps.ev_valid = pass_events(ps);
    ps.have_full = (mode == HF_MODE_FULL);
    return HF_OK;
}

int32_t hf_n_chunks(const hf_ctx* ctx) { return ctx ? ctx->tr.C : 0; }
int64_t hf_n_windows(const hf_ctx* ctx) { return ctx ? ctx->tr.N : 0; }
int64_t hf_chunk_stats_len(const hf_ctx* ctx) { return ctx ? ctx->tr.V : 0; }
double* hf_chunk_stats_dev(hf_ctx* ctx) { return ctx ? ctx->pass.d_chunk_stats : nullptr; }
int8_t* hf_labels_dev(hf_ctx* ctx) { return ctx ? ctx->pass.d_label : nullptr; }

int hf_set_stats_mode(hf_ctx* ctx, int mode) {
    if (!ctx || (mode != HF_STATS_CHUNKS && mode != HF_STATS_ROWS)) return set_err(HF_E_ARG, "hf_set_stats_mode: bad argument");
    ctx->pass.stats_mode = mode;
    return HF_OK;
}
int hf_get_stats_mode(const hf_ctx* ctx) {
    return ctx && ctx->pass.stats_mode == HF_STATS_ROWS && ctx->tr.rows_ready && ctx->tr.algo == HF_ALGO_SCAN ? HF_STATS_ROWS : HF_STATS_CHUNKS;
}

int hf_seg_launches(const hf_ctx* ctx) { return !ctx || !seg_pass(ctx->tr) ? 0 : (ctx->pass.seg_fused ? 1 : 2); }
int hf_sub_passes(const hf_ctx* ctx) { return !ctx || !seg_pass(ctx->tr) ? 0 : (int) ctx->tr.subs.size(); }
int64_t hf_sub_pass_windows(const hf_ctx* ctx, int k) {
    if (!ctx || k < 0 || (size_t) k >= ctx->tr.subs.size()) return 0;
    return ctx->tr.h_off[(size_t) ctx->tr.subs[(size_t) k].c1] - ctx->tr.h_off[(size_t) ctx->tr.subs[(size_t) k].c0];
}
int hf_seg_cached_steps(const hf_ctx* ctx) { return !ctx || !seg_pass(ctx->tr) || !ctx->pass.seg_fused ? 0 : ctx->tr.seg_nc; }
int hf_create_phases(const hf_ctx* ctx, int max, double* ms, const char** names) {
    if (!ctx) return 0;
    const Track& tr = ctx->tr;
    const int n = (int) tr.create_phases.size();
    for (int i = 0; i < n && i < max; i++) { if (ms) ms[i] = tr.create_phases[(size_t) i].second; if (names) names[i] = tr.create_phases[(size_t) i].first; }
    return n;
}

int hf_copy_chunk_stats(hf_ctx* ctx, double* dst_dev, void* stream) {
    if (!ctx || !dst_dev) return set_err(HF_E_ARG, "hf_copy_chunk_stats: bad argument");
    Pass& ps = ctx->pass; const Track& tr = ctx->tr;
    if (ps.pass_rows) return set_err(HF_E_ARG, "hf_copy_chunk_stats: the last pass ran in HF_STATS_ROWS mode (no per-chunk vectors)");
    HIPCHK(hipSetDevice(tr.device));
    if (dst_dev == ps.d_chunk_stats) return HF_OK;   // bound to the exchange buffer: the kernels already wrote in place
    HIPCHK(hipMemcpyAsync(dst_dev, ps.d_chunk_stats, (size_t) tr.C * tr.V * 8, hipMemcpyDeviceToDevice,
                          (hipStream_t) stream));
    return HF_OK;
}

int hf_rank_total(hf_ctx* ctx, double* out_dev, void* stream) {
    if (!ctx || !out_dev) return set_err(HF_E_ARG, "hf_rank_total: bad argument");
    Pass& ps = ctx->pass; const Track& tr = ctx->tr;
    HIPCHK(hipSetDevice(tr.device));
    if (ps.pass_rows && ps.pass_nb) return launch_nb_total(ps, (hipStream_t) stream, out_dev, false);
    if (ps.pass_rows && ps.pass_bound && out_dev == ps.d_rank_out) return HF_OK;   // hf_bind_rank_total: already there
    if (ps.pass_rows && ps.pass_host_total) {   // the pass sent its partials to the host: the total on the device from the copies in blk_stats / chunk_ll
        const int wpb = ps.pass_wpb;
        const dim3 grid((unsigned) (tr.R + 1)), blk((unsigned) (64 * wpb));
#define HF_LATE(KT) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rows_total_late<KT>), grid, blk, 0, (hipStream_t) stream, tr.d_rw_off, wpb, ps.d_rw_stats, ps.d_params, \
                                       tr.K, ps.d_chunk_ll, (int64_t) tr.C, out_dev)
        if (ps.pass_kc <= 4) HF_LATE(4); else if (ps.pass_kc <= 8) HF_LATE(8); else HF_LATE(16);
#undef HF_LATE
        HIPCHK(hipGetLastError());
        return HF_OK;
    }
    if (ps.pass_rows) {   // the pass left its total in d_total (or where it was bound to)
        hipLaunchKernelGGL(k_copy_total, dim3(1), dim3(256), 0, (hipStream_t) stream, ps.pass_bound ? ps.d_rank_out : ps.d_total, out_dev, tr.V);
        HIPCHK(hipGetLastError());
        return HF_OK;
    }
    return hf_reduce_chunks_indexed(ctx, ps.d_chunk_stats, nullptr, tr.C, out_dev, stream);
}

struct ExchangeGeom { int n_ranks = 0, rows_per_rank = 0, flag_row = 0; };   // n_ranks == 0: no flag rows to merge
static int reduce_chunks(Pass& ps, const double* chunk_stats_dev, const int32_t* row_index_dev, int64_t n_chunks,
                         double* out_dev, void* stream, ExchangeGeom xg = ExchangeGeom()) {
    const Track& tr = *ps.tr;
    if (!chunk_stats_dev || !out_dev || n_chunks < 0) return set_err(HF_E_ARG, "hf_reduce_chunks: bad argument");
    HIPCHK(hipSetDevice(tr.device));
    const bool own = chunk_stats_dev == ps.d_chunk_stats;
    const unsigned keep = ps.prof_mask;
    if (!own) ps.prof_mask = 0;
    {
        KTimer t(ps, (hipStream_t) stream, HF_K_REDUCE);
        launch_reduce(tr, (hipStream_t) stream, chunk_stats_dev, row_index_dev, n_chunks, out_dev,
                      (out_dev == ps.d_total || out_dev == ps.d_total_host) ? ps.d_flags : (const unsigned*) nullptr,
                      xg.n_ranks, xg.rows_per_rank, xg.flag_row);
    }
    ps.prof_mask = keep;
    HIPCHK(hipGetLastError());
    return HF_OK;
}
int hf_reduce_chunks_indexed(hf_ctx* ctx, const double* chunk_stats_dev, const int32_t* row_index_dev, int64_t n_chunks,
                             double* out_dev, void* stream) {
    if (!ctx) return set_err(HF_E_ARG, "hf_reduce_chunks: bad argument");
    return reduce_chunks(ctx->pass, chunk_stats_dev, row_index_dev, n_chunks, out_dev, stream);
}

int hf_reduce_chunks(hf_ctx* ctx, const double* chunk_stats_dev, int64_t n_chunks, double* out_dev, void* stream) {
    return hf_reduce_chunks_indexed(ctx, chunk_stats_dev, nullptr, n_chunks, out_dev, stream);
}

// running sums for hf_kernel_time_sums; the stream has been synchronised
static void accumulate_kernel_times(Pass& ps) {
    if (!ps.prof_mask) return;
    for (int i = 0; i < HF_NKERNELS; i++)
        if (ps.kran[i]) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ps.kev[2 * i], ps.kev[2 * i + 1]) == hipSuccess) { ps.ksum[i] += ms; ps.kcount[i]++; ps.klast[i] = ms; ps.klast_ok[i] = true; }
        }
}

extern "C++" int flags_to_code(unsigned fl) {
    if (fl & HF_FLAG_REGION) return set_err(HF_E_REGION, "a window's region index is >= n_regions");
    if (fl & HF_FLAG_SYNC) return set_err(HF_E_HIP, "a chunk segment waited too long for another segment's product (one-launch segment kernel)");
    if (fl & HF_FLAG_NAN) return set_err(HF_E_NAN, "[Error] prob is NAN");
    if (fl & HF_FLAG_SCALE) return set_err(HF_E_SCALE, "scale is very low!");
    return HF_OK;
}

// the flag word of a PASS, as hf_finish / hf_check report it: a pass that failed leaves nothing for the getters to answer for (they
// return HF_E_ARG until the next full pass, as hf_get_sample_labels does after a failed hf_sample_paths) — its labels, records and
// vectors are whatever the NaN or the underflow left
static int pass_flags_to_code(Pass& ps, unsigned fl) {
    const int code = flags_to_code(fl);
    if (code != HF_OK) ps.have_full = false;
    return code;
}

// the one-launch segment kernel gave up a wait (flag word `fl`): this pass runs two launches from now on, and the caller repeats the pass
static bool sync_fallback(Pass& ps, unsigned fl) {
    if (!(fl & HF_FLAG_SYNC) || !ps.seg_fused) return false;
    ps.seg_fused = false;
    std::fprintf(stderr, "[hmm_flagger_hip] one-launch segment kernel: a hand-off timed out; this context falls back to k_seg_prod + k_seg_fb\n");
    return true;
}

int hf_check(hf_ctx* ctx, void* stream) {
    if (!ctx) return set_err(HF_E_ARG, "hf_check: bad argument");
    Pass& ps = ctx->pass; const Track& tr = ctx->tr;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(hipSetDevice(tr.device));
    HIPCHK(hipMemcpyAsync(ps.h_flags, ps.d_flags, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    accumulate_kernel_times(ps);
    if (sync_fallback(ps, *ps.h_flags))   // as hf_finish
        return set_err(HF_E_RETRY, "a hand-off of the one-launch segment kernel timed out: the context now runs two launches, repeat hf_estep");
    return pass_flags_to_code(ps, *ps.h_flags);
}

// The total of a pass whose blocks wrote their partial vectors to the host (hf_rows.h part_host): rows_total_region and rows_total_ll restated —
// the same additions in the same order (nq interleaved accumulators per element over the region's blocks, then their sum; the log-likelihood
// by 64 strided sums and a halving tree), so h_total holds the bits the launch's own last blocks would have written.
extern "C++" {
template <int KT>
static void host_rows_total_t(Pass& ps) {
    const Track& tr = *ps.tr;
    constexpr int NA = (int) stat_acc_len(KT);
    const double* part = ps.h_part;
    const int nblk = ps.pass_rw_blocks, wpb = ps.pass_wpb, nt = 64 * wpb, Kctx = tr.K, nreg = tr.R;
    const int64_t V = tr.V, C = tr.C;
    const DevParams* P = ps.h_params;
    const int ncol = P->ncomp[3];
    const bool te = P->model_type == HF_MODEL_TRUNC_EXP_GAUSSIAN;
    const int rstride = 24 * Kctx + 16;
    double* out = ps.h_total;
    int nq = nt / NA;
    nq = nq < 1 ? 1 : (nq > 16 ? 16 : nq);
    for (int r = 0; r < nreg; r++) {
        double* dst = out + 1 + (int64_t) r * rstride;
        for (int v = 0; v < rstride; v++) dst[v] = 0.0;
        const int w0 = tr.h_rw_off[(size_t) r] / wpb, w1 = tr.h_rw_off[(size_t) r + 1] / wpb;
        if (w1 <= w0) continue;
        double red[NA], acc[16][NA];
        for (int q = 0; q < nq; q++) for (int i = 0; i < NA; i++) acc[q][i] = 0.0;
        for (int k = w0; k < w1; k++) {                              // (blocks in order, whole vectors: accumulator (k - w0) % nq takes block k, as on the device)
            double* a = acc[(k - w0) % nq];
            const double* pk = part + (size_t) k * NA;
            for (int i = 0; i < NA; i++) a[i] += pk[i];
        }
        for (int i = 0; i < NA; i++) {
            double tot = 0.0;
            for (int q = 0; q < nq; q++) tot += acc[q][i];
            red[i] = tot;
        }
        const StatAcc<KT>* Sa = reinterpret_cast<const StatAcc<KT>*>(red);
        for (int t = 0; t < 16; t++) dst[24 * Kctx + t] = Sa->trans[t];
        if (te) { dst[(0 * 2 + 0) * Kctx] = Sa->te_num; dst[(0 * 2 + 1) * Kctx] = Sa->te_den; }
        for (int st = 0; st < 3; st++)
            if (!(st == 0 && te)) {
                double* dd = dst + (st * 3) * 2 * Kctx;
                dd[(0 * 2 + 0) * Kctx] = Sa->g_mnum[st]; dd[(0 * 2 + 1) * Kctx] = Sa->g_den[st];
                dd[(1 * 2 + 0) * Kctx] = Sa->g_vnum[st]; dd[(1 * 2 + 1) * Kctx] = Sa->g_den[st];
                dd[(2 * 2 + 0) * Kctx] = Sa->g_den[st];  dd[(2 * 2 + 1) * Kctx] = Sa->g_den[st];
            }
        for (int cc = 0; cc < KT && cc < ncol; cc++) {
            double* dd = dst + (3 * 3) * 2 * Kctx;
            dd[(0 * 2 + 0) * Kctx + cc] = Sa->c_mnum[cc]; dd[(0 * 2 + 1) * Kctx + cc] = Sa->c_den[cc];
            dd[(1 * 2 + 0) * Kctx + cc] = Sa->c_vnum[cc]; dd[(1 * 2 + 1) * Kctx + cc] = Sa->c_den[cc];
            dd[(2 * 2 + 0) * Kctx + cc] = Sa->c_den[cc];  dd[(2 * 2 + 1) * Kctx + cc] = Sa->c_wden;
        }
    }
    {   // the log-likelihood: rows_total_ll's order
        const double* ll = part + (size_t) nblk * NA;
        double a[64];
        for (int l = 0; l < 64; l++) { double acc = 0.0; for (int64_t c = l; c < C; c += 64) acc += ll[c]; a[l] = acc; }
        for (int o = 32; o > 0; o >>= 1) for (int l = 0; l < o; l++) a[l] += a[l + o];
        out[0] = a[0];
    }
    out[V] = part[(size_t) nblk * NA + (size_t) C];      // the flag word
}
}
static void host_rows_total(Pass& ps) {
    if (ps.pass_kc <= 4) host_rows_total_t<4>(ps); else if (ps.pass_kc <= 8) host_rows_total_t<8>(ps); else host_rows_total_t<16>(ps);
}

// Completion of a pass: the stream's own stamp, or hipStreamSynchronize on the launch stream when the stamp is off or does not arrive —
// the HIP-defined ways to see the statistics block that the last kernel wrote into pinned host memory.
static int wait_total(Pass& ps, hipStream_t st, double* stats_host, bool host_total = false) {
    const Track& tr = *ps.tr;
    bool seen = false;
    if (ps.stream_stamp_ok) {
        // Completion through the stream itself: a 32-bit value that the command processor writes into the pinned block AFTER
        // everything enqueued before it has completed (hipStreamWriteValue32: a stream-ordered memory operation, so its order
        // against the kernel's own writes is defined — a stamp written by the last kernel itself has none: rounds 1-5 carried one behind
        // a checksum, and saw a stale element in one of ~2 000 passes without it), polled by the host.
        // Measured 4-5 us less per EM step than hipStreamSynchronize.  Bail-out: the stream after 2 s.
        volatile uint32_t* word = reinterpret_cast<volatile uint32_t*>(ps.h_flags) + 1;
        const uint32_t want = ++ps.stream_stamp;
        if (hipStreamWriteValue32(st, (void*) word, want, 0) == hipSuccess) {
            const auto t0 = std::chrono::steady_clock::now();
            long spins = 0;
            while (*word != want) {
                __builtin_ia32_pause();
                if ((++spins & 0xfffff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            seen = *word == want;
        } else { (void) hipGetLastError(); ps.stream_stamp_ok = false; }
        if (seen) {
            accumulate_kernel_times(ps);
            if (host_total) host_rows_total(ps);
            std::memcpy(stats_host, ps.h_total, (size_t) tr.V * 8);
            const unsigned fl2 = (unsigned) ps.h_total[tr.V];
            return sync_fallback(ps, fl2) ? HF_E_RETRY : pass_flags_to_code(ps, fl2);
        }
    }
    if (!seen) {
        HIPCHK(hipStreamSynchronize(st));
        // the stream has drained and the stamp still is not there: hipStreamWriteValue32 returns success on this stack but the write
        // does not land where the host polls — stop paying the 2 s bail-out in every later pass
        if (ps.stream_stamp_ok && ps.stream_stamp != 0 &&
            *(reinterpret_cast<volatile uint32_t*>(ps.h_flags) + 1) != ps.stream_stamp) {
            ps.stream_stamp_ok = false;
            std::fprintf(stderr, "[hmm_flagger_hip] the stream's completion stamp did not arrive; passes complete through hipStreamSynchronize from now on\n");
        }
    }
    accumulate_kernel_times(ps);   // events of the kernels before the last one have completed
    if (host_total) host_rows_total(ps);
    std::memcpy(stats_host, ps.h_total, (size_t) tr.V * 8);
    const unsigned fl = (unsigned) ps.h_total[tr.V];
    return sync_fallback(ps, fl) ? HF_E_RETRY : pass_flags_to_code(ps, fl);
}

static int pass_finish(Pass& ps, double* stats_host, void* stream) {
    const Track& tr = *ps.tr;
    if (!stats_host) return set_err(HF_E_ARG, "hf_finish: bad argument");
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(hipSetDevice(tr.device));
    // the reduction writes the V+1 doubles into pinned host memory over PCIe: no device-to-host copy afterwards
    double* out = ps.d_total_host ? ps.d_total_host : ps.d_total;
    const bool own_total = ps.pass_rows && !ps.pass_nb;   // k_row_stats already wrote the total
    int rc = own_total ? HF_OK
                       : (ps.pass_rows ? launch_nb_total(ps, st, out)
                                         : reduce_chunks(ps, ps.d_chunk_stats, nullptr, tr.C, out, stream));
    if (rc) return rc;
    if (pass_events(ps)) HIPCHK(hipEventRecord(ps.ev1, st));
    if (own_total && ps.pass_bound) {   // the pass wrote its total into a bound exchange slot (hf_bind_rank_total): fetch it from there
        HIPCHK(hipMemcpyAsync(ps.h_total, ps.d_rank_out, (size_t) tr.V * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ps.h_total + tr.V, ps.d_rank_flag, 8, hipMemcpyDeviceToHost, st));
    } else if (!ps.d_total_host)
        HIPCHK(hipMemcpyAsync(ps.h_total, ps.d_total, ((size_t) tr.V + 1) * 8, hipMemcpyDeviceToHost, st));
    rc = wait_total(ps, st, stats_host, own_total && ps.pass_host_total);
    if (rc == HF_E_RETRY) {   // the pass again, in two launches (the packed parameters are still in the pinned block)
        if (pass_events(ps)) HIPCHK(hipEventRecord(ps.ev0, st));
        rc = enqueue_pass(ps, &ps.last_p, ps.last_mode, st, true);
        if (rc) return rc;
        return pass_finish(ps, stats_host, stream);
    }
    return rc;
}
int hf_finish(hf_ctx* ctx, double* stats_host, void* stream) {
    return ctx ? pass_finish(ctx->pass, stats_host, stream) : set_err(HF_E_ARG, "hf_finish: bad argument");
}

// Multi-GPU counterpart of hf_finish: the rows of ALL chunks are in `rows_dev` (all-gathered, row_index_dev maps list
// position -> row); reduce them in the fixed order straight into pinned host memory, wait, translate the flags.
// With an exchange geometry the flag rows of all ranks are OR-ed in, so every rank reports the same error and nobody is
// left waiting in the next collective.  One synchronisation per EM step.
static int finish_rows(hf_ctx* ctx, const double* rows_dev, const int32_t* row_index_dev, int64_t n_rows, ExchangeGeom xg,
                       double* stats_host, void* stream, const char* who) {
    if (!ctx || !rows_dev || !stats_host || n_rows < 0) return set_err(HF_E_ARG, std::string(who) + ": bad argument");
    Pass& ps = ctx->pass; const Track& tr = ctx->tr;
    hipStream_t st = (hipStream_t) stream;
    HIPCHK(hipSetDevice(tr.device));
    double* out = ps.d_total_host ? ps.d_total_host : ps.d_total;
    int rc = reduce_chunks(ps, rows_dev, row_index_dev, n_rows, out, stream, xg);
    if (rc) return rc;
    if (pass_events(ps)) HIPCHK(hipEventRecord(ps.ev1, st));
    if (!ps.d_total_host)
        HIPCHK(hipMemcpyAsync(ps.h_total, ps.d_total, ((size_t) tr.V + 1) * 8, hipMemcpyDeviceToHost, st));
    return wait_total(ps, st, stats_host);
}

int hf_finish_gathered(hf_ctx* ctx, const double* rows_dev, const int32_t* row_index_dev, int64_t n_chunks, double* stats_host,
                       void* stream) {
    return finish_rows(ctx, rows_dev, row_index_dev, n_chunks, ExchangeGeom(), stats_host, stream, "hf_finish_gathered");
}

int hf_finish_exchange(hf_ctx* ctx, const double* rows_dev, const int32_t* row_index_dev, int64_t n_rows, int n_ranks,
                       int rows_per_rank, int flag_row, double* stats_host, void* stream) {
    if (n_ranks < 1 || rows_per_rank < 2 || flag_row < 0 || flag_row >= rows_per_rank)
        return set_err(HF_E_ARG, "hf_finish_exchange: bad exchange geometry");
    ExchangeGeom xg;
    xg.n_ranks = n_ranks; xg.rows_per_rank = rows_per_rank; xg.flag_row = flag_row;
    return finish_rows(ctx, rows_dev, row_index_dev, n_rows, xg, stats_host, stream, "hf_finish_exchange");
}

int hf_bind_chunk_stats(hf_ctx* ctx, double* rows_dev) {
    if (!ctx) return set_err(HF_E_ARG, "hf_bind_chunk_stats: bad argument");
    ctx->pass.d_chunk_stats = rows_dev ? rows_dev : ctx->pass.d_chunk_stats_own;   // (null: the pass's own array again)
    return HF_OK;
}

int hf_bind_rank_total(hf_ctx* ctx, double* total_dev, double* flag_row_dev) {
    if (!ctx || ((total_dev == nullptr) != (flag_row_dev == nullptr))) return set_err(HF_E_ARG, "hf_bind_rank_total: bad argument");
    Pass& ps = ctx->pass;
    ps.d_rank_out = total_dev; ps.d_rank_flag = flag_row_dev;
    return HF_OK;
}

int hf_write_flag_row(hf_ctx* ctx, double* row_dev, void* stream) {
    if (!ctx || !row_dev) return set_err(HF_E_ARG, "hf_write_flag_row: bad argument");
    Pass& ps = ctx->pass; const Track& tr = ctx->tr;
    HIPCHK(hipSetDevice(tr.device));
    if (ps.pass_rows && !ps.pass_nb && ps.pass_bound && row_dev == ps.d_rank_flag) return HF_OK;   // written by the pass itself
    hipLaunchKernelGGL(k_flag_row, dim3(1), dim3(64), 0, (hipStream_t) stream, ps.d_flags, row_dev);
    HIPCHK(hipGetLastError());
    return HF_OK;
}

// One EM step in one call: E-step with the model's current parameters, reduced statistics back on the host,
// then (do_mstep) HMM_estimateParameters.  What runHMMFlagger repeats (hmm_flagger.c:337-445) without going back
// to the caller between the two halves.
int hf_em_iterate(hf_ctx* ctx, hfm_model* model, int mode, int do_mstep, double tol, double* stats_host, int* converged,
                  void* stream) {
    if (!ctx || !model || !stats_host || (mode != HF_MODE_FULL && mode != HF_MODE_FORWARD_ONLY))
        return set_err(HF_E_ARG, "hf_em_iterate: bad argument");
    Pass& ps = ctx->pass;
    using clk = std::chrono::steady_clock;
    const auto tp = clk::now();
    hf_params p;
    hfm_params(model, &p);
    int rc = HF_OK;
    const auto t0 = clk::now();
    auto t1 = t0, t2 = t0;
    rc = hf_estep(ctx, &p, mode, stream);
    t1 = clk::now();
    if (rc == HF_OK) rc = hf_finish(ctx, stats_host, stream);
    t2 = clk::now();
    if (rc != HF_OK) return rc;
    em_step_tail(model, stats_host, do_mstep && mode == HF_MODE_FULL, tol, converged);
    if (ps.host_trace) {
        const auto t3 = clk::now();
        float gpu_ms = 0.f;
        (void) hipEventElapsedTime(&gpu_ms, ps.ev0, ps.ev1);
        auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        ps.ht[0] += us(t0, t1); ps.ht[1] += us(t1, t2); ps.ht[2] += us(t2, t3); ps.ht[3] += gpu_ms * 1e3; ps.ht[4] += us(tp, t0); ps.ht_n++;
    }
    return HF_OK;
}

// Windows may lie in no chunk (chunk_off[0] > 0, chunk_off[n_chunks] < n_windows: hf_create); the chunks themselves are contiguous.  A pass
// computes nothing for such a window, so the getters that answer for a range refuse one that touches it.
extern "C++" bool in_chunks(const Track& tr, int64_t first, int64_t last) {
    return tr.C > 0 && first >= tr.h_off.front() && last < tr.h_off.back();
}
extern "C++" bool all_in_chunks(const Track& tr) { return tr.N == 0 || in_chunks(tr, 0, tr.N - 1); }

static int pass_labels(Pass& ps, int8_t* labels_host) {
    const Track& tr = *ps.tr;
    if (!labels_host) return set_err(HF_E_ARG, "hf_get_labels: bad argument");
    if (!ps.have_full) return set_err(HF_E_ARG, "hf_get_labels: the last pass was not HF_MODE_FULL (a forward-only pass decodes nothing)");
    HIPCHK(hipSetDevice(tr.device));
    // through the context's pinned block (a pageable destination costs a staging copy inside the runtime: the first 1.5 MB download of a
    // process was measured at several milliseconds, in the middle of the command line's EM loop)
    // A KERNEL writes them into the context's pinned block (as the passes write their totals), the host copies them on: a process's first
    // device-to-host COPY into a fresh pinned block was measured at 8.9 ms (the second at 0.15 ms: profiles/r04e_cli_wall.txt) — in the
    // middle of the command line's EM loop, for the "initial" summary tables; the kernel takes ~0.1 ms the first time too.
    if (!ps.h_label && tr.N > 0 && ps.d_total_host) {
        char* p = pin_cache().acquire((size_t) tr.N + 16);
        void* dp = nullptr;
        if (p && hipHostGetDevicePointer(&dp, p, 0) == hipSuccess) { ps.h_label = reinterpret_cast<int8_t*>(p); ps.d_label_host = reinterpret_cast<int8_t*>(dp); }
        else { (void) hipGetLastError(); pin_cache().release(p); }
    }
    if (ps.d_label_host && tr.N > 0) {
        const int64_t n16 = (tr.N + 15) / 16;      // (d_label and the pinned block are padded to 16 bytes)
        hipLaunchKernelGGL(k_copy16, dim3((unsigned) ((n16 + 255) / 256)), dim3(256), 0, ps.last_stream, reinterpret_cast<const uint4*>(ps.d_label),
                           reinterpret_cast<uint4*>(ps.d_label_host), n16);   // (behind the pass, on its stream)
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ps.last_stream));
        std::memcpy(labels_host, ps.h_label, (size_t) tr.N);
    } else { HIPCHK(hipStreamSynchronize(ps.last_stream)); HIPCHK(hipMemcpy(labels_host, ps.d_label, (size_t) tr.N, hipMemcpyDeviceToHost)); }
    return HF_OK;
}

int hf_get_labels(hf_ctx* ctx, int8_t* labels_host) {
    return ctx ? pass_labels(ctx->pass, labels_host) : set_err(HF_E_ARG, "hf_get_labels: bad argument");
}

// The lazy block of the getters that read pair records (hf_get_forward_backward / hf_get_posterior, hf_get_interval_log_probs): the
// records of ALL windows and their scales, from the last full pass of the default algorithm
static int pass_all_records(Pass& ps) {
    const Track& tr = *ps.tr;
    if (!ps.recs_all || !ps.scales_all) {
        // the last full pass wrote no scales (statistics by emission row), or ran in sub-passes through the pass buffer (only its last sub-pass's records are left).  The segment kernel once
        // more over all segments, into the all-windows buffer (the tables of the pass are still in place: rows of A, parameters; labels,
        // scales and log-likelihood partials are rewritten with the same values)
        const int rc_ = all_records_buffer(ps);
        if (rc_) return rc_;
        if (!ps.d_scale_s) HIPCHK(hipMalloc((void**) &ps.d_scale_s, (size_t) tr.n_slots * 8));   // the scales: on first use (an EM pass writes none)
        // On the stream of the pass itself (the null stream is not ordered against a non-blocking user stream), and its flag
        // word is read like a pass's: a hand-off that timed out in THIS launch would otherwise leave silently wrong vectors — the context
        // falls back to two launches and the re-run is repeated; any other flag is the pass's own error, reported as hf_check would.
        hipStream_t st = ps.last_stream;
        for (int attempt = 0;; attempt++) {
            if (!ps.seg_fused) {
                if (!ps.d_segQ) HIPCHK(hipMalloc((void**) &ps.d_segQ, (size_t) tr.nseg * 64 * 16 * 8));
                hipLaunchKernelGGL(k_seg_prod, dim3((unsigned) tr.nseg), dim3(64), seg_lds_bytes(), st, tr.d_seg, tr.d_arow, ps.d_lutA, ps.d_segQ, ps.d_Pseg);
            }
            const unsigned epoch = ++ps.seg_epoch;
            launch_seg_fb(ps, st, true, ps.d_recs_all, -1, epoch, epoch, false);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(ps.h_flags, ps.d_flags, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            const unsigned fl = *ps.h_flags;
            if (attempt == 0 && sync_fallback(ps, fl)) {
                unsigned keep = fl & ~(unsigned) HF_FLAG_SYNC;        // (the pass's own flags stay for a later hf_check)
                HIPCHK(hipMemcpyAsync(ps.d_flags, &keep, 4, hipMemcpyHostToDevice, st));
                HIPCHK(hipStreamSynchronize(st));
                continue;
            }
            const int code = flags_to_code(fl);
            if (code != HF_OK) return code;
            break;
        }
        ps.recs_all = true; ps.scales_all = true;
    }
    return HF_OK;
}

static int pass_forward_backward(Pass& ps, int64_t first, int64_t n, double* f_host, double* b_host, double* scales_host) {
    const Track& tr = *ps.tr;
    if (first < 0 || n < 0 || first + n > tr.N) return set_err(HF_E_ARG, "hf_get_forward_backward: bad range");
    if (n > 0 && !in_chunks(tr, first, first + n - 1)) return set_err(HF_E_ARG, "hf_get_forward_backward: the range holds a window outside every chunk");
    if (!ps.have_full)   // a forward-only pass of the segment kernels keeps everything in registers: nothing of THIS pass to return
        return set_err(HF_E_ARG, "hf_get_forward_backward: the last pass was not HF_MODE_FULL (forward, backward and scale values would be stale)");
    HIPCHK(hipSetDevice(tr.device));
    if (n == 0) return HF_OK;
    HIPCHK(hipStreamSynchronize(ps.last_stream));   // (the copies below run on the null stream: not ordered against a non-blocking stream by itself)
    if (scales_host && !ps.fb_recs) HIPCHK(hipMemcpy(scales_host, ps.d_scale + first, (size_t) n * 8, hipMemcpyDeviceToHost));
    if (!f_host && !b_host && !ps.fb_recs) return HF_OK;
    if (ps.fb_recs) {   // pair records (hf_seg.h): b_t is the second half of the record at pos[t], f_t the first half of the one at pos_f[t]
        const int rc_ = pass_all_records(ps);
        if (rc_) return rc_;
        // the positions of a range are scattered over the plan: gathered on the device, one copy back (maps uploaded on first use)
        if (!ps.d_slot_of) {
            HIPCHK(hipMalloc((void**) &ps.d_slot_of, (size_t) tr.N * 4));
            std::vector<int32_t> so((size_t) tr.N, 0);     // window -> slot (the scales are kept in slot order)
            for (const SegDesc& d : tr.h_segs)
                for (int64_t x = 0; x < d.n; x++) so[(size_t) (d.t0 + x)] = seg_slot(d, x);
            HIPCHK(hipMemcpy(ps.d_slot_of, so.data(), (size_t) tr.N * 4, hipMemcpyHostToDevice));
        }
        double* d_out = nullptr;
        HIPCHK(hipMalloc((void**) &d_out, (size_t) n * 9 * 8));
        hipLaunchKernelGGL(k_gather_fb, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ps.last_stream, first, n, tr.d_pos, tr.d_pos_f, ps.d_slot_of,
                           ps.d_recs_all, ps.d_scale_s, d_out, d_out + n * 4, d_out + n * 8);
        HIPCHK(hipStreamSynchronize(ps.last_stream));
        hipError_t e1 = hipSuccess, e2 = hipSuccess, e3 = hipSuccess;
        if (f_host) e1 = hipMemcpy(f_host, d_out, (size_t) n * 32, hipMemcpyDeviceToHost);
        if (b_host) e2 = hipMemcpy(b_host, d_out + n * 4, (size_t) n * 32, hipMemcpyDeviceToHost);
        if (scales_host) e3 = hipMemcpy(scales_host, d_out + n * 8, (size_t) n * 8, hipMemcpyDeviceToHost);
        hipFree(d_out);
        HIPCHK(e1); HIPCHK(e2); HIPCHK(e3);
        return HF_OK;
    }
    // f and b live tile-major / lane-minor on the device (hf_scan.h fb_slot): fetch the tiles that cover the range and
    // put every window's four values back in window order
    constexpr int64_t L = HF_SCAN_L, TW = 64 * L;
    auto locate = [&](int64_t t, int64_t* tile, int* lane, int* j) {
        size_t c = (size_t) (std::upper_bound(tr.h_off.begin(), tr.h_off.end(), t) - tr.h_off.begin()) - 1;
        const int64_t w = t - tr.h_off[c];
        *tile = tr.h_tile0[c] + w / TW;
        const int rem = (int) (w % TW);
        *lane = rem / (int) L; *j = rem % (int) L;
    };
    int64_t tile_lo, tile_hi; int lane, j;
    locate(first, &tile_lo, &lane, &j);
    locate(first + n - 1, &tile_hi, &lane, &j);
    const size_t tile_doubles = (size_t) TW * 4;
    std::vector<double> buf((size_t) (tile_hi - tile_lo + 1) * tile_doubles);
    for (int which = 0; which < 2; which++) {
        double* dst = which == 0 ? f_host : b_host;
        if (!dst) continue;
        const double* src = which == 0 ? ps.d_f : ps.d_b;
        HIPCHK(hipMemcpy(buf.data(), src + (size_t) tile_lo * tile_doubles, buf.size() * 8, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; i++) {
            int64_t tile;
            locate(first + i, &tile, &lane, &j);
            for (int h = 0; h < 2; h++) {
                const size_t slot = (size_t) ((((tile - tile_lo) * L + j) * 2 + h) * 64 + lane);
                dst[i * 4 + 2 * h] = buf[slot * 2]; dst[i * 4 + 2 * h + 1] = buf[slot * 2 + 1];
            }
        }
    }
    return HF_OK;
}

int hf_get_forward_backward(hf_ctx* ctx, int64_t first, int64_t n, double* f_host, double* b_host, double* scales_host) {
    return ctx ? pass_forward_backward(ctx->pass, first, n, f_host, b_host, scales_host) : set_err(HF_E_ARG, "hf_get_forward_backward: bad range");
}

static int pass_posterior(Pass& ps, int64_t first, int64_t n, double* post_host) {
    if (!post_host) return set_err(HF_E_ARG, "hf_get_posterior: bad argument");
    // (before the buffers below are sized by n: a negative n would throw out of the C ABI)
    if (first < 0 || n < 0 || first + n > ps.tr->N) return set_err(HF_E_ARG, "hf_get_posterior: bad range");
    if (n > 0 && !in_chunks(*ps.tr, first, first + n - 1)) return set_err(HF_E_ARG, "hf_get_posterior: the range holds a window outside every chunk");
    std::vector<double> f((size_t) n * 4), b((size_t) n * 4), sc((size_t) n);
    int rc = pass_forward_backward(ps, first, n, f.data(), b.data(), sc.data());
    if (rc) return rc;
    for (int64_t i = 0; i < n; i++) { // hmm.c:671-685
        double total = 0.0;
        for (int s = 0; s < 4; s++) { post_host[i * 4 + s] = f[i * 4 + s] * b[i * 4 + s] * sc[i]; total += post_host[i * 4 + s]; }
        for (int s = 0; s < 4; s++) post_host[i * 4 + s] /= total;
    }
    return HF_OK;
}
int hf_get_posterior(hf_ctx* ctx, int64_t first, int64_t n, double* post_host) {
    return ctx ? pass_posterior(ctx->pass, first, n, post_host) : set_err(HF_E_ARG, "hf_get_posterior: bad argument");
}

int hf_set_profiling(hf_ctx* ctx, unsigned kernel_mask) {
    if (!ctx) return set_err(HF_E_ARG, "hf_set_profiling: bad argument");
    Pass& ps = ctx->pass; const Track& tr = ctx->tr;
    HIPCHK(hipSetDevice(tr.device));
    // timing-only events: no system-scope fence when they fire (the default event writes back and invalidates the caches — k_seg_fb's 130 MB
    // of records would leave the L2 before k_pair_sums reads them: a sampled step was measured 15 us slower than an unsampled one)
    if (kernel_mask && !ps.kev[0])
        for (int i = 0; i < 2 * HF_NKERNELS; i++)
            if (hipEventCreateWithFlags(&ps.kev[i], hipEventDisableSystemFence) != hipSuccess) { (void) hipGetLastError(); HIPCHK(hipEventCreate(&ps.kev[i])); }
    ps.prof_mask = kernel_mask & (((1u << HF_NKERNELS) - 1u) | HF_PROF_PASS);
    for (int i = 0; i < HF_NKERNELS; i++) { ps.kran[i] = false; ps.ksum[i] = 0.0; ps.kcount[i] = 0; }
    return HF_OK;
}

int hf_set_profiling_stride(hf_ctx* ctx, int every_nth_pass) {
    if (!ctx || every_nth_pass < 1) return set_err(HF_E_ARG, "hf_set_profiling_stride: bad argument");
    Pass& ps = ctx->pass;
    ps.prof_stride = every_nth_pass; ps.prof_pass = 0;
    return HF_OK;
}

int hf_kernel_time_sums(hf_ctx* ctx, double sum_ms[HF_NKERNELS], int64_t launches[HF_NKERNELS]) {
    if (!ctx || !sum_ms || !launches) return set_err(HF_E_ARG, "hf_kernel_time_sums: bad argument");
    Pass& ps = ctx->pass;
    for (int i = 0; i < HF_NKERNELS; i++) { sum_ms[i] = ps.ksum[i]; launches[i] = ps.kcount[i]; }
    return HF_OK;
}

int hf_kernel_times(hf_ctx* ctx, float ms[HF_NKERNELS]) {
    if (!ctx || !ms || !ctx->pass.prof_mask) return set_err(HF_E_ARG, "hf_kernel_times: profiling is off");
    Pass& ps = ctx->pass;
    for (int i = 0; i < HF_NKERNELS; i++) {
        ms[i] = 0.f;
        if (ps.kran[i]) {
            if (ps.klast_ok[i]) ms[i] = ps.klast[i];       // hf_finish has read this pair already
            else HIPCHK(hipEventElapsedTime(&ms[i], ps.kev[2 * i], ps.kev[2 * i + 1]));
        }
    }
    return HF_OK;
}

const char* hf_kernel_name(int k) {
    // slots 1-3 belonged to round 1's tile kernels (never launched since round 2); k_nb_total is the only kernel left in the
    // HF_K_ROWS_TOTAL slot (the Gaussian models' total is part of k_row_stats since round 3)
    static const char* names[HF_NKERNELS] = {"k_tables", "(retired)", "(retired)", "(retired)", "k_stats_tile", "k_chunk_stats",
                                             "k_reduce", "k_emit_rows", "k_fwd_seq", "k_bwd_seq", "k_pair_sums", "k_row_stats",
                                             "k_nb_total", "k_seg_prod", "k_seg_fb", "k_arows"};
    return k >= 0 && k < HF_NKERNELS ? names[k] : "?";
}

// self-test hook (tests/test_estep_gpu.py): quotient through prediv/divp next to the plain a / d, element-wise
__global__ void k_selftest_div(int64_t n, const double* __restrict__ a, const double* __restrict__ d,
                               double* __restrict__ fast, double* __restrict__ exact, int32_t* __restrict__ safe) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fast[i] = divp(a[i], prediv(d[i]));
    exact[i] = a[i] / d[i];
    safe[i] = (div_operand_safe(a[i]) && d[i] != 0.0 && div_operand_safe(d[i])) ? 1 : 0;
}

int hf_selftest_division(int device, int64_t n, const double* a, const double* d, double* fast, double* exact, int32_t* safe) {
    if (n < 0 || !a || !d || !fast || !exact || !safe) return set_err(HF_E_ARG, "hf_selftest_division: bad argument");
    if (hf_device_count() <= 0) return set_err(HF_E_NOGPU, "hf_selftest_division: no HIP device");
    HIPCHK(hipSetDevice(device));
    double *da = nullptr, *dd = nullptr, *df = nullptr, *de = nullptr; int32_t* ds = nullptr;
    const size_t b = (size_t) (n ? n : 1) * 8;
    HIPCHK(hipMalloc((void**) &da, b)); HIPCHK(hipMalloc((void**) &dd, b)); HIPCHK(hipMalloc((void**) &df, b));
    HIPCHK(hipMalloc((void**) &de, b)); HIPCHK(hipMalloc((void**) &ds, b));
    HIPCHK(hipMemcpy(da, a, (size_t) n * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dd, d, (size_t) n * 8, hipMemcpyHostToDevice));
    if (n) hipLaunchKernelGGL(k_selftest_div, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, n, da, dd, df, de, ds);
    HIPCHK(hipMemcpy(fast, df, (size_t) n * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(exact, de, (size_t) n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(safe, ds, (size_t) n * 4, hipMemcpyDeviceToHost));
    hipFree(da); hipFree(dd); hipFree(df); hipFree(de); hipFree(ds);
    return HF_OK;
}

// self-test hook (tests/test_estep_gpu.py): the emission densities' exp on the device (hf_exp.h) next to the same function and libm's exp on the host
__global__ void k_selftest_exp(int64_t n, const double* __restrict__ x, double* __restrict__ y) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = hf_exp(x[i]);      // (the restatement itself, whichever exp the emission kernels were built with)
}
int hf_selftest_exp(int device, int64_t n, const double* x, double* dev_out, double* host_out, double* libm_out) {
    if (n < 0 || !x || !dev_out || !host_out || !libm_out) return set_err(HF_E_ARG, "hf_selftest_exp: bad argument");
    if (hf_device_count() <= 0) return set_err(HF_E_NOGPU, "hf_selftest_exp: no HIP device");
    HIPCHK(hipSetDevice(device));
    double *dx = nullptr, *dy = nullptr;
    const size_t b = (size_t) (n ? n : 1) * 8;
    HIPCHK(hipMalloc((void**) &dx, b)); HIPCHK(hipMalloc((void**) &dy, b));
    HIPCHK(hipMemcpy(dx, x, (size_t) n * 8, hipMemcpyHostToDevice));
    if (n) hipLaunchKernelGGL(k_selftest_exp, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, n, dx, dy);
    HIPCHK(hipMemcpy(dev_out, dy, (size_t) n * 8, hipMemcpyDeviceToHost));
    hipFree(dx); hipFree(dy);
    for (int64_t i = 0; i < n; i++) { host_out[i] = hf_exp(x[i]); libm_out[i] = std::exp(x[i]); }
    return HF_OK;
}

int hf_last_kernel_ms(hf_ctx* ctx, float* ms) {
    if (!ctx || !ms || !ctx->pass.ev_valid) return set_err(HF_E_ARG, "hf_last_kernel_ms: nothing timed yet");
    Pass& ps = ctx->pass;
    HIPCHK(hipEventSynchronize(ps.ev1));
    HIPCHK(hipEventElapsedTime(ms, ps.ev0, ps.ev1));
    return HF_OK;
}

} // extern "C"

#include "hf_batch.h"

// the range getters and the alpha statistics, kernels and host side; they need only the __device__ helpers of hf_decode.h (its
// kernels belong to hf_decoders.hip), and every kernel header of this unit's own stands above
#define HF_HELPERS_ONLY

// The getters' build switches stand here, with the unit's others (EXTRA= of the Makefile reaches this file; the tests read the values
// from it).  Pieces and parts per device batch (hf_jobs.h): the interval getter's, and those of the moments, run moments and entropy
// getters (a piece's triple is 384 bytes: 96 MB of them at most)
#ifndef HF_IV_BATCH_PIECES
#define HF_IV_BATCH_PIECES (1 << 20)
#endif
#ifndef HF_IV_BATCH_PARTS
#define HF_IV_BATCH_PARTS (1 << 20)
#endif
#ifndef HF_MO_BATCH_PIECES
#define HF_MO_BATCH_PIECES (1 << 18)
#endif
#ifndef HF_MO_BATCH_PARTS
#define HF_MO_BATCH_PARTS (1 << 20)
#endif
// ... and the breakpoint getter's: a window's weight is 12 bytes, 2^15 pieces of 512 windows about 200 MB.  A part has at least one
// piece, so the parts' cap never binds before the pieces'
#ifndef HF_BP_BATCH_PIECES
#define HF_BP_BATCH_PIECES (1 << 15)
#endif
#ifndef HF_BP_BATCH_PARTS
#define HF_BP_BATCH_PARTS (1 << 15)
#endif
#include "hf_getters.h"
