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
#include "hf_device.h"
#include <hip/hip_ext.h>
#include "../../include/hmm_flagger_model.h"
#ifndef HF_SCAN_L
#define HF_SCAN_L 4   // consecutive windows per lane in the scan kernels
#endif
#include <string>
#include <algorithm>
#include <vector>
#include <cstring>
#include <cstdio>
#include <cmath>
#include <atomic>
#include <functional>
#include <condition_variable>
#include <mutex>
#include <memory>
#include <chrono>
#include <cstdlib>

#include <thread>
#include <unistd.h>
#include <immintrin.h>
static thread_local std::string g_err;

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
static int set_err(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) \
    return set_err(HF_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// entries of one statistics vector (hf_chunks.h StatAcc<KT>): what k_row_stats' blocks hand on per region
static constexpr size_t stat_acc_len(int kt) { return (size_t) (16 + 9 + 2 + 3 * kt + 1); }

// Device memory of hf_create and of every pass comes out of a few SLABS (round 5: ~45 hipMalloc calls and as many hipFree were ~0.5 ms
// of a 4 ms hf_create): bump allocation, 256-byte granules, freed all at once.  `first` sizes the first block; later blocks are 64 MiB.
struct Slab {
    std::vector<std::pair<char*, size_t>> blocks; char* cur = nullptr; size_t left = 0, first = 0;
    static size_t granule(size_t bytes) { return ((bytes ? bytes : 8) + 255) & ~(size_t) 255; }
    void* alloc(size_t bytes) {
        bytes = granule(bytes);
        if (bytes > left) {
            const size_t want = std::max(bytes, blocks.empty() ? first : (size_t) 64 << 20);
            char* p = nullptr;
            if (hipMalloc((void**) &p, want) != hipSuccess) {
                (void) hipGetLastError();
                if (want == bytes || hipMalloc((void**) &p, bytes) != hipSuccess) return nullptr;   // (a smaller block: just this request)
                blocks.emplace_back(p, bytes);
                return p;                                                                         // (the current block keeps its remainder)
            }
            blocks.emplace_back(p, want);
            cur = p; left = want;
        }
        char* r = cur;
        cur += bytes; left -= bytes;
        return r;
    }
    void release() { for (auto& b : blocks) hipFree(b.first); blocks.clear(); cur = nullptr; left = 0; }
};

// THE TRACK: what hf_create builds from the windows and nothing writes afterwards — the window store, the emission keys and slow windows,
// the tiles, the rows of A, the segment plan, the statistics plan, the job list of k_tables.  Every pass over it reads it.
struct Track {
    int device = 0, algo = HF_ALGO_SCAN;
    Slab slab;
    int64_t N = 0; int32_t C = 0; int32_t maxT = 0;
    int R = 1, K = 2;
    int64_t V = 0;                 // per-chunk stats vector length
    hf_windows meta{};             // scalar options only (pointers cleared)
    size_t lds_max = 64 * 1024;    // LDS one workgroup may use (hipDeviceAttributeMaxSharedMemoryPerBlock)
    double beta_star = 1.0;
    size_t params_bytes = 0;       // the parameter block (DevParams + one DevRegion per region past the first)
    // device-resident window store
    int64_t* d_off = nullptr;      // [C+1]
    uint32_t* d_rec = nullptr;     // [N]
    double* d_beta = nullptr;      // [N]
    uint64_t* d_regmask = nullptr; // [C] bit r set if region r occurs in the chunk
    unsigned* d_setup_flags = nullptr;   // k_setup's flag word (a region index out of range): read once, at the end of hf_create
    std::vector<int64_t> h_off; std::vector<int32_t> h_tile0;   // host copies for hf_get_forward_backward
    std::vector<int32_t> h_cs, h_ce;                            // Chunk.s / Chunk.e (a window's length in bases: hf_get_count_moments)
    // scan algorithm: tile table (per-chunk statistics, HF_ALGO_SEQ)
    TileDesc* d_tile_desc = nullptr;
    int ntiles = 0; int32_t* d_chunk_tile0 = nullptr;
    // per-iteration emission rows (k_tables): keys = occurring (region, x, x_prev) of interior windows,
    // slow = chunk-first and contig-end windows (beta != beta_star), ascending; slow_off[c] = chunk c's first entry
    int M = 1; int64_t n_lut = 0;
    int n_keys = 0; int32_t* d_keys = nullptr;
    int n_slow = 0; int64_t* d_slow_w = nullptr; int32_t* d_slow_off = nullptr;
    TableJob* d_jobs = nullptr; TabWork tabwork{};   // the job list of the per-pass tables (hf_scan.h k_build_jobs), built once; a pass adds its tables
    // rows of A_t = T_t∘e_t (hf_seg.h): one per (emission key, transition class) that occurs at an interior window, then one
    // per slow window; d_arow[t] = the row of window t (bit 31: chunk-first), d_arow_src / d_arow_cls = where a row comes from
    int32_t* d_arow = nullptr; int32_t* d_arow_src = nullptr; int32_t* d_arow_cls = nullptr;
    int n_arows = 0, n_combo = 0;
    // segment kernels (hf_seg.h): the forward-backward of the statistics-by-row path
    SegDesc* d_seg = nullptr; int nseg = 0; int32_t* d_chunk_seg0 = nullptr; int64_t n_slots = 0;
    std::vector<SegDesc> h_segs;                // the segment descriptors (the getters derive a window's slot from them)
    std::vector<int32_t> h_cseg0;               // first segment of every chunk (+ the end)
    int seg_nc = 0;                    // row blocks a segment workgroup keeps in LDS across its three walks (hf_seg.h: chosen so that all segments stay resident)
    // SUB-PASSES (round 5): a context whose records would not fit the Infinity Cache (256 MB; BASELINE configs[2] writes 130 MB) cuts its
    // chunk list into sub-passes of whole chunks; a pass runs k_seg_fb then k_pair_sums per sub-pass through ONE buffer that holds a
    // sub-pass's positions [p0, p1) at a time (Pass::d_recs; the plan's groups are numbered sub-pass by sub-pass, so a sub-pass's records are
    // contiguous) — the records never travel to HBM and back.  Everything that needs the records of ALL windows at once (the getters,
    // per-chunk statistics) runs the segment kernel into Pass::d_recs_all instead (allocated on first use; = d_recs with one sub-pass).
    struct SubPass { int c0, c1, seg0, seg1, g0, g1; int64_t p0, p1; };
    std::vector<SubPass> subs;
    // statistics by emission row (hf_rows.h): the static plan
    bool rows_ready = false;
    int n_groups = 0, n_rowwaves = 0;
    int rs_bpw = 1;                   // batches of 16 row slots per wavefront of k_row_stats
    bool plan_compact = false;        // the groups' records back to back (sparse rows) instead of 64 positions per group
    int32_t* d_grp_off = nullptr;     // compact plan: first position of every group (+ the end)
    int32_t* d_grp_ar = nullptr; int32_t* d_grp_n = nullptr;   // per group: its row of A, its pairs
    int32_t* d_pos = nullptr; int64_t n_pos = 0;   // [N] position of every window's pair record in the records (plan order; slot order without a plan)
    int32_t* d_pos_f = nullptr;    // [N] position of the record that holds every window's f (getters)
    RowSlot* d_rowslots = nullptr; int32_t* d_rw_region = nullptr; int32_t* d_rw_off = nullptr; std::vector<int32_t> h_rw_off;
    int32_t* d_bin_off = nullptr; int32_t* d_bin_list = nullptr;   // negative_binomial count-data plan: the row slots of every (region, x) bin
    std::vector<std::pair<const char*, double>> create_phases;   // hf_create_phases
    unsigned long long* d_seg_trace = nullptr;   // -DHF_SEG_TRACE builds only
};

// THE PASS STATE over a track: everything hf_estep, hf_finish and the getters write — parameter block, tables, rows of A, hand-off flags and
// epochs, pair records, sums, labels, flag word, totals, the pinned result block, profiling events.  A context has one; a batch
// (hf_batch.h) one per model, over the context's track.  Its device arrays come out of its own slab, sized by pass_layout.
struct Pass {
    const Track* tr = nullptr;
    Slab slab;
    // settings (a batch model starts from the context's: hf_batch_create)
    int stats_mode = HF_STATS_CHUNKS;
    bool seg_fused = true, seg_test_timeout = false;   // one-launch mode (hf_seg.h); a timed-out wait switches the pass to two launches
    bool kp_ok = true;             // HF_PARAMS_COPY=1 switches the kernel-argument path off
    bool host_total_ok = true;     // the total of a one-GPU pass summed by the HOST (HF_TOTAL=device: off)
    bool stream_stamp_ok = true;   // wait_total: completion through hipStreamWriteValue32 (HF_STREAM_STAMP=0: off)
    bool host_trace = false; double ht[5] = {0, 0, 0, 0, 0}; long ht_n = 0;   // HF_HOST_TRACE=1: where an EM step's host time goes
    // device arrays (slab)
    int8_t* d_label = nullptr;     // [N]
    double* d_chunk_stats = nullptr; // [C][V]: d_chunk_stats_own, or an exchange buffer (hf_bind_chunk_stats)
    double* d_chunk_stats_own = nullptr;
    double* d_total = nullptr;     // [V]
    unsigned* d_flags = nullptr;
    unsigned* d_done = nullptr;    // k_row_stats: blocks finished per part (the last one sums the part: hf_rows.h)
    DevParams* d_params = nullptr;
    double* d_lutE = nullptr; double* d_lutC = nullptr; double* d_Es = nullptr; double* d_Cs = nullptr;   // emission rows: keys, then slow windows
    double* d_lutA = nullptr;      // rows of A, then the identity row (pass_create writes it; no kernel does)
    double* d_tile_ll = nullptr;
    double* d_tile_stats = nullptr; // [ntiles][R][NA(16)]
    unsigned* d_seg_ready = nullptr; double* d_seg_ll = nullptr; double* d_Pseg = nullptr;
    double* d_recs = nullptr;      // pair records { f_{t-1}, b_t } of k_seg_fb, plan order; fb_recs: the last full pass wrote them
    double* d_grp_sums = nullptr; double* d_chunk_ll = nullptr; double* d_rw_stats = nullptr;   // statistics by emission row: per group, per chunk, per row wavefront
    double* d_E = nullptr;         // [N][16] emission rows, HF_ALGO_SEQ only
    double* d_f = nullptr;         // [ntiles][L][2][64] double2: tile-major, lane-minor (hf_scan.h fb_slot), HF_ALGO_SEQ only
    double* d_b = nullptr;         // same layout
    double* d_scale = nullptr;     // [N], HF_ALGO_SEQ only (hf_seg.h keeps the scales by slot)
    TabWork tabwork{};             // the track's job list with this pass's tables
    // allocated on first use (pass_destroy frees them)
    double* d_recs_all = nullptr;  // the records of ALL windows (= d_recs with one sub-pass)
    double* d_segQ = nullptr;      // [nseg][8][64] double2: lane products, lane-minor (two-launch mode only)
    double* d_scale_s = nullptr;   // [n_slots] scales by slot (hf_get_forward_backward)
    int32_t* d_slot_of = nullptr;  // window -> slot, built from the track's h_segs by the first getter call
    // negative_binomial model: device copies of hf_params.nb_* and the count data (first negative_binomial pass)
    double *d_nbE = nullptr, *d_nbP = nullptr, *d_nbDig = nullptr, *d_nbR = nullptr, *d_nbBeta = nullptr;   // d_nbE owns ONE buffer: E | P | dig | r | beta
    double *d_tile_hist = nullptr, *d_slot_h = nullptr, *d_H = nullptr;                                   // d_tile_hist owns ONE buffer: tile_hist | slot_h | H
    char* h_nb[2] = {nullptr, nullptr}; hipEvent_t nb_ev[2] = {nullptr, nullptr}; bool nb_ev_used[2] = {false, false}; unsigned nb_turn = 0;   // pinned staging of those tables
    double* h_part = nullptr; double* d_part_host = nullptr; size_t part_cap = 0;   // pinned partials [n_rw_blocks][NA] | [C] | flag word, their device address
    int8_t* h_label = nullptr;     // pinned [N]: staging of hf_get_labels, taken from the process's pinned cache on first use (1.5 MB of pinning = 0.15 ms of hf_create until round 5)
    int8_t* d_label_host = nullptr; // its device address (a kernel writes the labels there)
    // the pinned block: result vector (+ flag word) | flag word of hf_check | parameter block
    double* h_total = nullptr;     // pinned [V+1]: reduced vector + flag word, one copy per pass
    double* d_total_host = nullptr; // device address of the pinned h_total: k_reduce writes the result straight to the host
    unsigned* h_flags = nullptr; DevParams* h_params = nullptr;
    KParams kparams{};             // the parameter block as kernel arguments of k_tables (one region: pack_kparams)
    bool kp_now = false;           // this pass uses them
    // profiling
    hipEvent_t ev0 = nullptr, ev1 = nullptr; bool ev_valid = false;
    double ksum[HF_NKERNELS] = {}; int64_t kcount[HF_NKERNELS] = {};   // accumulated by hf_finish while profiling is on
    float klast[HF_NKERNELS] = {}; bool klast_ok[HF_NKERNELS] = {};      // the last pass's durations as hf_finish read them (hf_kernel_times returns these)
    unsigned prof_mask = 0;        // bit k: kernel k (HF_K_*) is bracketed by kev[2k], kev[2k+1]
    int prof_stride = 1; long prof_pass = 0; bool prof_now = true;   // events only in every prof_stride-th pass (hf_set_profiling_stride)
    hipEvent_t kev[2 * HF_NKERNELS] = {}; bool kran[HF_NKERNELS] = {};
    // what the last pass was and did
    hf_params last_p{}; int last_mode = HF_MODE_FULL;   // what the last hf_estep was given (the fallback re-runs the pass)
    hipStream_t last_stream = nullptr;                  // ... and the stream it ran on (the getters' re-run of the segment kernel goes there)
    bool have_full = false, launch_failed = false;
    bool pass_seg = false;         // the last pass ran the segment kernels (log-likelihood partials per segment)
    bool pass_rows = false; int pass_kc = 0, pass_wpb = 4;
    bool pass_nb = false;          // the last rows-mode pass ran the negative_binomial kernels (hf_nb_rows.h)
    bool pass_host_total = false; int pass_rw_blocks = 0;
    uint32_t stream_stamp = 0;
    double* d_rank_out = nullptr; double* d_rank_flag = nullptr;   // hf_bind_rank_total: where a rows-mode pass writes its total / flag word
    bool pass_bound = false;       // the last pass wrote them there
    bool fb_recs = false, pass_pairs_done = false;   // pass_pairs_done: enqueue_pass ran k_pair_sums itself (per sub-pass)
    bool recs_all = false;         // d_recs_all holds the records of every window of the last full pass
    bool scales_all = false;       // ... and d_scale_s its scales (an EM pass writes none: 8 of its 72 bytes per window that only
                                   // hf_get_forward_backward reads — the getter runs the segment kernel again, with the array)
    unsigned seg_epoch = 0;        // hand-off flags of the one-launch segment kernel are stamped with the launch's epoch
};

// THE DECODER STATE of the path decoders (hf_decode.h): buffers of its own, allocated by the decoder's first call, never shared with a pass or
// the other decoder.  The device arrays come out of a slab sized by the decoder's layout (vit_arrays, smp_arrays).
struct Decoder {
    Slab slab;
    DevParams* h_params = nullptr;             // pinned
    DevParams* d_params = nullptr; double* d_nbE = nullptr; unsigned* d_flags = nullptr;
    double2* d_rows = nullptr;                 // SCAN: [n_slots][8] slot-ordered pieces; SEQ: [N][8] window order
    double* d_P = nullptr; double* d_S = nullptr; double* d_vin = nullptr;     // SCAN: phases A, B
    int* d_PE = nullptr; int* d_SE = nullptr; long long* d_vinE = nullptr;     // ... their exponent sums (a decoder with a score)
    bool alloc = false, launched = false, done = false;
    void release() { if (h_params) hipHostFree(h_params); slab.release(); }
};

// a decoder that leaves one label per window and values per chunk (dec_finish_chunks, dec_labels, dec_chunk_values)
struct LabelDecoder : Decoder {
    int8_t* d_label = nullptr;
    double* d_chunk = nullptr;                 // [values per chunk][C]
    std::vector<double> h_chunk;               // ... of the last finished run
};

// most-probable-path decoding (hf_viterbi.h); the chunk values: the scores
struct Viterbi : LabelDecoder {
    uint8_t* d_bp = nullptr;                   // backpointer bytes (slot order / window order)
    int8_t* d_final = nullptr;
    uint8_t* d_lmap = nullptr; uint8_t* d_smap = nullptr; uint8_t* d_sexit = nullptr;   // SCAN: phases C, D
};

// minimum-run-length Viterbi (hf_minlen.h): rows always in window order, one 16-bit backpointer word per window; the chunk values: the scores
struct MinLenViterbi : LabelDecoder {
    uint16_t* d_bp = nullptr; uint8_t* d_final = nullptr;     // ... and the final lane of every chunk
    // hf_viterbi_minlen_joined: the groups of a call, window ranges [G + 1] and first chunks [G], G <= C
    int64_t* d_goff = nullptr; int32_t* d_gchunk = nullptr;
    std::vector<int64_t> h_goff; std::vector<int32_t> h_gchunk;
};

// THE PER-SAMPLE PART of the two samplers: `cap` samples in a slab of its own, replaced when a call asks for more (smp_grow); a sampler
// adds its own per-sample arrays, taken from the same slab
struct SampleSet {
    Slab samples;
    int cap = 0;
    uint64_t* d_keys = nullptr;                // [cap] key_k
    int8_t* d_label = nullptr;                 // [cap][N], the layout of hf_labels_dev per sample
    std::vector<uint64_t> h_keys;
    int n = 0;                                 // samples of the last call (the getters answer for it once it is finished)
};

// posterior path sampling (hf_sample.h)
struct Sampler : Decoder, SampleSet {
    uint8_t* d_maps = nullptr;                 // [cap][n_slots] (SCAN, slot order) / [cap][N] (SEQ, window order) map bytes
    int8_t* d_final = nullptr;                 // [cap][C] final states (SCAN)
    uint8_t* d_lmap = nullptr; uint8_t* d_smap = nullptr; uint8_t* d_sexit = nullptr;   // SCAN: [cap][nseg][64], [cap][nseg], [cap][nseg]
    void release() { samples.release(); Decoder::release(); }
};

// device scratch of a range getter (hf_get_interval_log_probs and those after it): one buffer per getter family, grown on demand and
// never shrunk, so that every getter's buffer stays as it is behind calls to the others
struct DevBuf {
    char* d_buf = nullptr; size_t cap = 0;
    void release() { if (d_buf) hipFree(d_buf); d_buf = nullptr; cap = 0; }
    int reserve(size_t bytes, const std::string& who) {
        if (bytes <= cap) return HF_OK;
        release();
        if (hipMalloc((void**) &d_buf, bytes) != hipSuccess) { (void) hipGetLastError(); d_buf = nullptr; return set_err(HF_E_HIP, who + ": out of device memory"); }
        cap = bytes;
        return HF_OK;
    }
};

// posteriors under minimum run lengths (hf_minlen_post.h): rows in window order; the forward lanes [N][sum of the lengths] are sized by
// the lengths of a call, grown on demand and never shrunk; the chunk values [2][C]: log Z_adm, log Z
struct MinLenPosterior : LabelDecoder {
    DevBuf fwd;
    double* d_post = nullptr;
    // hf_minlen_posterior_joined: the group-as-chunk offsets [C + 1] and the joined chunk-first windows [<= C] of a call (mlg_cut)
    DevBuf grp; std::vector<int64_t> h_grp;
    void release() { grp.release(); fwd.release(); Decoder::release(); }
};

// admissible path sampling (hf_minlen_sample.h): rows in window order, forward lanes of its own (as MinLenPosterior::fwd), log Z_adm per
// chunk, its per-sample arrays behind SampleSet's
struct MinLenSampler : Decoder, SampleSet {
    DevBuf fwd;
    double* d_chunk = nullptr;                 // [C] log Z_adm (k_mlp_fwd writes it; nothing returns it)
    uint16_t* d_words = nullptr;               // [N][Kp] words of k_mlv_fwd's format, Kp = a call's samples padded to HF_MLS_GROUP
    uint8_t* d_final = nullptr;                // [C][Kp] final lanes
    DevBuf grp; std::vector<int64_t> h_grp;    // hf_sample_paths_minlen_joined: as MinLenPosterior's
    void release() { grp.release(); fwd.release(); samples.release(); Decoder::release(); }
};

// the E-step under minimum run lengths (hf_minlen_em.h): a decoder front (parameter block, rows in window order, flag word), the forward
// lanes and xi_adm in one buffer sized by the lengths of a call, and a pass state of its own over the context's track, as each model of a
// batch has one: this call's tables (k_tables), tile and chunk statistics, the total.  The chunk values [2][C]: log Z_adm, log Z; ll0:
// the slot ranges k_chunk_stats sums into element 0, one slot per chunk
struct MinLenEM : Decoder {
    DevBuf fwd;                                // F [N][sum of the lengths] | xi_adm [N][16]
    double* d_xi = nullptr;                    // inside fwd (set by every call)
    double* d_chunk = nullptr; int32_t* d_ll0 = nullptr;
    Pass pass; bool pass_made = false;
    std::vector<double> h_total, h_chunk;      // of the last finished call: the reduced vector, the chunk values
    void release() { if (pass_made) drop_pass(); fwd.release(); Decoder::release(); }
    void drop_pass();
};

// maximum-expected-accuracy decoding under minimum run lengths (hf_mea.h): a getter of the last full pass with a state of its own, the
// slab allocated by its first call: gain rows, backpointer words, labels, block scores, final lanes, the unit-end parameter block and
// the flag word; the group-as-chunk offsets of a call (mlg_cut) in a buffer beside it
struct MeaDecoder {
    Slab slab;
    bool alloc = false;
    double2* d_rows = nullptr;                 // [N][8] window order, k_mlv_rows' layout
    uint16_t* d_bp = nullptr; int8_t* d_label = nullptr;
    double* d_score = nullptr; uint8_t* d_final = nullptr;     // [C] per block
    DevParams* d_params = nullptr;             // trans[s][4] = 1.0 in every region, 0 elsewhere: the walks' end column of zeros
    unsigned* d_flags = nullptr;
    DevBuf grp; std::vector<int64_t> h_grp;
    void release() { grp.release(); slab.release(); alloc = false; }
};

// the alpha statistics (hf_alpha.h): the switch, the plan of the pairs (built by the first call) and buffers of their own
struct AlphaStats {
    bool on = false;          // hf_set_alpha_stats
    bool pass = false;        // the last pass was a full pass with the switch on
    bool cached = false;      // `last` holds the statistics of the last pass
    bool planned = false;
    int64_t n_pairs = 0; int n_blocks = 0;
    char* d_buf = nullptr;    // pair_t | pair_c | blocks | rblk0 | part | out | terms
    long long* d_pair_t = nullptr; int32_t* d_pair_c = nullptr; void* d_blocks = nullptr; int32_t* d_rblk0 = nullptr;
    double* d_part = nullptr; double* d_out = nullptr; double* d_terms = nullptr;   // d_terms: [rows of A][32], HF_ALGO_SCAN
    std::vector<double> last;
    void release() { if (d_buf) hipFree(d_buf); d_buf = nullptr; planned = false; }
};

// the opaque handle of the C ABI: one track, the pass state of hf_estep over it, the decoders' buffers, the interval getter's buffer,
// the alpha statistics' plan and buffers, the count moments' buffer, the run moments' buffer, the entropy getters' buffers, the breakpoint
// getter's and the long-run getter's, the buffers of the posterior under minimum run lengths and of the admissible path sampler
struct hf_ctx {
    Track tr;
    Pass pass;
    Viterbi vit;
    MinLenViterbi mlv;
    MinLenPosterior mlp;
    MinLenSampler mls;
    Sampler smp;
    DevBuf iv;                // hf_interval.h: pieces, parts, piece products, results
    AlphaStats al;
    DevBuf mo;                // hf_moments.h: pieces, parts, piece triples, piece means, results
    DevBuf rn;                // hf_runs.h: pieces, parts, piece triples, piece sums of xi, results
    DevBuf en, en_lab;        // hf_entropy.h: pieces, parts, piece sums, results / the profile's two arrays; the labels of a call
    DevBuf bp;                // hf_breakpoint.h: pieces, parts, piece products, the chain's vectors, the windows' weights, results
    DevBuf lr;                // hf_longrun.h: parts, groups, results
    MeaDecoder mea;           // hf_mea.h: hf_get_mea_labels
    MinLenEM mle;             // hf_minlen_em.h: hf_estep_minlen
};

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

// Launch geometry of a one-wavefront-per-tile kernel: 4 wavefronts per block, fewer when the per-region transition
// tables (1088 B per region) plus the per-wavefront LDS do not fit (many regions / components); dynamic LDS above the
// default 64 KiB is requested explicitly.
struct TileGeom { unsigned blocks = 0, threads = 256; size_t lds = 0; bool ok = false; };
template <class Kern>
static TileGeom tile_geom(const Track& tr, Kern kernel, size_t per_wave_bytes, bool with_tab = true, int wmax = 4) {
    TileGeom g;
    const size_t tab = with_tab ? (size_t) tr.R * HF_TAB_STRIDE * 8 : 0;
    int w = wmax;
    while (w >= 1 && tab + (size_t) w * per_wave_bytes > tr.lds_max) w--;
    if (w < 1) return g;
    g.threads = 64u * (unsigned) w;
    g.blocks = (unsigned) ((tr.ntiles + w - 1) / w);
    g.lds = tab + (size_t) w * per_wave_bytes;
    g.ok = true;
    if (g.lds > 64 * 1024)
        g.ok = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) g.lds) == hipSuccess;
    return g;
}
#define TILE_GEOM_OR_FAIL(g) do { if (!(g).ok) { set_err(HF_E_ARG, "the per-region tables do not fit the LDS of one workgroup"); ps.launch_failed = true; return; } } while (0)

static RowSrc row_src(const Pass& ps) {
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
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chunk_stats<KT>), dim3((unsigned) tr.C), dim3(128), 0, st, tr.d_chunk_tile0, ll_off(ps),
                       tr.d_regmask, ps.d_tile_stats, ll_part(ps), ps.d_params, ps.d_chunk_stats, tr.V, tr.K,
                       full);
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
static int pass_create(const Track& tr, const Pass& settings, Pass* out, UploadStage* stg = nullptr) {
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
static void pass_destroy(Pass& ps) {
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
    ctx->mea.release();
    ctx->mle.release();
    ctx->tr.slab.release();
    delete ctx;
}

// pack one iteration's model: conditional transition tables (hmm_utils.c:2278-2292) and the
// distinct alpha values of each column
static int pack_params(const Track& tr, const hf_params* p, DevParams* dst) {
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
            // statistics by emission row: the job list of the Gaussian tables is the (key, class) list of the rows of A (hf_seg.h)
            const bool arows = !nbm && seg_pass(tr);
            const int nk = arows ? tr.n_combo : tr.n_keys;
            const int jobs = nk + tr.n_slow;
            if (nbm)
                hipLaunchKernelGGL(k_tables_nb, dim3((unsigned) (jobs / 256 + 1)), dim3(256), 0, st, tr.n_keys, tr.d_keys, tr.n_slow,
                                   tr.d_slow_w, tr.d_rec, tr.M, ps.d_nbE, ps.d_lutE, ps.d_Es, ps.d_flags);
            else
            {
#define HF_LAUNCH_TABLES(J, KA, KP) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tables<J, KA>), dim3((unsigned) ((jobs + J - 1) / J + (jobs == 0))), dim3(256), 0, st, \
                               ps.tabwork, ps.d_params, ps.d_flags, KP, ps.d_params)
                if (ps.kp_now) {     // the parameter block travels in the kernel arguments (pack_kparams): no copy was enqueued
                    if (jobs < 64 * 1024) HF_LAUNCH_TABLES(HF_TABLE_JOBS_SMALL, true, ps.kparams); else HF_LAUNCH_TABLES(HF_TABLE_JOBS_LARGE, true, ps.kparams);
                } else {
                    const NoKParams none{0};
                    if (jobs < 64 * 1024) HF_LAUNCH_TABLES(HF_TABLE_JOBS_SMALL, false, none); else HF_LAUNCH_TABLES(HF_TABLE_JOBS_LARGE, false, none);
                }
#undef HF_LAUNCH_TABLES
            }
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
        hipLaunchKernelGGL(k_reduce, dim3((unsigned) (tr.V + 1)), dim3(64), 0, (hipStream_t) stream, chunk_stats_dev, row_index_dev,
                           n_chunks, tr.V, out_dev,
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

static int flags_to_code(unsigned fl) {
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
    hfm_set_loglikelihood(model, stats_host[0]);
    if (do_mstep && mode == HF_MODE_FULL) {
        const int cv = hfm_estimate(model, stats_host, tol);
        if (converged) *converged = cv;
    }
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
static bool in_chunks(const Track& tr, int64_t first, int64_t last) {
    return tr.C > 0 && first >= tr.h_off.front() && last < tr.h_off.back();
}
static bool all_in_chunks(const Track& tr) { return tr.N == 0 || in_chunks(tr, 0, tr.N - 1); }

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


// ------------------------------------------------------------------------------------------
// the path decoders (hf_decode.h): Viterbi (hf_viterbi.h) and posterior path sampling (hf_sample.h).  Each has its own parameter block,
// rows, flags and outputs, so that the last pass's getters (which re-run the segment kernel over the pass's tables), the next pass and
// the other decoder see nothing of it.  Last in the file, their kernels included, so that no pass kernel's code moves relative to the
// ones around it.
// ------------------------------------------------------------------------------------------
#include "hf_viterbi.h"
#include "hf_sample.h"

static bool dec_scan(const Track& tr) { return tr.algo == HF_ALGO_SCAN; }
static size_t dec_nrow(const Track& tr) { return dec_scan(tr) ? (size_t) tr.n_slots : (size_t) tr.N; }   // rows and map bytes per path
static size_t dec_nseg(const Track& tr) { return dec_scan(tr) ? (size_t) tr.nseg : 0; }

// Every device array of a decoder, f(array, bytes) in turn: the ONE place that sizes them (dec_take allocates them, hf_sample_capacity
// counts them).  What dec_front fills and every decoder has (dec_front_arrays; nrow rows): parameter block, negative-binomial table,
// rows, flag word; SCAN: the arrays of A and B, with their exponent sums when the decoder reports a score.
template <class D, class F> static void dec_front_arrays(const Track& tr, D& d, size_t nrow, F&& f) {
    f(d.d_params, tr.params_bytes); f(d.d_nbE, (size_t) tr.R * 4 * HF_NB_NX * 8); f(d.d_rows, nrow * 128); f(d.d_flags, 4);
}
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

// a slab of exactly the arrays `arrays` lists (arrays(f) calls f(array, bytes) for each), every one of them taken from it
template <class A> static int dec_take(Slab& slab, A&& arrays) {
    slab.first = 0;
    arrays([&](auto&, size_t bytes) { slab.first += Slab::granule(bytes); });
    bool ok = true;
    arrays([&](auto& p, size_t bytes) {
        if (ok) { p = static_cast<std::remove_reference_t<decltype(p)>>(slab.alloc(bytes)); ok = p != nullptr; }
    });
    if (!ok) { (void) hipGetLastError(); return set_err(HF_E_HIP, "out of device memory for the decoder's buffers"); }
    return HF_OK;
}

// the fixed part of a decoder on its first call: the pinned parameter block and the slab of `arrays`
template <class A> static int dec_alloc(const Track& tr, Decoder& d, A&& arrays) {
    if (d.alloc) return HF_OK;
    HIPCHK(hipHostMalloc((void**) &d.h_params, tr.params_bytes));
    const int rc = dec_take(d.slab, arrays);
    if (rc) return rc;
    d.alloc = true;
    return HF_OK;
}

static bool dec_work(const Track& tr) { return tr.C > 0 && tr.N > 0; }

// What every decoder call does before its kernels, error messages naming the entry point `who`: the wait for a run nobody finished (it
// may still be reading the pinned parameter block), `prepare` (the decoder's buffers and inputs; it may refuse the call), the parameter
// block and the negative-binomial table, the flag word.  nbE: the table as the rows kernels take it (null for the other models).
template <class Prep>
static int dec_front(const Track& tr, Decoder& d, const hf_params* p, hipStream_t st, const std::string& w, Prep&& prepare, const double*& nbE) {
    HIPCHK(hipSetDevice(tr.device));
    if (d.launched) HIPCHK(hipDeviceSynchronize());
    d.launched = false; d.done = false;
    int rc = prepare();
    if (rc) return rc;
    rc = pack_params(tr, p, d.h_params);
    if (rc) return rc;
    const bool nbm = p->model_type == HF_MODEL_NEGATIVE_BINOMIAL;
    if (nbm) {
        if (!p->nb_E) return set_err(HF_E_ARG, w + ": negative_binomial needs hf_params.nb_E");
        if (p->nb_max_x > 0 && tr.M - 1 > p->nb_max_x)
            return set_err(HF_E_ARG, w + ": the windows hold coverage values above hf_params.nb_max_x (hfm_set_max_coverage)");
        // (synchronous: the caller's table may be rewritten as soon as this returns)
        HIPCHK(hipMemcpy(d.d_nbE, p->nb_E, (size_t) tr.R * 4 * HF_NB_NX * 8, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpyAsync(d.d_params, d.h_params, tr.params_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d.d_flags, 0, 4, st));
    nbE = nbm ? d.d_nbE : nullptr;
    return HF_OK;
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
    } else {
        hipLaunchKernelGGL(k_dec_rows_win, dim3((unsigned) ((tr.N + 255) / 256)), dim3(256), 0, st, tr.N, tr.d_rec, tr.d_beta, d.d_params, nbE,
                           d.d_rows, d.d_flags);
    }
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
static int dec_finish(const Track& tr, Decoder& d, void* stream) {
    HIPCHK(hipSetDevice(tr.device));
    HIPCHK(hipStreamSynchronize((hipStream_t) stream));
    d.launched = false;
    unsigned fl = 0;
    HIPCHK(hipMemcpy(&fl, d.d_flags, 4, hipMemcpyDeviceToHost));
    return fl ? flags_to_code(fl) : HF_OK;
}

// ---- the decoders that leave labels and `per` values per chunk (LabelDecoder) ----
// what the kernels do not write: the values of chunks without windows (0), the labels of windows outside every chunk (-1)
static int dec_clear_outputs(const Track& tr, LabelDecoder& d, int per, hipStream_t st) {
    if (tr.C > 0) HIPCHK(hipMemsetAsync(d.d_chunk, 0, (size_t) tr.C * per * 8, st));
    if (!all_in_chunks(tr)) HIPCHK(hipMemsetAsync(d.d_label, 0xff, (size_t) tr.N, st));
    return HF_OK;
}

// dec_finish, then the chunk values to the host copy; the run counts as finished
static int dec_finish_chunks(const Track& tr, LabelDecoder& d, int per, void* stream) {
    const int rc = dec_finish(tr, d, stream);
    if (rc) return rc;
    d.h_chunk.assign((size_t) tr.C * per, 0.0);
    if (tr.C > 0) HIPCHK(hipMemcpy(d.h_chunk.data(), d.d_chunk, (size_t) tr.C * per * 8, hipMemcpyDeviceToHost));
    d.done = true;
    return HF_OK;
}

// ... for a decoder with one score per chunk: their sum in chunk-list order
static int dec_finish_scores(const Track& tr, LabelDecoder& d, double* log_prob_host, void* stream) {
    const int rc = dec_finish_chunks(tr, d, 1, stream);
    if (rc) return rc;
    double tot = 0.0;
    for (double x : d.h_chunk) tot += x;
    if (log_prob_host) *log_prob_host = tot;
    return HF_OK;
}

static int dec_labels(const Track& tr, const LabelDecoder& d, int8_t* labels_host) {
    HIPCHK(hipSetDevice(tr.device));
    if (tr.N > 0) HIPCHK(hipMemcpy(labels_host, d.d_label, (size_t) tr.N, hipMemcpyDeviceToHost));
    return HF_OK;
}

// the first value of every chunk
static int dec_chunk_values(const Track& tr, const LabelDecoder& d, double* out_host) {
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

// the largest grid.y of the per-sample launches
#define HF_SMP_MAX_PER_CALL 65535

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

// ---- the per-sample part of a sampler (SampleSet) ----
// room for n samples: the slab replaced by one of exactly `arrays` (the sampler's per-sample arrays at n samples) when it holds fewer
template <class A> static int smp_grow(SampleSet& s, int n, A&& arrays) {
    if (n <= s.cap) return HF_OK;
    s.samples.release();
    s.cap = 0;
    const int rc = dec_take(s.samples, arrays);
    if (rc) return rc;
    s.cap = n;
    return HF_OK;
}

// the keys of samples first .. first + n - 1 (synchronous)
static int smp_keys(SampleSet& s, int64_t first, int n, uint64_t seed) {
    s.h_keys.resize((size_t) n);
    for (int k = 0; k < n; k++) s.h_keys[(size_t) k] = hf_sample_key(seed, (uint64_t) (first + k));
    HIPCHK(hipMemcpy(s.d_keys, s.h_keys.data(), (size_t) n * 8, hipMemcpyHostToDevice));
    return HF_OK;
}

// dec_finish; the run counts as finished
static int smp_finish(const Track& tr, Decoder& d, void* stream) {
    const int rc = dec_finish(tr, d, stream);
    if (rc) return rc;
    d.done = true;
    return HF_OK;
}

// the labels of sample k of the last call, for the getter `who`
static int smp_labels(const Track& tr, const SampleSet& s, const char* who, int k, int8_t* labels_host) {
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


// ------------------------------------------------------------------------------------------
// The range getters: values over window ranges under the model of the last full pass (hf_interval.h, hf_moments.h, hf_runs.h,
// hf_entropy.h) and the alpha statistics (hf_alpha.h).  Nothing of them runs inside a pass: they read what the pass left (on the scan
// path after the lazy re-run of the segment kernel, pass_all_records) and write buffers of their own.  Last in the file, behind
// hf_batch.h and the decoders, so that no pass kernel's code moves.
//
// THE SCAFFOLD of the four piece / chain getters (interval, count moments, run moments, entropy and labelling log-probability): rg_check
// refuses what every one of them refuses, pass_view says where the pass left its rows, f and b (hf_view.h), and rg_run takes the jobs through the
// device batch by batch: it cuts a batch into chunk-local parts and their pieces (hf_jobs.h), lays out the getter's scratch (pieces |
// parts | per-piece results, one or two arrays | per-part results), uploads, launches the getter's piece kernel and then its chain
// kernel, fetches the parts' results and hands the parts of every job, in chunk order, to the getter's fold.  A getter keeps its record
// builders, its scratch sizes, its two launches and its fold.
// ------------------------------------------------------------------------------------------
#include "hf_jobs.h"
#include "hf_view.h"
#include "hf_interval.h"
#include "hf_moments.h"
#include "hf_runs.h"
#include "hf_entropy.h"
#include <type_traits>

// pieces and parts per device batch (hf_jobs.h): the interval getter's, and those of the moments, run moments and entropy getters (a
// piece's triple is 384 bytes: 96 MB of them at most)
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

static_assert(HF_IV_PIECE == 512 && HF_MO_PIECE == 512 && HF_RN_PIECE == 512 && HF_EN_PIECE == 512, "one piece grid for every getter");

// f(std::true_type) for HF_ALGO_SEQ, f(std::false_type) for HF_ALGO_SCAN: one launch per kernel, its template argument the only difference
template <class F>
static void by_algo(const Track& tr, F&& f) {
    if (tr.algo == HF_ALGO_SEQ) f(std::true_type{}); else f(std::false_type{});
}

// What every range getter refuses, in this order: n < 0, `early` (a refusal of the getter's own that ranks here, or nullptr), NULL arrays,
// no full pass, `late` (the same), and job by job a bad range, a window outside every chunk, a state mask outside 1..15 (state_mask ==
// nullptr: the getter has none) and a region outside -1..n_regions-1 (region == nullptr: no filter).
static int rg_check(const hf_ctx* ctx, const std::string& who, int64_t n, bool null_array, const int64_t* first, const int64_t* last,
                    const uint8_t* state_mask, const int32_t* region = nullptr, const char* early = nullptr, const char* late = nullptr) {
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
static int pass_view(hf_ctx* ctx, const std::string& who, int64_t n, PassView& pv) {
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

// a batch on the device: np pieces, nq parts, the per-piece results pm and px of the piece kernel, the per-part results of the chain kernel
template <class Piece, class Part>
struct RgBatch {
    size_t np, nq;
    const Piece* pieces; const Part* parts;
    double* pm; double* px; double* out;
    dim3 piece_grid() const { return dim3((unsigned) np); }                  // one 64-lane workgroup per piece
    dim3 chain_grid() const { return dim3((unsigned) ((nq + 63) / 64)); }    // one thread per part
};

// The jobs of a call, batch by batch, on the stream of the pass.  pm_bytes, px_bytes: the piece kernel's results per piece (px_bytes == 0:
// one array only); out_doubles: the chain kernel's results per part.  launch(batch) enqueues the two kernels (the piece kernel only when
// the batch has pieces); fold(job, parts, val, k0, k1) gets the host's part records and the results of the batch and writes the value
// of the job from its parts k0 .. k1 - 1.
template <class Piece, class Part, int64_t GRID, class MkPart, class MkPiece, class Launch, class Fold>
static int rg_run(hf_ctx* ctx, const std::string& who, DevBuf& buf, int64_t n, const int64_t* first, const int64_t* last, size_t cap_pieces,
                  size_t cap_parts, size_t pm_bytes, size_t px_bytes, size_t out_doubles, MkPart&& mk_part, MkPiece&& mk_piece, Launch&& launch,
                  Fold&& fold) {
    hipStream_t st = ctx->pass.last_stream;
    JobCut<Piece, Part, GRID> jc;
    std::vector<double> val;
    for (int64_t j0 = 0; j0 < n;) {
        const int64_t j1 = jc.cut(ctx->tr.h_off, n, first, last, j0, cap_pieces, cap_parts, mk_part, mk_piece);
        const size_t np = jc.pieces.size(), nq = jc.parts.size();
        const size_t o_parts = Slab::granule(np * sizeof(Piece)), o_pm = o_parts + Slab::granule(nq * sizeof(Part));
        const size_t o_px = o_pm + Slab::granule(np * pm_bytes), o_out = px_bytes ? o_px + Slab::granule(np * px_bytes) : o_px;
        const int rc = buf.reserve(o_out + Slab::granule(nq * out_doubles * 8), who);
        if (rc) return rc;
        Piece* d_pieces = reinterpret_cast<Piece*>(buf.d_buf);
        Part* d_parts = reinterpret_cast<Part*>(buf.d_buf + o_parts);
        const RgBatch<Piece, Part> bt{np, nq, d_pieces, d_parts, reinterpret_cast<double*>(buf.d_buf + o_pm),
                                      px_bytes ? reinterpret_cast<double*>(buf.d_buf + o_px) : nullptr, reinterpret_cast<double*>(buf.d_buf + o_out)};
        if (np) HIPCHK(hipMemcpyAsync(d_pieces, jc.pieces.data(), np * sizeof(Piece), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_parts, jc.parts.data(), nq * sizeof(Part), hipMemcpyHostToDevice, st));
        launch(bt);
        HIPCHK(hipGetLastError());
        val.resize(nq * out_doubles);
        HIPCHK(hipMemcpyAsync(val.data(), bt.out, nq * out_doubles * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int64_t j = j0; j < j1; j++)      // the parts of a job in chunk order
            fold(j, jc.parts.data(), val.data(), jc.job_p0[(size_t) (j - j0)], jc.job_p0[(size_t) (j - j0) + 1]);
        j0 = j1;
    }
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
// after the getters' lazy re-run of the segment kernel).  Last in the file, so that no pass kernel's code moves.
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
            // to part k - 1 when it lies in the next chunk and that chunk continues the one before.  Three sums, each left to right:
            //   mean = sum E[R] - sum_joined q,  var = sum Var(R) + sum_joined [...] + 2 sum_{both joined} [...]   (q = e_{k-1} s_k)
            // so a job without a join is the plain sum of its parts.
            double m = 0.0, mq = 0.0, v = 0.0, vj = 0.0, vjj = 0.0;
            bool prev_join = false;
            for (int64_t k = k0; k < k1; k++) {
                const double* x = &val[(size_t) k * HF_RN_OUT];
                m += x[0]; v += x[1];
                bool join = false;
                if (k > k0 && joined) {
                    const int c = parts[(size_t) k].c;
                    join = parts[(size_t) k - 1].c == c - 1 && joined[c] != 0;
                }
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
// and the job cutter with the others; bp_run is rg_run's sibling for four launches and the per-window weight arrays of a batch.  Last in
// the file, so that no other kernel's code moves.
// ------------------------------------------------------------------------------------------
#include "hf_breakpoint.h"

// pieces and parts per device batch: a window's weight is 12 bytes, 2^15 pieces of 512 windows about 200 MB.  A part has at least one
// piece, so the parts' cap never binds before the pieces'
#ifndef HF_BP_BATCH_PIECES
#define HF_BP_BATCH_PIECES (1 << 15)
#endif
#ifndef HF_BP_BATCH_PARTS
#define HF_BP_BATCH_PARTS (1 << 15)
#endif

static_assert(HF_BP_PIECE == 512, "one piece grid for every getter");

// The jobs of a call, batch by batch, on the stream of the pass: k_bp_piece, k_bp_chain, k_bp_weights, k_bp_quant.  prof_host (a call of
// one job): its p_k.
static int bp_run(hf_ctx* ctx, const std::string& who, const PassView& pv, int64_t n, const int64_t* first, const int64_t* last,
                  const uint8_t* um, const uint8_t* vm, const BpProbs& pr, double* lpe_host, int64_t* quant_host, int64_t* mode_host,
                  double* mode_p_host, double* prof_host) {
    hipStream_t st = ctx->pass.last_stream;
    DevBuf& buf = ctx->bp;
    JobCut<BpPiece, BpPart, HF_BP_PIECE> jc;
    std::vector<double> vd;
    std::vector<long long> vi;
    constexpr size_t NI = HF_BP_MAX_PROBS + 1;
    for (int64_t j0 = 0; j0 < n;) {
        long long nw = 0;      // windows with a weight so far in the batch
        const int64_t j1 = jc.cut(ctx->tr.h_off, n, first, last, j0, HF_BP_BATCH_PIECES, HF_BP_BATCH_PARTS,
            [&](int64_t j, int c, int64_t a, int64_t b) { BpPart pt{a, b, nw, 0, 0, um[j], vm[j], c, 0}; nw += b - a; return pt; },
            [](const BpPart& pt, int64_t t, int len) { return BpPiece{t, pt.w0 + (t - pt.a - 1), len, pt.um, pt.vm, 0}; });
        const size_t np = jc.pieces.size(), nq = jc.parts.size();
        size_t o = 0;
        auto take = [&](size_t bytes) { const size_t at = o; o += Slab::granule(bytes); return at; };
        const size_t o_pieces = take(np * sizeof(BpPiece)), o_parts = take(nq * sizeof(BpPart)), o_pm = take(np * 48 * 8), o_pe = take(np * 4 * 4);
        const size_t o_lv = take(np * 4 * 8), o_le = take(np * 8), o_rv = take(np * 4 * 8), o_re = take(np * 8), o_nn = take(nq * 8);
        const size_t o_wm = take((size_t) nw * 8), o_we = take((size_t) nw * 4), o_prof = prof_host ? take((size_t) nw * 8) : 0;
        const size_t o_outd = take(nq * 2 * 8), o_outi = take(nq * NI * 8);
        const int rc = buf.reserve(o, who);
        if (rc) return rc;
        char* d = buf.d_buf;
        BpPiece* d_pieces = reinterpret_cast<BpPiece*>(d + o_pieces);
        BpPart* d_parts = reinterpret_cast<BpPart*>(d + o_parts);
        double* d_pm = reinterpret_cast<double*>(d + o_pm); int* d_pe = reinterpret_cast<int*>(d + o_pe);
        double* d_lv = reinterpret_cast<double*>(d + o_lv); long long* d_le = reinterpret_cast<long long*>(d + o_le);
        double* d_rv = reinterpret_cast<double*>(d + o_rv); long long* d_re = reinterpret_cast<long long*>(d + o_re);
        double* d_nn = reinterpret_cast<double*>(d + o_nn);
        double* d_wm = reinterpret_cast<double*>(d + o_wm); int* d_we = reinterpret_cast<int*>(d + o_we);
        double* d_prof = prof_host ? reinterpret_cast<double*>(d + o_prof) : nullptr;
        double* d_outd = reinterpret_cast<double*>(d + o_outd); long long* d_outi = reinterpret_cast<long long*>(d + o_outi);
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
        if (prof_host) HIPCHK(hipMemcpyAsync(prof_host, d_prof, (size_t) nw * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int64_t j = j0; j < j1; j++) {      // a job is one part
            const size_t k = (size_t) jc.job_p0[(size_t) (j - j0)];
            if (lpe_host) lpe_host[j] = vd[k * 2];
            if (mode_p_host) mode_p_host[j] = vd[k * 2 + 1];
            if (mode_host) mode_host[j] = vi[k * NI];
            for (int q = 0; q < pr.n; q++) quant_host[j * pr.n + q] = vi[k * NI + 1 + (size_t) q];
        }
        j0 = j1;
    }
    return HF_OK;
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
    int rc = minlen_front(ctx, &hf_ctx::mlv, p, min_len, st, w,
                          [&] { return whole && joined && ctx->tr.C > 0 && joined[0]
                                           ? set_err(HF_E_ARG, w + ": joined[0] must be 0 (the first chunk continues nothing)") : (int) HF_OK; },
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
                const bool cont = c > 0 && joined && joined[c] && off[(size_t) c + 1] > off[(size_t) c] && off[(size_t) c] > off[(size_t) c - 1];
                if (!cont) { v.h_gchunk.push_back(c); v.h_goff.push_back(off[(size_t) c]); }
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
// exact long-run probabilities (hf_longrun.h): the job cutter's parts fall into groups of joined parts (hf_jobs.h group_parts), one
// wavefront of k_lr_chain walks a group's expanded chain, a job is folded from its groups on the host.  Last in the file, its kernel
// included, so that no other kernel's code moves.
// ------------------------------------------------------------------------------------------
#include "hf_longrun.h"

static_assert(HF_LONGRUN_MAX_LANES == 64, "one wavefront holds the expanded chain");

// parts, and windows in pieces of 512 (the grid of the other getters), per device batch: a group is one workgroup and a window one step
// of it, so the caps bound a launch's run time, not its memory.  The environment variables of the same names lower them (tests).
#ifndef HF_LR_BATCH_PARTS
#define HF_LR_BATCH_PARTS (1 << 16)
#endif
#ifndef HF_LR_BATCH_PIECES
#define HF_LR_BATCH_PIECES (1 << 18)
#endif

static size_t lr_cap(const char* name, size_t dflt) {
    if (const char* e = std::getenv(name)) { const long v = std::atol(e); if (v >= 1) return std::min<size_t>((size_t) v, dflt); }
    return dflt;
}

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
    const size_t cap_pieces = lr_cap("HF_LR_BATCH_PIECES", HF_LR_BATCH_PIECES), cap_parts = lr_cap("HF_LR_BATCH_PARTS", HF_LR_BATCH_PARTS);
    JobCut<LrPiece, LrPart, 512> jc;
    std::vector<LrGroup> groups;
    std::vector<int64_t> job_g0;
    std::vector<double> val;
    for (int64_t j0 = 0; j0 < n;) {
        const int64_t j1 = jc.cut(tr.h_off, n, first, last, j0, cap_pieces, cap_parts,
            [](int64_t, int c, int64_t a, int64_t b) { return LrPart{a, b, 0, 0, c, 0}; },
            [](const LrPart&, int64_t, int) { return LrPiece{0}; });
        group_parts(jc.parts, jc.job_p0, joined, groups, job_g0,
            [&](int64_t j, int64_t q0, int64_t q1) { return LrGroup{(int) q0, (int) q1, state_mask[j0 + j], min_len[j0 + j]}; });
        const size_t nq = jc.parts.size(), ng = groups.size();
        const size_t o_groups = Slab::granule(nq * sizeof(LrPart)), o_out = o_groups + Slab::granule(ng * sizeof(LrGroup));
        rc = ctx->lr.reserve(o_out + Slab::granule(ng * 2 * 8), who);
        if (rc) return rc;
        LrPart* d_parts = reinterpret_cast<LrPart*>(ctx->lr.d_buf);
        LrGroup* d_groups = reinterpret_cast<LrGroup*>(ctx->lr.d_buf + o_groups);
        double* d_out = reinterpret_cast<double*>(ctx->lr.d_buf + o_out);
        HIPCHK(hipMemcpyAsync(d_parts, jc.parts.data(), nq * sizeof(LrPart), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_groups, groups.data(), ng * sizeof(LrGroup), hipMemcpyHostToDevice, st));
        by_algo(tr, [&](auto S) {
            constexpr bool SEQ = decltype(S)::value;
            hipLaunchKernelGGL(k_lr_chain<SEQ>, dim3((unsigned) ng), dim3(64), 0, st, d_groups, d_parts, pv, d_out);
        });
        HIPCHK(hipGetLastError());
        val.resize(ng * 2);
        HIPCHK(hipMemcpyAsync(val.data(), d_out, ng * 2 * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int64_t j = j0; j < j1; j++) {
            // the groups of a job in chunk order: log_p_none is their left-to-right sum.  log_p_some: -inf when no group can hold a run,
            // the kernel's own value (accurate however small) when exactly one can, else log(1 - exp(log_p_none))
            double none = 0.0, some = -__builtin_inf();
            int hits = 0;
            for (int64_t g = job_g0[(size_t) (j - j0)]; g < job_g0[(size_t) (j - j0) + 1]; g++) {
                none += val[(size_t) g * 2];
                const double s = val[(size_t) g * 2 + 1];
                if (!(s == -__builtin_inf())) { hits++; some = s; }
            }
            if (hits > 1) some = lr_log1mexp(none);
            if (log_p_none_host) log_p_none_host[j] = none;
            if (log_p_some_host) log_p_some_host[j] = some;
        }
        j0 = j1;
    }
    return HF_OK;
}


// ------------------------------------------------------------------------------------------
// posteriors under minimum run lengths (hf_minlen_post.h): the sum-product twin of hf_viterbi_minlen, a decoder of its own with one code
// path for both kinds of context.  Last in the file, its kernels included, so that no other kernel's code moves.
// ------------------------------------------------------------------------------------------
#include "hf_minlen_post.h"

// every device array of the decoder but the forward lanes (their size depends on the lengths of a call: MinLenPosterior::fwd)
template <class F> static void mlp_arrays(const Track& tr, MinLenPosterior& v, F&& f) {
    dec_front_arrays(tr, v, (size_t) tr.N, f);
    f(v.d_post, (size_t) tr.N * 32); f(v.d_label, (size_t) tr.N); f(v.d_chunk, (size_t) tr.C * 16);
}

// hf_minlen_posterior and hf_minlen_posterior_joined (hf_minlen_post_joined.h, at the end of this file): one front, the rows, then
// `walks(track, decoder, forward lanes)` launches the entry point's two walks; `refuse`: what it refuses beyond the family's front
template <class Refuse, class Walks>
static int mlp_run(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], hipStream_t st, const std::string& w, Refuse&& refuse,
                   Walks&& walks) {
    int64_t lanes = 0;
    const double* nbE = nullptr;
    int rc = minlen_front(ctx, &hf_ctx::mlp, p, min_len, st, w, refuse, [&](const Track& tr, MinLenPosterior& v) {
        // the forward lanes: what the decoder holds of them already counts as free
        const size_t f_bytes = (size_t) tr.N * (size_t) lanes * 8;
        if (f_bytes > v.fwd.cap) {
            size_t free_b = 0, total_b = 0;
            HIPCHK(hipMemGetInfo(&free_b, &total_b));
            if ((double) f_bytes > 0.9 * ((double) free_b + (double) v.fwd.cap))
                return set_err(HF_E_ARG, w + ": the forward lanes need " + std::to_string(f_bytes) + " bytes (n_windows x sum of the lengths x 8), above nine tenths of the free device memory");
        }
        const int rc = dec_alloc(tr, v, [&](auto&& f) { mlp_arrays(tr, v, f); });
        return rc ? rc : v.fwd.reserve(f_bytes, w);
    }, lanes, nbE);
    if (rc) return rc;
    const Track& tr = ctx->tr;
    MinLenPosterior& v = ctx->mlp;
    if ((rc = dec_clear_outputs(tr, v, 2, st))) return rc;
    if (dec_work(tr)) {
        hipLaunchKernelGGL(k_dec_rows_win, dim3((unsigned) ((tr.N + 255) / 256)), dim3(256), 0, st, tr.N, tr.d_rec, tr.d_beta, v.d_params, nbE,
                           v.d_rows, v.d_flags);
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
    const std::string w = "hf_get_minlen_posterior";
    if (!ctx || !post_host || !ctx->mlp.done) return set_err(HF_E_ARG, w + ": no finished hf_minlen_posterior");
    const Track& tr = ctx->tr;
    if (first < 0 || n < 0 || first + n > tr.N) return set_err(HF_E_ARG, w + ": bad range");
    if (n > 0 && !in_chunks(tr, first, first + n - 1)) return set_err(HF_E_ARG, w + ": the range holds a window outside every chunk");
    HIPCHK(hipSetDevice(tr.device));
    if (n > 0) HIPCHK(hipMemcpy(post_host, ctx->mlp.d_post + first * 4, (size_t) n * 32, hipMemcpyDeviceToHost));
    return HF_OK;
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
// beside the three before it, one code path for both kinds of context.  Last in the file, its kernels included, so that no other
// kernel's code moves.
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
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    double fixed = 0.0;
    mls_arrays(tr, v, [&](auto&, size_t bytes) { fixed += (double) Slab::granule(bytes); });
    const double f_bytes = (double) tr.N * (double) lanes * 8.0;
    const double held = (v.alloc ? fixed : 0.0) + (double) v.fwd.cap + (v.cap ? (double) v.samples.first : 0.0);   // (Slab::release keeps `first`)
    const double budget = 0.9 * ((double) free_b + held) - fixed - f_bytes;
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

// hf_sample_paths_minlen and hf_sample_paths_minlen_joined (hf_minlen_post_joined.h, at the end of this file): one front, the rows, then
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
        hipLaunchKernelGGL(k_dec_rows_win, dim3((unsigned) ((tr.N + 255) / 256)), dim3(256), 0, st, tr.N, tr.d_rec, tr.d_beta, v.d_params, nbE,
                           v.d_rows, v.d_flags);
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


// k_mea_rows, the one kernel of hf_get_mea_labels (its host side stands behind mlg_cut below).  Here, in front of
// hf_minlen_post_joined.h, no other kernel's code moves.
#include "hf_mea.h"


// ------------------------------------------------------------------------------------------
// the posterior and the sampler over groups of joined chunks (hf_minlen_post_joined.h): hf_minlen_posterior_joined shares ctx->mlp, its
// finish and its getters with hf_minlen_posterior (mlp_run above), hf_sample_paths_minlen_joined shares ctx->mls with
// hf_sample_paths_minlen (mls_run above).  The kernels are second bodies launched over the group-as-chunk offsets.  Here, in front of
// hf_minlen_joined.h, no other kernel's code moves.
// ------------------------------------------------------------------------------------------
#include "hf_minlen_post_joined.h"

// The groups of a call as a chunk list, hf_viterbi_minlen_joined's rule (a chunk continues its predecessor when it is joined to it and
// both have windows): h[0 .. C] the offsets in which a group's first chunk holds the group's window range and its other chunks none,
// h[C + 1 ..] the joined chunk-first windows.  Uploaded to `grp` on `st`; returns the number of those windows in *nb.
static int mlg_cut(const Track& tr, const uint8_t* joined, DevBuf& grp, std::vector<int64_t>& h, hipStream_t st, const std::string& w, int* nb) {
    const std::vector<int64_t>& off = tr.h_off;
    const size_t C = (size_t) tr.C;
    auto cont = [&](size_t c) { return c > 0 && c < C && joined && joined[c] && off[c + 1] > off[c] && off[c] > off[c - 1]; };
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

static int mlg_refuse(const hf_ctx* ctx, const uint8_t* joined, const std::string& w) {
    return joined && ctx->tr.C > 0 && joined[0] ? set_err(HF_E_ARG, w + ": joined[0] must be 0 (the first chunk continues nothing)") : (int) HF_OK;
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
        const size_t sizes[7] = {(size_t) tr.N * 128, (size_t) tr.N * 2, (size_t) tr.N, (size_t) tr.C * 8, (size_t) tr.C, tr.params_bytes, 4};
        size_t total = 0;
        for (size_t b : sizes) total += Slab::granule(b);
        m.slab.first = total;
        void* ptr[7];
        for (int i = 0; i < 7; i++)
            if (!(ptr[i] = m.slab.alloc(sizes[i]))) { m.slab.release(); return set_err(HF_E_HIP, who + ": out of device memory"); }
        m.d_rows = static_cast<double2*>(ptr[0]); m.d_bp = static_cast<uint16_t*>(ptr[1]); m.d_label = static_cast<int8_t*>(ptr[2]);
        m.d_score = static_cast<double*>(ptr[3]); m.d_final = static_cast<uint8_t*>(ptr[4]); m.d_params = static_cast<DevParams*>(ptr[5]);
        m.d_flags = static_cast<unsigned*>(ptr[6]);
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
// it is, k_mle_bwd, k_mle_tile, then k_chunk_stats and k_reduce as they are.  One code path for both kinds of context.  Behind every other
// section, its kernels included, and in front of k_mlvj_fwd alone, which keeps its code only as the file's last kernel.
// ------------------------------------------------------------------------------------------
#include "hf_minlen_em.h"

template <class F> static void mle_arrays(const Track& tr, MinLenEM& v, F&& f) {
    dec_front_arrays(tr, v, (size_t) tr.N, f);
    f(v.d_chunk, (size_t) tr.C * 16); f(v.d_ll0, ((size_t) tr.C + 1) * 4);
}

template <int KT>
static int mle_launch_stats(const Track& tr, MinLenEM& v, hipStream_t st, int ncol) {
    Pass& ps = v.pass;
    if (tr.ntiles > 0) {
        const TileGeom g = tile_geom(tr, k_mle_tile<KT>, (size_t) (3 * ncol > 28 ? 3 * ncol : 28) * 65 * 8, false);
        if (!g.ok) return set_err(HF_E_ARG, "hf_estep_minlen: the accumulators of one wavefront do not fit the LDS of one workgroup");
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mle_tile<KT>), dim3(g.blocks), dim3(g.threads), g.lds, st, tr.ntiles, tr.d_tile_desc, tr.d_rec,
                           row_src(ps), ps.d_params, v.d_xi, tr.d_regmask, ps.d_tile_stats);
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chunk_stats<KT>), dim3((unsigned) tr.C), dim3(128), 0, st, tr.d_chunk_tile0, v.d_ll0, tr.d_regmask,
                       ps.d_tile_stats, v.d_chunk, ps.d_params, ps.d_chunk_stats_own, tr.V, tr.K, tr.ntiles > 0 ? 1 : 0);
    return HF_OK;
}

int hf_estep_minlen(hf_ctx* ctx, const hf_params* p, const int32_t min_len[4], void* stream) {
    hipStream_t st = (hipStream_t) stream;
    const std::string w = "hf_estep_minlen";
    int64_t lanes = 0;
    const double* nbE = nullptr;
    int rc = minlen_front(ctx, &hf_ctx::mle, p, min_len, st, w, [&] {
        return p->model_type == HF_MODEL_NEGATIVE_BINOMIAL
                   ? set_err(HF_E_ARG, w + ": the negative_binomial model is not supported (its statistics are another path)") : (int) HF_OK;
    }, [&](const Track& tr, MinLenEM& v) {
        // the forward lanes and xi_adm: what the decoder holds of them already counts as free
        const size_t f_bytes = Slab::granule((size_t) tr.N * (size_t) lanes * 8), bytes = f_bytes + (size_t) tr.N * 128;
        if (bytes > v.fwd.cap) {
            size_t free_b = 0, total_b = 0;
            HIPCHK(hipMemGetInfo(&free_b, &total_b));
            if ((double) bytes > 0.9 * ((double) free_b + (double) v.fwd.cap))
                return set_err(HF_E_ARG, w + ": the forward lanes and xi_adm need " + std::to_string(bytes) + " bytes (n_windows x (sum of the lengths x 8 + 128)), above nine tenths of the free device memory");
        }
        const bool first = !v.alloc;
        int rc = dec_alloc(tr, v, [&](auto&& f) { mle_arrays(tr, v, f); });
        if (rc) return rc;
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
        const int l0 = (int) min_len[0], l1 = (int) min_len[1], l2 = (int) min_len[2], l3 = (int) min_len[3];
        double* d_F = reinterpret_cast<double*>(v.fwd.d_buf);
        HIPCHK(hipMemcpyAsync(ps.d_params, v.h_params, tr.params_bytes, hipMemcpyHostToDevice, st));
        {   // this call's tables; the kernel clears the flag word it is given, as dec_front has done
            const int jobs = (seg_pass(tr) ? tr.n_combo : tr.n_keys) + tr.n_slow;
            const NoKParams none{0};
#define HF_MLE_TABLES(J) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tables<J, false>), dim3((unsigned) ((jobs + J - 1) / J + (jobs == 0))), dim3(256), 0, st, \
                                            ps.tabwork, ps.d_params, v.d_flags, none, ps.d_params)
            if (jobs < 64 * 1024) HF_MLE_TABLES(HF_TABLE_JOBS_SMALL); else HF_MLE_TABLES(HF_TABLE_JOBS_LARGE);
#undef HF_MLE_TABLES
        }
        if (dec_work(tr)) {
            hipLaunchKernelGGL(k_dec_rows_win, dim3((unsigned) ((tr.N + 255) / 256)), dim3(256), 0, st, tr.N, tr.d_rec, tr.d_beta, v.d_params, nbE,
                               v.d_rows, v.d_flags);
            hipLaunchKernelGGL(k_mlp_fwd, dim3((unsigned) tr.C, 2), dim3(64), 0, st, (int) tr.C, tr.d_off, tr.d_rec, v.d_params, v.d_rows, l0, l1, l2, l3,
                               d_F, v.d_chunk, v.d_flags);
            hipLaunchKernelGGL(k_mle_bwd, dim3((unsigned) tr.C), dim3(64), 0, st, tr.d_off, tr.d_rec, v.d_params, v.d_rows, l0, l1, l2, l3, d_F, v.d_xi,
                               v.d_flags);
        }
        const int kc = p->ncomp[3];
        rc = kc <= 4 ? mle_launch_stats<4>(tr, v, st, kc) : kc <= 8 ? mle_launch_stats<8>(tr, v, st, kc) : mle_launch_stats<16>(tr, v, st, kc);
        if (rc) return rc;
        hipLaunchKernelGGL(k_reduce, dim3((unsigned) (tr.V + 1)), dim3(64), 0, st, ps.d_chunk_stats_own, (const int32_t*) nullptr, (int64_t) tr.C, tr.V,
                           ps.d_total, v.d_flags, 0, 0, 0);
    }
    HIPCHK(hipGetLastError());
    v.launched = true;
    return HF_OK;
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
    const std::string w = "hf_get_minlen_pair_posterior";
    if (!ctx || !xi_host || !ctx->mle.done) return set_err(HF_E_ARG, w + ": no finished hf_estep_minlen");
    const Track& tr = ctx->tr;
    if (first < 0 || n < 0 || first + n > tr.N) return set_err(HF_E_ARG, w + ": bad range");
    if (n > 0 && !in_chunks(tr, first, first + n - 1)) return set_err(HF_E_ARG, w + ": the range holds a window outside every chunk");
    HIPCHK(hipSetDevice(tr.device));
    if (n > 0) HIPCHK(hipMemcpy(xi_host, ctx->mle.d_xi + first * 16, (size_t) n * 128, hipMemcpyDeviceToHost));
    return HF_OK;
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
    hfm_set_loglikelihood(model, stats_host[0]);
    if (do_mstep) {
        const int cv = hfm_estimate(model, stats_host, tol);
        if (converged) *converged = cv;
    }
    return HF_OK;
}


// k_mlvj_fwd, the forward walk of hf_viterbi_minlen_joined (mlv_run above launches it).  Last in the file: hf_minlen_joined.h says why.
#include "hf_minlen_joined.h"
