// hf_host.h — the host side that the translation units of libhmmflagger_hip.so share: the error string, the slab, the track, the pass
// state, the decoders' states and the context; the host functions that cross a unit boundary; the host templates that take lambdas.
// No kernel is defined here.  Units: hf_estep.hip (context, hf_create, the pass, hf_batch.h, and hf_getters.h: range getters, alpha
// statistics), hf_decoders.hip (Viterbi, path sampling), hf_minlen.hip (the minimum-run-length family), hf_runlen.hip (the block-length
// spectrum) and hf_countdist.hip (the distribution of label totals).  EVERY __global__ FUNCTION IS
// COMPILED IN EXACTLY ONE UNIT: a unit that needs another's kernel calls the owner's launcher
// declared below (a second copy of a plain kernel is a duplicate symbol at link time), and a unit that needs only the __device__ helpers
// of a header whose kernels another unit owns defines HF_HELPERS_ONLY in front of its includes.
#pragma once
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
#include <type_traits>

#include <thread>
#include <unistd.h>
#include <immintrin.h>

// nothing below is part of the C ABI: the names stay inside the library
#pragma GCC visibility push(hidden)

extern thread_local std::string g_err;      // hf_last_error's string (defined in hf_estep.hip)
inline int set_err(int code, const std::string& msg) { g_err = msg; return code; }
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
    DevBuf grp; std::vector<int64_t> h_grp;    // hf_estep_minlen_joined: as MinLenPosterior's
    void release() { if (pass_made) drop_pass(); grp.release(); fwd.release(); Decoder::release(); }
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
    DevBuf rl;                // hf_runlen.hip: pieces, parts, piece bins, part records
    DevBuf cd;                // hf_countdist.hip: pieces, parts, piece transfers, part distributions
    MeaDecoder mea;           // hf_mea.h: hf_get_mea_labels
    MinLenEM mle;             // hf_minlen_em.h: hf_estep_minlen
};

// ------------------------------------------------------------------------------------------
// host functions that cross a unit boundary, each defined in the unit that owns it (its comment stands there)
// ------------------------------------------------------------------------------------------
struct PassView;      // hf_view.h
struct RowSrc;        // hf_scan.h
struct UploadStage;   // hf_estep.hip

// hf_estep.hip
int pack_params(const Track& tr, const hf_params* p, DevParams* dst);
int pass_create(const Track& tr, const Pass& settings, Pass* out, UploadStage* stg = nullptr);
void pass_destroy(Pass& ps);
RowSrc row_src(const Pass& ps);
int flags_to_code(unsigned fl);
bool in_chunks(const Track& tr, int64_t first, int64_t last);
bool all_in_chunks(const Track& tr);
// ... and the launchers of its kernels for the other units: this call's Gaussian tables into ps's arrays (k_tables clears `flags`; kp: the
// parameter block travels in the kernel arguments, pack_kparams), k_chunk_stats<KT> for ncol collapsed-state components, k_reduce
void launch_tables(const Pass& ps, unsigned* flags, bool kp, hipStream_t st);
void launch_chunk_stats(const Track& tr, hipStream_t st, int ncol, const int32_t* ll_off, const double* tile_stats, const double* ll_part,
                        const DevParams* params, double* chunk_stats, int full);
void launch_reduce(const Track& tr, hipStream_t st, const double* rows, const int32_t* row_index, int64_t n_rows, double* out,
                   const unsigned* flags, int n_ranks = 0, int rows_per_rank = 0, int flag_row = 0);
// hf_decoders.hip
void dec_launch_rows_win(const Track& tr, const Decoder& d, const double* nbE, hipStream_t st);
int dec_finish(const Track& tr, Decoder& d, void* stream);
int dec_clear_outputs(const Track& tr, LabelDecoder& d, int per, hipStream_t st);
int dec_finish_chunks(const Track& tr, LabelDecoder& d, int per, void* stream);
int dec_finish_scores(const Track& tr, LabelDecoder& d, double* log_prob_host, void* stream);
int dec_labels(const Track& tr, const LabelDecoder& d, int8_t* labels_host);
int dec_chunk_values(const Track& tr, const LabelDecoder& d, double* out_host);
int smp_keys(SampleSet& s, int64_t first, int n, uint64_t seed);
int smp_finish(const Track& tr, Decoder& d, void* stream);
int smp_labels(const Track& tr, const SampleSet& s, const char* who, int k, int8_t* labels_host);
// hf_estep.hip (hf_getters.h)
int pass_view(hf_ctx* ctx, const std::string& who, int64_t n, PassView& pv);
int rg_check(const hf_ctx* ctx, const std::string& who, int64_t n, bool null_array, const int64_t* first, const int64_t* last,
             const uint8_t* state_mask, const int32_t* region = nullptr, const char* early = nullptr, const char* late = nullptr);

// ------------------------------------------------------------------------------------------
// host templates that take kernels or lambdas and launch nothing
// ------------------------------------------------------------------------------------------
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

// f(std::true_type) for HF_ALGO_SEQ, f(std::false_type) for HF_ALGO_SCAN: one launch per kernel, its template argument the only difference
template <class F>
static void by_algo(const Track& tr, F&& f) {
    if (tr.algo == HF_ALGO_SEQ) f(std::true_type{}); else f(std::false_type{});
}

// What dec_front fills and every decoder has, f(array, bytes) in turn (nrow rows): parameter block, negative-binomial table, rows, flag word
template <class D, class F> static void dec_front_arrays(const Track& tr, D& d, size_t nrow, F&& f) {
    f(d.d_params, tr.params_bytes); f(d.d_nbE, (size_t) tr.R * 4 * HF_NB_NX * 8); f(d.d_rows, nrow * 128); f(d.d_flags, 4);
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

// the largest grid.y of the per-sample launches
#define HF_SMP_MAX_PER_CALL 65535

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

// the tail of an EM step: element 0 becomes the model's log-likelihood, then (mstep) HMM_estimateParameters
inline void em_step_tail(hfm_model* model, const double* stats_host, bool mstep, double tol, int* converged) {
    hfm_set_loglikelihood(model, stats_host[0]);
    if (mstep) {
        const int cv = hfm_estimate(model, stats_host, tol);
        if (converged) *converged = cv;
    }
}

#pragma GCC visibility pop
