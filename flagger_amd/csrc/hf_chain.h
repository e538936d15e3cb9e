// hf_chain.h — the core of the walkers of a chain expanded by run length, one lane of a 64-lane wavefront per expanded state:
// hf_viterbi_minlen and, over whole contigs, hf_viterbi_minlen_joined (hf_minlen.h), hf_get_long_run_log_probs (hf_longrun.h) and
// hf_minlen_posterior (hf_minlen_post.h; over whole contigs hf_minlen_post_joined.h).  Four things, each here once: the wave primitives, the lane geometry of the minimum-run-length
// expansion, the forward row staging (its tile and rules), and the posterior chain that hf_runlen.hip and hf_countdist.hip walk.
//
// THE EXPANSION by minimum run lengths.  min_len[s] >= 1 windows per state, sum <= 64.  Lanes (s, d), d = 1 .. min_len[s]: "in state s,
// the current run has d windows so far"; at d = min_len[s] "at least that many" (the SATURATED lane; d = 1 is the ENTRY lane; with
// min_len[s] == 1 one lane is both).  Lane index = sum_{q<s} min_len[q] + d - 1; the lanes from the sum of the lengths on are not ACTIVE.
//   an entry lane       is reached from the saturated lanes of p = 0 .. 3, taken in increasing order (a maximum replaces on strict >, so
//                       the lowest p wins a tie; a sum is ((v_0 + v_1) + v_2) + v_3); p == s takes part only when min_len[s] == 1 (the
//                       "stay"), else it is EXCLUDED: the entry lane takes no p == s
//   1 < d < min_len[s]  is reached from (s, d-1) alone, the lane below
//   d = min_len[s] > 1  is reached from (s, d-1) and from itself (the stay), in this order
// All three steps multiply by (in logs: add) A_t[p][s]; a lane reads its column A[0..3][s] and the diagonal A[s][s], a lane that is not
// active the pad column 16 in place of the diagonal.  A chunk's first and last run are exempt: the walk starts in the saturated lanes and
// ends in every lane.  k_lr_chain expands by a run counter with OUT and HIT lanes (hf_longrun.h) and keeps its own geometry.
//
// THE STAGING of a forward walk.  Rows come 64 windows at a time through the LDS tile ChainTile As[65][17] (17: no two rows of a column
// in one bank; row 64 is read ahead and never used), one lane per window; the rows of the next 64 windows wait in the lane's registers
// while these are walked, and the lane's column of window q + 1 is read during the step of window q, so neither global nor LDS latency is
// on the chain.  Column 16 is the "A[s][s]" of the lanes that are not active: -inf in logs (k_mlv_fwd), 0 in the linear domain
// (k_mlp_fwd), absent in k_lr_chain, whose tiles follow the parts of a group.  k_mlp_bwd walks back with the mirror image and a second
// tile of F (hf_minlen_post.h).
//
// WHAT IS CODE HERE AND WHAT IS NOT.  The wave primitives are functions.  The geometry is ONE definition, HF_CHAIN_LANE, that declares
// the calling kernel's constants: as a struct filled by an inlined constructor, together with a shared turn of the tile (put the rows,
// pad, load the next 64, barrier; parameterised by pad and loader), the kernels kept their resource figures and loop lengths, gave the
// same bits, and on the MI355X k_mlv_fwd took 1681 us against 1594 us and k_mlp_fwd 2351 us against 2275 us (configs[2], the two runs of
// the old code 4 us apart): these loops are bound by the latency of one window's chain, and the order in which the compiler meets the
// predicates and the loads decides how it schedules them.  With the declarations below and the turn of the tile written out in each
// forward kernel, every kernel's code is what it was before the three headers shared anything, instruction for instruction
// (profiles/chain_core_cfg2.txt).  A helper that reads a column of the tile, or one that sums the four admitted terms, changed
// k_mlv_fwd's or k_mlp_fwd's code as well, so those lines stay in the walks too.
#pragma once
#include "hf_decode.h"

// ---- wave primitives: every one needs all 64 lanes active -------------------------------------------------------------------------
__device__ __forceinline__ double ch_readlane(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// a DPP move of the two halves; a lane without a source keeps `v`
template <int CTRL>
__device__ __forceinline__ double ch_dpp(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ int ch_dpp(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }

__device__ __forceinline__ double ch_lane_below(double v) { return ch_dpp<0x138>(v); }   // lane - 1 (wave_shr:1), lane 0 its own
__device__ __forceinline__ double ch_lane_above(double v) { return ch_dpp<0x130>(v); }   // lane + 1 (wave_shl:1), lane 63 its own

// the sum of v over the wavefront, the same bits in every lane.  ONE order, part of the documented results: lane ^ 1, lane ^ 2, the
// mirror in 8, the mirror in 16, then the four rows of 16 left to right
__device__ __forceinline__ double ch_wave_sum(double v) {
    v += ch_dpp<0xB1>(v);       // quad_perm [1, 0, 3, 2]
    v += ch_dpp<0x4E>(v);       // quad_perm [2, 3, 0, 1]
    v += ch_dpp<0x141>(v);      // row_half_mirror
    v += ch_dpp<0x140>(v);      // row_mirror
    return ((ch_readlane(v, 0) + ch_readlane(v, 16)) + ch_readlane(v, 32)) + ch_readlane(v, 48);
}

// the largest lane of v (>= 0 everywhere, a NaN is passed over), the same bits in every lane
__device__ __forceinline__ double ch_wave_max(double v) {
    v = fmax(v, ch_dpp<0xB1>(v));
    v = fmax(v, ch_dpp<0x4E>(v));
    v = fmax(v, ch_dpp<0x141>(v));
    v = fmax(v, ch_dpp<0x140>(v));
    return fmax(fmax(ch_readlane(v, 0), ch_readlane(v, 16)), fmax(ch_readlane(v, 32), ch_readlane(v, 48)));
}

// the largest lane of an integer, the same in every lane
__device__ __forceinline__ int ch_wave_max(int v) {
    v = max(v, ch_dpp<0xB1>(v));
    v = max(v, ch_dpp<0x4E>(v));
    v = max(v, ch_dpp<0x141>(v));
    v = max(v, ch_dpp<0x140>(v));
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// the exponent a rescaling takes out to bring the (uniform) largest value mx to exponent `target`: 0 when mx is 0 or not finite
__device__ __forceinline__ int ch_shift(double mx, int target) {
    return (mx > 0.0 && !isinf(mx)) ? __builtin_amdgcn_readfirstlane(ilogb(mx)) - target : 0;
}

// ---- lane geometry of the expansion by minimum run lengths -----------------------------------------------------------------------
// min_len of state s out of the four lengths packed one per byte
__device__ __forceinline__ int ch_len(unsigned mpack, int s) { return (int) ((mpack >> (8 * s)) & 0xffu); }

// The wave-uniform part, as constants of the calling kernel: b1, b2, b3 the first lane of states 1, 2, 3 and total the number of active
// lanes; ent0..3 and sat0..3 every state's entry and saturated lane; mpack for ch_len.  k_mlv_back needs no more than this to turn a
// final lane into (state, d).
#define HF_CHAIN_LENS(m0, m1, m2, m3) \
    const int b1 = (m0), b2 = (m0) + (m1), b3 = b2 + (m2), total = b3 + (m3); \
    __attribute__((unused)) const int ent0 = 0, ent1 = b1, ent2 = b2, ent3 = b3; \
    __attribute__((unused)) const int sat0 = b1 - 1, sat1 = b2 - 1, sat2 = b3 - 1, sat3 = total - 1; \
    const unsigned mpack = (unsigned) (m0) | (unsigned) (m1) << 8 | (unsigned) (m2) << 16 | (unsigned) (m3) << 24
// ... and the lane's place: s, m = min_len[s], d; active; inner (d < m: the lane hands on to the lane above it), is_entry, is_sat; excl
// (the entry lane takes no p == s; mirrored, the saturated lane leaves to no q == s); diag, the column of the tile where the lane reads
// A[s][s]
#define HF_CHAIN_LANE(m0, m1, m2, m3, lane) \
    HF_CHAIN_LENS(m0, m1, m2, m3); \
    const int s = ((lane) >= b1) + ((lane) >= b2) + ((lane) >= b3); \
    const int base_s = s == 0 ? 0 : s == 1 ? b1 : s == 2 ? b2 : b3; \
    const int m = ch_len(mpack, s), d = (lane) - base_s + 1; \
    const bool active = (lane) < total; \
    __attribute__((unused)) const bool inner = d < m; \
    __attribute__((unused)) const bool is_entry = active && d == 1, is_sat = active && d == m && m > 1; \
    const bool excl = m > 1; \
    const int diag = active ? 5 * s : 16

// One step of a walk back through the backpointer words of hf_minlen.h: from (cs, cd) at a window to its predecessor's, by the window's
// word w.  An entry lane goes to the saturated lane of its predecessor; any other one lane down, unless the saturated lane stayed.
template <class W>
__device__ __forceinline__ void ch_step_back(unsigned mpack, W w, int& cs, int& cd) {
    const int p = (int) (w >> (2 * cs)) & 3, stayed = (int) (w >> (8 + cs)) & 1;
    const bool entry = cd == 1;
    const int down = (cd < ch_len(mpack, cs)) | (stayed ^ 1);
    cd = entry ? ch_len(mpack, p) : cd - down;
    cs = entry ? p : cs;
}

// ---- the posterior chain of the lane-per-age and lane-per-bin walkers (hf_runlen.hip, hf_countdist.hip) --------------------------
// Given the data the states of a chunk are a Markov chain.  Its rows at a window with row A of the pass and backward vector b:
// r[p * 4 + q] = Q[p][q] = A[p][q] b[q] / sum_q' A[p][q'] b[q'] (q' = 0..3 in order); a row whose denominator is 0 is a zero row
__device__ __forceinline__ void ch_post_rows(const double A[16], const double b[4], double r[16]) {
#pragma unroll
    for (int p = 0; p < 4; p++) {
        double y[4];
#pragma unroll
        for (int q = 0; q < 4; q++) y[q] = A[p * 4 + q] * b[q];
        const double den = ((y[0] + y[1]) + y[2]) + y[3];
#pragma unroll
        for (int q = 0; q < 4; q++) r[p * 4 + q] = den > 0.0 ? y[q] / den : 0.0;
    }
}

// ... and its start at a part's first window: g[s] = f[s] b[s] / sum_s' f[s'] b[s'] (s' in order) for the states of the bit set `keep`,
// 0.0 for the others and where the sum is 0
__device__ __forceinline__ void ch_post_start(const double f[4], const double b[4], int keep, double g[4]) {
    double y[4];
#pragma unroll
    for (int s = 0; s < 4; s++) y[s] = f[s] * b[s];
    const double tot = ((y[0] + y[1]) + y[2]) + y[3];
#pragma unroll
    for (int s = 0; s < 4; s++) g[s] = (((keep >> s) & 1) && tot > 0.0) ? y[s] / tot : 0.0;
}

// ---- forward row staging: the tile (the turn of it is written out in the three forward kernels, see above) -------------------------
typedef double ChainTile[65][17];
