// hf_minlen.h — minimum-run-length Viterbi (hf_viterbi_minlen): the most probable path among the paths whose runs meet a minimum length
// per state.  A decoder beside hf_viterbi: the same first, A_t and end (hf_decode.h), buffers of its own, ONE code path for both kinds of
// context (rows in window order, one wavefront per chunk).
//
// Definition.  min_len[s] >= 1 windows per state, sum <= HF_MINLEN_MAX_LANES.  A path of a chunk is ADMISSIBLE when every maximal run of
// equal state s has at least min_len[s] windows; a run that contains the chunk's first or last window is exempt (a chunk is a cut of a
// contig).  The decoder returns the admissible path of the largest weight first[s_0] * prod_t A_t[s_{t-1}][s_t] * end[s_{T-1}].
//
// The expanded chain: lanes (s, d), entry and saturated lanes, the exclusion of p == s and the tie rule as hf_chain.h defines them.
//   window 0     delta[(s, min_len[s])] = first[s], nothing elsewhere (the exempt left end)
//   entry        max over the admitted p of delta[(p, min_len[p])] + A_t[p][s]
//   1 < d < m    delta[(s, d-1)] + A_t[s][s]
//   d = m > 1    delta[(s, d-1)] + A_t[s][s], then delta[(s, d)] + A_t[s][s], strict >
//   end          max over all lanes in lane order of delta[(s, d)] + end[s], strict > (the exempt right end)
// With all four lengths 1 this is hf_viterbi's recurrence and tie rule.
//
// OVER WHOLE CONTIGS (hf_viterbi_minlen_joined): the same decoder with the rule applied to GROUPS of joined chunks instead of chunks.
// joined[c] != 0 says that chunk c continues chunk c-1 (the rule of hf_get_run_moments); a group is a maximal sequence of chunks joined
// to each other, one contiguous window range, and only a run that contains the group's first or last window is exempt.  Chunks stay
// independent chains: the weight of a group's path is the product of its chunks' weights, first * prod A_t * end per chunk.
// The chain is the one above: its lanes, its entry, in-between and saturated steps, its tie rules, in logs.  What differs:
//   window 0 and the end   are the group's first window and the end column of the group's last window
//   a joined chunk-first window t (the first window of a chunk that is not the group's first) is an ordinary step with the row
//                          J_t[p][s] = log end_{c-1}[p] + log first_c[s],  end_{c-1}[p] = trans[r_{t-1}][p][4],
//                          first_c[s] row pre = 0 of the chunk-first row as k_mlv_rows stores it; -inf when either term is -inf.  The
//                          run counter runs on across the boundary.
// HF_FLAG_NAN also for a NaN in an end column read at a joined boundary.
//
// Numerics: LOGS.  k_mlv_rows stores log of every entry of the row (-inf for 0), so a step of the chain is one add and one compare and
// nothing under- or overflows at any chunk length; the (mantissa, exponent) form of hf_decode.h would need a wave-wide maximum per
// window.  A chunk's score is the maximum itself.  HF_FLAG_NAN: a NaN in a row (k_mlv_rows, as dec_row) or in the end column;
// HF_FLAG_SCALE: the maximum of a chunk is -inf, no admissible path has weight.
//
// k_mlv_fwd: one 64-lane workgroup per chunk, lane = expanded state, the staging of hf_chain.h with -inf as the pad.  Per window a lane
// takes the four saturated lanes' values (readlane at wave-uniform indices) and the value of the lane below it (a DPP shift by one
// lane); nothing else crosses lanes.
// BACKPOINTERS: one 16-bit word per window: bits 2s, 2s+1 the predecessor state of state s's entry lane, bit 8+s set when state s's
// saturated lane stayed (clear: it arrived from d-1).  An owning lane keeps its own decisions of 16 windows in a register, 2 bits per
// window; after the 16, lane l builds the word of window l from the eight owning lanes' registers, read at their (uniform) lane
// indices, and the words of 64 windows go out in one store.
// k_mlvj_fwd: k_mlv_fwd's walk with one 64-lane workgroup per GROUP.  Rows come from k_mlv_rows unchanged.  Inside a group every window
// past the first whose record carries the chunk-first bit is a joined chunk-first window, so the group ranges are all the host uploads.
// The lane that stages such a window writes J_t into the tile in place of the staged row (four logs of the previous window's region's
// end column, once per boundary, off the chain); the step itself reads its five operands from the tile as everywhere.  The record word
// of the next 64 windows waits in a register beside their rows.  The word of a joined chunk-first window is read like any other, so the
// walk back is k_mlv_back over the group ranges.  A group is as long as a contig: the window index is 64-bit wherever k_mlv_fwd's is.
// TWO BODIES, ON PURPOSE.  k_mlvj_fwd is k_mlv_fwd line for line but for the block (goff / gchunk for off / c), the record word nr beside
// the rows, the J_t branch of the staging lane and the early `bad`: a fix to the tie rule, the word format or the flags goes into both.
// As one template <bool JOINED> body behind two __global__ wrappers k_mlv_fwd kept its code (operands of commutative instructions
// swapped) and k_mlvj_fwd its registers, LDS and per-window loops, with one more v_mov in the per-64-window loop and other registers;
// on the MI355X k_mlvj_fwd then took 9984 and 9906 us against 9800 and 9810 us (configs[2]), ten times what the two runs of the old
// code are apart, so the walks stay written out, as the turn of the tile does in hf_chain.h (profiles/minlen_front_cfg2.txt).  And
// k_mlvj_fwd stays the LAST kernel of the translation unit (hf_minlen_joined.h): its own text, put next to k_mlv_fwd or behind
// k_mlv_back in this header, is compiled into k_mlv_fwd's longer per-window loops (59 / 117 -> 62 / 120 instructions).
// k_mlv_back: one 64-lane workgroup per chunk (per group) walks back from its final lane: lane q loads the word of window t-q, and
// (s, d) is carried through the 64 words in registers on the scalar side — a word's address does not depend on the state — while lane
// q keeps label[t-q] for one store.
#pragma once
#include "hf_chain.h"

#define HF_MLV_NEG_INF (-__builtin_huge_val())

// rows: log of the row of every window, window order, the layout of k_dec_rows_win
__global__ void __launch_bounds__(256) k_mlv_rows(int64_t N, const uint32_t* __restrict__ rec, const double* __restrict__ beta,
                                                  const DevParams* __restrict__ P, const double* __restrict__ nbE,
                                                  double2* __restrict__ rows, unsigned* __restrict__ flags) {
    dec_rows_win<true>(N, rec, beta, P, nbE, rows, flags);
}

__global__ void __launch_bounds__(64) k_mlv_fwd(const int64_t* __restrict__ off, const uint32_t* __restrict__ rec,
                                                const DevParams* __restrict__ P, const double2* __restrict__ rows, int m0, int m1, int m2,
                                                int m3, uint16_t* __restrict__ bp, uint8_t* __restrict__ final_lane, double* __restrict__ ll,
                                                unsigned* __restrict__ flags) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int64_t t0 = off[c], T = off[c + 1] - t0;
    __shared__ ChainTile As;
    if (T <= 0) { if (lane == 0) { ll[c] = 0.0; final_lane[c] = 0; } return; }
    HF_CHAIN_LANE(m0, m1, m2, m3, lane);
    const int pf = (excl && s == 0) ? 1 : 0;                // the entry lane's first candidate

    double x = HF_MLV_NEG_INF;
    double2 nx[8];
    if (lane < T) {
#pragma unroll
        for (int k = 0; k < 8; k++) nx[k] = rows[(t0 + lane) * 8 + k];
    }
    for (int64_t base = 0; base < T; base += 64) {
        const int n = (int) ((T - base) < 64 ? (T - base) : 64);
        if (lane < n) {
#pragma unroll
            for (int k = 0; k < 8; k++) { As[lane][2 * k] = nx[k].x; As[lane][2 * k + 1] = nx[k].y; }
            As[lane][16] = HF_MLV_NEG_INF;
        }
        if (base + 64 + lane < T) {
#pragma unroll
            for (int k = 0; k < 8; k++) nx[k] = rows[(t0 + base + 64 + lane) * 8 + k];
        }
        __syncthreads();
        const int q0 = base == 0 ? 1 : 0;
        // window 0: first[s] (row pre = 0 of the chunk-first row) in every state's saturated lane
        if (base == 0 && active && d == m) x = As[0][s];
        int words = 0;
        double c0, c1, c2, c3, css;
        c0 = As[q0][s]; c1 = As[q0][4 + s]; c2 = As[q0][8 + s]; c3 = As[q0][12 + s]; css = As[q0][diag];
        for (int qb = q0; qb < n; qb += 16) {
            // 16 windows; a lane keeps its own decisions, 2 bits per window: an entry lane its predecessor, a saturated lane "stayed"
            const int cnt = n - qb < 16 ? n - qb : 16;
            unsigned hist = 0;
            for (int q = qb; q < qb + cnt; q++) {
                const double a0 = c0, a1 = c1, a2 = c2, a3 = c3, ass = css;
                c0 = As[q + 1][s]; c1 = As[q + 1][4 + s]; c2 = As[q + 1][8 + s]; c3 = As[q + 1][12 + s]; css = As[q + 1][diag];
                const double v0 = ch_readlane(x, sat0) + a0, v1 = ch_readlane(x, sat1) + a1;
                const double v2 = ch_readlane(x, sat2) + a2, v3 = ch_readlane(x, sat3) + a3;
                const double up = ch_lane_below(x) + ass, stay = x + ass;
                // the entry lane: candidates p = pf .. 3 in increasing order, without the excluded p == s
                double best = pf ? v1 : v0;
                unsigned arg = (unsigned) pf;
                if (pf < 1 && !(excl && s == 1) && v1 > best) { best = v1; arg = 1; }
                if (!(excl && s == 2) && v2 > best) { best = v2; arg = 2; }
                if (!(excl && s == 3) && v3 > best) { best = v3; arg = 3; }
                const bool stayed = is_sat && stay > up;
                x = is_entry ? best : (stayed ? stay : up);   // (a lane past the last one: up = -inf)
                hist = hist << 2 | (is_entry ? arg : (stayed ? 1u : 0u));
            }
            // the words of these windows: lane l takes the one of window l, its bits out of the eight owning lanes' histories
            const int sh = 2 * ((qb + cnt - 1 - lane) & 15);
            const unsigned e0 = (unsigned) __builtin_amdgcn_readlane((int) hist, ent0), e1 = (unsigned) __builtin_amdgcn_readlane((int) hist, ent1);
            const unsigned e2 = (unsigned) __builtin_amdgcn_readlane((int) hist, ent2), e3 = (unsigned) __builtin_amdgcn_readlane((int) hist, ent3);
            const unsigned s0 = (unsigned) __builtin_amdgcn_readlane((int) hist, sat0), s1 = (unsigned) __builtin_amdgcn_readlane((int) hist, sat1);
            const unsigned s2 = (unsigned) __builtin_amdgcn_readlane((int) hist, sat2), s3 = (unsigned) __builtin_amdgcn_readlane((int) hist, sat3);
            const unsigned w = ((e0 >> sh) & 3u) | ((e1 >> sh) & 3u) << 2 | ((e2 >> sh) & 3u) << 4 | ((e3 >> sh) & 3u) << 6 |
                               ((s0 >> sh) & (m0 > 1 ? 1u : 0u)) << 8 | ((s1 >> sh) & (m1 > 1 ? 1u : 0u)) << 9 |
                               ((s2 >> sh) & (m2 > 1 ? 1u : 0u)) << 10 | ((s3 >> sh) & (m3 > 1 ? 1u : 0u)) << 11;
            if (lane >= qb && lane < qb + cnt) words = (int) w;
        }
        if (lane < n) bp[t0 + base + lane] = (uint16_t) words;   // (the word of a chunk's first window is never read)
        __syncthreads();
    }

    // the end: the first largest lane in lane order
    const DevRegion* __restrict__ Rl = &P->reg[REC_REGION(rec[t0 + T - 1])];
    const double e = active ? Rl->trans[s][4] : 1.0;
    unsigned bad = e != e ? HF_FLAG_NAN : 0u;
    double fw = active ? x + (e == 0.0 ? HF_MLV_NEG_INF : log(e)) : HF_MLV_NEG_INF;
    if (fw != fw) bad |= HF_FLAG_NAN;
    int fl = lane;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double ow = __shfl_xor(fw, o, 64);
        const int ol = __shfl_xor(fl, o, 64);
        if (ow > fw || (ow == fw && ol < fl)) { fw = ow; fl = ol; }
    }
    if (!(fw > HF_MLV_NEG_INF) && fw == fw) bad |= HF_FLAG_SCALE;
    if (lane == 0) { ll[c] = fw; final_lane[c] = (uint8_t) fl; }
    if (bad) atomicOr(flags, bad);
}

// the walk back, wave-uniform: (cs, cd) through the words of 64 windows at a time
__global__ void __launch_bounds__(64) k_mlv_back(const int64_t* __restrict__ off, int m0, int m1, int m2, int m3,
                                                 const uint16_t* __restrict__ bp, const uint8_t* __restrict__ final_lane,
                                                 int8_t* __restrict__ label) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int64_t t0 = off[c], T = off[c + 1] - t0;
    if (T <= 0) return;
    HF_CHAIN_LENS(m0, m1, m2, m3);
    const int fl = __builtin_amdgcn_readfirstlane((int) final_lane[c]);
    int cs = (fl >= b1) + (fl >= b2) + (fl >= b3);
    int cd = fl - (cs == 0 ? 0 : cs == 1 ? b1 : cs == 2 ? b2 : b3) + 1;
    for (int64_t hi = T - 1; hi >= 0; hi -= 64) {
        const int n = (int) (hi + 1 < 64 ? hi + 1 : 64);
        const int wd = (lane < n && hi - lane >= 1) ? (int) bp[t0 + hi - lane] : 0;
        int lab = 0;
        for (int q = 0; q < n; q++) {
            lab = lane == q ? cs : lab;
            ch_step_back(mpack, __builtin_amdgcn_readlane(wd, q), cs, cd);
        }
        if (lane < n) label[t0 + hi - lane] = (int8_t) lab;
    }
}

// k_mlvj_fwd is defined in hf_minlen_joined.h, which hf_minlen.hip includes behind every other kernel header of the family (see above)
__global__ void k_mlvj_fwd(const int64_t* __restrict__ goff, const int32_t* __restrict__ gchunk, const uint32_t* __restrict__ rec,
                           const DevParams* __restrict__ P, const double2* __restrict__ rows, int m0, int m1, int m2, int m3, uint16_t* __restrict__ bp,
                           uint8_t* __restrict__ final_lane, double* __restrict__ ll, unsigned* __restrict__ flags);
