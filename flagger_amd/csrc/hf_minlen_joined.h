// hf_minlen_joined.h — k_mlvj_fwd, the forward walk of hf_viterbi_minlen_joined: k_mlv_fwd's walk with one 64-lane workgroup per group of
// joined chunks.  The rule, the kernel's description and why it is a second body are in hf_minlen.h; why it is a file of its own, the
// LAST KERNEL HEADER OF hf_minlen.hip: there its code is what it has been; in hf_minlen.h, behind k_mlv_fwd or behind k_mlv_back, the
// compiler gives its per-window loops the longer form of k_mlv_fwd's (59 / 117 -> 62 / 120 instructions;
// profiles/minlen_front_cfg2.txt).  The rule binds inside that unit only: no other unit's text stands in front of this kernel or behind it.
#pragma once
#include "hf_minlen.h"

// goff[G + 1]: the window range of every group; gchunk[G]: the group's first chunk, whose entry of ll takes the group's score (the
// entries of its other chunks stay 0); final_lane[g] per group
__global__ void __launch_bounds__(64) k_mlvj_fwd(const int64_t* __restrict__ goff, const int32_t* __restrict__ gchunk,
                                                 const uint32_t* __restrict__ rec, const DevParams* __restrict__ P,
                                                 const double2* __restrict__ rows, int m0, int m1, int m2, int m3, uint16_t* __restrict__ bp,
                                                 uint8_t* __restrict__ final_lane, double* __restrict__ ll, unsigned* __restrict__ flags) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int64_t t0 = goff[g], T = goff[g + 1] - t0;
    __shared__ ChainTile As;
    if (T <= 0) { if (lane == 0) { ll[gchunk[g]] = 0.0; final_lane[g] = 0; } return; }
    HF_CHAIN_LANE(m0, m1, m2, m3, lane);
    const int pf = (excl && s == 0) ? 1 : 0;                // the entry lane's first candidate

    double x = HF_MLV_NEG_INF;
    double2 nx[8];
    uint32_t nr = 0;                                        // the record of the window whose row waits in nx
    unsigned bad = 0;
    if (lane < T) {
#pragma unroll
        for (int k = 0; k < 8; k++) nx[k] = rows[(t0 + lane) * 8 + k];
        nr = rec[t0 + lane];
    }
    for (int64_t base = 0; base < T; base += 64) {
        const int n = (int) ((T - base) < 64 ? (T - base) : 64);
        if (lane < n) {
            if (base + lane > 0 && REC_FIRST(nr)) {
                // a joined chunk-first window: J_t[p][s] = log end[p] of the previous window's region + log first[s]
                const DevRegion* __restrict__ Rp = &P->reg[REC_REGION(rec[t0 + base + lane - 1])];
                const double f0 = nx[0].x, f1 = nx[0].y, f2 = nx[1].x, f3 = nx[1].y;
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const double e = Rp->trans[p][4];
                    if (e != e) bad |= HF_FLAG_NAN;
                    const double le = e == 0.0 ? HF_MLV_NEG_INF : log(e);
                    As[lane][4 * p] = le + f0; As[lane][4 * p + 1] = le + f1; As[lane][4 * p + 2] = le + f2; As[lane][4 * p + 3] = le + f3;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; k++) { As[lane][2 * k] = nx[k].x; As[lane][2 * k + 1] = nx[k].y; }
            }
            As[lane][16] = HF_MLV_NEG_INF;
        }
        if (base + 64 + lane < T) {
#pragma unroll
            for (int k = 0; k < 8; k++) nx[k] = rows[(t0 + base + 64 + lane) * 8 + k];
            nr = rec[t0 + base + 64 + lane];
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
        if (lane < n) bp[t0 + base + lane] = (uint16_t) words;   // (the word of a group's first window is never read)
        __syncthreads();
    }

    // the end: the end column of the group's last window, the first largest lane in lane order
    const DevRegion* __restrict__ Rl = &P->reg[REC_REGION(rec[t0 + T - 1])];
    const double e = active ? Rl->trans[s][4] : 1.0;
    if (e != e) bad |= HF_FLAG_NAN;
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
    if (lane == 0) { ll[gchunk[g]] = fw; final_lane[g] = (uint8_t) fl; }
    if (bad) atomicOr(flags, bad);
}
