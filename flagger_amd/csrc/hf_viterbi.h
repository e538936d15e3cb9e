// hf_viterbi.h — most-probable-path (Viterbi) decoding of every chunk: the shared decoder core (hf_decode.h) in the (max, x) semiring,
// with first-max backpointers as its map bytes.  hf_viterbi runs it once, with the parameters it is given, into buffers of its own.
//
// Definition.  With first, A_t and end of hf_decode.h, for a chunk of T windows:
//   s* = argmax over s_0 .. s_{T-1} of first[s_0] * prod_{t>=1} A_t[s_{t-1}][s_t] * end[s_{T-1}]
// Ties go to the lowest state index at every backpointer and at the final state (strict >, as posterior_label).  The chunk's score is
// log of that maximum; the run's score is the sum over chunks in list order (host).  A running maximum of exactly 0 raises HF_FLAG_SCALE,
// a NaN in a row of A or in the end column HF_FLAG_NAN (the flag bits of a pass, in a flag word of Viterbi's own).
//
// A backpointer is decided by a comparison of two products of the form (mantissas, exponent sum); the products themselves are formed in
// a different association order than a sequential run (lane products, then scans), so the two can differ in the last ulp and break a
// rounding-level tie differently.
//
// HF_ALGO_SCAN: rows, A, B and D of hf_decode.h, and
//   C  k_vit_replay  lane j enters with v_k (x) P_j and replays its windows: delta_t[s] = max_pre delta_{t-1}[pre] * A_t[pre][s] with
//                    first-max backpointers (four 2-bit backpointers = one byte per window, the single sample's maps); lane and segment
//                    maps as hf_decode.h composes them; the lane that holds the chunk's last window picks the final state and writes the
//                    chunk's score
// HF_ALGO_SEQ: k_vit_seq, one wavefront per chunk in window order (rows staged 64 windows at a time through LDS, one lane computes).
#pragma once
#include "hf_decode.h"

#define HF_VIT_LN2 0.6931471805599453094

// one replay step: d <- d (x) A with first-max backpointers packed 2 bits per state
__device__ __forceinline__ unsigned vit_step(double d[4], const double A[16]) {
    double nd[4];
    unsigned bp = 0;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        double best = d[0] * A[s];
        unsigned arg = 0;
#pragma unroll
        for (int p = 1; p < 4; p++) {
            const double v = d[p] * A[p * 4 + s];
            if (v > best) { best = v; arg = (unsigned) p; }
        }
        nd[s] = best;
        bp |= arg << (2 * s);
    }
#pragma unroll
    for (int s = 0; s < 4; s++) d[s] = nd[s];
    return bp;
}

// ---- C: replay with backpointers ---------------------------------------------------------------------------------------------------
// bp[slot] (one byte per window), lmap[seg][lane], smap[seg]; the chunk's last lane: final[c], ll[c]
__global__ void __launch_bounds__(64) k_vit_replay(const SegDesc* __restrict__ segs, const uint32_t* __restrict__ rec,
                                                   const DevParams* __restrict__ P, const double2* __restrict__ rows,
                                                   const double* __restrict__ Pm, const int* __restrict__ PE,
                                                   const double* __restrict__ vin, const long long* __restrict__ vinE,
                                                   uint8_t* __restrict__ bp, uint8_t* __restrict__ lmap, uint8_t* __restrict__ smap,
                                                   int8_t* __restrict__ final_state, double* __restrict__ ll, unsigned* __restrict__ flags) {
    const int g = blockIdx.x, j = threadIdx.x;
    const SegDesc d = segs[g];
    __shared__ uint8_t maps[64];
    const int cnt = dec_lane_count(d, j);
    unsigned map = HF_DEC_MAP_IDENT, bad = 0;
    if (cnt > 0) {
        double dl[4];
        long long e = vinE[g] + PE[(int64_t) g * 64 + j] + dec_enter<MaxTimes>(vin, Pm, g, j, dl);
        for (int i = 0; i < cnt; i++) {
            double A[16];
            dec_load_row(rows, d.slot0, i, j, A);
            const unsigned b = vit_step(dl, A);
            bp[(int64_t) d.slot0 + (int64_t) i * 64 + j] = (uint8_t) b;
            map = i == 0 ? b : dec_map_then(map, b);   // state at this window -> state before the lane's first window
            const double m = fmax(fmax(dl[0], dl[1]), fmax(dl[2], dl[3]));
            if (dl[0] != dl[0] || dl[1] != dl[1] || dl[2] != dl[2] || dl[3] != dl[3]) bad |= HF_FLAG_NAN;
            else if (!(m > 0.0)) bad |= HF_FLAG_SCALE;
            e += dec_norm<4>(dl);
        }
        if (j * d.L + cnt == d.n && d.k == d.nseg - 1) {   // the chunk's last window: final state and score
            const DevRegion* __restrict__ Rl = &P->reg[REC_REGION(rec[d.t0 + d.n - 1])];
            double best = dl[0] * Rl->trans[0][4];
            int arg = 0;
            for (int s = 1; s < 4; s++) {
                const double w = dl[s] * Rl->trans[s][4];
                if (w > best) { best = w; arg = s; }
            }
            if (best != best) bad |= HF_FLAG_NAN;
            else if (!(best > 0.0)) bad |= HF_FLAG_SCALE;
            final_state[d.chunk] = (int8_t) arg;
            ll[d.chunk] = log(best) + (double) e * HF_VIT_LN2;
        }
    }
    dec_seg_maps(d, j, map, maps, lmap + (int64_t) g * 64, smap + g);
    if (bad) atomicOr(flags, bad);
}

// ---- HF_ALGO_SEQ: one wavefront per chunk, window order ----------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_vit_seq(const int64_t* __restrict__ off, const uint32_t* __restrict__ rec,
                                                const DevParams* __restrict__ P, const double2* __restrict__ rows,
                                                uint8_t* __restrict__ bp, int8_t* __restrict__ label, double* __restrict__ ll,
                                                unsigned* __restrict__ flags) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int64_t t0 = off[c], T = off[c + 1] - t0;
    __shared__ double As[64][17];
    if (T <= 0) { if (lane == 0) ll[c] = 0.0; return; }
    double dl[4] = {1.0, 0.0, 0.0, 0.0};
    long long e = 0;
    unsigned bad = 0;
    for (int64_t base = 0; base < T; base += 64) {
        const int n = (int) ((T - base) < 64 ? (T - base) : 64);
        if (lane < n) dec_load_row_win(rows, t0 + base + lane, &As[lane][0]);
        __syncthreads();
        if (lane == 0)
            for (int q = 0; q < n; q++) {
                bp[t0 + base + q] = (uint8_t) vit_step(dl, &As[q][0]);   // (lane 0 stores and later reads its own backpointers)
                const double m = fmax(fmax(dl[0], dl[1]), fmax(dl[2], dl[3]));
                if (dl[0] != dl[0] || dl[1] != dl[1] || dl[2] != dl[2] || dl[3] != dl[3]) bad |= HF_FLAG_NAN;
                else if (!(m > 0.0)) bad |= HF_FLAG_SCALE;
                e += dec_norm<4>(dl);
            }
        __syncthreads();
    }
    if (lane != 0) return;
    const DevRegion* __restrict__ Rl = &P->reg[REC_REGION(rec[t0 + T - 1])];
    double best = dl[0] * Rl->trans[0][4];
    unsigned s = 0;
    for (int q = 1; q < 4; q++) {
        const double w = dl[q] * Rl->trans[q][4];
        if (w > best) { best = w; s = (unsigned) q; }
    }
    if (best != best) bad |= HF_FLAG_NAN;
    else if (!(best > 0.0)) bad |= HF_FLAG_SCALE;
    ll[c] = log(best) + (double) e * HF_VIT_LN2;
    for (int64_t t = t0 + T - 1; t >= t0; t--) {
        label[t] = (int8_t) s;
        s = dec_map_apply(bp[t], s);
    }
    if (bad) atomicOr(flags, bad);
}
