// hf_viterbi.h — most-probable-path (Viterbi) decoding of every chunk: the forward recurrence of the pass in the (max, x) semiring plus a
// backtrack.  Not part of an EM pass: hf_viterbi runs it once, with the parameters it is given, into buffers of its own.
//
// Definition.  For a chunk of T windows with parameters p (the same quantities a pass uses, hmm.c:333-420):
//   first[s]     = trans[r_0][4][s] * e_0[s]                      (start row x emission of the chunk's first window)
//   A_t[pre][s]  = T_t[pre][s] * e_t[pre][s],  t >= 1             (region change => 0.2, validity masks, alpha, beta: the rows of a pass)
//   end[s]       = trans[r_{T-1}][s][4]
//   s* = argmax over s_0 .. s_{T-1} of first[s_0] * prod_{t>=1} A_t[s_{t-1}][s_t] * end[s_{T-1}]
// Ties go to the lowest state index at every backpointer and at the final state (strict >, as posterior_label).  The chunk's score is
// log of that maximum; the run's score is the sum over chunks in list order (host).  A running maximum of exactly 0 raises HF_FLAG_SCALE,
// a NaN in a row of A or in the end column HF_FLAG_NAN (the flag bits of a pass, in a flag word of Viterbi's own).
//
// Rows.  k_vit_rows evaluates the emission row of every window directly (hf_emit_values, or the caller's negative-binomial table) and
// multiplies it by the window's transition row (load_T): one 128-byte row A_t per window.  The chunk-first window's row holds first[s]
// in row pre = 0 and zeros elsewhere, so every chunk starts from the vector (1, 0, 0, 0).
//
// Numerics.  Vectors and matrices are renormalised after every product by 2^-e, e = the exponent of their largest entry: exact
// (unless an entry falls out of the normal range relative to the largest), so the
// value carried is (mantissas, integer exponent sum) and the score is log(max) + e_sum * ln 2 with one log per chunk.  A backpointer
// is decided by a comparison of two products of that form; the products themselves are formed in a different association order than a
// sequential run (lane products, then scans), so the two can differ in the last ulp and break a rounding-level tie differently.
//
// HF_ALGO_SCAN: the segment plan of hf_create (SegDesc, hf_seg.h: segments of <= 64 x HF_SEG_LMAX windows, lane j owns windows
// j*L .. j*L+L-1 of its segment).  Rows and backpointers live in SLOT order (window w = j*L + i of a segment in slot slot0 + i*64 + j);
// a row is 8 pieces of 16 bytes stored piece-major inside a step, so the 64 lanes of a step read 1 KiB contiguous per instruction.
//   A  k_vit_prod    lane product Q_j = A_{jL} (x) ... (x) A_{jL+L-1}; inclusive scan over the 64 lanes (shuffles); every lane keeps
//                    the EXCLUSIVE prefix P_j, the segment its total S
//   B  k_vit_chain   per chunk, over its segments in order: v_0 = (1,0,0,0), v_{k+1} = v_k (x) S_k — the vector entering every segment
//   C  k_vit_replay  lane j enters with v_k (x) P_j and replays its windows: delta_t[s] = max_pre delta_{t-1}[pre] * A_t[pre][s] with
//                    first-max backpointers (four 2-bit backpointers = one byte per window); the lane's map (its exit state -> the
//                    state before its first window) is the composition of its backpointers, the segment's the composition of its
//                    lanes'; the lane that holds the chunk's last window picks the final state and writes the chunk's score
//   D  k_vit_exits   per chunk, over its segments from the end: the exit state of every segment (integer maps: exact)
//      k_vit_back    every lane gets its exit state from the lane maps, walks its backpointers and writes the labels (window order)
// HF_ALGO_SEQ: k_vit_seq, one wavefront per chunk in window order (rows staged 64 windows at a time through LDS, one lane computes):
// the on-device cross-check, as hf_seq.h is for the pass.
#pragma once
#include "hf_device.h"

#define HF_VIT_LN2 0.6931471805599453094

// emission x transition row of window t (layout [pre*4 + s]); chunk-first: first[s] in row 0
__device__ __forceinline__ void vit_row(const uint32_t* __restrict__ rec, const double* __restrict__ beta, const DevParams* __restrict__ P,
                                        const double* __restrict__ nbE, int64_t t, double out[16], unsigned* nan) {
    const uint32_t r = rec[t];
    const bool first = REC_FIRST(r) != 0;
    const DevRegion* __restrict__ R = &P->reg[REC_REGION(r)];
    if (nbE) {
        for (int s = 0; s < 4; s++) {
            const double e = nbE[((int64_t) REC_REGION(r) * 4 + s) * (HF_NB_MAX_COVERAGE + 1) + REC_X(r)];
            for (int p = 0; p < 4; p++) out[p * 4 + s] = (first && p != 0) ? 0.0 : e;
        }
    } else {
        const double x = (double) REC_X(r), px = first ? 0.0 : (double) REC_X(rec[t - 1]);
        hf_emit_values(P, R, x, px, first, beta[t], out, nan);
    }
    if (first) {
#pragma unroll
        for (int s = 0; s < 4; s++) out[s] *= R->trans[4][s];
    } else {
        double Tm[16];
        load_T(P, r, Tm);
#pragma unroll
        for (int k = 0; k < 16; k++) out[k] = Tm[k] * out[k];
    }
#pragma unroll
    for (int k = 0; k < 16; k++) if (out[k] != out[k]) *nan |= HF_FLAG_NAN;
}

// scale v[0..N) by 2^-e, e = exponent of the largest entry (exact for normal results); returns e (0 when every entry is 0)
template <int N>
__device__ __forceinline__ int vit_norm(double* v) {
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < N; k++) m = fmax(m, v[k]);
    if (!(m > 0.0) || isinf(m)) return 0;
    const int e = ilogb(m);
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = ldexp(v[k], -e);
    return e;
}

// C = A (x) B in the (max, x) semiring; C may alias neither
__device__ __forceinline__ void vit_mm(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            double m = A[i * 4] * B[k];
#pragma unroll
            for (int j = 1; j < 4; j++) m = fmax(m, A[i * 4 + j] * B[j * 4 + k]);
            C[i * 4 + k] = m;
        }
}

__device__ __forceinline__ void vit_ident(double* M) {
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

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

__device__ __forceinline__ unsigned vit_map_apply(unsigned map, unsigned s) { return (map >> (2 * s)) & 3u; }
#define HF_VIT_MAP_IDENT 0xE4u   // 3 2 1 0

// index (double2 units) of piece k of the row of step i, lane j of a segment whose first slot is slot0
__device__ __forceinline__ int64_t vit_slot_piece(int64_t slot0, int i, int k, int j) { return slot0 * 8 + ((int64_t) i * 8 + k) * 64 + j; }

// ---- rows ----------------------------------------------------------------------------------------------------------------------
// HF_ALGO_SCAN: one workgroup of 64 per segment, slot-ordered pieces
__global__ void __launch_bounds__(64) k_vit_rows_seg(const SegDesc* __restrict__ segs, const uint32_t* __restrict__ rec,
                                                     const double* __restrict__ beta, const DevParams* __restrict__ P,
                                                     const double* __restrict__ nbE, double2* __restrict__ rows, unsigned* __restrict__ flags) {
    const SegDesc d = segs[blockIdx.x];
    const int j = threadIdx.x;
    unsigned nan = 0;
    for (int i = 0; i < d.L; i++) {
        const int x = j * d.L + i;
        if (x >= d.n) break;
        double a[16];
        vit_row(rec, beta, P, nbE, d.t0 + x, a, &nan);
#pragma unroll
        for (int k = 0; k < 8; k++) rows[vit_slot_piece(d.slot0, i, k, j)] = make_double2(a[2 * k], a[2 * k + 1]);
    }
    if (nan) atomicOr(flags, nan);
}

// HF_ALGO_SEQ: one thread per window, window order
__global__ void __launch_bounds__(256) k_vit_rows_win(int64_t N, const uint32_t* __restrict__ rec, const double* __restrict__ beta,
                                                      const DevParams* __restrict__ P, const double* __restrict__ nbE,
                                                      double2* __restrict__ rows, unsigned* __restrict__ flags) {
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    unsigned nan = 0;
    double a[16];
    vit_row(rec, beta, P, nbE, t, a, &nan);
#pragma unroll
    for (int k = 0; k < 8; k++) rows[t * 8 + k] = make_double2(a[2 * k], a[2 * k + 1]);
    if (nan) atomicOr(flags, nan);
}

__device__ __forceinline__ void vit_load_row(const double2* __restrict__ rows, int64_t slot0, int i, int j, double A[16]) {
#pragma unroll
    for (int k = 0; k < 8; k++) { const double2 v = rows[vit_slot_piece(slot0, i, k, j)]; A[2 * k] = v.x; A[2 * k + 1] = v.y; }
}

// ---- A: lane products and their exclusive scan over the lanes --------------------------------------------------------------------
// P[seg][k][lane] (16 doubles, k-major: coalesced), PE[seg][lane]; S[seg][16], SE[seg]
__global__ void __launch_bounds__(64) k_vit_prod(const SegDesc* __restrict__ segs, const double2* __restrict__ rows,
                                                 double* __restrict__ Pm, int* __restrict__ PE, double* __restrict__ S, int* __restrict__ SE) {
    const int g = blockIdx.x, j = threadIdx.x;
    const SegDesc d = segs[g];
    double Q[16];
    int e = 0;
    vit_ident(Q);
    for (int i = 0; i < d.L; i++) {
        if (j * d.L + i >= d.n) break;
        double A[16], Nq[16];
        vit_load_row(rows, d.slot0, i, j, A);
        vit_mm(Q, A, Nq);
        e += vit_norm<16>(Nq);
#pragma unroll
        for (int k = 0; k < 16; k++) Q[k] = Nq[k];
    }
    // inclusive scan I_j = Q_0 (x) ... (x) Q_j (Hillis-Steele: the earlier product on the left)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        double L[16];
#pragma unroll
        for (int k = 0; k < 16; k++) L[k] = __shfl_up(Q[k], off, 64);
        const int le = __shfl_up(e, off, 64);
        if (j >= off) {
            double Nq[16];
            vit_mm(L, Q, Nq);
            e += le + vit_norm<16>(Nq);
#pragma unroll
            for (int k = 0; k < 16; k++) Q[k] = Nq[k];
        }
    }
    // exclusive: lane j takes lane j-1's inclusive product, lane 0 the identity
    double X[16];
#pragma unroll
    for (int k = 0; k < 16; k++) X[k] = __shfl_up(Q[k], 1, 64);
    int xe = __shfl_up(e, 1, 64);
    if (j == 0) { vit_ident(X); xe = 0; }
#pragma unroll
    for (int k = 0; k < 16; k++) Pm[((int64_t) g * 16 + k) * 64 + j] = X[k];
    PE[(int64_t) g * 64 + j] = xe;
    if (j == 63) {
#pragma unroll
        for (int k = 0; k < 16; k++) S[(int64_t) g * 16 + k] = Q[k];
        SE[g] = e;
    }
}

// ---- B: the vector entering every segment, one thread per chunk ------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_vit_chain(int C, const int32_t* __restrict__ cseg0, const double* __restrict__ S,
                                                  const int* __restrict__ SE, double* __restrict__ vin, long long* __restrict__ vinE) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double v[4] = {1.0, 0.0, 0.0, 0.0};
    long long e = 0;
    for (int g = cseg0[c]; g < cseg0[c + 1]; g++) {
#pragma unroll
        for (int s = 0; s < 4; s++) vin[(int64_t) g * 4 + s] = v[s];
        vinE[g] = e;
        const double* __restrict__ M = S + (int64_t) g * 16;
        double nv[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            double m = v[0] * M[s];
#pragma unroll
            for (int p = 1; p < 4; p++) m = fmax(m, v[p] * M[p * 4 + s]);
            nv[s] = m;
        }
        e += SE[g] + vit_norm<4>(nv);
#pragma unroll
        for (int s = 0; s < 4; s++) v[s] = nv[s];
    }
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
    const int cnt = d.n - j * d.L < d.L ? d.n - j * d.L : d.L;   // windows of this lane (<= 0: none)
    unsigned map = HF_VIT_MAP_IDENT, bad = 0;
    if (cnt > 0) {
        double v[4], X[16];
#pragma unroll
        for (int s = 0; s < 4; s++) v[s] = vin[(int64_t) g * 4 + s];
#pragma unroll
        for (int k = 0; k < 16; k++) X[k] = Pm[((int64_t) g * 16 + k) * 64 + j];
        double dl[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            double m = v[0] * X[s];
#pragma unroll
            for (int p = 1; p < 4; p++) m = fmax(m, v[p] * X[p * 4 + s]);
            dl[s] = m;
        }
        long long e = vinE[g] + PE[(int64_t) g * 64 + j] + vit_norm<4>(dl);
        for (int i = 0; i < cnt; i++) {
            double A[16];
            vit_load_row(rows, d.slot0, i, j, A);
            const unsigned b = vit_step(dl, A);
            bp[(int64_t) d.slot0 + (int64_t) i * 64 + j] = (uint8_t) b;
            // map: state at this window -> state before the lane's first window
            if (i == 0) map = b;
            else {
                unsigned nm = 0;
#pragma unroll
                for (int s = 0; s < 4; s++) nm |= vit_map_apply(map, vit_map_apply(b, (unsigned) s)) << (2 * s);
                map = nm;
            }
            const double m = fmax(fmax(dl[0], dl[1]), fmax(dl[2], dl[3]));
            if (dl[0] != dl[0] || dl[1] != dl[1] || dl[2] != dl[2] || dl[3] != dl[3]) bad |= HF_FLAG_NAN;
            else if (!(m > 0.0)) bad |= HF_FLAG_SCALE;
            e += vit_norm<4>(dl);
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
    maps[j] = (uint8_t) map;
    lmap[(int64_t) g * 64 + j] = (uint8_t) map;
    __syncthreads();
    if (j == 0) {   // segment map: exit state of the segment -> state before its first window
        const int na = (d.n + d.L - 1) / d.L;
        unsigned M = 0;
        for (int s = 0; s < 4; s++) {
            unsigned x = (unsigned) s;
            for (int q = na - 1; q >= 0; q--) x = vit_map_apply(maps[q], x);
            M |= x << (2 * s);
        }
        smap[g] = (uint8_t) M;
    }
    if (bad) atomicOr(flags, bad);
}

// ---- D: exit states, labels ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_vit_exits(int C, const int32_t* __restrict__ cseg0, const uint8_t* __restrict__ smap,
                                                  const int8_t* __restrict__ final_state, uint8_t* __restrict__ sexit) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    unsigned x = (unsigned) final_state[c];
    for (int g = cseg0[c + 1] - 1; g >= cseg0[c]; g--) {
        sexit[g] = (uint8_t) x;
        x = vit_map_apply(smap[g], x);
    }
}

__global__ void __launch_bounds__(64) k_vit_back(const SegDesc* __restrict__ segs, const uint8_t* __restrict__ bp,
                                                 const uint8_t* __restrict__ lmap, const uint8_t* __restrict__ sexit,
                                                 int8_t* __restrict__ label) {
    const int g = blockIdx.x, j = threadIdx.x;
    const SegDesc d = segs[g];
    __shared__ uint8_t maps[64], exits[64];
    maps[j] = lmap[(int64_t) g * 64 + j];
    __syncthreads();
    if (j == 0) {
        const int na = (d.n + d.L - 1) / d.L;
        unsigned x = sexit[g];
        for (int q = na - 1; q >= 0; q--) { exits[q] = (uint8_t) x; x = vit_map_apply(maps[q], x); }
    }
    __syncthreads();
    const int cnt = d.n - j * d.L < d.L ? d.n - j * d.L : d.L;
    if (cnt <= 0) return;
    unsigned s = exits[j];
    for (int i = cnt - 1; i >= 0; i--) {
        label[d.t0 + (int64_t) j * d.L + i] = (int8_t) s;
        s = vit_map_apply(bp[(int64_t) d.slot0 + (int64_t) i * 64 + j], s);
    }
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
        if (lane < n) {
            const int64_t t = t0 + base + lane;
#pragma unroll
            for (int k = 0; k < 8; k++) { const double2 v = rows[t * 8 + k]; As[lane][2 * k] = v.x; As[lane][2 * k + 1] = v.y; }
        }
        __syncthreads();
        if (lane == 0)
            for (int q = 0; q < n; q++) {
                bp[t0 + base + q] = (uint8_t) vit_step(dl, &As[q][0]);   // (lane 0 stores and later reads its own backpointers)
                const double m = fmax(fmax(dl[0], dl[1]), fmax(dl[2], dl[3]));
                if (dl[0] != dl[0] || dl[1] != dl[1] || dl[2] != dl[2] || dl[3] != dl[3]) bad |= HF_FLAG_NAN;
                else if (!(m > 0.0)) bad |= HF_FLAG_SCALE;
                e += vit_norm<4>(dl);
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
        s = vit_map_apply(bp[t], s);
    }
    if (bad) atomicOr(flags, bad);
}
