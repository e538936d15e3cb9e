// hf_decode.h — the core both path decoders run: hf_viterbi (hf_viterbi.h, the most probable path, in the (max, x) semiring) and
// hf_sample_paths (hf_sample.h, posterior path samples, in the (+, x) semiring).  Neither is part of an EM pass: each runs with the
// parameters it is given, into buffers of its own.
//
// The chain.  For a chunk of T windows with parameters p (the same quantities a pass uses, hmm.c:333-420):
//   first[s]     = trans[r_0][4][s] * e_0[s]                      (start row x emission of the chunk's first window)
//   A_t[pre][s]  = T_t[pre][s] * e_t[pre][s],  t >= 1             (region change => 0.2, validity masks, alpha, beta: the rows of a pass)
//   end[s]       = trans[r_{T-1}][s][4]
//
// Rows.  k_dec_rows_* evaluate the emission row of every window directly (hf_emit_values, or the caller's negative-binomial table) and
// multiply it by the window's transition row (load_T): one 128-byte row A_t per window.  The chunk-first window's row holds first[s]
// in row pre = 0 and zeros elsewhere, so every chunk starts from the vector (1, 0, 0, 0).
//
// Numerics.  Vectors and matrices are renormalised after every product by 2^-e, e = the exponent of their largest entry: exact
// (unless an entry falls out of the normal range relative to the largest).  In (max, x) the exponents are summed, so the value carried
// is (mantissas, integer exponent sum) and a score is log(max) + e_sum * ln 2; (+, x) needs no score and carries none.
//
// MAPS.  A decoder's work per window is one byte {0..3} -> {0..3}, 2 bits per state: the state at t-1 given the state at t (Viterbi's
// first-max backpointers, a sample's draws).  A path is a final state pushed back through the bytes.
//
// HF_ALGO_SCAN: the segment plan of hf_create (SegDesc, hf_seg.h: segments of <= 64 x HF_SEG_LMAX windows, lane j owns windows
// j*L .. j*L+L-1 of its segment).  Rows and map bytes live in SLOT order (window w = j*L + i of a segment in slot slot0 + i*64 + j);
// a row is 8 pieces of 16 bytes stored piece-major inside a step, so the 64 lanes of a step read 1 KiB contiguous per instruction.
//   A  k_dec_prod    lane product Q_j = A_{jL} (x) ... (x) A_{jL+L-1}; inclusive scan over the 64 lanes (shuffles); every lane keeps
//                    the EXCLUSIVE prefix P_j, the segment its total S
//   B  k_dec_chain   per chunk, over its segments in order: v_0 = (1,0,0,0), v_{k+1} = v_k (x) S_k — the vector entering every segment
//   C  (the decoder's own replay) lane j enters with v_k (x) P_j (dec_enter) and writes a map byte per window; the lane's map (its exit
//                    state -> the state before its first window) is the composition of its bytes, the segment's the composition of its
//                    lanes' (dec_seg_maps); the lane that holds the chunk's last window picks the final state
//   D  k_dec_exits   per chunk, over its segments from the end: the exit state of every segment (integer maps: exact)
//      k_dec_back    every lane gets its exit state from the lane maps, walks its map bytes and writes the labels (window order)
//   D runs with a sample axis (blockIdx.y = sample k: maps[k][slot], labels[k][window]); Viterbi is the single sample k = 0.
// HF_ALGO_SEQ: rows in window order (k_dec_rows_win), then one wavefront per chunk (the decoder's own *_seq kernel): the on-device
// cross-check, as hf_seq.h is for the pass.
#pragma once
#include "hf_device.h"

// the two semirings: add(a, b) is the sum, x the ordinary product; `score`: the decoder reports a log-probability (exponent sums)
struct MaxTimes {
    static constexpr bool score = true;
    static __device__ __forceinline__ double add(double a, double b) { return fmax(a, b); }
};
struct SumTimes {
    static constexpr bool score = false;
    static __device__ __forceinline__ double add(double a, double b) { return a + b; }
};

// emission x transition row of window t (layout [pre*4 + s]); chunk-first: first[s] in row 0
__device__ __forceinline__ void dec_row(const uint32_t* __restrict__ rec, const double* __restrict__ beta, const DevParams* __restrict__ P,
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
__device__ __forceinline__ int dec_norm(double* v) {
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < N; k++) m = fmax(m, v[k]);
    if (!(m > 0.0) || isinf(m)) return 0;
    const int e = ilogb(m);
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = ldexp(v[k], -e);
    return e;
}

__device__ __forceinline__ void dec_ident(double* M) {
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

// C = A (x) B (sums left to right); C may alias neither
template <class SR>
__device__ __forceinline__ void dec_mm(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            double m = A[i * 4] * B[k];
#pragma unroll
            for (int j = 1; j < 4; j++) m = SR::add(m, A[i * 4 + j] * B[j * 4 + k]);
            C[i * 4 + k] = m;
        }
}

// out = v (x) M for a row vector
template <class SR>
__device__ __forceinline__ void dec_vm(const double v[4], const double* M, double out[4]) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
        double m = v[0] * M[s];
#pragma unroll
        for (int p = 1; p < 4; p++) m = SR::add(m, v[p] * M[p * 4 + s]);
        out[s] = m;
    }
}

// index (double2 units) of piece k of the row of step i, lane j of a segment whose first slot is slot0
__device__ __forceinline__ int64_t dec_slot_piece(int64_t slot0, int i, int k, int j) { return slot0 * 8 + ((int64_t) i * 8 + k) * 64 + j; }

__device__ __forceinline__ void dec_load_row(const double2* __restrict__ rows, int64_t slot0, int i, int j, double A[16]) {
#pragma unroll
    for (int k = 0; k < 8; k++) { const double2 v = rows[dec_slot_piece(slot0, i, k, j)]; A[2 * k] = v.x; A[2 * k + 1] = v.y; }
}

// HF_ALGO_SEQ: the row of window t (window order)
__device__ __forceinline__ void dec_load_row_win(const double2* __restrict__ rows, int64_t t, double* A) {
#pragma unroll
    for (int k = 0; k < 8; k++) { const double2 v = rows[t * 8 + k]; A[2 * k] = v.x; A[2 * k + 1] = v.y; }
}

// windows of lane j of a segment (<= 0: none)
__device__ __forceinline__ int dec_lane_count(const SegDesc& d, int j) { return d.n - j * d.L < d.L ? d.n - j * d.L : d.L; }

// ---- maps ----------------------------------------------------------------------------------------------------------------------
#define HF_DEC_MAP_IDENT 0xE4u   // 3 2 1 0
__device__ __forceinline__ unsigned dec_map_apply(unsigned map, unsigned s) { return (map >> (2 * s)) & 3u; }

// a lane's map one window further on: byte b of that window, then `map` (the state before the lane's first window)
__device__ __forceinline__ unsigned dec_map_then(unsigned map, unsigned b) {
    unsigned nm = 0;
#pragma unroll
    for (int s = 0; s < 4; s++) nm |= dec_map_apply(map, dec_map_apply(b, (unsigned) s)) << (2 * s);
    return nm;
}

// every lane's map to lmap[lane] and to `lm` (64 bytes of LDS), then lane 0's segment map (exit state of the segment -> state before
// its first window) to *smap; all 64 lanes of the segment's workgroup call it
__device__ __forceinline__ void dec_seg_maps(const SegDesc& d, int j, unsigned map, uint8_t* lm, uint8_t* __restrict__ lmap,
                                             uint8_t* __restrict__ smap) {
    lm[j] = (uint8_t) map;
    lmap[j] = (uint8_t) map;
    __syncthreads();
    if (j == 0) {
        const int na = (d.n + d.L - 1) / d.L;
        unsigned M = 0;
        for (int s = 0; s < 4; s++) {
            unsigned x = (unsigned) s;
            for (int q = na - 1; q >= 0; q--) x = dec_map_apply(lm[q], x);
            M |= x << (2 * s);
        }
        *smap = (uint8_t) M;
    }
}

// ---- rows ----------------------------------------------------------------------------------------------------------------------
// HF_ALGO_SCAN: one workgroup of 64 per segment, slot-ordered pieces
#ifndef HF_HELPERS_ONLY   // (the plain kernels of this file: compiled by the unit that owns them alone, hf_host.h)
__global__ void __launch_bounds__(64) k_dec_rows_seg(const SegDesc* __restrict__ segs, const uint32_t* __restrict__ rec,
                                                     const double* __restrict__ beta, const DevParams* __restrict__ P,
                                                     const double* __restrict__ nbE, double2* __restrict__ rows, unsigned* __restrict__ flags) {
    const SegDesc d = segs[blockIdx.x];
    const int j = threadIdx.x;
    unsigned nan = 0;
    for (int i = 0; i < d.L; i++) {
        const int x = j * d.L + i;
        if (x >= d.n) break;
        double a[16];
        dec_row(rec, beta, P, nbE, d.t0 + x, a, &nan);
#pragma unroll
        for (int k = 0; k < 8; k++) rows[dec_slot_piece(d.slot0, i, k, j)] = make_double2(a[2 * k], a[2 * k + 1]);
    }
    if (nan) atomicOr(flags, nan);
}
#endif

// HF_ALGO_SEQ: one thread per window, window order.  LOG: the log of every entry (-inf for 0), k_mlv_rows of hf_minlen.h
template <bool LOG>
__device__ __forceinline__ void dec_rows_win(int64_t N, const uint32_t* __restrict__ rec, const double* __restrict__ beta,
                                             const DevParams* __restrict__ P, const double* __restrict__ nbE, double2* __restrict__ rows,
                                             unsigned* __restrict__ flags) {
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    unsigned nan = 0;
    double a[16];
    dec_row(rec, beta, P, nbE, t, a, &nan);
    if (LOG) {
#pragma unroll
        for (int k = 0; k < 16; k++) a[k] = a[k] == 0.0 ? -__builtin_huge_val() : log(a[k]);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) rows[t * 8 + k] = make_double2(a[2 * k], a[2 * k + 1]);
    if (nan) atomicOr(flags, nan);
}
#ifndef HF_HELPERS_ONLY
__global__ void __launch_bounds__(256) k_dec_rows_win(int64_t N, const uint32_t* __restrict__ rec, const double* __restrict__ beta,
                                                      const DevParams* __restrict__ P, const double* __restrict__ nbE,
                                                      double2* __restrict__ rows, unsigned* __restrict__ flags) {
    dec_rows_win<false>(N, rec, beta, P, nbE, rows, flags);
}
#endif

// ---- A: lane products and their exclusive scan over the lanes --------------------------------------------------------------------
// P[seg][k][lane] (16 doubles, k-major: coalesced), S[seg][16]; with a score also PE[seg][lane], SE[seg]
template <class SR>
__global__ void __launch_bounds__(64) k_dec_prod(const SegDesc* __restrict__ segs, const double2* __restrict__ rows,
                                                 double* __restrict__ Pm, int* __restrict__ PE, double* __restrict__ S, int* __restrict__ SE) {
    const int g = blockIdx.x, j = threadIdx.x;
    const SegDesc d = segs[g];
    double Q[16];
    int e = 0;
    dec_ident(Q);
    for (int i = 0; i < d.L; i++) {
        if (j * d.L + i >= d.n) break;
        double A[16], Nq[16];
        dec_load_row(rows, d.slot0, i, j, A);
        dec_mm<SR>(Q, A, Nq);
        e += dec_norm<16>(Nq);
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
            dec_mm<SR>(L, Q, Nq);
            e += le + dec_norm<16>(Nq);
#pragma unroll
            for (int k = 0; k < 16; k++) Q[k] = Nq[k];
        }
    }
    // exclusive: lane j takes lane j-1's inclusive product, lane 0 the identity
    double X[16];
#pragma unroll
    for (int k = 0; k < 16; k++) X[k] = __shfl_up(Q[k], 1, 64);
    int xe = __shfl_up(e, 1, 64);
    if (j == 0) { dec_ident(X); xe = 0; }
#pragma unroll
    for (int k = 0; k < 16; k++) Pm[((int64_t) g * 16 + k) * 64 + j] = X[k];
    if constexpr (SR::score) PE[(int64_t) g * 64 + j] = xe;
    if (j == 63) {
#pragma unroll
        for (int k = 0; k < 16; k++) S[(int64_t) g * 16 + k] = Q[k];
        if constexpr (SR::score) SE[g] = e;
    }
}

// ---- B: the vector entering every segment (vin[seg][4]; with a score vinE[seg]), one thread per chunk ----------------------------
template <class SR>
__global__ void __launch_bounds__(64) k_dec_chain(int C, const int32_t* __restrict__ cseg0, const double* __restrict__ S,
                                                  const int* __restrict__ SE, double* __restrict__ vin, long long* __restrict__ vinE) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double v[4] = {1.0, 0.0, 0.0, 0.0};
    long long e = 0;
    for (int g = cseg0[c]; g < cseg0[c + 1]; g++) {
#pragma unroll
        for (int s = 0; s < 4; s++) vin[(int64_t) g * 4 + s] = v[s];
        double nv[4];
        dec_vm<SR>(v, S + (int64_t) g * 16, nv);
        const int en = dec_norm<4>(nv);
        if constexpr (SR::score) { vinE[g] = e; e += SE[g] + en; }
#pragma unroll
        for (int s = 0; s < 4; s++) v[s] = nv[s];
    }
}

// ---- C: lane j of segment g enters with vin[g] (x) P_j, normalised (dl); returns the exponent taken out --------------------------
template <class SR>
__device__ __forceinline__ int dec_enter(const double* __restrict__ vin, const double* __restrict__ Pm, int g, int j, double dl[4]) {
    double v[4], X[16];
#pragma unroll
    for (int s = 0; s < 4; s++) v[s] = vin[(int64_t) g * 4 + s];
#pragma unroll
    for (int k = 0; k < 16; k++) X[k] = Pm[((int64_t) g * 16 + k) * 64 + j];
    dec_vm<SR>(v, X, dl);
    return dec_norm<4>(dl);
}

// ---- D: exit states (sexit[k][seg]), labels (label[k][window]); blockIdx.y = sample k ------------------------------------------------
#ifndef HF_HELPERS_ONLY
__global__ void __launch_bounds__(64) k_dec_exits(int C, int G, const int32_t* __restrict__ cseg0, const uint8_t* __restrict__ smap,
                                                  const int8_t* __restrict__ final_state, uint8_t* __restrict__ sexit) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (c >= C) return;
    const uint8_t* __restrict__ sm = smap + (int64_t) k * G;
    uint8_t* __restrict__ se = sexit + (int64_t) k * G;
    unsigned x = (unsigned) final_state[(int64_t) k * C + c];
    for (int g = cseg0[c + 1] - 1; g >= cseg0[c]; g--) {
        se[g] = (uint8_t) x;
        x = dec_map_apply(sm[g], x);
    }
}

__global__ void __launch_bounds__(64) k_dec_back(const SegDesc* __restrict__ segs, const uint8_t* __restrict__ maps, int64_t n_slots, int G,
                                                 int64_t N, const uint8_t* __restrict__ lmap, const uint8_t* __restrict__ sexit,
                                                 int8_t* __restrict__ label) {
    const int g = blockIdx.x, j = threadIdx.x, k = blockIdx.y;
    const SegDesc d = segs[g];
    __shared__ uint8_t lm[64], exits[64];
    lm[j] = lmap[((int64_t) k * G + g) * 64 + j];
    __syncthreads();
    if (j == 0) {
        const int na = (d.n + d.L - 1) / d.L;
        unsigned x = sexit[(int64_t) k * G + g];
        for (int q = na - 1; q >= 0; q--) { exits[q] = (uint8_t) x; x = dec_map_apply(lm[q], x); }
    }
    __syncthreads();
    const int cnt = dec_lane_count(d, j);
    if (cnt <= 0) return;
    const uint8_t* __restrict__ mk = maps + (int64_t) k * n_slots;
    int8_t* __restrict__ lk = label + (int64_t) k * N;
    unsigned s = exits[j];
    for (int i = cnt - 1; i >= 0; i--) {
        lk[d.t0 + (int64_t) j * d.L + i] = (int8_t) s;
        s = dec_map_apply(mk[(int64_t) d.slot0 + (int64_t) i * 64 + j], s);
    }
}
#endif
