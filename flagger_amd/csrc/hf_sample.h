// hf_sample.h — exact draws of whole state paths from P(path | data) for every chunk: forward filtering in the (+, x) semiring, backward
// sampling.  Not part of an EM pass: hf_sample_paths runs it with the parameters it is given, into buffers of its own.
//
// Definition.  For a chunk of T windows with parameters p, the quantities hf_viterbi uses (hf_viterbi.h):
//   first[s] = trans[r_0][4][s] * e_0[s],  A_t = the row a pass builds (t >= 1),  end[s] = trans[r_{T-1}][s][4]
// A sample is a path s_0 .. s_{T-1} drawn with probability proportional to first[s_0] * prod_{t>=1} A_t[s_{t-1}][s_t] * end[s_{T-1}]
// (the distribution whose marginals hf_get_posterior returns).
//
// Uniforms (counter-based: a draw depends on (seed, sample index, window index) alone, not on the algorithm, the segment plan or how
// samples are grouped into calls):  splitmix64(x) = the standard finaliser of x + 0x9E3779B97F4A7C15,
//   key_k  = splitmix64(seed ^ splitmix64(k))        k = absolute sample index
//   u(k,i) = (splitmix64(key_k + i) >> 11) * 2^-53   i = global window index t for window t's draw, n_windows + c for chunk c's final state
// Draw rule (device, sequential kernel and the numpy reference alike).  Window t >= 1 of a chunk, target state s: w_p = alpha_{t-1}[p] *
// A_t[p][s], c_0 = w_0, c_p = c_{p-1} + w_p (left to right), x = u * c_3; the state before is the smallest p with x < c_p, else the largest
// p with w_p > 0, else 0.  The final state: the same rule with w_s = alpha_{T-1}[s] * end[s].  alpha may carry any power-of-two scale.
// The chunk-first window's row holds first[s] in row 0 and the forward vector entering a chunk is (1, 0, 0, 0), so its draw is always 0.
//
// A window's draw for every target state is one MAP BYTE {0..3} -> {0..3} (2 bits per state, the layout of Viterbi's backpointers):
// the state at t-1 given the state at t.  A sample's path is the final state pushed back through the maps.
//
// HF_ALGO_SCAN (the segment plan of hf_create, Viterbi's slot layout; rows from k_vit_rows_seg into the sampler's own buffer):
//   A  k_smp_prod    lane products Q_j in (+, x), renormalised by powers of two; inclusive scan over the 64 lanes; each lane keeps the
//                    exclusive prefix P_j, the segment its total S
//   B  k_smp_chain   per chunk: the (+, x) vector entering every segment
//   C  k_smp_replay  lane j enters with v (x) P_j and walks its windows once: per window the 16 weights and 4 cumulative sums, then per
//                    sample one uniform and one map byte (maps[k][slot]); the lane that holds the chunk's last window draws the final
//                    state of every sample
//      k_smp_maps    (blockIdx.y = sample) every lane composes its bytes into its lane map, lane 0 the lane maps into the segment map
//   D  k_smp_exits, k_smp_back   Viterbi's D step with a sample axis (blockIdx.y): labels[k][window]
// HF_ALGO_SEQ: k_smp_seq, one wavefront per chunk in window order (lane 0 runs the forward recurrence 64 staged windows at a time, the
// wavefront draws the bytes of every sample, then every lane backtracks samples of its own): the on-device cross-check.
// Flags: HF_FLAG_NAN on a NaN in a forward vector or the final weights (a NaN in a row or in the end column ends up there),
// HF_FLAG_SCALE when a chunk's forward vector or final weights are all 0 — in a flag word of the sampler's own.
#pragma once
#include "hf_viterbi.h"

__host__ __device__ __forceinline__ uint64_t hf_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t hf_sample_key(uint64_t seed, uint64_t k) { return hf_splitmix64(seed ^ hf_splitmix64(k)); }
__device__ __forceinline__ double smp_uniform(uint64_t key, uint64_t i) { return (double) (hf_splitmix64(key + i) >> 11) * 0x1.0p-53; }

// the draw rule: w[p] weights, c[p] their left-to-right cumulative sums
__device__ __forceinline__ unsigned smp_pick(const double w[4], const double c[4], double u) {
    const double x = u * c[3];
    if (x < c[0]) return 0;
    if (x < c[1]) return 1;
    if (x < c[2]) return 2;
    if (x < c[3]) return 3;
    for (int p = 3; p >= 0; p--) if (w[p] > 0.0) return (unsigned) p;
    return 0;
}

// one window: W[s*4+p] = d[p] * A[p][s], Cm[s*4+p] their cumulative sums over p; d <- (Cm[s*4+3])_s (the forward vector at this window)
__device__ __forceinline__ void smp_weights(double d[4], const double A[16], double W[16], double Cm[16]) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
        double c = 0.0;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const double w = d[p] * A[p * 4 + s];
            c = p == 0 ? w : c + w;
            W[s * 4 + p] = w;
            Cm[s * 4 + p] = c;
        }
    }
#pragma unroll
    for (int s = 0; s < 4; s++) d[s] = Cm[s * 4 + 3];
}

// the map byte of one window for one uniform
__device__ __forceinline__ unsigned smp_byte(const double W[16], const double Cm[16], double u) {
    unsigned b = 0;
#pragma unroll
    for (int s = 0; s < 4; s++) b |= smp_pick(&W[s * 4], &Cm[s * 4], u) << (2 * s);
    return b;
}

__device__ __forceinline__ unsigned smp_check(const double d[4]) {
    if (d[0] != d[0] || d[1] != d[1] || d[2] != d[2] || d[3] != d[3]) return HF_FLAG_NAN;
    return (d[0] > 0.0 || d[1] > 0.0 || d[2] > 0.0 || d[3] > 0.0) ? 0u : HF_FLAG_SCALE;
}

// final weights of a chunk (w_s = d[s] * end[s]) and their cumulative sums
__device__ __forceinline__ unsigned smp_final_weights(const DevParams* __restrict__ P, uint32_t rec_last, const double d[4], double w[4], double c[4]) {
    const DevRegion* __restrict__ Rl = &P->reg[REC_REGION(rec_last)];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        w[s] = d[s] * Rl->trans[s][4];
        c[s] = s == 0 ? w[s] : c[s - 1] + w[s];
    }
    return smp_check(w);
}

// C = A (x) B in the (+, x) semiring (sums left to right); C may alias neither
__device__ __forceinline__ void smp_mm(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            double m = A[i * 4] * B[k];
#pragma unroll
            for (int j = 1; j < 4; j++) m = m + A[i * 4 + j] * B[j * 4 + k];
            C[i * 4 + k] = m;
        }
}

// v (x) M for a row vector
__device__ __forceinline__ void smp_vm(const double v[4], const double* M, double out[4]) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
        double m = v[0] * M[s];
#pragma unroll
        for (int p = 1; p < 4; p++) m = m + v[p] * M[p * 4 + s];
        out[s] = m;
    }
}

// ---- A: lane products and their exclusive scan over the lanes (P[seg][k][lane], S[seg][16]) -------------------------------------------
__global__ void __launch_bounds__(64) k_smp_prod(const SegDesc* __restrict__ segs, const double2* __restrict__ rows,
                                                 double* __restrict__ Pm, double* __restrict__ S) {
    const int g = blockIdx.x, j = threadIdx.x;
    const SegDesc d = segs[g];
    double Q[16];
    vit_ident(Q);
    for (int i = 0; i < d.L; i++) {
        if (j * d.L + i >= d.n) break;
        double A[16], Nq[16];
        vit_load_row(rows, d.slot0, i, j, A);
        smp_mm(Q, A, Nq);
        vit_norm<16>(Nq);
#pragma unroll
        for (int k = 0; k < 16; k++) Q[k] = Nq[k];
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        double L[16];
#pragma unroll
        for (int k = 0; k < 16; k++) L[k] = __shfl_up(Q[k], off, 64);
        if (j >= off) {
            double Nq[16];
            smp_mm(L, Q, Nq);
            vit_norm<16>(Nq);
#pragma unroll
            for (int k = 0; k < 16; k++) Q[k] = Nq[k];
        }
    }
    double X[16];
#pragma unroll
    for (int k = 0; k < 16; k++) X[k] = __shfl_up(Q[k], 1, 64);
    if (j == 0) vit_ident(X);
#pragma unroll
    for (int k = 0; k < 16; k++) Pm[((int64_t) g * 16 + k) * 64 + j] = X[k];
    if (j == 63) {
#pragma unroll
        for (int k = 0; k < 16; k++) S[(int64_t) g * 16 + k] = Q[k];
    }
}

// ---- B: the vector entering every segment, one thread per chunk ------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_smp_chain(int C, const int32_t* __restrict__ cseg0, const double* __restrict__ S,
                                                  double* __restrict__ vin) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double v[4] = {1.0, 0.0, 0.0, 0.0};
    for (int g = cseg0[c]; g < cseg0[c + 1]; g++) {
#pragma unroll
        for (int s = 0; s < 4; s++) vin[(int64_t) g * 4 + s] = v[s];
        double nv[4];
        smp_vm(v, S + (int64_t) g * 16, nv);
        vit_norm<4>(nv);
#pragma unroll
        for (int s = 0; s < 4; s++) v[s] = nv[s];
    }
}

// ---- C: replay: map bytes of every sample (maps[k][slot]), final states (final[k][chunk]) ----------------------------------------------
__global__ void __launch_bounds__(64) k_smp_replay(const SegDesc* __restrict__ segs, const uint32_t* __restrict__ rec,
                                                   const DevParams* __restrict__ P, const double2* __restrict__ rows,
                                                   const double* __restrict__ Pm, const double* __restrict__ vin,
                                                   const uint64_t* __restrict__ keys, int n_samples, int64_t N, int C, int64_t n_slots,
                                                   uint8_t* __restrict__ maps, int8_t* __restrict__ final_state, unsigned* __restrict__ flags) {
    const int g = blockIdx.x, j = threadIdx.x;
    const SegDesc d = segs[g];
    const int cnt = d.n - j * d.L < d.L ? d.n - j * d.L : d.L;
    if (cnt <= 0) return;
    unsigned bad = 0;
    double v[4], X[16], dl[4];
#pragma unroll
    for (int s = 0; s < 4; s++) v[s] = vin[(int64_t) g * 4 + s];
#pragma unroll
    for (int k = 0; k < 16; k++) X[k] = Pm[((int64_t) g * 16 + k) * 64 + j];
    smp_vm(v, X, dl);
    vit_norm<4>(dl);
    for (int i = 0; i < cnt; i++) {
        double A[16], W[16], Cm[16];
        vit_load_row(rows, d.slot0, i, j, A);
        smp_weights(dl, A, W, Cm);   // (sample-independent: once per window)
        const uint64_t t = (uint64_t) (d.t0 + (int64_t) j * d.L + i);
        const int64_t slot = (int64_t) d.slot0 + (int64_t) i * 64 + j;
        for (int k = 0; k < n_samples; k++) maps[(int64_t) k * n_slots + slot] = (uint8_t) smp_byte(W, Cm, smp_uniform(keys[k], t));
        bad |= smp_check(dl);
        vit_norm<4>(dl);
    }
    if (j * d.L + cnt == d.n && d.k == d.nseg - 1) {   // the chunk's last window: final states
        double w[4], c[4];
        bad |= smp_final_weights(P, rec[d.t0 + d.n - 1], dl, w, c);
        for (int k = 0; k < n_samples; k++)
            final_state[(int64_t) k * C + d.chunk] = (int8_t) smp_pick(w, c, smp_uniform(keys[k], (uint64_t) N + (uint64_t) d.chunk));
    }
    if (bad) atomicOr(flags, bad);
}

// lane maps (lmap[k][seg][lane]: the lane's exit state -> the state before its first window) and segment maps (smap[k][seg]);
// blockIdx.y = sample
__global__ void __launch_bounds__(64) k_smp_maps(const SegDesc* __restrict__ segs, const uint8_t* __restrict__ maps, int64_t n_slots, int G,
                                                 uint8_t* __restrict__ lmap, uint8_t* __restrict__ smap) {
    const int g = blockIdx.x, j = threadIdx.x, k = blockIdx.y;
    const SegDesc d = segs[g];
    const uint8_t* __restrict__ mk = maps + (int64_t) k * n_slots;
    __shared__ uint8_t lm[64];
    const int cnt = d.n - j * d.L < d.L ? d.n - j * d.L : d.L;
    unsigned map = HF_VIT_MAP_IDENT;
    for (int i = 0; i < cnt; i++) {
        const unsigned b = mk[(int64_t) d.slot0 + (int64_t) i * 64 + j];
        if (i == 0) map = b;
        else {
            unsigned nm = 0;
#pragma unroll
            for (int s = 0; s < 4; s++) nm |= vit_map_apply(map, vit_map_apply(b, (unsigned) s)) << (2 * s);
            map = nm;
        }
    }
    lm[j] = (uint8_t) map;
    lmap[((int64_t) k * G + g) * 64 + j] = (uint8_t) map;
    __syncthreads();
    if (j == 0) {
        const int na = (d.n + d.L - 1) / d.L;
        unsigned M = 0;
        for (int s = 0; s < 4; s++) {
            unsigned x = (unsigned) s;
            for (int q = na - 1; q >= 0; q--) x = vit_map_apply(lm[q], x);
            M |= x << (2 * s);
        }
        smap[(int64_t) k * G + g] = (uint8_t) M;
    }
}

// ---- D: exit states (sexit[k][seg]), labels (label[k][window]); blockIdx.y = sample ------------------------------------------------------
__global__ void __launch_bounds__(64) k_smp_exits(int C, int G, const int32_t* __restrict__ cseg0, const uint8_t* __restrict__ smap,
                                                  const int8_t* __restrict__ final_state, uint8_t* __restrict__ sexit) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (c >= C) return;
    const uint8_t* __restrict__ sm = smap + (int64_t) k * G;
    uint8_t* __restrict__ se = sexit + (int64_t) k * G;
    unsigned x = (unsigned) final_state[(int64_t) k * C + c];
    for (int g = cseg0[c + 1] - 1; g >= cseg0[c]; g--) {
        se[g] = (uint8_t) x;
        x = vit_map_apply(sm[g], x);
    }
}

__global__ void __launch_bounds__(64) k_smp_back(const SegDesc* __restrict__ segs, const uint8_t* __restrict__ maps, int64_t n_slots, int G,
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
        for (int q = na - 1; q >= 0; q--) { exits[q] = (uint8_t) x; x = vit_map_apply(lm[q], x); }
    }
    __syncthreads();
    const int cnt = d.n - j * d.L < d.L ? d.n - j * d.L : d.L;
    if (cnt <= 0) return;
    const uint8_t* __restrict__ mk = maps + (int64_t) k * n_slots;
    int8_t* __restrict__ lk = label + (int64_t) k * N;
    unsigned s = exits[j];
    for (int i = cnt - 1; i >= 0; i--) {
        lk[d.t0 + (int64_t) j * d.L + i] = (int8_t) s;
        s = vit_map_apply(mk[(int64_t) d.slot0 + (int64_t) i * 64 + j], s);
    }
}

// ---- HF_ALGO_SEQ: one wavefront per chunk, window order; maps[k][window] -------------------------------------------------------------
__global__ void __launch_bounds__(64) k_smp_seq(const int64_t* __restrict__ off, const uint32_t* __restrict__ rec,
                                                const DevParams* __restrict__ P, const double2* __restrict__ rows,
                                                const uint64_t* __restrict__ keys, int n_samples, int64_t N, int C,
                                                uint8_t* __restrict__ maps, int8_t* __restrict__ label, unsigned* __restrict__ flags) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int64_t t0 = off[c], T = off[c + 1] - t0;
    __shared__ double As[64][17];
    __shared__ double Ws[64][16], Cs[64][16];
    __shared__ double fw[4], fc[4];
    if (T <= 0) return;
    double dl[4] = {1.0, 0.0, 0.0, 0.0};
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
                smp_weights(dl, &As[q][0], &Ws[q][0], &Cs[q][0]);
                bad |= smp_check(dl);
                vit_norm<4>(dl);
            }
        __syncthreads();
        for (int64_t x = lane; x < (int64_t) n_samples * n; x += 64) {
            const int k = (int) (x / n), q = (int) (x % n);
            const uint64_t t = (uint64_t) (t0 + base + q);
            maps[(int64_t) k * N + (int64_t) t] = (uint8_t) smp_byte(&Ws[q][0], &Cs[q][0], smp_uniform(keys[k], t));
        }
        __syncthreads();
    }
    if (lane == 0) {
        double w[4], cc[4];
        bad |= smp_final_weights(P, rec[t0 + T - 1], dl, w, cc);
        for (int s = 0; s < 4; s++) { fw[s] = w[s]; fc[s] = cc[s]; }
        if (bad) atomicOr(flags, bad);
    }
    __syncthreads();
    double w[4], cc[4];
    for (int s = 0; s < 4; s++) { w[s] = fw[s]; cc[s] = fc[s]; }
    for (int k = lane; k < n_samples; k += 64) {
        const uint8_t* __restrict__ mk = maps + (int64_t) k * N;
        int8_t* __restrict__ lk = label + (int64_t) k * N;
        unsigned s = smp_pick(w, cc, smp_uniform(keys[k], (uint64_t) N + (uint64_t) c));
        for (int64_t t = t0 + T - 1; t >= t0; t--) {
            lk[t] = (int8_t) s;
            s = vit_map_apply(mk[t], s);
        }
    }
}
