// hf_sample.h — exact draws of whole state paths from P(path | data) for every chunk: forward filtering in the (+, x) semiring, backward
// sampling.  Not part of an EM pass: hf_sample_paths runs it with the parameters it is given, into buffers of its own.
//
// Definition.  With first, A_t and end of hf_decode.h, for a chunk of T windows:
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
// A window's draw for every target state is one map byte of hf_decode.h (the state at t-1 given the state at t); a sample's path is
// its final state pushed back through its maps.
//
// HF_ALGO_SCAN: rows, A, B and D of hf_decode.h in the (+, x) semiring (no exponent sums: the draws are scale-free), into the sampler's
// own buffers, D with a sample axis (blockIdx.y), and
//   C  k_smp_replay  lane j enters with v (x) P_j and walks its windows once: per window the 16 weights and 4 cumulative sums, then per
//                    sample one uniform and one map byte (maps[k][slot]); the lane that holds the chunk's last window draws the final
//                    state of every sample
//      k_smp_maps    (blockIdx.y = sample) every lane composes its bytes into its lane map, lane 0 the lane maps into the segment map
// HF_ALGO_SEQ: k_smp_seq, one wavefront per chunk in window order (lane 0 runs the forward recurrence 64 staged windows at a time, the
// wavefront draws the bytes of every sample, then every lane backtracks samples of its own): the on-device cross-check.
// Flags: HF_FLAG_NAN on a NaN in a forward vector or the final weights (a NaN in a row or in the end column ends up there),
// HF_FLAG_SCALE when a chunk's forward vector or final weights are all 0 — in a flag word of the sampler's own.
#pragma once
#include "hf_decode.h"

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

// ---- C: replay: map bytes of every sample (maps[k][slot]), final states (final[k][chunk]) ----------------------------------------------
#ifndef HF_HELPERS_ONLY   // (plain kernels, to the end of the file: compiled by the unit that owns them alone, hf_host.h)
__global__ void __launch_bounds__(64) k_smp_replay(const SegDesc* __restrict__ segs, const uint32_t* __restrict__ rec,
                                                   const DevParams* __restrict__ P, const double2* __restrict__ rows,
                                                   const double* __restrict__ Pm, const double* __restrict__ vin,
                                                   const uint64_t* __restrict__ keys, int n_samples, int64_t N, int C, int64_t n_slots,
                                                   uint8_t* __restrict__ maps, int8_t* __restrict__ final_state, unsigned* __restrict__ flags) {
    const int g = blockIdx.x, j = threadIdx.x;
    const SegDesc d = segs[g];
    const int cnt = dec_lane_count(d, j);
    if (cnt <= 0) return;
    unsigned bad = 0;
    double dl[4];
    dec_enter<SumTimes>(vin, Pm, g, j, dl);
    for (int i = 0; i < cnt; i++) {
        double A[16], W[16], Cm[16];
        dec_load_row(rows, d.slot0, i, j, A);
        smp_weights(dl, A, W, Cm);   // (sample-independent: once per window)
        const uint64_t t = (uint64_t) (d.t0 + (int64_t) j * d.L + i);
        const int64_t slot = (int64_t) d.slot0 + (int64_t) i * 64 + j;
        for (int k = 0; k < n_samples; k++) maps[(int64_t) k * n_slots + slot] = (uint8_t) smp_byte(W, Cm, smp_uniform(keys[k], t));
        bad |= smp_check(dl);
        dec_norm<4>(dl);
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
    const int cnt = dec_lane_count(d, j);
    unsigned map = HF_DEC_MAP_IDENT;
    for (int i = 0; i < cnt; i++) {
        const unsigned b = mk[(int64_t) d.slot0 + (int64_t) i * 64 + j];
        map = i == 0 ? b : dec_map_then(map, b);
    }
    dec_seg_maps(d, j, map, lm, lmap + ((int64_t) k * G + g) * 64, smap + (int64_t) k * G + g);
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
        if (lane < n) dec_load_row_win(rows, t0 + base + lane, &As[lane][0]);
        __syncthreads();
        if (lane == 0)
            for (int q = 0; q < n; q++) {
                smp_weights(dl, &As[q][0], &Ws[q][0], &Cs[q][0]);
                bad |= smp_check(dl);
                dec_norm<4>(dl);
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
            s = dec_map_apply(mk[t], s);
        }
    }
}
#endif
