// hf_minlen_sample.h — whole paths drawn from the posterior under minimum run lengths (hf_sample_paths_minlen): backward sampling over
// the expanded chain of hf_chain.h.  The third of the minimum-run-length family: hf_viterbi_minlen leaves the best admissible path,
// hf_minlen_posterior the per-window marginals given admissibility, this the admissible paths themselves, each with probability
// weight(path) / Z_adm.  A decoder beside the other two: the same first, A_t and end, buffers of its own, ONE code path for both kinds of
// context (linear rows in window order, k_dec_rows_win; the forward lanes of k_mlp_fwd, launched with grid (C, 1)).
//
// Definition (include/hmm_flagger_hip.h has it in full), m_s = min_len[s], F_t the forward vector of hf_minlen_post.h, u = u(k, i) of
// hf_sample.h (i the global window index for the draw of window t, n_windows + c for chunk c's final lane):
//   the draw rule over n candidates   weights w_0..w_{n-1}, c_0 = w_0, c_i = c_{i-1} + w_i, x = u * c_{n-1}: the smallest i with
//                                     x < c_i, else the largest i with w_i > 0, else 0 (smp_pick of hf_sample.h for n = 4)
//   the final lane of a chunk         all lanes in lane order, w_l = F_{T-1}[l] * end[s(l)]; the cumulative sums strictly left to right
//   the lane at t-1 given (s, d) at t >= 1
//     d = 1            four slots p, w_p = F_{t-1}[(p, m_p)] * A_t[p][s], w_s replaced by 0 when m_s > 1: to (p, m_p)
//     1 < d < m_s      (s, d-1), no draw
//     d = m_s > 1      two slots, w_0 = F_{t-1}[(s, m_s-1)] * A_t[s][s] ("arrived"), w_1 = F_{t-1}[(s, m_s)] * A_t[s][s] ("stayed")
// SCALING BEFORE THE PRODUCTS.  k_mlp_fwd keeps the largest lane of a window between exponent 300 and, eight floored rows later, 2e-270;
// the eight values a window's draws read (the four saturated lanes and the four lanes below them) are therefore scaled by 2^-e first,
// e = ilogb of the largest of the eight (0 when that is 0 or not finite), and the final weights' lanes by their largest lane: no
// product of a lane that matters falls into the subnormals, and a power of two changes no comparison.
//
// k_mls_draw   window-parallel, one thread per window (lanes = consecutive windows): the eight scaled values, the 16 + 8 weights and
//              their cumulative sums ONCE, then per sample one uniform and one 16-bit word in k_mlv_fwd's format (bits 2s, 2s+1 the
//              predecessor state of state s's entry lane, bit 8+s set when state s's saturated lane stayed).  A word holds the draw of
//              every lane the path could be in; the walk uses the one it is in, as the map bytes of hf_sample.h do for four states.
//              Words are stored sample-minor, [window][Kp], Kp the call's samples padded to HF_MLS_GROUP: a thread writes eight
//              samples per 16-byte store and the walk reads one line per window.  It reads F at a stride of sum(min_len) doubles (eight
//              of a window's lanes).  It raises no flag: the words of chunk-first windows are not written, those of windows outside
//              every chunk are formed from whatever F holds there, and neither is ever read.
// k_mls_final  one 64-lane workgroup per chunk: the weights, their scale, lane 0 their left-to-right sums, then lane j the final lanes
//              of samples j, j + 64, ... into final[chunk][Kp].
// k_mls_back   grid (C, Kp / 64), LANE = SAMPLE: per window the wavefront loads 64 words (one line) and every lane steps its own (s, d)
//              by k_mlv_back's rule in vector registers, no readlane per window; the words of the next 16 windows are in flight while
//              these are stepped.  Labels: four windows per dword into an LDS tile [sample][window] (64 x 64 bytes, rows padded to 17
//              dwords), then sample after sample the wavefront writes that sample's 64 consecutive labels.
// hf_sample_paths_minlen_joined (hf_minlen_post_joined.h) launches k_mls_draw, k_mls_final and k_mls_back unchanged, the last two over
// the group-as-chunk offsets, and fills in the words of the joined chunk-first windows with k_mlsj_bound, which forms its weights by
// k_mls_draw's operations: a change to the draw rule or to the scaling before the products goes into both.
#pragma once
#include "hf_chain.h"
#include "hf_sample.h"

#define HF_MLS_GROUP 64         // samples of one walk (a wavefront); a call's samples are padded to a multiple of it

// the draw rule over two slots
__device__ __forceinline__ unsigned mls_pick2(double w1, double c0, double c1, double u) {
    const double x = u * c1;
    if (x < c0) return 0;
    if (x < c1) return 1;
    return w1 > 0.0 ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_mls_draw(int64_t N, const uint32_t* __restrict__ rec, const double2* __restrict__ rows, int m0, int m1,
                                                  int m2, int m3, const double* __restrict__ F, const uint64_t* __restrict__ keys, int K, int Kp,
                                                  uint16_t* __restrict__ words) {
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    if (t == 0 || REC_FIRST(rec[t])) return;            // (no window before it: its word is never read)
    HF_CHAIN_LENS(m0, m1, m2, m3);
    const double* __restrict__ Fp = F + (t - 1) * total;
    // the four saturated lanes of window t-1 and the lanes below them, scaled by the largest of the eight
    double fs[4], fb[4];
    fs[0] = Fp[sat0]; fs[1] = Fp[sat1]; fs[2] = Fp[sat2]; fs[3] = Fp[sat3];
    fb[0] = m0 > 1 ? Fp[sat0 - 1] : 0.0; fb[1] = m1 > 1 ? Fp[sat1 - 1] : 0.0;
    fb[2] = m2 > 1 ? Fp[sat2 - 1] : 0.0; fb[3] = m3 > 1 ? Fp[sat3 - 1] : 0.0;
    double mx = 0.0;
#pragma unroll
    for (int p = 0; p < 4; p++) mx = fmax(mx, fmax(fs[p], fb[p]));
    const int e = (mx > 0.0 && !isinf(mx)) ? ilogb(mx) : 0;
#pragma unroll
    for (int p = 0; p < 4; p++) { fs[p] = ldexp(fs[p], -e); fb[p] = ldexp(fb[p], -e); }
    double A[16];
    dec_load_row_win(rows, t, A);
    // entry lanes: W[s*4+p], Cm[s*4+p] as smp_weights forms them, without the excluded p == s
    double W[16], Cm[16];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const bool excl = ch_len(mpack, s) > 1;
        double c = 0.0;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const double w = (excl && p == s) ? 0.0 : fs[p] * A[p * 4 + s];
            c = p == 0 ? w : c + w;
            W[s * 4 + p] = w;
            Cm[s * 4 + p] = c;
        }
    }
    // saturated lanes: arrived, stayed
    double w1[4], c0[4], c1[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        c0[s] = fb[s] * A[5 * s];
        w1[s] = fs[s] * A[5 * s];
        c1[s] = c0[s] + w1[s];
    }
    const unsigned smask = (m0 > 1 ? 1u : 0u) | (m1 > 1 ? 2u : 0u) | (m2 > 1 ? 4u : 0u) | (m3 > 1 ? 8u : 0u);
    uint4* __restrict__ out = reinterpret_cast<uint4*>(words + t * Kp);     // (Kp a multiple of 64: 16-byte aligned)
    for (int k8 = 0; k8 < K; k8 += 8) {
        unsigned h[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int k = k8 + j;
            if (k < K) {
                const double u = smp_uniform(keys[k], (uint64_t) t);
                unsigned w = smp_byte(W, Cm, u);
#pragma unroll
                for (int s = 0; s < 4; s++) w |= mls_pick2(w1[s], c0[s], c1[s], u) << (8 + s);
                h[j >> 1] |= (w & (0xffu | smask << 8)) << (16 * (j & 1));
            }
        }
        out[k8 >> 3] = make_uint4(h[0], h[1], h[2], h[3]);
    }
}

// final[chunk][Kp]: the lane of the chunk's last window, per sample
__global__ void __launch_bounds__(64) k_mls_final(int64_t N, const int64_t* __restrict__ off, const uint32_t* __restrict__ rec,
                                                  const DevParams* __restrict__ P, int m0, int m1, int m2, int m3, const double* __restrict__ F,
                                                  const uint64_t* __restrict__ keys, int K, int Kp, uint8_t* __restrict__ final_lane) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int64_t t0 = off[c], T = off[c + 1] - t0;
    __shared__ double ws[64], cs[64];
    if (T <= 0) return;
    HF_CHAIN_LENS(m0, m1, m2, m3);
    const int s = (lane >= b1) + (lane >= b2) + (lane >= b3);
    const bool active = lane < total;
    (void) mpack;
    const DevRegion* __restrict__ Rl = &P->reg[REC_REGION(rec[t0 + T - 1])];
    const double x = active ? F[(t0 + T - 1) * total + lane] : 0.0;
    const double end = active ? Rl->trans[s][4] : 0.0;
    ws[lane] = ldexp(x, -ch_shift(ch_wave_max(x), 0)) * end;
    __syncthreads();
    if (lane == 0) {
        double a = 0.0;
        for (int i = 0; i < total; i++) { a = i == 0 ? ws[0] : a + ws[i]; cs[i] = a; }
    }
    __syncthreads();
    for (int k = lane; k < K; k += 64) {
        const double xk = smp_uniform(keys[k], (uint64_t) N + (uint64_t) c) * cs[total - 1];
        int pick = -1;
        for (int i = 0; i < total && pick < 0; i++) if (xk < cs[i]) pick = i;
        for (int i = total - 1; i >= 0 && pick < 0; i--) if (ws[i] > 0.0) pick = i;
        final_lane[(int64_t) c * Kp + k] = (uint8_t) (pick < 0 ? 0 : pick);
    }
}

// the walk back, lane = sample blockIdx.y * 64 + lane: label[sample][window]
__global__ void __launch_bounds__(64) k_mls_back(int64_t N, const int64_t* __restrict__ off, int m0, int m1, int m2, int m3,
                                                 const uint16_t* __restrict__ words, const uint8_t* __restrict__ final_lane, int K, int Kp,
                                                 int8_t* __restrict__ label) {
    const int c = blockIdx.x, lane = threadIdx.x, k0 = blockIdx.y * HF_MLS_GROUP, k = k0 + lane;
    const int64_t t0 = off[c], T = off[c + 1] - t0;
    __shared__ unsigned tile[64][17];                   // [sample][window / 4], 17: the rows start in different banks
    if (T <= 0) return;
    HF_CHAIN_LENS(m0, m1, m2, m3);
    const bool live = k < K;
    const int fl = live ? (int) final_lane[(int64_t) c * Kp + k] : 0;
    int cs = (fl >= b1) + (fl >= b2) + (fl >= b3);
    int cd = fl - (cs == 0 ? 0 : cs == 1 ? b1 : cs == 2 ? b2 : b3) + 1;
    const uint16_t* __restrict__ wk = words + (live ? k : 0);
    // the words of 16 windows downwards from window `top` of the chunk (0 for the chunk's first window and below it)
    auto load16 = [&](int64_t top, unsigned w[16]) {
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = (live && top - j >= 1) ? (unsigned) wk[(t0 + top - j) * Kp] : 0u;
    };
    unsigned nx[16];
    load16(T - 1, nx);
    const int nk = K - k0 < HF_MLS_GROUP ? K - k0 : HF_MLS_GROUP;
    for (int64_t hi = T - 1; hi >= 0; hi -= 64) {
        const int n = (int) (hi + 1 < 64 ? hi + 1 : 64);
        unsigned acc = 0;
        for (int q0 = 0; q0 < n; q0 += 16) {
            unsigned w[16];
#pragma unroll
            for (int j = 0; j < 16; j++) w[j] = nx[j];
            load16(hi - q0 - 16, nx);                   // (the next 16, across the block boundary as well)
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int q = q0 + j;
                if (q < n) {
                    acc = acc << 8 | (unsigned) cs;
                    ch_step_back(mpack, w[j], cs, cd);
                    if ((q & 3) == 3) tile[lane][(63 - q) >> 2] = acc;
                }
            }
        }
        if (n & 3) tile[lane][(64 - n) >> 2] = acc << (8 * (4 - (n & 3)));
        __syncthreads();
        // window hi - 63 + lane of sample k0 + i
        if (lane >= 64 - n) {
            for (int i = 0; i < nk; i++)
                label[(int64_t) (k0 + i) * N + t0 + hi - 63 + lane] = (int8_t) ((tile[i][lane >> 2] >> (8 * (lane & 3))) & 0xffu);
        }
        __syncthreads();
    }
}
