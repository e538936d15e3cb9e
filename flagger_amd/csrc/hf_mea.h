// hf_mea.h — maximum-expected-accuracy decoding under minimum run lengths (hf_get_mea_labels): among the labellings whose runs meet a
// minimum length per state, the one with the largest expected gain under the posterior of the last full pass.  To posterior argmax what
// hf_viterbi_minlen is to hf_viterbi; a getter of the last HF_MODE_FULL pass, as the range getters are (hf_view.h).
//
// Definition.  For a window t of a chunk, with f_t, b_t of the pass:
//   p_s        = f_t[s] * b_t[s]
//   gamma_t(s) = p_s / (((p_0 + p_1) + p_2) + p_3)                                  hf_get_posterior's value to rounding
//   g_t(k)     = ((gamma_t(0) W[0][k] + gamma_t(1) W[1][k]) + gamma_t(2) W[2][k]) + gamma_t(3) W[3][k]
// W[s * 4 + k]: the gain of calling k when the truth is s (the identity: the expected number of correctly labelled windows).  A BLOCK
// is a chunk, or a group of joined chunks as hf_viterbi_minlen_joined cuts them.  A labelling of a block is ADMISSIBLE by the family's
// rule (hf_minlen.h, the block's first and last run exempt) and SUPPORTED when gamma_t(l_t) > 0 at every window and
// A_t[l_{t-1}][l_t] > 0 at every window that is not the first of its chunk (a step across a joined boundary carries no condition: the
// two chains are independent).  The result per block: the admissible supported labelling of the largest sum over windows of g_t(l_t).
//
// It is the walk of hf_viterbi_minlen in (max, +) over GAIN ROWS in place of log rows, with an end column of zeros:
//   gk_t(k)    = g_t(k) if gamma_t(k) > 0, else -inf
//   G_t[p][k]  = gk_t(k)                                   a chunk-first window: the four rows alike, so the first window of a block
//                                                          (row 0 is read) and a joined boundary (an ordinary step) use the same row
//   G_t[p][k]  = gk_t(k) if A_t[p][k] > 0, else -inf       every other window
// k_mea_rows writes G_t in k_mlv_rows' window-order layout; k_mlv_fwd and k_mlv_back (hf_minlen.h) then run AS THEY ARE, one workgroup
// per block over the block offsets, with a parameter block of the getter's own whose trans[s][4] is 1.0 in every region: log(end) adds
// exactly 0.  Lanes, entry, in-between and saturated steps, the exclusion of p == s and every tie rule are hf_chain.h's.
// HF_FLAG_NAN: a NaN in a gain row (k_mea_rows; a window whose p_s sum to 0 gives one); HF_FLAG_SCALE: a block's maximum is -inf
// (k_mlv_fwd), no admissible supported labelling.
//
// k_mea_rows: one thread per window, both kinds of context through PassView (mo_fb, iv_row).  The HF_ALGO_SEQ view finds f and b by
// (chunk, window in chunk): the thread searches the chunk in the offsets, log2(C) loads that stay in the L2 (a grid row per chunk would
// bound the chunk count by the grid's second dimension and launch mostly empty blocks on a track of uneven chunks).
#pragma once
#include "hf_minlen.h"
#include "hf_view.h"

struct MeaGain { double w[16]; };      // [truth * 4 + called]

template <bool SEQ>
__global__ void __launch_bounds__(256) k_mea_rows(int64_t N, int C, const int64_t* __restrict__ off, PassView pv, MeaGain W,
                                                  double2* __restrict__ rows, unsigned* __restrict__ flags) {
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N || t < off[0] || t >= off[C]) return;       // (a window outside every chunk: no block reads its row)
    int c = 0;
    if constexpr (SEQ) {
        // the last chunk whose offset is <= t: the chunk of t, chunks without windows passed over
        int lo = 0, hi = C;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (off[mid] <= t) lo = mid; else hi = mid;
        }
        c = lo;
    }
    double f[4], b[4];
    mo_fb<SEQ>(pv, c, t, f, b);
    const double p0 = f[0] * b[0], p1 = f[1] * b[1], p2 = f[2] * b[2], p3 = f[3] * b[3];
    const double tot = ((p0 + p1) + p2) + p3;
    const double gm[4] = {p0 / tot, p1 / tot, p2 / tot, p3 / tot};
    double gk[4];
    bool nan = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double g = ((gm[0] * W.w[k] + gm[1] * W.w[4 + k]) + gm[2] * W.w[8 + k]) + gm[3] * W.w[12 + k];
        nan |= g != g;
        gk[k] = gm[k] > 0.0 ? g : HF_MLV_NEG_INF;
    }
    double G[16];
    if (REC_FIRST(pv.rec[t])) {
#pragma unroll
        for (int o = 0; o < 16; o++) G[o] = gk[o & 3];
    } else {
        double A[16];
        iv_row<SEQ>(pv, t, A);
#pragma unroll
        for (int o = 0; o < 16; o++) G[o] = A[o] > 0.0 ? gk[o & 3] : HF_MLV_NEG_INF;
    }
    double2* __restrict__ dst = rows + t * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = make_double2(G[2 * k], G[2 * k + 1]);
    if (nan) atomicOr(flags, HF_FLAG_NAN);
}
