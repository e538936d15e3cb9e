// hf_entropy.h — exact path entropy and labelling log-probability (hf_get_path_entropy, hf_get_path_log_probs, hf_get_entropy_profile):
// for a window range, the Shannon entropy (nats) of the posterior distribution over the label paths of the range and the log-probability
// of one given labelling of it, under the model of the last HF_MODE_FULL pass.  Not part of an EM pass: it reads the pass's rows, forward
// and backward vectors and writes buffers of its own only.
//
// Definition.  Given the data, the label path of a chunk is an inhomogeneous Markov chain: P(s_t = s | s_{t-1} = p, data) is the pair
// posterior of (t-1, t) over its row marginal.  With f, b the pass's scaled vectors and A_t the row the pass multiplied by (iv_row), for a
// window t that is not the first of its chunk
//   x_t[p][s] = (f_{t-1}[p] A_t[p][s]) b_t[s],   m_t[p] = sum_s x_t[p][s] (state order),   Z_t = sum_p m_t[p]
//   cond_t    = - sum_p sum_s (x_t[p][s] / Z_t) log(x_t[p][s] / m_t[p])                     (x = 0 contributes 0)
// x <= m_p in floating point too (m_p is a sum of non-negatives that contains x): every term is >= 0, nothing is clamped, no difference
// of large numbers appears.  For any window
//   gamma_t[s] = f_t[s] b_t[s] / sum_s f_t[s] b_t[s]  (as mo_centre forms it),   marg_t = - sum_s gamma_t[s] log gamma_t[s]
// A job's chunk-local part [a, b]:
//   entropy(part)     = marg_a + sum_{t=a+1..b} cond_t                                       (the chain rule: exact)
//   log_prob(part; y) = log gamma_a[y_a] + sum_{t=a+1..b} log(x_t[y_{t-1}][y_t] / m_t[y_{t-1}])   (-inf as soon as one factor is 0)
//
// PIECES, as hf_runs.h cuts them: the interior windows (a, b] of every part at global window indices that are multiples of HF_EN_PIECE.
// Every window of a piece has its predecessor inside the part, so f_{t-1} (and y_{t-1}) is a plain read.
//   k_ent_piece    one 64-lane workgroup per piece: lane j takes windows t0 + j*HF_EN_LANE .. + HF_EN_LANE - 1 and adds their terms in
//                  window order (a lane without windows: 0.0; it reads f_{t-1} once and keeps the f_t it has just loaded), then the
//                  fixed-shape pairwise reduction of k_mo_piece (level k: lane j, j % 2^(k+1) == 0, adds lane j + 2^k).  LABELS: the
//                  term is the one log(x / m) of the labelled pair; it is <= 0 or -inf, so -inf propagates and no +inf can arise.
//   k_ent_chain    one thread per part: the first window's term (marg_a, or log gamma_a[y_a]) plus the part's piece sums in order.
//   k_ent_profile  one thread per window: marg_t and / or cond_t (cond_t := marg_t at a chunk-first window).
// The parts of a job are summed on the host in chunk order.  Nothing depends on the other jobs of a call.
#pragma once
#include "hf_view.h"
#include "hf_runs.h"

#define HF_EN_LANE 8                      // windows per lane of a piece
#define HF_EN_PIECE (64 * HF_EN_LANE)     // windows per piece at most; pieces are cut at global indices that are multiples of this

struct EnPiece { long long t0; int n, c; };           // windows t0 .. t0 + n - 1 of chunk c (t0 - 1 lies in the same part)
struct EnPart { long long a; int p0, p1, c, pad; };   // the first window a of a chunk-local part of chunk c, its pieces p0 .. p1 - 1

// x_t[p][s] and its row sums: fp = f_{t-1}, A = A_t, b = b_t
__device__ __forceinline__ void en_pair(const double fp[4], const double A[16], const double b[4], double x[16], double m[4]) {
#pragma unroll
    for (int p = 0; p < 4; p++) {
#pragma unroll
        for (int s = 0; s < 4; s++) x[p * 4 + s] = (fp[p] * A[p * 4 + s]) * b[s];
        m[p] = ((x[p * 4] + x[p * 4 + 1]) + x[p * 4 + 2]) + x[p * 4 + 3];
    }
}

// cond_t of the pair (t-1, t)
__device__ __forceinline__ double en_cond(const double fp[4], const double A[16], const double b[4]) {
    double x[16], m[4];
    en_pair(fp, A, b, x, m);
    const double Z = ((m[0] + m[1]) + m[2]) + m[3];
    double h = 0.0;
    if (!(Z > 0.0)) return h;                // (no weight left by the pass)
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const double v = x[k];
        if (v > 0.0) h += (v / Z) * -log(v / m[k >> 2]);
    }
    return h;
}

// log(x_t[yp][ys] / m_t[yp])
__device__ __forceinline__ double en_pair_log(const double fp[4], const double A[16], const double b[4], int yp, int ys) {
    double x[16], m[4];
    en_pair(fp, A, b, x, m);
    double v = x[0], mp = m[0];
#pragma unroll
    for (int k = 1; k < 16; k++) v = (k == yp * 4 + ys) ? x[k] : v;
#pragma unroll
    for (int p = 1; p < 4; p++) mp = (p == yp) ? m[p] : mp;
    return v > 0.0 ? log(v / mp) : -__builtin_inf();      // (a zero m makes the factor 0: x <= m)
}

// gamma_t as mo_centre forms it
__device__ __forceinline__ void en_gamma(const double f[4], const double b[4], double g[4]) {
#pragma unroll
    for (int s = 0; s < 4; s++) g[s] = f[s] * b[s];
    double tot = g[0];
#pragma unroll
    for (int s = 1; s < 4; s++) tot += g[s];
#pragma unroll
    for (int s = 0; s < 4; s++) g[s] = g[s] / tot;
}

__device__ __forceinline__ double en_marg(const double f[4], const double b[4]) {
    double g[4], h = 0.0;
    en_gamma(f, b, g);
#pragma unroll
    for (int s = 0; s < 4; s++)
        if (g[s] > 0.0) h += g[s] * -log(g[s]);
    return h;
}

__device__ __forceinline__ double en_gamma_log(const double f[4], const double b[4], int y) {
    double g[4];
    en_gamma(f, b, g);
    double v = g[0];
#pragma unroll
    for (int s = 1; s < 4; s++) v = (s == y) ? g[s] : v;
    return v > 0.0 ? log(v) : -__builtin_inf();
}

// out[g] = the piece's sum of cond_t (LABELS: of log(x_t[y_{t-1}][y_t] / m_t[y_{t-1}]); lab is indexed by t - lab0)
template <bool SEQ, bool LABELS>
__global__ void __launch_bounds__(64) k_ent_piece(const EnPiece* __restrict__ pieces, PassView pv, const int8_t* __restrict__ lab, long long lab0,
                                                  double* __restrict__ out) {
    const EnPiece pc = pieces[blockIdx.x];
    const int j = threadIdx.x;
    double m = 0.0;
    if (j * HF_EN_LANE < pc.n) {
        double fp[4], b[4];
        mo_fb<SEQ>(pv, pc.c, pc.t0 + j * HF_EN_LANE - 1, fp, b);      // f of the lane's first predecessor
        int yp = 0;
        if constexpr (LABELS) yp = lab[pc.t0 + j * HF_EN_LANE - 1 - lab0];
#pragma unroll 1
        for (int i = 0; i < HF_EN_LANE; i++) {
            const int x = j * HF_EN_LANE + i;
            if (x >= pc.n) break;
            const int64_t t = pc.t0 + x;
            double A[16], f[4];
            iv_row<SEQ>(pv, t, A);
            mo_fb<SEQ>(pv, pc.c, t, f, b);
            if constexpr (LABELS) {
                const int ys = lab[t - lab0];
                m += en_pair_log(fp, A, b, yp, ys);
                yp = ys;
            } else {
                m += en_cond(fp, A, b);
            }
#pragma unroll
            for (int s = 0; s < 4; s++) fp[s] = f[s];
        }
    }
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        const double qm = __shfl_down(m, off, 64);
        if ((j & (2 * off - 1)) == 0) m += qm;
    }
    if (j == 0) out[blockIdx.x] = m;
}

// one thread per part: out[i] = the first window's term + the part's piece sums in order
template <bool SEQ, bool LABELS>
__global__ void __launch_bounds__(64) k_ent_chain(int n_parts, const EnPart* __restrict__ parts, const double* __restrict__ px, PassView pv,
                                                  const int8_t* __restrict__ lab, long long lab0, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_parts) return;
    const EnPart pt = parts[i];
    double f[4], b[4];
    mo_fb<SEQ>(pv, pt.c, pt.a, f, b);
    double v;
    if constexpr (LABELS) v = en_gamma_log(f, b, lab[pt.a - lab0]);
    else v = en_marg(f, b);
    for (int g = pt.p0; g < pt.p1; g++) v += px[g];
    out[i] = v;
}

// one thread per window first + i, i < n: marg[i] and / or cond[i] (either may be NULL).  off: the C + 1 chunk offsets.
template <bool SEQ>
__global__ void __launch_bounds__(256) k_ent_profile(long long first, long long n, const int64_t* __restrict__ off, int C, PassView pv,
                                                     double* __restrict__ marg, double* __restrict__ cond) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t t = first + i;
    int lo = 0, hi = C;                       // the chunk of t: off[lo] <= t < off[lo + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= t) lo = mid; else hi = mid;
    }
    double f[4], b[4];
    mo_fb<SEQ>(pv, lo, t, f, b);
    const bool chunk_first = t == off[lo];
    if (marg || chunk_first) {
        const double h = en_marg(f, b);
        if (marg) marg[i] = h;
        if (cond && chunk_first) cond[i] = h;
    }
    if (cond && !chunk_first) {
        double fp[4], bp[4], A[16];
        mo_fb<SEQ>(pv, lo, t - 1, fp, bp);
        iv_row<SEQ>(pv, t, A);
        cond[i] = en_cond(fp, A, b);
    }
}
