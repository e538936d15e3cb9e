// hf_alpha.h — the alpha statistics of a pass (hf_get_alpha_stats): per region r and entry alpha[p][s], the exact derivative G of the
// pass's log-likelihood in that entry and the curvature H of the expected complete-data log-likelihood.  Not part of an EM pass: it reads
// the pass's rows, forward and backward vectors and parameter block and writes buffers of its own only.
//
// Definition (gaussian and trunc_exp_gaussian).  For a pair of windows (t-1, t) of one chunk, t >= 1 (the pair (0, 1) INCLUDED), with
// r the region of window t, x / x_prev the 8-bit coverage of t / t-1, beta = beta_t:
//   xi[p][s] = f_{t-1}[p] * A_t[p][s] * b_t[s] / HF_TERMINATION_PROB
// f, b the pass's scaled forward and backward vectors (hf_get_forward_backward) and A_t the row the pass multiplied by (hf_view.h
// iv_row).  For a Gaussian state s and component c, with a = alpha[p][s]:
//   v_c = var_c * beta,  d_c = x - ((1 - a) mu_c + a x_prev) beta,  u_c = beta (x_prev - mu_c)
//   P_c = w_c / sqrt(2 PI v_c) exp(-d_c^2 / (2 v_c)) floored at 1e-40 (phi_c = 0 where the floor was taken, else 1), g_c = P_c / sum_c P_c
//   G[r][p][s] = sum_t xi[p][s] sum_c g_c phi_c d_c u_c / v_c        H[r][p][s] = sum_t xi[p][s] sum_c g_c phi_c u_c^2 / v_c
// Err under trunc_exp_gaussian has no alpha: G = H = 0.
//
// TERMS.  T[p][s] = sum_c g_c phi_c d_c u_c / v_c and U[p][s] = sum_c g_c phi_c u_c^2 / v_c depend on (region, x, x_prev, beta) alone: on the
// emission row, not on the window.
//   HF_ALGO_SCAN  k_alpha_terms evaluates them once per row of A of the pass — row j of Pass::d_lutA is job j of the track's job list
//                 (hf_scan.h TableJob: region, x, x_prev, and beta_star for a table row / the window's own beta for a private row) —
//                 and k_alpha_pairs<false> reads the 32 values of window t's row (Track::d_arow) beside the row itself: the exps
//                 run once per row, not once per window (12 us against 285 us at BASELINE configs[2]).
//   HF_ALGO_SEQ   k_alpha_pairs<true> evaluates them per window from the window records and d_beta: the on-device cross-check.
// The pair counts xi come per window in both: HF_ALGO_SCAN from the pair records of all windows (what the lazy re-run of the getters
// leaves: b_t in the record at pos[t], f_{t-1} in the one at pos_f[t-1]) — in either statistics mode, and with the pair (0, 1) of every
// chunk like any other pair — HF_ALGO_SEQ from the tiles of k_fwd_seq / k_bwd_seq.
//
// PLAN, built by the first call of a context (hf_getters.h alpha_plan): the pairs of all chunks sorted by the region of window t and, inside
// a region, HF_ALGO_SCAN by the position of t's pair record (the statistics plan keeps the records of one row of A together, so a
// wavefront reads contiguous records and few rows), HF_ALGO_SEQ by t; cut into blocks of at most HF_AL_BLOCK pairs of ONE region.
//   k_alpha_pairs  one workgroup of 256 lanes per block: lane l takes pairs l, l + 256, ... of the block in that order (32 accumulators in
//                  registers; the division of xi by the termination probability is taken once, on the block's sum), then a fixed shuffle
//                  tree over the 64 lanes of every wavefront and the four wavefronts in order.  Out: part[block][32] (G then H, [p * 4 + s]).
//   k_alpha_sum    one workgroup of 1024 lanes per region: lane (j, k) adds part[b][k] of the region's blocks b = j, j + 32, ... in
//                  order, then j = 0..31 in order.  Out: out[r][32].
// The order of every addition is fixed by the plan: a run is reproducible bit for bit.
#pragma once
#include "hf_view.h"

#define HF_AL_THREADS 256
#define HF_AL_BLOCK (4 * HF_AL_THREADS)      // pairs per block at most (measured at configs[2]: 16 per lane 148 us, 4 per lane 105 us, 2 per lane 116 us)
#define HF_AL_SUM_THREADS 1024

struct AlBlock { long long p0; int n, r; };          // pairs p0 .. p0 + n - 1 of the sorted pair list, all of region r

// out[p * 4 + s] = T[p][s], out[16 + p * 4 + s] = U[p][s] of one emission row.  What does not depend on the previous state (v_c, the
// normalisation, u_c) is formed once per component; 1 / v_c is a reciprocal here where the emission divides (a rounding's difference).
__device__ __forceinline__ void alpha_terms(const DevParams* __restrict__ P, const DevRegion* __restrict__ R, double x, double px, double bt,
                                            double out[32]) {
    const bool te = hf_err_is_truncexp(P);
#pragma unroll
    for (int s = 0; s < 4; s++) {
        double tot[4] = {0.0, 0.0, 0.0, 0.0}, g[4] = {0.0, 0.0, 0.0, 0.0}, h[4] = {0.0, 0.0, 0.0, 0.0};
        const int nc = (s == 0 && te) ? 0 : P->ncomp[s];
        for (int c = 0; c < nc; c++) {
            const double mu = R->mean[s][c];
            const double var = R->var[s][c] * bt;
            const double norm = R->weight[s][c] / (sqrt(var * 2 * HF_PI));
            const double iv = 1.0 / var;
            const double u = bt * (px - mu), uiv = u * iv, uuiv = u * uiv;
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const double al = P->alpha[p * 4 + s];
                double mean = (1 - al) * mu + al * px;
                mean *= bt;
                const double d = x - mean;
                double pc = norm * hf_emit_exp(-0.5 * (d * d) * iv);
                if (pc < 1e-40) pc = 1e-40;          // phi_c = 0: the floor does not depend on alpha
                else { g[p] += pc * (d * uiv); h[p] += pc * uuiv; }
                tot[p] += pc;
            }
        }
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const double rt = nc > 0 ? 1.0 / tot[p] : 0.0;
            out[p * 4 + s] = g[p] * rt;
            out[16 + p * 4 + s] = h[p] * rt;
        }
    }
}

// HF_ALGO_SCAN: the terms of every row of A (job j = row j; chunk-first rows belong to no pair: zeros)
__global__ void __launch_bounds__(256) k_alpha_terms(int n_jobs, const TableJob* __restrict__ jobs, const DevParams* __restrict__ P,
                                                     double* __restrict__ terms) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_jobs) return;
    const TableJob J = jobs[j];
    double out[32];
    if (J.flags & 2) {
#pragma unroll
        for (int k = 0; k < 32; k++) out[k] = 0.0;
    } else alpha_terms(P, &P->reg[J.r], J.x, J.px, J.bt, out);
    double2* __restrict__ dst = reinterpret_cast<double2*>(terms) + (int64_t) j * 16;
#pragma unroll
    for (int k = 0; k < 16; k++) dst[k] = make_double2(out[2 * k], out[2 * k + 1]);
}

// f_{t-1} (mo_f) and b_t (mo_b) of a pair, and its row A_t: hf_view.h
template <bool SEQ>
__global__ void __launch_bounds__(HF_AL_THREADS) k_alpha_pairs(const AlBlock* __restrict__ blocks, const long long* __restrict__ pair_t,
                                                               const int32_t* __restrict__ pair_c, const double* __restrict__ beta,
                                                               const double* __restrict__ terms, PassView pv, double* __restrict__ part) {
    const AlBlock bk = blocks[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; k++) acc[k] = 0.0;
#pragma unroll 1
    for (int i = tid; i < bk.n; i += HF_AL_THREADS) {
        const int64_t t = pair_t[bk.p0 + i];
        double A[16], f[4], b[4], tm[32];
        iv_row<SEQ>(pv, t, A);
        int c = 0;                                   // (the chunk of the pair: the tiles of HF_ALGO_SEQ only)
        if constexpr (SEQ) {
            const uint32_t r1 = pv.rec[t], r0 = pv.rec[t - 1];
            alpha_terms(pv.Pm, &pv.Pm->reg[bk.r], (double) REC_X(r1), (double) REC_X(r0), beta[t], tm);
            c = pair_c[bk.p0 + i];
        } else {
            const double2* __restrict__ src = reinterpret_cast<const double2*>(terms) + (int64_t) ((uint32_t) pv.arow[t] & 0x7fffffffu) * 16;
#pragma unroll
            for (int k = 0; k < 16; k++) { const double2 v = src[k]; tm[2 * k] = v.x; tm[2 * k + 1] = v.y; }
        }
        mo_f<SEQ>(pv, c, t - 1, f);
        mo_b<SEQ>(pv, c, t, b);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const double w = f[k >> 2] * A[k] * b[k & 3];          // xi without its division by the termination probability: taken once, below
            acc[k] += w * tm[k];
            acc[16 + k] += w * tm[16 + k];
        }
    }
    __shared__ double red[4][32];
#pragma unroll
    for (int k = 0; k < 32; k++) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid < 32) part[(int64_t) blockIdx.x * 32 + tid] = (((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]) / HF_TERMINATION_PROB;
}

// rblk0[r] .. rblk0[r + 1] - 1: the blocks of region r
__global__ void __launch_bounds__(HF_AL_SUM_THREADS) k_alpha_sum(const int32_t* __restrict__ rblk0, const double* __restrict__ part,
                                                                 double* __restrict__ out) {
    const int r = blockIdx.x, k = threadIdx.x & 31, j = threadIdx.x >> 5;
    const int b0 = rblk0[r], b1 = rblk0[r + 1];
    double v = 0.0;
    constexpr int ST = HF_AL_SUM_THREADS / 32;
    int b = b0 + j;
    for (; b + 7 * ST < b1; b += 8 * ST) {   // 8 loads in flight, the adds stay in block order
        double xk[8];
#pragma unroll
        for (int q = 0; q < 8; q++) xk[q] = part[(int64_t) (b + q * ST) * 32 + k];
#pragma unroll
        for (int q = 0; q < 8; q++) v += xk[q];
    }
    for (; b < b1; b += ST) v += part[(int64_t) b * 32 + k];
    __shared__ double red[HF_AL_SUM_THREADS / 32][32];
    red[j][k] = v;
    __syncthreads();
    if (j == 0) {
        double s = red[0][k];
        for (int q = 1; q < HF_AL_SUM_THREADS / 32; q++) s += red[q][k];
        out[(int64_t) r * 32 + k] = s;
    }
}
