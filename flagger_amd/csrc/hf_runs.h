// hf_runs.h — exact mean and variance of block counts (hf_get_run_moments): for a window range and a state set S, the posterior mean and
// variance of the number of maximal runs of S under the model of the last HF_MODE_FULL pass.  Not part of an EM pass: it reads the pass's
// rows, forward and backward vectors and writes buffers of its own only.
//
// Definition.  A job's chunk-local part [a, b]:
//   R  = 1[s_a in S] + sum_{t=a+1..b} 1[s_{t-1} not in S, s_t in S]      (runs of S that start inside the part)
//   S0 = 1[s_a in S],  E0 = 1[s_b in S]
// R is a sum over PAIRS of windows, so the jet of hf_moments.h takes a pair tilt in place of its column tilt.  Centred as there:
//   d_a[s]     = 1_S[s] - gamma_a(S)                                      (the first window; gamma as mo_centre forms it)
//   D_t[p][s]  = J[p][s] - xi_t,  J[p][s] = 1[p not in S] 1[s in S]        (window t > a)
//   xi_t       = sum_{p not in S, s in S} f_{t-1}[p] A_t[p][s] b_t[s] / sum_{p, s} f_{t-1}[p] A_t[p][s] b_t[s]
// (both sums of xi_t run over p, then s, the numerator by a select: S = all four states has J = 0, xi_t = 0 and D_t = 0 exactly).
//   (v, v', v'') = (f_a, f_a o d_a, f_a o d_a^2)
//   t = a+1..b:  v'' <- v''A_t + 2 v'(A_t o D_t) + v(A_t o D_t^2),  v' <- v'A_t + v(A_t o D_t),  v <- vA_t
//   L = v.b_b, L' = v'.b_b, L'' = v''.b_b
//   E[R] = gamma_a(S) + sum_t xi_t (summed in the fixed order below, not taken from L'/L),  Var(R) = L''/L - (L'/L)^2
// and, with (u, u') = (f_a o 1_S, f_a o 1_S o d_a) through the same factors (u' <- u'A_t + u(A_t o D_t), u <- uA_t), s = gamma_a(S),
// e = gamma_b(S):
//   Cov(R, E0)  = v'.(b_b o 1_S)/L - (L'/L) e
//   Cov(R, S0)  = u'.b_b/L - (L'/L) s
//   Cov(S0, E0) = u.(b_b o 1_S)/L - s e
// THE STEP.  J^2 = J, so with G_t = diag(1_notS) A_t diag(1_S) (the entries of A_t that start a run)
//   A_t o D_t = G_t - xi_t A_t,   A_t o D_t^2 = (1 - 2 xi_t) G_t + xi_t^2 A_t
// and one window on the right of (P, P', P'') costs five 4x4 products, two of them with the masked G_t (X = P A, X1 = P' A, X2 = P'' A,
// Y = P G, Y1 = P' G):
//   P'' <- X2 + 2 (Y1 - xi X1) + (1 - 2 xi) Y + xi^2 X,   P' <- X1 + (Y - xi X),   P <- X
// A stretch of windows is again a triple with the product rule of hf_moments.h (mo_mul), which the lanes' reduction and the chain reuse.
//
// PIECES, as hf_moments.h cuts them: the interior windows (a, b] of every part at global window indices that are multiples of
// HF_RN_PIECE.  Every window of a piece has its predecessor inside the part, so f_{t-1} is a plain read.
//   k_run_piece  one 64-lane workgroup per piece: lane j takes windows t0 + j*HF_RN_LANE .. + HF_RN_LANE - 1 in order (a lane without
//                windows: the identity (I, 0, 0)), then the fixed-shape pairwise reduction of k_mo_piece; the lanes' sums of xi_t take
//                the same tree.  Every product is renormalised by 2^-e, shared by the three matrices (mo_norm).
//   k_run_chain  one thread per part: (v, v', v'') and (u, u') from window a through the part's pieces in order, all five by the 2^-e of
//                v, then the dot products.  Out: the seven numbers E[R], Var(R), s, e, Cov(R, E0), Cov(R, S0), Cov(S0, E0).
// The parts of a job are stitched on the host (hf_get_run_moments in hf_getters.h), left to right.  Nothing depends on the other jobs of
// a call.  S = all four states: d_a = 0 and D_t = 0 exactly, so Var(R) = 0.0 and every covariance is 0.0, E[R] = 1.0, s = e = 1.0.
#pragma once
#include "hf_view.h"
#include "hf_moments.h"

#define HF_RN_LANE 8                      // windows per lane of a piece
#define HF_RN_PIECE (64 * HF_RN_LANE)     // windows per piece at most; pieces are cut at global indices that are multiples of this
#define HF_RN_OUT 7                       // numbers per part

struct RnPiece { long long t0; int n, mask, c; };            // windows t0 .. t0 + n - 1 of chunk c (t0 - 1 lies in the same part)
struct RnPart { long long a, b; int p0, p1, mask, c; };      // chunk-local part [a, b] of chunk c, its pieces p0 .. p1 - 1

// xi_t of the pair (t-1, t): fp = f_{t-1}, A = A_t, b = b_t
__device__ __forceinline__ double rn_xi(const double fp[4], const double A[16], const double b[4], int mask) {
    double tot = 0.0, in = 0.0;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const bool out_p = !((mask >> p) & 1);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const double x = (fp[p] * A[p * 4 + s]) * b[s];
            tot += x;
            in += (out_p && ((mask >> s) & 1)) ? x : 0.0;
        }
    }
    return tot > 0.0 ? in / tot : 0.0;      // (no weight left by the pass: no tilt)
}

// (P, P1, P2) <- (P, P1, P2) (A, A o D, A o D^2), D = J - xi: one window on the right
__device__ __forceinline__ void rn_step(double P[16], double P1[16], double P2[16], const double A[16], int mask, double xi) {
    double G[16], X[16], Y[16];
#pragma unroll
    for (int k = 0; k < 16; k++) G[k] = (!((mask >> (k >> 2)) & 1) && ((mask >> (k & 3)) & 1)) ? A[k] : 0.0;
    const double c1 = 1.0 - 2.0 * xi, c2 = xi * xi;
    dec_mm<SumTimes>(P2, A, X);
#pragma unroll
    for (int k = 0; k < 16; k++) P2[k] = X[k];
    dec_mm<SumTimes>(P1, A, X);
    dec_mm<SumTimes>(P1, G, Y);
#pragma unroll
    for (int k = 0; k < 16; k++) { P2[k] += 2.0 * (Y[k] - xi * X[k]); P1[k] = X[k]; }
    dec_mm<SumTimes>(P, A, X);
    dec_mm<SumTimes>(P, G, Y);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        P2[k] = (P2[k] + c1 * Y[k]) + c2 * X[k];
        P1[k] += Y[k] - xi * X[k];
        P[k] = X[k];
    }
    mo_norm<16>(P, P1, P2);
}

// out[g][0..15] = P, [16..31] = P', [32..47] = P''; outx[g] = the piece's sum of xi_t
template <bool SEQ>
__global__ void __launch_bounds__(64) k_run_piece(const RnPiece* __restrict__ pieces, PassView pv, double* __restrict__ out,
                                                  double* __restrict__ outx) {
    const RnPiece pc = pieces[blockIdx.x];
    const int j = threadIdx.x;
    double P[16], P1[16], P2[16], m = 0.0;
    dec_ident(P);
#pragma unroll
    for (int k = 0; k < 16; k++) { P1[k] = 0.0; P2[k] = 0.0; }
    if (j * HF_RN_LANE < pc.n) {
        double fp[4], b[4];
        mo_fb<SEQ>(pv, pc.c, pc.t0 + j * HF_RN_LANE - 1, fp, b);      // f of the lane's first predecessor
#pragma unroll 1
        for (int i = 0; i < HF_RN_LANE; i++) {
            const int x = j * HF_RN_LANE + i;
            if (x >= pc.n) break;
            const int64_t t = pc.t0 + x;
            double A[16], f[4];
            iv_row<SEQ>(pv, t, A);
            mo_fb<SEQ>(pv, pc.c, t, f, b);
            const double xi = rn_xi(fp, A, b, pc.mask);
            m += xi;
            rn_step(P, P1, P2, A, pc.mask, xi);
#pragma unroll
            for (int s = 0; s < 4; s++) fp[s] = f[s];
        }
    }
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        double Q[16], Q1[16], Q2[16];
#pragma unroll
        for (int k = 0; k < 16; k++) { Q[k] = __shfl_down(P[k], off, 64); Q1[k] = __shfl_down(P1[k], off, 64); Q2[k] = __shfl_down(P2[k], off, 64); }
        const double qm = __shfl_down(m, off, 64);
        if ((j & (2 * off - 1)) == 0) {
            mo_mul(P, P1, P2, Q, Q1, Q2);
            m += qm;
        }
    }
    if (j == 0) {
        double* __restrict__ o = out + (int64_t) blockIdx.x * 48;
#pragma unroll
        for (int k = 0; k < 16; k++) { o[k] = P[k]; o[16 + k] = P1[k]; o[32 + k] = P2[k]; }
        outx[blockIdx.x] = m;
    }
}

// one thread per part: out[i][0..6] = E[R], Var(R), s, e, Cov(R, E0), Cov(R, S0), Cov(S0, E0)
template <bool SEQ>
__global__ void __launch_bounds__(64) k_run_chain(int n_parts, const RnPart* __restrict__ parts, const double* __restrict__ pm,
                                                  const double* __restrict__ px, PassView pv, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_parts) return;
    const RnPart pt = parts[i];
    double f[4], b[4], fe[4], bb[4], d[4], de[4];
    mo_fb<SEQ>(pv, pt.c, pt.a, f, b);
    mo_fb<SEQ>(pv, pt.c, pt.b, fe, bb);
    const double s0 = mo_centre(f, b, pt.mask, 1.0, d), e0 = mo_centre(fe, bb, pt.mask, 1.0, de);
    double mean = s0;
    double v[4], v1[4], v2[4], u[4], u1[4], bS[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const bool in = (pt.mask >> s) & 1;
        v[s] = f[s]; v1[s] = f[s] * d[s]; v2[s] = (f[s] * d[s]) * d[s];
        u[s] = in ? f[s] : 0.0; u1[s] = in ? f[s] * d[s] : 0.0;
        bS[s] = in ? bb[s] : 0.0;
    }
    for (int g = pt.p0; g < pt.p1; g++) {
        const double* __restrict__ Q = pm + (int64_t) g * 48;
        double a0[4], a1[4], a2[4], c0[4], c1[4], c2[4], w0[4], w1[4], w2[4];
        dec_vm<SumTimes>(v2, Q, a0);
        dec_vm<SumTimes>(v1, Q + 16, a1);
        dec_vm<SumTimes>(v, Q + 32, a2);
        dec_vm<SumTimes>(v1, Q, c0);
        dec_vm<SumTimes>(v, Q + 16, c1);
        dec_vm<SumTimes>(v, Q, c2);
        dec_vm<SumTimes>(u1, Q, w0);
        dec_vm<SumTimes>(u, Q + 16, w1);
        dec_vm<SumTimes>(u, Q, w2);
        double m = 0.0;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            v2[s] = (a0[s] + 2.0 * a1[s]) + a2[s]; v1[s] = c0[s] + c1[s]; v[s] = c2[s];
            u1[s] = w0[s] + w1[s]; u[s] = w2[s];
            m = fmax(m, v[s]);
        }
        if (m > 0.0 && !isinf(m)) {      // (the five share the scale of v)
            const int e = -ilogb(m);
#pragma unroll
            for (int s = 0; s < 4; s++) {
                v[s] = ldexp(v[s], e); v1[s] = ldexp(v1[s], e); v2[s] = ldexp(v2[s], e);
                u[s] = ldexp(u[s], e); u1[s] = ldexp(u1[s], e);
            }
        }
        mean += px[g];
    }
    const double L = iv_dot(v, bb), r = iv_dot(v1, bb) / L;
    double var = iv_dot(v2, bb) / L - r * r;
    if (!(var > 0.0)) var = 0.0;      // (a negative rounding residue; no weight left by the pass)
    double* __restrict__ o = out + (int64_t) i * HF_RN_OUT;
    o[0] = mean;
    o[1] = var;
    o[2] = s0;
    o[3] = e0;
    o[4] = iv_dot(v1, bS) / L - r * e0;
    o[5] = iv_dot(u1, bb) / L - r * s0;
    o[6] = iv_dot(u, bS) / L - s0 * e0;
}
