// hf_moments.h — exact mean and variance of label totals (hf_get_count_moments): for a window range, a state set S, a region filter and a
// unit, the posterior mean and variance of N = sum_t w_t 1[s_t in S] under the model of the last HF_MODE_FULL pass.  Not part of an EM
// pass: it reads the pass's rows, forward and backward vectors and writes buffers of its own only.
//
// Definition.  w_t = the weight of window t: 1 (HF_COUNT_WINDOWS) or the window's length in bases (HF_COUNT_BASES), 0 where the region
// filter rejects the window.  gamma_t(S) = sum_{s in S} f_t[s] b_t[s] / sum_s f_t[s] b_t[s]: hf_get_posterior's value (both sums in state
// order, so S = all four states gives exactly 1).  A job's chunk-local part [a, b]:
//   mean(part) = sum_t w_t gamma_t(S), summed in the fixed order below
//   var(part)  = L''/L - (L'/L)^2, from the second-order jet of the product with the CENTRED weight d_t[s] = w_t (1_S[s] - gamma_t(S)):
//     (v, v', v'') = (f_a, f_a o d_a, f_a o d_a^2)
//     t = a+1..b:  v'' <- v''A_t + 2 (v'A_t) o d_t + (vA_t) o d_t^2,  v' <- v'A_t + (vA_t) o d_t,  v <- vA_t
//     L = v.b_b, L' = v'.b_b, L'' = v''.b_b
// Centring changes nothing in exact arithmetic (a variance does not move with a shift) and everything in float64: uncentred, the variance
// is the small difference E[N^2] - E[N]^2 of two numbers of size mean^2; centred by gamma, L' is the sum of rounding residues only.
// In matrix form a stretch of windows is a triple (P, P', P''), (PQ)' = P'Q + PQ', (PQ)'' = P''Q + 2 P'Q' + PQ'': associative.
//
// PIECES, as hf_interval.h cuts them: the interior windows (a, b] of every part at global window indices that are multiples of
// HF_MO_PIECE, so a piece depends on its job alone.
//   k_mo_piece  one 64-lane workgroup per piece: lane j takes windows t0 + j*HF_MO_LANE .. + HF_MO_LANE - 1 in order (a lane without
//               windows: the identity (I, 0, 0)).  The right factor of a step is a single window's (A, A D, A D^2), D = diag(d_t): three
//               4x4 products and column scalings per window.  Then the fixed-shape pairwise reduction over the lanes (level k: lane j,
//               j % 2^(k+1) == 0, takes lane j + 2^k's triple on its right: six 4x4 products); the lanes' sums of w_t gamma_t take the same
//               tree.  Every product is renormalised by 2^-e, e the exponent of the largest entry of P, applied to P, P' and P'' alike
//               (the three share a scale); the exponents need not be kept: the results are the ratios L'/L and L''/L.
//   k_mo_chain  one thread per part: (v, v', v'') from window a through the part's pieces in order, then the dot products with b_b.
// Nothing depends on the other jobs of a call: a job's two values are bitwise the same whatever the call holds.  S = all four states has
// d = 0 exactly: var 0.0, mean the sum of the weights.
#pragma once
#include "hf_view.h"
#include "hf_interval.h"

#define HF_MO_LANE 8                      // windows per lane of a piece
#define HF_MO_PIECE (64 * HF_MO_LANE)     // windows per piece at most; pieces are cut at global indices that are multiples of this

// windows t0 .. t0 + n - 1 of chunk c (k0 = t0 - the chunk's first window; cs, ce: the chunk's first and last base), mask, region filter
struct MoPiece { long long t0; int n, mask, region, c, k0, cs, ce; };
// chunk-local part [a, b] of chunk c (ka = a - the chunk's first window), its pieces p0 .. p1 - 1
struct MoPart { long long a, b; int p0, p1, mask, region, c, ka, cs, ce; };

// the weight of window t (k-th of its chunk): 0 outside the region filter, else 1 or the window's bases (W = the window length; 0: count windows)
__device__ __forceinline__ double mo_weight(const uint32_t* __restrict__ rec, int64_t t, int k, int region, int W, int cs, int ce) {
    if (region >= 0 && (int) REC_REGION(rec[t]) != region) return 0.0;
    if (W <= 0) return 1.0;
    const long long s = (long long) cs + (long long) k * W, e = s + W - 1;
    return (double) ((e < ce ? e : (long long) ce) - s + 1);
}

// gamma_t(S) and the centred weight d[s] = w (1_S[s] - gamma); returns w gamma
__device__ __forceinline__ double mo_centre(const double f[4], const double b[4], int mask, double w, double d[4]) {
    double g[4];
#pragma unroll
    for (int s = 0; s < 4; s++) g[s] = f[s] * b[s];
    double tot = g[0], in = (mask & 1) ? g[0] : 0.0;
#pragma unroll
    for (int s = 1; s < 4; s++) { tot += g[s]; in += ((mask >> s) & 1) ? g[s] : 0.0; }
    const double gam = in / tot;
#pragma unroll
    for (int s = 0; s < 4; s++) d[s] = w * ((((mask >> s) & 1) ? 1.0 : 0.0) - gam);
    return w * gam;
}

// (P, P1, P2) by 2^-e, e = the exponent of the largest entry of P
template <int N>
__device__ __forceinline__ void mo_norm(double* P, double* P1, double* P2) {
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < N; k++) m = fmax(m, P[k]);
    if (!(m > 0.0) || isinf(m)) return;
    const int e = -ilogb(m);
#pragma unroll
    for (int k = 0; k < N; k++) { P[k] = ldexp(P[k], e); P1[k] = ldexp(P1[k], e); P2[k] = ldexp(P2[k], e); }
}

// (P, P1, P2) <- (P, P1, P2) (A, A D, A D^2), D = diag(d): one window on the right
__device__ __forceinline__ void mo_step(double P[16], double P1[16], double P2[16], const double A[16], const double d[4]) {
    double X[16], X1[16], X2[16];
    dec_mm<SumTimes>(P, A, X);
    dec_mm<SumTimes>(P1, A, X1);
    dec_mm<SumTimes>(P2, A, X2);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const double dk = d[k & 3];
        P2[k] = (X2[k] + 2.0 * (X1[k] * dk)) + (X[k] * dk) * dk;
        P1[k] = X1[k] + X[k] * dk;
        P[k] = X[k];
    }
    mo_norm<16>(P, P1, P2);
}

// (P, P1, P2) <- (P, P1, P2) (Q, Q1, Q2)
__device__ __forceinline__ void mo_mul(double P[16], double P1[16], double P2[16], const double Q[16], const double Q1[16], const double Q2[16]) {
    double X[16], Y[16], Z[16];
    dec_mm<SumTimes>(P2, Q, X);
    dec_mm<SumTimes>(P1, Q1, Y);
    dec_mm<SumTimes>(P, Q2, Z);
#pragma unroll
    for (int k = 0; k < 16; k++) P2[k] = (X[k] + 2.0 * Y[k]) + Z[k];
    dec_mm<SumTimes>(P1, Q, X);
    dec_mm<SumTimes>(P, Q1, Y);
#pragma unroll
    for (int k = 0; k < 16; k++) P1[k] = X[k] + Y[k];
    dec_mm<SumTimes>(P, Q, X);
#pragma unroll
    for (int k = 0; k < 16; k++) P[k] = X[k];
    mo_norm<16>(P, P1, P2);
}

// out[g][0..15] = P, [16..31] = P', [32..47] = P''; outm[g] = the piece's sum of w_t gamma_t
template <bool SEQ>
__global__ void __launch_bounds__(64) k_mo_piece(const MoPiece* __restrict__ pieces, int W, PassView pv, double* __restrict__ out,
                                                 double* __restrict__ outm) {
    const MoPiece pc = pieces[blockIdx.x];
    const int j = threadIdx.x;
    double P[16], P1[16], P2[16], m = 0.0;
    dec_ident(P);
#pragma unroll
    for (int k = 0; k < 16; k++) { P1[k] = 0.0; P2[k] = 0.0; }
#pragma unroll 1
    for (int i = 0; i < HF_MO_LANE; i++) {
        const int x = j * HF_MO_LANE + i;
        if (x >= pc.n) break;
        const int64_t t = pc.t0 + x;
        double A[16], f[4], b[4], d[4];
        iv_row<SEQ>(pv, t, A);
        mo_fb<SEQ>(pv, pc.c, t, f, b);
        m += mo_centre(f, b, pc.mask, mo_weight(pv.rec, t, pc.k0 + x, pc.region, W, pc.cs, pc.ce), d);
        mo_step(P, P1, P2, A, d);
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
        outm[blockIdx.x] = m;
    }
}

// one thread per part: out[i] = (mean, var)
template <bool SEQ>
__global__ void __launch_bounds__(64) k_mo_chain(int n_parts, const MoPart* __restrict__ parts, int W, const double* __restrict__ pm,
                                                 const double* __restrict__ pmean, PassView pv, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_parts) return;
    const MoPart pt = parts[i];
    double f[4], b[4], fe[4], bb[4], d[4];
    mo_fb<SEQ>(pv, pt.c, pt.a, f, b);
    mo_fb<SEQ>(pv, pt.c, pt.b, fe, bb);
    double mean = mo_centre(f, b, pt.mask, mo_weight(pv.rec, pt.a, pt.ka, pt.region, W, pt.cs, pt.ce), d);
    double v[4], v1[4], v2[4];
#pragma unroll
    for (int s = 0; s < 4; s++) { v[s] = f[s]; v1[s] = f[s] * d[s]; v2[s] = (f[s] * d[s]) * d[s]; }
    for (int g = pt.p0; g < pt.p1; g++) {
        const double* __restrict__ Q = pm + (int64_t) g * 48;
        double a0[4], a1[4], a2[4], c0[4], c1[4], c2[4];
        dec_vm<SumTimes>(v2, Q, a0);
        dec_vm<SumTimes>(v1, Q + 16, a1);
        dec_vm<SumTimes>(v, Q + 32, a2);
        dec_vm<SumTimes>(v1, Q, c0);
        dec_vm<SumTimes>(v, Q + 16, c1);
        dec_vm<SumTimes>(v, Q, c2);
#pragma unroll
        for (int s = 0; s < 4; s++) { v2[s] = (a0[s] + 2.0 * a1[s]) + a2[s]; v1[s] = c0[s] + c1[s]; v[s] = c2[s]; }
        mo_norm<4>(v, v1, v2);
        mean += pmean[g];
    }
    const double L = iv_dot(v, bb), r = iv_dot(v1, bb) / L;
    double var = iv_dot(v2, bb) / L - r * r;
    if (!(var > 0.0)) var = 0.0;      // (a negative rounding residue; no weight left by the pass)
    out[(int64_t) i * 2] = mean;
    out[(int64_t) i * 2 + 1] = var;
}
