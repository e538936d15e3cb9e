// hf_interval.h — exact interval probabilities (hf_get_interval_log_probs): for a window range and a state set S, the log of
// P(s_t in S for every t of the range | data) under the model of the last HF_MODE_FULL pass.  Not part of an EM pass: it reads the
// pass's rows, forward and backward vectors and writes buffers of its own only.
//
// Definition.  A job's chunk-local part [a, b] (a <= b in one chunk), D_S = diag(1_S):
//   M_S = prod_{t=a+1..b} (A_t D_S)   (the identity when a == b)
//   N_S = sum_{p in S} sum_{q in S} f_a[p] M_S[p][q] b_b[q],   N = the same with S = all four states
//   log_p(part) = log N_S - log N;  a job's value is the sum of its parts' in chunk order
// f, b are the pass's scaled forward and backward vectors (hf_get_forward_backward) and A_t the row the pass multiplied by at window t:
// hf_view.h says where either algorithm left them.
//
// PIECES.  The host cuts the interior windows (a, b] of every part at global window indices that are multiples of HF_IV_PIECE; a piece
// therefore depends on its job alone.
//   k_iv_piece  one 64-lane workgroup per piece: lane j multiplies the rows of windows t0 + j*HF_IV_LANE .. + HF_IV_LANE - 1 (lanes
//               without windows: the identity), masked (columns outside S zeroed by a select) and unmasked, in the (+, x) semiring of
//               hf_decode.h, renormalised after every product with integer exponent sums; then a fixed-shape pairwise reduction over
//               the 64 lanes (level k: lane j, j % 2^(k+1) == 0, takes lane j + 2^k's product on its right).  Out: (M_S, e_S, M, e).
//   k_iv_chain  one thread per part: v_S = f_a o 1_S, v = f_a through the part's pieces in order (renormalised), then the dot
//               products with b_b o 1_S and b_b: log N_S - log N + (E_S - E) ln 2.
// The masked and unmasked halves run the same operations, so S = all four states gives exactly 0.  Nothing depends on the other jobs
// of a call: a job's value is bitwise the same whatever the call holds.
#pragma once
#include "hf_view.h"

#define HF_IV_LANE 8                      // windows per lane of a piece
#define HF_IV_PIECE (64 * HF_IV_LANE)     // windows per piece at most; pieces are cut at global indices that are multiples of this

struct IvPiece { long long t0; int n, mask; };              // windows t0 .. t0 + n - 1, state mask
struct IvPart { long long a, b; int p0, p1, mask, c; };     // chunk-local part [a, b] of chunk c, its pieces p0 .. p1 - 1

// Q <- Q (x) X, renormalised; returns the exponent taken out
__device__ __forceinline__ int iv_mul(double Q[16], const double X[16]) {
    double Nq[16];
    dec_mm<SumTimes>(Q, X, Nq);
    const int e = dec_norm<16>(Nq);
#pragma unroll
    for (int k = 0; k < 16; k++) Q[k] = Nq[k];
    return e;
}

// out[g][0..15] = M_S, out[g][16..31] = M; oute[g] = (e_S, e)
template <bool SEQ>
__global__ void __launch_bounds__(64) k_iv_piece(const IvPiece* __restrict__ pieces, PassView pv, double* __restrict__ out,
                                                 int* __restrict__ oute) {
    const IvPiece pc = pieces[blockIdx.x];
    const int j = threadIdx.x;
    double QS[16], Q[16];
    int eS = 0, e = 0;
    dec_ident(QS);
    dec_ident(Q);
    for (int i = 0; i < HF_IV_LANE; i++) {
        const int x = j * HF_IV_LANE + i;
        if (x >= pc.n) break;
        double A[16], AS[16];
        iv_row<SEQ>(pv, pc.t0 + x, A);
#pragma unroll
        for (int k = 0; k < 16; k++) AS[k] = ((pc.mask >> (k & 3)) & 1) ? A[k] : 0.0;
        eS += iv_mul(QS, AS);
        e += iv_mul(Q, A);
    }
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        double RS[16], R[16];
#pragma unroll
        for (int k = 0; k < 16; k++) { RS[k] = __shfl_down(QS[k], off, 64); R[k] = __shfl_down(Q[k], off, 64); }
        const int reS = __shfl_down(eS, off, 64), re = __shfl_down(e, off, 64);
        if ((j & (2 * off - 1)) == 0) {
            eS += reS + iv_mul(QS, RS);
            e += re + iv_mul(Q, R);
        }
    }
    if (j == 0) {
        double* __restrict__ o = out + (int64_t) blockIdx.x * 32;
#pragma unroll
        for (int k = 0; k < 16; k++) { o[k] = QS[k]; o[16 + k] = Q[k]; }
        oute[(int64_t) blockIdx.x * 2] = eS;
        oute[(int64_t) blockIdx.x * 2 + 1] = e;
    }
}

// v <- v (x) M, renormalised; returns the exponent taken out
__device__ __forceinline__ int iv_vmul(double v[4], const double* __restrict__ M) {
    double nv[4];
    dec_vm<SumTimes>(v, M, nv);
    const int e = dec_norm<4>(nv);
#pragma unroll
    for (int s = 0; s < 4; s++) v[s] = nv[s];
    return e;
}

__device__ __forceinline__ double iv_dot(const double v[4], const double b[4]) {
    double d = v[0] * b[0];
#pragma unroll
    for (int q = 1; q < 4; q++) d += v[q] * b[q];
    return d;
}

// one thread per part: its log N_S - log N
template <bool SEQ>
__global__ void __launch_bounds__(64) k_iv_chain(int n_parts, const IvPart* __restrict__ parts, const double* __restrict__ pm,
                                                 const int* __restrict__ pe, PassView pv, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_parts) return;
    const IvPart pt = parts[i];
    double f[4], b[4];
    mo_f<SEQ>(pv, pt.c, pt.a, f);
    mo_b<SEQ>(pv, pt.c, pt.b, b);
    double vS[4], v[4], bS[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const bool in = (pt.mask >> s) & 1;
        vS[s] = in ? f[s] : 0.0; v[s] = f[s]; bS[s] = in ? b[s] : 0.0;
    }
    long long ES = 0, EN = 0;
    for (int g = pt.p0; g < pt.p1; g++) {
        ES += pe[(int64_t) g * 2] + iv_vmul(vS, pm + (int64_t) g * 32);
        EN += pe[(int64_t) g * 2 + 1] + iv_vmul(v, pm + (int64_t) g * 32 + 16);
    }
    const double NS = iv_dot(vS, bS), NN = iv_dot(v, b);
    double r;
    if (!(NN > 0.0) || isinf(NN)) r = __builtin_nan("");          // the pass left no weight (its own flags say why)
    else if (!(NS > 0.0)) r = NS == 0.0 ? -__builtin_inf() : __builtin_nan("");
    else r = (log(NS) - log(NN)) + (double) (ES - EN) * 0.69314718055994530942;
    out[i] = r;
}
