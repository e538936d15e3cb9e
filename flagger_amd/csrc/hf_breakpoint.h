// hf_breakpoint.h — exact breakpoint posteriors (hf_get_breakpoints, hf_get_breakpoint_profile): given that a window range [a, b] of one
// chunk switches once from a state set U to a state set V, the posterior over the switching window, under the model of the last
// HF_MODE_FULL pass.  Not part of an EM pass: it reads the pass's rows, forward and backward vectors and writes buffers of its own only.
//
// Definition.  A job is a range a < b in one chunk and two disjoint masks U, V; D_S = diag(1_S).  For k = a+1 .. b the event E_k is
// "s_t in U for a <= t < k and s_t in V for k <= t <= b" (k: the first window of the right side):
//   L_a = f_a o 1_U,  L_t = L_{t-1} (A_t D_U)          row vectors, t = a+1 .. b-1
//   r_b = b_b,        r_{t-1} = (A_t D_V) r_t          column vectors, t = b .. a+1
//   w_k = L_{k-1} . r_{k-1}                            (sum in state order)
//   N   = f_a (A_{a+1} ... A_b) b_b                    (the unmasked chain of hf_interval.h)
//   P(E_k | data) = w_k / N,  W = sum_k w_k,  p_k = w_k / W,  log_p_event = log W - log N
// f, b are the pass's scaled vectors and A_t the row the pass multiplied by at window t (hf_view.h).
//
// PIECES are those of hf_interval.h: the interior windows (a, b] cut at global window indices that are multiples of HF_BP_PIECE, 64
// lanes of HF_BP_LANE windows, every vector and matrix renormalised by a power of two after every product (dec_norm) with integer
// exponent sums.  A job is one part.  Four launches per device batch:
//   k_bp_piece    one workgroup per piece: the lane products of (A_t D_U), (A_t D_V) and A_t, then k_iv_piece's pairwise reduction over
//                 the lanes.  Out: three 4x4 products and their exponents.
//   k_bp_chain    one thread per part: forward through its pieces, storing the vector L that ENTERS every piece (L_{t0-1}, t0 the piece's
//                 first window); backward, storing the vector r that LEAVES every piece (r_{t0+n-1}); and N by the unmasked chain.  The
//                 exponents stored with r are relative to N's.
//   k_bp_weights  one workgroup per piece: the lane products under U and V again (8 rows per lane: cheaper than 64 stored matrices per
//                 piece), an exclusive prefix scan of the U products from the left and an exclusive suffix scan of the V products from the
//                 right (Hillis-Steele over shuffles, the earlier window's product on the left).  Lane j enters with L_piece (x) prefix_j
//                 and leaves with suffix_j (x) r_piece, walks its windows forward keeping L_{k-1} of each, then backward forming
//                 r_{k-1} = (A_k D_V) r_k and w_k = L_{k-1} . r_{k-1}.  The rows come from L2 on the second and third reading.  Out per
//                 window k: (mantissa, exponent relative to N) — nothing underflows before the job's largest exponent is known.
//   k_bp_quant    one wavefront per part, THE FIXED ORDER of every sum: the largest exponent emax over the windows with weight; then
//                 x_k = ldexp(mantissa_k, e_k - emax) in blocks of 64 consecutive k (block m: k = a+1+64m .. a+64m+64, lane = k's place
//                 in it), inside a block a Hillis-Steele inclusive scan over the lanes (step off = 1, 2, .. 32: lane l >= off adds lane
//                 l - off's value on its LEFT), the carry of the blocks before added on the left of every lane's sum, and the new carry
//                 the value of the block's last lane.  W is the last carry; p_k = x_k / W; c_k is the same blocked scan over p_k.
//                 quantile(q) = the smallest k with p_k > 0 and c_k >= q (a c_k reached at a window without weight is the c of the window
//                 before it); mode = the smallest k of maximal p_k.
// A weight's exponent is kept as an int relative to N's, clamped below at -2^30 (an event of probability 2^-(2^30) is reported as that).
// Nothing depends on the other jobs of a call: a job's values are bitwise the same whatever the call holds.
#pragma once
#include "hf_interval.h"

#define HF_BP_LANE HF_IV_LANE                 // windows per lane of a piece
#define HF_BP_PIECE HF_IV_PIECE               // the piece grid
#define HF_BP_MAX_PROBS 8
#define HF_BP_NO_WEIGHT (-2147483647 - 1)     // the exponent of a window without weight

struct BpPiece { long long t0, w0; int n, um, vm, pad; };                 // windows t0 .. t0 + n - 1, their weights at w0 .., the masks
struct BpPart { long long a, b, w0; int p0, p1, um, vm, c, pad; };        // part [a, b] of chunk c, its pieces p0 .. p1 - 1, weights at w0
struct BpProbs { double q[HF_BP_MAX_PROBS]; int n; };

// the columns outside mask m zeroed
__device__ __forceinline__ void bp_mask(const double A[16], int m, double AS[16]) {
#pragma unroll
    for (int k = 0; k < 16; k++) AS[k] = ((m >> (k & 3)) & 1) ? A[k] : 0.0;
}

// r <- M (x) r for a column vector, renormalised; returns the exponent taken out
__device__ __forceinline__ int bp_mv(const double* __restrict__ M, double r[4]) {
    double nr[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        double m = M[p * 4] * r[0];
#pragma unroll
        for (int q = 1; q < 4; q++) m += M[p * 4 + q] * r[q];
        nr[p] = m;
    }
    const int e = dec_norm<4>(nr);
#pragma unroll
    for (int p = 0; p < 4; p++) r[p] = nr[p];
    return e;
}

// Q <- X (x) Q, renormalised; returns the exponent taken out
__device__ __forceinline__ int bp_lmul(const double X[16], double Q[16]) {
    double Nq[16];
    dec_mm<SumTimes>(X, Q, Nq);
    const int e = dec_norm<16>(Nq);
#pragma unroll
    for (int k = 0; k < 16; k++) Q[k] = Nq[k];
    return e;
}

// the products of lane j of a piece under U and under V (lanes without windows: the identity)
template <bool SEQ>
__device__ __forceinline__ void bp_lane_products(const BpPiece& pc, const PassView& pv, int j, double QU[16], int& eU, double QV[16], int& eV) {
    dec_ident(QU);
    dec_ident(QV);
    eU = 0; eV = 0;
    for (int i = 0; i < HF_BP_LANE; i++) {
        const int x = j * HF_BP_LANE + i;
        if (x >= pc.n) break;
        double A[16], AS[16];
        iv_row<SEQ>(pv, pc.t0 + x, A);
        bp_mask(A, pc.um, AS);
        eU += iv_mul(QU, AS);
        bp_mask(A, pc.vm, AS);
        eV += iv_mul(QV, AS);
    }
}

// out[g][0..15] = prod (A_t D_U), [16..31] = prod (A_t D_V), [32..47] = prod A_t; oute[g][0..2] their exponents
template <bool SEQ>
__global__ void __launch_bounds__(64) k_bp_piece(const BpPiece* __restrict__ pieces, PassView pv, double* __restrict__ out, int* __restrict__ oute) {
    const BpPiece pc = pieces[blockIdx.x];
    const int j = threadIdx.x;
    double QU[16], QV[16], Q[16];
    int eU = 0, eV = 0, e = 0;
    dec_ident(QU);
    dec_ident(QV);
    dec_ident(Q);
    for (int i = 0; i < HF_BP_LANE; i++) {
        const int x = j * HF_BP_LANE + i;
        if (x >= pc.n) break;
        double A[16], AS[16];
        iv_row<SEQ>(pv, pc.t0 + x, A);
        bp_mask(A, pc.um, AS);
        eU += iv_mul(QU, AS);
        bp_mask(A, pc.vm, AS);
        eV += iv_mul(QV, AS);
        e += iv_mul(Q, A);
    }
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        double R[16];
        const bool take = (j & (2 * off - 1)) == 0;
#pragma unroll
        for (int k = 0; k < 16; k++) R[k] = __shfl_down(QU[k], off, 64);
        int re = __shfl_down(eU, off, 64);
        if (take) eU += re + iv_mul(QU, R);
#pragma unroll
        for (int k = 0; k < 16; k++) R[k] = __shfl_down(QV[k], off, 64);
        re = __shfl_down(eV, off, 64);
        if (take) eV += re + iv_mul(QV, R);
#pragma unroll
        for (int k = 0; k < 16; k++) R[k] = __shfl_down(Q[k], off, 64);
        re = __shfl_down(e, off, 64);
        if (take) e += re + iv_mul(Q, R);
    }
    if (j == 0) {
        double* __restrict__ o = out + (int64_t) blockIdx.x * 48;
#pragma unroll
        for (int k = 0; k < 16; k++) { o[k] = QU[k]; o[16 + k] = QV[k]; o[32 + k] = Q[k]; }
        int* __restrict__ oe = oute + (int64_t) blockIdx.x * 4;
        oe[0] = eU; oe[1] = eV; oe[2] = e; oe[3] = 0;
    }
}

// one thread per part.  Lv[g], LE[g]: the vector entering piece g and its exponent; Rv[g], RE[g]: the vector leaving piece g and its
// exponent minus N's; nn[i]: N's mantissa
template <bool SEQ>
__global__ void __launch_bounds__(64) k_bp_chain(int n_parts, const BpPart* __restrict__ parts, const double* __restrict__ pm,
                                                 const int* __restrict__ pe, PassView pv, double* __restrict__ Lv, long long* __restrict__ LE,
                                                 double* __restrict__ Rv, long long* __restrict__ RE, double* __restrict__ nn) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_parts) return;
    const BpPart pt = parts[i];
    double f[4], b[4];
    mo_f<SEQ>(pv, pt.c, pt.a, f);
    mo_b<SEQ>(pv, pt.c, pt.b, b);
    double L[4], v[4];
#pragma unroll
    for (int s = 0; s < 4; s++) { L[s] = ((pt.um >> s) & 1) ? f[s] : 0.0; v[s] = f[s]; }
    long long EL = 0, EN = 0;
    for (int g = pt.p0; g < pt.p1; g++) {
#pragma unroll
        for (int s = 0; s < 4; s++) Lv[(int64_t) g * 4 + s] = L[s];
        LE[g] = EL;
        EL += pe[(int64_t) g * 4] + iv_vmul(L, pm + (int64_t) g * 48);
        EN += pe[(int64_t) g * 4 + 2] + iv_vmul(v, pm + (int64_t) g * 48 + 32);
    }
    nn[i] = iv_dot(v, b);
    long long ER = -EN;
    for (int g = pt.p1 - 1; g >= pt.p0; g--) {
#pragma unroll
        for (int s = 0; s < 4; s++) Rv[(int64_t) g * 4 + s] = b[s];
        RE[g] = ER;
        ER += pe[(int64_t) g * 4 + 1] + bp_mv(pm + (int64_t) g * 48 + 16, b);
    }
}

// wm[w0 + x], we[w0 + x]: mantissa and exponent (relative to N) of the weight of window t0 + x of every piece
template <bool SEQ>
__global__ void __launch_bounds__(64) k_bp_weights(const BpPiece* __restrict__ pieces, PassView pv, const double* __restrict__ Lv,
                                                   const long long* __restrict__ LE, const double* __restrict__ Rv,
                                                   const long long* __restrict__ RE, double* __restrict__ wm, int* __restrict__ we) {
    const int g = blockIdx.x;
    const BpPiece pc = pieces[g];
    const int j = threadIdx.x;
    double QU[16], QV[16];
    int eU, eV;
    bp_lane_products<SEQ>(pc, pv, j, QU, eU, QV, eV);
    // inclusive prefix scan of the U products, I_j = Q_0 (x) .. (x) Q_j; the exclusive one enters lane j
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        double X[16];
#pragma unroll
        for (int k = 0; k < 16; k++) X[k] = __shfl_up(QU[k], off, 64);
        const int xe = __shfl_up(eU, off, 64);
        if (j >= off) eU += xe + bp_lmul(X, QU);
    }
    double lin[4];
    long long elin = LE[g] + RE[g];          // every exponent of a weight of this lane but the walks'
    {
        double X[16];
#pragma unroll
        for (int k = 0; k < 16; k++) X[k] = __shfl_up(QU[k], 1, 64);
        int xe = __shfl_up(eU, 1, 64);
        if (j == 0) { dec_ident(X); xe = 0; }
#pragma unroll
        for (int s = 0; s < 4; s++) lin[s] = Lv[(int64_t) g * 4 + s];
        elin += xe + iv_vmul(lin, X);
    }
    // inclusive suffix scan of the V products, I_j = Q_j (x) .. (x) Q_63; the exclusive one leaves lane j
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        double X[16];
#pragma unroll
        for (int k = 0; k < 16; k++) X[k] = __shfl_down(QV[k], off, 64);
        const int xe = __shfl_down(eV, off, 64);
        if (j + off < 64) eV += xe + iv_mul(QV, X);
    }
    double r[4];
    {
        double X[16];
#pragma unroll
        for (int k = 0; k < 16; k++) X[k] = __shfl_down(QV[k], 1, 64);
        int xe = __shfl_down(eV, 1, 64);
        if (j == 63) { dec_ident(X); xe = 0; }
#pragma unroll
        for (int s = 0; s < 4; s++) r[s] = Rv[(int64_t) g * 4 + s];
        elin += xe + bp_mv(X, r);
    }
    const int x0 = j * HF_BP_LANE;
    // forward: Lk[i] = the vector before window x0 + i, its exponent eL[i] (relative to lin's)
    double Lk[HF_BP_LANE][4];
    int eL[HF_BP_LANE];
    int ecur = 0;
#pragma unroll
    for (int i = 0; i < HF_BP_LANE; i++) {
#pragma unroll
        for (int s = 0; s < 4; s++) Lk[i][s] = lin[s];
        eL[i] = ecur;
        if (i + 1 < HF_BP_LANE && x0 + i + 1 < pc.n) {      // (the vector after the lane's last window is the next lane's)
            double A[16], AS[16];
            iv_row<SEQ>(pv, pc.t0 + x0 + i, A);
            bp_mask(A, pc.um, AS);
            ecur += iv_vmul(lin, AS);
        }
    }
    // backward: r_{k-1} = (A_k D_V) r_k, w_k = L_{k-1} . r_{k-1}
    int er = 0;
#pragma unroll
    for (int i = HF_BP_LANE - 1; i >= 0; i--) {
        if (x0 + i < pc.n) {
            double A[16], AS[16];
            iv_row<SEQ>(pv, pc.t0 + x0 + i, A);
            bp_mask(A, pc.vm, AS);
            er += bp_mv(AS, r);
            double w = iv_dot(Lk[i], r);
            const bool has = w > 0.0 && !isinf(w);
            long long e = elin + eL[i] + er;
            if (has) { const int ew = ilogb(w); w = ldexp(w, -ew); e += ew; }      // the mantissa in [1, 2)
            if (e < -(1ll << 30)) e = -(1ll << 30);
            if (e > (1ll << 30)) e = 1ll << 30;
            wm[pc.w0 + x0 + i] = has ? w : 0.0;
            we[pc.w0 + x0 + i] = has ? (int) e : HF_BP_NO_WEIGHT;
        }
    }
}

// inclusive scan over the 64 lanes: lane l >= off adds lane l - off's value on its left
__device__ __forceinline__ double bp_scan64(double x, int l) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double y = __shfl_up(x, off, 64);
        if (l >= off) x = y + x;
    }
    return x;
}

// one wavefront per part.  outd[i] = (log_p_event, mode_p); outi[i] = (mode, quantile[0..7]); prof (or null): p_k at w0 + (k - a - 1)
__global__ void __launch_bounds__(64) k_bp_quant(const BpPart* __restrict__ parts, const double* __restrict__ wm, const int* __restrict__ we,
                                                 const double* __restrict__ nn, BpProbs pr, double* __restrict__ outd,
                                                 long long* __restrict__ outi, double* __restrict__ prof) {
    const int i = blockIdx.x, l = threadIdx.x;
    const BpPart pt = parts[i];
    const long long nk = pt.b - pt.a;
    const double* __restrict__ m = wm + pt.w0;
    const int* __restrict__ ex = we + pt.w0;
    int emax = HF_BP_NO_WEIGHT;
    for (long long k = l; k < nk; k += 64) emax = max(emax, ex[k]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) emax = max(emax, __shfl_xor(emax, off, 64));
    const double NN = nn[i];
    const bool bad_n = !(NN > 0.0) || isinf(NN);      // the pass left no weight (its own flags say why)
    if (emax == HF_BP_NO_WEIGHT) {
        if (prof) for (long long k = l; k < nk; k += 64) prof[pt.w0 + k] = 0.0;
        if (l == 0) {
            outd[(int64_t) i * 2] = bad_n ? __builtin_nan("") : -__builtin_inf();
            outd[(int64_t) i * 2 + 1] = 0.0;
            for (int q = 0; q <= HF_BP_MAX_PROBS; q++) outi[(int64_t) i * (HF_BP_MAX_PROBS + 1) + q] = -1;
        }
        return;
    }
    double W = 0.0;
    for (long long k0 = 0; k0 < nk; k0 += 64) {
        const long long k = k0 + l;
        const double x = (k < nk && ex[k] != HF_BP_NO_WEIGHT) ? ldexp(m[k], ex[k] - emax) : 0.0;
        W = W + __shfl(bp_scan64(x, l), 63, 64);
    }
    double carry = 0.0, best = 0.0;
    long long best_k = -1, last_k = -1;
    long long quant = -1;                    // lane q holds quantile q
    for (long long k0 = 0; k0 < nk; k0 += 64) {
        const long long k = k0 + l;
        const double x = (k < nk && ex[k] != HF_BP_NO_WEIGHT) ? ldexp(m[k], ex[k] - emax) : 0.0;
        const double p = x / W;
        const double c = carry + bp_scan64(p, l);
        carry = __shfl(c, 63, 64);
        if (prof && k < nk) prof[pt.w0 + k] = p;
        if (p > best) { best = p; best_k = k; }
        if (p > 0.0) last_k = k;
        for (int q = 0; q < pr.n; q++) {
            const unsigned long long hit = __ballot(p > 0.0 && c >= pr.q[q]);
            if (hit && l == q && quant < 0) quant = k0 + (long long) __builtin_ctzll(hit);
        }
    }
    // the mode: the largest p, the smallest k among equals
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const long long ok = __shfl_xor(best_k, off, 64), ol = __shfl_xor(last_k, off, 64);
        if (ob > best || (ob == best && ok >= 0 && (best_k < 0 || ok < best_k))) { best = ob; best_k = ok; }
        last_k = ol > last_k ? ol : last_k;
    }
    if (l < pr.n) outi[(int64_t) i * (HF_BP_MAX_PROBS + 1) + 1 + l] = pt.a + 1 + (quant >= 0 ? quant : last_k);
    if (l >= pr.n && l < HF_BP_MAX_PROBS) outi[(int64_t) i * (HF_BP_MAX_PROBS + 1) + 1 + l] = -1;
    if (l == 0) {
        outd[(int64_t) i * 2] = bad_n ? __builtin_nan("") : (log(W) - log(NN)) + (double) emax * 0.69314718055994530942;
        outd[(int64_t) i * 2 + 1] = best;
        outi[(int64_t) i * (HF_BP_MAX_PROBS + 1)] = best_k >= 0 ? pt.a + 1 + best_k : -1;
    }
}
