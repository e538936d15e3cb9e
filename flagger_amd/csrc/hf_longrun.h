// hf_longrun.h — exact long-run probabilities (hf_get_long_run_log_probs): for a window range, a state set S and a length L, the
// probability that the range holds NO run of at least L consecutive windows in S, under the model of the last HF_MODE_FULL pass.  Not
// part of an EM pass: it reads the pass's rows, forward and backward vectors (hf_view.h) and writes buffers of its own only.
//
// Definition.  The job's chunk-local parts [a, b] fall into GROUPS of parts joined to each other (hf_jobs.h group_parts, the rule of
// hf_get_run_moments).  A group's label sequence is the concatenation of its parts' windows; HIT = "it contains L consecutive windows
// in S".  The expanded chain of a group, one lane of a wavefront per expanded state, k = |S|, s_0 < .. < s_{k-1} the states of S:
//   lanes (d-1)*k + j          (s_j, d), d = 1 .. L-1: "the current run of S has d windows, the last one in s_j" (d = 1: the ENTRY lanes)
//   lanes k(L-1) ..            one OUT lane per state outside S, in state order
//   the four lanes after them  the HIT lanes, one per state, absorbing
//   first window a of the group   f_a[s] into (s, 1) for s in S (L == 1: into HIT s), into OUT s otherwise
//   a step with the row A         T[p] = the non-HIT weight in state p (p in S: the sum of its counter lanes; else its OUT lane),
//                                 O[p] = the OUT lane of p (0 for p in S), H[p] = the HIT lane of p; every sum below over p = 0..3 in order
//       OUT q        sum_p A[p][q] T[p]
//       (s, 1)       sum_p A[p][s] O[p]
//       (s, d+1)     sum_{p in S} A[p][s] x[(p, d)]
//       HIT s        sum_p A[p][s] H[p]  +  2^(E_n - E_h) * inflow,  inflow = sum_{p in S} A[p][s] x[(p, L-1)] for s in S (L == 1:
//                    sum_p A[p][s] O[p]), 0 for s outside S
//   the rows: A_t inside a part; from the last window b of a part to the first window a' of the next one the rank-one row
//             b_b[p] * f_a'[s]
//   the end: N_none = sum over the non-HIT lanes of x * b_b[state of the lane], N_hit the same over the HIT lanes
//
// NUMERICS.  Linear domain; value = x * 2^E with two integer exponent sums, E_n of the non-HIT lanes and E_h of the HIT lanes.  The
// group's first vector: e_0 = ilogb(max_s f_a[s]) - HF_LR_TARGET (0 when that maximum is 0 or not finite), every lane is scaled by 2^-e_0
// and E_n = E_h = e_0, so that the first period starts from the target like every later one: a row's entries can be as small as a
// transition probability times the emission floor of 1e-40, and HF_LR_RENORM such steps from magnitude 1 end at 3.7e-321, a subnormal
// (from 2^HF_LR_TARGET at 1e-230).  A group that ends before its first renormalisation is scaled back by 2^e_0 before the end.  After
// every HF_LR_RENORM-th step, counted from the group's first window (so a group's bits depend on the job alone), with m_n = max_p T[p]
// and m_h = max_p H[p] taken BEFORE that step: e_n = ilogb(m_n) - HF_LR_TARGET (0 when m_n is 0 or not finite), the non-HIT lanes are
// scaled by 2^-e_n and E_n += e_n; e_h = ilogb(m_h) - HF_LR_TARGET, or E_n - E_h when m_h is 0 (the HIT lanes then hold fresh inflow
// only and take the non-HIT exponent); should E_n - E_h exceed HF_LR_HIT_LAG after that, E_h = E_n (inflow must not overflow; HIT
// weight that far below the non-HIT scale is carried at the non-HIT exponent for this period); when m_n is 0 no non-HIT weight is left and
// none can come back, and E_n = E_h.  The large target leaves a lane 2^-1300
// below its class's largest total representable, so a counter lane of a very improbable run keeps its bits.  Every sum over lanes
// is ch_wave_sum (hf_chain.h), which has one order.
// NOT COVERED: a joined boundary's row b_b[p] f_a'[s] is no probability.  The pass's vectors satisfy sum_s f_t[s] b_t[s] = 1e-4 / scale_t,
// so behind a floored window b_b is about 1e36 (2^120).  One such boundary in a period is harmless; HF_LR_RENORM joined one-window
// chunks on the floor in one period multiply by 2^960 on top of the target and overflow (Inf, then the NaN of the end).  Read from the
// code, not run; a renormalisation at every joined boundary would remove it.
// The two logs, with d = (log N_hit - log N_none) + (E_h - E_n) ln 2:
//   d < 0:   log_p_none = -log1p(exp(d)),       log_p_some = d - log1p(exp(d))
//   d >= 0:  log_p_none = -d - log1p(exp(-d)),  log_p_some = -log1p(exp(-d))
//   N_hit == 0: (0.0, -inf).  N_none == 0: (-inf, 0.0).  Neither positive, or one not finite: NaN (the pass left no weight).
//
// k_lr_chain: one 64-lane workgroup per group.  The staging of hf_chain.h without a pad, the tiles following the group's parts; a lane
// reads its column A[0..3][s] only.  Per window: up to four masked wave sums (T), up to seven lane reads at wave-uniform indices (O, H),
// up to four permutes at fixed per-lane sources (lane (s, d+1) takes the |S| lanes of d).  No scratch, no LDS beyond the staging.
#pragma once
#include "hf_view.h"
#include "hf_chain.h"

#define HF_LR_RENORM 8          // steps between renormalisations
#define HF_LR_TARGET 300        // exponent a class's largest total is brought to
#define HF_LR_HIT_LAG 600       // E_n - E_h at most, after a renormalisation

struct LrPiece { char unused; };                          // (the job cutter counts 512-window pieces for the batch cap; none is uploaded)
struct LrPart { long long a, b; int p0, p1, c, pad; };    // chunk-local part [a, b] of chunk c
struct LrGroup { int q0, q1, mask, len; };                // parts q0 .. q1 - 1 of the batch, state set, L

enum { LR_ENTRY = 0, LR_COUNT = 1, LR_OUT = 2, LR_HIT = 3, LR_NONE = 4 };

__device__ __forceinline__ double lr_pick(const double v[4], int s) { return s == 0 ? v[0] : s == 1 ? v[1] : s == 2 ? v[2] : v[3]; }

__device__ __forceinline__ double lr_dot(double c0, double c1, double c2, double c3, const double u[4]) {
    return ((c0 * u[0] + c1 * u[1]) + c2 * u[2]) + c3 * u[3];
}

// the row of the step INTO window pt.a + w of part q (w > 0: A_t; w == 0: the joined boundary's rank-one row, nothing for the group's
// first window), for the lanes whose window lies in the part
template <bool SEQ>
__device__ __forceinline__ void lr_load(const PassView& pv, const LrPart* __restrict__ parts, int q, int q_first, const LrPart& pt,
                                        long long w, double A[16]) {
    if (pt.a + w > pt.b) return;
    if (w > 0) { iv_row<SEQ>(pv, pt.a + w, A); return; }
    if (q == q_first) return;
    const LrPart pr = parts[q - 1];
    double b[4], f[4];
    mo_b<SEQ>(pv, pr.c, pr.b, b);
    mo_f<SEQ>(pv, pt.c, pt.a, f);
#pragma unroll
    for (int k = 0; k < 16; k++) A[k] = b[k >> 2] * f[k & 3];
}

// out[g] = (log_p_none, log_p_some) of group g
template <bool SEQ>
__global__ void __launch_bounds__(64) k_lr_chain(const LrGroup* __restrict__ groups, const LrPart* __restrict__ parts, PassView pv,
                                                 double* __restrict__ out) {
    const LrGroup g = groups[blockIdx.x];
    const int lane = threadIdx.x;
    const int mask = __builtin_amdgcn_readfirstlane(g.mask), L = __builtin_amdgcn_readfirstlane(g.len);
    const int q_first = __builtin_amdgcn_readfirstlane(g.q0), q_end = __builtin_amdgcn_readfirstlane(g.q1);
    const int k = __popc(mask), nc = k * (L - 1), h0 = nc + (4 - k), total = h0 + 4;
    __shared__ ChainTile As;

    // the lane's class and state, and where its permutes read: the lanes of d - 1, for a HIT lane those of L - 1
    int cls = LR_NONE, st = 0, src0 = 0;
    if (lane < nc) {
        const int j = lane % k, d = lane / k + 1;
        int seen = 0;
#pragma unroll
        for (int p = 0; p < 4; p++) if ((mask >> p) & 1) { if (seen == j) st = p; seen++; }
        cls = d == 1 ? LR_ENTRY : LR_COUNT;
        src0 = d == 1 ? 0 : (d - 2) * k;
    } else if (lane < h0) {
        int seen = 0;
#pragma unroll
        for (int p = 0; p < 4; p++) if (!((mask >> p) & 1)) { if (seen == lane - nc) st = p; seen++; }
        cls = LR_OUT;
    } else if (lane < total) {
        cls = LR_HIT; st = lane - h0;
        src0 = L > 1 ? (L - 2) * k : 0;
    }
    const bool st_in = (mask >> st) & 1;
    const bool counter = cls == LR_ENTRY || cls == LR_COUNT;
    int src[4], outl[4];      // per state: the permute's source lane (p in S), the OUT lane (p outside S)
#pragma unroll
    for (int p = 0; p < 4; p++) {
        src[p] = src0 + __popc(mask & ((1 << p) - 1));
        outl[p] = nc + __popc(~mask & ((1 << p) - 1));
    }

    int q = q_first;
    LrPart pt = parts[q];
    double x;
    long long En = 0, Eh = 0;
    {
        double f[4];
        mo_f<SEQ>(pv, pt.c, pt.a, f);
        const double fs = lr_pick(f, st);
        x = (L == 1 ? (cls == LR_OUT || (cls == LR_HIT && st_in)) : (cls == LR_ENTRY || cls == LR_OUT)) ? fs : 0.0;
        // the first vector goes to the target like every later period's: eight steps over floored rows (1e-40 each) from magnitude 1
        // would end subnormal.  Both classes take the one exponent, a power of two: every value of the first period is the unscaled
        // one times 2^-e0 exactly, and E_n, E_h after the first renormalisation are what they were without it
        const double fm = fmax(fmax(f[0], f[1]), fmax(f[2], f[3]));
        int e0 = 0;
        if (fm > 0.0 && !isinf(fm)) e0 = ilogb(fm) - HF_LR_TARGET;
        x = ldexp(x, -e0);
        En = Eh = e0;
    }
    int sh = 0;                 // E_n - E_h, clamped for ldexp
    unsigned step = 0;

    long long base = 0;
    double nx[16];
#pragma unroll
    for (int i = 0; i < 16; i++) nx[i] = 0.0;
    lr_load<SEQ>(pv, parts, q, q_first, pt, base + lane, nx);
    bool have = true;
    while (have) {
        const long long left = pt.b - pt.a - base + 1;
        const int n = (int) (left < 64 ? left : 64);
        if (lane < n) {
#pragma unroll
            for (int i = 0; i < 16; i++) As[lane][i] = nx[i];
        }
        // the block after this one: the same part's next 64 windows, else the next part of the group
        int nq = q;
        LrPart npt = pt;
        long long nbase = base + 64;
        bool have_next = true;
        if (pt.a + nbase > pt.b) {
            nq = q + 1; nbase = 0;
            have_next = nq < q_end;
            if (have_next) npt = parts[nq];
        }
        if (have_next) lr_load<SEQ>(pv, parts, nq, q_first, npt, nbase + lane, nx);
        __syncthreads();
        const int w0 = (q == q_first && base == 0) ? 1 : 0;
        double c0, c1, c2, c3;
        c0 = As[w0][st]; c1 = As[w0][4 + st]; c2 = As[w0][8 + st]; c3 = As[w0][12 + st];
        for (int w = w0; w < n; w++) {
            const double a0 = c0, a1 = c1, a2 = c2, a3 = c3;
            c0 = As[w + 1][st]; c1 = As[w + 1][4 + st]; c2 = As[w + 1][8 + st]; c3 = As[w + 1][12 + st];
            double T[4], O[4], H[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                if ((mask >> p) & 1) { T[p] = ch_wave_sum(counter && st == p ? x : 0.0); O[p] = 0.0; }
                else { O[p] = ch_readlane(x, outl[p]); T[p] = O[p]; }
                H[p] = ch_readlane(x, h0 + p);
            }
            double U[4];
#pragma unroll
            for (int p = 0; p < 4; p++) U[p] = cls == LR_OUT ? T[p] : cls == LR_HIT ? H[p] : O[p];
            const double dotU = lr_dot(a0, a1, a2, a3, U);
            double dotS = 0.0;
            if (L > 1) {
                if (mask & 1) dotS += a0 * __shfl(x, src[0], 64);
                if (mask & 2) dotS += a1 * __shfl(x, src[1], 64);
                if (mask & 4) dotS += a2 * __shfl(x, src[2], 64);
                if (mask & 8) dotS += a3 * __shfl(x, src[3], 64);
            } else {
                dotS = lr_dot(a0, a1, a2, a3, O);
            }
            const double inflow = st_in ? ldexp(dotS, sh) : 0.0;
            x = cls == LR_COUNT ? dotS : cls == LR_HIT ? dotU + inflow : cls == LR_NONE ? 0.0 : dotU;
            step++;
            if (step % HF_LR_RENORM == 0) {
                const double mn = fmax(fmax(T[0], T[1]), fmax(T[2], T[3])), mh = fmax(fmax(H[0], H[1]), fmax(H[2], H[3]));
                int en = 0;
                if (mn > 0.0 && !isinf(mn)) en = __builtin_amdgcn_readfirstlane(ilogb(mn)) - HF_LR_TARGET;
                En += en;
                long long eh = En - Eh;
                if (mh > 0.0 && !isinf(mh)) eh = __builtin_amdgcn_readfirstlane(ilogb(mh)) - HF_LR_TARGET;
                const bool dead = !(mn > 0.0);      // no non-HIT weight is left, none can come back: E_n follows E_h
                if (!dead && En - (Eh + eh) > HF_LR_HIT_LAG) eh = En - Eh;
                Eh += eh;
                if (dead) En = Eh;
                const long long lag = En - Eh;
                sh = (int) (lag < -4000 ? -4000 : lag);
                const long long mine = cls == LR_HIT ? eh : (long long) en;
                x = ldexp(x, (int) (mine > 4000 ? -4000 : mine < -4000 ? 4000 : -mine));
            }
        }
        __syncthreads();
        q = nq; pt = npt; base = nbase; have = have_next;
    }

    // the end: the dot products with b of the group's last window
    // (a group that was never renormalised goes back to the magnitude of its f_a first: log() of a value and of its 2^300-fold round
    // differently, and the result of so short a group shall not depend on HF_LR_TARGET)
    if (step < HF_LR_RENORM) x = ldexp(x, (int) En);        // (E_n = E_h = e_0 still)
    double bb[4];
    mo_b<SEQ>(pv, pt.c, pt.b, bb);
    const double xb = x * lr_pick(bb, st);
    const double Nn = ch_wave_sum(counter || cls == LR_OUT ? xb : 0.0), Nh = ch_wave_sum(cls == LR_HIT ? xb : 0.0);
    if (lane != 0) return;
    double none, some;
    const double inf = __builtin_inf();
    if (!(Nn >= 0.0) || !(Nh >= 0.0) || isinf(Nn) || isinf(Nh) || (Nn == 0.0 && Nh == 0.0)) none = some = __builtin_nan("");
    else if (Nh == 0.0) { none = 0.0; some = -inf; }
    else if (Nn == 0.0) { none = -inf; some = 0.0; }
    else {
        const double d = (log(Nh) - log(Nn)) + (double) (Eh - En) * 0.69314718055994530942;
        if (d < 0.0) { const double l = log1p(exp(d)); none = -l; some = d - l; }
        else { const double l = log1p(exp(-d)); none = -d - l; some = -l; }
    }
    out[(int64_t) blockIdx.x * 2] = none;
    out[(int64_t) blockIdx.x * 2 + 1] = some;
}
