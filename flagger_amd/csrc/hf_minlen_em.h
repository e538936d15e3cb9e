// hf_minlen_em.h — the E-step under minimum run lengths (hf_estep_minlen): the expected sufficient statistics of EM_updateEstimators under
// the posterior over ADMISSIBLE paths.  k_mlp_fwd (hf_minlen_post.h) runs as it is and leaves the forward lanes F, log Z_adm and log Z;
// k_mle_bwd walks back as k_mlp_bwd does and leaves the pair posterior xi_adm; k_mle_tile is k_stats_tile (hf_chunks.h) with the four
// counts of a column read from xi_adm; k_chunk_stats and k_reduce then run as they are.
//
// Definition (include/hmm_flagger_hip.h has it in full), m_s = min_len[s], pair (t-1, t), 1 <= t <= T-1:
//   p != s, or p == s with m_s == 1:  u_t[p][s] = F_{t-1}[(p, m_p)] * A_t[p][s] * B_t[(s, 1)]
//   p == s, m_s > 1:                  u_t[s][s] = the wave sum over the lanes (s, d), d = 2 .. m_s, of c_d * A_t[s][s] * B_t[(s, d)],
//                                     c_d = F_{t-1}[(s, d-1)] for d < m_s, c_{m_s} = F_{t-1}[(s, m_s-1)] + F_{t-1}[(s, m_s)]
//   tot_t = the sum over s ascending of ((u[0][s] + u[1][s]) + u[2][s]) + u[3][s], accumulated from the left
//   xi_adm_t[p][s] = u_t[p][s] / tot_t
// A TERM x * a * y (x from F_{t-1}, a from A_t, y from B_t) is formed as (mant(x) * mant(a)) * mant(y), the three frexp mantissas, with the
// exponent sum e = exp(x) + exp(a) + exp(y); e_t is the largest e over the window's non-zero terms (an integer maximum over the
// wavefront), and the term enters the sums as ldexp(mantissa product, max(e - e_t, -2000)): the window's largest term is in [1/8, 1),
// whatever the places of F_{t-1} and B_t in their rescaling periods.  The power of two cancels in xi_adm.
// The saturated lane of p (with m_p == 1: its one lane) forms u[p][0..3] from its row A_t[p][.] and the entry lanes of B_t, which the
// step back needs anyway; a lane (s, d >= 2) forms its term of u[s][s] from the lane below it.
// Flags: HF_FLAG_NAN when tot_t is a NaN, HF_FLAG_SCALE when it is not > 0.
//
// SECOND BODIES of k_mlp_bwd and k_stats_tile, not template parameters of them: A FIX TO THE BACKWARD RECURSION, ITS
// RESCALING OR AN ESTIMATOR TERM GOES INTO BOTH BODIES.
#pragma once
#include "hf_minlen_post.h"
#include "hf_chunks.h"      // k_mle_tile: load_recs, tile_slow_index, row_ptr (hf_scan.h), StatAccSmall

// the frexp form of a term's factor: mantissa (0 for a zero) and exponent
__device__ __forceinline__ double mle_mant(double v, int& e) { return frexp(v, &e); }

// xi[t][16], p-major (xi[t][p * 4 + s]), for the windows of every chunk; window 0 of a chunk gets zeros
__global__ void __launch_bounds__(64) k_mle_bwd(const int64_t* __restrict__ off, const uint32_t* __restrict__ rec,
                                                const DevParams* __restrict__ P, const double2* __restrict__ rows, int m0, int m1, int m2,
                                                int m3, const double* __restrict__ F, double* __restrict__ xi, unsigned* __restrict__ flags) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int64_t t0 = off[c], T = off[c + 1] - t0;
    __shared__ double As[64][17];   // column 16: 0, for the lanes past the last one
    __shared__ double Fs[64][64];
    if (T <= 0) return;
    HF_CHAIN_LANE(m0, m1, m2, m3, lane);
    const bool leaves = active && d == m;                  // the lane whose F leaves the state (and stays in it when m == 1)
    const bool selfl = active && d >= 2;                   // the lanes that hold a term of u[s][s] when m > 1

    const DevRegion* __restrict__ Rl = &P->reg[REC_REGION(rec[t0 + T - 1])];
    double B = active ? Rl->trans[s][4] : 0.0;
    B = ldexp(B, -ch_shift(ch_wave_max(B), HF_MLP_TARGET));                // the walk starts at the target exponent as well
    unsigned bad = 0;

    int64_t base = ((T - 1) / 64) * 64;
    double2 nx[8];
    double nf[64];
#pragma unroll
    for (int k = 0; k < 64; k++) nf[k] = 0.0;
    {
        const int n = (int) (T - base);
        if (lane < n) {
#pragma unroll
            for (int k = 0; k < 8; k++) nx[k] = rows[(t0 + base + lane) * 8 + k];
        }
        mlp_load_f(F, t0 + base, n, total, lane, active, nf);
    }
    for (; base >= 0; base -= 64) {
        const int n = (int) ((T - base) < 64 ? (T - base) : 64);
        if (lane < n) {
#pragma unroll
            for (int k = 0; k < 8; k++) { As[lane][2 * k] = nx[k].x; As[lane][2 * k + 1] = nx[k].y; }
            As[lane][16] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < 64; k++) Fs[k][lane] = nf[k];
        if (base >= 64) {                                     // the block before this one: 64 windows
#pragma unroll
            for (int k = 0; k < 8; k++) nx[k] = rows[(t0 + base - 64 + lane) * 8 + k];
            mlp_load_f(F, t0 + base - 64, 64, total, lane, active, nf);
        }
        __syncthreads();
        const double fcross = nf[63];                         // F of the window before this block's first one (base > 0)
        double r0 = As[n - 1][4 * s], r1 = As[n - 1][4 * s + 1], r2 = As[n - 1][4 * s + 2], r3 = As[n - 1][4 * s + 3];
        double rss = As[n - 1][diag];
        for (int q = n - 1; q >= 0; q--) {
            if (base + q == 0) {                              // the chunk's first window: no pair ends here
                if (lane < 16) xi[t0 * 16 + lane] = 0.0;
                break;
            }
            const double a0 = r0, a1 = r1, a2 = r2, a3 = r3, ass = rss;
            const int qn = q > 0 ? q - 1 : 0;
            r0 = As[qn][4 * s]; r1 = As[qn][4 * s + 1]; r2 = As[qn][4 * s + 2]; r3 = As[qn][4 * s + 3];
            rss = As[qn][diag];
            const double fp = !active ? 0.0 : q > 0 ? Fs[q - 1][lane] : fcross;   // F_{t-1} of the lane, t = base + q
            // ---- the pair (t-1, t): the lane's terms in frexp form ----
            const double be0 = ch_readlane(B, ent0), be1 = ch_readlane(B, ent1), be2 = ch_readlane(B, ent2), be3 = ch_readlane(B, ent3);
            int ef, e0, e1, e2, e3, g0, g1, g2, g3, ec, es, eb;
            const double mf = mle_mant(fp, ef);
            const double ma0 = mle_mant(a0, e0), ma1 = mle_mant(a1, e1), ma2 = mle_mant(a2, e2), ma3 = mle_mant(a3, e3);
            const double mb0 = mle_mant(be0, g0), mb1 = mle_mant(be1, g1), mb2 = mle_mant(be2, g2), mb3 = mle_mant(be3, g3);
            const bool k0 = leaves && !(excl && s == 0), k1 = leaves && !(excl && s == 1), k2 = leaves && !(excl && s == 2),
                       k3 = leaves && !(excl && s == 3);
            double o0 = k0 ? (mf * ma0) * mb0 : 0.0, o1 = k1 ? (mf * ma1) * mb1 : 0.0;
            double o2 = k2 ? (mf * ma2) * mb2 : 0.0, o3 = k3 ? (mf * ma3) * mb3 : 0.0;
            const double below = ch_lane_below(fp);
            const double cd = is_sat ? below + fp : below;    // c_d (used by the lanes d >= 2 of a state with m > 1 only)
            const double mc = mle_mant(cd, ec), ms = mle_mant(ass, es), mb = mle_mant(B, eb);
            double sf = selfl ? (mc * ms) * mb : 0.0;
            const int NONE = -(1 << 20);
            const int x0 = o0 > 0.0 ? ef + e0 + g0 : NONE, x1 = o1 > 0.0 ? ef + e1 + g1 : NONE;
            const int x2 = o2 > 0.0 ? ef + e2 + g2 : NONE, x3 = o3 > 0.0 ? ef + e3 + g3 : NONE;
            const int xs = sf > 0.0 ? ec + es + eb : NONE;
            const int et = ch_wave_max(max(max(max(x0, x1), max(x2, x3)), xs));
            o0 = ldexp(o0, max(x0 - et, -2000)); o1 = ldexp(o1, max(x1 - et, -2000));
            o2 = ldexp(o2, max(x2 - et, -2000)); o3 = ldexp(o3, max(x3 - et, -2000));
            sf = ldexp(sf, max(xs - et, -2000));
            // ---- u[p][s]: from the leaving lane of p, or the wave sum of the self terms ----
            double u[16];
            u[0] = ch_readlane(o0, sat0);  u[1] = ch_readlane(o1, sat0);  u[2] = ch_readlane(o2, sat0);  u[3] = ch_readlane(o3, sat0);
            u[4] = ch_readlane(o0, sat1);  u[5] = ch_readlane(o1, sat1);  u[6] = ch_readlane(o2, sat1);  u[7] = ch_readlane(o3, sat1);
            u[8] = ch_readlane(o0, sat2);  u[9] = ch_readlane(o1, sat2);  u[10] = ch_readlane(o2, sat2); u[11] = ch_readlane(o3, sat2);
            u[12] = ch_readlane(o0, sat3); u[13] = ch_readlane(o1, sat3); u[14] = ch_readlane(o2, sat3); u[15] = ch_readlane(o3, sat3);
            if (m0 > 1) u[0] = ch_wave_sum(s == 0 ? sf : 0.0);
            if (m1 > 1) u[5] = ch_wave_sum(s == 1 ? sf : 0.0);
            if (m2 > 1) u[10] = ch_wave_sum(s == 2 ? sf : 0.0);
            if (m3 > 1) u[15] = ch_wave_sum(s == 3 ? sf : 0.0);
            double tot = ((u[0] + u[4]) + u[8]) + u[12];
            tot += ((u[1] + u[5]) + u[9]) + u[13];
            tot += ((u[2] + u[6]) + u[10]) + u[14];
            tot += ((u[3] + u[7]) + u[11]) + u[15];
            if (tot != tot) bad |= HF_FLAG_NAN;
            else if (!(tot > 0.0)) bad |= HF_FLAG_SCALE;
            double mine = u[0];
#pragma unroll
            for (int i = 1; i < 16; i++) mine = lane == i ? u[i] : mine;
            if (lane < 16) xi[(t0 + base + q) * 16 + lane] = mine / tot;
            // ---- the step back over A of window base + q: step T - (base + q), counted from the chunk's last window ----
            const bool rs = ((T - (base + q)) % HF_MLP_RENORM) == 0;
            const double mx = rs ? ch_wave_max(B) : 0.0;
            const double w0 = a0 * be0, w1 = a1 * be1, w2 = a2 * be2, w3 = a3 * be3;
            // (mirrored: the saturated lane leaves to no q == s)
            const double out = (((excl && s == 0 ? 0.0 : w0) + (excl && s == 1 ? 0.0 : w1)) + (excl && s == 2 ? 0.0 : w2)) +
                               (excl && s == 3 ? 0.0 : w3);
            const double up = ass * ch_lane_above(B), stay = excl ? ass * B : 0.0;
            B = !active ? 0.0 : inner ? up : stay + out;
            if (rs) B = ldexp(B, -ch_shift(mx, HF_MLP_TARGET));
        }
        __syncthreads();
    }
    if (bad) atomicOr(flags, bad);
}

// k_stats_tile's body (hf_chunks.h) with the four counts of a column, count / terminationProb there, read from xi_adm: statistics of the
// pairs of one tile per wavefront, lane l owns the pairs that END at its L windows; the emission row and the collapsed state's component
// rows come from this call's tables (k_tables); the same accumulators in the same places, summed over the lanes in the same order.
// No transition tables are staged: xi_adm holds them already.
template <int KT>
__global__ void __launch_bounds__(256, 2) k_mle_tile(int ntiles, const TileDesc* __restrict__ td, const uint32_t* __restrict__ rec,
                                                     const RowSrc S, const DevParams* __restrict__ P, const double* __restrict__ xi,
                                                     const uint64_t* __restrict__ regmask, double* __restrict__ tile_stats) {
    constexpr int NA = 16 + 9 + 2 + 3 * KT + 1;
    constexpr int NS = 16 + 9 + 2;                  // scalar accumulators kept in registers
    constexpr int L = HF_SCAN_L;
    extern __shared__ __attribute__((aligned(16))) double s_tab[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = blockIdx.x * (blockDim.x >> 6) + wave;
    if (tile >= ntiles) return;
    constexpr int RS = 65;
    const int nrows = 3 * P->ncomp[3] > NS + 1 ? 3 * P->ncomp[3] : NS + 1;
    double* __restrict__ s_row = s_tab + wave * (nrows * RS);
    double* __restrict__ s_acc = s_row + lane;
    const TileDesc d = td[tile];
    const int64_t t0 = d.t0, T = d.T, base = d.base;
    const bool te = hf_err_is_truncexp(P);
    const int ncol = P->ncomp[3], nreg = P->n_regions;
    const int64_t a0 = base + (int64_t) lane * L;   // this lane owns windows a0..a0+L-1 and the pairs ending there
    uint32_t rr[L + 1];                             // rr[j+1] = window a0+j, rr[0] = the window before
    rr[0] = load_recs<L>(rec, t0, T, a0, lane, rr + 1);
    int sidx[L];
    tile_slow_index<L>(rr + 1, lane, d.slow0, sidx);
    bool ok[L];
    unsigned long long present = 0;
#pragma unroll
    for (int j = 0; j < L; j++) {
        const int64_t w = a0 + j;                             // pair (w-1, w), w = 2..T-1  (hmm.c:638-642)
        ok[j] = w >= 2 && w <= T - 1;
        if (ok[j]) present |= 1ull << (REC_REGION(rr[j + 1]) & 63u);
    }
    for (int o = 32; o > 0; o >>= 1) present |= __shfl_xor(present, o);
    const unsigned long long in_chunk = regmask[d.chunk];
    double xa[4], om[4];
    for (int r = 0; r < nreg; r++) {
        if (!((in_chunk >> r) & 1ull)) continue;   // k_chunk_stats never reads this slot
        double* __restrict__ dst = tile_stats + ((int64_t) tile * nreg + r) * NA;
        if (!((present >> r) & 1ull)) {            // region occurs in the chunk but not in this tile
            for (int i = lane; i < NA; i += 64) dst[i] = 0.0;
            continue;
        }
        const DevRegion* __restrict__ R = &P->reg[r];
        StatAccSmall a;
#pragma unroll
        for (int i = 0; i < NS; i++) reinterpret_cast<double*>(&a)[i] = 0.0;
        double c_wden = 0.0;
        for (int i = 0; i < 3 * ncol; i++) s_acc[i * RS] = 0.0;
#pragma unroll 1
        for (int j = 0; j < L; j++) {
            if (!(ok[j] && (int) REC_REGION(rr[j + 1]) == r)) continue;
            double Ev[16], X[16];
            load_row(row_ptr(S, rr[j + 1], rr[j], sidx[j]), Ev);
            load_row(reinterpret_cast<const double2*>(xi + (t0 + a0 + j) * 16), X);   // p-major: X[p * 4 + s]
            const unsigned xw = REC_X(rr[j + 1]), xp = REC_X(rr[j]);
            const double2* __restrict__ crow = crow_ptr(S, rr[j + 1], rr[j], sidx[j]);
            const double x = (double) xw, px = (double) xp;
            double adj3[4];
            bool okc = true;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                double adj[4];
#pragma unroll
                for (int p = 0; p < 4; p++) adj[p] = X[p * 4 + s];           // xi_adm in the place of count / terminationProb
#pragma unroll
                for (int p = 0; p < 4; p++) a.trans[p * 4 + s] += adj[p];   // hmm_utils.c:2010-2015
                if (s == 3) {
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        adj3[p] = adj[p];
                        okc &= Ev[HF_PS(p, 3)] != 0.0 && div_operand_safe(Ev[HF_PS(p, 3)]) && div_operand_safe(adj[p]);
                    }
                } else if (s == 0 && te) {                    // hmm_utils.c:1027-1034
#pragma unroll
                    for (int p = 0; p < 4; p++) { a.te_num += adj[p] * x; a.te_den += adj[p]; }
                } else {                                      // hmm_utils.c:812-839, one component
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        const int k = HF_PS(p, s);
                        const double alpha = P->alpha[p * 4 + s];
                        const double x_adj = alpha == 0.0 ? x : divp(x - alpha * px, prediv(1.0 - alpha));
                        const double w = Ev[k] == 0.0 ? __builtin_nan("") : adj[p];
                        a.g_mnum[s] += w * x_adj;
                        const double z = (x_adj - R->mean[s][0]) * (1.0 - alpha);
                        a.g_vnum[s] += w * z * z;
                        a.g_den[s] += w;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            const bool col_fast = __all(okc);
            // collapsed state, component-major: one 32-byte row per component serves all four pre states
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const double alpha = P->alpha[p * 4 + 3];
                xa[p] = alpha == 0.0 ? x : divp(x - alpha * px, prediv(1.0 - alpha));
                om[p] = 1.0 - alpha;
            }
            if (col_fast) {   // w = adj3 * pc / E3 with the four reciprocals of E3 prepared once for all components
                PreDiv e3[4];
#pragma unroll
                for (int p = 0; p < 4; p++) e3[p] = prediv(Ev[HF_PS(p, 3)]);
#pragma unroll 1
                for (int cc = 0; cc < ncol; cc++) {
                    const double2 u01 = crow[cc * 2], u23 = crow[cc * 2 + 1];
                    const double mu = R->mean[3][cc];
                    double mnum = s_acc[cc * RS], vnum = s_acc[(ncol + cc) * RS], den = s_acc[(2 * ncol + cc) * RS];
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        const double pc = p == 0 ? u01.x : p == 1 ? u01.y : p == 2 ? u23.x : u23.y;   // [component][previous state]
                        const double w = divp(adj3[p] * pc, e3[p]);
                        mnum += w * xa[p];
                        const double z = (xa[p] - mu) * om[p];
                        vnum += w * z * z;
                        den += w;
                        c_wden += w;
                    }
                    s_acc[cc * RS] = mnum; s_acc[(ncol + cc) * RS] = vnum; s_acc[(2 * ncol + cc) * RS] = den;
                }
            } else {
#pragma unroll 1
                for (int cc = 0; cc < ncol; cc++) {
                    const double2 u01 = crow[cc * 2], u23 = crow[cc * 2 + 1];
                    const double mu = R->mean[3][cc];
                    double mnum = s_acc[cc * RS], vnum = s_acc[(ncol + cc) * RS], den = s_acc[(2 * ncol + cc) * RS];
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        const double pc = p == 0 ? u01.x : p == 1 ? u01.y : p == 2 ? u23.x : u23.y;
                        const double w = adj3[p] * pc / Ev[HF_PS(p, 3)];
                        mnum += w * xa[p];
                        const double z = (xa[p] - mu) * om[p];
                        vnum += w * z * z;
                        den += w;
                        c_wden += w;
                    }
                    s_acc[cc * RS] = mnum; s_acc[(ncol + cc) * RS] = vnum; s_acc[(2 * ncol + cc) * RS] = den;
                }
            }
        }
        // sum over the 64 lanes in lane order: accumulator i is summed by lane i out of its LDS row (fixed order),
        // results stored in StatAcc<KT> order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        {
            double v = 0.0;
            if (lane < 3 * ncol) {
                const double* __restrict__ row = s_row + lane * RS;
#pragma unroll 8
                for (int l = 0; l < 64; l++) v += row[l];
            }
            for (int i = lane; i < 3 * KT; i += 64) dst[NS + i] = 0.0;       // slots of components >= ncol
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane < 3 * ncol) dst[NS + (lane / ncol) * KT + (lane % ncol)] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int i = 0; i < NS; i++) s_acc[i * RS] = reinterpret_cast<double*>(&a)[i];
        s_acc[NS * RS] = c_wden;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane <= NS) {
            const double* __restrict__ row = s_row + lane * RS;
            double v = 0.0;
#pragma unroll 8
            for (int l = 0; l < 64; l++) v += row[l];
            dst[lane < NS ? lane : NS + 3 * KT] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}
