// hf_minlen_em_joined.h — the E-step under minimum run lengths over groups of joined chunks (hf_estep_minlen_joined): k_mlej_bwd, the
// backward walk that leaves the pair posterior xi_adm of a group.  The rule is hf_minlen_posterior_joined's: the joined call on (chunk
// list, joined) is hf_estep_minlen's definition on the group-as-chunk list (hf_minlen_post_joined.h: LAUNCH), with the row of every
// joined chunk-first window t replaced by
//     J_t[p][s] = end_{c-1}[p] * first_c[s]
// formed first as one double (mlpj_stage) and then used like any A_t[p][s]: in the step back AND in the terms of the pair (t-1, t), so
// xi_adm of a joined chunk-first window is the boundary pair's and only a GROUP's first window holds zeros.  k_mlpj_fwd leaves F, log
// Z_adm and log Z of the groups; k_mle_tile, k_chunk_stats and k_reduce run as they are over the track's own tile plan, which never
// holds a boundary pair.  include/hmm_flagger_hip.h has the definition in full.
//
// SECOND BODY.  k_mlej_bwd is k_mle_bwd (hf_minlen_em.h) line for line over goff, with one change: the staging lane of a joined
// chunk-first window writes J_t into the LDS tile before the barrier, exactly as k_mlpj_bwd does.  The per-window loop, every sum order,
// the frexp form of a term and the rescaling (at the walk's first vector and after every HF_MLP_RENORM-th step, counted from the GROUP's
// last window) are k_mle_bwd's and k_mlpj_bwd's, so a group of one chunk gives k_mle_bwd's bits.  It is a second body and not a template
// parameter of the first: A FIX TO THE BACKWARD RECURSION, ITS RESCALING OR A TERM'S FREXP FORM GOES INTO k_mle_bwd,
// k_mlpj_bwd AND THIS ONE.
// Unlike k_mlpj_bwd it carries no record words beside the prefetched row: k_mle_bwd leaves no register for them.  The staging lane loads
// rec[t] and rec[t-1] where it stages, once per 64 windows, off the per-window chain.
// The pair across a 64-window block boundary takes F_{t-1} from the prefetched block (fcross) and A_t from lane 0's tile row; when that
// window is a joined chunk-first one the tile row is J_t, so the two meet without a case of their own.
//
// In hf_minlen.hip this file stands behind hf_minlen_em.h and in front of hf_minlen_joined.h: there no kernel of the family moved
// (profiles/minlen_em_joined_asm.txt).
#pragma once
#include "hf_minlen_em.h"
#include "hf_minlen_post_joined.h"      // mlpj_stage

// xi[t][16], p-major, for the windows of every group; window 0 of a group gets zeros, a joined chunk-first window the boundary pair
__global__ void __launch_bounds__(64) k_mlej_bwd(const int64_t* __restrict__ goff, const uint32_t* __restrict__ rec,
                                                 const DevParams* __restrict__ P, const double2* __restrict__ rows, int m0, int m1, int m2,
                                                 int m3, const double* __restrict__ F, double* __restrict__ xi, unsigned* __restrict__ flags) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int64_t t0 = goff[c], T = goff[c + 1] - t0;
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
            if (base + lane > 0 && REC_FIRST(rec[t0 + base + lane])) {
                // a joined chunk-first window: the lanes read their rows J_t[s][.] out of the same tile (a NaN in the end column is the
                // forward walk's to flag)
                (void) mlpj_stage(&As[lane][0], &P->reg[REC_REGION(rec[t0 + base + lane - 1])], nx[0].x, nx[0].y, nx[1].x, nx[1].y);
            } else {
#pragma unroll
                for (int k = 0; k < 8; k++) { As[lane][2 * k] = nx[k].x; As[lane][2 * k + 1] = nx[k].y; }
            }
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
            if (base + q == 0) {                              // the group's first window: no pair ends here
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
            // ---- the step back over A of window base + q: step T - (base + q), counted from the group's last window ----
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
