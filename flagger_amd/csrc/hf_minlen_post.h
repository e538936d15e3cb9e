// hf_minlen_post.h — posteriors under minimum run lengths (hf_minlen_posterior): the sum-product twin of hf_minlen.h.  Over the expanded
// chain of hf_viterbi_minlen (hf_chain.h: lanes (s, d), saturated and entry lanes) one forward and one backward walk give, per chunk,
// the weight Z_adm of the admissible paths, the weight Z of all paths, and per window the label probabilities given that the path is
// admissible.  A decoder beside hf_viterbi_minlen: the same first, A_t and end, buffers of its own, ONE code path for both kinds of context (linear rows in window order, k_dec_rows_win).
//
// Definition (include/hmm_flagger_hip.h has it in full), m = min_len[s]:
//   F_0[(s, m)] = first[s], 0 elsewhere
//   F_t[(s, 1)]  = ((v_0 + v_1) + v_2) + v_3, v_p = F_{t-1}[(p, m_p)] * A_t[p][s], v_s replaced by 0 when m > 1
//   F_t[(s, d)]  = F_{t-1}[(s, d-1)] * A_t[s][s]                                              1 < d < m
//   F_t[(s, m)]  = F_{t-1}[(s, m-1)] * A_t[s][s] + F_{t-1}[(s, m)] * A_t[s][s]                 m > 1
//   B_{T-1}[(s, d)] = end[s]
//   B_{t-1}[(s, d)] = A_t[s][s] * B_t[(s, d+1)]                                                d < m
//   B_{t-1}[(s, m)] = stay + (((w_0 + w_1) + w_2) + w_3), w_q = A_t[s][q] * B_t[(q, 1)], w_s replaced by 0 when m > 1;
//                     stay = A_t[s][s] * B_t[(s, m)] when m > 1, else 0
//   Z_adm = the wave sum of F_{T-1}[lane] * end[s(lane)];  g_t[s] = the wave sum of F_t[lane] * B_t[lane] * 2^-e_t over the lanes of
//   state s, e_t the window's largest exponent sum of a lane's two factors (below)
//   post[t][s] = g_t[s] / (((g_t[0] + g_t[1]) + g_t[2]) + g_t[3])
// Every wave sum is ch_wave_sum (hf_chain.h, where its one order is written down) with 0 in the lanes that do not take part.
//
// NUMERICS.  Linear domain, the scheme of hf_longrun.h: value = x * 2^E with one integer exponent sum E per walk.  A rescaling with the
// largest lane mx: e = ilogb(mx) - HF_MLP_TARGET (0 when mx is 0 or not finite), every lane is scaled by 2^-e and E += e.  It happens
// (a) at the walk's first vector, F_0 (forward) or B_{T-1} (backward), with mx its largest lane, before anything is stored or stepped, and
// (b) after every HF_MLP_RENORM-th step, counted from the chunk's first window (forward) or last window (backward), with mx the
// largest lane BEFORE that step.  So the largest lane is at exponent 300 at the start of every period of eight steps, the first one
// included (first[s] alone can sit at 1e-40), and between two rescalings it passes at most nine rows: emission floors of 1e-40 leave
// nine steps from exponent 300 normal (1e-360 * 2^300 = 2e-270).  log Z_adm = log(wave sum) + E ln 2.  post is a ratio within one
// window: the scales of F_t and B_t cancel, and the backward walk keeps no exponent.  THE PRODUCTS F_t B_t: at a window F_t and B_t are
// each somewhere in their own period, so the largest product can be as small as 2^600 * 1e-720; a lane's product is therefore formed as
// frexp-mantissa(F) * frexp-mantissa(B) * 2^(e_lane - e_t), e_lane the sum of the two frexp exponents, e_t the largest e_lane over the
// lanes with a non-zero product (an integer maximum over the wavefront): the largest term of a window is in [1/4, 1).
// Flags: HF_FLAG_NAN on a NaN in a row (k_dec_rows_win), in the end column or in a chunk's sum; HF_FLAG_SCALE when Z_adm or Z of a chunk
// is not > 0, or a window's g_t sum to nothing.
//
// k_mlp_fwd: grid (C, 2), one 64-lane workgroup per chunk and chain; blockIdx.y == 1 walks the chain with all four lengths 1 over the same
// rows with the same operations (lanes 0..3) and leaves log Z, it stores no F.  The staging of hf_chain.h with 0 as the pad; the four
// saturated lanes by readlane at uniform indices, the lane below by DPP.  Every lane stores its F_t at [t][lane], row stride sum(min_len).
// k_mlp_bwd: one 64-lane workgroup per chunk walks back with B in registers: the lane above by DPP, the four entry lanes by readlane, a
// lane reads its row A[s][0..3] and A[s][s]; F_t comes back 64 windows at a time through LDS (the block before is in registers while this
// one is walked).  Lanes 0..3 write post[t][lane]; lane q keeps the label of the block's window q for one store.
//
// SECOND BODIES.  hf_minlen_post_joined.h holds k_mlpj_fwd and k_mlpj_bwd, these two walks over groups of joined chunks
// (hf_minlen_posterior_joined, hf_sample_paths_minlen_joined): copies with another staging of the tile, not a template parameter of
// these kernels (what a shared template did to k_mlv_fwd).  A FIX TO A SUM ORDER OR TO THE RESCALING THEREFORE GOES INTO
// BOTH BODIES: a group of one chunk must give these kernels' bits.
#pragma once
#include "hf_chain.h"

#define HF_MLP_RENORM 8         // steps between rescalings
#define HF_MLP_TARGET 300       // exponent the largest lane is brought to

// lz[0][c] = log Z_adm, lz[1][c] = log Z; F[t][lane] for the windows of every chunk (row stride: the sum of the four lengths)
__global__ void __launch_bounds__(64) k_mlp_fwd(int C, const int64_t* __restrict__ off, const uint32_t* __restrict__ rec,
                                                const DevParams* __restrict__ P, const double2* __restrict__ rows, int m0, int m1, int m2,
                                                int m3, double* __restrict__ F, double* __restrict__ lz, unsigned* __restrict__ flags) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const bool plain = blockIdx.y == 1;
    const int64_t t0 = off[c], T = off[c + 1] - t0;
    __shared__ ChainTile As;
    if (T <= 0) { if (lane == 0) lz[(int64_t) blockIdx.y * C + c] = 0.0; return; }
    const int stride = m0 + m1 + m2 + m3;
    if (plain) m0 = m1 = m2 = m3 = 1;
    HF_CHAIN_LANE(m0, m1, m2, m3, lane);

    double x = 0.0;
    long long E = 0;
    double2 nx[8];
    if (lane < T) {
#pragma unroll
        for (int k = 0; k < 8; k++) nx[k] = rows[(t0 + lane) * 8 + k];
    }
    for (int64_t base = 0; base < T; base += 64) {
        const int n = (int) ((T - base) < 64 ? (T - base) : 64);
        if (lane < n) {
#pragma unroll
            for (int k = 0; k < 8; k++) { As[lane][2 * k] = nx[k].x; As[lane][2 * k + 1] = nx[k].y; }
            As[lane][16] = 0.0;
        }
        if (base + 64 + lane < T) {
#pragma unroll
            for (int k = 0; k < 8; k++) nx[k] = rows[(t0 + base + 64 + lane) * 8 + k];
        }
        __syncthreads();
        const int q0 = base == 0 ? 1 : 0;
        // window 0: first[s] (row pre = 0 of the chunk-first row) in every state's saturated lane
        if (base == 0) {
            if (active && d == m) x = As[0][s];
            const int e0 = ch_shift(ch_wave_max(x), HF_MLP_TARGET);        // the walk starts at the target exponent as well
            x = ldexp(x, -e0);
            E += e0;
            if (!plain && active) F[t0 * stride + lane] = x;
        }
        double c0, c1, c2, c3, css;
        c0 = As[q0][s]; c1 = As[q0][4 + s]; c2 = As[q0][8 + s]; c3 = As[q0][12 + s]; css = As[q0][diag];
        for (int q = q0; q < n; q++) {
            const double a0 = c0, a1 = c1, a2 = c2, a3 = c3, ass = css;
            c0 = As[q + 1][s]; c1 = As[q + 1][4 + s]; c2 = As[q + 1][8 + s]; c3 = As[q + 1][12 + s]; css = As[q + 1][diag];
            const bool rs = ((base + q) % HF_MLP_RENORM) == 0;      // (uniform) the step into window base + q is step base + q
            const double mx = rs ? ch_wave_max(x) : 0.0;
            const double v0 = ch_readlane(x, sat0) * a0, v1 = ch_readlane(x, sat1) * a1;
            const double v2 = ch_readlane(x, sat2) * a2, v3 = ch_readlane(x, sat3) * a3;
            const double ent = (((excl && s == 0 ? 0.0 : v0) + (excl && s == 1 ? 0.0 : v1)) + (excl && s == 2 ? 0.0 : v2)) +
                               (excl && s == 3 ? 0.0 : v3);
            const double up = ch_lane_below(x) * ass, stay = x * ass;
            x = is_entry ? ent : is_sat ? up + stay : active ? up : 0.0;
            if (rs) {
                const int e = ch_shift(mx, HF_MLP_TARGET);
                x = ldexp(x, -e);
                E += e;
            }
            if (!plain && active) F[(t0 + base + q) * stride + lane] = x;
        }
        __syncthreads();
    }

    // the end: the wave sum of x * end[s]
    const DevRegion* __restrict__ Rl = &P->reg[REC_REGION(rec[t0 + T - 1])];
    const double e = active ? Rl->trans[s][4] : 0.0;
    unsigned bad = e != e ? HF_FLAG_NAN : 0u;
    const double z = ch_wave_sum(active ? x * e : 0.0);
    if (z != z) bad |= HF_FLAG_NAN;
    else if (!(z > 0.0)) bad |= HF_FLAG_SCALE;
    if (lane == 0) lz[(int64_t) blockIdx.y * C + c] = log(z) + (double) E * 0.69314718055994530942;
    if (bad) atomicOr(flags, bad);
}

// F of the windows base .. base + n - 1 of a chunk, the lane's column: nf[k] = F[base + k][lane], windows past the last one repeat it
__device__ __forceinline__ void mlp_load_f(const double* __restrict__ F, int64_t w0, int n, int stride, int lane, bool active, double nf[64]) {
    if (!active) return;
#pragma unroll
    for (int k = 0; k < 64; k++) nf[k] = F[(w0 + (k < n ? k : n - 1)) * stride + lane];
}

__global__ void __launch_bounds__(64) k_mlp_bwd(const int64_t* __restrict__ off, const uint32_t* __restrict__ rec,
                                                const DevParams* __restrict__ P, const double2* __restrict__ rows, int m0, int m1, int m2,
                                                int m3, const double* __restrict__ F, double* __restrict__ post, int8_t* __restrict__ label,
                                                unsigned* __restrict__ flags) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int64_t t0 = off[c], T = off[c + 1] - t0;
    __shared__ double As[64][17];   // column 16: 0, for the lanes past the last one
    __shared__ double Fs[64][64];
    if (T <= 0) return;
    HF_CHAIN_LANE(m0, m1, m2, m3, lane);

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
        int lab = 0;
        // the lane's row and F of the window BEFORE is read while this one's step runs
        double r0 = As[n - 1][4 * s], r1 = As[n - 1][4 * s + 1], r2 = As[n - 1][4 * s + 2], r3 = As[n - 1][4 * s + 3];
        double rss = As[n - 1][diag], fq = Fs[n - 1][lane];
        for (int q = n - 1; q >= 0; q--) {
            const double a0 = r0, a1 = r1, a2 = r2, a3 = r3, ass = rss, f = fq;
            const int qn = q > 0 ? q - 1 : 0;
            r0 = As[qn][4 * s]; r1 = As[qn][4 * s + 1]; r2 = As[qn][4 * s + 2]; r3 = As[qn][4 * s + 3];
            rss = As[qn][diag]; fq = Fs[qn][lane];
            // window base + q: g[s], the posterior and its first largest entry
            // F_t and B_t are each within their own period of eight steps: the product of the two largest lanes can lie 2^-2400 below
            // 2^600, so the lanes' products are formed from mantissas and brought to the window's largest exponent sum
            int ef, eb;
            const double mf = frexp(f, &ef), mb = frexp(B, &eb);
            const double pm = active ? mf * mb : 0.0;         // 0, or in [1/4, 1)
            const int el = pm > 0.0 ? ef + eb : -(1 << 20);
            const int sh = el - ch_wave_max(el);           // <= 0
            const double fb = ldexp(pm, sh < -2000 ? -2000 : sh);
            const double g0 = ch_wave_sum(s == 0 ? fb : 0.0), g1 = ch_wave_sum(s == 1 ? fb : 0.0);
            const double g2 = ch_wave_sum(s == 2 ? fb : 0.0), g3 = ch_wave_sum(s == 3 ? fb : 0.0);
            const double tot = ((g0 + g1) + g2) + g3;
            if (tot != tot) bad |= HF_FLAG_NAN;
            else if (!(tot > 0.0)) bad |= HF_FLAG_SCALE;
            const int ls = lane & 3;
            const double pl = (ls == 0 ? g0 : ls == 1 ? g1 : ls == 2 ? g2 : g3) / tot;
            if (lane < 4) post[(t0 + base + q) * 4 + lane] = pl;
            const double p0 = ch_readlane(pl, 0), p1 = ch_readlane(pl, 1), p2 = ch_readlane(pl, 2), p3 = ch_readlane(pl, 3);
            double best = p0;
            int arg = 0;
            if (p1 > best) { best = p1; arg = 1; }
            if (p2 > best) { best = p2; arg = 2; }
            if (p3 > best) { best = p3; arg = 3; }
            lab = lane == q ? arg : lab;
            if (base + q == 0) break;
            // the step back over A of window base + q: step T - (base + q), counted from the chunk's last window
            const bool rs = ((T - (base + q)) % HF_MLP_RENORM) == 0;
            const double mx = rs ? ch_wave_max(B) : 0.0;
            const double w0 = a0 * ch_readlane(B, ent0), w1 = a1 * ch_readlane(B, ent1);
            const double w2 = a2 * ch_readlane(B, ent2), w3 = a3 * ch_readlane(B, ent3);
            // (mirrored: the saturated lane leaves to no q == s)
            const double out = (((excl && s == 0 ? 0.0 : w0) + (excl && s == 1 ? 0.0 : w1)) + (excl && s == 2 ? 0.0 : w2)) +
                               (excl && s == 3 ? 0.0 : w3);
            const double up = ass * ch_lane_above(B), stay = excl ? ass * B : 0.0;
            B = !active ? 0.0 : inner ? up : stay + out;
            if (rs) B = ldexp(B, -ch_shift(mx, HF_MLP_TARGET));
        }
        if (lane < n) label[t0 + base + lane] = (int8_t) lab;
        __syncthreads();
    }
    if (bad) atomicOr(flags, bad);
}
