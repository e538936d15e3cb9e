// hf_minlen_post_joined.h — the sum-product walks over groups of joined chunks: k_mlpj_fwd and k_mlpj_bwd, the walks of
// hf_minlen_posterior_joined (and, the forward one alone, of hf_sample_paths_minlen_joined), and k_mlsj_bound, which draws the words of
// the joined chunk-first windows for the sampler.  The rule is hf_viterbi_minlen_joined's in (+, x): the joined call on (chunk list,
// joined) is the per-chunk call on the list in which each group's first chunk holds the group's whole window range and its other chunks
// hold no windows, with the row of every joined chunk-first window t (first window of chunk c, joined to c - 1) replaced by
//     J_t[p][s] = end_{c-1}[p] * first_c[s]        end_{c-1}[p] = trans[r_{t-1}][p][4], first_c[s] = row pre = 0 of the chunk-first row
// formed first as one double and then used like any A_t[p][s]; `end` is taken at the group's last window.  include/hmm_flagger_hip.h has
// the definition in full.
//
// LAUNCH.  The kernels take the GROUP-AS-CHUNK offsets goff[C + 1]: goff[c] = off[c] for the first chunk of a group, the group's end for
// its other chunks, so the first chunk's range is the group's and the others are empty.  A block is a chunk of that list: the output
// index is the chunk index, and k_mls_final / k_mls_back of hf_minlen_sample.h are launched over goff unchanged (the final lane of a
// group draws with uniform index n_windows + its FIRST chunk).  k_mls_draw stays as it is and skips every chunk-first window;
// k_mlsj_bound fills in the joined ones.
//
// SECOND BODIES.  k_mlpj_fwd and k_mlpj_bwd are k_mlp_fwd and k_mlp_bwd (hf_minlen_post.h) with one change each, the staging lane of a
// joined chunk-first window writes J_t into the LDS tile before the barrier (k_mlvj_fwd does the same in logs); the per-window loops,
// every sum order, ch_wave_sum's tree, the rescaling (at a walk's first vector and after every HF_MLP_RENORM-th step, counted from the
// GROUP's first window forward and last window backward) and the frexp form of the products F_t B_t are theirs, so a group of one chunk
// gives k_mlp_fwd's and k_mlp_bwd's bits.  They are second bodies and not a template parameter of the first: DESIGN.md 7k-m measured
// what a shared template did to k_mlv_fwd.  A FIX TO A SUM ORDER OR TO THE RESCALING THEREFORE GOES INTO BOTH BODIES (hf_minlen_post.h
// says the same).  No rescaling is added at a joined boundary: J_t is a transition probability times first[s], the size of any row,
// and a period passes at most nine rows as before.
// Flags: HF_FLAG_NAN also for a NaN in an end column read at a joined boundary (the forward staging lane raises it).
//
// In hf_minlen.hip this file stands behind hf_mea.h and in front of hf_minlen_em.h and hf_minlen_joined.h, its place since it was added:
// there no kernel of the family moved (profiles/minlen_post_joined_asm.txt, profiles/split_units_asm.txt).
#pragma once
#include "hf_minlen_post.h"
#include "hf_minlen_sample.h"

// the tile row of a joined chunk-first window: J_t[p][s] = end[p] of the region of the window before it times first[s] (row pre = 0)
__device__ __forceinline__ unsigned mlpj_stage(double* __restrict__ As_row, const DevRegion* __restrict__ Rp, double f0, double f1, double f2,
                                               double f3) {
    unsigned bad = 0;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const double e = Rp->trans[p][4];
        if (e != e) bad |= HF_FLAG_NAN;
        As_row[4 * p] = e * f0; As_row[4 * p + 1] = e * f1; As_row[4 * p + 2] = e * f2; As_row[4 * p + 3] = e * f3;
    }
    return bad;
}

// lz[0][c] = log Z_adm, lz[1][c] = log Z of the group whose first chunk is c (0 for the other chunks); F[t][lane] as k_mlp_fwd
__global__ void __launch_bounds__(64) k_mlpj_fwd(int C, const int64_t* __restrict__ goff, const uint32_t* __restrict__ rec,
                                                 const DevParams* __restrict__ P, const double2* __restrict__ rows, int m0, int m1, int m2,
                                                 int m3, double* __restrict__ F, double* __restrict__ lz, unsigned* __restrict__ flags) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const bool plain = blockIdx.y == 1;
    const int64_t t0 = goff[c], T = goff[c + 1] - t0;
    __shared__ ChainTile As;
    if (T <= 0) { if (lane == 0) lz[(int64_t) blockIdx.y * C + c] = 0.0; return; }
    const int stride = m0 + m1 + m2 + m3;
    if (plain) m0 = m1 = m2 = m3 = 1;
    HF_CHAIN_LANE(m0, m1, m2, m3, lane);

    double x = 0.0;
    long long E = 0;
    double2 nx[8];
    uint32_t nr = 0;                                        // the record of the window whose row waits in nx
    unsigned bad = 0;
    if (lane < T) {
#pragma unroll
        for (int k = 0; k < 8; k++) nx[k] = rows[(t0 + lane) * 8 + k];
        nr = rec[t0 + lane];
    }
    for (int64_t base = 0; base < T; base += 64) {
        const int n = (int) ((T - base) < 64 ? (T - base) : 64);
        if (lane < n) {
            if (base + lane > 0 && REC_FIRST(nr)) {
                bad |= mlpj_stage(&As[lane][0], &P->reg[REC_REGION(rec[t0 + base + lane - 1])], nx[0].x, nx[0].y, nx[1].x, nx[1].y);
            } else {
#pragma unroll
                for (int k = 0; k < 8; k++) { As[lane][2 * k] = nx[k].x; As[lane][2 * k + 1] = nx[k].y; }
            }
            As[lane][16] = 0.0;
        }
        if (base + 64 + lane < T) {
#pragma unroll
            for (int k = 0; k < 8; k++) nx[k] = rows[(t0 + base + 64 + lane) * 8 + k];
            nr = rec[t0 + base + 64 + lane];
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

    // the end: the wave sum of x * end[s], end of the group's last window
    const DevRegion* __restrict__ Rl = &P->reg[REC_REGION(rec[t0 + T - 1])];
    const double e = active ? Rl->trans[s][4] : 0.0;
    if (e != e) bad |= HF_FLAG_NAN;
    const double z = ch_wave_sum(active ? x * e : 0.0);
    if (z != z) bad |= HF_FLAG_NAN;
    else if (!(z > 0.0)) bad |= HF_FLAG_SCALE;
    if (lane == 0) lz[(int64_t) blockIdx.y * C + c] = log(z) + (double) E * 0.69314718055994530942;
    if (bad) atomicOr(flags, bad);
}

__global__ void __launch_bounds__(64) k_mlpj_bwd(const int64_t* __restrict__ goff, const uint32_t* __restrict__ rec,
                                                 const DevParams* __restrict__ P, const double2* __restrict__ rows, int m0, int m1, int m2,
                                                 int m3, const double* __restrict__ F, double* __restrict__ post, int8_t* __restrict__ label,
                                                 unsigned* __restrict__ flags) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int64_t t0 = goff[c], T = goff[c + 1] - t0;
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
    uint32_t nr = 0, npr = 0;       // the records of the window whose row waits in nx and of the window before it
    double nf[64];
#pragma unroll
    for (int k = 0; k < 64; k++) nf[k] = 0.0;
    {
        const int n = (int) (T - base);
        if (lane < n) {
#pragma unroll
            for (int k = 0; k < 8; k++) nx[k] = rows[(t0 + base + lane) * 8 + k];
            nr = rec[t0 + base + lane];
            if (base + lane > 0) npr = rec[t0 + base + lane - 1];
        }
        mlp_load_f(F, t0 + base, n, total, lane, active, nf);
    }
    for (; base >= 0; base -= 64) {
        const int n = (int) ((T - base) < 64 ? (T - base) : 64);
        if (lane < n) {
            if (base + lane > 0 && REC_FIRST(nr)) {
                // a joined chunk-first window: the lanes read their rows J_t[s][.] out of the same tile (a NaN in the end column is the
                // forward walk's to flag)
                (void) mlpj_stage(&As[lane][0], &P->reg[REC_REGION(npr)], nx[0].x, nx[0].y, nx[1].x, nx[1].y);
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
            nr = rec[t0 + base - 64 + lane];
            npr = base - 64 + lane > 0 ? rec[t0 + base - 64 + lane - 1] : 0u;
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
            // window base + q: g[s], the posterior and its first largest entry (the frexp form of k_mlp_bwd)
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
            if (base + q == 0) break;                         // (the group's first window: the walk stops nowhere else)
            // the step back over A of window base + q: step T - (base + q), counted from the group's last window
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

// The words of the joined chunk-first windows bound[0 .. gridDim.x): one block per window, threads over samples.  Thread 0 forms the
// 16 + 8 weights and their cumulative sums ONCE, by k_mls_draw's operations with A_t := J_t; then every thread draws its samples' words
// with uniform index t, k_mls_draw's word format, one 16-bit store each.
__global__ void __launch_bounds__(256) k_mlsj_bound(const int64_t* __restrict__ bound, const uint32_t* __restrict__ rec,
                                                    const DevParams* __restrict__ P, const double2* __restrict__ rows, int m0, int m1, int m2,
                                                    int m3, const double* __restrict__ F, const uint64_t* __restrict__ keys, int K, int Kp,
                                                    uint16_t* __restrict__ words) {
    const int64_t t = bound[blockIdx.x];                    // (>= 1: a joined chunk has a predecessor with windows)
    __shared__ double W[16], Cm[16], w1[4], c0[4], c1[4];
    HF_CHAIN_LENS(m0, m1, m2, m3);
    if (threadIdx.x == 0) {
        const double* __restrict__ Fp = F + (t - 1) * total;
        // the four saturated lanes of window t-1 and the lanes below them, scaled by the largest of the eight
        double fs[4], fb[4];
        fs[0] = Fp[sat0]; fs[1] = Fp[sat1]; fs[2] = Fp[sat2]; fs[3] = Fp[sat3];
        fb[0] = m0 > 1 ? Fp[sat0 - 1] : 0.0; fb[1] = m1 > 1 ? Fp[sat1 - 1] : 0.0;
        fb[2] = m2 > 1 ? Fp[sat2 - 1] : 0.0; fb[3] = m3 > 1 ? Fp[sat3 - 1] : 0.0;
        double mx = 0.0;
#pragma unroll
        for (int p = 0; p < 4; p++) mx = fmax(mx, fmax(fs[p], fb[p]));
        const int e = (mx > 0.0 && !isinf(mx)) ? ilogb(mx) : 0;
#pragma unroll
        for (int p = 0; p < 4; p++) { fs[p] = ldexp(fs[p], -e); fb[p] = ldexp(fb[p], -e); }
        // J_t[p][s] = end[p] * first[s], each one double before it meets F
        const DevRegion* __restrict__ Rp = &P->reg[REC_REGION(rec[t - 1])];
        const double2 fa = rows[t * 8], fc = rows[t * 8 + 1];
        const double f[4] = {fa.x, fa.y, fc.x, fc.y};
        double A[16];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const double en = Rp->trans[p][4];
#pragma unroll
            for (int s = 0; s < 4; s++) A[p * 4 + s] = en * f[s];
        }
        // entry lanes, without the excluded p == s; saturated lanes: arrived, stayed
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const bool excl = ch_len(mpack, s) > 1;
            double c = 0.0;
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const double w = (excl && p == s) ? 0.0 : fs[p] * A[p * 4 + s];
                c = p == 0 ? w : c + w;
                W[s * 4 + p] = w;
                Cm[s * 4 + p] = c;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const double a = fb[s] * A[5 * s], b = fs[s] * A[5 * s];
            c0[s] = a;
            w1[s] = b;
            c1[s] = a + b;
        }
    }
    __syncthreads();
    const unsigned smask = (m0 > 1 ? 1u : 0u) | (m1 > 1 ? 2u : 0u) | (m2 > 1 ? 4u : 0u) | (m3 > 1 ? 8u : 0u);
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const double u = smp_uniform(keys[k], (uint64_t) t);
        unsigned w = smp_byte(W, Cm, u);
#pragma unroll
        for (int s = 0; s < 4; s++) w |= mls_pick2(w1[s], c0[s], c1[s], u) << (8 + s);
        words[t * Kp + k] = (uint16_t) (w & (0xffu | smask << 8));
    }
}
