// hf_runlen.hip — the exact block-length spectrum of the C ABI (hf_get_run_lengths, include/hmm_flagger_hip.h), a translation unit of
// its own, kernels and host side: for a window range, a state set S and a length L, the expected number of maximal runs of S of every
// length 1 .. L and of more than L windows, under the model of the last HF_MODE_FULL pass.  Not part of an EM pass: it reads the pass's
// rows, forward and backward vectors (hf_view.h, through pass_view of hf_host.h) and writes buffers of its own only (hf_ctx::rl).
//
// Definition.  Given the data the states of a chunk are a Markov chain, and only ratios of the pass's values are formed:
//   Q_u[p][q]  = A_u[p][q] b_u[q] / sum_q' A_u[p][q'] b_u[q']       the posterior chain, a < u <= b (ch_post_rows of hf_chain.h: the sum
//                                                                   over q' = 0..3 in order; a row whose denominator is 0 is a zero row)
//   sigma_a[s] = f_a[s] b_a[s] / sum_s' f_a[s'] b_a[s']             the start mass of a run at the part's first window a, s in S (ch_post_start)
//   sigma_t[s] = sum_{p not in S} f_{t-1}[p] A_t[p][s] b_t[s] / sum_{p, s'} f_{t-1}[p] A_t[p][s'] b_t[s']    at t > a (both sums over
//                                                                   p, then s', in order; the numerator by a select, never gamma - xi)
// The run started at t walks from v_1 = sigma_t; at age d it stands at window u = t + d - 1.  If u = b it is OPEN at b.  Otherwise
// w = v_d Q_{u+1} (w[q] = ((v[0] Q[0][q] + v[1] Q[1][q]) + v[2] Q[2][q]) + v[3] Q[3][q]); sum_{q not in S} w[q] closes a run of exactly d
// windows, and v_{d+1} = w o 1_S.  A run still in S at age L + 1 adds sum v_{L+1} to bin "> L" and is dropped: it is counted once, where
// it saturates.  Every bin is a sum of non-negative terms.
//
// k_rl_piece<SEQ>  one wavefront per piece of the getters' 512-window job grid (hf_jobs.h).  The expanded state is the run's AGE: lane
//                  d - 1 holds v_d of the run that is d windows old at the current window, so the lane's run started `lane` windows back.
//                  A step into window x: every lane forms w = v Q_x (the 16 entries of Q_x are the same for the wavefront), adds its exit
//                  mass to ITS OWN bin register (the run that started at a: the left-touching bins Lc, else I), lane L - 1 adds what
//                  survives to "> L", every lane takes w o 1_S from the lane below (wave_shr:1, hf_chain.h) and lane 0 takes sigma_x.
//                  Q_x and sigma_x are computed once per window, 64 windows at a time with lane = window, and staged through an LDS tile
//                  (stride 21 doubles: the lanes' rows fall into different banks) that the steps read back as broadcasts; the values of
//                  the next 64 windows wait in registers meanwhile.  A piece that does not start at a + 1 first rebuilds the ages alive
//                  in front of it: the same steps WITHOUT COUNTING over the up to L windows before its first one, none of them earlier
//                  than a (a itself comes in as the left-touching start where the halo reaches it).  A closing or saturating event
//                  belongs to the piece that holds the window x of its step; the piece that holds b writes the lanes' open masses.
//                  A bin is accumulated in window order in one lane: no atomics, no cross-lane sums, one order.
// k_rl_chain<SEQ>  one 64-lane workgroup per part, lane = bin: the pieces' bins summed in piece order, the open masses of the last piece
//                  (the whole part in S, W, taken out of them), gamma_a(S) and gamma_b(S), and the parts of one window.
// The host side is rg_run of hf_rg.h; its fold stitches the parts of every group of joined chunks (hf_runlen_stitch.h) and sums a job's
// groups in chunk order.  A piece depends on (a, its windows, S, L) alone, so a job's bits depend on no other job, order or device batch.
#define HF_HELPERS_ONLY   // of hf_decode.h (kernels: hf_decoders.hip)
#include "hf_rg.h"
#include "hf_view.h"
#include "hf_chain.h"
#include "hf_runlen_stitch.h"

static_assert(HF_RUN_LENGTHS_MAX == 64, "one lane per age");

#define HF_RL_PIECE 512       // the piece grid of the other range getters
#define HF_RL_STRIDE 21       // doubles per window of the tile: Q [16] | sigma [4] | pad

// parts, and pieces of 512 windows, per device batch (a piece's results are 3 (L + 1) doubles, a part's 3 (L + 1) + 2).  The environment
// variables of the same names lower them (rg_cap; tests).
#ifndef HF_RL_BATCH_PARTS
#define HF_RL_BATCH_PARTS (1 << 16)
#endif
#ifndef HF_RL_BATCH_PIECES
#define HF_RL_BATCH_PIECES (1 << 16)
#endif

struct RlPiece { long long t0, a; int n, mask, c, last; };   // windows t0 .. t0 + n - 1 of the part that starts at a (chunk c); last: it holds b
struct RlPart { long long a, b; int p0, p1, mask, c; };      // chunk-local part [a, b] of chunk c, its pieces p0 .. p1 - 1

// gamma_t(S), hf_get_posterior's value (0.0 where the pass left no weight)
__device__ __forceinline__ double rl_gamma(const double f[4], const double b[4], int mask) {
    double g[4];
#pragma unroll
    for (int s = 0; s < 4; s++) g[s] = f[s] * b[s];
    double tot = g[0], in = (mask & 1) ? g[0] : 0.0;
#pragma unroll
    for (int s = 1; s < 4; s++) { tot += g[s]; in += ((mask >> s) & 1) ? g[s] : 0.0; }
    return tot > 0.0 ? in / tot : 0.0;
}

// what the tile holds for window x of the part that starts at a: r[p * 4 + q] = Q_x[p][q] (zeros at x == a: nothing steps into a),
// r[16 + s] = sigma_x[s]
template <bool SEQ>
__device__ __forceinline__ void rl_window(const PassView& pv, int c, long long x, long long a, int mask, double r[20]) {
    double A[16], f[4], b[4];
    mo_b<SEQ>(pv, c, x, b);
    if (x == a) {
        mo_f<SEQ>(pv, c, x, f);
#pragma unroll
        for (int k = 0; k < 16; k++) r[k] = 0.0;
        ch_post_start(f, b, mask, r + 16);      // sigma_a
        return;
    }
    iv_row<SEQ>(pv, x, A);
    mo_f<SEQ>(pv, c, x - 1, f);
    // (the rows of Q as ch_post_rows forms them, written out: formed in front of this nest they lengthen k_rl_piece's loop)
    double tot = 0.0, num[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const bool out_p = !((mask >> p) & 1);
        double y[4];
#pragma unroll
        for (int q = 0; q < 4; q++) y[q] = A[p * 4 + q] * b[q];
        const double den = ((y[0] + y[1]) + y[2]) + y[3];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            r[p * 4 + q] = den > 0.0 ? y[q] / den : 0.0;
            const double z = (f[p] * A[p * 4 + q]) * b[q];
            tot += z;
            num[q] += out_p ? z : 0.0;
        }
    }
#pragma unroll
    for (int s = 0; s < 4; s++) r[16 + s] = (((mask >> s) & 1) && tot > 0.0) ? num[s] / tot : 0.0;
}

// out[g]: I [L + 1] | Lc [L + 1] | the lanes' open masses at b [L] (zeros unless the piece holds b), one pad
template <bool SEQ>
__global__ void __launch_bounds__(64) k_rl_piece(const RlPiece* __restrict__ pieces, PassView pv, int max_len, double* __restrict__ out) {
    const RlPiece pc = pieces[blockIdx.x];
    const int lane = threadIdx.x;
    const int L = __builtin_amdgcn_readfirstlane(max_len), mask = __builtin_amdgcn_readfirstlane(pc.mask);
    const long long a = pc.a, t0 = pc.t0, end = pc.t0 + pc.n - 1;
    const long long h = a > t0 - L ? a : t0 - L;      // the first window of the halo: ages of more than L windows have saturated before t0
    const bool in0 = mask & 1, in1 = mask & 2, in2 = mask & 4, in3 = mask & 8;
    __shared__ double tile[64][HF_RL_STRIDE];

    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;    // v of the lane's age at the current window
    double bI = 0.0, bL = 0.0, oI = 0.0, oL = 0.0;    // the lane's bins: closed inside / left-touching; lane L - 1: "> L" of the two
    double nx[20];
#pragma unroll
    for (int k = 0; k < 20; k++) nx[k] = 0.0;
    long long base = h;
    if (base + lane <= end) rl_window<SEQ>(pv, pc.c, base + lane, a, mask, nx);
    while (base <= end) {
        const long long left_n = end - base + 1;
        const int n = (int) (left_n < 64 ? left_n : 64);
        if (lane < n) {
#pragma unroll
            for (int k = 0; k < 20; k++) tile[lane][k] = nx[k];
        }
        const long long nbase = base + 64;
        if (nbase + lane <= end) rl_window<SEQ>(pv, pc.c, nbase + lane, a, mask, nx);
        __syncthreads();
        for (int w = 0; w < n; w++) {
            const long long x = base + w;
            const double* __restrict__ r = tile[w];
            if (x > h) {
                const double w0 = ((v0 * r[0] + v1 * r[4]) + v2 * r[8]) + v3 * r[12];
                const double w1 = ((v0 * r[1] + v1 * r[5]) + v2 * r[9]) + v3 * r[13];
                const double w2 = ((v0 * r[2] + v1 * r[6]) + v2 * r[10]) + v3 * r[14];
                const double w3 = ((v0 * r[3] + v1 * r[7]) + v2 * r[11]) + v3 * r[15];
                const double ex = (((in0 ? 0.0 : w0) + (in1 ? 0.0 : w1)) + (in2 ? 0.0 : w2)) + (in3 ? 0.0 : w3);
                const double n0 = in0 ? w0 : 0.0, n1 = in1 ? w1 : 0.0, n2 = in2 ? w2 : 0.0, n3 = in3 ? w3 : 0.0;
                if (x >= t0) {                          // the piece's own windows: count
                    const bool lt = x - 1 - lane == a;  // the lane's run started at a
                    const double sv = lane == L - 1 ? ((n0 + n1) + n2) + n3 : 0.0;
                    bL += lt ? ex : 0.0; bI += lt ? 0.0 : ex;
                    oL += lt ? sv : 0.0; oI += lt ? 0.0 : sv;
                }
                v0 = ch_lane_below(n0); v1 = ch_lane_below(n1); v2 = ch_lane_below(n2); v3 = ch_lane_below(n3);
                if (lane >= L) { v0 = 0.0; v1 = 0.0; v2 = 0.0; v3 = 0.0; }
            }
            if (lane == 0) { v0 = r[16]; v1 = r[17]; v2 = r[18]; v3 = r[19]; }
        }
        __syncthreads();
        base = nbase;
    }
    double* __restrict__ o = out + (int64_t) blockIdx.x * (3 * (L + 1));
    if (lane < L) {
        o[lane] = bI;
        o[L + 1 + lane] = bL;
        o[2 * (L + 1) + lane] = pc.last ? ((v0 + v1) + v2) + v3 : 0.0;
    }
    if (lane == L - 1) { o[L] = oI; o[2 * L + 1] = oL; o[3 * L + 2] = 0.0; }
}

// out[i]: a part's record (hf_runlen_stitch.h)
template <bool SEQ>
__global__ void __launch_bounds__(64) k_rl_chain(const RlPart* __restrict__ parts, const double* __restrict__ pm, PassView pv, int max_len,
                                                 double* __restrict__ out) {
    const RlPart pt = parts[blockIdx.x];
    const int lane = threadIdx.x;
    const int L = __builtin_amdgcn_readfirstlane(max_len);
    const int64_t PM = 3 * (L + 1), T = pt.b - pt.a + 1;
    double* __restrict__ o = out + (int64_t) blockIdx.x * (PM + 2);
    for (int k = lane; k <= L; k += 64) {
        double I = 0.0, Lc = 0.0;
        for (int g = pt.p0; g < pt.p1; g++) { I += pm[g * PM + k]; Lc += pm[g * PM + (L + 1) + k]; }
        o[k] = I;
        o[L + 1 + k] = Lc;
        // the open masses: the run that started at a is the whole part (W below), the others are Rc
        if (k < L) o[2 * (L + 1) + k] = (pt.p1 > pt.p0 && k + 1 != T) ? pm[(pt.p1 - 1) * PM + 2 * (L + 1) + k] : 0.0;
    }
    if (lane != 0) return;
    double f[4], b[4], fe[4], be[4];
    mo_fb<SEQ>(pv, pt.c, pt.a, f, b);
    mo_fb<SEQ>(pv, pt.c, pt.b, fe, be);
    double W = 0.0;
    if (T == 1) {
        double sg[4];
        ch_post_start(f, b, pt.mask, sg);
        W = ((sg[0] + sg[1]) + sg[2]) + sg[3];
    } else if (T <= L) {
        W = pm[(pt.p1 - 1) * PM + 2 * (L + 1) + (T - 1)];
    }
    o[2 * (L + 1) + L] = W;
    o[PM] = rl_gamma(f, b, pt.mask);
    o[PM + 1] = rl_gamma(fe, be, pt.mask);
}

int hf_get_run_lengths(hf_ctx* ctx, int64_t n, const int64_t* first, const int64_t* last, const uint8_t* state_mask, int32_t max_len,
                       const uint8_t* joined, double* spectrum_host) {
    const std::string who = "hf_get_run_lengths";
    if (!ctx) return set_err(HF_E_ARG, who + ": bad argument");
    const Track& tr = ctx->tr;
    int rc = rg_check(ctx, who, n, !first || !last || !state_mask || !spectrum_host, first, last, state_mask, nullptr,
                      max_len < 1 || max_len > HF_RUN_LENGTHS_MAX ? "max_len must be 1..HF_RUN_LENGTHS_MAX (64)" : nullptr,
                      joined && tr.C > 0 && joined[0] ? "joined[0] must be 0 (the first chunk continues nothing)" : nullptr);
    if (rc) return rc;
    PassView pv;
    rc = pass_view(ctx, who, n, pv);
    if (rc || n == 0) return rc;
    hipStream_t st = ctx->pass.last_stream;
    const int L = (int) max_len;
    const size_t PM = 3 * ((size_t) L + 1), PS = rl_part_len(L);
    RlStitch stitch(L);
    return rg_run<RlPiece, RlPart, HF_RL_PIECE>(ctx, who, ctx->rl, n, first, last, rg_cap("HF_RL_BATCH_PIECES", HF_RL_BATCH_PIECES),
        rg_cap("HF_RL_BATCH_PARTS", HF_RL_BATCH_PARTS), PM * 8, 0, PS,
        [&](int64_t j, int c, int64_t a, int64_t b) { return RlPart{a, b, 0, 0, state_mask[j], c}; },
        [](const RlPart& pt, int64_t t, int len) { return RlPiece{t, pt.a, len, pt.mask, pt.c, t + len - 1 == pt.b ? 1 : 0}; },
        [&](const RgBatch<RlPiece, RlPart>& bt) {      // (the chain kernel: one workgroup per part)
            by_algo(tr, [&](auto S) {
                constexpr bool SEQ = decltype(S)::value;
                if (bt.np) hipLaunchKernelGGL(k_rl_piece<SEQ>, bt.piece_grid(), dim3(64), 0, st, bt.pieces, pv, L, bt.pm);
                hipLaunchKernelGGL(k_rl_chain<SEQ>, dim3((unsigned) bt.nq), dim3(64), 0, st, bt.parts, bt.pm, pv, L, bt.out);
            });
        },
        [&](int64_t j, const RlPart* parts, const double* val, int64_t k0, int64_t k1) {
            // a job's bins: its groups' bins, summed in chunk order
            double* acc = spectrum_host + (size_t) j * ((size_t) L + 1);
            for (int l = 0; l <= L; l++) acc[l] = 0.0;
            for (int64_t k = k0; k < k1; k++) {
                if (!part_joined(parts, k, k0, joined)) {
                    if (k > k0) stitch.end(acc);
                    stitch.begin();
                }
                stitch.part(&val[(size_t) k * PS], parts[k].b - parts[k].a + 1);
            }
            if (k1 > k0) stitch.end(acc);
        });
}
