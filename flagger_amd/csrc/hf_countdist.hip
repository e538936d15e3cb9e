// hf_countdist.hip — the exact distribution of label totals of the C ABI (hf_get_count_distribution, include/hmm_flagger_hip.h), a
// translation unit of its own, kernels and host side: for a window range, a state set S and a count K, the posterior probability that
// exactly k = 0 .. K windows of the range lie in S, and that more than K do, under the model of the last HF_MODE_FULL pass.  Not part of
// an EM pass: it reads the pass's rows, forward and backward vectors (hf_view.h, through pass_view of hf_host.h) and writes buffers of
// its own only (hf_ctx::cd).
//
// Definition.  Given the data the states of a chunk are a Markov chain, and only ratios of the pass's values are formed:
//   Q_u[p][q]  = A_u[p][q] b_u[q] / sum_q' A_u[p][q'] b_u[q']       the posterior chain, a < u <= b (ch_post_rows of hf_chain.h: q' = 0..3 in
//                                                                   order; a row whose denominator is 0 is a zero row: no mass reaches it)
//   gamma_a[s] = f_a[s] b_a[s] / sum_s' f_a[s'] b_a[s']             the start at the part's first window (ch_post_start: 0.0 where the sum is 0)
// The walk carries v[s][k], "in state s, k windows of S so far" (k = 0 .. K, and K + 1 for "more than K"): v_a[s][1_S[s]] = gamma_a[s];
// per window u, w[q][k] = ((v[0][k] Q[0][q] + v[1][k] Q[1][q]) + v[2][k] Q[2][q]) + v[3][k] Q[3][q]; a column q outside S keeps w, a
// column in S moves up one bin: v[q][k] = w[q][k - 1], v[q][0] = 0, v[q][> K] = w[q][> K] + w[q][K].  The part's distribution is
// ((v_b[0] + v_b[1]) + v_b[2]) + v_b[3] per bin.  Every bin is a sum of non-negative terms; "> K" is carried, never formed as 1 - sum.
//
// k_cd_piece<SEQ>  one wavefront per piece of the getters' 512-window job grid (hf_jobs.h), LANE = BIN.  A lane holds the 4 x 4 transfer
//                  M[p][q] of its bin: "entered the piece in state p (the state of the window in front of it), now in state q, this many
//                  windows of S inside the piece so far"; it starts as the identity in lane 0.  A step is sixteen 4-term dot products
//                  against Q_u, whose 16 entries are the same for the wavefront: they are computed once per window, 64 windows at a time
//                  with lane = window, and staged through an LDS tile (stride 17 doubles: the lanes' rows fall into different banks)
//                  that the steps read back as broadcasts; the rows of the next 64 windows wait in registers meanwhile.  Then the columns
//                  q in S take the value of the lane below (wave_shr:1 on the two halves of each double, hf_chain.h): lane 0 takes 0.0,
//                  lane K + 1 adds what lane K held to its own, the lanes above K + 1 stay 0.0.  No atomics, no cross-lane sums, no
//                  rescaling (the entries are probabilities): one order of operations.
// k_cd_chain<SEQ>  one 64-lane workgroup per part, lane = bin.  From gamma_a it takes the pieces in order; with the piece's transfer in
//                  LDS, lane k <= K forms, for every (p, q), c[p][q] = sum_{j = 0 .. k} v[p][j] M[p][q][k - j], one accumulator from 0.0,
//                  j ascending, and lane K + 1 forms c[p][q] = sum_{j = 0 .. K + 1} v[p][j] r_j with the running tail sum
//                  r_j = sum_{m = K + 1 - j .. K + 1} M[p][q][m] that takes M[p][q][K + 1 - j] at step j (so it adds M downwards from "> K":
//                  r_0 = 0.0 + M[p][q][K + 1]; index K + 1 of v is its own "> K" bin, which meets the whole of M).  Then
//                  v[q] = ((c[0][q] + c[1][q]) + c[2][q]) + c[3][q].  At the end the lane sums its bin over q in state order.  A part with
//                  a == b has no piece and is gamma_a alone.
// The host side is rg_run of hf_rg.h; its fold convolves the parts of a job in chunk order (hf_countdist_stitch.h, the same two sums).
// A piece depends on (its windows, S, K) alone and a part on (a, b, S, K), so a job's bits depend on no other job, order or device batch.
#define HF_HELPERS_ONLY   // of hf_decode.h (kernels: hf_decoders.hip)
#include "hf_rg.h"
#include "hf_view.h"
#include "hf_chain.h"
#include "hf_countdist_stitch.h"

static_assert(HF_COUNT_DIST_MAX + 2 == 64, "one lane per bin");

#define HF_CD_PIECE 512       // the piece grid of the other range getters
#define HF_CD_STRIDE 17       // doubles per window of the tile: Q [16] | pad

// parts, and pieces of 512 windows, per device batch (a piece's result is 16 (K + 2) doubles, a part's K + 2).  The environment
// variables of the same names lower them (rg_cap; tests).
#ifndef HF_CD_BATCH_PARTS
#define HF_CD_BATCH_PARTS (1 << 16)
#endif
#ifndef HF_CD_BATCH_PIECES
#define HF_CD_BATCH_PIECES (1 << 14)
#endif

struct CdPiece { long long t0; int n, mask, c, pad; };      // windows t0 .. t0 + n - 1 of chunk c, none of them a part's first
struct CdPart { long long a, b; int p0, p1, mask, c; };     // chunk-local part [a, b] of chunk c, its pieces p0 .. p1 - 1

// r[p * 4 + q] = Q_x[p][q] of a window x that is not its part's first
template <bool SEQ>
__device__ __forceinline__ void cd_window(const PassView& pv, int c, long long x, double r[16]) {
    double A[16], b[4];
    mo_b<SEQ>(pv, c, x, b);
    iv_row<SEQ>(pv, x, A);
    ch_post_rows(A, b, r);
}

// out[g]: M[p][q][k] at (p * 4 + q) * (K + 2) + k, k = 0 .. K + 1
template <bool SEQ>
__global__ void __launch_bounds__(64) k_cd_piece(const CdPiece* __restrict__ pieces, PassView pv, int max_count, double* __restrict__ out) {
    const CdPiece pc = pieces[blockIdx.x];
    const int lane = threadIdx.x;
    const int K = __builtin_amdgcn_readfirstlane(max_count), mask = __builtin_amdgcn_readfirstlane(pc.mask);
    const long long end = pc.t0 + pc.n - 1;
    const bool in0 = mask & 1, in1 = mask & 2, in2 = mask & 4, in3 = mask & 8;
    const bool bottom = lane == 0, top = lane == K + 1, idle = lane > K + 1;
    __shared__ double tile[64][HF_CD_STRIDE];

    double M[16], nx[16];
#pragma unroll
    for (int k = 0; k < 16; k++) { M[k] = (bottom && k % 5 == 0) ? 1.0 : 0.0; nx[k] = 0.0; }
    long long base = pc.t0;
    if (base + lane <= end) cd_window<SEQ>(pv, pc.c, base + lane, nx);
    while (base <= end) {
        const long long left_n = end - base + 1;
        const int n = (int) (left_n < 64 ? left_n : 64);
        if (lane < n) {
#pragma unroll
            for (int k = 0; k < 16; k++) tile[lane][k] = nx[k];
        }
        const long long nbase = base + 64;
        if (nbase + lane <= end) cd_window<SEQ>(pv, pc.c, nbase + lane, nx);
        __syncthreads();
        for (int w = 0; w < n; w++) {
            const double* __restrict__ r = tile[w];
            double W[16];
#pragma unroll
            for (int p = 0; p < 4; p++) {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    W[p * 4 + q] = ((M[p * 4] * r[q] + M[p * 4 + 1] * r[4 + q]) + M[p * 4 + 2] * r[8 + q]) + M[p * 4 + 3] * r[12 + q];
            }
            // the columns of S move up one bin (every lane takes part in the moves: the conditions are the wavefront's)
#define HF_CD_UP(q) \
            _Pragma("unroll") for (int p = 0; p < 4; p++) { \
                const double own = W[p * 4 + (q)], below = ch_lane_below(own); \
                W[p * 4 + (q)] = (bottom || idle) ? 0.0 : top ? own + below : below; \
            }
            if (in0) { HF_CD_UP(0) }
            if (in1) { HF_CD_UP(1) }
            if (in2) { HF_CD_UP(2) }
            if (in3) { HF_CD_UP(3) }
#undef HF_CD_UP
#pragma unroll
            for (int k = 0; k < 16; k++) M[k] = W[k];
        }
        __syncthreads();
        base = nbase;
    }
    if (lane <= K + 1) {
        double* __restrict__ o = out + (int64_t) blockIdx.x * (16 * (K + 2)) + lane;
#pragma unroll
        for (int k = 0; k < 16; k++) o[k * (K + 2)] = M[k];
    }
}

// out[i]: the part's K + 2 bins
template <bool SEQ>
__global__ void __launch_bounds__(64) k_cd_chain(const CdPart* __restrict__ parts, const double* __restrict__ pm, PassView pv, int max_count,
                                                 double* __restrict__ out) {
    const CdPart pt = parts[blockIdx.x];
    const int lane = threadIdx.x;
    const int K = __builtin_amdgcn_readfirstlane(max_count), mask = __builtin_amdgcn_readfirstlane(pt.mask);
    const int B = K + 2;
    const bool live = lane < B, top = lane == K + 1;
    __shared__ double Ms[16][64];
    __shared__ double vs[4][64];

    double v[4];
    {
        double f[4], b[4], g[4];
        mo_fb<SEQ>(pv, pt.c, pt.a, f, b);
        ch_post_start(f, b, 15, g);
#pragma unroll
        for (int s = 0; s < 4; s++) v[s] = lane == ((mask >> s) & 1) ? g[s] : 0.0;
    }
    for (int g = pt.p0; g < pt.p1; g++) {
        const double* __restrict__ src = pm + (int64_t) g * (16 * B);
#pragma unroll
        for (int s = 0; s < 4; s++) vs[s][lane] = v[s];
        if (live) {
#pragma unroll
            for (int e = 0; e < 16; e++) Ms[e][lane] = src[e * B + lane];
        }
        __syncthreads();
        if (live) {
            double acc[16], r[16];
#pragma unroll
            for (int e = 0; e < 16; e++) { acc[e] = 0.0; r[e] = 0.0; }
            for (int j = 0; j < B; j++) {
                const int i = lane - j;
                const bool on = i >= 0;
                const int ii = on ? i : 0;
                double vj[4];
#pragma unroll
                for (int p = 0; p < 4; p++) vj[p] = vs[p][j];
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const double m = on ? Ms[e][ii] : 0.0;
                    r[e] = top ? r[e] + m : m;
                    acc[e] += vj[e >> 2] * r[e];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = ((acc[q] + acc[4 + q]) + acc[8 + q]) + acc[12 + q];
        }
        __syncthreads();
    }
    if (live) out[(int64_t) blockIdx.x * B + lane] = ((v[0] + v[1]) + v[2]) + v[3];
}

int hf_get_count_distribution(hf_ctx* ctx, int64_t n, const int64_t* first, const int64_t* last, const uint8_t* state_mask, int32_t max_count,
                              double* dist_host) {
    const std::string who = "hf_get_count_distribution";
    if (!ctx) return set_err(HF_E_ARG, who + ": bad argument");
    const Track& tr = ctx->tr;
    int rc = rg_check(ctx, who, n, !first || !last || !state_mask || !dist_host, first, last, state_mask, nullptr,
                      max_count < 1 || max_count > HF_COUNT_DIST_MAX ? "max_count must be 1..HF_COUNT_DIST_MAX (62)" : nullptr);
    if (rc) return rc;
    PassView pv;
    rc = pass_view(ctx, who, n, pv);
    if (rc || n == 0) return rc;
    hipStream_t st = ctx->pass.last_stream;
    const int K = (int) max_count;
    const size_t B = cd_part_len(K), PM = 16 * B;
    CdStitch stitch(K);
    return rg_run<CdPiece, CdPart, HF_CD_PIECE>(ctx, who, ctx->cd, n, first, last, rg_cap("HF_CD_BATCH_PIECES", HF_CD_BATCH_PIECES),
        rg_cap("HF_CD_BATCH_PARTS", HF_CD_BATCH_PARTS), PM * 8, 0, B,
        [&](int64_t j, int c, int64_t a, int64_t b) { return CdPart{a, b, 0, 0, state_mask[j], c}; },
        [](const CdPart& pt, int64_t t, int len) { return CdPiece{t, len, pt.mask, pt.c, 0}; },
        [&](const RgBatch<CdPiece, CdPart>& bt) {      // (the chain kernel: one workgroup per part)
            by_algo(tr, [&](auto S) {
                constexpr bool SEQ = decltype(S)::value;
                if (bt.np) hipLaunchKernelGGL(k_cd_piece<SEQ>, bt.piece_grid(), dim3(64), 0, st, bt.pieces, pv, K, bt.pm);
                hipLaunchKernelGGL(k_cd_chain<SEQ>, dim3((unsigned) bt.nq), dim3(64), 0, st, bt.parts, bt.pm, pv, K, bt.out);
            });
        },
        [&](int64_t j, const CdPart*, const double* val, int64_t k0, int64_t k1) {      // (hf_countdist_stitch.h)
            stitch.begin();
            for (int64_t k = k0; k < k1; k++) stitch.part(&val[(size_t) k * B]);
            stitch.end(dist_host + (size_t) j * B);
        });
}
