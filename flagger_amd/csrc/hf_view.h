// hf_view.h — what the last HF_MODE_FULL pass left on the device, as the getters' kernels read it (hf_interval.h, hf_moments.h, hf_runs.h,
// hf_entropy.h, hf_alpha.h): one struct passed by value, the row A_t of a window and the scaled forward and backward vectors f_t, b_t
// (hf_get_forward_backward).  The host fills it in one place (view_of in hf_getters.h); the pointers of the other algorithm are null.
//   HF_ALGO_SCAN  rows: the pass's deduplicated rows of A (lutA through arow; bit 31 marks a chunk-first window), stored state-major
//                 (o = s * 4 + pre, hf_seg.h HF_PS) and transposed on load.  f, b: the pair records (b_t: second half of the record at
//                 pos[t], f_t: first half of the one at pos_f[t])
//   HF_ALGO_SEQ   rows: T_t o e_t, the pass's emission rows (E, k_emit_rows) times the transition row of its own parameter block Pm
//                 (k_fwd_seq applies (f . T) . e: the same factors).  f, b: the tiles of k_fwd_seq / k_bwd_seq (hf_device.h fb_slot)
// rec, the packed window records, is set for both.  Loads only: no arithmetic on the values.
#pragma once
#include "hf_decode.h"

struct PassView {
    const int32_t* pos; const int32_t* pos_f; const double* recs;                          // f, b: HF_ALGO_SCAN
    const int64_t* off; const int32_t* chunk_tile0; const double* F; const double* B;      // f, b: HF_ALGO_SEQ
    const int32_t* arow; const double* lutA;                                               // rows: HF_ALGO_SCAN
    const double* E; const DevParams* Pm;                                                  // rows: HF_ALGO_SEQ
    const uint32_t* rec;
};

// the row A_t of the pass at window t (layout [pre * 4 + s])
template <bool SEQ>
__device__ __forceinline__ void iv_row(const PassView& S, int64_t t, double A[16]) {
    if constexpr (SEQ) {
        double Tm[16];
        load_T(S.Pm, S.rec[t], Tm);
        const double2* __restrict__ src = reinterpret_cast<const double2*>(S.E) + t * 8;
#pragma unroll
        for (int k = 0; k < 8; k++) { const double2 v = src[k]; A[2 * k] = Tm[2 * k] * v.x; A[2 * k + 1] = Tm[2 * k + 1] * v.y; }
    } else {   // (the table is state-major, o = s * 4 + pre: hf_seg.h HF_PS)
        const double2* __restrict__ src = reinterpret_cast<const double2*>(S.lutA) + (int64_t) ((uint32_t) S.arow[t] & 0x7fffffffu) * 8;
        double R[16];
#pragma unroll
        for (int k = 0; k < 8; k++) { const double2 v = src[k]; R[2 * k] = v.x; R[2 * k + 1] = v.y; }
#pragma unroll
        for (int k = 0; k < 16; k++) A[k] = R[(k & 3) * 4 + (k >> 2)];
    }
}

// f_t, b_t or both of window t of chunk c
template <bool SEQ>
__device__ __forceinline__ void mo_f(const PassView& S, int c, int64_t t, double f[4]) {
    if constexpr (SEQ) {
        const int64_t w = t - S.off[c];
        const int tile0 = S.chunk_tile0[c];
        const double2* __restrict__ F2 = reinterpret_cast<const double2*>(S.F);
#pragma unroll
        for (int h = 0; h < 2; h++) { const double2 x = F2[fb_slot_w<HF_SCAN_L>(tile0, w, h)]; f[2 * h] = x.x; f[2 * h + 1] = x.y; }
    } else {
        const double* __restrict__ rf = S.recs + (int64_t) S.pos_f[t] * 8;
#pragma unroll
        for (int s = 0; s < 4; s++) f[s] = rf[s];
    }
}

template <bool SEQ>
__device__ __forceinline__ void mo_b(const PassView& S, int c, int64_t t, double b[4]) {
    if constexpr (SEQ) {
        const int64_t w = t - S.off[c];
        const int tile0 = S.chunk_tile0[c];
        const double2* __restrict__ B2 = reinterpret_cast<const double2*>(S.B);
#pragma unroll
        for (int h = 0; h < 2; h++) { const double2 y = B2[fb_slot_w<HF_SCAN_L>(tile0, w, h)]; b[2 * h] = y.x; b[2 * h + 1] = y.y; }
    } else {
        const double* __restrict__ rb = S.recs + (int64_t) S.pos[t] * 8 + 4;
#pragma unroll
        for (int s = 0; s < 4; s++) b[s] = rb[s];
    }
}

template <bool SEQ>
__device__ __forceinline__ void mo_fb(const PassView& S, int c, int64_t t, double f[4], double b[4]) {
    mo_f<SEQ>(S, c, t, f);
    mo_b<SEQ>(S, c, t, b);
}
