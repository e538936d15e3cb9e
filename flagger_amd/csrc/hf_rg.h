// hf_rg.h — the host front of the range getters, for every unit that has one (hf_estep.hip through hf_getters.h, hf_runlen.hip,
// hf_countdist.hip): the cap of a device batch, the layout of a batch's scratch, the batch loop and the piece / chain driver over it.
// Host code with HIP, no kernel (rg_check and pass_view, which every getter calls first, are functions of hf_estep.hip: hf_host.h).  A NEW
// RANGE GETTER is two record types (hf_jobs.h), two kernels and a fold for rg_run; one with other launches or arrays gives rg_batches a body.
#pragma once
#include "hf_host.h"
#include "hf_jobs.h"

// A cap of a device batch: dflt, lowered (never raised) by the environment variable when it holds a number >= 1; read on every call.
// Only the getters that name a variable have one (tests cut their calls into many batches with it).
static size_t rg_cap(const char* env_name, size_t dflt) {
    if (const char* e = std::getenv(env_name)) { const long v = std::atol(e); if (v >= 1) return std::min<size_t>((size_t) v, dflt); }
    return dflt;
}

// The scratch of a batch in the getter's grow-only buffer: arrays(f) calls f(pointer, bytes) for every array in turn.  Sizes first, one
// reserve, then the pointers, each array on a granule of its own in the order given.
template <class A>
static int rg_take(DevBuf& buf, const std::string& who, A&& arrays) {
    size_t bytes = 0;
    arrays([&](auto&, size_t n) { bytes += Slab::granule(n); });
    if (const int rc = buf.reserve(bytes, who)) return rc;
    char* d = buf.d_buf;
    arrays([&](auto& p, size_t n) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(d); d += Slab::granule(n); });
    return HF_OK;
}

// The jobs of a call, batch by batch, on the stream of the pass: the cut (hf_jobs.h), body(jc, j0) for the batch that starts at job j0
// (it takes the scratch, enqueues uploads, launches and the copies back, and returns an error code), one synchronise, and fold(jc, j, i)
// for every job j of the batch, i its index in the batch.
template <class Piece, class Part, int64_t GRID, class MkPart, class MkPiece, class Body, class Fold>
static int rg_batches(hf_ctx* ctx, int64_t n, const int64_t* first, const int64_t* last, size_t cap_pieces, size_t cap_parts, MkPart&& mk_part,
                      MkPiece&& mk_piece, Body&& body, Fold&& fold) {
    hipStream_t st = ctx->pass.last_stream;
    JobCut<Piece, Part, GRID> jc;
    for (int64_t j0 = 0; j0 < n;) {
        const int64_t j1 = jc.cut(ctx->tr.h_off, n, first, last, j0, cap_pieces, cap_parts, mk_part, mk_piece);
        if (const int rc = body(jc, j0)) return rc;
        HIPCHK(hipStreamSynchronize(st));
        for (int64_t j = j0; j < j1; j++) fold(jc, j, (size_t) (j - j0));
        j0 = j1;
    }
    return HF_OK;
}

// a batch on the device: np pieces, nq parts, the per-piece results pm and px of the piece kernel, the per-part results of the chain kernel
template <class Piece, class Part>
struct RgBatch {
    size_t np, nq;
    Piece* pieces; Part* parts;
    double* pm; double* px; double* out;
    dim3 piece_grid() const { return dim3((unsigned) np); }                  // one 64-lane workgroup per piece
    dim3 chain_grid() const { return dim3((unsigned) ((nq + 63) / 64)); }    // one thread per part
};

// The piece / chain getters.  pm_bytes, px_bytes: the piece kernel's results per piece (px_bytes == 0: one array only); out_doubles: the
// chain kernel's per part.  launch(batch) enqueues the two kernels (the piece kernel only when the batch has pieces), on grids it chooses;
// fold(job, parts, val, k0, k1) writes the value of the job from the host's records and the results of its parts k0 .. k1 - 1 (chunk order).
template <class Piece, class Part, int64_t GRID, class MkPart, class MkPiece, class Launch, class Fold>
static int rg_run(hf_ctx* ctx, const std::string& who, DevBuf& buf, int64_t n, const int64_t* first, const int64_t* last, size_t cap_pieces,
                  size_t cap_parts, size_t pm_bytes, size_t px_bytes, size_t out_doubles, MkPart&& mk_part, MkPiece&& mk_piece, Launch&& launch,
                  Fold&& fold) {
    hipStream_t st = ctx->pass.last_stream;
    std::vector<double> val;
    return rg_batches<Piece, Part, GRID>(ctx, n, first, last, cap_pieces, cap_parts, mk_part, mk_piece,
        [&](const auto& jc, int64_t) -> int {
            const size_t np = jc.pieces.size(), nq = jc.parts.size();
            RgBatch<Piece, Part> bt{np, nq, nullptr, nullptr, nullptr, nullptr, nullptr};
            const int rc = rg_take(buf, who, [&](auto f) {
                f(bt.pieces, np * sizeof(Piece)); f(bt.parts, nq * sizeof(Part)); f(bt.pm, np * pm_bytes);
                if (px_bytes) f(bt.px, np * px_bytes);
                f(bt.out, nq * out_doubles * 8);
            });
            if (rc) return rc;
            if (np) HIPCHK(hipMemcpyAsync(bt.pieces, jc.pieces.data(), np * sizeof(Piece), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(bt.parts, jc.parts.data(), nq * sizeof(Part), hipMemcpyHostToDevice, st));
            launch(bt);
            HIPCHK(hipGetLastError());
            val.resize(nq * out_doubles);
            HIPCHK(hipMemcpyAsync(val.data(), bt.out, nq * out_doubles * 8, hipMemcpyDeviceToHost, st));
            return HF_OK;
        },
        [&](const auto& jc, int64_t j, size_t i) { fold(j, jc.parts.data(), val.data(), jc.job_p0[i], jc.job_p0[i + 1]); });
}
