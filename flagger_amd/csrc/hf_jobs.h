// hf_jobs.h — how every range getter (the interval, count-moment, run-moment, entropy, breakpoint and long-run getters of hf_getters.h,
// hf_get_run_lengths, hf_get_count_distribution) cuts a call's jobs into device work; hf_rg.h runs the batches.  Host code only, no HIP
// header: tests/test_jobcut_cpu.py compiles it with the host compiler (jobcut_check.cpp).
//
// THE CUTTING RULE.  A job is a window range [first, last] inside the chunks.  It becomes one PART per chunk it touches, [a, b] = the
// job's windows in that chunk, in chunk order; chunks without windows are skipped.  A part's interior windows (a, b] become PIECES, cut at
// global window indices that are multiples of GRID: a piece therefore depends on its job alone, and a part with a == b has none.
//
// THE BATCHING RULE.  A call's jobs go to the device in batches, in order: a job joins the batch while the batch holds fewer than
// cap_pieces pieces and fewer than cap_parts parts; a batch holds at least one job; a job is never split.  The caller gives the caps
// (every getter's HF_*_BATCH_PIECES and HF_*_BATCH_PARTS stand with its code: hf_estep.hip, hf_getters.h, hf_runlen.hip, hf_countdist.hip).
//
// THE JOIN RULE (hf_get_run_moments, hf_get_long_run_log_probs, hf_get_run_lengths), part_joined below.  joined[c] != 0 says that chunk c
// continues chunk c - 1 (joined == nullptr: no chunk does).  Part k of a job is joined to part k - 1 when it lies in the next chunk and
// that chunk has joined != 0; a chunk without windows has no part, so it ends a sequence of joined chunks, and a job's first part is
// joined to nothing.  A GROUP (group_parts) is a maximal sequence of parts joined to each other.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// One batch of a call.  Part has int members p0, p1 (its pieces p0 .. p1 - 1 of the batch), set here; everything else of a record is the
// getter's: mk_part(job, chunk, a, b) builds a part and mk_piece(part, t, n) a piece of it (windows t .. t + n - 1; what a piece shares
// with its part is read from the part, once per part).  The vectors are reused from batch to batch.
template <class Piece, class Part, int64_t GRID>
struct JobCut {
    std::vector<Piece> pieces;
    std::vector<Part> parts;
    std::vector<int64_t> job_p0;      // the first part of every job of the batch, and the end

    // cuts jobs j0 .. of the n of a call (off: the chunks' first windows and the end); returns the first job of the next batch
    template <class MkPart, class MkPiece>
    int64_t cut(const std::vector<int64_t>& off, int64_t n, const int64_t* first, const int64_t* last, int64_t j0, size_t cap_pieces,
                size_t cap_parts, MkPart&& mk_part, MkPiece&& mk_piece) {
        pieces.clear(); parts.clear(); job_p0.clear();
        int64_t j1 = j0;
        while (j1 < n && (j1 == j0 || (pieces.size() < cap_pieces && parts.size() < cap_parts))) {
            job_p0.push_back((int64_t) parts.size());
            int c = (int) (std::upper_bound(off.begin(), off.end(), first[j1]) - off.begin()) - 1;
            for (int64_t a = first[j1]; a <= last[j1]; c++) {
                while (off[(size_t) c + 1] <= a) c++;      // (chunks without windows)
                const int64_t b = std::min<int64_t>(last[j1], off[(size_t) c + 1] - 1);
                Part pt = mk_part(j1, c, a, b);
                pt.p0 = (int) pieces.size();
                for (int64_t t = a + 1; t <= b;) {
                    const int64_t e = std::min<int64_t>(b, (t / GRID + 1) * GRID - 1);
                    pieces.push_back(mk_piece(pt, t, (int) (e - t + 1)));
                    t = e + 1;
                }
                pt.p1 = (int) pieces.size();
                parts.push_back(pt);
                a = b + 1;
            }
            j1++;
        }
        job_p0.push_back((int64_t) parts.size());
        return j1;
    }
};

// THE statement of "chunk c continues chunk c - 1" over a chunk list (off: the C chunks' first windows and the end): it is joined to it
// and both have windows.  The groups of the whole-contig decoders (hf_minlen.hip) and of the command line (hf_cli_scopes.h group_end)
// are the maximal sequences of chunks that continue each other.
inline bool chunk_continues(const int64_t* off, int64_t C, const uint8_t* joined, int64_t c) {
    return c > 0 && c < C && joined && joined[c] != 0 && off[c + 1] > off[c] && off[c] > off[c - 1];
}

// the join rule: is part k of the job whose first part is k0 joined to part k - 1?  (Part has an int member c, its chunk.)  This is
// chunk_continues over parts: a chunk without windows has no part, so two parts in chunks c - 1 and c say that both have windows.
template <class Part>
inline bool part_joined(const Part* parts, int64_t k, int64_t k0, const uint8_t* joined) {
    return k > k0 && joined && parts[k].c == parts[k - 1].c + 1 && joined[parts[k].c] != 0;
}

// The groups of a cut batch, in order: mk_group(job index in the batch, q0, q1) builds the group of parts q0 .. q1 - 1.
// job_g0: the first group of every job of the batch, and the end.
template <class Part, class Group, class MkGroup>
void group_parts(const std::vector<Part>& parts, const std::vector<int64_t>& job_p0, const uint8_t* joined, std::vector<Group>& groups,
                 std::vector<int64_t>& job_g0, MkGroup&& mk_group) {
    groups.clear(); job_g0.clear();
    for (size_t j = 0; j + 1 < job_p0.size(); j++) {
        job_g0.push_back((int64_t) groups.size());
        for (int64_t q0 = job_p0[j], q = q0 + 1; q0 < job_p0[j + 1]; q++)
            if (q == job_p0[j + 1] || !part_joined(parts.data(), q, job_p0[j], joined)) { groups.push_back(mk_group((int64_t) j, q0, q)); q0 = q; }
    }
    job_g0.push_back((int64_t) groups.size());
}

// lanes of the expanded chain of hf_get_long_run_log_probs: the states outside S, the counters (s, d), d = 1 .. L - 1, the four HIT lanes
inline int64_t long_run_lanes(int mask, int64_t len) {
    int k = 0;
    for (int s = 0; s < 4; s++) k += (mask >> s) & 1;
    return (4 - k) + k * (len - 1) + 4;
}
