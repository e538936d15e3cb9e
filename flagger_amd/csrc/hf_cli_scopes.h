// hf_cli_scopes.h — the chunk-list rules of the command line's reports (hf_cli_reports.h, hf_cli.cpp), each stated once.  Host code over
// std and hf_jobs.h alone: tests/test_cli_scopes_cpu.py compiles it with the host compiler (scopes_check.cpp).
//
// JOINED.  joined[c] != 0: chunk c has the contig name of chunk c - 1 (joined_by_contig).  Chunk c CONTINUES chunk c - 1 when it is joined
// to it and both have windows (chunk_continues, hf_jobs.h); a GROUP is a maximal sequence of chunks that continue each other (group_end).
//
// THE SCOPES of a per-scope report: "all", then every contig by name in the order of first appearance in the chunk list; a contig is a
// scope even when none of its chunks has windows.  A scope has two views:
//   runs     its maximal runs [c0, c1) of consecutive list positions.  Chunks of different runs are independent chains, chunks of one run
//            go on into each other by `joined`; a report over runs skips a run without windows (no_windows).
//   ranges   the window ranges [a, b) of its chunks that have windows, merged where the next begins at the end of the one before (so a
//            chunk without windows between two chunks of a contig splits the run, not the range).
// "all" is the run [0, C) and the range [0, N): the offsets of a table start at 0 and end at N, so the merged ranges of all chunks with
// windows are that one range too.  A sum over a scope is taken over its runs or ranges in this order.
#pragma once
#include "hf_jobs.h"
#include <map>
#include <string>
#include <utility>
#include <vector>

static const char* const kRunLabelNames[] = {"Err", "Dup", "Hap", "Col"};   // the final BED's names (hf_io.cpp kLabelNames)
static const uint8_t kLabelSets[5] = {1, 2, 4, 8, 11};                     // the label sets of the per-set reports, as state masks
static const char* const kLabelSetNames[5] = {"Err", "Dup", "Hap", "Col", "Err+Dup+Col"};

// the name of state l in a column header (--labelNames where it reaches) and of a label in a row (-1 and the like: Unk)
inline const char* state_column_name(const std::vector<std::string>& labelNames, size_t l) {
    return labelNames.size() > l ? labelNames[l].c_str() : kRunLabelNames[l];
}
inline const char* run_label_name(int label) { return label >= 0 && label < 4 ? kRunLabelNames[label] : "Unk"; }

// the chunk list: C chunks, the first window of each and the end (off[0 .. C]), the contig name of each
struct ChunkList {
    int C = 0;
    const int64_t* off = nullptr;
    std::vector<std::string> ctg;
    bool no_windows(int c0, int c1) const { return off[c0] == off[c1]; }      // chunks c0 .. c1 - 1
};

inline std::vector<uint8_t> joined_by_contig(const ChunkList& l) {
    std::vector<uint8_t> joined((size_t) std::max(l.C, 1), 0);
    for (int c = 1; c < l.C; c++) joined[(size_t) c] = l.ctg[(size_t) c] == l.ctg[(size_t) c - 1];
    return joined;
}

// the first chunk behind the group that chunk c0 starts
inline int group_end(const ChunkList& l, const uint8_t* joined, int c0) {
    int c1 = c0 + 1;
    while (chunk_continues(l.off, l.C, joined, c1)) c1++;
    return c1;
}

struct Scope {
    std::string name;
    std::vector<std::pair<int, int>> runs;               // chunks [c0, c1)
    std::vector<std::pair<int64_t, int64_t>> ranges;     // windows [a, b)
};
struct Scopes {
    std::vector<Scope> scopes;              // [0]: "all"
    std::vector<size_t> scope_of_chunk;     // the contig's scope, >= 1
};
inline Scopes contig_scopes(const ChunkList& l) {
    Scopes s;
    s.scopes.push_back(Scope{"all", {}, {}});
    if (l.C > 0) s.scopes[0].runs.push_back({0, l.C});
    if (l.C > 0 && !l.no_windows(0, l.C)) s.scopes[0].ranges.push_back({l.off[0], l.off[l.C]});
    std::map<std::string, size_t> byName;
    for (int c = 0; c < l.C; c++) {
        auto it = byName.find(l.ctg[(size_t) c]);
        if (it == byName.end()) { it = byName.emplace(l.ctg[(size_t) c], s.scopes.size()).first; s.scopes.push_back(Scope{l.ctg[(size_t) c], {}, {}}); }
        s.scope_of_chunk.push_back(it->second);
        Scope& sc = s.scopes[it->second];
        if (!sc.runs.empty() && sc.runs.back().second == c) sc.runs.back().second = c + 1;
        else sc.runs.push_back({c, c + 1});
        if (l.no_windows(c, c + 1)) continue;
        if (!sc.ranges.empty() && sc.ranges.back().second == l.off[c]) sc.ranges.back().second = l.off[c + 1];
        else sc.ranges.push_back({l.off[c], l.off[c + 1]});
    }
    return s;
}
