// scopes_check — the command line's chunk-list rules (hf_cli_scopes.h) on the host alone, for tests/test_cli_scopes_cpu.py (make
// scopes_check: built with the address and undefined-behaviour sanitizers).
//   scopes_check FILE    FILE: the number of chunks C, the C + 1 offsets, the C contig names (whitespace-separated)
// Prints, one line each:
//   joined j0 j1 ...                       joined_by_contig (max(C, 1) entries)
//   names n0 n1 ...                        the scopes in order ("all" first)
//   scope_of_chunk s0 s1 ...
//   runs <scope index> c0 c1 ...           the scope's chunk runs [c0, c1), flattened; then
//   ranges <scope index> a b ...           its window ranges [a, b), flattened
//   group_end e0 e1 ...                    group_end for every start c0 = 0 .. C - 1
#include "hf_cli_scopes.h"
#include <cstdio>

int main(int argc, char** argv) {
    FILE* f = argc == 2 ? std::fopen(argv[1], "r") : nullptr;
    if (!f) { std::fprintf(stderr, "usage: scopes_check FILE\n"); return 2; }
    int C = 0;
    if (std::fscanf(f, "%d", &C) != 1 || C < 0) return 2;
    std::vector<int64_t> off((size_t) C + 1);
    for (auto& o : off) { long long v; if (std::fscanf(f, "%lld", &v) != 1) return 2; o = v; }
    ChunkList l;
    l.C = C; l.off = off.data();
    for (int c = 0; c < C; c++) {
        char name[256];
        if (std::fscanf(f, "%255s", name) != 1) return 2;
        l.ctg.push_back(name);
    }
    std::fclose(f);
    const std::vector<uint8_t> joined = joined_by_contig(l);
    const Scopes s = contig_scopes(l);
    std::printf("joined");
    for (uint8_t j : joined) std::printf(" %d", (int) j);
    std::printf("\nnames");
    for (const Scope& sc : s.scopes) std::printf(" %s", sc.name.c_str());
    std::printf("\nscope_of_chunk");
    for (size_t i : s.scope_of_chunk) std::printf(" %zu", i);
    std::printf("\n");
    for (size_t i = 0; i < s.scopes.size(); i++) {
        std::printf("runs %zu", i);
        for (const auto& r : s.scopes[i].runs) std::printf(" %d %d", r.first, r.second);
        std::printf("\nranges %zu", i);
        for (const auto& r : s.scopes[i].ranges) std::printf(" %lld %lld", (long long) r.first, (long long) r.second);
        std::printf("\n");
    }
    std::printf("group_end");
    for (int c = 0; c < C; c++) std::printf(" %d", group_end(l, joined.data(), c));
    std::printf("\n");
    return 0;
}
