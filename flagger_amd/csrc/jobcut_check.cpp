// jobcut_check — the range getters' job cutter (hf_jobs.h) on the host alone, for tests/test_jobcut_cpu.py (make jobcut_check: built with
// the address and undefined-behaviour sanitizers).
//   jobcut_check FILE    FILE: cap_pieces cap_parts, the number of chunk offsets and the offsets, the number of jobs and every job's
//                        first and last window (whitespace-separated integers)
// Prints rows of seven integers, batch by batch:
//   0 job batch n_parts n_pieces 0 0      a job and the device batch it lands in
//   1 job chunk a b p0 p1                 its parts, in order, each followed by
//   2 job chunk t n g k                   the part's pieces: windows t .. t + n - 1, g = the piece's index and k = the part's in the batch
// Before that, on every run, the join rule (part_joined, group_parts) and chunk_continues against answers written out by hand: a wrong one goes to stderr and ends it with status 3.
#include "hf_jobs.h"
#include <cstdio>
#include <string>

struct Piece { long long t; int n, c; long long job; };
struct Part { long long a, b; int p0, p1, c; long long job; };
struct Group { long long q0, q1; };
static Part mk_part(int64_t j, int c, int64_t a, int64_t b) { return Part{a, b, 0, 0, c, j}; }
static Piece mk_piece(const Part& pt, int64_t t, int len) { return Piece{t, len, pt.c, pt.job}; }

// One call of jobs on the chunk offsets `off`; want: a letter per part in order, 'J' joined to the part before it, '.' not.  The groups
// must begin exactly at the '.' parts.
static bool join_case(const char* name, std::vector<int64_t> off, std::vector<int64_t> first, std::vector<int64_t> last, const uint8_t* joined,
                      const std::string& want) {
    JobCut<Piece, Part, 512> jc;
    jc.cut(off, (int64_t) first.size(), first.data(), last.data(), 0, 1 << 20, 1 << 20, mk_part, mk_piece);
    std::vector<Group> groups; std::vector<int64_t> job_g0;
    group_parts(jc.parts, jc.job_p0, joined, groups, job_g0, [](int64_t, int64_t q0, int64_t q1) { return Group{q0, q1}; });
    std::string got, heads(jc.parts.size(), 'J');
    for (size_t j = 0; j + 1 < jc.job_p0.size(); j++)
        for (int64_t k = jc.job_p0[j]; k < jc.job_p0[j + 1]; k++) got += part_joined(jc.parts.data(), k, jc.job_p0[j], joined) ? 'J' : '.';
    for (const Group& g : groups) heads[(size_t) g.q0] = '.';
    const bool ok = got == want && heads == want && job_g0.size() == jc.job_p0.size();
    if (!ok) std::fprintf(stderr, "join rule, %s: want %s, part_joined %s, group_parts %s\n", name, want.c_str(), got.c_str(), heads.c_str());
    return ok;
}

// chunks 0 .. 4 of ten windows, chunk 2 without windows; and three chunks of ten
static bool join_rule() {
    const std::vector<int64_t> gap{0, 10, 20, 20, 30, 40}, three{0, 10, 20, 30};
    const uint8_t all5[] = {0, 1, 1, 1, 1}, some5[] = {0, 0, 1, 1, 0}, all3[] = {0, 1, 1};
    bool ok = join_case("joined == nullptr", gap, {0}, {39}, nullptr, "....");
    ok &= join_case("a chunk without windows ends the sequence", gap, {0}, {39}, all5, ".J.J");
    ok &= join_case("joined[c] == 0", gap, {0}, {39}, some5, "....");
    ok &= join_case("three chunks all joined", three, {0}, {29}, all3, ".JJ");
    // (the first parts of jobs 2 and 3 follow, in the batch, a part of the chunk before theirs, which theirs continues)
    ok &= join_case("a job's first part", three, {10, 0, 10, 25}, {29, 9, 19, 25}, all3, ".J...");
    // chunk_continues, a letter per chunk: the chunk without windows continues nothing and nothing continues it
    auto continues = [&](const char* name, const std::vector<int64_t>& off, const uint8_t* joined, const std::string& want) {
        const int64_t C = (int64_t) off.size() - 1;
        std::string got;
        for (int64_t c = 0; c < C; c++) got += chunk_continues(off.data(), C, joined, c) ? 'J' : '.';
        const bool good = got == want && !chunk_continues(off.data(), C, joined, C);      // (behind the list: nothing)
        if (!good) std::fprintf(stderr, "chunk_continues, %s: want %s, got %s\n", name, want.c_str(), got.c_str());
        return good;
    };
    ok &= continues("joined == nullptr", gap, nullptr, ".....");
    ok &= continues("a chunk without windows", gap, all5, ".J..J");
    ok &= continues("joined[c] == 0", gap, some5, ".....");
    ok &= continues("three chunks all joined", three, all3, ".JJ");
    return ok;
}

int main(int argc, char** argv) {
    if (!join_rule()) return 3;
    FILE* f = argc == 2 ? std::fopen(argv[1], "r") : nullptr;
    if (!f) { std::fprintf(stderr, "usage: jobcut_check FILE\n"); return 2; }
    long long cap_pieces, cap_parts, n_off, n;
    if (std::fscanf(f, "%lld %lld %lld", &cap_pieces, &cap_parts, &n_off) != 3 || cap_pieces < 1 || cap_parts < 1 || n_off < 2) return 2;
    std::vector<int64_t> off((size_t) n_off);
    for (auto& o : off) { long long v; if (std::fscanf(f, "%lld", &v) != 1) return 2; o = v; }
    if (std::fscanf(f, "%lld", &n) != 1 || n < 0) return 2;
    std::vector<int64_t> first((size_t) n), last((size_t) n);
    for (long long j = 0; j < n; j++) {
        long long a, b;
        if (std::fscanf(f, "%lld %lld", &a, &b) != 2 || a < off.front() || a > b || b >= off.back()) return 2;
        first[(size_t) j] = a; last[(size_t) j] = b;
    }
    std::fclose(f);
    JobCut<Piece, Part, 512> jc;
    int batch = 0;
    for (int64_t j0 = 0; j0 < n; batch++) {
        const int64_t j1 = jc.cut(off, n, first.data(), last.data(), j0, (size_t) cap_pieces, (size_t) cap_parts, mk_part, mk_piece);
        for (int64_t j = j0; j < j1; j++) {
            const int64_t k0 = jc.job_p0[(size_t) (j - j0)], k1 = jc.job_p0[(size_t) (j - j0) + 1];
            std::printf("0 %lld %d %lld %d 0 0\n", (long long) j, batch, (long long) (k1 - k0), jc.parts[(size_t) k1 - 1].p1 - jc.parts[(size_t) k0].p0);
            for (int64_t k = k0; k < k1; k++) {
                const Part& pt = jc.parts[(size_t) k];
                std::printf("1 %lld %d %lld %lld %d %d\n", pt.job, pt.c, pt.a, pt.b, pt.p0, pt.p1);
                for (int g = pt.p0; g < pt.p1; g++) {
                    const Piece& pc = jc.pieces[(size_t) g];
                    std::printf("2 %lld %d %lld %d %d %lld\n", pc.job, pc.c, pc.t, pc.n, g, (long long) k);
                }
            }
        }
        j0 = j1;
    }
    return 0;
}
