// countdist_check.cpp — the stitch of hf_get_count_distribution (hf_countdist_stitch.h) as a stand-alone host program, for
// tests/test_countdist_cpu.py: `make countdist_check` compiles it under the address and undefined-behaviour sanitizers.
//   input (a file named by the first argument, else standard input):
//     K  n_jobs
//     per job:  n_parts, then per part the cd_part_len(K) = K + 2 numbers of its record (p_0 .. p_K, p_gtK)
//   output: per job one line, its K + 2 bins, as %.17g
#include "hf_countdist_stitch.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
    FILE* in = argc > 1 ? std::fopen(argv[1], "r") : stdin;
    if (!in) { std::fprintf(stderr, "countdist_check: cannot open %s\n", argv[1]); return 2; }
    int K = 0;
    long jobs = 0;
    if (std::fscanf(in, "%d %ld", &K, &jobs) != 2 || K < 1 || K > 62 || jobs < 0) { std::fprintf(stderr, "countdist_check: bad header\n"); return 2; }
    CdStitch st(K);
    std::vector<double> rec(cd_part_len(K)), acc(cd_part_len(K));
    for (long g = 0; g < jobs; g++) {
        long parts = 0;
        if (std::fscanf(in, "%ld", &parts) != 1 || parts < 0) { std::fprintf(stderr, "countdist_check: bad job %ld\n", g); return 2; }
        st.begin();
        for (long k = 0; k < parts; k++) {
            for (double& x : rec)
                if (std::fscanf(in, "%lf", &x) != 1) { std::fprintf(stderr, "countdist_check: short record\n"); return 2; }
            st.part(rec.data());
        }
        st.end(acc.data());
        for (size_t l = 0; l < acc.size(); l++) std::printf("%.17g%c", acc[l], l + 1 < acc.size() ? ' ' : '\n');
    }
    if (in != stdin) std::fclose(in);
    return 0;
}
