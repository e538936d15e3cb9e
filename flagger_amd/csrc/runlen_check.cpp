// runlen_check.cpp — the stitch of hf_get_run_lengths (hf_runlen_stitch.h) as a stand-alone host program, for
// tests/test_runlen_cpu.py: `make runlen_check` compiles it under the address and undefined-behaviour sanitizers.
//   input (a file named by the first argument, else standard input):
//     L  n_groups
//     per group:  n_parts, then per part:  T  and the rl_part_len(L) numbers of its record (I | Lc | Rc, W | s, e)
//   output: per group one line, the L + 1 bins of the group added to 0.0, as %.17g
#include "hf_runlen_stitch.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
    FILE* in = argc > 1 ? std::fopen(argv[1], "r") : stdin;
    if (!in) { std::fprintf(stderr, "runlen_check: cannot open %s\n", argv[1]); return 2; }
    int L = 0;
    long groups = 0;
    if (std::fscanf(in, "%d %ld", &L, &groups) != 2 || L < 1 || L > 64 || groups < 0) { std::fprintf(stderr, "runlen_check: bad header\n"); return 2; }
    RlStitch st(L);
    std::vector<double> rec(rl_part_len(L)), acc((size_t) L + 1);
    for (long g = 0; g < groups; g++) {
        long parts = 0;
        if (std::fscanf(in, "%ld", &parts) != 1 || parts < 1) { std::fprintf(stderr, "runlen_check: bad group %ld\n", g); return 2; }
        for (double& x : acc) x = 0.0;
        st.begin();
        for (long k = 0; k < parts; k++) {
            long long T = 0;
            if (std::fscanf(in, "%lld", &T) != 1 || T < 1) { std::fprintf(stderr, "runlen_check: bad part\n"); return 2; }
            for (double& x : rec)
                if (std::fscanf(in, "%lf", &x) != 1) { std::fprintf(stderr, "runlen_check: short record\n"); return 2; }
            st.part(rec.data(), (int64_t) T);
        }
        st.end(acc.data());
        for (size_t l = 0; l < acc.size(); l++) std::printf("%.17g%c", acc[l], l + 1 < acc.size() ? ' ' : '\n');
    }
    if (in != stdin) std::fclose(in);
    return 0;
}
