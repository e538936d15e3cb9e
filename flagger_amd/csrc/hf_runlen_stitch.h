// hf_runlen_stitch.h — how hf_get_run_lengths puts the parts of a group of joined chunks together.  Host code only, no HIP header:
// tests/test_runlen_cpu.py compiles it with the host compiler under the sanitizers (runlen_check.cpp), as hf_jobs.h is.
//
// A PART's record, rl_part_len(L) doubles, as k_rl_chain writes it (bin l, 1 <= l <= L + 1, at index l - 1; bin L + 1 is "> L"):
//   I[L + 1]    expected runs of every length that start and end inside the part, touching neither end
//   Lc[L + 1]   the same for the run that starts at the part's first window and ends inside it (left-touching)
//   Rc[L]       expected runs of length d that start behind the first window and are open at the last one
//   W           the probability that the whole part is one run, when its T windows are at most L (else 0.0: it saturated in Lc)
//   s, e        the probabilities that the first and the last window lie in S
// THE STITCH, left to right over the parts of a group, from o[1..L] = 0 (the open run at the end of the parts so far, by length, while
// it is at most L), O = 0 (the probability that their last window lies in S) and N = 0; the chunks are independent given the data:
//   N += I;  N[l'] += o[l'] (1 - s): the open run ends at the boundary
//   for l = 1 .. L + 1:  N[l] += (1 - O) Lc[l];  N[min(l' + l, L + 1)] += o[l'] Lc[l] for l' = 1 .. L
//   T <= L: the new o gets (1 - O) W at T and o[l'] W at l' + T, or N[L + 1] gets the latter where l' + T > L
//   the new o[d] += Rc[d];  O = e
// and after the last part N[l'] += o[l'].  An open run that had saturated was counted where it saturated, so merging with it adds
// nothing.  Every sum runs in the order written here, so a group's bits depend on its parts alone, and a group of one part, added to
// 0.0, is that part's own sum.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

inline size_t rl_part_len(int L) { return 3 * ((size_t) L + 1) + 2; }

struct RlStitch {
    int L;
    std::vector<double> o, on, N;
    double O = 0.0;
    explicit RlStitch(int max_len) : L(max_len), o((size_t) max_len, 0.0), on((size_t) max_len, 0.0), N((size_t) max_len + 1, 0.0) {}

    void begin() {
        for (double& x : o) x = 0.0;
        for (double& x : N) x = 0.0;
        O = 0.0;
    }

    // the next part of the group: its record x and its number of windows T
    void part(const double* x, int64_t T) {
        const size_t n = (size_t) L;
        const double* I = x;
        const double* Lc = x + n + 1;
        const double* Rc = x + 2 * (n + 1);
        const double W = x[2 * (n + 1) + n], s = x[3 * (n + 1)], e = x[3 * (n + 1) + 1];
        for (size_t l = 0; l <= n; l++) N[l] += I[l];
        for (size_t k = 0; k < n; k++) N[k] += o[k] * (1.0 - s);
        for (size_t l = 0; l <= n; l++) {                  // (index l: length l + 1)
            N[l] += (1.0 - O) * Lc[l];
            for (size_t k = 0; k < n; k++) {
                const size_t m = k + l + 1;                // index of the length (k + 1) + (l + 1)
                N[m < n ? m : n] += o[k] * Lc[l];
            }
        }
        for (double& y : on) y = 0.0;
        if (T <= (int64_t) L) {
            on[(size_t) T - 1] += (1.0 - O) * W;
            for (size_t k = 0; k < n; k++) {
                const size_t m = k + (size_t) T;           // index of the length (k + 1) + T
                if (m < n) on[m] += o[k] * W; else N[n] += o[k] * W;
            }
        }
        for (size_t d = 0; d < n; d++) on[d] += Rc[d];
        o.swap(on);
        O = e;
    }

    // closes the group and adds its bins to acc[0 .. L]
    void end(double* acc) {
        for (size_t k = 0; k < (size_t) L; k++) N[k] += o[k];
        for (size_t l = 0; l <= (size_t) L; l++) acc[l] += N[l];
    }
};
