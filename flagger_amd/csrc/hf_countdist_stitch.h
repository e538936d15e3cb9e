// hf_countdist_stitch.h — how hf_get_count_distribution puts the parts of a job together.  Host code only, no HIP header:
// tests/test_countdist_cpu.py compiles it with the host compiler under the sanitizers (countdist_check.cpp), as hf_runlen_stitch.h is.
//
// A PART's record, cd_part_len(K) = K + 2 doubles, as k_cd_chain writes it: d[k] = P(N = k | data) of the part's windows, k = 0 .. K, and
// d[K + 1] = P(N > K | data).
// THE STITCH.  Chunks are independent given the data, so a job's distribution is the truncated convolution of its parts' distributions,
// left to right in chunk order.  The first part is taken as it is (a job of one part is that part, bit for bit); every further part d is
// folded into the distribution acc of the parts so far:
//   k = 0 .. K:  new[k]     = sum_{j = 0 .. k} acc[j] d[k - j]                  one accumulator from 0.0, j ascending
//   "> K":       new[K + 1] = sum_{j = 0 .. K + 1} acc[j] r_j,  r_j = sum_{m = K + 1 - j .. K + 1} d[m]
// where r_j is ONE running tail sum that takes d[K + 1 - j] at step j (so it adds d downwards from "> K": r_0 = 0.0 + d[K + 1]) and the
// outer sum is one accumulator from 0.0, j ascending.  Index K + 1 of acc is its own "> K" bin, which meets every bin of d (r_{K+1} is
// the whole of d).  Sums of non-negative products only: "> K" is never formed as 1 - sum, a bin that no pair of non-zero bins reaches is
// exactly 0.0, and a job's bits depend on its parts alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

inline size_t cd_part_len(int K) { return (size_t) K + 2; }

struct CdStitch {
    int K;
    bool any = false;
    std::vector<double> acc, nw;
    explicit CdStitch(int max_count) : K(max_count), acc((size_t) max_count + 2, 0.0), nw((size_t) max_count + 2, 0.0) {}

    void begin() { any = false; }

    // the next part of the job: its record d
    void part(const double* d) {
        const size_t B = (size_t) K + 2;
        if (!any) {
            for (size_t k = 0; k < B; k++) acc[k] = d[k];
            any = true;
            return;
        }
        for (size_t k = 0; k + 1 < B; k++) {
            double s = 0.0;
            for (size_t j = 0; j <= k; j++) s += acc[j] * d[k - j];
            nw[k] = s;
        }
        double s = 0.0, r = 0.0;
        for (size_t j = 0; j < B; j++) {
            r += d[B - 1 - j];
            s += acc[j] * r;
        }
        nw[B - 1] = s;
        acc.swap(nw);
    }

    // writes the job's K + 2 bins (a job without a part has no window: N = 0)
    void end(double* out) const {
        const size_t B = (size_t) K + 2;
        for (size_t k = 0; k < B; k++) out[k] = any ? acc[k] : (k == 0 ? 1.0 : 0.0);
    }
};
