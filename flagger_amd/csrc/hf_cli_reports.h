// hf_cli_reports.h — the report files behind the final BED (late_outputs of hf_cli.cpp, which includes this header where the writers
// stood): one context (Report), one job list (Jobs), one table file (TableFile); the scopes "all" + every contig, the joined chunks, the
// label sets and the label names come from hf_cli_scopes.h.  Every writer returns an HF_* code and leaves the text of an error of its own
// in hf_cli_set_error.  Part of hf_cli.cpp's translation unit: it stands behind Run, Region and hf_cli_set_error.

// the table's chunk list for hf_cli_scopes.h
static ChunkList chunk_list(const hfio_table* tab, const hf_windows& w) {
    ChunkList l;
    l.C = w.n_chunks; l.off = w.chunk_off;
    for (int c = 0; c < l.C; c++) l.ctg.push_back(hfio_chunk_ctg(tab, c));
    return l;
}

// a table file: open() and close() report "<path> cannot be opened" / "cannot be written" (HF_E_ARG); what an early return leaves open is
// closed without a word
struct TableFile {
    std::string path;
    FILE* f = nullptr;
    TableFile() = default;
    TableFile(const TableFile&) = delete;
    ~TableFile() { if (f) fclose(f); }
    int open(const std::string& p) {
        path = p;
        f = fopen(p.c_str(), "w");
        if (!f) hf_cli_set_error(path + " cannot be opened");
        return f ? HF_OK : HF_E_ARG;
    }
    int close() {
        FILE* const g = f;
        f = nullptr;
        if (g && fclose(g) != 0) { hf_cli_set_error(path + " cannot be written"); return HF_E_ARG; }
        return HF_OK;
    }
    operator FILE*() const { return f; }
};

// the jobs of a getter call: windows [a, b) in, the getters' first / last out
struct Jobs {
    std::vector<int64_t> first, last;
    std::vector<uint8_t> mask;
    void add(int64_t a, int64_t b, unsigned m = 0) { first.push_back(a); last.push_back(b - 1); mask.push_back((uint8_t) m); }
    int64_t n() const { return (int64_t) first.size(); }
};

// window i of chunk c covers [s + i W, min(s + (i+1) W - 1, e)]: its number of bases and its region
static void window_bases(const hf_windows& w, int C, std::vector<int64_t>& wbases, std::vector<int32_t>& wreg) {
    wbases.assign((size_t) w.n_windows, 0);
    wreg.assign((size_t) w.n_windows, 0);
    for (int c = 0; c < C; c++)
        for (int64_t t = w.chunk_off[c]; t < w.chunk_off[c + 1]; t++) {
            const int64_t i = t - w.chunk_off[c];
            const int64_t s = (int64_t) w.chunk_s[c] + i * w.window_len;
            const int64_t e = std::min<int64_t>((int64_t) w.chunk_s[c] + (i + 1) * w.window_len - 1, (int64_t) w.chunk_e[c]);
            wbases[(size_t) t] = e - s + 1;
            wreg[(size_t) t] = (int32_t) (w.annot[t] >> 58);
        }
}

// the runs of the final labels (final_label_runs_support.bed, final_label_runs_confidence.bed): a new run where the label changes or a
// chunk starts a different contig; windows a .. b - 1, bases s .. e; runOf: every window's run
struct LRun { int64_t a, b; int label; int64_t s, e; const char* ctg; };
static std::vector<LRun> label_runs(const hfio_table* tab, const hf_windows& w, int C, const std::vector<int64_t>& wbases,
                                    const int8_t* finalLabels, std::vector<int32_t>& runOf) {
    std::vector<LRun> runs;
    runOf.assign((size_t) w.n_windows, 0);
    const char* preCtg = nullptr;
    for (int c = 0; c < C; c++) {
        const char* ctg = hfio_chunk_ctg(tab, c);
        for (int64_t t = w.chunk_off[c]; t < w.chunk_off[c + 1]; t++) {
            const int64_t i = t - w.chunk_off[c];
            const int64_t s = (int64_t) w.chunk_s[c] + i * w.window_len;
            const int64_t e = s + wbases[(size_t) t] - 1;
            const bool newCtg = t == w.chunk_off[c] && (!preCtg || strcmp(preCtg, ctg) != 0);
            if (runs.empty() || newCtg || runs.back().label != finalLabels[t]) runs.push_back(LRun{t, t, finalLabels[t], s, e, ctg});
            runs.back().b = t + 1; runs.back().e = e;
            runOf[(size_t) t] = (int32_t) (runs.size() - 1);
            if (t == w.chunk_off[c]) preCtg = ctg;
        }
    }
    return runs;
}

// The windows of every region (those whose bases meet [start, end) on the region's contig), sorted, and the same as maximal ranges
// [a, b) of consecutive window indices; a region on an unknown contig has none.
struct RegionWindows {
    std::vector<std::vector<int64_t>> wins;
    std::vector<std::vector<std::pair<int64_t, int64_t>>> ranges;
};
static RegionWindows region_windows(const hfio_table* tab, const hf_windows& w, int C, const std::vector<int64_t>& wbases, const std::vector<Region>& regions) {
    // every contig's windows in base order: (first base, last base, window)
    std::map<std::string, std::vector<std::array<int64_t, 3>>> byCtg;
    for (int c = 0; c < C; c++) {
        auto& v = byCtg[hfio_chunk_ctg(tab, c)];
        for (int64_t t = w.chunk_off[c]; t < w.chunk_off[c + 1]; t++) {
            const int64_t s = (int64_t) w.chunk_s[c] + (t - w.chunk_off[c]) * w.window_len;
            v.push_back({s, s + wbases[(size_t) t] - 1, t});
        }
    }
    for (auto& kv : byCtg) std::sort(kv.second.begin(), kv.second.end());
    RegionWindows rw;
    rw.wins.assign(regions.size(), {});
    rw.ranges.assign(regions.size(), {});
    for (size_t i = 0; i < regions.size(); i++) {
        const Region& g = regions[i];
        auto it = byCtg.find(g.ctg);
        if (it == byCtg.end()) continue;
        for (const auto& x : it->second)
            if (x[0] < g.end && x[1] >= g.start) rw.wins[i].push_back(x[2]);
        std::sort(rw.wins[i].begin(), rw.wins[i].end());
        for (int64_t t : rw.wins[i]) {
            if (!rw.ranges[i].empty() && rw.ranges[i].back().second == t) rw.ranges[i].back().second = t + 1;
            else rw.ranges[i].push_back({t, t + 1});
        }
    }
    return rw;
}

// What every report of a run reads: the context and the table, the final labels, the windows' bases and regions, the chunk list with its
// scopes and joins.  The label runs and the region windows are host work that several reports share: made at first use, then kept.
struct Report {
    hf_ctx* const ctx;
    hfio_table* const tab;
    const hf_windows& w;
    const int64_t N;
    const int C, R;
    const int8_t* const labels;                       // the final labels
    const std::vector<Region>* const regions;         // --regionProbs, or null
    const int32_t* const minLen;                      // --minimumLengths in windows
    const std::vector<std::string>& labelNames;
    const std::string& dir;
    std::vector<int64_t> wbases;
    std::vector<int32_t> wreg;
    const ChunkList list;
    const std::vector<uint8_t> joined;
    const Scopes sc;
    Report(Run& s, const int8_t* finalLabels, const std::string& outDir)
        : ctx(s.ctx), tab(s.tab), w(s.w), N(s.N), C(s.w.n_chunks), R(hfio_n_regions(s.tab)), labels(finalLabels),
          regions(s.opt.regionProbsPath ? &s.regions : nullptr), minLen(s.minLenWindows), labelNames(s.opt.labelNames), dir(outDir),
          list(chunk_list(s.tab, s.w)), joined(joined_by_contig(list)), sc(contig_scopes(list)) {
        window_bases(w, C, wbases, wreg);
    }
    const std::vector<LRun>& runs() {
        if (!haveRuns) { runs_ = label_runs(tab, w, C, wbases, labels, runOf_); haveRuns = true; }
        return runs_;
    }
    const std::vector<int32_t>& runOf() { runs(); return runOf_; }
    const RegionWindows& regionWindows() {
        if (!haveRegionWindows) { regionWindows_ = region_windows(tab, w, C, wbases, *regions); haveRegionWindows = true; }
        return regionWindows_;
    }
    const char* state_name(int l) const { return state_column_name(labelNames, (size_t) l); }
    // one job per label set for every run with windows of every scope (--numBlocks, --runLengths), in the order their sums are read in
    Jobs run_jobs() const {
        Jobs jobs;
        for (const Scope& s : sc.scopes)
            for (const auto& rg : s.runs) {
                if (list.no_windows(rg.first, rg.second)) continue;
                for (int k = 0; k < 5; k++) jobs.add(w.chunk_off[rg.first], w.chunk_off[rg.second], kLabelSets[k]);
            }
        return jobs;
    }
private:
    bool haveRuns = false, haveRegionWindows = false;
    std::vector<LRun> runs_;
    std::vector<int32_t> runOf_;
    RegionWindows regionWindows_;
};

// --uncertaintySamples: N posterior path samples (hf_sample_paths) with the final parameters, reduced on the host per sample as each
// group of hf_sample_capacity samples comes down.  Two files:
//   posterior_samples_summary.tsv   per (region, label): the final labels' bases, and over the samples the mean, standard deviation
//                                   (divisor N - 1) and the values at index floor(q (N-1)) of the sorted N (q = 0.025, 0.5, 0.975) of the
//                                   bases, and the mean of the windows; region "all", then region_<r>
//   final_label_runs_support.bed    per maximal run of equal final label over consecutive windows of one contig (the runs of
//                                   hfio_write_final_bed before --minimumLengths): the fraction of samples in which the whole run has
//                                   that label, and the mean over samples of the fraction of its windows that have it
// The sampler: capacity() = samples per call (< 1: none fit, or an HF_E_* code), draw(p, first, n) = the call and its finish,
// labels(k, out) = sample k of the last call.  --admissibleSamples writes the same two files from hf_sample_paths_minlen.
struct PathSampler {
    std::function<int()> capacity;
    std::function<int(const hf_params*, int64_t, int)> draw;
    std::function<int(int, int8_t*)> labels;
};
static int write_sample_outputs(Report& r, const PathSampler& smp, hfm_model* model, int nSamples, const char* summaryName, const char* supportName) {
    const int64_t N = r.N;
    const std::vector<int64_t>& wbases = r.wbases;
    const std::vector<int32_t>&wreg = r.wreg, &runOf = r.runOf();
    const std::vector<LRun>& runs = r.runs();
    const int8_t* const finalLabels = r.labels;
    const size_t G = (size_t) r.R + 1, NR = runs.size();
    std::vector<int64_t> basesS((size_t) nSamples * G * 4), winS(G * 4, 0), cnt(NR);
    std::vector<double> support(NR, 0.0), meanFrac(NR, 0.0);
    std::vector<int64_t> basesFinal(G * 4, 0);
    for (int64_t t = 0; t < N; t++) {
        const int l = finalLabels[t];
        if (l < 0 || l > 3) continue;
        basesFinal[(size_t) l] += wbases[(size_t) t];
        basesFinal[((size_t) wreg[(size_t) t] + 1) * 4 + (size_t) l] += wbases[(size_t) t];
    }
    std::vector<int8_t> lab((size_t) N);
    hf_params p;
    hfm_params(model, &p);
    const int cap = smp.capacity();
    if (cap < 1) return cap < 0 ? cap : HF_E_ARG;
    for (int k0 = 0; k0 < nSamples; k0 += cap) {
        const int n = std::min(cap, nSamples - k0);
        int rc = smp.draw(&p, k0, n);
        if (rc != HF_OK) return rc;
        for (int k = 0; k < n; k++) {
            if ((rc = smp.labels(k, lab.data())) != HF_OK) return rc;
            int64_t* b = basesS.data() + (size_t) (k0 + k) * G * 4;
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int64_t t = 0; t < N; t++) {
                const size_t l = (size_t) lab[(size_t) t], g = (size_t) wreg[(size_t) t] + 1;
                b[l] += wbases[(size_t) t]; b[g * 4 + l] += wbases[(size_t) t];
                winS[l]++; winS[g * 4 + l]++;
                const int32_t ri = runOf[(size_t) t];
                cnt[(size_t) ri] += (int) l == runs[(size_t) ri].label;
            }
            for (size_t ri = 0; ri < NR; ri++) {
                const int64_t len = runs[ri].b - runs[ri].a;
                support[ri] += cnt[ri] == len;
                meanFrac[ri] += (double) cnt[ri] / (double) len;
            }
        }
    }
    TableFile f;
    int rc = f.open(r.dir + "/" + summaryName);
    if (rc != HF_OK) return rc;
    fprintf(f, "#Region\tLabel\tBases_Final\tBases_Mean\tBases_SD\tBases_Q025\tBases_Q500\tBases_Q975\tWindows_Mean\n");
    std::vector<int64_t> v((size_t) nSamples);
    for (size_t g = 0; g < G; g++)
        for (size_t l = 0; l < 4; l++) {
            double mean = 0.0, ss = 0.0;
            for (int k = 0; k < nSamples; k++) { v[(size_t) k] = basesS[((size_t) k * G + g) * 4 + l]; mean += (double) v[(size_t) k]; }
            mean /= nSamples;
            for (int k = 0; k < nSamples; k++) ss += ((double) v[(size_t) k] - mean) * ((double) v[(size_t) k] - mean);
            const double sd = nSamples > 1 ? std::sqrt(ss / (nSamples - 1)) : 0.0;
            std::sort(v.begin(), v.end());
            auto q = [&](double x) { return v[(size_t) std::floor(x * (nSamples - 1))]; };
            const std::string region = g == 0 ? std::string("all") : "region_" + std::to_string(g - 1);
            fprintf(f, "%s\t%s\t%ld\t%.4f\t%.4f\t%ld\t%ld\t%ld\t%.4f\n", region.c_str(), r.state_name((int) l), (long) basesFinal[g * 4 + l], mean, sd,
                    (long) q(0.025), (long) q(0.5), (long) q(0.975), (double) winS[g * 4 + l] / nSamples);
        }
    if ((rc = f.close()) != HF_OK || (rc = f.open(r.dir + "/" + supportName)) != HF_OK) return rc;
    fprintf(f, "#ctg\tstart\tend\tlabel\tsupport\tmean_fraction\n");
    for (size_t ri = 0; ri < NR; ri++)
        fprintf(f, "%s\t%ld\t%ld\t%s\t%.4f\t%.4f\n", runs[ri].ctg, (long) runs[ri].s, (long) runs[ri].e + 1, run_label_name(runs[ri].label),
                support[ri] / nSamples, meanFrac[ri] / nSamples);
    return f.close();
}

// --runConfidence / --regionProbs: exact label probabilities of windows ranges (hf_get_interval_log_probs) under the model of the last
// full pass, and the mean posterior (hf_get_posterior).
//   final_label_runs_confidence.bed    per run of final_label_runs_support.bed (same rows, same order): p_all = P(every window has the
//                                      run's label), qual = min(100, -10 log10(1 - p_all)), mean_posterior of that label
//   region_label_probabilities.tsv     per region (file order), for every label L: p_any_L = P(some window has L), p_all_L, mean_L over
//                                      the windows whose bases meet [start, end) (a union of index ranges: the sum of their logs)
static int write_interval_outputs(Report& r, bool runConfidence) {
    const int64_t N = r.N;
    std::vector<double> post((size_t) N * 4);
    int rc = N > 0 ? hf_get_posterior(r.ctx, 0, N, post.data()) : HF_OK;
    if (rc != HF_OK) return rc;
    auto mean_post = [&](int64_t a, int64_t b, int l) {   // windows a .. b - 1
        double m = 0.0;
        for (int64_t t = a; t < b; t++) m += post[(size_t) t * 4 + (size_t) l];
        return m / (double) (b - a);
    };
    if (runConfidence) {
        const std::vector<LRun>& runs = r.runs();
        Jobs jobs;
        for (const LRun& run : runs)
            if (run.label >= 0 && run.label < 4) jobs.add(run.a, run.b, 1u << run.label);
        std::vector<double> lp((size_t) jobs.n());
        if ((rc = hf_get_interval_log_probs(r.ctx, jobs.n(), jobs.first.data(), jobs.last.data(), jobs.mask.data(), lp.data())) != HF_OK) return rc;
        TableFile f;
        if ((rc = f.open(r.dir + "/final_label_runs_confidence.bed")) != HF_OK) return rc;
        fprintf(f, "#ctg\tstart\tend\tlabel\tp_all\tqual\tmean_posterior\n");
        size_t k = 0;
        for (const LRun& run : runs) {
            const bool lab = run.label >= 0 && run.label < 4;
            fprintf(f, "%s\t%ld\t%ld\t%s\t", run.ctg, (long) run.s, (long) run.e + 1, run_label_name(run.label));
            if (!lab) { fprintf(f, "NA\tNA\tNA\n"); continue; }
            const double l = lp[k++];
            const double miss = -std::expm1(l);
            const double qual = miss > 0.0 ? std::min(100.0, -10.0 * std::log10(miss)) + 0.0 : 100.0;
            fprintf(f, "%.6g\t%.2f\t%.6f\n", std::exp(l), qual, mean_post(run.a, run.b, run.label));
        }
        if ((rc = f.close()) != HF_OK) return rc;
    }
    if (r.regions) {
        // the windows of every region, as maximal index ranges; one job per range and mask (Err..Col alone, and all but each)
        const RegionWindows& rw = r.regionWindows();
        Jobs jobs;
        for (const auto& ranges : rw.ranges)
            for (const auto& rg : ranges)
                for (int m = 0; m < 8; m++) jobs.add(rg.first, rg.second, m < 4 ? 1u << m : 15u & ~(1u << (m - 4)));
        std::vector<double> lp((size_t) jobs.n());
        if ((rc = hf_get_interval_log_probs(r.ctx, jobs.n(), jobs.first.data(), jobs.last.data(), jobs.mask.data(), lp.data())) != HF_OK) return rc;
        TableFile f;
        if ((rc = f.open(r.dir + "/region_label_probabilities.tsv")) != HF_OK) return rc;
        fprintf(f, "#ctg\tstart\tend\tname\tn_windows");
        for (int l = 0; l < 4; l++) fprintf(f, "\tp_any_%s\tp_all_%s\tmean_%s", r.state_name(l), r.state_name(l), r.state_name(l));
        fprintf(f, "\n");
        size_t k = 0;
        for (size_t i = 0; i < r.regions->size(); i++) {
            const Region& g = (*r.regions)[i];
            const std::vector<int64_t>& wins = rw.wins[i];
            fprintf(f, "%s\t%ld\t%ld\t%s\t%zu", g.ctg.c_str(), (long) g.start, (long) g.end, g.name.c_str(), wins.size());
            double all[4] = {0, 0, 0, 0}, none[4] = {0, 0, 0, 0};     // sums over the ranges, range order
            for (size_t q = 0; q < rw.ranges[i].size(); q++, k += 8)
                for (int l = 0; l < 4; l++) { all[l] += lp[k + (size_t) l]; none[l] += lp[k + 4 + (size_t) l]; }
            for (int l = 0; l < 4; l++) {
                if (wins.empty()) { fprintf(f, "\tNA\tNA\tNA"); continue; }
                double m = 0.0;
                for (int64_t t : wins) m += post[(size_t) t * 4 + (size_t) l];
                fprintf(f, "\t%.6g\t%.6g\t%.6f", -std::expm1(none[l]) + 0.0, std::exp(all[l]), m / (double) wins.size());
            }
            fprintf(f, "\n");
        }
        if ((rc = f.close()) != HF_OK) return rc;
    }
    return HF_OK;
}

// --exactTotals: exact posterior mean and standard deviation of the label totals (hf_get_count_moments, HF_COUNT_BASES) under the model
// of the last full pass.
//   label_totals_exact.tsv   one row per scope and label set.  Scopes: those of hf_cli_scopes.h (a contig's chunks are independent
//                            chains, so its mean and variance are the sums over its ranges), then region_<r> for every annotation
//                            region (the whole track with the region filter r).  Label sets: Err, Dup, Hap, Col, Err+Dup+Col.  Columns:
//                            windows (of the scope), bases_final_labels (bases whose final label lies in the set), bases_expected, bases_sd.
static int write_exact_totals(Report& r) {
    struct Filtered { const Scope* sc; std::string name; int region; };      // a scope with its region filter
    std::vector<Filtered> scopes;
    for (const Scope& sc : r.sc.scopes) scopes.push_back(Filtered{&sc, sc.name, -1});
    for (int g = 0; g < r.R; g++) scopes.push_back(Filtered{&r.sc.scopes[0], "region_" + std::to_string(g), g});
    Jobs jobs;
    std::vector<int32_t> region;
    for (const Filtered& sc : scopes)
        for (const auto& rg : sc.sc->ranges)
            for (int k = 0; k < 5; k++) { jobs.add(rg.first, rg.second, kLabelSets[k]); region.push_back(sc.region); }
    std::vector<double> mean((size_t) jobs.n()), var((size_t) jobs.n());
    int rc = hf_get_count_moments(r.ctx, jobs.n(), jobs.first.data(), jobs.last.data(), jobs.mask.data(), region.data(), HF_COUNT_BASES,
                                  mean.data(), var.data());
    if (rc != HF_OK) return rc;
    TableFile f;
    if ((rc = f.open(r.dir + "/label_totals_exact.tsv")) != HF_OK) return rc;
    fprintf(f, "#scope\tlabel_set\twindows\tbases_final_labels\tbases_expected\tbases_sd\n");
    size_t j = 0;
    for (const Filtered& sc : scopes) {
        int64_t windows = 0, finalBases[5] = {0, 0, 0, 0, 0};
        double m[5] = {0, 0, 0, 0, 0}, v[5] = {0, 0, 0, 0, 0};       // sums over the ranges, list order
        for (const auto& rg : sc.sc->ranges) {
            for (int64_t t = rg.first; t < rg.second; t++) {
                if (sc.region >= 0 && r.wreg[(size_t) t] != sc.region) continue;
                windows++;
                const int l = r.labels[t];
                if (l < 0 || l > 3) continue;
                for (int k = 0; k < 5; k++) if ((kLabelSets[k] >> l) & 1) finalBases[k] += r.wbases[(size_t) t];
            }
            for (int k = 0; k < 5; k++, j++) { m[k] += mean[j]; v[k] += var[j]; }
        }
        for (int k = 0; k < 5; k++)
            fprintf(f, "%s\t%s\t%ld\t%ld\t%.10g\t%.10g\n", sc.name.c_str(), kLabelSetNames[k], (long) windows, (long) finalBases[k], m[k], std::sqrt(v[k]));
    }
    return f.close();
}

// --runBoundaries: the exact posterior of the position of every boundary between two runs of the final labels (hf_get_breakpoints,
// hf_get_breakpoint_profile) under the model of the last full pass.
//   final_label_run_boundaries.tsv   one row per two adjacent runs of final_label_runs_support.bed on one contig, in run order.  With m the
//                                    first window of the right run and m - 1, m in one chunk, the job is first = max(start of the left
//                                    run, first window of the chunk), last = min(end of the right run, last window of the chunk), U =
//                                    {left label}, V = {right label}: p_event = P(the range switches exactly once, U -> V), and given
//                                    that, p_called = p_m, lo / median / hi = the 2.5 / 50 / 97.5 % quantiles and mode, mode_p.  pos, lo,
//                                    median, hi and mode are the first base of the window named.  A boundary at a chunk start, and a job
//                                    without weight, have NA from p_event on.
static int write_run_boundaries(Report& r) {
    const hf_windows& w = r.w;
    const std::vector<LRun>& runs = r.runs();
    auto chunk_of = [&](int64_t t) { return (int) (std::upper_bound(w.chunk_off, w.chunk_off + r.C + 1, t) - w.chunk_off) - 1; };
    auto base_of = [&](int c, int64_t t) { return (long) ((int64_t) w.chunk_s[c] + (t - w.chunk_off[c]) * w.window_len); };
    Jobs jobs;                                                          // mask: the left label's, vm: the right one's
    std::vector<uint8_t> vm;
    std::vector<int> job(runs.size(), -1), chunk(runs.size(), 0);      // of the boundary between runs i - 1 and i
    for (size_t i = 1; i < runs.size(); i++) {
        const LRun &l = runs[i - 1], &rt = runs[i];
        const int c = chunk_of(rt.a);
        chunk[i] = c;
        if (l.b != rt.a || rt.a == w.chunk_off[c] || l.label < 0 || l.label > 3 || rt.label < 0 || rt.label > 3 || l.label == rt.label) continue;
        job[i] = (int) jobs.n();
        jobs.add(std::max<int64_t>(l.a, w.chunk_off[c]), std::min<int64_t>(rt.b, w.chunk_off[c + 1]), 1u << l.label);
        vm.push_back((uint8_t) (1u << rt.label));
    }
    const std::vector<int64_t>&first = jobs.first, &last = jobs.last;
    const int64_t n = jobs.n();
    const double probs[3] = {0.025, 0.5, 0.975};
    std::vector<double> lpe((size_t) n), modeP((size_t) n), pCalled((size_t) n, 0.0), prof;
    std::vector<int64_t> quant((size_t) n * 3), mode((size_t) n);
    int rc = hf_get_breakpoints(r.ctx, n, first.data(), last.data(), jobs.mask.data(), vm.data(), 3, probs, lpe.data(), quant.data(), mode.data(), modeP.data());
    if (rc != HF_OK) return rc;
    for (size_t i = 1; i < runs.size(); i++) {      // p_called: one profile per boundary
        if (job[i] < 0) continue;
        const size_t k = (size_t) job[i];
        double lp = 0.0;
        prof.resize((size_t) (last[k] - first[k]));
        if ((rc = hf_get_breakpoint_profile(r.ctx, first[k], last[k], jobs.mask[k], vm[k], prof.data(), &lp)) != HF_OK) return rc;
        pCalled[k] = prof[(size_t) (runs[i].a - first[k] - 1)];
    }
    TableFile f;
    if ((rc = f.open(r.dir + "/final_label_run_boundaries.tsv")) != HF_OK) return rc;
    fprintf(f, "#ctg\tpos\tleft\tright\tp_event\tp_called\tlo\tmedian\thi\tmode\tmode_p\n");
    for (size_t i = 1; i < runs.size(); i++) {
        const LRun &l = runs[i - 1], &rt = runs[i];
        if (strcmp(l.ctg, rt.ctg) != 0) continue;      // (the first run of a contig has no boundary on its left)
        const int c = chunk[i];
        fprintf(f, "%s\t%ld\t%s\t%s\t", rt.ctg, (long) rt.s, run_label_name(l.label), run_label_name(rt.label));
        const int k = job[i];
        if (k < 0 || mode[(size_t) k] < 0 || !(lpe[(size_t) k] > -INFINITY)) { fprintf(f, "NA\tNA\tNA\tNA\tNA\tNA\tNA\n"); continue; }
        fprintf(f, "%.6g\t%.6g\t%ld\t%ld\t%ld\t%ld\t%.6g\n", std::exp(lpe[(size_t) k]), pCalled[(size_t) k], base_of(c, quant[(size_t) k * 3]),
                base_of(c, quant[(size_t) k * 3 + 1]), base_of(c, quant[(size_t) k * 3 + 2]), base_of(c, mode[(size_t) k]), modeP[(size_t) k]);
    }
    return f.close();
}

// --numBlocks: exact posterior mean and standard deviation of the block counts (hf_get_run_moments) under the model of the last full pass.
//   label_blocks_exact.tsv   one row per scope and label set.  Scopes: those of hf_cli_scopes.h (a contig's mean and variance are the
//                            sums over its runs of chunks).  No annotation-region scope: a block does not belong to one region.  Label
//                            sets: Err, Dup, Hap, Col, Err+Dup+Col.  Columns: blocks_final_labels (the runs of the set in the final
//                            labels), blocks_expected, blocks_sd.  A run continues from chunk c-1 into chunk c where the two are joined
//                            (hf_cli_scopes.h): the rule hfio_write_final_bed merges by, so that for a single label and the default
//                            --minimumLengths blocks_final_labels of "all" is the number of the label's rows in the final BED.
static int write_exact_blocks(Report& r) {
    const hf_windows& w = r.w;
    const Jobs jobs = r.run_jobs();
    std::vector<double> mean((size_t) jobs.n()), var((size_t) jobs.n());
    int rc = hf_get_run_moments(r.ctx, jobs.n(), jobs.first.data(), jobs.last.data(), jobs.mask.data(), r.joined.data(), mean.data(), var.data());
    if (rc != HF_OK) return rc;
    TableFile f;
    if ((rc = f.open(r.dir + "/label_blocks_exact.tsv")) != HF_OK) return rc;
    fprintf(f, "#scope\tlabel_set\tblocks_final_labels\tblocks_expected\tblocks_sd\n");
    size_t j = 0;
    for (const Scope& sc : r.sc.scopes) {
        int64_t finalBlocks[5] = {0, 0, 0, 0, 0};
        double m[5] = {0, 0, 0, 0, 0}, v[5] = {0, 0, 0, 0, 0};       // sums over the runs, list order
        for (const auto& rg : sc.runs) {
            if (r.list.no_windows(rg.first, rg.second)) continue;
            bool in[5] = {false, false, false, false, false};        // the window before lies in the set and continues into this one
            for (int c = rg.first; c < rg.second; c++) {
                if (c == rg.first || !r.joined[(size_t) c]) for (int k = 0; k < 5; k++) in[k] = false;
                for (int64_t t = w.chunk_off[c]; t < w.chunk_off[c + 1]; t++) {
                    const int l = r.labels[t];
                    for (int k = 0; k < 5; k++) {
                        const bool now = l >= 0 && l <= 3 && ((kLabelSets[k] >> l) & 1);
                        if (now && !in[k]) finalBlocks[k]++;
                        in[k] = now;
                    }
                }
            }
            for (int k = 0; k < 5; k++, j++) { m[k] += mean[j]; v[k] += var[j]; }
        }
        for (int k = 0; k < 5; k++)
            fprintf(f, "%s\t%s\t%ld\t%.10g\t%.10g\n", sc.name.c_str(), kLabelSetNames[k], (long) finalBlocks[k], m[k], std::sqrt(v[k]));
    }
    return f.close();
}

// --runLengths L: the exact block-length spectrum (hf_get_run_lengths) under the model of the last full pass.
//   label_block_lengths_exact.tsv   per scope (those of hf_cli_scopes.h: the sums over its runs of chunks) and label set (Err, Dup, Hap,
//                                   Col, Err+Dup+Col) one row per length 1..L and a row ">L": blocks_final_labels (the runs of that
//                                   length of the set in the final labels) and blocks_expected.  Runs go on across chunks by the rule of
//                                   --numBlocks.
//   label_blocks_kept_exact.tsv     with --minimumLengths (minLenWindows not null): per scope and label its minimum in windows, the
//                                   expected blocks, the expected blocks at or above the minimum (bin ">L" included) and the expected
//                                   windows in the shorter ones, sum_{l < min} l N_l.
static int write_block_lengths(Report& r, int L, const int32_t* minLenWindows) {
    const hf_windows& w = r.w;
    const size_t B = (size_t) L + 1;
    const Jobs jobs = r.run_jobs();
    std::vector<double> spec((size_t) jobs.n() * B);
    int rc = hf_get_run_lengths(r.ctx, jobs.n(), jobs.first.data(), jobs.last.data(), jobs.mask.data(), L, r.joined.data(), spec.data());
    if (rc != HF_OK) return rc;
    TableFile f, g;
    if ((rc = f.open(r.dir + "/label_block_lengths_exact.tsv")) != HF_OK) return rc;
    if (minLenWindows && (rc = g.open(r.dir + "/label_blocks_kept_exact.tsv")) != HF_OK) return rc;
    fprintf(f, "#scope\tlabel_set\tlength\tblocks_final_labels\tblocks_expected\n");
    if (g) fprintf(g, "#scope\tlabel\tmin_len_windows\tblocks_expected\tblocks_expected_kept\twindows_expected_dropped\n");
    size_t j = 0;
    std::vector<int64_t> finalBlocks(5 * B);
    std::vector<double> m(5 * B);
    for (const Scope& sc : r.sc.scopes) {
        std::fill(finalBlocks.begin(), finalBlocks.end(), 0);
        std::fill(m.begin(), m.end(), 0.0);                               // sums over the runs, list order
        for (const auto& rg : sc.runs) {
            if (r.list.no_windows(rg.first, rg.second)) continue;
            int64_t run[5] = {0, 0, 0, 0, 0};                             // the windows of the set's current run
            auto close = [&](int k) { if (run[k] > 0) finalBlocks[(size_t) k * B + (size_t) std::min<int64_t>(run[k], L + 1) - 1]++; run[k] = 0; };
            for (int c = rg.first; c < rg.second; c++) {
                if (c > rg.first && !r.joined[(size_t) c]) for (int k = 0; k < 5; k++) close(k);
                for (int64_t t = w.chunk_off[c]; t < w.chunk_off[c + 1]; t++) {
                    const int l = r.labels[t];
                    for (int k = 0; k < 5; k++) {
                        if (l >= 0 && l <= 3 && ((kLabelSets[k] >> l) & 1)) run[k]++;
                        else close(k);
                    }
                }
            }
            for (int k = 0; k < 5; k++) close(k);
            for (int k = 0; k < 5; k++, j++)
                for (size_t b = 0; b < B; b++) m[(size_t) k * B + b] += spec[j * B + b];
        }
        for (int k = 0; k < 5; k++)
            for (size_t b = 0; b < B; b++) {
                if (b < (size_t) L) fprintf(f, "%s\t%s\t%zu\t%ld\t%.10g\n", sc.name.c_str(), kLabelSetNames[k], b + 1, (long) finalBlocks[(size_t) k * B + b], m[(size_t) k * B + b]);
                else fprintf(f, "%s\t%s\t>%d\t%ld\t%.10g\n", sc.name.c_str(), kLabelSetNames[k], L, (long) finalBlocks[(size_t) k * B + b], m[(size_t) k * B + b]);
            }
        for (int k = 0; g && k < 4; k++) {
            double all = 0.0, kept = 0.0, dropped = 0.0;                  // in bin order
            for (size_t b = 0; b < B; b++) {
                const double x = m[(size_t) k * B + b];
                all += x;
                if ((int64_t) b + 1 >= minLenWindows[k]) kept += x; else dropped += (double) (b + 1) * x;
            }
            fprintf(g, "%s\t%s\t%d\t%.10g\t%.10g\t%.10g\n", sc.name.c_str(), kLabelSetNames[k], (int) minLenWindows[k], all, kept, dropped);
        }
    }
    return (rc = f.close()) != HF_OK ? rc : g.close();
}

// --totalsDistribution K: the exact distribution of a region's label totals (hf_get_count_distribution) under the model of the last full
// pass.
//   region_label_totals_exact.tsv   per region (file order) and label set (Err, Dup, Hap, Col, Err+Dup+Col) one row: the leading columns
//                                   of region_label_probabilities.tsv (ctg start end name n_windows: the windows whose bases meet
//                                   [start, end)), label_set, mean = sum k p_k in increasing k (NA where p_gtK > 0), q025 q50 q975 (the
//                                   smallest k whose cumulative sum in increasing k reaches the level; >K when bin K does not reach it),
//                                   then p_0 .. p_K p_gtK.  A region without windows: NA in every column behind label_set.
// A region's windows are a union of index ranges that lie in different chunks (region_windows), so its distribution is the convolution
// of its ranges' in range order: the getter's own stitch (hf_countdist_stitch.h).
static int write_region_totals(Report& r, int K) {
    const size_t B = cd_part_len(K);
    const RegionWindows& rw = r.regionWindows();
    Jobs jobs;
    for (const auto& ranges : rw.ranges)
        for (const auto& rg : ranges)
            for (int k = 0; k < 5; k++) jobs.add(rg.first, rg.second, kLabelSets[k]);
    std::vector<double> dist((size_t) jobs.n() * B);
    int rc = hf_get_count_distribution(r.ctx, jobs.n(), jobs.first.data(), jobs.last.data(), jobs.mask.data(), K, dist.data());
    if (rc != HF_OK) return rc;
    TableFile f;
    if ((rc = f.open(r.dir + "/region_label_totals_exact.tsv")) != HF_OK) return rc;
    fprintf(f, "#ctg\tstart\tend\tname\tn_windows\tlabel_set\tmean\tq025\tq50\tq975");
    for (int k = 0; k <= K; k++) fprintf(f, "\tp_%d", k);
    fprintf(f, "\tp_gtK\n");
    size_t j = 0;                                                  // the region's first job
    CdStitch stitch(K);
    std::vector<double> p(B);
    for (size_t i = 0; i < r.regions->size(); i++) {
        const Region& g = (*r.regions)[i];
        for (int k = 0; k < 5; k++) {
            fprintf(f, "%s\t%ld\t%ld\t%s\t%zu\t%s", g.ctg.c_str(), (long) g.start, (long) g.end, g.name.c_str(), rw.wins[i].size(), kLabelSetNames[k]);
            if (rw.wins[i].empty()) {
                for (size_t b = 0; b < B + 4; b++) fprintf(f, "\tNA");
                fprintf(f, "\n");
                continue;
            }
            stitch.begin();
            for (size_t q = 0; q < rw.ranges[i].size(); q++) stitch.part(&dist[(j + q * 5 + (size_t) k) * B]);
            stitch.end(p.data());
            double mean = 0.0, cum = 0.0;
            int q[3] = {-1, -1, -1};                               // (-1: beyond bin K)
            static const double kLevels[3] = {0.025, 0.5, 0.975};
            for (int b = 0; b <= K; b++) {
                mean += (double) b * p[(size_t) b];
                cum += p[(size_t) b];
                for (int l = 0; l < 3; l++) if (q[l] < 0 && cum >= kLevels[l]) q[l] = b;
            }
            if (p[B - 1] > 0.0) fprintf(f, "\tNA"); else fprintf(f, "\t%.6f", mean);
            for (int l = 0; l < 3; l++) { if (q[l] < 0) fprintf(f, "\t>%d", K); else fprintf(f, "\t%d", q[l]); }
            for (size_t b = 0; b < B; b++) fprintf(f, "\t%.6g", p[b]);
            fprintf(f, "\n");
        }
        j += rw.ranges[i].size() * 5;
    }
    return f.close();
}

// --keptBlocks: the exact probability that a scope holds a block of a label that --minimumLengths would keep (hf_get_long_run_log_probs)
// under the model of the last full pass.
//   kept_block_probabilities.tsv   one row per scope of hf_cli_scopes.h ("all", then "contig" rows) and, with --regionProbs FILE, one per
//                                  region in file order (a region without windows: NA).  Per label L: min_windows_L (the length in
//                                  windows), p_block_L = P(some run of at least that many consecutive windows of L), p_none_L = 1 -
//                                  p_block_L.  A run goes on from chunk c-1 into chunk c where the two are joined (the rule of
//                                  --numBlocks); the pieces of a scope that no such join connects are independent, and their
//                                  log_p_none add.
static int write_kept_blocks(Report& r) {
    // a row: scope, name, its windows and its window ranges
    struct Row { const char* scope; const std::string& name; int64_t n; const std::vector<std::pair<int64_t, int64_t>>& ranges; };
    std::vector<Row> rows;
    for (const Scope& sc : r.sc.scopes) {
        int64_t n = 0;
        for (const auto& rg : sc.ranges) n += rg.second - rg.first;
        rows.push_back(Row{rows.empty() ? "all" : "contig", sc.name, n, sc.ranges});
    }
    if (r.regions) {
        const RegionWindows& rw = r.regionWindows();
        for (size_t i = 0; i < r.regions->size(); i++) rows.push_back(Row{"region", (*r.regions)[i].name, (int64_t) rw.wins[i].size(), rw.ranges[i]});
    }
    Jobs jobs;
    std::vector<int32_t> len;
    for (const Row& row : rows)
        for (const auto& rg : row.ranges)
            for (int l = 0; l < 4; l++) { jobs.add(rg.first, rg.second, 1u << l); len.push_back(r.minLen[l]); }
    std::vector<double> none((size_t) jobs.n());
    int rc = hf_get_long_run_log_probs(r.ctx, jobs.n(), jobs.first.data(), jobs.last.data(), jobs.mask.data(), len.data(), r.joined.data(),
                                       none.data(), nullptr);
    if (rc != HF_OK) return rc;
    TableFile f;
    if ((rc = f.open(r.dir + "/kept_block_probabilities.tsv")) != HF_OK) return rc;
    fprintf(f, "#scope\tname\tn_windows");
    for (int l = 0; l < 4; l++) fprintf(f, "\tmin_windows_%s\tp_block_%s\tp_none_%s", r.state_name(l), r.state_name(l), r.state_name(l));
    fprintf(f, "\n");
    size_t j = 0;
    for (const Row& row : rows) {
        fprintf(f, "%s\t%s\t%ld", row.scope, row.name.c_str(), (long) row.n);
        double s[4] = {0, 0, 0, 0};                                   // sums over the ranges, in order
        for (size_t k = 0; k < row.ranges.size(); k++)
            for (int l = 0; l < 4; l++) s[l] += none[j++];
        for (int l = 0; l < 4; l++) {
            if (row.n == 0) fprintf(f, "\tNA\tNA\tNA");
            else fprintf(f, "\t%d\t%.6g\t%.6g", (int) r.minLen[l], -std::expm1(s[l]) + 0.0, std::exp(s[l]));
        }
        fprintf(f, "\n");
    }
    return f.close();
}

// --constrainedPosterior: the posterior under --minimumLengths (hf_minlen_posterior, run by the caller) and the mass the rule keeps.
//   admissible_mass.tsv                      a header line and a line with the four lengths in windows; then a header line and one row per
//                                            scope of hf_cli_scopes.h: chunks, windows, log_mass = the chunks' log P(path admissible |
//                                            data) summed in list order.
//                                            perChunkRule (--mergedChunks: the chunks' masses of a run under the per-chunk rule, while the
//                                            context holds the run over the joined chunks) adds the column log_mass_per_chunk_rule.
//   posterior_prediction_min_lengths.bed     hfio_write_posterior_bed with the constrained posterior and its argmax labels
static int write_constrained_posterior(Report& r, const std::vector<double>* perChunkRule = nullptr) {
    const int64_t N = r.N;
    const int32_t* const minLenWindows = r.minLen;
    std::vector<double> mass((size_t) std::max(r.C, 1));
    int rc = hf_get_minlen_chunk_log_mass(r.ctx, mass.data(), nullptr);
    if (rc != HF_OK) return rc;
    struct Row { int chunks; int64_t n; double log_mass, per_chunk; };
    std::vector<Row> rows(r.sc.scopes.size(), Row{0, 0, 0.0, 0.0});
    for (int c = 0; c < r.C; c++)
        for (size_t ri : {(size_t) 0, r.sc.scope_of_chunk[(size_t) c]}) {
            Row& row = rows[ri];
            row.chunks++;
            row.n += r.w.chunk_off[c + 1] - r.w.chunk_off[c];
            row.log_mass += mass[(size_t) c];
            if (perChunkRule) row.per_chunk += (*perChunkRule)[(size_t) c];
        }
    TableFile f;
    if ((rc = f.open(r.dir + "/admissible_mass.tsv")) != HF_OK) return rc;
    fprintf(f, "#min_windows_Err\tmin_windows_Dup\tmin_windows_Hap\tmin_windows_Col\n%d\t%d\t%d\t%d\n", minLenWindows[0], minLenWindows[1],
            minLenWindows[2], minLenWindows[3]);
    fprintf(f, "#scope\tchunks\twindows\tlog_mass%s\n", perChunkRule ? "\tlog_mass_per_chunk_rule" : "");
    for (size_t i = 0; i < rows.size(); i++) {
        fprintf(f, "%s\t%d\t%ld\t%.17g", r.sc.scopes[i].name.c_str(), rows[i].chunks, (long) rows[i].n, rows[i].log_mass + 0.0);
        if (perChunkRule) fprintf(f, "\t%.17g", rows[i].per_chunk + 0.0);
        fprintf(f, "\n");
    }
    if ((rc = f.close()) != HF_OK) return rc;
    std::vector<double> post((size_t) N * 4);
    std::vector<int8_t> lab((size_t) N);
    if ((rc = hf_get_minlen_posterior(r.ctx, 0, N, post.data())) != HF_OK) return rc;
    if ((rc = hf_get_minlen_posterior_labels(r.ctx, lab.data())) != HF_OK) return rc;
    const std::string pp = r.dir + "/posterior_prediction_min_lengths.bed";
    if (hfio_write_posterior_bed(r.tab, post.data(), lab.data(), pp.c_str()) != 0) { hf_cli_set_error(pp + " cannot be written"); return HF_E_ARG; }
    return HF_OK;
}

// --jointEntropy: exact path entropy and log-probability of the final labels (hf_get_path_entropy, hf_get_path_log_probs,
// hf_get_entropy_profile) under the model of the last full pass.
//   path_uncertainty.tsv   one row per scope of hf_cli_scopes.h (chunks are independent chains, so a contig's values are the sums over its
//                          ranges).  Columns: windows, path_entropy_nats, entropy_nats_per_window, window_entropy_sum_nats (the sum of
//                          the per-window posterior entropies in window order: what the posterior alone gives), final_labels_log_prob
//                          (-inf where the labels are impossible, NA where a label of the scope is outside 0..3).
static int write_path_uncertainty(Report& r) {
    const int64_t N = r.N;
    const int8_t* const finalLabels = r.labels;
    // the jobs: every range of every scope; the labelled ones only where every label of the range is a state
    Jobs jobs, ljobs;
    std::vector<char> labelled;
    for (const Scope& sc : r.sc.scopes)
        for (const auto& rg : sc.ranges) {
            jobs.add(rg.first, rg.second);
            bool ok = true;
            for (int64_t t = rg.first; t < rg.second && ok; t++) ok = finalLabels[t] >= 0 && finalLabels[t] <= 3;
            labelled.push_back(ok);
            if (ok) ljobs.add(rg.first, rg.second);
        }
    std::vector<double> ent((size_t) jobs.n()), lp((size_t) ljobs.n()), marg((size_t) N);
    int rc = hf_get_path_entropy(r.ctx, jobs.n(), jobs.first.data(), jobs.last.data(), ent.data());
    if (rc != HF_OK) return rc;
    if ((rc = hf_get_path_log_probs(r.ctx, ljobs.n(), ljobs.first.data(), ljobs.last.data(), finalLabels, lp.data())) != HF_OK) return rc;
    if (N > 0 && (rc = hf_get_entropy_profile(r.ctx, 0, N, marg.data(), nullptr)) != HF_OK) return rc;
    TableFile f;
    if ((rc = f.open(r.dir + "/path_uncertainty.tsv")) != HF_OK) return rc;
    fprintf(f, "#scope\twindows\tpath_entropy_nats\tentropy_nats_per_window\twindow_entropy_sum_nats\tfinal_labels_log_prob\n");
    size_t j = 0, jl = 0;
    for (const Scope& sc : r.sc.scopes) {
        int64_t windows = 0;
        double h = 0.0, hw = 0.0, l = 0.0;       // sums over the ranges, list order
        bool known = true;
        for (const auto& rg : sc.ranges) {
            windows += rg.second - rg.first;
            h += ent[j];
            for (int64_t t = rg.first; t < rg.second; t++) hw += marg[(size_t) t];
            if (labelled[j]) l += lp[jl++];
            else known = false;
            j++;
        }
        fprintf(f, "%s\t%ld\t%.9g\t%.9g\t%.9g\t", sc.name.c_str(), (long) windows, h, windows > 0 ? h / (double) windows : 0.0, hw);
        if (!known) fprintf(f, "NA\n");
        else if (std::isinf(l)) fprintf(f, "-inf\n");
        else fprintf(f, "%.9g\n", l);
    }
    return f.close();
}
