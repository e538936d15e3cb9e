// hf_cli.cpp — `hmm_flagger` command line of the MI355X build: same options, inputs and output files as
// mobinasri/flagger programs/src/hmm_flagger.c (main :611-1077, runHMMFlagger :285-488), with every E-step
// delegated to the HIP kernels through the C ABI (include/hmm_flagger_hip.h).  No CPU E-step exists here.
//
// The stages, in the order main() calls them; all but the first take the session (struct Run: options, table, context):
//   parse_options, read_environment   argv and the three HF_* variables -> Options
//   check_options      every refusal before the input is read; the preset, the --sweepAlpha list, the alpha TSV, the region file, the lengths
//                      in windows (min_len_windows, called again once a .bin input has shown its window length)
//   load_input, make_model, create_context   the table and the collapsed components; createModel; one hf_ctx or the sharded GPU list
//   run_em             one whole run into a directory: em_loop, final_inference, final_outputs, late_outputs
//                      late_outputs builds one Report from the session and hands it to the writers of hf_cli_reports.h, one per report file;
//                      which chunks are joined, what a group is and the scopes "all" + every contig are defined once, in hf_cli_scopes.h
//                      (final_inference's --wholeContigs and --expectedAccuracy read them there too)
//   sweep_batched | sweep_sequential, write_sweep_table   --sweepAlpha: every candidate through hf_batch, or through run_em
#include "../../include/hmm_flagger_hip.h"
#include "../../include/hmm_flagger_io.h"
#include "../../include/hmm_flagger_model.h"
#include "../../include/hmm_flagger_multi.h"
#include "hf_cli_scopes.h"
#include "hf_countdist_stitch.h"
#include "hf_squarem.h"
#include <getopt.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <unistd.h>
#include <algorithm>
#include <array>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <vector>

static const char* ts() {                                   // common.c:116 get_timestamp
    static thread_local char buf[64];
    time_t t = time(nullptr);
    struct tm tmv;
    localtime_r(&t, &tmv);
    strftime(buf, sizeof buf, "%Y-%m-%d %H:%M:%S", &tmv);
    return buf;
}
static double real_time() { struct timeval tp; gettimeofday(&tp, nullptr); return tp.tv_sec + tp.tv_usec * 1e-6; }
static double cpu_time() {
    struct rusage r; getrusage(RUSAGE_SELF, &r);
    return r.ru_utime.tv_sec + r.ru_stime.tv_sec + 1e-6 * (r.ru_utime.tv_usec + r.ru_stime.tv_usec);
}
static double peak_rss_gb() { struct rusage r; getrusage(RUSAGE_SELF, &r); return r.ru_maxrss * 1024.0 / 1073741824.0; }

// the options without a letter: their codes in long_options and in parse_options' switch
enum LongOnly {
    kOptDevice = 1001, kOptHipAlgo, kOptGpus, kOptExchange, kOptViterbi, kOptSweepAlpha, kOptUncertaintySamples, kOptUncertaintySeed,
    kOptRunConfidence, kOptRegionProbs, kOptFitAlpha, kOptFitAlphaEntries, kOptFitAlphaMax, kOptFitAlphaEvery, kOptExactTotals,
    kOptNumBlocks, kOptJointEntropy, kOptRunBoundaries, kOptEnforceMinLen, kOptKeptBlocks, kOptConstrainedPosterior, kOptAdmissibleSamples, kOptWholeContigs, kOptMergedChunks,
    kOptExpectedAccuracy, kOptExpectedGains, kOptLengthConstrainedEM, kOptCrossChunkEM, kOptRunLengths, kOptTotalsDistribution
};
static struct option long_options[] = {                   // hmm_flagger.c:578-608
    {"input", required_argument, nullptr, 'i'}, {"preset", required_argument, nullptr, 'x'},
    {"iterations", required_argument, nullptr, 'n'}, {"convergenceTol", required_argument, nullptr, 't'},
    {"disableAdjustContigEnds", no_argument, nullptr, 'e'}, {"minReadFractionAtEnds", required_argument, nullptr, 'f'},
    {"modelType", required_argument, nullptr, 'm'}, {"maxHighMapqRatio", required_argument, nullptr, 'q'},
    {"minHighMapqRatio", required_argument, nullptr, 'Q'}, {"chunkLen", required_argument, nullptr, 'C'},
    {"windowLen", required_argument, nullptr, 'W'}, {"contigsList", required_argument, nullptr, 'c'},
    {"threads", required_argument, nullptr, '@'}, {"collapsedComps", required_argument, nullptr, 'p'},
    {"alphaTsv", required_argument, nullptr, 'A'}, {"binArrayFile", required_argument, nullptr, 'a'},
    {"writeParameterStatsPerIteration", no_argument, nullptr, 'w'},
    {"writeBenchmarkingStatsPerIteration", no_argument, nullptr, 'k'},
    {"writePosteriorProbs", no_argument, nullptr, 'P'}, {"outputDir", required_argument, nullptr, 'o'},
    {"overlapRatioThreshold", required_argument, nullptr, 'v'}, {"labelNames", required_argument, nullptr, 'l'},
    {"initialRandomDev", required_argument, nullptr, 'D'}, {"trackName", required_argument, nullptr, 'N'},
    {"dumpBin", no_argument, nullptr, 'B'}, {"accelerate", no_argument, nullptr, 's'},
    {"minimumLengths", required_argument, nullptr, 'M'},
    // additions of this build (not in the reference), named so that every unique prefix the reference's getopt_long accepted
    // still resolves to the same option (tests/test_cli_prefix_cpu.py): nothing new starts like an existing name's prefix
    {"device", required_argument, nullptr, kOptDevice},
    {"hipAlgo", required_argument, nullptr, kOptHipAlgo},         // scan (default) | seq (the on-device sequential cross-check)
    {"gpus", required_argument, nullptr, kOptGpus},            // chunks sharded over GPUs device..device+N-1, one RCCL all-gather per pass
    {"exchange", required_argument, nullptr, kOptExchange},        // chunks (default: bit-identical for every N) | ranks (one vector per GPU: faster)
    {"viterbi", no_argument, nullptr, kOptViterbi},               // final labels by most-probable path (hf_viterbi) instead of posterior argmax
    {"sweepAlpha", required_argument, nullptr, kOptSweepAlpha},      // one run per alpha TSV of a list, one load (not `alpha...`: --alpha stays unique)
    {"uncertaintySamples", required_argument, nullptr, kOptUncertaintySamples},   // N posterior path samples after the final inference (hf_sample_paths)
    {"uncertaintySeed", required_argument, nullptr, kOptUncertaintySeed},      // their seed [0]
    {"runConfidence", no_argument, nullptr, kOptRunConfidence},              // exact per-run label probabilities (hf_get_interval_log_probs)
    {"regionProbs", required_argument, nullptr, kOptRegionProbs},          // exact per-region label probabilities for the regions of a BED file
    {"fitAlpha", no_argument, nullptr, kOptFitAlpha},                   // fit the alpha matrix inside the EM (hf_get_alpha_stats, hfm_estimate_alpha)
    {"fitAlphaEntries", required_argument, nullptr, kOptFitAlphaEntries},      // the free entries, pre,state pairs separated by ':'
    {"fitAlphaMax", required_argument, nullptr, kOptFitAlphaMax},          // their upper bound [0.8]
    {"fitAlphaEvery", required_argument, nullptr, kOptFitAlphaEvery},        // every P-th iteration is an alpha-iteration [2]
    {"exactTotals", no_argument, nullptr, kOptExactTotals},                // exact mean and SD of the label totals (hf_get_count_moments)
    {"numBlocks", no_argument, nullptr, kOptNumBlocks},                  // exact mean and SD of the block counts (hf_get_run_moments)
    {"jointEntropy", no_argument, nullptr, kOptJointEntropy},               // exact path entropy and log-probability of the final labels (hf_get_path_entropy)
    {"runBoundaries", no_argument, nullptr, kOptRunBoundaries},              // exact posterior of every block boundary (hf_get_breakpoints; not `b...`: --b stays --binArrayFile)
    {"keptBlocks", no_argument, nullptr, kOptKeptBlocks},                 // exact probability of a block --minimumLengths would keep (hf_get_long_run_log_probs)
    {"enforceMinimumLengths", no_argument, nullptr, kOptEnforceMinLen},      // --viterbi decodes UNDER --minimumLengths (hf_viterbi_minlen; not `min...`: --mini stays --minimumLengths)
    {"constrainedPosterior", no_argument, nullptr, kOptConstrainedPosterior},       // the posterior UNDER --minimumLengths (hf_minlen_posterior; --cons is its shortest prefix: --c, --co, --con were ambiguous in the reference)
    {"admissibleSamples", required_argument, nullptr, kOptAdmissibleSamples},    // N paths drawn from the posterior UNDER --minimumLengths (hf_sample_paths_minlen; nothing else starts with --ad)
    {"wholeContigs", no_argument, nullptr, kOptWholeContigs},             // --enforceMinimumLengths over the joined chunks of a contig (hf_viterbi_minlen_joined; nothing else starts with --wh, --w was ambiguous already; not `j...`: --j stays --jointEntropy)
    {"mergedChunks", no_argument, nullptr, kOptMergedChunks},             // --constrainedPosterior and --admissibleSamples over the joined chunks of a contig (hf_minlen_posterior_joined, hf_sample_paths_minlen_joined; nothing else starts with --me, --m was ambiguous already)
    {"expectedAccuracy", required_argument, nullptr, kOptExpectedAccuracy},   // final labels by maximum expected accuracy UNDER --minimumLengths, chunks | contigs (hf_get_mea_labels; both new names start with --exp: --ex was ambiguous already, --e and --ex stay --exchange)
    {"expectedGains", required_argument, nullptr, kOptExpectedGains},         // its 4x4 gain matrix [identity]
    {"lengthConstrainedEM", no_argument, nullptr, kOptLengthConstrainedEM},     // the EM iterations fit UNDER --minimumLengths (hf_estep_minlen; --l stays --labelNames: parse_options' kept[])
    {"crossChunkEM", no_argument, nullptr, kOptCrossChunkEM},             // --lengthConstrainedEM over the joined chunks of a contig (hf_estep_minlen_joined; nothing else starts with --cr, --c was ambiguous already, --le stays --lengthConstrainedEM, --l --labelNames)
    {"runLengths", required_argument, nullptr, kOptRunLengths},          // the exact block-length spectrum up to L windows (hf_get_run_lengths; no reference option starts with r, --ru and --run stay --runConfidence: parse_options' kept[]; --runL is its shortest prefix)
    {"totalsDistribution", required_argument, nullptr, kOptTotalsDistribution},   // the exact distribution of a region's label totals up to K windows (hf_get_count_distribution; no option starts with --to: it is its shortest prefix, --t was ambiguous already, --th stays --threads and --tr --trackName)
    {nullptr, 0, nullptr, 0}};

static void usage(const char* program) {
    fprintf(stderr, "\nUsage: %s  -i <INPUT_FILE> -o <OUTPUT_DIR> \n", program);
    fprintf(stderr,
            "Options (as mobinasri/flagger hmm_flagger v1.2.0):\n"
            "         --input, -i                  cov / cov.gz / bin input\n"
            "         --preset, -x                 hifi | ont-r9 | ont-r10 [hifi]\n"
            "         --outputDir, -o              existing directory for the output files\n"
            "         --modelType, -m              gaussian | trunc_exp_gaussian | negative_binomial [trunc_exp_gaussian]\n"
            "         --trackName, -N              track name of the final BED [final_hmm_flagger]\n"
            "         --chunkLen, -C               chunk length in bases [20000000]\n"
            "         --windowLen, -W              window length in bases [preset]\n"
            "         --iterations, -n             maximum EM iterations [100]\n"
            "         --convergenceTol, -t         [0.001]\n"
            "         --contigsList, -c            file with contig names to keep (first token of every line)\n"
            "         --disableAdjustContigEnds, -e\n"
            "         --minReadFractionAtEnds, -f  [preset]\n"
            "         --maxHighMapqRatio, -q       [0.25]     --minHighMapqRatio   [0.75]\n"
            "         --alphaTsv, -A               4x4 tab-separated alpha matrix [all zero]\n"
            "         --collapsedComps, -p         components of the collapsed state [auto 2..10]\n"
            "         --writeParameterStatsPerIteration, -w     --writePosteriorProbs, -P\n"
            "         --dumpBin, -B                --accelerate, -s (SQUAREM)\n"
            "         --minimumLengths, -M         Err,Dup,Col minimum lengths [0,0,0]\n"
            "         --threads, -@                accepted for compatibility (the E-step runs on the GPU)\n"
            "         --labelNames -l, --binArrayFile -a, --overlapRatioThreshold -v, -k: summary tables (prediction_summary_*.tsv)\n"
            "         --device                     (first) GPU index [0]        --hipAlgo scan|seq [scan]\n"
            "         --gpus N                     shard the chunks over GPUs device..device+N-1 (one process, one thread + one RCCL\n"
            "                                      rank per GPU, one all-gather of statistics per EM pass)\n"
            "         --exchange chunks|ranks      what the GPUs exchange: per-chunk vectors summed in chunk-list order (default: results are\n"
            "                                      bit-identical for every N) | one statistics vector per GPU summed in rank order (faster per\n"
            "                                      pass; equal across N only up to the rounding of the order of additions, which --accelerate\n"
            "                                      can carry into the last printed digits)\n"
            "         --viterbi                    final labels (final BED, final summary tables) by the most probable state path with\n"
            "                                      the final parameters instead of the posterior argmax; its log-probability goes to\n"
            "                                      viterbi_log_probability.tsv (-P still writes the posterior BED)\n"
            "         --sweepAlpha LIST            one EM run per alpha TSV listed in LIST (one path per line; blank lines and lines starting\n"
            "                                      with # are skipped), the input loaded once: line i writes every output file of an\n"
            "                                      --alphaTsv run into <outputDir>/alpha_<i>/, and <outputDir>/alpha_sweep.tsv sums them up\n"
            "         --uncertaintySamples N       after the final inference, draw N state paths from the posterior with the final parameters\n"
            "                                      and write posterior_samples_summary.tsv (bases per region and label: final labels, mean,\n"
            "                                      SD, 2.5/50/97.5 %% quantiles over the samples) and final_label_runs_support.bed (every run of\n"
            "                                      equal final label: fraction of samples that give the whole run its label, mean fraction of\n"
            "                                      its windows); one GPU, not with --gpus N>1 or --sweepAlpha\n"
            "         --uncertaintySeed S          seed of those samples (a sample depends on the seed and its index only) [0]\n"
            "         --runConfidence              write final_label_runs_confidence.bed: for every run of equal final label (the runs of\n"
            "                                      final_label_runs_support.bed) the exact probability that all its windows have that label,\n"
            "                                      as a Phred quality, and the mean posterior; one GPU, not with --gpus N>1 or --sweepAlpha\n"
            "         --regionProbs FILE           for every region of a BED file (ctg start end [name]) write the exact probabilities that\n"
            "                                      any / every window it meets has each label, and the mean posterior, to\n"
            "                                      region_label_probabilities.tsv; one GPU, not with --gpus N>1 or --sweepAlpha\n"
            "         --fitAlpha                   fit the alpha matrix inside the EM, starting from --alphaTsv (or 0): every P-th iteration\n"
            "                                      updates the free alpha entries (each to the maximiser of the expected log-likelihood, from the\n"
            "                                      exact gradient and curvature of its pass) instead of the other parameters; writes\n"
            "                                      alpha_fitted.tsv (readable by --alphaTsv) and alpha_trace.tsv (per alpha-iteration: iteration,\n"
            "                                      log-likelihood, 16 alpha before, 16 gradients, 16 curvatures); gaussian and trunc_exp_gaussian,\n"
            "                                      one GPU, not with --accelerate, --gpus N>1 or --sweepAlpha\n"
            "         --fitAlphaEntries LIST       the free entries as pre,state pairs separated by ':' (states 0 Err, 1 Dup, 2 Hap, 3 Col)\n"
            "                                      [0,0:0,2:1,1:1,2:2,0:2,1:2,2:2,3:3,2:3,3]\n"
            "         --fitAlphaMax X              upper bound of a fitted entry, 0 <= X < 1 (the lower bound is 0) [0.8]\n"
            "         --fitAlphaEvery P            iterations P, 2P, ... are alpha-iterations [2]\n"
            "         --exactTotals                after the final inference, write label_totals_exact.tsv: for the whole track, every contig and\n"
            "                                      every annotation region, and for Err, Dup, Hap, Col and Err+Dup+Col, the windows of the scope,\n"
            "                                      the bases of the final labels, and the exact posterior mean and standard deviation of the bases\n"
            "                                      (what --uncertaintySamples estimates from samples); one GPU, not with --gpus N>1 or --sweepAlpha\n"
            "         --numBlocks                  after the final inference, write label_blocks_exact.tsv: for the whole track and every contig,\n"
            "                                      and for Err, Dup, Hap, Col and Err+Dup+Col, the number of blocks (maximal runs of windows, merged\n"
            "                                      across the chunks of a contig as the final BED merges them) in the final labels, and the exact\n"
            "                                      posterior mean and standard deviation of that number; no annotation-region scope (a block does\n"
            "                                      not belong to one region); one GPU, not with --gpus N>1 or --sweepAlpha\n"
            "         --jointEntropy               after the final inference, write path_uncertainty.tsv: for the whole track and every contig, the\n"
            "                                      exact entropy (nats) of the posterior distribution over label paths (exp of it: the effective\n"
            "                                      number of plausible segmentations), that entropy per window, the sum of the per-window posterior\n"
            "                                      entropies (which ignores the chain's correlations and is never smaller), and the exact\n"
            "                                      log-probability of the final labels; one GPU, not with --gpus N>1 or --sweepAlpha\n"
            "         --runBoundaries              after the final inference, write final_label_run_boundaries.tsv: for every two adjacent runs of\n"
            "                                      equal final label (the runs of final_label_runs_support.bed) inside one chunk, the exact\n"
            "                                      probability that the two runs' range switches once from the left label to the right one, and\n"
            "                                      given that, the posterior of where: the probability of the called position, the 2.5 / 50 /\n"
            "                                      97.5 %% quantiles and the mode; one GPU, not with --gpus N>1 or --sweepAlpha\n"
            "         --enforceMinimumLengths      with --viterbi: the final labels are the most probable path AMONG THE PATHS WHOSE RUNS MEET\n"
            "                                      --minimumLengths (Err, Dup, Col: ceil(length / windowLen) windows, at least 1; Hap: 1; at most 64\n"
            "                                      windows in sum; runs at a chunk's ends are exempt, the final BED's filter still acts on those), not\n"
            "                                      the best path with its short runs relabelled afterwards; viterbi_log_probability.tsv holds the score\n"
            "                                      of the path written, viterbi_min_length_cost.tsv the four window counts, the constrained and the\n"
            "                                      unconstrained score, their difference and the number of chunks whose two paths differ; one GPU, not\n"
            "                                      with --gpus N>1 or --sweepAlpha\n"
            "         --wholeContigs               with --viterbi --enforceMinimumLengths: the minimum lengths hold over the whole contig, not per\n"
            "                                      chunk: chunks adjacent in the chunk list with the same contig name are joined (the rule of\n"
            "                                      --numBlocks), a run counts across their boundary, and only runs at the ends of such a group are\n"
            "                                      exempt, so that the final BED's filter has nothing left to relabel inside a contig; the final\n"
            "                                      labels and viterbi_log_probability.tsv are the joined decoder's, viterbi_min_length_cost.tsv is\n"
            "                                      filled from the joined run and gains two columns: log_prob_constrained_per_chunk (the score\n"
            "                                      under the per-chunk rule) and short_runs_per_chunk_rule (the runs of the per-chunk labels, merged\n"
            "                                      over the chunks of a contig, that touch neither end of their group and are shorter than their\n"
            "                                      minimum: what the BED filter relabelled); one GPU, not with --gpus N>1 or --sweepAlpha\n"
            "         --keptBlocks                 with --minimumLengths: after every other output, write kept_block_probabilities.tsv: for the whole\n"
            "                                      track, every contig and (with --regionProbs FILE) every region, and for every label, the exact\n"
            "                                      probability that the scope holds a block of the label long enough to be kept (lengths in windows\n"
            "                                      as for --enforceMinimumLengths: ceil(length / windowLen), at least 1; Hap: 1; at most 58 windows),\n"
            "                                      runs merged across the chunks of a contig as the final BED merges them; one GPU, not with\n"
            "                                      --gpus N>1 or --sweepAlpha\n"
            "         --admissibleSamples N        with --minimumLengths: after every other output, draw N state paths from the posterior GIVEN THAT\n"
            "                                      EVERY RUN MEETS --minimumLengths (lengths in windows as for --enforceMinimumLengths, at most 64\n"
            "                                      windows in sum; runs at a chunk's ends are exempt) with the final parameters, and write\n"
            "                                      admissible_samples_summary.tsv and admissible_label_runs_support.bed in the formats of the two\n"
            "                                      --uncertaintySamples files; the seed is --uncertaintySeed; one GPU, not with --gpus N>1 or --sweepAlpha\n"
            "         --constrainedPosterior       with --minimumLengths: after the final inference, write admissible_mass.tsv: the four lengths in\n"
            "                                      windows (as for --enforceMinimumLengths: ceil(length / windowLen), at least 1; Hap: 1; at most 64\n"
            "                                      in sum), then for the whole track and every contig the chunks, the windows and the log of the\n"
            "                                      posterior probability that every run meets its length (runs at a chunk's ends are exempt; chunks\n"
            "                                      are independent, their logs add), and posterior_prediction_min_lengths.bed: the posterior BED of\n"
            "                                      -P given that the path meets the lengths; the final labels and every other output stay as they\n"
            "                                      are; one GPU, not with --gpus N>1 or --sweepAlpha\n"
            "         --mergedChunks               with --constrainedPosterior and / or --admissibleSamples: the minimum lengths hold over the whole\n"
            "                                      contig, not per chunk: chunks adjacent in the chunk list with the same contig name are joined (the\n"
            "                                      rule of --numBlocks and --wholeContigs), a run counts across their boundary, and only runs at the\n"
            "                                      ends of such a group are exempt; the files keep their names and formats, admissible_mass.tsv gains\n"
            "                                      one column, log_mass_per_chunk_rule (the mass under the per-chunk rule); it does not touch\n"
            "                                      --viterbi; one GPU, not with --gpus N>1 or --sweepAlpha\n"
            "         --expectedAccuracy chunks|contigs   the final labels (final BED, final summary tables) are the labelling of the LARGEST\n"
            "                                      EXPECTED NUMBER OF CORRECTLY LABELLED WINDOWS under the posterior of the final pass AMONG THE\n"
            "                                      LABELLINGS WHOSE RUNS MEET --minimumLengths (lengths in windows as for --enforceMinimumLengths, at\n"
            "                                      most 64 windows in sum): the exact form of what the final BED approximates by relabelling short\n"
            "                                      runs of the posterior argmax.  chunks: runs at a chunk's ends are exempt; contigs: the lengths\n"
            "                                      hold over the joined chunks of a contig.  Writes expected_accuracy.tsv (per contig and for the\n"
            "                                      track: windows, the unconstrained bound, the gain of the final BED's own rule, the gain decoded,\n"
            "                                      whether the final BED's own labelling has positive probability); every other file is the run's\n"
            "                                      without the option.  Needs --minimumLengths; not with --viterbi; one GPU, not with --gpus N>1,\n"
            "                                      HF_LOOPBACK_RANKS or --sweepAlpha\n"
            "         --expectedGains FILE         with --expectedAccuracy: a 4x4 tab-separated gain matrix, rows the true label, columns the label\n"
            "                                      called (Err, Dup, Hap, Col); the labelling of the largest expected gain is decoded [identity]\n"
            "         --lengthConstrainedEM        with --minimumLengths: the EM iterations take their statistics from the posterior GIVEN THAT EVERY\n"
            "                                      RUN MEETS --minimumLengths (lengths in windows as for --enforceMinimumLengths, at most 64 in sum;\n"
            "                                      runs at a chunk's ends are exempt), so the model is fitted for the constrained decoders: the\n"
            "                                      iteration rows of loglikelihood.tsv hold the objective, the sum of log Z_adm, and\n"
            "                                      length_constrained_em.tsv per iteration log Z_adm, log Z and their difference; the final inference\n"
            "                                      pass and every output stay the plain ones.  Not with --accelerate, --fitAlpha or --modelType\n"
            "                                      negative_binomial; one GPU, not with --gpus N>1, HF_LOOPBACK_RANKS or --sweepAlpha\n"
            "         --crossChunkEM               with --lengthConstrainedEM: the lengths hold over the joined chunks of a contig (the rule of\n"
            "                                      --wholeContigs and of the final BED), only runs at a contig's ends are exempt: the rows of\n"
            "                                      loglikelihood.tsv and length_constrained_em.tsv hold the sums over contigs; every other output\n"
            "                                      stays as it is\n"
            "         --runLengths L               after the final inference, write label_block_lengths_exact.tsv: for the whole track and every\n"
            "                                      contig, and for the label sets Err, Dup, Hap, Col and Err+Dup+Col, the exact posterior expectation\n"
            "                                      of the number of blocks of every length 1..L windows and of more than L (L in 1..64), beside the\n"
            "                                      counts in the final labels; blocks are merged across the chunks of a contig (the rule of\n"
            "                                      --numBlocks).  With --minimumLengths also label_blocks_kept_exact.tsv: per scope and label the\n"
            "                                      expected blocks, the expected blocks at or above the label's minimum (lengths in windows as for\n"
            "                                      --enforceMinimumLengths; L must reach the largest of them less one) and the expected windows in the\n"
            "                                      shorter ones; one GPU, not with --gpus N>1, HF_LOOPBACK_RANKS or --sweepAlpha\n"
            "         --totalsDistribution K       with --regionProbs FILE: after the final inference, write region_label_totals_exact.tsv: for every\n"
            "                                      region and the label sets Err, Dup, Hap, Col and Err+Dup+Col the exact posterior distribution of the\n"
            "                                      NUMBER OF WINDOWS of the region in the set: p_0 .. p_K and p_gtK (K in 1..62), their mean (NA where\n"
            "                                      p_gtK > 0) and the quantiles q025, q50, q975 (the smallest k whose cumulative probability reaches the\n"
            "                                      level; >K beyond the bins); one GPU, not with --gpus N>1, HF_LOOPBACK_RANKS or --sweepAlpha\n");
}

static bool dir_exists(const char* p) { struct stat sb; return stat(p, &sb) == 0 && S_ISDIR(sb.st_mode); }

static double random_factor(double dev) {                  // hmm_flagger.c:113-116 with (1-dev, 1+dev)
    if (dev == 0.0) return 1.0;
    srand((unsigned) time(nullptr));
    const double start = 1.0 - dev, end = 1.0 + dev;
    return (double) rand() / (double) (RAND_MAX / (end - start)) + start;
}

static std::string g_cli_error;      // an error of the command line's own (a table set that failed), reported like the library's
static void hf_cli_set_error(const std::string& e) { g_cli_error = e; }
static const char* cli_error_or(const char* lib) { return g_cli_error.empty() ? lib : g_cli_error.c_str(); }

// every value that comes from argv or from the environment, with its default; check_options fills in what the preset decides
struct Options {
    const char *program = nullptr, *trackName = "final_hmm_flagger";
    std::string preset = "hifi";
    const char *inputPath = nullptr, *alphaTsvPath = nullptr, *contigListPath = nullptr, *outputDir = nullptr, *sweepListPath = nullptr;
    int numberOfIterations = 100, numberOfCollapsedComps = -1, chunkLen = 20000000, windowLen = -1, threads = 4;
    double convergenceTol = 0.001, maxHighMapqRatio = 0.25, minHighMapqRatio = 0.75, minReadFractionAtEnds = -1.0, initialRandomDeviation = 0.0;
    bool adjustContigEnds = true, writeParamsPerIter = false, writePosterior = false, dumpBin = false, acceleration = false;
    bool viterbi = false, enforceMinLen = false, wholeContigs = false, mergedChunks = false, keptBlocks = false, constrainedPost = false, minLenGiven = false, lengthConstrainedEM = false, crossChunkEM = false;
    int uncertaintySamples = 0; bool uncertaintySet = false, uncertaintySeedBad = false; uint64_t uncertaintySeed = 0;
    int admissibleSamples = 0; bool admissibleSet = false;
    const char *expectedAccuracy = nullptr, *expectedGainsPath = nullptr;   // chunks | contigs; the gain TSV
    bool runConfidence = false, exactTotals = false, numBlocks = false, jointEntropy = false, runBoundaries = false;
    int runLengths = 0; bool runLengthsSet = false;   // --runLengths L
    int totalsDistribution = 0; bool totalsDistributionSet = false;   // --totalsDistribution K
    const char* regionProbsPath = nullptr;
    bool fitAlpha = false, fitAlphaBad = false, fitAlphaOptions = false;
    uint8_t fitAlphaMask[16] = {1, 0, 1, 0,  0, 1, 1, 0,  1, 1, 1, 1,  0, 0, 1, 1};   // the ten entries the reference's tuner frees
    double fitAlphaMax = 0.8;                                                          // its --upperBound (its --lowerBound is 0)
    int fitAlphaEvery = 2;
    int modelType = -1, device = 0, algo = HF_ALGO_SCAN, nGpus = 0, exchange = -1;
    const char* binArrayFilePath = nullptr;
    bool writeBenchmarkingStatsPerIteration = false;
    double overlapRatioThreshold = 0.4;
    std::vector<std::string> labelNames;
    int32_t minLenPerState[4] = {0, 0, 0, 0};
    int loopbackRanks = 0;     // test transport, not an option: HF_LOOPBACK_RANKS=N runs N ranks that share ONE GPU (no RCCL) through the multi-GPU path
    bool phaseTiming = false;  // HF_CLI_TIMING=1: wall time of every phase on stderr (where does a run go now that the E-step is milliseconds?)
    bool warmPasses = true;    // HF_CLI_WARM=0: bring up the runtime only
};

// --regionProbs: a region of a BED3+ file (ctg start end [name])
struct Region { std::string ctg, name; int64_t start, end; };

// The session of a run, with the E-step behind runHMMFlagger: one context on one GPU, or the sharded multi-GPU list (hmm_flagger_multi.h)
struct Run {
    Options opt;
    std::vector<Region> regions;                               // --regionProbs
    std::vector<std::string> sweepPaths;                       // --sweepAlpha: the TSVs of the list and what they hold
    std::vector<std::vector<double>> sweepAlphas;
    double alpha[16] = {0};                                    // --alphaTsv
    double gains[16] = {1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1};   // --expectedGains [truth * 4 + called]
    int32_t minLenWindows[4] = {1, 1, 1, 1};                   // --minimumLengths in windows (min_len_windows)
    hf_windows w{};                                            // the table's windows, once the input is read (load_input)
    int64_t N = 0; int nChunks = 0;
    double realtimeStart = 0.0, phaseStart = 0.0;
    void phase(const char* name) {
        if (!opt.phaseTiming) return;
        const double now = real_time();
        fprintf(stderr, "[phase] %-28s %8.1f ms\n", name, (now - phaseStart) * 1e3);
        phaseStart = now;
    }
    hf_ctx* ctx = nullptr;
    hf_multi* multi = nullptr;
    hfio_table* tab = nullptr;
    std::vector<double> stats;
    static hf_params params(hfm_model* m) { hf_params p; hfm_params(m, &p); return p; }
    int estep(hfm_model* m, int mode, double* out) {
        const hf_params p = params(m);
        if (multi) return hf_multi_estep(multi, &p, mode, out);
        int rc = hf_estep(ctx, &p, mode, nullptr);
        if (rc == HF_OK) rc = hf_finish(ctx, out, nullptr);
        return rc;
    }
    int labels(int8_t* out) { return multi ? hf_multi_get_labels(multi, out) : hf_get_labels(ctx, out); }
    // most-probable path with the model's current parameters: labels (list order) and the run's log-probability
    int viterbi(hfm_model* m, int8_t* out, double* log_prob) {
        const hf_params p = params(m);
        if (multi) {
            const int rc = hf_multi_viterbi(multi, &p, log_prob);
            return rc != HF_OK ? rc : hf_multi_get_viterbi_labels(multi, out);
        }
        int rc = hf_viterbi(ctx, &p, nullptr);
        if (rc == HF_OK) rc = hf_viterbi_finish(ctx, log_prob, nullptr);
        return rc != HF_OK ? rc : hf_get_viterbi_labels(ctx, out);
    }
    // ... among the paths whose runs meet min_len windows per state (one GPU)
    int viterbi_minlen(hfm_model* m, const int32_t min_len[4], int8_t* out, double* log_prob) {
        const hf_params p = params(m);
        int rc = hf_viterbi_minlen(ctx, &p, min_len, nullptr);
        if (rc == HF_OK) rc = hf_viterbi_minlen_finish(ctx, log_prob, nullptr);
        return rc != HF_OK ? rc : hf_get_viterbi_minlen_labels(ctx, out);
    }
    // ... with the rule over the groups of joined chunks (--wholeContigs)
    int viterbi_minlen_joined(hfm_model* m, const int32_t min_len[4], const uint8_t* joined, int8_t* out, double* log_prob) {
        const hf_params p = params(m);
        int rc = hf_viterbi_minlen_joined(ctx, &p, min_len, joined, nullptr);
        if (rc == HF_OK) rc = hf_viterbi_minlen_finish(ctx, log_prob, nullptr);
        return rc != HF_OK ? rc : hf_get_viterbi_minlen_labels(ctx, out);
    }
    // (joined: null for the per-chunk rule, else the rule over the groups of joined chunks, --mergedChunks)
    int minlen_posterior(hfm_model* m, const int32_t min_len[4], const uint8_t* joined, double* log_mass_total) {
        const hf_params p = params(m);
        const int rc = joined ? hf_minlen_posterior_joined(ctx, &p, min_len, joined, nullptr) : hf_minlen_posterior(ctx, &p, min_len, nullptr);
        return rc != HF_OK ? rc : hf_minlen_posterior_finish(ctx, log_mass_total, nullptr);
    }
    // the E-step under min_len windows per state (one GPU): the statistics, and the plain sum of log Z of the same parameters
    // (joined: null for the per-chunk rule, else the rule over the groups of joined chunks, --crossChunkEM)
    int estep_minlen(hfm_model* m, const int32_t min_len[4], const uint8_t* joined, double* out, double* log_z) {
        const hf_params p = params(m);
        const int rc = joined ? hf_estep_minlen_joined(ctx, &p, min_len, joined, nullptr) : hf_estep_minlen(ctx, &p, min_len, nullptr);
        return rc != HF_OK ? rc : hf_estep_minlen_finish(ctx, out, log_z, nullptr);
    }
    int posterior(int64_t first, int64_t n, double* out) {
        return multi ? hf_multi_get_posterior(multi, first, n, out) : hf_get_posterior(ctx, first, n, out);
    }
    const char* error() const { return multi ? hf_multi_last_error() : hf_last_error(); }
};
static Run* g_run = nullptr;
static const char* run_error() { return cli_error_or(g_run ? g_run->error() : hf_last_error()); }

// writeBenchmarkingStats, hmm_flagger.c:134-162.  The tables are OUTPUT: the labels of the pass come down (pinned buffer), and the
// tables are computed and written by a worker thread while the EM goes on (the "initial" tables used to sit inside
// the EM phase).  Round 5: every table set has a worker of its own — the "final" tables no longer queue behind the
// "initial" ones, and the final BED is written beside them; summary_join() before the process reports that it is done.
struct SummaryJob {
    std::thread th;
    std::vector<int8_t> labels;
    int rc = 0;
    std::string err, path;
};
static std::vector<std::unique_ptr<SummaryJob>> g_summaries;
static void summary_wait_quietly() { for (auto& j : g_summaries) if (j->th.joinable()) j->th.join(); }
static int die_estep(int rc) {
    summary_wait_quietly();                                                         // (a worker still writing tables: let it finish before the process unwinds)
    if (rc == HF_E_SCALE) fprintf(stderr, "scale is very low!\n");                 // hmm.c:413
    else if (rc == HF_E_NAN) fprintf(stderr, "[Error] prob is NAN\n");             // hmm_utils.c:784
    else fprintf(stderr, "[%s] Error: %s\n", ts(), run_error());
    return EXIT_FAILURE;
}
// --sweepAlpha: wait for every table worker; a failed table set is reported and fails its candidate only (the sweep goes on)
static bool summary_join_report() {
    summary_wait_quietly();
    bool ok = true;
    for (auto& j : g_summaries)
        if (j->rc != 0) { fprintf(stderr, "[%s] %s\n", ts(), j->err.c_str()); ok = false; }
    g_summaries.clear();
    return ok;
}
static void summary_join() {
    summary_wait_quietly();
    for (auto& j : g_summaries)
        if (j->rc != 0) { fprintf(stderr, "[%s] %s\n", ts(), j->err.c_str()); exit(EXIT_FAILURE); }
}
// `labels`: the labels of the pass when the caller has them already (N bytes), nullptr: they are fetched here
static int write_summary(Run& run, const std::string& dir, const std::string& suffix, const int8_t* labels) {
    const double t_begin = real_time();
    const int64_t N = hfio_n_windows(run.tab);
    // At most three table sets in flight (--writeBenchmarkingStatsPerIteration starts one per EM iteration, an iteration takes
    // 0.1 ms and a table set several: a hundred jobs with an N-byte label copy and `threads` workers each would pile up) — the oldest is
    // joined first, and a table set that failed is reported at the next call instead of at the very end.
    {
        size_t running = 0;
        for (auto& j : g_summaries) running += j->th.joinable();
        for (auto& j : g_summaries) {
            if (running < 3) break;
            if (j->th.joinable()) { j->th.join(); running--; std::vector<int8_t>().swap(j->labels); }
        }
        for (auto& j : g_summaries)
            if (!j->th.joinable() && j->rc != 0) { hf_cli_set_error(j->err); return HF_E_ARG; }
    }
    g_summaries.emplace_back(new SummaryJob());
    SummaryJob* job = g_summaries.back().get();
    job->labels.resize((size_t) N);
    if (labels) memcpy(job->labels.data(), labels, (size_t) N);
    else {
        const int rc = run.labels(job->labels.data());
        if (rc != HF_OK) return rc;
    }
    job->path = dir + "/prediction_summary_" + suffix + ".tsv";
    const bool timing = run.opt.phaseTiming;
    job->th = std::thread([&run, job, labelNames = run.opt.labelNames, binArrayFilePath = run.opt.binArrayFilePath,
                           overlapRatioThreshold = run.opt.overlapRatioThreshold, threads = run.opt.threads, suffix, timing, t_begin] {
        std::vector<const char*> names;
        for (const auto& s : labelNames) names.push_back(s.c_str());
        if (hfio_write_summary(run.tab, job->labels.data(), job->path.c_str(), binArrayFilePath, names.empty() ? nullptr : names.data(),
                               (int) names.size(), overlapRatioThreshold, threads) != 0) {
            job->rc = -1; job->err = hfio_last_error();
            return;
        }
        fprintf(stderr, "[%s] Writing tables to file %s is done.\n", ts(), job->path.c_str());
        if (timing) fprintf(stderr, "[phase]   (summary tables %s: %.1f ms on their own thread)\n", suffix.c_str(), (real_time() - t_begin) * 1e3);
    });
    if (timing) fprintf(stderr, "[phase]   (summary tables %s: labels down + worker started in %.2f ms)\n", suffix.c_str(), (real_time() - t_begin) * 1e3);
    return HF_OK;
}

static void write_params(const hfm_model* m, const std::string& dir, const std::string& suffix) {   // hmm_flagger.c:119-132
    fprintf(stderr, "[%s] Writing transition tsv...\n", ts());
    hfm_write_transition_tsv(m, (dir + "/transition_" + suffix + ".tsv").c_str());
    fprintf(stderr, "[%s] Writing emission tsv ...\n", ts());
    hfm_write_emission_tsv(m, (dir + "/emission_" + suffix + ".tsv").c_str());
}

// --regionProbs: the regions of a BED3+ file (ctg start end [name]), every line checked before the input is read
static bool read_regions(const char* path, std::vector<Region>& regions) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "[%s] Error: --regionProbs: cannot read %s\n", ts(), path); return false; }
    char* line = nullptr; size_t cap = 0; ssize_t len; long ln = 0;
    bool ok = true;
    while ((len = getline(&line, &cap, f)) >= 0) {
        ln++;
        std::string l(line, (size_t) len);
        while (!l.empty() && (l.back() == '\n' || l.back() == '\r')) l.pop_back();
        if (l.find_first_not_of(" \t") == std::string::npos || l[0] == '#' || l.compare(0, 5, "track") == 0 || l.compare(0, 7, "browser") == 0) continue;
        std::vector<std::string> fld;
        size_t a = 0;
        while (a <= l.size()) {
            size_t b = l.find_first_of(" \t", a);
            if (b == std::string::npos) b = l.size();
            if (b > a) fld.push_back(l.substr(a, b - a));
            a = b + 1;
        }
        auto integer = [](const std::string& x, int64_t* v) {
            char* end = nullptr;
            errno = 0;
            const long long r = strtoll(x.c_str(), &end, 10);
            if (x.empty() || *end != 0 || errno != 0) return false;
            *v = (int64_t) r;
            return true;
        };
        Region r;
        if (fld.size() < 3) { fprintf(stderr, "[%s] Error: --regionProbs %s line %ld: expected at least 3 fields (ctg start end [name])\n", ts(), path, ln); ok = false; break; }
        if (!integer(fld[1], &r.start) || !integer(fld[2], &r.end)) {
            fprintf(stderr, "[%s] Error: --regionProbs %s line %ld: start and end should be integers\n", ts(), path, ln); ok = false; break;
        }
        if (r.start < 0 || r.start >= r.end) { fprintf(stderr, "[%s] Error: --regionProbs %s line %ld: expected 0 <= start < end\n", ts(), path, ln); ok = false; break; }
        r.ctg = fld[0];
        r.name = fld.size() > 3 ? fld[3] : ".";
        regions.push_back(r);
    }
    free(line);
    fclose(f);
    return ok;
}

// the report files of late_outputs: Report, Jobs, TableFile and every write_* (the scopes and joins: hf_cli_scopes.h)
#include "hf_cli_reports.h"

// --sweepAlpha: the alpha TSV paths of the list (blank lines and lines starting with '#' skipped), every TSV read and checked
static bool read_sweep_list(const char* listPath, std::vector<std::string>& paths, std::vector<std::vector<double>>& alphas) {
    FILE* f = fopen(listPath, "r");
    if (!f) { fprintf(stderr, "[%s] Error: cannot read the --sweepAlpha list %s\n", ts(), listPath); return false; }
    char line[8192];
    while (fgets(line, sizeof line, f)) {
        std::string t(line);
        while (!t.empty() && (t.back() == '\n' || t.back() == '\r' || t.back() == ' ' || t.back() == '\t')) t.pop_back();
        size_t a = 0;
        while (a < t.size() && (t[a] == ' ' || t[a] == '\t')) a++;
        t = t.substr(a);
        if (t.empty() || t[0] == '#') continue;
        paths.push_back(t);
    }
    fclose(f);
    if (paths.empty()) { fprintf(stderr, "[%s] Error: the --sweepAlpha list %s names no alpha TSV.\n", ts(), listPath); return false; }
    for (const auto& pth : paths) {
        std::vector<double> al(16, 0.0);
        const int rc = hfm_read_alpha_tsv(pth.c_str(), al.data());
        if (rc == -2) { fprintf(stderr, "[%s] Error: There is at least one alpha value in '%s' not between 0 and 1. \n", ts(), pth.c_str()); return false; }
        if (rc != 0) { fprintf(stderr, "[%s] Error: cannot read %s (--sweepAlpha list %s)\n", ts(), pth.c_str(), listPath); return false; }
        alphas.push_back(al);
    }
    return true;
}

// closes the log-likelihood table of a run however the run ends (a failed E-step leaves what it wrote, as a separate process does)
struct FileCloser { FILE*& f; ~FileCloser() { if (f) fclose(f); f = nullptr; } };

// a positive integer that fits an int, or -1
static int positive_int(const char* s) {
    char* end = nullptr;
    const long v = strtol(s, &end, 10);
    return (end != s && *end == 0 && v > 0 && v <= INT32_MAX) ? (int) v : -1;
}

// the options that only raise a flag or store their argument (as text, atoi, atof): code -> member; parse_options' switch has the others
static const struct { int code; bool Options::*flag; } kFlagOptions[] = {
    {'B', &Options::dumpBin}, {'k', &Options::writeBenchmarkingStatsPerIteration}, {'w', &Options::writeParamsPerIter}, {'P', &Options::writePosterior},
    {'s', &Options::acceleration}, {kOptViterbi, &Options::viterbi}, {kOptRunConfidence, &Options::runConfidence}, {kOptExactTotals, &Options::exactTotals},
    {kOptNumBlocks, &Options::numBlocks}, {kOptRunBoundaries, &Options::runBoundaries}, {kOptJointEntropy, &Options::jointEntropy}, {kOptFitAlpha, &Options::fitAlpha},
    {kOptEnforceMinLen, &Options::enforceMinLen}, {kOptKeptBlocks, &Options::keptBlocks}, {kOptConstrainedPosterior, &Options::constrainedPost}, {kOptWholeContigs, &Options::wholeContigs}, {kOptMergedChunks, &Options::mergedChunks},
    {kOptLengthConstrainedEM, &Options::lengthConstrainedEM}, {kOptCrossChunkEM, &Options::crossChunkEM}};
static const struct { int code; const char* Options::*text; } kTextOptions[] = {
    {'i', &Options::inputPath}, {'N', &Options::trackName}, {'a', &Options::binArrayFilePath}, {'c', &Options::contigListPath}, {'A', &Options::alphaTsvPath},
    {'o', &Options::outputDir}, {kOptSweepAlpha, &Options::sweepListPath}, {kOptRegionProbs, &Options::regionProbsPath},
    {kOptExpectedAccuracy, &Options::expectedAccuracy}, {kOptExpectedGains, &Options::expectedGainsPath}};
static const struct { int code; int Options::*number; } kIntOptions[] = {
    {'n', &Options::numberOfIterations}, {'p', &Options::numberOfCollapsedComps}, {'@', &Options::threads}, {'C', &Options::chunkLen}, {'W', &Options::windowLen},
    {kOptDevice, &Options::device}, {kOptGpus, &Options::nGpus}};
static const struct { int code; double Options::*real; } kRealOptions[] = {
    {'t', &Options::convergenceTol}, {'f', &Options::minReadFractionAtEnds}, {'v', &Options::overlapRatioThreshold}, {'D', &Options::initialRandomDeviation},
    {'q', &Options::maxHighMapqRatio}, {'Q', &Options::minHighMapqRatio}};

// argv -> o.  false: the command line ends here (a message or the usage is printed); only --minimumLengths' format and --exchange's value
// are refused this early, so they win over every check of check_options
static bool parse_options(int argc, char* argv[], Options& o) {
    o.program = strrchr(argv[0], '/');
    o.program = o.program ? o.program + 1 : argv[0];
    // "--e" and "--ex" were unique prefixes of --exchange until --exactTotals came, "--ru" and "--run" of --runConfidence until
    // --runBoundaries came, "--l" of --labelNames until --lengthConstrainedEM came: they keep their meaning (the rule of long_options
    // above: a prefix that resolved once resolves to the same option in every later build)
    static const struct { const char *pre, *full; } kept[] = {{"--ex", "--exchange"}, {"--e", "--exchange"}, {"--run", "--runConfidence"}, {"--ru", "--runConfidence"},
                                                              {"--l", "--labelNames"}};
    static std::vector<std::string> rewritten;                   // (argv points into it from here on)
    rewritten.reserve((size_t) argc);
    for (int i = 1; i < argc && strcmp(argv[i], "--") != 0; i++)
        for (const auto& k : kept) {
            const size_t n = strlen(k.pre);
            if (strncmp(argv[i], k.pre, n) == 0 && (argv[i][n] == '\0' || argv[i][n] == '=')) {
                rewritten.push_back(std::string(k.full) + (argv[i] + n));
                argv[i] = rewritten.back().data();
                break;
            }
        }
    int c;
    while (~(c = getopt_long(argc, argv, "i:x:f:en:t:m:q:C:W:c:@:p:A:a:wkPo:v:l:D:BN:M:s", long_options, nullptr))) {
        bool plain = false;
        for (const auto& p : kFlagOptions) if (p.code == c) { o.*p.flag = true; plain = true; }
        for (const auto& p : kTextOptions) if (p.code == c) { o.*p.text = optarg; plain = true; }
        for (const auto& p : kIntOptions) if (p.code == c) { o.*p.number = atoi(optarg); plain = true; }
        for (const auto& p : kRealOptions) if (p.code == c) { o.*p.real = atof(optarg); plain = true; }
        if (plain) continue;
        switch (c) {
            case 'x': o.preset = optarg; break;
            case 'e': o.adjustContigEnds = false; break;
            case 'm':                                           // hmm_utils.c:18-29
                if (!strcmp(optarg, "gaussian")) o.modelType = HF_MODEL_GAUSSIAN;
                else if (!strcmp(optarg, "trunc_exp_gaussian") || !strcmp(optarg, "truncated_exponential_gaussian"))
                    o.modelType = HF_MODEL_TRUNC_EXP_GAUSSIAN;
                else if (!strcmp(optarg, "nb") || !strcmp(optarg, "negative_binomial")) o.modelType = HF_MODEL_NEGATIVE_BINOMIAL;
                else o.modelType = -2;
                break;
            case 'l': {                                          // hmm_flagger.c:721-724: names + "Unk"
                std::string s(optarg);
                size_t a = 0;
                o.labelNames.clear();
                while (true) {
                    const size_t b = s.find(',', a);
                    o.labelNames.push_back(s.substr(a, b == std::string::npos ? std::string::npos : b - a));
                    if (b == std::string::npos) break;
                    a = b + 1;
                }
                o.labelNames.push_back("Unk");
                break;
            }
            case 'M': {                                          // hmm_flagger.c:737-749
                int a, b, d;
                if (sscanf(optarg, "%d,%d,%d", &a, &b, &d) != 3 || strchr(strchr(strchr(optarg, ',') + 1, ',') + 1, ',')) {
                    fprintf(stderr, "[%s] Error: --minimumLengths should contain only 3 tab-delimited positive integers.\n", ts()); return false;
                }
                o.minLenPerState[0] = a; o.minLenPerState[1] = b; o.minLenPerState[3] = d;
                o.minLenGiven = true;
                break;
            }
            case kOptHipAlgo: o.algo = !strcmp(optarg, "seq") ? HF_ALGO_SEQ : HF_ALGO_SCAN; break;
            case kOptUncertaintySamples: o.uncertaintySet = true; o.uncertaintySamples = positive_int(optarg); break;
            case kOptUncertaintySeed: {
                char* end = nullptr;
                o.uncertaintySeed = strtoull(optarg, &end, 10);
                o.uncertaintySeedBad = end == optarg || *end != 0 || optarg[0] == '-';
                break;
            }
            case kOptAdmissibleSamples: o.admissibleSet = true; o.admissibleSamples = positive_int(optarg); break;
            case kOptRunLengths: o.runLengthsSet = true; o.runLengths = positive_int(optarg); break;
            case kOptTotalsDistribution: o.totalsDistributionSet = true; o.totalsDistribution = positive_int(optarg); break;
            case kOptFitAlphaEntries: {                          // pre,state[:pre,state...]
                o.fitAlphaOptions = true;
                memset(o.fitAlphaMask, 0, sizeof o.fitAlphaMask);
                const char* q = optarg;
                bool ok = *q != 0;
                while (ok && *q) {
                    ok = q[0] >= '0' && q[0] <= '3' && q[1] == ',' && q[2] >= '0' && q[2] <= '3' && (q[3] == 0 || (q[3] == ':' && q[4] != 0));
                    if (!ok) break;
                    o.fitAlphaMask[(q[0] - '0') * 4 + (q[2] - '0')] = 1;
                    q += q[3] ? 4 : 3;
                }
                if (!ok) o.fitAlphaBad = true;
                break;
            }
            case kOptFitAlphaMax: {
                char* end = nullptr;
                o.fitAlphaOptions = true;
                o.fitAlphaMax = strtod(optarg, &end);
                if (end == optarg || *end != 0 || !(o.fitAlphaMax >= 0.0 && o.fitAlphaMax < 1.0)) o.fitAlphaMax = -1.0;
                break;
            }
            case kOptFitAlphaEvery: o.fitAlphaOptions = true; o.fitAlphaEvery = positive_int(optarg); break;
            case kOptExchange:
                if (!strcmp(optarg, "chunks")) o.exchange = HF_EXCHANGE_CHUNKS;
                else if (!strcmp(optarg, "ranks")) o.exchange = HF_EXCHANGE_RANKS;
                else { fprintf(stderr, "[%s] Error: --exchange can be chunks or ranks.\n", ts()); return false; }
                break;
            default:
                if (c != 'h') fprintf(stderr, "[E::main] undefined option %c\n", c);
                usage(o.program);
                return false;
        }
    }
    return true;
}

static void read_environment(Options& o) {
    if (const char* e = getenv("HF_LOOPBACK_RANKS")) o.loopbackRanks = atoi(e);
    o.phaseTiming = getenv("HF_CLI_TIMING") != nullptr;
    o.warmPasses = !(getenv("HF_CLI_WARM") && getenv("HF_CLI_WARM")[0] == '0');
}

// Which one-GPU rule an option's refusal follows.  The options that came up to --jointEntropy (and --fitAlpha) refuse --gpus N>1 and
// --sweepAlpha only: under HF_LOOPBACK_RANKS they pass here and fail after the EM with "needs a single-GPU context".  The four that came
// later refuse HF_LOOPBACK_RANKS here as well.  The difference is today's behaviour and is kept as it is.
enum OneGpuRule { kNoGpuRule, kOneGpu, kOneGpuNoLoopback };
// One row of refusals: the option as printed, whether it was given, then what is tried in this order: `refusal` (the rest of the sentence
// when its argument is bad or an option it needs is missing; nullptr: fine) and its one-GPU rule
struct OptionCheck { const char* name; bool given; const char* refusal; OneGpuRule rule; };
template <size_t n> static bool check_rows(const Options& o, const OptionCheck (&rows)[n]) {
    for (const OptionCheck& r : rows) {
        if (!r.given) continue;
        if (r.refusal) { fprintf(stderr, "[%s] Error: %s %s.\n", ts(), r.name, r.refusal); return false; }
        if (r.rule == kNoGpuRule || !(o.nGpus > 1 || o.sweepListPath || (r.rule == kOneGpuNoLoopback && o.loopbackRanks > 0))) continue;
        fprintf(stderr, r.rule == kOneGpu ? "[%s] Error: %s runs on one GPU: it cannot be combined with --gpus N>1 or --sweepAlpha.\n"
                                          : "[%s] Error: %s runs on one GPU: it cannot be combined with --gpus N>1, HF_LOOPBACK_RANKS or --sweepAlpha.\n", ts(), r.name);
        return false;
    }
    return true;
}

// --enforceMinimumLengths and its kin: the lengths in windows of W bases.  A run of k windows passes the final BED's `len < minlen` test
// exactly when k * W >= minlen; Hap has no minimum.  false: they do not fit the lanes (said)
static bool min_len_windows(Run& s, int W) {
    const Options& o = s.opt;
    long long sum = 0;
    for (int st = 0; st < 4; st++) {
        const long long w = st == 2 ? 1 : std::max(1LL, ((long long) o.minLenPerState[st] + W - 1) / W);
        s.minLenWindows[st] = (int32_t) std::min(w, 1000000LL);
        sum += s.minLenWindows[st];
    }
    const int32_t* const mw = s.minLenWindows;
    // --keptBlocks: one label at a time, each within the lanes of hf_get_long_run_log_probs
    for (int st = 0; o.keptBlocks && st < 4; st++)
        if (long_run_lanes(1 << st, mw[st]) > HF_LONGRUN_MAX_LANES) {
            fprintf(stderr, "[%s] Error: --keptBlocks: the minimum lengths %d,%d,%d (Err,Dup,Col) are %d,%d,%d,%d windows of %d bases (Err,Dup,Hap,Col); a label's may be %d windows at most.\n",
                    ts(), o.minLenPerState[0], o.minLenPerState[1], o.minLenPerState[3], mw[0], mw[1], mw[2], mw[3], W, HF_LONGRUN_MAX_LANES - 6);
            return false;
        }
    // --runLengths with --minimumLengths: the bins below a label's minimum are counted one by one, so the spectrum must reach them
    if (o.runLengthsSet && o.minLenGiven && o.runLengths < *std::max_element(mw, mw + 4) - 1) {
        fprintf(stderr, "[%s] Error: --runLengths %d: --minimumLengths %d,%d,%d (Err,Dup,Col) are %d,%d,%d,%d windows of %d bases (Err,Dup,Hap,Col); label_blocks_kept_exact.tsv needs --runLengths of at least %d.\n",
                ts(), o.runLengths, o.minLenPerState[0], o.minLenPerState[1], o.minLenPerState[3], mw[0], mw[1], mw[2], mw[3], W, *std::max_element(mw, mw + 4) - 1);
        return false;
    }
    if (!(o.enforceMinLen || o.constrainedPost || o.admissibleSet || o.expectedAccuracy || o.lengthConstrainedEM) || sum <= HF_MINLEN_MAX_LANES) return true;
    std::string who;                                           // the options that walk the expanded chain, as given
    for (const char* n : {o.enforceMinLen ? "enforceMinimumLengths" : nullptr, o.wholeContigs ? "wholeContigs" : nullptr, o.constrainedPost ? "constrainedPosterior" : nullptr,
                          o.admissibleSet ? "admissibleSamples" : nullptr, o.mergedChunks ? "mergedChunks" : nullptr, o.expectedAccuracy ? "expectedAccuracy" : nullptr,
                          o.lengthConstrainedEM ? "lengthConstrainedEM" : nullptr, o.crossChunkEM ? "crossChunkEM" : nullptr})
        if (n) who += (who.empty() ? "" : ", --") + std::string(n);
    fprintf(stderr, "[%s] Error: --%s: the minimum lengths are %d,%d,%d,%d windows of %d bases (Err,Dup,Hap,Col), above %d in sum.\n",
            ts(), who.c_str(), mw[0], mw[1], mw[2], mw[3], W, HF_MINLEN_MAX_LANES);
    return false;
}
static bool uses_min_len_windows(const Options& o) { return o.enforceMinLen || o.keptBlocks || o.constrainedPost || o.admissibleSet || o.expectedAccuracy || o.lengthConstrainedEM || (o.runLengthsSet && o.minLenGiven); }

// --expectedGains: four lines of four tab-separated numbers, rows the true label, columns the label called, read line by line and
// token by token as the alpha TSV is; unlike an alpha a gain may be any finite number up to 1e100 in magnitude.  false: not such a file
static bool read_gains_tsv(const char* path, double gains[16]) {
    FILE* f = fopen(path, "r");
    if (!f) return false;
    char* line = nullptr; size_t cap = 0;
    int rows = 0;
    bool ok = true;
    while (ok && getline(&line, &cap, f) != -1) {
        size_t L = strlen(line);
        while (L > 0 && (line[L - 1] == '\n' || line[L - 1] == '\r')) line[--L] = '\0';
        if (L == 0) continue;                                  // (an empty line, e.g. behind the last row)
        int j = 0; char* save = nullptr;
        for (char* tok = strtok_r(line, "\t", &save); tok && ok; tok = strtok_r(nullptr, "\t", &save)) {
            char* end = nullptr;
            const double v = strtod(tok, &end);
            ok = rows < 4 && j < 4 && end != tok && *end == '\0' && std::fabs(v) <= 1e100;   // (a NaN fails the comparison)
            if (ok) gains[rows * 4 + j++] = v;
        }
        ok = ok && j == 4;
        rows++;
    }
    free(line);
    fclose(f);
    return ok && rows == 4;
}

// Everything that can be refused before the input is read, in a fixed order (tests/test_cli_refusals_cpu.py: of two bad options the one
// checked first is reported).  false: refused (said).  Fills in the session: regions, sweep list, alpha, and the options the preset decides.
static bool check_options(Run& s) {
    Options& o = s.opt;
    const char* const positive = "should be a positive integer";
    const char* const needsMinLen = o.minLenGiven ? nullptr : "needs --minimumLengths";
    // the rows in the order of the refusals (--uncertaintySamples has two: the seed's argument is checked between its own argument and its
    // one-GPU rule); the --fitAlpha group has its place between --jointEntropy and the region file
    const OptionCheck beforeRegions[] = {
        {"--uncertaintySamples", o.uncertaintySet, o.uncertaintySamples < 1 ? positive : nullptr, kNoGpuRule},
        {"--uncertaintySeed", true, o.uncertaintySeedBad ? "should be a non-negative integer" : nullptr, kNoGpuRule},
        {"--uncertaintySamples", o.uncertaintySet, nullptr, kOneGpu},
        {o.runConfidence ? "--runConfidence" : "--regionProbs", o.runConfidence || o.regionProbsPath, nullptr, kOneGpu},
        {"--runBoundaries", o.runBoundaries, nullptr, kOneGpu},
        {"--exactTotals", o.exactTotals, nullptr, kOneGpu},
        {"--numBlocks", o.numBlocks, nullptr, kOneGpu},
        {"--jointEntropy", o.jointEntropy, nullptr, kOneGpu},
        {"--fitAlphaEntries", true, o.fitAlphaBad ? "should be pre,state pairs of state indices 0..3 separated by ':' (e.g. 0,0:2,2)" : nullptr, kNoGpuRule},
        {"--fitAlphaMax", true, o.fitAlphaMax < 0.0 ? "should be a number in [0, 1)" : nullptr, kNoGpuRule},
        {"--fitAlphaEvery", true, o.fitAlphaEvery < 1 ? positive : nullptr, kNoGpuRule},
        {"--fitAlphaEntries, --fitAlphaMax and --fitAlphaEvery", o.fitAlphaOptions, o.fitAlpha ? nullptr : "need --fitAlpha", kNoGpuRule},
        {"--fitAlpha", o.fitAlpha, o.acceleration ? "cannot be combined with --accelerate (SQUAREM extrapolates the other parameters only)" : nullptr, kOneGpu},
        {"--fitAlpha", o.fitAlpha, o.modelType != HF_MODEL_NEGATIVE_BINOMIAL ? nullptr :
                                   "needs --modelType gaussian or trunc_exp_gaussian (the negative_binomial emission has no alpha)", kNoGpuRule},
    };
    const OptionCheck afterRegions[] = {
        {"--gpus", true, o.nGpus < 0 || o.nGpus > 64 || o.loopbackRanks < 0 || o.loopbackRanks > 64 ? "should be between 1 and 64" : nullptr, kNoGpuRule},
        {"--gpus and HF_LOOPBACK_RANKS", o.nGpus > 0 && o.loopbackRanks > 0, "exclude each other", kNoGpuRule},
        // (--wholeContigs is refused wherever --enforceMinimumLengths is, and its row comes first so that the line names it)
        {"--wholeContigs", o.wholeContigs, o.viterbi && o.enforceMinLen ? nullptr : "needs --viterbi --enforceMinimumLengths", kOneGpuNoLoopback},
        {"--enforceMinimumLengths", o.enforceMinLen, o.viterbi ? nullptr : "needs --viterbi", kOneGpuNoLoopback},
        {"--keptBlocks", o.keptBlocks, needsMinLen, kOneGpuNoLoopback},
        // (--mergedChunks is refused wherever the option it acts on is: that option's line names it too, its own row comes last)
        {o.mergedChunks ? "--constrainedPosterior --mergedChunks" : "--constrainedPosterior", o.constrainedPost, needsMinLen, kOneGpuNoLoopback},
        {o.mergedChunks ? "--admissibleSamples --mergedChunks" : "--admissibleSamples", o.admissibleSet, o.admissibleSamples < 1 ? positive : needsMinLen, kOneGpuNoLoopback},
        {"--mergedChunks", o.mergedChunks, o.constrainedPost || o.admissibleSet ? nullptr : "needs --constrainedPosterior or --admissibleSamples", kOneGpuNoLoopback},
        {"--expectedAccuracy", o.expectedAccuracy != nullptr,
         o.expectedAccuracy && strcmp(o.expectedAccuracy, "chunks") != 0 && strcmp(o.expectedAccuracy, "contigs") != 0 ? "can be chunks or contigs" : needsMinLen, kNoGpuRule},
        {"--expectedAccuracy", o.expectedAccuracy != nullptr, o.viterbi ? "cannot be combined with --viterbi" : nullptr, kOneGpuNoLoopback},
        {"--expectedGains", o.expectedGainsPath != nullptr, o.expectedAccuracy ? nullptr : "needs --expectedAccuracy", kNoGpuRule},
        {"--lengthConstrainedEM", o.lengthConstrainedEM, needsMinLen, kNoGpuRule},
        {"--lengthConstrainedEM", o.lengthConstrainedEM, o.acceleration ? "cannot be combined with --accelerate (SQUAREM under the constraint is not built)" : nullptr, kNoGpuRule},
        {"--lengthConstrainedEM", o.lengthConstrainedEM, o.fitAlpha ? "cannot be combined with --fitAlpha (the alpha statistics come from the plain pass)" : nullptr, kNoGpuRule},
        {"--lengthConstrainedEM", o.lengthConstrainedEM, o.modelType != HF_MODEL_NEGATIVE_BINOMIAL ? nullptr :
                                   "needs --modelType gaussian or trunc_exp_gaussian (the negative_binomial statistics are another path)", kOneGpuNoLoopback},
        {"--crossChunkEM", o.crossChunkEM, o.lengthConstrainedEM ? nullptr : "needs --lengthConstrainedEM", kNoGpuRule},
        {"--runLengths", o.runLengthsSet, o.runLengths < 1 || o.runLengths > HF_RUN_LENGTHS_MAX ? "should be a number of windows between 1 and 64" : nullptr, kOneGpuNoLoopback},
        {"--totalsDistribution", o.totalsDistributionSet, o.totalsDistribution < 1 || o.totalsDistribution > HF_COUNT_DIST_MAX ? "should be a number of windows between 1 and 62" :
                                  o.regionProbsPath ? nullptr : "needs --regionProbs", kOneGpuNoLoopback},
    };
    // (every line of the region file is checked here)
    if (!check_rows(o, beforeRegions) || (o.regionProbsPath && !read_regions(o.regionProbsPath, s.regions)) || !check_rows(o, afterRegions)) return false;
    if (o.expectedGainsPath && !read_gains_tsv(o.expectedGainsPath, s.gains)) {
        fprintf(stderr, "[%s] Error: --expectedGains: %s is not a file of 4x4 tab-separated finite numbers.\n", ts(), o.expectedGainsPath);
        return false;
    }
    if (!o.inputPath) { fprintf(stderr, "[%s] Error: Input path cannot be NULL.\n", ts()); return false; }
    if (o.convergenceTol <= 0.0 || o.convergenceTol > 1.0) { fprintf(stderr, "[%s] Error: convergence tol = %2.f should be between 0 and 1.\n", ts(), o.convergenceTol); return false; }
    if (!o.outputDir) { fprintf(stderr, "[%s] Error: --outputDir, -o should be specified.\n", ts()); return false; }
    if (!dir_exists(o.outputDir)) { fprintf(stderr, "[%s] Error: Output directory %s does not exist!\n", ts(), o.outputDir); return false; }

    // presets: hmm_flagger.c:17-58, 536-575, 945-956.  The preset alpha arrays are declared `int`, so every
    // preset alpha is 0: alpha is non-zero only through --alphaTsv (:21,36,50,518-533).
    int presetW; double presetF;
    if (o.preset == "hifi") { presetW = 16000; presetF = 0.95; }
    else if (o.preset == "ont-r9") { presetW = 16000; presetF = 1.0; }
    else if (o.preset == "ont-r10") { presetW = 8000; presetF = 0.8; }
    else { fprintf(stderr, "[%s] Error: preset can be one of hifi, ont-r9, ont-r10. It cannot be %s . \n", ts(), o.preset.c_str()); return false; }
    // --sweepAlpha: the list and every TSV in it are checked before the input is read or a device is touched
    if (o.sweepListPath) {
        if (o.alphaTsvPath) { fprintf(stderr, "[%s] Error: --sweepAlpha and --alphaTsv exclude each other.\n", ts()); return false; }
        if (!read_sweep_list(o.sweepListPath, s.sweepPaths, s.sweepAlphas)) return false;
    }
    if (o.alphaTsvPath) {
        const int rc = hfm_read_alpha_tsv(o.alphaTsvPath, s.alpha);
        if (rc == -2) { fprintf(stderr, "[%s] Error: There is at least one alpha value in '%s' not between 0 and 1. \n", ts(), o.alphaTsvPath); return false; }
        if (rc != 0) { fprintf(stderr, "[%s] Error: cannot read %s\n", ts(), o.alphaTsvPath); return false; }
    }
    if (o.minReadFractionAtEnds < 0.0 && o.adjustContigEnds) o.minReadFractionAtEnds = presetF;
    if (o.windowLen < 0) o.windowLen = presetW;
    if (o.modelType == -1) o.modelType = HF_MODEL_TRUNC_EXP_GAUSSIAN;
    if (o.adjustContigEnds && (o.minReadFractionAtEnds > 1.0 || o.minReadFractionAtEnds < 0.0)) { fprintf(stderr, "[%s] Error: --minReadFractionAtEnds, -f should be between 0 and 1.\n", ts()); return false; }
    if (o.modelType == -2) { fprintf(stderr, "[%s] Error: Model type is not defined. Specify the model type with --model (-m) argument.\n", ts()); return false; }
    if (o.windowLen <= 0) { fprintf(stderr, "[%s] Error: windowLen cannot be <= 0.\n", ts()); return false; }
    // (a bin input carries its own window length: load_input checks the lengths again once it is read)
    if (uses_min_len_windows(o) && !min_len_windows(s, o.windowLen)) return false;
    if (0.5 < o.initialRandomDeviation) { fprintf(stderr, "[%s] Error: Initial random deviation for the model parameters cannot be greater than 0.5. \n", ts()); return false; }
    return true;
}

// 1. windows; the HIP runtime and the device context come up on a second thread while the input is read
// 2. number of collapsed components (hmm_flagger.c:1008-1022)
static bool load_input(Run& s) {
    Options& o = s.opt;
    fprintf(stderr, "[%s] Parsing/Creating coverage chunks. \n", ts());
    std::thread warm([device = o.device, warmPasses = o.warmPasses] { (void) (warmPasses ? hfm_warmup_pipeline(device) : hf_warmup(device)); });
    s.tab = hfio_load(o.inputPath, o.chunkLen, o.windowLen);
    warm.join();
    if (!s.tab) { fprintf(stderr, "[%s] %s\n", ts(), hfio_last_error()); return false; }
    hfio_table* tab = s.tab;
    if (o.contigListPath) {                                      // hmm_flagger.c:915-921, 93-99
        int nNames = 0;
        char** names = hfio_read_name_list(o.contigListPath, &nNames);
        if (!names) { fprintf(stderr, "[%s] %s\n", ts(), hfio_last_error()); return false; }
        fprintf(stderr, "[%s] Including only the chunks whose contigs match the given contig list.\n", ts());
        hfio_subset_contigs(tab, names, nNames);
        for (int i = 0; i < nNames; i++) free(names[i]);
        free(names);
    }
    if (o.dumpBin) {
        char binPath[2200];
        snprintf(binPath, sizeof binPath, "%s/chunks.c_%d.w_%d.bin", o.outputDir, hfio_chunk_len(tab), hfio_window_len(tab));
        fprintf(stderr, "[%s] Writing bin file into %s . \n", ts(), binPath);
        if (hfio_write_bin(tab, binPath) != 0) { fprintf(stderr, "[%s] Error: cannot write %s\n", ts(), binPath); return false; }
    }
    hfio_windows(tab, &s.w);
    s.N = hfio_n_windows(tab);
    s.nChunks = hfio_n_chunks(tab);
    fprintf(stderr, "[%s] %d chunks are parsed (%ld windows of %d bases). \n", ts(), s.nChunks, (long) s.N, hfio_window_len(tab));
    if (s.N == 0 || s.nChunks == 0) { fprintf(stderr, "[%s] Error: no windows in the input.\n", ts()); return false; }

    if (uses_min_len_windows(o) && hfio_window_len(tab) != o.windowLen && !min_len_windows(s, hfio_window_len(tab))) return false;
    s.phase("load input (+ HIP start-up)");
    if (o.numberOfCollapsedComps == -1) {
        o.numberOfCollapsedComps = hfm_best_collapsed_comps(s.w.cov, s.N, hfio_region_coverages(tab), hfio_n_regions(tab));
        if (o.numberOfCollapsedComps < 0) { fprintf(stderr, "[%s] Error: a region coverage of 0 in the header.\n", ts()); return false; }
        fprintf(stderr, "[%s] The number of collapsed components (n=%d) is determined and adjusted automatically by taking the maximum observed coverage. \n", ts(), o.numberOfCollapsedComps);
    } else {
        fprintf(stderr, "[%s] The number of components for the 'collapsed' state is set by the program argument %d. \n", ts(), o.numberOfCollapsedComps);
    }
    return true;
}

// 3. model (createModel, hmm_flagger.c:164-237); --sweepAlpha builds every candidate's model the same way, with its own alpha
static hfm_model* make_model(const Run& s, const double* alpha16) {
    const Options& o = s.opt;
    hfio_table* tab = s.tab;
    fprintf(stderr, "[%s] Creating HMM model. \n", ts());
    hfm_model* m = hfm_create(o.modelType, o.numberOfCollapsedComps, hfio_region_coverages(tab), hfio_n_regions(tab), hfio_start_only(tab),
                              hfio_avg_alignment_len(tab), hfio_window_len(tab), alpha16, o.maxHighMapqRatio, o.minHighMapqRatio);
    if (!m) { fprintf(stderr, "[%s] Error: cannot create the model (collapsedComps must be 1..%d, regions 1..%d).\n", ts(), HF_MAXCOMP, HF_MAXREGIONS); return nullptr; }
    if (o.modelType == HF_MODEL_NEGATIVE_BINOMIAL) {       // the model's per-x tables: only up to the largest coverage present
        int maxx = 0;
        for (int64_t i = 0; i < s.w.n_windows; i++) { const int x = s.w.cov[i] & 0xff; if (x > maxx) maxx = x; }
        hfm_set_max_coverage(m, maxx);
    }
    if (o.initialRandomDeviation > 0.0) hfm_scale_initial_means(m, random_factor(o.initialRandomDeviation));   // hmm_flagger.c:213-220: same factor within one second
    return m;
}

// 4. device context: windows resident in HBM for the whole run
static bool create_context(Run& s, const hfm_model* model) {
    const Options& o = s.opt;
    hfio_table* tab = s.tab;
    hf_windows& w = s.w;
    w.adjust_contig_ends = o.adjustContigEnds ? 1 : 0; w.min_read_frac = o.adjustContigEnds ? o.minReadFractionAtEnds : 0.0;
    w.max_high_mapq_ratio = o.maxHighMapqRatio; w.min_high_mapq_ratio = o.minHighMapqRatio;
    w.min_highly_clipped_ratio = hfm_min_highly_clipped_ratio(model);
    // one GPU: one context (statistics by emission row).  --gpus N (or an explicit --exchange): the sharded list — by default with the
    // chunk-order exchange (per-chunk vectors summed in chunk-list order, the reference's own merge order hmm.c:759-763: a result that
    // is independent of N bit for bit by construction; ADVICE r04: SQUAREM amplifies last-bit differences, so the command line's default
    // must not depend on N).  --exchange ranks: every GPU sums its shard by emission row and one vector per GPU is gathered — the
    // north-star's single collective and the fast statistics kernels, equal across N up to rounding (plain EM prints the same files for
    // every N at full size, configs[2] and [4]: tests/test_multi_gpu.py); what bench.py --gpus N measures
    const bool sharded = o.nGpus > 1 || o.loopbackRanks > 0 || (o.nGpus == 1 && o.exchange >= 0);
    if (sharded) {
        const int world = o.loopbackRanks > 0 ? o.loopbackRanks : o.nGpus;
        std::vector<int> devs((size_t) world);
        for (int i = 0; i < world; i++) devs[(size_t) i] = o.loopbackRanks > 0 ? o.device : o.device + i;
        const int rc = hf_multi_create(&w, hfio_n_regions(tab), o.numberOfCollapsedComps, world, devs.data(), o.algo,
                                       o.exchange < 0 ? HF_EXCHANGE_CHUNKS : o.exchange, o.loopbackRanks > 0 ? HF_TRANSPORT_LOOPBACK : HF_TRANSPORT_RCCL, &s.multi);
        if (rc != HF_OK) { fprintf(stderr, "[%s] Error: %s\n", ts(), hf_multi_last_error()); return false; }
        for (int r = 0; r < world; r++)
            fprintf(stderr, "[%s] GPU %d: %d chunks, %ld windows\n", ts(), devs[(size_t) r], hf_multi_shard_chunks(s.multi, r), (long) hf_multi_shard_windows(s.multi, r));
        s.stats.assign((size_t) hf_multi_stats_len(s.multi), 0.0);
    } else {
        const int rc = hf_create(&w, hfio_n_regions(tab), o.numberOfCollapsedComps, o.device, o.algo, &s.ctx);
        if (rc != HF_OK) { fprintf(stderr, "[%s] Error: %s\n", ts(), hf_last_error()); return false; }
        s.stats.assign((size_t) hf_chunk_stats_len(s.ctx), 0.0);
    }
    return true;
}

// what one run reports to the --sweepAlpha summary
struct RunResult { int iterations = 0; bool converged = false; double ll = 0.0; int status = HF_OK; bool have_ll = false; };

// What a run of run_em and a candidate of the batched --sweepAlpha engine write alike (failures are said here):
// loglikelihood.tsv with its header, and a row of it
static FILE* open_loglikelihood(const std::string& dir) {
    FILE* llf = fopen((dir + "/loglikelihood.tsv").c_str(), "w+");
    if (!llf) { fprintf(stderr, "[%s] Error: cannot write into %s\n", ts(), dir.c_str()); return nullptr; }
    fprintf(llf, "#Iteration\tEffective_Iteration\tLoglikelihood\n");
    return llf;
}
static void loglikelihood_row(FILE* llf, int iter, bool accelerated, double ll) { fprintf(llf, "%d\t%d\t%.4f\n", iter - 1, accelerated ? 3 * (iter - 1) : iter - 1, ll); }
static std::string iteration_suffix(bool accelerated, int k) { return (accelerated ? "iteration_accelerated_" : "iteration_") + std::to_string(k); }
static bool write_viterbi_log_prob(const std::string& dir, double vlp) {
    const std::string vp = dir + "/viterbi_log_probability.tsv";
    FILE* vf = fopen(vp.c_str(), "w");
    if (!vf) { fprintf(stderr, "[%s] Error: %s cannot be opened.\n", ts(), vp.c_str()); return false; }
    fprintf(vf, "%.6f\n", vlp);
    fclose(vf);
    return true;
}
static bool write_final_bed(const Run& s, const int8_t* finalLabels, const std::string& dir) {
    if (hfio_write_final_bed(s.tab, finalLabels, (dir + "/final_flagger_prediction.bed").c_str(), s.opt.trackName, s.opt.minLenPerState) == 0) return true;
    fprintf(stderr, "[%s] Error: %s/final_flagger_prediction.bed cannot be opened.\n", ts(), dir.c_str());
    return false;
}
// --sweepAlpha: candidate i's directory, its model (the first candidate's is the run's) and its announcement; nullptr: failed (said)
static hfm_model* start_candidate(const Run& s, size_t i, hfm_model* first, std::string& dir) {
    dir = std::string(s.opt.outputDir) + "/alpha_" + std::to_string(i + 1);
    if (!dir_exists(dir.c_str()) && mkdir(dir.c_str(), 0777) != 0) { fprintf(stderr, "[%s] Error: cannot create %s\n", ts(), dir.c_str()); return nullptr; }
    hfm_model* m = i == 0 ? first : make_model(s, s.sweepAlphas[i].data());
    if (!m) return nullptr;
    fprintf(stderr, "[%s] --sweepAlpha: candidate %zu of %zu (%s) into %s\n", ts(), i + 1, s.sweepPaths.size(), s.sweepPaths[i].c_str(), dir.c_str());
    return m;
}
static bool has_single_gpu_context(const Run& s, const char* who, const char* tail = "") {   // who: the option(s) and the verb
    if (!s.ctx) fprintf(stderr, "[%s] Error: %s a single-GPU context%s.\n", ts(), who, tail);
    return s.ctx != nullptr;
}

// One run of run_em: what its stages hand on
struct EmRun {
    hfm_model* model;
    const std::string& dir;
    RunResult& res;
    FILE *llf = nullptr, *atf = nullptr, *lcf = nullptr;    // loglikelihood.tsv, --fitAlpha's alpha_trace.tsv, --lengthConstrainedEM's length_constrained_em.tsv
    std::vector<double> alphaStats;
    std::vector<uint8_t> crossJoined;                       // --crossChunkEM: joined_by_contig of the table (empty: the per-chunk rule)
    int iter = 1, passes = 0;
    // EM+decode time (BASELINE metric): E-steps (decode included), M-steps and SQUAREM's algebra; writing the
    // log-likelihood, parameter and summary files and the log lines is output and not counted (it is still part of `emWall`)
    double emStart = 0.0, emTime = 0.0, emWall = 0.0;
    std::vector<double> passMs;                             // HF_CLI_TIMING: every E-step of the loop
    std::vector<int8_t> labels, vlabels;                    // of the final pass; of --viterbi or --expectedAccuracy
    const int8_t* finalLabels = nullptr;                    // the one of the two that the final BED and tables take
    int die(int r) { res.status = r; return die_estep(r); }
};
static int timed_full_pass(Run& s, EmRun& em) {
    const double t0 = real_time();
    const int r = s.estep(em.model, HF_MODE_FULL, s.stats.data());
    const double dt = real_time() - t0;
    em.emTime += dt; em.passes++;
    if (s.opt.phaseTiming) em.passMs.push_back(dt * 1e3);
    return r;
}

// --lengthConstrainedEM: the E-step under --minimumLengths in the place of a full pass, and its row of length_constrained_em.tsv
static int timed_minlen_pass(Run& s, EmRun& em) {
    const double t0 = real_time();
    double logZ = 0.0;
    const int r = s.estep_minlen(em.model, s.minLenWindows, em.crossJoined.empty() ? nullptr : em.crossJoined.data(), s.stats.data(), &logZ);
    const double dt = real_time() - t0;
    em.emTime += dt; em.passes++;
    if (s.opt.phaseTiming) em.passMs.push_back(dt * 1e3);
    if (r == HF_OK) fprintf(em.lcf, "%d\t%.4f\t%.4f\t%.4f\n", em.iter - 1, s.stats[0], logZ, s.stats[0] - logZ);
    return r;
}

// 5a. the EM loop (runHMMFlagger, hmm_flagger.c:285-488), with --accelerate and the --fitAlpha trace
static int em_loop(Run& s, EmRun& em) {
    const Options& o = s.opt;
    const std::string& dir = em.dir;
    const char* const accelerated = o.acceleration ? "accelerated" : "";
    int rc;
    // --fitAlpha: iterations P, 2P, ... are alpha-iterations (their pass is followed by hfm_estimate_alpha alone), the others today's; the
    // run has converged when the latest iteration of each kind reported convergence
    bool converged = false, convergedEm = false, convergedAlpha = false;
    if (o.fitAlpha) {
        if (!has_single_gpu_context(s, "--fitAlpha needs", " (no --exchange)")) return EXIT_FAILURE;
        if ((rc = hf_set_alpha_stats(s.ctx, 1)) != HF_OK) return em.die(rc);
        em.alphaStats.assign((size_t) hf_alpha_stats_len(s.ctx), 0.0);
        em.atf = fopen((dir + "/alpha_trace.tsv").c_str(), "w");
        if (!em.atf) { fprintf(stderr, "[%s] Error: cannot write into %s\n", ts(), dir.c_str()); return EXIT_FAILURE; }
        fprintf(em.atf, "#Iteration\tLoglikelihood");
        for (const char* what : {"alpha", "G", "H"})
            for (int k = 0; k < 16; k++) fprintf(em.atf, "\t%s_%d_%d", what, k / 4, k % 4);
        fprintf(em.atf, "\n");
    }
    if (o.lengthConstrainedEM) {
        if (!has_single_gpu_context(s, "--lengthConstrainedEM needs")) return EXIT_FAILURE;
        em.lcf = fopen((dir + "/length_constrained_em.tsv").c_str(), "w");
        if (!em.lcf) { fprintf(stderr, "[%s] Error: cannot write into %s\n", ts(), dir.c_str()); return EXIT_FAILURE; }
        fprintf(em.lcf, "#Iteration\tLog_Z_adm\tLog_Z\tLog_mass\n");
        if (o.crossChunkEM) em.crossJoined = joined_by_contig(chunk_list(s.tab, s.w));
        fprintf(stderr, "[%s] --lengthConstrainedEM%s: the EM iterations fit under minimum run lengths of %d,%d,%d,%d windows (Err,Dup,Hap,Col)%s\n", ts(),
                o.crossChunkEM ? " --crossChunkEM" : "", s.minLenWindows[0], s.minLenWindows[1], s.minLenWindows[2], s.minLenWindows[3],
                o.crossChunkEM ? " over the joined chunks of a contig (only runs at a contig's ends are exempt)" : "");
    }
    em.emStart = real_time();
    int& iter = em.iter;
    while (iter <= o.numberOfIterations && !converged) {
        fprintf(stderr, "[%s] [Iteration %s = %d] Running EM jobs for %d chunks (on GPU %d) ...\n", ts(), accelerated, iter, s.nChunks, o.device);
        const bool tablesDue = o.writeBenchmarkingStatsPerIteration || iter == 1;   // hmm_flagger.c:360-379
        const std::string tablesName = iter == 1 ? "initial" : iteration_suffix(o.acceleration, iter - 1);
        if (o.lengthConstrainedEM) {
            // the tables of an iteration are those of the plain pass with its parameters; the statistics are the constrained step's
            if (tablesDue && ((rc = timed_full_pass(s, em)) != HF_OK || (rc = write_summary(s, dir, tablesName, nullptr)) != HF_OK)) return em.die(rc);
            if ((rc = timed_minlen_pass(s, em)) != HF_OK) return em.die(rc);
        } else if ((rc = timed_full_pass(s, em)) != HF_OK) return em.die(rc);
        fprintf(stderr, "[%s] [Iteration %s = %d] EM jobs are all finished.\n", ts(), accelerated, iter);
        loglikelihood_row(em.llf, iter, o.acceleration, s.stats[0]);
        em.res.ll = s.stats[0]; em.res.have_ll = true;
        if (!o.lengthConstrainedEM && tablesDue && (rc = write_summary(s, dir, tablesName, nullptr)) != HF_OK) return em.die(rc);
        if (o.acceleration) {                                // hmm_flagger.c:382-416
            fprintf(stderr, "[%s] [Iteration accelerated = %d] Running SQUAREM acceleration.\n", ts(), iter);
            auto estep_cb = [&s, &em](hfm_model* m, int mode, double* st) -> int {   // (the whole accelerated iteration is timed as one block)
                const double t1 = real_time();
                const int r = s.estep(m, mode, st);
                if (s.opt.phaseTiming) em.passMs.push_back((real_time() - t1) * 1e3);
                return r;
            };
            const double t0 = real_time();
            rc = squarem_iteration(&em.model, s.stats, o.convergenceTol, estep_cb, &em.passes);
            em.emTime += real_time() - t0;
            if (rc != HF_OK) return em.die(rc);
            fprintf(stderr, "[%s] [Iteration accelerated = %d] Finished SQUAREM acceleration.\n", ts(), iter);
        }
        if (o.fitAlpha && iter % o.fitAlphaEvery == 0) {
            const double t0 = real_time();
            if ((rc = hf_get_alpha_stats(s.ctx, em.alphaStats.data())) != HF_OK) return em.die(rc);
            double a0[16], gh[32] = {0};
            hfm_get_alpha(em.model, a0);
            for (size_t r = 0; r * 32 < em.alphaStats.size(); r++)          // region order
                for (int k = 0; k < 32; k++) gh[k] += em.alphaStats[r * 32 + (size_t) k];
            const int cv = hfm_estimate_alpha(em.model, em.alphaStats.data(), s.stats.data(), o.fitAlphaMask, 0.0, o.fitAlphaMax, o.convergenceTol);
            em.emTime += real_time() - t0;
            if (cv < 0) { fprintf(stderr, "[%s] Error: hfm_estimate_alpha refused its arguments.\n", ts()); return EXIT_FAILURE; }
            convergedAlpha = cv != 0;
            converged = convergedEm && convergedAlpha;
            fprintf(em.atf, "%d\t%.17g", iter - 1, s.stats[0]);
            for (int k = 0; k < 16; k++) fprintf(em.atf, "\t%.17g", a0[k]);
            for (int k = 0; k < 32; k++) fprintf(em.atf, "\t%.17g", gh[k]);
            fprintf(em.atf, "\n");
        } else {
            const double t0 = real_time();
            converged = hfm_estimate(em.model, s.stats.data(), o.convergenceTol) != 0;
            em.emTime += real_time() - t0;
            if (o.fitAlpha) { convergedEm = converged; converged = convergedEm && convergedAlpha; }
        }
        fprintf(stderr, "[%s] [Iteration %s = %d] Parameters are estimated and updated.\n", ts(), accelerated, iter);
        if (o.writeParamsPerIter) write_params(em.model, dir, iteration_suffix(o.acceleration, iter));
        iter += 1;
    }
    if (converged) fprintf(stderr, "[%s] Parameters converged after %d iterations (tol=%.2e)\n", ts(), iter - 1, o.convergenceTol);
    else fprintf(stderr, "[%s] Parameter estimation stopped (not yet converged based on the given tolerance) after %d iterations (tol=%.2e)\n", ts(), iter - 1, o.convergenceTol);
    em.res.iterations = iter - 1; em.res.converged = converged;
    return 0;
}

// --wholeContigs: the maximal runs of `labels`, merged over every group of joined chunks (group_end, hf_cli_scopes.h), that touch neither
// end of their group and have fewer than min_len windows of their label
static long long short_inner_runs(const ChunkList& list, const std::vector<uint8_t>& joined, const int8_t* labels, const int32_t min_len[4]) {
    long long count = 0;
    for (int c0 = 0; c0 < list.C;) {
        const int c1 = group_end(list, joined.data(), c0);
        const int64_t t0 = list.off[c0], t1 = list.off[c1];
        for (int64_t a = t0; a < t1;) {
            int64_t b = a;
            while (b + 1 < t1 && labels[b + 1] == labels[a]) b++;
            if (a > t0 && b < t1 - 1 && labels[a] >= 0 && labels[a] < 4 && b - a + 1 < min_len[labels[a]]) count++;
            a = b + 1;
        }
        c0 = c1;
    }
    return count;
}

// --expectedAccuracy chunks|contigs: the labelling of the largest expected gain under --minimumLengths (hf_get_mea_labels) into
// `decoded`, and expected_accuracy.tsv: per contig (the scopes of hf_cli_scopes.h behind "all") and for the track (the sum of the contig rows, in
// row order) the windows, the unconstrained bound sum_t max_k g_t(k), the gain of the labels the final BED would carry without the
// option (`argmax`, the labels of the final pass, with every run, merged over the joined chunks of a contig, shorter than its length in
// windows turned to Hap), the gain decoded, and whether the final BED's own labelling is supported: every chunk's part of it has
// positive probability (hf_get_path_log_probs).  g_t(k) on the host: hf_get_posterior's gamma and the getter's order of additions.
static int expected_accuracy(Run& s, const int8_t* argmax, std::vector<int8_t>& decoded, const std::string& dir) {
    const Options& o = s.opt;
    const int64_t N = s.N;
    const int C = s.w.n_chunks;
    const int64_t* const off = s.w.chunk_off;
    const int32_t* const mw = s.minLenWindows;
    const double* const W = s.gains;
    const ChunkList list = chunk_list(s.tab, s.w);
    const std::vector<uint8_t> joined = joined_by_contig(list);
    decoded.assign((size_t) N, -1);
    std::vector<double> block((size_t) C, 0.0), post((size_t) N * 4);
    double total = 0.0;
    int rc = hf_get_mea_labels(s.ctx, o.expectedGainsPath ? W : nullptr, mw, strcmp(o.expectedAccuracy, "contigs") == 0 ? joined.data() : nullptr,
                               decoded.data(), block.data(), &total);
    if (rc != HF_OK) return rc;
    if ((rc = s.posterior(0, N, post.data())) != HF_OK) return rc;
    // the final BED's own rule, in windows
    std::vector<int8_t> rule(argmax, argmax + N);
    for (int c0 = 0; c0 < C;) {
        const int c1 = group_end(list, joined.data(), c0);
        for (int64_t a = off[c0]; a < off[c1];) {
            int64_t b = a;
            while (b + 1 < off[c1] && argmax[b + 1] == argmax[a]) b++;
            if (argmax[a] >= 0 && argmax[a] < 4 && b - a + 1 < mw[argmax[a]])
                for (int64_t t = a; t <= b; t++) rule[(size_t) t] = 2;
            a = b + 1;
        }
        c0 = c1;
    }
    Jobs jobs;
    std::vector<int> jobChunk;
    for (int c = 0; c < C; c++)
        if (off[c + 1] > off[c]) { jobs.add(off[c], off[c + 1]); jobChunk.push_back(c); }
    std::vector<double> lp((size_t) jobs.n());
    if ((rc = hf_get_path_log_probs(s.ctx, jobs.n(), jobs.first.data(), jobs.last.data(), rule.data(), lp.data())) != HF_OK) return rc;
    std::vector<char> chunkSupported((size_t) C, 1);
    for (size_t j = 0; j < lp.size(); j++) chunkSupported[(size_t) jobChunk[j]] = lp[j] > -HUGE_VAL;
    struct Row { std::string scope; long long windows = 0; double argmaxGain = 0.0, ruleGain = 0.0, decodedGain = 0.0; bool supported = true; };
    const Scopes sc = contig_scopes(list);
    std::vector<Row> rows(sc.scopes.size() - 1);               // the contigs; the track's row comes last here
    for (size_t i = 0; i < rows.size(); i++) rows[i].scope = sc.scopes[i + 1].name;
    for (int c = 0; c < C; c++) {
        Row& r = rows[sc.scope_of_chunk[(size_t) c] - 1];
        r.windows += off[c + 1] - off[c];
        r.decodedGain += block[(size_t) c];
        r.supported = r.supported && chunkSupported[(size_t) c];
        for (int64_t t = off[c]; t < off[c + 1]; t++) {
            const double* g = &post[(size_t) t * 4];
            double best = -HUGE_VAL;
            for (int k = 0; k < 4; k++) {
                const double gk = ((g[0] * W[k] + g[1] * W[4 + k]) + g[2] * W[8 + k]) + g[3] * W[12 + k];
                if (gk > best) best = gk;
                if (k == rule[(size_t) t]) r.ruleGain += gk;
            }
            r.argmaxGain += best;
        }
    }
    Row track;
    track.scope = "track";
    for (const Row& r : rows) {
        track.windows += r.windows; track.argmaxGain += r.argmaxGain; track.ruleGain += r.ruleGain; track.decodedGain += r.decodedGain;
        track.supported = track.supported && r.supported;
    }
    rows.push_back(track);
    TableFile f;
    if ((rc = f.open(dir + "/expected_accuracy.tsv")) != HF_OK) return rc;
    fprintf(f, "#scope\twindows\tgain_argmax\tgain_final_bed_rule\tgain_decoded\tfinal_bed_rule_supported\n");
    for (const Row& r : rows)
        fprintf(f, "%s\t%lld\t%.17g\t%.17g\t%.17g\t%d\n", r.scope.c_str(), r.windows, r.argmaxGain, r.ruleGain, r.decodedGain, r.supported ? 1 : 0);
    if ((rc = f.close()) != HF_OK) return rc;
    fprintf(stderr, "[%s] [Final Inference] Minimum run lengths %d,%d,%d,%d windows (%s): expected gain %.6f (unconstrained bound %.6f, the final BED's own rule %.6f)\n",
            ts(), mw[0], mw[1], mw[2], mw[3], o.expectedAccuracy, track.decodedGain, track.argmaxGain, track.ruleGain);
    return HF_OK;
}

// 5b. the final inference: the last pass, its labels, --expectedAccuracy with its table, --viterbi and --enforceMinimumLengths with the cost file
static int final_inference(Run& s, EmRun& em) {
    const Options& o = s.opt;
    const std::string& dir = em.dir;
    const int64_t N = s.N;
    int rc;
    fprintf(stderr, "[%s] [Final Inference] Running EM jobs for %d chunks (on GPU %d) ...\n", ts(), s.nChunks, o.device);
    if ((rc = timed_full_pass(s, em)) != HF_OK) return em.die(rc);
    em.emWall = real_time() - em.emStart;
    fprintf(stderr, "[%s] [Final Inference] EM jobs are all finished.\n", ts());
    loglikelihood_row(em.llf, em.iter, o.acceleration, s.stats[0]);
    em.res.ll = s.stats[0]; em.res.have_ll = true;
    fclose(em.llf);
    em.llf = nullptr;
    if (em.lcf) { fclose(em.lcf); em.lcf = nullptr; }
    write_params(em.model, dir, "final");
    if (o.fitAlpha) {        // four tab-separated rows that --alphaTsv reads back to the same doubles
        double a[16];
        hfm_get_alpha(em.model, a);
        FILE* af = fopen((dir + "/alpha_fitted.tsv").c_str(), "w");
        if (!af) { fprintf(stderr, "[%s] Error: cannot write into %s\n", ts(), dir.c_str()); return EXIT_FAILURE; }
        for (int i = 0; i < 4; i++) fprintf(af, "%.17g\t%.17g\t%.17g\t%.17g\n", a[i * 4], a[i * 4 + 1], a[i * 4 + 2], a[i * 4 + 3]);
        fclose(af);
        (void) hf_set_alpha_stats(s.ctx, 0);
    }
    em.labels.resize((size_t) N);
    if ((rc = s.labels(em.labels.data())) != HF_OK) return em.die(rc);
    em.finalLabels = em.labels.data();
    // --expectedAccuracy: the final BED and the final tables take the labelling of the largest expected gain under --minimumLengths
    if (o.expectedAccuracy) {
        if (!has_single_gpu_context(s, "--expectedAccuracy needs")) return EXIT_FAILURE;
        fprintf(stderr, "[%s] [Final Inference] Maximum expected accuracy under the minimum run lengths (%s) ...\n", ts(), o.expectedAccuracy);
        if ((rc = expected_accuracy(s, em.labels.data(), em.vlabels, dir)) != HF_OK) return em.die(rc);
        em.finalLabels = em.vlabels.data();
        return 0;
    }
    // --viterbi: the final BED and the final tables take the most probable path under the final parameters; everything else
    // (the posterior BED of -P among it) keeps the posterior labels of the final pass
    if (!o.viterbi) return 0;
    std::vector<int8_t>& vlabels = em.vlabels;
    fprintf(stderr, "[%s] [Final Inference] Most probable state path of %d chunks ...\n", ts(), s.nChunks);
    vlabels.resize((size_t) N);
    double vlp = 0.0;
    if ((rc = s.viterbi(em.model, vlabels.data(), &vlp)) != HF_OK) return em.die(rc);
    // --enforceMinimumLengths: the path written is the best one that respects the lengths; the unconstrained run above is what it cost
    if (o.enforceMinLen) {
        if (!has_single_gpu_context(s, "--enforceMinimumLengths needs")) return EXIT_FAILURE;
        const int32_t* const mw = s.minLenWindows;
        std::vector<int8_t> clabels((size_t) N);
        double clp = 0.0;
        if ((rc = s.viterbi_minlen(em.model, mw, clabels.data(), &clp)) != HF_OK) return em.die(rc);
        // --wholeContigs: the rule over the joined chunks of a contig; the per-chunk run above is what the whole-contig rule is compared with
        double pclp = 0.0;
        long long shortRuns = 0;
        if (o.wholeContigs) {
            const ChunkList list = chunk_list(s.tab, s.w);
            const std::vector<uint8_t> joined = joined_by_contig(list);
            pclp = clp;
            shortRuns = short_inner_runs(list, joined, clabels.data(), mw);
            if ((rc = s.viterbi_minlen_joined(em.model, mw, joined.data(), clabels.data(), &clp)) != HF_OK) return em.die(rc);
        }
        int differ = 0;
        for (int c = 0; c < s.w.n_chunks; c++)
            differ += memcmp(clabels.data() + s.w.chunk_off[c], vlabels.data() + s.w.chunk_off[c], (size_t) (s.w.chunk_off[c + 1] - s.w.chunk_off[c])) != 0;
        const std::string cp = dir + "/viterbi_min_length_cost.tsv";
        FILE* cf = fopen(cp.c_str(), "w");
        if (!cf) { fprintf(stderr, "[%s] Error: %s cannot be opened.\n", ts(), cp.c_str()); return EXIT_FAILURE; }
        fprintf(cf, "#min_windows_Err\tmin_windows_Dup\tmin_windows_Hap\tmin_windows_Col\tlog_prob_constrained\tlog_prob_unconstrained\tlog_prob_difference\tchunks_changed%s\n",
                o.wholeContigs ? "\tlog_prob_constrained_per_chunk\tshort_runs_per_chunk_rule" : "");
        fprintf(cf, "%d\t%d\t%d\t%d\t%.6f\t%.6f\t%.6f\t%d", mw[0], mw[1], mw[2], mw[3], clp, vlp, clp - vlp, differ);
        if (o.wholeContigs) fprintf(cf, "\t%.6f\t%lld", pclp, shortRuns);
        fprintf(cf, "\n");
        fclose(cf);
        fprintf(stderr, "[%s] [Final Inference] Minimum run lengths %d,%d,%d,%d windows: log-probability %.6f (unconstrained %.6f), %d chunks changed\n",
                ts(), mw[0], mw[1], mw[2], mw[3], clp, vlp, differ);
        vlabels.swap(clabels);
        vlp = clp;
    }
    if (!write_viterbi_log_prob(dir, vlp)) return EXIT_FAILURE;
    fprintf(stderr, "[%s] [Final Inference] Most probable path: log-probability %.6f\n", ts(), vlp);
    em.finalLabels = vlabels.data();
    return 0;
}

// 5c.-6. the final outputs: the final tables (on their worker), the posterior BED of -P, the final BED
static int final_outputs(Run& s, EmRun& em) {
    const std::string& dir = em.dir;
    int rc;
    if ((rc = write_summary(s, dir, "final", em.finalLabels)) != HF_OK) return em.die(rc);
    memcpy(hfio_prediction(s.tab), em.labels.data(), (size_t) s.N);
    if (s.opt.writePosterior) {
        std::vector<double> post((size_t) s.N * 4);
        if ((rc = s.posterior(0, s.N, post.data())) != HF_OK) return em.die(rc);
        const std::string pp = dir + "/posterior_prediction_final.bed";
        fprintf(stderr, "[%s] Writing posterior bed : %s\n", ts(), pp.c_str());
        hfio_write_posterior_bed(s.tab, post.data(), em.labels.data(), pp.c_str());
    }
    if (s.opt.phaseTiming && !em.passMs.empty()) {
        fprintf(stderr, "[phase]   E-step passes (ms):");
        for (size_t k = 0; k < em.passMs.size(); k++) fprintf(stderr, " %.3f", em.passMs[k]);
        fprintf(stderr, "\n");
    }
    s.phase("EM + final inference");
    fprintf(stderr, "[%s] Writing final BED file. \n", ts());
    return write_final_bed(s, em.finalLabels, dir) ? 0 : EXIT_FAILURE;
}

// the samplers of --uncertaintySamples and --admissibleSamples (paths drawn UNDER --minimumLengths) behind write_sample_outputs
static PathSampler posterior_sampler(hf_ctx* ctx, uint64_t seed) {
    return PathSampler{[ctx] { return hf_sample_capacity(ctx); },
                       [ctx, seed](const hf_params* p, int64_t first, int n) {
                           const int rc = hf_sample_paths(ctx, p, first, n, seed, nullptr);
                           return rc == HF_OK ? hf_sample_finish(ctx, nullptr) : rc;
                       },
                       [ctx](int k, int8_t* out) { return hf_get_sample_labels(ctx, k, out); }};
}
// (joined: null for the per-chunk rule, else the rule over the groups of joined chunks, --mergedChunks)
static PathSampler admissible_sampler(hf_ctx* ctx, const int32_t* ml, const uint8_t* joined, uint64_t seed) {
    return PathSampler{[ctx, ml] { return hf_minlen_sample_capacity(ctx, ml); },
                       [ctx, ml, joined, seed](const hf_params* p, int64_t first, int n) {
                           const int rc = joined ? hf_sample_paths_minlen_joined(ctx, p, ml, joined, first, n, seed, nullptr)
                                                 : hf_sample_paths_minlen(ctx, p, ml, first, n, seed, nullptr);
                           return rc == HF_OK ? hf_sample_minlen_finish(ctx, nullptr) : rc;
                       },
                       [ctx](int k, int8_t* out) { return hf_get_minlen_sample_labels(ctx, k, out); }};
}
// 6b. The outputs behind the final BED: after every other output of the run (which does not depend on them), in the order of the table.
// A row: whether the options ask for it, who needs the single-GPU context (the option(s) with the verb), what is reported when it is
// done (nullptr: the call reports itself), and the call (an HF_* code).
static int late_outputs(Run& s, EmRun& em) {
    const Options& o = s.opt;
    hf_ctx* const ctx = s.ctx;
    const int32_t* const mw = s.minLenWindows;
    std::unique_ptr<Report> rep;      // what the writers share: built for the first output that is wanted
    // --mergedChunks: --constrainedPosterior and --admissibleSamples apply the lengths over the joined chunks of a contig
    auto merged = [&] { return o.mergedChunks ? rep->joined.data() : nullptr; };
    double t0 = 0.0;
    struct LateOutput { bool wanted; const char *who, *done; std::function<int()> write; };
    const LateOutput outputs[] = {
        {o.uncertaintySamples > 0, "--uncertaintySamples needs", "posterior_samples_summary.tsv and final_label_runs_support.bed are written", [&] {
             fprintf(stderr, "[%s] [Final Inference] Drawing %d posterior state paths (seed %llu) ...\n", ts(), o.uncertaintySamples, (unsigned long long) o.uncertaintySeed);
             return write_sample_outputs(*rep, posterior_sampler(ctx, o.uncertaintySeed), em.model, o.uncertaintySamples, "posterior_samples_summary.tsv",
                                         "final_label_runs_support.bed");
         }},
        {o.runConfidence || o.regionProbsPath, "--runConfidence and --regionProbs need", "exact interval probabilities written",
         [&] { return write_interval_outputs(*rep, o.runConfidence); }},
        {o.runBoundaries, "--runBoundaries needs", "final_label_run_boundaries.tsv is written", [&] { return write_run_boundaries(*rep); }},
        {o.exactTotals, "--exactTotals needs", "label_totals_exact.tsv is written", [&] { return write_exact_totals(*rep); }},
        {o.numBlocks, "--numBlocks needs", "label_blocks_exact.tsv is written", [&] { return write_exact_blocks(*rep); }},
        {o.runLengthsSet, "--runLengths needs", o.minLenGiven ? "label_block_lengths_exact.tsv and label_blocks_kept_exact.tsv are written" : "label_block_lengths_exact.tsv is written",
         [&] { return write_block_lengths(*rep, o.runLengths, o.minLenGiven ? mw : nullptr); }},
        {o.jointEntropy, "--jointEntropy needs", "path_uncertainty.tsv is written", [&] { return write_path_uncertainty(*rep); }},
        {o.keptBlocks, "--keptBlocks needs", "kept_block_probabilities.tsv is written", [&] { return write_kept_blocks(*rep); }},
        // (a decoder of its own: it reads the final parameters, not the last pass; its line carries the mass it found)
        {o.constrainedPost, "--constrainedPosterior needs", nullptr, [&] {
             const uint8_t* const joined = merged();
             double logMass = 0.0, perChunkMass = 0.0;
             // --mergedChunks: one run under the per-chunk rule first, for the column the whole-contig masses are compared with
             std::vector<double> perChunk;
             int rc = HF_OK;
             if (joined) {
                 perChunk.resize((size_t) std::max(rep->C, 1));
                 rc = s.minlen_posterior(em.model, mw, nullptr, &perChunkMass);
                 if (rc == HF_OK) rc = hf_get_minlen_chunk_log_mass(ctx, perChunk.data(), nullptr);
             }
             if (rc == HF_OK) rc = s.minlen_posterior(em.model, mw, joined, &logMass);
             if (rc == HF_OK) rc = write_constrained_posterior(*rep, joined ? &perChunk : nullptr);
             if (rc == HF_OK && joined)
                 fprintf(stderr, "[%s] [Final Inference] Minimum run lengths %d,%d,%d,%d windows over merged chunks keep posterior mass exp(%.6f) (per chunk: exp(%.6f)); admissible_mass.tsv and posterior_prediction_min_lengths.bed are written (%.1f ms).\n",
                         ts(), mw[0], mw[1], mw[2], mw[3], logMass, perChunkMass, (real_time() - t0) * 1e3);
             else if (rc == HF_OK) fprintf(stderr, "[%s] [Final Inference] Minimum run lengths %d,%d,%d,%d windows keep posterior mass exp(%.6f); admissible_mass.tsv and posterior_prediction_min_lengths.bed are written (%.1f ms).\n",
                                      ts(), mw[0], mw[1], mw[2], mw[3], logMass, (real_time() - t0) * 1e3);
             return rc;
         }},
        {o.admissibleSamples > 0, "--admissibleSamples needs", "admissible_samples_summary.tsv and admissible_label_runs_support.bed are written", [&] {
             fprintf(stderr, "[%s] [Final Inference] Drawing %d admissible state paths (minimum run lengths %d,%d,%d,%d windows%s, seed %llu) ...\n", ts(),
                     o.admissibleSamples, mw[0], mw[1], mw[2], mw[3], merged() ? " over merged chunks" : "", (unsigned long long) o.uncertaintySeed);
             return write_sample_outputs(*rep, admissible_sampler(ctx, mw, merged(), o.uncertaintySeed), em.model, o.admissibleSamples,
                                         "admissible_samples_summary.tsv", "admissible_label_runs_support.bed");
         }},
        {o.totalsDistributionSet, "--totalsDistribution needs", "region_label_totals_exact.tsv is written", [&] { return write_region_totals(*rep, o.totalsDistribution); }},
    };
    for (const LateOutput& out : outputs) {
        if (!out.wanted) continue;
        if (!has_single_gpu_context(s, out.who)) return EXIT_FAILURE;
        t0 = real_time();
        if (!rep) rep.reset(new Report(s, em.finalLabels, em.dir));
        const int rc = out.write();
        if (rc != HF_OK) return em.die(rc);
        if (out.done) fprintf(stderr, "[%s] [Final Inference] %s (%.1f ms).\n", ts(), out.done, (real_time() - t0) * 1e3);
    }
    return 0;
}

// 5.-6. one whole run with `model` into `dir`: EM, final inference, every output file (runHMMFlagger, hmm_flagger.c:285-488).
// 0, or the exit status of a run that failed (said; res.status holds the HF_* code of a failed device call)
static int run_em(Run& s, hfm_model* model, const std::string& dir, RunResult& res) {
    fprintf(stderr, "[%s] Running EM for estimating parameters. \n", ts());
    EmRun em{model, dir, res};
    if (!(em.llf = open_loglikelihood(dir))) return EXIT_FAILURE;
    FileCloser llfClose{em.llf}, atfClose{em.atf}, lcfClose{em.lcf};
    write_params(model, dir, "initial");
    for (int (*stage)(Run&, EmRun&) : {em_loop, final_inference, final_outputs, late_outputs}) {
        const int r = stage(s, em);
        if (r != 0) return r;
    }
    fprintf(stderr, "[%s] EM+decode: %d passes over %ld windows in %.4f s = %.3e windows/s on GPU %d (E-steps, M-steps; the loop with its "
            "log lines and output files took %.4f s)\n", ts(), em.passes, (long) s.N, em.emTime, (double) s.N * em.passes / em.emTime, s.opt.device, em.emWall);
    s.phase("final BED");
    if (!s.opt.sweepListPath) summary_join();      // the table workers (the reference writes the tables before the BED; the files are the same)
    else if (!summary_join_report()) return EXIT_FAILURE;
    s.phase("summary tables joined");
    return 0;
}

// --sweepAlpha, the BATCHED engine (hf_batch_*, flagger_amd/csrc/hf_batch.h): every pass runs all unconverged candidates of a group of at
// most `cap` together; a candidate leaves the active set after its final inference pass, so its iterations and files are those of a
// separate --alphaTsv run.  A candidate that fails is reported in results and the sweep goes on (anyFailed); false: the sweep cannot (said)
static bool sweep_batched(Run& s, hfm_model* model, int cap, std::vector<RunResult>& results, bool& anyFailed) {
    const Options& o = s.opt;
    const size_t n = s.sweepPaths.size();
    const int64_t N = s.N;
    const int G = (int) std::min<size_t>((size_t) cap, n);
    fprintf(stderr, "[%s] --sweepAlpha: %zu candidates on one loaded input, engine: batched (hf_batch), %d models per group\n", ts(), n, G);
    const int64_t V = hf_chunk_stats_len(s.ctx);
    struct Cand { hfm_model* m = nullptr; FILE* llf = nullptr; int iter = 1; bool converged = false, final = false, done = false; std::string dir; };
    for (size_t g0 = 0; g0 < n; g0 += (size_t) G) {
        const int ng = (int) std::min<size_t>((size_t) G, n - g0);
        hf_batch* bt = nullptr;
        if (hf_batch_create(s.ctx, ng, &bt) != HF_OK) { fprintf(stderr, "[%s] Error: %s\n", ts(), hf_last_error()); return false; }
        std::vector<Cand> cs((size_t) ng);
        for (int j = 0; j < ng; j++) {
            Cand& c = cs[(size_t) j];
            if (!(c.m = start_candidate(s, g0 + (size_t) j, model, c.dir))) return false;
            if (!(c.llf = open_loglikelihood(c.dir))) return false;
            write_params(c.m, c.dir, "initial");
            c.final = o.numberOfIterations < 1;
        }
        std::vector<int8_t> lab((size_t) N);
        while (true) {
            std::vector<int32_t> act;
            std::vector<hf_params> ps;
            for (int j = 0; j < ng; j++) if (!cs[(size_t) j].done) { act.push_back(j); ps.emplace_back(); hfm_params(cs[(size_t) j].m, &ps.back()); }
            if (act.empty()) break;
            std::vector<double> stats(act.size() * (size_t) V);
            std::vector<int32_t> status(act.size(), HF_OK);
            int rc = hf_batch_estep(bt, ps.data(), act.data(), (int) act.size(), HF_MODE_FULL, nullptr);
            if (rc == HF_OK) rc = hf_batch_finish(bt, stats.data(), status.data(), nullptr);
            if (rc != HF_OK) { die_estep(rc); return false; }
            for (size_t k = 0; k < act.size(); k++) {
                const int j = act[k];
                Cand& c = cs[(size_t) j];
                RunResult& res = results[g0 + (size_t) j];
                const double* st = stats.data() + k * (size_t) V;
                auto fail = [&](int r) {
                    if (r == HF_E_SCALE) fprintf(stderr, "scale is very low!\n");
                    else if (r == HF_E_NAN) fprintf(stderr, "[Error] prob is NAN\n");
                    else fprintf(stderr, "[%s] Error: %s\n", ts(), cli_error_or(hf_last_error()));
                    g_cli_error.clear();
                    res.status = r == HF_OK ? HF_E_ARG : r; anyFailed = true; c.done = true;
                    if (c.llf) fclose(c.llf);
                    c.llf = nullptr;
                };
                if (status[k] != HF_OK) { fail(status[k]); continue; }
                loglikelihood_row(c.llf, c.iter, false, st[0]);
                res.ll = st[0]; res.have_ll = true;
                if (!c.final) {
                    if (o.writeBenchmarkingStatsPerIteration || c.iter == 1) {
                        if ((rc = hf_batch_get_labels(bt, j, lab.data())) != HF_OK ||
                            (rc = write_summary(s, c.dir, c.iter == 1 ? "initial" : iteration_suffix(false, c.iter - 1), lab.data())) != HF_OK) { fail(rc); continue; }
                    }
                    c.converged = hfm_estimate(c.m, st, o.convergenceTol) != 0;
                    if (o.writeParamsPerIter) write_params(c.m, c.dir, iteration_suffix(false, c.iter));
                    c.iter += 1;
                    if (c.iter > o.numberOfIterations || c.converged) {
                        res.iterations = c.iter - 1; res.converged = c.converged;
                        c.final = true;                          // the next pass of this candidate is its final inference
                    }
                    continue;
                }
                // the final inference pass: every output of a separate run
                res.iterations = c.iter - 1; res.converged = c.converged;
                fclose(c.llf);
                c.llf = nullptr;
                write_params(c.m, c.dir, "final");
                if ((rc = hf_batch_get_labels(bt, j, lab.data())) != HF_OK) { fail(rc); continue; }
                std::vector<int8_t> vlabels;
                if (o.viterbi) {
                    vlabels.resize((size_t) N);
                    double vlp = 0.0;
                    if ((rc = s.viterbi(c.m, vlabels.data(), &vlp)) != HF_OK) { fail(rc); continue; }
                    if (!write_viterbi_log_prob(c.dir, vlp)) { fail(HF_E_ARG); continue; }
                }
                const int8_t* finalLabels = o.viterbi ? vlabels.data() : lab.data();
                if ((rc = write_summary(s, c.dir, "final", finalLabels)) != HF_OK) { fail(rc); continue; }
                memcpy(hfio_prediction(s.tab), lab.data(), (size_t) N);
                if (o.writePosterior) {
                    std::vector<double> post((size_t) N * 4);
                    if ((rc = hf_batch_get_posterior(bt, j, 0, N, post.data())) != HF_OK) { fail(rc); continue; }
                    hfio_write_posterior_bed(s.tab, post.data(), lab.data(), (c.dir + "/posterior_prediction_final.bed").c_str());
                }
                if (!write_final_bed(s, finalLabels, c.dir)) { fail(HF_E_ARG); continue; }
                c.done = true;
            }
        }
        if (!summary_join_report()) { anyFailed = true; }
        hf_batch_destroy(bt);
    }
    return true;
}

// --sweepAlpha: the candidates one after another on the context (or GPU list) of the session, each exactly a separate run
static bool sweep_sequential(Run& s, hfm_model* model, std::vector<RunResult>& results, bool& anyFailed) {
    const size_t n = s.sweepPaths.size();
    fprintf(stderr, "[%s] --sweepAlpha: %zu candidates on one loaded input, engine: sequential (%s), 1 model per group\n", ts(), n, s.multi ? "sharded GPU list" : "one context");
    for (size_t i = 0; i < n; i++) {
        std::string cdir;
        hfm_model* m = start_candidate(s, i, model, cdir);
        if (!m) return false;
        if (run_em(s, m, cdir, results[i]) != 0) {
            anyFailed = true;
            if (results[i].status == HF_OK) results[i].status = HF_E_ARG;
            g_cli_error.clear();
            // (a failed table set of this candidate has been reported; the next candidate starts with no worker of its own pending)
            summary_wait_quietly();
            g_summaries.clear();
        }
    }
    return true;
}

// <outputDir>/alpha_sweep.tsv: one row per candidate
static bool write_sweep_table(const Run& s, const std::vector<RunResult>& results, const std::string& sp) {
    FILE* sf = fopen(sp.c_str(), "w");
    if (!sf) { fprintf(stderr, "[%s] Error: %s cannot be opened.\n", ts(), sp.c_str()); return false; }
    fprintf(sf, "#Index\tAlpha_Tsv\tIterations\tConverged\tLoglikelihood\tStatus\n");
    for (size_t i = 0; i < results.size(); i++) {
        const RunResult& r = results[i];
        const char* st = r.status == HF_OK ? "ok" : r.status == HF_E_SCALE ? "scale_too_low" : r.status == HF_E_NAN ? "nan" : "error";
        if (r.have_ll) fprintf(sf, "%zu\t%s\t%d\t%d\t%.4f\t%s\n", i + 1, s.sweepPaths[i].c_str(), r.iterations, r.converged ? 1 : 0, r.ll, st);
        else fprintf(sf, "%zu\t%s\t%d\t%d\tNA\t%s\n", i + 1, s.sweepPaths[i].c_str(), r.iterations, r.converged ? 1 : 0, st);
    }
    fclose(sf);
    return true;
}

int main(int argc, char* argv[]) {
    Run run;
    g_run = &run;
    if (!parse_options(argc, argv, run.opt)) return EXIT_FAILURE;
    read_environment(run.opt);
    run.realtimeStart = run.phaseStart = real_time();
    if (!check_options(run) || !load_input(run)) return EXIT_FAILURE;
    hfm_model* model = make_model(run, run.opt.sweepListPath ? run.sweepAlphas[0].data() : run.alpha);
    if (!model) return EXIT_FAILURE;
    run.phase("model");
    if (!create_context(run, model)) return EXIT_FAILURE;
    run.phase("hf_create");
    if (!run.opt.sweepListPath) {
        RunResult res;
        const int r = run_em(run, model, std::string(run.opt.outputDir), res);
        if (r != 0) return r;
    } else {
        std::vector<RunResult> results(run.sweepPaths.size());
        bool anyFailed = false;
        // plain EM on one context of the default algorithm, Gaussian models: the batched engine.  Everything else: the candidates one after another.
        const int cap = (!run.multi && !run.opt.acceleration && run.opt.modelType != HF_MODEL_NEGATIVE_BINOMIAL) ? hf_batch_capacity(run.ctx) : 0;
        if (!(cap > 0 ? sweep_batched(run, model, cap, results, anyFailed) : sweep_sequential(run, model, results, anyFailed))) return EXIT_FAILURE;
        const std::string sp = std::string(run.opt.outputDir) + "/alpha_sweep.tsv";
        if (!write_sweep_table(run, results, sp)) return EXIT_FAILURE;
        if (anyFailed) {
            if (run.multi) hf_multi_destroy(run.multi);
            fprintf(stderr, "[%s] Error: at least one --sweepAlpha candidate failed (%s)\n", ts(), sp.c_str());
            fflush(nullptr);
            _exit(EXIT_FAILURE);
        }
    }
    if (run.multi) hf_multi_destroy(run.multi);   // (joins the ranks' threads and communicators: RCCL wants an orderly end)
    // the one-GPU context, the model and the window table are NOT destroyed: the process ends below without unwinding anything
    // (freeing ~40 device allocations one by one was 5 ms of a 0.15 s run)
    fprintf(stderr, "[%s] Done! \n", ts());
    run.phase("outputs");
    const double realtime = real_time() - run.realtimeStart, cputime = cpu_time();
    fprintf(stderr, "Real time:  %.3f sec; CPU: %.3f sec; Peak RSS: %.3f GB; CPU usage: %.1f%%\n", realtime, cputime,
            peak_rss_gb(), (cputime + 1e-9) / (realtime + 1e-9) * 100.0);
    // every output is written and closed: leave without unwinding the HIP runtime and the device allocations (the
    // operating system reclaims them; the orderly teardown costs several tens of milliseconds of a half-second run)
    fflush(nullptr);
    _exit(0);
}
