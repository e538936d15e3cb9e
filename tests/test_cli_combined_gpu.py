"""hmm_flagger with ALL final-inference options in one run: --uncertaintySamples, --runConfidence, --regionProbs, --exactTotals, --numBlocks,
--jointEntropy, --runBoundaries and --keptBlocks (with and without --viterbi, with --viterbi --enforceMinimumLengths and with --fitAlpha)
run one after another on one context, each building lazy state on top of what the ones
before it left.  Every file an option writes must be byte-identical to the file of a run with that option alone: a getter that answered
for a decoder's parameters, for a stale lazy block or for half-built state would change a digit somewhere.  The suite otherwise runs
each option by itself."""
import os
import subprocess

import pytest

from flagger_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")

COMMON = ["final_flagger_prediction.bed", "loglikelihood.tsv"]


def _cli(args, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


def _rows(path):
    return [l.split("\t") for l in path.read_text().splitlines() if not l.startswith("#")]


MINIMUM_LENGTHS = ["--minimumLengths", "12000,20000,28000"]      # (the kept-block lengths come from it: every run carries it)


@pytest.mark.parametrize("base", [[], ["--viterbi"], ["--fitAlpha"], ["--viterbi", "--enforceMinimumLengths"]],
                         ids=["posterior", "viterbi", "fitAlpha", "viterbi-minlen"])
def test_cli_all_final_inference_options_in_one_run(tmp_path, base):
    """The input and base arguments of tests/test_interval_gpu.py::test_cli_run_confidence_and_regions.  With --fitAlpha the alpha statistics are
    switched on during EM and off before the getters run."""
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    args = ["-i", str(binp), "-W", "4000", "-n", "4", "-P"] + MINIMUM_LENGTHS + base
    # each option alone (the first run also supplies the regions: a run, a one-window region, an unknown contig, a region of two runs)
    _cli(args + ["--uncertaintySamples", "4"], tmp_path / "samples")
    runs_sup = _rows(tmp_path / "samples" / "final_label_runs_support.bed")
    w0 = _rows(tmp_path / "samples" / "posterior_prediction_final.bed")[0]
    r0 = runs_sup[len(runs_sup) // 2]
    regions = [(r0[0], r0[1], r0[2], "run"), (w0[0], w0[1], str(int(w0[1]) + 1), None), ("no_such_contig", "0", "100", "x"),
               (runs_sup[0][0], runs_sup[0][1], runs_sup[1][2], "two")]
    bed = tmp_path / "regions.bed"
    bed.write_text("#ctg\tstart\tend\n" + "".join("\t".join([c, s, e] + ([n] if n else [])) + "\n" for c, s, e, n in regions))
    alone = {
        "samples": (["--uncertaintySamples", "4"], ["posterior_samples_summary.tsv", "final_label_runs_support.bed"]),
        "confidence": (["--runConfidence"], ["final_label_runs_confidence.bed"]),
        "regions": (["--regionProbs", str(bed)], ["region_label_probabilities.tsv"]),
        "totals": (["--exactTotals"], ["label_totals_exact.tsv"]),
        "blocks": (["--numBlocks"], ["label_blocks_exact.tsv"]),
        "entropy": (["--jointEntropy"], ["path_uncertainty.tsv"]),
        "boundaries": (["--runBoundaries"], ["final_label_run_boundaries.tsv"]),
        # (with --regionProbs the option adds a row per region to its rows for the track and the contigs, by design: the single run
        # carries the regions too, and --keptBlocks by itself is compared below)
        "kept": (["--keptBlocks", "--regionProbs", str(bed)], ["kept_block_probabilities.tsv", "region_label_probabilities.tsv"]),
    }
    for name, (opt, _) in alone.items():
        if name != "samples":
            _cli(args + opt, tmp_path / name)
    _cli(args + [a for opt, _ in alone.values() for a in opt], tmp_path / "all")
    every = tmp_path / "all"
    written = set(os.listdir(every))
    for name, (_, files) in alone.items():
        for f in files + COMMON:
            assert f in written and f in os.listdir(tmp_path / name), (name, f)
            assert (every / f).read_bytes() == (tmp_path / name / f).read_bytes(), "%s differs between the combined run and the run with %s alone" % (f, name)
            assert (every / f).stat().st_size > 0, f
        # and everything else the single run wrote (summary tables, parameter files, the posterior BED) is the combined run's too
        for f in os.listdir(tmp_path / name):
            assert (every / f).read_bytes() == (tmp_path / name / f).read_bytes(), (name, f)
    # --keptBlocks without the regions: its file is the combined run's up to the region rows, every other file the combined run's
    _cli(args + ["--keptBlocks"], tmp_path / "kept_alone")
    head = (tmp_path / "kept_alone" / "kept_block_probabilities.tsv").read_bytes()
    both = (every / "kept_block_probabilities.tsv").read_bytes()
    assert len(head) > 0 and both.startswith(head) and [l.split(b"\t")[0] for l in both[len(head):].splitlines()] == [b"region"] * len(regions)
    for f in os.listdir(tmp_path / "kept_alone"):
        if f != "kept_block_probabilities.tsv":
            assert (every / f).read_bytes() == (tmp_path / "kept_alone" / f).read_bytes(), ("kept_alone", f)
    if base == ["--fitAlpha"]:
        assert "alpha_fitted.tsv" in written
    if "--viterbi" in base:
        assert "viterbi_log_probability.tsv" in written
    if "--enforceMinimumLengths" in base:                   # (compared above: every single run wrote it too)
        assert "viterbi_min_length_cost.tsv" in written and "viterbi_min_length_cost.tsv" in os.listdir(tmp_path / "kept")
