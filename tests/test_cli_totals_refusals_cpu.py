"""The refusals of --totalsDistribution and its prefixes: one line, a failure, before the input is read (every case names an input that
does not exist; no GPU needed).  Its row comes behind every earlier option's, so a refusal pinned before it is still the one reported:
with the --regionProbs it needs, --gpus N>1 and --sweepAlpha are refused in --regionProbs' own words (its row is an early one), and
HF_LOOPBACK_RANKS, which --regionProbs lets pass until after the EM, in this option's."""
import subprocess

import pytest

from test_cli_lcem_refusals_cpu import CLI, ONE_GPU, _run
from test_cli_prefix_cpu import REFERENCE, unique_prefixes
from test_cli_runlengths_refusals_cpu import EARLIER as BEFORE_RUN_LENGTHS, OPT as RUN_LENGTHS

OPT = "--totalsDistribution"
EARLIER = BEFORE_RUN_LENGTHS + [RUN_LENGTHS[2:]]
BAD_K = "[TIME] Error: %s should be a number of windows between 1 and 62." % OPT
NO_REGIONS = "[TIME] Error: %s needs --regionProbs." % OPT
REGIONS_ONE_GPU = "[TIME] Error: --regionProbs runs on one GPU: it cannot be combined with --gpus N>1 or --sweepAlpha."


@pytest.fixture
def bed(tmp_path):
    p = tmp_path / "regions.bed"
    p.write_text("ctg1\t0\t1000\tr0\n")
    return str(p)


def test_bad_counts(tmp_path, bed):
    for k in ("0", "63", "-3", "many", "1.5", "99999999999"):
        for more in ([], ["--regionProbs", bed]):
            status, lines = _run([OPT, k] + more, tmp_path)
            assert status == 1 and lines == [BAD_K], (k, more, lines)


def test_missing_region_file_option(tmp_path):
    for more in ([], ["--gpus", "2"], ["--sweepAlpha", "no_such_list"]):
        status, lines = _run([OPT, "8"] + more, tmp_path)
        assert status == 1 and lines == [NO_REGIONS], (more, lines)
    status, lines = _run([OPT, "8"], tmp_path, {"HF_LOOPBACK_RANKS": "2"})
    assert status == 1 and lines == [NO_REGIONS]


def test_more_than_one_gpu(tmp_path, bed):
    # --regionProbs' row is an earlier one: its words
    status, lines = _run([OPT, "8", "--regionProbs", bed, "--gpus", "2"], tmp_path)
    assert status == 1 and lines == [REGIONS_ONE_GPU]
    status, lines = _run([OPT, "8", "--regionProbs", bed, "--sweepAlpha", "no_such_list"], tmp_path)
    assert status == 1 and lines == [REGIONS_ONE_GPU]
    # HF_LOOPBACK_RANKS passes --regionProbs' row and is refused here, before the input is read
    status, lines = _run([OPT, "8", "--regionProbs", bed], tmp_path, {"HF_LOOPBACK_RANKS": "2"})
    assert status == 1 and lines == ["[TIME] Error: %s %s" % (OPT, ONE_GPU)]
    status, lines = _run(["--regionProbs", bed], tmp_path, {"HF_LOOPBACK_RANKS": "2"})      # (without the option: the loader is reached)
    assert status == 1 and lines[-1].endswith("Unable to open no_such_input.cov"), lines


def test_accepted_options_reach_the_loader(tmp_path, bed):
    for args in ([OPT, "1"], [OPT, "62"], ["--to", "8"], ["--totals=8"]):
        status, lines = _run(args + ["--regionProbs", bed], tmp_path)
        assert status == 1 and lines[-1].endswith("Unable to open no_such_input.cov"), (args, lines)


def test_an_earlier_refusal_still_wins(tmp_path, bed):
    status, lines = _run([OPT, "0", "--keptBlocks"], tmp_path)
    assert status == 1 and lines == ["[TIME] Error: --keptBlocks needs --minimumLengths."]
    status, lines = _run([OPT, "8", "--numBlocks", "--gpus", "2"], tmp_path)
    assert status == 1 and lines == ["[TIME] Error: --numBlocks runs on one GPU: it cannot be combined with --gpus N>1 or --sweepAlpha."]
    status, lines = _run([OPT, "0", RUN_LENGTHS, "0"], tmp_path)                             # the row right in front of it
    assert status == 1 and lines == ["[TIME] Error: %s should be a number of windows between 1 and 64." % RUN_LENGTHS]
    status, lines = _run([OPT, "0", RUN_LENGTHS, "8"], tmp_path, {"HF_LOOPBACK_RANKS": "2"})
    assert status == 1 and lines == ["[TIME] Error: %s %s" % (RUN_LENGTHS, ONE_GPU)]
    status, lines = _run([OPT, "0", "--regionProbs", str(tmp_path / "no_such.bed")], tmp_path)
    assert status == 1 and len(lines) == 1 and "--regionProbs: cannot read" in lines[0]


def test_option_keeps_every_reference_prefix_and_every_earlier_one():
    ref = unique_prefixes(list(REFERENCE))
    before = dict(unique_prefixes(list(REFERENCE) + EARLIER))
    now = dict(unique_prefixes(list(REFERENCE) + EARLIER + [OPT[2:]]))
    assert [(p, n) for p, n in ref if now.get(p) != n and before.get(p) == n] == []
    assert {p: n for p, n in before.items() if now.get(p) != n} == {}
    assert not any(n.startswith("to") for n in list(REFERENCE) + EARLIER)      # no option started with --to
    assert "t" not in before                                                 # --t was ambiguous already (--threads, --trackName)
    assert now.get("to") == OPT[2:] and now.get("th") == "threads" and now.get("tr") == "trackName"


def test_the_binary_resolves_the_prefixes():
    for p in ("--to", "--total", "--totalsD", OPT):
        r = subprocess.run([CLI, p, "0"], capture_output=True, text=True)
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr, (p, r.stderr[-300:])
        assert "%s should be a number of windows between 1 and 62." % OPT in r.stderr, (p, r.stderr[-300:])
    r = subprocess.run([CLI, "--t", "1"], capture_output=True, text=True)      # as before
    assert "ambiguous" in r.stderr
    for p, msg in (("--th", "Input path cannot be NULL"), ("--tr", "Input path cannot be NULL")):
        r = subprocess.run([CLI, p, "1"], capture_output=True, text=True)
        assert "ambiguous" not in r.stderr and msg in r.stderr, (p, r.stderr[-300:])


def test_help_names_the_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert OPT in r.stderr and "region_label_totals_exact.tsv" in r.stderr
