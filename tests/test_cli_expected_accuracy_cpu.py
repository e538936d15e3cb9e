"""The refusals of hmm_flagger --expectedAccuracy and --expectedGains: every one ends before the input is read, so no GPU is needed
(the input named does not exist).  A refusal is one line on stderr and exit status 1."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
M = ["--minimumLengths", "8000,12000,8000"]


def _refused(args, tmp_path, env=None):
    e = dict(os.environ)
    e.pop("HF_LOOPBACK_RANKS", None)
    e.update(env or {})
    r = subprocess.run([CLI, "-i", "no_such_input.cov", "-o", str(tmp_path)] + args, capture_output=True, text=True, env=e)
    assert r.returncode == 1, (args, r.returncode, r.stderr)
    lines = r.stderr.splitlines()
    assert len(lines) == 1, (args, lines)
    return re.sub(r"^\[[^\]]*\] ", "", lines[0])


def _gains(tmp_path, text):
    p = tmp_path / "gains.tsv"
    p.write_text(text)
    return str(p)


IDENTITY = "1\t0\t0\t0\n0\t1\t0\t0\n0\t0\t1\t0\n0\t0\t0\t1\n"


@pytest.mark.parametrize("args,line", [
    (["--expectedAccuracy", "windows"] + M, "Error: --expectedAccuracy can be chunks or contigs."),
    (["--expectedAccuracy", "Chunks"] + M, "Error: --expectedAccuracy can be chunks or contigs."),
    (["--expectedAccuracy", "chunks"], "Error: --expectedAccuracy needs --minimumLengths."),
    (["--expectedAccuracy", "contigs"], "Error: --expectedAccuracy needs --minimumLengths."),
    (["--expectedAccuracy", "contigs", "--viterbi"] + M, "Error: --expectedAccuracy cannot be combined with --viterbi."),
    (["--expectedAccuracy", "chunks", "--gpus", "2"] + M,
     "Error: --expectedAccuracy runs on one GPU: it cannot be combined with --gpus N>1, HF_LOOPBACK_RANKS or --sweepAlpha."),
    (["--expectedAccuracy", "chunks", "--minimumLengths", "1000000,1000000,1000000", "-W", "1000"],
     "Error: --expectedAccuracy: the minimum lengths are 1000,1000,1,1000 windows of 1000 bases (Err,Dup,Hap,Col), above 64 in sum."),
])
def test_refusals_of_the_option(args, line, tmp_path):
    assert _refused(args, tmp_path) == line


def test_the_order_of_the_refusals(tmp_path):
    # the argument before the missing lengths, the lengths before --viterbi, --viterbi before the one-GPU rule
    assert _refused(["--expectedAccuracy", "x", "--viterbi"], tmp_path) == "Error: --expectedAccuracy can be chunks or contigs."
    assert _refused(["--expectedAccuracy", "chunks", "--viterbi"], tmp_path) == "Error: --expectedAccuracy needs --minimumLengths."
    assert _refused(["--expectedAccuracy", "chunks", "--viterbi", "--gpus", "2"] + M, tmp_path) == \
        "Error: --expectedAccuracy cannot be combined with --viterbi."
    # behind --mergedChunks' row
    assert _refused(["--expectedAccuracy", "x", "--mergedChunks"], tmp_path) == \
        "Error: --mergedChunks needs --constrainedPosterior or --admissibleSamples."


def test_loopback_ranks_are_refused(tmp_path):
    assert _refused(["--expectedAccuracy", "chunks"] + M, tmp_path, {"HF_LOOPBACK_RANKS": "2"}) == \
        "Error: --expectedAccuracy runs on one GPU: it cannot be combined with --gpus N>1, HF_LOOPBACK_RANKS or --sweepAlpha."


def test_gains_without_the_option(tmp_path):
    g = _gains(tmp_path, IDENTITY)
    assert _refused(["--expectedGains", g], tmp_path) == "Error: --expectedGains needs --expectedAccuracy."
    assert _refused(["--expectedGains", g] + M, tmp_path) == "Error: --expectedGains needs --expectedAccuracy."


@pytest.mark.parametrize("text", [
    "1\t0\t0\t0\n0\t1\t0\t0\n0\t0\t1\t0\n",                           # three rows
    IDENTITY + "0\t0\t0\t1\n",                                        # five rows
    "1\t0\t0\n0\t1\t0\t0\n0\t0\t1\t0\n0\t0\t0\t1\n",                  # a row of three
    "1\t0\t0\t0\t0\n0\t1\t0\t0\n0\t0\t1\t0\n0\t0\t0\t1\n",            # a row of five
    "1\t0\t0\t0\n0\tx\t0\t0\n0\t0\t1\t0\n0\t0\t0\t1\n",               # not a number
    "1\t0\t0\t0\n0\t1.5e\t0\t0\n0\t0\t1\t0\n0\t0\t0\t1\n",            # a number with a tail
    "1\t0\t0\t0\n0\tinf\t0\t0\n0\t0\t1\t0\n0\t0\t0\t1\n",
    "1\t0\t0\t0\n0\tnan\t0\t0\n0\t0\t1\t0\n0\t0\t0\t1\n",
    "1\t0\t0\t0\n0\t1e101\t0\t0\n0\t0\t1\t0\n0\t0\t0\t1\n",           # above 1e100 in magnitude
    "",
], ids=["3rows", "5rows", "3cols", "5cols", "text", "tail", "inf", "nan", "large", "empty"])
def test_a_gain_file_that_is_not_four_by_four_finite_numbers(text, tmp_path):
    g = _gains(tmp_path, text)
    want = "Error: --expectedGains: %s is not a file of 4x4 tab-separated finite numbers." % g
    assert _refused(["--expectedAccuracy", "contigs", "--expectedGains", g] + M, tmp_path) == want


def test_a_missing_gain_file(tmp_path):
    g = str(tmp_path / "none.tsv")
    assert _refused(["--expectedAccuracy", "contigs", "--expectedGains", g] + M, tmp_path) == \
        "Error: --expectedGains: %s is not a file of 4x4 tab-separated finite numbers." % g


def test_prefixes(tmp_path):
    """--expectedA resolves to --expectedAccuracy, --expectedG to --expectedGains; --exp is ambiguous between the two; --ex and --e stay
    --exchange."""
    assert _refused(["--expectedA", "x"] + M, tmp_path) == "Error: --expectedAccuracy can be chunks or contigs."
    assert _refused(["--expectedG", _gains(tmp_path, IDENTITY)], tmp_path) == "Error: --expectedGains needs --expectedAccuracy."
    r = subprocess.run([CLI, "--exp", "chunks", "-i", "no_such_input.cov", "-o", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 1 and "ambiguous" in r.stderr and "Usage:" in r.stderr
    for pre in ("--ex", "--e"):
        assert _refused([pre, "neither"], tmp_path) == "Error: --exchange can be chunks or ranks."
    # a served gain file passes every check of the option: the run ends at the loader
    r = subprocess.run([CLI, "-i", "no_such_input.cov", "-o", str(tmp_path), "--expectedA", "contigs", "--expectedG",
                        _gains(tmp_path, "1\t0\t0.25\t0\n0\t1.5\t-0.5\t0.25\n0.125\t0\t1\t0\n0\t0.5\t0\t-1e100\n\n")] + M, capture_output=True, text=True)
    assert r.returncode == 1 and "Parsing/Creating coverage chunks." in r.stderr and "Unable to open no_such_input.cov" in r.stderr
