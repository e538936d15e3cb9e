"""The refusals of --runLengths and its prefixes: one line, a failure, before the input is read (every case names an input that does
not exist; no GPU needed).  Its row comes behind every earlier option's, so a refusal pinned before it is still the one reported; the
line of a spectrum that ends below the largest minimum length names both options and the numbers."""
import subprocess

import pytest

from test_cli_lcem_refusals_cpu import CLI, LENGTHS, ONE_GPU, _run
from test_cli_crosschunk_refusals_cpu import EARLIER as BEFORE_CROSS, OPT as CROSS
from test_cli_prefix_cpu import REFERENCE, unique_prefixes

OPT = "--runLengths"
EARLIER = BEFORE_CROSS + [CROSS[2:]]
BAD_L = "[TIME] Error: %s should be a number of windows between 1 and 64." % OPT

CASES = [
    ("zero", [OPT, "0"], None, BAD_L),
    ("above 64", [OPT, "65"], None, BAD_L),
    ("negative", [OPT, "-3"], None, BAD_L),
    ("not a number", [OPT, "many"], None, BAD_L),
    ("gpus", [OPT, "8", "--gpus", "2"], None, "[TIME] Error: %s %s" % (OPT, ONE_GPU)),
    ("loopback", [OPT, "8"], {"HF_LOOPBACK_RANKS": "2"}, "[TIME] Error: %s %s" % (OPT, ONE_GPU)),
    ("sweepAlpha", [OPT, "8", "--sweepAlpha", "no_such_list"], None, "[TIME] Error: %s %s" % (OPT, ONE_GPU)),
    ("below the largest minimum", [OPT, "5", "-W", "4000"] + LENGTHS, None,
     "[TIME] Error: --runLengths 5: --minimumLengths 12000,20000,28000 (Err,Dup,Col) are 3,5,1,7 windows of 4000 bases (Err,Dup,Hap,Col); "
     "label_blocks_kept_exact.tsv needs --runLengths of at least 6."),
]


@pytest.mark.parametrize("name,args,env,want", CASES, ids=[c[0] for c in CASES])
def test_refusal(name, args, env, want, tmp_path):
    status, lines = _run(args, tmp_path, env)
    assert status == 1 and lines == [want], (status, lines)


def test_accepted_options_reach_the_loader(tmp_path):
    for args in ([OPT, "1"], [OPT, "64"], [OPT, "6", "-W", "4000"] + LENGTHS, ["--runL", "8"]):
        status, lines = _run(args, tmp_path)
        assert status == 1 and lines[-1].endswith("Unable to open no_such_input.cov"), (args, lines)


def test_an_earlier_refusal_still_wins(tmp_path):
    status, lines = _run([OPT, "0", "--keptBlocks"], tmp_path)
    assert status == 1 and lines == ["[TIME] Error: --keptBlocks needs --minimumLengths."]
    status, lines = _run([OPT, "8", "--numBlocks", "--gpus", "2"], tmp_path)
    assert status == 1 and lines == ["[TIME] Error: --numBlocks runs on one GPU: it cannot be combined with --gpus N>1 or --sweepAlpha."]
    status, lines = _run([OPT, "0", CROSS], tmp_path)
    assert status == 1 and lines == ["[TIME] Error: %s needs --lengthConstrainedEM." % CROSS]


def test_option_keeps_every_reference_prefix_and_every_earlier_one():
    ref = unique_prefixes(list(REFERENCE))
    before = dict(unique_prefixes(list(REFERENCE) + EARLIER))
    now = dict(unique_prefixes(list(REFERENCE) + EARLIER + [OPT[2:]]))
    assert [(p, n) for p, n in ref if now.get(p) != n and before.get(p) == n] == []
    assert {p: n for p, n in before.items() if now.get(p) != n} == {}
    assert not any(n.startswith("r") for n in REFERENCE)      # no reference option starts with r
    assert "run" not in before and "ru" not in before         # --ru and --run were ambiguous already (kept for --runConfidence by the command line)
    assert now.get("runL") == OPT[2:] and "runC" in before and "runB" in before


def test_the_binary_resolves_the_prefixes():
    for p in ("--runL", "--runLen", OPT):
        r = subprocess.run([CLI, p, "0"], capture_output=True, text=True)
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr, (p, r.stderr[-300:])
        assert "%s should be a number of windows between 1 and 64." % OPT in r.stderr, (p, r.stderr[-300:])
    for p in ("--ru", "--run", "--runC"):                     # they stay --runConfidence
        r = subprocess.run([CLI, p, "--gpus", "2"], capture_output=True, text=True)
        assert "ambiguous" not in r.stderr and "--runConfidence runs on one GPU" in r.stderr, (p, r.stderr[-300:])
    r = subprocess.run([CLI, "--runB", "--gpus", "2"], capture_output=True, text=True)
    assert "--runBoundaries runs on one GPU" in r.stderr


def test_help_names_the_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert OPT in r.stderr and "label_block_lengths_exact.tsv" in r.stderr and "label_blocks_kept_exact.tsv" in r.stderr
