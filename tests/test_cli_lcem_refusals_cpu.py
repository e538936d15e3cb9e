"""The refusals of --lengthConstrainedEM: one line each, a failure, before the input is read (every case names an input that does not
exist; no GPU needed).  Its rows come after every earlier row of check_options, so of an earlier bad option and one of these the
earlier one is still reported (tests/test_cli_refusals_cpu.py pins the earlier ones)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
OPT = "--lengthConstrainedEM"
LENGTHS = ["--minimumLengths", "12000,20000,28000"]
ONE_GPU = "runs on one GPU: it cannot be combined with --gpus N>1, HF_LOOPBACK_RANKS or --sweepAlpha."


def _run(args, tmp_path, env=None):
    e = dict(os.environ)
    e.pop("HF_LOOPBACK_RANKS", None)
    e.update(env or {})
    r = subprocess.run([CLI, "-i", "no_such_input.cov", "-o", str(tmp_path)] + args, capture_output=True, text=True, env=e)
    return r.returncode, re.sub(r"^\[[^\]]*\]", "[TIME]", r.stderr, flags=re.M).splitlines()


CASES = [
    ("no lengths", [OPT], None, "[TIME] Error: %s needs --minimumLengths." % OPT),
    ("accelerate", [OPT, "--accelerate"] + LENGTHS, None, "[TIME] Error: %s cannot be combined with --accelerate" % OPT),
    ("fitAlpha", [OPT, "--fitAlpha"] + LENGTHS, None, "[TIME] Error: %s cannot be combined with --fitAlpha" % OPT),
    ("negative_binomial", [OPT, "--modelType", "negative_binomial"] + LENGTHS, None, "[TIME] Error: %s needs --modelType gaussian or trunc_exp_gaussian" % OPT),
    ("gpus", [OPT, "--gpus", "2"] + LENGTHS, None, "[TIME] Error: %s %s" % (OPT, ONE_GPU)),
    ("loopback", [OPT] + LENGTHS, {"HF_LOOPBACK_RANKS": "2"}, "[TIME] Error: %s %s" % (OPT, ONE_GPU)),
    ("lanes", [OPT, "-W", "1000", "--minimumLengths", "30000,20000,16000"], None,
     "[TIME] Error: --lengthConstrainedEM: the minimum lengths are 30,20,1,16 windows of 1000 bases (Err,Dup,Hap,Col), above 64 in sum."),
]


@pytest.mark.parametrize("name,args,env,want", CASES, ids=[c[0] for c in CASES])
def test_refusal(name, args, env, want, tmp_path):
    status, lines = _run(args, tmp_path, env)
    assert status == 1 and len(lines) == 1, (status, lines)
    assert lines[0].startswith(want), lines


def test_sweep_alpha_is_refused(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("")
    status, lines = _run([OPT, "--sweepAlpha", str(lst)] + LENGTHS, tmp_path)
    assert status == 1 and lines == ["[TIME] Error: %s %s" % (OPT, ONE_GPU)]


def test_an_earlier_refusal_still_wins(tmp_path):
    status, lines = _run([OPT, "--keptBlocks"], tmp_path)
    assert status == 1 and lines == ["[TIME] Error: --keptBlocks needs --minimumLengths."]


def test_accepted_options_reach_the_loader(tmp_path):
    status, lines = _run([OPT] + LENGTHS, tmp_path)
    assert status == 1 and lines[-1].endswith("Unable to open no_such_input.cov"), lines


def test_prefixes():
    """--l stays --labelNames (kept[]); --le is the new option's shortest prefix; the help text names it."""
    r = subprocess.run([CLI, "--l", "a,b,c,d"], capture_output=True, text=True)
    assert "ambiguous" not in r.stderr and "Input path cannot be NULL" in r.stderr
    r = subprocess.run([CLI, "--le"], capture_output=True, text=True)
    assert "ambiguous" not in r.stderr and "--lengthConstrainedEM needs --minimumLengths" in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--lengthConstrainedEM" in r.stderr
