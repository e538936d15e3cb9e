"""The refusal of --crossChunkEM and its prefixes: one line, a failure, before the input is read (every case names an input that does
not exist; no GPU needed).  Its one row comes behind the rows of --lengthConstrainedEM, so every refusal pinned before it
(tests/test_cli_lcem_refusals_cpu.py, tests/test_cli_refusals_cpu.py) is still the one reported; everything else the option is
refused for is --lengthConstrainedEM's refusal, and the line of the lengths above 64 in sum names both options."""
import subprocess

import pytest

from test_cli_lcem_refusals_cpu import CASES as LCEM_CASES, CLI, LENGTHS, ONE_GPU, OPT as LCEM, _run
from test_cli_prefix_cpu import REFERENCE, unique_prefixes
from test_minlen_sum_joined_cpu import EARLIER as BEFORE_MERGED, OPTION as MERGED

OPT = "--crossChunkEM"
EARLIER = BEFORE_MERGED + [MERGED, "expectedAccuracy", "expectedGains", "lengthConstrainedEM"]


def test_the_option_alone_is_refused(tmp_path):
    status, lines = _run([OPT], tmp_path)
    assert status == 1 and lines == ["[TIME] Error: %s needs --lengthConstrainedEM." % OPT]
    status, lines = _run([OPT] + LENGTHS, tmp_path)
    assert status == 1 and lines == ["[TIME] Error: %s needs --lengthConstrainedEM." % OPT]


@pytest.mark.parametrize("name,args,env,want", LCEM_CASES, ids=[c[0] for c in LCEM_CASES])
def test_every_refusal_of_the_option_it_needs_is_still_the_one_reported(name, args, env, want, tmp_path):
    status, lines = _run(args + [OPT], tmp_path, env)
    assert status == 1 and len(lines) == 1, (status, lines)
    if name == "lanes":                                      # the line names every option that walks the expanded chain, as given
        want = want.replace("--lengthConstrainedEM:", "--lengthConstrainedEM, --crossChunkEM:")
    assert lines[0].startswith(want), lines


def test_an_earlier_refusal_still_wins(tmp_path):
    status, lines = _run([OPT, "--keptBlocks"], tmp_path)
    assert status == 1 and lines == ["[TIME] Error: --keptBlocks needs --minimumLengths."]
    status, lines = _run([OPT, "--mergedChunks"], tmp_path)
    assert status == 1 and lines == ["[TIME] Error: --mergedChunks needs --constrainedPosterior or --admissibleSamples."]
    status, lines = _run([OPT, LCEM, "--gpus", "2"] + LENGTHS, tmp_path)
    assert status == 1 and lines == ["[TIME] Error: %s %s" % (LCEM, ONE_GPU)]


def test_accepted_options_reach_the_loader(tmp_path):
    status, lines = _run([LCEM, OPT] + LENGTHS, tmp_path)
    assert status == 1 and lines[-1].endswith("Unable to open no_such_input.cov"), lines


def test_option_keeps_every_reference_prefix_and_every_earlier_one():
    ref = unique_prefixes(list(REFERENCE))
    before = dict(unique_prefixes(list(REFERENCE) + EARLIER))
    now = dict(unique_prefixes(list(REFERENCE) + EARLIER + [OPT[2:]]))
    assert [(p, n) for p, n in ref if now.get(p) != n and before.get(p) == n] == []      # (what kept[] holds up was lost before)
    assert {p: n for p, n in before.items() if now.get(p) != n} == {}
    assert "c" not in before and "cr" not in before          # --c was ambiguous already, nothing started with --cr
    assert now.get("cr") == OPT[2:] and now.get("le") == "lengthConstrainedEM"


def test_the_binary_resolves_the_prefixes():
    for p in ("--cr", "--cross", OPT):
        r = subprocess.run([CLI, p], capture_output=True, text=True)
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr, (p, r.stderr[-300:])
        assert "%s needs --lengthConstrainedEM." % OPT in r.stderr, (p, r.stderr[-300:])
    r = subprocess.run([CLI, "--le"], capture_output=True, text=True)
    assert "ambiguous" not in r.stderr and "--lengthConstrainedEM needs --minimumLengths" in r.stderr
    r = subprocess.run([CLI, "--l", "a,b,c,d"], capture_output=True, text=True)
    assert "ambiguous" not in r.stderr and "Input path cannot be NULL" in r.stderr
    r = subprocess.run([CLI, "--c"], capture_output=True, text=True)
    assert "ambiguous" in r.stderr
    for p, name in (("--wh", "--wholeContigs"), ("--cons", "--constrainedPosterior"), ("--me", "--mergedChunks")):
        r = subprocess.run([CLI, p, "--gpus", "2"], capture_output=True, text=True)
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and name in r.stderr, (p, r.stderr[-300:])


def test_help_names_the_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert OPT in r.stderr and "joined chunks of a contig" in r.stderr
