"""Every refusal of the command line, alone and in pairs, replayed against the built `hmm_flagger` and compared with what the binary of
tests/golden/cli_refusals.json's `parent_commit` printed: exit status and stderr, byte for byte (timestamps aside).  Pins the messages and
the order in which check_options tries them: of two bad options the one checked first is reported.  No GPU needed: every case names an
input that does not exist, and all but a few end before the loader.  The cases: tests/cli_refusal_cases.py."""
import os

import pytest

import cli_refusal_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")


@pytest.fixture(scope="module")
def differences():
    return {name: (want, got) for name, want, got in C.check(CLI)}


def test_the_golden_file_holds_every_case_and_its_parent_commit():
    with open(C.GOLDEN) as f:
        g = C.json.load(f)
    assert len(g["parent_commit"]) == 40
    cases = C.cases()
    assert set(g["singles"]) | set(g["pairs"]) == set(cases)
    assert len(g["singles"]) == len(C.triggers()) >= 60 and len(g["pairs"]) > 1000


def test_every_trigger_alone_is_answered_as_before(differences):
    bad = {k: v for k, v in differences.items() if "+" not in k}
    assert not bad, list(bad.items())[:5]


def test_of_two_triggers_the_same_one_wins_as_before(differences):
    bad = {k: v for k, v in differences.items() if "+" in k}
    assert not bad, (len(bad), list(bad.items())[:5])


def test_a_refusal_is_one_line_and_a_failure():
    """What the golden file itself must show: a refused command line prints exactly one line and fails; the only other end of a case
    is the loader's, after `Parsing/Creating coverage chunks.`"""
    for name, e in C.expected().items():
        lines = e["stderr"].splitlines()
        assert e["status"] == 1, name
        if "Parsing/Creating coverage chunks." in e["stderr"]:
            assert len(lines) == 2 and lines[1].endswith("Unable to open no_such_input.cov"), (name, lines)
        else:
            assert len(lines) == 1 and lines[0].startswith("[TIME] Error: "), (name, lines)
