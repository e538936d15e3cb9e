"""CPU checks of the minimum-run-length Viterbi decoder's ground: the numpy reference the GPU tests rely on (tests/minlen_ref.py)
against mpmath enumeration of all admissible paths, and the command line's --enforceMinimumLengths option (prefixes, help text,
refusals before the input is read)."""
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

from test_cli_prefix_cpu import ADDED, CLI, REFERENCE, unique_prefixes
import minlen_ref
import viterbi_ref

# the additions of this build before this option, in the order they came (hf_cli.cpp long_options)
EARLIER = ADDED + ["viterbi", "sweepAlpha", "uncertaintySamples", "uncertaintySeed", "runConfidence", "regionProbs", "fitAlpha",
                   "fitAlphaEntries", "fitAlphaMax", "fitAlphaEvery", "exactTotals", "numBlocks", "jointEntropy", "runBoundaries"]
OPTION = "enforceMinimumLengths"


@pytest.mark.parametrize("model_type,seed,hifi", minlen_ref.TINY_CASES)
def test_numpy_reference_against_path_enumeration(model_type, seed, hifi):
    store, model, alpha, enum = minlen_ref.tiny_case(model_type, seed, hifi)
    off = store.chunk_off
    for min_len in minlen_ref.TINY_MIN_LENS:
        labels, score, plp, free = minlen_ref.reference(store, model, alpha, min_len)
        assert minlen_ref.admissible(labels, off, min_len).all()
        got = plp(labels)
        bites = int(np.sum(~minlen_ref.admissible(free, off, min_len)))
        if min_len == (3, 2, 2, 2):
            assert bites >= 1, "the constraint changes no chunk of this case: the test would pass vacuously"
        else:
            assert bites == 0
        checked = 0
        for c in range(store.n_chunks):
            path, lbest, l2 = enum[min_len][c]
            assert abs(score[c] - float(lbest)) <= 1e-12 * abs(float(lbest)), (min_len, c, score[c], lbest)
            assert abs(got[c] - float(lbest)) <= 1e-12 * abs(float(lbest)), (min_len, c, got[c], lbest)
            if lbest - l2 > mp.mpf("1e-9") * abs(lbest):
                assert tuple(int(v) for v in labels[off[c]:off[c + 1]]) == path, (min_len, c, labels[off[c]:off[c + 1]], path)
                checked += 1
        assert checked >= store.n_chunks - 1


@pytest.mark.parametrize("model_type,seed,hifi", minlen_ref.TINY_CASES)
def test_all_ones_is_the_unconstrained_reference_bitwise(model_type, seed, hifi):
    store, model, alpha, _ = minlen_ref.tiny_case(model_type, seed, hifi)
    logA, logend = viterbi_ref.tables(store, model, alpha)
    la, sa = minlen_ref.viterbi_minlen(logA, logend, store.chunk_off, (1, 1, 1, 1))
    lb, sb = viterbi_ref.viterbi(logA, logend, store.chunk_off)
    assert np.array_equal(la, lb) and np.array_equal(sa, sb)


def test_admissible_exempts_the_runs_at_the_chunk_ends():
    off = [0, 6, 6, 7, 13]
    #          chunk 0 (6)        chunk 2 (1)  chunk 3 (6)
    lab = [0, 2, 2, 2, 2, 3,      1,           2, 2, 3, 2, 2, 2]
    assert minlen_ref.admissible(lab, off, (3, 2, 2, 2)).tolist() == [True, True, True, False]      # the 1-window Col run inside chunk 3
    assert minlen_ref.admissible(lab, off, (3, 2, 2, 1)).tolist() == [True, True, True, True]
    assert minlen_ref.admissible([1] * 13, off, (9, 9, 9, 9)).all()                                  # constant paths are always admissible


def test_reference_ties_go_to_the_lowest_state_and_lane():
    logA = np.log(np.full((5, 4, 4), 0.25))
    logA[0] = -np.inf
    logA[0, 0, :] = np.log(0.25)
    logend = np.log(np.full((1, 4), 0.5))
    labels, score = minlen_ref.viterbi_minlen(logA, logend, [0, 5], (2, 3, 1, 2))
    # every path has the same weight.  The end takes the first largest lane, (Err, 1), whose predecessor is the lowest p != Err: Dup's
    # saturated lane, which did not stay (no strict >) but arrived through (Dup, 2) and (Dup, 1), entered from the lowest p: Err
    assert labels.tolist() == [0, 1, 1, 1, 0]
    assert abs(score[0] - (5 * np.log(0.25) + np.log(0.5))) < 1e-15


def test_option_keeps_every_reference_prefix_and_every_earlier_one():
    ref = unique_prefixes(list(REFERENCE))
    now = dict(unique_prefixes(list(REFERENCE) + EARLIER + [OPTION]))
    lost = [(p, n) for p, n in ref if now.get(p) != n]
    assert not lost, lost
    before = dict(unique_prefixes(list(REFERENCE) + EARLIER))
    # (--e, --ex, --ru and --run are kept by the command line's own table: they were ambiguous before this option already)
    assert {p: n for p, n in before.items() if now.get(p) != n} == {}
    assert now.get("mini") == "minimumLengths" and now.get("en") == OPTION


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("HF_LOOPBACK_RANKS", None)
    e.update(env or {})
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=e)


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_help_mentions_the_option():
    r = _run(["--help"])
    assert "--" + OPTION in r.stderr + r.stdout


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_the_binary_resolves_the_prefixes(tmp_path):
    for p in ("--mini", "--minimumLengths"):
        r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), p, "1,2"])
        assert "ambiguous" not in r.stderr and "--minimumLengths" in r.stderr, (p, r.stderr[-300:])
    for p in ("--en", "--enforce", "--" + OPTION):
        r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), p])
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and "--enforceMinimumLengths needs --viterbi" in r.stderr, p


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
@pytest.mark.parametrize("extra,env,needle", [
    ([], {}, "needs --viterbi"),
    (["--viterbi", "--gpus", "2"], {}, "one GPU"),
    (["--viterbi"], {"HF_LOOPBACK_RANKS": "2"}, "one GPU"),
    (["--viterbi", "--sweepAlpha", "x"], {}, "one GPU"),
    (["--viterbi", "-W", "1000", "--minimumLengths", "30000,20000,13001"], {}, "30,20,1,14"),
])
def test_refusals_come_before_the_input_is_read(tmp_path, extra, env, needle):
    """The input named here does not exist, so only the refusal can be the error."""
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--" + OPTION] + extra, env)
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert r.returncode != 0
    assert len(lines) == 1 and "--" + OPTION in lines[0] and needle in lines[0], r.stderr[-500:]


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_lengths_within_the_lane_budget_pass_the_option_checks(tmp_path):
    """30 + 20 + 1 + 13 = 64 windows: not refused; the run stops at the missing input."""
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--" + OPTION, "--viterbi", "-W", "1000", "--minimumLengths",
              "30000,20000,13000"])
    assert r.returncode != 0 and OPTION not in r.stderr
