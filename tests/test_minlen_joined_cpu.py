"""CPU checks of the ground of the whole-contig minimum-run-length decoder (hf_viterbi_minlen_joined): the numpy reference the GPU
tests rely on (tests/minlen_joined_ref.py) against 50-digit enumeration of the admissible paths of every joined group, its exact cases,
a hand-counted case, and the command line's --wholeContigs option (prefixes, help text, refusals before the input is read)."""
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

from test_cli_prefix_cpu import ADDED, CLI, REFERENCE, unique_prefixes
import minlen_joined_ref as JR
import minlen_ref
import viterbi_ref

# the additions of this build before this option, in the order they came (hf_cli.cpp long_options)
EARLIER = ADDED + ["viterbi", "sweepAlpha", "uncertaintySamples", "uncertaintySeed", "runConfidence", "regionProbs", "fitAlpha",
                   "fitAlphaEntries", "fitAlphaMax", "fitAlphaEvery", "exactTotals", "numBlocks", "jointEntropy", "runBoundaries",
                   "keptBlocks", "enforceMinimumLengths", "constrainedPosterior", "admissibleSamples"]
OPTION = "wholeContigs"


def _tables(case):
    store, model, alpha, _ = minlen_ref.tiny_case(*case)
    return store, viterbi_ref.tables(store, model, alpha)


# ---- 1. the reference against enumeration ----------------------------------------------------------------------------------------

def _check_case_against_enumeration(case, decode):
    """decode(joined, min_len) -> (labels, chunk scores).  Every group of more than one chunk against its enumeration, the groups of
    one chunk against minlen_ref's.  Returns (groups checked by path, groups whose joined optimum is not its chunks' per-chunk optima)."""
    store, (logA, logend) = _tables(case)
    off = store.chunk_off
    enum1 = minlen_ref.tiny_case(*case)[3]
    groups = JR.tiny_groups(*case)
    checked = differ = 0
    for joined in JR.TINY_JOINS:
        goff, gf, gl = JR.group_offsets(off, joined)
        for ml in minlen_ref.TINY_MIN_LENS:
            labels, score = decode(joined, ml)
            per_chunk = minlen_ref.viterbi_minlen(logA, logend, off, ml)[0]
            multi = {a: (b, path, lbest, l2) for a, b, path, lbest, l2 in groups[(joined, ml)]}
            for g in range(gf.size):
                a, b = int(gf[g]), int(gl[g])
                if a in multi:
                    assert multi[a][0] == b
                    _, path, lbest, l2 = multi[a]
                else:
                    path, lbest, l2 = enum1[ml][a]
                assert abs(score[a] - float(lbest)) <= 1e-12 * abs(float(lbest)), (joined, ml, a, score[a], lbest)
                assert np.all(score[a + 1:b + 1] == 0.0)
                got = tuple(int(v) for v in labels[goff[g]:goff[g + 1]])
                if lbest - l2 > mp.mpf("1e-9") * abs(lbest):
                    assert got == path, (joined, ml, a, got, path)
                    checked += a in multi
                    differ += a in multi and got != tuple(int(v) for v in per_chunk[goff[g]:goff[g + 1]])
    return checked, differ


@pytest.mark.parametrize("case", minlen_ref.TINY_CASES)
def test_numpy_reference_against_group_enumeration(case):
    store, (logA, logend) = _tables(case)
    off = store.chunk_off

    def decode(joined, ml):
        labels, score, goff = JR.viterbi_minlen_joined(logA, logend, off, joined, ml)
        assert minlen_ref.admissible(labels, goff, ml).all()
        # by evaluation too: the weight of a group's path is the product of its chunks' weights
        val = JR.group_sums(viterbi_ref.path_log_prob(logA, logend, off, labels), off, joined)
        assert np.all(np.abs(val - score) <= 1e-12 * np.abs(score))
        return labels, score

    checked, _ = _check_case_against_enumeration(case, decode)
    assert checked >= 6                                      # of the 8 enumerated (pattern, lengths, group) cells


def test_the_join_bites_somewhere_in_the_parameter_set():
    """With the reference alone: in at least one group the joined optimum is not the concatenation of its chunks' per-chunk optima."""
    bites = 0
    for case in minlen_ref.TINY_CASES:
        store, (logA, logend) = _tables(case)
        off = store.chunk_off
        for joined in JR.TINY_JOINS:
            labels, _, goff = JR.viterbi_minlen_joined(logA, logend, off, joined, (3, 2, 2, 2))
            per_chunk = minlen_ref.viterbi_minlen(logA, logend, off, (3, 2, 2, 2))[0]
            bites += sum(not np.array_equal(labels[goff[g]:goff[g + 1]], per_chunk[goff[g]:goff[g + 1]]) for g in range(goff.size - 1))
    assert bites >= 1, "no join changes a path: the tests could not tell the two decoders apart"


# ---- 2. exact cases ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", minlen_ref.TINY_CASES)
def test_exact_cases_of_the_reference(case):
    store, (logA, logend) = _tables(case)
    off = store.chunk_off
    free = viterbi_ref.viterbi(logA, logend, off)[0]
    for ml in minlen_ref.TINY_MIN_LENS:
        la, sa = minlen_ref.viterbi_minlen(logA, logend, off, ml)
        for none in (None, np.zeros(store.n_chunks, bool)):
            lb, sb, goff = JR.viterbi_minlen_joined(logA, logend, off, none, ml)
            assert np.array_equal(la, lb) and np.array_equal(sa, sb) and np.array_equal(goff, off)
        for joined in JR.TINY_JOINS:
            lj, sj, _ = JR.viterbi_minlen_joined(logA, logend, off, joined, ml)
            bound = JR.group_sums(sa, off, joined)
            assert np.all(sj <= bound + 1e-12 * np.abs(bound)), (ml, joined, sj - bound)
            if ml == (1, 1, 1, 1):
                assert np.array_equal(lj, free)


def test_hand_counted_case():
    """Two chunks of two windows, joined, lengths (2, 1, 1, 1).  Per chunk the optima are (Hap, Err) and (Hap, Hap): 0.9 * 0.6 * 0.5 and
    0.9 * 0.8 * 0.5.  Over the group the single Err window at the end of chunk 0 is inside, so that path is out; what is left:
    (Hap, Hap, Hap, Hap) 0.9 * 0.3 * 0.5 * 0.9 * 0.8 * 0.5 = 0.0486, (Err, Err, Hap, Hap) 0.1 * 0.5 * 0.5 * 0.36 = 0.009 and
    (Hap, Err, Err, Err) 0.27 * 0.05 * 0.7 * 0.5 = 0.004725, whose Err run reaches the group's end."""
    A = np.zeros((4, 4, 4))
    A[0, 0] = [0.1, 0, 0.9, 0]
    A[1, 2, 0], A[1, 2, 2], A[1, 0, 0], A[1, 0, 2] = 0.6, 0.3, 0.5, 0.1
    A[2, 0] = [0.05, 0, 0.9, 0]
    A[3, 2, 2], A[3, 0, 0] = 0.8, 0.7
    with np.errstate(divide="ignore"):
        logA = np.log(A)
    logend = np.log(np.full((2, 4), 0.5))
    off = [0, 2, 4]
    m = (2, 1, 1, 1)
    lab, score = minlen_ref.viterbi_minlen(logA, logend, off, m)
    assert lab.tolist() == [2, 0, 2, 2]
    assert abs(score[0] - np.log(0.27)) < 1e-15 and abs(score[1] - np.log(0.36)) < 1e-15
    lab, score, goff = JR.viterbi_minlen_joined(logA, logend, off, [0, 1], m)
    assert lab.tolist() == [2, 2, 2, 2] and goff.tolist() == [0, 4]
    assert abs(score[0] - np.log(0.0486)) < 1e-14 and score[1] == 0.0
    assert JR.short_inner_runs([2, 0, 2, 2], goff, m) == [(1, 1, 0)] and JR.short_inner_runs(lab, goff, m) == []
    # the Err run that reaches the group's end is exempt: take Hap out of chunk 1
    logA2 = logA.copy()
    logA2[2, 0, 2] = -np.inf
    lab, score, _ = JR.viterbi_minlen_joined(logA2, logend, off, [0, 1], m)
    assert lab.tolist() == [2, 0, 0, 0] and abs(score[0] - np.log(0.004725)) < 1e-14


def test_a_chunk_without_windows_ends_a_group():
    off = [0, 3, 3, 5, 9, 9]
    assert JR.group_first_chunks(off, [0, 1, 1, 1, 1]).tolist() == [0, 1, 2, 4]
    assert JR.group_first_chunks(off, None).tolist() == [0, 1, 2, 3, 4]
    goff, gf, gl = JR.group_offsets(off, [0, 1, 1, 1, 1])
    assert goff.tolist() == [0, 3, 3, 9, 9] and gl.tolist() == [0, 1, 3, 4]


# ---- 3. the command line's option ---------------------------------------------------------------------------------------------------

def test_option_keeps_every_reference_prefix_and_every_earlier_one():
    ref = unique_prefixes(list(REFERENCE))
    now = dict(unique_prefixes(list(REFERENCE) + EARLIER + [OPTION]))
    lost = [(p, n) for p, n in ref if now.get(p) != n]
    assert not lost, lost
    before = dict(unique_prefixes(list(REFERENCE) + EARLIER))
    assert {p: n for p, n in before.items() if now.get(p) != n} == {}
    assert before.get("j") == "jointEntropy" and before.get("cons") == "constrainedPosterior" and before.get("en") == "enforceMinimumLengths"
    assert "w" not in before and "wh" not in before          # --w was ambiguous already, nothing started with --wh
    assert now.get("wh") == OPTION


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
    for p in ("--wh", "--whole", "--" + OPTION):
        r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), p])
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr, (p, r.stderr[-300:])
        assert "--wholeContigs needs --viterbi --enforceMinimumLengths" in r.stderr, (p, r.stderr[-300:])
    for p, name in (("--j", "--jointEntropy"), ("--cons", "--constrainedPosterior"), ("--en", "--enforceMinimumLengths")):
        r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), p, "--gpus", "2"])
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and name in r.stderr, (p, r.stderr[-300:])


BOTH = ["--viterbi", "--enforceMinimumLengths"]


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
@pytest.mark.parametrize("extra,env,needle", [
    ([], {}, "needs --viterbi --enforceMinimumLengths"),
    (["--viterbi"], {}, "needs --viterbi --enforceMinimumLengths"),
    (["--enforceMinimumLengths"], {}, "needs --viterbi --enforceMinimumLengths"),
    (BOTH + ["--gpus", "2"], {}, "one GPU"),
    (BOTH, {"HF_LOOPBACK_RANKS": "2"}, "one GPU"),
    (BOTH + ["--sweepAlpha", "x"], {}, "one GPU"),
    (BOTH + ["-W", "1000", "--minimumLengths", "30000,20000,13001"], {}, "30,20,1,14"),
])
def test_refusals_come_before_the_input_is_read(tmp_path, extra, env, needle):
    """The input named here does not exist, so only the refusal can be the error."""
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--" + OPTION] + extra, env)
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert r.returncode != 0
    assert len(lines) == 1 and "--" + OPTION in lines[0] and needle in lines[0], r.stderr[-500:]


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_the_option_with_what_it_needs_passes_the_option_checks(tmp_path):
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--" + OPTION] + BOTH)
    assert r.returncode != 0 and OPTION not in r.stderr
