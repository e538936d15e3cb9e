"""The reference of the exact breakpoint posteriors (tests/breakpoint_ref.py) against itself, and what the command line decides about
--runBoundaries before it reads any input.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_bruteforce_cpu import _tiny_store
from test_cli_prefix_cpu import REFERENCE, unique_prefixes
from test_viterbi_cpu import perturbed_model
import breakpoint_ref as BR
import sampling_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
LENGTHS = [7, 5, 1, 6, 3, 40]
TINY = [(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 0), (N.HF_MODEL_GAUSSIAN, 1), (N.HF_MODEL_NEGATIVE_BINOMIAL, 2)]
# every long option this command line adds to the reference's (hf_cli.cpp)
OWN = ["device", "hipAlgo", "gpus", "exchange", "viterbi", "sweepAlpha", "uncertaintySamples", "uncertaintySeed", "runConfidence",
       "regionProbs", "fitAlpha", "fitAlphaEntries", "fitAlphaMax", "fitAlphaEvery", "exactTotals", "numBlocks", "jointEntropy",
       "runBoundaries"]


def tiny(model_type, seed):
    """(store, model, alpha, A, end) of a tiny case: the stores of test_interval_gpu.py's first test."""
    rng = np.random.default_rng(1950 + seed)
    alpha = synth.HIFI_ALPHA if seed % 2 == 0 else np.zeros((4, 4))
    regions = [20, 31] if seed % 2 == 0 else [25]
    store = _tiny_store(rng, LENGTHS, regions)
    model = perturbed_model(store, model_type, 2 + seed % 3, alpha, rng)
    A, end = S.rows(store, model, alpha)
    return store, model, alpha, A, end


def tiny_jobs(store, seed):
    """Every a < b inside every chunk with a random disjoint mask pair, and all 12 ordered single-state pairs on the 40-window chunk."""
    rng = np.random.default_rng(77 + seed)
    off = np.asarray(store.chunk_off, np.int64)
    F, L, U, V = [], [], [], []
    for c in range(off.size - 1):
        for a in range(int(off[c]), int(off[c + 1])):
            for b in range(a + 1, int(off[c + 1])):
                u = int(rng.integers(1, 15))
                rest = [v for v in range(1, 16) if not (v & u)]
                F.append(a); L.append(b); U.append(u); V.append(int(rng.choice(rest)))
    t0, t1 = int(off[-2]), int(off[-1]) - 1
    for p in range(4):
        for q in range(4):
            if p != q:
                F.append(t0); L.append(t1); U.append(1 << p); V.append(1 << q)
    return tuple(np.array(x, np.int64) for x in (F, L, U, V))


def _same(x, y, tol=1e-10):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.isneginf(x) & np.isneginf(y)) | (np.abs(x - y) <= tol + 1e-9 * np.abs(y))
    return bool(np.all(ok))


@pytest.mark.parametrize("model_type,seed", TINY)
def test_masked_forward_equals_enumeration(model_type, seed):
    store, _, _, A, end = tiny(model_type, seed)
    off = np.asarray(store.chunk_off, np.int64)
    F, L, U, V = tiny_jobs(store, seed)
    n = 0
    for a, b, u, v in zip(F, L, U, V):
        c = BR.chunk_of(off, a)
        if off[c + 1] - off[c] > 7:
            continue
        assert _same(BR.masked_events(A, end, off, a, b, u, v), BR.brute_force(A, end, off, a, b, u, v)), (a, b, u, v)
        n += 1
    assert n == 21 + 10 + 15 + 3           # every pair of the chunks of 7, 5, 6 and 3 windows


@pytest.mark.parametrize("model_type,seed", TINY)
def test_recursion_equals_masked_forward(model_type, seed):
    store, _, _, A, end = tiny(model_type, seed)
    off = np.asarray(store.chunk_off, np.int64)
    F, L, U, V = tiny_jobs(store, seed)
    pick = np.concatenate([np.arange(0, F.size - 12, 7), np.arange(F.size - 12, F.size)])     # (route (i) costs a forward per k)
    got = BR.LongDouble(A, end, off).events(F[pick], L[pick], U[pick], V[pick])
    finite = 0
    for g, i in zip(got, pick):
        ref = BR.masked_events(A, end, off, F[i], L[i], U[i], V[i])
        assert _same(g, ref), (F[i], L[i], U[i], V[i])
        lpe, p = BR.summary(g)
        assert lpe <= 1e-12
        if np.isfinite(lpe):
            finite += 1
            assert abs(p.sum() - 1.0) < 1e-12
    assert finite >= pick.size // 2


def test_added_options_shadow_no_prefix_of_a_reference_option():
    """The rule of test_cli_prefix_cpu.py with every option this command line has added, --runBoundaries among them: `--b` stays the
    reference's shortest spelling of --binArrayFile."""
    ref = unique_prefixes(list(REFERENCE))
    now = dict(unique_prefixes(list(REFERENCE) + OWN))
    lost = [(p, n) for p, n in ref if now.get(p) != n]
    assert not lost, lost
    assert now.get("b") == "binArrayFile" and now.get("runB") == "runBoundaries"
    usage = subprocess.run([CLI, "--help"], capture_output=True, text=True).stderr
    for name in OWN:
        assert "--" + name in usage, name


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--sweepAlpha", "x"]])
def test_run_boundaries_refuses_before_the_input_is_read(extra, tmp_path):
    r = subprocess.run([CLI, "--runBoundaries"] + extra + ["-o", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0
    assert "--runBoundaries" in r.stderr and "one GPU" in r.stderr, r.stderr[-500:]


def test_python_surface():
    assert hasattr(hmm.EMList, "breakpoints") and hasattr(hmm.EMList, "breakpoint_profile") and hasattr(hmm, "EM_getBreakpointsForList")
    L = N.lib()
    assert L.hf_get_breakpoints.argtypes is not None and L.hf_get_breakpoint_profile.argtypes is not None


@pytest.mark.parametrize("spelling,option", [("--ru", "--runConfidence"), ("--run", "--runConfidence"), ("--runC", "--runConfidence"),
                                             ("--runB", "--runBoundaries")])
def test_prefixes_of_run_confidence_keep_their_meaning(spelling, option):
    """`--ru` and `--run` resolved to --runConfidence before --runBoundaries came, and still do (the rule of `--e` for --exchange)."""
    r = subprocess.run([CLI, spelling, "--gpus", "2"], capture_output=True, text=True)
    assert r.returncode != 0 and "ambiguous" not in r.stderr and "Error: " + option + " runs on one GPU" in r.stderr, r.stderr[-400:]
