"""CPU checks of the exact path entropy's ground: the two routes of the numpy reference (tests/entropy_ref.py: path enumeration (a),
log-partition minus expected log-weight in long double (b)) against one another, the chain-rule sums of the definition in float64 against
(b), the C ABI entry points (declared, exported, bound) and the command line's --jointEntropy option (help text, prefixes, refusals made
before the input is read).

The tolerance of the device tests is sized here: test_chain_rule_float64_against_long_double prints the largest deviation of the float64
chain-rule sums from route (b), in units of the device tolerance's own scale 1e-3 + |ref| (absolute 1e-12, relative 1e-9), over the jobs
of the tiny stores and of the reduced configs (see tests/test_entropy_gpu.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm
from test_cli_prefix_cpu import CLI, unique_prefixes
from test_interval_cpu import BUILD, NEW
from test_moments_cpu import REDUCED, TINY, reduced_case, tiny_case
import entropy_ref as ER
import sampling_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm_flagger_hip.h")

# the device tests' |dev - ref| <= ATOL + RTOL |ref|: the project's standing bound for posterior values
RTOL, ATOL = 1e-9, 1e-12
# every long option of the command line before --jointEntropy
EARLIER = list(BUILD) + list(NEW) + ["fitAlpha", "fitAlphaEntries", "fitAlphaMax", "fitAlphaEvery", "exactTotals", "numBlocks"]


def tiny_jobs(model_type, seed):
    """The store, model and jobs of the tiny-store tests (CPU and GPU): the ranges of the count-moments tests without their mask and
    region filter, and every sub-range of every small chunk, small chunks with their neighbours and all of them together."""
    store, model, alpha, (F, L, _, _) = tiny_case(model_type, seed)
    f2, l2 = ER.tiny_ranges(store.chunk_off)
    return store, model, alpha, (np.concatenate([F, f2]), np.concatenate([L, l2]))


def reduced_jobs(cfg, model_type, hifi, model=None):
    """The store, model and jobs of the reduced-config tests (CPU and GPU): moments_ref.jobs(..., piece=512, lane=8) with mask and
    region dropped."""
    store, model, alpha, (F, L, _, _) = reduced_case(cfg, model_type, hifi, model)
    return store, model, alpha, (F, L)


def deviation(got, ref):
    """The largest |got - ref| / (ATOL / RTOL + |ref|) over the jobs with a finite reference: 1 is the device tolerance over RTOL;
    -inf must agree exactly."""
    got, ref = np.asarray(got), np.asarray(ref)
    inf = np.isneginf(ref)
    assert np.array_equal(np.isneginf(got), inf)
    assert not np.any(np.isnan(got)) and not np.any(np.isnan(ref))
    return float(np.max(np.abs(got[~inf] - ref[~inf]) / (ATOL / RTOL + np.abs(ref[~inf])), initial=0.0))


@pytest.mark.parametrize("model_type,seed", TINY)
def test_two_routes_agree_on_tiny_stores(model_type, seed):
    store, model, alpha, (F, L) = tiny_jobs(model_type, seed)
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    assert list(np.diff(off)) == [7, 5, 1, 6, 3, 40]
    small = L < off[5]                                   # route (a) where it can go: the chunks of <= 7 windows
    assert small.sum() >= 28 + 15 + 1 + 21 + 6 + 5
    Fs, Ls = F[small], L[small]
    assert np.any((Fs < off[2]) & (Ls >= off[3]))        # a job over three chunks, the one-window chunk in the middle
    assert np.any((Fs == off[2]) & (Ls == off[2]))       # the one-window chunk alone
    ld = ER.LongDouble(A, end, off)
    ha, hb = ER.brute_force(A, end, off, Fs, Ls), ld.entropy(Fs, Ls)
    d = deviation(hb, ha)
    print("tiny store %d: entropy (b) against (a): %.3e of the device tolerance's scale, %d jobs" % (seed, d, Fs.size))
    assert d <= 1e-9 and np.all(ha >= -1e-12)              # (the enumeration's own rounding)
    assert np.sum(ha > 1e-3) >= 20
    ninf = 0
    for name, y in ER.labellings(A, end, off, 50 + seed):
        pa, pb = ER.brute_force(A, end, off, Fs, Ls, y), ld.log_probs(Fs, Ls, y)
        assert deviation(pb, pa) <= 1e-9, name
        assert np.all(pa <= 1e-12)
        ninf += int(np.isneginf(pa).sum())
    print("tiny store %d: impossible labellings among the jobs: %d" % (seed, ninf))


def test_chain_rule_float64_against_long_double():
    """Sizes the tolerance of the device tests: the largest deviation of the definition's chain-rule sums in float64 from route (b),
    relative to 1e-3 + |ref| (printed below); the device tolerance RTOL of that scale is at least a hundredfold of it, and at most 1e-9
    (the hundredfold is for the device's association order and its differently rounded rows and vectors).  The reference alone shows
    that the kernel is exercised: at least 20 jobs per reduced config have an entropy above 1e-3."""
    worst = 0.0
    cases = [(tiny_jobs(mt, seed), "tiny store %d" % seed, 50 + seed) for mt, seed in TINY]
    cases += [(reduced_jobs(cfg, mt, hifi), "cfg %d" % cfg, 60 + cfg) for cfg, mt, hifi in REDUCED]
    for (store, model, alpha, (F, L)), what, seed in cases:
        A, end = S.rows(store, model, alpha)
        off = np.asarray(store.chunk_off, np.int64)
        ld = ER.LongDouble(A, end, off)
        ref = ld.entropy(F, L)
        dev = deviation(ER.chain_rule(A, end, off, F, L), ref)
        whole = float(ld.entropy([0], [off[-1] - 1])[0])
        print("%s: entropy: max deviation %.3e; jobs with entropy > 1e-3: %d of %d; whole track %.1f nats" % (what, dev, int(np.sum(ref > 1e-3)), ref.size, whole))
        assert np.sum(ref > 1e-3) >= 20 and np.all(ref >= -1e-12)
        worst = max(worst, dev)
        marg, cond = ER.profile(A, end, off)
        assert np.all(cond >= 0) and np.all(cond <= marg + 1e-12)            # conditioning cannot raise entropy
        for name, y in ER.labellings(A, end, off, seed):
            lref = ld.log_probs(F, L, y)
            d = deviation(ER.chain_rule(A, end, off, F, L, y), lref)
            print("%s: log-probability of %s: max deviation %.3e, -inf in %d jobs" % (what, name, d, int(np.isneginf(lref).sum())))
            assert np.all(lref <= 1e-12)
            worst = max(worst, d)
    print("overall: %.3e" % worst)
    assert 100.0 * worst <= RTOL <= 1e-9


def test_declared_exported_and_bound():
    """The getters are declared in the public header, exported by the library and bound in _native and hmm."""
    text = open(HEADER).read()
    for name, nargs in (("hf_get_path_entropy", 5), ("hf_get_path_log_probs", 6), ("hf_get_entropy_profile", 5)):
        assert re.search(r"int\s+%s\s*\(\s*hf_ctx\s*\*\s*ctx\s*,\s*int64_t\s+" % name, text), name
        f = getattr(N.lib(), name)
        assert f.restype is not None and len(f.argtypes) == nargs, name
    assert re.search(r"hf_batch_\* and hf_multi_\* have no counterpart\. \*/\s*int hf_get_path_entropy", text)
    for m in ("path_entropy", "path_log_probs", "entropy_profile"):
        assert hasattr(hmm.EMList, m), m
    for f in ("EM_getPathEntropyForList", "EM_getPathLogProbsForList", "EM_getEntropyProfileForList"):
        assert hasattr(hmm, f), f


# ---- command line --------------------------------------------------------------------------------------------------------------
def test_help_names_the_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--jointEntropy" in r.stderr + r.stdout


def test_every_prefix_resolves_as_before(tmp_path):
    """No earlier option starts with "j": every prefix that resolved before resolves to the same option, and every prefix of
    --jointEntropy resolves to it (its refusal with --gpus 2 is what the command line complains about)."""
    def run(*args):
        r = subprocess.run([CLI, "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path)] + list(args), capture_output=True, text=True)
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and "undefined option" not in r.stderr, (args, r.stderr[-300:])
        return r.stderr
    for p in ("--j", "--joint", "--jointEntropy"):
        assert "--jointEntropy" in run(p, "--gpus", "2"), p
    for p in ("--n", "--numBlocks"):
        assert "--numBlocks" in run(p, "--gpus", "2"), p
    before = dict(unique_prefixes(EARLIER))
    now = dict(unique_prefixes(EARLIER + ["jointEntropy"]))
    assert {p: n for p, n in before.items() if now.get(p) != n} == {}
    assert all(now.get("jointEntropy"[:k]) == "jointEntropy" for k in range(1, 13))


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--sweepAlpha", "x"]])
def test_refused_combinations(tmp_path, extra):
    """Refused before the input is read and before any device use: the input named here does not exist, so only the refusal can be the
    error."""
    r = subprocess.run([CLI, "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--jointEntropy"] + extra,
                       capture_output=True, text=True)
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert r.returncode != 0
    assert len(lines) == 1 and "--jointEntropy" in lines[0], r.stderr[-500:]
