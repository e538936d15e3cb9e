"""CPU checks of the exact block-length spectrum's ground (hf_get_run_lengths): the float64 restatement of the device's formulation
(tests/runlen_ref.py route (c): the posterior chain Q, the start masses sigma, the stitch) against path enumeration (a) and the
long-double joint route (b) on the tiny stores, the reduced configs and the same with their chunks cut; the host's stitch
(flagger_amd/csrc/hf_runlen_stitch.h) as a stand-alone program under the sanitizers against (a); the C ABI entry point (declared,
exported, bound).  The command line's refusals are in tests/test_cli_runlengths_refusals_cpu.py.

The device tests' bound |dev - ref| <= ATOL + RTOL |ref| per bin is the standing one of the posterior and run-moment means (every bin
is a sum of non-negative terms on the scale of one per window); test_restated_against_the_other_routes prints the largest relative
deviation of (c) from (a) and (b), the formulation's own error, which must stay a hundredfold below it."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_bruteforce_cpu import _tiny_store
from test_moments_cpu import REDUCED, TINY, tiny_case
from test_runs_cpu import TINY_JOINS
from test_viterbi_cpu import perturbed_model
import runlen_ref as RL
import runs_ref as RR
import sampling_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flagger_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hmm_flagger_hip.h")
RTOL, ATOL = 1e-9, 1e-12
TINY_L = (1, 2, 3, 7, 39, 40, 64)      # T < L, T = L, T = L + 1 on the chunks of 1, 3, 6, 7 and 40 windows; saturation across a join


def close(got, ref):
    return np.abs(got - ref) <= ATOL + RTOL * np.abs(ref)


def deviation(got, ref):
    """(largest absolute, largest relative over the bins above 1e-3) deviation."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    big = ref > 1e-3
    return float(np.max(np.abs(got - ref), initial=0.0)), float(np.max(np.abs(got - ref)[big] / ref[big], initial=0.0))


def tiny_ranges(off):
    """The ranges of the tiny-store tests: every small chunk, every sub-range of the 5-window chunk, the five small chunks together, the
    40-window chunk, the whole track; each with every mask (tiny_jobs)."""
    first = [off[c] for c in range(5)] + [0, off[5], 0] + [a for a in range(off[1], off[2]) for b in range(a, off[2])]
    last = [off[c + 1] - 1 for c in range(5)] + [off[5] - 1, off[6] - 1, off[6] - 1] + [b for a in range(off[1], off[2]) for b in range(a, off[2])]
    return np.array(first, np.int64), np.array(last, np.int64)


def tiny_jobs(model_type, seed):
    store, model, alpha, _ = tiny_case(model_type, seed)
    off = np.asarray(store.chunk_off, np.int64)
    assert list(np.diff(off)) == [7, 5, 1, 6, 3, 40]
    f, l = tiny_ranges(off)
    r, m = (x.ravel() for x in np.meshgrid(np.arange(f.size), np.arange(1, 16), indexing="ij"))
    return store, model, alpha, (f[r], l[r], m)


_TINY_REF = {}


def tiny_reference(model_type, seed, joined, L):
    """float64[n][L + 1] for tiny_jobs: route (a) where every group of the job can be enumerated, route (b) elsewhere; and which."""
    key = (model_type, seed, joined, L)
    if key not in _TINY_REF:
        store, model, alpha, (F, La, M) = tiny_jobs(model_type, seed)
        A, end = S.rows(store, model, alpha)
        joins = TINY_JOINS if joined else None
        ref = np.asarray(RL.joint(A, end, store.chunk_off, F, La, M, L, joins), np.float64)
        small = RL.groups_fit_enumeration(store.chunk_off, F, La, joins)
        ref[small] = RL.brute_force(A, end, store.chunk_off, F[small], La[small], M[small], L, joins)
        ref.setflags(write=False)
        _TINY_REF[key] = (ref, small)
    return _TINY_REF[key]


def range_jobs(off, rng, n_random, spans=(4, 64, 700, 3000)):
    """Jobs of a larger store: random ranges of the given lengths (they cross chunk boundaries), every chunk-aligned start among them,
    two whole-track ranges; random masks, the single labels and Err+Dup+Col among them."""
    off = np.asarray(off, np.int64)
    n = int(off[-1])
    span = rng.choice(spans, n_random)
    f = rng.integers(0, n, n_random)
    f[::5] = off[rng.integers(0, off.size - 1, f[::5].size)]
    l = np.minimum(n - 1, f + rng.integers(0, span) )
    f = np.concatenate([f, [0, 0]]); l = np.concatenate([l, [n - 1, n - 1]])
    m = rng.choice([1, 2, 4, 8, 11, 3, 5, 6, 12, 15], f.size)
    m[-2:] = (11, 4)
    return f.astype(np.int64), l.astype(np.int64), m.astype(np.int64)


def reduced_store(cfg, model_type, hifi, split, model=None):
    store = synth.config(cfg, 0.04)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    if model is None:
        model = perturbed_model(store, model_type, 3, alpha, np.random.default_rng(cfg))
    if split:
        store = RR.split_store(store)
    return store, model, alpha, range_jobs(store.chunk_off, np.random.default_rng(4100 + cfg + (50 if split else 0)), 60)


def test_restated_against_the_other_routes():
    """Route (c) against (a) and (b): the tiny stores apart and with TINY_JOINS at every L of the device tests, the reduced configs as they
    are and cut at L = 5 and 64.  Prints the largest deviations; the relative one is the number in DESIGN.md 7q and in the docstring of
    tests/test_runlen_gpu.py."""
    worst = 0.0
    for mt, seed in TINY:
        store, model, alpha, (F, La, M) = tiny_jobs(mt, seed)
        A, end = S.rows(store, model, alpha)
        rs = RL.Restated(A, end, store.chunk_off)
        for joined in (False, True):
            for L in TINY_L:
                ref, small = tiny_reference(mt, seed, joined, L)
                assert small.sum() >= 15 * 20 and (~small).sum() >= 15 * 2
                got = rs.spectrum(F, La, M, L, TINY_JOINS if joined else None)
                # (a) and (b) agree where both apply
                both = np.asarray(RL.joint(A, end, store.chunk_off, F[small], La[small], M[small], L, TINY_JOINS if joined else None), np.float64)
                assert np.all(close(both, ref[small]))
                a, r = deviation(got, ref)
                assert np.all(close(got, ref)), (seed, joined, L, a, r)
                assert np.sum(ref > 1e-3) >= 20
                worst = max(worst, r)
        print("tiny store %d: max relative deviation so far %.3e" % (seed, worst))
    for cfg, mt, hifi in REDUCED:
        for split in (False, True):
            store, model, alpha, (F, La, M) = reduced_store(cfg, mt, hifi, split)
            A, end = S.rows(store, model, alpha)
            joins = RR.contig_joins(store)
            assert joins.sum() >= (40 if split else 0)
            jt, rs = RL.Joint(A, end, store.chunk_off), RL.Restated(A, end, store.chunk_off)
            for L in (5, 64):
                ref = np.asarray(jt.spectrum(F, La, M, L, joins), np.float64)
                got = rs.spectrum(F, La, M, L, joins)
                a, r = deviation(got, ref)
                print("cfg %d%s L %d: max abs %.3e, max relative %.3e, bins above 1e-3: %d" % (cfg, " cut" if split else "", L, a, r, int(np.sum(ref > 1e-3))))
                assert np.all(close(got, ref)) and np.sum(ref > 1e-3) >= 20
                worst = max(worst, r)
                if split and L == 64:                     # the joins matter to the jobs that span them
                    apart = rs.spectrum(F, La, M, L, None)
                    assert np.sum(np.abs(apart - got) > 1e-3) >= 20
    print("overall: max relative deviation %.3e" % worst)
    assert 100.0 * worst <= RTOL


def test_sum_of_the_bins_is_the_expected_number_of_runs():
    """Two identities of the reference alone: the bins add up to the expected number of runs (runs_ref), and with L at least the longest
    group sum l N_l is the expected number of windows in S."""
    mt, seed = TINY[0]
    store, model, alpha, (F, La, M) = tiny_jobs(mt, seed)
    A, end = S.rows(store, model, alpha)
    for joins in (None, TINY_JOINS):
        mean, _, _ = RR.jet_long(A, end, store.chunk_off, F, La, M, joins)
        spec = RL.restated(A, end, store.chunk_off, F, La, M, 64, joins)
        assert np.allclose(spec.sum(axis=1), mean, rtol=1e-11, atol=1e-12)
        al, be = RR.alpha_beta(A, end, store.chunk_off)
        g = al * be
        g /= g.sum(axis=1, keepdims=True)
        inS = ((M[:, None] >> np.arange(4)) & 1).astype(bool)
        windows = np.array([(g[f:l + 1] * inS[j]).sum() for j, (f, l) in enumerate(zip(F, La))])
        assert np.all(spec[:, 64] == 0.0)
        assert np.allclose((spec[:, :64] * np.arange(1, 65)).sum(axis=1), windows, rtol=1e-11, atol=1e-12)


# ---- the stitch as a stand-alone program -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program():
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx) or not shutil.which("make"):
        pytest.skip("no host compiler")
    subprocess.run(["make", "-s", "-C", CSRC, "runlen_check", "CXX=" + cxx], check=True)
    return os.path.join(CSRC, "runlen_check")


def test_stitch_program_against_enumeration(program):
    """Groups of 1-4 parts of 1-4 windows, L = 1..6 (T = L and T = L + 1 and a one-window part inside a group among them): the parts'
    records of route (c) through the compiled stitch, against the enumerated paths of the group."""
    rng = np.random.default_rng(77)
    lengths = [int(x) for x in rng.integers(1, 5, 40)]
    lengths[5:9] = [3, 1, 4, 2]                                           # a one-window part inside a group
    store = _tiny_store(rng, lengths, [20, 31])
    model = perturbed_model(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, rng)
    A, end = S.rows(store, model, synth.HIFI_ALPHA)
    off = np.asarray(store.chunk_off, np.int64)
    rs = RL.Restated(A, end, off)
    groups = []                                                          # (first chunk, chunks, mask)
    c = 0
    while c < len(lengths):
        k = min(int(rng.integers(1, 5)), len(lengths) - c)
        if sum(lengths[c:c + k]) <= 10:
            groups.append((c, k, int(rng.integers(1, 16))))
        c += k
    groups.append((5, 4, 7))
    assert len(groups) >= 10 and {k for _, k, _ in groups} == {1, 2, 3, 4}
    worst = 0.0
    for L in range(1, 7):
        text = ["%d %d" % (L, len(groups))]
        ref = []
        for c0, k, mask in groups:
            joined = np.zeros(len(lengths), bool)
            joined[c0 + 1:c0 + k] = True
            ref.append(RL.brute_force(A, end, off, [off[c0]], [off[c0 + k] - 1], [mask], L, joined)[0])
            text.append(str(k))
            for c in range(c0, c0 + k):
                I, Lc, Rc, W, s, e = rs.part(int(off[c]), int(off[c + 1]) - 1, RL._bits(mask), L)
                text.append("%d %s" % (lengths[c], " ".join(repr(float(x)) for x in list(I) + list(Lc) + list(Rc) + [W, s, e])))
        if L <= 3:                                            # parts of exactly L and of L + 1 windows
            assert {L, L + 1} <= {lengths[c0 + i] for c0, k, _ in groups for i in range(k)}
        r = subprocess.run([program], input="\n".join(text) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]           # (a sanitizer report ends the program with an error)
        got = np.array(r.stdout.split(), np.float64).reshape(len(groups), L + 1)
        ref = np.array(ref)
        assert np.all(close(got, ref)), (L, deviation(got, ref))
        assert np.all(got >= 0.0)
        worst = max(worst, deviation(got, ref)[0])
    print("stitch program: max absolute deviation %.3e" % worst)


def test_declared_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"int\s+hf_get_run_lengths\s*\(\s*hf_ctx\s*\*\s*ctx\s*,\s*int64_t\s+n\s*,", text)
    assert re.search(r"#define\s+HF_RUN_LENGTHS_MAX\s+64", text)
    f = getattr(N.lib(), "hf_get_run_lengths")
    assert f.restype is not None and len(f.argtypes) == 8
    assert hasattr(hmm.EMList, "run_lengths") and hasattr(hmm, "EM_getRunLengthsForList")
