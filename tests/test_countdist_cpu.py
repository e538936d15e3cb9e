"""CPU checks of the ground of the exact distribution of label totals (hf_get_count_distribution): the float64 restatement of the
device's formulation (tests/countdist_ref.py route (c): the posterior chain Q, the pieces' transfers, the chain's truncated
convolutions, the stitch) against path enumeration (a) and the long-double joint route (b) on the tiny stores, with the piece grid cut
inside their chunks, and on the reduced configs whole and cut; the host's stitch (flagger_amd/csrc/hf_countdist_stitch.h) as a
stand-alone program under the sanitizers against (a); the C ABI entry point (declared, exported, bound).  The command line's refusals
are in tests/test_cli_totals_refusals_cpu.py.

The device tests' bound |dev - ref| <= ATOL + RTOL |ref| per bin is the standing one of the posterior sums of non-negative terms
(DESIGN.md 7q); test_restated_against_the_other_routes prints the largest relative deviation of (c) from (a) and (b) over the bins
above 1e-3, the formulation's own error, which must stay a hundredfold below it."""
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
from test_runlen_cpu import ATOL, RTOL, close, deviation, range_jobs, tiny_ranges
from test_viterbi_cpu import perturbed_model
import countdist_ref as CD
import runs_ref as RR
import sampling_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flagger_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hmm_flagger_hip.h")
TINY_K = (1, 2, 3, 7, 61, 62)         # with jobs of 1, 2, K and K + 1 windows (K = 62: the whole track has 62; 63 is in the device tests)


def tiny_jobs(model_type, seed):
    """tiny_ranges of the block-length tests (every small chunk, every sub-range of the 5-window chunk, the five small chunks together,
    the 40-window chunk, the whole track) and ranges of 1, 2, 3, 4, 7, 8, 39 windows at the head of the 40-window chunk, of 2, 3, 4, 8
    windows across the first chunk boundaries, of 61 windows at either end of the track; each with every mask."""
    store, model, alpha, _ = tiny_case(model_type, seed)
    off = np.asarray(store.chunk_off, np.int64)
    assert list(np.diff(off)) == [7, 5, 1, 6, 3, 40] and off[-1] == 62
    f, l = tiny_ranges(off)
    head = [1, 2, 3, 4, 7, 8, 39]
    across = [2, 3, 4, 8]
    f = np.concatenate([f, [off[5]] * len(head), [5] * len(across), [0, 1]])
    l = np.concatenate([l, [off[5] + t - 1 for t in head], [5 + t - 1 for t in across], [60, 61]])
    r, m = (x.ravel() for x in np.meshgrid(np.arange(f.size), np.arange(1, 16), indexing="ij"))
    return store, model, alpha, (f[r].astype(np.int64), l[r].astype(np.int64), m.astype(np.int64))


_TINY_REF = {}


def tiny_reference(model_type, seed, K):
    """float64[n][K + 2] for tiny_jobs: route (a) where the job can be enumerated, route (b) elsewhere; and which."""
    key = (model_type, seed, K)
    if key not in _TINY_REF:
        store, model, alpha, (F, La, M) = tiny_jobs(model_type, seed)
        A, end = S.rows(store, model, alpha)
        ref = np.asarray(CD.joint(A, end, store.chunk_off, F, La, M, K), np.float64)
        small = CD.fits_enumeration(store.chunk_off, F, La)
        ref[small] = CD.brute_force(A, end, store.chunk_off, F[small], La[small], M[small], K)
        ref.setflags(write=False)
        _TINY_REF[key] = (ref, small)
    return _TINY_REF[key]


def reduced_jobs(store, seed):
    """Jobs of a reduced config: 40 random ranges of up to 4, 64, 700 and 2000 windows (they cross chunk boundaries and the 512 grid),
    ranges of exactly 62 and 63 windows, one whole-track range; random masks."""
    F, La, M = range_jobs(store.chunk_off, np.random.default_rng(seed), 40, spans=(4, 64, 700, 2000))
    F, La, M = F[:-1], La[:-1], M[:-1]                                     # (one whole-track range: Err+Dup+Col)
    n = int(store.chunk_off[-1])
    F = np.concatenate([F, [100, 100, n - 63, 511, 450]]); La = np.concatenate([La, [161, 162, n - 1, 572, 512]])
    M = np.concatenate([M, [11, 11, 4, 3, 15]])
    return F.astype(np.int64), La.astype(np.int64), M.astype(np.int64)


def reduced_store(cfg, model_type, hifi, split):
    store = synth.config(cfg, 0.04)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    model = perturbed_model(store, model_type, 3, alpha, np.random.default_rng(cfg))
    if split:
        store = RR.split_store(store)
    return store, model, alpha, reduced_jobs(store, 5100 + cfg + (50 if split else 0))


def test_restated_against_the_other_routes(monkeypatch):
    """Route (c) against (a) and (b): the tiny stores at every K of the device tests, the same with the piece grid at 5 windows (cuts
    inside the chunks), the reduced configs as they are at K = 5 and cut at K = 62.  Prints the largest deviations; the relative one is the
    number in DESIGN.md 7r and in the docstring of tests/test_countdist_gpu.py."""
    worst = 0.0
    for mt, seed in TINY:
        store, model, alpha, (F, La, M) = tiny_jobs(mt, seed)
        A, end = S.rows(store, model, alpha)
        rs = CD.Restated(A, end, store.chunk_off)
        for K in TINY_K:
            ref, small = tiny_reference(mt, seed, K)
            assert small.sum() >= 15 * 20 and (~small).sum() >= 15 * 5
            both = np.asarray(CD.joint(A, end, store.chunk_off, F[small], La[small], M[small], K), np.float64)
            assert np.all(close(both, ref[small]))                         # (a) and (b) agree where both apply
            for grid in (512, 5):
                monkeypatch.setattr(CD, "GRID", grid)
                got = rs.distribution(F, La, M, K)
                a, r = deviation(got, ref)
                assert np.all(close(got, ref)), (seed, K, grid, a, r)
                assert np.all(got >= 0.0) and np.sum(ref > 1e-3) >= 20
                worst = max(worst, r)
        print("tiny store %d: max relative deviation so far %.3e" % (seed, worst))
    monkeypatch.setattr(CD, "GRID", 512)
    for cfg, mt, hifi in REDUCED:
        for split in (False, True):
            store, model, alpha, (F, La, M) = reduced_store(cfg, mt, hifi, split)
            A, end = S.rows(store, model, alpha)
            jt, rs = CD.Joint(A, end, store.chunk_off), CD.Restated(A, end, store.chunk_off)
            for K in ((62,) if split else (5,)):
                ref = np.asarray(jt.distribution(F, La, M, K), np.float64)
                got = rs.distribution(F, La, M, K)
                a, r = deviation(got, ref)
                print("cfg %d%s K %d: max abs %.3e, max relative %.3e, bins above 1e-3: %d" % (cfg, " cut" if split else "", K, a, r, int(np.sum(ref > 1e-3))))
                assert np.all(close(got, ref)) and np.sum(ref > 1e-3) >= 20
                worst = max(worst, r)
    print("overall: max relative deviation %.3e" % worst)
    assert 100.0 * worst <= RTOL


def test_identities_of_the_reference():
    """The reference alone: the bins add up to 1; the mean of the bins is the sum of the posteriors; bin 0 and bin T are the interval
    probabilities of the complement and of S; S and its complement mirror each other (all for jobs of at most K windows); the exact
    zeros of the header."""
    mt, seed = TINY[0]
    store, model, alpha, (F, La, M) = tiny_jobs(mt, seed)
    A, end = S.rows(store, model, alpha)
    K = 62
    d = CD.restated(A, end, store.chunk_off, F, La, M, K)
    T = La - F + 1
    assert np.allclose(d.sum(axis=1), 1.0, rtol=0, atol=1e-13)
    al, be = RR.alpha_beta(A, end, store.chunk_off)
    g = al * be
    g /= g.sum(axis=1, keepdims=True)
    inS = ((M[:, None] >> np.arange(4)) & 1).astype(bool)
    windows = np.array([(g[f:l + 1] * inS[j]).sum() for j, (f, l) in enumerate(zip(F, La))])
    assert np.allclose((d[:, :K + 1] * np.arange(K + 1)).sum(axis=1), windows, rtol=1e-11, atol=1e-12)
    assert np.all(d[:, K + 1] == 0.0)
    for j in range(F.size):
        assert np.all(d[j, T[j] + 1:] == 0.0)
        if M[j] == 15:
            assert d[j, T[j]] == pytest.approx(1.0, abs=1e-13) and np.all(np.delete(d[j], T[j]) == 0.0)
    sel = M != 15
    mirror = CD.restated(A, end, store.chunk_off, F[sel], La[sel], 15 - M[sel], K)
    for row, back, t in zip(d[sel], mirror, T[sel]):
        assert np.allclose(row[:t + 1], back[:t + 1][::-1], rtol=1e-11, atol=1e-13)
    # K below the total: the bins up to K stay, the rest is gathered
    for k in (1, 3, 7):
        low = CD.restated(A, end, store.chunk_off, F, La, M, k)
        assert np.allclose(low[:, :k + 1], d[:, :k + 1], rtol=1e-12, atol=1e-15)
        assert np.allclose(low[:, k + 1], d[:, k + 1:].sum(axis=1), rtol=1e-11, atol=1e-13)
        assert np.all(low[T <= k, k + 1] == 0.0) and np.any(low[T == k + 1, k + 1] > 1e-3)


# ---- the stitch as a stand-alone program -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program():
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx) or not shutil.which("make"):
        pytest.skip("no host compiler")
    subprocess.run(["make", "-s", "-C", CSRC, "countdist_check", "CXX=" + cxx], check=True)
    return os.path.join(CSRC, "countdist_check")


def test_stitch_program_against_enumeration(program):
    """Jobs of 1-4 parts of 1-4 windows, K = 1..6 (K below, at and above the job's total): the parts' distributions of route (c) through
    the compiled stitch, against the enumerated paths of the job; bitwise the Python restatement of the stitch."""
    rng = np.random.default_rng(78)
    lengths = [int(x) for x in rng.integers(1, 5, 40)]
    lengths[5:9] = [3, 1, 4, 2]                                           # a one-window part inside a job
    store = _tiny_store(rng, lengths, [20, 31])
    model = perturbed_model(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, rng)
    A, end = S.rows(store, model, synth.HIFI_ALPHA)
    off = np.asarray(store.chunk_off, np.int64)
    rs = CD.Restated(A, end, off)
    jobs = []                                                            # (first chunk, chunks, mask)
    c = 0
    while c < len(lengths):
        k = min(int(rng.integers(1, 5)), len(lengths) - c)
        if sum(lengths[c:c + k]) <= 10:
            jobs.append((c, k, int(rng.integers(1, 16))))
        c += k
    three = next(c for c in range(12, 37) if sum(lengths[c:c + 3]) <= 10)
    jobs += [(5, 4, 7), (5, 4, 15), (three, 3, 9)]
    assert len(jobs) >= 10 and {k for _, k, _ in jobs} == {1, 2, 3, 4}
    totals = np.array([sum(lengths[c0:c0 + k]) for c0, k, _ in jobs])
    worst = 0.0
    for K in range(1, 7):
        assert np.any(totals < K) or K == 1
        assert np.any(totals == K) and np.any(totals == K + 1) and np.any(totals > K + 1)
        text = ["%d %d" % (K, len(jobs))]
        ref, py = [], []
        for c0, k, mask in jobs:
            ref.append(CD.brute_force(A, end, off, [off[c0]], [off[c0 + k] - 1], [mask], K)[0])
            text.append(str(k))
            parts = [rs.part(int(off[c]), int(off[c + 1]) - 1, CD._bits(mask), K) for c in range(c0, c0 + k)]
            text += [" ".join(repr(float(x)) for x in d) for d in parts]
            py.append(CD.stitch(parts, K))
        r = subprocess.run([program], input="\n".join(text) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]           # (a sanitizer report ends the program with an error)
        got = np.array(r.stdout.split(), np.float64).reshape(len(jobs), K + 2)
        ref = np.array(ref)
        assert np.all(close(got, ref)), (K, deviation(got, ref))
        assert np.array_equal(got, np.array(py))
        assert np.all(got >= 0.0)
        assert np.all(got[totals <= K, K + 1] == 0.0) and np.any(got[totals == K + 1, K + 1] > 1e-3)
        for row, t, (_, _, mask) in zip(got, totals, jobs):
            assert np.all(row[t + 1:] == 0.0)
            if mask == 15:
                assert np.all(np.delete(row, min(t, K + 1)) == 0.0)
        worst = max(worst, deviation(got, ref)[0])
    # a job without a part: N = 0
    r = subprocess.run([program], input="3 1\n0\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["1", "0", "0", "0", "0"]
    print("stitch program: max absolute deviation %.3e" % worst)


def test_declared_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"int\s+hf_get_count_distribution\s*\(\s*hf_ctx\s*\*\s*ctx\s*,\s*int64_t\s+n\s*,", text)
    assert re.search(r"#define\s+HF_COUNT_DIST_MAX\s+62", text)
    f = getattr(N.lib(), "hf_get_count_distribution")
    assert f.restype is not None and len(f.argtypes) == 7
    assert hasattr(hmm.EMList, "count_distribution") and hasattr(hmm, "EM_getCountDistributionForList")
    assert not any(hasattr(N.lib(), n) for n in ("hf_batch_get_count_distribution", "hf_multi_get_count_distribution"))
