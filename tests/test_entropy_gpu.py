"""Exact path entropy and labelling log-probability on the GPU (hf_get_path_entropy, hf_get_path_log_probs, hf_get_entropy_profile,
hmm.EMList.path_entropy / path_log_probs / entropy_profile, hmm_flagger --jointEntropy) against the numpy reference
(tests/entropy_ref.py), which forms them by other routes: path enumeration (a) on the chunks of at most 7 windows, log-partition minus
expected log-weight in long double (b) everywhere.

Tolerance: |dev - ref| <= 1e-12 + 1e-9 |ref|, the project's standing bound for posterior values and for the means of the moment getters;
-inf must agree exactly.  tests/test_entropy_cpu.py::test_chain_rule_float64_against_long_double measures the float64 chain-rule sums of
the definition against (b) on the same jobs: 9.7e-13 of the scale 1e-3 + |ref| at most, a thousandth of this bound.
Every test prints its largest absolute and relative deviations before it asserts (pytest -s).  Measured on an MI355X (both algorithms,
the largest over the cases; relative: over the values with |ref| > 1e-3):
    tiny stores       entropy 1.8e-15 absolute, 3.8e-13 relative; log-probabilities 4.5e-13 absolute, 4.9e-13 relative
    reduced configs   entropy 1.1e-13 absolute, 2.3e-13 relative; log-probabilities 1.5e-11 absolute (a constant path over the whole track,
                      log p = -4.1e4: 3.6e-16 relative), 8.8e-13 relative; whole-track entropies of the trained models 196.0, 170.9 and
                      1010.0 nats on configs 2, 4 and 6, and 390, 426 and 462 of 544 jobs with an entropy above 1e-3
    identities        one window against hf_get_posterior 1.4e-14 absolute; a constant label against hf_get_interval_log_probs 9.1e-13
                      absolute, 1.3e-12 relative, -inf in the same 1 226 jobs; entropy against the profile's sums 3.6e-15 absolute"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_entropy_cpu import ATOL, RTOL, reduced_jobs, tiny_jobs
from test_moments_cpu import REDUCED, TINY
from test_runs_gpu import _trained_model
import entropy_ref as ER
import interval_ref as IR
import runs_ref as RR
import sampling_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]


def _tol(ref):
    return ATOL + RTOL * np.abs(ref)


def _close(dev, ref, what):
    """Prints the largest absolute and relative deviation, then asserts the tolerance; -inf must agree exactly, nothing may be NaN."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    assert dev.shape == ref.shape
    assert not np.any(np.isnan(dev)), what
    inf = np.isneginf(ref)
    fin = ~inf
    err = np.abs(dev[fin] - ref[fin])
    big = np.abs(ref[fin]) > 1e-3
    print("%s: max |dev - ref| %.3e, max relative deviation (|ref| > 1e-3) %.3e over %d values, -inf in %d"
          % (what, float(np.max(err, initial=0.0)), float(np.max(err[big] / np.abs(ref[fin][big]), initial=0.0)), int(big.sum()), int(inf.sum())))
    assert np.array_equal(np.isneginf(dev), inf), what
    bad = np.flatnonzero(~(err <= _tol(ref[fin])))
    assert bad.size == 0, (what, [(int(i), float(dev[fin][i]), float(ref[fin][i])) for i in bad[:8]])


def _pass(store, model, algo=N.HF_ALGO_SCAN):
    em = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model)            # the pass whose model the getters answer for
    return em


# ---- 1. tiny stores ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_reference(model_type, seed):
    """The references of a tiny case, once for both algorithms: (b) for every job, (a) for the jobs inside the chunks of <= 7 windows."""
    store, model, alpha, (F, L) = tiny_jobs(model_type, seed)
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    small = L < off[5]
    ld = ER.LongDouble(A, end, off)
    labs = ER.labellings(A, end, off, 50 + seed)
    ent = (ld.entropy(F, L), ER.brute_force(A, end, off, F[small], L[small]))
    lps = [(name, y, ld.log_probs(F, L, y), ER.brute_force(A, end, off, F[small], L[small], y)) for name, y in labs]
    return small, ent, lps


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed", TINY)
def test_tiny_stores_equal_reference(algo, model_type, seed):
    store, model, alpha, (F, L) = tiny_jobs(model_type, seed)
    off = np.asarray(store.chunk_off, np.int64)
    assert list(np.diff(off)) == [7, 5, 1, 6, 3, 40]
    assert np.any((F == off[2]) & (L == off[2]))                       # the one-window chunk
    assert np.any((F < off[2]) & (L >= off[3]))                        # a job over three chunks
    assert np.any((F == L) & (F > off[5])) and np.any(L == off[6] - 1)
    small, (hb, ha), lps = _tiny_reference(model_type, seed)
    em = _pass(store, model, algo)
    h = em.path_entropy(F, L)
    _close(h, hb, "tiny %d entropy against (b)" % seed)
    _close(h[small], ha, "tiny %d entropy against (a)" % seed)
    assert np.all(h >= 0.0) and np.sum(h > 1e-3) >= 20
    for name, y, lb, la in lps:
        lp = em.path_log_probs(F, L, y)
        _close(lp, lb, "tiny %d log-probability of %s against (b)" % (seed, name))
        _close(lp[small], la, "tiny %d log-probability of %s against (a)" % (seed, name))
        assert np.all(lp <= 0.0)
    em.close()


# ---- 2. reduced configs --------------------------------------------------------------------------------------------------------------
def _reduced_model(cfg):
    """Store, trained model (as test_runs_gpu trains it), alpha and jobs of a reduced config."""
    mt, hifi = next((m, h) for c, m, h in REDUCED if c == cfg)
    return reduced_jobs(cfg, mt, hifi, _trained_model(cfg))


@functools.lru_cache(maxsize=None)
def _reduced(cfg):
    """Store, trained model, jobs, reference (b) and labellings of a reduced config, once for every test that uses it (nothing here is
    changed later: a pass with the model writes its estimators only)."""
    store, model, alpha, (F, L) = _reduced_model(cfg)
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    ld = ER.LongDouble(A, end, off)
    ent = ld.entropy(F, L)
    lps = [(name, y, ld.log_probs(F, L, y)) for name, y in ER.labellings(A, end, off, 60 + cfg)]
    return store, model, (F, L), ent, lps


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("cfg", [c for c, _, _ in REDUCED])
def test_reduced_configs_equal_reference(algo, cfg):
    store, model, (F, L), ent, lps = _reduced(cfg)
    off = np.asarray(store.chunk_off, np.int64)
    assert store.n_windows == {2: 61120, 4: 30568, 6: 61120}[cfg] and off.size - 1 == 46
    assert np.diff(off).max() > 2 * 512 + 16
    assert np.any((F % 512 == 0) & (L > F)) and np.any((F % 512 == 511) & (L > F))
    print("cfg %d: jobs with entropy > 1e-3 in the reference: %d of %d, whole track %.3f nats" % (cfg, int(np.sum(ent > 1e-3)), ent.size, ent[0]))
    assert np.sum(ent > 1e-3) >= 20                          # the trained model leaves enough uncertain jobs
    em = _pass(store, model, algo)
    h = hmm.EM_getPathEntropyForList(em, F, L)
    _close(h, ent, "cfg %d entropy" % cfg)
    assert np.all(h >= 0.0) and np.sum(h > 1e-3) >= 20
    kinds = set()
    for name, y, ref in lps:
        lp = hmm.EM_getPathLogProbsForList(em, F, L, y)
        _close(lp, ref, "cfg %d log-probability of %s" % (cfg, name))
        assert np.all(lp <= 0.0)
        kinds.add(name.split()[0])
    assert kinds == {"viterbi", "drawn", "constant"}
    em.close()


# ---- 3. identities against what the device already answers ------------------------------------------------------------------------------
def test_identities_against_the_other_getters():
    store, model, (F, L), ent, _ = _reduced(2)
    off = np.asarray(store.chunk_off, np.int64)
    n = store.n_windows
    em = _pass(store, model)
    post = em.posterior()
    rng = np.random.default_rng(17)
    # one-window jobs
    w = np.concatenate([rng.integers(0, n, 300), off[:-1], off[1:] - 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        lg = np.where(post > 0, np.log(np.where(post > 0, post, 1.0)), -np.inf)
        hw = -np.where(post > 0, post * lg, 0.0).sum(axis=1)
    _close(em.path_entropy(w, w), hw[w], "one-window entropy against the posterior")
    y = rng.integers(0, 4, n)
    _close(em.path_log_probs(w, w, y), lg[w, y[w]], "one-window log-probability against the posterior")
    # a constant label against the interval getter: the ranges of the job set cross piece and chunk boundaries
    spans = np.array([np.searchsorted(off, a, "right") != np.searchsorted(off, b, "right") for a, b in zip(F, L)])
    cross = (F // 512 != L // 512)
    assert spans.sum() >= 20 and cross.sum() >= 20
    ninf = 0
    for k in range(4):
        lp = em.path_log_probs(F, L, np.full(n, k))
        iv = em.interval_log_probs(F, L, 1 << k)
        _close(lp, iv, "constant label %d against hf_get_interval_log_probs" % k)
        ninf += int(np.isneginf(lp).sum())
    print("constant labels: -inf in %d jobs" % ninf)
    # the profile
    marg, cond = em.entropy_profile()
    h = em.path_entropy(F, L)
    J, Cc, pa, pb, _ = IR.split(off, F, L, np.ones(F.size, np.int64))
    want = np.zeros(F.size)
    for j, a, b in zip(J, pa, pb):
        want[j] += marg[a] + cond[a + 1:b + 1].sum()
    _close(h, want, "entropy against the profile's sums")
    firstw = off[:-1][np.diff(off) > 0]
    assert np.array_equal(cond[firstw], marg[firstw])
    assert np.all(cond >= 0.0) and np.all(cond <= marg + 1e-12)
    _close(marg, hw, "profile's marg against the posterior")
    assert np.array_equal(em.entropy_profile(100, 700)[1], cond[100:800]) and np.array_equal(em.entropy_profile(n - 5)[0], marg[n - 5:])
    cm = np.concatenate([[0.0], np.cumsum(marg)])
    msum = cm[L + 1] - cm[F]
    print("path entropy over the sum of window entropies: whole track %.3f of %.3f nats" % (h[0], msum[0]))
    assert np.all(h <= msum + _tol(msum) + 1e-16 * (L - F + 1))
    assert h[0] < msum[0]                               # the chain's correlations matter
    # the most probable path is at least as probable as any other, chunk by chunk
    vit, _, _ = em.viterbi(model)
    labels = em.labels()
    assert labels.min() >= 0 and labels.max() <= 3
    cf, cl = off[:-1], off[1:] - 1
    lv = em.path_log_probs(cf, cl, vit)
    assert np.all(np.isfinite(lv))
    others = [("posterior labels", labels)] + [("sample %d" % k, p) for k, p in enumerate(em.sample_paths(model, 8, 3))]
    for name, p in others:
        lo = em.path_log_probs(cf, cl, p)
        assert np.all(lo <= lv + _tol(lv)), name
    print("whole-chunk log-probabilities: viterbi %.3f, posterior labels %.3f (sums over the chunks)" % (lv.sum(), em.path_log_probs(cf, cl, labels).sum()))
    em.close()


# ---- 4. a job depends on nothing but itself ----------------------------------------------------------------------------------------------
def _both(em, F, L, y):
    return em.path_entropy(F, L), em.path_log_probs(F, L, y)


def _same(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def test_bitwise_independence_of_the_call():
    store, model, (F, L), ent, lps = _reduced(2)
    y = lps[1][1]                                        # a drawn path: finite everywhere
    assert lps[1][0].startswith("drawn")
    em = _pass(store, model)
    rng = np.random.default_rng(5)
    base = _both(em, F, L, y)
    assert np.sum(base[0] > 1e-3) >= 20 and np.all(np.isfinite(base[1]))
    assert _same(_both(em, F, L, y), base)                                                        # two consecutive calls on the same pass
    perm = rng.permutation(F.size)
    assert _same(_both(em, F[perm], L[perm], y), (base[0][perm], base[1][perm]))
    dup = np.concatenate([np.arange(F.size), np.arange(0, F.size, 3)])
    assert _same(_both(em, F[dup], L[dup], y), (base[0][dup], base[1][dup]))
    for i in np.r_[0:40, F.size - 40:F.size]:                                                     # one job per call
        assert _same(_both(em, F[i:i + 1], L[i:i + 1], y), (base[0][i:i + 1], base[1][i:i + 1])), i
    # the labels outside a job's range do not matter
    z = y.copy()
    i = int(np.argmax((L - F > 600) & (L - F < 5000)))
    assert 600 < L[i] - F[i] < 5000
    z[:F[i]] = 3 - z[:F[i]]
    z[L[i] + 1:] = 3 - z[L[i] + 1:]
    assert em.path_log_probs(F[i:i + 1], L[i:i + 1], z)[0] == base[1][i]
    # a chunk-spanning job = the left-to-right sum of its chunk-local parts as separate jobs
    off = np.asarray(store.chunk_off, np.int64)
    spans = [i for i in range(F.size) if np.searchsorted(off, F[i], "right") != np.searchsorted(off, L[i], "right")]
    assert len(spans) >= 20
    for i in spans:
        _, _, pa, pb, _ = IR.split(off, [F[i]], [L[i]], [1])
        ph, pl = _both(em, pa, pb, y)
        sh = sl = 0.0
        for a, b in zip(ph, pl):
            sh += a
            sl += b
        assert (sh, sl) == (base[0][i], base[1][i]), i
    em.close()


_CHILD = """
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from flagger_amd import hmm
from test_entropy_gpu import _reduced_model
store, model, alpha, (F, L) = _reduced_model(2)
y = np.load(sys.argv[3])
os.environ["HF_SUBPASSES"] = "2"
em = hmm.EMList(store, model)
assert em.sub_passes >= 2, em.sub_passes
hmm.EM_runOneIterationForList(em, model)
marg, cond = em.entropy_profile()
np.savez(sys.argv[2], h=em.path_entropy(F, L), lp=em.path_log_probs(F, L, y), marg=marg, cond=cond)
em.close()
"""


def test_sub_passes_give_the_same_bits(tmp_path):
    """A context that runs its full pass in several sub-passes (HF_SUBPASSES=2, in a child process) returns the bits of the
    one-sub-pass context."""
    store, model, (F, L), ent, lps = _reduced(2)
    y = lps[1][1]
    em = hmm.EMList(store, model)
    assert em.sub_passes == 1
    hmm.EM_runOneIterationForList(em, model)
    h, lp = _both(em, F, L, y)
    marg, cond = em.entropy_profile()
    em.close()
    out, lab = str(tmp_path / "sub.npz"), str(tmp_path / "y.npy")
    np.save(lab, y)
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "tests"), out, lab], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")])))
    assert r.returncode == 0, r.stderr[-2000:]
    sub = np.load(out)
    assert np.array_equal(sub["h"], h) and np.array_equal(sub["lp"], lp)
    assert np.array_equal(sub["marg"], marg) and np.array_equal(sub["cond"], cond)


# ---- 5. nothing else moves -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_no_disturbance(algo):
    store, model, (F, L), _, lps = _reduced(2)
    y = lps[0][1]
    M = 1 + (np.arange(F.size) % 15)
    model = model.copy()
    em_a = hmm.EMList(store, model, algo=algo)
    em_b = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em_a, model)
    st_a = model.estimators.copy()
    hmm.EM_runOneIterationForList(em_b, model)
    assert np.array_equal(st_a, model.estimators)
    em_a.path_entropy(F[:10], L[:10])
    em_a.path_log_probs(F, L, y)
    em_a.entropy_profile(0, 1000)
    em_a.path_entropy(np.concatenate([F, F]), np.concatenate([L, L]))                              # (the buffer grows)
    em_a.entropy_profile()                                                                         # (and again)
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    assert np.array_equal(em_a.interval_log_probs(F, L, M), em_b.interval_log_probs(F, L, M))
    assert _same(em_a.count_moments(F, L, M), em_b.count_moments(F, L, M))
    assert _same(em_a.run_moments(F, L, M), em_b.run_moments(F, L, M))
    assert np.array_equal(em_a.labels(), em_b.labels())
    hmm.EM_runOneIterationForList(em_a, model); st2_a = model.estimators.copy()   # the next pass
    hmm.EM_runOneIterationForList(em_b, model); st2_b = model.estimators.copy()
    assert np.array_equal(st2_a, st2_b)
    assert np.array_equal(em_a.labels(), em_b.labels())
    em_a.close(); em_b.close()


# ---- 6. error codes --------------------------------------------------------------------------------------------------------------------
def test_errors():
    store = synth.config(2, 0.02)
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, store, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model)
    L_ = N.lib()
    n = store.n_windows
    one = lambda *a: np.array(a, np.int64)
    i64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    good = np.full(n, 2, np.int8)

    def ent(cnt, f, l, out=True):
        o = np.empty(max(cnt, 1))
        return L_.hf_get_path_entropy(em._h, cnt, i64p(f), i64p(l), dp(o) if out else None)

    def lpr(cnt, f, l, lab=good, out=True):
        o = np.empty(max(cnt, 1))
        return L_.hf_get_path_log_probs(em._h, cnt, i64p(f), i64p(l), lab.ctypes.data_as(C.POINTER(C.c_int8)) if lab is not None else None,
                                        dp(o) if out else None)

    def prof(first, cnt, marg=True, cond=True):
        m, c = np.empty(max(cnt, 1)), np.empty(max(cnt, 1))
        return L_.hf_get_entropy_profile(em._h, first, cnt, dp(m) if marg else None, dp(c) if cond else None)

    assert ent(1, one(0), one(0)) == N.HF_E_ARG and lpr(1, one(0), one(0)) == N.HF_E_ARG and prof(0, 1) == N.HF_E_ARG   # no pass yet
    hmm.EM_runForwardForList(em, model)
    assert ent(1, one(0), one(0)) == N.HF_E_ARG and lpr(1, one(0), one(0)) == N.HF_E_ARG and prof(0, 1) == N.HF_E_ARG   # forward-only
    hmm.EM_runOneIterationForList(em, model)
    assert ent(1, one(0), one(0)) == N.HF_OK and lpr(1, one(0), one(0)) == N.HF_OK and prof(0, 1) == N.HF_OK
    assert ent(0, None, None, out=False) == N.HF_OK and lpr(0, None, None, lab=None, out=False) == N.HF_OK           # n = 0
    assert prof(0, 0) == N.HF_OK and prof(n, 0) == N.HF_OK
    assert ent(-1, one(0), one(0)) == N.HF_E_ARG and lpr(-1, one(0), one(0)) == N.HF_E_ARG and prof(0, -1) == N.HF_E_ARG
    assert ent(1, None, one(0)) == N.HF_E_ARG and lpr(1, None, one(0)) == N.HF_E_ARG
    assert ent(1, one(0), None) == N.HF_E_ARG and lpr(1, one(0), None) == N.HF_E_ARG
    assert ent(1, one(0), one(0), out=False) == N.HF_E_ARG and lpr(1, one(0), one(0), out=False) == N.HF_E_ARG
    assert lpr(1, one(0), one(0), lab=None) == N.HF_E_ARG
    for f, l in [(-1, 0), (0, n), (5, 4), (n, n)]:
        assert ent(1, one(f), one(l)) == N.HF_E_ARG and lpr(1, one(f), one(l)) == N.HF_E_ARG, (f, l)
    for f, c in [(-1, 1), (0, n + 1), (n, 1), (n + 1, 0)]:
        assert prof(f, c) == N.HF_E_ARG, (f, c)
    assert prof(0, 4, marg=False, cond=False) == N.HF_E_ARG                  # both output arrays NULL
    assert prof(0, 4, marg=False) == N.HF_OK and prof(0, 4, cond=False) == N.HF_OK
    assert ent(2, one(0, 0), one(3, n)) == N.HF_E_ARG                        # any bad job refuses the call
    for bad in (4, -1):                                                      # a label outside 0..3: refused inside a range only
        lab = good.copy()
        lab[10] = bad
        assert lpr(1, one(5), one(10), lab) == N.HF_E_ARG and lpr(2, one(0, 10), one(3, 10), lab) == N.HF_E_ARG, bad
        assert lpr(2, one(0, 11), one(9, n - 1), lab) == N.HF_OK, bad
    with pytest.raises(N.HFError):
        em.path_entropy([0], [n])
    with pytest.raises(N.HFError):
        em.path_log_probs([0], [3], np.full(n, 7))
    with pytest.raises(ValueError):
        em.path_log_probs([0], [3], np.zeros(n + 1, np.int8))
    h = em.path_entropy([0, n - 1], [n - 1, n - 1])                          # and the context still answers afterwards
    lp = em.path_log_probs([0, n - 1], [n - 1, n - 1], em.labels())
    assert h[0] >= h[1] >= 0.0 and np.all(lp <= 0.0) and not np.any(np.isnan(lp))
    em.close()


# ---- 7. command line -------------------------------------------------------------------------------------------------------------
def _cli(args, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


@pytest.mark.parametrize("viterbi", [False, True], ids=["posterior", "viterbi"])
def test_cli_joint_entropy(tmp_path, viterbi):
    store = RR.split_store(synth.config(2, 0.04))      # chunks cut, so that a contig is a run of several chunks
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    args = ["-i", str(binp), "-W", "4000", "-n", "2", "-t", "0.001", "-f", "0.95", "-p", str(K)] + (["--viterbi"] if viterbi else [])
    _cli(args, tmp_path / "plain")
    _cli(args + ["--jointEntropy"], tmp_path / "joint")
    a, b = tmp_path / "plain", tmp_path / "joint"
    names = sorted(os.listdir(a))
    assert sorted(set(os.listdir(b)) - set(names)) == ["path_uncertainty.tsv"]
    for nme in names:
        assert (a / nme).read_bytes() == (b / nme).read_bytes(), nme
    text = (b / "path_uncertainty.tsv").read_text().splitlines()
    assert text[0] == "#scope\twindows\tpath_entropy_nats\tentropy_nats_per_window\twindow_entropy_sum_nats\tfinal_labels_log_prob"
    rows = [l.split("\t") for l in text[1:]]
    # the same run through the bindings: the final model, its last full pass, the final labels
    st = synth.WindowStore.read_bin(str(binp))
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, np.zeros((4, 4)))
    em = hmm.EMList(st, model)
    hmm.runHMMFlagger(em, model, 2, 0.001)
    labels = em.viterbi(model)[0] if viterbi else em.labels()
    assert labels.min() >= 0 and labels.max() <= 3
    off = np.asarray(st.chunk_off, np.int64)
    nc = off.size - 1
    scopes = [("all", [(0, nc)])]
    for c, ctg in enumerate(st.chunk_ctg):
        k = next((i for i, s in enumerate(scopes) if s[0] == ctg and i > 0), None)
        if k is None:
            scopes.append((ctg, []))
            k = len(scopes) - 1
        rg = scopes[k][1]
        if rg and rg[-1][1] == c:
            rg[-1] = (rg[-1][0], c + 1)
        else:
            rg.append((c, c + 1))
    assert [r[0] for r in rows] == [s[0] for s in scopes] and len(scopes) >= 3
    assert any(c1 - c0 > 1 for _, rg in scopes[1:] for c0, c1 in rg)
    marg, _ = em.entropy_profile()
    near = lambda got, want: got == "%.9g" % want or abs(float(got) - want) <= 1e-8 * abs(want)
    for row, (name, ranges) in zip(rows, scopes):
        h = hw = lp = 0.0
        windows = 0
        for c0, c1 in ranges:
            f, l = off[c0], off[c1] - 1
            h += em.path_entropy([f], [l])[0]
            lp += em.path_log_probs([f], [l], labels)[0]
            hw += marg[f:l + 1].sum()
            windows += int(l - f + 1)
        assert int(row[1]) == windows
        assert near(row[2], h) and near(row[3], h / windows) and near(row[4], hw), (row, h, hw)
        assert (row[5] == "-inf" and np.isneginf(lp)) or near(row[5], lp), (row, lp)
        assert float(row[4]) >= float(row[2]) * (1.0 - 1e-8)
    tot = sum(float(r[2]) for r in rows[1:])
    assert abs(tot - float(rows[0][2])) <= 1e-8 * float(rows[0][2]) and float(rows[0][2]) > 1.0
    em.close()
