"""The exact distribution of label totals on the GPU (hf_get_count_distribution, hmm.EMList.count_distribution, hmm_flagger
--totalsDistribution) against the numpy references of tests/countdist_ref.py: path enumeration (a) where a job can be enumerated, the
long-double joint route (b) elsewhere.  Neither forms the posterior chain Q, the pieces' transfers or the host's stitch, which the
device does.

Value checks: |dev - ref| <= 1e-12 + 1e-9 |ref| per bin, the standing bound of the posterior sums of non-negative terms;
no entry is excused, and every test prints its largest absolute and relative deviation before it asserts.  The formulation's own
deviation from (a) and (b), in float64 on the CPU, is 2.4e-13 relative at most over the bins above 1e-3
(tests/test_countdist_cpu.py test_restated_against_the_other_routes, over the stores of the first two tests here)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_countdist_cpu import TINY_K, reduced_jobs, tiny_jobs, tiny_reference
from test_moments_cpu import REDUCED, TINY
from test_runlen_cpu import ATOL, RTOL, close, deviation, range_jobs
from test_viterbi_gpu import _trained
import countdist_ref as CD
import floor_cases as FC
import geometry_cases as G
import hip_streams as HS
import interval_ref as IR
import runs_ref as RR
import sampling_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]


def _check(got, ref, what):
    ref = np.asarray(ref, np.float64)
    a, r = deviation(got, ref)
    print("%s: max abs %.3e, max relative %.3e, bins above 1e-3: %d of %d" % (what, a, r, int(np.sum(ref > 1e-3)), ref.size))
    assert not np.any(np.isnan(got)) and np.all(got >= 0.0), what
    assert np.all(close(got, ref)), (what, a, r)
    assert np.sum(ref > 1e-3) >= 20, what


def _sums_close(got, ref, bins):
    """A sum of bins against a single value: the bound of a bin, summed (`bins`: the sum of the bins' weights)."""
    return np.abs(got - ref) <= bins * ATOL + RTOL * np.abs(ref)


def _exact_cases(got, T, M, K):
    """The zeros of the header: bins above the job's windows, and with mask 15 every bin but the total's."""
    assert np.all(got[T <= K, K + 1] == 0.0)
    for row, t, m in zip(got, T, M):
        assert np.all(row[t + 1:] == 0.0)
        if m == 15:
            assert np.all(np.delete(row, min(t, K + 1)) == 0.0) and row[min(t, K + 1)] == pytest.approx(1.0, abs=1e-12)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed", TINY)
def test_tiny_stores_equal_reference(algo, model_type, seed):
    """Every mask on every small chunk, on every sub-range of the 5-window chunk, on ranges of 1, 2, 3, 4, 7, 8, 39, 40, 61 and 62
    windows inside and across chunks, at K = 1, 2, 3, 7, 61, 62 (so that jobs of K and of K + 1 windows exist for every K but 62), and
    the exact cases of the header."""
    store, model, alpha, (F, La, M) = tiny_jobs(model_type, seed)
    off = np.asarray(store.chunk_off, np.int64)
    T = La - F + 1
    em = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model)
    for K in TINY_K:
        ref, small = tiny_reference(model_type, seed, K)
        got = hmm.EM_getCountDistributionForList(em, F, La, M, K)
        assert got.shape == (F.size, K + 2) and got.dtype == np.float64
        _check(got, ref, "tiny %d K %d" % (seed, K))
        _exact_cases(got, T, M, K)
        # bin ">K" is exactly 0.0 up to K windows and first non-zero at K + 1
        assert np.sum(T == K) >= 15 and np.sum(T <= K) >= 15
        if K < 62:
            assert np.sum(T == K + 1) >= 15 and np.any(got[T == K + 1, K + 1] > 1e-3)
        # a job that spans chunks = the host's stitch of its parts asked as separate jobs
        for i in np.flatnonzero(np.searchsorted(off, F, "right") != np.searchsorted(off, La, "right"))[::7][:8]:
            _, _, pa, pb, _ = IR.split(off, [F[i]], [La[i]], [M[i]])
            assert pa.size >= 2
            assert np.array_equal(CD.stitch(list(em.count_distribution(pa, pb, M[i], K)), K), got[i]), i
    em.close()


def _all_bits_equal(em, F, La, M, K, base, monkeypatch, rng):
    """The same bits whatever the order, the number of jobs and the device batch."""
    perm = rng.permutation(F.size)
    assert np.array_equal(em.count_distribution(F[perm], La[perm], M[perm], K), base[perm])
    h = F.size // 3
    assert np.array_equal(np.concatenate([em.count_distribution(F[:h], La[:h], M[:h], K), em.count_distribution(F[h:], La[h:], M[h:], K)]), base)
    for name, cap in (("HF_CD_BATCH_PARTS", "7"), ("HF_CD_BATCH_PIECES", "3")):
        monkeypatch.setenv(name, cap)
        got = em.count_distribution(F, La, M, K)
        monkeypatch.delenv(name)
        assert np.array_equal(got, base), name


@pytest.mark.parametrize("split", [False, True], ids=["whole", "cut"])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("cfg,model_type,hifi", REDUCED)
def test_reduced_configs_equal_reference(algo, cfg, model_type, hifi, split, monkeypatch):
    """The reduced configs as they are and with their chunks cut, the trained model, K = 5 and 62 (jobs of 62 and of 63 windows among
    them), against route (b); and the identities with the other getters on the device: the bins add up to 1; bin 0 is
    hf_get_interval_log_probs' p_all of the complement and bin T that of S; the mean and the variance of the bins are
    hf_get_count_moments'; S and its complement mirror each other (the last four for jobs of at most K windows)."""
    store = synth.config(cfg, 0.04)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    if split:
        store = RR.split_store(store)
    K_ = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    em, model = _trained(store, model_type, K_, alpha, algo=algo)
    hmm.EM_runOneIterationForList(em, model)
    F, La, M = reduced_jobs(store, 5100 + cfg + (50 if split else 0))
    T = La - F + 1
    A, end = S.rows(store, model, alpha)
    jt = CD.Joint(A, end, store.chunk_off)
    for K in (5, 62):
        got = em.count_distribution(F, La, M, K)
        _check(got, jt.distribution(F, La, M, K), "cfg %d%s K %d" % (cfg, " cut" if split else "", K))
        _exact_cases(got, T, M, K)
        assert np.all(_sums_close(got.sum(axis=1), 1.0, K + 2))
        short = (T <= K) & (M != 15)
        assert short.sum() >= (10 if K == 62 else 3)
        f, l, m, g, t = F[short], La[short], M[short], got[short], T[short]
        assert np.all(close(g[:, 0], np.exp(em.interval_log_probs(f, l, 15 - m))))
        assert np.all(close(g[np.arange(t.size), t], np.exp(em.interval_log_probs(f, l, m))))
        mean, var = em.count_moments(f, l, m)
        k = np.arange(K + 1)
        m1, m2 = (g[:, :K + 1] * k).sum(axis=1), (g[:, :K + 1] * k * k).sum(axis=1)
        assert np.all(_sums_close(m1, mean, K * (K + 1) // 2))
        # (the variance is a difference of the two sums: the bound of the second moment, which is what the bins give)
        assert np.all(_sums_close(m2, var + mean * mean, K * (K + 1) * (2 * K + 1) // 6))
        back = em.count_distribution(f, l, 15 - m, K)
        for row, other, tt in zip(g, back, t):
            assert np.all(close(row[:tt + 1], other[:tt + 1][::-1]))
    assert np.any(T == 62) and np.any(T == 63) and np.any(got[T == 63, 63] > 1e-3)
    if split and algo == N.HF_ALGO_SCAN:
        _all_bits_equal(em, F, La, M, 62, em.count_distribution(F, La, M, 62), monkeypatch, np.random.default_rng(cfg))
    em.close()


@functools.lru_cache(maxsize=None)
def _geometry_jobs():
    """About 100 of the grid store's 903 boundary-point ranges (a seeded choice, the whole track and the ranges around 512 and 1024
    among them) with the case's masks, and ranges of at most 62 windows around the grid points 512 and 1024."""
    model_type, seed = G.CASES[0]
    _, _, _, (F, La, M, _) = G.case(model_type, seed)
    pick = np.random.default_rng(31).choice(F.size, 96, replace=False)
    must = [int(np.flatnonzero((F == f) & (La == l))[0]) for f, l in ((0, G.N_WINDOWS - 1), (504, 1535), (511, 513), (1023, 2048))]
    pick = np.unique(np.concatenate([pick, must]))
    near = [(500, 515, 11), (511, 512, 4), (512, 540, 2), (1000, 1061, 15), (1020, 1030, 7), (2040, 2101, 8)]
    return (np.concatenate([F[pick], [x[0] for x in near]]).astype(np.int64), np.concatenate([La[pick], [x[1] for x in near]]).astype(np.int64),
            np.concatenate([M[pick], [x[2] for x in near]]).astype(np.int64))


@functools.lru_cache(maxsize=None)
def _geometry_reference(K):
    model_type, seed = G.CASES[0]
    A, end = G.rows(model_type, seed)
    F, La, M = _geometry_jobs()
    ref = np.asarray(CD.joint(A, end, G.OFF, F, La, M, K), np.float64)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("algo", ALGOS)
def test_grid_store(algo, monkeypatch):
    """The grid store of tests/geometry_cases.py at K = 62 and 9: parts that start and end on, one before and one after multiples of
    512, one- and two-window chunks, jobs over two and three chunks; the same with chunks without windows and with windows outside
    every chunk; calls of more than one device batch; bitwise equal between batchings and job orders; a job over several chunks is
    bitwise the stitch of its parts."""
    model_type, seed = G.CASES[0]
    store, model, alpha, _ = G.case(model_type, seed)
    F, La, M = _geometry_jobs()
    off = np.asarray(G.OFF, np.int64)
    em = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model)
    base = {}
    for K in (62, 9):
        got = em.count_distribution(F, La, M, K)
        _check(got, _geometry_reference(K), "grid K %d" % K)
        _exact_cases(got, La - F + 1, M, K)
        _all_bits_equal(em, F, La, M, K, got, monkeypatch, np.random.default_rng(3))
        base[K] = got
    n_parts = np.searchsorted(off, La, "right") - np.searchsorted(off, F, "right") + 1
    assert np.sum(n_parts == 2) >= 3 and np.sum(n_parts == 3) >= 3
    for i in np.concatenate([np.flatnonzero(n_parts == 2)[:4], np.flatnonzero(n_parts == 3)[:4], np.flatnonzero(n_parts > 3)[:2]]):
        _, _, pa, pb, _ = IR.split(off, [F[i]], [La[i]], [M[i]])
        assert np.array_equal(CD.stitch(list(em.count_distribution(pa, pb, M[i], 62)), 62), base[62][i]), i
    em.close()
    # chunks without windows: the values of the store without them
    est, src = G.with_empty_chunks(store)
    em = hmm.EMList(est, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model)
    assert np.array_equal(em.count_distribution(F, La, M, 62), base[62])
    em.close()
    # windows outside every chunk: refused; the others shifted (the piece grid is global, so the walks are cut elsewhere: not the same bits)
    ust = G.with_uncovered_windows(store, np.random.default_rng(5))
    a, n = G.FRONT, ust.n_windows
    em = hmm.EMList(ust, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model)
    for f, l in [(0, 0), (a - 1, a + 3), (0, n - 1), (n - 1, n - 1)]:
        with pytest.raises(N.HFError) as e:
            em.count_distribution([a, f], [a + 1, l], 5, 8)
        assert e.value.code == N.HF_E_ARG
    _check(em.count_distribution(F + a, La + a, M, 62), _geometry_reference(62), "grid, uncovered windows")
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_floor_stretches(algo):
    """The long floored store of tests/floor_cases.py: ranges whose pieces lie wholly inside the stretch 930..1372 (it crosses the grid
    point 1024), ranges over the chunk boundary 1949 | 1950 that is floored on both sides, the whole track.  No NaN, route (b)."""
    store, model, alpha = FC.fixture("long")
    F0, L0, M0, _ = FC.range_jobs("long")
    pick = np.random.default_rng(12).choice(F0.size, 80, replace=False)
    F = np.concatenate([F0[pick], [930, 930, 1000, 1939, 1945, 0, 0, 1000]]).astype(np.int64)
    La = np.concatenate([L0[pick], [1372, 1023, 1372, 1960, 1955, 2149, 2149, 1050]]).astype(np.int64)
    M = np.concatenate([M0[pick], [15, 4, 11, 15, 7, 4, 11, 3]]).astype(np.int64)
    A, end = FC.rows("long")
    em = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model)
    for K in (7, 62):
        got = em.count_distribution(F, La, M, K)
        _check(got, CD.joint(A, end, store.chunk_off, F, La, M, K), "floor K %d" % K)
        _exact_cases(got, La - F + 1, M, K)
    em.close()


def test_zero_posterior_puts_the_mass_in_bin_zero():
    """Where S has posterior 0 bin 0 carries the mass and every other bin is exactly 0.0: a model whose Err and Dup states cannot be
    entered or started in."""
    mt, seed = TINY[1]
    store, model, alpha, (F, La, M) = tiny_jobs(mt, seed)
    R = model.numberOfRegions
    v = model.param_vector().reshape(R, -1).copy()
    for r in range(R):
        t = v[r, :25].reshape(5, 5)
        t[:, :2] = 0.0
        t[:4, 2:4] *= ((1 - 1e-4) / t[:4, 2:4].sum(axis=1))[:, None]
        t[4, 2:4] /= t[4, 2:4].sum()
    model.set_param_vector(v.ravel())
    em = hmm.EMList(store, model)
    hmm.EM_runOneIterationForList(em, model)
    got = em.count_distribution(F, La, M, 7)
    assert not np.any(np.isnan(got)) and np.all(got >= 0.0)
    dead = (M & ~3) == 0
    assert dead.sum() >= 20 and np.all(got[dead, 1:] == 0.0) and np.all(np.abs(got[dead, 0] - 1.0) <= ATOL + RTOL)
    assert np.any(got[~dead, 1:] > 0.1)
    em.close()


def _record(em, model, F, La, M, order, with_dist):
    """The calls of `order` on the context, the distribution getter between them: (the distributions, the other calls' results)."""
    dists, others = [], []
    for op in order:
        if op == "estep":
            hmm.EM_runOneIterationForList(em, model)
            others.append(model.estimators.copy())
        elif op == "viterbi":
            lab, ll, lp = em.viterbi(model)
            others += [lab.copy(), ll.copy()]
        elif op == "count_moments":
            others += [x.copy() for x in em.count_moments(F, La, M)]
        elif op == "run_lengths":
            others.append(em.run_lengths(F, La, M, 9).copy())
        elif op == "posterior":
            others.append(em.posterior().copy())
        if with_dist:
            dists.append(em.count_distribution(F, La, M, 9))
    return dists, others


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("order_seed", [0, 1])
def test_interleaved_with_the_pass_and_the_other_getters(algo, order_seed):
    """The getter between hf_estep, hf_viterbi, hf_get_count_moments, hf_get_run_lengths and hf_get_posterior in a seeded order returns
    the same bits every time, those calls' results are bitwise what they are without it, and the same holds on a context whose pass ran
    on a caller's non-blocking stream with filler work in front of every call."""
    store = RR.split_store(synth.config(2, 0.03))
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 4, store, synth.HIFI_ALPHA)
    F, La, M = range_jobs(store.chunk_off, np.random.default_rng(6), 40)
    order = ["estep"] + list(np.random.default_rng(order_seed).permutation(["estep", "viterbi", "count_moments", "posterior", "viterbi", "run_lengths"]))
    em0 = hmm.EMList(store, model, algo=algo)
    _, plain = _record(em0, model, F, La, M, order, False)
    em0.close()
    em1 = hmm.EMList(store, model, algo=algo)
    dists, others = _record(em1, model, F, La, M, order, True)
    em1.close()
    assert len(plain) == len(others) and all(np.array_equal(x, y) for x, y in zip(plain, others))
    assert all(np.array_equal(s, dists[0]) for s in dists) and np.sum(dists[0] > 1e-3) >= 20      # (the model is not re-estimated: one pass)
    with HS.Streams() as st:
        s = st.new(non_blocking=True)
        em = hmm.EMList(store, model, algo=algo, stream=s)
        dists2, others2 = [], []
        for op in order:
            st.h.delay(s)
            sp, ot = _record(em, model, F, La, M, [op], True)
            dists2 += sp; others2 += ot
        em.close()
    assert all(np.array_equal(x, y) for x, y in zip(plain, others2))
    assert all(np.array_equal(x, dists[0]) for x in dists2)


def test_errors():
    store = synth.config(2, 0.02)
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, store, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model)
    L_ = N.lib()
    n = store.n_windows
    one = lambda *a: np.array(a, np.int64)
    def call(cnt, f, l, m, max_count, out=True):
        ptr = lambda x, t: x.ctypes.data_as(C.POINTER(t)) if x is not None else None
        mm = np.asarray(m, np.uint8) if m is not None else None
        o = np.empty(max(cnt, 1) * 64)
        return L_.hf_get_count_distribution(em._h, cnt, ptr(f, C.c_int64), ptr(l, C.c_int64), ptr(mm, C.c_uint8), max_count,
                                            ptr(o, C.c_double) if out else None)
    assert call(1, one(0), one(0), [1], 4) == N.HF_E_ARG                       # no pass yet
    hmm.EM_runForwardForList(em, model)
    assert call(1, one(0), one(0), [1], 4) == N.HF_E_ARG                       # forward-only
    hmm.EM_runOneIterationForList(em, model)
    assert call(1, one(0), one(0), [1], 4) == N.HF_OK
    assert call(1, one(0), one(0), [1], 4, out=False) == N.HF_E_ARG
    assert call(0, None, None, None, 4, out=False) == N.HF_OK                  # n = 0: a successful no-op
    assert call(-1, one(0), one(0), [1], 4) == N.HF_E_ARG
    assert call(1, None, one(0), [1], 4) == N.HF_E_ARG
    assert call(1, one(0), None, [1], 4) == N.HF_E_ARG
    assert call(1, one(0), one(0), None, 4) == N.HF_E_ARG
    for f, l in [(-1, 0), (0, n), (5, 4), (n, n)]:
        assert call(1, one(f), one(l), [1], 4) == N.HF_E_ARG, (f, l)
    for m in (0, 16, 255):
        assert call(1, one(0), one(3), [m], 4) == N.HF_E_ARG, m
    for k in (0, -1, 63, 64, 2 ** 31 - 1, -2 ** 31):
        assert call(1, one(0), one(3), [1], k) == N.HF_E_ARG, k
    assert call(0, None, None, None, 63, out=False) == N.HF_E_ARG
    for k in (1, 62):
        assert call(1, one(0), one(3), [1], k) == N.HF_OK, k
    assert call(2, one(0, 0), one(3, 3), [1, 0], 2) == N.HF_E_ARG               # any bad job refuses the call
    with pytest.raises(N.HFError):
        em.count_distribution([0], [n], [1], 4)
    with pytest.raises(N.HFError):
        em.count_distribution([0], [3], [1], 63)
    with pytest.raises(ValueError):
        em.count_distribution([0], [3], [1], 4.5)
    with pytest.raises(ValueError):
        em.count_distribution([0], [3], [300], 4)
    got = em.count_distribution([0, n - 1], [3, n - 1], [15, 15], 3)           # and the context still answers afterwards
    assert got.shape == (2, 5) and got[1, 1] == pytest.approx(1.0, rel=1e-12) and np.all(np.delete(got[1], 1) == 0.0)
    assert got[0, 4] == pytest.approx(1.0, rel=1e-12) and np.all(got[0, :4] == 0.0)
    em.close()


# ---- command line --------------------------------------------------------------------------------------------------------------
def _cli(args, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


SETS = [("Err", 1), ("Dup", 2), ("Hap", 4), ("Col", 8), ("Err+Dup+Col", 11)]


def test_cli_totals_distribution(tmp_path):
    store = RR.split_store(synth.config(2, 0.04))      # chunks cut, so that a region can cross a chunk boundary inside a contig
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    Kc = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    K = 12
    off = np.asarray(store.chunk_off, np.int64)
    W = 4000
    joins = RR.contig_joins(store)
    cj = int(np.flatnonzero(joins)[0])                  # chunk cj continues chunk cj - 1

    def region(a, b, name):                             # the windows a .. b of one contig
        ca, cb = int(np.searchsorted(off, a, "right")) - 1, int(np.searchsorted(off, b, "right")) - 1
        assert store.chunk_ctg[ca] == store.chunk_ctg[cb]
        return (store.chunk_ctg[ca], int(store.chunk_s[ca]) + int(a - off[ca]) * W, int(store.chunk_s[cb]) + int(b - off[cb]) * W + 1, name, a, b)

    regions = [region(int(off[cj]) - 5, int(off[cj]) + 4, "across"), region(3, 3, "one"), ("no_such_contig", 0, 100, "x", 0, -1),
               region(10, 10 + K - 1, "K"), region(40, 40 + K, "K+1"), region(100, 139, "long")]
    bed = tmp_path / "regions.bed"
    bed.write_text("".join("%s\t%d\t%d\t%s\n" % r[:4] for r in regions))
    args = ["-i", str(binp), "-W", str(W), "-n", "2", "-t", "0.001", "-f", "0.95", "-p", str(Kc), "--regionProbs", str(bed)]
    a, b = tmp_path / "plain", tmp_path / "totals"
    _cli(args, a)
    _cli(args + ["--totalsDistribution", str(K)], b)
    names = sorted(os.listdir(a))
    assert sorted(set(os.listdir(b)) - set(names)) == ["region_label_totals_exact.tsv"]
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    text = (b / "region_label_totals_exact.tsv").read_text().splitlines()
    assert text[0].split("\t") == ["#ctg", "start", "end", "name", "n_windows", "label_set", "mean", "q025", "q50", "q975"] + \
        ["p_%d" % k for k in range(K + 1)] + ["p_gtK"]
    rows = [l.split("\t") for l in text[1:]]
    probs = [l.split("\t") for l in (b / "region_label_probabilities.tsv").read_text().splitlines()[1:]]
    assert [r[:5] for r in rows] == [p[:5] for p in probs for _ in SETS]
    assert [r[5] for r in rows] == [s for _ in regions for s, _ in SETS]
    # the same run through the bindings: the final model, its last full pass
    st = synth.WindowStore.read_bin(str(binp))
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, Kc, st, np.zeros((4, 4)))
    em = hmm.EMList(st, model)
    hmm.runHMMFlagger(em, model, 2, 0.001)
    seen_gt = seen_mean = 0
    for i, reg in enumerate(regions):
        for k, (_, mask) in enumerate(SETS):
            row = rows[i * 5 + k]
            if reg[5] < reg[4]:
                assert row[4] == "0" and row[6:] == ["NA"] * (K + 6)
                continue
            assert int(row[4]) == reg[5] - reg[4] + 1
            d = em.count_distribution([reg[4]], [reg[5]], [mask], K)[0]
            for got, want in zip(row[10:], d):
                assert got == "%.6g" % want or abs(float(got) - want) <= 1e-9 + 1e-5 * want, (row, d)
            cum = np.cumsum(d[:K + 1])
            for got, level in zip(row[7:10], (0.025, 0.5, 0.975)):
                want = ">%d" % K if cum[K] < level else str(int(np.argmax(cum >= level)))
                near = np.any(np.abs(cum - level) < 1e-9)                       # (a cumulative sum on the level itself: either side)
                assert got == want or near, (row, level, cum)
            if d[K + 1] > 0.0:
                assert row[6] == "NA"
                seen_gt += 1
            else:
                assert abs(float(row[6]) - (d[:K + 1] * np.arange(K + 1)).sum()) <= 1e-6
                seen_mean += 1
    assert seen_gt >= 3 and seen_mean >= 15
    assert all(r[6] != "NA" for r in rows[15:20])              # K windows: p_gtK is exactly 0
    em.close()
