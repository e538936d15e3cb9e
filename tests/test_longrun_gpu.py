"""Exact long-run probabilities on the GPU (hf_get_long_run_log_probs, hmm.EMList.long_run_log_probs, hmm_flagger --keptBlocks) against
the float64 numpy reference (tests/longrun_ref.py), which carries the run-length counter through every chunk's posterior Markov chain.
Value checks: |dev - ref| <= 1e-10 + 1e-9 |ref|, -inf equal to -inf, a log compared where the reference's value is >= -650 or exactly -inf
(at most 5 % of a test's jobs are left out by that: asserted here, and for the references alone in tests/test_longrun_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_longrun_cpu import JOINS, LENGTHS, SMALL_SPAN, close, comparable, jobs, store_case
from test_moments_cpu import TINY
from test_viterbi_gpu import SIZES, _trained
import geometry_cases as G
import hip_streams as HS
import interval_ref as IR
import longrun_ref as LR
import runs_ref as RR
import sampling_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]
NEG_INF = -np.inf


def _check(got, ref, what=""):
    """Both logs of every job against the reference; at most 5 % of the jobs left out."""
    use = close(got[0], ref[0]) & close(got[1], ref[1])
    assert not np.any(np.isnan(got[0])) and not np.any(np.isnan(got[1])), what
    assert np.mean(use) >= 0.95, (what, float(np.mean(use)))


def _all_joined(store):
    j = np.ones(store.n_chunks, bool)
    j[0] = False
    return j


@pytest.mark.parametrize("which", list(LENGTHS))
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed", TINY)
def test_small_stores_equal_reference(algo, model_type, seed, which):
    store, model, alpha = store_case(model_type, seed, which)
    assert list(np.diff(store.chunk_off)) == LENGTHS[which]
    em = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model)
    F, L, M, K = jobs(store.chunk_off, np.random.default_rng(seed), 200, span=SMALL_SPAN)
    A, end = S.rows(store, model, alpha)
    chain = LR.Chain(A, end, store.chunk_off)
    for joins in (None, _all_joined(store), JOINS[which]):
        got = em.long_run_log_probs(F, L, M, K, joins)
        _check(got, chain.log_probs(F, L, M, K, joins), (which, seed, joins))
        assert np.all(got[0] <= 0.0) and np.all(got[1] <= 0.0)
    em.close()


def test_grid_store_with_empty_chunks_and_uncovered_windows():
    """One chunk list of tests/geometry_cases.py: chunks on the 512 grid, the same with chunks that hold no window (an empty chunk ends a
    group), and windows outside every chunk (refused).  The jobs and their reference are geometry_cases.longrun_jobs /
    longrun_reference, the value checks test_geometry_gpu.check_long_runs (which holds every call to _check above): the geometry tests
    run the same on both algorithms and in the launch variants."""
    import test_geometry_gpu as TG                          # (here: that module imports this one)
    model_type, seed = G.CASES[0]
    store, model, alpha, _ = G.case(model_type, seed)
    F, L, M, K = G.longrun_jobs(model_type, seed)
    em = hmm.EMList(store, model)
    hmm.EM_runOneIterationForList(em, model)
    base = dict(zip(("none", "contig"), TG.check_long_runs(em, model_type, seed, "grid")))
    em.close()
    # chunks without windows: the values of the store without them, with the joins an empty chunk cuts
    est, src = G.with_empty_chunks(store)
    jd, jr = G.empty_chunk_joins(src, G.joins())
    em = hmm.EMList(est, model)
    hmm.EM_runOneIterationForList(em, model)
    TG.check_long_runs(em, model_type, seed, "empty chunks", joined=((jd, jr),))
    em.close()
    # windows outside every chunk
    ust = G.with_uncovered_windows(store, np.random.default_rng(5))
    a, n = G.FRONT, ust.n_windows
    em = hmm.EMList(ust, model)
    hmm.EM_runOneIterationForList(em, model)
    for f, l in [(0, 0), (a - 1, a + 3), (0, n - 1), (n - 1, n - 1)]:
        with pytest.raises(N.HFError) as e:
            em.long_run_log_probs([a, f], [a + 1, l], 5, 2)
        assert e.value.code == N.HF_E_ARG
    got = TG.check_long_runs(em, model_type, seed, "uncovered windows", shift=a)[1]
    close(got[0], base["contig"][0]); close(got[1], base["contig"][1])
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("cfg,model_type,hifi", [(2, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, True), (4, N.HF_MODEL_GAUSSIAN, True),
                                                 (6, N.HF_MODEL_NEGATIVE_BINOMIAL, False)])
def test_reduced_configs_equal_reference(algo, cfg, model_type, hifi):
    store = synth.config(cfg, 0.04)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    K_ = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    em, model = _trained(store, model_type, K_, alpha, algo=algo)
    hmm.EM_runOneIterationForList(em, model)
    F, L, M, K = jobs(store.chunk_off, np.random.default_rng(3200 + cfg), 200, whole=False)
    A, end = S.rows(store, model, alpha)
    got = hmm.EM_getLongRunLogProbsForList(em, F, L, M, K)
    _check(got, LR.log_probs(A, end, store.chunk_off, F, L, M, K), cfg)
    em.close()


def test_invariants(monkeypatch):
    store = RR.split_store(synth.config(2, 0.04))
    joins = RR.contig_joins(store)
    assert joins.sum() >= 40
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, synth.HIFI_ALPHA)
    hmm.EM_runOneIterationForList(em, model)
    rng = np.random.default_rng(5)
    F, L, M, K = jobs(store.chunk_off, rng, 300)
    n = store.n_windows
    none, some = em.long_run_log_probs(F, L, M, K, joins)
    assert not np.any(np.isnan(none)) and not np.any(np.isnan(some)) and np.all(none <= 0.0) and np.all(some <= 0.0)
    assert np.all(np.abs(np.exp(none) + np.exp(some) - 1.0) <= 1e-12)
    # the exact cases: no group as long as L; all four states with L within the (single) group
    un, us = em.long_run_log_probs(F, L, M, K)
    off = np.asarray(store.chunk_off, np.int64)
    one_chunk = np.searchsorted(off, F, "right") == np.searchsorted(off, L, "right")
    short = one_chunk & (K > L - F + 1)
    assert short.sum() >= 20 and np.all(un[short] == 0.0) and np.all(np.isneginf(us[short]))
    assert np.all(none[short] == 0.0) and np.all(np.isneginf(some[short]))
    full = one_chunk & (M == 15) & (K <= L - F + 1)
    assert full.sum() >= 5 and np.all(np.isneginf(un[full])) and np.all(us[full] == 0.0)
    w15 = (M == 15) & (F == 0) & (L == n - 1)
    assert w15.sum() >= 1 and np.all(np.isneginf(none[w15])) and np.all(some[w15] == 0.0)
    # L = 1: "some window in S" = the interval getter's complement, for the whole track and random ranges
    a = np.concatenate([np.zeros(15, np.int64), rng.integers(0, n, 200)])
    b = np.concatenate([np.full(15, n - 1), np.minimum(n - 1, a[15:] + rng.integers(0, 400, 200))])
    m = np.concatenate([np.arange(1, 16), rng.integers(1, 16, 200)])
    n1, s1 = em.long_run_log_probs(a, b, m, 1, joins)
    part = m != 15
    iv = em.interval_log_probs(a[part], b[part], 15 & ~m[part])
    close(n1[part], iv)
    assert np.all(np.isneginf(n1[~part])) and np.all(s1[~part] == 0.0)
    # monotone in L
    prev = None
    for k in (1, 2, 3, 5, 9, 16):
        _, s = em.long_run_log_probs(a, b, m, k, joins)
        if prev is not None:
            fin = np.isfinite(prev)
            assert np.all(np.isneginf(s[~fin])) and np.all(s[fin] <= prev[fin] + 1e-9 + 1e-9 * np.abs(prev[fin]))
        prev = s
    # bitwise: order, call splitting, duplicated jobs, a second device batch
    perm = rng.permutation(F.size)
    got = em.long_run_log_probs(F[perm], L[perm], M[perm], K[perm], joins)
    assert np.array_equal(got[0], none[perm]) and np.array_equal(got[1], some[perm])
    h0 = em.long_run_log_probs(F[:100], L[:100], M[:100], K[:100], joins)
    h1 = em.long_run_log_probs(F[100:], L[100:], M[100:], K[100:], joins)
    assert np.array_equal(np.concatenate([h0[0], h1[0]]), none) and np.array_equal(np.concatenate([h0[1], h1[1]]), some)
    dup = np.concatenate([np.arange(F.size), np.arange(0, F.size, 3)])
    got = em.long_run_log_probs(F[dup], L[dup], M[dup], K[dup], joins)
    assert np.array_equal(got[0], none[dup]) and np.array_equal(got[1], some[dup])
    monkeypatch.setenv("HF_LR_BATCH_PARTS", "7")
    got = em.long_run_log_probs(F, L, M, K, joins)
    monkeypatch.delenv("HF_LR_BATCH_PARTS")
    assert np.array_equal(got[0], none) and np.array_equal(got[1], some)
    monkeypatch.setenv("HF_LR_BATCH_PIECES", "3")
    got = em.long_run_log_probs(F, L, M, K, joins)
    monkeypatch.delenv("HF_LR_BATCH_PIECES")
    assert np.array_equal(got[0], none) and np.array_equal(got[1], some)
    # an unjoined chunk-spanning job = the left-to-right sum of its chunk-local parts as separate jobs
    spans = np.flatnonzero(~one_chunk)[:40]
    assert spans.size >= 20
    for i in spans:
        _, _, pa, pb, _ = IR.split(off, [F[i]], [L[i]], [M[i]])
        parts, _ = em.long_run_log_probs(pa, pb, M[i], K[i])
        s = 0.0
        for v in parts:
            s += v
        assert s == un[i] or (np.isneginf(s) and np.isneginf(un[i])), (i, s, un[i])
    # scan agrees with seq
    seq = hmm.EMList(store, model, algo=N.HF_ALGO_SEQ)
    hmm.EM_runOneIterationForList(seq, model)
    sn, ss = seq.long_run_log_probs(F, L, M, K, joins)
    ok = (none >= -650) | np.isneginf(none)
    close(sn[ok], none[ok])
    ok = (some >= -650) | np.isneginf(some)
    close(ss[ok], some[ok])
    seq.close()
    em.close()


@pytest.mark.parametrize("env", [{"HF_SEG_LAUNCHES": "2"}, {"HF_SUBPASSES": "3"}])
def test_launch_modes_and_sub_passes(env, monkeypatch):
    """The first call after a pass re-runs the segment kernel, also in two launches and in several sub-passes."""
    store = synth.synthesize([n * 1000 for n in SIZES], 1000, 10 ** 9, [20], seed=11)
    em0, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, iters=1)
    hmm.EM_runOneIterationForList(em0, model)
    F, L, M, K = jobs(store.chunk_off, np.random.default_rng(8), 100, whole=False)
    base = em0.long_run_log_probs(F, L, M, K)
    em0.close()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    em = hmm.EMList(store, model)
    if "HF_SEG_LAUNCHES" in env:
        assert em.seg_launches == 2
    else:
        assert em.sub_passes >= 2
    hmm.EM_runOneIterationForList(em, model)
    got = em.long_run_log_probs(F, L, M, K)
    for x, y in zip(got, base):
        ok = (y >= -650) | np.isneginf(y)
        close(x[ok], y[ok])
    em.close()


def _has_run(lab, mask, k):
    """bool[n_samples]: the label rows that hold k consecutive windows in the set."""
    inS = ((mask >> lab.astype(np.int64)) & 1).astype(bool)
    run = np.zeros(lab.shape[0], np.int64)
    hit = np.zeros(lab.shape[0], bool)
    for t in range(lab.shape[1]):
        run = np.where(inS[:, t], run + 1, 0)
        hit |= run >= k
    return hit


def test_against_the_sampler():
    store = synth.config(2, 0.03)
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, synth.HIFI_ALPHA)
    hmm.EM_runOneIterationForList(em, model)
    off = np.asarray(store.chunk_off, np.int64)
    C_ = off.size - 1
    lens = (3, 5, 1, 7)
    F = np.repeat(off[:-1], 4); L = np.repeat(off[1:] - 1, 4)
    M = np.tile(1 << np.arange(4), C_); K = np.tile(lens, C_)
    _, some = em.long_run_log_probs(F, L, M, K)
    p = np.exp(some)
    n = 512
    lab = em.sample_paths(model, n, 4242)
    support = np.array([np.mean(_has_run(lab[:, F[i]:L[i] + 1], int(M[i]), int(K[i]))) for i in range(F.size)])
    bound = 6 * np.sqrt(p * (1 - p) / n) + 2 / n
    bad = np.flatnonzero(np.abs(support - p) > bound)
    assert bad.size == 0, [(int(i), float(support[i]), float(p[i])) for i in bad[:8]]
    assert np.sum((p > 0.01) & (p < 0.99)) >= 5                     # the comparison says something
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_no_disturbance(algo):
    store = synth.config(2, 0.03)
    em_a, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, synth.HIFI_ALPHA, iters=1, algo=algo)
    em_b = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em_a, model)
    st_a = model.estimators.copy()
    hmm.EM_runOneIterationForList(em_b, model)
    assert np.array_equal(st_a, model.estimators)
    F, L, M, K = jobs(store.chunk_off, np.random.default_rng(3), 200)
    iv = em_a.interval_log_probs(F, L, M)
    rm = em_a.run_moments(F, L, M)
    em_a.long_run_log_probs(F, L, M, K)
    em_a.long_run_log_probs(np.concatenate([F, F]), np.concatenate([L, L]), np.concatenate([M, M]), np.concatenate([K, K]))   # (the buffer grows)
    assert np.array_equal(em_a.interval_log_probs(F, L, M), iv)
    assert all(np.array_equal(x, y) for x, y in zip(em_a.run_moments(F, L, M), rm))
    assert np.array_equal(em_a.labels(), em_b.labels())
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    for x, y in zip(em_a.forward_backward(), em_b.forward_backward()):
        assert np.array_equal(x, y)
    hmm.EM_runOneIterationForList(em_a, model); st2_a = model.estimators.copy()   # the next pass
    hmm.EM_runOneIterationForList(em_b, model); st2_b = model.estimators.copy()
    assert np.array_equal(st2_a, st2_b)
    assert np.array_equal(em_a.labels(), em_b.labels())
    em_a.close(); em_b.close()


def test_errors():
    store = synth.config(2, 0.02)
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, store, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model)
    L_ = N.lib()
    n = store.n_windows
    one = lambda *a: np.array(a, np.int64)
    def call(cnt, f, l, m, k, joined=None, none=True, some=True):
        ptr = lambda x, t: x.ctypes.data_as(C.POINTER(t)) if x is not None else None
        mm = np.asarray(m, np.uint8) if m is not None else None
        kk = np.asarray(k, np.int32) if k is not None else None
        jj = np.asarray(joined, np.uint8) if joined is not None else None
        o1, o2 = np.empty(max(cnt, 1)), np.empty(max(cnt, 1))
        return L_.hf_get_long_run_log_probs(em._h, cnt, ptr(f, C.c_int64), ptr(l, C.c_int64), ptr(mm, C.c_uint8), ptr(kk, C.c_int32),
                                            ptr(jj, C.c_uint8), ptr(o1, C.c_double) if none else None, ptr(o2, C.c_double) if some else None)
    assert call(1, one(0), one(0), [1], [1]) == N.HF_E_ARG                     # no pass yet
    hmm.EM_runForwardForList(em, model)
    assert call(1, one(0), one(0), [1], [1]) == N.HF_E_ARG                     # forward-only
    hmm.EM_runOneIterationForList(em, model)
    assert call(1, one(0), one(0), [1], [1]) == N.HF_OK
    assert call(1, one(0), one(0), [1], [1], none=False) == N.HF_OK            # either output alone
    assert call(1, one(0), one(0), [1], [1], some=False) == N.HF_OK
    assert call(1, one(0), one(0), [1], [1], none=False, some=False) == N.HF_E_ARG
    assert call(0, None, None, None, None, none=False, some=False) == N.HF_OK
    assert call(-1, one(0), one(0), [1], [1]) == N.HF_E_ARG
    assert call(1, None, one(0), [1], [1]) == N.HF_E_ARG
    assert call(1, one(0), None, [1], [1]) == N.HF_E_ARG
    assert call(1, one(0), one(0), None, [1]) == N.HF_E_ARG
    assert call(1, one(0), one(0), [1], None) == N.HF_E_ARG
    for f, l in [(-1, 0), (0, n), (5, 4), (n, n)]:
        assert call(1, one(f), one(l), [1], [1]) == N.HF_E_ARG, (f, l)
    for m in (0, 16, 255):
        assert call(1, one(0), one(3), [m], [1]) == N.HF_E_ARG, m
    for k in (0, -1, -2 ** 31):
        assert call(1, one(0), one(3), [1], [k]) == N.HF_E_ARG, k
    for m, k in ((1, 58), (3, 30), (7, 20), (15, 16)):                        # the lane cap: met, and one over
        assert call(1, one(0), one(3), [m], [k]) == N.HF_OK, (m, k)
        assert call(1, one(0), one(3), [m], [k + 1]) == N.HF_E_ARG, (m, k)
    assert call(1, one(0), one(3), [1], [2 ** 31 - 1]) == N.HF_E_ARG
    joined = np.zeros(store.n_chunks, np.uint8)
    assert call(1, one(0), one(3), [1], [2], joined) == N.HF_OK
    joined[0] = 1
    assert call(1, one(0), one(3), [1], [2], joined) == N.HF_E_ARG
    assert call(2, one(0, 0), one(3, 3), [1, 1], [2, 0]) == N.HF_E_ARG          # any bad job refuses the call
    with pytest.raises(N.HFError):
        em.long_run_log_probs([0], [n], [1], [1])
    with pytest.raises(ValueError):
        em.long_run_log_probs([0], [3], [1], [1], joined=[0, 1])
    none, some = em.long_run_log_probs([0, n - 1], [n - 1, n - 1], [15, 3], [1, 2])   # and the context still answers afterwards
    assert np.isneginf(none[0]) and some[0] == 0.0 and none[1] == 0.0 and np.isneginf(some[1])
    em.close()


def test_callers_stream():
    """The same jobs on a caller's non-blocking stream, with filler work in front, give bitwise the null-stream context's values."""
    model_type, seed = TINY[0]
    store, model, alpha = store_case(model_type, seed, "period")
    F, L, M, K = jobs(store.chunk_off, np.random.default_rng(seed), 100, span=SMALL_SPAN)
    em0 = hmm.EMList(store, model)
    hmm.EM_runOneIterationForList(em0, model)
    base = em0.long_run_log_probs(F, L, M, K, JOINS["period"])
    em0.close()
    with HS.Streams() as st:
        s = st.new(non_blocking=True)
        em = hmm.EMList(store, model, stream=s)
        st.h.delay(s)
        hmm.EM_runOneIterationForList(em, model)
        st.h.delay(s)
        got = em.long_run_log_probs(F, L, M, K, JOINS["period"])
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
        em.close()


# ---- command line --------------------------------------------------------------------------------------------------------------
def _cli(args, out, ok=True):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr[-2000:])
    return r


def _rows(path):
    return [l.split("\t") for l in path.read_text().splitlines() if not l.startswith("#")]


def test_cli_kept_blocks(tmp_path):
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    bare = ["-i", str(binp), "-W", "4000", "-n", "3", "-P"]
    args = bare + ["--minimumLengths", "12000,20000,28000"]
    a, b = tmp_path / "plain", tmp_path / "kept"
    _cli(args, a)
    post_rows = _rows(a / "posterior_prediction_final.bed")
    ctg0 = post_rows[0][0]
    regions = [(ctg0, post_rows[0][1], post_rows[40][2], "r0"), ("no_such_contig", "0", "100", "x"), (ctg0, post_rows[5][1], post_rows[5][2], "one")]
    bed = tmp_path / "regions.bed"
    bed.write_text("".join("\t".join(r) + "\n" for r in regions))
    _cli(args + ["--regionProbs", str(bed)], a)
    _cli(args + ["--regionProbs", str(bed), "--keptBlocks"], b)
    names = sorted(os.listdir(a))
    assert sorted(set(os.listdir(b)) - set(names)) == ["kept_block_probabilities.tsv"]
    for nme in names:
        assert (a / nme).read_bytes() == (b / nme).read_bytes(), nme
    text = (b / "kept_block_probabilities.tsv").read_text().splitlines()
    head = text[0].split("\t")
    assert head[:3] == ["#scope", "name", "n_windows"]
    assert head[3:] == [f"{c}_{l}" for l in ("Err", "Dup", "Hap", "Col") for c in ("min_windows", "p_block", "p_none")]
    rows = [l.split("\t") for l in text[1:]]
    contigs = []
    for c in store.chunk_ctg:
        if c not in contigs:
            contigs.append(c)
    assert [r[0] for r in rows] == ["all"] + ["contig"] * len(contigs) + ["region"] * 3
    assert [r[1] for r in rows[1:1 + len(contigs)]] == contigs and [r[1] for r in rows[-3:]] == ["r0", "x", "one"]
    assert int(rows[0][2]) == store.n_windows
    assert rows[-2][2] == "0" and rows[-2][3:] == ["NA"] * 12
    for r in rows:
        if r[3] == "NA":
            continue
        assert [r[3], r[6], r[9], r[12]] == ["3", "5", "1", "7"]
        for l in range(4):
            pb, pn = float(r[4 + 3 * l]), float(r[5 + 3 * l])
            assert 0.0 <= pb <= 1.0 and 0.0 <= pn <= 1.0 and abs(pb + pn - 1.0) <= 2e-6
    # Hap at length 1 = p_any_Hap of --regionProbs for the same region
    reg = _rows(b / "region_label_probabilities.tsv")
    for kr, rr in zip(rows[-3:], reg):
        if rr[4] == "0":
            continue
        assert float(kr[4 + 3 * 2]) == pytest.approx(float(rr[5 + 3 * 2]), rel=2e-5, abs=2e-6)
    # refusals
    for extra, word in ((["--keptBlocks"], "--minimumLengths"),
                        (["--keptBlocks", "--minimumLengths", "12000,20000,400000"], "400000"),
                        (["--keptBlocks", "--minimumLengths", "12000,20000,28000", "--gpus", "2"], "--keptBlocks")):
        r = _cli(bare + extra, tmp_path / "bad", ok=False)
        assert "--keptBlocks" in r.stderr and word in r.stderr, r.stderr[-500:]
