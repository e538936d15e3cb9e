"""Exact count moments on the GPU (hf_get_count_moments, hmm.EMList.count_moments, hmm_flagger --exactTotals) against the numpy
reference (tests/moments_ref.py), which forms them by other routes: path enumeration (a) and pairwise joint posteriors (b) on the tiny
stores, the uncentred long-double jet over the whole chunk (c) on the reduced configs.

Tolerance of a variance: |dev - ref| <= ATOL scale + RTOL ref, scale = 1 (windows^2) or window_len^2 (bases^2), ATOL = 1e-12 and
RTOL = 3.3e-12: a hundredfold of 3.3e-14, the largest relative deviation of the gamma-centred float64 recursion from (c) over the jobs of
the tiny-store and reduced-config tests, measured on the CPU by tests/test_moments_cpu.py::test_centred_float64_against_the_long_double_jet
(the hundredfold is for the device's association order and its differently rounded rows and posterior); under the standing 1e-9.
Measured on an MI355X: reduced configs at most 6.2e-14 relative (var > 1e-3) and 2.3e-13 windows^2 absolute, tiny stores 9.6e-14 windows^2
absolute (7.6e-12 of a variance of 0.013), means 7e-15 relative.
A mean is a sum of posterior values: |dev - ref| <= 1e-12 sqrt(scale) + 1e-9 |ref| against the reference (the posterior tests' bound),
1e-12 relative against the same sum over hf_get_posterior's values."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_moments_cpu import ATOL, REDUCED, RTOL, TINY, reduced_case, tiny_case
from test_viterbi_gpu import _trained
import interval_ref as IR
import moments_ref as MR
import sampling_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]


def _scale(store, unit):
    return float(store.window_len) ** 2 if unit == "bases" else 1.0


def _close_var(dev, ref, scale, what=""):
    dev, ref = np.asarray(dev), np.asarray(ref)
    err = np.abs(dev - ref)
    big = ref > 1e-3 * scale
    print("%s variance: max |dev - ref| / scale %.3e, max relative deviation (var > 1e-3) %.3e over %d jobs"
          % (what, float(np.max(err, initial=0.0)) / scale, float(np.max(err[big] / ref[big], initial=0.0)), int(big.sum())))
    bad = np.flatnonzero(~(err <= ATOL * scale + RTOL * np.abs(ref)))
    assert bad.size == 0, [(int(i), float(dev[i]), float(ref[i])) for i in bad[:8]]
    assert np.all(dev >= 0.0)


def _close_mean(dev, ref, scale, what=""):
    dev, ref = np.asarray(dev), np.asarray(ref)
    err = np.abs(dev - ref)
    print("%s mean: max relative deviation %.3e" % (what, float(np.max(err / np.maximum(np.abs(ref), 1e-300), initial=0.0))))
    bad = np.flatnonzero(~(err <= 1e-12 * math.sqrt(scale) + 1e-9 * np.abs(ref)))
    assert bad.size == 0, [(int(i), float(dev[i]), float(ref[i])) for i in bad[:8]]


def _weight_totals(store, unit, F, L, R):
    w = MR.weights(store, unit)
    reg = store.regions().astype(np.int64)
    return np.array([np.where((r < 0) | (reg[a:b + 1] == r), w[a:b + 1], 0.0).sum() for a, b, r in zip(F, L, R)])


def _exact_for_all_states(store, unit, F, L, M, R, mean, var):
    full = M == 15
    assert full.sum() >= 2
    assert np.all(var[full] == 0.0)
    assert np.array_equal(mean[full], _weight_totals(store, unit, F[full], L[full], R[full]))


# ---- 1. tiny stores ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_reference(model_type, seed):
    """The reference of a tiny case, once for both algorithms: (a) for the jobs inside the chunks of <= 7 windows, (b) for the others."""
    store, model, alpha, (F, L, M, R) = tiny_case(model_type, seed)
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    reg = store.regions().astype(np.int64)
    small = L < off[5]
    ref = {}
    for unit in MR.UNITS:
        w = MR.weights(store, unit)
        mean, var = MR.moments(A, end, off, w, reg, F, L, M, R)
        ma, va = MR.brute_force(A, end, off, w, reg, F[small], L[small], M[small], R[small])
        mean[small], var[small] = ma, va
        ref[unit] = (mean, var)
    return ref


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed", TINY)
def test_tiny_stores_equal_reference(algo, model_type, seed):
    store, model, alpha, (F, L, M, R) = tiny_case(model_type, seed)
    ref = _tiny_reference(model_type, seed)
    em = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model)
    for unit in MR.UNITS:
        mean, var = em.count_moments(F, L, M, R, unit)
        _close_mean(mean, ref[unit][0], _scale(store, unit), unit)
        _close_var(var, ref[unit][1], _scale(store, unit), unit)
        _exact_for_all_states(store, unit, F, L, M, R, mean, var)
        assert np.sum(var > 1e-3 * _scale(store, unit)) >= 20
    em.close()


# ---- 2. reduced configs --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reduced(cfg):
    """Store, trained model, jobs and reference (c) of a reduced config, once for every test that uses it (nothing here is changed later:
    a pass with the model writes its estimators only)."""
    mt, hifi = next((m, h) for c, m, h in REDUCED if c == cfg)
    store = synth.config(cfg, 0.04)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    em, model = _trained(store, mt, K, alpha)
    em.close()
    _, _, _, jobs = reduced_case(cfg, mt, hifi, model)
    A, end = S.rows(store, model, alpha)
    ref = MR.moments_long(A, end, store.chunk_off, MR.weights(store, "windows"), store.regions().astype(np.int64), *jobs)
    assert np.sum(ref[1] > 1e-3) >= 20
    return store, model, jobs, ref


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("cfg", [c for c, _, _ in REDUCED])
def test_reduced_configs_equal_reference(algo, cfg):
    store, model, (F, L, M, R), ref = _reduced(cfg)
    assert np.diff(store.chunk_off).max() > 2 * 512 + 16
    em = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model)            # the pass whose model the getter answers for
    mean, var = hmm.EM_getCountMomentsForList(em, F, L, M, R)
    _close_mean(mean, ref[0], 1.0, "cfg %d" % cfg)
    _close_var(var, ref[1], 1.0, "cfg %d" % cfg)
    _exact_for_all_states(store, "windows", F, L, M, R, mean, var)
    assert np.sum(var > 1e-3) >= 20
    em.close()


# ---- 3. invariants -------------------------------------------------------------------------------------------------------------------
def test_invariants():
    store, model, (F, L, M, R), ref = _reduced(2)
    W = store.window_len
    em = hmm.EMList(store, model)
    hmm.EM_runOneIterationForList(em, model)
    rng = np.random.default_rng(5)
    got = {u: em.count_moments(F, L, M, R, u) for u in MR.UNITS}
    mean, var = got["windows"]
    assert np.sum(var > 1e-3) >= 20
    post = em.posterior()
    reg = store.regions().astype(np.int64)
    bits = ((M[:, None] >> np.arange(4)) & 1).astype(np.float64)
    for u in MR.UNITS:
        m_u, v_u = got[u]
        _exact_for_all_states(store, u, F, L, M, R, m_u, v_u)             # exactly
        assert not np.any(np.isnan(v_u)) and np.all(v_u >= 0.0) and not np.any(np.isnan(m_u))
        # the mean is the sum of the posterior getter's values
        w = MR.weights(store, u)
        want = np.array([(np.where((r < 0) | (reg[a:b + 1] == r), w[a:b + 1], 0.0) * (post[a:b + 1] @ s)).sum()
                         for a, b, r, s in zip(F, L, R, bits)])
        assert np.all(np.abs(m_u - want) <= 1e-12 * np.abs(want) + 1e-300)
        # the complement of a set has the same variance (the two totals sum to a constant)
        part = M != 15
        _, v_c = em.count_moments(F[part], L[part], 15 & ~M[part], R[part], u)
        _close_var(v_c, v_u[part], _scale(store, u), "complement " + u)
    # single windows: mean = gamma, var = gamma (1 - gamma)
    t = rng.integers(0, store.n_windows, 200)
    m = rng.integers(1, 16, 200)
    gam = np.where(((m[:, None] >> np.arange(4)) & 1).astype(bool), post[t], 0.0).sum(axis=1)
    m1, v1 = em.count_moments(t, t, m)
    assert np.all(np.abs(m1 - gam) <= 1e-12 * gam + 1e-300)
    _close_var(v1, gam * (1.0 - gam), 1.0, "single windows")
    # bitwise: order, call splitting, duplicated jobs
    def same(x, y):
        return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    perm = rng.permutation(F.size)
    assert same(em.count_moments(F[perm], L[perm], M[perm], R[perm]), (mean[perm], var[perm]))
    h = [em.count_moments(F[s], L[s], M[s], R[s]) for s in (slice(0, 100), slice(100, None))]
    assert same((np.concatenate([h[0][0], h[1][0]]), np.concatenate([h[0][1], h[1][1]])), (mean, var))
    dup = np.concatenate([np.arange(F.size), np.arange(0, F.size, 3)])
    assert same(em.count_moments(F[dup], L[dup], M[dup], R[dup]), (mean[dup], var[dup]))
    # more pieces than one device batch holds (2^18): the bits of the same jobs asked alone
    a2 = rng.integers(0, store.n_windows - 1, 300_000)
    big = em.count_moments(a2, a2 + 1, 5)
    pick = np.r_[0:50, 299_950:300_000]
    assert same(em.count_moments(a2[pick], a2[pick] + 1, 5), (big[0][pick], big[1][pick]))
    # a chunk-spanning job = the left-to-right sum of its chunk-local parts as separate jobs
    off = np.asarray(store.chunk_off, np.int64)
    spans = [i for i in range(F.size) if np.searchsorted(off, F[i], "right") != np.searchsorted(off, L[i], "right")]
    assert len(spans) >= 20
    for u in MR.UNITS:
        for i in spans:
            J, Cc, pa, pb, pm = IR.split(off, [F[i]], [L[i]], [M[i]])
            pm_, pv_ = em.count_moments(pa, pb, pm, R[i], u)
            sm = sv = 0.0
            for x, y in zip(pm_, pv_):
                sm += x
                sv += y
            assert (sm, sv) == (got[u][0][i], got[u][1][i]), (u, i)
    # bases = window_len x windows on jobs that avoid every chunk's last window (the only windows that can be shorter)
    ends = off[1:] - 1
    inner = np.array([not np.any((ends >= a) & (ends <= b)) for a, b in zip(F, L)])
    assert inner.sum() >= 100
    mb, vb = got["bases"]
    assert np.all(np.abs(mb[inner] - W * mean[inner]) <= 1e-12 * W * mean[inner])
    _close_var(vb[inner], float(W) ** 2 * var[inner], float(W) ** 2, "bases against windows")
    # scan agrees with seq (same parameters, same last pass)
    seq = hmm.EMList(store, model, algo=N.HF_ALGO_SEQ)
    hmm.EM_runOneIterationForList(seq, model)
    ms, vs = seq.count_moments(F, L, M, R)
    _close_mean(ms, mean, 1.0, "seq")
    _close_var(vs, var, 1.0, "seq")
    seq.close()
    em.close()


# ---- 4. launch variants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"HF_SEG_LAUNCHES": "2"}, {"HF_SUBPASSES": "3"}])
def test_launch_modes_and_sub_passes(env, monkeypatch):
    store, model, (F, L, M, R), ref = _reduced(2)
    em0 = hmm.EMList(store, model)
    hmm.EM_runOneIterationForList(em0, model)
    base = em0.count_moments(F, L, M, R)
    em0.close()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    em = hmm.EMList(store, model)
    if "HF_SEG_LAUNCHES" in env:
        assert em.seg_launches == 2
    else:
        assert em.sub_passes >= 2
    hmm.EM_runOneIterationForList(em, model)
    mean, var = em.count_moments(F, L, M, R)
    _close_mean(mean, ref[0], 1.0)
    _close_var(var, ref[1], 1.0)
    _close_mean(mean, base[0], 1.0)
    _close_var(var, base[1], 1.0)
    full = M == 15
    assert np.array_equal(mean[full], base[0][full]) and np.all(var[full] == 0.0)
    em.close()


# ---- 5. nothing else moves -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_no_disturbance(algo):
    store, model, (F, L, M, R), _ = _reduced(2)
    model = model.copy()
    em_a = hmm.EMList(store, model, algo=algo)
    em_b = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em_a, model)
    st_a = model.estimators.copy()
    hmm.EM_runOneIterationForList(em_b, model)
    assert np.array_equal(st_a, model.estimators)
    em_a.count_moments(F, L, M, R)
    em_a.count_moments(np.concatenate([F, F]), np.concatenate([L, L]), np.concatenate([M, M]), np.concatenate([R, R]), "bases")   # (the buffer grows)
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    assert np.array_equal(em_a.interval_log_probs(F, L, M), em_b.interval_log_probs(F, L, M))
    assert np.array_equal(em_a.labels(), em_b.labels())
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
    def call(cnt, f, l, m, r=None, unit=0, out=(True, True)):
        fp = f.ctypes.data_as(C.POINTER(C.c_int64)) if f is not None else None
        lp = l.ctypes.data_as(C.POINTER(C.c_int64)) if l is not None else None
        mm = np.asarray(m, np.uint8) if m is not None else None
        mp = mm.ctypes.data_as(C.POINTER(C.c_uint8)) if mm is not None else None
        rr = np.asarray(r, np.int32) if r is not None else None
        rp = rr.ctypes.data_as(C.POINTER(C.c_int32)) if rr is not None else None
        o1, o2 = np.empty(max(cnt, 1)), np.empty(max(cnt, 1))
        return L_.hf_get_count_moments(em._h, cnt, fp, lp, mp, rp, unit, o1.ctypes.data_as(C.POINTER(C.c_double)) if out[0] else None,
                                       o2.ctypes.data_as(C.POINTER(C.c_double)) if out[1] else None)
    assert call(1, one(0), one(0), [1]) == N.HF_E_ARG                     # no pass yet
    hmm.EM_runForwardForList(em, model)
    assert call(1, one(0), one(0), [1]) == N.HF_E_ARG                     # forward-only
    hmm.EM_runOneIterationForList(em, model)
    assert call(1, one(0), one(0), [1]) == N.HF_OK
    assert call(1, one(0), one(0), [1], [0], N.HF_COUNT_BASES) == N.HF_OK
    assert call(0, None, None, None, out=(False, False)) == N.HF_OK
    assert call(-1, one(0), one(0), [1]) == N.HF_E_ARG
    assert call(1, None, one(0), [1]) == N.HF_E_ARG
    assert call(1, one(0), None, [1]) == N.HF_E_ARG
    assert call(1, one(0), one(0), None) == N.HF_E_ARG
    assert call(1, one(0), one(0), [1], out=(False, True)) == N.HF_E_ARG
    assert call(1, one(0), one(0), [1], out=(True, False)) == N.HF_E_ARG
    for f, l in [(-1, 0), (0, n), (5, 4), (n, n)]:
        assert call(1, one(f), one(l), [1]) == N.HF_E_ARG, (f, l)
    for m in (0, 16, 255):
        assert call(1, one(0), one(3), [m]) == N.HF_E_ARG, m
    for r in (-2, store.n_regions, 64):
        assert call(1, one(0), one(3), [1], [r]) == N.HF_E_ARG, r
    for u in (-1, 2):
        assert call(1, one(0), one(3), [1], unit=u) == N.HF_E_ARG, u
    assert call(2, one(0, 0), one(3, 3), [1, 0]) == N.HF_E_ARG             # any bad job refuses the call
    with pytest.raises(N.HFError):
        em.count_moments([0], [n], [1])
    with pytest.raises(ValueError):
        em.count_moments([0], [0], [1], unit="reads")
    mean, var = em.count_moments([0, n - 1], [n - 1, n - 1], [15, 3])      # and the context still answers afterwards
    assert mean[0] == n and var[0] == 0.0 and 0.0 <= mean[1] <= 1.0
    em.close()


# ---- 6. command line -------------------------------------------------------------------------------------------------------------
def _cli(args, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


SETS = [("Err", 1), ("Dup", 2), ("Hap", 4), ("Col", 8), ("Err+Dup+Col", 11)]


def test_cli_exact_totals(tmp_path):
    store = synth.config(2, 0.04)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    args = ["-i", str(binp), "-W", "4000", "-n", "2", "-t", "0.001", "-f", "0.95", "-p", str(K)]
    _cli(args, tmp_path / "plain")
    _cli(args + ["--exactTotals"], tmp_path / "exact")
    a, b = tmp_path / "plain", tmp_path / "exact"
    names = sorted(os.listdir(a))
    assert sorted(set(os.listdir(b)) - set(names)) == ["label_totals_exact.tsv"]
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    text = (b / "label_totals_exact.tsv").read_text().splitlines()
    assert text[0] == "#scope\tlabel_set\twindows\tbases_final_labels\tbases_expected\tbases_sd"
    rows = [l.split("\t") for l in text[1:]]
    # the same run through the bindings: the final model, its last full pass, the final labels
    st = synth.WindowStore.read_bin(str(binp))
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, np.zeros((4, 4)))
    em = hmm.EMList(st, model)
    hmm.runHMMFlagger(em, model, 2, 0.001)
    labels = em.labels()
    off = np.asarray(st.chunk_off, np.int64)
    n = st.n_windows
    reg = st.regions().astype(np.int64)
    w = MR.weights(st, "bases")
    scopes = [("all", [(0, n - 1)], -1)]
    for c, ctg in enumerate(st.chunk_ctg):
        k = next((i for i, s in enumerate(scopes) if s[0] == ctg and i > 0), None)
        if k is None:
            scopes.append((ctg, [], -1))
            k = len(scopes) - 1
        rg = scopes[k][1]
        if off[c + 1] > off[c]:
            if rg and rg[-1][1] + 1 == off[c]:
                rg[-1] = (rg[-1][0], int(off[c + 1]) - 1)
            else:
                rg.append((int(off[c]), int(off[c + 1]) - 1))
    scopes += [("region_%d" % r, [(0, n - 1)], r) for r in range(st.n_regions)]
    assert [(r[0], r[1]) for r in rows] == [(s[0], name) for s in scopes for name, _ in SETS]
    assert len(scopes) >= 3 + st.n_regions
    for si, (name, ranges, r) in enumerate(scopes):
        inside = np.zeros(n, bool)
        for x, y in ranges:
            inside[x:y + 1] = True
        if r >= 0:
            inside &= reg == r
        total = 0.0
        for k, (_, mask) in enumerate(SETS):
            row = rows[si * 5 + k]
            mean = var = 0.0
            for x, y in ranges:
                m_, v_ = em.count_moments([x], [y], [mask], [r], "bases")
                mean += m_[0]
                var += v_[0]
            assert int(row[2]) == int(inside.sum())
            assert int(row[3]) == int(w[inside & (((mask >> np.clip(labels, 0, 3)) & 1) == 1) & (labels >= 0)].sum())
            assert row[4] == "%.10g" % mean or abs(float(row[4]) - mean) <= 1e-9 * mean, (row, mean)
            sd = math.sqrt(var)
            assert row[5] == "%.10g" % sd or abs(float(row[5]) - sd) <= 1e-9 * sd, (row, sd)
            if k < 4:
                total += float(row[4])
        assert abs(total - w[inside].sum()) <= 1e-9 * w[inside].sum()
    assert any(float(r[5]) > 0.0 for r in rows)
    em.close()
