"""Exact run moments on the GPU (hf_get_run_moments, hmm.EMList.run_moments, hmm_flagger --numBlocks) against the numpy reference
(tests/runs_ref.py), which forms them by other routes: path enumeration with a dynamic programme over the chunks (a) and explicit joint
probabilities (b) on the tiny stores, the uncentred long-double jet over the part (c) plus the stitching formula on the reduced configs.

Tolerance of a variance: |dev - ref| <= ATOL + RTOL scale, in runs^2, ATOL = 1e-12 (the absolute term of the count-moments tests, whose
quantity has the same scale of 1 per window) and RTOL = 2e-11: a hundredfold of 1.92e-13, the largest relative deviation of the centred
float64 recursion from (c) over the jobs of the tiny-store and reduced-config tests, measured on the CPU by
tests/test_runs_cpu.py::test_centred_float64_against_the_long_double_jet (the hundredfold is for the device's association order and its
differently rounded rows and posterior); under the standing 1e-9.  scale is the reference variance; with joins the variance is a sum of
terms of both signs, and scale is the sum of the absolute values of the stitching formula's terms (runs_ref.stitch).
A mean: |dev - ref| <= 1e-12 + 1e-9 |ref|, the posterior tests' bound.
Every test prints its largest absolute and relative deviations before it asserts (pytest -s).  Measured on an MI355X (both algorithms,
apart and joined): tiny stores 2.5e-14 runs^2 absolute, 9.4e-13 of the scale (the other two stores 1.6e-13 and 9.4e-14), means 1.2e-14
relative; reduced configs, as they are and with their chunks cut, 5.7e-14 absolute, 8.6e-14 of the scale, means 5.8e-15 relative."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_moments_cpu import REDUCED, TINY
from test_runs_cpu import ATOL, RTOL, TINY_JOINS, reduced_jobs, tiny_jobs
from test_viterbi_gpu import _trained
import interval_ref as IR
import runs_ref as RR
import sampling_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]


def _close_var(dev, ref, scale, what=""):
    dev, ref, scale = np.asarray(dev), np.asarray(ref), np.asarray(scale)
    err = np.abs(dev - ref)
    big = ref > 1e-3
    print("%s variance: max |dev - ref| %.3e, max deviation relative to the scale (var > 1e-3) %.3e over %d jobs"
          % (what, float(np.max(err, initial=0.0)), float(np.max(err[big] / scale[big], initial=0.0)), int(big.sum())))
    bad = np.flatnonzero(~(err <= ATOL + RTOL * scale))
    assert bad.size == 0, [(int(i), float(dev[i]), float(ref[i])) for i in bad[:8]]
    assert np.all(dev >= 0.0)


def _close_mean(dev, ref, what=""):
    dev, ref = np.asarray(dev), np.asarray(ref)
    err = np.abs(dev - ref)
    print("%s mean: max relative deviation %.3e" % (what, float(np.max(err / np.maximum(np.abs(ref), 1e-300), initial=0.0))))
    bad = np.flatnonzero(~(err <= 1e-12 + 1e-9 * np.abs(ref)))
    assert bad.size == 0, [(int(i), float(dev[i]), float(ref[i])) for i in bad[:8]]


def _exact_for_all_states(off, F, L, M, joins, mean, var):
    full = M == 15
    assert full.sum() >= 2
    assert np.all(var[full] == 0.0)
    assert np.array_equal(mean[full], RR.groups(off, F[full], L[full], joins).astype(np.float64))


def _same(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


# ---- 1. tiny stores ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_reference(model_type, seed, joined):
    """The reference of a tiny case, once for both algorithms: (a) for the jobs inside the chunks of <= 7 windows, (b) for the others."""
    store, model, alpha, (F, L, M) = tiny_jobs(model_type, seed)
    joins = TINY_JOINS if joined else None
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    small = L < off[5]
    mean, var, scale = RR.pairwise(A, end, off, F, L, M, joins)
    mean[small], var[small] = RR.brute_force(A, end, off, F[small], L[small], M[small], joins)
    return mean, var, scale


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed", TINY)
def test_tiny_stores_equal_reference(algo, model_type, seed):
    store, model, alpha, (F, L, M) = tiny_jobs(model_type, seed)
    off = np.asarray(store.chunk_off, np.int64)
    em = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model)
    for joined in (False, True):
        joins = TINY_JOINS if joined else None
        ref = _tiny_reference(model_type, seed, joined)
        mean, var = em.run_moments(F, L, M, joins)
        what = "tiny %d %s" % (seed, "joined" if joined else "apart")
        _close_mean(mean, ref[0], what)
        _close_var(var, ref[1], ref[2], what)
        _exact_for_all_states(off, F, L, M, joins, mean, var)
        assert np.sum(var > 1e-3) >= 20
    assert _same(em.run_moments(F, L, M, np.zeros(6, bool)), em.run_moments(F, L, M))      # no join: NULL
    em.close()


# ---- 2. reduced configs --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trained_model(cfg):
    mt, hifi = next((m, h) for c, m, h in REDUCED if c == cfg)
    store = synth.config(cfg, 0.04)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    em, model = _trained(store, mt, K, alpha)
    em.close()
    return model


def _reduced_model(cfg, split):
    """Store, trained model, jobs and joins of a reduced config.  Every contig of these stores is one chunk, so joined, set between
    consecutive chunks of one contig, is all zero; split: the same windows and model with the chunks cut (runs_ref.split_store), which
    gives joined groups of two and three chunks, the middle one of one window."""
    mt, hifi = next((m, h) for c, m, h in REDUCED if c == cfg)
    store, model, alpha, (F, L, M) = reduced_jobs(cfg, mt, hifi, split, _trained_model(cfg))
    return store, model, alpha, (F, L, M), RR.contig_joins(store)


@functools.lru_cache(maxsize=None)
def _reduced(cfg, split):
    """Store, trained model, jobs, joins and reference (c) of a reduced config, once for every test that uses it (nothing here is changed
    later: a pass with the model writes its estimators only)."""
    store, model, alpha, (F, L, M), joins = _reduced_model(cfg, split)
    A, end = S.rows(store, model, alpha)
    ref = RR.jet_long(A, end, store.chunk_off, F, L, M, joins)
    assert np.sum(ref[1] > 1e-3) >= 20
    return store, model, (F, L, M), joins, ref


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("split", [False, True], ids=["contigs", "cut"])
@pytest.mark.parametrize("cfg", [c for c, _, _ in REDUCED])
def test_reduced_configs_equal_reference(algo, cfg, split):
    store, model, (F, L, M), joins, ref = _reduced(cfg, split)
    assert np.diff(store.chunk_off).max() > 2 * 512 + 16
    assert joins.sum() >= (40 if split else 0)
    em = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model)            # the pass whose model the getter answers for
    mean, var = hmm.EM_getRunMomentsForList(em, F, L, M, joins)
    what = "cfg %d%s" % (cfg, " cut" if split else "")
    _close_mean(mean, ref[0], what)
    _close_var(var, ref[1], ref[2], what)
    _exact_for_all_states(store.chunk_off, F, L, M, joins, mean, var)
    assert np.sum(var > 1e-3) >= 20
    assert not np.any(np.isnan(mean)) and not np.any(np.isnan(var))
    em.close()


_CHILD = """
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from flagger_amd import hmm
from test_runs_gpu import _reduced_model
store, model, alpha, (F, L, M), joins = _reduced_model(2, True)
os.environ["HF_SUBPASSES"] = "2"
em = hmm.EMList(store, model)
assert em.sub_passes >= 2, em.sub_passes
hmm.EM_runOneIterationForList(em, model)
mean, var = em.run_moments(F, L, M, joins)
np.save(sys.argv[2], np.stack([mean, var]))
em.close()
"""


def test_sub_passes_give_the_same_bits(tmp_path):
    """A context that runs its full pass in several sub-passes (HF_SUBPASSES=2, in a child process) returns the bits of the
    one-sub-pass context."""
    store, model, (F, L, M), joins, ref = _reduced(2, True)
    em = hmm.EMList(store, model)
    assert em.sub_passes == 1
    hmm.EM_runOneIterationForList(em, model)
    base = em.run_moments(F, L, M, joins)
    em.close()
    out = str(tmp_path / "sub.npy")
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "tests"), out], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")])))
    assert r.returncode == 0, r.stderr[-2000:]
    sub = np.load(out)
    assert np.array_equal(sub[0], base[0]) and np.array_equal(sub[1], base[1])


# ---- 3. identities against what the device already answers ------------------------------------------------------------------------------
def test_mean_is_the_sum_of_pair_posteriors():
    """For a single part [a, b]: mean = gamma_a(S) + sum_t [gamma_t(S) - P(s_{t-1} in S, s_t in S)], gamma from hf_get_posterior, the
    pair probability from hf_get_interval_log_probs; 1e-9 relative, the standing bound of the posterior tests.  A part of one window:
    the count is 1[s_a in S], so the mean is the count moments' mean of that window, bitwise, and the variance gamma (1 - gamma)."""
    store, model, _, _, _ = _reduced(2, False)
    off = np.asarray(store.chunk_off, np.int64)
    c = int(np.argmax(np.diff(off)))
    a, b = int(off[c]), int(off[c + 1]) - 1
    em = hmm.EMList(store, model)
    hmm.EM_runOneIterationForList(em, model)
    post = em.posterior()
    t = np.arange(a + 1, b + 1)
    worst = 0.0
    for mask in (1, 2, 4, 8, 11, 6, 15):
        bits = ((mask >> np.arange(4)) & 1).astype(np.float64)
        gam = post[a:b + 1] @ bits
        stay = np.exp(em.interval_log_probs(t - 1, t, mask))
        starts = gam[1:] - stay
        # whole chunk, a part that ends inside it, a part that starts inside it
        for x, y in ((a, b), (a, a + 700), (a + 513, b), (a + 5, a + 6)):
            want = gam[x - a] + starts[x - a:y - a].sum()
            got, _ = em.run_moments([x], [y], [mask])
            worst = max(worst, abs(got[0] - want) / max(want, 1e-300))
            assert abs(got[0] - want) <= 1e-9 * want + 1e-300, (mask, x, y, got[0], want)
    print("mean against posterior and interval getters: max relative deviation %.3e" % worst)
    rng = np.random.default_rng(11)
    w = rng.integers(0, store.n_windows, 200)
    m = rng.integers(1, 16, 200)
    m1, v1 = em.run_moments(w, w, m)
    mc, vc = em.count_moments(w, w, m)
    assert np.array_equal(m1, mc)
    assert np.all(np.abs(v1 - m1 * (1.0 - m1)) <= ATOL + RTOL * m1 * (1.0 - m1))
    assert np.all(np.abs(v1 - vc) <= ATOL + RTOL * vc)
    em.close()


# ---- 4. a job depends on nothing but itself ----------------------------------------------------------------------------------------------
def test_bitwise_independence_of_the_call():
    store, model, (F, L, M), joins, ref = _reduced(2, True)
    em = hmm.EMList(store, model)
    hmm.EM_runOneIterationForList(em, model)
    rng = np.random.default_rng(5)
    mean, var = em.run_moments(F, L, M, joins)
    assert np.sum(var > 1e-3) >= 20
    assert _same(em.run_moments(F, L, M, joins), (mean, var))                                  # two consecutive calls on the same pass
    perm = rng.permutation(F.size)
    assert _same(em.run_moments(F[perm], L[perm], M[perm], joins), (mean[perm], var[perm]))
    dup = np.concatenate([np.arange(F.size), np.arange(0, F.size, 3)])
    assert _same(em.run_moments(F[dup], L[dup], M[dup], joins), (mean[dup], var[dup]))
    pick = np.r_[0:40, F.size - 40:F.size]
    for i in pick:                                                                                  # one job per call
        assert _same(em.run_moments(F[i:i + 1], L[i:i + 1], M[i:i + 1], joins), (mean[i:i + 1], var[i:i + 1])), i
    # a chunk-spanning job with no join = the left-to-right sum of its chunk-local parts as separate jobs
    off = np.asarray(store.chunk_off, np.int64)
    m0, v0 = em.run_moments(F, L, M)
    spans = [i for i in range(F.size) if np.searchsorted(off, F[i], "right") != np.searchsorted(off, L[i], "right")]
    assert len(spans) >= 20
    differ = 0
    for i in spans:
        J, Cc, pa, pb, pm = IR.split(off, [F[i]], [L[i]], [M[i]])
        pm_, pv_ = em.run_moments(pa, pb, pm)
        sm = sv = 0.0
        for x, y in zip(pm_, pv_):
            sm += x
            sv += y
        assert (sm, sv) == (m0[i], v0[i]), i
        differ += mean[i] != m0[i]
    assert differ >= 10                                                                             # and the joins do change those jobs
    em.close()


# ---- 5. nothing else moves -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_no_disturbance(algo):
    store, model, (F, L, M), joins, _ = _reduced(2, True)
    model = model.copy()
    em_a = hmm.EMList(store, model, algo=algo)
    em_b = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em_a, model)
    st_a = model.estimators.copy()
    hmm.EM_runOneIterationForList(em_b, model)
    assert np.array_equal(st_a, model.estimators)
    em_a.run_moments(F, L, M, joins)
    em_a.run_moments(np.concatenate([F, F]), np.concatenate([L, L]), np.concatenate([M, M]))       # (the buffer grows)
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    assert np.array_equal(em_a.interval_log_probs(F, L, M), em_b.interval_log_probs(F, L, M))
    assert _same(em_a.count_moments(F, L, M), em_b.count_moments(F, L, M))
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
    nc = len(store.chunk_off) - 1
    one = lambda *a: np.array(a, np.int64)
    def call(cnt, f, l, m, joined=None, out=(True, True)):
        fp = f.ctypes.data_as(C.POINTER(C.c_int64)) if f is not None else None
        lp = l.ctypes.data_as(C.POINTER(C.c_int64)) if l is not None else None
        mm = np.asarray(m, np.uint8) if m is not None else None
        mp = mm.ctypes.data_as(C.POINTER(C.c_uint8)) if mm is not None else None
        jj = np.asarray(joined, np.uint8) if joined is not None else None
        jp = jj.ctypes.data_as(C.POINTER(C.c_uint8)) if jj is not None else None
        o1, o2 = np.empty(max(cnt, 1)), np.empty(max(cnt, 1))
        return L_.hf_get_run_moments(em._h, cnt, fp, lp, mp, jp, o1.ctypes.data_as(C.POINTER(C.c_double)) if out[0] else None,
                                     o2.ctypes.data_as(C.POINTER(C.c_double)) if out[1] else None)
    assert call(1, one(0), one(0), [1]) == N.HF_E_ARG                     # no pass yet
    hmm.EM_runForwardForList(em, model)
    assert call(1, one(0), one(0), [1]) == N.HF_E_ARG                     # forward-only
    hmm.EM_runOneIterationForList(em, model)
    assert call(1, one(0), one(0), [1]) == N.HF_OK
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
    first_joined = np.zeros(nc, np.uint8)
    first_joined[0] = 1
    assert call(1, one(0), one(3), [1], first_joined) == N.HF_E_ARG
    assert call(1, one(0), one(3), [1], np.zeros(nc, np.uint8)) == N.HF_OK
    assert call(2, one(0, 0), one(3, 3), [1, 0]) == N.HF_E_ARG             # any bad job refuses the call
    with pytest.raises(N.HFError):
        em.run_moments([0], [n], [1])
    with pytest.raises(ValueError):
        em.run_moments([0], [0], [1], np.zeros(nc + 1, bool))
    mean, var = em.run_moments([0, n - 1], [n - 1, n - 1], [15, 3])        # and the context still answers afterwards
    assert mean[0] == RR.groups(store.chunk_off, [0], [n - 1], None)[0] and var[0] == 0.0 and 0.0 <= mean[1] <= 1.0
    em.close()


# ---- 7. command line -------------------------------------------------------------------------------------------------------------
def _cli(args, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


SETS = [("Err", 1), ("Dup", 2), ("Hap", 4), ("Col", 8), ("Err+Dup+Col", 11)]


def _final_blocks(labels, off, joins, c0, c1, mask):
    """The runs of the set in the final labels over the chunks c0 .. c1 - 1, a run continuing into a joined chunk."""
    cnt, prev = 0, False
    for c in range(c0, c1):
        if c == c0 or not joins[c]:
            prev = False
        lab = labels[off[c]:off[c + 1]]
        now = (lab >= 0) & (((mask >> np.clip(lab, 0, 3)) & 1) == 1)
        if now.size:
            before = np.concatenate([[prev], now[:-1]])
            cnt += int(np.sum(now & ~before))
            prev = bool(now[-1])
    return cnt


def test_cli_num_blocks(tmp_path):
    store = RR.split_store(synth.config(2, 0.04))      # chunks cut, so that blocks cross chunk boundaries inside a contig
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    args = ["-i", str(binp), "-W", "4000", "-n", "2", "-t", "0.001", "-f", "0.95", "-p", str(K)]
    _cli(args, tmp_path / "plain")
    _cli(args + ["--numBlocks"], tmp_path / "blocks")
    a, b = tmp_path / "plain", tmp_path / "blocks"
    names = sorted(os.listdir(a))
    assert sorted(set(os.listdir(b)) - set(names)) == ["label_blocks_exact.tsv"]
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    text = (b / "label_blocks_exact.tsv").read_text().splitlines()
    assert text[0] == "#scope\tlabel_set\tblocks_final_labels\tblocks_expected\tblocks_sd"
    rows = [l.split("\t") for l in text[1:]]
    # the same run through the bindings: the final model, its last full pass, the final labels
    st = synth.WindowStore.read_bin(str(binp))
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, np.zeros((4, 4)))
    em = hmm.EMList(st, model)
    hmm.runHMMFlagger(em, model, 2, 0.001)
    labels = em.labels()
    off = np.asarray(st.chunk_off, np.int64)
    nc = off.size - 1
    joins = RR.contig_joins(st)
    assert joins.sum() >= 2
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
    assert [(r[0], r[1]) for r in rows] == [(s[0], name) for s in scopes for name, _ in SETS]
    assert len(scopes) >= 3
    bed = [l.split("\t") for l in (b / "final_flagger_prediction.bed").read_text().splitlines()[1:]]
    for si, (name, ranges) in enumerate(scopes):
        for k, (set_name, mask) in enumerate(SETS):
            row = rows[si * 5 + k]
            mean = var = 0.0
            blocks = 0
            for c0, c1 in ranges:
                m_, v_ = em.run_moments([off[c0]], [off[c1] - 1], [mask], joins)
                mean += m_[0]
                var += v_[0]
                blocks += _final_blocks(labels, off, joins, c0, c1, mask)
            assert int(row[2]) == blocks, row
            if k < 4:                                   # a single label: the rows of that label in the final BED
                in_bed = sum(1 for l in bed if l[3] == set_name and (name == "all" or l[0] == name))
                assert blocks == in_bed, (row, in_bed)
            assert row[3] == "%.10g" % mean or abs(float(row[3]) - mean) <= 1e-9 * mean, (row, mean)
            sd = math.sqrt(var)
            assert row[4] == "%.10g" % sd or abs(float(row[4]) - sd) <= 1e-9 * sd, (row, sd)
    for k in range(5):                                  # the contig scopes sum to "all"
        assert int(rows[k][2]) == sum(int(rows[si * 5 + k][2]) for si in range(1, len(scopes)))
    assert any(float(r[4]) > 0.0 for r in rows)
    em.close()
