"""Exact interval probabilities on the GPU (hf_get_interval_log_probs, hmm.EMList.interval_log_probs, hmm_flagger --runConfidence /
--regionProbs) against the float64 numpy reference (tests/interval_ref.py), which forms them another way: a forward over the whole chunk
with the columns outside the state set zeroed on the interval.  Value checks: |dev - ref| <= 1e-10 + 1e-9 |ref|, -inf equal to -inf."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_bruteforce_cpu import _tiny_store
from test_viterbi_cpu import perturbed_model
from test_viterbi_gpu import SIZES, _trained
import interval_ref as IR
import sampling_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]


def _close(dev, ref):
    dev, ref = np.asarray(dev), np.asarray(ref)
    ok = (np.isneginf(dev) & np.isneginf(ref)) | (np.abs(dev - ref) <= 1e-10 + 1e-9 * np.abs(ref))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, [(int(i), float(dev[i]), float(ref[i])) for i in bad[:8]]


def _jobs(store, rng, n_random):
    """Single windows, whole chunks, chunk-spanning jobs, the whole track (all 15 masks), random ranges."""
    off = np.asarray(store.chunk_off, np.int64)
    N_ = int(off[-1])
    live = np.flatnonzero(np.diff(off) > 0)
    F, L, M = [], [], []
    def add(a, b, m):
        F.append(int(a)); L.append(int(b)); M.append(int(m))
    for m in range(1, 16):
        add(0, N_ - 1, m)
        t = int(rng.integers(0, N_))
        add(t, t, m)
    for c in live[:40]:
        add(off[c], off[c + 1] - 1, rng.integers(1, 16))
        add(off[c], off[c], rng.integers(1, 16))
        add(off[c + 1] - 1, off[c + 1] - 1, rng.integers(1, 16))
    for k in range(min(40, live.size - 1)):
        c0 = live[k]
        c1 = live[min(live.size - 1, k + 1 + int(rng.integers(0, 3)))]
        add(rng.integers(off[c0], off[c0 + 1]), rng.integers(off[c1], off[c1 + 1]), rng.integers(1, 16))
    for _ in range(n_random):
        a = int(rng.integers(0, N_))
        b = min(N_ - 1, a + int(rng.integers(0, 1 + int(rng.choice([4, 64, 700, 3000])))))
        add(a, b, rng.integers(1, 16))
    return np.array(F, np.int64), np.array(L, np.int64), np.array(M, np.int64)


def _reference(store, model, alpha, F, L, M):
    A, end = S.rows(store, model, alpha)
    return IR.log_probs(A, end, store.chunk_off, F, L, M)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed", [(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 0), (N.HF_MODEL_GAUSSIAN, 1),
                                             (N.HF_MODEL_NEGATIVE_BINOMIAL, 2)])
def test_tiny_stores_equal_reference(algo, model_type, seed):
    rng = np.random.default_rng(1950 + seed)
    alpha = synth.HIFI_ALPHA if seed % 2 == 0 else np.zeros((4, 4))
    regions = [20, 31] if seed % 2 == 0 else [25]
    store = _tiny_store(rng, [7, 5, 1, 6, 3, 40], regions)
    model = perturbed_model(store, model_type, 2 + seed % 3, alpha, rng)
    em = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model)
    F, L, M = _jobs(store, rng, 200)
    got = em.interval_log_probs(F, L, M)
    _close(got, _reference(store, model, alpha, F, L, M))
    assert np.all(got[M == 15] == 0.0)
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("cfg,model_type,hifi", [(2, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, True), (4, N.HF_MODEL_GAUSSIAN, True),
                                                 (6, N.HF_MODEL_NEGATIVE_BINOMIAL, False)])
def test_reduced_configs_equal_reference(algo, cfg, model_type, hifi):
    store = synth.config(cfg, 0.04)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    em, model = _trained(store, model_type, K, alpha, algo=algo)
    hmm.EM_runOneIterationForList(em, model)            # the pass whose model the getter answers for
    F, L, M = _jobs(store, np.random.default_rng(cfg), 300)
    got = hmm.EM_getIntervalLogProbsForList(em, F, L, M)
    _close(got, _reference(store, model, alpha, F, L, M))
    em.close()


def test_invariants():
    store = synth.config(2, 0.04)
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, synth.HIFI_ALPHA)
    hmm.EM_runOneIterationForList(em, model)
    rng = np.random.default_rng(5)
    F, L, M = _jobs(store, rng, 300)
    got = em.interval_log_probs(F, L, M)
    assert np.all(got[M == 15] == 0.0)                              # exactly
    assert np.all(got <= 0.0) and not np.any(np.isnan(got))
    # single windows: exp(log_p) = the posterior mass of the set
    t = rng.integers(0, store.n_windows, 200)
    m = rng.integers(1, 16, 200)
    post = em.posterior()
    bits = ((m[:, None] >> np.arange(4)) & 1).astype(bool)
    mass = np.where(bits, post[t], 0.0).sum(axis=1)
    one = np.exp(em.interval_log_probs(t, t, m))
    assert np.allclose(one, mass, rtol=1e-13, atol=1e-300)
    # bitwise: order, call splitting, duplicated jobs
    perm = rng.permutation(F.size)
    assert np.array_equal(em.interval_log_probs(F[perm], L[perm], M[perm]), got[perm])
    halves = np.concatenate([em.interval_log_probs(F[:100], L[:100], M[:100]), em.interval_log_probs(F[100:], L[100:], M[100:])])
    assert np.array_equal(halves, got)
    dup = np.concatenate([np.arange(F.size), np.arange(0, F.size, 3)])
    assert np.array_equal(em.interval_log_probs(F[dup], L[dup], M[dup]), got[dup])
    # a chunk-spanning job = the left-to-right sum of its chunk-local parts as separate jobs
    off = np.asarray(store.chunk_off, np.int64)
    spans = [i for i in range(F.size) if np.searchsorted(off, F[i], "right") != np.searchsorted(off, L[i], "right")]
    assert len(spans) >= 20
    for i in spans:
        J, Cc, pa, pb, pm = IR.split(off, [F[i]], [L[i]], [M[i]])
        parts = em.interval_log_probs(pa, pb, pm)
        s = 0.0
        for v in parts:
            s += v
        assert s == got[i] or (np.isneginf(s) and np.isneginf(got[i])), (i, s, got[i])
    # scan agrees with seq (same parameters, same last pass)
    seq = hmm.EMList(store, model, algo=N.HF_ALGO_SEQ)
    hmm.EM_runOneIterationForList(seq, model)
    _close(seq.interval_log_probs(F, L, M), got)
    seq.close()
    em.close()


@pytest.mark.parametrize("env", [{"HF_SEG_LAUNCHES": "2"}, {"HF_SUBPASSES": "3"}])
def test_launch_modes_and_sub_passes(env, monkeypatch):
    store = synth.synthesize([n * 1000 for n in SIZES], 1000, 10 ** 9, [20], seed=11)
    em0, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, iters=1)
    hmm.EM_runOneIterationForList(em0, model)
    F, L, M = _jobs(store, np.random.default_rng(8), 200)
    base = em0.interval_log_probs(F, L, M)
    _close(base, _reference(store, model, synth.HIFI_ALPHA, F, L, M))
    em0.close()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    em = hmm.EMList(store, model)
    if "HF_SEG_LAUNCHES" in env:
        assert em.seg_launches == 2
    else:
        assert em.sub_passes >= 2
    hmm.EM_runOneIterationForList(em, model)
    got = em.interval_log_probs(F, L, M)
    _close(got, base)
    assert np.array_equal(got[M == 15], base[M == 15])
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
    F, L, M = _jobs(store, np.random.default_rng(3), 200)
    em_a.interval_log_probs(F, L, M)
    em_a.interval_log_probs(np.concatenate([F, F]), np.concatenate([L, L]), np.concatenate([M, M]))   # (the buffer grows)
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
    def call(cnt, f, l, m, out=True):
        fp = f.ctypes.data_as(C.POINTER(C.c_int64)) if f is not None else None
        lp = l.ctypes.data_as(C.POINTER(C.c_int64)) if l is not None else None
        mm = np.asarray(m, np.uint8) if m is not None else None
        mp = mm.ctypes.data_as(C.POINTER(C.c_uint8)) if mm is not None else None
        o = np.empty(max(cnt, 1))
        op = o.ctypes.data_as(C.POINTER(C.c_double)) if out else None
        return L_.hf_get_interval_log_probs(em._h, cnt, fp, lp, mp, op)
    assert call(1, one(0), one(0), [1]) == N.HF_E_ARG                     # no pass yet
    hmm.EM_runForwardForList(em, model)
    assert call(1, one(0), one(0), [1]) == N.HF_E_ARG                     # forward-only
    hmm.EM_runOneIterationForList(em, model)
    assert call(1, one(0), one(0), [1]) == N.HF_OK
    assert call(0, None, None, None, out=False) == N.HF_OK
    assert call(-1, one(0), one(0), [1]) == N.HF_E_ARG
    assert call(1, None, one(0), [1]) == N.HF_E_ARG
    assert call(1, one(0), None, [1]) == N.HF_E_ARG
    assert call(1, one(0), one(0), None) == N.HF_E_ARG
    assert call(1, one(0), one(0), [1], out=False) == N.HF_E_ARG
    for f, l in [(-1, 0), (0, n), (5, 4), (n, n)]:
        assert call(1, one(f), one(l), [1]) == N.HF_E_ARG, (f, l)
    for m in (0, 16, 255):
        assert call(1, one(0), one(3), [m]) == N.HF_E_ARG, m
    assert call(2, one(0, 0), one(3, 3), [1, 0]) == N.HF_E_ARG             # any bad job refuses the call
    with pytest.raises(N.HFError):
        em.interval_log_probs([0], [n], [1])
    got = em.interval_log_probs([0, n - 1], [n - 1, n - 1], [15, 3])      # and the context still answers afterwards
    assert got[0] == 0.0 and got[1] <= 0.0
    em.close()


def _runs(labels, chunk_off):
    """Maximal runs of equal label inside a chunk (a new run at every chunk start): (first, last, label)."""
    off = np.asarray(chunk_off, np.int64)
    out = []
    for c in range(off.size - 1):
        a = int(off[c])
        for t in range(int(off[c]) + 1, int(off[c + 1]) + 1):
            if t == off[c + 1] or labels[t] != labels[a]:
                out.append((a, t - 1, int(labels[a])))
                a = t
    return np.array(out, np.int64).reshape(-1, 3)


def test_against_the_sampler():
    store = synth.config(2, 0.03)
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, synth.HIFI_ALPHA)
    hmm.EM_runOneIterationForList(em, model)
    runs = _runs(em.labels(), store.chunk_off)
    lp = em.interval_log_probs(runs[:, 0], runs[:, 1], 1 << runs[:, 2])
    p = np.exp(lp)
    n = 512
    lab = em.sample_paths(model, n, 4242)
    cs = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(lab == -1, axis=1)], axis=1)   # (shape only)
    support = np.empty(len(runs))
    for i, (a, b, l) in enumerate(runs):
        support[i] = np.mean(np.all(lab[:, a:b + 1] == l, axis=1))
    bound = 6 * np.sqrt(p * (1 - p) / n) + 2 / n
    bad = np.flatnonzero(np.abs(support - p) > bound)
    assert bad.size == 0, [(int(i), float(support[i]), float(p[i])) for i in bad[:8]]
    assert cs.shape[0] == n
    em.close()


def test_full_size_config2():
    store = synth.config(2, 1.0)
    K = hmm.getBestNumberOfCollapsedComps(store)
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, K, synth.HIFI_ALPHA)
    hmm.EM_runOneIterationForList(em, model)
    runs = _runs(em.labels(), store.chunk_off)
    lp = em.interval_log_probs(runs[:, 0], runs[:, 1], 1 << runs[:, 2])
    assert not np.any(np.isnan(lp)) and np.all(lp <= 0.0)
    rng = np.random.default_rng(2)
    pick = rng.choice(len(runs), min(200, len(runs)), replace=False)
    Fr, Lr, Mr = runs[pick, 0], runs[pick, 1], 1 << runs[pick, 2]
    off = np.asarray(store.chunk_off, np.int64)
    a = rng.integers(0, store.n_windows, 200)
    b = np.minimum(store.n_windows - 1, a + rng.integers(0, 2000, 200))
    F = np.concatenate([Fr, a]); L = np.concatenate([Lr, b]); M = np.concatenate([Mr, rng.integers(1, 16, 200)])
    got = em.interval_log_probs(F, L, M)
    assert np.array_equal(got[:len(pick)], lp[pick])
    _close(got, _reference(store, model, synth.HIFI_ALPHA, F, L, M))
    assert off[-1] == store.n_windows
    em.close()


# ---- command line --------------------------------------------------------------------------------------------------------------

def _cli(args, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


NEW_FILES = ["final_label_runs_confidence.bed", "region_label_probabilities.tsv"]


def _rows(path):
    return [l.split("\t") for l in path.read_text().splitlines() if not l.startswith("#")]


@pytest.mark.parametrize("viterbi", [False, True])
def test_cli_run_confidence_and_regions(tmp_path, viterbi):
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    args = ["-i", str(binp), "-W", "4000", "-n", "4", "-P"] + (["--viterbi"] if viterbi else [])
    _cli(args + ["--uncertaintySamples", "4"], tmp_path / "plain")
    a = tmp_path / "plain"
    runs_sup = _rows(a / "final_label_runs_support.bed")
    post_rows = _rows(a / "posterior_prediction_final.bed")
    # regions: a run, a one-window region, an unknown contig, a region of two runs
    r0 = runs_sup[len(runs_sup) // 2]
    ctg = r0[0]
    w0 = post_rows[0]
    regions = [(r0[0], r0[1], r0[2], "run"), (w0[0], w0[1], str(int(w0[1]) + 1), None), ("no_such_contig", "0", "100", "x"),
               (runs_sup[0][0], runs_sup[0][1], runs_sup[1][2], "two")]
    bed = tmp_path / "regions.bed"
    bed.write_text("#ctg\tstart\tend\n" + "".join("\t".join([c, s, e] + ([n] if n else [])) + "\n" for c, s, e, n in regions))
    _cli(args + ["--uncertaintySamples", "4", "--runConfidence", "--regionProbs", str(bed)], tmp_path / "iv")
    b = tmp_path / "iv"
    names = sorted(os.listdir(a))
    assert sorted(set(os.listdir(b)) - set(names)) == NEW_FILES
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    conf = _rows(b / "final_label_runs_confidence.bed")
    assert (b / "final_label_runs_confidence.bed").read_text().splitlines()[0] == "#ctg\tstart\tend\tlabel\tp_all\tqual\tmean_posterior"
    assert [r[:4] for r in conf] == [r[:4] for r in runs_sup]
    for r in conf:
        p, q, mp = float(r[4]), float(r[5]), float(r[6])
        assert 0.0 <= p <= 1.0 and 0.0 <= q <= 100.0 and 0.0 <= mp <= 1.0
        assert p <= mp + 1e-9                                       # all windows in L implies each is
    reg = (b / "region_label_probabilities.tsv").read_text().splitlines()
    head = reg[0].split("\t")
    assert head[:5] == ["#ctg", "start", "end", "name", "n_windows"] and head[5:8] == ["p_any_Err", "p_all_Err", "mean_Err"]
    rows = [l.split("\t") for l in reg[1:]]
    assert [r[3] for r in rows] == ["run", ".", "x", "two"]
    labels = ["Err", "Dup", "Hap", "Col"]
    # the run's region reproduces its p_all
    li = labels.index(r0[3])
    run_conf = conf[len(runs_sup) // 2]
    assert float(rows[0][6 + 3 * li]) == pytest.approx(float(run_conf[4]), rel=1e-5, abs=1e-12)
    # a one-window region reproduces -P's posterior: p_all_L = p_any_L = the posterior of L
    assert rows[1][4] == "1"
    names_p = [x for x in (a / "posterior_prediction_final.bed").read_text().splitlines()[0].split("\t")]
    for l in range(4):
        pa, pl = float(rows[1][5 + 3 * l]), float(rows[1][6 + 3 * l])
        assert pa == pytest.approx(pl, rel=1e-5, abs=1e-9)
        assert float(rows[1][7 + 3 * l]) == pytest.approx(pl, abs=2e-6)
    assert rows[2][4] == "0" and rows[2][5:] == ["NA"] * 12
    assert int(rows[3][4]) >= 2
    assert names_p


def test_cli_one_window_region_equals_posterior_file(tmp_path):
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    args = ["-i", str(binp), "-W", "4000", "-n", "3", "-P"]
    _cli(args, tmp_path / "plain")
    post_rows = _rows(tmp_path / "plain" / "posterior_prediction_final.bed")
    pick = post_rows[:: max(1, len(post_rows) // 20)]
    bed = tmp_path / "regions.bed"
    bed.write_text("".join(f"{r[0]}\t{r[1]}\t{int(r[1]) + 1}\n" for r in pick))
    _cli(args + ["--regionProbs", str(bed)], tmp_path / "iv")
    rows = _rows(tmp_path / "iv" / "region_label_probabilities.tsv")
    for r, pr in zip(rows, pick):
        assert r[4] == "1"
        means = [float(r[7 + 3 * l]) for l in range(4)]
        alls = [float(r[6 + 3 * l]) for l in range(4)]
        assert sum(means) == pytest.approx(1.0, abs=1e-5)
        assert np.allclose(alls, means, rtol=1e-4, atol=1e-6)
        assert np.allclose(alls, [float(x) for x in pr[3:7]], atol=0.0051)     # -P prints the posterior with two decimals
