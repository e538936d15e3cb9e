"""Posterior path sampling on the GPU (hf_sample_paths, hmm.EMList.sample_paths, hmm_flagger --uncertaintySamples) against the
float64 numpy sampler (tests/sampling_ref.py), which uses the same uniforms and the same draw rule.

Exactness.  The device's forward vectors are formed in another association order than the reference's (lane products and scans), so a
draw whose uniform lands within rounding of a cumulative-sum boundary may go the other way.  A sample may therefore differ from the
reference only like this: in a chunk, the last differing window (in backward order: the first one met) was decided by a draw whose
reference margin min_p |x - c_p| / c_3 is below 1e-12, and only earlier windows of that chunk differ after it."""
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
import sampling_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]
MARGIN = 1e-12


def _near_tie_events(got, ref, marg, fmarg, chunk_off):
    """Check `got` against `ref` ([K][N] labels) under the rule above; returns the number of near-tie events (asserts the rest)."""
    off = np.asarray(chunk_off, np.int64)
    events = 0
    for k in np.flatnonzero((got != ref).any(axis=1)):
        diff = np.flatnonzero(got[k] != ref[k])
        for c in np.unique(np.searchsorted(off, diff, side="right") - 1):
            t_last = diff[(diff >= off[c]) & (diff < off[c + 1])].max()
            m = fmarg[k, c] if t_last == off[c + 1] - 1 else marg[k, t_last + 1]
            assert m < MARGIN, ("sample", k, "chunk", c, "window", t_last, "reference margin", m)
            events += 1
    return events


def _reference(store, model, alpha, seed, ks):
    A, end = S.rows(store, model, alpha)
    return S.ffbs(A, end, store.chunk_off, seed, ks)


def _check(store, model, alpha, got, seed, first=0):
    ref, marg, fmarg = _reference(store, model, alpha, seed, range(first, first + got.shape[0]))
    events = _near_tie_events(got, ref, marg, fmarg, store.chunk_off)
    assert events <= 1, events       # none expected at these sizes
    return ref


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed", [(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 0), (N.HF_MODEL_GAUSSIAN, 1),
                                             (N.HF_MODEL_NEGATIVE_BINOMIAL, 2)])
def test_tiny_stores_equal_numpy_sampler(algo, model_type, seed):
    rng = np.random.default_rng(950 + seed)
    alpha = synth.HIFI_ALPHA if seed % 2 == 0 else np.zeros((4, 4))
    regions = [20, 31] if seed % 2 == 0 else [25]
    store = _tiny_store(rng, [7, 5, 1, 6, 3, 40], regions)
    model = perturbed_model(store, model_type, 2 + seed % 3, alpha, rng)
    em = hmm.EMList(store, model, algo=algo)
    got = hmm.EM_samplePathsForList(em, model, 200, 17 + seed)
    assert got.shape == (200, store.n_windows) and got.dtype == np.int8
    _check(store, model, alpha, got, 17 + seed)
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("cfg,model_type,hifi,scale", [(2, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, True, 0.04),
                                                       (4, N.HF_MODEL_GAUSSIAN, True, 0.04),
                                                       (6, N.HF_MODEL_NEGATIVE_BINOMIAL, False, 0.04)])
def test_reduced_configs_equal_numpy_sampler(algo, cfg, model_type, hifi, scale):
    store = synth.config(cfg, scale)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    em, model = _trained(store, model_type, K, alpha, algo=algo)
    got = em.sample_paths(model, 16, 2024, first_sample=5)
    _check(store, model, alpha, got, 2024, first=5)
    em.close()


@pytest.mark.parametrize("env", [{}, {"HF_SEG_LAUNCHES": "2"}, {"HF_SUBPASSES": "3"}])
def test_segmentation_edge_cases(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    store = synth.synthesize([n * 1000 for n in SIZES], 1000, 10 ** 9, [20], seed=11)
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, iters=1)
    got = em.sample_paths(model, 24, 3)
    _check(store, model, synth.HIFI_ALPHA, got, 3)
    em.close()


def test_scan_equals_seq():
    store = synth.config(2, 0.05)
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, synth.HIFI_ALPHA)
    seq = hmm.EMList(store, model, algo=N.HF_ALGO_SEQ)
    a = em.sample_paths(model, 32, 99)
    b = seq.sample_paths(model, 32, 99)
    _, marg, fmarg = _reference(store, model, synth.HIFI_ALPHA, 99, range(32))
    assert _near_tie_events(a, b, marg, fmarg, store.chunk_off) <= 1
    em.close(); seq.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_grouping_and_seeds(algo):
    store = synth.config(2, 0.03)
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, synth.HIFI_ALPHA, iters=1, algo=algo)
    whole = em.sample_paths(model, 64, 5)
    parts = np.concatenate([em.sample_paths(model, 24, 5), em.sample_paths(model, 40, 5, first_sample=24)])
    assert np.array_equal(whole, parts)
    assert np.array_equal(whole, em.sample_paths(model, 64, 5))
    other = em.sample_paths(model, 64, 6)
    assert not np.array_equal(whole, other)
    assert np.mean(whole != other) > 1e-4
    assert np.array_equal(whole[10:20], em.sample_paths(model, 10, 5, first_sample=10))
    em.close()


def test_marginals_agree_with_the_posterior():
    store = synth.config(2, 0.07)
    assert 80_000 < store.n_windows < 140_000
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, synth.HIFI_ALPHA)
    hmm.EM_runOneIterationForList(em, model)            # the posterior of the parameters the samples use
    post = em.posterior()
    n = 256
    lab = em.sample_paths(model, n, 31337)
    for s in range(4):
        x = (lab == s).sum(axis=1).astype(np.float64) - post[:, s].sum()    # per sample: windows in s minus their expectation
        sd = x.std(ddof=1)
        if sd == 0:
            assert abs(x.mean()) < 1e-6 * store.n_windows
            continue
        z = x.mean() / (sd / np.sqrt(n))                   # samples are independent: a t statistic of the summed deviations
        assert abs(z) < 5, (s, z)
    freq = np.stack([(lab == s).mean(axis=0) for s in range(4)], axis=1)
    mad = np.mean(np.abs(freq - post))
    expect = np.mean(np.sqrt(2 / np.pi * post * (1 - post) / n))
    assert mad <= 1.25 * expect + 1e-4, (mad, expect)
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
    va, vb = em_a.viterbi(model), em_b.viterbi(model)
    other = model.copy()                                 # samples with DIFFERENT parameters, twice (the buffers grow in between)
    v = other.param_vector().reshape(other.numberOfRegions, -1)
    v[:, 27:27 + 4 * 16] *= 1.1
    other.set_param_vector(v.ravel())
    em_a.sample_paths(other, 8, 1)
    em_a.sample_paths(other, 40, 2)
    L = N.lib()
    lab = np.empty(store.n_windows, np.int8)
    assert L.hf_get_viterbi_labels(em_a._h, lab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
    assert np.array_equal(lab, va[0]) and np.array_equal(va[0], vb[0])
    ll = np.empty(store.n_chunks)
    assert L.hf_get_viterbi_chunk_log_probs(em_a._h, ll.ctypes.data_as(C.POINTER(C.c_double))) == N.HF_OK
    assert np.array_equal(ll, va[1])
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
    L = N.lib()
    lab = np.empty(store.n_windows, np.int8)
    lp = lab.ctypes.data_as(C.POINTER(C.c_int8))
    assert L.hf_get_sample_labels(em._h, 0, lp) == N.HF_E_ARG                 # before any call
    assert L.hf_sample_finish(em._h, None) == N.HF_E_ARG
    p = model.params()
    assert L.hf_sample_paths(em._h, C.byref(p), 0, 0, 1, None) == N.HF_E_ARG
    cap = em.sample_capacity
    assert cap >= 64
    assert L.hf_sample_paths(em._h, C.byref(p), 0, cap + 1, 1, None) == N.HF_E_ARG
    assert L.hf_sample_paths(em._h, C.byref(p), 0, 3, 1, None) == N.HF_OK
    assert L.hf_get_sample_labels(em._h, 0, lp) == N.HF_E_ARG                 # launched, not finished
    assert L.hf_sample_finish(em._h, None) == N.HF_OK
    assert L.hf_get_sample_labels(em._h, 2, lp) == N.HF_OK
    assert L.hf_get_sample_labels(em._h, 3, lp) == N.HF_E_ARG
    assert L.hf_get_sample_labels(em._h, -1, lp) == N.HF_E_ARG
    R = model.numberOfRegions
    bad = model.copy()
    v = bad.param_vector().reshape(R, -1)
    v[:, 20:24] = 0.0                                    # start row: no path has weight
    bad.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.sample_paths(bad, 4, 1)
    assert ei.value.code == N.HF_E_SCALE
    nan = model.copy()
    v = nan.param_vector().reshape(R, -1)
    v[:, 27 + 3 * 16] = np.nan                           # mean of Col, component 0
    nan.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.sample_paths(nan, 4, 1)
    assert ei.value.code == N.HF_E_NAN
    assert L.hf_get_sample_labels(em._h, 0, lp) == N.HF_E_ARG                 # the last call failed: nothing to get
    got = em.sample_paths(model, 4, 1)                    # and the context still samples afterwards
    _check(store, model, synth.HIFI_ALPHA, got, 1)
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunk_list(algo):
    full = synth.synthesize([50_000], 1000, 20_000, [20], seed=2)
    store = full.subset_chunks([])
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, full, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model, algo=algo)
    got = em.sample_paths(model, 5, 1)
    assert got.shape == (5, 0)
    em.close()


# ---- command line --------------------------------------------------------------------------------------------------------------

def _cli(args, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


NEW_FILES = ["final_label_runs_support.bed", "posterior_samples_summary.tsv"]


@pytest.mark.parametrize("viterbi", [False, True])
def test_cli_uncertainty_samples(tmp_path, viterbi):
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    args = ["-i", str(binp), "-W", "4000", "-n", "4", "-P"] + (["--viterbi"] if viterbi else [])
    _cli(args, tmp_path / "plain")
    _cli(args + ["--uncertaintySamples", "32", "--uncertaintySeed", "7"], tmp_path / "smp")
    a, b = tmp_path / "plain", tmp_path / "smp"
    names = sorted(os.listdir(a))
    assert sorted(set(os.listdir(b)) - set(names)) == NEW_FILES
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    # the runs are the final BED's blocks (no --minimumLengths), in order
    final = [l.split("\t")[:4] for l in (b / "final_flagger_prediction.bed").read_text().splitlines()[1:]]
    runs = [l.split("\t") for l in (b / "final_label_runs_support.bed").read_text().splitlines() if not l.startswith("#")]
    assert [r[:4] for r in runs] == final
    for r in runs:
        sup, frac = float(r[4]), float(r[5])
        assert 0.0 <= sup <= frac <= 1.0
    # bases: every sample assigns every base once
    total = sum(int(r[2]) - int(r[1]) for r in runs)
    rows = [l.split("\t") for l in (b / "posterior_samples_summary.tsv").read_text().splitlines() if not l.startswith("#")]
    allr = [r for r in rows if r[0] == "all"]
    assert [r[1] for r in allr] == ["Err", "Dup", "Hap", "Col"]
    assert abs(sum(float(r[3]) for r in allr) - total) <= 0.01
    assert sum(int(r[2]) for r in allr) == total
    for r in rows:
        q025, q500, q975 = int(r[5]), int(r[6]), int(r[7])
        assert q025 <= q500 <= q975
    # the same samples from the library: the summary's means
    st = synth.WindowStore.read_bin(str(binp))
    assert abs(sum(float(r[8]) for r in allr) - st.n_windows) <= 0.01
