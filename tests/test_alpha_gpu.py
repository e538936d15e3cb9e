"""The alpha statistics on the GPU (hf_set_alpha_stats / hf_get_alpha_stats, hmm.EMList.alpha_stats, hmm_flagger --fitAlpha) against the
float64 numpy reference (tests/alpha_ref.py).  G is a signed sum, so its tolerance is relative to the magnitude of what is summed (the
reference's Gabs, the same sum with |d_c u_c|):
    |G - G_ref| <= 1e-9 max(Gabs, 1e-6 max Gabs)        |H - H_ref| <= 1e-9 max(H_ref, 1e-6 max H_ref)
1e-9 relative is the project's bar for the statistics vector."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_bruteforce_cpu import _tiny_store
from test_viterbi_cpu import perturbed_model
from test_viterbi_gpu import _trained
from test_alpha_cpu import DISTINCT, TRUE
import alpha_ref as AR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
ALPHAS = {"zero": np.zeros((4, 4)), "hifi": synth.HIFI_ALPHA, "ont_r10": synth.ONT_R10_ALPHA, "distinct": DISTINCT}
MODELS = [N.HF_MODEL_TRUNC_EXP_GAUSSIAN, N.HF_MODEL_GAUSSIAN]
# (algorithm, environment of hf_create)
MODES = {"seq": (N.HF_ALGO_SEQ, {}), "scan": (N.HF_ALGO_SCAN, {}), "scan_two_launches": (N.HF_ALGO_SCAN, {"HF_SEG_LAUNCHES": "2"}),
         "scan_sub_passes": (N.HF_ALGO_SCAN, {"HF_SUBPASSES": "3"})}


def _close(got, ref, what=""):
    """got [R][2][4][4] against the reference's dict, each entry against its own magnitude."""
    for k, mag in ((0, ref["Gabs"]), (1, ref["H"])):
        want = ref["G"] if k == 0 else ref["H"]
        tol = 1e-9 * np.maximum(mag, 1e-6 * mag.max())
        err = np.abs(got[:, k] - want)
        bad = np.argwhere(~(err <= tol))
        assert bad.size == 0, (what, "GH"[k], [(tuple(i), float(got[:, k][tuple(i)]), float(want[tuple(i)]), float(tol[tuple(i)])) for i in bad[:6]])


def _store(name):
    if name == "config2":
        return synth.config(2, scale=0.01)
    if name == "ragged":     # the multi-region ragged store of test_estep_gpu.py: chunks of 1, 2, 3, 63, 64, 65, 129 ... windows, two regions
        W = 100
        lens = [1 * W, 2 * W, 3 * W, 63 * W, 64 * W, 65 * W, 129 * W, 1000 * W + 37, 5 * W - 1, 2049 * W]
        return synth.synthesize(lens, W, 10_000_000, [20, 25], seed=5, region_run_bases=(2_000, 30_000))
    return _tiny_store(np.random.default_rng(77), [1, 2, 1, 2, 9, 1, 2], [20, 31], avg_len=6000)      # chunks of one and two windows


def _model(store, name, model_type, alpha):
    if name == "tiny":
        return perturbed_model(store, model_type, 3, alpha, np.random.default_rng(5))
    em, model = _trained(store, model_type, 3, alpha, iters=1)
    em.close()
    return model


def _stats(store, model, mode, monkeypatch):
    algo, env = MODES[mode]
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        em = hmm.EMList(store, model, algo=algo)
    if mode == "scan_two_launches":
        assert em.seg_launches == 2
    em.set_alpha_stats(True)
    hmm.EM_runOneIterationForList(em, model)
    got = em.alpha_stats()
    again = em.alpha_stats()
    assert np.array_equal(got, again)                 # two calls on the same pass
    em.close()
    return got


# ---- 1., 2. G and H against the reference; scan, seq and the launch modes against each other ---------------------------------------
@pytest.mark.parametrize("alpha_name", list(ALPHAS))
@pytest.mark.parametrize("model_type", MODELS)
@pytest.mark.parametrize("store_name", ["config2", "ragged", "tiny"])
def test_statistics_equal_reference(store_name, model_type, alpha_name, monkeypatch):
    store = _store(store_name)
    alpha = ALPHAS[alpha_name]
    model = _model(store, store_name, model_type, alpha)
    ref = AR.stats(store, model, alpha)
    got = {}
    for mode in MODES:
        got[mode] = _stats(store, model, mode, monkeypatch)
        assert got[mode].shape == (store.n_regions, 2, 4, 4)
        _close(got[mode], ref, mode)
        assert np.all(got[mode][:, 1] >= 0.0)
        if model_type == N.HF_MODEL_TRUNC_EXP_GAUSSIAN:
            assert np.all(got[mode][:, :, :, 0] == 0.0)
    # scan and seq agree with each other to the same bar (magnitudes from the reference)
    for mode in ("scan", "scan_two_launches", "scan_sub_passes"):
        _close(got[mode], {"G": got["seq"][:, 0], "H": got["seq"][:, 1], "Gabs": ref["Gabs"]}, mode + " vs seq")
    # two runs return the same bits
    assert np.array_equal(_stats(store, model, "scan", monkeypatch), got["scan"])
    assert np.array_equal(_stats(store, model, "seq", monkeypatch), got["seq"])


def test_one_window_chunks_contribute_nothing():
    store = _tiny_store(np.random.default_rng(3), [1, 1, 1], [20], avg_len=6000)
    model = perturbed_model(store, N.HF_MODEL_GAUSSIAN, 2, DISTINCT, np.random.default_rng(4))
    for algo in (N.HF_ALGO_SCAN, N.HF_ALGO_SEQ):
        em = hmm.EMList(store, model, algo=algo)
        em.set_alpha_stats(True)
        hmm.EM_runOneIterationForList(em, model)
        assert np.all(em.alpha_stats() == 0.0)
        em.close()


def test_per_chunk_statistics_mode():
    """HF_STATS_CHUNKS on the scan path is served by the same per-window kernel."""
    store = _store("ragged")
    model = _model(store, "ragged", N.HF_MODEL_TRUNC_EXP_GAUSSIAN, synth.HIFI_ALPHA)
    ref = AR.stats(store, model, synth.HIFI_ALPHA)
    out = []
    for mode in (N.HF_STATS_CHUNKS, N.HF_STATS_ROWS):
        em = hmm.EMList(store, model)
        em.set_stats_mode(mode)
        em.set_alpha_stats(True)
        hmm.EM_runOneIterationForList(em, model)
        out.append(em.alpha_stats())
        _close(out[-1], ref)
        em.close()
    assert np.array_equal(out[0], out[1])             # the forward-backward of both modes is the same


# ---- 3. the switch changes nothing else ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ])
def test_switch_on_equals_switch_off(algo):
    store = synth.config(2, 0.03)
    em_a, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, synth.HIFI_ALPHA, iters=1, algo=algo)
    em_b = hmm.EMList(store, model, algo=algo)
    em_a.set_alpha_stats(True)
    hmm.EM_runOneIterationForList(em_a, model)
    st_a = model.estimators.copy()
    hmm.EM_runOneIterationForList(em_b, model)
    assert np.array_equal(st_a, model.estimators)
    g = em_a.alpha_stats()
    assert np.abs(g).max() > 0.0
    assert np.array_equal(em_a.labels(), em_b.labels())
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    for x, y in zip(em_a.forward_backward(), em_b.forward_backward()):
        assert np.array_equal(x, y)
    va, vb = em_a.viterbi(model), em_b.viterbi(model)
    assert np.array_equal(va[0], vb[0]) and np.array_equal(va[1], vb[1]) and va[2] == vb[2]
    assert np.array_equal(em_a.sample_paths(model, 3, 99), em_b.sample_paths(model, 3, 99))
    n = store.n_windows
    F = np.array([0, 5, n // 2, n - 40]); L = np.array([n - 1, 900, n // 2 + 3000, n - 1]); M = np.array([15, 4, 6, 11])
    assert np.array_equal(em_a.interval_log_probs(F, L, M), em_b.interval_log_probs(F, L, M))
    assert np.array_equal(em_a.alpha_stats(), g)                    # ... and none of them disturbs the statistics of the pass
    hmm.EM_runOneIterationForList(em_a, model); st2_a = model.estimators.copy()   # the next pass
    hmm.EM_runOneIterationForList(em_b, model); st2_b = model.estimators.copy()
    assert np.array_equal(st2_a, st2_b) and np.array_equal(st2_a, st_a)
    assert np.array_equal(em_a.labels(), em_b.labels())
    assert np.array_equal(em_a.alpha_stats(), g)                    # same model, same pass: same bits
    em_a.close(); em_b.close()


def test_errors():
    """Argument checks that return before any launch."""
    store = synth.config(2, 0.02)
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, store, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model)
    L_ = N.lib()
    assert L_.hf_alpha_stats_len(em._h) == 32 * store.n_regions
    out = np.empty(32 * store.n_regions)
    op = out.ctypes.data_as(C.POINTER(C.c_double))
    assert L_.hf_set_alpha_stats(None, 1) == N.HF_E_ARG
    assert L_.hf_get_alpha_stats(em._h, op) == N.HF_E_ARG                  # no pass yet
    hmm.EM_runOneIterationForList(em, model)
    assert L_.hf_get_alpha_stats(em._h, op) == N.HF_E_ARG                  # a full pass, but the switch was off
    assert b"hf_set_alpha_stats" in L_.hf_last_error()
    em.set_alpha_stats(True)
    assert L_.hf_get_alpha_stats(em._h, op) == N.HF_E_ARG                  # switched on after the pass
    hmm.EM_runForwardForList(em, model)
    assert L_.hf_get_alpha_stats(em._h, op) == N.HF_E_ARG                  # forward-only
    hmm.EM_runOneIterationForList(em, model)
    assert L_.hf_get_alpha_stats(em._h, None) == N.HF_E_ARG
    assert L_.hf_get_alpha_stats(em._h, op) == N.HF_OK
    em.set_alpha_stats(False)
    assert L_.hf_get_alpha_stats(em._h, op) == N.HF_E_ARG                  # switched off again
    with pytest.raises(N.HFError):
        em.alpha_stats()
    em.close()
    # negative_binomial: its emission has no alpha
    nb = hmm.createModel(hmm.MODEL_NEGATIVE_BINOMIAL, 3, store, np.zeros((4, 4)))
    em = hmm.EMList(store, nb)
    em.set_alpha_stats(True)                                               # (hf_create takes no model type)
    hmm.EM_runOneIterationForList(em, nb)
    assert L_.hf_get_alpha_stats(em._h, op) == N.HF_E_ARG
    assert L_.hf_set_alpha_stats(em._h, 1) == N.HF_E_ARG                   # the context is now known to serve negative_binomial
    assert b"negative_binomial" in L_.hf_last_error()
    em.close()


# ---- 4. an alpha-step through the library ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_type", MODELS)
@pytest.mark.parametrize("algo", [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ])
def test_alpha_step_does_not_lower_the_loglikelihood(algo, model_type):
    """hfm_estimate_alpha from the device's statistics, one more pass: the log-likelihood the device reports did not fall (1e-9 |LL|, the
    pass's own bar)."""
    store = AR.simulate(12000, 1500, TRUE, seed=7)
    em, model = _trained(store, model_type, 3, np.zeros((4, 4)), iters=2, algo=algo)
    em.set_alpha_stats(True)
    lls = []
    for _ in range(4):
        hmm.EM_runOneIterationForList(em, model)
        lls.append(model.loglikelihood)
        before = model.alpha
        hmm.HMM_estimateAlpha(model, em.alpha_stats(), 1e-3)
        assert np.all((model.alpha >= 0.0) & (model.alpha <= hmm.FIT_ALPHA_MAX))
        assert np.array_equal(model.alpha[hmm.alpha_free_mask() == 0], before[hmm.alpha_free_mask() == 0])
    hmm.EM_runOneIterationForList(em, model)
    lls.append(model.loglikelihood)
    print("log-likelihoods:", lls)
    d = np.diff(lls)
    assert np.all(d >= -1e-9 * np.abs(lls[0])), lls
    assert lls[-1] - lls[0] > 100.0                   # the track is autocorrelated: alpha = 0 is far from the maximum
    em.close()


def test_run_hmm_flagger_fit_alpha(tmp_path):
    store = AR.simulate(12000, 1500, TRUE, seed=7)
    K = hmm.getBestNumberOfCollapsedComps(store)
    res = {}
    for fit in (False, True):
        model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, np.zeros((4, 4)))
        em = hmm.EMList(store, model)
        out = tmp_path / ("fit" if fit else "plain")
        out.mkdir()
        res[fit] = hmm.runHMMFlagger(em, model, 10, 1e-3, str(out), fitAlpha=fit)
        if fit:
            assert np.array_equal(hmm.getAlphaMatrix(str(out / "alpha_fitted.tsv")), model.alpha)
            assert model.alpha.max() > 0.1
        em.close()
    assert res[True][-1] >= res[False][-1]


# ---- 5. command line -------------------------------------------------------------------------------------------------------------
def _cli(args, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


def _rows(path):
    return [l.split("\t") for l in path.read_text().splitlines() if not l.startswith("#")]


def test_cli_fit_alpha(tmp_path):
    """A track simulated from the model with the alpha matrix TRUE (autocorrelated).  The reference's own alternating fit on this input,
    run on the CPU (oracle E-step and M-step, alpha_ref alpha-steps, 10 iterations, P = 2): final log-likelihood -35266.4 against
    -37339.2 of the run without the fit."""
    store = AR.simulate(12000, 1500, TRUE, seed=7)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    args = ["-i", str(binp), "-W", "4000", "-n", "10"]
    _cli(args, tmp_path / "plain")
    _cli(args + ["--fitAlpha"], tmp_path / "fit")
    a, b = tmp_path / "plain", tmp_path / "fit"
    assert sorted(set(os.listdir(b)) - set(os.listdir(a))) == ["alpha_fitted.tsv", "alpha_trace.tsv"]
    ll_plain = [float(r[2]) for r in _rows(a / "loglikelihood.tsv")]
    ll_rows = _rows(b / "loglikelihood.tsv")
    ll_fit = [float(r[2]) for r in ll_rows]
    assert all(len(r) == 3 for r in ll_rows)
    assert ll_fit[-1] >= ll_plain[-1]
    assert ll_fit[-1] - ll_plain[-1] > 100.0
    # one trace row per alpha-iteration: iterations 2, 4, ... of the loop (rows 1, 3, ... of loglikelihood.tsv)
    trace = _rows(b / "alpha_trace.tsv")
    n_iter = len(ll_rows) - 1
    assert [int(r[0]) for r in trace] == list(range(1, n_iter, 2))
    assert all(len(r) == 2 + 48 for r in trace)
    for r in trace:
        assert float(r[1]) == pytest.approx(ll_fit[int(r[0])], abs=1e-4)
        assert all(float(x) >= 0.0 for x in r[34:])                 # H
    assert all(float(x) == 0.0 for x in trace[0][2:18])               # the fit starts from 0 without --alphaTsv
    # alpha_fitted.tsv round-trips through --alphaTsv: the same doubles, and a run from it starts where the fit ended
    fitted = hmm.getAlphaMatrix(str(b / "alpha_fitted.tsv"))
    text = (b / "alpha_fitted.tsv").read_text().splitlines()
    assert len(text) == 4 and all(len(l.split("\t")) == 4 for l in text)
    assert np.array_equal(fitted, np.array([[float(x) for x in l.split("\t")] for l in text]))
    free = hmm.alpha_free_mask() == 1
    assert np.all(fitted[~free] == 0.0) and np.all((fitted >= 0.0) & (fitted <= 0.8)) and fitted.max() > 0.1
    _cli(args + ["--alphaTsv", str(b / "alpha_fitted.tsv"), "--fitAlpha", "--fitAlphaEntries", "2,2", "--fitAlphaEvery", "1", "-n", "2"],
         tmp_path / "again")
    again = _rows(tmp_path / "again" / "alpha_trace.tsv")
    assert [int(r[0]) for r in again] == [0, 1]
    assert np.array_equal(np.array([float(x) for x in again[0][2:18]]).reshape(4, 4), fitted)
    refit = hmm.getAlphaMatrix(str(tmp_path / "again" / "alpha_fitted.tsv"))
    mask22 = np.zeros((4, 4), bool); mask22[2, 2] = True
    assert np.array_equal(refit[~mask22], fitted[~mask22])
    # without the flag: the files of a run made before the options existed (the oracle byte-compares of test_cli_gpu.py cover the bytes)
    _cli(args, tmp_path / "plain2")
    for n in os.listdir(a):
        assert (a / n).read_bytes() == (tmp_path / "plain2" / n).read_bytes(), n
