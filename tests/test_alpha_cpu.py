"""CPU checks of the alpha fit's ground: the numpy reference of the alpha statistics (tests/alpha_ref.py) against a central difference of
its own log-likelihood, the host model's conditional maximisation (hfm_estimate_alpha) against a few lines of numpy, monotonicity and
recovery of the alpha-step in the reference, and the command line's --fitAlpha options (checks made before the input is read)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm
from test_bruteforce_cpu import _tiny_store
from test_cli_prefix_cpu import ADDED, CLI, REFERENCE, unique_prefixes
from test_viterbi_cpu import perturbed_model
import alpha_ref as AR
import viterbi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fitAlpha": 0, "fitAlphaEntries": 1, "fitAlphaMax": 1, "fitAlphaEvery": 1}
BUILD = {**REFERENCE, **{n: 1 for n in ADDED}, "viterbi": 0, "sweepAlpha": 1, "uncertaintySamples": 1, "uncertaintySeed": 1,
         "runConfidence": 0, "regionProbs": 1}
DISTINCT = np.array([[0.31, 0.12, 0.45, 0.07], [0.22, 0.41, 0.18, 0.33], [0.05, 0.27, 0.52, 0.14], [0.38, 0.09, 0.24, 0.61]])
TRUE = np.array([[0.75, 0, 0.24, 0], [0, 0.46, 0.44, 0], [0.5, 0.16, 0.40, 0.22], [0, 0, 0.04, 0.21]])


def gradient_fixture(model_type):
    """Two regions, chunks of 60, 2, 1, 45 and 7 windows on contigs a few reads long (13 distinct beta values), 16 distinct alphas."""
    rng = np.random.default_rng(2024)
    store = _tiny_store(rng, [60, 2, 1, 45, 7], [20, 31], avg_len=6000)
    model = perturbed_model(store, model_type, 3, DISTINCT, rng)
    return store, model


# ---- 1. the gradient ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_type", [N.HF_MODEL_TRUNC_EXP_GAUSSIAN, N.HF_MODEL_GAUSSIAN])
def test_gradient_equals_central_difference(model_type):
    """G summed over the regions against (LL(a + h) - LL(a - h)) / 2h of the reference's own sum of log scale, all 16 entries, h = 1e-5.
    Measured on this fixture: 2.95e-9 (trunc_exp_gaussian) and 4.34e-9 (gaussian) of the largest |G|, the truncation term of the
    central difference (it falls 100x from h = 1e-4 to 1e-5; at h = 1e-6 rounding takes over at 1e-9).  Bound: 100x the larger
    measurement, 4.4e-7 of the largest |G| (the issue allows 1e-6 at most).
    Without the pair (0, 1) of every chunk the same check misses by 67 % / 79 % of the largest |G|: asserted to miss by more than
    1000x the bound, so the reference cannot drop that pair silently."""
    store, model = gradient_fixture(model_type)
    assert len(np.unique(viterbi_ref.betas(store))) > 4 and sorted(np.diff(store.chunk_off))[:2] == [1, 2]
    st = AR.stats(store, model, DISTINCT)
    G = st["G"].sum(axis=0)
    h = 1e-5
    D = np.zeros((4, 4))
    for p in range(4):
        for s in range(4):
            up, dn = DISTINCT.copy(), DISTINCT.copy()
            up[p, s] += h
            dn[p, s] -= h
            D[p, s] = (AR.loglik(store, model, up) - AR.loglik(store, model, dn)) / (2 * h)
    scale = np.abs(G).max()
    err = np.abs(D - G).max() / scale
    print("gradient error / max|G| =", err)
    bound = 4.4e-7
    assert bound <= 1e-6
    assert err <= bound, err
    if model_type == N.HF_MODEL_TRUNC_EXP_GAUSSIAN:
        assert np.all(G[:, 0] == 0.0) and np.all(st["H"][:, :, 0] == 0.0)
    assert np.all(st["H"] >= 0.0)
    skipped = AR.stats(store, model, DISTINCT, skip_first_pair=True)["G"].sum(axis=0)
    err_skipped = np.abs(D - skipped).max() / scale
    print("without the pair (0, 1):", err_skipped)
    assert err_skipped > 1000 * bound, err_skipped


def test_one_and_two_window_chunks():
    """A chunk of one window contributes nothing, a chunk of two windows its one pair (which the transition counts skip)."""
    rng = np.random.default_rng(5)
    store = _tiny_store(rng, [1, 2, 1], [20], avg_len=6000)
    model = perturbed_model(store, N.HF_MODEL_GAUSSIAN, 2, DISTINCT, rng)
    st = AR.stats(store, model, DISTINCT)
    assert np.all(st["count"] == 0.0) and np.abs(st["G"]).max() > 0.0
    one = _tiny_store(rng, [1, 1], [20], avg_len=6000)
    st1 = AR.stats(one, perturbed_model(one, N.HF_MODEL_GAUSSIAN, 2, DISTINCT, rng), DISTINCT)
    assert np.all(st1["G"] == 0.0) and np.all(st1["H"] == 0.0)


# ---- 2. the host model ----------------------------------------------------------------------------------------------------------
def _estimate(model, G, H, count, mask, lo, hi, tol):
    R, K = model.numberOfRegions, model.maxNumberOfComps
    stats = np.zeros(N.stats_len(R, K))
    stride = N.region_stride(K)
    a = np.zeros((R, 2, 4, 4))
    for r in range(R):
        a[r, 0], a[r, 1] = G[r], H[r]
        stats[1 + r * stride + 24 * K:1 + r * stride + 24 * K + 16] = count[r].ravel()
    model.estimators = stats
    return a


def test_estimate_alpha_equals_numpy():
    rng = np.random.default_rng(11)
    store = _tiny_store(rng, [7, 5], [20, 31])
    model = hmm.createModel(N.HF_MODEL_GAUSSIAN, 2, store, DISTINCT)
    assert np.array_equal(model.alpha, DISTINCT)
    G = rng.normal(0, 30, size=(2, 4, 4))
    H = rng.uniform(50, 500, size=(2, 4, 4))
    count = rng.uniform(20, 100, size=(2, 4, 4))
    mask = np.ones((4, 4), int)
    mask[1, 2] = mask[3, 0] = 0                     # not free
    count[:, 0, 1] = [4.0, 6.0]                     # the gate at exactly 10: 10 < count is false
    count[:, 0, 2] = [4.0, 6.0 + 2e-15]             # ... and just above
    H[:, 2, 2] = 0.0                                # H = 0
    G[:, 3, 3], H[:, 3, 3] = [400.0, 500.0], [1.0, 1.0]       # clamp at hi
    G[:, 2, 0], H[:, 2, 0] = [-400.0, -500.0], [1.0, 1.0]     # clamp at lo
    lo, hi = 0.02, 0.8
    entries = [(p, s) for p in range(4) for s in range(4) if mask[p, s]]
    a = _estimate(model, G, H, count, mask, lo, hi, 1e-3)
    conv = hmm.HMM_estimateAlpha(model, a, 1e-3, entries, lo, hi)
    Gs, Hs, Cs = G[0] + G[1], H[0] + H[1], count[0] + count[1]
    want = DISTINCT.copy()
    for p, s in entries:
        if Hs[p, s] > 0 and 10 < Cs[p, s]:
            want[p, s] = min(max(DISTINCT[p, s] + Gs[p, s] / Hs[p, s], lo), hi)
    got = model.alpha
    assert np.array_equal(got, want)
    assert got[1, 2] == DISTINCT[1, 2] and got[3, 0] == DISTINCT[3, 0]
    assert got[0, 1] == DISTINCT[0, 1] and got[0, 2] != DISTINCT[0, 2]
    assert got[2, 2] == DISTINCT[2, 2] and got[3, 3] == hi and got[2, 0] == lo
    assert conv is False
    # the convergence flag: a second step from the same statistics moves the clamped entries by 0 and the others by G / H again
    small = _estimate(model, G * 1e-6, np.where(H > 0, H, 0.0), count, mask, lo, hi, 1e-3)
    before = model.alpha
    assert hmm.HMM_estimateAlpha(model, small, 1e-3, entries, lo, hi) is True
    assert np.abs(model.alpha - before).max() < 1e-3
    assert hmm.HMM_estimateAlpha(model, small, 1e-9, entries, lo, hi) is False
    # bad bounds, a negative_binomial model
    with pytest.raises(ValueError):
        hmm.HMM_estimateAlpha(model, small, 1e-3, entries, 0.0, 1.0)
    with pytest.raises(ValueError):
        hmm.HMM_estimateAlpha(model, small, 1e-3, entries, -0.1, 0.5)
    nb = hmm.createModel(N.HF_MODEL_NEGATIVE_BINOMIAL, 2, store, np.zeros((4, 4)))
    nb.estimators = model.estimators
    with pytest.raises(ValueError):
        hmm.HMM_estimateAlpha(nb, small, 1e-3)


def test_set_alpha_refuses_values_outside_the_unit_interval():
    rng = np.random.default_rng(12)
    store = _tiny_store(rng, [7], [20])
    model = hmm.createModel(N.HF_MODEL_GAUSSIAN, 2, store, np.zeros((4, 4)))
    model.set_alpha(DISTINCT)
    assert np.array_equal(model.alpha, DISTINCT)
    assert np.array_equal(np.ctypeslib.as_array(model.params().alpha).reshape(4, 4), DISTINCT)
    for bad in (1.0, -0.1, np.nan):
        a = DISTINCT.copy()
        a[2, 1] = bad
        with pytest.raises(ValueError):
            model.set_alpha(a)
        assert np.array_equal(model.alpha, DISTINCT)
    a = DISTINCT.copy()
    a[0, 0] = np.nextafter(1.0, 0.0)
    model.set_alpha(a)


def test_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "hmm_flagger_hip.h")).read()
    for decl in (r"int\s+hf_set_alpha_stats\s*\(\s*hf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)", r"int64_t\s+hf_alpha_stats_len\s*\(\s*const\s+hf_ctx",
                 r"int\s+hf_get_alpha_stats\s*\(\s*hf_ctx\s*\*\s*ctx\s*,\s*double\s*\*\s*out_host\s*\)"):
        assert re.search(decl, text), decl
    text = open(os.path.join(ROOT, "include", "hmm_flagger_model.h")).read()
    for name in ("hfm_get_alpha", "hfm_set_alpha", "hfm_estimate_alpha"):
        assert name in text and hasattr(N.lib(), name)
    for name in ("hf_set_alpha_stats", "hf_alpha_stats_len", "hf_get_alpha_stats"):
        assert getattr(N.lib(), name).argtypes is not None
    assert hasattr(hmm.EMList, "set_alpha_stats") and hasattr(hmm.EMList, "alpha_stats") and hasattr(hmm, "HMM_estimateAlpha")
    assert list(zip(*np.nonzero(hmm.alpha_free_mask()))) == list(hmm.FIT_ALPHA_ENTRIES)


# ---- 3., 4. the alpha-step in the reference -----------------------------------------------------------------------------------
def test_alpha_steps_never_lower_the_loglikelihood():
    """Other parameters fixed, repeated conditional maximisations: exact in theory because the pair (0, 1) is in; 1e-12 |LL| for rounding."""
    for model_type, seed in ((N.HF_MODEL_GAUSSIAN, 3), (N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4)):
        store = AR.simulate(6000, 700, TRUE, seed=seed)
        model = AR.true_model(store, model_type)
        a = np.zeros((4, 4))
        lls = []
        for _ in range(6):
            st = AR.stats(store, model, a)
            lls.append(st["ll"])
            a, _ = AR.alpha_step(a, st, hmm.alpha_free_mask())
        lls.append(AR.loglik(store, model, a))
        d = np.diff(lls)
        assert np.all(d >= -1e-12 * np.abs(lls[0])), d
        assert lls[-1] - lls[0] > 100.0


def test_alpha_steps_recover_the_diagonal():
    """20 000 windows simulated from the model definition with a known alpha; from alpha = 0, with the other parameters at their true
    values, the alpha-steps move each diagonal entry strictly closer to the truth than 0 was, and the 10 < count gate passes on all four."""
    store = AR.simulate(20000, 2500, TRUE, seed=3)
    model = AR.true_model(store)
    for mask in (np.eye(4, dtype=int), hmm.alpha_free_mask()):
        a = np.zeros((4, 4))
        for _ in range(5):
            st = AR.stats(store, model, a)
            assert np.all(np.diag(st["count"][0]) > 10)
            a, _ = AR.alpha_step(a, st, mask)
        assert np.all(np.abs(np.diag(a) - np.diag(TRUE)) < np.abs(np.diag(TRUE))), np.diag(a)
        assert np.all(np.abs(np.diag(a) - np.diag(TRUE)) < 0.05), np.diag(a)
        assert np.all(a[mask == 0] == 0.0)


# ---- 5. command line -------------------------------------------------------------------------------------------------------------
def test_new_options_move_no_unique_prefix():
    for before in (list(REFERENCE), list(BUILD)):
        now = dict(unique_prefixes(list(BUILD) + list(NEW)))
        lost = [(p, n) for p, n in unique_prefixes(before) if now.get(p) != n]
        assert not lost, lost
    r = subprocess.run([CLI, "--alpha", "1"], capture_output=True, text=True)
    assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr


def test_help_names_the_options():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    for n in NEW:
        assert "--" + n in r.stderr + r.stdout


def _run(tmp_path, extra):
    args = [CLI, "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path)] + extra
    r = subprocess.run(args, capture_output=True, text=True, env={**os.environ, "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"})
    return r, [l for l in r.stderr.splitlines() if l.strip()]


@pytest.mark.parametrize("extra,word", [(["--accelerate"], "--accelerate"), (["--gpus", "2"], "--gpus"), (["--sweepAlpha", "list.txt"], "--sweepAlpha"),
                                        (["--modelType", "negative_binomial"], "negative_binomial")])
def test_refused_combinations(tmp_path, extra, word):
    """Refused before the input is read and before any device use: the input named here does not exist and no device is visible, so only
    the refusal can be the error."""
    r, lines = _run(tmp_path, ["--fitAlpha"] + extra)
    assert r.returncode != 0
    assert len(lines) == 1 and "--fitAlpha" in lines[0] and word in lines[0], r.stderr[-500:]


@pytest.mark.parametrize("bad", ["", "0", "0,0:", "0,4", "4,0", "0;0", "0,0,1,1", "a,b", "0,0:1", ":0,0", "0,0::1,1", "-1,0"])
def test_malformed_entry_lists_are_rejected(tmp_path, bad):
    r, lines = _run(tmp_path, ["--fitAlpha", "--fitAlphaEntries", bad])
    assert r.returncode != 0
    assert len(lines) == 1 and "--fitAlphaEntries" in lines[0], r.stderr[-500:]


@pytest.mark.parametrize("extra,word", [(["--fitAlpha", "--fitAlphaMax", "1.0"], "--fitAlphaMax"), (["--fitAlpha", "--fitAlphaMax", "-0.1"], "--fitAlphaMax"),
                                        (["--fitAlpha", "--fitAlphaEvery", "0"], "--fitAlphaEvery"), (["--fitAlphaEvery", "3"], "need --fitAlpha"),
                                        (["--fitAlphaEntries", "0,0"], "need --fitAlpha")])
def test_bad_values_are_rejected(tmp_path, extra, word):
    r, lines = _run(tmp_path, extra)
    assert r.returncode != 0
    assert len(lines) == 1 and word in lines[0], r.stderr[-500:]


def test_good_options_pass_to_the_input_check(tmp_path):
    r, lines = _run(tmp_path, ["--fitAlpha", "--fitAlphaEntries", "0,0:2,2:3,3", "--fitAlphaMax", "0.5", "--fitAlphaEvery", "3"])
    assert r.returncode != 0
    assert "--fitAlpha" not in r.stderr, r.stderr[-500:]
