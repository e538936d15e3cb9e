"""The E-step under minimum run lengths on the GPU (hf_estep_minlen, hf_em_iterate_minlen, EMList.estep_minlen /
minlen_pair_posterior / em_iterate_minlen, hmm_flagger --lengthConstrainedEM) against the float64 numpy reference
(tests/minlen_em_ref.py), which tests/test_minlen_em_cpu.py pins to path enumeration and to the oracle's estimators.

Tolerances, the project's: xi_adm within 1e-10 + 1e-9 |ref| wherever ref >= 1e-250, elsewhere 0 <= got <= 1e-249 (close_post's
rule); every statistics element within 1e-9 of the summed magnitude of its terms (the alpha statistics' rule); log Z_adm and log Z
within 1e-9 relative.  The marginal identities against hf_get_minlen_posterior: 1e-12 absolute: both sides are ratios of sums of at
most 64 non-negative terms formed from the same F and B bits, so each carries at most ~70 roundings of 1.1e-16 relative to a value
<= 1, and a sum of four of them stays below 1e-13.  Every test prints its largest deviations before it asserts (pytest -s)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from hip_streams import Streams
from test_bruteforce_cpu import _tiny_store
from test_viterbi_cpu import perturbed_model
import alpha_ref
import floor_cases
import geometry_cases as G
import minlen_em_ref as E
import minlen_post_ref as MP
import sampling_ref
import test_minlen_gpu as TML

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]
ONES = (1, 1, 1, 1)
TRACK_LEN = (3, 5, 1, 7)
# no pair, or one; one rescaling period; the 64-window block of the backward walk and of F
LENGTHS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 129]
MIN_LENS = [ONES, (2, 1, 1, 3), TRACK_LEN, (30, 16, 1, 17), (1, 1, 12, 1)]     # the lane cap met exactly; a length above the chunks of <= 9
TEG, GAU = N.HF_MODEL_TRUNC_EXP_GAUSSIAN, N.HF_MODEL_GAUSSIAN
# (model type, region coverages, components of the collapsed state, HiFi alpha)
MODELS = {"teg-2regions-K3": (TEG, (20, 31), 3, True), "gaussian-1region-K2": (GAU, (25,), 2, False),
          "teg-2regions-K16": (TEG, (20, 31), N.HF_MAXCOMP, True)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(store, model, alpha): chunks of LENGTHS windows, a region per window at random (region changes inside the chunks)."""
    mt, regions, K, hifi = MODELS[name]
    rng = np.random.default_rng(7700 + len(name))
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    store = _tiny_store(rng, LENGTHS, list(regions))
    model = perturbed_model(store, mt, K, alpha, rng)
    return store, model, alpha


@functools.lru_cache(maxsize=None)
def _ref(name, min_len):
    store, model, alpha = _case(name)
    return E.stats(store, model, alpha, min_len)


def _run(em, model, min_len):
    """(stats, log_z, xi, chunk vectors, log Z_adm per chunk, log Z per chunk) of one call."""
    st, lz = em.estep_minlen(model, min_len)
    cs, lza, lzc = em.minlen_em_chunk_stats()
    return st, lz, em.minlen_pair_posterior(), cs, lza, lzc


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _covered(store):
    return slice(int(store.chunk_off[0]), int(store.chunk_off[-1]))


def _check(store, ref, got, what):
    st, lz, xi, cs, lza, lzc = got
    w = _covered(store)
    rxi = ref["xi"]
    big = rxi >= 1e-250
    dev = np.abs(xi[w][big] - rxi[big]) / rxi[big]
    print("%s: xi_adm largest relative deviation %.3e over %d entries, %d below the floor" % (what, float(dev.max()) if dev.size else 0.0,
                                                                                           int(big.sum()), int((~big).sum())))
    MP.close_post(xi[w], rxi, rel=1e-9, extra_abs=1e-10)
    for g, r, nm in ((lza, ref["lza"], "log Z_adm"), (lzc, ref["lz"], "log Z")):
        err = np.abs(g - r)
        print("%s: %s largest relative deviation %.3e" % (what, nm, float(np.max(err / np.maximum(np.abs(r), 1e-300))) if r.size else 0.0))
        assert np.all(err <= 1e-9 * np.abs(r)), nm
    assert abs(lz - ref["lz"].sum()) <= 1e-9 * abs(ref["lz"].sum())
    E.close_stats(st, ref["vec"], ref["mag"], what + " statistics")
    assert np.array_equal(cs[:, 0], lza)                    # element 0 of every chunk vector: its log Z_adm


# ---- chunk lengths, length sets, models, both kinds of context ----------------------------------------------------------------------

@pytest.mark.parametrize("min_len", MIN_LENS)
@pytest.mark.parametrize("name", list(MODELS))
def test_lengths_models_and_both_algorithms(name, min_len):
    store, model, alpha = _case(name)
    ref = _ref(name, min_len)
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        res.append(_run(em, model, min_len))
        if algo == ALGOS[0]:
            r = em.minlen_posterior(model, min_len)          # the identities, and element 0 bit for bit
            post = r.posterior()
            assert np.array_equal(res[0][4], r.chunk_log_z_adm)
            off = np.asarray(store.chunk_off)
            first = np.zeros(store.n_windows, bool)
            first[off[:-1]] = True
            t = np.flatnonzero(~first)
            xi = res[0][2]
            d1, d2 = np.abs(xi[t].sum(axis=1) - post[t]), np.abs(xi[t].sum(axis=2) - post[t - 1])
            print("identities: %.3e, %.3e (bound 1e-12)" % (float(d1.max()), float(d2.max())))
            assert np.all(d1 <= 1e-12) and np.all(d2 <= 1e-12)
            assert np.all(xi[first] == 0.0)
            assert _same(res[0], _run(em, model, min_len))  # a second call: identical bits
        em.close()
    _check(store, ref, res[0], "%s %s" % (name, min_len))
    assert _same(res[0], res[1])                            # SCAN == SEQ
    T = np.diff(store.chunk_off)
    cs = res[0][3]
    assert not cs[T <= 2, 1:].any()                         # no pair (w-1, w) with w >= 2: exactly zero behind element 0
    assert all(cs[c, 1:].any() for c in np.flatnonzero(T >= 3))
    if min_len != ONES:
        assert not np.allclose(ref["xi"], _ref(name, ONES)["xi"], rtol=0, atol=1e-6)     # the rule says something here


@pytest.mark.parametrize("name", list(MODELS))
def test_all_ones_is_the_plain_estep(name):
    """With all four lengths 1: the statistics of hf_estep + hf_finish behind element 0, xi from hf_get_forward_backward."""
    store, model, alpha = _case(name)
    ref = _ref(name, ONES)
    em = hmm.EMList(store, model)
    st, lz, xi, cs, lza, lzc = _run(em, model, ONES)
    assert np.array_equal(lza, lzc)
    hmm.EM_runOneIterationForList(em, model)
    plain = model.estimators.copy()
    hmm.HMM_resetEstimators(model)
    E.close_stats(st[1:], plain[1:], ref["mag"][1:], name + " against hf_estep + hf_finish")
    f, b, sc = em.forward_backward()
    A, end = sampling_ref.rows(store, model, alpha)
    off = np.asarray(store.chunk_off)
    local = np.arange(store.n_windows) - np.repeat(off[:-1], np.diff(off))
    t = np.flatnonzero(local >= 1)
    want = np.zeros_like(xi)
    want[t] = f[t - 1][:, :, None] * A[t] * b[t][:, None, :] / alpha_ref.TERMINATION
    MP.close_post(xi, want, rel=1e-9, extra_abs=1e-10)
    # element 0 is log Z: the pass's log-likelihood plus the end column it leaves out
    live = np.diff(off) > 0
    ends = float(np.sum(np.log(np.sum(f[off[1:][live] - 1] * end[live], axis=1))))
    assert abs(st[0] - (plain[0] + ends)) <= 1e-9 * abs(st[0])
    em.close()


# ---- chunks without windows, windows outside every chunk ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _grid_ref():
    model_type, seed = G.CASES[0]
    store, model, alpha, _ = G.case(model_type, seed)
    return E.stats(store, model, alpha, TRACK_LEN)


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunks_and_uncovered_windows(algo):
    model_type, seed = G.CASES[0]
    store, model, alpha, _ = G.case(model_type, seed)
    em0 = hmm.EMList(store, model, algo=algo)
    base = _run(em0, model, TRACK_LEN)
    _check(store, _grid_ref(), base, "grid store")
    em0.close()
    est, src = G.with_empty_chunks(store)
    em = hmm.EMList(est, model, algo=algo)
    st, lz, xi, cs, lza, lzc = _run(em, model, TRACK_LEN)
    assert np.array_equal(xi, base[2]) and np.array_equal(cs[src >= 0], base[3])
    assert not cs[src < 0].any() and not lza[src < 0].any() and not lzc[src < 0].any()
    E.close_stats(st, base[0], _grid_ref()["mag"], "with chunks without windows", rel=1e-13)   # (k_reduce's lanes hold other chunks)
    em.close()
    ust = G.with_uncovered_windows(store, np.random.default_rng(5))
    a, n = G.FRONT, ust.n_windows
    b = a + store.n_windows
    em = hmm.EMList(ust, model, algo=algo)
    st, lz = em.estep_minlen(model, TRACK_LEN)
    cs, lza, lzc = em.minlen_em_chunk_stats()
    assert np.array_equal(st, base[0]) and lz == base[1] and np.array_equal(cs, base[3])
    assert np.array_equal(em.minlen_pair_posterior(a, store.n_windows), base[2])
    for f, cnt in [(0, 1), (a - 1, 1), (a - 1, 4), (0, n), (a, store.n_windows + 1), (b, 1), (n - 1, 1)]:
        with pytest.raises(N.HFError) as ei:
            em.minlen_pair_posterior(f, cnt)
        assert ei.value.code == N.HF_E_ARG, (f, cnt)
    assert em.minlen_pair_posterior(a, 0).shape == (0, 4, 4)
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunk_list(algo):
    full = synth.synthesize([50_000], 1000, 20_000, [20], seed=2)
    store = full.subset_chunks([])
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, full, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model, algo=algo)
    st, lz = em.estep_minlen(model, TRACK_LEN)
    assert not st.any() and lz == 0.0 and em.minlen_pair_posterior().shape == (0, 4, 4)
    em.close()


# ---- stretches at the emission floor ---------------------------------------------------------------------------------------------------

def test_floored_stretches():
    """floor_cases' short store: stretches of rows at the 1e-40 emission floor across a rescaling period and at the chunks' ends."""
    store, model, alpha = floor_cases.fixture("short")
    ref = E.stats(store, model, alpha, TRACK_LEN)
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        res.append(_run(em, model, TRACK_LEN))
        em.close()
    _check(store, ref, res[0], "floored")
    assert _same(res[0], res[1])


# ---- three EM iterations ---------------------------------------------------------------------------------------------------------------

EM_SEED = 3        # chosen on the CPU: no estimator count of the three reference iterations within 1e-6 of the 10 < count gate


def _em_case():
    rng = np.random.default_rng(8800 + EM_SEED)
    store = _tiny_store(rng, [200, 129, 65, 300], [20, 31])
    model = perturbed_model(store, TEG, 3, synth.HIFI_ALPHA, rng)
    return store, model


def test_three_em_iterations():
    store, model = _em_case()
    alpha = synth.HIFI_ALPHA
    em = hmm.EMList(store, model)
    before = None
    for it in range(3):
        at = model.copy()                                   # the parameters this iteration's E-step runs with
        ref = E.stats(store, at, alpha, TRACK_LEN)
        assert np.all(np.abs(ref["vec"][1:] - 10.0) > 1e-6)
        em.em_iterate_minlen(model, TRACK_LEN, True, 1e-3)
        E.close_stats(model.estimators, ref["vec"], ref["mag"], "iteration %d" % it)
        assert model.loglikelihood == model.estimators[0]
        assert abs(em.last_log_z - ref["lz"].sum()) <= 1e-9 * abs(ref["lz"].sum())
        assert not np.array_equal(model.param_vector(), at.param_vector())
        if before is not None:
            print("objective %.6f -> %.6f" % (before, model.loglikelihood))
        before = model.loglikelihood
        hmm.HMM_resetEstimators(model)
    em.close()


# ---- arguments and errors ----------------------------------------------------------------------------------------------------------------

def test_arguments_getters_and_errors():
    store, model, alpha = _case("teg-2regions-K3")
    em = hmm.EMList(store, model)
    L = N.lib()
    pd = C.POINTER(C.c_double)
    xi = np.empty((store.n_windows, 16))
    st = np.empty(em.stats_len)
    one = (C.c_int32 * 4)(1, 1, 1, 1)

    def getters_refuse():
        assert L.hf_get_minlen_pair_posterior(em._h, 0, store.n_windows, xi.ctypes.data_as(pd)) == N.HF_E_ARG
        assert L.hf_get_minlen_em_chunk_stats(em._h, None, None, None) == N.HF_E_ARG

    getters_refuse()                                       # before any call
    assert L.hf_estep_minlen_finish(em._h, st.ctypes.data_as(pd), None, None) == N.HF_E_ARG
    p = model.params()
    assert L.hf_estep_minlen(em._h, C.byref(p), None, None) == N.HF_E_ARG
    assert L.hf_estep_minlen(em._h, None, one, None) == N.HF_E_ARG
    assert L.hf_estep_minlen(None, C.byref(p), one, None) == N.HF_E_ARG
    assert L.hf_em_iterate_minlen(em._h, None, one, 1, 1e-3, st.ctypes.data_as(pd), None, None, None) == N.HF_E_ARG
    for bad_len in ((3, 0, 1, 1), (-1, 1, 1, 1), (62, 1, 1, 1)):
        with pytest.raises(N.HFError) as ei:
            em.estep_minlen(model, bad_len)
        assert ei.value.code == N.HF_E_ARG, bad_len
    getters_refuse()
    with pytest.raises(TypeError):
        hmm.EM_runOneMinLengthIterationForList(object(), model, ONES)
    good = _run(em, model, (30, 16, 1, 17))
    assert L.hf_estep_minlen(em._h, C.byref(p), one, None) == N.HF_OK
    assert L.hf_estep_minlen_finish(em._h, None, None, None) == N.HF_E_ARG           # NULL statistics
    assert L.hf_estep_minlen_finish(em._h, st.ctypes.data_as(pd), None, None) == N.HF_OK   # log_z may be NULL
    assert L.hf_get_minlen_pair_posterior(em._h, 0, store.n_windows, None) == N.HF_E_ARG
    assert L.hf_get_minlen_pair_posterior(em._h, -1, 2, xi.ctypes.data_as(pd)) == N.HF_E_ARG
    assert L.hf_get_minlen_pair_posterior(em._h, 1, store.n_windows, xi.ctypes.data_as(pd)) == N.HF_E_ARG
    R_ = model.numberOfRegions
    nan = model.copy()
    v = nan.param_vector().reshape(R_, -1)
    v[:, 27 + 3 * 16] = np.nan                             # mean of Col, component 0
    nan.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.estep_minlen(nan, TRACK_LEN)
    assert ei.value.code == N.HF_E_NAN
    getters_refuse()                                       # a failed call is no finished call
    bad = model.copy()
    v = bad.param_vector().reshape(R_, -1)
    v[:, 20:24] = 0.0                                      # start row: no path has weight
    bad.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.estep_minlen(bad, TRACK_LEN)
    assert ei.value.code == N.HF_E_SCALE
    assert _same(good, _run(em, model, (30, 16, 1, 17)))   # and the context answers correctly afterwards
    em.close()


def test_negative_binomial_is_refused():
    store = synth.config(2, 0.02)
    model = hmm.createModel(hmm.MODEL_NEGATIVE_BINOMIAL, 3, store, np.zeros((4, 4)))
    em = hmm.EMList(store, model)
    with pytest.raises(N.HFError) as ei:
        em.estep_minlen(model, TRACK_LEN)
    assert ei.value.code == N.HF_E_ARG and "negative_binomial" in str(ei.value)
    em.close()


# ---- no disturbance ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
def test_no_disturbance_of_the_last_pass_and_the_decoders(algo):
    store = synth.config(2, 0.05)
    alpha = synth.HIFI_ALPHA
    model = hmm.createModel(TEG, 4, store, alpha)
    em_a = hmm.EMList(store, model, algo=algo)
    em_b = hmm.EMList(store, model, algo=algo)
    for em in (em_a, em_b):
        hmm.EM_runOneIterationForList(em, model)
    hmm.HMM_estimateParameters(model, 1e-3)
    hmm.HMM_resetEstimators(model)
    hmm.EM_runOneIterationForList(em_a, model); st_a = model.estimators.copy(); hmm.HMM_resetEstimators(model)
    hmm.EM_runOneIterationForList(em_b, model); st_b = model.estimators.copy(); hmm.HMM_resetEstimators(model)
    assert np.array_equal(st_a, st_b)
    mlv = em_a.viterbi_minlen(model, TRACK_LEN)
    r = em_a.minlen_posterior(model, TRACK_LEN)
    mpost = r.posterior()
    other = model.copy()                                   # the feature runs with DIFFERENT parameters
    v = other.param_vector().reshape(other.numberOfRegions, -1)
    v[:, 27:27 + 4 * 16] *= 1.1
    other.set_param_vector(v.ravel())
    r1 = _run(em_a, other, TRACK_LEN)
    r2 = _run(em_a, other, (2, 2, 2, 2))
    assert not np.array_equal(r1[0], r2[0]) and not np.array_equal(r1[0][1:], st_a[1:])
    assert np.array_equal(em_a.labels(), em_b.labels())
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    for x, y in zip(em_a.forward_backward(), em_b.forward_backward()):
        assert np.array_equal(x, y)
    L = N.lib()
    mlab = np.empty(store.n_windows, np.int8)
    mll = np.empty(store.n_chunks)
    assert L.hf_get_viterbi_minlen_labels(em_a._h, mlab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
    assert L.hf_get_viterbi_minlen_chunk_log_probs(em_a._h, mll.ctypes.data_as(C.POINTER(C.c_double))) == N.HF_OK
    assert np.array_equal(mlab, mlv[0]) and np.array_equal(mll, mlv[1])
    assert np.array_equal(r.posterior(), mpost)
    lab2 = np.empty(store.n_windows, np.int8)
    assert L.hf_get_minlen_posterior_labels(em_a._h, lab2.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
    assert np.array_equal(lab2, r.labels)
    hmm.EM_runOneIterationForList(em_a, model); st2_a = model.estimators.copy(); hmm.HMM_resetEstimators(model)   # the next pass
    hmm.EM_runOneIterationForList(em_b, model); st2_b = model.estimators.copy()
    assert np.array_equal(st2_a, st2_b)
    assert np.array_equal(em_a.labels(), em_b.labels())
    em_a.close(); em_b.close()


# ---- a caller's stream -------------------------------------------------------------------------------------------------------------------

def test_callers_stream():
    store, model, alpha = _case("teg-2regions-K3")
    em0 = hmm.EMList(store, model)
    want = _run(em0, model, TRACK_LEN)
    em0.close()
    with Streams() as streams:
        s = streams.new(non_blocking=True)
        em = hmm.EMList(store, model, stream=s)
        streams.h.delay(s)                                 # whatever ran on the null stream instead would run ahead of this
        got = _run(em, model, TRACK_LEN)
        assert _same(want, got)
        em.close()


# ---- command line ------------------------------------------------------------------------------------------------------------------------

def _tsv(path):
    return [line.split("\t") for line in open(path).read().splitlines() if not line.startswith("#")]


def test_cli_lengths_below_one_window_are_plain_em(tmp_path):
    """--minimumLengths below one window each: every length becomes 1 window, the constrained step is the plain step to rounding."""
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = hmm.getBestNumberOfCollapsedComps(store)
    args = ["-i", str(binp), "-W", "4000", "-n", "3", "-p", str(K)]
    TML._cli(args, tmp_path / "plain")
    TML._cli(args + ["--minimumLengths", "100,100,100", "--lengthConstrainedEM"], tmp_path / "con")
    a, b = tmp_path / "plain", tmp_path / "con"
    assert (a / "final_flagger_prediction.bed").read_bytes() == (b / "final_flagger_prediction.bed").read_bytes()
    for name in ("emission_final.tsv", "transition_final.tsv"):
        for ra, rb in zip(_tsv(a / name), _tsv(b / name)):
            for x, y in zip(ra, rb):
                try:
                    fx, fy = float(x), float(y)
                except ValueError:
                    assert x == y
                    continue
                assert abs(fx - fy) <= 1e-6 * abs(fx), (name, x, y)
    rows = _tsv(b / "length_constrained_em.tsv")
    assert len(rows) == 3 and all(float(r[3]) == 0.0 for r in rows)


def test_cli_equals_the_python_loop(tmp_path):
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = hmm.getBestNumberOfCollapsedComps(store)
    wl = 4000
    args = ["-i", str(binp), "-W", str(wl), "-n", "3", "-p", str(K), "--minimumLengths", "%d,%d,%d" % (wl * TRACK_LEN[0], wl * TRACK_LEN[1], wl * TRACK_LEN[3]),
            "--lengthConstrainedEM"]
    TML._cli(args, tmp_path / "cli")
    st = synth.WindowStore.read_bin(str(binp))
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, np.zeros((4, 4)))
    em = hmm.EMList(st, model)
    os.makedirs(tmp_path / "py")
    lls = hmm.runHMMFlagger(em, model, 3, 0.001, str(tmp_path / "py"), constrainedMinLen=TRACK_LEN)
    em.close()
    for name in ("emission_final.tsv", "transition_final.tsv", "length_constrained_em.tsv", "loglikelihood.tsv"):
        assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / "py" / name).read_bytes(), name
    rows = _tsv(tmp_path / "cli" / "length_constrained_em.tsv")
    assert len(rows) == 3 and all(float(r[3]) < 0.0 for r in rows)
    assert [float(r[1]) for r in rows] == [float("%.4f" % v) for v in lls[:3]]
