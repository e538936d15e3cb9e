"""The posterior under minimum run lengths on the GPU (hf_minlen_posterior, hmm.EM_runMinLengthPosteriorForList, hmm_flagger
--constrainedPosterior) against mpmath enumeration of the admissible paths on tiny stores and the float64 numpy reference
(tests/minlen_post_ref.py) elsewhere.

Tolerances: against enumeration log_mass within 1e-12 (1 + |log Z|) and post within 1e-12 absolute + 1e-9 relative; against the numpy
reference log_mass and log Z_adm within 1e-10 + 1e-9 |ref| (the range getters' tolerance) and post within 1e-9 relative where the
reference is at least 1e-250, elsewhere 0 <= post <= 1e-249; no entry is left out.  Every test prints its largest deviations before it
asserts (pytest -s)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from hip_streams import Streams
import geometry_cases as G
import minlen_post_ref as R
import minlen_ref
import test_minlen_gpu as TML

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]
ONES = (1, 1, 1, 1)
TRACK_LEN = TML.TRACK_LEN


def _result(em, model, min_len):
    """(post, labels, chunk_log_mass, chunk_log_z_adm, log_mass) of one call, the posterior fetched."""
    r = hmm.EM_runMinLengthPosteriorForList(em, model, min_len)
    return r.posterior(), r.labels, r.chunk_log_mass, r.chunk_log_z_adm, r.log_mass


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def _close_logs(got, ref, what):
    err = np.abs(got - ref)
    print("%s: largest deviation %.3e (bound 1e-10 + 1e-9 |ref|)" % (what, float(err.max()) if err.size else 0.0))
    assert np.all(err <= 1e-10 + 1e-9 * np.abs(ref)), what


def _check(store, ref, got, what):
    """`got` against the numpy reference; argmax labels; the total."""
    post, labels, mass, lza, tot = got
    rpost, rmass, rlza, _ = ref
    _close_logs(mass, rmass, what + " log_mass")
    _close_logs(lza, rlza, what + " log_z_adm")
    big = rpost >= 1e-250
    print("%s: post largest relative deviation %.3e over %d entries, %d entries below the floor"
          % (what, float(np.max(np.abs(post[big] - rpost[big]) / rpost[big])), int(big.sum()), int((~big).sum())))
    R.close_post(post, rpost)
    assert np.array_equal(labels, np.argmax(post, axis=1).astype(np.int8))          # (numpy's argmax: the first largest entry)
    assert tot == float(np.sum(mass)) or abs(tot - np.sum(mass)) <= 1e-12 * abs(tot)


# ---- tiny stores against enumeration ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed,hifi", minlen_ref.TINY_CASES)
def test_tiny_stores_equal_path_enumeration(algo, model_type, seed, hifi):
    store, model, alpha, enum = R.tiny_case(model_type, seed, hifi)
    em = hmm.EMList(store, model, algo=algo)
    T = np.diff(store.chunk_off)
    for min_len in minlen_ref.TINY_MIN_LENS:
        post, labels, mass, lza, tot = _result(em, model, min_len)
        below_one = R.check_against_enumeration(store, enum, min_len, post, mass, lza, post_rel=1e-9)
        assert below_one >= 1 if min_len == (3, 2, 2, 2) else below_one == 0
        assert np.all(np.abs(mass[T <= 2]) <= 1e-12 * (1 + np.abs(lza[T <= 2])))      # one or two windows: mass 1
        if min_len == ONES:
            assert np.all(mass == 0.0) and tot == 0.0
        assert np.array_equal(labels, np.argmax(post, axis=1).astype(np.int8))
    em.close()


# ---- lane and block geometry -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_len", [(3, 5, 1, 7), (16, 16, 16, 16), (61, 1, 1, 1)])
def test_lane_and_block_geometry(min_len):
    """Chunks around the 64-window staging block, the 8-step rescaling and a minimum length of 16; 64 lanes, one state owning 61."""
    store, model = TML._geometry()
    ref = R.reference(store, model, synth.HIFI_ALPHA, min_len)
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        res.append(_result(em, model, min_len))
        em.close()
    _check(store, ref, res[0], "geometry %s" % (min_len,))
    assert np.sum(ref[1] < -1e-6) >= store.n_chunks // 2                         # the rule removes mass in most chunks
    assert _same(res[0], res[1])


# ---- chunk ends at the emission floor -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_len", [(3, 5, 1, 7), ONES, (16, 16, 16, 16)])
def test_chunk_ends_at_the_emission_floor(min_len):
    """Twelve windows at a chunk's first end, last end or both (and a chunk that is almost nothing else) whose rows are the 1e-40
    emission floor times a transition probability: both walks lose 40 decimal digits per step from their very first window, before
    the first of the 8-step rescalings.  The values stay at the tolerances of every other store, and no error is raised."""
    store, model, alpha = R.floored_case()
    ref = R.reference(store, model, alpha, min_len)
    assert np.all(np.isfinite(ref[2])) and np.all(ref[2] < -1000)
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        res.append(_result(em, model, min_len))
        em.close()
    _check(store, ref, res[0], "floored ends %s" % (min_len,))
    dev = np.abs(res[0][0].sum(axis=1) - 1.0)
    assert np.all(dev <= 4 * np.finfo(float).eps)
    if min_len == ONES:
        assert np.all(res[0][2] == 0.0)
    assert _same(res[0], res[1])


def test_an_older_result_refuses_the_posterior_of_a_later_run():
    store, model = TML._geometry()
    em = hmm.EMList(store, model)
    first = em.minlen_posterior(model, TRACK_LEN)
    want = first.posterior()
    second = em.minlen_posterior(model, ONES)
    with pytest.raises(RuntimeError):
        first.posterior()
    assert not np.array_equal(second.posterior(), want)
    em.close()
    with pytest.raises(RuntimeError):
        second.posterior()


# ---- a realistic track -----------------------------------------------------------------------------------------------------------

def test_realistic_track():
    store, model, refs, _ = TML._track()
    ref = R.reference(store, model, synth.HIFI_ALPHA, TRACK_LEN)
    em = hmm.EMList(store, model)
    a = _result(em, model, TRACK_LEN)
    _check(store, ref, a, "track")
    post, labels, mass, lza, tot = a
    dev = np.abs(post.sum(axis=1) - 1.0)
    print("track: |sum_s post - 1| at most %.3e; log_mass total %.6f, smallest chunk %.6f" % (float(dev.max()), tot, float(mass.min())))
    assert np.all(dev <= 4 * np.finfo(float).eps)
    assert np.all(mass <= 1e-12) and np.any(mass < 0.0)
    vit = em.viterbi_minlen(model, TRACK_LEN)[0]
    assert np.all(post[np.arange(store.n_windows), vit] > 0.0)                     # the best admissible path is possible under the rule
    assert _same(a, _result(em, model, TRACK_LEN))                                 # a second call: identical bits
    em.close()


def test_all_ones_is_the_posterior_of_a_full_pass():
    store, model, _, _ = TML._track()
    em = hmm.EMList(store, model)
    post, labels, mass, lza, tot = _result(em, model, ONES)
    assert np.all(mass == 0.0) and tot == 0.0
    hmm.EM_runOneIterationForList(em, model)
    hmm.HMM_resetEstimators(model)
    want = em.posterior()
    big = want >= 1e-250
    print("all ones: largest relative deviation from hf_get_posterior %.3e" % float(np.max(np.abs(post[big] - want[big]) / want[big])))
    R.close_post(post, want)
    em.close()


# ---- chunks without windows, windows outside every chunk -------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunks_and_uncovered_windows(algo):
    """The grid store of tests/test_geometry_gpu.py (tests/geometry_cases.py) with chunks without windows put in, and with windows in
    front of the first chunk and behind the last one: the values are the bits of the store without them."""
    model_type, seed = G.CASES[0]
    store, model, alpha, _ = G.case(model_type, seed)
    em0 = hmm.EMList(store, model, algo=algo)
    base = _result(em0, model, TRACK_LEN)
    _check(store, R.reference(store, model, alpha, TRACK_LEN), base, "grid store")
    em0.close()
    est, src = G.with_empty_chunks(store)
    em = hmm.EMList(est, model, algo=algo)
    post, labels, mass, lza, tot = _result(em, model, TRACK_LEN)
    assert np.array_equal(post, base[0]) and np.array_equal(labels, base[1])
    assert np.array_equal(mass[src >= 0], base[2]) and np.array_equal(lza[src >= 0], base[3])
    assert np.all(mass[src < 0] == 0.0) and np.all(lza[src < 0] == 0.0) and not np.signbit(mass[src < 0]).any()
    em.close()
    ust = G.with_uncovered_windows(store, np.random.default_rng(5))
    a, n = G.FRONT, ust.n_windows
    b = a + store.n_windows
    em = hmm.EMList(ust, model, algo=algo)
    r = hmm.EM_runMinLengthPosteriorForList(em, model, TRACK_LEN)
    outside = np.r_[0:a, b:n]
    assert np.all(r.labels[outside] == -1) and np.array_equal(r.labels[a:b], base[1])
    assert np.array_equal(r.chunk_log_mass, base[2]) and np.array_equal(r.chunk_log_z_adm, base[3]) and r.log_mass == base[4]
    assert np.array_equal(r.posterior(a, store.n_windows), base[0])
    for f, cnt in [(0, 1), (a - 1, 1), (a - 1, 4), (0, n), (a, store.n_windows + 1), (b, 1), (n - 1, 1)]:
        with pytest.raises(N.HFError) as ei:
            r.posterior(f, cnt)
        assert ei.value.code == N.HF_E_ARG, (f, cnt)
    assert r.posterior(a, 0).shape == (0, 4)
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunk_list(algo):
    full = synth.synthesize([50_000], 1000, 20_000, [20], seed=2)
    store = full.subset_chunks([])
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, full, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model, algo=algo)
    r = hmm.EM_runMinLengthPosteriorForList(em, model, TRACK_LEN)
    assert r.labels.size == 0 and r.chunk_log_mass.size == 0 and r.log_mass == 0.0 and r.posterior().shape == (0, 4)
    em.close()


# ---- arguments and errors --------------------------------------------------------------------------------------------------------

def test_arguments_getters_and_errors():
    store = synth.config(2, 0.02)
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, store, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model)
    L = N.lib()
    lab = np.empty(store.n_windows, np.int8)
    post = np.empty((store.n_windows, 4))
    m = np.empty(store.n_chunks)
    pd, pi8 = C.POINTER(C.c_double), C.POINTER(C.c_int8)

    def getters_refuse():
        assert L.hf_get_minlen_posterior(em._h, 0, store.n_windows, post.ctypes.data_as(pd)) == N.HF_E_ARG
        assert L.hf_get_minlen_posterior_labels(em._h, lab.ctypes.data_as(pi8)) == N.HF_E_ARG
        assert L.hf_get_minlen_chunk_log_mass(em._h, m.ctypes.data_as(pd), None) == N.HF_E_ARG

    getters_refuse()                                       # before any run
    assert L.hf_minlen_posterior_finish(em._h, None, None) == N.HF_E_ARG
    p = model.params()
    assert L.hf_minlen_posterior(em._h, C.byref(p), None, None) == N.HF_E_ARG
    assert L.hf_minlen_posterior(em._h, None, (C.c_int32 * 4)(1, 1, 1, 1), None) == N.HF_E_ARG
    assert L.hf_minlen_posterior(None, C.byref(p), (C.c_int32 * 4)(1, 1, 1, 1), None) == N.HF_E_ARG
    for bad_len in ((3, 0, 1, 1), (-1, 1, 1, 1), (62, 1, 1, 1), (2 ** 31 - 1, 2 ** 31 - 1, 1, 1)):
        with pytest.raises(N.HFError) as ei:
            em.minlen_posterior(model, bad_len)
        assert ei.value.code == N.HF_E_ARG, bad_len
    getters_refuse()                                       # still no finished run
    with pytest.raises(TypeError):
        hmm.EM_runMinLengthPosteriorForList(object(), model, ONES)
    good = em.minlen_posterior(model, (61, 1, 1, 1))       # a sum of exactly 64 is served
    good = (good.posterior(), good.labels, good.chunk_log_mass, good.chunk_log_z_adm, good.log_mass)
    assert not np.isnan(good[0]).any()
    assert L.hf_get_minlen_posterior(em._h, 0, store.n_windows, None) == N.HF_E_ARG
    assert L.hf_get_minlen_posterior(em._h, -1, 2, post.ctypes.data_as(pd)) == N.HF_E_ARG
    assert L.hf_get_minlen_posterior(em._h, 1, store.n_windows, post.ctypes.data_as(pd)) == N.HF_E_ARG
    assert L.hf_get_minlen_chunk_log_mass(em._h, None, m.ctypes.data_as(pd)) == N.HF_E_ARG
    assert L.hf_get_minlen_chunk_log_mass(em._h, m.ctypes.data_as(pd), None) == N.HF_OK and np.array_equal(m, good[2])
    R_ = model.numberOfRegions
    bad = model.copy()
    v = bad.param_vector().reshape(R_, -1)
    v[:, 20:24] = 0.0                                      # start row: no path has weight
    bad.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.minlen_posterior(bad, TRACK_LEN)
    assert ei.value.code == N.HF_E_SCALE
    getters_refuse()                                       # a failed run is no finished run
    nan = model.copy()
    v = nan.param_vector().reshape(R_, -1)
    v[:, 27 + 3 * 16] = np.nan                             # mean of Col, component 0
    nan.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.minlen_posterior(nan, TRACK_LEN)
    assert ei.value.code == N.HF_E_NAN
    again = em.minlen_posterior(model, (61, 1, 1, 1))      # and the context answers correctly afterwards
    assert _same(good, (again.posterior(), again.labels, again.chunk_log_mass, again.chunk_log_z_adm, again.log_mass))
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_rows_that_leave_a_chunk_no_weight_are_reported(algo):
    """The construction of test_estep_gpu.test_scale_underflow_is_reported with the small transition entries exactly 0: every
    transition leads to Err, and a window above the trunc point has Err emission exactly 0, so no path of the chunk has weight."""
    store = synth.synthesize([400_000], 1000, 1_000_000, [20], seed=2)
    store.cov[100:104] = 250
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 2, store, np.zeros((4, 4)))
    v = model.param_vector().reshape(1, -1)
    t = v[0, :25].reshape(5, 5)
    t[:4, :4] = 0.0
    t[:4, 0] = 1.0 - 1e-4
    model.set_param_vector(v.ravel())
    em = hmm.EMList(store, model, algo=algo)
    for min_len in (ONES, TRACK_LEN):
        with pytest.raises(N.HFError) as ei:
            em.minlen_posterior(model, min_len)
        assert ei.value.code == N.HF_E_SCALE, min_len
    em.close()


# ---- no disturbance --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
def test_no_disturbance_of_the_last_pass_and_the_decoders(algo):
    store = synth.config(2, 0.05)
    alpha = synth.HIFI_ALPHA
    model = hmm.createModel(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, store, alpha)
    em_a = hmm.EMList(store, model, algo=algo)
    em_b = hmm.EMList(store, model, algo=algo)
    for em in (em_a, em_b):
        hmm.EM_runOneIterationForList(em, model)
    hmm.HMM_estimateParameters(model, 1e-3)
    hmm.HMM_resetEstimators(model)
    hmm.EM_runOneIterationForList(em_a, model); st_a = model.estimators.copy(); hmm.HMM_resetEstimators(model)
    hmm.EM_runOneIterationForList(em_b, model); st_b = model.estimators.copy(); hmm.HMM_resetEstimators(model)
    assert np.array_equal(st_a, st_b)
    vit = em_a.viterbi(model)
    mlv = em_a.viterbi_minlen(model, TRACK_LEN)
    smp = em_a.sample_paths(model, 2, 7)
    other = model.copy()                                   # the feature runs with DIFFERENT parameters
    v = other.param_vector().reshape(other.numberOfRegions, -1)
    v[:, 27:27 + 4 * 16] *= 1.1
    other.set_param_vector(v.ravel())
    r1 = _result(em_a, other, TRACK_LEN)
    r2 = _result(em_a, other, (2, 2, 2, 2))
    assert not np.array_equal(r1[0], r2[0])
    assert not np.array_equal(r1[0], em_a.posterior())
    assert np.array_equal(em_a.labels(), em_b.labels())
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    for x, y in zip(em_a.forward_backward(), em_b.forward_backward()):
        assert np.array_equal(x, y)
    lab, ll = TML._viterbi_results(em_a)                   # hf_viterbi's last results, hf_viterbi_minlen's and the sampler's
    assert np.array_equal(lab, vit[0]) and np.array_equal(ll, vit[1])
    L = N.lib()
    mlab = np.empty(store.n_windows, np.int8)
    mll = np.empty(store.n_chunks)
    assert L.hf_get_viterbi_minlen_labels(em_a._h, mlab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
    assert L.hf_get_viterbi_minlen_chunk_log_probs(em_a._h, mll.ctypes.data_as(C.POINTER(C.c_double))) == N.HF_OK
    assert np.array_equal(mlab, mlv[0]) and np.array_equal(mll, mlv[1])
    assert np.array_equal(TML._sample_results(em_a, 2), smp)
    hmm.EM_runOneIterationForList(em_a, model); st2_a = model.estimators.copy(); hmm.HMM_resetEstimators(model)   # the next pass
    hmm.EM_runOneIterationForList(em_b, model); st2_b = model.estimators.copy()
    assert np.array_equal(st2_a, st2_b)
    assert np.array_equal(em_a.labels(), em_b.labels())
    em_a.close(); em_b.close()


# ---- a caller's stream -----------------------------------------------------------------------------------------------------------

def test_callers_stream():
    store, model, _, _ = TML._track()
    em0 = hmm.EMList(store, model)
    want = _result(em0, model, TRACK_LEN)
    em0.close()
    with Streams() as streams:
        s = streams.new(non_blocking=True)
        em = hmm.EMList(store, model, stream=s)
        streams.h.delay(s)                                 # whatever ran on the null stream instead would run ahead of this
        got = _result(em, model, TRACK_LEN)
        assert _same(want, got)
        em.close()


# ---- command line ----------------------------------------------------------------------------------------------------------------

def test_cli_writes_the_two_files_and_changes_nothing_else(tmp_path):
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = hmm.getBestNumberOfCollapsedComps(store)
    args = ["-i", str(binp), "-W", "4000", "-n", "0", "-P", "-p", str(K)] + TML.MINLEN_ARGS      # 2, 3, 1, 2 windows
    TML._cli(args, tmp_path / "plain")
    TML._cli(args + ["--constrainedPosterior"], tmp_path / "con")
    a, b = tmp_path / "plain", tmp_path / "con"
    names = sorted(os.listdir(a))
    assert sorted(set(os.listdir(b)) - set(names)) == ["admissible_mass.tsv", "posterior_prediction_min_lengths.bed"]
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    assert "posterior_prediction_final.bed" in names and "final_flagger_prediction.bed" in names
    st = synth.WindowStore.read_bin(str(binp))
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, np.zeros((4, 4)))
    em = hmm.EMList(st, model)
    r = em.minlen_posterior(model, (2, 3, 1, 2))
    rows = (b / "admissible_mass.tsv").read_text().splitlines()
    assert rows[0].startswith("#") and [int(x) for x in rows[1].split("\t")] == [2, 3, 1, 2] and rows[2].startswith("#")
    f = rows[3].split("\t")
    assert f[0] == "all" and int(f[1]) == st.n_chunks and int(f[2]) == st.n_windows
    assert abs(float(f[3]) - r.log_mass) <= 1e-9 * (1 + abs(r.log_mass)) and r.log_mass < 0.0
    per = {}
    for c in range(st.n_chunks):
        per[st.chunk_ctg[c]] = per.get(st.chunk_ctg[c], 0.0) + r.chunk_log_mass[c]
    assert len(rows) == 4 + len(per)
    for line in rows[4:]:
        g = line.split("\t")
        assert abs(float(g[3]) - per[g[0]]) <= 1e-9 * (1 + abs(per[g[0]])), g
    bed = (b / "posterior_prediction_min_lengths.bed").read_text()
    assert bed != (a / "posterior_prediction_final.bed").read_text() and len(bed.splitlines()) >= 2
    em.close()
