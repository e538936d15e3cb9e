"""The admissible path sampler on the GPU (hf_sample_paths_minlen, hmm.EMList.sample_paths_minlen, hmm_flagger --admissibleSamples)
against the float64 numpy sampler (tests/minlen_sample_ref.py), which uses the same uniforms and the same draw rule.

Exactness.  The device's rows come from its own exp and the reference's from numpy's, so a draw whose uniform lands within rounding of a
cumulative-sum boundary may go the other way.  test_sampling_gpu's rule: a sample may differ from the reference only where, in a
chunk, the last differing window was decided by a draw whose reference margin min_i |x - c_i| / c_{n-1} is below 1e-12, and at most one
such event per check (with margins uniform on [0, 1] the expected number over these shapes is below 1e-5).  Admissibility is an exact
integer check of every sample."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from hip_streams import Streams
from test_sampling_gpu import _near_tie_events
import geometry_cases as G
import minlen_post_ref
import minlen_ref
import minlen_sample_ref as R
import sampling_ref as S
import test_minlen_gpu as TML

pytestmark = pytest.mark.gpu
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]
ONES = (1, 1, 1, 1)
TRACK_LEN = TML.TRACK_LEN
GEOMETRY_LENS = [(3, 5, 1, 7), (16, 16, 16, 16), (61, 1, 1, 1)]


def _admissible(labels, store, min_len):
    for k, row in enumerate(labels):
        ok = minlen_ref.admissible(row, store.chunk_off, min_len)
        assert ok.all(), ("sample", k, "chunks", np.flatnonzero(~ok)[:5])


def _check(store, ref, got, min_len, first=0):
    """`got` = samples first .. of the reference's: equal under the margin rule, and admissible."""
    lab, marg, fmarg = (x[first:first + got.shape[0]] for x in ref)
    assert got.shape == lab.shape and got.dtype == np.int8
    events = _near_tie_events(got, lab, marg, fmarg, store.chunk_off)
    assert events <= 1, events
    _admissible(got, store, min_len)


# ---- tiny stores -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed,hifi", minlen_ref.TINY_CASES)
def test_tiny_stores_equal_the_numpy_sampler(algo, model_type, seed, hifi):
    store, model, alpha, _ = minlen_ref.tiny_case(model_type, seed, hifi)
    em = hmm.EMList(store, model, algo=algo)
    for min_len in minlen_ref.TINY_MIN_LENS:
        got = hmm.EM_sampleMinLengthPathsForList(em, model, min_len, 64, 17 + seed)
        _check(store, R.reference(store, model, alpha, min_len, 17 + seed, range(64)), got, min_len)
    em.close()


# ---- lane and block geometry -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _geometry_reference(min_len):
    store, model = TML._geometry()
    return R.reference(store, model, synth.HIFI_ALPHA, min_len, 23, range(65))


@pytest.mark.parametrize("min_len", GEOMETRY_LENS)
def test_lane_and_block_geometry(min_len):
    """Chunks around the 64-window block of the walk and the 16-window groups of its loads; 64 lanes, one state owning 61; a partial
    group of samples, a full one, and a second group of one."""
    store, model = TML._geometry()
    ref = _geometry_reference(min_len)
    ems = [hmm.EMList(store, model, algo=algo) for algo in ALGOS]
    for K in (1, 5, 64, 65):
        res = [em.sample_paths_minlen(model, min_len, K, 23) for em in ems]
        _check(store, ref, res[0], min_len)
        assert np.array_equal(res[0], res[1])
    free = ems[0].sample_paths(model, 8, 23)
    assert not all(minlen_ref.admissible(row, store.chunk_off, min_len).all() for row in free)      # the rule does bite here
    for em in ems:
        em.close()


# ---- a realistic track -----------------------------------------------------------------------------------------------------------

def test_realistic_track():
    store, model, _, _ = TML._track()
    em = hmm.EMList(store, model)
    got = em.sample_paths_minlen(model, TRACK_LEN, 8, 2024)
    _check(store, R.reference(store, model, synth.HIFI_ALPHA, TRACK_LEN, 2024, range(8)), got, TRACK_LEN)
    post = em.minlen_posterior(model, TRACK_LEN).posterior()
    for row in got:
        assert np.all(post[np.arange(store.n_windows), row] > 0.0)        # no sample visits a state the constrained posterior excludes
    em.close()


def test_all_ones_is_hf_sample_paths():
    store, model, _, _ = TML._track()
    em = hmm.EMList(store, model)
    a = em.sample_paths_minlen(model, ONES, 16, 99, first_sample=5)
    b = em.sample_paths(model, 16, 99, first_sample=5)
    A, end = S.rows(store, model, synth.HIFI_ALPHA)
    _, marg, fmarg = S.ffbs(A, end, store.chunk_off, 99, range(5, 21))
    assert _near_tie_events(a, b, marg, fmarg, store.chunk_off) <= 1
    em.close()


def test_grouping_repeatability_contexts_and_a_callers_stream():
    store, model, _, _ = TML._track()
    em = hmm.EMList(store, model)
    whole = em.sample_paths_minlen(model, TRACK_LEN, 64, 5)
    parts = np.concatenate([em.sample_paths_minlen(model, TRACK_LEN, 24, 5), em.sample_paths_minlen(model, TRACK_LEN, 40, 5, first_sample=24)])
    assert np.array_equal(whole, parts)
    assert np.array_equal(whole, em.sample_paths_minlen(model, TRACK_LEN, 64, 5))                # a second call: identical bits
    other = em.sample_paths_minlen(model, TRACK_LEN, 64, 6)
    assert np.mean(whole != other) > 1e-4
    assert not np.array_equal(whole, em.sample_paths_minlen(model, (2, 2, 2, 2), 64, 5))         # the lengths are part of a sample
    em.close()
    seq = hmm.EMList(store, model, algo=N.HF_ALGO_SEQ)
    assert np.array_equal(whole, seq.sample_paths_minlen(model, TRACK_LEN, 64, 5))
    seq.close()
    with Streams() as streams:
        s = streams.new(non_blocking=True)
        ems = hmm.EMList(store, model, stream=s)
        streams.h.delay(s)                                 # whatever ran on the null stream instead would run ahead of this
        assert np.array_equal(whole, ems.sample_paths_minlen(model, TRACK_LEN, 64, 5))
        ems.close()


# ---- chunks without windows, windows outside every chunk -------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunks_and_uncovered_windows(algo):
    model_type, seed = G.CASES[0]
    store, model, alpha, _ = G.case(model_type, seed)
    em0 = hmm.EMList(store, model, algo=algo)
    base = em0.sample_paths_minlen(model, TRACK_LEN, 8, 3)
    _check(store, R.reference(store, model, alpha, TRACK_LEN, 3, range(8)), base, TRACK_LEN)
    em0.close()
    # The uniform of a window's draw is indexed by the window's global index and that of a chunk's final lane by n_windows + the
    # chunk's index in the list (include/hmm_flagger_hip.h, as hf_sample_paths: tests/test_geometry_gpu.py _check_decoders).  A track
    # with chunks without windows, or with windows in front of its first chunk, therefore draws the same weights with other
    # uniforms: its samples are the reference's on THAT chunk list, not the bits of the grid store's.
    A, end = S.rows(store, model, alpha)
    est, src = G.with_empty_chunks(store)
    end_e = np.zeros((est.n_chunks, 4))
    end_e[src >= 0] = end
    em = hmm.EMList(est, model, algo=algo)
    got = em.sample_paths_minlen(model, TRACK_LEN, 8, 3)
    _check(est, R.sample(R.tables(A, end_e, est.chunk_off, TRACK_LEN), 3, range(8)), got, TRACK_LEN)
    assert np.any(got != base)                                              # (other uniforms for the final lanes)
    em.close()
    ust = G.with_uncovered_windows(store, np.random.default_rng(5))
    a, n = G.FRONT, ust.n_windows
    b = a + store.n_windows
    em = hmm.EMList(ust, model, algo=algo)
    got = em.sample_paths_minlen(model, TRACK_LEN, 8, 3)
    assert got.shape == (8, n)
    assert np.all(got[:, np.r_[0:a, b:n]] == -1)                              # exactly -1 outside every chunk
    _admissible(got[:, a:b], store, TRACK_LEN)
    tab = R.tables(A, end, store.chunk_off, TRACK_LEN)
    tab["off"] = tab["off"] + a
    for key in ("W4", "C4", "W2", "C2"):
        tab[key] = np.concatenate([np.zeros((a,) + tab[key].shape[1:]), tab[key], np.zeros((n - b,) + tab[key].shape[1:])])
    lab, marg, fmarg = R.sample(tab, 3, range(8), n)
    assert _near_tie_events(got[:, a:b], lab[:, a:b], marg[:, a:b], fmarg, store.chunk_off) <= 1
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunk_list(algo):
    full = synth.synthesize([50_000], 1000, 20_000, [20], seed=2)
    store = full.subset_chunks([])
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, full, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model, algo=algo)
    assert em.sample_paths_minlen(model, TRACK_LEN, 5, 1).shape == (5, 0)
    em.close()


# ---- chunk ends at the emission floor -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_len", [(3, 5, 1, 7), (16, 16, 16, 16)])
def test_chunk_ends_at_the_emission_floor(min_len):
    """minlen_post_ref.floored_case: the stored lanes sink to 2e-270 over eight floored rows; the scaling before the products keeps
    the draws' weights normal, and no error is raised."""
    store, model, alpha = minlen_post_ref.floored_case()
    ref = R.reference(store, model, alpha, min_len, 41, range(8))
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        res.append(em.sample_paths_minlen(model, min_len, 8, 41))
        em.close()
    _check(store, ref, res[0], min_len)
    assert np.array_equal(res[0], res[1])


# ---- no disturbance --------------------------------------------------------------------------------------------------------------

def _mls_results(em, n):
    L = N.lib()
    out = np.empty((n, em.store.n_windows), np.int8)
    for k in range(n):
        assert L.hf_get_minlen_sample_labels(em._h, k, out[k].ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
    return out


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

    def decoders(em):
        vit = em.viterbi(model)
        mlv = em.viterbi_minlen(model, TRACK_LEN)
        smp = em.sample_paths(model, 2, 7)
        r = em.minlen_posterior(model, TRACK_LEN)
        return vit, mlv, smp, (r.posterior(), r.labels, r.chunk_log_mass, r.chunk_log_z_adm, r.log_mass)

    want = decoders(em_b)                                  # the twin never samples admissible paths
    vit, mlv, smp, mlp = decoders(em_a)
    other = model.copy()                                   # the feature runs with DIFFERENT parameters, twice (the buffers grow in between)
    v = other.param_vector().reshape(other.numberOfRegions, -1)
    v[:, 27:27 + 4 * 16] *= 1.1
    other.set_param_vector(v.ravel())
    em_a.sample_paths_minlen(other, (2, 2, 2, 2), 3, 1)
    mine = em_a.sample_paths_minlen(other, TRACK_LEN, 70, 2)
    assert np.array_equal(em_a.labels(), em_b.labels())
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    for x, y in zip(em_a.forward_backward(), em_b.forward_backward()):
        assert np.array_equal(x, y)
    lab, ll = TML._viterbi_results(em_a)
    assert np.array_equal(lab, vit[0]) and np.array_equal(ll, vit[1]) and np.array_equal(lab, want[0][0])
    L = N.lib()
    mlab = np.empty(store.n_windows, np.int8)
    mll = np.empty(store.n_chunks)
    pd = C.POINTER(C.c_double)
    assert L.hf_get_viterbi_minlen_labels(em_a._h, mlab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
    assert L.hf_get_viterbi_minlen_chunk_log_probs(em_a._h, mll.ctypes.data_as(pd)) == N.HF_OK
    assert np.array_equal(mlab, mlv[0]) and np.array_equal(mll, mlv[1]) and np.array_equal(mlab, want[1][0])
    assert np.array_equal(TML._sample_results(em_a, 2), smp) and np.array_equal(smp, want[2])
    post = np.empty((store.n_windows, 4))                  # hf_minlen_posterior's forward lanes are its own: the getters answer as before
    assert L.hf_get_minlen_posterior(em_a._h, 0, store.n_windows, post.ctypes.data_as(pd)) == N.HF_OK
    assert L.hf_get_minlen_posterior_labels(em_a._h, mlab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
    mass, lza = np.empty(store.n_chunks), np.empty(store.n_chunks)
    assert L.hf_get_minlen_chunk_log_mass(em_a._h, mass.ctypes.data_as(pd), lza.ctypes.data_as(pd)) == N.HF_OK
    for got, a, b in zip((post, mlab, mass, lza), mlp[:4], want[3][:4]):
        assert np.array_equal(got, a) and np.array_equal(got, b)
    assert mlp[4] == want[3][4]
    r = em_a.minlen_posterior(model, (2, 2, 2, 2))          # ... and a later run of it leaves the sampler's labels alone
    assert not np.array_equal(r.posterior(), post)
    assert np.array_equal(_mls_results(em_a, 70), mine)
    hmm.EM_runOneIterationForList(em_a, model); st2_a = model.estimators.copy(); hmm.HMM_resetEstimators(model)   # the next pass
    hmm.EM_runOneIterationForList(em_b, model); st2_b = model.estimators.copy()
    assert np.array_equal(st2_a, st2_b)
    assert np.array_equal(em_a.labels(), em_b.labels())
    em_a.close(); em_b.close()


# ---- arguments and errors --------------------------------------------------------------------------------------------------------

def test_arguments_getters_and_errors():
    store = synth.config(2, 0.02)
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, store, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model)
    L = N.lib()
    lab = np.empty(store.n_windows, np.int8)
    lp = lab.ctypes.data_as(C.POINTER(C.c_int8))
    four = lambda *v: (C.c_int32 * 4)(*v)
    assert L.hf_get_minlen_sample_labels(em._h, 0, lp) == N.HF_E_ARG                     # before any call
    assert L.hf_sample_minlen_finish(em._h, None) == N.HF_E_ARG
    p = model.params()
    assert L.hf_sample_paths_minlen(em._h, C.byref(p), None, 0, 1, 1, None) == N.HF_E_ARG
    assert L.hf_sample_paths_minlen(em._h, None, four(1, 1, 1, 1), 0, 1, 1, None) == N.HF_E_ARG
    assert L.hf_sample_paths_minlen(None, C.byref(p), four(1, 1, 1, 1), 0, 1, 1, None) == N.HF_E_ARG
    assert L.hf_minlen_sample_capacity(None, four(1, 1, 1, 1)) == N.HF_E_ARG
    assert L.hf_minlen_sample_capacity(em._h, None) == N.HF_E_ARG
    assert L.hf_get_minlen_sample_labels(None, 0, lp) == N.HF_E_ARG
    for bad_len in ((3, 0, 1, 1), (-1, 1, 1, 1), (62, 1, 1, 1), (2 ** 31 - 1, 2 ** 31 - 1, 1, 1)):     # a length 0, a sum of 65
        with pytest.raises(N.HFError) as ei:
            em.sample_paths_minlen(model, bad_len, 4, 1)
        assert ei.value.code == N.HF_E_ARG, bad_len
        assert L.hf_minlen_sample_capacity(em._h, four(*bad_len)) == N.HF_E_ARG
    with pytest.raises(TypeError):
        hmm.EM_sampleMinLengthPathsForList(object(), model, ONES, 4, 1)
    cap = em.minlen_sample_capacity(TRACK_LEN)
    assert cap >= 64 and em.minlen_sample_capacity((61, 1, 1, 1)) <= em.minlen_sample_capacity(ONES)
    ml = four(*TRACK_LEN)
    assert L.hf_sample_paths_minlen(em._h, C.byref(p), ml, 0, 0, 1, None) == N.HF_E_ARG
    assert L.hf_sample_paths_minlen(em._h, C.byref(p), ml, 0, cap + 1, 1, None) == N.HF_E_ARG
    assert L.hf_sample_paths_minlen(em._h, C.byref(p), ml, -1, 3, 1, None) == N.HF_E_ARG
    assert L.hf_get_minlen_sample_labels(em._h, 0, lp) == N.HF_E_ARG                     # still no finished call
    assert L.hf_sample_paths_minlen(em._h, C.byref(p), ml, 0, 3, 1, None) == N.HF_OK
    assert L.hf_get_minlen_sample_labels(em._h, 0, lp) == N.HF_E_ARG                     # launched, not finished
    assert L.hf_sample_minlen_finish(em._h, None) == N.HF_OK
    assert L.hf_get_minlen_sample_labels(em._h, 2, lp) == N.HF_OK
    assert L.hf_get_minlen_sample_labels(em._h, 2, None) == N.HF_E_ARG
    assert L.hf_get_minlen_sample_labels(em._h, 3, lp) == N.HF_E_ARG
    assert L.hf_get_minlen_sample_labels(em._h, -1, lp) == N.HF_E_ARG
    good = em.sample_paths_minlen(model, (61, 1, 1, 1), 4, 1)                            # a sum of exactly 64 is served
    _admissible(good, store, (61, 1, 1, 1))
    R_ = model.numberOfRegions
    bad = model.copy()
    v = bad.param_vector().reshape(R_, -1)
    v[:, 20:24] = 0.0                                      # start row: no path has weight
    bad.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.sample_paths_minlen(bad, TRACK_LEN, 4, 1)
    assert ei.value.code == N.HF_E_SCALE
    assert L.hf_get_minlen_sample_labels(em._h, 0, lp) == N.HF_E_ARG                     # a failed call is no finished call
    nan = model.copy()
    v = nan.param_vector().reshape(R_, -1)
    v[:, 27 + 3 * 16] = np.nan                             # mean of Col, component 0
    nan.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.sample_paths_minlen(nan, TRACK_LEN, 4, 1)
    assert ei.value.code == N.HF_E_NAN
    assert L.hf_get_minlen_sample_labels(em._h, 0, lp) == N.HF_E_ARG
    assert np.array_equal(good, em.sample_paths_minlen(model, (61, 1, 1, 1), 4, 1))      # and the context samples correctly afterwards
    em.close()


# ---- command line ----------------------------------------------------------------------------------------------------------------

NEW_FILES = ["admissible_label_runs_support.bed", "admissible_samples_summary.tsv"]
UNCERTAINTY_FILES = ["final_label_runs_support.bed", "posterior_samples_summary.tsv"]


def test_cli_writes_the_two_files_and_changes_nothing_else(tmp_path):
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = hmm.getBestNumberOfCollapsedComps(store)
    args = ["-i", str(binp), "-W", "4000", "-n", "0", "-P", "-p", str(K), "--uncertaintySeed", "7"] + TML.MINLEN_ARGS      # 2, 3, 1, 2 windows
    TML._cli(args, tmp_path / "plain")
    TML._cli(args + ["--admissibleSamples", "16"], tmp_path / "adm")
    TML._cli(args + ["--uncertaintySamples", "16"], tmp_path / "unc")
    TML._cli(args + ["--ad", "16", "--uncertaintySamples", "16"], tmp_path / "both")
    plain, adm, unc, both = (tmp_path / d for d in ("plain", "adm", "unc", "both"))
    names = sorted(os.listdir(plain))
    assert sorted(set(os.listdir(adm)) - set(names)) == NEW_FILES
    assert sorted(set(os.listdir(both)) - set(names)) == sorted(NEW_FILES + UNCERTAINTY_FILES)
    for n in names:
        assert (plain / n).read_bytes() == (adm / n).read_bytes(), n
        assert (plain / n).read_bytes() == (both / n).read_bytes(), n
    for n in NEW_FILES:
        assert (adm / n).read_bytes() == (both / n).read_bytes(), n
    for n in UNCERTAINTY_FILES:
        assert (unc / n).read_bytes() == (both / n).read_bytes(), n
    assert (adm / NEW_FILES[0]).read_bytes() != (unc / UNCERTAINTY_FILES[0]).read_bytes()
    # the same samples from the library (-n 0: the final parameters are the initial model's), reduced here as the command line reduces them
    st = synth.WindowStore.read_bin(str(binp))
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, np.zeros((4, 4)))
    em = hmm.EMList(st, model)
    lab = em.sample_paths_minlen(model, (2, 3, 1, 2), 16, 7)
    em.close()
    _admissible(lab, st, (2, 3, 1, 2))
    off = np.asarray(st.chunk_off, np.int64)
    chunk = np.searchsorted(off, np.arange(st.n_windows), side="right") - 1
    i = np.arange(st.n_windows) - off[chunk]
    ws = st.chunk_s[chunk].astype(np.int64) + i * st.window_len
    we = np.minimum(ws + st.window_len - 1, st.chunk_e[chunk])
    bases = we - ws + 1
    reg = st.regions().astype(np.int64)
    names4 = ["Err", "Dup", "Hap", "Col"]
    # admissible_label_runs_support.bed: the runs are the final labels'; support and mean fraction from the samples
    runs = [l.split("\t") for l in (adm / NEW_FILES[0]).read_text().splitlines() if not l.startswith("#")]
    assert [r[:4] for r in runs] == [l.split("\t")[:4] for l in (unc / UNCERTAINTY_FILES[0]).read_text().splitlines() if not l.startswith("#")]
    ctg = np.array([st.chunk_ctg[c] for c in chunk])
    for r in runs:
        sel = (ctg == r[0]) & (ws >= int(r[1])) & (we + 1 <= int(r[2]))
        hit = lab[:, sel] == names4.index(r[3])
        assert r[4] == "%.4f" % (hit.all(axis=1).sum() / 16) and r[5] == "%.4f" % (hit.mean(axis=1).sum() / 16), r
    # admissible_samples_summary.tsv: per (region, label) the mean, SD and quantiles of the bases and the mean of the windows
    rows = [l.split("\t") for l in (adm / NEW_FILES[1]).read_text().splitlines() if not l.startswith("#")]
    assert len(rows) == 4 * (st.n_regions + 1)
    for row in rows:
        g = np.ones(st.n_windows, bool) if row[0] == "all" else reg == int(row[0].split("_")[1])
        l = [r[1] for r in rows[:4]].index(row[1])
        b = ((lab == l) & g[None, :]).astype(np.int64) @ bases
        srt = np.sort(b)
        assert row[3] == "%.4f" % b.mean() and row[4] == "%.4f" % b.std(ddof=1), row
        assert [int(x) for x in row[5:8]] == [int(srt[int(np.floor(q * 15))]) for q in (0.025, 0.5, 0.975)], row
        assert row[8] == "%.4f" % (((lab == l) & g[None, :]).sum() / 16), row
