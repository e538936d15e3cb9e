"""Minimum-run-length Viterbi on the GPU (hf_viterbi_minlen, hmm.EM_runMinLengthViterbiForList, hmm_flagger --enforceMinimumLengths)
against mpmath enumeration of the admissible paths on tiny stores and the float64 numpy reference (tests/minlen_ref.py) elsewhere.
"Optimal" is shown by evaluation: the returned labels are admissible (an exact integer check), and their path_log_prob and the
reported chunk score are within TOL of the reference optimum."""
import ctypes as C
import functools
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from hip_streams import Streams
from test_bruteforce_cpu import _tiny_store
from test_viterbi_cpu import perturbed_model
import minlen_ref
import viterbi_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]
TOL = 1e-9
ONES = (1, 1, 1, 1)
TRACK_LEN = (3, 5, 1, 7)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _check(store, ref, min_len, got):
    """Admissible, and optimal by evaluation.  Returns the number of chunks in which the constraint bites (reference)."""
    labels, chunk_ll, lp = got
    ref_lab, ref_ll, plp, free = ref
    off = store.chunk_off
    assert minlen_ref.admissible(labels, off, min_len).all()
    assert minlen_ref.admissible(ref_lab, off, min_len).all()
    scale = np.abs(ref_ll)
    val = plp(labels)
    assert np.all(np.abs(val - ref_ll) <= TOL * scale), np.max(np.abs(val - ref_ll) / scale)
    assert np.all(np.abs(chunk_ll - ref_ll) <= TOL * scale), np.max(np.abs(chunk_ll - ref_ll) / scale)
    assert lp == float(np.sum(chunk_ll)) or abs(lp - np.sum(chunk_ll)) <= 1e-12 * abs(lp)
    return int(np.sum(~minlen_ref.admissible(free, off, min_len)))


# ---- tiny stores against enumeration ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed,hifi", minlen_ref.TINY_CASES)
def test_tiny_stores_equal_path_enumeration(algo, model_type, seed, hifi):
    store, model, alpha, enum = minlen_ref.tiny_case(model_type, seed, hifi)
    off = store.chunk_off
    em = hmm.EMList(store, model, algo=algo)
    for min_len in minlen_ref.TINY_MIN_LENS:
        labels, chunk_ll, lp = hmm.EM_runMinLengthViterbiForList(em, model, min_len)
        assert minlen_ref.admissible(labels, off, min_len).all()
        gaps = 0
        for c in range(store.n_chunks):
            path, lbest, l2 = enum[min_len][c]
            assert abs(chunk_ll[c] - float(lbest)) <= 1e-12 * abs(float(lbest)), (min_len, c, chunk_ll[c], lbest)
            if lbest - l2 > mp.mpf("1e-9") * abs(lbest):
                assert tuple(int(v) for v in labels[off[c]:off[c + 1]]) == path, (min_len, c, labels[off[c]:off[c + 1]], path)
                gaps += 1
        assert gaps >= store.n_chunks - 1
        assert lp == float(np.sum(chunk_ll)) or abs(lp - np.sum(chunk_ll)) <= 1e-12 * abs(lp)
    em.close()


# ---- lane and block geometry -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _geometry():
    rng = np.random.default_rng(5)
    store = _tiny_store(rng, [63, 64, 65, 129, 15, 16, 17, 31, 32, 33], [20, 31])
    model = perturbed_model(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, rng)
    return store, model


@pytest.mark.parametrize("min_len", [(3, 5, 1, 7), (16, 16, 16, 16), (61, 1, 1, 1)])
def test_lane_and_block_geometry(min_len):
    """Chunks around the 64-window staging block and around a minimum length of 16; 64 lanes, one state owning 61 of them."""
    store, model = _geometry()
    ref = minlen_ref.reference(store, model, synth.HIFI_ALPHA, min_len)
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        res.append(hmm.EM_runMinLengthViterbiForList(em, model, min_len))
        em.close()
    bites = _check(store, ref, min_len, res[0])
    assert bites >= store.n_chunks // 2, bites
    assert _same(res[0], res[1])


# ---- a realistic track -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _track():
    store = synth.config(2, 0.02)
    model = hmm.createModel(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, store, synth.HIFI_ALPHA)      # untrained
    logA, logend = viterbi_ref.tables(store, model, synth.HIFI_ALPHA)
    plp = lambda lab: viterbi_ref.path_log_prob(logA, logend, store.chunk_off, lab)
    free, free_ll = viterbi_ref.viterbi(logA, logend, store.chunk_off)
    refs = {ml: minlen_ref.viterbi_minlen(logA, logend, store.chunk_off, ml) + (plp, free) for ml in (TRACK_LEN, ONES)}
    return store, model, refs, free_ll


def test_realistic_track():
    store, model, refs, free_ll = _track()
    em = hmm.EMList(store, model)
    a = hmm.EM_runMinLengthViterbiForList(em, model, TRACK_LEN)
    bites = _check(store, refs[TRACK_LEN], TRACK_LEN, a)
    assert bites >= 1
    assert np.all(a[1] <= free_ll + TOL * np.abs(free_ll)) and a[2] < float(np.sum(free_ll))     # the constraint costs something
    b = hmm.EM_runMinLengthViterbiForList(em, model, TRACK_LEN)                                 # a second call: identical bits
    assert _same(a, b)
    seq = hmm.EMList(store, model, algo=N.HF_ALGO_SEQ)                                          # the other kind of context: identical bits
    assert _same(a, hmm.EM_runMinLengthViterbiForList(seq, model, TRACK_LEN))
    em.close(); seq.close()


def test_all_ones_against_hf_viterbi():
    store, model, refs, _ = _track()
    off = store.chunk_off
    em = hmm.EMList(store, model)
    la, lla, lpa = hmm.EM_runMinLengthViterbiForList(em, model, ONES)
    lb, llb, lpb = hmm.EM_runViterbiForList(em, model)
    _check(store, refs[ONES], ONES, (la, lla, lpa))
    assert np.all(np.abs(lla - llb) <= TOL * np.abs(llb))
    plp = refs[ONES][2]
    pa, pb = plp(la), plp(lb)
    for c in range(store.n_chunks):
        if not np.array_equal(la[off[c]:off[c + 1]], lb[off[c]:off[c + 1]]):
            assert abs(pa[c] - pb[c]) <= TOL * abs(pa[c]), (c, pa[c], pb[c])   # a rounding-level tie, shown by evaluation
    em.close()


# ---- no disturbance --------------------------------------------------------------------------------------------------------------

def _viterbi_results(em):
    L = N.lib()
    lab = np.empty(em.store.n_windows, np.int8)
    ll = np.empty(em.store.n_chunks)
    assert L.hf_get_viterbi_labels(em._h, lab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
    assert L.hf_get_viterbi_chunk_log_probs(em._h, ll.ctypes.data_as(C.POINTER(C.c_double))) == N.HF_OK
    return lab, ll


def _sample_results(em, n):
    L = N.lib()
    out = np.empty((n, em.store.n_windows), np.int8)
    for k in range(n):
        assert L.hf_get_sample_labels(em._h, k, out[k].ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
    return out


@pytest.mark.parametrize("algo", ALGOS)
def test_no_disturbance_of_the_last_pass_and_the_other_decoders(algo):
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
    smp = em_a.sample_paths(model, 2, 7)
    other = model.copy()                                   # the constrained decoder runs with DIFFERENT parameters
    v = other.param_vector().reshape(other.numberOfRegions, -1)
    v[:, 27:27 + 4 * 16] *= 1.1
    other.set_param_vector(v.ravel())
    r1 = em_a.viterbi_minlen(other, TRACK_LEN)
    r2 = em_a.viterbi_minlen(other, TRACK_LEN)
    assert _same(r1, r2)
    assert not np.array_equal(r1[0], vit[0])
    assert np.array_equal(em_a.labels(), em_b.labels())
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    for x, y in zip(em_a.forward_backward(), em_b.forward_backward()):
        assert np.array_equal(x, y)
    lab, ll = _viterbi_results(em_a)                       # hf_viterbi's last results and the sampler's
    assert np.array_equal(lab, vit[0]) and np.array_equal(ll, vit[1])
    assert np.array_equal(_sample_results(em_a, 2), smp)
    hmm.EM_runOneIterationForList(em_a, model); st2_a = model.estimators.copy(); hmm.HMM_resetEstimators(model)   # the next pass
    hmm.EM_runOneIterationForList(em_b, model); st2_b = model.estimators.copy()
    assert np.array_equal(st2_a, st2_b)
    assert np.array_equal(em_a.labels(), em_b.labels())
    em_a.close(); em_b.close()


# ---- edges and errors ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunk_list(algo):
    full = synth.synthesize([50_000], 1000, 20_000, [20], seed=2)
    store = full.subset_chunks([])
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, full, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model, algo=algo)
    labels, chunk_ll, lp = hmm.EM_runMinLengthViterbiForList(em, model, TRACK_LEN)
    assert labels.size == 0 and chunk_ll.size == 0 and lp == 0.0
    em.close()


def test_arguments_getters_and_errors():
    store = synth.config(2, 0.02)
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, store, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model)
    L = N.lib()
    assert N.HF_MINLEN_MAX_LANES == 64
    lab = np.empty(store.n_windows, np.int8)
    ll = np.empty(store.n_chunks)
    # getters before any run
    assert L.hf_get_viterbi_minlen_labels(em._h, lab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_E_ARG
    assert L.hf_get_viterbi_minlen_chunk_log_probs(em._h, ll.ctypes.data_as(C.POINTER(C.c_double))) == N.HF_E_ARG
    assert L.hf_viterbi_minlen_finish(em._h, None, None) == N.HF_E_ARG
    p = model.params()
    assert L.hf_viterbi_minlen(em._h, C.byref(p), None, None) == N.HF_E_ARG
    assert L.hf_viterbi_minlen(em._h, None, (C.c_int32 * 4)(1, 1, 1, 1), None) == N.HF_E_ARG
    for bad_len in ((3, 0, 1, 1), (-1, 1, 1, 1), (62, 1, 1, 1), (2 ** 31 - 1, 2 ** 31 - 1, 1, 1)):
        with pytest.raises(N.HFError) as ei:
            em.viterbi_minlen(model, bad_len)
        assert ei.value.code == N.HF_E_ARG, bad_len
    assert L.hf_get_viterbi_minlen_labels(em._h, lab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_E_ARG      # still no finished run
    with pytest.raises(TypeError):
        hmm.EM_runMinLengthViterbiForList(object(), model, ONES)
    good = em.viterbi_minlen(model, (61, 1, 1, 1))          # a sum of exactly 64 is served
    assert minlen_ref.admissible(good[0], store.chunk_off, (61, 1, 1, 1)).all()
    R = model.numberOfRegions
    bad = model.copy()
    v = bad.param_vector().reshape(R, -1)
    v[:, 20:24] = 0.0                                      # start row: no path has weight
    bad.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.viterbi_minlen(bad, TRACK_LEN)
    assert ei.value.code == N.HF_E_SCALE
    nan = model.copy()
    v = nan.param_vector().reshape(R, -1)
    v[:, 27 + 3 * 16] = np.nan                             # mean of Col, component 0
    nan.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.viterbi_minlen(nan, TRACK_LEN)
    assert ei.value.code == N.HF_E_NAN
    assert L.hf_get_viterbi_minlen_labels(em._h, lab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_E_ARG      # a failed run is no finished run
    again = em.viterbi_minlen(model, (61, 1, 1, 1))         # and the context decodes correctly afterwards
    assert _same(good, again)
    em.close()


# ---- a caller's stream -----------------------------------------------------------------------------------------------------------

def test_callers_stream():
    store, model, refs, _ = _track()
    em0 = hmm.EMList(store, model)
    want = em0.viterbi_minlen(model, TRACK_LEN)
    em0.close()
    with Streams() as streams:
        s = streams.new(non_blocking=True)
        em = hmm.EMList(store, model, stream=s)
        streams.h.delay(s)                                 # whatever ran on the null stream instead would run ahead of this
        got = em.viterbi_minlen(model, TRACK_LEN)
        assert _same(want, got)
        em.close()


# ---- command line ----------------------------------------------------------------------------------------------------------------

def _cli(args, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


def _bed_from_labels(binp, labels, path, lens, track="final_hmm_flagger"):
    L = N.lib()
    tab = L.hfio_load(str(binp).encode(), 0, 0)
    assert tab
    lens = (C.c_int32 * 4)(*lens)
    lab = np.ascontiguousarray(labels, np.int8)
    assert L.hfio_write_final_bed(tab, lab.ctypes.data_as(C.POINTER(C.c_int8)), str(path).encode(), track.encode(), lens) == 0
    L.hfio_destroy(tab)


MINLEN_ARGS = ["--minimumLengths", "8000,12000,8000"]      # with -W 4000: 2, 3, 1, 2 windows


def test_cli_fixed_parameter_decode(tmp_path):
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = hmm.getBestNumberOfCollapsedComps(store)
    _cli(["-i", str(binp), "-W", "4000", "-n", "0", "--viterbi", "--enforceMinimumLengths", "-p", str(K)] + MINLEN_ARGS, tmp_path / "o")
    st = synth.WindowStore.read_bin(str(binp))
    assert st.window_len == 4000
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, np.zeros((4, 4)))
    w = (2, 3, 1, 2)
    ref_lab, ref_ll, _, free = minlen_ref.reference(st, model, np.zeros((4, 4)), w)
    logA, logend = viterbi_ref.tables(st, model, np.zeros((4, 4)))
    free_ll = viterbi_ref.viterbi(logA, logend, st.chunk_off)[1]
    _bed_from_labels(binp, ref_lab, tmp_path / "ref.bed", (8000, 12000, 0, 8000))
    assert (tmp_path / "o" / "final_flagger_prediction.bed").read_text() == (tmp_path / "ref.bed").read_text()
    lp = float((tmp_path / "o" / "viterbi_log_probability.tsv").read_text())
    assert abs(lp - ref_ll.sum()) <= 1e-6 + TOL * abs(lp)
    rows = (tmp_path / "o" / "viterbi_min_length_cost.tsv").read_text().splitlines()
    assert len(rows) == 2 and rows[0].startswith("#") and len(rows[0].split("\t")) == 8
    f = rows[1].split("\t")
    assert [int(x) for x in f[:4]] == list(w)
    con, unc, dif = float(f[4]), float(f[5]), float(f[6])
    assert abs(con - ref_ll.sum()) <= 1e-6 + TOL * abs(con)
    assert abs(unc - free_ll.sum()) <= 1e-6 + TOL * abs(unc)
    assert abs(dif - (con - unc)) <= 2e-6 and dif <= 0.0
    assert con == lp
    off = st.chunk_off
    differ = sum(not np.array_equal(ref_lab[off[c]:off[c + 1]], free[off[c]:off[c + 1]]) for c in range(st.n_chunks))
    assert int(f[7]) == differ


def test_cli_option_changes_only_the_final_labels(tmp_path):
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    args = ["-i", str(binp), "-W", "4000", "-n", "4", "-P", "--viterbi"] + MINLEN_ARGS
    _cli(args, tmp_path / "vit")
    _cli(args + ["--enforceMinimumLengths"], tmp_path / "con")
    a, b = tmp_path / "vit", tmp_path / "con"
    names = sorted(os.listdir(a))
    assert sorted(set(os.listdir(b)) - set(names)) == ["viterbi_min_length_cost.tsv"]
    for n in names:
        if n == "final_flagger_prediction.bed" or n.startswith("prediction_summary_final") or n == "viterbi_log_probability.tsv":
            continue
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    assert "posterior_prediction_final.bed" in names and "loglikelihood.tsv" in names and "viterbi_log_probability.tsv" in names
    f = (b / "viterbi_min_length_cost.tsv").read_text().splitlines()[1].split("\t")
    assert float(f[5]) == float((a / "viterbi_log_probability.tsv").read_text())          # the unconstrained run is the other run's
    assert float(f[4]) == float((b / "viterbi_log_probability.tsv").read_text()) and float(f[4]) <= float(f[5])
