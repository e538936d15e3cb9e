"""Most-probable-path decoding on the GPU (hf_viterbi, hf_multi_viterbi, hmm.EM_runViterbiForList, hmm_flagger --viterbi) against
mpmath path enumeration on tiny stores and the float64 numpy reference (tests/viterbi_ref.py) at full size."""
import ctypes as C
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_bruteforce_cpu import Params, _tiny_store
from test_viterbi_cpu import enumerate_map, perturbed_model
import viterbi_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]
TOL = 1e-9


def _check_against_reference(store, model, alpha, labels, chunk_ll, log_prob):
    ref_lab, ref_ll, plp = viterbi_ref.reference(store, model, alpha)
    got = plp(labels)
    scale = np.abs(ref_ll)
    assert np.all(np.abs(got - ref_ll) <= TOL * scale), np.max(np.abs(got - ref_ll) / scale)
    assert np.all(np.abs(chunk_ll - ref_ll) <= TOL * scale), np.max(np.abs(chunk_ll - ref_ll) / scale)
    if store.n_windows:
        assert np.mean(labels == ref_lab) >= 0.9999, np.mean(labels == ref_lab)
    assert log_prob == float(np.sum(chunk_ll)) or abs(log_prob - np.sum(chunk_ll)) <= 1e-12 * abs(log_prob)
    return ref_lab


def _trained(store, model_type, K, alpha, iters=2, algo=N.HF_ALGO_SCAN):
    model = hmm.createModel(model_type, K, store, alpha)
    em = hmm.EMList(store, model, algo=algo)
    for _ in range(iters):
        hmm.EM_runOneIterationForList(em, model)
        hmm.HMM_estimateParameters(model, 1e-3)
        hmm.HMM_resetEstimators(model)
    return em, model


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed,hifi", [(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 0, True), (N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 1, False),
                                                  (N.HF_MODEL_GAUSSIAN, 2, True), (N.HF_MODEL_NEGATIVE_BINOMIAL, 4, False)])
def test_tiny_stores_equal_path_enumeration(algo, model_type, seed, hifi):
    rng = np.random.default_rng(700 + seed)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    regions = [20, 31] if seed % 2 == 0 else [25]
    store = _tiny_store(rng, [7, 5, 1, 6, 3], regions)
    K = 2 + seed % 3
    model = perturbed_model(store, model_type, K, alpha, rng)
    em = hmm.EMList(store, model, algo=algo)
    labels, chunk_ll, lp = hmm.EM_runViterbiForList(em, model)
    P = Params(model.param_vector(), len(regions), K, model_type, alpha)
    nbE = None
    if model_type == N.HF_MODEL_NEGATIVE_BINOMIAL:
        p = model.params()
        nbE = np.ctypeslib.as_array(p.nb_E, shape=(len(regions) * 4 * viterbi_ref.NX,)).reshape(len(regions), 4, viterbi_ref.NX).copy()
    gaps = 0
    for c in range(store.n_chunks):
        path, lbest, l2 = enumerate_map(store, c, P, model, nbE)
        assert abs(chunk_ll[c] - float(lbest)) <= 1e-12 * abs(float(lbest)), (c, chunk_ll[c], lbest)
        if lbest - l2 > mp.mpf("1e-9") * abs(lbest):
            t0, t1 = int(store.chunk_off[c]), int(store.chunk_off[c + 1])
            assert tuple(int(v) for v in labels[t0:t1]) == path, (c, labels[t0:t1], path)
            gaps += 1
    assert gaps >= store.n_chunks - 1
    assert lp == float(np.sum(chunk_ll))
    em.close()


@pytest.mark.parametrize("cfg,model_type,hifi,scale", [(2, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, True, 1.0),
                                                       (4, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, True, 1.0),
                                                       (5, N.HF_MODEL_GAUSSIAN, True, 1.0),
                                                       (6, N.HF_MODEL_NEGATIVE_BINOMIAL, False, 0.5),
                                                       (7, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, False, 1.0)])
def test_full_size_against_numpy_reference(cfg, model_type, hifi, scale):
    store = synth.config(cfg, scale)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    em, model = _trained(store, model_type, K, alpha)
    labels, chunk_ll, lp = hmm.EM_runViterbiForList(em, model)
    _check_against_reference(store, model, alpha, labels, chunk_ll, lp)
    em.close()


SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 4097, 13_000]   # 13 000 windows: 26 segments, more than HF_SEG_PSTAGE


@pytest.mark.parametrize("env", [{}, {"HF_SEG_LAUNCHES": "2"}, {"HF_SUBPASSES": "3"}])
def test_segmentation_edge_cases(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    store = synth.synthesize([n * 1000 for n in SIZES], 1000, 10 ** 9, [20], seed=11)
    assert sorted(np.diff(store.chunk_off).tolist()) == sorted(SIZES)
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, iters=1)
    if "HF_SEG_LAUNCHES" in env:
        assert em.seg_launches == 2
    if "HF_SUBPASSES" in env:
        assert em.sub_passes == 3
    labels, chunk_ll, lp = hmm.EM_runViterbiForList(em, model)
    _check_against_reference(store, model, synth.HIFI_ALPHA, labels, chunk_ll, lp)
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunk_list(algo):
    full = synth.synthesize([50_000], 1000, 20_000, [20], seed=2)
    store = full.subset_chunks([])
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, full, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model, algo=algo)
    labels, chunk_ll, lp = hmm.EM_runViterbiForList(em, model)
    assert labels.size == 0 and chunk_ll.size == 0 and lp == 0.0
    em.close()


def test_scan_against_seq():
    store = synth.config(2, 0.1)
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, synth.HIFI_ALPHA)
    la, lla, lpa = hmm.EM_runViterbiForList(em, model)
    seq = hmm.EMList(store, model, algo=N.HF_ALGO_SEQ)
    lb, llb, lpb = hmm.EM_runViterbiForList(seq, model)
    assert np.all(np.abs(lla - llb) <= TOL * np.abs(lla))
    assert np.mean(la == lb) >= 0.9999
    _, _, plp = viterbi_ref.reference(store, model, synth.HIFI_ALPHA)
    pa, pb = plp(la), plp(lb)
    for c in np.flatnonzero([not np.array_equal(la[store.chunk_off[c]:store.chunk_off[c + 1]], lb[store.chunk_off[c]:store.chunk_off[c + 1]])
                             for c in range(store.n_chunks)]):
        assert abs(pa[c] - pb[c]) <= TOL * abs(pa[c]), (c, pa[c], pb[c])   # a rounding-level tie, shown by evaluation
    em.close(); seq.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_no_disturbance_of_the_last_pass(algo):
    store = synth.config(2, 0.05)
    alpha = synth.HIFI_ALPHA
    em_a, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, alpha, iters=1, algo=algo)
    em_b = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em_a, model)
    st_a = model.estimators.copy()
    hmm.EM_runOneIterationForList(em_b, model)
    st_b = model.estimators.copy()
    assert np.array_equal(st_a, st_b)
    other = model.copy()                                   # Viterbi with DIFFERENT parameters
    v = other.param_vector().reshape(other.numberOfRegions, -1)
    v[:, 27:27 + 4 * 16] *= 1.1
    other.set_param_vector(v.ravel())
    r1 = em_a.viterbi(other)
    r2 = em_a.viterbi(other)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and r1[2] == r2[2]   # two runs: identical bits
    assert np.array_equal(em_a.labels(), em_b.labels())
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    fa, fb = em_a.forward_backward(), em_b.forward_backward()
    for x, y in zip(fa, fb):
        assert np.array_equal(x, y)
    hmm.EM_runOneIterationForList(em_a, model); st2_a = model.estimators.copy()   # the next pass
    hmm.EM_runOneIterationForList(em_b, model); st2_b = model.estimators.copy()
    assert np.array_equal(st2_a, st2_b)
    assert np.array_equal(em_a.labels(), em_b.labels())
    em_a.close(); em_b.close()


def test_getters_before_any_run():
    store = synth.config(2, 0.02)
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, store, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model)
    L = N.lib()
    lab = np.empty(store.n_windows, np.int8)
    assert L.hf_get_viterbi_labels(em._h, lab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_E_ARG
    ll = np.empty(store.n_chunks)
    assert L.hf_get_viterbi_chunk_log_probs(em._h, ll.ctypes.data_as(C.POINTER(C.c_double))) == N.HF_E_ARG
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_multi_loopback_bit_identical(algo):
    store = synth.config(2, 0.1)
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, synth.HIFI_ALPHA, iters=1, algo=algo)
    lab1, ll1, lp1 = hmm.EM_runViterbiForList(em, model)
    em.close()
    for world in (1, 2, 3, 8):
        m = hmm.MultiEMList(store, model, world, algo=algo, transport=N.HF_TRANSPORT_LOOPBACK)
        lab, ll, lp = hmm.EM_runViterbiForList(m, model)
        assert np.array_equal(lab, lab1), world
        assert np.array_equal(ll, ll1) and lp == lp1, world
        m.close()


def test_errors():
    store = synth.config(2, 0.02)
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, store, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model)
    R = model.numberOfRegions
    bad = model.copy()
    v = bad.param_vector().reshape(R, -1)
    v[:, 20:24] = 0.0                                      # start row: no path has weight
    bad.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.viterbi(bad)
    assert ei.value.code == N.HF_E_SCALE
    nan = model.copy()
    v = nan.param_vector().reshape(R, -1)
    v[:, 27 + 3 * 16] = np.nan                             # mean of Col, component 0
    nan.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.viterbi(nan)
    assert ei.value.code == N.HF_E_NAN
    labels, _, _ = em.viterbi(model)                       # and the context still decodes afterwards
    assert labels.size == store.n_windows
    em.close()


# ---- command line --------------------------------------------------------------------------------------------------------------

def _cli(args, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


def _bed_from_labels(binp, labels, path, track="final_hmm_flagger"):
    L = N.lib()
    tab = L.hfio_load(str(binp).encode(), 0, 0)
    assert tab
    lens = (C.c_int32 * 3)(0, 0, 0)
    lab = np.ascontiguousarray(labels, np.int8)
    assert L.hfio_write_final_bed(tab, lab.ctypes.data_as(C.POINTER(C.c_int8)), str(path).encode(), track.encode(), lens) == 0
    L.hfio_destroy(tab)


def test_cli_fixed_parameter_decode(tmp_path):
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = hmm.getBestNumberOfCollapsedComps(store)
    _cli(["-i", str(binp), "-W", "4000", "-n", "0", "--viterbi", "-p", str(K)], tmp_path / "o")
    st = synth.WindowStore.read_bin(str(binp))
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, np.zeros((4, 4)))
    ref_lab, ref_ll, _ = viterbi_ref.reference(st, model, np.zeros((4, 4)))
    _bed_from_labels(binp, ref_lab, tmp_path / "ref.bed")
    assert (tmp_path / "o" / "final_flagger_prediction.bed").read_text() == (tmp_path / "ref.bed").read_text()
    lp = float((tmp_path / "o" / "viterbi_log_probability.tsv").read_text())
    assert abs(lp - ref_ll.sum()) <= 1e-6 + TOL * abs(lp)


def test_cli_viterbi_changes_only_the_final_labels(tmp_path):
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    args = ["-i", str(binp), "-W", "4000", "-n", "4", "-P", "--minimumLengths", "8000,12000,8000"]
    _cli(args, tmp_path / "post")
    _cli(args + ["--viterbi"], tmp_path / "vit")
    a, b = tmp_path / "post", tmp_path / "vit"
    names = sorted(os.listdir(a))
    assert sorted(set(os.listdir(b)) - set(names)) == ["viterbi_log_probability.tsv"]
    for n in names:
        if n == "final_flagger_prediction.bed" or n.startswith("prediction_summary_final"):
            continue
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    assert "posterior_prediction_final.bed" in names and "loglikelihood.tsv" in names


@pytest.mark.skipif(N.lib().hf_device_count() < 2, reason="needs two GPUs")
def test_cli_two_gpus(tmp_path):
    store = synth.config(1, 0.5)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    args = ["-i", str(binp), "-W", "4000", "-n", "3", "--viterbi"]
    _cli(args, tmp_path / "one")
    _cli(args + ["--gpus", "2"], tmp_path / "two")
    for n in ("final_flagger_prediction.bed", "viterbi_log_probability.tsv"):
        assert (tmp_path / "one" / n).read_bytes() == (tmp_path / "two" / n).read_bytes(), n
