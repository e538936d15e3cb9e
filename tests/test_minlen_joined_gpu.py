"""Minimum-run-length Viterbi over whole contigs on the GPU (hf_viterbi_minlen_joined, EMList.viterbi_minlen(joined=...),
hmm_flagger --wholeContigs) against 50-digit enumeration of the admissible group paths on tiny stores and the float64 numpy reference
(tests/minlen_joined_ref.py) elsewhere.  The tolerances are the family's (test_minlen_gpu.py): scores within 1e-9 relative of the
reference; labels accepted when they are admissible over the groups and their evaluated log-probability equals the reference score
within 1e-9 relative; enumeration within 1e-12 relative.

The realistic track is configs[2] at scale 0.02 with the chunk length scaled like the contigs (400 kb): 286 chunks in 46 contigs, 30 568
windows.  synth.config(2, 0.02) itself keeps the 20 Mb chunk length, so each of its contigs is one chunk and no chunk is joined; it
serves the exact cases."""
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
import geometry_cases as G
import minlen_joined_ref as JR
import minlen_ref
import test_minlen_gpu as TML
import test_minlen_joined_cpu as TJC
import viterbi_ref

pytestmark = pytest.mark.gpu
ALGOS = TML.ALGOS
TOL = TML.TOL
ONES = TML.ONES
TRACK_LEN = TML.TRACK_LEN
_same = TML._same


def _check(off, tables, joined, min_len, got):
    """Admissible over the groups, optimal by evaluation, chunk entries in the getter's convention.  Returns the reference."""
    labels, chunk_ll, lp = got
    logA, logend = tables
    n = int(np.asarray(off)[-1])
    ref_lab, ref_ll, goff = JR.viterbi_minlen_joined(logA, logend, off, joined, min_len)
    assert minlen_ref.admissible(labels[:n], goff, min_len).all()
    assert minlen_ref.admissible(ref_lab, goff, min_len).all()
    scale = np.abs(ref_ll)
    val = JR.group_sums(viterbi_ref.path_log_prob(logA, logend, off, labels[:n]), off, joined)
    print("min_len %s: largest deviation of the evaluated labels %.3e, of the chunk entries %.3e (relative, over the groups)"
          % (min_len, np.max(np.abs(val - ref_ll)[scale > 0] / scale[scale > 0]), np.max(np.abs(chunk_ll - ref_ll)[scale > 0] / scale[scale > 0])))
    assert np.all(np.abs(val - ref_ll) <= TOL * scale)
    assert np.all(np.abs(chunk_ll - ref_ll) <= TOL * scale)
    assert np.all(chunk_ll[ref_ll == 0.0] == 0.0)            # exactly 0.0 in the entries of a group's other chunks
    assert lp == float(np.sum(chunk_ll)) or abs(lp - np.sum(chunk_ll)) <= 1e-12 * abs(lp)
    return ref_lab, ref_ll, goff


# ---- 4. tiny stores against enumeration ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("case", minlen_ref.TINY_CASES)
def test_tiny_stores_equal_group_enumeration(algo, case):
    store, model, alpha, _ = minlen_ref.tiny_case(*case)
    em = hmm.EMList(store, model, algo=algo)

    def decode(joined, ml):
        labels, chunk_ll, lp = hmm.EM_runMinLengthViterbiForList(em, model, ml, joined)
        goff = JR.group_offsets(store.chunk_off, joined)[0]
        assert minlen_ref.admissible(labels, goff, ml).all()
        assert lp == float(np.sum(chunk_ll)) or abs(lp - np.sum(chunk_ll)) <= 1e-12 * abs(lp)
        return labels, chunk_ll

    checked, _ = TJC._check_case_against_enumeration(case, decode)
    assert checked >= 6
    em.close()


# ---- 5. geometry: joined boundaries around the staging block and inside a backpointer block -----------------------------------------

GEOMETRY_LENGTHS = [63, 64, 65, 129, 15, 16, 17, 31, 32, 33]
GEOMETRY_JOINED = [0, 1, 1, 1, 0, 1, 1, 1, 1, 1]
GEOMETRY_SEED = 7        # chosen on the CPU: the per-chunk reference breaks the whole-group rule in both groups for all three length sets


@functools.lru_cache(maxsize=None)
def _geometry():
    rng = np.random.default_rng(GEOMETRY_SEED)
    store = _tiny_store(rng, GEOMETRY_LENGTHS, [20, 31])
    model = perturbed_model(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, rng)
    return store, model, viterbi_ref.tables(store, model, synth.HIFI_ALPHA)


@pytest.mark.parametrize("min_len", [(3, 5, 1, 7), (16, 16, 16, 16), (61, 1, 1, 1)])
def test_joined_boundaries_around_the_blocks(min_len):
    """Group 0: boundaries at windows 63, 127 and 192 (one before, on and one after a multiple of 64); group 1: at 15, 31, 48, 79 and
    111 of the group, on and inside the 16-window backpointer blocks."""
    store, model, tables = _geometry()
    off = store.chunk_off
    goff = JR.group_offsets(off, GEOMETRY_JOINED)[0]
    assert goff.tolist() == [0, 321, 465]
    per_chunk = minlen_ref.viterbi_minlen(tables[0], tables[1], off, min_len)[0]
    if min_len == (3, 5, 1, 7):
        assert (~minlen_ref.admissible(per_chunk, goff, min_len)).sum() >= 1, "the test could not tell the two decoders apart"
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        res.append(em.viterbi_minlen(model, min_len, GEOMETRY_JOINED))
        res.append(em.viterbi_minlen(model, min_len, GEOMETRY_JOINED))      # a second call
        em.close()
    _check(off, tables, GEOMETRY_JOINED, min_len, res[0])
    assert all(_same(res[0], r) for r in res[1:])


# ---- 6. the realistic track ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _track():
    store = synth.synthesize(synth.human_diploid_lengths(0.02), 4000, 400_000, [20], 1234 + 2, contig_prefix="hap_ctg")
    assert store.n_windows == 30568 and store.n_chunks == 286
    model = hmm.createModel(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, store, synth.HIFI_ALPHA)      # untrained
    return store, model, viterbi_ref.tables(store, model, synth.HIFI_ALPHA), hmm.joined_chunks(store)


def test_realistic_track():
    store, model, tables, joined = _track()
    off = store.chunk_off
    goff = JR.group_offsets(off, joined)[0]
    assert goff.size - 1 == 46 and joined.sum() == 240
    pc_lab, pc_ll = minlen_ref.viterbi_minlen(tables[0], tables[1], off, TRACK_LEN)
    assert not minlen_ref.admissible(pc_lab, goff, TRACK_LEN).all()        # the reference first: the per-chunk rule leaves short runs
    em = hmm.EMList(store, model)
    per_chunk = em.viterbi_minlen(model, TRACK_LEN)
    assert not minlen_ref.admissible(per_chunk[0], goff, TRACK_LEN).all()
    got = em.viterbi_minlen(model, TRACK_LEN, joined)
    _check(off, tables, joined, TRACK_LEN, got)
    bound = JR.group_sums(per_chunk[1], off, joined)
    assert np.all(got[1] <= bound + TOL * np.abs(bound)) and got[2] < per_chunk[2]
    print("whole-contig rule: %.6f nats below the per-chunk rule, %d short runs in the per-chunk labels"
          % (per_chunk[2] - got[2], len(JR.short_inner_runs(per_chunk[0], goff, TRACK_LEN))))
    em.close()


# ---- 7. exact cases ----------------------------------------------------------------------------------------------------------------------

def _raw(em, model, min_len, joined_ptr):
    """hf_viterbi_minlen_joined by hand (joined_ptr may be None: NULL), then what EMList.viterbi_minlen returns."""
    L = N.lib()
    p = model.params()
    lp = C.c_double(0.0)
    N.check(L.hf_viterbi_minlen_joined(em._h, C.byref(p), (C.c_int32 * 4)(*min_len), joined_ptr, em.stream), "hf_viterbi_minlen_joined")
    N.check(L.hf_viterbi_minlen_finish(em._h, C.byref(lp), em.stream), "hf_viterbi_minlen_finish")
    lab = np.empty(em.store.n_windows, np.int8)
    ll = np.empty(em.store.n_chunks)
    N.check(L.hf_get_viterbi_minlen_labels(em._h, lab.ctypes.data_as(C.POINTER(C.c_int8))), "labels")
    N.check(L.hf_get_viterbi_minlen_chunk_log_probs(em._h, ll.ctypes.data_as(C.POINTER(C.c_double))), "chunk values")
    return lab, ll, float(lp.value)


@pytest.mark.parametrize("algo", ALGOS)
def test_no_join_is_hf_viterbi_minlen_bit_for_bit(algo):
    for store, model in (TML._track()[:2], _track()[:2], _geometry()[:2]):
        em = hmm.EMList(store, model, algo=algo)
        for ml in (TRACK_LEN, (16, 16, 16, 16)):
            want = em.viterbi_minlen(model, ml)
            assert _same(want, em.viterbi_minlen(model, ml, None))
            assert _same(want, em.viterbi_minlen(model, ml, np.zeros(store.n_chunks, bool)))
            assert _same(want, _raw(em, model, ml, None))
        em.close()


def test_all_ones_gives_hf_viterbi_whatever_joined_says():
    store, model, tables, joined = _track()
    off = store.chunk_off
    em = hmm.EMList(store, model)
    lb, llb, lpb = em.viterbi(model)
    pb = viterbi_ref.path_log_prob(tables[0], tables[1], off, lb)
    for jn in (joined, np.zeros(store.n_chunks, bool)):
        la, lla, lpa = em.viterbi_minlen(model, ONES, jn)
        pa = viterbi_ref.path_log_prob(tables[0], tables[1], off, la)
        for c in range(store.n_chunks):
            if not np.array_equal(la[off[c]:off[c + 1]], lb[off[c]:off[c + 1]]):
                assert abs(pa[c] - pb[c]) <= TOL * abs(pa[c]), (c, pa[c], pb[c])   # a rounding-level tie, shown by evaluation
        assert abs(lpa - lpb) <= TOL * abs(lpb)
        want = JR.group_sums(llb, off, jn)
        assert np.all(np.abs(lla - want) <= TOL * np.abs(want))
    em.close()


# ---- 8. the geometry cases -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model_type,seed", G.CASES)
def test_empty_chunks_and_uncovered_windows(model_type, seed):
    store, model, alpha, _ = G.case(model_type, seed)
    tables = viterbi_ref.tables(store, model, alpha)
    off = np.asarray(G.OFF)
    est, src = G.with_empty_chunks(store)
    dev_j, ref_j = G.empty_chunk_joins(src, G.joins())
    ust = G.with_uncovered_windows(store, np.random.default_rng(3))
    a, b = G.FRONT, G.FRONT + store.n_windows
    for ml in ((3, 5, 1, 7), (16, 16, 16, 16)):
        for algo in ALGOS:
            # a chunk without windows ends the group, whatever its own and its successor's entries say
            em = hmm.EMList(est, model, algo=algo)
            lab, cll, lp = em.viterbi_minlen(model, ml, dev_j)
            em.close()
            assert np.all(cll[src < 0] == 0.0)
            _check(off, tables, ref_j, ml, (lab, cll[src >= 0], lp))
            # windows outside every chunk get -1, the rest is the grid store's
            em0 = hmm.EMList(store, model, algo=algo)
            want = em0.viterbi_minlen(model, ml, G.joins())
            em0.close()
            _check(off, tables, G.joins(), ml, want)
            em = hmm.EMList(ust, model, algo=algo)
            lab, cll, lp = em.viterbi_minlen(model, ml, G.joins())
            em.close()
            assert np.all(lab[:a] == -1) and np.all(lab[b:] == -1)
            assert np.array_equal(lab[a:b], want[0]) and np.array_equal(cll, want[1]) and lp == want[2]


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunk_list(algo):
    full = synth.synthesize([50_000], 1000, 20_000, [20], seed=2)
    store = full.subset_chunks([])
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, full, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model, algo=algo)
    for jn in (np.zeros(0, bool), None):
        labels, chunk_ll, lp = _raw(em, model, TRACK_LEN, None) if jn is None else em.viterbi_minlen(model, TRACK_LEN, jn)
        assert labels.size == 0 and chunk_ll.size == 0 and lp == 0.0
    em.close()


# ---- 9. no disturbance, streams, errors ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
def test_no_disturbance_of_the_last_pass_and_the_other_decoders(algo):
    store = synth.synthesize(synth.human_diploid_lengths(0.005), 4000, 100_000, [20], 1236, contig_prefix="hap_ctg")
    joined = hmm.joined_chunks(store)
    assert joined.sum() >= 40
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
    adm = em_a.sample_paths_minlen(model, TRACK_LEN, 2, 11)
    post = em_a.minlen_posterior(model, TRACK_LEN)
    post_values = post.posterior(0, store.n_windows).copy()
    other = model.copy()                                   # the joined decoder runs with DIFFERENT parameters
    v = other.param_vector().reshape(other.numberOfRegions, -1)
    v[:, 27:27 + 4 * 16] *= 1.1
    other.set_param_vector(v.ravel())
    r1 = em_a.viterbi_minlen(other, TRACK_LEN, joined)
    r2 = em_a.viterbi_minlen(other, TRACK_LEN, joined)
    assert _same(r1, r2)
    assert not np.array_equal(r1[0], vit[0])
    assert np.array_equal(em_a.labels(), em_b.labels())
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    for x, y in zip(em_a.forward_backward(), em_b.forward_backward()):
        assert np.array_equal(x, y)
    lab, ll = TML._viterbi_results(em_a)                   # hf_viterbi's last results, both samplers', the constrained posterior's
    assert np.array_equal(lab, vit[0]) and np.array_equal(ll, vit[1])
    assert np.array_equal(TML._sample_results(em_a, 2), smp)
    L = N.lib()
    for k in range(2):
        out = np.empty(store.n_windows, np.int8)
        assert L.hf_get_minlen_sample_labels(em_a._h, k, out.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
        assert np.array_equal(out, adm[k])
    assert np.array_equal(post.posterior(0, store.n_windows), post_values)
    hmm.EM_runOneIterationForList(em_a, model); st2_a = model.estimators.copy(); hmm.HMM_resetEstimators(model)   # the next pass
    hmm.EM_runOneIterationForList(em_b, model); st2_b = model.estimators.copy()
    assert np.array_equal(st2_a, st2_b)
    assert np.array_equal(em_a.labels(), em_b.labels())
    em_a.close(); em_b.close()


def test_callers_stream():
    store, model, _, joined = _track()
    em0 = hmm.EMList(store, model)
    want = em0.viterbi_minlen(model, TRACK_LEN, joined)
    em0.close()
    with Streams() as streams:
        s = streams.new(non_blocking=True)
        em = hmm.EMList(store, model, stream=s)
        streams.h.delay(s)                                 # whatever ran on the null stream instead would run ahead of this
        got = em.viterbi_minlen(model, TRACK_LEN, joined)
        assert _same(want, got)
        em.close()


def test_arguments_and_errors():
    store, model, tables, joined = _track()
    em = hmm.EMList(store, model)
    L = N.lib()
    p = model.params()
    four = (C.c_int32 * 4)(*TRACK_LEN)
    jn = np.ascontiguousarray(joined, np.uint8)
    jp = jn.ctypes.data_as(C.POINTER(C.c_uint8))
    lab = np.empty(store.n_windows, np.int8)
    assert L.hf_viterbi_minlen_joined(None, C.byref(p), four, jp, None) == N.HF_E_ARG
    assert L.hf_viterbi_minlen_joined(em._h, None, four, jp, None) == N.HF_E_ARG
    assert L.hf_viterbi_minlen_joined(em._h, C.byref(p), None, jp, None) == N.HF_E_ARG
    bad0 = jn.copy()
    bad0[0] = 1
    assert L.hf_viterbi_minlen_joined(em._h, C.byref(p), four, bad0.ctypes.data_as(C.POINTER(C.c_uint8)), None) == N.HF_E_ARG
    assert b"joined[0]" in L.hf_last_error()
    with pytest.raises(N.HFError) as ei:
        em.viterbi_minlen(model, TRACK_LEN, bad0)
    assert ei.value.code == N.HF_E_ARG
    for bad_len in ((3, 0, 1, 1), (62, 1, 1, 1)):          # a length 0, a sum of 65
        with pytest.raises(N.HFError) as ei:
            em.viterbi_minlen(model, bad_len, joined)
        assert ei.value.code == N.HF_E_ARG, bad_len
    assert L.hf_get_viterbi_minlen_labels(em._h, lab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_E_ARG      # no finished run yet
    for wrong in (joined[:-1], np.concatenate([joined, [False]])):
        with pytest.raises(ValueError):
            em.viterbi_minlen(model, TRACK_LEN, wrong)
        with pytest.raises(ValueError):
            hmm.EM_runMinLengthViterbiForList(em, model, TRACK_LEN, wrong)
    good = em.viterbi_minlen(model, (61, 1, 1, 1), joined)     # a sum of exactly 64 is served
    R = model.numberOfRegions
    bad = model.copy()
    v = bad.param_vector().reshape(R, -1)
    v[:, 20:24] = 0.0                                      # start row: no path of any group has weight
    bad.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.viterbi_minlen(bad, TRACK_LEN, joined)
    assert ei.value.code == N.HF_E_SCALE
    assert L.hf_get_viterbi_minlen_labels(em._h, lab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_E_ARG      # a failed run is no finished run
    assert _same(good, em.viterbi_minlen(model, (61, 1, 1, 1), joined))
    em.close()


def test_a_group_without_admissible_weight_is_a_scale_error():
    """Every chunk starts in Dup (start row) and ends in Hap (end column).  Per chunk the Hap run is at the chunk's end and exempt; over
    the group of both chunks the Hap run that ends chunk 0 lies inside (Dup follows at once) and cannot have 61 windows: no admissible
    path of the group has weight, while every chunk alone has."""
    rng = np.random.default_rng(17)
    store = _tiny_store(rng, [6, 5], [25])
    model = perturbed_model(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 2, np.zeros((4, 4)), rng)
    v = model.param_vector().reshape(1, -1)
    v[0, 20:24] = [0.0, 1.0, 0.0, 0.0]                      # start row: Dup
    v[0, [4, 9, 14, 19]] = [0.0, 0.0, 1e-3, 0.0]            # end column: Hap
    model.set_param_vector(v.ravel())
    logA, logend = viterbi_ref.tables(store, model, np.zeros((4, 4)))
    m = (1, 1, 61, 1)
    assert np.all(np.isfinite(minlen_ref.viterbi_minlen(logA, logend, store.chunk_off, m)[1]))
    assert JR.viterbi_minlen_joined(logA, logend, store.chunk_off, [0, 1], m)[1][0] == -np.inf
    assert np.isfinite(JR.viterbi_minlen_joined(logA, logend, store.chunk_off, [0, 1], (1, 1, 3, 1))[1][0])
    em = hmm.EMList(store, model)
    assert np.isfinite(em.viterbi_minlen(model, m, [0, 0])[2])
    _check(store.chunk_off, (logA, logend), [0, 1], (1, 1, 3, 1), em.viterbi_minlen(model, (1, 1, 3, 1), [0, 1]))
    with pytest.raises(N.HFError) as ei:
        em.viterbi_minlen(model, m, [0, 1])
    assert ei.value.code == N.HF_E_SCALE
    em.close()


def test_nan_in_an_end_column_that_only_a_joined_boundary_reads():
    """Two regions; region 1 holds one window, the last of chunk 0, which chunk 1 continues.  Its end column is read at the boundary
    alone: the group ends in region 0, and on the same windows as ONE chunk nothing reads it."""
    rng = np.random.default_rng(23)
    two = _tiny_store(rng, [6, 5], [20, 31])
    one = _tiny_store(np.random.default_rng(23), [11], [20, 31])
    for st in (two, one):
        reg = np.zeros(st.n_windows, np.uint64)
        reg[5] = 1
        st.annot = (st.annot & np.uint64((1 << 58) - 1)) | (reg << np.uint64(58))
    model = perturbed_model(two, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, rng)
    nan = model.copy()
    v = nan.param_vector().reshape(2, -1)
    v[1, 14] = np.nan                                      # trans[region 1][Hap][End]
    nan.set_param_vector(v.ravel())
    em1 = hmm.EMList(one, model)
    ok = em1.viterbi_minlen(nan, (2, 2, 1, 2), [0])
    assert np.isfinite(ok[2])
    em1.close()
    em = hmm.EMList(two, model)
    assert np.isfinite(em.viterbi_minlen(model, (2, 2, 1, 2), [0, 1])[2])
    with pytest.raises(N.HFError) as ei:
        em.viterbi_minlen(nan, (2, 2, 1, 2), [0, 1])
    assert ei.value.code == N.HF_E_NAN
    assert np.isfinite(em.viterbi_minlen(model, (2, 2, 1, 2), [0, 1])[2])      # and the context decodes afterwards
    em.close()


# ---- 10. command line ------------------------------------------------------------------------------------------------------------------

def test_cli_whole_contigs(tmp_path):
    """Fixed-parameter decode (-n 0) of two contigs in 40 chunks of 20 windows (80 kb chunks, 4 kb windows)."""
    store = synth.synthesize([2_000_000, 1_200_000], 4000, 80_000, [20], 1235)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = hmm.getBestNumberOfCollapsedComps(store)
    args = ["-i", str(binp), "-W", "4000", "-n", "0", "-P", "--viterbi", "--enforceMinimumLengths", "-p", str(K)] + TML.MINLEN_ARGS
    TML._cli(args, tmp_path / "chunk")
    TML._cli(args + ["--wholeContigs"], tmp_path / "whole")
    st = synth.WindowStore.read_bin(str(binp))
    assert st.window_len == 4000 and st.n_chunks == 40 and np.all(np.diff(st.chunk_off) == 20)
    zero = np.zeros((4, 4))
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, zero)
    w = (2, 3, 1, 2)
    joined = hmm.joined_chunks(st)
    off = st.chunk_off
    goff = JR.group_offsets(off, joined)[0]
    assert goff.tolist() == [0, 500, 800]
    logA, logend = viterbi_ref.tables(st, model, zero)
    ref_pc = minlen_ref.viterbi_minlen(logA, logend, off, w)
    assert len(JR.short_inner_runs(ref_pc[0], goff, w)) >= 1           # the reference: the per-chunk rule leaves short runs here
    em = hmm.EMList(st, model)
    free = em.viterbi(model)
    pc = em.viterbi_minlen(model, w)
    got = em.viterbi_minlen(model, w, joined)
    em.close()
    _check(off, (logA, logend), joined, w, got)
    # the final BED is the one written from the Python route's joined labels, and in those labels the BED's filter finds a short run
    # only where the run contains a group's first or last window
    TML._bed_from_labels(binp, got[0], tmp_path / "ref.bed", (8000, 12000, 0, 8000))
    a, b = tmp_path / "chunk", tmp_path / "whole"
    assert (b / "final_flagger_prediction.bed").read_text() == (tmp_path / "ref.bed").read_text()
    assert JR.short_inner_runs(got[0], goff, w) == []
    lp = float((b / "viterbi_log_probability.tsv").read_text())
    assert abs(lp - got[2]) <= 1e-6 + TOL * abs(lp)
    rows = (b / "viterbi_min_length_cost.tsv").read_text().splitlines()
    head = rows[0].split("\t")
    assert len(rows) == 2 and rows[0].startswith("#") and len(head) == 10
    assert head[8:] == ["log_prob_constrained_per_chunk", "short_runs_per_chunk_rule"]
    assert head[:8] == (a / "viterbi_min_length_cost.tsv").read_text().splitlines()[0].split("\t")
    f = rows[1].split("\t")
    assert [int(x) for x in f[:4]] == list(w)
    con, unc, dif, pcs = float(f[4]), float(f[5]), float(f[6]), float(f[8])
    assert con == lp and abs(unc - free[2]) <= 1e-6 + TOL * abs(unc) and abs(dif - (con - unc)) <= 2e-6 and dif <= 0.0
    assert abs(pcs - pc[2]) <= 1e-6 + TOL * abs(pcs) and con <= pcs + 1e-6
    assert int(f[7]) == sum(not np.array_equal(got[0][off[c]:off[c + 1]], free[0][off[c]:off[c + 1]]) for c in range(st.n_chunks))
    short = int(f[9])
    assert short == len(JR.short_inner_runs(pc[0], goff, w)) and short >= 1
    # every other file is the run's without the flag
    names = sorted(os.listdir(a))
    assert sorted(os.listdir(b)) == names
    for n in names:
        if n in ("final_flagger_prediction.bed", "viterbi_log_probability.tsv", "viterbi_min_length_cost.tsv") or n.startswith("prediction_summary_final"):
            continue
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    assert "posterior_prediction_final.bed" in names
