"""The E-step under minimum run lengths over groups of joined chunks on the GPU (hf_estep_minlen_joined, hf_em_iterate_minlen_joined,
EMList.estep_minlen / em_iterate_minlen with joined=, hmm_flagger --lengthConstrainedEM --crossChunkEM) against the float64 numpy
reference (tests/minlen_em_joined_ref.py), which tests/test_minlen_em_joined_cpu.py pins to the enumeration of a group's admissible
paths and to the per-chunk reference.

Tolerances, the project's, imported and not restated: xi_adm by close_post(rel=1e-9, extra_abs=1e-10); every statistics element
within 1e-9 of the summed magnitude of its terms (close_stats); log Z_adm and log Z within 1e-9 relative; the marginal identities
against hf_get_minlen_posterior of an hf_minlen_posterior_joined call within 1e-12 absolute (test_minlen_em_gpu.py says why); the
enumeration within 1e-12.  Every test prints its largest deviations before it asserts (pytest -s)."""
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
import floor_cases as FC
import geometry_cases as G
import minlen_em_joined_ref as EJ
import minlen_em_ref as E
import minlen_joined_ref as JR
import minlen_post_ref as MP
import minlen_ref
import minlen_sum_joined_ref as R
import test_minlen_em_gpu as TE
import test_minlen_gpu as TML
import test_minlen_sum_joined_gpu as TSJ

pytestmark = pytest.mark.gpu
ALGOS = TE.ALGOS
ONES = TE.ONES
TRACK_LEN = TE.TRACK_LEN
LENS = TSJ.LENS
TEG = N.HF_MODEL_TRUNC_EXP_GAUSSIAN
_same = TE._same
STAT_CASES = [c for c in minlen_ref.TINY_CASES if c[0] != N.HF_MODEL_NEGATIVE_BINOMIAL]

# test_minlen_sum_joined_gpu's boundary store (joined boundaries at windows 63, 127 and 192 of a group, 192 lane 0 of a block of the
# backward walk, where the pair across the block boundary is the J pair; positions 0, 1 and 7 mod 8 from either end) and two groups
# more: boundaries at windows 1 and 2 of a group with one-window chunks, whose statistics are all zero behind element 0; a group
# that ends exactly on a block, with its boundary at window 64
BOUNDARY_LENGTHS = TSJ.BOUNDARY_LENGTHS + [1, 1, 70] + [64, 64]
BOUNDARY_JOINED = TSJ.BOUNDARY_JOINED + [0, 1, 1] + [0, 1]
BOUNDARY_SEED = 11


def _run(em, model, min_len, joined):
    """(stats, log_z, xi, chunk vectors, log Z_adm per chunk, log Z per chunk) of one call."""
    st, lz = em.estep_minlen(model, min_len, joined)
    cs, lza, lzc = em.minlen_em_chunk_stats()
    return st, lz, em.minlen_pair_posterior(), cs, lza, lzc


def _raw(em, model, min_len, joined_ptr):
    """_run through the C ABI, `joined_ptr` as it is (NULL included)."""
    L = N.lib()
    p = model.params()
    pd = C.POINTER(C.c_double)
    st = np.empty(em.stats_len)
    lz = C.c_double(0.0)
    N.check(L.hf_estep_minlen_joined(em._h, C.byref(p), (C.c_int32 * 4)(*min_len), joined_ptr, em.stream), "hf_estep_minlen_joined")
    N.check(L.hf_estep_minlen_finish(em._h, st.ctypes.data_as(pd), C.byref(lz), em.stream), "hf_estep_minlen_finish")
    cs, lza, lzc = em.minlen_em_chunk_stats()
    return st, float(lz.value), em.minlen_pair_posterior(), cs, lza, lzc


def _check(store, joined, ref, got, what):
    """TE._check, and a group's values in its first chunk's entries: exactly 0.0 in its other chunks."""
    TE._check(store, ref, got, what)
    st, lz, xi, cs, lza, lzc = got
    inner = sorted(set(range(store.n_chunks)) - set(JR.group_first_chunks(store.chunk_off, joined).tolist()))
    assert np.all(lza[inner] == 0.0) and np.all(lzc[inner] == 0.0) and np.all(cs[inner, 0] == 0.0)
    assert not np.signbit(lza[inner]).any() and not np.signbit(lzc[inner]).any()
    assert abs(st[0] - ref["lza"].sum()) <= 1e-9 * abs(ref["lza"].sum())       # element 0 of the total: the sum over groups


def _group_first_mask(store, joined):
    goff = JR.group_offsets(store.chunk_off, joined)[0]
    first = np.zeros(store.n_windows, bool)
    first[goff[:-1][np.diff(goff) > 0]] = True
    return first


def _check_identities(em, model, store, joined, min_len, xi):
    """sum_p xi = post[t], sum_s xi = post[t-1] of hf_minlen_posterior_joined; zeros at a group's first window and nowhere else."""
    r = em.minlen_posterior(model, min_len, joined)
    post = r.posterior()
    first = _group_first_mask(store, joined)
    t = np.flatnonzero(~first)
    d1, d2 = np.abs(xi[t].sum(axis=1) - post[t]), np.abs(xi[t].sum(axis=2) - post[t - 1])
    print("identities: %.3e, %.3e (bound 1e-12)" % (float(d1.max()), float(d2.max())))
    assert np.all(d1 <= 1e-12) and np.all(d2 <= 1e-12)
    assert np.all(xi[first] == 0.0)
    assert np.all(np.abs(xi[t].sum(axis=(1, 2)) - 1.0) <= 1e-12)
    return r, post


# ---- tiny stores against the reference and the enumeration ------------------------------------------------------------------------

@pytest.mark.parametrize("case", STAT_CASES)
def test_tiny_stores_equal_group_enumeration(case):
    store, model, alpha, _ = minlen_ref.tiny_case(*case)
    off = np.asarray(store.chunk_off)
    weights = R.tiny_chunk_weights(*case)
    ems = [hmm.EMList(store, model, algo=algo) for algo in ALGOS]
    checked = 0
    for joined in JR.TINY_JOINS:
        for ml in minlen_ref.TINY_MIN_LENS:
            got = _run(ems[0], model, ml, joined)
            assert _same(got, _run(ems[1], model, ml, joined))                  # SCAN == SEQ
            _check(store, joined, EJ.stats(store, model, alpha, joined, ml), got, "tiny %s %s" % (joined, ml))
            _, gf, gl = JR.group_offsets(off, joined)
            for a, b in zip(gf.tolist(), gl.tolist()):
                if a == b:
                    continue
                pairs = EJ.enumerate_group_pairs([weights[c] for c in range(a, b + 1)], ml)
                want = np.array([[[float(v) for v in row] for row in mat] for mat in pairs])
                dev = float(np.max(np.abs(got[2][off[a]:off[b + 1]] - want)))
                print("group of chunks %d..%d %s: largest |xi - enumeration| %.3e (bound 1e-12)" % (a, b, ml, dev))
                assert dev <= 1e-12
                checked += 1
    assert checked == 8
    for em in ems:
        em.close()


# ---- the boundary store ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _boundary():
    rng = np.random.default_rng(BOUNDARY_SEED)
    store = _tiny_store(rng, BOUNDARY_LENGTHS, [20, 31])
    model = perturbed_model(store, TEG, 3, synth.HIFI_ALPHA, rng)
    goff = JR.group_offsets(store.chunk_off, BOUNDARY_JOINED)[0]
    assert goff.tolist() == [0, 321, 465, 528, 655, 727, 855]
    assert EJ.boundary_windows(store.chunk_off, BOUNDARY_JOINED).tolist()[:3] == [63, 127, 192]
    return store, model


@functools.lru_cache(maxsize=None)
def _boundary_ref(min_len, joined=tuple(BOUNDARY_JOINED)):
    store, model = _boundary()
    return EJ.stats(store, model, synth.HIFI_ALPHA, np.array(joined, bool), min_len)


@functools.lru_cache(maxsize=None)
def _boundary_per_chunk_ref(min_len):
    store, model = _boundary()
    return E.stats(store, model, synth.HIFI_ALPHA, min_len)


@functools.lru_cache(maxsize=None)
def _chunk_magnitudes(min_len):
    """[C][V]: the summed magnitude of the terms of every element of every chunk's vector (accumulate returns the total's alone: the
    total of the counts of one chunk, the others' zeroed, is that chunk's)."""
    store, model = _boundary()
    ref = _boundary_ref(min_len)
    off = np.asarray(store.chunk_off)
    out = []
    for c in range(store.n_chunks):
        xi = np.zeros_like(ref["xi"])
        xi[off[c]:off[c + 1]] = ref["xi"][off[c]:off[c + 1]]
        lza = np.zeros_like(ref["lza"])
        lza[c] = ref["lza"][c]
        out.append(E.accumulate(store, model, synth.HIFI_ALPHA, xi, lza)[1])
    return np.array(out)


@pytest.mark.parametrize("min_len", LENS)
def test_joined_boundaries_around_the_blocks_and_the_rescaling_period(min_len):
    store, model = _boundary()
    ref = _boundary_ref(min_len)
    bound = ref["bound"]
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        for _ in range(2):                                   # a second call: identical bits
            res.append(_run(em, model, min_len, BOUNDARY_JOINED))
        if algo == ALGOS[0]:
            r, post = _check_identities(em, model, store, BOUNDARY_JOINED, min_len, res[0][2])
            assert np.array_equal(res[0][4], r.chunk_log_z_adm)                 # element 0 bit for bit the posterior's log Z_adm
            if min_len == ONES:                              # the group factorises: the per-chunk call, the boundary pair a product
                pc = TE._run(em, model, ONES)
                inside = np.ones(store.n_windows, bool)
                inside[bound] = False
                MP.close_post(res[0][2][inside], pc[2][inside], rel=1e-9, extra_abs=1e-10)
                MP.close_post(res[0][2][bound], post[bound - 1][:, :, None] * post[bound][:, None, :], rel=1e-9, extra_abs=1e-10)
                E.close_stats(res[0][0], pc[0], _boundary_per_chunk_ref(ONES)["mag"], "all ones against the per-chunk call")
                assert abs(res[0][4].sum() - pc[4].sum()) <= 1e-9 * abs(pc[4].sum())
                assert abs(res[0][1] - pc[1]) <= 1e-9 * abs(pc[1])
        em.close()
    _check(store, BOUNDARY_JOINED, ref, res[0], "boundary store %s" % (min_len,))
    assert all(_same(res[0], r) for r in res[1:])
    T = np.diff(store.chunk_off)
    cs = res[0][3]
    assert not cs[T <= 2, 1:].any()                          # the one-window chunks: exactly zero behind element 0
    assert all(cs[c, 1:].any() for c in np.flatnonzero(T >= 3))
    # per chunk: every chunk's vector against the reference's, within 1e-9 of the summed magnitude of that chunk's own terms
    cmag = _chunk_magnitudes(min_len)
    for c in range(store.n_chunks):
        err = np.abs(cs[c] - ref["chunk"][c])
        assert np.all(err <= 1e-9 * cmag[c]), (c, int(np.argmax(err - 1e-9 * cmag[c])))
    if min_len == TRACK_LEN:                                 # the rule says something on this store
        inside = np.ones(store.n_windows, bool)
        inside[bound] = False
        assert float(np.max(np.abs(ref["xi"][inside] - _boundary_per_chunk_ref(min_len)["xi"][inside]))) > 1e-6


# ---- joined = NULL and all-zero joined ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
def test_no_join_is_the_per_chunk_entry_point_bit_for_bit(algo):
    store, model = _boundary()
    em = hmm.EMList(store, model, algo=algo)
    zero = np.zeros(store.n_chunks, bool)
    for ml in (TRACK_LEN, (16, 16, 16, 16), ONES):
        want = TE._run(em, model, ml)
        assert _same(want, _run(em, model, ml, zero))
        assert _same(want, _raw(em, model, ml, None))
        assert _same(want, _run(em, model, ml, None))
        assert not _same(want, _run(em, model, ml, BOUNDARY_JOINED))
        assert _same(want, TE._run(em, model, ml))          # and the per-chunk call replaces the joined one's results
    em.close()


# ---- geometry, the emission floor ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _grid_ref(joined_key):
    model_type, seed = G.CASES[0]
    store, model, alpha, _ = G.case(model_type, seed)
    return EJ.stats(store, model, alpha, np.array(joined_key, bool), TRACK_LEN)


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunks_and_uncovered_windows(algo):
    model_type, seed = G.CASES[0]
    store, model, alpha, _ = G.case(model_type, seed)
    ml = TRACK_LEN
    em0 = hmm.EMList(store, model, algo=algo)
    base = _run(em0, model, ml, G.joins())
    _check(store, G.joins(), _grid_ref(G.joins_key(G.joins())), base, "grid store")
    # a chunk without windows between joined chunks ends the group, whatever its own and its successor's entries say
    est, src = G.with_empty_chunks(store)
    dev_j, ref_j = G.empty_chunk_joins(src, G.joins())
    cut = _run(em0, model, ml, ref_j)
    _check(store, ref_j, _grid_ref(G.joins_key(ref_j)), cut, "grid store, groups cut")
    em0.close()
    em = hmm.EMList(est, model, algo=algo)
    st, lz, xi, cs, lza, lzc = _run(em, model, ml, dev_j)
    assert np.array_equal(xi, cut[2]) and np.array_equal(cs[src >= 0], cut[3])
    assert np.array_equal(lza[src >= 0], cut[4]) and np.array_equal(lzc[src >= 0], cut[5])
    assert not cs[src < 0].any() and not lza[src < 0].any() and not lzc[src < 0].any()
    E.close_stats(st, cut[0], _grid_ref(G.joins_key(ref_j))["mag"], "with chunks without windows", rel=1e-13)   # (k_reduce's lanes hold other chunks)
    em.close()
    # windows outside every chunk
    ust = G.with_uncovered_windows(store, np.random.default_rng(5))
    a, n = G.FRONT, ust.n_windows
    b = a + store.n_windows
    em = hmm.EMList(ust, model, algo=algo)
    st, lz = em.estep_minlen(model, ml, G.joins())
    cs, lza, lzc = em.minlen_em_chunk_stats()
    assert np.array_equal(st, base[0]) and lz == base[1] and np.array_equal(cs, base[3])
    assert np.array_equal(lza, base[4]) and np.array_equal(lzc, base[5])
    assert np.array_equal(em.minlen_pair_posterior(a, store.n_windows), base[2])
    for f, cnt in [(0, 1), (a - 1, 4), (0, n), (b, 1)]:
        with pytest.raises(N.HFError) as ei:
            em.minlen_pair_posterior(f, cnt)
        assert ei.value.code == N.HF_E_ARG, (f, cnt)
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunk_list(algo):
    full = synth.synthesize([50_000], 1000, 20_000, [20], seed=2)
    store = full.subset_chunks([])
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, full, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model, algo=algo)
    st, lz = em.estep_minlen(model, TRACK_LEN, np.zeros(0, bool))
    assert not st.any() and lz == 0.0 and em.minlen_pair_posterior().shape == (0, 4, 4)
    assert not _raw(em, model, TRACK_LEN, None)[0].any()
    em.close()


def test_a_floored_stretch_across_a_joined_boundary():
    """floor_cases.long(): windows 1940..1959 at the 1e-40 emission floor, ten on either side of the boundary between chunks 2 and 3,
    which the fixture joins: a whole rescaling period of the walk on both sides of J_t.  Same tolerances, no NaN, no HF_E_SCALE."""
    store, model, alpha = FC.long()
    joined = FC.joins("long")
    off = np.asarray(store.chunk_off)
    assert joined[3] and all(store.cov[t] == FC.COV for t in range(int(off[3]) - 10, int(off[3]) + 10))
    ref = EJ.stats(store, model, alpha, joined, TRACK_LEN)
    assert np.all(np.isfinite(ref["lza"])) and ref["lza"][2] < -1000
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        res.append(_run(em, model, TRACK_LEN, joined))
        if algo == ALGOS[0]:
            _check_identities(em, model, store, joined, TRACK_LEN, res[0][2])
        em.close()
    _check(store, joined, ref, res[0], "floored boundary")
    assert _same(res[0], res[1])


# ---- three EM iterations ---------------------------------------------------------------------------------------------------------------

EM_SEED = 0        # chosen on the CPU: the first seed from 0 with no estimator count of the three reference iterations within 1e-6 of
                   # the 10 < count gate
EM_LENGTHS = [200, 129, 65, 300, 90]
EM_JOINED = [0, 1, 0, 1, 1]              # two groups of more than one chunk: 329 and 455 windows


def _em_case(seed=EM_SEED):
    rng = np.random.default_rng(8900 + seed)
    store = _tiny_store(rng, EM_LENGTHS, [20, 31])
    model = perturbed_model(store, TEG, 3, synth.HIFI_ALPHA, rng)
    return store, model


def test_three_em_iterations():
    store, model = _em_case()
    alpha = synth.HIFI_ALPHA
    assert JR.group_offsets(store.chunk_off, EM_JOINED)[0].tolist() == [0, 329, 784]
    em = hmm.EMList(store, model)
    before = None
    for it in range(3):
        at = model.copy()                                   # the parameters this iteration's E-step runs with
        ref = EJ.stats(store, at, alpha, EM_JOINED, TRACK_LEN)
        assert np.all(np.abs(ref["vec"][1:] - 10.0) > 1e-6)
        em.em_iterate_minlen(model, TRACK_LEN, True, 1e-3, joined=EM_JOINED)
        E.close_stats(model.estimators, ref["vec"], ref["mag"], "iteration %d" % it)
        assert model.loglikelihood == model.estimators[0]
        assert abs(model.loglikelihood - ref["lza"].sum()) <= 1e-9 * abs(ref["lza"].sum())
        assert abs(em.last_log_z - ref["lz"].sum()) <= 1e-9 * abs(ref["lz"].sum())
        assert not np.array_equal(model.param_vector(), at.param_vector())
        if before is not None:
            print("objective %.6f -> %.6f" % (before, model.loglikelihood))
        before = model.loglikelihood
        hmm.HMM_resetEstimators(model)
    # the function of the reference's naming, one E-step: the same call
    want = em.estep_minlen(model, TRACK_LEN, EM_JOINED)
    lz = hmm.EM_runOneMinLengthIterationForList(em, model, TRACK_LEN, EM_JOINED)
    assert np.array_equal(model.estimators, want[0]) and lz == want[1] and model.loglikelihood == want[0][0]
    em.close()


# ---- arguments and errors ----------------------------------------------------------------------------------------------------------------

def test_arguments_getters_and_errors():
    store, model = _boundary()
    joined = np.array(BOUNDARY_JOINED, bool)
    em = hmm.EMList(store, model)
    L = N.lib()
    pd = C.POINTER(C.c_double)
    xi = np.empty((store.n_windows, 16))
    st = np.empty(em.stats_len)
    four = (C.c_int32 * 4)(*TRACK_LEN)
    jn = np.ascontiguousarray(joined, np.uint8)
    jp = jn.ctypes.data_as(C.POINTER(C.c_uint8))
    p = model.params()
    who = b"hf_estep_minlen_joined"

    def getters_refuse():
        assert L.hf_get_minlen_pair_posterior(em._h, 0, store.n_windows, xi.ctypes.data_as(pd)) == N.HF_E_ARG
        assert L.hf_get_minlen_em_chunk_stats(em._h, None, None, None) == N.HF_E_ARG

    getters_refuse()                                       # before any call
    assert L.hf_estep_minlen_finish(em._h, st.ctypes.data_as(pd), None, None) == N.HF_E_ARG
    assert L.hf_estep_minlen_joined(None, C.byref(p), four, jp, None) == N.HF_E_ARG
    assert L.hf_estep_minlen_joined(em._h, None, four, jp, None) == N.HF_E_ARG and who in L.hf_last_error()
    assert L.hf_estep_minlen_joined(em._h, C.byref(p), None, jp, None) == N.HF_E_ARG and who in L.hf_last_error()
    assert L.hf_em_iterate_minlen_joined(em._h, None, four, jp, 1, 1e-3, st.ctypes.data_as(pd), None, None, None) == N.HF_E_ARG
    bad0 = jn.copy()
    bad0[0] = 1
    assert L.hf_estep_minlen_joined(em._h, C.byref(p), four, bad0.ctypes.data_as(C.POINTER(C.c_uint8)), None) == N.HF_E_ARG
    assert b"joined[0]" in L.hf_last_error() and who in L.hf_last_error()
    for bad_len in ((3, 0, 1, 1), (-1, 1, 1, 1), (62, 1, 1, 1)):          # the last: 65 in sum
        with pytest.raises(N.HFError) as ei:
            em.estep_minlen(model, bad_len, joined)
        assert ei.value.code == N.HF_E_ARG and "hf_estep_minlen_joined" in str(ei.value), bad_len
    assert b"above HF_MINLEN_MAX_LANES" in L.hf_last_error()
    for wrong in (joined[:-1], np.concatenate([joined, [False]])):
        with pytest.raises(ValueError):
            em.estep_minlen(model, TRACK_LEN, wrong)
        with pytest.raises(ValueError):
            em.em_iterate_minlen(model, TRACK_LEN, joined=wrong)
    getters_refuse()                                       # a refused call is no finished call
    assert L.hf_estep_minlen_finish(em._h, st.ctypes.data_as(pd), None, None) == N.HF_E_ARG
    with pytest.raises(ValueError):
        hmm.runHMMFlagger(em, model, 1, constrainedJoined=joined)
    good = _run(em, model, (61, 1, 1, 1), joined)           # a sum of exactly 64 is served
    assert L.hf_estep_minlen_joined(em._h, C.byref(p), four, jp, None) == N.HF_OK
    getters_refuse()                                       # launched, not finished
    assert L.hf_estep_minlen_finish(em._h, st.ctypes.data_as(pd), None, None) == N.HF_OK   # log_z may be NULL
    bad = model.copy()
    v = bad.param_vector().reshape(model.numberOfRegions, -1)
    v[:, 20:24] = 0.0                                      # start row: no path of any group has weight
    bad.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.estep_minlen(bad, TRACK_LEN, joined)
    assert ei.value.code == N.HF_E_SCALE
    getters_refuse()                                       # a failed call is no finished call
    assert _same(good, _run(em, model, (61, 1, 1, 1), joined))   # and the context answers correctly afterwards
    em.close()


def test_negative_binomial_is_refused():
    store = synth.config(2, 0.02)
    model = hmm.createModel(hmm.MODEL_NEGATIVE_BINOMIAL, 3, store, np.zeros((4, 4)))
    em = hmm.EMList(store, model)
    with pytest.raises(N.HFError) as ei:
        em.estep_minlen(model, TRACK_LEN, hmm.joined_chunks(store))
    assert ei.value.code == N.HF_E_ARG and "negative_binomial" in str(ei.value) and "hf_estep_minlen_joined" in str(ei.value)
    em.close()


# ---- no disturbance ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
def test_no_disturbance_of_the_last_pass_and_the_decoders(algo):
    store = synth.synthesize(synth.human_diploid_lengths(0.005), 4000, 100_000, [20], 1236, contig_prefix="hap_ctg")
    joined = hmm.joined_chunks(store)
    assert joined.sum() >= 40
    model = hmm.createModel(TEG, 4, store, synth.HIFI_ALPHA)
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
    mlv = em_a.viterbi_minlen(model, TRACK_LEN, joined)
    smp = em_a.sample_paths(model, 2, 7)
    mls = em_a.sample_paths_minlen(model, TRACK_LEN, 3, 2, joined=joined)
    r = em_a.minlen_posterior(model, TRACK_LEN, joined)
    mpost = r.posterior()
    other = model.copy()                                   # the feature runs with DIFFERENT parameters
    v = other.param_vector().reshape(other.numberOfRegions, -1)
    v[:, 27:27 + 4 * 16] *= 1.1
    other.set_param_vector(v.ravel())
    r1 = _run(em_a, other, TRACK_LEN, joined)
    r2 = _run(em_a, other, (2, 2, 2, 2), joined)
    r3 = TE._run(em_a, other, TRACK_LEN)
    assert not np.array_equal(r1[0], r2[0]) and not np.array_equal(r1[0], r3[0]) and not np.array_equal(r1[0][1:], st_a[1:])
    assert r1[0][0] < r3[0][0] - 1e-6                       # the rule over the groups keeps less mass on this store
    assert np.array_equal(em_a.labels(), em_b.labels())
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    for x, y in zip(em_a.forward_backward(), em_b.forward_backward()):
        assert np.array_equal(x, y)
    lab, ll = TML._viterbi_results(em_a)
    assert np.array_equal(lab, vit[0]) and np.array_equal(ll, vit[1])
    L = N.lib()
    mlab = np.empty(store.n_windows, np.int8)
    mll = np.empty(store.n_chunks)
    assert L.hf_get_viterbi_minlen_labels(em_a._h, mlab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
    assert L.hf_get_viterbi_minlen_chunk_log_probs(em_a._h, mll.ctypes.data_as(C.POINTER(C.c_double))) == N.HF_OK
    assert np.array_equal(mlab, mlv[0]) and np.array_equal(mll, mlv[1])
    assert np.array_equal(TML._sample_results(em_a, 2), smp)
    for k in range(3):
        assert L.hf_get_minlen_sample_labels(em_a._h, k, mlab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
        assert np.array_equal(mlab, mls[k])
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
    store, model = _boundary()
    em0 = hmm.EMList(store, model)
    want = _run(em0, model, TRACK_LEN, BOUNDARY_JOINED)
    em0.close()
    with Streams() as streams:
        s = streams.new(non_blocking=True)
        em = hmm.EMList(store, model, stream=s)
        streams.h.delay(s)                                 # whatever ran on the null stream instead would run ahead of this
        got = _run(em, model, TRACK_LEN, BOUNDARY_JOINED)
        assert _same(want, got)
        em.close()


# ---- command line ------------------------------------------------------------------------------------------------------------------------

def test_cli_cross_chunk_em(tmp_path):
    """test_minlen_em_gpu.test_cli_equals_the_python_loop's reduced store cut into five chunks of 250 windows, so that its contig has
    more than one chunk: --crossChunkEM is the Python loop over the joined step, and without it the run writes what it wrote."""
    store = synth.synthesize([5_000_000], 4000, 1_000_000, [20], 1235)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = hmm.getBestNumberOfCollapsedComps(store)
    wl = 4000
    args = ["-i", str(binp), "-W", str(wl), "-n", "3", "-p", str(K), "--minimumLengths", "%d,%d,%d" % (wl * TRACK_LEN[0], wl * TRACK_LEN[1], wl * TRACK_LEN[3]),
            "--lengthConstrainedEM"]
    TML._cli(args, tmp_path / "chunk")
    r = TML._cli(args + ["--crossChunkEM"], tmp_path / "cross")
    assert "--crossChunkEM" in r.stderr and "joined chunks of a contig" in r.stderr
    st = synth.WindowStore.read_bin(str(binp))
    joined = hmm.joined_chunks(st)
    assert st.n_chunks == 5 and joined.tolist() == [False, True, True, True, True]
    names = ("emission_final.tsv", "transition_final.tsv", "length_constrained_em.tsv", "loglikelihood.tsv")
    lls = {}
    for out, jn in (("py_cross", joined), ("py_chunk", None)):
        model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, np.zeros((4, 4)))
        em = hmm.EMList(st, model)
        os.makedirs(tmp_path / out)
        lls[out] = hmm.runHMMFlagger(em, model, 3, 0.001, str(tmp_path / out), constrainedMinLen=TRACK_LEN, constrainedJoined=jn)
        em.close()
    for name in names:
        assert (tmp_path / "cross" / name).read_bytes() == (tmp_path / "py_cross" / name).read_bytes(), name
        assert (tmp_path / "chunk" / name).read_bytes() == (tmp_path / "py_chunk" / name).read_bytes(), name      # as before
    rows = TE._tsv(tmp_path / "cross" / "length_constrained_em.tsv")
    assert open(tmp_path / "cross" / "length_constrained_em.tsv").readline() == hmm.LCEM_HEADER
    assert len(rows) == 3 and all(float(x[3]) < 0.0 for x in rows)
    assert [float(x[1]) for x in rows] == [float("%.4f" % v) for v in lls["py_cross"][:3]]
    rows_pc = TE._tsv(tmp_path / "chunk" / "length_constrained_em.tsv")
    # the first iteration runs with the same parameters: less mass under the contig rule, the same log Z (a group's is the sum of
    # its chunks' to rounding; two numbers printed with four decimals)
    assert float(rows[0][1]) < float(rows_pc[0][1]) - 1e-3 and abs(float(rows[0][2]) - float(rows_pc[0][2])) <= 2e-4
    assert sorted(os.listdir(tmp_path / "cross")) == sorted(os.listdir(tmp_path / "chunk"))
