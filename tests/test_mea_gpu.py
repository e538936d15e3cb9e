"""Maximum-expected-accuracy decoding under minimum run lengths on the GPU (hf_get_mea_labels, EMList.mea_labels,
hmm.EM_getMaxExpectedGainLabelsForList) against enumeration of all labellings on tiny stores and the float64 numpy reference
(tests/mea_ref.py) elsewhere.  "Optimal" is shown by evaluation, as in test_minlen_gpu: the returned labels are admissible and
supported (exact checks), and their expected gain under the reference posterior and the reported block score are within
TOL * windows_of_block * max|W| of the reference optimum.  No bitwise equality is asked between the two kinds of context (their f
and b differ in the last bit); it is asked across repeated calls."""
import ctypes as C
import functools

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_bruteforce_cpu import _tiny_store
from test_viterbi_cpu import perturbed_model
import mea_ref
import minlen_ref
import posterior_ref
import viterbi_ref

pytestmark = pytest.mark.gpu
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]
TOL = 1e-9
ONES = (1, 1, 1, 1)
TRACK_LEN = (3, 5, 1, 7)
GEOMETRY_LENS = [(3, 5, 1, 7), (16, 16, 16, 16), (61, 1, 1, 1)]
GEOMETRY_JOINED = np.array([0, 1, 1, 1, 0, 1, 1, 1, 1, 1], bool)        # two groups: 63+64+65+129 and 15+16+17+31+32+33 windows


def _context(store, model, algo=N.HF_ALGO_SCAN):
    """A context whose last pass is a full pass with the model's parameters (the model is left as it was)."""
    em = hmm.EMList(store, model, algo=algo)
    em.launch(model, N.HF_MODE_FULL)
    em.finish()
    return em


def _blocks(store, joined):
    if joined is None:
        return np.asarray(store.chunk_off, np.int64), np.arange(store.n_chunks)
    return mea_ref.group_off(store.chunk_off, joined)


def _list_sum(x):
    tot = 0.0
    for v in x:
        tot += float(v)
    return tot


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _check(store, post, logA, W, min_len, joined, got):
    """Admissible, supported, and optimal by evaluation.  Returns the reference's block scores."""
    labels, block, total = got
    boff, gchunk = _blocks(store, joined)
    assert minlen_ref.admissible(labels, boff, min_len).all()
    assert mea_ref.supported(labels, post, logA, store.chunk_off).all()
    G = mea_ref.gain_rows(post, logA, store.chunk_off, W)
    ref_lab, ref_score = mea_ref.decode(G, boff, min_len)
    tol = TOL * np.diff(boff) * np.abs(W).max()
    val = mea_ref.expected_gain(labels, post, W, boff)
    assert np.all(np.abs(val - ref_score) <= tol), np.max(np.abs(val - ref_score) - tol)
    assert np.all(np.abs(block[gchunk] - ref_score) <= tol), np.max(np.abs(block[gchunk] - ref_score) - tol)
    rest = np.ones(store.n_chunks, bool)
    rest[gchunk] = False
    assert np.all(block[rest] == 0.0)                      # a group's score sits in the entry of its first chunk
    assert total == _list_sum(block)
    return ref_score


# ---- tiny stores against enumeration ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _enumerated(case, min_len, wi, joined):
    store, model, alpha, post, logA = mea_ref.tiny(*case)
    boff, _ = _blocks(store, mea_ref.TINY_JOINED if joined else None)
    G = mea_ref.gain_rows(post, logA, store.chunk_off, mea_ref.TINY_GAINS[wi])
    return [mea_ref.enumerate_block(G, int(boff[b]), int(boff[b + 1]), min_len) for b in range(boff.size - 1)]


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed,hifi", minlen_ref.TINY_CASES)
def test_tiny_stores_equal_enumeration(algo, model_type, seed, hifi):
    case = (model_type, seed, hifi)
    store, model, alpha, post, logA = mea_ref.tiny(*case)
    em = _context(store, model, algo)
    for min_len in minlen_ref.TINY_MIN_LENS:
        for wi, W in enumerate(mea_ref.TINY_GAINS):
            for joined in (None, mea_ref.TINY_JOINED):
                got = hmm.EM_getMaxExpectedGainLabelsForList(em, min_len, joined, W)
                _check(store, post, logA, W, min_len, joined, got)
                labels, block, total = got
                boff, gchunk = _blocks(store, joined)
                enum = _enumerated(case, min_len, wi, joined is not None)
                clear = 0
                for b, (path, best, second) in enumerate(enum):
                    T = int(boff[b + 1] - boff[b])
                    assert abs(block[gchunk[b]] - best) <= TOL * T * np.abs(W).max(), (min_len, wi, b, block[gchunk[b]], best)
                    if best - second > 1e-9:
                        assert np.array_equal(labels[boff[b]:boff[b + 1]], path), (min_len, wi, b, labels[boff[b]:boff[b + 1]], path)
                        clear += 1
                assert clear >= (boff.size - 1) // 2
    em.close()


# ---- lane and block geometry -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _geometry():
    """The store of test_minlen_gpu._geometry with its reference posterior and rows."""
    rng = np.random.default_rng(5)
    store = _tiny_store(rng, [63, 64, 65, 129, 15, 16, 17, 31, 32, 33], [20, 31])
    model = perturbed_model(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, rng)
    post = posterior_ref.reference(store, model, synth.HIFI_ALPHA)[0]
    logA, _ = viterbi_ref.tables(store, model, synth.HIFI_ALPHA)
    return store, model, post, logA


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("min_len", GEOMETRY_LENS)
def test_lane_and_block_geometry(algo, min_len):
    """Chunks around the 64-window staging block and around a minimum length of 16; 64 lanes, one state owning 61 of them; per chunk
    and joined in two groups."""
    store, model, post, logA = _geometry()
    bites = int(np.sum(~minlen_ref.admissible(np.argmax(post, axis=1), store.chunk_off, min_len)))
    assert bites >= store.n_chunks // 2, bites             # posterior argmax is inadmissible: the constraint bites
    em = _context(store, model, algo)
    per_chunk = _check(store, post, logA, mea_ref.IDENTITY, min_len, None, em.mea_labels(min_len))
    joined = _check(store, post, logA, mea_ref.IDENTITY, min_len, GEOMETRY_JOINED, em.mea_labels(min_len, GEOMETRY_JOINED))
    assert joined.size == 2 and joined.sum() <= per_chunk.sum() + TOL * store.n_windows
    em.close()


# ---- a realistic track -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _track():
    store = synth.config(2, 0.02)
    model = hmm.createModel(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, store, synth.HIFI_ALPHA)      # untrained
    post = posterior_ref.reference(store, model, synth.HIFI_ALPHA)[0]
    logA, _ = viterbi_ref.tables(store, model, synth.HIFI_ALPHA)
    return store, model, post, logA


def test_realistic_track():
    store, model, post, logA = _track()
    W = mea_ref.IDENTITY
    joined = hmm.joined_chunks(store)
    assert int(np.sum(~minlen_ref.admissible(np.argmax(post, axis=1), store.chunk_off, TRACK_LEN))) >= 1
    em = _context(store, model)
    a = em.mea_labels(TRACK_LEN)
    aj = em.mea_labels(TRACK_LEN, joined)
    _check(store, post, logA, W, TRACK_LEN, None, a)
    _check(store, post, logA, W, TRACK_LEN, joined, aj)
    tol = TOL * store.n_windows
    gain_argmax = float(post.max(axis=1).sum())
    assert aj[2] <= a[2] + tol and a[2] <= gain_argmax + tol
    goff, _ = mea_ref.group_off(store.chunk_off, joined)
    rule = mea_ref.final_bed_rule(post, store.chunk_off, joined, TRACK_LEN)
    assert minlen_ref.admissible(rule, goff, TRACK_LEN).all()          # (Hap may be one window long: relabelling to Hap breaks nothing)
    if mea_ref.supported(rule, post, logA, store.chunk_off).all():
        assert aj[2] >= float(mea_ref.expected_gain(rule, post, W, goff).sum()) - tol
    assert _same(a, em.mea_labels(TRACK_LEN))                          # a second call: identical bits
    assert _same(aj, em.mea_labels(TRACK_LEN, joined))
    em.close()


# ---- exact cases -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["geometry", "track"])
@pytest.mark.parametrize("algo", ALGOS)
def test_exact_cases(algo, which):
    store, model, post, logA = _geometry() if which == "geometry" else _track()
    joined = GEOMETRY_JOINED if which == "geometry" else hmm.joined_chunks(store)
    off = store.chunk_off
    em = _context(store, model, algo)
    # lengths 1 with the identity: posterior argmax wherever the two largest posteriors are clearly apart
    srt = np.sort(post, axis=1)
    clear = srt[:, 3] - srt[:, 2] > 1e-9
    assert clear.mean() >= 0.99
    pass_labels = em.labels()
    for jn in (None, joined):
        lab, block, total = em.mea_labels(ONES, jn)
        assert np.array_equal(lab[clear], pass_labels[clear])
    # a gain four times as large: the same labels bit for bit, scores exactly four times as large
    for jn in (None, joined):
        one = em.mea_labels(TRACK_LEN, jn, mea_ref.ASYM)
        four = em.mea_labels(TRACK_LEN, jn, mea_ref.ASYM * 4)
        assert np.array_equal(one[0], four[0]) and np.array_equal(one[1] * 4, four[1]) and one[2] * 4 == four[2]
    # a gain whose only non-zero column is k: the constant label k in every chunk where that is supported
    checked = 0
    for k in range(4):
        W = np.zeros((4, 4))
        W[:, k] = 1.0
        lab, block, total = em.mea_labels(TRACK_LEN, None, W)
        const = np.full(store.n_windows, k, np.int8)
        sup = mea_ref.supported(const, post, logA, off)
        for c in np.flatnonzero(sup):
            assert np.all(lab[off[c]:off[c + 1]] == k), (k, c)
        checked += int(sup.sum())
    assert checked >= store.n_chunks                       # (Hap is supported everywhere; Err and Dup are not where their column is masked)
    em.close()


# ---- support ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _forbidden_step():
    """A one-region store (no region change re-opens the step) and a model whose transition Hap -> Col is 0.  Seed and entry are chosen
    so that the reference that ignores support takes the step (8 times, in 5 chunks) while every scale of the pass stays above its
    floor of 1e-50 (the smallest is 1e-40)."""
    rng = np.random.default_rng(5)
    store = _tiny_store(rng, [63, 64, 65, 129, 15, 16, 17, 31, 32, 33], [25])
    model = perturbed_model(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, rng)
    R = model.numberOfRegions
    assert R == 1
    v = model.param_vector().reshape(R, -1)
    v[:, 2 * 5 + 3] = 0.0
    model.set_param_vector(v.ravel())
    post = posterior_ref.reference(store, model, synth.HIFI_ALPHA)[0]
    logA, _ = viterbi_ref.tables(store, model, synth.HIFI_ALPHA)
    return store, model, post, logA


def _chunks_with_step(labels, off, p, k):
    lab = np.asarray(labels)
    return [c for c in range(off.size - 1) if np.any((lab[off[c]:off[c + 1] - 1] == p) & (lab[off[c] + 1:off[c + 1]] == k))]


@pytest.mark.parametrize("algo", ALGOS)
def test_support_keeps_a_forbidden_step_out(algo):
    store, model, post, logA = _forbidden_step()
    off = np.asarray(store.chunk_off, np.int64)
    free = mea_ref.gain_rows(post, logA, off, mea_ref.IDENTITY, support=False)
    ignored, _ = mea_ref.decode(free, off, TRACK_LEN)
    assert len(_chunks_with_step(ignored, off, 2, 3)) >= 1             # without the support rule the optimum takes the step
    em = _context(store, model, algo)
    got = em.mea_labels(TRACK_LEN)
    assert _chunks_with_step(got[0], off, 2, 3) == []
    _check(store, post, logA, mea_ref.IDENTITY, TRACK_LEN, None, got)
    em.close()


# ---- isolation and refusals ------------------------------------------------------------------------------------------------------

def _decoder_results(em):
    L = N.lib()
    n, c = em.store.n_windows, em.store.n_chunks
    i8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int8))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    vl, vs, pl, pm, pz, pp = np.empty(n, np.int8), np.empty(c), np.empty(n, np.int8), np.empty(c), np.empty(c), np.empty((n, 4))
    assert L.hf_get_viterbi_minlen_labels(em._h, i8(vl)) == N.HF_OK
    assert L.hf_get_viterbi_minlen_chunk_log_probs(em._h, dp(vs)) == N.HF_OK
    assert L.hf_get_minlen_posterior_labels(em._h, i8(pl)) == N.HF_OK
    assert L.hf_get_minlen_chunk_log_mass(em._h, dp(pm), dp(pz)) == N.HF_OK
    assert L.hf_get_minlen_posterior(em._h, 0, n, dp(pp)) == N.HF_OK
    return [em.labels(), em.posterior(), vl, vs, pl, pm, pz, pp]


@pytest.mark.parametrize("algo", ALGOS)
def test_isolation(algo):
    store, model, post, logA = _geometry()
    em = hmm.EMList(store, model, algo=algo)
    em.launch(model, N.HF_MODE_FULL)
    stats = em.finish()
    em.viterbi_minlen(model, TRACK_LEN)
    em.minlen_posterior(model, TRACK_LEN)
    before = _decoder_results(em)
    first = em.mea_labels(TRACK_LEN, GEOMETRY_JOINED, mea_ref.ASYM)
    em.mea_labels((16, 16, 16, 16))
    after = _decoder_results(em)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    em.launch(model, N.HF_MODE_FULL)                       # the next pass, and the getter behind it
    assert np.array_equal(stats, em.finish())
    assert _same(first, em.mea_labels(TRACK_LEN, GEOMETRY_JOINED, mea_ref.ASYM))
    em.close()


def test_refusals():
    store, model, post, logA = _geometry()
    em = hmm.EMList(store, model)
    L = N.lib()
    lab = np.empty(store.n_windows, np.int8)
    labp = lab.ctypes.data_as(C.POINTER(C.c_int8))
    ones = (C.c_int32 * 4)(1, 1, 1, 1)
    assert L.hf_get_mea_labels(em._h, None, ones, None, labp, None, None) == N.HF_E_ARG      # before any full pass
    with pytest.raises(N.HFError) as ei:
        em.mea_labels(ONES)
    assert ei.value.code == N.HF_E_ARG
    em.launch(model, N.HF_MODE_FORWARD_ONLY)
    em.finish()
    assert L.hf_get_mea_labels(em._h, None, ones, None, labp, None, None) == N.HF_E_ARG      # a forward-only pass is none
    em.launch(model, N.HF_MODE_FULL)
    em.finish()
    assert L.hf_get_mea_labels(em._h, None, ones, None, labp, None, None) == N.HF_OK         # block and total may be NULL
    good = em.mea_labels(TRACK_LEN, GEOMETRY_JOINED)
    assert L.hf_get_mea_labels(em._h, None, ones, None, None, None, None) == N.HF_E_ARG      # a NULL label array
    assert L.hf_get_mea_labels(em._h, None, None, None, labp, None, None) == N.HF_E_ARG
    assert L.hf_get_mea_labels(None, None, ones, None, labp, None, None) == N.HF_E_ARG
    for bad_len in ((3, 0, 1, 1), (-1, 1, 1, 1), (62, 1, 1, 1), (2 ** 31 - 1, 2 ** 31 - 1, 1, 1)):
        with pytest.raises(N.HFError) as ei:
            em.mea_labels(bad_len)
        assert ei.value.code == N.HF_E_ARG, bad_len
    with pytest.raises(ValueError):
        em.mea_labels((1, 1, 1))
    bad_joined = GEOMETRY_JOINED.copy()
    bad_joined[0] = True
    with pytest.raises(N.HFError) as ei:
        em.mea_labels(ONES, bad_joined)
    assert ei.value.code == N.HF_E_ARG
    with pytest.raises(ValueError):
        em.mea_labels(ONES, GEOMETRY_JOINED[:-1])
    for bad in (np.inf, -np.inf, np.nan, 1.0000001e100, -2e100):
        W = np.eye(4)
        W[1, 2] = bad
        with pytest.raises(N.HFError) as ei:
            em.mea_labels(ONES, None, W)
        assert ei.value.code == N.HF_E_ARG, bad
    W = np.eye(4)
    W[1, 2] = -1e100                                       # the largest magnitude that is served
    em.mea_labels(ONES, None, W)
    with pytest.raises(ValueError):
        em.mea_labels(ONES, None, np.eye(3))
    with pytest.raises(TypeError):
        hmm.EM_getMaxExpectedGainLabelsForList(object(), ONES)
    assert _same(good, em.mea_labels(TRACK_LEN, GEOMETRY_JOINED))     # and the context decodes as before
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunk_list(algo):
    full = synth.synthesize([50_000], 1000, 20_000, [20], seed=2)
    store = full.subset_chunks([])
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, full, synth.HIFI_ALPHA)
    em = _context(store, model, algo)
    labels, block, total = em.mea_labels(TRACK_LEN)
    assert labels.size == 0 and block.size == 0 and total == 0.0
    em.close()
