"""The VALUES of the posterior getters (hf_get_posterior, hf_multi_get_posterior, hf_batch_get_posterior) and the `trans` block of the
statistics against the float64 numpy forward-backward of tests/posterior_ref.py (pinned by tests/test_posterior_cpu.py): every entry
within rtol = 1e-9 (atol 1e-300: the bar the forward and backward vectors are held to against the oracle), exact zeros where the
reference has them.  Rows that sum to 1 and whose argmax is the label would also come out of a wrong scale, of swapped pos / pos_f records
or of a stale lazy re-run of the segment kernel; the values would not."""
import ctypes as C
import functools

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
import posterior_ref as PR

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 4097, 13_000]      # as tests/test_viterbi_gpu.py: tile and segment edges, 26 segments in one chunk
SCAN_CHUNKS = 100 + N.HF_ALGO_SCAN
ALGOS = [pytest.param(N.HF_ALGO_SEQ, id="seq"), pytest.param(N.HF_ALGO_SCAN, id="scan-rows"), pytest.param(SCAN_CHUNKS, id="scan-chunks")]
MODELS = [pytest.param(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, id="trunc_exp_gaussian"), pytest.param(N.HF_MODEL_GAUSSIAN, id="gaussian"),
          pytest.param(N.HF_MODEL_NEGATIVE_BINOMIAL, id="negative_binomial")]


def _sizes_store():
    store = synth.synthesize([n * 1000 for n in SIZES], 1000, 10 ** 9, [20], seed=11)
    assert sorted(np.diff(store.chunk_off).tolist()) == sorted(SIZES)
    return store


def _long_store():
    store = synth.synthesize([45_000_000, 256_000, 32_768_000], 1000, 60_000_000, [20], seed=21)
    assert sorted(np.diff(store.chunk_off).tolist()) == [256, 32768, 45000]
    return store


def _regions_store():
    store = synth.config(4, 0.03)
    assert store.n_regions == 7
    return store


GEOMETRY = {"sizes": (_sizes_store, synth.HIFI_ALPHA, 0.95, 3), "long": (_long_store, synth.HIFI_ALPHA, 0.95, 4),
            "regions": (_regions_store, synth.ONT_R10_ALPHA, 0.8, 6)}


def make_em(store, model, frac, algo):
    em = hmm.EMList(store, model, True, frac, algo=algo % 100)
    if algo >= 100:
        em.set_stats_mode(N.HF_STATS_CHUNKS)
        assert em.stats_mode == N.HF_STATS_CHUNKS
    return em


@functools.lru_cache(maxsize=None)
def _case(geometry, model_type):
    """(store, alpha, frac, K, parameters before, parameters after one M-step, reference posterior and trans block of the latter)."""
    make, alpha, frac, K = GEOMETRY[geometry]
    store = make()
    if model_type == N.HF_MODEL_NEGATIVE_BINOMIAL:
        alpha = np.zeros((4, 4))
    model = hmm.createModel(model_type, K, store, alpha)
    v0 = model.param_vector().copy()
    em = hmm.EMList(store, model, True, frac)
    hmm.EM_runOneIterationForList(em, model)
    hmm.HMM_estimateParameters(model, 1e-3)
    hmm.HMM_resetEstimators(model)
    em.close()
    v1 = model.param_vector().copy()
    assert not np.array_equal(v0, v1)
    post, trans, _, ll = PR.reference(store, model, alpha, True, frac)
    return store, alpha, frac, K, v0, v1, post, trans, float(ll.sum())


def _model(geometry, model_type, which):
    store, alpha, frac, K, v0, v1 = _case(geometry, model_type)[:6]
    model = hmm.createModel(model_type, K, store, alpha)
    model.set_param_vector(v1 if which else v0)
    return model


def _check_values(got, ref, what=""):
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    print("posterior %s: max relative error %.3g over %d entries above 1e-290, %d exact zeros in the reference"
          % (what, float(err[np.abs(ref) > 1e-290].max(initial=0.0)), int((np.abs(ref) > 1e-290).sum()), int((ref == 0).sum())))
    assert np.allclose(got, ref, rtol=1e-9, atol=1e-300), what
    assert np.all(got[ref == 0] == 0), what


def _check_trans(stats, geometry, model_type):
    """The `trans` block and the log-likelihood of a statistics vector at the E-step's bar against the oracle (tests/test_estep_gpu.py)."""
    store, _, _, K, _, _, _, trans, ll = _case(geometry, model_type)
    R = len(store.region_coverages)
    got = PR.trans_block(stats, R, _kmax(stats, R))
    scale = np.maximum(np.abs(trans), 1e-6 * np.abs(trans).max())
    assert np.all(np.abs(got - trans) <= 1e-9 * scale), float(np.max(np.abs(got - trans) / scale))
    assert abs(stats[0] - ll) <= 1e-9 * abs(ll), (stats[0], ll)


def _kmax(stats, R):
    return ((stats.size - 1) // R - 16) // 24


def _raw(fn, handle, *args):
    """The C getter itself with a range the Python wrappers cannot size a buffer for (a negative n): its return code."""
    buf = np.zeros(16, dtype=np.float64)
    return int(fn(handle, *args, buf.ctypes.data_as(C.POINTER(C.c_double))))


def _ranges(store):
    """Sub-ranges: across a chunk border, across a segment border (512 windows) inside the longest chunk, the two ends, nothing."""
    off = np.asarray(store.chunk_off, np.int64)
    n = int(off[-1])
    T = np.diff(off)
    c = int(np.argmax(T))
    border = int(off[1 + int(np.argmax(T[:-1] > 0))])
    out = [(border - 1, 2), (max(border - 40, 0), min(100, n - max(border - 40, 0))), (0, 1), (n - 1, 1), (n // 2, 0), (0, 0), (n, 0)]
    if T[c] > 512:
        out += [(int(off[c]) + 511, 2), (int(off[c]) + 500, 600 if T[c] > 1100 else int(T[c]) - 500)]
    return out


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type", MODELS)
@pytest.mark.parametrize("geometry", list(GEOMETRY))
def test_posterior_values_single_context(geometry, model_type, algo):
    """EMList.posterior after a SECOND pass with changed parameters (the getter of the first pass has already run its lazy block and
    left its records behind): the values of the second pass, the `trans` block of its statistics, every sub-range."""
    store, alpha, frac, K, v0, v1, ref, _, _ = _case(geometry, model_type)
    m0, m1 = _model(geometry, model_type, 0), _model(geometry, model_type, 1)
    em = make_em(store, m0, frac, algo)
    try:
        hmm.EM_runOneIterationForList(em, m0)
        first = em.posterior()
        assert not np.allclose(first, ref, rtol=1e-6, atol=1e-300)         # another model: the cases below can tell the passes apart
        hmm.EM_runOneIterationForList(em, m1)
        got = em.posterior()
        _check_values(got, ref, "%s/%s/%s" % (geometry, model_type, algo))
        assert np.array_equal(got.argmax(axis=1).astype(np.int8), em.labels())
        _check_trans(m1.estimators, geometry, model_type)
        for a, cnt in _ranges(store):
            part = em.posterior(a, cnt)
            assert part.shape == (cnt, 4) and np.array_equal(part, got[a:a + cnt]), (a, cnt)
    finally:
        em.close()


@pytest.mark.parametrize("stats_mode", [N.HF_STATS_ROWS, N.HF_STATS_CHUNKS], ids=["rows", "chunks"])
@pytest.mark.parametrize("env", [{"HF_SEG_LAUNCHES": "2"}, {"HF_SUBPASSES": "3"}], ids=["two launches", "three sub-passes"])
def test_posterior_values_under_the_environment_switches(env, stats_mode, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for geometry in ("sizes", "regions"):
        store, alpha, frac, K, v0, v1, ref, _, _ = _case(geometry, N.HF_MODEL_TRUNC_EXP_GAUSSIAN)
        m0, m1 = _model(geometry, 0, 0), _model(geometry, 0, 1)
        em = hmm.EMList(store, m0, True, frac)
        try:
            assert em.seg_launches == int(env.get("HF_SEG_LAUNCHES", 1)) and em.sub_passes == int(env.get("HF_SUBPASSES", 1))
            em.set_stats_mode(stats_mode)
            hmm.EM_runOneIterationForList(em, m0)
            em.posterior(3, 700)
            hmm.EM_runOneIterationForList(em, m1)
            got = em.posterior()
            _check_values(got, ref, "%s %s" % (geometry, env))
            _check_trans(m1.estimators, geometry, 0)
            for a, cnt in _ranges(store):
                assert np.array_equal(em.posterior(a, cnt), got[a:a + cnt]), (a, cnt)
        finally:
            em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_posterior_after_the_other_decoders_have_run(algo):
    """hf_viterbi, hf_sample_paths (both with OTHER parameters) and hf_get_interval_log_probs between the pass and the getter: the
    posterior is still the last full pass's, and the getter's lazy block run first does not go stale either."""
    geometry, mt = "sizes", N.HF_MODEL_TRUNC_EXP_GAUSSIAN
    store, alpha, frac, K, v0, v1, ref, _, _ = _case(geometry, mt)
    m0, m1 = _model(geometry, mt, 0), _model(geometry, mt, 1)
    em = make_em(store, m0, frac, algo)
    try:
        hmm.EM_runOneIterationForList(em, m0)
        em.posterior(0, 10)
        hmm.EM_runOneIterationForList(em, m1)
        hmm.EM_runViterbiForList(em, m0)
        hmm.EM_samplePathsForList(em, m0, 2, 77)
        n = store.n_windows
        hmm.EM_getIntervalLogProbsForList(em, [0, n // 2], [n - 1, n // 2 + 5], [15, 4])
        got = em.posterior()
        _check_values(got, ref, "after viterbi, sampling and intervals, algo %s" % algo)
        hmm.EM_runViterbiForList(em, m0)
        hmm.EM_samplePathsForList(em, m0, 1, 78)
        assert np.array_equal(em.posterior(), got)
        assert np.array_equal(em.posterior(n - 700, 700), got[n - 700:])
    finally:
        em.close()


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("geometry", ["sizes", "regions"])
def test_posterior_values_sharded(geometry, world):
    """MultiEMList.posterior (loopback ranks on one device): ranges that lie in one shard, span shards, and the whole list."""
    mt = N.HF_MODEL_TRUNC_EXP_GAUSSIAN
    store, alpha, frac, K, v0, v1, ref, _, _ = _case(geometry, mt)
    m0, m1 = _model(geometry, mt, 0), _model(geometry, mt, 1)
    m = hmm.MultiEMList(store, m0, world, True, frac, exchange=N.HF_EXCHANGE_CHUNKS, transport=N.HF_TRANSPORT_LOOPBACK)
    try:
        m.run_sharded(m0, N.HF_MODE_FULL)
        m.posterior(0, min(50, store.n_windows))
        stats = m.run_sharded(m1, N.HF_MODE_FULL)
        got = m.posterior()
        _check_values(got, ref, "%s, %d ranks" % (geometry, world))
        _check_trans(stats, geometry, mt)
        assert np.array_equal(got.argmax(axis=1).astype(np.int8), m.labels())
        for a, cnt in _ranges(store):
            assert np.array_equal(m.posterior(a, cnt), got[a:a + cnt]), (a, cnt)
        bounds = np.cumsum([0] + [w for _, w in m.shard_sizes()])
        n = store.n_windows
        for b in bounds[1:-1]:
            a, cnt = max(int(b) - 3, 0), min(6, n - max(int(b) - 3, 0))
            assert np.array_equal(m.posterior(a, cnt), got[a:a + cnt]), (a, cnt)
        for a, cnt in ((-1, 2), (0, n + 1), (n, 1)):
            with pytest.raises(hmm.MultiHFError):
                m.posterior(a, cnt)
        assert _raw(N.lib().hf_multi_get_posterior, m._h, 5, -1) == N.HF_E_ARG
        m.run_sharded(m1, N.HF_MODE_FORWARD_ONLY)
        with pytest.raises(hmm.MultiHFError):
            m.posterior(0, 4)
    finally:
        m.close()


def _alphas():
    rnd = np.random.default_rng(4242).uniform(0.0, 1.0, (4, 4))
    return [synth.HIFI_ALPHA, np.zeros((4, 4)), synth.ONT_R10_ALPHA, rnd]


@pytest.mark.parametrize("stats_mode", [N.HF_STATS_ROWS, N.HF_STATS_CHUNKS], ids=["rows", "chunks"])
@pytest.mark.parametrize("geometry", ["sizes", "regions"])
def test_posterior_values_batched(geometry, stats_mode):
    """EMBatch.posterior of four models with their own alpha (the shared launch in the rows mode, a pass of its own per model in the
    chunks mode), after a second pass with changed parameters, each against its own reference."""
    make, _, frac, K = GEOMETRY[geometry]
    store = make()
    models = [hmm.createModel(N.HF_MODEL_TRUNC_EXP_GAUSSIAN if i != 2 else N.HF_MODEL_GAUSSIAN, K, store, a) for i, a in enumerate(_alphas())]
    em = hmm.EMList(store, models[0], True, frac)
    em.set_stats_mode(stats_mode)
    batch = hmm.EMBatch(em, models)
    try:
        status = hmm.EM_runBatchForList(batch)
        assert (status == N.HF_OK).all()
        for m in range(4):
            batch.posterior(m, 0, 5)
            hmm.HMM_estimateParameters(models[m], 1e-3)
            hmm.HMM_resetEstimators(models[m])
        status = hmm.EM_runBatchForList(batch)
        assert (status == N.HF_OK).all()
        assert batch.shared_models == (4 if stats_mode == N.HF_STATS_ROWS else 0)
        R = len(store.region_coverages)
        for m, a in enumerate(_alphas()):
            ref, trans, _, ll = PR.reference(store, models[m], a, True, frac)
            got = batch.posterior(m)
            _check_values(got, ref, "%s, model %d" % (geometry, m))
            assert np.array_equal(got.argmax(axis=1).astype(np.int8), batch.labels(m))
            st = models[m].estimators
            tb = PR.trans_block(st, R, _kmax(st, R))
            scale = np.maximum(np.abs(trans), 1e-6 * np.abs(trans).max())
            assert np.all(np.abs(tb - trans) <= 1e-9 * scale), m
            assert abs(st[0] - ll.sum()) <= 1e-9 * abs(ll.sum())
            for a0, cnt in _ranges(store):
                assert np.array_equal(batch.posterior(m, a0, cnt), got[a0:a0 + cnt]), (m, a0, cnt)
    finally:
        batch.close()
        em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_refusals(algo):
    """A bad range, a getter after a forward-only pass and before any pass: HF_E_ARG, and the context goes on."""
    geometry, mt = "sizes", N.HF_MODEL_TRUNC_EXP_GAUSSIAN
    store, alpha, frac, K, v0, v1, ref, _, _ = _case(geometry, mt)
    m1 = _model(geometry, mt, 1)
    n = store.n_windows
    em = make_em(store, m1, frac, algo)
    try:
        with pytest.raises(N.HFError) as ei:
            em.posterior(0, 4)                               # no pass yet
        assert ei.value.code == N.HF_E_ARG
        hmm.EM_runOneIterationForList(em, m1)
        for a, cnt in ((-1, 2), (0, n + 1), (n, 1), (n - 1, 2), (-3, 0)):
            with pytest.raises(N.HFError) as ei:
                em.posterior(a, cnt)
            assert ei.value.code == N.HF_E_ARG, (a, cnt)
        assert _raw(N.lib().hf_get_posterior, em._h, 5, -1) == N.HF_E_ARG           # (sized its buffers by n before the range check once)
        assert _raw(N.lib().hf_get_posterior, em._h, n, -2) == N.HF_E_ARG
        got = em.posterior()
        _check_values(got, ref, "after the refusals")
        hmm.EM_runForwardForList(em, m1)
        with pytest.raises(N.HFError) as ei:
            em.posterior(0, 4)
        assert ei.value.code == N.HF_E_ARG
        hmm.EM_runOneIterationForList(em, m1)
        assert np.array_equal(em.posterior(), got)
    finally:
        em.close()


def test_refusals_batched():
    geometry, mt = "sizes", N.HF_MODEL_TRUNC_EXP_GAUSSIAN
    store, alpha, frac, K, v0, v1, ref, _, _ = _case(geometry, mt)
    models = [_model(geometry, mt, 1) for _ in range(3)]
    n = store.n_windows
    batch = hmm.EMBatch(store, models, True, frac)
    try:
        stats, status = batch.estep(active=[0, 2])
        assert (status == N.HF_OK).all()
        with pytest.raises(N.HFError) as ei:
            batch.posterior(1)                               # a model that has never run
        assert ei.value.code == N.HF_E_ARG
        with pytest.raises(N.HFError):
            batch.labels(1)
        for m in (-1, 3):
            with pytest.raises(N.HFError):
                batch.posterior(m, 0, 1)
        for a, cnt in ((-1, 2), (0, n + 1), (n, 1)):
            with pytest.raises(N.HFError) as ei:
                batch.posterior(0, a, cnt)
            assert ei.value.code == N.HF_E_ARG, (a, cnt)
        assert _raw(N.lib().hf_batch_get_posterior, batch._b, 0, 5, -1) == N.HF_E_ARG
        for m in (0, 2):
            _check_values(batch.posterior(m), ref, "batch model %d" % m)
        stats, status = batch.estep(active=[2], mode=N.HF_MODE_FORWARD_ONLY)
        assert status[0] == N.HF_OK
        with pytest.raises(N.HFError):
            batch.posterior(2, 0, 4)
        _check_values(batch.posterior(0), ref, "the model beside a forward-only one")
    finally:
        batch.close()
