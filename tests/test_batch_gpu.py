"""Many models on one context (hf_batch_*, hmm.EMBatch, hmm_flagger --sweepAlpha): every model of a batched pass holds the bits of the
same model's hf_estep on a single context, agrees with the oracle, and leaves the other models and the context alone — over the stores,
switches and modes the single path is tested with (tests/test_estep_gpu.py), more models than one launch of k_seg_fb_batch takes, the
hand-off epochs and the hand-off time-out."""
import os
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from oracle_py import Oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
GOLDEN = os.path.join(ROOT, "tests", "golden")
ALPHA_HIFI = os.path.join(GOLDEN, "alpha_hifi.tsv")
ALPHA_ONT = os.path.join(GOLDEN, "alpha_ont_r10.tsv")


def _alphas():
    rnd = np.random.default_rng(4242).uniform(0.0, 1.0, (4, 4))
    return [np.loadtxt(ALPHA_HIFI), np.zeros((4, 4)), np.loadtxt(ALPHA_ONT), rnd]


def _small_store(seed=3):
    return synth.synthesize([2_500_000, 1_300_000, 700_000], 4000, 1_500_000, [20, 30], seed=seed)


def _single(em, model):
    """The single path: hf_estep + hf_finish on the context, then its labels."""
    hmm.EM_runOneIterationForList(em, model)
    return model.estimators.copy(), em.labels()


def _expected_shared(em, n):
    """Models whose segment kernel runs in the shared launch: all of them on the default pass (one launch, statistics by row, one sub-pass)."""
    return n if (em.stats_mode == N.HF_STATS_ROWS and em.seg_launches == 1 and em.sub_passes == 1) else 0


def _models(store, model_type, K, alphas):
    return [hmm.createModel(model_type, K, store, a) for a in alphas]


def _check_identity(store, model_type, iters=2):
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    alphas = _alphas()
    models = _models(store, model_type, K, alphas)
    em = hmm.EMList(store, models[0])
    batch = hmm.EMBatch(em, models)
    assert batch.capacity() >= len(models)
    for _ in range(iters):
        stats, status = batch.estep()
        assert (status == N.HF_OK).all(), status
        assert batch.shared_models == _expected_shared(em, len(models))   # one launch of k_seg_fb_batch served every model
        for m, model in enumerate(models):
            ref, lab = _single(em, model)
            assert np.array_equal(stats[m], ref), (m, np.max(np.abs(stats[m] - ref)))
            assert np.array_equal(batch.labels(m), lab), m
            hmm.HMM_estimateParameters(model, 1e-3)
            hmm.HMM_resetEstimators(model)
    batch.close()
    em.close()


@pytest.mark.parametrize("model_type", [N.HF_MODEL_TRUNC_EXP_GAUSSIAN, N.HF_MODEL_GAUSSIAN])
def test_bit_identity_small(model_type):
    _check_identity(_small_store(), model_type)


@pytest.mark.parametrize("model_type", [N.HF_MODEL_TRUNC_EXP_GAUSSIAN, N.HF_MODEL_GAUSSIAN])
def test_bit_identity_config2(model_type):
    store = synth.config(2, 1.0)
    em = hmm.EMList(store, hmm.createModel(model_type, 6, store, np.zeros((4, 4))))
    assert _expected_shared(em, 1) == 1                # the default pass: the shared launch is what is tested here
    em.close()
    _check_identity(store, model_type, iters=1)


@pytest.mark.parametrize("model_type", [N.HF_MODEL_TRUNC_EXP_GAUSSIAN, N.HF_MODEL_GAUSSIAN])
def test_against_the_oracle(model_type):
    store = _small_store(5)
    K = hmm.getBestNumberOfCollapsedComps(store)
    alphas = _alphas()
    models = _models(store, model_type, K, alphas)
    batch = hmm.EMBatch(store, models)
    status = hmm.EM_runBatchForList(batch)
    assert (status == N.HF_OK).all(), status
    for m, a in enumerate(alphas):
        orc = Oracle(store, model_type, K, a)
        assert orc.run_iteration() == 0
        ref = orc.stats_vector(models[m].maxNumberOfComps)
        got = models[m].estimators
        assert abs(got[0] - ref[0]) <= 1e-9 * abs(ref[0]), (m, got[0], ref[0])
        assert np.allclose(got, ref, rtol=1e-8, atol=1e-12), m
        assert (batch.labels(m) == orc.labels()).all(), m
    batch.close()


def test_active_subset():
    store = _small_store(7)
    K = hmm.getBestNumberOfCollapsedComps(store)
    models = _models(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, K, _alphas())
    em = hmm.EMList(store, models[0])
    batch = hmm.EMBatch(em, models)
    stats0, status = batch.estep()
    assert (status == N.HF_OK).all()
    labels0 = [batch.labels(m) for m in range(4)]
    for m in (1, 3):
        models[m].estimators = stats0[m]
        hmm.HMM_estimateParameters(models[m], 1e-3)
        hmm.HMM_resetEstimators(models[m])
    stats, status = batch.estep(active=[3, 1])
    assert (status == N.HF_OK).all() and stats.shape[0] == 2
    for i, m in enumerate((3, 1)):
        ref, lab = _single(em, models[m])
        assert np.array_equal(stats[i], ref)
        assert np.array_equal(batch.labels(m), lab)
    for m in (0, 2):
        assert np.array_equal(batch.labels(m), labels0[m])
    batch.close()
    em.close()


@pytest.mark.parametrize("launches", ["1", "2"])
def test_launch_modes(launches, monkeypatch):
    monkeypatch.setenv("HF_SEG_LAUNCHES", launches)
    store = _small_store(9)
    K = hmm.getBestNumberOfCollapsedComps(store)
    models = _models(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, K, _alphas())
    em = hmm.EMList(store, models[0])
    assert em.seg_launches == int(launches)
    if launches == "1":
        assert em.seg_cached_steps > 0         # a store this small runs the CACHED variant of k_seg_fb
    batch = hmm.EMBatch(em, models)
    stats, status = batch.estep()
    assert (status == N.HF_OK).all()
    assert batch.shared_models == _expected_shared(em, len(models))   # two launches: each model runs its own pass
    for m, model in enumerate(models):
        ref, lab = _single(em, model)
        assert np.array_equal(stats[m], ref) and np.array_equal(batch.labels(m), lab), m
    batch.close()
    em.close()


def test_a_failing_model_is_isolated():
    store = _small_store(11)
    K = hmm.getBestNumberOfCollapsedComps(store)
    models = _models(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, K, _alphas())
    v = models[2].param_vector()
    v[:] = np.nan
    models[2].set_param_vector(v)
    em = hmm.EMList(store, models[0])
    batch = hmm.EMBatch(em, models)
    stats, status = batch.estep()
    # the single path's verdict on the same parameters
    em_bad = hmm.EMList(store, models[0])
    em_bad.launch(models[2])
    with pytest.raises(N.HFError) as ei:
        em_bad.finish()
    assert status[2] == ei.value.code, (status, ei.value.code)
    assert status[2] in (N.HF_E_NAN, N.HF_E_SCALE)
    em_bad.close()
    for m in (0, 1, 3):
        assert status[m] == N.HF_OK
        ref, lab = _single(em, models[m])
        assert np.array_equal(stats[m], ref) and np.array_equal(batch.labels(m), lab), m
    # the context under the batch still answers as a fresh one
    fresh = hmm.EMList(store, models[0])
    a, la = _single(em, models[0])
    b, lb = _single(fresh, models[0])
    assert np.array_equal(a, b) and np.array_equal(la, lb)
    fresh.close()
    batch.close()
    em.close()


def test_refusals(monkeypatch):
    store = _small_store(13)
    K = hmm.getBestNumberOfCollapsedComps(store)
    model = hmm.createModel(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
    L = N.lib()
    seq = hmm.EMList(store, model, algo=N.HF_ALGO_SEQ)
    assert L.hf_batch_capacity(seq._h) == 0
    with pytest.raises(N.HFError):
        hmm.EMBatch(seq, [model, model])
    seq.close()
    nbm = hmm.createModel(N.HF_MODEL_NEGATIVE_BINOMIAL, K, store, np.zeros((4, 4)))
    em = hmm.EMList(store, nbm)
    batch = hmm.EMBatch(em, [model])
    with pytest.raises(N.HFError):                    # a negative_binomial pass is refused by the batch
        batch.estep(models=[nbm])
    batch.close()
    hmm.EM_runOneIterationForList(em, nbm)
    assert L.hf_batch_capacity(em._h) == 0            # ... and a context that has run one cannot carry a batch
    with pytest.raises(N.HFError):
        hmm.EMBatch(em, [model])
    em.close()
    monkeypatch.setenv("HF_SUBPASSES", "3")
    sub = hmm.EMList(store, model)
    assert sub.sub_passes == 3
    assert L.hf_batch_capacity(sub._h) == 0
    with pytest.raises(N.HFError):
        hmm.EMBatch(sub, [model])
    sub.close()


# ---- the single path's coverage, through the batch ------------------------------------------------------------------------------

def _check_geometry(store, model_type, K, adjust=True, frac=0.95, stats_mode=None, context_check=None):
    """One batch of the four _alphas() models, two EM passes: every model holds the bits (statistics, labels, posterior) of the single
    path on a fresh context, agrees with the oracle at this file's bars, and the shared launch served whom it should."""
    alphas = _alphas()
    models = _models(store, model_type, K, alphas)
    em = hmm.EMList(store, models[0], adjust, frac)
    fresh = hmm.EMList(store, models[0], adjust, frac)
    if stats_mode is not None:
        em.set_stats_mode(stats_mode)
        fresh.set_stats_mode(stats_mode)
    if context_check is not None:
        context_check(em)
    batch = hmm.EMBatch(em, models)
    orcs = [Oracle(store, model_type, K, a, 0.25, 0.75, adjust, frac, threads=8) for a in alphas]
    try:
        assert batch.capacity() >= len(models)
        for it in range(2):
            stats, status = batch.estep()
            assert (status == N.HF_OK).all(), status
            assert batch.shared_models == _expected_shared(em, len(models))
            for m, model in enumerate(models):
                ref, lab = _single(fresh, model)
                assert np.array_equal(stats[m], ref), (it, m, np.max(np.abs(stats[m] - ref)))
                assert np.array_equal(batch.labels(m), lab), (it, m)
                assert np.array_equal(batch.posterior(m), fresh.posterior()), (it, m)
                orc = orcs[m]
                orc.set_param_vector(model.param_vector())
                assert orc.run_iteration() == 0
                o = orc.stats_vector(model.maxNumberOfComps)
                assert abs(stats[m][0] - o[0]) <= 1e-9 * abs(o[0]), (it, m, stats[m][0], o[0])
                assert np.allclose(stats[m], o, rtol=1e-8, atol=1e-12), (it, m, np.max(np.abs(stats[m] - o) / (1e-12 + 1e-8 * np.abs(o))))
                assert (lab == orc.labels()).all(), (it, m)
                hmm.HMM_estimateParameters(model, 1e-3)
                hmm.HMM_resetEstimators(model)
        return batch.shared_models
    finally:
        for orc in orcs:
            orc.close()
        batch.close()
        fresh.close()
        em.close()


def _ragged_store():
    W = 100
    lens = [1 * W, 2 * W, 3 * W, 63 * W, 64 * W, 65 * W, 129 * W, 1000 * W + 37, 5 * W - 1, 2049 * W]
    store = synth.synthesize(lens, W, 10_000_000, [20, 25], seed=5, region_run_bases=(2_000, 30_000))
    assert sorted(np.diff(store.chunk_off))[:3] == [1, 2, 3]
    return store, 3, True, 0.95


def _long_store():
    store = synth.synthesize([45_000_000, 256_000, 32_768_000], 1000, 60_000_000, [20], seed=21)
    assert sorted(np.diff(store.chunk_off).tolist()) == [256, 32768, 45000]          # 88 segments: more than HF_SEG_PSTAGE = 24
    return store, 4, True, 0.95


def _seven_regions_store():
    store = synth.config(4, 0.03)
    assert store.n_regions == 7 and len(np.unique(store.regions())) > 3
    return store, hmm.getBestNumberOfCollapsedComps(store), True, 0.8


def _compact_plan_store():
    store = synth.config(5, 0.01)       # coverage over 0..250 in 7 regions: nearly every window has its own emission row
    K = hmm.getBestNumberOfCollapsedComps(store)
    assert K == 10 and store.n_regions == 7 and int(store.cov.max()) == 250
    return store, K, True, 0.8


def _all_regions_store():
    store = synth.synthesize([600_000, 90_000], 1000, 100_000, [20 + (i % 7) for i in range(64)], seed=5, region_run_bases=(3_000, 20_000))
    assert len(np.unique(store.annot >> np.uint64(58))) > 12 and int((store.annot >> np.uint64(58)).max()) > 60
    return store, 16, True, 0.95


def _thirteen_components_store():
    return synth.config(2, 0.01), 13, True, 0.95      # K >= 13: the parameter block no longer fits k_tables' kernel arguments


def _long_reads_store(adjust):
    return synth.synthesize([700_000, 90_000, 4_100], 1000, 200_000, [20], seed=11, avg_alignment_len=200000), 4, adjust, 0.95


GEOMETRIES = {"ragged and one-window chunks": _ragged_store, "88 segments in a chunk": _long_store, "seven regions": _seven_regions_store,
              "compact statistics plan": _compact_plan_store, "64 regions, 16 components": _all_regions_store,
              "13 components": _thirteen_components_store, "reads longer than chunks, adjusted": lambda: _long_reads_store(True),
              "reads longer than chunks, not adjusted": lambda: _long_reads_store(False)}


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_geometries_of_the_single_path(geometry):
    store, K, adjust, frac = GEOMETRIES[geometry]()

    def check(em):
        assert em.seg_launches == 1 and em.stats_mode == N.HF_STATS_ROWS and em.sub_passes == 1
        if geometry.startswith("64 regions"):
            assert em.seg_cached_steps == 8       # nine row blocks of 8 KiB: the dynamic LDS request of k_seg_fb_batch is above 64 KiB
    assert _check_geometry(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, K, adjust, frac, context_check=check) == 4


def _segments(store):
    return int(sum(-(-int(t) // 512) for t in np.diff(store.chunk_off)))


SWITCHES = {
    "no cached row blocks": ({"HF_SEG_CACHED_STEPS": "0"}, lambda em: em.seg_launches == 1 and em.seg_cached_steps == 0),
    "three cached row blocks": ({"HF_SEG_CACHED_STEPS": "3"}, lambda em: em.seg_launches == 1 and em.seg_cached_steps == 3),
    "a device that holds just the segments": ({"HF_SEG_RESIDENT": "segments"}, lambda em: em.seg_launches == 1 and em.seg_cached_steps == 0),
    "parameter copy": ({"HF_PARAMS_COPY": "1"}, lambda em: em.n_regions == 1),
    "device total": ({"HF_TOTAL": "device"}, lambda em: True),
    "compact plan, three batches": ({"HF_STATS_PLAN": "compact,bpw=3"}, lambda em: True),
    "padded plan, two batches": ({"HF_STATS_PLAN": "padded,bpw=2"}, lambda em: True),
}


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_switches_of_the_single_path(switch, monkeypatch):
    """The switches hf_create reads, on the context under the batch and on the fresh single context alike."""
    env, ok = SWITCHES[switch]
    store = synth.config(2, 0.05)
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    for k, v in env.items():
        monkeypatch.setenv(k, str(_segments(store)) if v == "segments" else v)

    def check(em):
        assert ok(em), switch
    assert _check_geometry(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, K, context_check=check) == 4


@pytest.mark.parametrize("model_type", [N.HF_MODEL_TRUNC_EXP_GAUSSIAN, N.HF_MODEL_GAUSSIAN])
def test_per_chunk_statistics_mode(model_type):
    """The mode set on the context before the batch is made: no model joins the shared launch, the bits are the single path's."""
    store = synth.config(4, 0.03)
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    assert _check_geometry(store, model_type, K, True, 0.8, stats_mode=N.HF_STATS_CHUNKS) == 0


def test_forward_only_through_the_batch():
    store = _small_store(15)
    K = hmm.getBestNumberOfCollapsedComps(store)
    models = _models(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, K, _alphas())
    em = hmm.EMList(store, models[0])
    fresh = hmm.EMList(store, models[0])
    batch = hmm.EMBatch(em, models)
    try:
        full, status = batch.estep()
        assert (status == N.HF_OK).all() and batch.shared_models == 4
        posts = [batch.posterior(m) for m in range(4)]
        fwd, status = batch.estep(mode=N.HF_MODE_FORWARD_ONLY)
        assert (status == N.HF_OK).all() and batch.shared_models == 0
        for m, model in enumerate(models):
            assert fwd[m][0] == full[m][0], (m, fwd[m][0], full[m][0])
            hmm.EM_runForwardForList(fresh, model)
            assert model.loglikelihood == fwd[m][0], m
            with pytest.raises(N.HFError) as ei:
                batch.labels(m)
            assert ei.value.code == N.HF_E_ARG
            with pytest.raises(N.HFError) as ei:
                batch.posterior(m)
            assert ei.value.code == N.HF_E_ARG
        # forward-only for two models only: the others keep their full pass
        full2, status = batch.estep()
        assert np.array_equal(full2, full)
        batch.estep(active=[2, 0], mode=N.HF_MODE_FORWARD_ONLY)
        for m in (1, 3):
            assert np.array_equal(batch.posterior(m), posts[m])
        for m in (0, 2):
            with pytest.raises(N.HFError):
                batch.posterior(m)
    finally:
        batch.close(); fresh.close(); em.close()


def _multi_segment(store):
    """Mask over the context's segments (ceil(T / 512) per chunk, in chunk order): those of chunks with more than one segment — the ones
    that publish a product and a flag word."""
    nseg = [-(-int(t) // 512) for t in np.diff(store.chunk_off)]
    return np.repeat(np.array(nseg) > 1, nseg)


def test_hand_off_epochs_advance_by_the_batch():
    """Every model has hand-off flags and an epoch counter of its own.  A shared launch advances the epoch of each model in it by one and
    stamps the model's flags with it; a model that sits a pass out keeps both.  After passes of different subsets the models' epochs all
    differ: an epoch taken from another model's row of the launch table, or one not advanced, shows in the flag words themselves (the
    results alone would only show it when a segment happens to overtake the one it waits for)."""
    store = synth.synthesize([2_500_000, 1_300_000, 700_000, 9_000_000], 4000, 10 ** 9, [20, 30], seed=23)   # 1 + 1 + 1 + 5 segments
    multi = _multi_segment(store)
    assert multi.sum() >= 5 and (~multi).sum() >= 2
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    models = _models(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, K, _alphas())
    em = hmm.EMList(store, models[0])
    fresh = hmm.EMList(store, models[0])
    batch = hmm.EMBatch(em, models)
    try:
        assert em.seg_launches == 1
        want = [0, 0, 0, 0]
        for m in range(4):
            epoch, flags = batch.handoff(m)
            assert epoch == 0 and flags.size == multi.size and not flags.any()
        for act in ([0, 1, 2, 3], [3, 1], [1], [2, 3, 1], [0, 1, 2, 3]):
            stats, status = batch.estep(active=act)
            assert (status == N.HF_OK).all() and batch.shared_models == len(act)
            for m in act:
                want[m] += 1
            for m in range(4):
                epoch, flags = batch.handoff(m)
                assert epoch == want[m], (act, m, epoch, want)
                assert (flags[multi] == want[m]).all() and not flags[~multi].any(), (act, m, flags, want)
            for i, m in enumerate(act):
                ref, lab = _single(fresh, models[m])
                assert np.array_equal(stats[i], ref) and np.array_equal(batch.labels(m), lab), (act, m)
        assert len(set(want)) == 4, want
        # a getter's lazy re-run of the segment kernel is one more launch of that model alone
        batch.posterior(2, 0, 10)
        epoch, flags = batch.handoff(2)
        assert epoch == want[2] + 1 and (flags[multi] == epoch).all()
        assert batch.handoff(0)[0] == want[0]
        with pytest.raises(N.HFError):
            batch.handoff(4)
    finally:
        batch.close(); fresh.close(); em.close()


@pytest.mark.parametrize("n_models", [65, 130])
def test_more_models_than_one_launch_takes(n_models):
    """HF_SEG_BATCH_MAX = 64 models per launch of k_seg_fb_batch: a pass of 65 or 130 models is two or three launches, each with its own
    table of models and epochs; an active subset in shuffled order takes models from both sides of index 64 into one launch."""
    store = _small_store(17)
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    rng = np.random.default_rng(6400 + n_models)
    alphas = rng.uniform(0.0, 0.9, (n_models, 4, 4))
    models = _models(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, K, alphas)
    em = hmm.EMList(store, models[0])
    fresh = hmm.EMList(store, models[0])
    assert N.lib().hf_batch_capacity(em._h) >= 130
    batch = hmm.EMBatch(em, models)
    try:
        stats, status = batch.estep()
        assert (status == N.HF_OK).all() and batch.shared_models == n_models
        assert len({stats[m].tobytes() for m in range(n_models)}) == n_models          # every model has an answer of its own
        labels = []
        for m, model in enumerate(models):
            ref, lab = _single(fresh, model)
            assert np.array_equal(stats[m], ref), m
            assert np.array_equal(batch.labels(m), lab), m
            if m in (0, 63, 64, n_models - 1):
                assert np.array_equal(batch.posterior(m), fresh.posterior()), m
            labels.append(lab)
        n_act = 10 if n_models == 65 else 100
        act = np.concatenate([rng.choice(64, n_act // 2, replace=False), 64 + rng.choice(n_models - 64, min(n_act // 2, n_models - 64), replace=False)])
        act = rng.permutation(act).astype(np.int32)
        assert (act < 64).any() and (act >= 64).any() and not np.array_equal(act, np.sort(act))
        for m in act:
            hmm.HMM_estimateParameters(models[m], 1e-3)
            hmm.HMM_resetEstimators(models[m])
        stats2, status = batch.estep(active=act)
        assert (status == N.HF_OK).all() and batch.shared_models == act.size and stats2.shape[0] == act.size
        for i, m in enumerate(act):
            ref, lab = _single(fresh, models[m])
            assert np.array_equal(stats2[i], ref) and not np.array_equal(ref, stats[m]), m
            assert np.array_equal(batch.labels(int(m)), lab), m
            assert np.array_equal(batch.posterior(int(m)), fresh.posterior()), m
        for m in sorted(set(range(n_models)) - set(act.tolist())):
            assert np.array_equal(batch.labels(m), labels[m]), m
    finally:
        batch.close(); fresh.close(); em.close()


_TIMEOUT = r"""
import os, sys, json, hashlib, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from flagger_amd import hmm, synth, _native as N
from test_batch_gpu import _small_store, _alphas, _models, _single
store = _small_store(19)
K = hmm.getBestNumberOfCollapsedComps(store)
models = _models(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, K, _alphas())
em = hmm.EMList(store, models[0])
batch = hmm.EMBatch(em, models)
out = {"launches_at_create": em.seg_launches}
stats, status = batch.estep()
out["status"], out["shared"] = status.tolist(), batch.shared_models
out["stats"] = stats.tolist()
out["labels"] = [hashlib.sha1(batch.labels(m).tobytes()).hexdigest() for m in range(4)]
out["posterior"] = [hashlib.sha1(batch.posterior(m).tobytes()).hexdigest() for m in range(4)]
for m in range(4):
    models[m].estimators = stats[m]
    hmm.HMM_estimateParameters(models[m], 1e-3)
    hmm.HMM_resetEstimators(models[m])
stats2, status2 = batch.estep()
out["status2"], out["shared2"], out["stats2"] = status2.tolist(), batch.shared_models, stats2.tolist()
out["labels2"] = [hashlib.sha1(batch.labels(m).tobytes()).hexdigest() for m in range(4)]
out["context_launches"] = em.seg_launches
for k in ("HF_SEG_TEST_TIMEOUT", "HF_SEG_LAUNCHES"):
    os.environ.pop(k, None)
fresh = hmm.EMList(store, models[0])              # a single context beside the batch: one launch, nothing timed out
out["fresh_launches"] = fresh.seg_launches
same = True
for m in range(4):
    ref, lab = _single(fresh, models[m])
    same = same and bool(np.array_equal(ref, stats2[m])) and hashlib.sha1(lab.tobytes()).hexdigest() == out["labels2"][m]
out["fresh_same"], out["fresh_launches_after"] = same, fresh.seg_launches
print(json.dumps(out))
batch.close(); fresh.close(); em.close()
"""


def _timeout_run(env):
    import json
    import sys
    r = subprocess.run([sys.executable, "-c", _TIMEOUT % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       env=dict(os.environ, **env), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]), r.stderr


def test_hand_off_time_out_in_the_shared_launch():
    """DESIGN.md 7b.  HF_SEG_TEST_TIMEOUT=1: every model's first one-launch pass — here the shared launch — waits for flags nobody writes.
    Each model's flag word alone carries the time-out, hf_batch_finish re-runs that model's pass in two launches and the caller sees an
    ordinary result: the bits of a batch that ran two launches from the start.  The models stay in two-launch mode (no shared launch
    afterwards); the context's own pass and a fresh single context are not touched.  (One run: the waits are bounded.)"""
    a, err_a = _timeout_run({"HF_SEG_TEST_TIMEOUT": "1"})
    b, err_b = _timeout_run({"HF_SEG_LAUNCHES": "2"})
    assert a["status"] == [N.HF_OK] * 4 and a["status2"] == [N.HF_OK] * 4
    assert err_a.count("falls back to k_seg_prod + k_seg_fb") == 4, err_a[-2000:]        # one line per model
    assert "falls back" not in err_b
    assert a["launches_at_create"] == 1 and b["launches_at_create"] == 2
    assert a["shared"] == 4 and a["shared2"] == 0 and b["shared"] == 0 and b["shared2"] == 0
    for k in ("stats", "labels", "posterior", "stats2", "labels2"):
        assert a[k] == b[k], k
    assert a["context_launches"] == 1                       # the context's own pass is never written by a batch
    assert a["fresh_launches"] == 1 and a["fresh_launches_after"] == 1 and a["fresh_same"] and b["fresh_same"]


def test_empty_chunk_list_carries_no_batch():
    full = synth.synthesize([50_000], 1000, 20_000, [20], seed=2)
    store = full.subset_chunks([])
    model = hmm.createModel(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, full, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model)
    assert N.lib().hf_batch_capacity(em._h) == 0
    with pytest.raises(N.HFError) as ei:
        hmm.EMBatch(em, [model, model])
    assert ei.value.code == N.HF_E_ARG
    hmm.EM_runOneIterationForList(em, model)               # the context itself goes on
    assert model.loglikelihood == 0.0
    em.close()


# ---- command line --------------------------------------------------------------------------------------------------------------

def _cli(args, out, ok=True):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


def _tree(d):
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def _sweep_against_separate_runs(tmp_path, extra, engine):
    zeros = tmp_path / "alpha_zero.tsv"
    zeros.write_text("\n".join(["0\t0\t0\t0"] * 4) + "\n")
    tsvs = [ALPHA_HIFI, str(zeros), ALPHA_ONT]
    lst = tmp_path / "list.txt"
    lst.write_text("# three candidates\n" + "\n".join(tsvs) + "\n")
    inp = os.path.join(GOLDEN, "sim_gaussian_30k.bin")
    base = ["-i", inp, "-P", "--viterbi"] + extra
    r = _cli(base + ["--sweepAlpha", str(lst)], tmp_path / "sweep")
    assert "--sweepAlpha: 3 candidates on one loaded input, engine: " + engine in r.stderr, r.stderr[-1500:]
    assert r.stderr.count("Parsing/Creating coverage chunks") == 1
    rows = [l.split("\t") for l in (tmp_path / "sweep" / "alpha_sweep.tsv").read_text().splitlines() if not l.startswith("#")]
    assert len(rows) == 3
    for i, tsv in enumerate(tsvs):
        sep = tmp_path / ("sep%d" % i)
        _cli(base + ["--alphaTsv", tsv], sep)
        a, b = _tree(tmp_path / "sweep" / ("alpha_%d" % (i + 1))), _tree(sep)
        assert sorted(a) == sorted(b)
        for n in b:
            assert a[n] == b[n], (i, n)
        ll = [l.split("\t") for l in (sep / "loglikelihood.tsv").read_text().splitlines()[1:]]
        assert rows[i][0] == str(i + 1) and rows[i][1] == tsv
        assert rows[i][4] == ll[-1][2] and rows[i][5] == "ok"
        assert int(rows[i][2]) == int(ll[-1][0])


def test_cli_sweep_plain_em(tmp_path):
    _sweep_against_separate_runs(tmp_path, ["-n", "100"], "batched (hf_batch), 3 models per group")


def test_cli_sweep_accelerated(tmp_path):
    _sweep_against_separate_runs(tmp_path, ["-n", "20", "--accelerate"], "sequential (one context)")


def test_cli_sweep_more_candidates_than_one_launch_takes(tmp_path):
    """66 candidates in one group: every pass of the sweep is two launches of k_seg_fb_batch until candidates converge.  Candidates 1,
    64, 65 and 66 against separate --alphaTsv runs, file by file."""
    rng = np.random.default_rng(66)
    tsvs = []
    for i in range(66):
        p = tmp_path / ("alpha_in_%02d.tsv" % (i + 1))
        p.write_text("\n".join("\t".join("%.6f" % v for v in row) for row in rng.uniform(0.0, 0.8, (4, 4))) + "\n")
        tsvs.append(str(p))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(tsvs) + "\n")
    inp = os.path.join(GOLDEN, "sim_gaussian_30k.bin")
    base = ["-i", inp, "-P", "--viterbi", "-n", "20"]
    r = _cli(base + ["--sweepAlpha", str(lst)], tmp_path / "sweep")
    assert "--sweepAlpha: 66 candidates on one loaded input, engine: batched (hf_batch), 66 models per group" in r.stderr, r.stderr[-1500:]
    rows = [l.split("\t") for l in (tmp_path / "sweep" / "alpha_sweep.tsv").read_text().splitlines() if not l.startswith("#")]
    assert len(rows) == 66 and all(row[5] == "ok" for row in rows)
    for i in (0, 63, 64, 65):
        sep = tmp_path / ("sep%d" % i)
        _cli(base + ["--alphaTsv", tsvs[i]], sep)
        a, b = _tree(tmp_path / "sweep" / ("alpha_%d" % (i + 1))), _tree(sep)
        assert sorted(a) == sorted(b)
        for n in b:
            assert a[n] == b[n], (i, n)
        ll = [l.split("\t") for l in (sep / "loglikelihood.tsv").read_text().splitlines()[1:]]
        assert rows[i][0] == str(i + 1) and rows[i][1] == tsvs[i]
        assert rows[i][4] == ll[-1][2] and int(rows[i][2]) == int(ll[-1][0])
