"""Many models on one context (hf_batch_*, hmm.EMBatch, hmm_flagger --sweepAlpha): every model of a batched pass holds the bits of the
same model's hf_estep on a single context, agrees with the oracle, and leaves the other models and the context alone."""
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
