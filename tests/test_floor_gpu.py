"""The pass, every range getter and the decoders on stretches of windows at the emission floor (tests/floor_cases.py: rows whose every
entry is a transition probability times 1e-40, for whole lanes, a whole renormalisation period, a whole segment, across the getters'
grid, a region change and a joined chunk boundary; tests/test_floor_cpu.py checks the fixtures, the references on floored rows and that
the job lists say something).  A walk in the linear domain loses 133 binary orders of magnitude per floored window.

Every comparison is the one of the feature's own device test, imported and not restated: test_estep_gpu._check_pass (labels exact,
log-likelihood, statistics and forward / backward 1e-9), test_alpha_gpu._close, test_interval_gpu._close, _close_mean / _close_var
of test_moments_gpu and test_runs_gpu, test_entropy_gpu._close, test_posterior_gpu._check_values, test_breakpoint_gpu._check,
test_longrun_gpu._check (test_longrun_cpu.close: 1e-10 + 1e-9 |ref| where the reference is >= -650 or -inf),
test_viterbi_gpu._check_against_reference, test_sampling_gpu._near_tie_events, test_minlen_gpu._check, test_minlen_post_gpu._check,
test_minlen_sample_gpu._check, test_batch_gpu._check_identity.  Every test prints its largest deviations before it asserts (pytest -s);
profiles/floor_cases.txt holds them as measured on an MI355X.

test_long_runs was written for a defect read from the code: k_lr_chain started its walk from f_a at magnitude 1 and renormalised after
the eighth step only, so that a range beginning on eight floored windows went through 3.7e-321, a subnormal, first (hf_longrun.h
NUMERICS; what the device returned before the first vector was scaled: profiles/floor_cases.txt)."""
import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm
from oracle_py import Oracle
import alpha_ref as AR
import floor_cases as FC
import minlen_post_ref
import minlen_ref
import minlen_sample_ref
import moments_ref as MR
import test_alpha_gpu as TA
import test_batch_gpu as TBT
import test_breakpoint_gpu as TB
import test_entropy_gpu as TE
import test_estep_gpu as TEG
import test_interval_gpu as TI
import test_longrun_gpu as TL
import test_minlen_gpu as TML
import test_minlen_post_gpu as TMP
import test_minlen_sample_gpu as TMS
import test_moments_gpu as TM
import test_posterior_gpu as TP
import test_runs_gpu as TR
import test_sampling_gpu as TS
import test_viterbi_gpu as TV

pytestmark = pytest.mark.gpu
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]
BOTH = pytest.mark.parametrize("name", FC.NAMES)


def _pass(name, algo=N.HF_ALGO_SCAN):
    """A full pass with the fixture's model: no error flag (the scale of a floored window is about 1e-40 times a transition
    probability, not an underflow), the log-likelihood against the sum of posterior_ref's chunk log-likelihoods (a context has no
    getter for one chunk's; the decoders' chunk scores are checked per chunk in their own tests below)."""
    store, model, alpha = FC.fixture(name)
    em = hmm.EMList(store, model, algo=algo)
    em.launch(model)
    stats = em.finish().copy()
    ll = FC.pass_reference(name)[1]
    assert ll.sum() < -92.0 * np.sum(np.asarray(store.cov) == FC.COV)
    assert abs(stats[0] - ll.sum()) <= 1e-9 * abs(ll.sum()), (stats[0], ll.sum())
    return em, stats


# ---- the pass -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", TEG.ALGOS)
@BOTH
def test_pass_equals_the_oracle(name, algo):
    """One full pass with the fixture's model against the oracle at the bars of test_estep_gpu._check_pass (labels exact, log-likelihood,
    statistics, forward, backward and scales 1e-9), statistics by rows and by chunks, both algorithms; then the M-step.  The fixture's
    model and not createModel's: under createModel's symmetric transitions 23 floored windows of short() have their two largest posteriors
    equal to 1e-12 (14 of them exactly, by the oracle), and a label there is decided by rounding (tests/test_neartie_gpu.py); under the
    fixture's model the smallest relative gap is 1e-2 on both fixtures."""
    store, model0, alpha = FC.fixture(name)
    model = hmm.createModel(model0.modelType, model0.maxNumberOfComps, store, alpha)
    model.set_param_vector(model0.param_vector())
    em = TEG.make_em(store, model, True, 0.95, device=0, algo=algo)
    orc = Oracle(store, model.modelType, model.maxNumberOfComps, alpha, 0.25, 0.75, True, 0.95, threads=8)
    try:
        orc.set_param_vector(model.param_vector())
        hmm.EM_runOneIterationForList(em, model)
        assert orc.run_iteration() == 0
        ref, got = orc.stats_vector(model.maxNumberOfComps), model.estimators
        scale = np.maximum(np.abs(ref), 1e-6 * np.abs(ref).max())
        print("%s: log-likelihood %.3e relative, statistics %.3e of the scale" % (name, abs(got[0] - ref[0]) / abs(ref[0]), float(np.max(np.abs(got - ref) / scale))))
        assert abs(got[0] - ref[0]) <= TEG.LL_RTOL * abs(ref[0]), (got[0], ref[0])
        assert np.all(np.abs(got - ref) <= TEG.STAT_RTOL * scale), np.max(np.abs(got - ref) / scale)
        lab, olab = em.labels(), orc.labels()
        assert np.array_equal(lab, olab), f"{np.count_nonzero(lab != olab)} label mismatches of {lab.size}"
        f, b, sc = em.forward_backward()
        of, ob, osc = orc.forward_backward()
        assert sc.min() > 1e-50 and np.sum(sc < 1e-39) >= np.sum(np.asarray(store.cov) == FC.COV) - store.n_chunks
        assert np.allclose(sc, osc, rtol=1e-10, atol=0)
        assert np.allclose(f, of, rtol=1e-9, atol=1e-300)
        assert np.allclose(b, ob, rtol=1e-9, atol=1e-300)
        assert hmm.HMM_estimateParameters(model, 1e-3) == orc.estimate_parameters(1e-3)
        assert np.allclose(model.param_vector(), orc.param_vector(), rtol=1e-8, atol=1e-300)
    finally:
        em.close()
        orc.close()


def _pass_outputs(em, model):
    em.launch(model)
    stats = em.finish().copy()
    return (stats, em.labels().copy(), em.posterior().copy()) + tuple(x.copy() for x in em.forward_backward())


def test_two_launches_equal_one_launch_bit_for_bit(monkeypatch):
    """long(): the floored segment's published product consists of floored rows only; k_seg_prod + k_seg_fb and the one launch that hands
    the products over inside itself do the same arithmetic."""
    store, model, alpha = FC.long()
    em = hmm.EMList(store, model)
    assert em.seg_launches == 1
    one = _pass_outputs(em, model)
    em.close()
    monkeypatch.setenv("HF_SEG_LAUNCHES", "2")
    em = hmm.EMList(store, model)
    assert em.seg_launches == 2
    two = _pass_outputs(em, model)
    em.close()
    for x, y in zip(one, two):
        assert np.array_equal(x, y)
    TP._check_values(two[2], FC.pass_reference("long")[0], "long, two launches")


@pytest.mark.parametrize("mode", list(TA.MODES))
@BOTH
def test_alpha_statistics(name, mode, monkeypatch):
    store, model, alpha = FC.fixture(name)
    ref = AR.stats(store, model, alpha)
    got = TA._stats(store, model, mode, monkeypatch)
    assert got.shape == (store.n_regions, 2, 4, 4) and not np.any(np.isnan(got))
    TA._close(got, ref, "%s %s" % (name, mode))
    assert np.all(got[:, 1] >= 0.0)


# ---- the range getters --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@BOTH
def test_interval_moments_entropy_posterior(name, algo):
    store, model, alpha = FC.fixture(name)
    F, L, M, R = FC.range_jobs(name)
    off, n = FC.off_of(name), store.n_windows
    em, _ = _pass(name, algo)
    what = "%s algo %d" % (name, algo)
    full = M == 15
    iv = em.interval_log_probs(F, L, M)
    ref = FC.interval_reference(name)
    fin = np.isfinite(ref)
    print("%s interval: max |dev - ref| %.3e over %d finite jobs, -inf in %d" % (what, float(np.max(np.abs(iv[fin] - ref[fin]))), int(fin.sum()), int((~fin).sum())))
    assert np.array_equal(np.isneginf(iv), np.isneginf(ref)) and not np.any(np.isnan(iv))
    TI._close(iv, ref)
    assert np.all(iv[full] == 0.0)
    for unit in MR.UNITS:
        mean, var = em.count_moments(F, L, M, R, unit)
        ref = FC.count_reference(name, unit)
        TM._close_mean(mean, ref[0], TM._scale(store, unit), what + " count " + unit)
        TM._close_var(var, ref[1], TM._scale(store, unit), what + " count " + unit)
        TM._exact_for_all_states(store, unit, F, L, M, R, mean, var)
    for joined in (False, True):
        j = FC.joins(name) if joined else None
        mean, var = em.run_moments(F, L, M, j)
        ref = FC.run_reference(name, joined)
        TR._close_mean(mean, ref[0], what + " runs " + ("joined" if joined else "apart"))
        TR._close_var(var, ref[1], ref[2], what + " runs " + ("joined" if joined else "apart"))
        TR._exact_for_all_states(off, F, L, M, j, mean, var)
    h = em.path_entropy(F, L)
    TE._close(h, FC.entropy_reference(name), what + " entropy")
    assert np.all(h >= 0.0)
    for nm, y, ref in FC.log_prob_reference(name):
        lp = em.path_log_probs(F, L, np.asarray(y, np.int64))
        TE._close(lp, ref, what + " log-probability of " + nm)
        assert np.all(lp <= 0.0)
    post_ref, _, marg_ref, cond_ref = FC.pass_reference(name)
    marg, cond = em.entropy_profile(0, n)
    TE._close(marg, marg_ref, what + " profile (marg)")
    TE._close(cond, cond_ref, what + " profile (cond)")
    TP._check_values(em.posterior(0, n), post_ref, what)
    fw, bw, sc = em.forward_backward(0, n)
    g = fw * bw
    TP._check_values(g / g.sum(axis=1, keepdims=True), post_ref, what + " (f b)")
    assert np.array_equal(em.labels(), em.posterior().argmax(axis=1).astype(np.int8))
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
@BOTH
def test_breakpoints(name, algo):
    (F, L, U, V), events = FC.breakpoint_reference(name)
    what = "%s algo %d" % (name, algo)
    TB._not_empty(events, what)
    em, _ = _pass(name, algo)
    base = TB._check(em, F, L, U, V, events, what + " breakpoints", profiles=False)
    pick = np.flatnonzero((np.arange(F.size) % 5 == 0) | (L - F == 1))
    got = TB._check(em, F[pick], L[pick], U[pick], V[pick], [events[i] for i in pick], what + " breakpoint profiles")
    assert TB._same_bits(got, [x[pick] for x in base])
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
@BOTH
def test_long_runs(name, algo):
    """hf_get_long_run_log_probs on floor_cases.longrun_jobs: ranges that start 0, 1, 7 and 8 windows before a stretch of at least nine
    floored windows, inside one and at every boundary point, apart and joined.  Before k_lr_chain scaled its first vector this test
    failed on the jobs that walk eight floored windows before the first renormalisation (profiles/floor_cases.txt)."""
    F, L, M, K, D = FC.longrun_jobs(name)
    em, _ = _pass(name, algo)
    for joined in (False, True):
        what = "%s algo %d long runs %s" % (name, algo, "joined" if joined else "apart")
        got = em.long_run_log_probs(F, L, M, K, FC.joins(name) if joined else None)
        ref = FC.longrun_reference(name, joined)
        for k, nm in ((0, "log_p_none"), (1, "log_p_some")):
            fin = np.isfinite(ref[k]) & TL.comparable(ref[k])
            with np.errstate(invalid="ignore"):
                err = np.abs(got[k][fin] - ref[k][fin]) / (1e-10 + 1e-9 * np.abs(ref[k][fin]))
            err = np.where(np.isnan(err), np.inf, err)
            worst = int(np.flatnonzero(fin)[np.argmax(err)])
            rel = np.abs(got[k][fin] - ref[k][fin])[np.isfinite(err)] / np.maximum(np.abs(ref[k][fin])[np.isfinite(err)], 1e-300)
            print("%s %s: %d jobs, %d compared and finite, NaN %d; beyond the bound %d, of them not finite %d; largest finite deviation %.3g of the "
                  "bound, %.3g relative; the worst job %d: %d..%d mask %d L %d, %d before a stretch, device %r reference %r"
                  % (what, nm, F.size, int(fin.sum()), int(np.isnan(got[k]).sum()), int(np.sum(err > 1.0)), int(np.sum(~np.isfinite(err))),
                     float(np.max(err[np.isfinite(err)], initial=0.0)), float(np.max(rel, initial=0.0)), worst, F[worst], L[worst], M[worst], K[worst], D[worst],
                     float(got[k][worst]), float(ref[k][worst])))
        TL._check(got, ref, what)
        assert np.all(got[0] <= 0.0) and np.all(got[1] <= 0.0)
    em.close()


# ---- the decoders -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@BOTH
def test_viterbi_and_samples(name, algo):
    store, model, alpha = FC.fixture(name)
    em, _ = _pass(name, algo)
    labels, chunk_ll, lp = em.viterbi(model)
    TV._check_against_reference(store, model, alpha, labels, chunk_ll, lp)
    got = em.sample_paths(model, FC.SAMPLES, FC.SAMPLE_SEED)
    ref, marg, fmarg = FC.sample_reference(name)
    events = TS._near_tie_events(got, ref, marg, fmarg, FC.off_of(name))
    print("%s algo %d: viterbi labels equal to the reference's in %.4f%% of the windows, sampler near-tie events %d"
          % (name, algo, 100.0 * np.mean(labels == FC.viterbi_reference(name)[0]), events))
    assert events <= 1
    em.close()


def test_minimum_length_decoders_on_the_long_store():
    """hf_viterbi_minlen, hf_minlen_posterior and hf_sample_paths_minlen at (3, 5, 1, 7) on long() (short() is their own tests')."""
    store, model, alpha = FC.long()
    ml = FC.MIN_LEN
    ref_v = minlen_ref.reference(store, model, alpha, ml)
    ref_p = minlen_post_ref.reference(store, model, alpha, ml)
    ref_s = minlen_sample_ref.reference(store, model, alpha, ml, FC.SAMPLE_SEED, range(FC.SAMPLES))
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        vit = em.viterbi_minlen(model, ml)
        post = TMP._result(em, model, ml)
        smp = em.sample_paths_minlen(model, ml, FC.SAMPLES, FC.SAMPLE_SEED)
        em.close()
        bites = TML._check(store, ref_v, ml, vit)
        assert bites >= 2, bites
        TMP._check(store, ref_p, post, "long algo %d" % algo)
        TMS._check(store, ref_s, smp, ml)
        res.append((vit, post, smp))
    assert TML._same(res[0][0], res[1][0]) and TMP._same(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


# ---- the batched engine -------------------------------------------------------------------------------------------------------------
def test_batch_is_bit_identical_to_single_passes():
    store, model, alpha = FC.long()
    TBT._check_identity(store, model.modelType, iters=1)
