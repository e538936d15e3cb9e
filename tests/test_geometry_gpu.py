"""The range getters (hf_get_interval_log_probs, hf_get_count_moments, hf_get_run_moments, hf_get_path_entropy, hf_get_path_log_probs,
hf_get_entropy_profile, hf_get_posterior, hf_get_forward_backward, hf_get_breakpoints, hf_get_breakpoint_profile,
hf_get_long_run_log_probs), Viterbi, minimum-length Viterbi and the sampler on track geometries and call sizes that no other store of
the suite produces (tests/geometry_cases.py; tests/test_geometry_cpu.py checks the references and that every boundary
point matters):

A. a chunk list laid against the getters' global piece grid (chunks that start or end on, one before and one after a multiple of 512,
   one- and two-window chunks on and across it, parts without interior, region changes on it) and all 903 jobs over its boundary points;
B. calls that need more than one device batch (HF_IV_BATCH_PIECES / _PARTS, HF_MO_BATCH_PIECES of hf_estep.hip): every value is the bits
   of the same job asked alone;
C. chunks without windows, in front, behind, two in a row and between two joined chunks;
D. windows outside every chunk: labels -1, every range getter refuses a job that touches one, hf_create refuses a chunk list that leaves
   the window arrays.

Tolerances are those of the getters' own device tests (test_interval_gpu._close, ATOL / RTOL of test_moments_cpu, test_runs_cpu and
test_entropy_cpu, test_posterior_gpu._check_values, test_breakpoint_gpu._check, test_longrun_gpu._check, test_minlen_gpu._check and
its TOL); -inf must agree exactly, the full mask gives exactly 0 / variance exactly 0.
Every test prints its largest deviations before it asserts (pytest -s).  Measured on an MI355X (the largest over the cases, both
algorithms, the launch variants and parts C and D; relative: over the values with |ref| > 1e-3, variances over those above 1e-3):
    interval        7.6e-10 absolute, 1.0e-9 relative (the Gaussian case, the same figure from both algorithms; the bound is the sum 1e-10 +
                    1e-9 |ref|); the other cases 8.0e-11 and 7.3e-11; batch pool 1.2e-11 absolute
    count moments   means 1.0e-14 relative; variances 8.5e-13 windows^2 absolute, 2.3e-14 relative
    run moments     means 1.0e-14 relative; variances 3.4e-13 absolute, 5.1e-14 of the scale, apart and joined
    entropy         2.3e-13 absolute, 7.3e-14 relative; log-probabilities 5.8e-11 absolute (a constant path over long ranges), 9.4e-14
                    relative; the profile 1.3e-15 absolute, 2.1e-13 relative
    posterior       1.1e-14 relative, exact zeros included; Viterbi labels equal to the reference's in every window, no near-tie
                    event of the sampler
    two batches     1 051 574 interval jobs (by pieces and by parts) and 265 142 jobs of the other getters: every value the bits of
                    the job asked alone
    breakpoints     log_p_event 9.1e-13 absolute, p_k 4.0e-14, mode_p 9.4e-14, |sum p_k - 1| 2.2e-16 (86 jobs, 46 profiles)
    long runs       2.3e-13 absolute over the 431 jobs, apart and joined
    min-length      the reference's labels in every window for the three length sets (7, 7 and 6 chunks bite), an empty chunk's score
                    exactly 0, labels exactly -1 outside the chunks
All of it passed as the code stood, except part D: see test_windows_outside_every_chunk."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm
import geometry_cases as G
import entropy_ref as ER
import interval_ref as IR
import moments_ref as MR
import runs_ref as RR
import sampling_ref as S
import test_breakpoint_gpu as TB
import test_entropy_gpu as TE
import test_interval_gpu as TI
import test_longrun_gpu as TL
import test_minlen_gpu as TML
import test_moments_gpu as TM
import test_posterior_gpu as TP
import test_runs_gpu as TR
import test_sampling_gpu as TS
import test_viterbi_gpu as TV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESTEP = os.path.join(ROOT, "flagger_amd", "csrc", "hf_estep.hip")
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]
OFF = np.asarray(G.OFF, np.int64)
NW = G.N_WINDOWS


def _pass(store, model, algo=N.HF_ALGO_SCAN, stats_mode=None):
    em = hmm.EMList(store, model, algo=algo)
    if stats_mode is not None:
        em.set_stats_mode(stats_mode)
    em.launch(model)                                        # the pass whose model the getters answer for
    return em, em.finish().copy()


def _close_interval(dev, ref, what):
    fin = np.isfinite(ref)
    err = np.abs(dev[fin] - ref[fin])
    big = np.abs(ref[fin]) > 1e-3
    print("%s interval: max |dev - ref| %.3e, max relative deviation (|ref| > 1e-3) %.3e over %d jobs, -inf in %d"
          % (what, float(np.max(err, initial=0.0)), float(np.max(err[big] / np.abs(ref[fin][big]), initial=0.0)), int(big.sum()), int((~fin).sum())))
    assert np.array_equal(np.isneginf(dev), np.isneginf(ref)) and not np.any(np.isnan(dev))
    TI._close(dev, ref)


def _check_getters(em, model_type, seed, what, shift=0, joined=None, sel=None):
    """Every range getter of `em` on the jobs of the case (all of them, or those of the mask `sel`) against the references of the grid
    store; shift: where the grid store's window 0 lies in em's track; joined: (joins over em's chunks, the same over the grid store's)."""
    store, model, alpha, (F, L, M, R) = G.case(model_type, seed)
    k = np.ones(F.size, bool) if sel is None else sel
    f, l, m, r = F[k] + shift, L[k] + shift, M[k], R[k]
    full = m == 15
    n = em.store.n_windows
    # interval
    iv = em.interval_log_probs(f, l, m)
    _close_interval(iv, G.interval_reference(model_type, seed)[k], what)
    assert np.all(iv[full] == 0.0)
    # count moments, both units
    for unit in MR.UNITS:
        mean, var = em.count_moments(f, l, m, r, unit)
        ref = G.count_reference(model_type, seed, unit)
        TM._close_mean(mean, ref[0][k], TM._scale(store, unit), what + " count " + unit)
        TM._close_var(var, ref[1][k], TM._scale(store, unit), what + " count " + unit)
        TM._exact_for_all_states(store, unit, F[k], L[k], m, r, mean, var)
    # run moments, without and with the joins
    for jd, jr in ((None, None), (G.joins(), G.joins())) if joined is None else joined:
        mean, var = em.run_moments(f, l, m, jd)
        ref = G.run_reference(model_type, seed, G.joins_key(jr))
        TR._close_mean(mean, ref[0][k], what + " runs " + ("apart" if jd is None else "joined"))
        TR._close_var(var, ref[1][k], ref[2][k], what + " runs " + ("apart" if jd is None else "joined"))
        TR._exact_for_all_states(OFF, F[k], L[k], m, jr, mean, var)
    # entropy, labelling log-probabilities, the profile
    h = em.path_entropy(f, l)
    TE._close(h, G.entropy_reference(model_type, seed)[k], what + " entropy")
    assert np.all(h >= 0.0)
    for name, y, ref in G.log_prob_reference(model_type, seed):
        yy = np.zeros(n, np.int64)
        yy[shift:shift + NW] = y
        lp = em.path_log_probs(f, l, yy)
        TE._close(lp, ref[k], what + " log-probability of " + name)
        assert np.all(lp <= 0.0)
    post_ref, ll_ref, marg_ref, cond_ref = G.pass_reference(model_type, seed)
    marg, cond = em.entropy_profile(shift, NW)
    TE._close(marg, marg_ref, what + " profile (marg)")
    TE._close(cond, cond_ref, what + " profile (cond)")
    # posterior, forward and backward
    post = em.posterior(shift, NW)
    TP._check_values(post, post_ref, what)
    fw, bw, sc = em.forward_backward(shift, NW)
    g = fw * bw
    TP._check_values(g / g.sum(axis=1, keepdims=True), post_ref, what + " (f b)")
    if sel is None:
        check_breakpoints(em, model_type, seed, what, shift)
        check_long_runs(em, model_type, seed, what, shift, joined)
    return iv


def check_breakpoints(em, model_type, seed, what, shift=0, profile_every=3):
    """hf_get_breakpoints on the breakpoint jobs of the case (G.breakpoint_reference) with the default quantiles and with none, and
    hf_get_breakpoint_profile on every profile_every-th job and every two-window job, by test_breakpoint_gpu._check (its bounds)."""
    (F, L, U, V), events = G.breakpoint_reference(model_type, seed)
    TB._not_empty(events, what)
    f, l = F + shift, L + shift
    base = TB._check(em, f, l, U, V, events, what + " breakpoints", profiles=False)
    none = em.breakpoints(f, l, U, V, [])
    assert none[1].shape == (F.size, 0) and TB._same_bits([none[0], none[2], none[3]], [base[0], base[2], base[3]])
    pick = np.flatnonzero((np.arange(F.size) % profile_every == 0) | (L - F == 1))
    assert np.sum((L - F)[pick] == 1) >= 10
    if profile_every > 1:
        got = TB._check(em, f[pick], l[pick], U[pick], V[pick], [events[i] for i in pick], what + " breakpoint profiles")
        assert TB._same_bits(got, [x[pick] for x in base])
    else:
        TB._check(em, f, l, U, V, events, what + " breakpoint profiles")
    return base


def check_long_runs(em, model_type, seed, what, shift=0, joined=None):
    """hf_get_long_run_log_probs on the long-run jobs of the case without and with joins (joined: as _check_getters), by
    test_longrun_gpu._check; returns the values per pair of joins."""
    F, L, M, K = G.longrun_jobs(model_type, seed)
    out = []
    for jd, jr in ((None, None), (G.joins(), G.joins())) if joined is None else joined:
        got = em.long_run_log_probs(F + shift, L + shift, M, K, jd)
        ref = G.longrun_reference(model_type, seed, G.joins_key(jr))
        TL._check(got, ref, what + " long runs " + ("apart" if jd is None else "joined"))
        assert np.all(got[0] <= 0.0) and np.all(got[1] <= 0.0)
        fin = np.isfinite(ref[0]) & TL.comparable(ref[0])
        print("%s long runs %s: %d jobs, max |d log_p_none| %.3g" % (what, "apart" if jd is None else "joined", F.size,
                                                                      float(np.max(np.abs(got[0][fin] - ref[0][fin]), initial=0.0))))
        out.append(got)
    return out


def _check_decoders(em, model_type, seed, what, shift=0):
    """Viterbi against viterbi_ref.reference, SAMPLES samples against sampling_ref under the same uniforms; returns both.  The
    uniform of a draw is indexed by the window's global index, and that of a chunk's final state by n_windows + the chunk's index in
    the list (include/hmm_flagger_hip.h): the samples of a track with chunks without windows or with windows outside every chunk are
    those of the reference on that chunk list, not those of the grid store.  Then hf_viterbi_minlen for the three length sets of
    geometry_cases.MINLEN_SETS by test_minlen_gpu._check (admissible, and optimal by evaluation within its TOL: a label may differ
    from the reference's only where both paths evaluate to the same score at that level); returns {min_len: (labels, chunk scores,
    score)} last."""
    store, model, alpha, _ = G.case(model_type, seed)
    labels, chunk_ll, lp = em.viterbi(model)
    live = np.diff(np.asarray(em.store.chunk_off)) > 0
    TV._check_against_reference(store, model, alpha, labels[shift:shift + NW], chunk_ll[live], lp)
    assert np.all(chunk_ll[~live] == 0.0)                   # a chunk without windows: score 0
    got = em.sample_paths(model, G.SAMPLES, G.SAMPLE_SEED + seed)
    off = np.asarray(em.store.chunk_off, np.int64)
    if shift == 0 and list(off) == G.OFF:
        ref, marg, fmarg = G.sample_reference(model_type, seed)
    else:
        A, end = G.rows(model_type, seed)
        n = em.store.n_windows
        A_e, end_e = np.zeros((n, 4, 4)), np.zeros((off.size - 1, 4))
        A_e[shift:shift + NW], end_e[live] = A, end
        ref, marg, fmarg = S.ffbs(A_e, end_e, off, G.SAMPLE_SEED + seed, range(G.SAMPLES), n_windows=n)
        ref, marg = ref[:, shift:shift + NW], marg[:, shift:shift + NW]
    events = TS._near_tie_events(got[:, shift:shift + NW], ref, marg, fmarg, off - shift)
    print("%s: viterbi labels equal to the reference's in %.4f%% of the windows, sampler near-tie events %d"
          % (what, 100.0 * np.mean(labels[shift:shift + NW] == G.viterbi_reference(model_type, seed)[0]), events))
    assert events <= 1
    outside = np.r_[0:shift, shift + NW:em.store.n_windows]
    minlen = {}
    for ml in G.MINLEN_SETS:
        ref = G.minlen_reference(model_type, seed, ml)
        lab, cll, lp = em.viterbi_minlen(model, ml)
        bites = TML._check(store, ref, ml, (lab[shift:shift + NW], cll[live], lp))
        assert bites >= 3, (ml, bites)
        assert np.all(cll[~live] == 0.0) and np.all(lab[outside] == -1) and lab[shift:shift + NW].min() >= 0
        differ = [c for c in range(OFF.size - 1) if not np.array_equal(lab[shift + OFF[c]:shift + OFF[c + 1]], ref[0][OFF[c]:OFF[c + 1]])]
        print("%s: min-length labels %s: %d chunks bite, labels other than the reference's (ties by evaluation) in chunks %s" % (what, ml, bites, differ))
        assert not np.array_equal(lab[shift:shift + NW], labels[shift:shift + NW])               # the constrained path is another one
        minlen[ml] = (lab, cll, lp)
    lab, cll = TML._viterbi_results(em)                     # three decoders, none overwrites another
    assert np.array_equal(lab, labels) and np.array_equal(cll, chunk_ll)
    assert np.array_equal(TML._sample_results(em, G.SAMPLES), got)
    return labels, chunk_ll, got, minlen


# ---- A. the grid store --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed", G.CASES)
def test_grid_store_equals_reference(algo, model_type, seed):
    store, model, alpha, (F, L, M, R) = G.case(model_type, seed)
    assert F.size == 903 and list(store.chunk_off) == G.OFF
    em, stats = _pass(store, model, algo)
    ll = G.pass_reference(model_type, seed)[1].sum()
    assert abs(stats[0] - ll) <= 1e-9 * abs(ll), (stats[0], ll)
    what = "case %d algo %d" % (seed, algo)
    iv = _check_getters(em, model_type, seed, what)
    assert np.sum(np.isfinite(iv) & (iv < -1e-3)) >= 400
    _check_decoders(em, model_type, seed, what)
    assert np.array_equal(em.labels(), em.posterior().argmax(axis=1).astype(np.int8))
    em.close()


@pytest.mark.parametrize("env", [{"HF_SEG_LAUNCHES": "2"}, {"HF_SUBPASSES": "3"}])
def test_launch_modes_and_sub_passes(env, monkeypatch):
    model_type, seed = G.CASES[0]
    store, model, alpha, (F, L, M, R) = G.case(model_type, seed)
    em0, stats0 = _pass(store, model)
    base = (em0.interval_log_probs(F, L, M), em0.count_moments(F, L, M, R), em0.run_moments(F, L, M, G.joins()), em0.path_entropy(F, L))
    em0.close()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    em, stats = _pass(store, model)
    if "HF_SEG_LAUNCHES" in env:
        assert em.seg_launches == 2
    else:
        assert em.sub_passes == 3
    assert abs(stats[0] - stats0[0]) <= 1e-9 * abs(stats0[0])
    what = "case %d %s" % (seed, " ".join("%s=%s" % kv for kv in env.items()))
    iv = _check_getters(em, model_type, seed, what)
    _check_decoders(em, model_type, seed, what)
    TI._close(iv, base[0])                                   # and against the default launch
    mean, var = em.count_moments(F, L, M, R)
    TM._close_mean(mean, base[1][0], 1.0)
    TM._close_var(var, base[1][1], 1.0)
    TE._close(em.path_entropy(F, L), base[3], what + " entropy against the default launch")
    em.close()


# ---- B. more than one device batch ----------------------------------------------------------------------------------------------------
def _caps():
    """The getters' batch caps, read from the source: a changed cap cannot silently empty these tests."""
    text = open(ESTEP).read()
    caps = {}
    for name in ("HF_IV_BATCH_PIECES", "HF_IV_BATCH_PARTS", "HF_MO_BATCH_PIECES", "HF_MO_BATCH_PARTS"):
        m = re.search(r"#define\s+%s\s+\(1\s*<<\s*(\d+)\)" % name, text)
        assert m, name
        caps[name] = 1 << int(m.group(1))
    for g, hdr in (("IV", "hf_interval.h"), ("MO", "hf_moments.h"), ("RN", "hf_runs.h"), ("EN", "hf_entropy.h")):      # the grid this store is laid against
        text = open(os.path.join(ROOT, "flagger_amd", "csrc", hdr)).read()
        assert re.search(r"#define\s+HF_%s_PIECE\s+\(64\s*\*\s*HF_%s_LANE\)" % (g, g), text), hdr
        lane = re.search(r"#define\s+HF_%s_LANE\s+(\w+)" % g, text)
        assert lane and lane.group(1) in (str(G.LANE), "HF_IV_LANE", "HF_MO_LANE", "HF_RN_LANE"), (hdr, lane and lane.group(1))
    return caps


@functools.lru_cache(maxsize=None)
def _pool():
    """The distinct jobs of the batch tests (trunc-exp-Gaussian case): index ranges (two-window jobs: one part, one piece each;
    one-window jobs: one part, no piece; three chunk-spanning jobs, the first one the whole track with mask 11) and their references."""
    model_type, seed = G.CASES[0]
    store, model, alpha, _ = G.case(model_type, seed)
    A, end = G.rows(model_type, seed)
    rng = np.random.default_rng(77)
    chunk = np.searchsorted(OFF, np.arange(NW), "right") - 1
    t2 = np.unique(np.concatenate([G.POINTS[G.POINTS + 1 < NW], rng.integers(0, NW - 1, 260)]))
    t2 = t2[chunk[t2] == chunk[t2 + 1]]
    t1 = np.unique(np.concatenate([G.POINTS, rng.integers(0, NW, 60)]))
    span = np.array([[0, NW - 1, 11], [500, 1030, 7], [1020, 3080, 13]], np.int64)
    F = np.concatenate([t2, t1, span[:, 0]])
    L = np.concatenate([t2 + 1, t1, span[:, 1]])
    M = np.concatenate([rng.integers(1, 15, t2.size + t1.size), span[:, 2]])
    R = rng.integers(-1, store.n_regions, F.size)
    two, one, spans = np.arange(t2.size), t2.size + np.arange(t1.size), t2.size + t1.size + np.arange(3)
    parts, pieces = G.pieces_of(OFF, F, L)
    assert np.all(parts[two] == 1) and np.all(pieces[two] == 1) and np.all(parts[one] == 1) and np.all(pieces[one] == 0)
    assert parts[spans[0]] == 13 and np.all(parts[spans] >= 4) and two.size >= 200
    reg, w = store.regions().astype(np.int64), MR.weights(store, "windows")
    ld = G.long_double(model_type, seed)
    y = G.labellings(model_type, seed)[1][1]                 # a drawn path: finite everywhere
    ref = dict(interval=IR.log_probs(A, end, OFF, F, L, M), count=MR.moments_long(A, end, OFF, w, reg, F, L, M, R),
               runs=RR.jet_long(A, end, OFF, F, L, M, G.joins()), entropy=ld.entropy(F, L), log_probs=ld.log_probs(F, L, y))
    return (F, L, M, R), (two, one, spans), (parts, pieces), y, ref


def _call_order(filler, spans, count_of, cap):
    """Pool indices of a call: fillers in a cycle until the batch is a few short of the cap, the whole-track job (the count crosses the
    cap inside it), another chunk-spanning job (the first of the second batch), more fillers, the third chunk-spanning job last."""
    per = int(count_of[filler[0]])
    assert per == 1 and np.all(count_of[filler] == 1)
    n1 = cap - 5
    order = np.concatenate([np.resize(filler, n1), [spans[0], spans[1]], np.resize(filler[::-1], 3000), [spans[2]]])
    return order, n1


def _batch_case(getter, call, filler_kind, cap_name, close):
    model_type, seed = G.CASES[0]
    store, model, alpha, _ = G.case(model_type, seed)
    (F, L, M, R), (two, one, spans), (parts, pieces), y, ref = _pool()
    caps = _caps()
    cap_pieces, cap_parts = (caps["HF_IV_BATCH_PIECES"], caps["HF_IV_BATCH_PARTS"]) if getter == "interval" else \
        (caps["HF_MO_BATCH_PIECES"], caps["HF_MO_BATCH_PARTS"])
    by_parts = cap_name.endswith("PARTS")
    order, n1 = _call_order(one if filler_kind == "one" else two, spans, parts if by_parts else pieces, caps[cap_name])
    starts = G._batches(parts[order], pieces[order], cap_pieces, cap_parts)
    assert len(starts) >= 2 and starts[1] == n1 + 1, starts          # the whole-track job closes the first batch, a spanning job opens the second
    assert order[starts[1] - 1] == spans[0] and order[starts[1]] == spans[1] and order[-1] == spans[2]
    before = (np.cumsum(parts[order]) if by_parts else np.cumsum(pieces[order]))[n1 - 1]
    assert before < caps[cap_name] < before + (parts if by_parts else pieces)[spans[0]]      # the count crosses the cap inside that job
    em, _ = _pass(store, model)
    f = lambda idx: call(em, F[idx], L[idx], M[idx], R[idx], y)
    alone = [np.empty(F.size) for _ in range(2)]
    for i in range(F.size):                                  # every distinct job asked alone
        for a, v in zip(alone, f(np.array([i]))):
            a[i] = v[0]
    close(alone, ref)
    got = f(order)
    print("%s: %d jobs, %d parts, %d pieces in %d device batches" % (getter, order.size, int(parts[order].sum()), int(pieces[order].sum()), len(starts)))
    for a, v in zip(alone, got):
        bad = np.flatnonzero(~((v == a[order]) | (np.isnan(v) & np.isnan(a[order]))))
        assert bad.size == 0, (getter, [(int(i), int(order[i]), float(v[i]), float(a[order[i]])) for i in bad[:8]])
    small = np.concatenate([spans, two[:30], one[:20]])      # the slab after it has grown: a small call answers as before
    for a, v in zip(alone, f(small)):
        assert np.array_equal(v, a[small])
    em.close()


def _two(x):
    return x if isinstance(x, tuple) else (x, x)


def _close_iv(alone, ref):
    _close_interval(alone[0], ref["interval"], "batch pool")


@pytest.mark.parametrize("filler,cap", [("two", "HF_IV_BATCH_PIECES"), ("one", "HF_IV_BATCH_PARTS")], ids=["pieces", "parts"])
def test_second_device_batch_interval(filler, cap):
    _batch_case("interval", lambda em, f, l, m, r, y: _two(em.interval_log_probs(f, l, m)), filler, cap, _close_iv)


def test_second_device_batch_count_moments():
    def close(alone, ref):
        TM._close_mean(alone[0], ref["count"][0], 1.0, "batch pool count")
        TM._close_var(alone[1], ref["count"][1], 1.0, "batch pool count")
    _batch_case("count", lambda em, f, l, m, r, y: em.count_moments(f, l, m, r), "two", "HF_MO_BATCH_PIECES", close)


def test_second_device_batch_run_moments():
    def close(alone, ref):
        TR._close_mean(alone[0], ref["runs"][0], "batch pool runs")
        TR._close_var(alone[1], ref["runs"][1], ref["runs"][2], "batch pool runs")
    _batch_case("runs", lambda em, f, l, m, r, y: em.run_moments(f, l, m, G.joins()), "two", "HF_MO_BATCH_PIECES", close)


def test_second_device_batch_entropy_and_log_probs():
    def close(alone, ref):
        TE._close(alone[0], ref["entropy"], "batch pool entropy")
        TE._close(alone[1], ref["log_probs"], "batch pool log-probability")
    _batch_case("entropy", lambda em, f, l, m, r, y: (em.path_entropy(f, l), em.path_log_probs(f, l, y)), "two", "HF_MO_BATCH_PIECES", close)


# ---- C. chunks without windows --------------------------------------------------------------------------------------------------------
def _chunk_vectors(em):
    """The per-chunk statistics vectors of the last pass (HF_STATS_CHUNKS: hf_chunk_stats_dev), each fetched as the fixed-order sum over
    a chunk list of that one row (hf_finish_gathered, what hf_finish does with all rows)."""
    base, V = em._L.hf_chunk_stats_dev(em._h), em.stats_len
    assert base
    return np.array([em.finish_gathered(base + c * V * 8, 0, 1).copy() for c in range(em.store.n_chunks)])


# (HF_ALGO_SEQ has the per-chunk statistics only)
@pytest.mark.parametrize("algo,stats_mode", [(N.HF_ALGO_SCAN, N.HF_STATS_ROWS), (N.HF_ALGO_SCAN, N.HF_STATS_CHUNKS), (N.HF_ALGO_SEQ, N.HF_STATS_CHUNKS)],
                         ids=["scan-rows", "scan-chunks", "seq-chunks"])
def test_chunks_without_windows(algo, stats_mode):
    """A pass, the decoders and every getter with chunks that hold no window in front, behind, two in a row and between two joined
    chunks, against the same store without them (the samples against the reference sampler on this chunk list: a chunk's final-state
    uniform is indexed by the chunk's position in the list, so they are not those of the store without the empty chunks).  Measured on an MI355X (printed below; the assertion is the suite's 1e-9): the log-likelihood
    has the same bits with and without the empty chunks in every mode; the statistics vector has the same bits in HF_STATS_ROWS, and
    in HF_STATS_CHUNKS differs in the last bit (2.1e-16 of the scale: the fixed-order sum over the chunk list goes by the position of
    a chunk in the list, which the empty chunks shift).  A chunk without windows ends a run of joined chunks (include/hmm_flagger_hip.h): joined is set for every empty chunk and
    its successor here, and the values are those of the grid store with these joins cut."""
    model_type, seed = G.CASES[0]
    store, model, alpha, (F, L, M, R) = G.case(model_type, seed)
    est, src = G.with_empty_chunks(store)
    empty = np.flatnonzero(src < 0)
    assert list(np.diff(est.chunk_off)[empty]) == [0] * 5 and empty[0] == 0 and empty[-1] == est.n_chunks - 1 and np.any(np.diff(empty) == 1)
    em0, stats0 = _pass(store, model, algo, stats_mode)
    em, stats = _pass(est, model, algo, stats_mode)
    assert em.stats_mode == em0.stats_mode == stats_mode
    scale = np.maximum(np.abs(stats0), 1e-6 * np.abs(stats0).max())
    print("empty chunks, algo %d, statistics mode %d: log-likelihood %s, statistics %s (max deviation %.3e of the scale)"
          % (algo, stats_mode, "same bits" if stats[0] == stats0[0] else "%.3e relative" % (abs(stats[0] - stats0[0]) / abs(stats0[0])),
             "same bits" if np.array_equal(stats, stats0) else "differ", float(np.max(np.abs(stats - stats0) / scale))))
    assert abs(stats[0] - stats0[0]) <= 1e-9 * abs(stats0[0])
    assert np.all(np.abs(stats - stats0) <= 1e-9 * scale)
    assert np.array_equal(em.labels(), em0.labels())
    what = "empty chunks algo %d" % algo
    vit, cll, smp, minlen = _check_decoders(em, model_type, seed, what)
    vit0, cll0, lp0 = em0.viterbi(model)
    assert np.array_equal(vit, vit0) and np.array_equal(cll[src >= 0], cll0) and np.all(cll[empty] == 0.0)
    for ml, (mlab, mcll, mlp) in minlen.items():           # the minimum-length decoder: an empty chunk scores exactly 0
        mlab0, mcll0, _ = em0.viterbi_minlen(model, ml)
        assert np.array_equal(mlab, mlab0) and np.array_equal(mcll[src >= 0], mcll0) and np.all(mcll[empty] == 0.0), ml
        ref_ll = np.zeros(est.n_chunks)
        ref_ll[src >= 0] = G.minlen_reference(model_type, seed, ml)[1]
        assert np.all(np.abs(mcll - ref_ll) <= TML.TOL * np.abs(ref_ll)) and abs(mlp - ref_ll.sum()) <= TML.TOL * abs(ref_ll.sum()), ml
    assert np.any(smp != em0.sample_paths(model, G.SAMPLES, G.SAMPLE_SEED + seed))       # (other uniforms for the final states: _check_decoders)
    # the getters: every job, and most of them span an empty chunk (one lies in front of window 0, one behind the last window)
    spans = np.zeros(F.size, bool)
    for k in empty:
        t = int(est.chunk_off[k])
        spans |= (F < t) & (L >= t)
    assert spans.sum() >= 300
    jd, jr = G.empty_chunk_joins(src, G.joins())
    assert jd.sum() > jr.sum() and jr.sum() == G.joins().sum() - 1 and not jr[6]
    _check_getters(em, model_type, seed, what, joined=((None, None), (jd, jr)))
    with_joins, cut = G.run_reference(model_type, seed, G.joins_key(G.joins())), G.run_reference(model_type, seed, G.joins_key(jr))
    assert np.sum(np.abs(with_joins[0] - cut[0]) > 1e-3) >= 20              # the cut join matters to the reference
    if stats_mode == N.HF_STATS_CHUNKS:                     # (last: the fetch goes through the pass's total block)
        rows, rows0 = _chunk_vectors(em), _chunk_vectors(em0)
        assert rows.shape == (est.n_chunks, em.stats_len) and np.all(rows[empty] == 0.0)
        assert np.array_equal(rows[src >= 0], rows0) and np.any(rows0 != 0.0, axis=1).all()
    em.close(); em0.close()


# ---- D. windows outside every chunk ---------------------------------------------------------------------------------------------------
def _refused(fn):
    with pytest.raises(N.HFError) as e:
        fn()
    assert e.value.code == N.HF_E_ARG, e.value


@pytest.mark.parametrize("algo", ALGOS)
def test_windows_outside_every_chunk(algo):
    """FRONT windows in front of the first chunk and BEHIND windows behind the last one.  Before this test the range getters checked a
    range against n_windows only and indexed the chunk list with -1 or n_chunks + 1 for such a job, the decoders' label buffers were
    left as allocated outside the chunks, and HF_ALGO_SEQ evaluated rows from the unwritten records of those windows."""
    model_type, seed = G.CASES[0]
    store, model, alpha, (F, L, M, R) = G.case(model_type, seed)
    ust = G.with_uncovered_windows(store, np.random.default_rng(5))
    a, n = G.FRONT, ust.n_windows
    b = a + NW                                              # the first window behind the chunks
    assert n == NW + G.FRONT + G.BEHIND and ust.chunk_off[0] == a and ust.chunk_off[-1] == b and ust.n_chunks == store.n_chunks
    em0, stats0 = _pass(store, model, algo)
    em, stats = _pass(ust, model, algo)
    scale = np.maximum(np.abs(stats0), 1e-6 * np.abs(stats0).max())
    print("uncovered windows, algo %d: log-likelihood %s, statistics max deviation %.3e of the scale"
          % (algo, "same bits" if stats[0] == stats0[0] else "%.3e relative" % (abs(stats[0] - stats0[0]) / abs(stats0[0])),
             float(np.max(np.abs(stats - stats0) / scale))))
    assert np.array_equal(stats, stats0)
    outside = np.r_[0:a, b:n]
    lab = em.labels()
    assert np.all(lab[outside] == -1) and np.array_equal(lab[a:b], em0.labels())
    what = "uncovered windows algo %d" % algo
    vit, cll, smp, minlen = _check_decoders(em, model_type, seed, what, shift=a)
    vit0, cll0, _ = em0.viterbi(model)
    assert np.all(vit[outside] == -1) and np.array_equal(vit[a:b], vit0) and np.array_equal(cll, cll0)
    for ml, (mlab, mcll, mlp) in minlen.items():           # the minimum-length decoder: -1 outside the chunks, the rest the grid store's
        mlab0, mcll0, mlp0 = em0.viterbi_minlen(model, ml)
        assert np.all(mlab[outside] == -1) and np.array_equal(mlab[a:b], mlab0) and np.array_equal(mcll, mcll0) and mlp == mlp0, ml
    assert np.all(smp[:, outside] == -1) and smp[:, a:b].min() >= 0      # (in-chunk samples: other uniforms than the compacted store's, _check_decoders)
    # every getter refuses a range that touches an uncovered window, and answers afterwards
    y = np.zeros(n, np.int64)
    for f, l in [(0, 0), (a - 1, a - 1), (a - 1, a + 3), (0, n - 1), (a, b), (b - 2, b), (b, b), (n - 1, n - 1)]:
        cnt = l - f + 1
        _refused(lambda: em.interval_log_probs([a, f], [a + 1, l], 5))
        _refused(lambda: em.count_moments([f], [l], 5))
        _refused(lambda: em.count_moments([a, f], [a, l], 5, 0, "bases"))
        _refused(lambda: em.run_moments([f], [l], 5))
        _refused(lambda: em.run_moments([a, f, a], [a, l, a], 5, G.joins()))
        _refused(lambda: em.path_entropy([f], [l]))
        _refused(lambda: em.path_log_probs([a, f], [a, l], y))
        _refused(lambda: em.entropy_profile(f, cnt))
        _refused(lambda: em.posterior(f, cnt))
        _refused(lambda: em.forward_backward(f, cnt))
        _refused(lambda: em.breakpoints([a, f], [a + 1, max(l, f + 1)], 1, 4))
        _refused(lambda: em.breakpoint_profile(f, max(l, f + 1), 1, 4))
        _refused(lambda: em.long_run_log_probs([a, f], [a + 1, l], 5, 2))
        _refused(lambda: em.long_run_log_probs([a, f, a], [a, l, a], 5, 2, G.joins()))
    assert em.posterior(a, 0).shape == (0, 4) and em.posterior(n, 0).shape == (0, 4)      # no window: nothing to refuse
    _check_getters(em, model_type, seed, what, shift=a)
    assert np.array_equal(em.posterior(a, NW), em0.posterior())
    TI._close(em.interval_log_probs(F + a, L + a, M), em0.interval_log_probs(F, L, M))      # (other bits: the piece grid is global, the track moved by 5)
    em.close(); em0.close()


def test_create_refuses_a_chunk_list_outside_the_windows():
    model_type, seed = G.CASES[0]
    store, model, _, _ = G.case(model_type, seed)
    L_ = N.lib()
    def create(edit):
        w, keep = hmm._windows_struct(store, model, True, 0.95)
        off = keep["off"].copy()                            # (the struct's array is the store's own)
        edit(off)
        w.chunk_off = off.ctypes.data_as(C.POINTER(C.c_int64))
        h = C.c_void_p()
        rc = L_.hf_create(C.byref(w), model.numberOfRegions, model.maxNumberOfComps, 0, N.HF_ALGO_SCAN, C.byref(h))
        if rc == N.HF_OK:
            L_.hf_destroy(h)
        return rc
    def first_below_zero(off):
        off[0] = -1
    def last_behind(off):
        off[-1] = NW + 1
    def all_behind(off):
        off[1:] += 1
    assert create(first_below_zero) == N.HF_E_ARG
    assert create(last_behind) == N.HF_E_ARG
    assert create(all_behind) == N.HF_E_ARG
    assert create(lambda off: None) == N.HF_OK
    assert list(store.chunk_off) == G.OFF
