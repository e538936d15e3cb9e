"""CPU checks of the ground of tests/test_floor_gpu.py: the fixtures of tests/floor_cases.py (the floored rows do sit on the floor; the
stretches lie against the pass's lanes and segments, the getters' grid, a region change and a joined chunk boundary as the module text
says), the numpy references on floored rows against path enumeration (a tiny floored store, the bound each reference's own CPU test
asserts), the oracle and alpha_ref on a floored store, the conditions that keep the device tests from passing emptily (on the
REFERENCE values, for the committed job lists), and the premise of the long-run jobs: the plain float64 product of f_a with the eight
rows behind such a start is subnormal."""
import functools

import numpy as np
import pytest

from flagger_amd import _native as N
from oracle_py import Oracle
from test_bruteforce_cpu import Params, _tiny_store
from test_longrun_cpu import close, comparable, max_len
from test_viterbi_cpu import enumerate_map, perturbed_model
import alpha_ref as AR
import breakpoint_ref as BR
import entropy_ref as ER
import floor_cases as FC
import interval_ref as IR
import longrun_ref as LR
import minlen_ref
import moments_ref as MR
import posterior_ref as PR
import runs_ref as RR
import sampling_ref as S
import test_breakpoint_cpu as TBC
import test_entropy_cpu as TEC
import test_posterior_cpu as TPC
import viterbi_ref

FLOOR = np.log(1e-40)
BOTH = pytest.mark.parametrize("name", FC.NAMES)


# ---- the fixtures' facts ----------------------------------------------------------------------------------------------------------------
@BOTH
def test_the_floored_rows_sit_on_the_floor(name):
    store, model, alpha = FC.fixture(name)
    logA, _ = viterbi_ref.tables(store, model, alpha)
    top = logA.max(axis=(1, 2))
    hit = np.asarray(store.cov) == FC.COV
    assert top[hit].max() <= FLOOR and np.all(top[hit] > FLOOR - 12.0)          # a transition probability times 1e-40, no smaller
    for a, b in FC.stretches(name):                                             # a stretch has exactly its windows: its neighbours are ordinary
        c = int(np.searchsorted(FC.off_of(name), a, "right") - 1)
        lo, hi = FC.off_of(name)[c], FC.off_of(name)[c + 1]
        assert np.all(hit[a:b + 1])
        if a - 1 >= lo + 1:
            assert top[a - 1] > -60.0, (a, top[a - 1])
        if b + 1 < hi:
            assert top[b + 1] > -60.0, (b, top[b + 1])
    A, end = FC.rows(name)
    assert np.all(np.isfinite(FC.pass_reference(name)[1])) and not np.any(np.isnan(FC.pass_reference(name)[0]))


def test_short_is_the_minlen_fixture():
    import minlen_post_ref
    assert FC.short() is minlen_post_ref.floored_case()
    assert list(np.diff(FC.off_of("short"))) == [40, 64, 100, 24, 70] and FC.short()[1].numberOfRegions == 1
    assert FC.stretches("short") == ((0, 11), (92, 103), (104, 115), (192, 203), (204, 227), (249, 278))
    assert FC.range_jobs("short")[0].size >= 1326


def test_long_lies_against_lanes_segments_grid_region_and_join():
    store, model, alpha = FC.long()
    off = FC.off_of("long")
    assert list(np.diff(off)) == FC.LONG_LENGTHS and store.n_windows <= 2500 and model.numberOfRegions == 2
    assert model.modelType == N.HF_MODEL_TRUNC_EXP_GAUSSIAN and alpha is FC.synth.HIFI_ALPHA
    assert FC.stretches("long") == tuple(FC.LONG_FLOORED)
    hit = np.asarray(store.cov) == FC.COV
    def segments(c):
        """[(first window, windows, L)] of chunk c: ceil(T / 512) equal segments (hf_create.h), L = ceil(n / 64) windows per lane."""
        T = int(off[c + 1] - off[c])
        nsg = -(-T // FC.SEG)
        sz = -(-T // nsg)
        return [(int(off[c]) + k * sz, min(sz, T - k * sz), -(-min(sz, T - k * sz) // 64)) for k in range(-(-T // sz))]
    # chunk 0: one segment with L = 8; a stretch of at least 24 windows that covers two whole lanes, one of exactly 8, one of exactly 7
    (t0, n, L), = segments(0)
    assert 449 <= n <= 512 and L == 8
    lens = [b - a + 1 for a, b in FC.LONG_FLOORED[:3]]
    assert lens[0] >= 24 and lens[1] == 8 and lens[2] == 7
    whole = [j for j in range(64) if j * L + L <= n and np.all(hit[t0 + j * L:t0 + j * L + L])]
    assert len(whole) >= 3 and {12, 13, 14, 15, 25} <= set(whole)
    # chunk 1: at least three segments, one of them floored as a whole, the stretch a few windows into both neighbours
    segs = segments(1)
    assert len(segs) >= 3
    a, b = FC.LONG_FLOORED[3]
    s0, sn, _ = segs[1]
    assert np.all(hit[s0:s0 + sn]) and 1 <= s0 - a <= 8 and 1 <= b - (s0 + sn - 1) <= 8
    assert not np.all(hit[segs[0][0]:segs[0][0] + segs[0][1]]) and not np.all(hit[segs[2][0]:segs[2][0] + segs[2][1]])
    # the getters' grid: the stretch crosses a global multiple of 512 (and so of 8)
    g = (a // FC.PIECE + 1) * FC.PIECE
    assert a < g - 1 and g + 1 < b and g % FC.LANE == 0
    # a region change inside it, and only one
    reg = store.regions()
    assert np.flatnonzero(reg[a + 1:b + 1] != reg[a:b]).tolist() == [FC.LONG_REGION_CHANGE - a - 1]
    # chunks 2 and 3 on one contig, floored on both sides of the boundary
    assert store.chunk_ctg[3] == store.chunk_ctg[2] and list(FC.joins("long")) == [False, False, False, True]
    assert hit[off[3] - 1] and hit[off[3]] and off[3] - FC.LONG_FLOORED[4][0] >= FC.LR_STRETCH and FC.LONG_FLOORED[5][1] - off[3] + 1 >= FC.LR_STRETCH


@BOTH
def test_the_boundary_points(name):
    P = set(int(p) for p in FC.points(name))
    off = FC.off_of(name)
    n = int(off[-1])
    want = set()
    for c in range(off.size - 1):
        want.update([off[c] - 1, off[c], off[c] + 1, off[c + 1] - 2, off[c + 1] - 1, off[c + 1]])
    for a, b in FC.stretches(name):
        want.update([a - 1, a, a + 1, b - 1, b, b + 1, a - 8, a + 8, a - 9, a + 9])
    for g in range(FC.PIECE, n, FC.PIECE):
        want.update([g - 1, g, g + 1])
    assert P == set(int(t) for t in want if 0 <= t < n)
    F, L, M, R = FC.range_jobs(name)
    assert F.size == len(P) * (len(P) + 1) // 2 and np.all(F <= L)


# ---- the references on floored rows against enumeration --------------------------------------------------------------------------------
TINY_LENGTHS = [7, 5, 1, 6, 3, 7]
TINY_JOINS = np.array([0, 1, 1, 0, 1, 1], bool)
TINY_CASES = [(N.HF_MODEL_GAUSSIAN, 1), (N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 0)]


@functools.lru_cache(maxsize=None)
def _tiny(model_type, seed):
    """Chunks of at most 7 windows with several windows each at coverage 250: at a chunk's first end, its last end, inside, all of one."""
    rng = np.random.default_rng(8800 + seed)
    alpha = FC.synth.HIFI_ALPHA if seed % 2 == 0 else np.zeros((4, 4))
    store = _tiny_store(rng, TINY_LENGTHS, [20, 24] if seed % 2 == 0 else [25])
    off = np.asarray(store.chunk_off, np.int64)
    for c, (a, b) in enumerate([(0, 3), (2, 5), (0, 1), (2, 4), (0, 3), (3, 7)]):
        store.cov[off[c] + a:off[c] + b] = FC.COV
    if seed % 2 == 0:                                        # (one region inside a stretch: floor_cases.long)
        reg = store.regions().astype(np.uint64)
        reg[np.asarray(store.cov) == FC.COV] = 0
        store.annot = (store.annot & np.uint64((1 << 58) - 1)) | (reg << np.uint64(58))
    model = perturbed_model(store, model_type, 2, alpha, rng)
    A, end = S.rows(store, model, alpha)
    logA, _ = viterbi_ref.tables(store, model, alpha)
    hit = np.asarray(store.cov) == FC.COV
    assert hit.sum() >= 15 and logA[hit].max() <= FLOOR
    return store, model, alpha, A, end


def _tiny_jobs(off, seed):
    """Every range inside a chunk and every range over two or three neighbouring chunks of at most 10 windows."""
    rng = np.random.default_rng(seed)
    F, L = [], []
    n = int(off[-1])
    for a in range(n):
        for b in range(a, min(n, a + 10)):
            F.append(a); L.append(b)
    F, L = np.array(F, np.int64), np.array(L, np.int64)
    return F, L, rng.integers(1, 16, F.size), rng.integers(-1, 2, F.size)


@pytest.mark.parametrize("model_type,seed", TINY_CASES)
def test_references_equal_enumeration_on_floored_rows(model_type, seed):
    store, model, alpha, A, end = _tiny(model_type, seed)
    off = np.asarray(store.chunk_off, np.int64)
    F, L, M, R = _tiny_jobs(off, seed)
    R = np.minimum(R, store.n_regions - 1)
    # interval (test_interval_cpu)
    ref, bf = IR.log_probs(A, end, off, F, L, M), IR.brute_force(A, end, off, F, L, M)
    assert np.array_equal(np.isneginf(ref), np.isneginf(bf))
    fin = np.isfinite(bf)
    assert np.allclose(np.exp(ref[fin]), np.exp(bf[fin]), rtol=1e-12, atol=0) and fin.sum() >= 100
    # count moments (test_moments_cpu)
    reg = store.regions().astype(np.int64)
    for unit in MR.UNITS:
        w = MR.weights(store, unit)
        scale = float(store.window_len) ** 2 if unit == "bases" else 1.0
        ma, va = MR.brute_force(A, end, off, w, reg, F, L, M, R)
        m2, v2 = MR.moments_long(A, end, off, w, reg, F, L, M, R)
        assert np.allclose(ma, m2, rtol=1e-11, atol=1e-12 * np.sqrt(scale))
        assert np.allclose(va, v2, rtol=1e-9, atol=1e-12 * scale)
    # run moments (test_runs_cpu)
    for joins in (None, TINY_JOINS):
        ma, va = RR.brute_force(A, end, off, F, L, M, joins)
        m2, v2, s2 = RR.jet_long(A, end, off, F, L, M, joins)
        assert np.allclose(ma, m2, rtol=1e-11, atol=1e-12)
        assert np.all(np.abs(va - v2) <= 1e-12 + 1e-10 * s2)
    # entropy and labelling log-probabilities (test_entropy_cpu)
    ld = ER.LongDouble(A, end, off)
    assert TEC.deviation(ld.entropy(F, L), ER.brute_force(A, end, off, F, L)) <= 1e-9
    for nm, y in ER.labellings(A, end, off, 50 + seed):
        assert TEC.deviation(ld.log_probs(F, L, y), ER.brute_force(A, end, off, F, L, y)) <= 1e-9, nm
    # long runs (test_longrun_cpu)
    rng = np.random.default_rng(seed + 1)
    K = np.minimum(rng.choice(FC.LR_LENGTHS[:4], F.size), [max_len(m) for m in M])
    for joins in (None, TINY_JOINS):
        rn, rs = LR.log_probs(A, end, off, F, L, M, K, joins)
        bn, bs = LR.brute_force(A, end, off, F, L, M, K, joins)
        close(rn, bn, rtol=1e-12, atol=1e-12)
        close(rs, bs, rtol=1e-12, atol=1e-12)
        assert np.all(comparable(bn) & comparable(bs))
    # breakpoints (test_breakpoint_cpu: the recursion against the masked forward against enumeration)
    inside = np.flatnonzero((F < L) & (np.searchsorted(off, F, "right") == np.searchsorted(off, L, "right")))
    U = rng.integers(1, 15, inside.size).astype(np.int64)
    V = 15 & ~U
    got = BR.LongDouble(A, end, off).events(F[inside], L[inside], U, V)
    for g, i, u, v in zip(got, inside, U, V):
        assert TBC._same(g, BR.brute_force(A, end, off, F[i], L[i], u, v)), (F[i], L[i], u, v)
    # the posterior, the pair counts and the log-likelihood (test_posterior_cpu)
    A2, end2 = PR.rows(store, model, alpha)
    post, xi, ll = PR.forward_backward(A2, end2, off, PR.regions_of(store), model.numberOfRegions)
    bpost, bxi, bll = PR.brute_force(A2, end2, off, PR.regions_of(store), model.numberOfRegions)
    TPC._agree(post, bpost)
    TPC._agree(xi, bxi)
    assert np.allclose(ll, bll, rtol=TPC.RTOL, atol=0) and ll.max() < -90.0


@pytest.mark.parametrize("model_type,seed", TINY_CASES)
def test_tables_and_viterbi_equal_enumeration_in_50_digits(model_type, seed):
    """The rows themselves (viterbi_ref.tables, which every reference is built on) against the 50-digit path weights computed from the
    store and the parameters: the best path's weight of every chunk, floored windows included (test_viterbi_cpu's bound)."""
    store, model, alpha, A, end = _tiny(model_type, seed)
    P = Params(model.param_vector(), model.numberOfRegions, 2, model_type, alpha)
    labels, score, plp = viterbi_ref.reference(store, model, alpha)
    for c in range(store.n_chunks):
        path, lbest, l2 = enumerate_map(store, c, P, model)
        assert abs(score[c] - float(lbest)) <= 1e-12 * abs(float(lbest)), (c, score[c], lbest)
        assert abs(plp(labels)[c] - float(lbest)) <= 1e-12 * abs(float(lbest))


@BOTH
def test_the_oracle_and_alpha_ref_on_a_floored_store(name):
    """The oracle raises no scale error on floored windows (its bound is 1e-50) and its posterior is posterior_ref's; alpha_ref's
    statistics are finite."""
    store, model, alpha = FC.fixture(name)
    orc = Oracle(store, model.modelType, model.maxNumberOfComps, alpha, threads=4)
    try:
        orc.set_param_vector(model.param_vector())
        assert orc.run_iteration() == 0
        f, b, sc = orc.forward_backward()
        assert sc.min() > 1e-50 and np.sum(sc < 1e-39) >= np.sum(np.asarray(store.cov) == FC.COV) - store.n_chunks
        g = f * b
        post = g / g.sum(axis=1, keepdims=True)
        assert np.allclose(post, FC.pass_reference(name)[0], rtol=1e-9, atol=1e-300)
        assert np.array_equal(orc.labels(), FC.pass_reference(name)[0].argmax(axis=1))
    finally:
        orc.close()
    ref = AR.stats(store, model, alpha)
    for k in ("G", "H", "Gabs"):
        assert np.all(np.isfinite(ref[k]))
    assert ref["H"].max() > 0.0


# ---- the job lists say something ---------------------------------------------------------------------------------------------------------
@BOTH
def test_the_jobs_say_something(name):
    """On the reference's values: the -650 rule of test_longrun_gpu._check leaves out at most 5 % of the long-run jobs, at least half of
    them walk the chain to a value that is neither 0 nor -inf, at least 30 start within eight windows before a stretch of at least nine
    floored windows (each of 0, 1, 7, 8 among them) and some start inside one; test_breakpoint_gpu._not_empty holds; the range jobs
    have finite values away from 0 and full masks."""
    F, L, M, K, D = FC.longrun_jobs(name)
    assert set(K.tolist()) <= set(FC.LR_LENGTHS) and np.all(K <= [max_len(m) for m in M])
    assert np.sum(D >= 0) >= 30 and all(np.sum(D == d) >= 4 for d in FC.LR_BEFORE)
    inside = np.zeros(F.size, bool)
    for a, b in FC.lr_stretches(name):
        inside |= (F > a) & (F + 8 <= b) & (L >= F + 8)
    assert inside.sum() >= 10
    for joined in (False, True):
        none, some = FC.longrun_reference(name, joined)
        assert not np.any(np.isnan(none)) and not np.any(np.isnan(some))
        out = 1.0 - np.mean(comparable(none) & comparable(some))
        walk = np.mean(np.isfinite(none) & (none != 0.0) & np.isfinite(some) & (some != 0.0))
        hazard = (D >= 0) | inside
        live = np.mean(np.isfinite(none[hazard]) & (none[hazard] != 0.0) & comparable(none[hazard]) & comparable(some[hazard]))
        print("%s long runs %s: %d jobs, %.2f %% left out, %.1f %% walk the chain (%.1f %% of the %d that start at a stretch)"
              % (name, "joined" if joined else "apart", F.size, 100 * out, 100 * walk, 100 * live, int(hazard.sum())))
        assert out <= 0.05 and walk >= 0.5 and live >= 0.5
    if FC.JOINS[name] and name == "long":                  # the join matters to the reference
        a, b = FC.longrun_reference(name, False), FC.longrun_reference(name, True)
        with np.errstate(invalid="ignore"):
            assert np.sum(~((a[0] == b[0]) | (np.abs(a[0] - b[0]) <= 1e-6))) >= 3
    import test_breakpoint_gpu as TB
    (bF, bL, U, V), events = FC.breakpoint_reference(name)
    chunk = np.searchsorted(FC.off_of(name), np.arange(int(FC.off_of(name)[-1])), "right") - 1
    assert np.all(bF < bL) and np.all(chunk[bF] == chunk[bL]) and not np.any(U & V) and bF.size >= 80
    TB._not_empty(events, name)
    iv = FC.interval_reference(name)
    Fr, Lr, Mr, Rr = FC.range_jobs(name)
    assert np.sum(np.isfinite(iv) & (iv < -1e-3)) >= 400 and np.sum(Mr == 15) >= 50
    mean, var, scale = FC.run_reference(name, True)
    assert np.sum(var > 1e-3) >= 400
    assert np.sum(FC.entropy_reference(name) > 1e-3) >= 400
    for x in (iv, mean, var, FC.entropy_reference(name)) + tuple(FC.count_reference(name, "windows")):
        assert not np.any(np.isnan(x))


def test_the_minimum_lengths_bite_on_the_long_store():
    store, model, alpha = FC.long()
    ref = minlen_ref.reference(store, model, alpha, FC.MIN_LEN)
    assert int(np.sum(~minlen_ref.admissible(ref[3], store.chunk_off, FC.MIN_LEN))) >= 2


# ---- the premise of the long-run jobs ----------------------------------------------------------------------------------------------------
@BOTH
def test_eight_floored_steps_from_magnitude_one_end_subnormal(name):
    """The recurrence a linear-domain walker runs, x <- x A_t in plain float64, from the pass's normalised forward vector at a job's
    first window over the eight windows behind it: where those are floored the largest entry is below the smallest normal number
    (2.2e-308) after the eighth step and above it after the seventh.  This is why floor_cases.longrun_jobs start where they do; it says
    nothing about the device."""
    A, end = FC.rows(name)
    off = FC.off_of(name)
    al, _ = RR.alpha_beta(A, end, off)
    tiny = np.finfo(np.float64).tiny
    starts = 0
    for a, b in FC.lr_stretches(name):
        for s in (a - 1, a, a + 1):
            c = int(np.searchsorted(off, a, "right") - 1)
            if s < off[c] or s + 8 > b:
                continue
            x = al[s] / al[s].sum()
            with np.errstate(under="ignore"):
                for k in range(1, 9):
                    x = x @ A[s + k]
                    if k == 7:
                        assert x.max() > tiny, (s, x.max())
            assert 0.0 < x.max() < tiny, (s, x.max())
            starts += 1
    assert starts >= 6
    F, L, M, K, D = FC.longrun_jobs(name)
    assert np.sum((D == 0) | (D == 1)) >= 8
