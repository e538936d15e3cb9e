"""CPU checks of the ground tests/test_geometry_gpu.py stands on (tests/geometry_cases.py: the grid store, its 903 jobs, its references).

1. The two routes of every reference agree on this store within the bound the getter's own CPU test holds them to.
2. The jobs exercise the kernels: enough of them have a value that is neither 0 nor -inf.
3. Every boundary point matters: for every getter and every point there is a job that has the point as its first or last window and
   whose reference value moves by more than 100 device tolerances when that end point moves by one window, so a cut that is off by one
   at that point cannot pass the device test.
Every test prints what it measured before it asserts (pytest -s).  Measured on the three cases:
    routes      interval against path enumeration 1.4e-14 to 5.7e-14 relative (of the probability) over the 30 jobs inside the chunks of
                at most 7 windows; entropy chain rule against long double 9.7e-14 to 1.9e-13 of the scale 1e-3 + |ref| (log-probabilities
                of the labellings the same); count variances 8.3e-15 to 2.5e-14 relative; run variances 1.1e-14 to 1.4e-14 of the scale
    exercised   428 / 643 / 670 finite interval jobs below -1e-3 (391 / 168 / 158 at -inf); 868 / 864 / 895 jobs with an entropy, 770 /
                781 / 782 with a count variance and 766 to 795 with a run variance above 1e-3
    sensitive   47 to 100 % of the moved jobs move by more than 100 tolerances; per point and getter at least 1 and up to 23 jobs do
The store's coverage is random, and with the draw as it came a few boundary windows had a posterior so certain that no job could tell a
cut at them from a cut one window off: geometry_cases.COV_AT sets the coverage of those nine windows by hand.

4. The inputs of the minimum-length decoder, the breakpoint getter and the long-run getter on this store can fail: the constrained
   reference path differs from the unconstrained one in at least three chunks for every length set (all three cases' draws give them:
   chunks 2, 7, 9, 10, 11, 12 for every set, chunk 3 as well for the first two; COV_AT is as it was), it equals path enumeration on
   the chunks of at most 7 windows, at least half of the breakpoint jobs have a finite log_p_event, and at least half of the long-run
   jobs have two values that are finite and not 0 (248 to 315 of 431)."""
import numpy as np
import pytest

from test_bruteforce_cpu import Params
from test_longrun_cpu import comparable
import geometry_cases as G
import breakpoint_ref as BR
import minlen_ref
import viterbi_ref
import test_entropy_cpu as TE
import test_moments_cpu as TM
import test_runs_cpu as TR
import entropy_ref as ER
import interval_ref as IR
import longrun_ref as LR
import moments_ref as MR
import runs_ref as RR

OFF = np.asarray(G.OFF, np.int64)


def test_layout():
    assert G.POINTS.size == 42
    T = np.diff(OFF)
    assert [int(OFF[c]) for c in np.flatnonzero(T == 1)] == [0, 511, 512, 513]
    assert (1023, 1025) in zip(G.OFF[:-1], G.OFF[1:]) and 504 % G.LANE == 0 and 1536 % G.PIECE == 0
    assert (1536, 2048) in zip(G.OFF[:-1], G.OFF[1:]) and (2048, 3073) in zip(G.OFF[:-1], G.OFF[1:])
    for mt, seed in G.CASES:
        store, model, alpha, (F, L, M, R) = G.case(mt, seed)
        assert F.size == 903 and np.all(F <= L) and M.min() == 1 and M.max() == 15
        assert np.sum(M == 15) >= 50
        assert R.min() == -1 and R.max() == store.n_regions - 1
        if store.n_regions > 1:
            reg = store.regions()
            assert reg[511] != reg[512] and reg[1023] != reg[1024]
        parts, pieces = G.pieces_of(OFF, F, L)
        chunk = np.searchsorted(OFF, np.arange(G.N_WINDOWS), "right") - 1
        for i in range(0, F.size, 7):                       # the restated cut rule against a count window by window
            t = np.arange(F[i], L[i] + 1)
            inner = t[1:][chunk[t[1:]] == chunk[t[:-1]]]
            assert parts[i] == np.unique(chunk[t]).size and pieces[i] == np.unique(chunk[inner] * 16 + inner // G.PIECE).size, i
        assert parts.max() == 13
    # the cut rule restated: a piece of exactly one window and a piece of exactly 512 windows in one job, a part without interior
    # between parts with pieces
    assert [int(x[0]) for x in G.pieces_of(OFF, [1535], [3072])] == [3, 4]      # 1535 | 1537..2047 | 2049..2559, 2560..3071, 3072
    assert [int(x[0]) for x in G.pieces_of(OFF, [510], [514])] == [5, 0]
    assert [int(x[0]) for x in G.pieces_of(OFF, [509], [515])] == [5, 2]


@pytest.mark.parametrize("model_type,seed", G.CASES)
def test_interval_routes_agree(model_type, seed):
    _, _, _, (F, L, M, _) = G.case(model_type, seed)
    A, end = G.rows(model_type, seed)
    ref = G.interval_reference(model_type, seed)
    tiny = np.zeros(G.N_WINDOWS, bool)                     # windows of chunks of at most 7 windows
    for c in np.flatnonzero(np.diff(OFF) <= 7):
        tiny[OFF[c]:OFF[c + 1]] = True
    small = np.array([tiny[a:b + 1].all() for a, b in zip(F, L)])
    assert small.sum() == 30                                # all pairs over 0, 1, 2; over 504, 505, 510..513; over 1023, 1024
    bf = IR.brute_force(A, end, OFF, F[small], L[small], M[small])
    assert np.array_equal(np.isneginf(ref[small]), np.isneginf(bf))
    fin = np.isfinite(bf)
    dev = np.abs(np.exp(ref[small][fin]) - np.exp(bf[fin])) / np.exp(bf[fin])
    print("case %d interval: reference against path enumeration %.3e relative over %d jobs (%d finite)" % (seed, dev.max(), small.sum(), fin.sum()))
    assert np.allclose(np.exp(ref[small][fin]), np.exp(bf[fin]), rtol=1e-12, atol=0)
    busy = int(np.sum(np.isfinite(ref) & (ref < -1e-3)))
    print("case %d interval: %d finite jobs below -1e-3, %d at -inf" % (seed, busy, int(np.isneginf(ref).sum())))
    assert busy >= 400
    assert np.all(ref[M == 15] == 0.0)


@pytest.mark.parametrize("model_type,seed", G.CASES)
def test_entropy_routes_agree(model_type, seed):
    _, _, _, (F, L, _, _) = G.case(model_type, seed)
    A, end = G.rows(model_type, seed)
    ref = G.entropy_reference(model_type, seed)
    dev = TE.deviation(ER.chain_rule(A, end, OFF, F, L), ref)
    print("case %d entropy: chain rule against long double %.3e of the scale; %d jobs above 1e-3" % (seed, dev, int(np.sum(ref > 1e-3))))
    assert 100.0 * dev <= TE.RTOL
    assert np.sum(ref > 1e-3) >= 700 and np.all(ref >= -1e-12)
    for name, y, lref in G.log_prob_reference(model_type, seed):
        d = TE.deviation(ER.chain_rule(A, end, OFF, F, L, y), lref)
        print("case %d log-probability of %s: %.3e, -inf in %d jobs" % (seed, name, d, int(np.isneginf(lref).sum())))
        assert 100.0 * d <= TE.RTOL and np.all(lref <= 1e-12)


@pytest.mark.parametrize("model_type,seed", G.CASES)
def test_count_moment_routes_agree(model_type, seed):
    store, _, _, (F, L, M, R) = G.case(model_type, seed)
    A, end = G.rows(model_type, seed)
    reg = store.regions().astype(np.int64)
    for unit in MR.UNITS:
        scale = float(store.window_len) ** 2 if unit == "bases" else 1.0
        mean, var = G.count_reference(model_type, seed, unit)
        m64, v64 = MR.moments_centred(A, end, OFF, MR.weights(store, unit), reg, F, L, M, R)
        dev = TM.rel_dev(v64, var, scale)
        print("case %d count moments (%s): centred float64 against long double %.3e relative; %d jobs with a variance above 1e-3"
              % (seed, unit, dev, int(np.sum(var > 1e-3 * scale))))
        assert 100.0 * dev <= TM.RTOL
        assert np.allclose(m64, mean, rtol=1e-11, atol=1e-12 * np.sqrt(scale))
        assert np.sum(var > 1e-3 * scale) >= 700


@pytest.mark.parametrize("model_type,seed", G.CASES)
def test_run_moment_routes_agree(model_type, seed):
    _, _, _, (F, L, M, _) = G.case(model_type, seed)
    A, end = G.rows(model_type, seed)
    for j in (None, G.joins()):
        mean, var, scale = G.run_reference(model_type, seed, G.joins_key(j))
        m64, v64, _ = RR.jet_centred(A, end, OFF, F, L, M, j)
        dev = TR.rel_dev(v64, var, scale)
        print("case %d run moments (%s): centred float64 against long double %.3e of the scale; %d jobs with a variance above 1e-3"
              % (seed, "apart" if j is None else "joined", dev, int(np.sum(var > 1e-3))))
        assert 100.0 * dev <= TR.RTOL
        assert np.allclose(m64, mean, rtol=1e-11, atol=1e-12)
        assert np.sum(var > 1e-3) >= 700
    m0 = G.run_reference(model_type, seed, None)[0]
    assert np.sum(m0 - mean > 1e-3) >= 100                 # the joins matter


SHORT = 600          # the jobs of at most this many windows are moved (the long-double routes cost a second per 100 000 windows)


def insensitive_points(model_type, seed, name):
    """The boundary points p without a job of at most SHORT windows that has p as its first or last window and whose reference value of
    getter `name` moves by more than 100 device tolerances when that end moves by one window (either way); and the share of the moved
    jobs that do."""
    store, _, _, (F, L, M, R) = G.case(model_type, seed)
    A, end = G.rows(model_type, seed)
    n = G.N_WINDOWS
    if name == "interval":
        ref = G.interval_reference(model_type, seed)
        fn, tol = (lambda f, l, k: IR.log_probs(A, end, OFF, f, l, M[k])), 1e-10 + 1e-9 * np.abs(ref)
    elif name == "entropy":
        ref, ld = G.entropy_reference(model_type, seed), G.long_double(model_type, seed)
        fn, tol = (lambda f, l, k: ld.entropy(f, l)), TE.ATOL + TE.RTOL * np.abs(ref)
    elif name == "count variance":
        ref = G.count_reference(model_type, seed, "windows")[1]
        reg, w = store.regions().astype(np.int64), MR.weights(store, "windows")
        fn, tol = (lambda f, l, k: MR.moments_long(A, end, OFF, w, reg, f, l, M[k], R[k])[1]), TM.ATOL + TM.RTOL * np.abs(ref)
    else:
        j = G.joins()
        _, ref, scale = G.run_reference(model_type, seed, G.joins_key(j))
        fn, tol = (lambda f, l, k: RR.jet_long(A, end, OFF, f, l, M[k], j)[1]), TR.ATOL + TR.RTOL * scale
    short = L - F < SHORT
    far = {}
    for mv, (f2, l2) in {"L+1": (F, L + 1), "L-1": (F, L - 1), "F+1": (F + 1, L), "F-1": (F - 1, L)}.items():
        ok = short & (f2 >= 0) & (l2 < n) & (f2 <= l2)
        val = fn(f2[ok], l2[ok], ok)
        with np.errstate(invalid="ignore"):
            d = np.abs(val - ref[ok])
        d = np.where(np.isfinite(val) & np.isfinite(ref[ok]), d, np.where(np.isfinite(val) != np.isfinite(ref[ok]), np.inf, 0.0))
        far[mv] = np.zeros(F.size, bool)
        far[mv][ok] = d > 100.0 * tol[ok]                   # (finite against -inf: as far apart as can be)
    counts = np.array([int(np.sum((far["L+1"] | far["L-1"]) & (L == p)) + np.sum((far["F+1"] | far["F-1"]) & (F == p))) for p in G.POINTS])
    share = float(np.mean((far["L+1"] | far["L-1"] | far["F+1"] | far["F-1"])[short]))
    return [int(p) for p in G.POINTS[counts == 0]], counts, share


@pytest.mark.parametrize("name", ["interval", "entropy", "count variance", "run variance"])
@pytest.mark.parametrize("model_type,seed", G.CASES)
def test_every_boundary_point_matters(model_type, seed, name):
    bad, counts, share = insensitive_points(model_type, seed, name)
    print("case %d %s: %.0f%% of the jobs of at most %d windows move by more than 100 tolerances with an end point; per point %d-%d such jobs"
          % (seed, name, 100 * share, SHORT, counts.min(), counts.max()))
    assert not bad, bad


# ---- 4. the minimum-length decoder, breakpoints and long runs --------------------------------------------------------------------------
def _runs(path):
    return 1 + int(np.sum(np.diff(np.asarray(path, np.int64)) != 0))


@pytest.mark.parametrize("min_len", G.MINLEN_SETS)
@pytest.mark.parametrize("model_type,seed", G.CASES)
def test_min_length_reference_bites_and_equals_enumeration(model_type, seed, min_len):
    store, model, alpha, _ = G.case(model_type, seed)
    lab, score, plp, free = G.minlen_reference(model_type, seed, min_len)
    assert np.array_equal(free, G.viterbi_reference(model_type, seed)[0])
    assert minlen_ref.admissible(lab, OFF, min_len).all()
    T = np.diff(OFF)
    same = np.array([np.array_equal(lab[OFF[c]:OFF[c + 1]], free[OFF[c]:OFF[c + 1]]) for c in range(T.size)])
    print("case %d min_len %s: the constrained path differs from the unconstrained one in chunks %s" % (seed, min_len, [int(c) for c in np.flatnonzero(~same)]))
    assert np.sum(~same) >= 3
    assert np.all(score <= plp(free) + 1e-9 * np.abs(score)) and np.all(score[~same] < plp(free)[~same])     # the constraint costs something there
    if min_len == (16, 16, 16, 16):
        # a chunk of at most 16 windows has no room for a run that touches neither end: an admissible path has at most two runs, so
        # the unconstrained path stays where it has at most two (every one- and two-window chunk) and goes where it has more
        kinds = set()
        for c in np.flatnonzero(T <= 16):
            two = _runs(free[OFF[c]:OFF[c + 1]]) <= 2
            assert same[c] == two and _runs(lab[OFF[c]:OFF[c + 1]]) <= 2, c
            kinds.add(bool(two))
        assert same[T <= 2].all() and kinds == {True, False}
    # path enumeration in 50 digits on the chunks of at most 7 windows (one, two and seven windows)
    regions = model.numberOfRegions
    P = Params(model.param_vector(), regions, 2 + seed % 3, model_type, alpha)
    nbE = None
    if model_type == G.CASES[2][0]:
        p = model.params()
        nbE = np.ctypeslib.as_array(p.nb_E, shape=(regions * 4 * viterbi_ref.NX,)).reshape(regions, 4, viterbi_ref.NX).copy()
    small = np.flatnonzero(T <= 7)
    assert sorted(T[small]) == [1, 1, 1, 1, 2, 2, 7]
    clear = 0
    for c in small:
        path, best, second = minlen_ref.best_admissible(_weights(model_type, seed, int(c), P, nbE), min_len)
        assert abs(score[c] - float(best)) <= 1e-12 * abs(float(best)), (c, score[c], best)
        if best - second > 1e-9 * abs(best):
            assert tuple(int(v) for v in lab[OFF[c]:OFF[c + 1]]) == path, (c, path)
            clear += 1
    assert clear >= small.size - 1


_WEIGHTS = {}


def _weights(model_type, seed, c, P, nbE):
    """All 4^T paths of a small chunk with their weights, once for the three length sets."""
    key = (model_type, seed, c)
    if key not in _WEIGHTS:
        store, model, _, _ = G.case(model_type, seed)
        _WEIGHTS[key] = minlen_ref.chunk_path_weights(store, c, P, model, nbE)
    return _WEIGHTS[key]


@pytest.mark.parametrize("model_type,seed", G.CASES)
def test_breakpoint_and_long_run_jobs_are_exercised(model_type, seed):
    (F, L, U, V), events = G.breakpoint_reference(model_type, seed)
    chunk = np.searchsorted(OFF, np.arange(G.N_WINDOWS), "right") - 1
    assert np.all(F < L) and np.all(chunk[F] == chunk[L]) and not np.any(U & V)
    finite = sum(bool(np.isfinite(BR.summary(e)[0])) for e in events)
    print("case %d breakpoints: %d of %d jobs with a finite log_p_event" % (seed, finite, F.size))
    assert 2 * finite >= F.size
    f, l, m, k = G.longrun_jobs(model_type, seed)
    assert np.all(f <= l) and m.min() >= 1 and m.max() <= 15 and k.min() >= 1
    assert max(LR.lanes(int(a), int(b)) for a, b in zip(m, k)) <= 64
    for j in (None, G.joins()):
        none, some = G.longrun_reference(model_type, seed, G.joins_key(j))
        busy = np.isfinite(none) & np.isfinite(some) & (none != 0.0) & (some != 0.0)
        use = comparable(none) & comparable(some)
        print("case %d long runs (%s): %d of %d jobs with both values finite and not 0, %.1f%% compared"
              % (seed, "apart" if j is None else "joined", int(busy.sum()), f.size, 100.0 * use.mean()))
        assert 2 * busy.sum() >= f.size and use.mean() >= 0.95
    assert np.any(G.longrun_reference(model_type, seed, None)[1] != some)                 # the joins matter
