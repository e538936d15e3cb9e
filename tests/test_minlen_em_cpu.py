"""CPU checks of the ground of the E-step under minimum run lengths: the numpy reference the GPU tests rely on
(tests/minlen_em_ref.py) against mpmath enumeration of all admissible paths, against the posterior reference
(tests/minlen_post_ref.py), and, with all four lengths 1, against the alpha statistics' xi (tests/alpha_ref.py) and the oracle's
estimators, which pins the numpy restatement of the estimator accumulators to the checker the whole suite trusts."""
import functools

import numpy as np
import pytest

from flagger_amd import _native as N
from oracle_py import Oracle
from test_bruteforce_cpu import Params
import alpha_ref
import minlen_em_ref as E
import minlen_post_ref
import minlen_ref
import sampling_ref

CASES = [c for c in minlen_ref.TINY_CASES if c[0] != N.HF_MODEL_NEGATIVE_BINOMIAL]
ONES = (1, 1, 1, 1)
LENGTHS = [ONES, (2, 1, 1, 3), (3, 2, 1, 2), (1, 9, 1, 1)]       # the last: a length above every chunk's


@functools.lru_cache(maxsize=None)
def _enumerated(model_type, seed, hifi):
    """{min_len: {chunk: pair marginals}} of the chunks of at most 7 windows of one tiny case."""
    store, model, alpha, _ = minlen_ref.tiny_case(model_type, seed, hifi)
    P = Params(model.param_vector(), model.numberOfRegions, 2 + seed % 3, model_type, alpha)
    out = {ml: {} for ml in LENGTHS}
    T = np.diff(store.chunk_off)
    for c in range(store.n_chunks):
        if T[c] > 7:
            continue
        w = minlen_ref.chunk_path_weights(store, c, P, model, None)
        for ml in LENGTHS:
            out[ml][c] = E.enumerate_pairs(w, ml)
    return out


@pytest.mark.parametrize("model_type,seed,hifi", CASES)
def test_xi_adm_against_path_enumeration(model_type, seed, hifi):
    store, model, alpha, _ = minlen_ref.tiny_case(model_type, seed, hifi)
    A, end = sampling_ref.rows(store, model, alpha)
    off = store.chunk_off
    enum = _enumerated(model_type, seed, hifi)
    differs = 0
    for ml in LENGTHS:
        xi, _, _ = E.xi_adm(A, end, off, ml)
        for c, pairs in enum[ml].items():
            want = np.array([[[float(v) for v in row] for row in mat] for mat in pairs])
            got = xi[off[c]:off[c + 1]]
            assert np.all(np.abs(got - want) <= 1e-12), (ml, c, float(np.max(np.abs(got - want))))
            assert np.all(got[0] == 0.0)
        if ml != ONES:
            differs += not np.allclose(xi, E.xi_adm(A, end, off, ONES)[0], rtol=0, atol=1e-6)
    assert differs >= 2, "the rules change nothing in this case: the test would pass vacuously"


@pytest.mark.parametrize("model_type,seed,hifi", CASES)
@pytest.mark.parametrize("min_len", LENGTHS + [(3, 5, 1, 7)])
def test_marginal_identities(model_type, seed, hifi, min_len):
    """sum_p xi_adm_t[p][s] = post[t][s] and sum_s xi_adm_t[p][s] = post[t-1][p], post and log Z_adm those of minlen_post_ref."""
    store, model, alpha, _ = minlen_ref.tiny_case(model_type, seed, hifi)
    A, end = sampling_ref.rows(store, model, alpha)
    xi, post_own, lza_own = E.xi_adm(A, end, store.chunk_off, min_len)
    post, _, lza, _ = minlen_post_ref.reference(store, model, alpha, min_len)
    assert np.all(np.abs(post_own - post) <= 1e-12)
    assert np.all(np.abs(lza_own - lza) <= 1e-12 * (1 + np.abs(lza)))
    off = np.asarray(store.chunk_off)
    first = np.zeros(store.n_windows, bool)
    first[off[:-1][np.diff(off) > 0]] = True
    t = np.flatnonzero(~first)
    assert np.all(np.abs(xi[t].sum(axis=1) - post[t]) <= 1e-12)
    assert np.all(np.abs(xi[t].sum(axis=2) - post[t - 1]) <= 1e-12)
    assert np.all(xi[first] == 0.0)


@pytest.mark.parametrize("model_type,seed,hifi", CASES)
def test_all_ones_is_the_plain_xi_and_the_oracles_estimators(model_type, seed, hifi):
    store, model, alpha, _ = minlen_ref.tiny_case(model_type, seed, hifi)
    A, end = sampling_ref.rows(store, model, alpha)
    off = np.asarray(store.chunk_off)
    f, sc = alpha_ref.forward(A, off)
    b = alpha_ref.backward(A, end, sc, off)
    local = np.arange(store.n_windows) - np.repeat(off[:-1], np.diff(off))
    t = np.flatnonzero(local >= 1)
    want = f[t - 1][:, :, None] * A[t] * b[t][:, None, :] / alpha_ref.TERMINATION
    ref = E.stats(store, model, alpha, ONES)
    assert np.all(np.abs(ref["xi"][t] - want) <= 1e-12)
    assert np.array_equal(ref["lza"], ref["lz"])
    K = model.maxNumberOfComps
    orc = Oracle(store, model_type, K, alpha, threads=1)
    try:
        orc.set_param_vector(model.param_vector())
        assert orc.run_iteration() == 0
        ovec = orc.stats_vector(K)
    finally:
        orc.close()
    assert np.count_nonzero(ovec) > 20
    # element 0: log Z holds the end column, which the oracle's log-likelihood (the sum of the log scales) leaves out
    live = np.diff(off) > 0
    ovec[0] += float(np.sum(np.log(np.sum(f[off[1:][live] - 1] * end[live], axis=1))))
    E.close_stats(ref["vec"], ovec, ref["mag"], "restated estimators against the oracle's")


def test_short_chunks_have_no_statistics():
    """A chunk of one or two windows has no pair (w-1, w) with 2 <= w <= T-1: zeros behind element 0, which is log Z_adm; a chunk of
    three windows has the one pair (1, 2)."""
    model_type, seed, hifi = CASES[0]
    store, model, alpha, _ = minlen_ref.tiny_case(model_type, seed, hifi)
    ref = E.stats(store, model, alpha, (2, 1, 1, 3))
    T = np.diff(store.chunk_off)
    assert {1, 2, 3} <= set(T.tolist())
    for c in range(store.n_chunks):
        assert ref["chunk"][c, 0] == ref["lza"][c]
        assert (not ref["chunk"][c, 1:].any()) == (T[c] <= 2)
        if T[c] == 3:                                          # the transition counts of the one pair sum to 1
            R, K = model.numberOfRegions, model.maxNumberOfComps
            cnt = sum(ref["chunk"][c, 1 + r * (24 * K + 16) + 24 * K:1 + (r + 1) * (24 * K + 16)].sum() for r in range(R))
            assert abs(cnt - 1.0) <= 1e-12
