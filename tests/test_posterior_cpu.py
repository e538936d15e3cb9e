"""CPU checks of the posterior reference (tests/posterior_ref.py), which the GPU tests of the posterior getters and of the batched engine
measure the device against: path enumeration on tiny chunks, the oracle's f * b * scale (normalised) and labels on four stores after one
M-step, and the oracle's `trans` statistics."""
import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from oracle_py import Oracle
from test_sampling_cpu import _tiny
import posterior_ref as PR

# Two float64 forward-backwards of the same chain in different operation orders: ~1e2 roundings of 1.1e-16 per entry were measured at
# <= 9e-15 relative; 1e-12 leaves two orders of magnitude and is three below the device bar (1e-9).  An entry below 1e-200 is the product
# of two scaled factors of which one may be subnormal (few significant bits): there only the magnitude is compared.
RTOL = 1e-12
TINY = 1e-200


def _agree(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    assert np.array_equal(a == 0, b == 0), int(np.count_nonzero((a == 0) != (b == 0)))
    big = np.maximum(np.abs(a), np.abs(b)) > TINY
    err = np.abs(a[big] - b[big]) / np.abs(b[big])
    assert np.all(err <= RTOL), float(err.max())
    assert np.all(np.abs(a[~big]) <= TINY) and np.all(np.abs(b[~big]) <= TINY)


@pytest.mark.parametrize("model_type,seed", [(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 0), (N.HF_MODEL_GAUSSIAN, 1),
                                             (N.HF_MODEL_NEGATIVE_BINOMIAL, 2), (N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4)])
def test_reference_equals_path_enumeration(model_type, seed):
    """Posterior, pair counts by region and log-likelihood of every chunk of a tiny store (chunks of 1 .. 6 windows)."""
    store, model, alpha = _tiny(seed, model_type, [6, 3, 1, 5, 2, 4])
    A, end = PR.rows(store, model, alpha)
    reg, R = PR.regions_of(store), model.numberOfRegions
    post, xi, ll = PR.forward_backward(A, end, store.chunk_off, reg, R)
    bpost, bxi, bll = PR.brute_force(A, end, store.chunk_off, reg, R)
    _agree(post, bpost)
    _agree(xi, bxi)
    assert np.allclose(ll, bll, rtol=RTOL, atol=0)
    assert np.allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    T = np.diff(store.chunk_off)
    assert np.allclose(xi.sum(axis=(1, 2, 3)), np.maximum(T - 2, 0), rtol=1e-9, atol=0)   # every End entry is the termination probability
    assert (xi != 0).any()


def _ragged():
    W = 100
    lens = [1 * W, 2 * W, 3 * W, 63 * W, 64 * W, 65 * W, 129 * W, 1000 * W + 37, 5 * W - 1, 2049 * W]
    return synth.synthesize(lens, W, 10_000_000, [20, 25], seed=5, region_run_bases=(2_000, 30_000))


CASES = {
    "ragged": (_ragged, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, 0.95),
    "config4": (lambda: synth.config(4, 0.01), N.HF_MODEL_TRUNC_EXP_GAUSSIAN, None, synth.ONT_R10_ALPHA, 0.8),
    "negative_binomial": (lambda: synth.config(2, 0.004), N.HF_MODEL_NEGATIVE_BINOMIAL, 5, np.zeros((4, 4)), 0.95),
    "gaussian": (lambda: synth.config(2, 0.01), N.HF_MODEL_GAUSSIAN, None, synth.HIFI_ALPHA, 0.95),
}


@pytest.mark.parametrize("name", list(CASES))
def test_reference_equals_the_oracle_after_one_m_step(name):
    make, model_type, K, alpha, frac = CASES[name]
    store = make()
    K = hmm.getBestNumberOfCollapsedComps(store) if K is None else K
    orc = Oracle(store, model_type, K, alpha, 0.25, 0.75, True, frac, threads=4)
    try:
        assert orc.run_iteration() == 0
        orc.estimate_parameters(1e-3)
        model = hmm.createModel(model_type, K, store, alpha)
        model.set_param_vector(orc.param_vector())
        assert orc.run_iteration() == 0
        f, b, sc = orc.forward_backward()
        opost = f * b * sc[:, None]
        opost /= opost.sum(axis=1, keepdims=True)
        post, trans, xi, ll = PR.reference(store, model, alpha, True, frac)
        _agree(post, opost)
        assert np.array_equal(post.argmax(axis=1).astype(np.int8), orc.labels())
        assert (post == 0).any()            # invalid states: exact zeros on both sides
        # the log-likelihood and the pair counts of the statistics: sums over up to ~1e4 windows in another order
        stats = orc.stats_vector(model.maxNumberOfComps)
        assert abs(ll.sum() - stats[0]) <= 1e-11 * abs(stats[0])
        otrans = PR.trans_block(stats, model.numberOfRegions, model.maxNumberOfComps)
        assert np.allclose(trans, otrans, rtol=1e-10, atol=1e-12 * otrans.max())
    finally:
        orc.close()
