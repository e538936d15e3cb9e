"""CPU checks of the most-probable-path decoder's ground: the numpy reference the GPU tests rely on (tests/viterbi_ref.py) against
mpmath enumeration of all 4^T state paths, and the command line's --viterbi option (prefixes, help text)."""
import itertools
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_bruteforce_cpu import MAXC, Params, _tiny_store, beta_of
from test_cli_prefix_cpu import ADDED, CLI, REFERENCE, unique_prefixes
import viterbi_ref

mp.mp.dps = 50


def perturbed_model(store, model_type, K, alpha, rng):
    """createModel + a nudge of means / variances / transitions so that nothing is symmetric (as test_bruteforce_cpu)."""
    model = hmm.createModel(model_type, K, store, alpha)
    R = model.numberOfRegions
    v = model.param_vector().reshape(R, -1)
    if model_type != N.HF_MODEL_NEGATIVE_BINOMIAL:
        v[:, 27:27 + 4 * MAXC] *= rng.uniform(0.8, 1.2, size=(R, 4 * MAXC))
        v[:, 27 + 4 * MAXC:27 + 8 * MAXC] *= rng.uniform(0.8, 1.5, size=(R, 4 * MAXC))
    for r in range(R):
        t = v[r, :25].reshape(5, 5)
        t[:4, :4] *= rng.uniform(0.5, 2.0, size=(4, 4))
        t[:4, :4] *= ((1 - 1e-4) / t[:4, :4].sum(axis=1))[:, None]
        t[4, :4] = rng.uniform(0.1, 1.0, size=4)
        t[4, :4] /= t[4, :4].sum()
    model.set_param_vector(v.ravel())
    return model


def enumerate_map(store, c, P, model, nbE=None):
    """(best path, its log-weight, the second-best log-weight) of chunk c by enumeration in 50 digits."""
    t0, T = int(store.chunk_off[c]), int(store.chunk_off[c + 1] - store.chunk_off[c])
    x = [mp.mpf(int(store.cov[t0 + t]) & 0xff) for t in range(T)]
    reg = [int(store.annot[t0 + t] >> np.uint64(58)) for t in range(T)]
    beta = [beta_of(store, c, t, True, 0.95) for t in range(T)]
    L = N.lib()
    mx, mn, mc = L.hfm_max_high_mapq_ratio(model._h), L.hfm_min_high_mapq_ratio(model._h), L.hfm_min_highly_clipped_ratio(model._h)

    def emit(t, s, px, a):
        if nbE is not None:
            return mp.mpf(float(nbE[reg[t], s, int(x[t])]))
        return P.emit(reg[t], s, x[t], px, a, beta[t])

    first = [P.trans[reg[0]][4][s] * emit(0, s, mp.mpf(0), mp.mpf(0)) for s in range(4)]
    A = [None]
    for t in range(1, T):
        cov, mapq, clip = float(int(store.cov[t0 + t])), float(int(store.mapq[t0 + t])), float(int(store.clip[t0 + t]))
        A.append([[(mp.mpf(1) / 5 if reg[t] != reg[t - 1] else P.tcond(reg[t], pre, s, cov, mapq, clip, mx, mn, mc))
                   * emit(t, s, x[t - 1], P.alpha[pre][s]) for s in range(4)] for pre in range(4)])
    end = [P.trans[reg[T - 1]][s][4] for s in range(4)]
    best, second, arg = mp.mpf(0), mp.mpf(0), None
    for path in itertools.product(range(4), repeat=T):
        w = first[path[0]]
        for t in range(1, T):
            w *= A[t][path[t - 1]][path[t]]
        w *= end[path[-1]]
        if w > best:
            best, second, arg = w, best, path
        elif w > second:
            second = w
    return arg, mp.log(best), (mp.log(second) if second > 0 else mp.mpf("-inf"))


CASES = [(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 0, "hifi"), (N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 1, "zero"), (N.HF_MODEL_GAUSSIAN, 2, "hifi"),
         (N.HF_MODEL_GAUSSIAN, 3, "zero"), (N.HF_MODEL_NEGATIVE_BINOMIAL, 4, "zero")]


@pytest.mark.parametrize("model_type,seed,alpha_kind", CASES)
def test_numpy_reference_against_path_enumeration(model_type, seed, alpha_kind):
    rng = np.random.default_rng(700 + seed)
    alpha = synth.HIFI_ALPHA if alpha_kind == "hifi" else np.zeros((4, 4))
    regions = [20, 31] if seed % 2 == 0 else [25]
    store = _tiny_store(rng, [7, 5, 1, 6, 3], regions)
    K = 2 + seed % 3
    model = perturbed_model(store, model_type, K, alpha, rng)
    labels, score, plp = viterbi_ref.reference(store, model, alpha)
    P = Params(model.param_vector(), len(regions), K, model_type, alpha)
    nbE = None
    if model_type == N.HF_MODEL_NEGATIVE_BINOMIAL:
        p = model.params()
        nbE = np.ctypeslib.as_array(p.nb_E, shape=(len(regions) * 4 * viterbi_ref.NX,)).reshape(len(regions), 4, viterbi_ref.NX).copy()
    # the stores exercise what the definition has in it: masks that drop a column, region changes inside a chunk
    regs = (np.asarray(store.annot) >> np.uint64(58)).astype(int)
    if len(regions) > 1:
        assert any(regs[t] != regs[t - 1] for c in range(store.n_chunks)
                   for t in range(int(store.chunk_off[c]) + 1, int(store.chunk_off[c + 1])))
    checked = 0
    for c in range(store.n_chunks):
        path, lbest, l2 = enumerate_map(store, c, P, model, nbE)
        t0, t1 = int(store.chunk_off[c]), int(store.chunk_off[c + 1])
        assert abs(score[c] - float(lbest)) <= 1e-12 * abs(float(lbest)), (c, score[c], lbest)
        assert abs(plp(labels)[c] - float(lbest)) <= 1e-12 * abs(float(lbest))
        if lbest - l2 > mp.mpf("1e-9") * abs(lbest):
            assert tuple(int(v) for v in labels[t0:t1]) == path, (c, labels[t0:t1], path)
            checked += 1
    assert checked >= store.n_chunks - 1


def test_numpy_reference_ties_go_to_the_lowest_state():
    """Two identical states everywhere: the path must use the lower index (first-max, as posterior_label)."""
    logA = np.log(np.full((3, 4, 4), 0.25))
    logA[0] = -np.inf
    logA[0, 0, :] = np.log(0.25)
    logend = np.log(np.full((1, 4), 0.5))
    labels, score = viterbi_ref.viterbi(logA, logend, [0, 3])
    assert labels.tolist() == [0, 0, 0]
    assert abs(score[0] - (3 * np.log(0.25) + np.log(0.5))) < 1e-15


def test_viterbi_option_keeps_every_reference_prefix():
    ref = unique_prefixes(list(REFERENCE))
    now = dict(unique_prefixes(list(REFERENCE) + ADDED + ["viterbi"]))
    lost = [(p, n) for p, n in ref if now.get(p) != n]
    assert not lost, lost


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_help_mentions_viterbi():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--viterbi" in r.stderr + r.stdout
