"""CPU checks of the ground of the admissible path sampler (hf_sample_paths_minlen): the numpy reference the GPU tests rely on
(tests/minlen_sample_ref.py) against mpmath enumeration of the admissible paths — the draw rule's probabilities exactly, the draw code
by a chi-square test — its all-ones case against sampling_ref.ffbs, and the command line's --admissibleSamples option (prefix,
refusals before the input is read)."""
import os
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from test_bruteforce_cpu import Params
from test_cli_prefix_cpu import CLI, REFERENCE, unique_prefixes
from test_minlen_post_cpu import EARLIER as BEFORE_POSTERIOR, OPTION as POSTERIOR
import minlen_ref
import minlen_sample_ref as R
import sampling_ref as S
import viterbi_ref

EARLIER = BEFORE_POSTERIOR + [POSTERIOR]
OPTION = "admissibleSamples"
ONES = (1, 1, 1, 1)


def _weights(store, model, alpha, model_type, seed, c):
    """[(path, weight)] of chunk c in 50 digits (minlen_ref.chunk_path_weights with the tiny case's parameters)."""
    regions = model.numberOfRegions
    P = Params(model.param_vector(), regions, 2 + seed % 3, model_type, alpha)
    nbE = None
    if model_type == N.HF_MODEL_NEGATIVE_BINOMIAL:
        p = model.params()
        nbE = np.ctypeslib.as_array(p.nb_E, shape=(regions * 4 * viterbi_ref.NX,)).reshape(regions, 4, viterbi_ref.NX).copy()
    return minlen_ref.chunk_path_weights(store, c, P, model, nbE)


@pytest.mark.parametrize("model_type,seed,hifi", minlen_ref.TINY_CASES)
def test_the_draw_rule_gives_every_admissible_path_its_share(model_type, seed, hifi):
    """The product of the conditional draw probabilities (from the weights, no drawing) is weight / Z_adm for every admissible path of
    every chunk, within 1e-12, and the products sum to 1 over the admissible paths."""
    store, model, alpha, _ = minlen_ref.tiny_case(model_type, seed, hifi)
    A, end = S.rows(store, model, alpha)
    worst = 0.0
    for min_len in minlen_ref.TINY_MIN_LENS:
        tab = R.tables(A, end, store.chunk_off, min_len)
        for c in range(store.n_chunks):
            w = [(path, wt) for path, wt in _weights(store, model, alpha, model_type, seed, c) if minlen_ref._path_ok(path, list(min_len))]
            za = sum(wt for _, wt in w)
            tot = 0.0
            for path, wt in w:
                pr = R.path_prob(tab, c, path)
                worst = max(worst, abs(pr - float(wt / za)))
                assert abs(pr - float(wt / za)) <= 1e-12, (min_len, c, path, pr, float(wt / za))
                tot += pr
            assert abs(tot - 1.0) <= 1e-12, (min_len, c, tot)
    print("largest |product of draw probabilities - weight / Z_adm|: %.3e" % worst)


def test_the_draw_code_samples_that_distribution():
    """20 000 reference samples of one tiny chunk under (3, 2, 2, 2): all admissible, and Pearson's chi-square of the path frequencies
    against enumeration (paths of expected count below 5 pooled into one cell) is at most dof + 5 sqrt(2 dof).  The chunk: seven windows
    of random rows with zeros among them, flat enough for some hundred paths to be seen (a fitted model leaves a handful)."""
    import itertools
    min_len = (3, 2, 2, 2)
    T = 7
    rng = np.random.default_rng(2718)
    A = rng.uniform(0.05, 1.0, (T, 4, 4)) * (rng.uniform(size=(T, 4, 4)) > 0.1)
    A[0, 1:] = 0.0                                                   # a chunk-first row: first[s] in row 0
    end = rng.uniform(0.1, 1.0, (1, 4))
    tab = R.tables(A, end, [0, T], min_len)
    n_s = 20_000
    labels = R.sample(tab, 4242, range(n_s))[0]
    assert all(minlen_ref._path_ok(row.tolist(), list(min_len)) for row in np.unique(labels, axis=0))
    code = lambda path: sum(int(s) * 4 ** (T - 1 - i) for i, s in enumerate(path))
    expect = np.zeros(4 ** T)
    for path in itertools.product(range(4), repeat=T):
        if minlen_ref._path_ok(path, list(min_len)):
            w = A[0, 0, path[0]] * end[0, path[-1]]
            for t in range(1, T):
                w *= A[t, path[t - 1], path[t]]
            expect[code(path)] = w
    expect *= n_s / expect.sum()
    counts = np.bincount((labels.astype(np.int64) * (4 ** np.arange(T - 1, -1, -1))).sum(axis=1), minlength=4 ** T).astype(np.float64)
    assert np.all(counts[expect == 0] == 0)
    big = expect >= 5
    cells_o = np.append(counts[big], counts[~big].sum())
    cells_e = np.append(expect[big], expect[~big].sum())
    keep = cells_e > 0
    chi2 = float(np.sum((cells_o[keep] - cells_e[keep]) ** 2 / cells_e[keep]))
    dof = int(keep.sum()) - 1
    print("chi-square %.2f over %d cells (dof %d, bound %.2f)" % (chi2, int(keep.sum()), dof, dof + 5 * np.sqrt(2 * dof)))
    assert dof >= 100
    assert chi2 <= dof + 5 * np.sqrt(2 * dof), (chi2, dof)


def _ragged():
    from flagger_amd import synth
    from test_bruteforce_cpu import _tiny_store
    from test_viterbi_cpu import perturbed_model
    rng = np.random.default_rng(321)
    store = _tiny_store(rng, [40, 1, 25, 2, 60, 7], [20, 31])
    model = perturbed_model(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, rng)
    return store, model, synth.HIFI_ALPHA


def test_all_ones_is_the_plain_sampler_bit_for_bit():
    store, model, alpha = _ragged()
    A, end = S.rows(store, model, alpha)
    want, wm, wf = S.ffbs(A, end, store.chunk_off, 9, range(3, 53))
    got, gm, gf = R.sample(R.tables(A, end, store.chunk_off, ONES), 9, range(3, 53))
    assert np.array_equal(got, want)
    first = np.zeros(store.n_windows, bool)
    first[np.asarray(store.chunk_off[:-1])] = True
    assert np.array_equal(gm[:, ~first], wm[:, ~first]) and np.array_equal(gf, wf)


def test_samples_depend_on_seed_and_index_only_and_are_admissible():
    store, model, alpha = _ragged()
    A, end = S.rows(store, model, alpha)
    min_len = (3, 5, 1, 7)
    tab = R.tables(A, end, store.chunk_off, min_len)
    whole = R.sample(tab, 5, range(64))[0]
    parts = np.concatenate([R.sample(tab, 5, range(24))[0], R.sample(tab, 5, range(24, 64))[0]])
    assert np.array_equal(whole, parts)
    assert not np.array_equal(whole, R.sample(tab, 6, range(64))[0])
    for row in whole:
        assert minlen_ref.admissible(row, store.chunk_off, min_len).all()
    free = S.ffbs(A, end, store.chunk_off, 5, range(64))[0]
    assert not all(minlen_ref.admissible(row, store.chunk_off, min_len).all() for row in free)   # the rule does bite on this store


# ---- command line ----------------------------------------------------------------------------------------------------------------

def test_option_keeps_every_reference_prefix_and_every_earlier_one():
    ref = unique_prefixes(list(REFERENCE))
    now = dict(unique_prefixes(list(REFERENCE) + EARLIER + [OPTION]))
    lost = [(p, n) for p, n in ref if now.get(p) != n]
    assert not lost, lost
    before = dict(unique_prefixes(list(REFERENCE) + EARLIER))
    assert {p: n for p, n in before.items() if now.get(p) != n} == {}
    assert now.get("ad") == OPTION and now.get("cons") == POSTERIOR


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("HF_LOOPBACK_RANKS", None)
    e.update(env or {})
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=e)


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_the_binary_resolves_the_prefix_and_names_the_option_in_its_help(tmp_path):
    for p in ("--ad", "--admissible", "--" + OPTION):
        r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), p, "4"])
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and "--admissibleSamples needs --minimumLengths" in r.stderr, p
    r = _run(["--help"])
    assert "--" + OPTION in r.stderr + r.stdout


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
@pytest.mark.parametrize("n,extra,env,needle", [
    ("4", [], {}, "needs --minimumLengths"),
    ("0", ["--minimumLengths", "1,2,3"], {}, "positive integer"),
    ("-3", ["--minimumLengths", "1,2,3"], {}, "positive integer"),
    ("x", ["--minimumLengths", "1,2,3"], {}, "positive integer"),
    ("4", ["--minimumLengths", "1,2,3", "--gpus", "2"], {}, "one GPU"),
    ("4", ["--minimumLengths", "1,2,3"], {"HF_LOOPBACK_RANKS": "2"}, "one GPU"),
    ("4", ["--minimumLengths", "1,2,3", "--sweepAlpha", "x"], {}, "one GPU"),
    ("4", ["-W", "1000", "--minimumLengths", "30000,20000,13001"], {}, "30,20,1,14"),
])
def test_refusals_come_before_the_input_is_read(tmp_path, n, extra, env, needle):
    """The input named here does not exist, so only the refusal can be the error."""
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--" + OPTION, n] + extra, env)
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert r.returncode != 0
    assert len(lines) == 1 and "--" + OPTION in lines[0] and needle in lines[0], r.stderr[-500:]


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_lengths_within_the_lane_budget_pass_the_option_checks(tmp_path):
    """30 + 20 + 1 + 13 = 64 windows: not refused; the run stops at the missing input."""
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--" + OPTION, "4", "-W", "1000", "--minimumLengths", "30000,20000,13000"])
    assert r.returncode != 0 and OPTION not in r.stderr
