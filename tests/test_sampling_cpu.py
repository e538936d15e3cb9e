"""CPU checks of the posterior path sampler's ground: the counter-based uniforms, the numpy sampler the GPU tests rely on
(tests/sampling_ref.py) against brute-force path probabilities and a numpy forward-backward, and the command line's
--uncertaintySamples / --uncertaintySeed options (prefixes, help text, refused combinations)."""
import os
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import synth
from test_bruteforce_cpu import _tiny_store
from test_cli_prefix_cpu import ADDED, CLI, REFERENCE, unique_prefixes
from test_viterbi_cpu import perturbed_model
import sampling_ref as S

NEW = {"uncertaintySamples": 1, "uncertaintySeed": 1}
BUILD = {**REFERENCE, **{n: 1 for n in ADDED}, "viterbi": 0, "sweepAlpha": 1}


def test_splitmix64_known_values():
    # the first outputs of the splitmix64 generator seeded with 0 (state += golden gamma, then the finaliser)
    assert S.splitmix64(0) == 0xE220A8397B1DCDAF
    assert S.splitmix64(S.GOLDEN) == 0x6E789E6AA1B965F4
    assert S.splitmix64((2 * S.GOLDEN) & S.M64) == 0x06C45D188009454F
    xs = np.array([0, S.GOLDEN, (2 * S.GOLDEN) & S.M64, 12345, S.M64], np.uint64)
    assert [int(v) for v in S.splitmix64(xs)] == [S.splitmix64(int(x)) for x in xs]   # the array form wraps like the integer form


def test_uniforms():
    key = S.sample_key(7, 3)
    assert key == S.splitmix64(7 ^ S.splitmix64(3))
    u = S.uniforms(key, np.arange(1000))
    assert u[5] == (S.splitmix64((key + 5) & S.M64) >> 11) * 2.0 ** -53
    assert np.all((u >= 0) & (u < 1)) and abs(u.mean() - 0.5) < 0.05
    assert S.sample_key(7, 3) != S.sample_key(8, 3) and S.sample_key(7, 3) != S.sample_key(7, 4)


def test_draw_rule_edges():
    W = np.array([[0.0, 2.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]])
    Cm = np.cumsum(W, axis=1)
    ch, _ = S._pick(W, Cm, np.array([0.0, 0.5, 0.999999]))
    assert ch.tolist() == [1, 0, 3]                  # u = 0 skips a zero-weight state; all zero -> 0
    ch, _ = S._pick(W[:1], Cm[:1], np.array([0.7]))
    assert ch.tolist() == [3]


def _tiny(seed, model_type, lengths):
    rng = np.random.default_rng(900 + seed)
    alpha = synth.HIFI_ALPHA if seed % 2 == 0 else np.zeros((4, 4))
    regions = [20, 31] if seed % 2 == 0 else [25]
    store = _tiny_store(rng, lengths, regions)
    model = perturbed_model(store, model_type, 2 + seed % 3, alpha, rng)
    return store, model, alpha


@pytest.mark.parametrize("model_type,seed", [(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 0), (N.HF_MODEL_GAUSSIAN, 1),
                                             (N.HF_MODEL_NEGATIVE_BINOMIAL, 2)])
def test_numpy_sampler_path_frequencies(model_type, seed):
    store, model, alpha = _tiny(seed, model_type, [5, 3, 6, 1])
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    n_s = 100_000
    fwd = S.forward(A, off)
    labels = np.concatenate([S.ffbs(A, end, off, 11 + seed, range(k0, k0 + 25_000), fwd)[0] for k0 in range(0, n_s, 25_000)])
    for c in range(store.n_chunks):
        t0, T = int(off[c]), int(off[c + 1] - off[c])
        probs = S.path_probs(A, end[c], t0, T)
        codes = (labels[:, t0:t0 + T].astype(np.int64) * (4 ** np.arange(T - 1, -1, -1))).sum(axis=1)
        freq = np.bincount(codes, minlength=4 ** T) / n_s
        exact = np.zeros(4 ** T)
        for path, pr in probs.items():
            exact[sum(s * 4 ** (T - 1 - i) for i, s in enumerate(path))] = pr
        tv = 0.5 * np.abs(freq - exact).sum()
        assert tv < 0.01, (c, T, tv)


@pytest.mark.parametrize("model_type,seed", [(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3), (N.HF_MODEL_GAUSSIAN, 4)])
def test_numpy_sampler_marginals(model_type, seed):
    store, model, alpha = _tiny(seed, model_type, [40, 25, 1, 60])
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    post = S.forward_backward(A, end, off)
    for c in range(store.n_chunks):                  # the forward-backward itself against brute force on a short chunk
        if off[c + 1] - off[c] <= 6:
            probs = S.path_probs(A, end[c], int(off[c]), int(off[c + 1] - off[c]))
            for t in range(int(off[c + 1] - off[c])):
                m = np.zeros(4)
                for path, pr in probs.items():
                    m[path[t]] += pr
                assert np.allclose(post[off[c] + t], m, atol=1e-12)
    n_s = 20_000
    labels = S.ffbs(A, end, off, 5, range(n_s))[0]
    freq = np.stack([(labels == s).mean(axis=0) for s in range(4)], axis=1)
    sd = np.sqrt(np.maximum(post * (1 - post), 1.0 / n_s) / n_s)   # (floor: a state of probability ~0 seen once is no evidence)
    assert np.max(np.abs(freq - post) / sd) < 5.5


def test_sample_depends_on_seed_and_index_only():
    store, model, alpha = _tiny(5, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, [30, 20])
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    a = S.ffbs(A, end, off, 9, range(0, 40))[0]
    b = np.concatenate([S.ffbs(A, end, off, 9, range(0, 15))[0], S.ffbs(A, end, off, 9, range(15, 40))[0]])
    assert np.array_equal(a, b)
    assert not np.array_equal(a, S.ffbs(A, end, off, 10, range(0, 40))[0])


# ---- command line --------------------------------------------------------------------------------------------------------------

def test_new_options_move_no_unique_prefix():
    """Every prefix that is unique among the reference's options, or among this build's, resolves to the same option afterwards."""
    for before in (list(REFERENCE), list(BUILD)):
        now = dict(unique_prefixes(list(BUILD) + list(NEW)))
        lost = [(p, n) for p, n in unique_prefixes(before) if now.get(p) != n]
        assert not lost, lost


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_the_binary_resolves_every_shortest_prefix(tmp_path):
    names = {**BUILD, **NEW}
    shortest = {}
    for p, n in unique_prefixes(list(names)):
        if n not in shortest or len(p) < len(shortest[n]):
            shortest[n] = p
    for n, p in shortest.items():
        args = [CLI, "--" + p] + (["1"] if names[n] else []) + ["-o", str(tmp_path)]
        r = subprocess.run(args, capture_output=True, text=True)
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and "undefined option" not in r.stderr, (p, r.stderr[-300:])


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_help_names_both_options():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--uncertaintySamples" in r.stderr + r.stdout and "--uncertaintySeed" in r.stderr + r.stdout


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--sweepAlpha", "list.txt"], [], ["--uncertaintySeed", "x"]])
def test_refused_combinations(tmp_path, extra):
    """Refused before the input is read: the input named here does not exist, so only the refusal can be the error."""
    n = "0" if not extra else "4"
    args = [CLI, "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--uncertaintySamples", n] + extra
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode != 0
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert len(lines) == 1 and "uncertainty" in lines[0], r.stderr[-500:]
