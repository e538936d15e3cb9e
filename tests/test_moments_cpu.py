"""CPU checks of the exact count moments' ground: the three routes of the numpy reference (tests/moments_ref.py: path enumeration,
pairwise joint posteriors, the uncentred long-double jet) against one another, the C ABI entry point (declared, exported, bound) and the
command line's --exactTotals option (help text, refusals made before the input is read).

The tolerance of the device tests is sized here: test_centred_float64_against_the_long_double_jet prints the largest relative deviation of
the gamma-centred float64 recursion from route (c) over the jobs of the tiny stores and of the reduced configs (see tests/test_moments_gpu.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_bruteforce_cpu import _tiny_store
from test_cli_prefix_cpu import CLI, unique_prefixes
from test_interval_cpu import BUILD, NEW
from test_viterbi_cpu import perturbed_model
import moments_ref as MR
import sampling_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm_flagger_hip.h")
TINY = [(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 0), (N.HF_MODEL_GAUSSIAN, 1), (N.HF_MODEL_NEGATIVE_BINOMIAL, 2)]


def tiny_case(model_type, seed):
    """The store, model and jobs of the tiny-store tests (CPU and GPU): chunks of 7, 5, 1, 6, 3 and 40 windows."""
    rng = np.random.default_rng(2750 + seed)
    alpha = synth.HIFI_ALPHA if seed % 2 == 0 else np.zeros((4, 4))
    regions = [20, 31] if seed % 2 == 0 else [25]
    store = _tiny_store(rng, [7, 5, 1, 6, 3, 40], regions)
    model = perturbed_model(store, model_type, 2 + seed % 3, alpha, rng)
    return store, model, alpha, MR.jobs(store, rng, 200, all_regions=True)


RTOL, ATOL = 3.3e-12, 1e-12       # the device tests' |dev - ref| <= ATOL scale + RTOL ref (scale: 1 windows^2, window_len^2 bases^2)


def rel_dev(got, ref, scale):
    """The largest relative deviation over the jobs whose variance is worth the name (ref > 1e-3 scale: the jobs the device tests count);
    the other jobs must agree within ATOL scale."""
    got, ref = np.asarray(got), np.asarray(ref)
    big = ref > 1e-3 * scale
    assert np.all(np.abs(got - ref)[~big] <= ATOL * scale)
    return float(np.max(np.abs(got - ref)[big] / ref[big], initial=0.0))


@pytest.mark.parametrize("model_type,seed", TINY)
def test_three_routes_agree_on_tiny_stores(model_type, seed):
    store, model, alpha, (F, L, M, R) = tiny_case(model_type, seed)
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    reg = store.regions().astype(np.int64)
    # route (a) where it can go, the chunks of <= 7 windows: every such job of the set, and every mask on every small chunk as a whole and
    # on every sub-range of the 5-window chunk, without and with every region filter
    small = np.flatnonzero(L < off[5])
    assert small.size >= 20
    first = np.array([off[c] for c in range(5)] + [a for a in range(off[1], off[2]) for b in range(a, off[2])], np.int64)
    last = np.array([off[c + 1] - 1 for c in range(5)] + [b for a in range(off[1], off[2]) for b in range(a, off[2])], np.int64)
    ea, em_, er = (x.ravel() for x in np.meshgrid(np.arange(first.size), np.arange(1, 16), np.arange(-1, store.n_regions), indexing="ij"))
    Fa, La, Ma, Ra = np.concatenate([F[small], first[ea]]), np.concatenate([L[small], last[ea]]), np.concatenate([M[small], em_]), \
        np.concatenate([R[small], er])
    for unit in MR.UNITS:
        w = MR.weights(store, unit)
        scale = float(store.window_len) ** 2 if unit == "bases" else 1.0
        mb, vb = MR.moments(A, end, off, w, reg, F, L, M, R)
        mc, vc = MR.moments_long(A, end, off, w, reg, F, L, M, R)
        assert np.allclose(mb, mc, rtol=1e-11, atol=1e-12 * np.sqrt(scale))
        assert np.allclose(vb, vc, rtol=1e-9, atol=1e-12 * scale)
        ma, va = MR.brute_force(A, end, off, w, reg, Fa, La, Ma, Ra)
        for route in (MR.moments, MR.moments_long):
            m2, v2 = route(A, end, off, w, reg, Fa, La, Ma, Ra)
            assert np.allclose(ma, m2, rtol=1e-11, atol=1e-12 * np.sqrt(scale))
            assert np.allclose(va, v2, rtol=1e-9, atol=1e-12 * scale)
        full = M == 15
        assert np.all(np.abs(vb[full]) <= 1e-12 * scale)
        wsum = np.array([np.where((r < 0) | (reg[a:b + 1] == r), w[a:b + 1], 0.0).sum() for a, b, r in zip(F[full], L[full], R[full])])
        assert np.allclose(mb[full], wsum, rtol=1e-12)
        assert np.sum(vb > 1e-3 * scale) >= 20


def test_bases_weights_are_the_final_bed_lengths():
    store = synth.synthesize([10_500, 4_000, 900], 1000, 10 ** 9, [20], seed=3)
    w = MR.weights(store, "bases")
    assert w.sum() == sum(int(e) - int(s) + 1 for s, e in zip(store.chunk_s, store.chunk_e))
    off = np.asarray(store.chunk_off, np.int64)
    assert w[off[1] - 1] == 500 and w[off[3] - 1] == 900 and np.all(w[:off[1] - 1] == 1000)


def test_centred_float64_against_the_long_double_jet():
    """Sizes the tolerance of the device tests: the largest relative deviation of the gamma-centred float64 recursion from route (c) over
    the jobs of GPU tests 1 and 2 is 3.3e-14 (printed below; cfg 2); RTOL is a hundredfold of it, and under the standing 1e-9."""
    worst = 0.0
    for mt, seed in TINY:
        store, model, alpha, (F, L, M, R) = tiny_case(mt, seed)
        A, end = S.rows(store, model, alpha)
        reg = store.regions().astype(np.int64)
        for unit in MR.UNITS:
            w = MR.weights(store, unit)
            scale = float(store.window_len) ** 2 if unit == "bases" else 1.0
            _, vc = MR.moments_long(A, end, store.chunk_off, w, reg, F, L, M, R)
            _, v64 = MR.moments_centred(A, end, store.chunk_off, w, reg, F, L, M, R)
            worst = max(worst, rel_dev(v64, vc, scale))
    print("tiny stores: max relative deviation %.3e" % worst)
    for cfg, mt, hifi in REDUCED:
        store, model, alpha, (F, L, M, R) = reduced_case(cfg, mt, hifi)
        A, end = S.rows(store, model, alpha)
        reg = store.regions().astype(np.int64)
        w = MR.weights(store, "windows")
        _, vc = MR.moments_long(A, end, store.chunk_off, w, reg, F, L, M, R)
        _, v64 = MR.moments_centred(A, end, store.chunk_off, w, reg, F, L, M, R)
        dev = rel_dev(v64, vc, 1.0)
        print("cfg %d: max relative deviation %.3e, jobs with var > 1e-3: %d" % (cfg, dev, int(np.sum(vc > 1e-3))))
        worst = max(worst, dev)
        assert np.sum(vc > 1e-3) >= 20                      # the reference alone: a kernel that returns zeros cannot pass the device tests
    print("overall: %.3e" % worst)
    assert 100.0 * worst <= RTOL <= 1e-9


REDUCED = [(2, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, True), (4, N.HF_MODEL_GAUSSIAN, True), (6, N.HF_MODEL_NEGATIVE_BINOMIAL, False)]


def reduced_case(cfg, model_type, hifi, model=None):
    """The store and jobs of the reduced-config tests; on the CPU with a perturbed initial model, on the GPU with the trained one."""
    store = synth.config(cfg, 0.04)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    rng = np.random.default_rng(40 + cfg)
    if model is None:
        model = perturbed_model(store, model_type, 3, alpha, np.random.default_rng(cfg))
    return store, model, alpha, MR.jobs(store, rng, 300, piece=512, lane=8)


def test_declared_exported_and_bound():
    """The getter is declared in the public header, exported by the library and bound in _native and hmm."""
    text = open(HEADER).read()
    assert re.search(r"int\s+hf_get_count_moments\s*\(\s*hf_ctx\s*\*\s*ctx\s*,\s*int64_t\s+n\s*,", text)
    assert re.search(r"HF_COUNT_WINDOWS\s*=\s*0\s*,\s*HF_COUNT_BASES\s*=\s*1", text)
    f = getattr(N.lib(), "hf_get_count_moments")
    assert f.restype is not None and len(f.argtypes) == 9
    assert (N.HF_COUNT_WINDOWS, N.HF_COUNT_BASES) == (0, 1)
    assert hasattr(hmm.EMList, "count_moments") and hasattr(hmm, "EM_getCountMomentsForList")


# ---- command line --------------------------------------------------------------------------------------------------------------
def test_help_names_the_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--exactTotals" in r.stderr + r.stdout


def test_every_prefix_resolves_as_before(tmp_path):
    """--exactTotals shares "e" and "ex" with --exchange, an earlier addition of this build: those two keep meaning --exchange (its bad
    value is what the command line complains about), every longer prefix of either name resolves to that name, and every other option's
    prefixes are untouched."""
    def run(*args):
        r = subprocess.run([CLI, "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path)] + list(args), capture_output=True, text=True)
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and "undefined option" not in r.stderr, (args, r.stderr[-300:])
        return r.stderr
    for p in ("--e", "--ex", "--exc", "--exchange"):
        assert "--exchange" in run(p, "no_such_exchange"), p
        assert "--exchange" in run(p + "=no_such_exchange"), p
    for p in ("--exa", "--exact", "--exactTotals"):
        err = run(p, "--gpus", "2")
        assert "--exactTotals" in err and "--exchange" not in err, p
    before = dict(unique_prefixes(list(BUILD) + list(NEW)))
    now = dict(unique_prefixes(list(BUILD) + list(NEW) + ["exactTotals"]))
    lost = {p: n for p, n in before.items() if now.get(p) != n}
    assert lost == {"e": "exchange", "ex": "exchange"}, lost


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--sweepAlpha", "x"]])
def test_refused_combinations(tmp_path, extra):
    """Refused before the input is read and before any device use: the input named here does not exist, so only the refusal can be the
    error."""
    r = subprocess.run([CLI, "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--exactTotals"] + extra,
                       capture_output=True, text=True)
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert r.returncode != 0
    assert len(lines) == 1 and "--exactTotals" in lines[0], r.stderr[-500:]
