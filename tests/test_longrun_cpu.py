"""CPU checks of the exact long-run probabilities' ground: the numpy reference (tests/longrun_ref.py: the run-length counter carried
through every chunk's posterior Markov chain) against path enumeration, with and without joins between the chunks, the L = 1 identity
against the interval reference, the lane-count formula, the share of the device tests' jobs that the -650 rule leaves out, the C ABI entry
point (declared, exported, bound) and the command line's --keptBlocks option (help text, prefixes, refusals made before the input is
read)."""
import os
import re
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm
from test_cli_prefix_cpu import CLI, unique_prefixes
from test_interval_cpu import BUILD, NEW
from test_bruteforce_cpu import _tiny_store
from test_moments_cpu import REDUCED, TINY, reduced_case, tiny_case
from test_viterbi_cpu import perturbed_model
from flagger_amd import synth
import interval_ref as IR
import longrun_ref as LR
import sampling_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm_flagger_hip.h")
TINY_JOINS = np.array([0, 1, 1, 1, 0, 1], bool)       # over the chunks of 7, 5, 1, 6, 3, 40 windows
FLOOR = -650.0                                        # a log is compared where the reference's value is >= FLOOR or exactly -inf


LENGTHS = {"tiny": [7, 5, 1, 6, 3, 40], "period": [63, 64, 65, 129, 7, 8, 9]}      # (the device renormalises every 8 steps)
JOINS = {"tiny": TINY_JOINS, "period": np.array([0, 1, 0, 1, 1, 0, 1], bool)}
STORE_SEED = 3600                                    # (chosen on the CPU: test_few_jobs_fall_under_the_floor)
SMALL_SPAN = (4, 16, 64)                               # the random ranges' lengths on the small stores


def store_case(model_type, seed, which):
    """The store, model and alpha of the device tests' small stores (CPU and GPU): chunk lengths LENGTHS[which]."""
    rng = np.random.default_rng(STORE_SEED + 10 * seed + (which == "period"))
    alpha = synth.HIFI_ALPHA if seed % 2 == 0 else np.zeros((4, 4))
    store = _tiny_store(rng, LENGTHS[which], [20, 31] if seed % 2 == 0 else [25])
    return store, perturbed_model(store, model_type, 2 + seed % 3, alpha, rng), alpha


def max_len(mask):
    """The largest L whose expanded chain fits 64 lanes."""
    return 56 // bin(int(mask)).count("1") + 2


def jobs(chunk_off, rng, n_random, span=(4, 64, 700, 3000), whole=True):
    """(first, last, mask, min_len) of the device tests: the whole track, single windows, whole chunks, chunk-spanning and random ranges;
    all 15 masks; L out of {1, 2, 3, 7, the range's length, that + 1}, cut to what 64 lanes hold; and the lane cap exactly met.
    whole False (the reduced configs, whose windows are nearly all Hap): no job over the whole track, and a range of more than 64 windows
    asks for the other labels only -- a run of 58 Hap windows in a thousand is so certain that the log of its complement lies under
    FLOOR."""
    off = np.asarray(chunk_off, np.int64)
    n = int(off[-1])
    live = np.flatnonzero(np.diff(off) > 0)
    F, L, M, K = [], [], [], []
    def add(a, b, m, k=None):
        a, b, m = int(a), int(b), int(m)
        if not whole and b - a + 1 > 64:
            m = (m & ~4) or (1, 2, 8)[int(rng.integers(0, 3))]
        if k is None:
            k = int(rng.choice([1, 2, 3, 7, b - a + 1, b - a + 2]))
        F.append(a); L.append(b); M.append(m); K.append(max(1, min(int(k), max_len(m))))
    for m in range(1, 16):
        if whole:
            add(0, n - 1, m, (1, 2, 3, 7)[m % 4])
        t = int(rng.integers(0, n))
        add(t, t, m, 1); add(t, t, m, 2)
    for c in live[:40]:
        for k in (1, 2, 3, 7, off[c + 1] - off[c], off[c + 1] - off[c] + 1):
            add(off[c], off[c + 1] - 1, rng.integers(1, 16), k)
    for i in range(min(40, live.size - 1)):
        c0 = live[i]
        c1 = live[min(live.size - 1, i + 1 + int(rng.integers(0, 3)))]
        add(rng.integers(off[c0], off[c0 + 1]), rng.integers(off[c1], off[c1 + 1]), rng.integers(1, 16))
    for _ in range(n_random):
        a = int(rng.integers(0, n))
        add(a, min(n - 1, a + int(rng.integers(0, 1 + int(rng.choice(span))))), rng.integers(1, 16))
    c = live[np.argmax(np.diff(off)[live])]                # the lane cap: 64 lanes exactly, on the longest chunk and across chunks
    for m, k in ((4, 58), (1, 58), (6, 30), (9, 30), (15, 16)):
        assert LR.lanes(m, k) == 64 and LR.lanes(m, k + 1) > 64 and max_len(m) == k
        add(off[c], off[c + 1] - 1, m, k)
        if whole:
            add(0, n - 1, m, k)
    return np.array(F, np.int64), np.array(L, np.int64), np.array(M, np.int64), np.array(K, np.int64)


def comparable(ref):
    """bool[n]: where a log of the reference is compared."""
    return (ref >= FLOOR) | np.isneginf(ref)


def close(dev, ref, rtol=1e-9, atol=1e-10):
    dev, ref = np.asarray(dev), np.asarray(ref)
    use = comparable(ref)
    with np.errstate(invalid="ignore"):
        ok = (np.isneginf(dev) & np.isneginf(ref)) | (np.abs(dev - ref) <= atol + rtol * np.abs(ref)) | ~use
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, [(int(i), float(dev[i]), float(ref[i])) for i in bad[:8]]
    return use


def _tiny_groups():
    """Ranges on the tiny chunks: inside one chunk, and over two chunks of at most 10 windows in sum."""
    off = np.array([0, 7, 12, 13, 19, 22, 62], np.int64)
    ranges = [(0, 6), (1, 5), (3, 3), (7, 11), (13, 18), (7, 12), (9, 12), (13, 21), (15, 20), (12, 18)]
    return off, ranges


@pytest.mark.parametrize("joins", [None, TINY_JOINS], ids=["apart", "joined"])
@pytest.mark.parametrize("model_type,seed", TINY)
def test_reference_equals_enumeration(model_type, seed, joins):
    store, model, alpha, _ = tiny_case(model_type, seed)
    A, end = S.rows(store, model, alpha)
    off, ranges = _tiny_groups()
    assert list(np.asarray(store.chunk_off)) == list(off)
    F, L, M, K = [], [], [], []
    for a, b in ranges:
        n = b - a + 1
        for m in (1, 2, 6, 11, 15):
            for k in (1, 2, 3, n, n + 1):
                F.append(a); L.append(b); M.append(m); K.append(k)
    F, L, M, K = (np.array(x, np.int64) for x in (F, L, M, K))
    rn, rs = LR.log_probs(A, end, off, F, L, M, K, joins)
    bn, bs = LR.brute_force(A, end, off, F, L, M, K, joins)
    close(rn, bn, rtol=1e-12, atol=1e-12)
    close(rs, bs, rtol=1e-12, atol=1e-12)
    assert np.all(comparable(bn) & comparable(bs))
    # the exact cases: a range shorter than L, and all four states with L within the range
    n = L - F + 1
    if joins is None:                                        # (apart, a range over two chunks is two groups, each shorter still)
        assert np.all(rn[K > n] == 0.0) and np.all(np.isneginf(rs[K > n]))
    inside = (M == 15) & (K <= n) & (F >= 0) & (L <= 6)      # one chunk
    assert inside.sum() >= 4 and np.all(np.isneginf(rn[inside])) and np.all(rs[inside] == 0.0)
    assert np.sum(np.isfinite(rn) & (rn < -1e-6)) >= 50      # the jobs say something
    if joins is not None:                                    # the joins matter
        un, us = LR.log_probs(A, end, off, F, L, M, K, None)
        differ = ~((un == rn) | (np.abs(un - rn) <= 1e-6)) | ~((us == rs) | (np.abs(us - rs) <= 1e-6 * np.abs(rs)))
        assert np.sum(differ) >= 10


@pytest.mark.parametrize("model_type,seed", TINY)
def test_length_one_is_the_interval_identity(model_type, seed):
    store, model, alpha, _ = tiny_case(model_type, seed)
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    F, L, M, _ = jobs(off, np.random.default_rng(seed), 100, span=(4, 30))
    none, some = LR.log_probs(A, end, off, F, L, M, 1, TINY_JOINS)
    part = M != 15
    iv = IR.log_probs(A, end, off, F[part], L[part], 15 & ~M[part])
    assert np.all(np.abs(none[part] - iv)[np.isfinite(iv)] <= 1e-11 + 1e-11 * np.abs(iv[np.isfinite(iv)]))
    assert np.array_equal(np.isneginf(none[part]), np.isneginf(iv))
    assert np.all(np.isneginf(none[~part])) and np.all(some[~part] == 0.0)


def test_lane_formula():
    for m in range(1, 16):
        k = bin(m).count("1")
        for n in (1, 2, 7, 16, 30, 58):
            assert LR.lanes(m, n) == (4 - k) + k * (n - 1) + 4
        assert LR.lanes(m, max_len(m)) <= 64 < LR.lanes(m, max_len(m) + 1)
    assert [max_len(m) for m in (1, 3, 7, 15)] == [58, 30, 20, 16]


def test_few_jobs_fall_under_the_floor():
    """The device tests compare a log where the reference's is >= -650 or -inf; at most 5 % of their jobs may be left out.  Checked here
    for the job sets and seeds those tests use (the reduced configs with the CPU tests' perturbed model)."""
    for mt, seed in TINY:
        for which in LENGTHS:
            store, model, alpha = store_case(mt, seed, which)
            A, end = S.rows(store, model, alpha)
            F, L, M, K = jobs(store.chunk_off, np.random.default_rng(seed), 200, span=SMALL_SPAN)
            for joins in (None, JOINS[which]):
                none, some = LR.log_probs(A, end, store.chunk_off, F, L, M, K, joins)
                out = 1.0 - np.mean(comparable(none) & comparable(some))
                print("%s store %d: %d jobs, %.2f %% left out" % (which, seed, F.size, 100 * out))
                assert out <= 0.05
    cfg, mt, hifi = REDUCED[0]
    store, model, alpha, _ = reduced_case(cfg, mt, hifi)
    A, end = S.rows(store, model, alpha)
    F, L, M, K = jobs(store.chunk_off, np.random.default_rng(3200 + cfg), 200, whole=False)
    none, some = LR.log_probs(A, end, store.chunk_off, F, L, M, K, None)
    out = 1.0 - np.mean(comparable(none) & comparable(some))
    print("cfg %d: %d jobs, %.2f %% left out" % (cfg, F.size, 100 * out))
    assert out <= 0.05


def test_declared_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"int\s+hf_get_long_run_log_probs\s*\(\s*hf_ctx\s*\*\s*ctx\s*,\s*int64_t\s+n\s*,", text)
    assert re.search(r"#define\s+HF_LONGRUN_MAX_LANES\s+64", text)
    f = getattr(N.lib(), "hf_get_long_run_log_probs")
    assert f.restype is not None and len(f.argtypes) == 9
    assert hasattr(hmm.EMList, "long_run_log_probs") and hasattr(hmm, "EM_getLongRunLogProbsForList")


# ---- command line --------------------------------------------------------------------------------------------------------------
def test_help_names_the_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--keptBlocks" in r.stderr + r.stdout


def test_every_prefix_resolves_as_before(tmp_path):
    """No earlier option starts with "k": every prefix that resolved before resolves to the same option, and every prefix of
    --keptBlocks resolves to it."""
    def run(*args):
        r = subprocess.run([CLI, "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path)] + list(args), capture_output=True, text=True)
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and "undefined option" not in r.stderr, (args, r.stderr[-300:])
        return r.stderr
    for p in ("--k", "--kept", "--keptBlocks"):
        assert "--keptBlocks" in run(p, "--gpus", "2"), p
    earlier = list(BUILD) + list(NEW) + ["exactTotals", "numBlocks", "runBoundaries", "enforceMinimumLengths"]
    before = dict(unique_prefixes(earlier))
    now = dict(unique_prefixes(earlier + ["keptBlocks"]))
    assert {p: n for p, n in before.items() if now.get(p) != n} == {}
    assert all(now.get("keptBlocks"[:k]) == "keptBlocks" for k in range(1, 11))


@pytest.mark.parametrize("extra,word", [(["--minimumLengths", "3,5,7", "--gpus", "2"], "--keptBlocks"),
                                        (["--minimumLengths", "3,5,7", "--sweepAlpha", "x"], "--keptBlocks"),
                                        ([], "--minimumLengths"),
                                        (["--minimumLengths", "400000,5,7", "-W", "4000"], "400000")])
def test_refused_combinations(tmp_path, extra, word):
    """Refused before the input is read and before any device use: the input named here does not exist, so only the refusal can be the
    error.  The last case: a length whose expanded chain needs more than 64 lanes, named in the message."""
    r = subprocess.run([CLI, "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--keptBlocks"] + extra,
                       capture_output=True, text=True)
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert r.returncode != 0
    assert len(lines) == 1 and "--keptBlocks" in lines[0] and word in lines[0], r.stderr[-500:]
