"""CPU checks of the exact run moments' ground: the routes of the numpy reference (tests/runs_ref.py: path enumeration with the dynamic
programme over the chunks, explicit joint probabilities, the uncentred long-double jet) against one another, with and without joins
between the chunks, the C ABI entry point (declared, exported, bound) and the command line's --numBlocks option (help text, prefixes,
refusals made before the input is read).

The tolerance of the device tests is sized here: test_centred_float64_against_the_long_double_jet prints the largest relative deviation of
the centred float64 recursion from route (c) over the jobs of the tiny stores and of the reduced configs (see tests/test_runs_gpu.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm
from test_cli_prefix_cpu import CLI, unique_prefixes
from test_interval_cpu import BUILD, NEW
from test_moments_cpu import REDUCED, TINY, reduced_case, tiny_case
import moments_ref as MR
import runs_ref as RR
import sampling_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm_flagger_hip.h")
TINY_JOINS = np.array([0, 1, 1, 1, 0, 1], bool)       # over the chunks of 7, 5, 1, 6, 3, 40 windows: the 1-window chunk inside a joined group

# the device tests' |dev - ref| <= ATOL + RTOL scale (runs^2; scale: the variance, or with joins the sum of the absolute values of the
# stitching formula's terms: runs_ref.stitch)
RTOL, ATOL = 2e-11, 1e-12


def tiny_jobs(model_type, seed):
    """The store, model and jobs of the tiny-store tests (CPU and GPU): the jobs of the count-moments tests without their region
    filter, and every mask on every small chunk, on every sub-range of the 5-window chunk and on the five small chunks together."""
    store, model, alpha, (F, L, M, _) = tiny_case(model_type, seed)
    off = np.asarray(store.chunk_off, np.int64)
    first = np.array([off[c] for c in range(5)] + [0] + [a for a in range(off[1], off[2]) for b in range(a, off[2])], np.int64)
    last = np.array([off[c + 1] - 1 for c in range(5)] + [off[5] - 1] + [b for a in range(off[1], off[2]) for b in range(a, off[2])], np.int64)
    ea, em_ = (x.ravel() for x in np.meshgrid(np.arange(first.size), np.arange(1, 16), indexing="ij"))
    return store, model, alpha, (np.concatenate([F, first[ea]]), np.concatenate([L, last[ea]]), np.concatenate([M, em_]))


def reduced_jobs(cfg, model_type, hifi, split, model=None):
    """The store, model and jobs of the reduced-config tests (CPU and GPU).  split False: reduced_case as it is; every contig of these
    stores is one chunk, so the contig rule joins nothing.  split True: the same windows with the chunks cut (runs_ref.split_store), so
    that the contig rule joins chunks, and the jobs of moments_ref.jobs on those chunks."""
    store, model, alpha, (F, L, M, _) = reduced_case(cfg, model_type, hifi, model)
    if split:
        store = RR.split_store(store)
        F, L, M, _ = MR.jobs(store, np.random.default_rng(140 + cfg), 300, piece=512, lane=8)
    return store, model, alpha, (F, L, M)


def rel_dev(got, ref, scale):
    """The largest deviation relative to the scale over the jobs whose variance is worth the name (ref > 1e-3: the jobs the device
    tests count); the other jobs must agree within ATOL."""
    got, ref, scale = np.asarray(got), np.asarray(ref), np.asarray(scale)
    big = ref > 1e-3
    assert np.all(np.abs(got - ref)[~big] <= ATOL + RTOL * scale[~big])
    return float(np.max(np.abs(got - ref)[big] / scale[big], initial=0.0))


@pytest.mark.parametrize("joins", [None, TINY_JOINS], ids=["apart", "joined"])
@pytest.mark.parametrize("model_type,seed", TINY)
def test_three_routes_agree_on_tiny_stores(model_type, seed, joins):
    store, model, alpha, (F, L, M) = tiny_jobs(model_type, seed)
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    assert list(np.diff(off)) == [7, 5, 1, 6, 3, 40]
    mb, vb, sb = RR.pairwise(A, end, off, F, L, M, joins)
    mc, vc, sc = RR.jet_long(A, end, off, F, L, M, joins)
    assert np.allclose(mb, mc, rtol=1e-11, atol=1e-12)
    assert np.all(np.abs(vb - vc) <= 1e-12 + 1e-10 * sb)
    small = L < off[5]                                   # route (a) where it can go: the chunks of <= 7 windows
    assert small.sum() >= 21 * 15 + 20
    ma, va = RR.brute_force(A, end, off, F[small], L[small], M[small], joins)
    for m2, v2, s2 in ((mb, vb, sb), (mc, vc, sc)):
        assert np.allclose(ma, m2[small], rtol=1e-11, atol=1e-12)
        assert np.all(np.abs(va - v2[small]) <= 1e-12 + 1e-10 * s2[small])
    # the one-window chunk between two joins is inside jobs of route (a)
    assert np.any(small & (F <= off[2] - 1) & (L >= off[3]))
    full = M == 15
    assert full.sum() >= 20
    assert np.all(np.abs(vb[full]) <= 1e-12) and np.all(va[M[small] == 15] <= 1e-12)
    assert np.allclose(mb[full], RR.groups(off, F[full], L[full], joins), rtol=1e-12)
    assert np.sum(vb > 1e-3) >= 20
    if joins is not None:                                # the joins matter: without them some jobs count more blocks
        m0, _, _ = RR.pairwise(A, end, off, F, L, M, None)
        assert np.sum(m0 - mb > 1e-3) >= 20 and np.all(m0 - mb >= -1e-12)


def test_all_states_give_the_group_count():
    off = np.array([0, 7, 12, 13, 19, 22, 62], np.int64)
    F = np.array([0, 0, 3, 12, 7, 19, 20], np.int64)
    L = np.array([61, 21, 12, 12, 18, 61, 61], np.int64)
    assert list(RR.groups(off, F, L, None)) == [6, 5, 3, 1, 3, 2, 2]
    assert list(RR.groups(off, F, L, TINY_JOINS)) == [2, 2, 1, 1, 1, 1, 1]


def test_centred_float64_against_the_long_double_jet():
    """Sizes the tolerance of the device tests: the largest deviation of the centred float64 recursion from route (c), relative to the
    scale of runs_ref.stitch, over the jobs of GPU tests 1 and 2 (printed below); RTOL is at least a hundredfold of it, and under the
    standing 1e-9."""
    worst = 0.0
    for mt, seed in TINY:
        store, model, alpha, (F, L, M) = tiny_jobs(mt, seed)
        A, end = S.rows(store, model, alpha)
        for joins in (None, TINY_JOINS):
            _, vc, sc = RR.jet_long(A, end, store.chunk_off, F, L, M, joins)
            _, v64, _ = RR.jet_centred(A, end, store.chunk_off, F, L, M, joins)
            print("tiny store %d: jobs with var > 1e-3: %d of %d" % (seed, int(np.sum(vc > 1e-3)), vc.size))
            assert np.sum(vc > 1e-3) >= 20
            worst = max(worst, rel_dev(v64, vc, sc))
    print("tiny stores: max relative deviation %.3e" % worst)
    for cfg, mt, hifi in REDUCED:
        for split in (False, True):
            store, model, alpha, (F, L, M) = reduced_jobs(cfg, mt, hifi, split)
            A, end = S.rows(store, model, alpha)
            joins = RR.contig_joins(store)
            assert joins.sum() >= (40 if split else 0)
            mc, vc, sc = RR.jet_long(A, end, store.chunk_off, F, L, M, joins)
            _, v64, _ = RR.jet_centred(A, end, store.chunk_off, F, L, M, joins)
            dev = rel_dev(v64, vc, sc)
            print("cfg %d%s: max relative deviation %.3e, jobs with var > 1e-3: %d, largest variance %.3f"
                  % (cfg, " cut" if split else "", dev, int(np.sum(vc > 1e-3)), vc.max()))
            worst = max(worst, dev)
            assert np.sum(vc > 1e-3) >= 20                  # the reference alone: a kernel that returns zeros cannot pass the device tests
            if split:                                       # and the joins matter to the jobs that span them
                m0, v0, _ = RR.jet_long(A, end, store.chunk_off, F, L, M, None)
                assert np.sum(m0 - mc > 1e-3) >= 20 and np.sum(np.abs(v0 - vc) > 1e-3) >= 20
    print("overall: %.3e" % worst)
    assert 100.0 * worst <= RTOL <= 1e-9


def test_declared_exported_and_bound():
    """The getter is declared in the public header, exported by the library and bound in _native and hmm."""
    text = open(HEADER).read()
    assert re.search(r"int\s+hf_get_run_moments\s*\(\s*hf_ctx\s*\*\s*ctx\s*,\s*int64_t\s+n\s*,", text)
    f = getattr(N.lib(), "hf_get_run_moments")
    assert f.restype is not None and len(f.argtypes) == 8
    assert hasattr(hmm.EMList, "run_moments") and hasattr(hmm, "EM_getRunMomentsForList")


# ---- command line --------------------------------------------------------------------------------------------------------------
def test_help_names_the_option():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--numBlocks" in r.stderr + r.stdout


def test_every_prefix_resolves_as_before(tmp_path):
    """No earlier option starts with "n": every prefix that resolved before resolves to the same option, and every prefix of
    --numBlocks resolves to it (its refusal with --gpus 2 is what the command line complains about)."""
    def run(*args):
        r = subprocess.run([CLI, "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path)] + list(args), capture_output=True, text=True)
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and "undefined option" not in r.stderr, (args, r.stderr[-300:])
        return r.stderr
    for p in ("--n", "--num", "--numBlocks"):
        assert "--numBlocks" in run(p, "--gpus", "2"), p
    for p in ("--exa", "--exact", "--exactTotals"):
        err = run(p, "--gpus", "2")
        assert "--exactTotals" in err and "--exchange" not in err, p
    for p in ("--e", "--ex"):
        assert "--exchange" in run(p, "no_such_exchange"), p
    earlier = list(BUILD) + list(NEW) + ["exactTotals"]
    before = dict(unique_prefixes(earlier))
    now = dict(unique_prefixes(earlier + ["numBlocks"]))
    assert {p: n for p, n in before.items() if now.get(p) != n} == {}
    assert all(now.get("numBlocks"[:k]) == "numBlocks" for k in range(1, 10))


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--sweepAlpha", "x"]])
def test_refused_combinations(tmp_path, extra):
    """Refused before the input is read and before any device use: the input named here does not exist, so only the refusal can be the
    error."""
    r = subprocess.run([CLI, "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--numBlocks"] + extra,
                       capture_output=True, text=True)
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert r.returncode != 0
    assert len(lines) == 1 and "--numBlocks" in lines[0], r.stderr[-500:]
