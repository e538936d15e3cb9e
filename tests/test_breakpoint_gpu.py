"""Exact breakpoint posteriors on the GPU (hf_get_breakpoints, hf_get_breakpoint_profile, hmm.EMList.breakpoints / breakpoint_profile,
hmm_flagger --runBoundaries) against the numpy references of tests/breakpoint_ref.py, which form them another way: a forward over the
whole chunk with a column mask per window (route (i)), the prefix / suffix recursion in long double (route (ii)) and path enumeration.

Tolerances, those of the interval getter's tests: log_p_event |dev - ref| <= 1e-10 + 1e-9 |ref| (-inf equal to -inf); p_k and mode_p
|dev - ref| <= 1e-12 + 1e-9 ref; sum_k p_k within 1e-10 of 1.  Quantiles and the mode are indices and are checked by a band: a quantile k
for probability q passes iff c_ref[k] >= q - 1e-9 and c_ref[k - 1] < q + 1e-9, a mode iff p_ref[mode] >= max p_ref - (1e-12 + 1e-9 max).

Largest errors observed on an MI355X (every value test prints its own): log_p_event 1.14e-12, p_k and mode_p 9.4e-14, |sum p_k - 1|
4.4e-16."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from test_breakpoint_cpu import TINY, tiny, tiny_jobs
from test_viterbi_gpu import SIZES, _trained
import breakpoint_ref as BR
import geometry_cases as G
import hip_streams as HS
import runs_ref as RR
import sampling_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
ESTEP = os.path.join(ROOT, "flagger_amd", "csrc", "hf_estep.hip")
ALGOS = [N.HF_ALGO_SCAN, N.HF_ALGO_SEQ]
PROBS = (0.025, 0.5, 0.975)
NAMES = ["Err", "Dup", "Hap", "Col"]


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
def _lpe_close(dev, ref, what):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.isneginf(dev) & np.isneginf(ref)) | (np.abs(dev - ref) <= 1e-10 + 1e-9 * np.abs(ref))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (what, [(int(i), float(dev[i]), float(ref[i])) for i in bad[:8]])
    fin = np.isfinite(ref)
    return float(np.max(np.abs(dev[fin] - ref[fin]))) if fin.any() else 0.0


def _p_close(dev, ref, what):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    err = np.abs(dev - ref)
    bad = np.flatnonzero(~(err <= 1e-12 + 1e-9 * ref))
    assert bad.size == 0, (what, [(int(i), float(dev[i]), float(ref[i])) for i in bad[:8]])
    return float(err.max()) if err.size else 0.0


def _check(em, F, L, U, V, events, what, profiles=True, probs=PROBS):
    """Every output of a call against the reference's log P(E_k) per job; returns the device's outputs."""
    lpe, quant, mode, mode_p = em.breakpoints(F, L, U, V, probs)
    assert not np.any(np.isnan(lpe)) and not np.any(np.isnan(mode_p)), what
    assert np.all(lpe <= 1e-12), (what, float(lpe.max()))
    ref = [BR.summary(e) for e in events]
    e_lpe = _lpe_close(lpe, [r[0] for r in ref], what)
    e_p = e_mp = e_sum = 0.0
    for j, (lr, pr) in enumerate(ref):
        a, b = int(F[j]), int(L[j])
        if not np.isfinite(lr):
            assert np.isneginf(lpe[j]) and mode[j] == -1 and np.all(quant[j] == -1) and mode_p[j] == 0.0, (what, j)
            if profiles:
                p, lp1 = em.breakpoint_profile(a, b, int(U[j]), int(V[j]))
                assert np.isneginf(lp1) and np.all(p == 0.0), (what, j)
            continue
        for q, k in zip(probs, quant[j]):
            assert BR.quantile_ok(pr, a, k, q, 1e-9), (what, j, a, b, q, int(k))
        assert BR.mode_ok(pr, a, mode[j]), (what, j, int(mode[j]))
        e_mp = max(e_mp, _p_close([mode_p[j]], [pr.max()], (what, "mode_p", j)))
        if profiles:
            p, lp1 = em.breakpoint_profile(a, b, int(U[j]), int(V[j]))
            assert p.size == b - a and np.array(lp1).tobytes() == lpe[j].tobytes(), (what, j)
            e_p = max(e_p, _p_close(p, pr, (what, "profile", j)))
            e_sum = max(e_sum, abs(float(p.sum()) - 1.0))
            assert abs(float(p.sum()) - 1.0) <= 1e-10, (what, j)
            # against the device's own profile: bitwise mode, a 1e-10 band for the quantiles
            assert mode_p[j] == p.max() and mode[j] == a + 1 + int(np.argmax(p)), (what, j)
            for q, k in zip(probs, quant[j]):
                assert BR.quantile_ok(p, a, k, q, 1e-10), (what, "own profile", j, q, int(k))
    print("%s: %d jobs; max |d log_p_event| %.3g, max |d p_k| %.3g, max |d mode_p| %.3g, max |sum p - 1| %.3g"
          % (what, len(ref), e_lpe, e_p, e_mp, e_sum))
    return lpe, quant, mode, mode_p


def _not_empty(events, what):
    """The conditions that keep a value test from passing emptily, on the REFERENCE values."""
    ref = [BR.summary(e) for e in events]
    finite = [r for r in ref if np.isfinite(r[0])]
    assert 2 * len(finite) >= len(ref), (what, len(finite), len(ref))
    wide = [r for r in finite if r[1].size >= 8]
    spread = [r for r in wide if r[1].max() < 0.99]
    assert wide and 4 * len(spread) >= len(wide), (what, len(spread), len(wide))


def _disjoint_masks(rng, n):
    U = rng.integers(1, 15, n)
    V = np.array([rng.choice([v for v in range(1, 16) if not (v & int(u))]) for u in U], np.int64)
    return U.astype(np.int64), V


def _pass(store, model, algo=N.HF_ALGO_SCAN, stream=0):
    em = hmm.EMList(store, model, algo=algo, stream=stream)
    hmm.EM_runOneIterationForList(em, model)                # the pass whose model the getter answers for
    return em


# ---- 1. tiny stores: route (i) and enumeration -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_reference(model_type, seed):
    store, model, alpha, A, end = tiny(model_type, seed)
    off = np.asarray(store.chunk_off, np.int64)
    F, L, U, V = tiny_jobs(store, seed)
    events = [BR.masked_events(A, end, off, a, b, u, v) for a, b, u, v in zip(F, L, U, V)]
    for j in range(0, F.size, 5):                           # and enumeration, where the chunk is small enough
        c = BR.chunk_of(off, F[j])
        if off[c + 1] - off[c] <= 7:
            brute = BR.brute_force(A, end, off, F[j], L[j], U[j], V[j])
            with np.errstate(invalid="ignore"):
                assert np.all((np.isneginf(brute) & np.isneginf(events[j])) | (np.abs(brute - events[j]) <= 1e-10))
    return (F, L, U, V), events


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("model_type,seed", TINY)
def test_tiny_stores_equal_reference(algo, model_type, seed):
    store, model, _, _, _ = tiny(model_type, seed)
    (F, L, U, V), events = _tiny_reference(model_type, seed)
    em = _pass(store, model, algo)
    _check(em, F, L, U, V, events, "tiny %d algo %d" % (seed, algo))
    em.close()


def test_a_job_without_weight():
    """One off-diagonal transition entry zeroed in every region before the pass: the job from that state to the other has no weight."""
    model_type, seed = TINY[1]                              # (one region: no region change takes the zeroed entry's place)
    store, model0, alpha, _, _ = tiny(model_type, seed)
    model = model0.copy()
    R = model.numberOfRegions
    v = model.param_vector().reshape(R, -1)
    for r in range(R):
        v[r, :25].reshape(5, 5)[2, 3] = 0.0                 # Hap -> Col
    model.set_param_vector(v.ravel())
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    a, b = int(off[-2]), int(off[-1]) - 1
    F, L, U, V = (np.array(x, np.int64) for x in ([a, a, a + 3], [b, b, a + 9], [4, 8, 4], [8, 4, 8]))
    events = [BR.masked_events(A, end, off, f, l, u, w) for f, l, u, w in zip(F, L, U, V)]
    assert np.all(np.isneginf(events[0])) and np.all(np.isneginf(events[2])) and np.any(np.isfinite(events[1]))
    for algo in ALGOS:
        em = _pass(store, model, algo)
        lpe, quant, mode, mode_p = _check(em, F, L, U, V, events, "no weight, algo %d" % algo)
        assert np.isneginf(lpe[0]) and np.all(quant[0] == -1) and mode[0] == -1 and mode_p[0] == 0.0
        em.close()


# ---- 2. the grid store: the piece grid, the lane scans and the chain ------------------------------------------------------------------------
# the jobs (every pair a < b of the boundary points inside one chunk, a random left mask and its complement) and their reference, route
# (ii), are geometry_cases.breakpoint_reference: tests/test_geometry_gpu.py runs them on the variants of the grid store as well
_grid_reference = G.breakpoint_reference


@pytest.mark.parametrize("model_type,seed,algo", [(mt, s, N.HF_ALGO_SCAN) for mt, s in G.CASES] + [G.CASES[0] + (N.HF_ALGO_SEQ,)])
def test_grid_store_equals_reference(model_type, seed, algo):
    import test_geometry_gpu as TG                          # (here: that module imports this one)
    store, model, _, _ = G.case(model_type, seed)
    em = _pass(store, model, algo)
    TG.check_breakpoints(em, model_type, seed, "grid %d algo %d" % (seed, algo), profile_every=1)      # every job, every profile
    em.close()


# ---- 3. a trained model, the command line's jobs ---------------------------------------------------------------------------------------
def boundaries(labels, store):
    """The command line's rule: the runs of the labels (a new run where the label changes or a chunk starts another contig); for every two
    adjacent runs of one contig (m, left, right, job), job = (first, last, U, V) or None where m is a chunk start."""
    off = np.asarray(store.chunk_off, np.int64)
    ctg = list(store.chunk_ctg)
    runs, pre = [], None                                    # [a, b) label chunk-of-a; the contig of the chunk before
    for c in range(off.size - 1):
        for t in range(int(off[c]), int(off[c + 1])):
            new_ctg = t == off[c] and pre != ctg[c]
            pre = ctg[c]
            if not runs or new_ctg or runs[-1][2] != labels[t]:
                runs.append([t, t, int(labels[t]), c])
            runs[-1][1] = t + 1
    out = []
    for l, r in zip(runs[:-1], runs[1:]):
        m = r[0]
        c = r[3]
        if ctg[BR.chunk_of(off, l[0])] != ctg[c]:
            continue
        job = None
        if m != off[c] and l[2] != r[2]:
            job = (max(l[0], int(off[c])), min(r[1], int(off[c + 1])) - 1, 1 << l[2], 1 << r[2])
        out.append((m, l[2], r[2], job))
    return out


def test_trained_model_with_the_command_lines_jobs():
    store = synth.config(2, 0.04)
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, K, synth.HIFI_ALPHA)
    hmm.EM_runOneIterationForList(em, model)
    jobs = [b[3] for b in boundaries(em.labels(), store) if b[3] is not None]
    assert len(jobs) >= 20
    F, L, U, V = (np.array(x, np.int64) for x in zip(*jobs))
    A, end = S.rows(store, model, synth.HIFI_ALPHA)
    events = BR.LongDouble(A, end, store.chunk_off).events(F, L, U, V)
    _not_empty(events, "trained")
    lpe, quant, mode, mode_p = _check(em, F, L, U, V, events, "trained config 2")
    assert np.all(quant[:, 0] <= quant[:, 1]) and np.all(quant[:, 1] <= quant[:, 2])
    got = hmm.EM_getBreakpointsForList(em, F, L, U, V)
    assert all(np.array_equal(x, y) for x, y in zip(got, (lpe, quant, mode, mode_p)))
    em.close()


# ---- 7. invariants ----------------------------------------------------------------------------------------------------------------------
def test_invariants():
    model_type, seed = G.CASES[0]
    store, model, alpha, _ = G.case(model_type, seed)
    (F, L, U, V), _ = _grid_reference(model_type, seed)
    em = _pass(store, model)
    lpe, quant, mode, mode_p = em.breakpoints(F, L, U, V)
    assert not np.any(np.isnan(lpe)) and np.all(lpe <= 1e-12)
    # the three events "one switch U -> V", "all in U", "all in V" are disjoint subsets of "all in U | V"
    iv = em.interval_log_probs
    lhs = np.exp(lpe) + np.exp(iv(F, L, U)) + np.exp(iv(F, L, V))
    rhs = np.exp(iv(F, L, U | V))
    assert np.all(lhs <= rhs * (1 + 1e-9)), float(np.max(lhs / np.maximum(rhs, 1e-300)))
    # a two-window job: the pair posterior mass from hf_get_forward_backward and the rows
    A, _ = G.rows(model_type, seed)
    f, b, _ = em.forward_backward()
    two = np.flatnonzero(L - F == 1)
    assert two.size >= 10
    want = np.empty(two.size)
    for i, j in enumerate(two):
        x = f[F[j]][:, None] * A[L[j]] * b[L[j]][None, :]
        inU, inV = ((U[j] >> np.arange(4)) & 1).astype(bool), ((V[j] >> np.arange(4)) & 1).astype(bool)
        want[i] = x[np.ix_(inU, inV)].sum() / x.sum()
    with np.errstate(divide="ignore"):
        _lpe_close(lpe[two], np.log(want), "two-window jobs")
    assert np.all(mode[two][np.isfinite(lpe[two])] == L[two][np.isfinite(lpe[two])])
    assert np.all(mode_p[two][np.isfinite(lpe[two])] == 1.0)
    em.close()


# ---- 8. bitwise independence -------------------------------------------------------------------------------------------------------------
def _same_bits(x, y):
    return all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(x, y))


def test_a_jobs_outputs_do_not_depend_on_the_call():
    model_type, seed = G.CASES[0]
    store, model, _, _ = G.case(model_type, seed)
    (F, L, U, V), _ = _grid_reference(model_type, seed)
    em = _pass(store, model)
    base = em.breakpoints(F, L, U, V)
    rng = np.random.default_rng(4)
    perm = rng.permutation(F.size)
    assert _same_bits(em.breakpoints(F[perm], L[perm], U[perm], V[perm]), [x[perm] for x in base])
    h = F.size // 3
    halves = [em.breakpoints(F[s], L[s], U[s], V[s]) for s in (slice(0, h), slice(h, None))]
    assert _same_bits([np.concatenate([x, y]) for x, y in zip(*halves)], base)
    dup = np.concatenate([np.arange(F.size), np.arange(0, F.size, 3)])
    assert _same_bits(em.breakpoints(F[dup], L[dup], U[dup], V[dup]), [x[dup] for x in base])
    order = [2, 0, 1]
    re_ = em.breakpoints(F, L, U, V, [PROBS[i] for i in order])
    assert _same_bits([re_[0], re_[1], re_[2], re_[3]], [base[0], base[1][:, order], base[2], base[3]])
    none = em.breakpoints(F, L, U, V, [])
    assert none[1].shape == (F.size, 0) and _same_bits([none[0], none[2], none[3]], [base[0], base[2], base[3]])
    for j in range(0, F.size, 7):                          # the profile call against the batch call
        p, lp1 = em.breakpoint_profile(F[j], L[j], U[j], V[j])
        assert np.array(lp1).tobytes() == base[0][j].tobytes()
        if base[2][j] >= 0:
            assert base[3][j] == p.max() and base[2][j] == F[j] + 1 + int(np.argmax(p))
    em.close()


# ---- 9. more than one device batch -------------------------------------------------------------------------------------------------------
def _caps():
    text = open(ESTEP).read()
    caps = {}
    for name in ("HF_BP_BATCH_PIECES", "HF_BP_BATCH_PARTS"):
        m = re.search(r"#define\s+%s\s+\(1\s*<<\s*(\d+)\)" % name, text)
        assert m, name
        caps[name] = 1 << int(m.group(1))
    return caps


def test_second_device_batch():
    """Two-window fillers up to two pieces short of the cap, the three-piece job across it, more fillers: every value has the bits of
    the job asked alone."""
    model_type, seed = G.CASES[0]
    store, model, _, _ = G.case(model_type, seed)
    caps = _caps()
    cap = caps["HF_BP_BATCH_PIECES"]
    assert caps["HF_BP_BATCH_PARTS"] >= cap                 # (a part has a piece: the pieces' cap binds)
    off = np.asarray(G.OFF, np.int64)
    rng = np.random.default_rng(12)
    chunk = np.searchsorted(off, np.arange(G.N_WINDOWS), "right") - 1
    t2 = np.unique(np.concatenate([G.POINTS[G.POINTS + 1 < G.N_WINDOWS], rng.integers(0, G.N_WINDOWS - 1, 200)]))
    t2 = t2[chunk[t2] == chunk[t2 + 1]]
    F = np.concatenate([t2, [3073]])
    L = np.concatenate([t2 + 1, [4172]])
    U, V = _disjoint_masks(rng, F.size)
    _, pieces = G.pieces_of(off, F, L)
    big = F.size - 1
    assert np.all(pieces[:big] == 1) and pieces[big] == 3
    order = np.concatenate([np.resize(np.arange(big), cap - 2), [big], np.resize(np.arange(big)[::-1], 700)])
    starts = G._batches(np.ones(order.size, np.int64), pieces[order], cap, caps["HF_BP_BATCH_PARTS"])
    assert starts == [0, cap - 1], starts                   # the three-piece job closes the first batch
    em = _pass(store, model)
    alone = [em.breakpoints(F[i:i + 1], L[i:i + 1], U[i:i + 1], V[i:i + 1]) for i in range(F.size)]
    alone = [np.concatenate([a[k] for a in alone]) for k in range(4)]
    got = em.breakpoints(F[order], L[order], U[order], V[order])
    assert _same_bits(got, [a[order] for a in alone])
    assert np.isfinite(alone[0]).sum() >= F.size // 4
    small = em.breakpoints(F[-5:], L[-5:], U[-5:], V[-5:])  # the buffer after it has grown: a small call answers as before
    assert _same_bits(small, [a[-5:] for a in alone])
    em.close()


# ---- 10. paths and variants ---------------------------------------------------------------------------------------------------------------
def _variant_case():
    store = synth.synthesize([n * 1000 for n in SIZES], 1000, 10 ** 9, [20], seed=11)
    off = np.asarray(store.chunk_off, np.int64)
    rng = np.random.default_rng(8)
    F, L = [], []
    for c in np.flatnonzero(np.diff(off) > 1):
        for _ in range(6):
            a = int(rng.integers(off[c], off[c + 1] - 1))
            F.append(a)
            L.append(int(rng.integers(a + 1, min(off[c + 1], a + 1 + int(rng.choice([2, 40, 1500]))))))
    F, L = np.array(F, np.int64), np.array(L, np.int64)
    U, V = _disjoint_masks(rng, F.size)
    return store, (F, L, U, V)


_CHILD = """
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from flagger_amd import hmm, synth
from flagger_amd import _native as N
from test_breakpoint_gpu import _variant_case
from test_viterbi_gpu import _trained
store, (F, L, U, V) = _variant_case()
em0, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, iters=1)
em0.close()
os.environ[sys.argv[3]] = sys.argv[4]
em = hmm.EMList(store, model)
assert (em.seg_launches == 2) if sys.argv[3] == "HF_SEG_LAUNCHES" else (em.sub_passes >= 2)
hmm.EM_runOneIterationForList(em, model)
lpe, quant, mode, mode_p = em.breakpoints(F, L, U, V)
np.savez(sys.argv[2], lpe=lpe, quant=quant, mode=mode, mode_p=mode_p)
em.close()
"""


@pytest.mark.parametrize("name,value", [("HF_SEG_LAUNCHES", "2"), ("HF_SUBPASSES", "3")])
def test_launch_modes_and_sub_passes_give_the_same_bits(name, value, tmp_path):
    store, (F, L, U, V) = _variant_case()
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, iters=1)
    hmm.EM_runOneIterationForList(em, model)
    base = em.breakpoints(F, L, U, V)
    A, end = S.rows(store, model, synth.HIFI_ALPHA)
    _check(em, F, L, U, V, BR.LongDouble(A, end, store.chunk_off).events(F, L, U, V), "variant base", profiles=False)
    em.close()
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "tests"), out, name, value], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")])))
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert _same_bits([z["lpe"], z["quant"], z["mode"], z["mode_p"]], base)


def test_seq_agrees_with_scan():
    store, (F, L, U, V) = _variant_case()
    em, model = _trained(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, iters=1)
    hmm.EM_runOneIterationForList(em, model)
    scan = em.breakpoints(F, L, U, V)
    seq_em = _pass(store, model, N.HF_ALGO_SEQ)
    seq = seq_em.breakpoints(F, L, U, V)
    _lpe_close(seq[0], scan[0], "seq against scan")
    _p_close(seq[3], scan[3], "seq against scan, mode_p")
    for j in np.flatnonzero(np.isfinite(scan[0]))[::5]:
        p, _ = em.breakpoint_profile(F[j], L[j], U[j], V[j])
        ps, _ = seq_em.breakpoint_profile(F[j], L[j], U[j], V[j])
        _p_close(ps, p, ("seq against scan, profile", int(j)))
        for q, k in zip(PROBS, seq[1][j]):
            assert BR.quantile_ok(p, F[j], k, q, 1e-9)
        assert BR.mode_ok(p, F[j], seq[2][j])
    em.close(); seq_em.close()


def test_errors():
    store = synth.config(2, 0.02)
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, store, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model)
    L_ = N.lib()
    off = np.asarray(store.chunk_off, np.int64)
    n = store.n_windows
    i64p, u8p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_double)

    def call(cnt, f, l, u, v, probs=PROBS, n_probs=None, null=()):
        arr = dict(f=np.array(f, np.int64), l=np.array(l, np.int64), u=np.array(u, np.uint8), v=np.array(v, np.uint8),
                   probs=np.array(probs, np.float64), lpe=np.empty(max(cnt, 1)), quant=np.empty((max(cnt, 1), 8), np.int64),
                   mode=np.empty(max(cnt, 1), np.int64), mode_p=np.empty(max(cnt, 1)))
        typ = dict(f=i64p, l=i64p, u=u8p, v=u8p, probs=dp, lpe=dp, quant=i64p, mode=i64p, mode_p=dp)
        p = {k: (None if k in null else a.ctypes.data_as(typ[k])) for k, a in arr.items()}
        rc = L_.hf_get_breakpoints(em._h, cnt, p["f"], p["l"], p["u"], p["v"], len(probs) if n_probs is None else n_probs, p["probs"],
                                   p["lpe"], p["quant"], p["mode"], p["mode_p"])
        if rc != N.HF_OK:
            assert rc == N.HF_E_ARG and b"hf_get_breakpoints" in L_.hf_last_error()
        return rc

    def profile(f, l, u, v, null=()):
        p, lp = np.empty(max(l - f, 1)), np.empty(1)
        rc = L_.hf_get_breakpoint_profile(em._h, f, l, u, v, None if "p" in null else p.ctypes.data_as(dp),
                                          None if "lpe" in null else lp.ctypes.data_as(dp))
        if rc != N.HF_OK:
            assert rc == N.HF_E_ARG and b"hf_get_breakpoint_profile" in L_.hf_last_error()
        return rc

    ok = ([0], [3], [1], [4])
    assert call(1, *ok) == N.HF_E_ARG and profile(0, 3, 1, 4) == N.HF_E_ARG          # no pass yet
    hmm.EM_runForwardForList(em, model)
    assert call(1, *ok) == N.HF_E_ARG and profile(0, 3, 1, 4) == N.HF_E_ARG          # forward-only
    hmm.EM_runOneIterationForList(em, model)
    assert call(1, *ok) == N.HF_OK and profile(0, 3, 1, 4) == N.HF_OK
    assert call(0, [], [], [], [], null=("f", "l", "u", "v", "lpe", "quant", "mode", "mode_p", "probs"), n_probs=0) == N.HF_OK
    assert call(-1, *ok) == N.HF_E_ARG
    for k in ("f", "l", "u", "v", "lpe", "mode", "mode_p", "quant", "probs"):
        assert call(1, *ok, null=(k,)) == N.HF_E_ARG, k
    assert call(1, *ok, null=("quant", "probs"), n_probs=0) == N.HF_OK               # neither is read without probabilities
    assert profile(0, 3, 1, 4, null=("p",)) == N.HF_E_ARG and profile(0, 3, 1, 4, null=("lpe",)) == N.HF_E_ARG
    for f, l in [(-1, 0), (0, n), (5, 4), (n, n)]:                                   # the ranges of the interval getter
        assert call(1, [f], [l], [1], [4]) == N.HF_E_ARG, (f, l)
    assert call(1, [3], [3], [1], [4]) == N.HF_E_ARG and profile(3, 3, 1, 4) == N.HF_E_ARG          # first == last
    c = int(np.flatnonzero(np.diff(off) > 1)[0])
    assert call(1, [off[c + 1] - 1], [off[c + 1]], [1], [4]) == N.HF_E_ARG                           # two chunks
    assert profile(int(off[c + 1]) - 1, int(off[c + 1]), 1, 4) == N.HF_E_ARG
    for u, v in [(0, 4), (16, 4), (1, 0), (1, 16), (3, 6), (15, 15), (255, 1)]:                      # masks: range, overlap
        assert call(1, [0], [3], [u], [v]) == N.HF_E_ARG, (u, v)
        assert profile(0, 3, u, v) == N.HF_E_ARG, (u, v)
    assert call(1, *ok, n_probs=-1) == N.HF_E_ARG and call(1, *ok, probs=[0.5] * 9) == N.HF_E_ARG
    for q in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert call(1, *ok, probs=[0.5, q]) == N.HF_E_ARG, q
    assert call(2, [0, 0], [3, 3], [1, 1], [4, 1]) == N.HF_E_ARG                     # any bad job refuses the call
    with pytest.raises(N.HFError):
        em.breakpoints([0], [0], [1], [4])
    lpe, quant, mode, mode_p = em.breakpoints([0], [3], [1], [14], [0.5] * 8)         # and the context still answers afterwards
    assert lpe[0] <= 1e-12 and quant.shape == (1, 8)
    em.close()


def test_on_a_callers_stream_behind_filler_work():
    model_type, seed = G.CASES[0]
    store, model, _, _ = G.case(model_type, seed)
    (F, L, U, V), _ = _grid_reference(model_type, seed)
    twin = _pass(store, model)
    base = twin.breakpoints(F, L, U, V)
    j = int(np.argmax(L - F))
    base_p = twin.breakpoint_profile(F[j], L[j], U[j], V[j])
    twin.close()
    with HS.Streams() as streams:
        s = streams.new(True)
        h = HS.hip()
        em = hmm.EMList(store, model, stream=s)
        h.delay(s)
        hmm.EM_runOneIterationForList(em, model)
        h.delay(s)
        got = em.breakpoints(F, L, U, V)                    # (the first call: behind the lazy re-run of the segment kernel)
        h.delay(s)
        got_p = em.breakpoint_profile(F[j], L[j], U[j], V[j])
        assert _same_bits(got, base) and _same_bits(got_p, base_p)
        em.close()


# ---- 11. command line --------------------------------------------------------------------------------------------------------------------
def _cli(args, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


def _rows(path):
    return [l.split("\t") for l in path.read_text().splitlines() if not l.startswith("#")]


@pytest.mark.parametrize("viterbi", [False, True])
def test_cli_run_boundaries(tmp_path, viterbi):
    store = RR.split_store(synth.config(2, 0.04))          # chunks cut, so that boundaries fall on chunk starts inside a contig
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    args = ["-i", str(binp), "-W", "4000", "-n", "2", "-t", "0.001", "-f", "0.95", "-p", str(K), "--uncertaintySamples", "4"] + \
        (["--viterbi"] if viterbi else [])
    _cli(args, tmp_path / "plain")
    _cli(args + ["--runBoundaries"], tmp_path / "bnd")
    _cli(args + ["--runBoundaries", "--runConfidence", "--numBlocks"], tmp_path / "more")
    a, b, m = tmp_path / "plain", tmp_path / "bnd", tmp_path / "more"
    names = sorted(os.listdir(a))
    assert sorted(set(os.listdir(b)) - set(names)) == ["final_label_run_boundaries.tsv"]
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    assert (b / "final_label_run_boundaries.tsv").read_bytes() == (m / "final_label_run_boundaries.tsv").read_bytes()
    text = (b / "final_label_run_boundaries.tsv").read_text().splitlines()
    assert text[0] == "#ctg\tpos\tleft\tright\tp_event\tp_called\tlo\tmedian\thi\tmode\tmode_p"
    rows = [l.split("\t") for l in text[1:]]
    # the same run through the bindings: the final model, its last full pass, the final labels
    st = synth.WindowStore.read_bin(str(binp))
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, np.zeros((4, 4)))
    em = hmm.EMList(st, model)
    hmm.runHMMFlagger(em, model, 2, 0.001)
    labels = em.viterbi(model)[0] if viterbi else em.labels()
    off = np.asarray(st.chunk_off, np.int64)
    bnd = boundaries(labels, st)
    # one row per boundary of final_label_runs_support.bed: two adjacent rows of one contig
    sup = _rows(b / "final_label_runs_support.bed")
    pairs = [(x, y) for x, y in zip(sup[:-1], sup[1:]) if x[0] == y[0]]
    assert len(rows) == len(pairs) == len(bnd)
    inside = [x for x in bnd if x[3] is not None]
    assert len(inside) >= 20 and len(inside) < len(bnd)     # boundaries inside chunks, and some on chunk starts
    base = lambda t: int(st.chunk_s[BR.chunk_of(off, t)]) + (int(t) - int(off[BR.chunk_of(off, t)])) * 4000
    n_na = 0
    for row, (x, y), (mwin, ll, rl, job) in zip(rows, pairs, bnd):
        assert row[:4] == [y[0], y[1], x[3], y[3]] and row[2:4] == [NAMES[ll], NAMES[rl]] and int(row[1]) == base(mwin), row
        if job is None:
            assert row[4:] == ["NA"] * 7, row
            n_na += 1
            continue
        f, l, u, v = job
        lpe, quant, mode, mode_p = em.breakpoints([f], [l], [u], [v])
        if not np.isfinite(lpe[0]):
            assert row[4:] == ["NA"] * 7, row
            n_na += 1
            continue
        p, _ = em.breakpoint_profile(f, l, u, v)
        want = ["%.6g" % np.exp(lpe[0]), "%.6g" % p[mwin - f - 1]] + [str(base(k)) for k in quant[0]] + [str(base(mode[0])), "%.6g" % mode_p[0]]
        assert row[4:] == want, (row, want)
        assert int(row[6]) <= int(row[7]) <= int(row[8]), row
    assert n_na == len(bnd) - len(inside) or n_na > len(bnd) - len(inside)
    em.close()
