"""The posterior and the sampler under minimum run lengths over whole contigs on the GPU (hf_minlen_posterior_joined,
hf_sample_paths_minlen_joined, EMList.minlen_posterior(joined=...), EMList.sample_paths_minlen(joined=...), hmm_flagger --mergedChunks)
against the float64 numpy reference (tests/minlen_sum_joined_ref.py) and, on the tiny stores, the 50-digit enumeration of every joined
group.

Tolerances are those of the per-chunk features' tests, imported and not restated: test_minlen_post_gpu._check (log_mass and log Z_adm
within 1e-10 + 1e-9 |ref|, post within 1e-9 relative where the reference is at least 1e-250, labels the first largest entry of post),
minlen_post_ref's enumeration tolerances (1e-12 (1 + |log Z|); post 1e-12 absolute + 1e-9 relative), and for the sampler the margin rule
of test_minlen_sample_gpu.py (a sample may differ from the reference only behind a draw whose reference margin is below 1e-12, at most
one such event per check; every store and seed below was checked on the CPU to hold no reference margin below 1e-9).  Admissibility over
the groups is an exact integer check of every sample (minlen_joined_ref.short_inner_runs).

THE BOUNDARY STORE.  test_minlen_joined_gpu's lengths (joined boundaries at windows 63, 127 and 192 of a group of 321 windows, whose
last block of 64 holds ONE window; at 15, 31, 48, 79 and 111 of a group of 144) and two groups of three chunks: 8 + 1 + 54 = 63 windows
(one partial block of 63; boundaries at positions 8 and 9: 0 and 1 mod 8 from the group's first window, 55 = 7 mod 8 steps from its last)
and 7 + 2 + 118 = 127 windows (a last block of 63; boundaries at 7 and 9: 7 and 1 mod 8 from the first window, 120 = 0 mod 8 from the
last); the boundary at 192 of the first group is 129 = 1 mod 8 steps from that group's last window."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
from hip_streams import Streams
from test_bruteforce_cpu import _tiny_store
from test_sampling_gpu import _near_tie_events
import test_sampling_gpu as TSG
from test_viterbi_cpu import perturbed_model
import floor_cases as FC
import geometry_cases as G
import minlen_joined_ref as JR
import minlen_ref
import minlen_sample_ref as SR
import minlen_sum_joined_ref as R
import sampling_ref as S
import test_minlen_gpu as TML
import test_minlen_joined_gpu as TJ
import test_minlen_post_gpu as TMP
import viterbi_ref

pytestmark = pytest.mark.gpu
ALGOS = TML.ALGOS
ONES = TML.ONES
TRACK_LEN = TML.TRACK_LEN
LENS = [(3, 5, 1, 7), (16, 16, 16, 16), (61, 1, 1, 1), ONES]
_same = TMP._same

BOUNDARY_LENGTHS = TJ.GEOMETRY_LENGTHS + [8, 1, 54] + [7, 2, 118]
BOUNDARY_JOINED = TJ.GEOMETRY_JOINED + [0, 1, 1] + [0, 1, 1]
BOUNDARY_SEED = 11
SAMPLE_SEED = 29


def _post(em, model, min_len, joined):
    """(post, labels, chunk_log_mass, chunk_log_z_adm, log_mass) of one call, the posterior fetched."""
    r = hmm.EM_runMinLengthPosteriorForList(em, model, min_len, joined)
    return r.posterior(), r.labels, r.chunk_log_mass, r.chunk_log_z_adm, r.log_mass


def _check_post(store, joined, ref, got, what):
    TMP._check(store, ref, got, what)
    inner = sorted(set(range(store.n_chunks)) - set(JR.group_first_chunks(store.chunk_off, joined).tolist()))
    assert np.all(got[2][inner] == 0.0) and np.all(got[3][inner] == 0.0)          # exactly 0.0 in a group's other chunks


def _check_samples(off, joined, ref, got, min_len, first=0):
    """`got` = samples first .. of the reference's under the margin rule, every one admissible over its group."""
    lab, marg, fmarg = (x[first:first + got.shape[0]] for x in ref)
    assert got.shape == lab.shape and got.dtype == np.int8
    events = _near_tie_events(got, lab, marg, fmarg, R.group_chunk_offsets(off, joined))
    assert events <= 1, events
    for k, row in enumerate(got):
        assert R.admissible_over_groups(row, off, joined, min_len), ("sample", k)


def _quiet_reference(ref):
    """The reference alone leaves nothing to the margin rule: no draw it takes lies within 1e-9 of a boundary."""
    assert float(ref[1].min()) >= 1e-9 and float(ref[2].min()) >= 1e-9
    return ref


@functools.lru_cache(maxsize=None)
def _boundary():
    rng = np.random.default_rng(BOUNDARY_SEED)
    store = _tiny_store(rng, BOUNDARY_LENGTHS, [20, 31])
    model = perturbed_model(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, rng)
    goff = JR.group_offsets(store.chunk_off, BOUNDARY_JOINED)[0]
    assert goff.tolist() == [0, 321, 465, 528, 655]
    return store, model, viterbi_ref.tables(store, model, synth.HIFI_ALPHA), S.rows(store, model, synth.HIFI_ALPHA)


@functools.lru_cache(maxsize=None)
def _boundary_refs(min_len, joined=tuple(BOUNDARY_JOINED)):
    store, model, (logA, logend), (A, end) = _boundary()
    post = R.posterior_tables(logA, logend, store.chunk_off, joined, min_len)
    smp = SR.sample(R.sample_tables(A, end, store.chunk_off, joined, min_len), SAMPLE_SEED, range(65), store.n_windows)
    return post, smp


# ---- tiny stores against enumeration ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("case", minlen_ref.TINY_CASES)
def test_tiny_stores_equal_group_enumeration(algo, case):
    store, model, alpha, _ = minlen_ref.tiny_case(*case)
    logA, logend = viterbi_ref.tables(store, model, alpha)
    A, end = S.rows(store, model, alpha)
    off = store.chunk_off
    em = hmm.EMList(store, model, algo=algo)
    checked = 0
    for joined in JR.TINY_JOINS:
        for ml in minlen_ref.TINY_MIN_LENS:
            got = _post(em, model, ml, joined)
            checked += R.check_against_enumeration(store, case, joined, ml, got[0], got[2], got[3], post_rel=1e-9)
            _check_post(store, joined, R.posterior_tables(logA, logend, off, joined, ml), got, "tiny %s %s" % (joined, ml))
            if ml == ONES:
                assert np.all(got[2] == 0.0) and got[4] == 0.0
            smp = em.sample_paths_minlen(model, ml, 64, 17, joined=joined)
            _check_samples(off, joined, SR.sample(R.sample_tables(A, end, off, joined, ml), 17, range(64)), smp, ml)
    assert checked == 8
    em.close()


# ---- the boundary store ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_len", LENS)
def test_joined_boundaries_around_the_blocks_and_the_rescaling_period(min_len):
    store, model, _, _ = _boundary()
    off = store.chunk_off
    ref_post, ref_smp = _boundary_refs(min_len)
    _quiet_reference(ref_smp)
    posts, smps = [], []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        for _ in range(2):                                   # a second call: identical bits
            posts.append(_post(em, model, min_len, BOUNDARY_JOINED))
            smps.append(em.sample_paths_minlen(model, min_len, 65, SAMPLE_SEED, joined=BOUNDARY_JOINED))
        em.close()
    _check_post(store, BOUNDARY_JOINED, ref_post, posts[0], "boundary store %s" % (min_len,))
    _check_samples(off, BOUNDARY_JOINED, ref_smp, smps[0], min_len)
    assert all(_same(posts[0], p) for p in posts[1:]) and all(np.array_equal(smps[0], s) for s in smps[1:])
    if min_len == ONES:
        assert np.all(posts[0][2] == 0.0) and posts[0][4] == 0.0
    else:
        # the join bites: the per-chunk sampler's paths break the rule over the groups
        em = hmm.EMList(store, model)
        per_chunk = em.sample_paths_minlen(model, min_len, 65, SAMPLE_SEED)
        em.close()
        assert not all(R.admissible_over_groups(row, off, BOUNDARY_JOINED, min_len) for row in per_chunk)


def test_samples_depend_on_their_own_group_alone():
    """Grouped into calls in two ways; with and without the joins of the other groups: the windows of a group keep their samples."""
    store, model, _, _ = _boundary()
    off = np.asarray(store.chunk_off)
    ml = TRACK_LEN
    em = hmm.EMList(store, model)
    whole = em.sample_paths_minlen(model, ml, 64, 5, joined=BOUNDARY_JOINED)
    parts = np.concatenate([em.sample_paths_minlen(model, ml, 24, 5, joined=BOUNDARY_JOINED),
                            em.sample_paths_minlen(model, ml, 40, 5, joined=BOUNDARY_JOINED, first_sample=24)])
    assert np.array_equal(whole, parts)
    assert np.mean(whole != em.sample_paths_minlen(model, ml, 64, 6, joined=BOUNDARY_JOINED)) > 1e-4
    only_first = np.array(BOUNDARY_JOINED)
    only_first[4:] = 0                                       # the first group stays joined, every other chunk is a group of its own
    other = em.sample_paths_minlen(model, ml, 64, 5, joined=only_first)
    assert np.array_equal(other[:, :321], whole[:, :321]) and not np.array_equal(other[:, 321:], whole[:, 321:])
    only_last = np.zeros(len(BOUNDARY_JOINED), int)
    only_last[-2:] = 1
    other = em.sample_paths_minlen(model, ml, 64, 5, joined=only_last)
    assert np.array_equal(other[:, 528:], whole[:, 528:]) and not np.array_equal(other[:, :321], whole[:, :321])
    per_chunk = em.sample_paths_minlen(model, ml, 64, 5)
    assert np.array_equal(other[:, off[4]:off[5]], per_chunk[:, off[4]:off[5]])      # a chunk that is a group of its own
    em.close()


# ---- the sample axis ---------------------------------------------------------------------------------------------------------------

MANY = 577                                                 # pads to 640 words per window: ten wavefront groups, the last of ONE sample
HIGH = 2 ** 40 + 3                                         # an absolute sample index no 32-bit integer holds


@functools.lru_cache(maxsize=None)
def _boundary_sample_refs(min_len, first, n):
    """(the joined sampler's reference, the per-chunk sampler's) for samples first .. first + n - 1 of the boundary store."""
    store, _, _, (A, end) = _boundary()
    off, ks = store.chunk_off, range(first, first + n)
    return (SR.sample(R.sample_tables(A, end, off, tuple(BOUNDARY_JOINED), min_len), SAMPLE_SEED, ks, store.n_windows),
            SR.sample(SR.tables(A, end, off, min_len), SAMPLE_SEED, ks, store.n_windows))


@pytest.mark.parametrize("min_len", LENS)
def test_sample_counts_beyond_one_block_of_k_mlsj_bound(min_len):
    """577 samples in one call, joined and per chunk.  The minimum-length samplers ran at 70 samples at the most so far (128 padded): here
    k_mlsj_bound's loop over the samples (256 threads) makes three trips, the last a ragged one of 65, k_mls_back runs with gridDim.y =
    10 and k_mls_final's loop ten times, and the last wavefront group holds a single sample.  Against the reference over range(577)
    (its smallest margin over the four lengths sets, joined and per chunk, is 1.3e-6 for windows and 1.0e-5 for final lanes, so the
    near-tie rule has nothing to excuse: _quiet_reference asserts 1e-9), every sample admissible over its group (_check_samples);
    bitwise: the two kinds of context, rows [0:65] against a call of 65 in the slab the 577 left, and rows [256:577] against
    first_sample = 256, n = 321 on a second, fresh context."""
    store, model, _, _ = _boundary()
    off = store.chunk_off
    ref_j, ref_c = (_quiet_reference(r) for r in _boundary_sample_refs(min_len, 0, MANY))
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        assert em.minlen_sample_capacity(min_len) >= MANY        # one call each
        res.append((em.sample_paths_minlen(model, min_len, MANY, SAMPLE_SEED, joined=BOUNDARY_JOINED),
                    em.sample_paths_minlen(model, min_len, MANY, SAMPLE_SEED),
                    em.sample_paths_minlen(model, min_len, 65, SAMPLE_SEED, joined=BOUNDARY_JOINED),
                    em.sample_paths_minlen(model, min_len, 65, SAMPLE_SEED)))
        em.close()
        em = hmm.EMList(store, model, algo=algo)
        res[-1] += (em.sample_paths_minlen(model, min_len, MANY - 256, SAMPLE_SEED, first_sample=256, joined=BOUNDARY_JOINED),)
        res[-1] += (em.sample_paths_minlen(model, min_len, MANY - 256, SAMPLE_SEED, first_sample=256),)
        em.close()
    joined, chunk, joined65, chunk65, joined_tail, chunk_tail = res[0]
    assert joined.shape == chunk.shape == (MANY, store.n_windows)
    _check_samples(off, BOUNDARY_JOINED, ref_j, joined, min_len)
    _check_samples(off, None, ref_c, chunk, min_len)
    assert all(np.array_equal(x, y) for x, y in zip(res[0], res[1]))             # the two kinds of context
    assert np.array_equal(joined[:65], joined65) and np.array_equal(chunk[:65], chunk65)
    assert np.array_equal(joined[256:], joined_tail) and np.array_equal(chunk[256:], chunk_tail)
    if min_len != ONES:
        assert not np.array_equal(joined[256:], chunk[256:])                    # the join bites behind the first 256 samples too


def test_absolute_sample_indices_are_64_bit():
    """first_sample = 2^40 + 3, 70 samples of the three samplers on the boundary store against the references over range(2^40 + 3,
    2^40 + 73) (their smallest margins are 5.1e-6 and more; sampling_ref.ffbs reports margin 0 at chunk-first windows by its own
    convention, so hf_sample_paths goes through test_sampling_gpu._check as it stands).  hf_sample_key takes the index as 64 bits:
    truncated to 32 it would be 3, and the rows would be those of first_sample = 3, from which the references differ in 9 % of the
    labels."""
    store, model, _, _ = _boundary()
    off = store.chunk_off
    ml = LENS[0]
    refs = {first: _boundary_sample_refs(ml, first, 70) for first in (HIGH, 3)}
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        res.append({first: (em.sample_paths(model, 70, SAMPLE_SEED, first_sample=first),
                            em.sample_paths_minlen(model, ml, 70, SAMPLE_SEED, first_sample=first),
                            em.sample_paths_minlen(model, ml, 70, SAMPLE_SEED, first_sample=first, joined=BOUNDARY_JOINED)) for first in (HIGH, 3)})
        em.close()
    for first in (HIGH, 3):
        plain, chunk, joined = res[0][first]
        TSG._check(store, model, synth.HIFI_ALPHA, plain, SAMPLE_SEED, first=first)
        _check_samples(off, None, _quiet_reference(refs[first][1]), chunk, ml)
        _check_samples(off, BOUNDARY_JOINED, _quiet_reference(refs[first][0]), joined, ml)
        assert all(np.array_equal(x, y) for x, y in zip(res[0][first], res[1][first]))
    for high, low in zip(res[0][HIGH], res[0][3]):
        assert np.mean(high != low) > 0.01                  # (independent samples differ in about 9 % of the labels)


def test_requests_above_the_capacity_are_split_into_calls(monkeypatch):
    """EMList._drawn, the Python path alone: with the capacity forced to 24, a request for 70 samples arrives as calls of 24, 24 and 22
    with first_sample + k0 passed on and rows k0 .. written; bitwise the one-call result of a context with its own capacity, for the
    three samplers, from first_sample 0 and 5.  (The capacity of these cards is about 60 000 samples: no request in the suite is split
    otherwise.)"""
    store, model, _, _ = _boundary()
    ml = LENS[0]

    def draws(em, first):
        return (em.sample_paths(model, 70, SAMPLE_SEED, first_sample=first),
                em.sample_paths_minlen(model, ml, 70, SAMPLE_SEED, first_sample=first),
                em.sample_paths_minlen(model, ml, 70, SAMPLE_SEED, first_sample=first, joined=BOUNDARY_JOINED))

    em = hmm.EMList(store, model)
    assert em.sample_capacity >= 70 and em.minlen_sample_capacity(ml) >= 70
    want = {first: draws(em, first) for first in (0, 5)}
    em.close()
    assert not np.array_equal(want[0][1], want[5][1]) and np.array_equal(want[0][1][5:], want[5][1][:65])
    em = hmm.EMList(store, model)
    calls = []
    drawn = em._drawn

    def spy(out, cap, finish, get, draw):
        def counted(k0, n):
            calls.append((cap, k0, n))
            return draw(k0, n)
        return drawn(out, cap, finish, get, counted)

    monkeypatch.setattr(hmm.EMList, "sample_capacity", property(lambda self: 24))
    monkeypatch.setattr(em, "minlen_sample_capacity", lambda min_len: 24)
    monkeypatch.setattr(em, "_drawn", spy)
    for first in (0, 5):
        got = draws(em, first)
        for name, x, y in zip(("sample_paths", "sample_paths_minlen", "sample_paths_minlen, joined"), got, want[first]):
            assert x.shape == y.shape and np.array_equal(x, y), (name, first)
    assert calls == [(24, 0, 24), (24, 24, 24), (24, 48, 22)] * 6
    em.close()


# ---- exact cases -----------------------------------------------------------------------------------------------------------------

def _raw_post(em, model, min_len, joined_ptr):
    L = N.lib()
    p = model.params()
    tot = C.c_double(0.0)
    pd = C.POINTER(C.c_double)
    N.check(L.hf_minlen_posterior_joined(em._h, C.byref(p), (C.c_int32 * 4)(*min_len), joined_ptr, em.stream), "hf_minlen_posterior_joined")
    N.check(L.hf_minlen_posterior_finish(em._h, C.byref(tot), em.stream), "hf_minlen_posterior_finish")
    n, c = em.store.n_windows, em.store.n_chunks
    post, lab, mass, lza = np.empty((n, 4)), np.empty(n, np.int8), np.empty(c), np.empty(c)
    N.check(L.hf_get_minlen_posterior(em._h, 0, n, post.ctypes.data_as(pd)), "post")
    N.check(L.hf_get_minlen_posterior_labels(em._h, lab.ctypes.data_as(C.POINTER(C.c_int8))), "labels")
    N.check(L.hf_get_minlen_chunk_log_mass(em._h, mass.ctypes.data_as(pd), lza.ctypes.data_as(pd)), "mass")
    return post, lab, mass, lza, float(tot.value)


def _raw_samples(em, model, min_len, joined_ptr, n, seed):
    L = N.lib()
    p = model.params()
    N.check(L.hf_sample_paths_minlen_joined(em._h, C.byref(p), (C.c_int32 * 4)(*min_len), joined_ptr, 0, n, seed, em.stream),
            "hf_sample_paths_minlen_joined")
    N.check(L.hf_sample_minlen_finish(em._h, em.stream), "hf_sample_minlen_finish")
    out = np.empty((n, em.store.n_windows), np.int8)
    for k in range(n):
        N.check(L.hf_get_minlen_sample_labels(em._h, k, out[k].ctypes.data_as(C.POINTER(C.c_int8))), "labels")
    return out


@pytest.mark.parametrize("algo", ALGOS)
def test_no_join_is_the_per_chunk_entry_point_bit_for_bit(algo):
    for store, model in (TJ._track()[:2], _boundary()[:2]):
        em = hmm.EMList(store, model, algo=algo)
        zero = np.zeros(store.n_chunks, bool)
        for ml in (TRACK_LEN, (16, 16, 16, 16)):
            want = _post(em, model, ml, None)
            assert _same(want, _post(em, model, ml, zero))
            assert _same(want, _raw_post(em, model, ml, None))
            smp = em.sample_paths_minlen(model, ml, 65, 3)
            assert np.array_equal(smp, em.sample_paths_minlen(model, ml, 65, 3, joined=zero))
            assert np.array_equal(smp, _raw_samples(em, model, ml, None, 65, 3))
        em.close()


def test_all_ones_is_the_posterior_of_a_full_pass_whatever_joined_says():
    store, model, _, joined = TJ._track()
    em = hmm.EMList(store, model)
    post, labels, mass, lza, tot = _post(em, model, ONES, joined)
    assert np.all(mass == 0.0) and tot == 0.0 and not np.signbit(mass).any()
    hmm.EM_runOneIterationForList(em, model)
    hmm.HMM_resetEstimators(model)
    want = em.posterior()
    big = want >= 1e-250
    print("all ones: largest relative deviation from hf_get_posterior %.3e" % float(np.max(np.abs(post[big] - want[big]) / want[big])))
    R_ = TMP.R
    R_.close_post(post, want)
    em.close()


def test_group_masses_against_the_per_chunk_masses_and_the_joined_viterbi_path():
    store, model, (logA, logend), (A, end) = _boundary()
    off = store.chunk_off
    em = hmm.EMList(store, model)
    for ml in LENS[:3]:
        pc = _post(em, model, ml, None)
        jn = _post(em, model, ml, BOUNDARY_JOINED)
        bound = JR.group_sums(pc[2], off, BOUNDARY_JOINED)
        assert np.all(jn[2] <= bound + 1e-10 + 1e-9 * np.abs(bound)), (ml, jn[2] - bound)
        zsum = JR.group_sums(pc[3] - pc[2], off, BOUNDARY_JOINED)
        assert np.all(np.abs((jn[3] - jn[2]) - zsum) <= 1e-10 + 1e-9 * np.abs(zsum)), ml
        assert jn[4] < pc[4] - 1e-6                          # the rule over the groups keeps less mass on this store
        vit = em.viterbi_minlen(model, ml, BOUNDARY_JOINED)[0]
        assert np.all(jn[0][np.arange(store.n_windows), vit] > 0.0)
        tab = R.sample_tables(A, end, off, BOUNDARY_JOINED, ml)
        goff, gf, _ = JR.group_offsets(off, BOUNDARY_JOINED)
        for g in range(gf.size):
            assert SR.path_prob(tab, int(gf[g]), [int(v) for v in vit[goff[g]:goff[g + 1]]]) > 0.0, (ml, g)
    em.close()


# ---- a floored stretch across a joined boundary --------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_len", [(3, 5, 1, 7), ONES, (16, 16, 16, 16)])
def test_a_floored_stretch_across_a_joined_boundary(min_len):
    """floor_cases.long(): windows 1940..1959 at the 1e-40 emission floor, ten on either side of the boundary between chunks 2 and 3,
    which the fixture joins: a whole rescaling period of both walks on both sides of J_t.  Same tolerances, no NaN, no HF_E_SCALE."""
    store, model, alpha = FC.long()
    joined = FC.joins("long")
    off = np.asarray(store.chunk_off)
    assert joined[3] and all(store.cov[t] == FC.COV for t in range(int(off[3]) - 10, int(off[3]) + 10))
    ref = R.posterior(store, model, alpha, joined, min_len)
    assert np.all(np.isfinite(ref[2])) and ref[2][2] < -1000
    ref_s = _quiet_reference(R.sample(store, model, alpha, joined, min_len, 41, range(8)))
    res = []
    for algo in ALGOS:
        em = hmm.EMList(store, model, algo=algo)
        res.append((_post(em, model, min_len, joined), em.sample_paths_minlen(model, min_len, 8, 41, joined=joined)))
        em.close()
    _check_post(store, joined, ref, res[0][0], "floored boundary %s" % (min_len,))
    assert np.all(np.abs(res[0][0][0].sum(axis=1) - 1.0) <= 4 * np.finfo(float).eps)
    _check_samples(off, joined, ref_s, res[0][1], min_len)
    assert _same(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ---- geometry --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunks_and_uncovered_windows(algo):
    model_type, seed = G.CASES[0]
    store, model, alpha, _ = G.case(model_type, seed)
    logA, logend = viterbi_ref.tables(store, model, alpha)
    A, end = S.rows(store, model, alpha)
    off = np.asarray(G.OFF)
    ml = TRACK_LEN
    em0 = hmm.EMList(store, model, algo=algo)
    base = _post(em0, model, ml, G.joins())
    base_s = em0.sample_paths_minlen(model, ml, 8, 3, joined=G.joins())
    em0.close()
    _check_post(store, G.joins(), R.posterior_tables(logA, logend, off, G.joins(), ml), base, "grid store")
    _check_samples(off, G.joins(), SR.sample(R.sample_tables(A, end, off, G.joins(), ml), 3, range(8)), base_s, ml)
    # a chunk without windows between joined chunks ends the group, whatever its own and its successor's entries say
    est, src = G.with_empty_chunks(store)
    dev_j, ref_j = G.empty_chunk_joins(src, G.joins())
    em = hmm.EMList(est, model, algo=algo)
    post, labels, mass, lza, tot = _post(em, model, ml, dev_j)
    smp = em.sample_paths_minlen(model, ml, 8, 3, joined=dev_j)
    em.close()
    assert np.all(mass[src < 0] == 0.0) and np.all(lza[src < 0] == 0.0)
    _check_post(store, ref_j, R.posterior_tables(logA, logend, off, ref_j, ml), (post, labels, mass[src >= 0], lza[src >= 0], tot), "empty chunks")
    end_e = np.zeros((est.n_chunks, 4))
    end_e[src >= 0] = end
    _check_samples(est.chunk_off, dev_j, SR.sample(R.sample_tables(A, end_e, est.chunk_off, dev_j, ml), 3, range(8)), smp, ml)
    # windows outside every chunk: label -1, a posterior range that touches one is refused, the rest is the grid store's
    ust = G.with_uncovered_windows(store, np.random.default_rng(5))
    a, n = G.FRONT, ust.n_windows
    b = a + store.n_windows
    em = hmm.EMList(ust, model, algo=algo)
    r = hmm.EM_runMinLengthPosteriorForList(em, model, ml, G.joins())
    outside = np.r_[0:a, b:n]
    assert np.all(r.labels[outside] == -1) and np.array_equal(r.labels[a:b], base[1])
    assert np.array_equal(r.chunk_log_mass, base[2]) and np.array_equal(r.chunk_log_z_adm, base[3]) and r.log_mass == base[4]
    assert np.array_equal(r.posterior(a, store.n_windows), base[0])
    for f, cnt in [(0, 1), (a - 1, 4), (0, n), (b, 1)]:
        with pytest.raises(N.HFError) as ei:
            r.posterior(f, cnt)
        assert ei.value.code == N.HF_E_ARG, (f, cnt)
    got = em.sample_paths_minlen(model, ml, 8, 3, joined=G.joins())
    assert got.shape == (8, n) and np.all(got[:, outside] == -1)
    for row in got:
        assert R.admissible_over_groups(row[a:b], off, G.joins(), ml)
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_chunk_list(algo):
    full = synth.synthesize([50_000], 1000, 20_000, [20], seed=2)
    store = full.subset_chunks([])
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, full, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model, algo=algo)
    r = hmm.EM_runMinLengthPosteriorForList(em, model, TRACK_LEN, np.zeros(0, bool))
    assert r.labels.size == 0 and r.chunk_log_mass.size == 0 and r.log_mass == 0.0 and r.posterior().shape == (0, 4)
    assert _raw_post(em, model, TRACK_LEN, None)[4] == 0.0
    assert em.sample_paths_minlen(model, TRACK_LEN, 5, 1, joined=np.zeros(0, bool)).shape == (5, 0)
    em.close()


# ---- the realistic track ---------------------------------------------------------------------------------------------------------

def test_realistic_track():
    """configs[2] at scale 0.02 with the chunk length scaled: 286 chunks in 46 contigs, 30 568 windows (test_minlen_joined_gpu._track)."""
    store, model, (logA, logend), joined = TJ._track()
    off = store.chunk_off
    ref = R.posterior_tables(logA, logend, off, joined, TRACK_LEN)
    ref_s = _quiet_reference(R.sample(store, model, synth.HIFI_ALPHA, joined, TRACK_LEN, 2024, range(8)))
    em = hmm.EMList(store, model)
    got = _post(em, model, TRACK_LEN, joined)
    _check_post(store, joined, ref, got, "track")
    pc = _post(em, model, TRACK_LEN, None)
    bound = JR.group_sums(pc[2], off, joined)
    assert np.all(got[2] <= bound + 1e-10 + 1e-9 * np.abs(bound)) and got[4] < pc[4]
    smp = em.sample_paths_minlen(model, TRACK_LEN, 8, 2024, joined=joined)
    _check_samples(off, joined, ref_s, smp, TRACK_LEN)
    for row in smp:
        assert np.all(got[0][np.arange(store.n_windows), row] > 0.0)     # no sample visits a state the joined posterior excludes
    goff = JR.group_offsets(off, joined)[0]
    per_chunk = em.sample_paths_minlen(model, TRACK_LEN, 8, 2024)
    short = sum(len(JR.short_inner_runs(row, goff, TRACK_LEN)) for row in per_chunk)
    print("track: log_mass %.6f over the contigs, %.6f per chunk; the per-chunk sampler leaves %d short runs in 8 samples" % (got[4], pc[4], short))
    assert short >= 1
    em.close()


# ---- shared state, no disturbance, streams ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ALGOS)
def test_shared_decoder_state_in_mixed_call_orders(algo):
    """On one context, bitwise against a twin context that made only the later call: a per-chunk call then a joined call and the
    reverse (no entry of the earlier run survives in a group's other chunks), and narrower lengths after wider ones in the grown
    forward-lane buffer."""
    store, model, _, _ = _boundary()
    wide, narrow = (16, 16, 16, 16), (3, 5, 1, 7)

    def alone(f):
        em = hmm.EMList(store, model, algo=algo)
        out = f(em)
        em.close()
        return out

    calls = {
        "post chunk wide": lambda em: _post(em, model, wide, None),
        "post joined narrow": lambda em: _post(em, model, narrow, BOUNDARY_JOINED),
        "post joined wide": lambda em: _post(em, model, wide, BOUNDARY_JOINED),
        "post chunk narrow": lambda em: _post(em, model, narrow, None),
    }
    want = {k: alone(f) for k, f in calls.items()}
    em = hmm.EMList(store, model, algo=algo)
    for k in ("post chunk wide", "post joined narrow", "post chunk narrow", "post joined wide", "post chunk wide", "post joined wide", "post joined narrow"):
        assert _same(want[k], calls[k](em)), k
    em.close()
    scalls = {
        "chunk wide": lambda em: em.sample_paths_minlen(model, wide, 70, 2),
        "joined narrow": lambda em: em.sample_paths_minlen(model, narrow, 5, 2, joined=BOUNDARY_JOINED),
        "joined wide": lambda em: em.sample_paths_minlen(model, wide, 70, 2, joined=BOUNDARY_JOINED),
        "chunk narrow": lambda em: em.sample_paths_minlen(model, narrow, 5, 2),
    }
    swant = {k: alone(f) for k, f in scalls.items()}
    em = hmm.EMList(store, model, algo=algo)
    for k in ("chunk wide", "joined narrow", "chunk narrow", "joined wide", "chunk wide", "joined wide", "joined narrow"):
        assert np.array_equal(swant[k], scalls[k](em)), k
    em.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_no_disturbance_of_the_last_pass_and_the_other_decoders(algo):
    store = synth.synthesize(synth.human_diploid_lengths(0.005), 4000, 100_000, [20], 1236, contig_prefix="hap_ctg")
    joined = hmm.joined_chunks(store)
    assert joined.sum() >= 40
    model = hmm.createModel(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, store, synth.HIFI_ALPHA)
    em_a = hmm.EMList(store, model, algo=algo)
    em_b = hmm.EMList(store, model, algo=algo)
    for em in (em_a, em_b):
        hmm.EM_runOneIterationForList(em, model)
    hmm.HMM_estimateParameters(model, 1e-3)
    hmm.HMM_resetEstimators(model)
    hmm.EM_runOneIterationForList(em_a, model); st_a = model.estimators.copy(); hmm.HMM_resetEstimators(model)
    hmm.EM_runOneIterationForList(em_b, model); st_b = model.estimators.copy(); hmm.HMM_resetEstimators(model)
    assert np.array_equal(st_a, st_b)
    vit = em_a.viterbi(model)
    mlv = em_a.viterbi_minlen(model, TRACK_LEN, joined)
    smp = em_a.sample_paths(model, 2, 7)
    other = model.copy()                                   # the feature runs with DIFFERENT parameters
    v = other.param_vector().reshape(other.numberOfRegions, -1)
    v[:, 27:27 + 4 * 16] *= 1.1
    other.set_param_vector(v.ravel())
    r1 = _post(em_a, other, TRACK_LEN, joined)
    assert not np.array_equal(r1[0], em_a.posterior())
    mine = em_a.sample_paths_minlen(other, TRACK_LEN, 3, 2, joined=joined)
    assert np.array_equal(em_a.labels(), em_b.labels())
    assert np.array_equal(em_a.posterior(), em_b.posterior())
    for x, y in zip(em_a.forward_backward(), em_b.forward_backward()):
        assert np.array_equal(x, y)
    lab, ll = TML._viterbi_results(em_a)
    assert np.array_equal(lab, vit[0]) and np.array_equal(ll, vit[1])
    L = N.lib()
    mlab = np.empty(store.n_windows, np.int8)
    mll = np.empty(store.n_chunks)
    assert L.hf_get_viterbi_minlen_labels(em_a._h, mlab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
    assert L.hf_get_viterbi_minlen_chunk_log_probs(em_a._h, mll.ctypes.data_as(C.POINTER(C.c_double))) == N.HF_OK
    assert np.array_equal(mlab, mlv[0]) and np.array_equal(mll, mlv[1])
    assert np.array_equal(TML._sample_results(em_a, 2), smp)
    # the two decoders of the feature leave each other alone as well
    post = np.empty((store.n_windows, 4))
    assert L.hf_get_minlen_posterior(em_a._h, 0, store.n_windows, post.ctypes.data_as(C.POINTER(C.c_double))) == N.HF_OK
    assert np.array_equal(post, r1[0])
    _post(em_a, model, (2, 2, 2, 2), joined)
    for k in range(3):
        assert L.hf_get_minlen_sample_labels(em_a._h, k, mlab.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
        assert np.array_equal(mlab, mine[k])
    hmm.EM_runOneIterationForList(em_a, model); st2_a = model.estimators.copy(); hmm.HMM_resetEstimators(model)   # the next pass
    hmm.EM_runOneIterationForList(em_b, model); st2_b = model.estimators.copy()
    assert np.array_equal(st2_a, st2_b)
    assert np.array_equal(em_a.labels(), em_b.labels())
    em_a.close(); em_b.close()


def test_callers_stream():
    store, model, _, _ = _boundary()
    em0 = hmm.EMList(store, model)
    want = _post(em0, model, TRACK_LEN, BOUNDARY_JOINED)
    want_s = em0.sample_paths_minlen(model, TRACK_LEN, 65, 5, joined=BOUNDARY_JOINED)
    em0.close()
    with Streams() as streams:
        s = streams.new(non_blocking=True)
        em = hmm.EMList(store, model, stream=s)
        streams.h.delay(s)                                 # whatever ran on the null stream instead would run ahead of this
        assert _same(want, _post(em, model, TRACK_LEN, BOUNDARY_JOINED))
        streams.h.delay(s)
        assert np.array_equal(want_s, em.sample_paths_minlen(model, TRACK_LEN, 65, 5, joined=BOUNDARY_JOINED))
        em.close()


# ---- arguments and errors --------------------------------------------------------------------------------------------------------

def test_arguments_and_errors():
    store, model, _, _ = _boundary()
    joined = np.array(BOUNDARY_JOINED, bool)
    em = hmm.EMList(store, model)
    L = N.lib()
    p = model.params()
    four = (C.c_int32 * 4)(*TRACK_LEN)
    jn = np.ascontiguousarray(joined, np.uint8)
    jp = jn.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.hf_minlen_posterior_joined(None, C.byref(p), four, jp, None) == N.HF_E_ARG
    assert L.hf_minlen_posterior_joined(em._h, None, four, jp, None) == N.HF_E_ARG
    assert L.hf_minlen_posterior_joined(em._h, C.byref(p), None, jp, None) == N.HF_E_ARG
    assert L.hf_sample_paths_minlen_joined(None, C.byref(p), four, jp, 0, 1, 1, None) == N.HF_E_ARG
    assert L.hf_sample_paths_minlen_joined(em._h, None, four, jp, 0, 1, 1, None) == N.HF_E_ARG
    assert L.hf_sample_paths_minlen_joined(em._h, C.byref(p), None, jp, 0, 1, 1, None) == N.HF_E_ARG
    bad0 = jn.copy()
    bad0[0] = 1
    bp = bad0.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.hf_minlen_posterior_joined(em._h, C.byref(p), four, bp, None) == N.HF_E_ARG and b"joined[0]" in L.hf_last_error()
    assert L.hf_sample_paths_minlen_joined(em._h, C.byref(p), four, bp, 0, 1, 1, None) == N.HF_E_ARG and b"joined[0]" in L.hf_last_error()
    assert L.hf_minlen_posterior_finish(em._h, None, None) == N.HF_E_ARG                  # a refused call is no run to finish
    assert L.hf_sample_minlen_finish(em._h, None) == N.HF_E_ARG
    for bad_len in ((3, 0, 1, 1), (62, 1, 1, 1)):          # a length 0, a sum of 65
        with pytest.raises(N.HFError) as ei:
            em.minlen_posterior(model, bad_len, joined)
        assert ei.value.code == N.HF_E_ARG, bad_len
        with pytest.raises(N.HFError) as ei:
            em.sample_paths_minlen(model, bad_len, 2, 1, joined=joined)
        assert ei.value.code == N.HF_E_ARG, bad_len
    for wrong in (joined[:-1], np.concatenate([joined, [False]])):
        with pytest.raises(ValueError):
            em.minlen_posterior(model, TRACK_LEN, wrong)
        with pytest.raises(ValueError):
            em.sample_paths_minlen(model, TRACK_LEN, 2, 1, joined=wrong)
        with pytest.raises(ValueError):
            hmm.EM_runMinLengthPosteriorForList(em, model, TRACK_LEN, wrong)
        with pytest.raises(ValueError):
            hmm.EM_sampleMinLengthPathsForList(em, model, TRACK_LEN, 2, 1, wrong)
    cap = em.minlen_sample_capacity(TRACK_LEN)               # the capacity holds for both entry points
    assert L.hf_sample_paths_minlen_joined(em._h, C.byref(p), four, jp, 0, cap + 1, 1, None) == N.HF_E_ARG
    assert L.hf_sample_paths_minlen_joined(em._h, C.byref(p), four, jp, 0, 0, 1, None) == N.HF_E_ARG
    assert L.hf_sample_paths_minlen_joined(em._h, C.byref(p), four, jp, -1, 2, 1, None) == N.HF_E_ARG
    good = _post(em, model, (61, 1, 1, 1), joined)          # a sum of exactly 64 is served
    bad = model.copy()
    v = bad.param_vector().reshape(model.numberOfRegions, -1)
    v[:, 20:24] = 0.0                                      # start row: no path of any group has weight
    bad.set_param_vector(v.ravel())
    with pytest.raises(N.HFError) as ei:
        em.minlen_posterior(bad, TRACK_LEN, joined)
    assert ei.value.code == N.HF_E_SCALE
    with pytest.raises(N.HFError) as ei:
        em.sample_paths_minlen(bad, TRACK_LEN, 2, 1, joined=joined)
    assert ei.value.code == N.HF_E_SCALE
    assert _same(good, _post(em, model, (61, 1, 1, 1), joined))
    em.close()


def test_nan_in_an_end_column_that_only_a_joined_boundary_reads():
    """test_minlen_joined_gpu's construction: region 1 holds one window, the last of chunk 0, which chunk 1 continues; its end column
    is read at the boundary alone."""
    rng = np.random.default_rng(23)
    two = _tiny_store(rng, [6, 5], [20, 31])
    reg = np.zeros(two.n_windows, np.uint64)
    reg[5] = 1
    two.annot = (two.annot & np.uint64((1 << 58) - 1)) | (reg << np.uint64(58))
    model = perturbed_model(two, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 3, synth.HIFI_ALPHA, rng)
    nan = model.copy()
    v = nan.param_vector().reshape(2, -1)
    v[1, 14] = np.nan                                      # trans[region 1][Hap][End]
    nan.set_param_vector(v.ravel())
    ml = (2, 2, 1, 2)
    em = hmm.EMList(two, model)
    good = _post(em, model, ml, [0, 1])
    assert np.isfinite(good[4])
    with pytest.raises(N.HFError) as ei:
        em.minlen_posterior(nan, ml, [0, 1])
    assert ei.value.code == N.HF_E_NAN
    with pytest.raises(N.HFError) as ei:
        em.sample_paths_minlen(nan, ml, 2, 1, joined=[0, 1])
    assert ei.value.code == N.HF_E_NAN
    assert _same(good, _post(em, model, ml, [0, 1]))       # and the context answers afterwards
    assert em.sample_paths_minlen(model, ml, 2, 1, joined=[0, 1]).shape == (2, 11)
    em.close()


# ---- command line ----------------------------------------------------------------------------------------------------------------

def test_cli_merged_chunks(tmp_path):
    """Fixed-parameter run (-n 0) of two contigs in 40 chunks of 20 windows (80 kb chunks, 4 kb windows), as test_minlen_joined_gpu's."""
    store = synth.synthesize([2_000_000, 1_200_000], 4000, 80_000, [20], 1235)
    binp = tmp_path / "in.bin"
    store.write_bin(str(binp))
    K = hmm.getBestNumberOfCollapsedComps(store)
    args = (["-i", str(binp), "-W", "4000", "-n", "0", "-P", "-p", str(K), "--uncertaintySeed", "7", "--constrainedPosterior",
             "--admissibleSamples", "8"] + TML.MINLEN_ARGS)
    TML._cli(args, tmp_path / "chunk")
    r = TML._cli(args + ["--mergedChunks"], tmp_path / "merged")
    a, b = tmp_path / "chunk", tmp_path / "merged"
    st = synth.WindowStore.read_bin(str(binp))
    assert st.n_chunks == 40
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, np.zeros((4, 4)))
    w = (2, 3, 1, 2)
    joined = hmm.joined_chunks(st)
    assert JR.group_offsets(st.chunk_off, joined)[0].tolist() == [0, 500, 800]
    em = hmm.EMList(st, model)
    pc = em.minlen_posterior(model, w)
    jn = em.minlen_posterior(model, w, joined)
    jpost = jn.posterior()
    lab = em.sample_paths_minlen(model, w, 8, 7, joined=joined)
    lab_pc = em.sample_paths_minlen(model, w, 8, 7)
    em.close()
    assert jn.log_mass < pc.log_mass - 1e-6
    # admissible_mass.tsv: the joined masses and, in the new column, the per-chunk rule's
    rows = (b / "admissible_mass.tsv").read_text().splitlines()
    assert [int(x) for x in rows[1].split("\t")] == list(w)
    assert rows[2] == "#scope\tchunks\twindows\tlog_mass\tlog_mass_per_chunk_rule"
    want = {"all": (jn.log_mass, pc.log_mass)}
    for c in range(st.n_chunks):
        x = want.get(st.chunk_ctg[c], (0.0, 0.0))
        want[st.chunk_ctg[c]] = (x[0] + jn.chunk_log_mass[c], x[1] + pc.chunk_log_mass[c])
    assert len(rows) == 3 + len(want)
    for line in rows[3:]:
        g = line.split("\t")
        assert len(g) == 5
        for got, ref in zip(g[3:], want[g[0]]):
            assert abs(float(got) - ref) <= 1e-9 * (1 + abs(ref)), g
    assert "over merged chunks keep posterior mass" in r.stderr and "per chunk: exp(" in r.stderr
    # posterior_prediction_min_lengths.bed: written from the joined posterior
    L = N.lib()
    tab = L.hfio_load(str(binp).encode(), 0, 0)
    assert tab
    ref_bed = tmp_path / "ref.bed"
    assert L.hfio_write_posterior_bed(tab, np.ascontiguousarray(jpost).ctypes.data_as(C.POINTER(C.c_double)),
                                      np.ascontiguousarray(jn.labels).ctypes.data_as(C.POINTER(C.c_int8)), str(ref_bed).encode()) == 0
    L.hfio_destroy(tab)
    assert (b / "posterior_prediction_min_lengths.bed").read_bytes() == ref_bed.read_bytes()
    assert (a / "posterior_prediction_min_lengths.bed").read_bytes() != ref_bed.read_bytes()
    # admissible_label_runs_support.bed: the support column counted over the joined sampler's paths
    off = np.asarray(st.chunk_off, np.int64)
    chunk = np.searchsorted(off, np.arange(st.n_windows), side="right") - 1
    ws = st.chunk_s[chunk].astype(np.int64) + (np.arange(st.n_windows) - off[chunk]) * st.window_len
    we = np.minimum(ws + st.window_len - 1, st.chunk_e[chunk])
    ctg = np.array([st.chunk_ctg[c] for c in chunk])
    names4 = ["Err", "Dup", "Hap", "Col"]
    runs = [l.split("\t") for l in (b / "admissible_label_runs_support.bed").read_text().splitlines() if not l.startswith("#")]
    differ = 0
    for run in runs:
        sel = (ctg == run[0]) & (ws >= int(run[1])) & (we + 1 <= int(run[2]))
        hit = lab[:, sel] == names4.index(run[3])
        assert run[4] == "%.4f" % (hit.all(axis=1).sum() / 8) and run[5] == "%.4f" % (hit.mean(axis=1).sum() / 8), run
        differ += run[4] != "%.4f" % ((lab_pc[:, sel] == names4.index(run[3])).all(axis=1).sum() / 8)
    assert differ >= 1                                       # the per-chunk sampler's paths would have given other supports
    # without the flag the files are the per-chunk entry points' (four columns), and the flag changes nothing but the three files
    rows_a = (a / "admissible_mass.tsv").read_text().splitlines()
    assert rows_a[2] == "#scope\tchunks\twindows\tlog_mass" and all(len(l.split("\t")) == 4 for l in rows_a[3:])
    assert abs(float(rows_a[3].split("\t")[3]) - pc.log_mass) <= 1e-9 * (1 + abs(pc.log_mass))
    names = sorted(os.listdir(a))
    assert sorted(os.listdir(b)) == names
    changed = {"admissible_mass.tsv", "posterior_prediction_min_lengths.bed", "admissible_label_runs_support.bed", "admissible_samples_summary.tsv"}
    for n in names:
        if n not in changed:
            assert (a / n).read_bytes() == (b / n).read_bytes(), n
