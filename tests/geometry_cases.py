"""The grid store of tests/test_geometry_cpu.py and tests/test_geometry_gpu.py: a track whose chunk list is laid against the range
getters' global piece grid (pieces of 512 windows cut at global multiples of 512, lanes of 8 windows), its jobs, its references and
the variants of it with chunks that hold no window and with windows that lie in no chunk.

Chunks (one contig each), first window .. last window:
    0..0, 511..511, 512..512, 513..513   one window, at the track's start, one before, on and one after a grid point
    1..2, 1023..1024                     two windows; the second pair lies across a grid point
    3..503                               ends on a lane boundary (504)
    504..510, 514..1022                  between the one-window chunks
    1025..1535                           ends on the grid
    1536..2047                           exactly one aligned piece
    2048..3072                           starts on the grid: a first window, two pieces less that window, one window over
    3073..4172                           long and unaligned
Jobs: every pair first <= last over the boundary points (POINTS: every chunk's first and last window +- 1, every multiple of 512 +- 1,
and 7, 8, 9, 503, 504, 505), a random mask 1..15 and a random region filter each.  The breakpoint jobs (every pair first < last of the
boundary points inside one chunk), the long-run jobs (the short ranges of the 903 and twenty long ones) and the length sets of the
minimum-length decoder are here too, each with its reference, once for the getters' own device tests and the geometry tests."""
import dataclasses
import functools

import numpy as np

from flagger_amd import synth
from test_bruteforce_cpu import _tiny_store
from test_longrun_cpu import max_len
from test_moments_cpu import TINY
from test_viterbi_cpu import perturbed_model
import breakpoint_ref as BR
import entropy_ref as ER
import interval_ref as IR
import longrun_ref as LR
import minlen_ref
import moments_ref as MR
import posterior_ref as PR
import runs_ref as RR
import sampling_ref as S
import viterbi_ref

OFF = [0, 1, 3, 504, 511, 512, 513, 514, 1023, 1025, 1536, 2048, 3073, 4173]
N_WINDOWS = OFF[-1]
JOINED = (4, 5, 6, 7, 9)            # chunks that continue their predecessor (hf_get_run_moments): 504..1022 and 1023..1535 are one contig each
PIECE, LANE = 512, 8
CASES = TINY                         # trunc-exp-Gaussian / HiFi alpha / two regions; Gaussian / alpha 0 / one region; negative binomial
SAMPLES, SAMPLE_SEED = 8, 41
# the generator of a case's store and model: chosen so that every boundary point matters to every getter (tests/test_geometry_cpu.py)
STORE_SEED = {0: 9100, 1: 9101, 2: 9102}
# coverage set by hand at the few windows whose posterior the draw left certain (window: coverage, mapq the same, no clipping)
COV_AT = {0: {0: 30, 2560: 30, 4095: 46, 4096: 6, 4172: 18}, 1: {9: 30, 3073: 26, 3583: 30, 3584: 34}, 2: {}}


def _points():
    B = set()
    for o in OFF:
        B.update([o - 1, o, o + 1])
    for g in range(PIECE, N_WINDOWS, PIECE):
        B.update([g - 1, g, g + 1])
    B.update([503, 504, 505, 7, 8, 9])
    return np.array(sorted(b for b in B if 0 <= b < N_WINDOWS), np.int64)


POINTS = _points()


def joins():
    j = np.zeros(len(OFF) - 1, bool)
    j[list(JOINED)] = True
    return j


@functools.lru_cache(maxsize=None)
def case(model_type, seed):
    """(store, model, alpha, (F, L, M, R)) of a case, once for every test that uses it; nothing of it is changed later (a pass with
    the model writes its estimators only)."""
    rng = np.random.default_rng(STORE_SEED[seed])
    alpha = synth.HIFI_ALPHA if seed % 2 == 0 else np.zeros((4, 4))
    regions = [20, 31] if seed % 2 == 0 else [25]
    store = _tiny_store(rng, list(np.diff(OFF)), regions)
    assert list(store.chunk_off) == OFF
    for t, v in COV_AT[seed].items():
        store.cov[t] = store.mapq[t] = v
        store.clip[t] = 0
    if len(regions) > 1:                                    # a region change exactly on the grid points 512 and 1024
        reg = store.regions().astype(np.uint64)
        reg[[511, 1023]], reg[[512, 1024]] = 0, 1
        store.annot = (store.annot & np.uint64((1 << 58) - 1)) | (reg << np.uint64(58))
    ctg = list(store.chunk_ctg)
    for c in JOINED:                                        # a joined chunk lies on its predecessor's contig
        ctg[c] = ctg[c - 1]
    store.chunk_ctg = ctg
    model = perturbed_model(store, model_type, 2 + seed % 3, alpha, rng)
    F, L = np.meshgrid(POINTS, POINTS, indexing="ij")
    keep = F <= L
    F, L = F[keep], L[keep]
    M = np.random.default_rng(9202 + seed).integers(1, 16, F.size)     # (a generator of its own: the full mask in at least 50 jobs)
    R = np.random.default_rng(9150 + seed).integers(-1, len(regions), F.size)
    for a in (F, L, M, R):
        a.setflags(write=False)
    return store, model, alpha, (F, L, M, R)


@functools.lru_cache(maxsize=None)
def rows(model_type, seed):
    store, model, alpha, _ = case(model_type, seed)
    return S.rows(store, model, alpha)


def pieces_of(off, first, last):
    """(parts, pieces) of every job as the getters cut it: a part per chunk the job touches, and per part the 512-blocks of the global
    grid that intersect its interior windows (a, b]."""
    off = np.asarray(off, np.int64)
    first, last = np.asarray(first, np.int64), np.asarray(last, np.int64)
    parts, pieces = np.zeros(first.size, np.int64), np.zeros(first.size, np.int64)
    for c in range(off.size - 1):
        if off[c + 1] <= off[c]:
            continue
        a, b = np.maximum(first, off[c]), np.minimum(last, off[c + 1] - 1)
        hit = a <= b
        parts += hit
        pieces += np.where(hit & (b > a), b // PIECE - (a + 1) // PIECE + 1, 0)
    return parts, pieces


def _batches(parts, pieces, cap_pieces, cap_parts):
    """The first job of every device batch of a call, by the getters' rule: a job is added while the batch holds fewer than cap_pieces
    pieces and fewer than cap_parts parts; a batch holds at least one job; a job is never split."""
    cp, cq = np.concatenate([[0], np.cumsum(pieces)]), np.concatenate([[0], np.cumsum(parts)])
    starts, j0, n = [], 0, parts.size
    while j0 < n:
        starts.append(j0)
        j1 = min(n, int(np.searchsorted(cp, cp[j0] + cap_pieces, "left")), int(np.searchsorted(cq, cq[j0] + cap_parts, "left")))
        j0 = max(j1, j0 + 1)          # (the job that reaches the cap is the batch's last)
    return starts


# ---- the references, each once per case ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def interval_reference(model_type, seed):
    _, _, _, (F, L, M, _) = case(model_type, seed)
    A, end = rows(model_type, seed)
    return IR.log_probs(A, end, OFF, F, L, M)


@functools.lru_cache(maxsize=None)
def long_double(model_type, seed):
    A, end = rows(model_type, seed)
    return ER.LongDouble(A, end, np.asarray(OFF, np.int64))


@functools.lru_cache(maxsize=None)
def entropy_reference(model_type, seed):
    _, _, _, (F, L, _, _) = case(model_type, seed)
    return long_double(model_type, seed).entropy(F, L)


@functools.lru_cache(maxsize=None)
def labellings(model_type, seed):
    A, end = rows(model_type, seed)
    return ER.labellings(A, end, np.asarray(OFF, np.int64), 70 + seed)


@functools.lru_cache(maxsize=None)
def log_prob_reference(model_type, seed):
    """[(name, labels, log-probability of every job)]"""
    _, _, _, (F, L, _, _) = case(model_type, seed)
    ld = long_double(model_type, seed)
    return [(name, y, ld.log_probs(F, L, y)) for name, y in labellings(model_type, seed)]


@functools.lru_cache(maxsize=None)
def count_reference(model_type, seed, unit):
    store, _, _, (F, L, M, R) = case(model_type, seed)
    A, end = rows(model_type, seed)
    return MR.moments_long(A, end, OFF, MR.weights(store, unit), store.regions().astype(np.int64), F, L, M, R)


def joins_key(j):
    return None if j is None else tuple(bool(x) for x in j)


@functools.lru_cache(maxsize=None)
def run_reference(model_type, seed, joined_key):
    """(mean, var, scale) with the joins of joined_key (a tuple, or None)."""
    _, _, _, (F, L, M, _) = case(model_type, seed)
    A, end = rows(model_type, seed)
    return RR.jet_long(A, end, OFF, F, L, M, None if joined_key is None else np.array(joined_key, bool))


@functools.lru_cache(maxsize=None)
def pass_reference(model_type, seed):
    """(posterior [N][4], chunk log-likelihoods [C], marg [N], cond [N])"""
    store, model, _, _ = case(model_type, seed)
    A, end = rows(model_type, seed)
    post, _, ll = PR.forward_backward(A, end, OFF, PR.regions_of(store), model.numberOfRegions)
    marg, cond = ER.profile(A, end, OFF)
    return post, ll, marg, cond


@functools.lru_cache(maxsize=None)
def viterbi_reference(model_type, seed):
    store, model, alpha, _ = case(model_type, seed)
    return viterbi_ref.reference(store, model, alpha)


@functools.lru_cache(maxsize=None)
def sample_reference(model_type, seed):
    A, end = rows(model_type, seed)
    return S.ffbs(A, end, OFF, SAMPLE_SEED + seed, range(SAMPLES))


# the length sets of hf_viterbi_minlen: the realistic one; one longer than the one-, two- and seven-window chunks, whose runs are all
# exempt; one state owning 61 of the 64 lanes
MINLEN_SETS = ((3, 5, 1, 7), (16, 16, 16, 16), (61, 1, 1, 1))


@functools.lru_cache(maxsize=None)
def minlen_reference(model_type, seed, min_len):
    """(labels, chunk scores, path_log_prob, unconstrained labels): minlen_ref.reference on the grid store; min_len a tuple."""
    store, model, alpha, _ = case(model_type, seed)
    return minlen_ref.reference(store, model, alpha, min_len)


# the generators of the breakpoint jobs' masks, chosen on the CPU so that the REFERENCE meets test_breakpoint_gpu._not_empty with room:
# of the finite jobs with at least 8 candidate windows, 17 of 48, 17 of 43 and 24 of 48 have mode_p < 0.99, none within 1e-3 of that bound
BREAKPOINT_MASK_SEED = {0: 38, 1: 26, 2: 0}


@functools.lru_cache(maxsize=None)
def breakpoint_reference(model_type, seed):
    """((F, L, U, V), log P(E_k) per job): every pair a < b of the boundary points inside one chunk, a random left mask and its
    complement, route (ii) of tests/breakpoint_ref.py."""
    A, end = rows(model_type, seed)
    P = POINTS
    chunk = np.searchsorted(np.asarray(OFF), P, "right") - 1
    F, L = np.meshgrid(P, P, indexing="ij")
    keep = (F < L) & (chunk[:, None] == chunk[None, :])
    F, L = F[keep], L[keep]
    U = np.random.default_rng(BREAKPOINT_MASK_SEED[seed]).integers(1, 15, F.size).astype(np.int64)
    V = 15 & ~U                                             # (the complement: of the disjoint pairs the ones whose posterior spreads most)
    events = BR.LongDouble(A, end, OFF).events(F, L, U, V)
    _, pieces = pieces_of(OFF, F, L)
    assert pieces.max() == 3 and np.sum(L - F == 1) >= 10 and F.size >= 80
    for a in (F, L, U, V):
        a.setflags(write=False)
    return (F, L, U, V), events


@functools.lru_cache(maxsize=None)
def longrun_jobs(model_type, seed):
    """(F, L, M, K): every range of the case of at most 48 windows (half of them span chunks) and 20 long ones, the case's masks, a
    length out of 1, 2, 3, 7, 16, 58 cut to what 64 lanes hold; then the short ranges again with short lengths."""
    _, _, _, (F, L, M, _) = case(model_type, seed)
    n_ = L - F + 1
    pick = np.concatenate([np.flatnonzero(n_ <= 48), np.random.default_rng(7).choice(np.flatnonzero(n_ > 64), 20, replace=False)])
    F, L, M = F[pick], L[pick], M[pick]
    M = np.where(L - F + 1 > 64, (M & ~4) | ((M & ~4) == 0), M)            # (long ranges: the other labels, tests/test_longrun_cpu.py jobs)
    K = np.minimum(np.random.default_rng(8).choice([1, 2, 3, 7, 16, 58], F.size), [max_len(m) for m in M])
    # in half of those the length is above the range's or the mask is full: exactly 0 and -inf.  The short ranges once more with a
    # length of at most half the range's out of 1, 2, 3, 7, for a mask that is not full and for its complement, so that more than half of all jobs walk the chain to a
    # value that is neither (tests/test_geometry_cpu.py)
    short = np.flatnonzero(L - F + 1 <= 48)
    rng = np.random.default_rng(9)
    K2 = np.minimum(rng.choice([1, 2, 3, 7], F.size), np.maximum(1, (L - F + 2) // 2))
    M2 = np.where(M == 15, rng.integers(1, 15, F.size), M)
    F, L, M, K = (np.concatenate([x, y[short], z[short]]) for x, y, z in ((F, F, F), (L, L, L), (M, M2, 15 & ~M2), (K, K2, K2)))
    for a in (F, L, M, K):
        a.setflags(write=False)
    return F, L, M, K


@functools.lru_cache(maxsize=None)
def longrun_reference(model_type, seed, joined_key):
    """(log_p_none, log_p_some) of longrun_jobs with the joins of joined_key (a tuple, or None)."""
    A, end = rows(model_type, seed)
    F, L, M, K = longrun_jobs(model_type, seed)
    return LR.Chain(A, end, OFF).log_probs(F, L, M, K, None if joined_key is None else np.array(joined_key, bool))


# ---- the variants --------------------------------------------------------------------------------------------------------------------
# chunks without windows, as positions in the grid store's chunk list they are put in front of (13: behind the last chunk): first, last,
# two in a row in the middle, one between the joined chunks 5 and 6
EMPTY_BEFORE = (0, 6, 11, 11, 13)


def with_empty_chunks(store):
    """(the store with chunks without windows put in, for every chunk of it the chunk of `store` it is or -1).  No window moves."""
    src = []
    for c in range(store.n_chunks + 1):
        src += [-1] * EMPTY_BEFORE.count(c)
        if c < store.n_chunks:
            src.append(c)
    src = np.array(src)
    near = np.where(src >= 0, src, 0)                       # (an empty chunk: a contig of its own, no bases)
    off, t = [0], 0
    for s in src:
        t += int(store.chunk_off[s + 1] - store.chunk_off[s]) if s >= 0 else 0
        off.append(t)
    ctg = [store.chunk_ctg[s] if s >= 0 else "empty_%d" % k for k, s in enumerate(src)]
    st = dataclasses.replace(store, chunk_off=np.asarray(off, np.int64), chunk_ctg=ctg, chunk_ctg_len=store.chunk_ctg_len[near].copy(),
                             chunk_s=np.where(src >= 0, store.chunk_s[near], 0).astype(np.int32),
                             chunk_e=np.where(src >= 0, store.chunk_e[near], 0).astype(np.int32))
    assert st.n_windows == store.n_windows and st.n_chunks == store.n_chunks + len(EMPTY_BEFORE)
    return st, src


def empty_chunk_joins(src, j):
    """(joined over the chunks of with_empty_chunks: every chunk without windows and its successor marked as continuing, joined over
    the chunks of the store it was made from as the getter must read that: a chunk without windows ends a run of joined chunks)."""
    dev = np.zeros(src.size, bool)
    ref = np.array(j, bool)
    for k, s in enumerate(src):
        if s >= 0:
            dev[k] = j[s] or (k > 0 and src[k - 1] < 0 and s > 0)
            if k > 0 and src[k - 1] < 0:
                ref[s] = False
        else:
            dev[k] = k > 0
    dev[0] = False
    return dev, ref


FRONT, BEHIND = 5, 7                 # windows in no chunk, before the first chunk and behind the last one


@dataclasses.dataclass
class UncoveredStore(synth.WindowStore):
    """A store whose window arrays hold windows that lie in no chunk: chunk_off[0] > 0 and chunk_off[-1] < n_windows."""
    total: int = 0

    @property
    def n_windows(self) -> int:
        return self.total


def with_uncovered_windows(store, rng):
    """The store with FRONT windows in front of its first chunk and BEHIND windows behind its last one (random values in them)."""
    n = store.n_windows + FRONT + BEHIND
    def pad(a, hi):
        a = np.asarray(a)
        return np.concatenate([rng.integers(0, hi, FRONT).astype(a.dtype), a, rng.integers(0, hi, BEHIND).astype(a.dtype)])
    fields = {f.name: getattr(store, f.name) for f in dataclasses.fields(store)}
    fields.update(cov=pad(store.cov, 70), mapq=pad(store.mapq, 70), clip=pad(store.clip, 70),
                  annot=np.concatenate([store.annot[:1].repeat(FRONT), store.annot, store.annot[-1:].repeat(BEHIND)]),
                  truth=pad(store.truth, 1), prediction=pad(store.prediction, 1),
                  chunk_off=np.asarray(store.chunk_off, np.int64) + FRONT)
    return UncoveredStore(**fields, total=n)
