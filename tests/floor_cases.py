"""The floored stores of tests/test_floor_cpu.py and tests/test_floor_gpu.py: tracks with STRETCHES of windows whose coverage (250) is
an outlier for every state, so that every entry of those windows' rows A_t is a transition probability times the emission floor of
1e-40 (hf_device.h).  A walk in the linear domain loses 133 binary orders of magnitude per such window: the hardest input for every
kernel that carries a vector along the chain.  Each fixture, its jobs and its references are built once per process (lru_cache).

short()   minlen_post_ref.floored_case() as it is: 298 windows, five chunks (40, 64, 100, 24, 70), Gaussian model, one region; floored at a
          chunk's first end, last end, both ends, all of a chunk, and 30 windows inside one.
long()    2 150 windows, four chunks, trunc-exp-Gaussian with two components, HiFi alpha, two regions (coverages 20 and 24: with HiFi
          alpha a state's mean follows the previous window's coverage by up to 46 %, and 250 behind 250 must stay an outlier for every
          component; a region per window at random outside the stretches, one region inside a stretch, but for one change at window
          1100: a region change makes a row uniform).  The pass cuts a chunk of T windows into ceil(T / 512) equal segments of ceil(T / segments) windows, lane j of a
          segment of n windows holds its windows j*L .. j*L + L - 1 with L = ceil(n / 64) (hf_create.h, hf_seg.h):
    chunk 0   0 .. 499        one segment, L = 8.  Floored: 96..127 (32 windows: the whole lanes 12..15), 200..207 (exactly 8: the whole
                              lane 25), 301..307 (exactly 7, inside lane 37)
    chunk 1   500 .. 1799     three segments of 434, 434 and 432 windows.  Floored: 930..1372 = the whole second segment (934..1367)
                              and four windows of each neighbour; the stretch crosses the global grid point 1024 (a multiple of 512 and of 8)
    chunk 2   1800 .. 1949    floored at its last 10 windows
    chunk 3   1950 .. 2149    on chunk 2's contig (joined for run_moments and long_run_log_probs); floored at its first 10 windows

Boundary points (points): every chunk's first and last window +- 1, every stretch's first and last window +- 1, a stretch's first window
+- 8 and +- 9, every multiple of 512 +- 1.  Range jobs: every pair first <= last of them with a seeded mask and region filter; the
breakpoint jobs: the pairs inside one chunk with a mask and its complement; the long-run jobs: longrun_jobs.  The generators' seeds
and the rule for the masks of the long-run jobs were chosen on the CPU so that the REFERENCE meets the device tests' "not vacuous"
conditions (tests/test_floor_cpu.py asserts them: an unselected draw left out 7.4 % of the long-run jobs on short(), these lists 2.1 %
and 0.9 %)."""
import functools

import numpy as np

from flagger_amd import _native as N
from flagger_amd import synth
from test_bruteforce_cpu import _tiny_store
from test_longrun_cpu import max_len
from test_viterbi_cpu import perturbed_model
import breakpoint_ref as BR
import entropy_ref as ER
import interval_ref as IR
import longrun_ref as LR
import minlen_post_ref as MP
import moments_ref as MR
import posterior_ref as PR
import runs_ref as RR
import sampling_ref as S
import viterbi_ref

NAMES = ("short", "long")
COV = 250                                 # the coverage that is an outlier for every state
PIECE, LANE, SEG = 512, 8, 512            # the range getters' grid; the pass's segment cut (HF_SEG_SPLIT)
LONG_LENGTHS = [500, 1300, 150, 200]
LONG_FLOORED = [(96, 127), (200, 207), (301, 307), (930, 1372), (1940, 1949), (1950, 1959)]     # first .. last window, global
LONG_SEED = 5100
LONG_REGIONS = [20, 24]
LONG_REGION_CHANGE = 1100                 # the first window of region 1 inside the stretch 930..1372
JOINS = {"short": (False, False, True, True, True), "long": (False, False, False, True)}
SAMPLES, SAMPLE_SEED = 8, 43
MIN_LEN = (3, 5, 1, 7)
LR_LENGTHS = (1, 2, 3, 7, 9, 16)
LR_BEFORE = (0, 1, 7, 8)                  # a long-run job starts this many windows before a stretch of at least LR_STRETCH windows
LR_STRETCH = 9
# the generators of the masks (tests/test_floor_cpu.py: test_the_jobs_say_something)
MASK_SEED = {"short": 9300, "long": 9301}
BREAKPOINT_MASK_SEED = {"short": 3, "long": 1}
LONGRUN_SEED = {"short": 0, "long": 0}


@functools.lru_cache(maxsize=None)
def long():
    """(store, model, alpha) of the long fixture; nothing of it is changed later."""
    rng = np.random.default_rng(LONG_SEED)
    store = _tiny_store(rng, LONG_LENGTHS, LONG_REGIONS)
    reg = store.regions().astype(np.uint64)
    for a, b in LONG_FLOORED:
        store.cov[a:b + 1] = COV
        reg[a:b + 1] = 0 if b < LONG_REGION_CHANGE else 1      # one region inside a stretch (a region change makes the row uniform) ...
        for t in (a - 1, b + 1):                                # ... and ordinary windows next to it: the stretch has exactly its length
            if 0 <= t < store.n_windows and store.cov[t] != COV:
                store.cov[t] = store.mapq[t] = LONG_REGIONS[int(reg[t])]
                store.clip[t] = 0
    reg[LONG_FLOORED[3][0]:LONG_REGION_CHANGE] = 0              # ... but for the one change inside the long stretch
    store.annot = (store.annot & np.uint64((1 << 58) - 1)) | (reg << np.uint64(58))
    ctg = list(store.chunk_ctg)
    ctg[3] = ctg[2]
    store.chunk_ctg = ctg
    alpha = synth.HIFI_ALPHA
    model = perturbed_model(store, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 2, alpha, rng)
    return store, model, alpha


def short():
    return MP.floored_case()


def fixture(name):
    return {"short": short, "long": long}[name]()


def off_of(name):
    return np.asarray(fixture(name)[0].chunk_off, np.int64)


def joins(name):
    return np.array(JOINS[name], bool)


@functools.lru_cache(maxsize=None)
def stretches(name):
    """[(first, last)] of the maximal runs of windows at coverage COV inside one chunk, in track order."""
    store = fixture(name)[0]
    off = off_of(name)
    hit = np.asarray(store.cov) == COV
    out = []
    for c in range(off.size - 1):
        t = int(off[c])
        while t < off[c + 1]:
            if hit[t]:
                e = t
                while e + 1 < off[c + 1] and hit[e + 1]:
                    e += 1
                out.append((t, e))
                t = e + 1
            else:
                t += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def points(name):
    off = off_of(name)
    n = int(off[-1])
    B = set()
    for o in off:
        B.update([o - 2, o - 1, o, o + 1])                      # (o - 1: a chunk's last window)
    for a, b in stretches(name):
        B.update([a - 1, a, a + 1, b - 1, b, b + 1, a - 8, a + 8, a - 9, a + 9])
    for g in range(PIECE, n, PIECE):
        B.update([g - 1, g, g + 1])
    p = np.array(sorted(int(b) for b in B if 0 <= b < n), np.int64)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def range_jobs(name):
    """(F, L, M, R): every pair first <= last of the boundary points, a mask 1..15 and a region filter -1 .. n_regions - 1."""
    store = fixture(name)[0]
    P = points(name)
    F, L = np.meshgrid(P, P, indexing="ij")
    keep = F <= L
    F, L = F[keep], L[keep]
    rng = np.random.default_rng(MASK_SEED[name])
    M = rng.integers(1, 16, F.size)
    R = rng.integers(-1, store.n_regions, F.size)
    for a in (F, L, M, R):
        a.setflags(write=False)
    return F, L, M, R


@functools.lru_cache(maxsize=None)
def rows(name):
    store, model, alpha = fixture(name)
    return S.rows(store, model, alpha)


# ---- the references, each once per fixture --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def interval_reference(name):
    F, L, M, _ = range_jobs(name)
    A, end = rows(name)
    return IR.log_probs(A, end, off_of(name), F, L, M)


@functools.lru_cache(maxsize=None)
def count_reference(name, unit):
    store = fixture(name)[0]
    F, L, M, R = range_jobs(name)
    A, end = rows(name)
    return MR.moments_long(A, end, off_of(name), MR.weights(store, unit), store.regions().astype(np.int64), F, L, M, R)


@functools.lru_cache(maxsize=None)
def run_reference(name, joined):
    """(mean, var, scale) without (joined False) or with the fixture's joins."""
    F, L, M, _ = range_jobs(name)
    A, end = rows(name)
    return RR.jet_long(A, end, off_of(name), F, L, M, joins(name) if joined else None)


@functools.lru_cache(maxsize=None)
def long_double(name):
    A, end = rows(name)
    return ER.LongDouble(A, end, off_of(name))


@functools.lru_cache(maxsize=None)
def entropy_reference(name):
    F, L, _, _ = range_jobs(name)
    return long_double(name).entropy(F, L)


@functools.lru_cache(maxsize=None)
def log_prob_reference(name):
    """[(name of the labelling, labels, log-probability of every range job)]"""
    F, L, _, _ = range_jobs(name)
    A, end = rows(name)
    ld = long_double(name)
    return [(nm, y, ld.log_probs(F, L, y)) for nm, y in ER.labellings(A, end, off_of(name), 80 + NAMES.index(name))]


@functools.lru_cache(maxsize=None)
def pass_reference(name):
    """(posterior [N][4], chunk log-likelihoods [C], marg [N], cond [N])"""
    store, model, _ = fixture(name)
    A, end = rows(name)
    post, _, ll = PR.forward_backward(A, end, off_of(name), PR.regions_of(store), model.numberOfRegions)
    marg, cond = ER.profile(A, end, off_of(name))
    return post, ll, marg, cond


@functools.lru_cache(maxsize=None)
def sample_reference(name):
    A, end = rows(name)
    return S.ffbs(A, end, off_of(name), SAMPLE_SEED, range(SAMPLES))


@functools.lru_cache(maxsize=None)
def breakpoint_reference(name):
    """((F, L, U, V), log P(E_k) per job): every pair a < b of the boundary points inside one chunk, a left mask and its complement."""
    A, end = rows(name)
    off = off_of(name)
    P = points(name)
    chunk = np.searchsorted(off, P, "right") - 1
    F, L = np.meshgrid(P, P, indexing="ij")
    keep = (F < L) & (chunk[:, None] == chunk[None, :])
    F, L = F[keep], L[keep]
    U = np.random.default_rng(BREAKPOINT_MASK_SEED[name]).integers(1, 15, F.size).astype(np.int64)
    V = 15 & ~U
    events = BR.LongDouble(A, end, off).events(F, L, U, V)
    for a in (F, L, U, V):
        a.setflags(write=False)
    return (F, L, U, V), events


def lr_stretches(name):
    return [s for s in stretches(name) if s[1] - s[0] + 1 >= LR_STRETCH]


@functools.lru_cache(maxsize=None)
def longrun_jobs(name):
    """(F, L, M, K, D): ranges of 4, 12, 20 and 40 windows (cut at the track's end; they may leave their chunk) that start LR_BEFORE
    windows before every stretch of at least LR_STRETCH windows, 3 and 9 windows inside it, and at every boundary point; twelve long
    ranges; a mask that is not full; a length out of LR_LENGTHS cut to what 64 lanes hold, in three jobs of four one that is at most
    half the range.  D: how far before such a stretch the job starts (-1: it does not start within 8 windows before one)."""
    off = off_of(name)
    n = int(off[-1])
    rng = np.random.default_rng(LONGRUN_SEED[name])
    starts = set(int(p) for p in points(name))
    for a, b in lr_stretches(name):
        starts.update(a - d for d in LR_BEFORE if a - d >= 0)
        starts.update([a + 3, a + 9 if a + 9 <= b else b])
    F, L = [], []
    for s in sorted(starts):
        for w in (4, 12, 20, 40):
            F.append(s); L.append(min(n - 1, s + w - 1))
    P = points(name)
    for _ in range(12):
        a, b = sorted(rng.choice(P, 2, replace=False))
        F.append(int(a)); L.append(int(b))
    F, L = np.array(F, np.int64), np.array(L, np.int64)
    M = rng.integers(1, 15, F.size)
    M = np.where(L - F + 1 > 64, (M & ~4) | ((M & ~4) == 0), M)                    # (long ranges: the other labels, test_longrun_cpu.jobs)
    K = rng.choice(LR_LENGTHS, F.size)
    half = np.maximum(1, (L - F + 1) // 2)
    small = np.array([max(k for k in LR_LENGTHS if k <= h) for h in half])
    D = np.full(F.size, -1, np.int64)
    at = np.zeros(F.size, bool)                                                  # the job starts at most 8 windows before or inside such a stretch
    for a, b in lr_stretches(name):
        d = a - F
        D = np.where((d >= 0) & (d <= 8) & (L >= a + 8), d, D)
        at |= (F >= a - 8) & (F <= b)
    # on a floored window of long() only Dup and Hap have weight (Err is beyond its truncation point, Col fails the mapq rule): a job
    # that starts at a stretch asks for a set with exactly one of the two, and for a length of at most half its range, so that its
    # value is neither 0 nor -inf
    M = np.where(at, (M & 9) | rng.choice([2, 4], F.size), M)
    K = np.where(at | (rng.random(F.size) < 0.75), np.minimum(K, small), K)
    K = np.minimum(K, [max_len(m) for m in M]).astype(np.int64)
    for a in (F, L, M, K, D):
        a.setflags(write=False)
    return F, L, M, K, D


@functools.lru_cache(maxsize=None)
def longrun_reference(name, joined):
    """(log_p_none, log_p_some) of longrun_jobs without (joined False) or with the fixture's joins."""
    A, end = rows(name)
    F, L, M, K, _ = longrun_jobs(name)
    return LR.Chain(A, end, off_of(name)).log_probs(F, L, M, K, joins(name) if joined else None)


@functools.lru_cache(maxsize=None)
def viterbi_reference(name):
    return viterbi_ref.reference(*fixture(name))
