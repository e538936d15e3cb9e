"""The C ABI on caller-owned streams and in mixed call orders (DESIGN.md "Streams"): the pass, the thirteen getters (the breakpoint and
long-run getters among them), the eight decoders (hf_viterbi, hf_sample_paths, hf_viterbi_minlen, hf_minlen_posterior,
hf_sample_paths_minlen, hf_viterbi_minlen_joined, hf_minlen_posterior_joined, hf_sample_paths_minlen_joined) and the batch.

Every entry point that enqueues GPU work takes a `void *stream`; the getters run on the stream of the last pass.  Here the stream is a
non-blocking one of the caller's (tests/hip_streams.py), and directly in front of every library call the caller enqueues filler work on
it, so that whatever the library does on the null stream instead, or reads on the host without waiting for the stream, runs ahead of the
stream's work and sees stale data.  Right after an entry point that is asynchronous by contract has returned, hipStreamQuery must still
say hipErrorNotReady: the filler was long enough to matter.

Every comparison is BITWISE (np.array_equal, equal return codes) against a twin that makes the same calls on stream 0 without filler:
the library promises bitwise reproducibility, so there is no tolerance.

The three newest decoders carry state from call to call: hf_viterbi_minlen_joined shares hf_viterbi_minlen's decoder state (backpointer
words, final lanes, chunk scores indexed per chunk by one and per group by the other), and the forward lanes of hf_minlen_posterior and
hf_sample_paths_minlen and the sampler's per-sample slab are sized by a call's arguments, grow and never shrink.  The sequences of
generation 3 (tests/stream_sequences.py) therefore change the arguments from call to call (lanes 16, 64, 4, 64, 7; samples 8, 65, 3,
64; four kinds of joined vector), and because stale state would be equally wrong on the twin, every decoder call of such a sequence
is also compared, bitwise, with the same call on a FRESH context that has run nothing else.  test_generation_3_arguments_equal_the_references
ties those fresh-context results to the float64 numpy references of the features' own tests.  A call that grows a buffer frees the
old one, and hipFree waits for the device: there the busy-stream check only records what it finds (printed; pytest -s).

Generation 4 adds the two whole-contig entry points hf_minlen_posterior_joined and hf_sample_paths_minlen_joined.  They run in the
states of hf_minlen_posterior and hf_sample_paths_minlen, so a state's forward lanes and per-sample slab are grown by either entry
point and serve the narrower calls of both (samples 8, 130, 3, 64 for the joined sampler: three wavefront groups of padded samples,
then one), and each state takes one more buffer, the groups of a call as a chunk list, in its first joined call, which uploads into
it from a host vector of the state's in every joined call.  The busy-stream claim is made for both under their own names wherever
stream_sequences.decoder_arguments says the call grows nothing; the stored results are read per state; and
test_generation_4_arguments_equal_the_references ties the fresh-context results to the references of
tests/test_minlen_sum_joined_gpu.py."""
import collections
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth
import hip_streams as HS
import minlen_joined_ref
import minlen_post_ref
import minlen_ref
import minlen_sample_ref
import minlen_sum_joined_ref
import sampling_ref
import stream_sequences as SQ
import test_minlen_gpu as TML
import test_minlen_joined_gpu as TMJ
import test_minlen_post_gpu as TMP
import test_minlen_sample_gpu as TMS
import test_minlen_sum_joined_gpu as TSJ
import viterbi_ref
from test_posterior_gpu import _ranges, _regions_store, _sizes_store

pytestmark = pytest.mark.gpu

TEG, NB = N.HF_MODEL_TRUNC_EXP_GAUSSIAN, N.HF_MODEL_NEGATIVE_BINOMIAL
# name -> (store, model type, components, alpha, minReadFractionAtEnds)
INPUTS = {
    "config2": (lambda: synth.config(2, 0.03), TEG, 4, synth.HIFI_ALPHA, 0.95),
    "sizes": (_sizes_store, TEG, 3, synth.HIFI_ALPHA, 0.95),           # chunks of 1, 2, 63, 64, 65, 511, 512, 513, 4097 and 13 000 windows
    "regions": (_regions_store, TEG, 6, synth.ONT_R10_ALPHA, 0.8),     # 7 regions
    "negative_binomial": (lambda: synth.config(2, 0.03), NB, 4, np.zeros((4, 4)), 0.95),
}
# name -> (algorithm, statistics mode, environment)
KINDS = {
    "seq": (N.HF_ALGO_SEQ, None, {}),
    "scan-rows": (N.HF_ALGO_SCAN, N.HF_STATS_ROWS, {}),
    "scan-chunks": (N.HF_ALGO_SCAN, N.HF_STATS_CHUNKS, {}),
    # the contexts whose getters run the segment kernel again, into a buffer allocated on first use
    "scan-rows-2-launches": (N.HF_ALGO_SCAN, N.HF_STATS_ROWS, {"HF_SEG_LAUNCHES": "2"}),
    "scan-rows-3-sub-passes": (N.HF_ALGO_SCAN, N.HF_STATS_ROWS, {"HF_SUBPASSES": "3"}),
    "scan-chunks-3-sub-passes": (N.HF_ALGO_SCAN, N.HF_STATS_CHUNKS, {"HF_SUBPASSES": "3"}),
}
GETTERS = SQ.GETTERS
NEW_GETTERS = ("breakpoints", "breakpoint_profile", "long_run_log_probs")
SAMPLES, SAMPLE_SEED = 8, 20261019
MIN_LEN = (3, 5, 1, 7)
BP_MASKS = ((4, 11), (6, 9), (1, 2), (8, 4))      # disjoint (left, right) state sets: one state and several


def _longrun_max_lanes():
    """HF_LONGRUN_MAX_LANES as the header defines it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"#define\s+HF_LONGRUN_MAX_LANES\s+(\d+)", open(os.path.join(root, "include", "hmm_flagger_hip.h")).read())
    assert m
    return int(m.group(1))


class Jobs:
    """The arguments of the getters for one store: whole-track ranges, and sub-ranges across a chunk border and across a 512-window
    border inside the longest chunk (the segment length of the scan path).  The breakpoint jobs (bF < bL inside one chunk) and the
    long-run jobs (F, L, M with the lengths K; `joins`: a chunk continues its predecessor on the same contig) are derived from them."""

    def __init__(self, store):
        off = np.asarray(store.chunk_off, np.int64)
        n = int(off[-1])
        assert off[0] == 0 and n == store.n_windows
        T = np.diff(off)
        c = int(np.argmax(T))
        border = int(off[1 + int(np.argmax(T[:-1] > 0))])
        rng = np.random.default_rng(5)
        a = rng.integers(0, n, 12)
        b = np.minimum(n - 1, a + rng.integers(0, 1500, 12))
        F = [0, max(border - 3, 0), border - 1, 0, n - 1, int(off[c])]
        L = [n - 1, min(border + 3, n - 1), border, 0, n - 1, int(off[c + 1]) - 1]
        assert T[c] > 520                                                                   # (regions: 932 windows in the longest chunk)
        F += [int(off[c]) + 500, int(off[c]) + 511, int(off[c]) + 3]
        L += [int(off[c]) + 520, int(off[c]) + 512, int(off[c]) + min(1100, int(T[c]) - 1)]
        self.n = n
        self.F = np.concatenate([np.asarray(F, np.int64), a])
        self.L = np.concatenate([np.asarray(L, np.int64), b])
        assert np.all(self.F <= self.L)
        self.M = (1 + (np.arange(self.F.size) % 15)).astype(np.int64)
        self.y = np.where(rng.random(n) < 0.95, 2, rng.integers(0, 4, n)).astype(np.int8)
        self.ranges = [(0, n)] + _ranges(store)
        assert any(a0 < border < a0 + cnt for a0, cnt in self.ranges)                      # across a chunk border
        assert any(a0 < int(off[c]) + 512 < a0 + cnt <= int(off[c + 1]) for a0, cnt in self.ranges[1:])   # across a 512-window border
        # breakpoints: the two-window job over the border first, across it, a whole chunk, the random ranges clipped to their chunk
        bF = [int(off[c]) + 511, int(off[c]) + 500, int(off[c]) + 3, int(off[c])]
        bL = [int(off[c]) + 512, int(off[c]) + 520, int(off[c]) + min(1100, int(T[c]) - 1), int(off[c + 1]) - 1]
        for a0, b0 in zip(a, b):
            k = int(np.searchsorted(off, a0, "right")) - 1
            if T[k] < 2:                                   # (a one-window chunk holds no job)
                continue
            lo = min(int(a0), int(off[k + 1]) - 2)
            bF.append(lo)
            bL.append(max(lo + 1, min(int(b0), int(off[k + 1]) - 1)))
        self.bF, self.bL = np.asarray(bF, np.int64), np.asarray(bL, np.int64)
        assert self.bF.size >= 12 and np.all(self.bF < self.bL)
        assert np.array_equal(np.searchsorted(off, self.bF, "right"), np.searchsorted(off, self.bL, "right"))      # one chunk
        assert (self.bF[0], self.bL[0]) == (off[c] + 511, off[c] + 512) and (self.bF[3], self.bL[3]) == (off[c], off[c + 1] - 1)
        self.bU, self.bV = (np.array([BP_MASKS[i % len(BP_MASKS)][k] for i in range(self.bF.size)], np.int64) for k in (0, 1))
        assert not np.any(self.bU & self.bV)
        # long runs: lanes(S, L) = (4 - |S|) + |S| (L - 1) + 4 of include/hmm_flagger_hip.h within HF_LONGRUN_MAX_LANES
        self.K = np.array([(1, 2, 3, 7, 16)[i % 5] for i in range(self.F.size)], np.int64)
        size = np.array([bin(int(m)).count("1") for m in self.M])
        assert np.all((4 - size) + size * (self.K - 1) + 4 <= _longrun_max_lanes()) and set(self.K) == {1, 2, 3, 7, 16}
        ctg = list(store.chunk_ctg)
        self.joins = np.array([k > 0 and ctg[k] == ctg[k - 1] for k in range(T.size)], bool)


@functools.lru_cache(maxsize=None)
def _input(name):
    """(store, model type, K, alpha, frac, parameters A, parameters B, jobs): B is A after one M-step, so the two models' tables, labels
    and posteriors differ."""
    make, mt, K, alpha, frac = INPUTS[name]
    store = make()
    model = hmm.createModel(mt, K, store, alpha)
    va = model.param_vector().copy()
    em = hmm.EMList(store, model, True, frac)
    hmm.EM_runOneIterationForList(em, model)
    la = em.labels()
    hmm.HMM_estimateParameters(model, 1e-3)
    hmm.HMM_resetEstimators(model)
    vb = model.param_vector().copy()
    hmm.EM_runOneIterationForList(em, model)
    assert not np.array_equal(la, em.labels())                 # a getter that answers for the other pass is told apart
    em.close()
    assert not np.array_equal(va, vb)
    return store, mt, K, alpha, frac, va, vb, Jobs(store)


def _model(name, which):
    store, mt, K, alpha, frac, va, vb, _ = _input(name)
    model = hmm.createModel(mt, K, store, alpha)
    model.set_param_vector(vb if which == "b" else va)
    return model


def _call(fn, *args, **kw):
    """(return code, results) of a wrapper of flagger_amd.hmm: the code of the HFError it raises, or HF_OK and copies of what it returns."""
    try:
        out = fn(*args, **kw)
    except N.HFError as e:
        assert e.code != N.HF_OK
        return int(e.code), ()
    if out is None:
        return N.HF_OK, ()
    return N.HF_OK, tuple(np.array(x, copy=True) for x in (out if isinstance(out, tuple) else (out,)))


def _getter_calls(em, kind, J):
    """The calls of one getter operation: [(code, arrays)], the whole track first, then the sub-ranges."""
    if kind == "labels":
        return [_call(em.labels)]
    if kind == "posterior":
        return [_call(em.posterior, a, c) for a, c in J.ranges]
    if kind == "forward_backward":
        return [_call(em.forward_backward, a, c) for a, c in J.ranges]
    if kind == "interval_log_probs":
        return [_call(em.interval_log_probs, J.F, J.L, J.M)]
    if kind == "count_moments":
        return [_call(em.count_moments, J.F, J.L, J.M), _call(em.count_moments, J.F[:4], J.L[:4], J.M[:4], unit="bases")]
    if kind == "run_moments":
        return [_call(em.run_moments, J.F, J.L, J.M)]
    if kind == "path_entropy":
        return [_call(em.path_entropy, J.F, J.L)]
    if kind == "path_log_probs":
        return [_call(em.path_log_probs, J.F, J.L, J.y)]
    if kind == "entropy_profile":
        return [_call(em.entropy_profile, a, c) for a, c in J.ranges]
    if kind == "alpha_stats":
        return [_call(em.alpha_stats)]
    if kind == "breakpoints":
        return [_call(em.breakpoints, J.bF, J.bL, J.bU, J.bV), _call(em.breakpoints, J.bF, J.bL, J.bU, J.bV, ())]
    if kind == "breakpoint_profile":
        return [_call(em.breakpoint_profile, int(J.bF[i]), int(J.bL[i]), int(J.bU[i]), int(J.bV[i])) for i in (0, 1, 5)]
    if kind == "long_run_log_probs":
        return [_call(em.long_run_log_probs, J.F, J.L, J.M, J.K), _call(em.long_run_log_probs, J.F, J.L, J.M, J.K, J.joins)]
    raise KeyError(kind)


def _equal(a, b, what):
    """Two records [(code, arrays)] of the same calls: equal codes, bitwise equal arrays."""
    assert len(a) == len(b), what
    for i, ((ca, xa), (cb, xb)) in enumerate(zip(a, b)):
        assert ca == cb, (what, i, ca, cb)
        assert len(xa) == len(xb), (what, i)
        for k, (x, y) in enumerate(zip(xa, xb)):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), \
                (what, "call %d, array %d" % (i, k), int(np.sum(x != y)) if x.shape == y.shape else (x.shape, y.shape))


def _differ(a, b):
    """Two records of the same calls hold an array that is not bitwise the other's."""
    return any(not np.array_equal(x, y) for (_, xa), (_, xb) in zip(a, b) for x, y in zip(xa, xb))


def _codes(calls):
    return [c for c, _ in calls]


class Side:
    """One side of a comparison: the caller's streams with filler in front of every call and the busy-stream assertions, or (streams all
    0) the twin on the null stream without either.  Contexts made through it are closed before its streams go."""

    def __init__(self, name, kind, streams, non_blocking=True):
        self.name, self.kind, self.streams, self.non_blocking = name, kind, list(streams), non_blocking
        self.store, self.mt, self.K, self.alpha, self.frac, _, _, self.J = _input(name)
        self.h = HS.hip()
        self.contexts = []
        self.busy_checked = 0
        self.busy = collections.Counter()      # (entry point, "asserted" | "grow, busy" | "grow, idle") -> calls (the five newest decoders)
        self.last_samples = {}                 # context -> the samples of the last run in its sampler state (either entry point)

    @property
    def stream(self):
        return self.streams[0]

    def delay(self, s=None):
        self.h.delay(self.stream if s is None else s)

    def assert_busy(self, s, what):
        """The stream still has work when an asynchronous entry point has returned: the filler outlasted the call's host side."""
        if s and self.non_blocking:            # (a null-stream operation inside the call waits for a blocking stream: no hazard, and no claim)
            assert self.h.stream_query(s) == HS.hipErrorNotReady, "%s returned with its stream idle: the filler is too short, or the call blocked" % what
            self.busy_checked += 1

    def check_busy(self, s, what, grows=()):
        """assert_busy for a call of `what` that grows none of its buffers.  A call that grows one (`grows`: the buffers, as
        stream_sequences.decoder_arguments names them) frees the old one, and hipFree waits for the device by design: no claim there,
        only the record of whether the stream was still busy."""
        if not (s and self.non_blocking):
            return
        if not grows:
            self.assert_busy(s, what)
            self.busy[what, "asserted"] += 1
        else:
            self.busy[what, "grow, busy" if self.h.stream_query(s) == HS.hipErrorNotReady else "grow, idle"] += 1

    def context(self, stream=None, model=None, alpha_stats=False):
        algo, mode, env = KINDS[self.kind]
        s = self.stream if stream is None else stream
        em = hmm.EMList(self.store, model or _model(self.name, "a"), True, self.frac, algo=algo, stream=s)
        self.contexts.append(em)
        if algo == N.HF_ALGO_SCAN:
            assert em.seg_launches == int(env.get("HF_SEG_LAUNCHES", 1)) and em.sub_passes == int(env.get("HF_SUBPASSES", 1))
            em.set_stats_mode(mode)
        if alpha_stats and self.mt != NB:
            em.set_alpha_stats(True)
        return em

    def close(self):
        for em in self.contexts:
            em.close()
        self.contexts = []

    # --- the calls, each behind a delay -------------------------------------------------------------------------------------
    def estep(self, em, model, mode=N.HF_MODE_FULL):
        """hf_estep + hf_finish: (code, (statistics,))."""
        s = em.stream.value or 0
        self.delay(s)
        code, _ = _call(em.launch, model, mode)
        if code != N.HF_OK:
            return code, ()
        self.assert_busy(s, "hf_estep")
        return self.finish(em)

    def finish(self, em):
        self.delay(em.stream.value or 0)
        return _call(em.finish)

    def getter(self, em, kind):
        self.delay(em.stream.value or 0)
        return _getter_calls(em, kind, self.J)

    def viterbi(self, em, model, s=None):
        """hf_viterbi + hf_viterbi_finish on stream `s` (default: the context's) and its getters: (code, (labels, chunk scores, score))."""
        L, s = N.lib(), (em.stream.value or 0) if s is None else s
        p, lp = model.params(), C.c_double(0.0)
        self.delay(s)
        rc = L.hf_viterbi(em._h, C.byref(p), C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        self.assert_busy(s, "hf_viterbi")
        rc = L.hf_viterbi_finish(em._h, C.byref(lp), C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        labels = np.empty(self.store.n_windows, dtype=np.int8)
        ll = np.empty(self.store.n_chunks, dtype=np.float64)
        self.delay(s)
        r1 = L.hf_get_viterbi_labels(em._h, labels.ctypes.data_as(C.POINTER(C.c_int8)))
        r2 = L.hf_get_viterbi_chunk_log_probs(em._h, ll.ctypes.data_as(C.POINTER(C.c_double)))
        assert r1 == N.HF_OK and r2 == N.HF_OK
        return N.HF_OK, (labels, ll, np.float64(lp.value))

    def sample(self, em, model, s=None, n=SAMPLES, seed=SAMPLE_SEED):
        """hf_sample_paths + hf_sample_finish on stream `s` and the samples' labels: (code, (int8[n][n_windows],))."""
        L, s = N.lib(), (em.stream.value or 0) if s is None else s
        assert em.sample_capacity >= n
        p = model.params()
        self.delay(s)
        rc = L.hf_sample_paths(em._h, C.byref(p), 0, n, seed, C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        self.assert_busy(s, "hf_sample_paths")
        rc = L.hf_sample_finish(em._h, C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        out = np.empty((n, self.store.n_windows), dtype=np.int8)
        self.delay(s)
        for k in range(n):
            assert L.hf_get_sample_labels(em._h, k, out[k].ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_OK
        return N.HF_OK, (out,)

    def viterbi_minlen(self, em, model, s=None, min_len=MIN_LEN):
        """hf_viterbi_minlen + hf_viterbi_minlen_finish on stream `s` (default: the context's) and its getters: (code, (labels, chunk
        scores, score))."""
        L, s = N.lib(), (em.stream.value or 0) if s is None else s
        p, lp = model.params(), C.c_double(0.0)
        ml = (C.c_int32 * 4)(*min_len)
        self.delay(s)
        rc = L.hf_viterbi_minlen(em._h, C.byref(p), ml, C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        self.assert_busy(s, "hf_viterbi_minlen")
        rc = L.hf_viterbi_minlen_finish(em._h, C.byref(lp), C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        labels = np.empty(self.store.n_windows, dtype=np.int8)
        ll = np.empty(self.store.n_chunks, dtype=np.float64)
        self.delay(s)
        r1 = L.hf_get_viterbi_minlen_labels(em._h, labels.ctypes.data_as(C.POINTER(C.c_int8)))
        r2 = L.hf_get_viterbi_minlen_chunk_log_probs(em._h, ll.ctypes.data_as(C.POINTER(C.c_double)))
        assert r1 == N.HF_OK and r2 == N.HF_OK
        return N.HF_OK, (labels, ll, np.float64(lp.value))

    def viterbi_minlen_joined(self, em, model, s=None, min_len=MIN_LEN, join="null"):
        """hf_viterbi_minlen_joined + hf_viterbi_minlen_finish on stream `s` with the joined vector stream_sequences.join_vector(join)
        and the getters it shares with hf_viterbi_minlen: (code, (labels, chunk scores, score)).  Asynchronous "as hf_viterbi_minlen
        is": the stream is still busy when it returns, in every call."""
        L, s = N.lib(), (em.stream.value or 0) if s is None else s
        p, lp = model.params(), C.c_double(0.0)
        ml = (C.c_int32 * 4)(*min_len)
        jv = SQ.join_vector(join, self.store.n_chunks)
        ja = None if jv is None else np.asarray(jv, np.uint8)
        self.delay(s)
        rc = L.hf_viterbi_minlen_joined(em._h, C.byref(p), ml, None if ja is None else ja.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        self.check_busy(s, "hf_viterbi_minlen_joined")
        rc = L.hf_viterbi_minlen_finish(em._h, C.byref(lp), C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        labels = np.empty(self.store.n_windows, dtype=np.int8)
        ll = np.empty(self.store.n_chunks, dtype=np.float64)
        self.delay(s)
        r1 = L.hf_get_viterbi_minlen_labels(em._h, labels.ctypes.data_as(C.POINTER(C.c_int8)))
        r2 = L.hf_get_viterbi_minlen_chunk_log_probs(em._h, ll.ctypes.data_as(C.POINTER(C.c_double)))
        assert r1 == N.HF_OK and r2 == N.HF_OK
        return N.HF_OK, (labels, ll, np.float64(lp.value))

    def _minlen_posterior_results(self, em):
        """(code, (posterior over every window in a chunk, labels, chunk log mass, chunk log Z_adm)) of the getters."""
        L, n, pd = N.lib(), self.store.n_windows, C.POINTER(C.c_double)
        assert self.J.n == n                                   # (every window of these stores lies in a chunk)
        post = np.empty((n, 4), dtype=np.float64)
        labels = np.empty(n, dtype=np.int8)
        mass, lza = np.empty(self.store.n_chunks, dtype=np.float64), np.empty(self.store.n_chunks, dtype=np.float64)
        for rc in (L.hf_get_minlen_posterior(em._h, 0, n, post.ctypes.data_as(pd)),
                   L.hf_get_minlen_posterior_labels(em._h, labels.ctypes.data_as(C.POINTER(C.c_int8))),
                   L.hf_get_minlen_chunk_log_mass(em._h, mass.ctypes.data_as(pd), lza.ctypes.data_as(pd))):
            if rc != N.HF_OK:
                return int(rc), ()
        return N.HF_OK, (post, labels, mass, lza)

    def minlen_posterior(self, em, model, s=None, min_len=MIN_LEN, grows=()):
        """hf_minlen_posterior + hf_minlen_posterior_finish on stream `s` and its getters: (code, (posterior, labels, chunk log mass,
        chunk log Z_adm, total)).  `grows`: the buffers the call grows (check_busy)."""
        L, s = N.lib(), (em.stream.value or 0) if s is None else s
        p, tot = model.params(), C.c_double(0.0)
        ml = (C.c_int32 * 4)(*min_len)
        self.delay(s)
        rc = L.hf_minlen_posterior(em._h, C.byref(p), ml, C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        self.check_busy(s, "hf_minlen_posterior", grows)
        rc = L.hf_minlen_posterior_finish(em._h, C.byref(tot), C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        self.delay(s)
        code, arrays = self._minlen_posterior_results(em)
        assert code == N.HF_OK
        return N.HF_OK, arrays + (np.float64(tot.value),)

    def _minlen_samples(self, em, n):
        """(code, (int8[n][n_windows],)) of hf_get_minlen_sample_labels; the sample behind the last one is refused."""
        L = N.lib()
        out = np.empty((n, self.store.n_windows), dtype=np.int8)
        for k in range(n):
            rc = L.hf_get_minlen_sample_labels(em._h, k, out[k].ctypes.data_as(C.POINTER(C.c_int8)))
            if rc != N.HF_OK:
                return int(rc), ()
        spare = np.empty(self.store.n_windows, dtype=np.int8)
        assert L.hf_get_minlen_sample_labels(em._h, n, spare.ctypes.data_as(C.POINTER(C.c_int8))) == N.HF_E_ARG
        return N.HF_OK, (out,)

    def sample_minlen(self, em, model, s=None, min_len=MIN_LEN, n=SAMPLES, seed=SAMPLE_SEED, grows=()):
        """hf_sample_paths_minlen + hf_sample_minlen_finish on stream `s` and the samples' labels: (code, (int8[n][n_windows],)).
        `grows`: the buffers the call grows (check_busy)."""
        L, s = N.lib(), (em.stream.value or 0) if s is None else s
        assert em.minlen_sample_capacity(min_len) >= n
        p = model.params()
        ml = (C.c_int32 * 4)(*min_len)
        self.delay(s)
        rc = L.hf_sample_paths_minlen(em._h, C.byref(p), ml, 0, n, seed, C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        self.check_busy(s, "hf_sample_paths_minlen", grows)
        rc = L.hf_sample_minlen_finish(em._h, C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        self.last_samples[id(em)] = n
        self.delay(s)
        code, arrays = self._minlen_samples(em, n)
        assert code == N.HF_OK
        return N.HF_OK, arrays

    def _joined_pointer(self, join):
        """(the uint8 array that holds stream_sequences.join_vector(join), its pointer for the C ABI): (None, None) for "null"."""
        jv = SQ.join_vector(join, self.store.n_chunks)
        if jv is None:
            return None, None
        ja = np.asarray(jv, np.uint8)
        return ja, ja.ctypes.data_as(C.POINTER(C.c_uint8))

    def minlen_posterior_joined(self, em, model, s=None, min_len=MIN_LEN, join="null", grows=()):
        """hf_minlen_posterior_joined + hf_minlen_posterior_finish on stream `s` with the joined vector stream_sequences.join_vector(join)
        and the getters it shares with hf_minlen_posterior: (code, (posterior, labels, chunk log mass, chunk log Z_adm, total)).
        Asynchronous "as hf_minlen_posterior is": the stream is still busy when it returns, unless the call grows a buffer (`grows`)."""
        L, s = N.lib(), (em.stream.value or 0) if s is None else s
        p, tot = model.params(), C.c_double(0.0)
        ml = (C.c_int32 * 4)(*min_len)
        ja, jp = self._joined_pointer(join)
        self.delay(s)
        rc = L.hf_minlen_posterior_joined(em._h, C.byref(p), ml, jp, C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        self.check_busy(s, "hf_minlen_posterior_joined", grows)
        rc = L.hf_minlen_posterior_finish(em._h, C.byref(tot), C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        self.delay(s)
        code, arrays = self._minlen_posterior_results(em)
        assert code == N.HF_OK
        return N.HF_OK, arrays + (np.float64(tot.value),)

    def sample_minlen_joined(self, em, model, s=None, min_len=MIN_LEN, n=SAMPLES, seed=SAMPLE_SEED, join="null", grows=()):
        """hf_sample_paths_minlen_joined + hf_sample_minlen_finish on stream `s` with the joined vector
        stream_sequences.join_vector(join) and the getter it shares with hf_sample_paths_minlen: (code, (int8[n][n_windows],))."""
        L, s = N.lib(), (em.stream.value or 0) if s is None else s
        assert em.minlen_sample_capacity(min_len) >= n
        p = model.params()
        ml = (C.c_int32 * 4)(*min_len)
        ja, jp = self._joined_pointer(join)
        self.delay(s)
        rc = L.hf_sample_paths_minlen_joined(em._h, C.byref(p), ml, jp, 0, n, seed, C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        self.check_busy(s, "hf_sample_paths_minlen_joined", grows)
        rc = L.hf_sample_minlen_finish(em._h, C.c_void_p(s))
        if rc != N.HF_OK:
            return int(rc), ()
        self.last_samples[id(em)] = n
        self.delay(s)
        code, arrays = self._minlen_samples(em, n)
        assert code == N.HF_OK
        return N.HF_OK, arrays

    def decoder(self, em, which, model, s=None, args=None, grows=()):
        """Decoder `which` with the arguments stream_sequences.decoder_arguments gives for the call (default: MIN_LEN, SAMPLES, no join)."""
        args = args or {}
        kw = {"min_len": args["min_len"]} if "min_len" in args else {}
        if which == "minlen_posterior_joined":
            return self.minlen_posterior_joined(em, model, s, join=args.get("join", "null"), grows=grows, **kw)
        if which == "sample_minlen_joined":
            return self.sample_minlen_joined(em, model, s, n=args.get("n_samples", SAMPLES), join=args.get("join", "null"), grows=grows, **kw)
        if which == "minlen_posterior":
            return self.minlen_posterior(em, model, s, grows=grows, **kw)
        if which == "sample_minlen":
            return self.sample_minlen(em, model, s, n=args.get("n_samples", SAMPLES), grows=grows, **kw)
        if which == "viterbi_minlen_joined":
            return self.viterbi_minlen_joined(em, model, s, join=args.get("join", "null"), **kw)
        if which == "viterbi_minlen":
            return self.viterbi_minlen(em, model, s, **kw)
        return {"viterbi": self.viterbi, "sample": self.sample}[which](em, model, s)

    def stored(self, em, which, s=None):
        """What the getters of decoder `which` answer now, behind a delay: (code, arrays) with the arrays in the order of the decoder's
        own record (its score, a value of the finish call, is not stored).  "viterbi_minlen" and "viterbi_minlen_joined" share their
        state and their getters: either name reads the results of the later of the two calls, and so do "minlen_posterior" and
        "minlen_posterior_joined", "sample_minlen" and "sample_minlen_joined" (as many samples as the later of the two calls on `em`
        drew)."""
        L = N.lib()
        self.delay((em.stream.value or 0) if s is None else s)
        if which in ("minlen_posterior", "minlen_posterior_joined"):
            return self._minlen_posterior_results(em)
        if which in ("sample_minlen", "sample_minlen_joined"):
            return self._minlen_samples(em, self.last_samples[id(em)])
        if which == "sample":
            out = np.empty((SAMPLES, self.store.n_windows), dtype=np.int8)
            for k in range(SAMPLES):
                rc = L.hf_get_sample_labels(em._h, k, out[k].ctypes.data_as(C.POINTER(C.c_int8)))
                if rc != N.HF_OK:
                    return int(rc), ()
            return N.HF_OK, (out,)
        get_labels, get_ll = (L.hf_get_viterbi_labels, L.hf_get_viterbi_chunk_log_probs) if which == "viterbi" else \
            (L.hf_get_viterbi_minlen_labels, L.hf_get_viterbi_minlen_chunk_log_probs)
        labels = np.empty(self.store.n_windows, dtype=np.int8)
        ll = np.empty(self.store.n_chunks, dtype=np.float64)
        r1 = get_labels(em._h, labels.ctypes.data_as(C.POINTER(C.c_int8)))
        r2 = get_ll(em._h, ll.ctypes.data_as(C.POINTER(C.c_double)))
        if r1 != N.HF_OK or r2 != N.HF_OK:
            return int(r1 or r2), ()
        return N.HF_OK, (labels, ll)


# decoder -> the name under which Side.stored reads its state, where two entry points share one
STATE_READER = {"viterbi_minlen_joined": "viterbi_minlen", "minlen_posterior_joined": "minlen_posterior", "sample_minlen_joined": "sample_minlen"}


def _first_call_grows(decoder):
    """What the first call of `decoder` on a context grows: every buffer of its state, and "grp" where it is a joined entry point."""
    return SQ.STATE_BUFFERS.get(SQ.STATES.get(decoder), ()) + (("grp",) if decoder in SQ.JOINED_DECODERS else ())


def _stored_equals(stored, returned, what):
    """A decoder's stored results against the record of the call that made them."""
    (code, arrays), (rcode, rarrays) = stored, returned
    assert code == rcode == N.HF_OK, (what, code, rcode)
    _equal([(code, arrays)], [(rcode, rarrays[:len(arrays)])], what)


def _run_both(name, kind, monkeypatch, scenario, n_streams=1, non_blocking=True):
    """`scenario(side)` -> {tag: [(code, arrays)]} on the caller's streams and on the null stream: the two records are equal.  Returns the
    record of the streams' side."""
    for k, v in KINDS[kind][2].items():
        monkeypatch.setenv(k, v)
    _input(name)
    recs = []
    with HS.Streams() as streams:
        for which in ("streams", "twin"):
            side = Side(name, kind, [streams.new(non_blocking) if which == "streams" else 0 for _ in range(n_streams)], non_blocking)
            try:
                recs.append(scenario(side))
            finally:
                side.close()
    got, twin = recs
    assert list(got) == list(twin)
    for tag in got:
        _equal(got[tag], twin[tag], "%s / %s / %s" % (name, kind, tag))
    return got


CASES = [pytest.param(n, k, id="%s-%s" % (n, k)) for n in INPUTS for k in KINDS]
ON_CONFIG2 = [pytest.param("config2", k, id=k) for k in KINDS]


# ---- a. the pass -------------------------------------------------------------------------------------------------------------------
def _pass_scenario(side):
    ma, mb = _model(side.name, "a"), _model(side.name, "b")
    em = side.context()
    rec = {}
    rec["full a"] = [side.estep(em, ma)]
    side.delay()
    rec["labels a"] = [_call(em.labels)]
    rec["full b"] = [side.estep(em, mb)]                         # must not see a's parameter block or tables
    side.delay()
    rec["labels b"] = [_call(em.labels)]
    # two passes back to back: hf_estep(a), hf_estep(b), then one hf_finish — b is enqueued while a's parameter upload and tables still
    # wait behind the filler (the pinned parameter block is packed again under a pending copy): b's results must be b's
    side.delay()
    c1, _ = _call(em.launch, ma, N.HF_MODE_FULL)
    c2, _ = _call(em.launch, mb, N.HF_MODE_FULL)
    side.assert_busy(side.stream, "hf_estep")
    rec["a then b, back to back"] = [(c1, ()), (c2, ()), side.finish(em)]
    side.delay()
    rec["labels b, back to back"] = [_call(em.labels)]
    rec["forward a"] = [side.estep(em, ma, N.HF_MODE_FORWARD_ONLY)]
    rec["forward b"] = [side.estep(em, mb, N.HF_MODE_FORWARD_ONLY)]
    # hf_estep + hf_check (what the multi-GPU path of flagger_amd/dist.py calls), then the statistics through hf_finish
    side.delay()
    code, _ = _call(em.launch, ma, N.HF_MODE_FULL)
    side.assert_busy(side.stream, "hf_estep")
    side.delay()
    rec["check a"] = [(code, ()), _call(em.check), _call(em.finish)]
    # hf_em_iterate: two iterations, the model moves in between
    mi = _model(side.name, "a")
    it = []
    for _ in range(2):
        side.delay()
        code, out = _call(em.em_iterate, mi, True, 1e-3)
        it.append((code, out + (mi.estimators.copy(), mi.param_vector().copy(), np.float64(mi.loglikelihood))))
    rec["em_iterate"] = it
    side.delay()
    rec["labels after em_iterate"] = [_call(em.labels)]
    return rec


def _check_pass_record(rec):
    assert all(c == N.HF_OK for calls in rec.values() for c in _codes(calls)), {t: _codes(c) for t, c in rec.items()}
    sa, sb = rec["full a"][0][1][0], rec["full b"][0][1][0]
    assert not np.array_equal(sa, sb) and not np.array_equal(rec["labels a"][0][1][0], rec["labels b"][0][1][0])
    assert rec["forward a"][0][1][0][0] != rec["forward b"][0][1][0][0]                               # the log-likelihoods
    assert np.array_equal(rec["check a"][2][1][0], sa)
    assert np.array_equal(rec["a then b, back to back"][2][1][0], sb)
    _equal(rec["labels b, back to back"], rec["labels b"], "labels of b enqueued right behind a")
    assert np.array_equal(rec["em_iterate"][0][1][1], sa)


@pytest.mark.parametrize("name,kind", CASES)
def test_pass_on_a_non_blocking_stream(name, kind, monkeypatch):
    _check_pass_record(_run_both(name, kind, monkeypatch, _pass_scenario))


@pytest.mark.parametrize("name,kind", ON_CONFIG2)
def test_pass_on_a_blocking_stream(name, kind, monkeypatch):
    """The same on a stream created with the default flags (the null stream waits for it, so nothing can run ahead: the values only)."""
    _check_pass_record(_run_both(name, kind, monkeypatch, _pass_scenario, non_blocking=False))


# ---- b. every getter, first and second call ----------------------------------------------------------------------------------------
def _getters_of(side):
    return [g for g in GETTERS if not (g == "alpha_stats" and side.mt == NB)]


@pytest.mark.parametrize("name,kind", CASES)
def test_getters_first_and_second_call(name, kind, monkeypatch):
    def scenario(side):
        em = side.context(alpha_stats=True)
        rec = {"pass a": [side.estep(em, _model(name, "a"))]}
        for g in NEW_GETTERS:
            rec[g + ", after pass a"] = side.getter(em, g)          # (their lazy state is in place, for pass a, when pass b runs)
        rec["pass b"] = [side.estep(em, _model(name, "b"))]
        for g in _getters_of(side):
            rec[g + ", first call"] = side.getter(em, g)            # builds the getter's lazy state
            rec[g + ", second call"] = side.getter(em, g)           # uses it
        return rec

    rec = _run_both(name, kind, monkeypatch, scenario)
    for tag, calls in rec.items():
        assert all(c == N.HF_OK for c in _codes(calls)), (tag, _codes(calls))
        if tag.endswith("first call"):
            _equal(calls, rec[tag.replace("first", "second")], tag)
    for g in NEW_GETTERS:                                           # a getter that answers for the wrong pass is told apart
        assert _differ(rec[g + ", first call"], rec[g + ", after pass a"]), g
    whole = rec["posterior, first call"][0][1][0]
    assert np.array_equal(whole.argmax(axis=1).astype(np.int8), rec["labels, first call"][0][1][0])
    for (a, c), (_, part) in zip(_input(name)[7].ranges, rec["posterior, first call"]):
        assert np.array_equal(part[0], whole[a:a + c]), (a, c)


@pytest.mark.parametrize("name,kind", CASES)
def test_each_getter_as_the_first_after_the_pass(name, kind, monkeypatch):
    """A context of its own per getter: the getter's first call is the first thing after the pass, behind a delay, with nothing of any
    other getter's lazy state in place."""
    def scenario(side):
        rec = {}
        for i, g in enumerate(_getters_of(side)):
            em = side.context(alpha_stats=True)
            w = "ab"[i % 2]
            side.estep(em, _model(name, "ab"[1 - i % 2]))
            rec[g + " pass " + w] = [side.estep(em, _model(name, w))]
            rec[g] = side.getter(em, g)
            em.close()
        return rec

    rec = _run_both(name, kind, monkeypatch, scenario)
    assert all(c == N.HF_OK for calls in rec.values() for c in _codes(calls))


# ---- c. decoders --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["same-stream", "second-stream"])
@pytest.mark.parametrize("name,kind", CASES)
def test_decoders_with_other_parameters(name, kind, where, monkeypatch):
    """hf_viterbi, hf_sample_paths and hf_viterbi_minlen with parameters other than the pass's, on the pass's stream or on a second
    non-blocking stream: their own results, afterwards every getter still answers for the pass — its first (lazy) call included —
    and each decoder's stored results are its own: three decoders, none overwrites another."""
    def scenario(side):
        ma, mb = _model(name, "a"), _model(name, "b")
        s2 = side.streams[1] if where == "second-stream" else None
        em = side.context(alpha_stats=True)
        rec = {"pass b": [side.estep(em, mb)]}
        rec["viterbi a"] = [side.viterbi(em, ma, s2)]
        rec["sample a"] = [side.sample(em, ma, s2)]
        rec["viterbi_minlen a"] = [side.viterbi_minlen(em, ma, s2)]
        for g in _getters_of(side):
            rec[g + " after the decoders"] = side.getter(em, g)
        rec["viterbi a again"] = [side.viterbi(em, ma, s2)]
        rec["sample a again"] = [side.sample(em, ma, s2)]
        rec["viterbi_minlen a again"] = [side.viterbi_minlen(em, ma, s2)]
        for g in _getters_of(side):
            rec[g + " after the decoders again"] = side.getter(em, g)
        for d in SQ.DECODERS:
            rec[d + " stored"] = [side.stored(em, d, s2)]
        # what the getters must still answer: the pass alone, on a context that never decoded
        alone = side.context(alpha_stats=True)
        rec["alone pass b"] = [side.estep(alone, mb)]
        for g in _getters_of(side):
            rec[g + " alone"] = side.getter(alone, g)
        rec["viterbi b alone"] = [side.viterbi(alone, mb, s2)]
        return rec

    rec = _run_both(name, kind, monkeypatch, scenario, n_streams=2)
    assert all(c == N.HF_OK for calls in rec.values() for c in _codes(calls)), {t: _codes(c) for t, c in rec.items()}
    _equal(rec["viterbi a"], rec["viterbi a again"], "viterbi")
    _equal(rec["sample a"], rec["sample a again"], "sample")
    _equal(rec["viterbi_minlen a"], rec["viterbi_minlen a again"], "viterbi_minlen")
    assert not np.array_equal(rec["viterbi_minlen a"][0][1][0], rec["viterbi a"][0][1][0])         # the constraint bites
    for d in SQ.DECODERS:
        _stored_equals(rec[d + " stored"][0], rec[d + " a again"][0], d + " stored")
    assert not np.array_equal(rec["viterbi a"][0][1][0], rec["viterbi b alone"][0][1][0])          # (the decoders' model is another one)
    for g in GETTERS:
        if g + " alone" in rec:
            _equal(rec[g + " after the decoders"], rec[g + " alone"], g)
            _equal(rec[g + " after the decoders again"], rec[g + " alone"], g)


SIX = SQ.DECODERS + SQ.MINLEN_DECODERS
EIGHT = SIX + SQ.JOINED_DECODERS
FAMILY_ARGS = {"min_len": MIN_LEN, "n_samples": SAMPLES, "join": "random"}
FAMILY_ZEROS = dict(FAMILY_ARGS, join="zeros")
FAMILY = [pytest.param(n, k, id="%s-%s" % (n, k)) for n in ("config2", "sizes") for k in ("seq", "scan-rows")]


@pytest.mark.parametrize("where", ["same-stream", "second-stream"])
@pytest.mark.parametrize("name,kind", FAMILY)
def test_minlen_family_with_other_parameters(name, kind, where, monkeypatch):
    """All eight decoders with parameters other than the pass's, on the pass's stream or on a second non-blocking stream, twice: the two
    runs are equal (the second grows no buffer: the stream is still busy when each of the new entry points returns), afterwards every
    getter still answers for the pass, and each decoder's stored results are its own last ones.  hf_viterbi_minlen and
    hf_viterbi_minlen_joined share their state: the stored results are those of the later of the two, in every chunk entry (the exact
    zeros a joined call leaves in a group's other chunks included), and nothing of the earlier one's — in either order.  So do
    hf_minlen_posterior and hf_minlen_posterior_joined (both arrays of hf_get_minlen_chunk_log_mass), and hf_sample_paths_minlen and
    hf_sample_paths_minlen_joined: the six are read once the six have run (the per-chunk entry points the later ones), the two
    shared states again after the joined calls, and again after a per-chunk call that follows those.  At the end both joined entry
    points run with another joined vector (all zero: nothing is joined) and with the first again: the results are those of a context
    that ran that call alone and, the header's exact case, those of the per-chunk entry point, so the groups of the call before are
    gone from the state's device buffer."""
    def scenario(side):
        ma, mb = _model(name, "a"), _model(name, "b")
        s2 = side.streams[1] if where == "second-stream" else None
        em = side.context(alpha_stats=True)
        rec = {"pass b": [side.estep(em, mb)]}
        for d in EIGHT:                                           # (a state's first call grows every buffer, its first joined call "grp")
            rec[d + " a"] = [side.decoder(em, d, ma, s2, FAMILY_ARGS, SQ.BUFFERS.get(d, ()) + (("grp",) if d in SQ.JOINED_DECODERS else ()))]
        for g in _getters_of(side):
            rec[g + " after the decoders"] = side.getter(em, g)
        for d in SIX:
            rec[d + " a again"] = [side.decoder(em, d, ma, s2, FAMILY_ARGS)]
        for d in SIX:                                             # "viterbi_minlen": the shared state, the joined call the later one
            rec[d + " stored"] = [side.stored(em, d, s2)]
        for d in SQ.JOINED_DECODERS:                              # per-chunk, then joined
            rec[d + " a again"] = [side.decoder(em, d, ma, s2, FAMILY_ARGS)]
        for g in _getters_of(side):
            rec[g + " after the decoders again"] = side.getter(em, g)
        for d in SQ.JOINED_DECODERS:
            rec[d + " stored"] = [side.stored(em, d, s2)]
        rec["viterbi_minlen a, after the joined call"] = [side.viterbi_minlen(em, ma, s2)]
        rec["viterbi_minlen stored, after the joined call"] = [side.stored(em, "viterbi_minlen", s2)]
        for d in SQ.JOINED_DECODERS:                              # joined, then per-chunk
            rec[STATE_READER[d] + " a, after the joined call"] = [side.decoder(em, STATE_READER[d], ma, s2, FAMILY_ARGS)]
            rec[STATE_READER[d] + " stored, after the joined call"] = [side.stored(em, STATE_READER[d], s2)]
        fresh = side.context()
        for d in SQ.JOINED_DECODERS:                              # another joined vector, then the first again: the groups are cut per call
            rec[d + " a, zeros"] = [side.decoder(em, d, ma, s2, FAMILY_ZEROS)]
            rec[d + " a, random again"] = [side.decoder(em, d, ma, s2, FAMILY_ARGS)]
            rec[d + " a, zeros, alone"] = [side.decoder(fresh, d, ma, s2, FAMILY_ZEROS, _first_call_grows(d))]
        alone = side.context(alpha_stats=True)
        rec["alone pass b"] = [side.estep(alone, mb)]
        for g in _getters_of(side):
            rec[g + " alone"] = side.getter(alone, g)
        if side.stream:
            print("%s %s %s: busy-stream checks in the family: %s" % (name, kind, where, _busy_counts(side.busy)))
        return rec

    rec = _run_both(name, kind, monkeypatch, scenario, n_streams=2)
    store = _input(name)[0]
    assert all(c == N.HF_OK for calls in rec.values() for c in _codes(calls)), {t: _codes(c) for t, c in rec.items()}
    for d in EIGHT:
        _equal(rec[d + " a"], rec[d + " a again"], d)
    for d in ("viterbi", "sample", "minlen_posterior", "sample_minlen", "viterbi_minlen_joined"):
        _stored_equals(rec[d + " stored"][0], rec[d + " a again"][0], d + " stored")
    # the shared state: the joined call was the later one; then hf_viterbi_minlen is
    joined, minlen = rec["viterbi_minlen_joined a again"][0], rec["viterbi_minlen a again"][0]
    assert sum(SQ.join_vector("random", store.n_chunks)) >= 1
    assert not np.array_equal(joined[1][1], minlen[1][1])                                          # (the two differ, so a mix would show)
    _stored_equals(rec["viterbi_minlen stored"][0], joined, "the shared state after the joined call")
    _check_chunk_entries(store, rec["viterbi_minlen stored"][0][1][1], "viterbi_minlen_joined", FAMILY_ARGS)
    _equal(rec["viterbi_minlen a, after the joined call"], rec["viterbi_minlen a again"], "hf_viterbi_minlen after a joined call")
    _stored_equals(rec["viterbi_minlen stored, after the joined call"][0], minlen, "the shared state after hf_viterbi_minlen")
    _check_chunk_entries(store, rec["viterbi_minlen stored, after the joined call"][0][1][1], "viterbi_minlen", FAMILY_ARGS)
    assert not np.array_equal(rec["viterbi_minlen a"][0][1][0], rec["viterbi a"][0][1][0])         # the constraint bites
    # the two newer shared states: the joined call the later one, then the per-chunk call
    for d in SQ.JOINED_DECODERS:
        per_chunk = STATE_READER[d]
        joined, chunk = rec[d + " a again"][0], rec[per_chunk + " a again"][0]
        assert not np.array_equal(joined[1][0], chunk[1][0]), d                                    # (the two differ, so a mix would show)
        _stored_equals(rec[d + " stored"][0], joined, "the shared state after " + d)
        _equal(rec[per_chunk + " a, after the joined call"], rec[per_chunk + " a again"], per_chunk + " after a joined call")
        _stored_equals(rec[per_chunk + " stored, after the joined call"][0], chunk, "the shared state after " + per_chunk)
    for tag, op in (("minlen_posterior_joined stored", "minlen_posterior_joined"), ("minlen_posterior stored", "minlen_posterior"),
                    ("minlen_posterior stored, after the joined call", "minlen_posterior")):
        _check_mass_entries(store, rec[tag][0][1][2], rec[tag][0][1][3], op, FAMILY_ARGS)
    joined, chunk = rec["minlen_posterior_joined a again"][0][1], rec["minlen_posterior a again"][0][1]
    assert not np.array_equal(joined[2], chunk[2]) and not np.array_equal(joined[3], chunk[3])
    for d in SQ.JOINED_DECODERS:
        _equal(rec[d + " a, zeros"], rec[d + " a, zeros, alone"], d + " with another joined vector")
        _equal(rec[d + " a, random again"], rec[d + " a again"], d + " with the first joined vector again")
        _equal(rec[d + " a, zeros"], rec[STATE_READER[d] + " a again"], d + " with nothing joined against the per-chunk entry point")
        assert _differ(rec[d + " a, zeros"], rec[d + " a again"]), d
    _check_mass_entries(store, rec["minlen_posterior_joined a, zeros"][0][1][2], rec["minlen_posterior_joined a, zeros"][0][1][3], "minlen_posterior_joined", FAMILY_ZEROS)
    for g in GETTERS:
        if g + " alone" in rec:
            _equal(rec[g + " after the decoders"], rec[g + " alone"], g)
            _equal(rec[g + " after the decoders again"], rec[g + " alone"], g)


# ---- c2. the arguments of generation 3 against the float64 references ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(decoder, which, min_len, n_samples, join):
    """The numpy reference of one decoder call on input "sizes" with model `which`, computed once."""
    store, _, _, alpha = _input("sizes")[:4]
    model = _model("sizes", which)
    if decoder == "viterbi_minlen":
        return minlen_ref.reference(store, model, alpha, min_len)
    if decoder == "viterbi_minlen_joined":
        return viterbi_ref.tables(store, model, alpha)           # (the feature's checker computes the reference from the tables)
    if decoder == "minlen_posterior":
        return minlen_post_ref.reference(store, model, alpha, min_len)
    assert decoder == "sample_minlen"
    return minlen_sample_ref.reference(store, model, alpha, min_len, SAMPLE_SEED, range(n_samples))


def _cycle_arguments(decoder, ordinal, generation=3):
    """What stream_sequences.decoder_arguments gives the call number `ordinal` of `decoder`."""
    return list(SQ.decoder_arguments([decoder] * (ordinal + 1), generation))[-1][1]


ANCHORS = [pytest.param(d, n, id="%s-%d" % (d, n)) for d in SQ.MINLEN_USERS for n in range(len(SQ.LENS_CYCLE))]


@pytest.mark.parametrize("decoder,ordinal", ANCHORS)
def test_generation_3_arguments_equal_the_references(decoder, ordinal):
    """Input "sizes", both models, a fresh context per call on a caller's busy stream: the arguments of the first five calls of a decoder
    in a generation-3 sequence (every entry of LENS_CYCLE and SAMPLE_CYCLE, every kind of join; no sequence of the committed seeds holds
    more than four calls of one decoder) against the float64 numpy references of the features' own device tests, with their checkers and
    tolerances (the sampler's near ties as tests/test_minlen_sample_gpu.py handles them).  test_mixed_orders compares every decoder
    call of a sequence bitwise with such a fresh context, so this ties the mixed-order results to the references.  The whole store is
    anchored: one reference on its 18 828 windows takes 1 to 3 s."""
    import time
    args = _cycle_arguments(decoder, ordinal)
    min_len = args["min_len"]
    store = _input("sizes")[0]
    with HS.Streams() as streams:
        side = Side("sizes", "scan-rows", [streams.new(True)])
        try:
            for which in "ab":
                t0 = time.perf_counter()
                ref = _reference(decoder, which, min_len, args.get("n_samples"), args.get("join"))
                t1 = time.perf_counter()
                em = side.context()
                code, got = side.decoder(em, decoder, _model("sizes", which), None, args, SQ.BUFFERS.get(decoder, ()))
                em.close()
                print("%s %s model %s: reference %.2f s, device call with its getters %.2f s" % (decoder, args, which, t1 - t0, time.perf_counter() - t1))
                assert code == N.HF_OK, (decoder, args, which, code)          # (the "all" join among them: no HF_E_SCALE on this input)
                if decoder == "viterbi_minlen":
                    TML._check(store, ref, min_len, (got[0], got[1], float(got[2])))
                elif decoder == "viterbi_minlen_joined":
                    TMJ._check(store.chunk_off, ref, SQ.join_vector(args["join"], store.n_chunks), min_len, (got[0], got[1], float(got[2])))
                elif decoder == "minlen_posterior":
                    TMP._check(store, ref, (got[0], got[1], got[2], got[3], float(got[4])), "%s model %s" % (min_len, which))
                else:
                    TMS._check(store, ref, got[0], min_len)
            print("%s %d: busy-stream checks on the anchors' fresh contexts: %s" % (decoder, ordinal, _busy_counts(side.busy)))
        finally:
            side.close()


@functools.lru_cache(maxsize=None)
def _sizes_tables(which):
    """(log tables, linear rows) of input "sizes" under model `which`, as the joined references take them."""
    store, _, _, alpha = _input("sizes")[:4]
    model = _model("sizes", which)
    return viterbi_ref.tables(store, model, alpha), sampling_ref.rows(store, model, alpha)


ANCHORS_4 = [pytest.param(d, n, w, id="%s-%d-%s" % (d, n, w)) for d in SQ.JOINED_DECODERS for n in range(len(SQ.LENS_CYCLE)) for w in "ab"]


@pytest.mark.parametrize("decoder,ordinal,which", ANCHORS_4)
def test_generation_4_arguments_equal_the_references(decoder, ordinal, which):
    """Input "sizes", both models, a fresh context per call on a caller's busy stream: the arguments of the first five calls of the two
    whole-contig entry points in a generation-4 sequence (every entry of LENS_CYCLE and JOINED_SAMPLE_CYCLE, the joins all, random,
    zeros, null, all) against the float64 numpy references of tests/test_minlen_sum_joined_gpu.py (minlen_sum_joined_ref.posterior_tables;
    sample_tables fed to minlen_sample_ref.sample), with that file's checkers at their tolerances.  Before a case is relied on, the
    reference itself is checked: Z_adm > 0 in every group (a finite log Z_adm), and no draw of the sampler's reference within 1e-9 of
    a boundary (_quiet_reference).  Both hold for every case here, the "all" join (one group of 18 828 windows) included, with log
    Z_adm between -57 959 and -39 578 and margins of 2.1e-7 and more.  One reference takes 1 to 2 s, so a case is one model."""
    import time
    args = _cycle_arguments(decoder, ordinal, 4)
    min_len = args["min_len"]
    store = _input("sizes")[0]
    off = store.chunk_off
    joined = SQ.join_vector(args["join"], store.n_chunks)
    (logA, logend), (A, end) = _sizes_tables(which)
    t0 = time.perf_counter()
    if decoder == "minlen_posterior_joined":
        ref = minlen_sum_joined_ref.posterior_tables(logA, logend, off, joined, min_len)
        gf = minlen_joined_ref.group_first_chunks(off, joined)
        assert np.all(np.isfinite(ref[2][gf])) and np.all(np.isfinite(ref[1][gf])), (args, ref[2][gf])       # Z_adm > 0 in every group
    else:
        ref = TSJ._quiet_reference(minlen_sample_ref.sample(minlen_sum_joined_ref.sample_tables(A, end, off, joined, min_len), SAMPLE_SEED,
                                                            range(args["n_samples"]), store.n_windows))
    t1 = time.perf_counter()
    with HS.Streams() as streams:
        side = Side("sizes", "scan-rows", [streams.new(True)])
        try:
            em = side.context()
            code, got = side.decoder(em, decoder, _model("sizes", which), None, args, _first_call_grows(decoder))
            em.close()
            print("%s %s model %s: reference %.2f s, device call with its getters %.2f s" % (decoder, args, which, t1 - t0, time.perf_counter() - t1))
            assert code == N.HF_OK, (decoder, args, which, code)
            if decoder == "minlen_posterior_joined":
                TSJ._check_post(store, joined, ref, (got[0], got[1], got[2], got[3], float(got[4])), "%s %s model %s" % (min_len, args["join"], which))
            else:
                TSJ._check_samples(off, joined, ref, got[0], min_len)
            print("%s %d: busy-stream checks on the anchor's fresh context: %s" % (decoder, ordinal, _busy_counts(side.busy)))
        finally:
            side.close()


# ---- d. mixed orders ----------------------------------------------------------------------------------------------------------------
def _mixed_scenario(side, seed, generation=1):
    """One sequence of tests/stream_sequences.py on a context; after every getter, the same getter on a FRESH context that ran only the last
    pass (with the switches as they stood then, and as they stand now for the getter).  At the end every decoder's stored results are
    read again: they are what that decoder returned at its last call in the sequence (hf_viterbi_minlen and hf_viterbi_minlen_joined
    share their state: what the later of the two returned; so do the two pairs of generation 4, and after the posterior's the chunk
    entries are checked as well: _check_mass_entries).  From generation 3 on the decoders' arguments change from call to call
    (stream_sequences.decoder_arguments), and after every decoder call the same call runs on a fresh context that has run nothing
    else: bitwise the same results and codes, whatever the context's buffers held from wider calls or the other entry point."""
    name = side.name
    scan = KINDS[side.kind][0] == N.HF_ALGO_SCAN
    base_mode = KINDS[side.kind][1]
    other_mode = {N.HF_STATS_ROWS: N.HF_STATS_CHUNKS, N.HF_STATS_CHUNKS: N.HF_STATS_ROWS}.get(base_mode)
    models = {"pass_a": _model(name, "a"), "pass_b": _model(name, "b")}
    em = side.context()
    rec, fresh_cache, last_decoded = {}, {}, {}
    last_model = "pass_a"

    def run_pass(ctx, op, which):
        if op == "forward":
            return side.estep(ctx, models[which], N.HF_MODE_FORWARD_ONLY)
        return side.estep(ctx, models[op])

    def fresh(op, st, which):
        key = (op, st["last_pass"], which if st["last_pass"] == "forward" else None, st["pass_alpha"], st["pass_flipped"], st["alpha"], st["flipped"],
               st["alpha_answers"])
        if key not in fresh_cache:
            f = side.context()
            if scan and st["pass_flipped"]:
                f.set_stats_mode(other_mode)
            if st["pass_alpha"]:
                _call(f.set_alpha_stats, True)
            if st["last_pass"]:
                run_pass(f, st["last_pass"], which)
            if scan and st["flipped"] != st["pass_flipped"]:
                f.set_stats_mode(other_mode if st["flipped"] else base_mode)
            if st["pass_alpha"] and not st["alpha_answers"]:                      # (switched off since the pass, and perhaps on again)
                _call(f.set_alpha_stats, False)
            if st["alpha"] != (st["pass_alpha"] and st["alpha_answers"]):
                _call(f.set_alpha_stats, st["alpha"])
            fresh_cache[key] = side.getter(f, op)
            f.close()
        return fresh_cache[key]

    def fresh_decoder(op, which, args):
        """The same decoder call on a context that has run nothing else: no pass, no other decoder, no earlier call of this one."""
        key = (op, which, args.get("min_len"), args.get("n_samples"), args.get("join"))
        if key not in fresh_decoders:
            f = side.context()
            before = collections.Counter(side.busy)
            fresh_decoders[key] = side.decoder(f, op, models[which], None, args, _first_call_grows(op))      # (a first call grows every buffer)
            fresh_busy.update(side.busy - before)             # (counted apart from the sequence's own calls)
            side.busy = before
            f.close()
        return fresh_decoders[key]

    fresh_decoders, compared, fresh_busy = {}, collections.Counter(), collections.Counter()
    ops = SQ.sequence(seed, generation)
    fwd_model = "pass_a"
    for i, ((op, st), (_, args, grows)) in enumerate(zip(SQ.replay(ops), SQ.decoder_arguments(ops, generation))):
        tag = "%02d %s" % (i, op)
        if op in ("pass_a", "pass_b"):
            rec[tag] = [run_pass(em, op, None)]
            last_model = op
        elif op == "forward":
            fwd_model = "pass_b" if last_model == "pass_a" else "pass_a"
            rec[tag] = [run_pass(em, op, fwd_model)]
            last_model = fwd_model
        elif op == "flip":
            if scan:
                em.set_stats_mode(base_mode if st["flipped"] else other_mode)
        elif op in ("alpha_on", "alpha_off"):
            rec[tag] = [_call(em.set_alpha_stats, op == "alpha_on")]
        elif op in SQ.ALL_DECODERS:
            which = "pass_b" if last_model == "pass_a" else "pass_a"                             # parameters other than the last pass's
            rec[tag] = [side.decoder(em, op, models[which], None, args, grows)]
            last_decoded[STATE_READER.get(op, op)] = (tag, op, args)                             # one record per shared state: the later call
            if generation >= 3 and side.stream:                                                   # (once: the twin equals this side)
                _equal(rec[tag], [fresh_decoder(op, which, args)], "%s %s against a fresh context" % (tag, args))
                assert _codes(rec[tag]) == [N.HF_OK], (tag, args, _codes(rec[tag]))
                compared[op] += 1
        else:
            got = side.getter(em, op)
            rec[tag] = got
            if side.stream:                                                                       # (once: the twin equals this side)
                _equal(got, fresh(op, st, fwd_model), "%s against a fresh context" % tag)
            if st["last_pass"] in (None, "forward"):
                assert all(c == N.HF_E_ARG for c in _codes(got)), (tag, _codes(got))
            elif op != "alpha_stats":
                assert all(c == N.HF_OK for c in _codes(got)), (tag, _codes(got))
            elif st["alpha_answers"] and side.mt != NB:
                assert _codes(got) == [N.HF_OK], (tag, _codes(got))
            else:
                assert _codes(got) == [N.HF_E_ARG], (tag, _codes(got))
    for key, (tag, op, args) in last_decoded.items():
        rec["stored " + key] = [side.stored(em, key)]
        _stored_equals(rec["stored " + key][0], rec[tag][0], "the stored results of %s at the end" % tag)
        if key == "viterbi_minlen":                          # the shared state answers to both getters' contracts, for the later call
            _check_chunk_entries(side.store, rec["stored " + key][0][1][1], op, args)
        if key == "minlen_posterior":
            _check_mass_entries(side.store, rec["stored " + key][0][1][2], rec["stored " + key][0][1][3], op, args)
    if generation >= 3 and side.stream:
        calls = collections.Counter(op for op in ops if op in SQ.ALL_DECODERS)
        assert compared == calls, (compared, calls)
        print("%s %s seed %d: decoder calls compared with a fresh context: %s; %d fresh contexts" % (name, side.kind, seed, dict(compared), len(fresh_decoders)))
        print("%s %s seed %d: busy-stream checks in the sequence: %s" % (name, side.kind, seed, _busy_counts(side.busy)))
        print("%s %s seed %d: busy-stream checks on the fresh contexts: %s" % (name, side.kind, seed, _busy_counts(fresh_busy)))
    return rec


def _busy_counts(counter):
    """Side.busy for printing: {"entry point, asserted | grow, busy | grow, idle": calls}."""
    return {"%s, %s" % k: v for k, v in sorted(counter.items())}


def _check_chunk_entries(store, chunk_ll, op, args):
    """The chunk scores the shared minimum-length state holds after a call of `op`: hf_viterbi_minlen leaves a score (a log-probability,
    never 0.0) in the entry of every chunk with windows; hf_viterbi_minlen_joined leaves one in the entry of every group's first chunk
    and exactly 0.0 in the entries of the group's other chunks."""
    T = np.diff(np.asarray(store.chunk_off, np.int64))
    first = np.zeros(T.size, bool)
    first[minlen_joined_ref.group_first_chunks(store.chunk_off, SQ.join_vector(args["join"], T.size) if op == "viterbi_minlen_joined" else None)] = True
    assert np.all(chunk_ll[~first] == 0.0) and not np.signbit(chunk_ll[~first]).any(), (op, args)
    assert np.all(chunk_ll[first & (T > 0)] != 0.0), (op, args)


def _check_mass_entries(store, log_mass, log_z_adm, op, args):
    """_check_chunk_entries' twin for hf_get_minlen_chunk_log_mass, the two arrays the posterior's shared state holds after a call of
    `op`: hf_minlen_posterior_joined leaves a group's values in the entry of its first chunk and exactly 0.0, without a sign bit, in
    the entries of the group's other chunks, in both arrays; hf_minlen_posterior leaves its values in the entry of every chunk, a
    chunk being a group of its own.  log Z_adm is not 0.0 wherever the group has windows (the log-probability of the data under the
    rule), so a per-chunk call leaves no entry of a chunk with windows at 0.0.  log_mass makes no such claim: it IS exactly 0.0 where
    the rule excludes nothing (one or two windows: a run that touches an end of the group is exempt) or less than half an ulp of Z
    (config2 under (61, 1, 1, 1): chunks without an Err window worth 1e-16 of their mass), and with all four lengths 1 it is exactly
    0.0 in every entry, the header's exact case; its entries are compared bitwise with a fresh context's instead."""
    goff, gf, _ = minlen_joined_ref.group_offsets(store.chunk_off, SQ.join_vector(args["join"], store.n_chunks) if op == "minlen_posterior_joined" else None)
    size = np.diff(goff)
    inner = np.ones(store.n_chunks, bool)
    inner[gf] = False
    for x in (log_mass, log_z_adm):
        assert np.all(x[inner] == 0.0) and not np.signbit(x[inner]).any(), (op, args)
    assert np.all(log_z_adm[gf[size > 0]] != 0.0), (op, args)
    if max(args["min_len"]) == 1:
        assert np.all(log_mass == 0.0) and not np.signbit(log_mass).any(), (op, args)


def _mixed_cases(generation, tag):
    seeds = SQ.GENERATIONS[generation][3]
    return [pytest.param("config2", k, generation, s, id="config2-%s-%sseed%d" % (k, tag, s)) for k in KINDS for s in seeds] + \
        [pytest.param(n, k, generation, seeds[i % len(seeds)], id="%s-%s-%sseed%d" % (n, k, tag, seeds[i % len(seeds)]))
         for i, (n, k) in enumerate((n, k) for n in ("sizes", "regions", "negative_binomial") for k in ("seq", "scan-rows", "scan-chunks-3-sub-passes"))]


# generation 1: the ten getters and two decoders its seeds were chosen with; generation 2: all thirteen getters and three decoders;
# generation 3: the thirteen getters and six decoders, the decoders' arguments changing from call to call; generation 4: all eight
# decoders, the two whole-contig entry points of the posterior and the sampler in the states of the per-chunk ones
MIXED = _mixed_cases(1, "") + _mixed_cases(2, "gen2-") + _mixed_cases(3, "gen3-") + _mixed_cases(4, "gen4-")


@pytest.mark.parametrize("name,kind,generation,seed", MIXED)
def test_mixed_orders(name, kind, generation, seed, monkeypatch):
    _run_both(name, kind, monkeypatch, lambda side: _mixed_scenario(side, seed, generation))


# ---- e. two contexts, two streams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", ON_CONFIG2 + [pytest.param("negative_binomial", "scan-rows", id="negative_binomial-scan-rows")])
def test_two_contexts_on_two_streams(name, kind, monkeypatch):
    """estep(a), estep(b), finish(b), finish(a), then getters alternating between the two: each context's results as if it ran alone."""
    def scenario(side):
        ma, mb = _model(name, "a"), _model(name, "b")
        s1, s2 = side.streams
        a, b = side.context(s1, alpha_stats=True), side.context(s2, alpha_stats=True)
        rec = {}
        side.delay(s1)
        ca, _ = _call(a.launch, ma)
        side.assert_busy(s1, "hf_estep")
        side.delay(s2)
        cb, _ = _call(b.launch, mb)
        side.assert_busy(s2, "hf_estep")
        rec["b pass"] = [(cb, ()), side.finish(b)]
        rec["a pass"] = [(ca, ()), side.finish(a)]
        for g in _getters_of(side):
            rec["a " + g] = side.getter(a, g)
            rec["b " + g] = side.getter(b, g)
        for g in reversed(_getters_of(side)):
            rec["b again " + g] = side.getter(b, g)
            rec["a again " + g] = side.getter(a, g)
        for w, m in (("a", ma), ("b", mb)):
            alone = side.context(s1, alpha_stats=True)
            rec[w + " alone pass"] = [(N.HF_OK, ()), side.estep(alone, m)]
            for g in _getters_of(side):
                rec[w + " alone " + g] = side.getter(alone, g)
            alone.close()
        return rec

    rec = _run_both(name, kind, monkeypatch, scenario, n_streams=2)
    assert all(c == N.HF_OK for calls in rec.values() for c in _codes(calls))
    for w in "ab":
        _equal(rec[w + " pass"], rec[w + " alone pass"], w)
        for g in GETTERS:
            if w + " " + g in rec:
                _equal(rec[w + " " + g], rec[w + " alone " + g], w + " " + g)
                _equal(rec[w + " again " + g], rec[w + " alone " + g], w + " again " + g)
    assert not np.array_equal(rec["a labels"][0][1][0], rec["b labels"][0][1][0])


# ---- f. the batch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stats_mode", [N.HF_STATS_ROWS, N.HF_STATS_CHUNKS], ids=["rows", "chunks"])
@pytest.mark.parametrize("name", ["config2", "regions"])
def test_batch_on_a_stream(name, stats_mode, monkeypatch):
    """EMBatch(..., stream=s) with three models: statistics, statuses, labels(m) and posterior(m) of the stream-0 batch; then a pass and
    getters on the underlying single context, and the batch's results are still there."""
    def scenario(side):
        store, mt, K, alpha, frac = side.store, side.mt, side.K, side.alpha, side.frac
        models = [_model(name, "a"), _model(name, "b"), hmm.createModel(mt, K, store, np.zeros((4, 4)))]
        em = hmm.EMList(store, models[0], True, frac, stream=side.stream)
        side.contexts.append(em)
        em.set_stats_mode(stats_mode)
        batch = hmm.EMBatch(em, models)
        assert (batch.stream.value or 0) == side.stream
        rec = {}
        try:
            for rnd in range(2):
                side.delay()
                act = batch.launch()
                side.assert_busy(side.stream, "hf_batch_estep")
                side.delay()
                stats, status = batch.finish(len(act))
                rec["batch pass %d" % rnd] = [(N.HF_OK, (stats.copy(), status.copy()))]
                assert (status == N.HF_OK).all()
                for m in range(3):
                    side.delay()
                    rec["batch labels %d.%d" % (rnd, m)] = [_call(batch.labels, m)]
                    side.delay()
                    rec["batch posterior %d.%d" % (rnd, m)] = [_call(batch.posterior, m)] + [_call(batch.posterior, m, a, c) for a, c in side.J.ranges[1:4]]
                if rnd == 0:
                    for i, m in enumerate(models):                       # other parameters for the second round
                        m.estimators = stats[i].copy()
                        hmm.HMM_estimateParameters(m, 1e-3)
                        hmm.HMM_resetEstimators(m)
            rec["single pass"] = [side.estep(em, _model(name, "b"))]
            rec["single posterior"] = side.getter(em, "posterior")
            rec["single interval_log_probs"] = side.getter(em, "interval_log_probs")
            side.delay()
            rec["batch labels after the single pass"] = [_call(batch.labels, 1)]
        finally:
            batch.close()
        return rec

    rec = _run_both(name, "scan-rows", monkeypatch, scenario)
    assert all(c == N.HF_OK for calls in rec.values() for c in _codes(calls))
    _equal(rec["batch labels after the single pass"], rec["batch labels 1.1"], "the batch's labels after a pass of the single context")
    assert not np.array_equal(rec["batch labels 0.1"][0][1][0], rec["batch labels 1.1"][0][1][0])


# ---- g. after a failed pass --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["seq", "scan-rows", "scan-chunks"])
def test_after_a_failed_pass(kind):
    """The negative-variance model of tests/test_estep_gpu.py::test_nan_emission_is_reported on a caller's stream: hf_finish and every
    getter return the twin's codes, and no getter answers HF_OK for a pass that failed."""
    store = synth.synthesize([400_000, 150_000], 1000, 200_000, [20], seed=3)
    K = 3
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
    v = model.param_vector()
    km = (v.size - 27) // 12
    v[27 + 4 * km + 2 * km] = -1.0           # variance of the Hap state
    model.set_param_vector(v)
    n = store.n_windows
    algo, mode, _ = KINDS[kind]
    h = HS.hip()
    recs = []
    with HS.Streams() as streams:
        for s in (streams.new(), 0):
            em = hmm.EMList(store, model, algo=algo, stream=s)
            try:
                if mode is not None:
                    em.set_stats_mode(mode)
                em.set_alpha_stats(True)
                rec = []
                h.delay(s)
                rec.append(_call(em.launch, model)[0])
                h.delay(s)
                rec.append(_call(em.finish)[0])
                F, L_, M = np.array([0, 5]), np.array([n - 1, 40]), np.array([15, 4])
                calls = {"labels": (em.labels,), "posterior": (em.posterior,), "forward_backward": (em.forward_backward,),
                         "interval_log_probs": (em.interval_log_probs, F, L_, M), "count_moments": (em.count_moments, F, L_, M),
                         "run_moments": (em.run_moments, F, L_, M), "path_entropy": (em.path_entropy, F, L_),
                         "path_log_probs": (em.path_log_probs, F, L_, np.full(n, 2, np.int8)), "entropy_profile": (em.entropy_profile,),
                         "alpha_stats": (em.alpha_stats,), "breakpoints": (em.breakpoints, F, np.array([3, 40]), 1, 4),
                         "breakpoint_profile": (em.breakpoint_profile, 5, 40, 1, 4), "long_run_log_probs": (em.long_run_log_probs, F, L_, M, 2)}
                assert sorted(calls) == sorted(GETTERS)
                for g in GETTERS:
                    h.delay(s)
                    rec.append(_call(*calls[g])[0])
                recs.append(rec)
            finally:
                em.close()
    got, twin = recs
    assert got == twin
    assert got[0] == N.HF_OK and got[1] == N.HF_E_NAN
    assert all(c != N.HF_OK for c in got[2:]), dict(zip(GETTERS, got[2:]))


def test_batch_after_a_failed_model():
    """A batch of a good model and the negative-variance one on a caller's stream: the bad model's status is HF_E_NAN and its getters
    return HF_E_ARG, the good model's labels and posterior are those of a batch without the bad one; all as on stream 0."""
    store = synth.synthesize([400_000, 150_000], 1000, 200_000, [20], seed=3)
    good = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, store, synth.HIFI_ALPHA)
    bad = good.copy()
    v = bad.param_vector()
    km = (v.size - 27) // 12
    v[27 + 4 * km + 2 * km] = -1.0           # variance of the Hap state
    bad.set_param_vector(v)
    h = HS.hip()
    recs = []
    with HS.Streams() as streams:
        for s in (streams.new(), 0):
            for models in ([good, bad], [good]):
                batch = hmm.EMBatch(store, models, stream=s)
                try:
                    h.delay(s)
                    act = batch.launch()
                    h.delay(s)
                    stats, status = batch.finish(len(act))
                    rec = [(N.HF_OK, (status.copy(), stats[0].copy()))]
                    for m in range(len(models)):
                        h.delay(s)
                        rec += [_call(batch.labels, m), _call(batch.posterior, m)]
                    recs.append(rec)
                finally:
                    batch.close()
                    batch.em.close()
    both, alone, both0, alone0 = recs
    _equal(both, both0, "good and bad model against stream 0")
    _equal(alone, alone0, "good model alone against stream 0")
    assert list(both[0][1][0]) == [N.HF_OK, N.HF_E_NAN]
    assert _codes(both[1:]) == [N.HF_OK, N.HF_OK, N.HF_E_ARG, N.HF_E_ARG]
    _equal(both[1:3], alone[1:3], "the good model beside a failing one")
    assert np.array_equal(both[0][1][1], alone[0][1][1])


# ---- h. PyTorch plumbing ---------------------------------------------------------------------------------------------------------------
def test_torch_stream():
    """A torch.cuda.Stream's handle, passed the way flagger_amd/dist.py passes the current stream's: in a fresh process that imports
    torch BEFORE the library, as a dist.py caller does (tests/torch_stream_child.py).  Skips only when that process reports that torch
    sees no GPU; torch and the library on two HIP runtime objects is a failure — the handle would mean nothing to the library."""
    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torch_stream_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=120)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(lines[0][len("RESULT "):])
    if res["status"] == "no gpu":
        pytest.skip("torch sees no GPU in a fresh process")
    assert res["status"] == "ok", res
    assert len(res["runtimes"]) == 1, res                 # torch and the library share one HIP runtime object
    assert res["busy_after_estep"] and res["codes_ok"] and res["equal"], res
    assert res["compared_arrays"] >= 4 and res["current_stream_is_the_handle"], res
