"""Test-side reference of maximum-expected-accuracy decoding under minimum run lengths (hf_get_mea_labels): float64 numpy, written from
the definition in include/hmm_flagger_hip.h, not from the kernel.

The posterior is posterior_ref.reference's, the rows of the pass are viterbi_ref.tables' (log A_t, -inf for 0).  `gain_rows` builds

    g_t(k)    = ((post_t[0] W[0][k] + post_t[1] W[1][k]) + post_t[2] W[2][k]) + post_t[3] W[3][k]
    gk_t(k)   = g_t(k) if post_t[k] > 0, else -inf
    G_t[p][k] = gk_t(k)                                    a chunk-first window (all four rows alike)
    G_t[p][k] = gk_t(k) if A_t[p][k] > 0, else -inf        every other window

and the decoder is minlen_ref.viterbi_minlen(G, zeros, block_off, min_len): that function is the generic (max, +) walk of the expanded
chain; its blocks are chunk offsets or group offsets (`group_off`).  `expected_gain` and `supported` evaluate any labelling,
`enumerate_block` goes through all 4^T labellings of a tiny block, `final_bed_rule` restates the relabel-to-Hap filter of the final BED
in windows."""
from __future__ import annotations

import functools

import numpy as np

from flagger_amd import _native as N
from flagger_amd import synth
import minlen_ref
import posterior_ref
import viterbi_ref

IDENTITY = np.eye(4)
ASYM = np.array([[1.0, 0.0, 0.25, 0.0],          # an asymmetric matrix with a negative entry: calling Hap on a Dup window costs
                 [0.0, 1.5, -0.5, 0.25],
                 [0.125, 0.0, 1.0, 0.0],
                 [0.0, 0.5, 0.0, 2.0]])


def gains(post, W):
    """g_t(k) in the definition's order of additions: [N][4]."""
    W = np.asarray(W, np.float64)
    p = np.asarray(post, np.float64)
    return ((p[:, 0:1] * W[0][None, :] + p[:, 1:2] * W[1][None, :]) + p[:, 2:3] * W[2][None, :]) + p[:, 3:4] * W[3][None, :]


def chunk_first(chunk_off, n):
    off = np.asarray(chunk_off, np.int64)
    first = np.zeros(n, bool)
    first[off[:-1][np.diff(off) > 0]] = True
    return first


def gain_rows(post, logA, chunk_off, W, support=True):
    """G [N][p][k] as defined; support=False leaves every -inf out (the decoder that ignores support)."""
    n = post.shape[0]
    g = gains(post, W)
    if not support:
        return np.repeat(g[:, None, :], 4, axis=1)
    gk = np.where(post > 0, g, -np.inf)
    G = np.repeat(gk[:, None, :], 4, axis=1)
    inner = ~chunk_first(chunk_off, n)
    G[inner] = np.where(logA[inner] > -np.inf, G[inner], -np.inf)
    return G


def group_off(chunk_off, joined):
    """The window ranges of the groups of hf_viterbi_minlen_joined, and every group's first chunk."""
    off = np.asarray(chunk_off, np.int64)
    C_ = off.size - 1
    goff, gchunk = [], []
    for c in range(C_):
        cont = c > 0 and joined is not None and bool(joined[c]) and off[c + 1] > off[c] and off[c] > off[c - 1]
        if not cont:
            gchunk.append(c)
            goff.append(off[c])
    goff.append(off[C_])
    return np.asarray(goff, np.int64), np.asarray(gchunk, np.int64)


def decode(G, block_off, min_len):
    """(labels, block scores) of the reference decoder."""
    nb = np.asarray(block_off).size - 1
    return minlen_ref.viterbi_minlen(G, np.zeros((nb, 4)), block_off, min_len)


def expected_gain(labels, post, W, block_off):
    """The sum over the windows of every block of g_t(l_t): float64[blocks]."""
    g = gains(post, W)
    off = np.asarray(block_off, np.int64)
    lab = np.asarray(labels, np.int64)
    val = g[np.arange(lab.size), lab]
    return np.array([val[off[b]:off[b + 1]].sum() for b in range(off.size - 1)])


def supported(labels, post, logA, chunk_off):
    """Per chunk: post_t[l_t] > 0 at every window and A_t[l_{t-1}][l_t] > 0 at every window that is not the chunk's first."""
    off = np.asarray(chunk_off, np.int64)
    lab = np.asarray(labels, np.int64)
    n = lab.size
    ok = post[np.arange(n), lab] > 0
    inner = np.flatnonzero(~chunk_first(off, n))
    ok[inner] &= logA[inner, lab[inner - 1], lab[inner]] > -np.inf
    return np.array([ok[off[c]:off[c + 1]].all() for c in range(off.size - 1)], bool)


def block_scores(chunk_scores_by_group, gchunk, n_chunks):
    """Group scores in the entries of the groups' first chunks, 0.0 elsewhere."""
    out = np.zeros(n_chunks)
    out[gchunk] = chunk_scores_by_group
    return out


def enumerate_block(G, t0, t1, min_len):
    """All 4^T labellings of the block of windows t0 .. t1 - 1 over the rows G: (best admissible supported labelling, its gain, the
    second best gain; None, -inf, -inf when there is none)."""
    T = t1 - t0
    m = np.asarray([int(v) for v in min_len])
    P = np.stack([a.ravel() for a in np.indices((4,) * T)], axis=1)          # [4^T][T]
    score = G[t0, 0, P[:, 0]].copy()
    bad = np.zeros(P.shape[0], bool)
    run = np.ones(P.shape[0], np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            score = score + G[t0 + t, P[:, t - 1], P[:, t]]
            change = P[:, t] != P[:, t - 1]
            bad |= change & (t - run > 0) & (run < m[P[:, t - 1]])           # a run that began behind window 0 and ends before the last
            run = np.where(change, 1, run + 1)
    score[bad] = -np.inf
    order = np.argsort(-score, kind="stable")
    best = score[order[0]]
    if not best > -np.inf:
        return None, -np.inf, -np.inf
    second = score[order[1]] if order.size > 1 else -np.inf
    return P[order[0]].astype(np.int8), float(best), float(second)


def final_bed_rule(post, chunk_off, joined, min_len):
    """Posterior argmax with every run, merged over joined chunks, shorter than its length in windows turned to Hap (2): the labels the
    final BED carries (hfio_write_final_bed).  One pass over the runs of the argmax, as the writer makes it."""
    lab = np.argmax(post, axis=1).astype(np.int8)
    goff, _ = group_off(chunk_off, joined)
    out = lab.copy()
    for g in range(goff.size - 1):
        a = int(goff[g])
        end = int(goff[g + 1])
        while a < end:
            b = a
            while b + 1 < end and lab[b + 1] == lab[a]:
                b += 1
            if b - a + 1 < int(min_len[lab[a]]):
                out[a:b + 1] = 2
            a = b + 1
    return out


@functools.lru_cache(maxsize=None)
def tiny(model_type, seed, hifi):
    """(store, model, alpha, post, logA) of one of minlen_ref.TINY_CASES: the store and model of minlen_ref.tiny_case (the same draws)
    without its 50-digit enumerations."""
    from test_bruteforce_cpu import _tiny_store
    from test_viterbi_cpu import perturbed_model
    rng = np.random.default_rng(900 + seed)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    regions = [20, 31] if seed % 2 == 0 else [25]
    store = _tiny_store(rng, minlen_ref.TINY_LENGTHS, regions)
    model = perturbed_model(store, model_type, 2 + seed % 3, alpha, rng)
    post = posterior_ref.reference(store, model, alpha)[0]
    logA, _ = viterbi_ref.tables(store, model, alpha)
    return store, model, alpha, post, logA


TINY_JOINED = np.array([0, 0, 0, 1, 0, 0, 1, 0], bool)      # groups of TINY_LENGTHS: 8 | 7 | 5+1 | 6 | 3+2 | 4  (at most 8 windows)
TINY_GAINS = [IDENTITY, ASYM]
