"""Test-side reference of the minimum-run-length Viterbi decoder over whole contigs (hf_viterbi_minlen_joined), written from the
definition in include/hmm_flagger_hip.h and built on what exists: the joined decoder on (chunk list, joined) is
minlen_ref.viterbi_minlen on the chunk list whose chunks are the GROUPS, with the row of every joined chunk-first window t replaced by

    J_t[p][s] = log end_{c-1}[p] + log first_c[s]

and `end` taken from the group's last chunk.  A group is a maximal sequence of chunks joined to each other; a chunk without windows
ends a group whatever its own entry and its successor's entry say.  Scores follow the chunk getter's convention: the group's score in
the entry of the group's first chunk, exactly 0.0 in the others.

`enumerate_group` enumerates a tiny group in 50 digits as the cross product of minlen_ref.chunk_path_weights of its chunks, filtered by
admissibility of the concatenation; `tiny_groups` does it once per process for the join patterns the CPU and the GPU test share."""
from __future__ import annotations

import functools

import mpmath as mp
import numpy as np

from test_bruteforce_cpu import Params
import minlen_ref
import viterbi_ref

mp.mp.dps = 50


def group_first_chunks(chunk_off, joined):
    """The first chunk of every group (a chunk without windows is a group of its own)."""
    off = np.asarray(chunk_off, np.int64)
    C = off.size - 1
    j = np.zeros(C, bool) if joined is None else np.asarray(joined).ravel() != 0
    assert j.size == C and (C == 0 or not j[0])
    T = np.diff(off)
    return np.array([c for c in range(C) if not (c > 0 and j[c] and T[c] > 0 and T[c - 1] > 0)], np.int64)


def group_offsets(chunk_off, joined):
    """(group window offsets [G + 1], first chunk of every group [G], last chunk of every group [G])."""
    off = np.asarray(chunk_off, np.int64)
    gf = group_first_chunks(off, joined)
    gl = np.concatenate([gf[1:], [off.size - 1]]).astype(np.int64) - 1
    return np.concatenate([off[gf], off[-1:]]), gf, gl


def joined_tables(logA, logend, chunk_off, joined):
    """(logA with J_t at the joined chunk-first windows, log end per group, group offsets, first chunk per group)."""
    off = np.asarray(chunk_off, np.int64)
    goff, gf, gl = group_offsets(off, joined)
    A = np.array(logA, copy=True)
    inner = sorted(set(range(off.size - 1)) - set(gf.tolist()))
    for c in inner:                                         # (every one of them has windows, and so has its predecessor)
        t = int(off[c])
        A[t] = logend[c - 1][:, None] + logA[t, 0, :][None, :]
    return A, np.asarray(logend)[gl], goff, gf


def viterbi_minlen_joined(logA, logend, chunk_off, joined, min_len):
    """(labels int8[N], chunk scores float64[C] in the getter's convention, group offsets)."""
    A, gend, goff, gf = joined_tables(logA, logend, chunk_off, joined)
    labels, gscore = minlen_ref.viterbi_minlen(A, gend, goff, min_len)
    score = np.zeros(np.asarray(chunk_off).size - 1)
    score[gf] = gscore
    return labels, score, goff


def group_sums(per_chunk, chunk_off, joined):
    """Per-chunk values summed over every group, in the getter's convention (the sum in the first chunk's entry, 0.0 elsewhere)."""
    gf = group_first_chunks(chunk_off, joined)
    out = np.zeros(len(per_chunk))
    ends = np.concatenate([gf[1:], [len(per_chunk)]])
    for a, b in zip(gf, ends):
        out[a] = float(np.sum(np.asarray(per_chunk)[a:b]))
    return out


def short_inner_runs(labels, goff, min_len):
    """Maximal runs that touch neither end of their group and are shorter than their label's minimum: [(first, last, label)]."""
    m = [int(v) for v in min_len]
    lab = np.asarray(labels)
    out = []
    for g in range(len(goff) - 1):
        t0, t1 = int(goff[g]), int(goff[g + 1])
        a = t0
        while a < t1:
            b = a
            while b + 1 < t1 and lab[b + 1] == lab[a]:
                b += 1
            if a > t0 and b < t1 - 1 and b - a + 1 < m[int(lab[a])]:
                out.append((a, b, int(lab[a])))
            a = b + 1
    return out


# ---- enumeration ---------------------------------------------------------------------------------------------------------------

def enumerate_group(chunk_weights, min_len):
    """(best admissible path of the group, log of its weight, log of the second-best admissible weight): the cross product of the
    chunks' [(path, weight)] lists, filtered by admissibility of the concatenation."""
    m = [int(v) for v in min_len]
    combos = chunk_weights[0]
    for w in chunk_weights[1:-1]:
        combos = [(pa + pb, wa * wb) for pa, wa in combos for pb, wb in w]
    last = chunk_weights[-1] if len(chunk_weights) > 1 else [((), mp.mpf(1))]
    best, second, arg = mp.mpf(0), mp.mpf(0), None
    ok = minlen_ref._path_ok
    for pa, wa in combos:
        for pb, wb in last:
            path = pa + pb
            if not ok(path, m):
                continue
            w = wa * wb
            if w > best:
                best, second, arg = w, best, path
            elif w > second:
                second = w
    return arg, mp.log(best), (mp.log(second) if second > 0 else mp.mpf("-inf"))


# the tiny stores' chunk lengths are 8, 7, 5, 1, 6, 3, 2, 4: groups of 6 (5 + 1) and 5 (3 + 2) windows; of 7 (1 + 6) and 9 (3 + 2 + 4)
# windows, the latter with a middle chunk shorter than a minimum
TINY_JOINS = [(0, 0, 0, 1, 0, 0, 1, 0), (0, 0, 0, 0, 1, 0, 1, 1)]
MAX_ENUMERATED = 9


@functools.lru_cache(maxsize=None)
def tiny_groups(model_type, seed, hifi):
    """{(joined, min_len): [(first chunk, last chunk, path, log best, log second) per group of more than one chunk]} of a tiny case of
    minlen_ref.tiny_case; the groups of one chunk are that module's own enumeration."""
    store, model, alpha, _ = minlen_ref.tiny_case(model_type, seed, hifi)
    regions = model.numberOfRegions
    K = 2 + seed % 3
    P = Params(model.param_vector(), regions, K, model_type, alpha)
    nbE = None
    from flagger_amd import _native as N
    if model_type == N.HF_MODEL_NEGATIVE_BINOMIAL:
        p = model.params()
        nbE = np.ctypeslib.as_array(p.nb_E, shape=(regions * 4 * viterbi_ref.NX,)).reshape(regions, 4, viterbi_ref.NX).copy()
    weights = {}
    out = {}
    for joined in TINY_JOINS:
        goff, gf, gl = group_offsets(store.chunk_off, joined)
        for ml in minlen_ref.TINY_MIN_LENS:
            res = []
            for g in range(gf.size):
                a, b = int(gf[g]), int(gl[g])
                if a == b:
                    continue
                assert goff[g + 1] - goff[g] <= MAX_ENUMERATED
                for c in range(a, b + 1):
                    if c not in weights:
                        weights[c] = minlen_ref.chunk_path_weights(store, c, P, model, nbE)
                res.append((a, b) + enumerate_group([weights[c] for c in range(a, b + 1)], ml))
            out[(joined, ml)] = res
    return out
