"""Test-side reference of the E-step under minimum run lengths over groups of joined chunks (hf_estep_minlen_joined), built on what
exists: the joined call on (chunk list, joined) is hf_estep_minlen's definition on the group-as-chunk list, with the row of every
joined chunk-first window t replaced by J_t[p][s] = end_{c-1}[p] * first_c[s] and `end` taken at the group's last window
(minlen_sum_joined_ref.joined_rows), so the pair posterior is minlen_em_ref.xi_adm on those rows and offsets; the statistics are
minlen_em_ref.accumulate over the ORIGINAL chunk list (the pairs (w-1, w), w = 2..T_c-1 of each chunk: no boundary pair) with that xi.
A group's log Z_adm and log Z sit in the entry of its first chunk, 0.0 in its other chunks.

    xi_adm(A, end, chunk_off, joined, min_len)   -> xi [N][4][4] (zeros at a group's first window), post [N][4], log Z_adm [C]
    stats(store, model, alpha, joined, min_len)  -> dict as minlen_em_ref.stats, and "bound": the joined chunk-first windows
    enumerate_group_pairs(chunk_weights, min_len) -> mpf [T][4][4]: the pair marginals of a tiny group given admissibility over the
                                                    group, the boundary pairs included, by enumeration"""
from __future__ import annotations

import itertools

import mpmath as mp
import numpy as np

import minlen_em_ref as E
import minlen_joined_ref as JR
import minlen_ref
import minlen_sum_joined_ref as R
import sampling_ref

ONES = (1, 1, 1, 1)


def boundary_windows(chunk_off, joined):
    """The joined chunk-first windows: the first window of every chunk that is not the first of its group."""
    off = np.asarray(chunk_off, np.int64)
    first = set(JR.group_first_chunks(off, joined).tolist())
    return np.array([int(off[c]) for c in range(off.size - 1) if c not in first and off[c + 1] > off[c]], np.int64)


def xi_adm(A, end, chunk_off, joined, min_len):
    Aj, endj, goff = R.joined_rows(A, end, chunk_off, joined)
    return E.xi_adm(Aj, endj, goff, min_len)


def stats(store, model, alpha, joined, min_len, K_ctx=None, adjust=True, min_frac=0.95):
    A, end = sampling_ref.rows(store, model, alpha, adjust, min_frac)
    Aj, endj, goff = R.joined_rows(A, end, store.chunk_off, joined)
    xi, post, lza = E.xi_adm(Aj, endj, goff, min_len)
    _, _, lz = E.lanes_fb(Aj, endj, goff, ONES)
    vec, mag, chunk = E.accumulate(store, model, alpha, xi, lza, K_ctx, adjust, min_frac)
    return {"vec": vec, "mag": mag, "chunk": chunk, "xi": xi, "post": post, "lza": lza, "lz": lz,
            "bound": boundary_windows(store.chunk_off, joined)}


def enumerate_group_pairs(chunk_weights, min_len):
    """Pair marginals mpf[T][4][4] of the group whose chunks have the [(path, weight)] lists `chunk_weights` (row 0: zeros).  A group
    path's weight is the product of its chunks' weights, which is the chain with J = end * first at the boundaries."""
    m = [int(v) for v in min_len]
    T = sum(len(w[0][0]) for w in chunk_weights)
    ints = [R._as_ints(w)[0] for w in chunk_weights]       # exact integers: the common power of two cancels in the ratio
    pair = [[[0] * 4 for _ in range(4)] for _ in range(T)]
    za = 0
    for combo in itertools.product(*ints):
        w = 1
        for _, wi in combo:
            w *= wi
        if w == 0:
            continue
        path = tuple(itertools.chain.from_iterable(p for p, _ in combo))
        if not minlen_ref._path_ok(path, m):
            continue
        za += w
        for t in range(1, T):
            pair[t][path[t - 1]][path[t]] += w
    return [[[mp.mpf(v) / mp.mpf(za) for v in row] for row in mat] for mat in pair]
