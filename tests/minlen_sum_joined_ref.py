"""Test-side reference of the posterior and the sampler under minimum run lengths over whole contigs (hf_minlen_posterior_joined,
hf_sample_paths_minlen_joined), written from the restatement in include/hmm_flagger_hip.h and built on what exists: the joined call on
(chunk list, joined) is the per-chunk call on the chunk list in which each group's first chunk holds the group's whole window range and
its other chunks hold no windows (`group_chunk_offsets`), with the row of every joined chunk-first window t replaced by

    J_t[p][s] = end_{c-1}[p] * first_c[s]

and `end` taken at the group's last window.  No rescaling is added at a joined boundary, here or on the device: J_t is the size of any
row.  The posterior: minlen_joined_ref.joined_tables (in logs, as the tables of viterbi_ref come) into
minlen_post_ref.forward_backward.  The sampler: the same row in the linear domain (`joined_rows`, one product per entry as on the
device) into minlen_sample_ref.tables / sample / path_prob; the final lane of a group draws with uniform index n_windows + its FIRST
chunk, which is what minlen_sample_ref.sample does on the group-as-chunk list.

`enumerate_group_sums` enumerates a tiny group from the 50-digit path weights of its chunks (minlen_ref.chunk_path_weights): the cross
product, summed over the concatenations that are admissible over the group and over all.  The chunk weights are taken as the exact
binary rationals they are and combined in integer arithmetic, so nothing is rounded after them."""
from __future__ import annotations

import functools
import itertools

import mpmath as mp
import numpy as np

from flagger_amd import _native as N
from test_bruteforce_cpu import Params
import minlen_joined_ref as JR
import minlen_post_ref as PR
import minlen_ref
import minlen_sample_ref as SR
import sampling_ref as S
import viterbi_ref

mp.mp.dps = 50
ONES = (1, 1, 1, 1)


def group_chunk_offsets(chunk_off, joined):
    """The groups as a chunk list, int64[C + 1]: the first chunk of a group holds the group's range, its other chunks are empty."""
    off = np.asarray(chunk_off, np.int64)
    C = off.size - 1
    goff, gf, gl = JR.group_offsets(off, joined)
    out = np.empty(C + 1, np.int64)
    out[C] = off[C]
    for g in range(gf.size):
        out[gf[g]] = goff[g]
        out[gf[g] + 1:gl[g] + 1] = goff[g + 1]
    return out


def _group_end(end, chunk_off, joined):
    """end per chunk of the group-as-chunk list: the last chunk's in the entry of the group's first chunk (the others are never read)."""
    _, gf, gl = JR.group_offsets(chunk_off, joined)
    out = np.array(end, copy=True)
    out[gf] = np.asarray(end)[gl]
    return out


def joined_rows(A, end, chunk_off, joined):
    """Linear domain: (A with J_t = end_{c-1}[p] * first_c[s] at the joined chunk-first windows, end per chunk of the group-as-chunk list,
    the group-as-chunk offsets)."""
    off = np.asarray(chunk_off, np.int64)
    _, gf, _ = JR.group_offsets(off, joined)
    out = np.array(A, copy=True)
    for c in sorted(set(range(off.size - 1)) - set(gf.tolist())):
        t = int(off[c])
        out[t] = np.asarray(end)[c - 1][:, None] * A[t, 0, :][None, :]
    return out, _group_end(end, off, joined), group_chunk_offsets(off, joined)


def forward_backward(logA, logend, chunk_off, joined, min_len):
    """(post [N][4], log Z_adm [C]) in the getter's convention: a group's value in the entry of its first chunk, 0.0 in the others."""
    A, _, _, _ = JR.joined_tables(logA, logend, chunk_off, joined)
    return PR.forward_backward(A, _group_end(logend, chunk_off, joined), group_chunk_offsets(chunk_off, joined), min_len)


def posterior_tables(logA, logend, chunk_off, joined, min_len):
    """(post [N][4], log_mass [C], log Z_adm [C], log Z [C]) from the log tables of viterbi_ref.tables."""
    post, lza = forward_backward(logA, logend, chunk_off, joined, min_len)
    _, lz = forward_backward(logA, logend, chunk_off, joined, ONES)
    return post, lza - lz, lza, lz


def posterior(store, model, alpha, joined, min_len):
    logA, logend = viterbi_ref.tables(store, model, alpha)
    return posterior_tables(logA, logend, store.chunk_off, joined, min_len)


def sample_tables(A, end, chunk_off, joined, min_len):
    """minlen_sample_ref.tables of the joined call (linear rows A, end as sampling_ref.rows gives them)."""
    Aj, endj, goff = joined_rows(A, end, chunk_off, joined)
    return SR.tables(Aj, endj, goff, min_len)


def sample(store, model, alpha, joined, min_len, seed, ks):
    """(labels, window margins, final margins [K][C]) of the whole store; the margins of a group's final lane in its first chunk's entry."""
    A, end = S.rows(store, model, alpha)
    return SR.sample(sample_tables(A, end, store.chunk_off, joined, min_len), seed, ks, store.n_windows)


def admissible_over_groups(labels, chunk_off, joined, min_len):
    """The integer check of one label row: no run inside a group is shorter than its label's minimum."""
    goff = JR.group_offsets(chunk_off, joined)[0]
    return JR.short_inner_runs(labels, goff, min_len) == []


# ---- enumeration ---------------------------------------------------------------------------------------------------------------

def _as_ints(weights):
    """[(path, integer)] and the exponent e with weight = integer * 2^e, exactly (an mpf is a binary rational)."""
    parts = []
    for path, w in weights:
        sign, man, exp, _ = mp.mpf(w)._mpf_
        assert sign == 0
        parts.append((path, int(man), int(exp)))
    lo = min(e for _, m, e in parts if m) if any(m for _, m, _ in parts) else 0
    return [(path, m << (e - lo) if m else 0) for path, m, e in parts], lo


def enumerate_group_sums(chunk_weights, min_len, with_paths=False):
    """(log Z_adm, log Z, marginals mpf[T][4] given admissibility over the group, {path: probability} of the admissible paths or None)
    of the group whose chunks have the [(path, weight)] lists `chunk_weights`."""
    m = [int(v) for v in min_len]
    ints, shift = zip(*[_as_ints(w) for w in chunk_weights])
    T = sum(len(w[0][0]) for w in chunk_weights)
    marg = [[0] * 4 for _ in range(T)]
    za = z = 0
    paths = {} if with_paths else None
    ok = minlen_ref._path_ok
    for combo in itertools.product(*ints):
        w = 1
        for _, wi in combo:
            w *= wi
        z += w
        if w == 0:
            continue
        path = tuple(itertools.chain.from_iterable(p for p, _ in combo))
        if not ok(path, m):
            continue
        za += w
        for t, s in enumerate(path):
            marg[t][s] += w
        if with_paths:
            paths[path] = w
    scale = mp.mpf(sum(shift)) * mp.log(2)
    f = lambda v: mp.mpf(v) / mp.mpf(za)
    return (mp.log(mp.mpf(za)) + scale, mp.log(mp.mpf(z)) + scale, [[f(v) for v in row] for row in marg],
            {p: f(v) for p, v in paths.items()} if with_paths else None)


@functools.lru_cache(maxsize=None)
def tiny_chunk_weights(model_type, seed, hifi):
    """{chunk: [(path, weight)]} for the chunks of minlen_joined_ref.TINY_JOINS' groups of more than one chunk."""
    store, model, alpha, _ = minlen_ref.tiny_case(model_type, seed, hifi)
    regions = model.numberOfRegions
    P = Params(model.param_vector(), regions, 2 + seed % 3, model_type, alpha)
    nbE = None
    if model_type == N.HF_MODEL_NEGATIVE_BINOMIAL:
        p = model.params()
        nbE = np.ctypeslib.as_array(p.nb_E, shape=(regions * 4 * viterbi_ref.NX,)).reshape(regions, 4, viterbi_ref.NX).copy()
    out = {}
    for joined in JR.TINY_JOINS:
        _, gf, gl = JR.group_offsets(store.chunk_off, joined)
        for a, b in zip(gf, gl):
            for c in range(int(a), int(b) + 1):
                if a != b and c not in out:
                    out[c] = minlen_ref.chunk_path_weights(store, c, P, model, nbE)
    return out


@functools.lru_cache(maxsize=None)
def tiny_groups(model_type, seed, hifi):
    """{(joined, min_len): [(first chunk, last chunk, log Z_adm, log Z, marginals, path distribution or None)]} of the groups of more
    than one chunk of a tiny case (5, 6, 7 and 9 windows); the path distribution for the groups of at most 7 windows and, under lengths
    that are not all 1, for every group."""
    store = minlen_ref.tiny_case(model_type, seed, hifi)[0]
    w = tiny_chunk_weights(model_type, seed, hifi)
    out = {}
    for joined in JR.TINY_JOINS:
        goff, gf, gl = JR.group_offsets(store.chunk_off, joined)
        for ml in minlen_ref.TINY_MIN_LENS:
            res = []
            for g in range(gf.size):
                a, b = int(gf[g]), int(gl[g])
                if a == b:
                    continue
                n = int(goff[g + 1] - goff[g])
                assert n <= JR.MAX_ENUMERATED
                res.append((a, b) + enumerate_group_sums([w[c] for c in range(a, b + 1)], ml, with_paths=n <= 7 or ml != ONES))
            out[(joined, ml)] = res
    return out


def check_against_enumeration(store, case, joined, min_len, post, log_mass, log_z_adm, post_rel=0.0):
    """The multi-chunk groups of `joined` against tiny_groups, at minlen_post_ref.check_against_enumeration's tolerances: log_mass and
    log Z_adm within 1e-12 (1 + |log Z|), post within 1e-12 absolute (+ post_rel relative).  Returns (groups checked, groups whose mass is
    below the product of their chunks' per-chunk masses by more than 1e-6)."""
    off = np.asarray(store.chunk_off, np.int64)
    checked = 0
    for a, b, lza, lz, marg, _ in tiny_groups(*case)[(tuple(joined), tuple(min_len))]:
        tol = 1e-12 * (1 + abs(float(lz)))
        assert abs(log_mass[a] - float(lza - lz)) <= tol, (joined, min_len, a, log_mass[a], float(lza - lz))
        assert abs(log_z_adm[a] - float(lza)) <= tol, (joined, min_len, a, log_z_adm[a], float(lza))
        assert np.all(np.asarray(log_mass)[a + 1:b + 1] == 0.0) and np.all(np.asarray(log_z_adm)[a + 1:b + 1] == 0.0)
        ref = np.array([[float(v) for v in row] for row in marg])
        got = post[off[a]:off[b + 1]]
        assert np.all(np.abs(got - ref) <= 1e-12 + post_rel * ref), (joined, min_len, a, float(np.max(np.abs(got - ref))))
        checked += 1
    return checked
