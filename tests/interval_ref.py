"""Test-side reference of the exact interval probabilities (hf_get_interval_log_probs): float64 numpy, written from the definition of
include/hmm_flagger_hip.h and not from the kernels.

A job is a window range first..last (global, inclusive) and a state mask S (bit s = state s).  Chunks are independent chains with the
first / A / end of viterbi_ref.tables (sampling_ref.rows in linear scale), so

    log_p = sum over the chunks c the range meets of  log Z_S(c) - log Z(c)

where Z(c) is the chunk's total weight and Z_S(c) the weight of the paths whose windows of [a, b] = the range cut to chunk c are all in S.
Both come out of one scaled forward over the WHOLE chunk in which the columns outside S are zeroed on [a, b] (all columns kept for Z):
another formulation than the device's f_a . M_S . b_b."""
from __future__ import annotations

import numpy as np


def split(chunk_off, first, last, mask):
    """The chunk-local parts of jobs: (job, chunk, a, b, mask) arrays, chunk order inside a job."""
    off = np.asarray(chunk_off, np.int64)
    J, Cc, A_, B_, M_ = [], [], [], [], []
    for j, (f, l, m) in enumerate(zip(np.asarray(first, np.int64), np.asarray(last, np.int64), np.asarray(mask, np.int64))):
        c = int(np.searchsorted(off, f, side="right") - 1)
        a = int(f)
        while a <= l:
            while off[c + 1] <= a:
                c += 1
            b = min(int(l), int(off[c + 1]) - 1)
            J.append(j); Cc.append(c); A_.append(a); B_.append(b); M_.append(int(m))
            a = b + 1
    return tuple(np.asarray(x, np.int64) for x in (J, Cc, A_, B_, M_))


def restricted_log_z(A, end, chunk_off, pc, pa, pb, pm):
    """log of the weight of chunk pc[m]'s paths whose windows pa[m]..pb[m] are in the state set pm[m] (vectorised over m; chunks side by
    side, local window index in lockstep; the forward vector renormalised to sum 1 after every window)."""
    off = np.asarray(chunk_off, np.int64)
    pc = np.asarray(pc, np.int64)
    t0 = off[pc]
    T = off[pc + 1] - t0
    m = pc.size
    inS = ((np.asarray(pm, np.int64)[:, None] >> np.arange(4)) & 1).astype(np.float64)
    logz = np.zeros(m)
    if m == 0:
        return logz
    v = np.zeros((m, 4))
    for k in range(int(T.max())):
        act = np.flatnonzero(T > k)
        idx = t0[act] + k
        if k == 0:
            w = A[idx, 0, :].copy()                                   # first[s] in row 0 of the chunk-first window's row
        else:
            w = np.einsum("mp,mps->ms", v[act], A[idx])
        inside = (pa[act] <= idx) & (idx <= pb[act])
        w = w * np.where(inside[:, None], inS[act], 1.0)
        s = w.sum(axis=1)
        pos = s > 0
        with np.errstate(divide="ignore"):
            logz[act] += np.where(pos, np.log(np.where(pos, s, 1.0)), -np.inf)
        v[act] = np.where(pos[:, None], w / np.where(pos, s, 1.0)[:, None], 0.0)
    z = (v * end[pc]).sum(axis=1)
    with np.errstate(divide="ignore"):
        logz += np.where(z > 0, np.log(np.where(z > 0, z, 1.0)), -np.inf)
    return logz


def log_probs(A, end, chunk_off, first, last, mask):
    """float64[n]: log P(s_t in mask[i] for every t in first[i]..last[i] | data)."""
    n = np.asarray(first).size
    J, Cc, pa, pb, pm = split(chunk_off, first, last, mask)
    if J.size == 0:
        return np.zeros(n)
    zs = restricted_log_z(A, end, chunk_off, Cc, pa, pb, pm)
    uc = np.unique(Cc)
    z_all = np.zeros(int(np.max(Cc)) + 1)
    z_all[uc] = restricted_log_z(A, end, chunk_off, uc, np.zeros(uc.size, np.int64), np.zeros(uc.size, np.int64) - 1,
                                 np.full(uc.size, 15))
    part = zs - z_all[Cc]
    out = np.zeros(n)
    for j, v in zip(J, part):          # chunk order
        out[j] += v
    return out


def brute_force(A, end, chunk_off, first, last, mask):
    """The same by enumeration of every path of every chunk the range meets (4^T paths: tiny chunks only)."""
    import itertools
    off = np.asarray(chunk_off, np.int64)
    out = []
    for f, l, m in zip(first, last, mask):
        J, Cc, pa, pb, pm = split(off, [f], [l], [m])
        tot = 0.0
        for c, a, b in zip(Cc, pa, pb):
            t0, T = int(off[c]), int(off[c + 1] - off[c])
            paths = np.array(list(itertools.product(range(4), repeat=T)), np.int64)
            w = A[t0, 0, paths[:, 0]].copy()
            for t in range(1, T):
                w *= A[t0 + t, paths[:, t - 1], paths[:, t]]
            w *= end[c][paths[:, -1]]
            ok = np.all(((int(m) >> paths[:, a - t0:b - t0 + 1]) & 1) == 1, axis=1)
            ps = w[ok].sum() / w.sum()
            tot += np.log(ps) if ps > 0 else -np.inf
        out.append(tot)
    return np.array(out)
