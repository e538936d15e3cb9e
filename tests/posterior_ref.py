"""Test-side reference of the posterior getters (hf_get_posterior, hf_multi_get_posterior, hf_batch_get_posterior) and of the `trans`
block of the statistics: float64 numpy, written from the definitions (tests/test_bruteforce_cpu.py states them in
path-sum form), not from the kernels and not from the oracle's C.

A chunk is an independent chain with the weights of viterbi_ref.tables in linear scale:

    w(path) = first[s_0] * prod_{t >= 1} A_t[s_{t-1}][s_t]            Z  = sum_paths w             (the log-likelihood is log Z)
    we(path) = w(path) * end[s_{T-1}]                                  Ze = sum_paths we

    posterior of window t     post_t[s]      = sum_{paths, s_t = s} we / Ze
    pair count (t, t+1)       xi_t[pre][s]   = sum_{paths, s_t = pre, s_{t+1} = s} we / (Z * TERMINATION)

The pair counts carry the reference's own normalisation (by Z, not Ze, and by the termination probability: every row of the transition
matrix ends with 1e-4, so a pair's sixteen counts sum to 1); the statistics add them for t = 1 .. T-2 (the pair of the first two windows is
left out) under the region of window t+1.

Method: per chunk a forward pass whose vector is renormalised to sum 1 after every window (c_t the divisor), a backward pass from `end`
scaled by the same c_t, post = f*b / sum_s f*b, xi_t = f_t[pre] A_{t+1}[pre][s] b_{t+1}[s] / c_{t+1} * (1 / TERMINATION) — with that scaling
sum_s f_t[s] b_t[s] = Ze / Z for every t, which is the pair counts' normalisation.  All chunks run side by side, the local window index in
lockstep."""
from __future__ import annotations

import itertools

import numpy as np

import viterbi_ref

TERMINATION = 1e-4          # the End column of every transition row (hmm_utils.c:2112)


def rows(store, model, alpha, adjust=True, min_frac=0.95):
    """(A [N][pre][s] with first[s] in row 0 of every chunk-first window, end [C][4]) in linear scale."""
    logA, logend = viterbi_ref.tables(store, model, alpha, adjust, min_frac)
    return np.exp(logA), np.exp(logend)


def regions_of(store):
    return (np.asarray(store.annot, np.uint64) >> np.uint64(58)).astype(np.int64)


def forward_backward(A, end, chunk_off, reg=None, n_regions=1):
    """(post [N][4], xi [C][n_regions][4][4], chunk log-likelihoods [C]): the posterior of every window and every chunk's pair counts by
    region (see the module text); `reg`: region of every window (default: all 0)."""
    off = np.asarray(chunk_off, np.int64)
    T = np.diff(off)
    C_, n = T.size, int(off[-1])
    reg = np.zeros(n, np.int64) if reg is None else np.asarray(reg, np.int64)
    post = np.zeros((n, 4))
    xi = np.zeros((C_, n_regions, 4, 4))
    ll = np.zeros(C_)
    if n == 0:
        return post, xi, ll
    f = np.zeros((n, 4))
    cdiv = np.ones(n)
    live = np.flatnonzero(T > 0)
    Tmax = int(T.max())
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        v = None
        for k in range(Tmax):
            act = live[T[live] > k]
            idx = off[act] + k
            if k == 0:
                w = A[idx, 0, :].copy()
            else:
                w = np.einsum("mp,mps->ms", f[idx - 1], A[idx])
            c = w.sum(axis=1)
            f[idx] = w / c[:, None]
            cdiv[idx] = c
            ll[act] += np.log(c)
        b = np.zeros((n, 4))
        last = off[live + 1] - 1
        b[last] = end[live]
        for k in range(Tmax - 2, -1, -1):
            act = live[T[live] > k + 1]
            idx = off[act] + k                              # window t; t+1 exists
            bn = b[idx + 1] / cdiv[idx + 1][:, None]
            b[idx] = np.einsum("mps,ms->mp", A[idx + 1], bn)
            if k >= 1:                                      # pairs (t, t+1), t = 1 .. T-2, under the region of window t+1
                x = f[idx][:, :, None] * A[idx + 1] * bn[:, None, :] / TERMINATION
                np.add.at(xi, (act, reg[idx + 1]), x)
        fb = f * b
        post = fb / fb.sum(axis=1, keepdims=True)
    return post, xi, ll


def reference(store, model, alpha, adjust=True, min_frac=0.95):
    """(post [N][4], trans [n_regions][4][4] summed over the chunks in list order, xi [C][n_regions][4][4], chunk log-likelihoods)."""
    A, end = rows(store, model, alpha, adjust, min_frac)
    post, xi, ll = forward_backward(A, end, store.chunk_off, regions_of(store), model.numberOfRegions)
    return post, xi.sum(axis=0), xi, ll


def brute_force(A, end, chunk_off, reg=None, n_regions=1):
    """The same three results by enumeration of every path of every chunk (4^T paths: tiny chunks only)."""
    off = np.asarray(chunk_off, np.int64)
    n = int(off[-1])
    reg = np.zeros(n, np.int64) if reg is None else np.asarray(reg, np.int64)
    post = np.zeros((n, 4))
    xi = np.zeros((off.size - 1, n_regions, 4, 4))
    ll = np.zeros(off.size - 1)
    for c in range(off.size - 1):
        t0, T = int(off[c]), int(off[c + 1] - off[c])
        if T == 0:
            continue
        paths = np.array(list(itertools.product(range(4), repeat=T)), np.int64)
        w = A[t0, 0, paths[:, 0]].copy()
        for t in range(1, T):
            w *= A[t0 + t, paths[:, t - 1], paths[:, t]]
        Z = w.sum()
        we = w * end[c][paths[:, -1]]
        ll[c] = np.log(Z)
        for t in range(T):
            for s in range(4):
                post[t0 + t, s] = we[paths[:, t] == s].sum() / we.sum()
        for t in range(1, T - 1):
            for pre in range(4):
                for s in range(4):
                    xi[c, reg[t0 + t + 1], pre, s] += we[(paths[:, t] == pre) & (paths[:, t + 1] == s)].sum() / Z / TERMINATION
    return post, xi, ll


def trans_block(stats, n_regions, K):
    """The `trans` block [n_regions][4][4] of a statistics vector (include/hmm_flagger_hip.h: 24 K + 16 doubles per region behind the
    log-likelihood, the sixteen pair counts last)."""
    st = 24 * K + 16
    v = np.asarray(stats, np.float64)[1:1 + n_regions * st].reshape(n_regions, st)
    return v[:, 24 * K:].reshape(n_regions, 4, 4).copy()
