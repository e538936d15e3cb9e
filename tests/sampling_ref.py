"""Test-side reference of the posterior path sampler (hf_sample_paths): float64 numpy, written from the definition in
include/hmm_flagger_hip.h, not from the kernels.  The rows come from viterbi_ref.tables (first[s] in row 0 of a chunk-first window,
A_t elsewhere, end per chunk).

    rng: splitmix64, sample_key, uniforms                 the counter-based uniforms
    ffbs(A, end, chunk_off, seed, ks)                     sequential forward filtering, backward sampling with the draw rule:
                                                          (labels int8[K][N], window margins float32[K][N], final margins [K][C])
    path_probs(A, end, T)                                 brute force: the probability of every path of a tiny chain
    forward_backward(A, end, chunk_off)                   posterior marginals [N][4]"""
from __future__ import annotations

import itertools

import numpy as np

import viterbi_ref

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def splitmix64(x):
    """The standard splitmix64 finaliser of x + 0x9E3779B97F4A7C15, on Python ints or uint64 arrays (wrapping)."""
    if isinstance(x, np.ndarray):
        with np.errstate(over="ignore"):
            z = x.astype(np.uint64) + np.uint64(GOLDEN)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))
    z = (int(x) + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_key(seed: int, k: int) -> int:
    return splitmix64((int(seed) & M64) ^ splitmix64(int(k)))


def uniforms(key: int, idx) -> np.ndarray:
    """u(k, i) = (splitmix64(key_k + i) >> 11) * 2^-53 for an array of counters i."""
    with np.errstate(over="ignore"):
        z = splitmix64(np.asarray(idx, np.uint64) + np.uint64(key))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def rows(store, model, alpha, adjust=True, min_frac=0.95):
    """(A [N][pre][s], end [C][4]) in linear scale."""
    logA, logend = viterbi_ref.tables(store, model, alpha, adjust, min_frac)
    return np.exp(logA), np.exp(logend)


def _norm(v):
    """Scale every row of v by 2^-e, e = the exponent of its largest entry (exact): the renormalisation of the kernels."""
    m = v.max(axis=-1)
    e = np.where(m > 0, np.frexp(np.where(m > 0, m, 1.0))[1] - 1, 0)
    return np.ldexp(v, -e[..., None])


def _pick(W, Cm, u):
    """The draw rule, vectorised: W, Cm [m][4], u [m] -> (choice [m], margin [m])."""
    x = u * Cm[:, 3]
    below = x[:, None] < Cm
    choice = np.where(below.any(axis=1), np.argmax(below, axis=1), -1)
    pos = W > 0
    last_pos = np.where(pos.any(axis=1), 3 - np.argmax(pos[:, ::-1], axis=1), 0)
    choice = np.where(choice >= 0, choice, last_pos)
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.min(np.abs(x[:, None] - Cm), axis=1) / Cm[:, 3]
    return choice.astype(np.int64), margin


def forward(A, chunk_off):
    """Per window t: weights W[t][s][p] = alpha_{t-1}[p] * A_t[p][s] and their cumulative sums over p (left to right), alpha_{-1} =
    (1, 0, 0, 0) at every chunk start; returns (W, Cm, alpha_last [C][4])."""
    off = np.asarray(chunk_off, np.int64)
    T = np.diff(off)
    n = int(off[-1])
    W = np.zeros((n, 4, 4))
    Cm = np.zeros((n, 4, 4))
    alast = np.zeros((T.size, 4))
    if n == 0:
        return W, Cm, alast
    live = np.flatnonzero(T > 0)
    a = np.zeros((live.size, 4))
    a[:, 0] = 1.0
    for k in range(int(T.max())):
        act = T[live] > k
        idx = off[live[act]] + k
        w = a[act][:, :, None] * A[idx]                  # [m][p][s]
        w = np.transpose(w, (0, 2, 1))                   # [m][s][p]
        c = np.cumsum(w, axis=2)
        W[idx], Cm[idx] = w, c
        a[act] = _norm(c[:, :, 3])
    alast[live] = a
    return W, Cm, alast


def ffbs(A, end, chunk_off, seed, ks, fwd=None, n_windows=None):
    """Samples `ks` (absolute indices), vectorised over samples and chunks: (labels int8[K][N], window margins float32[K][N] (0 at
    chunk-first windows), final margins float32[K][C]).  n_windows: the track's window count where it is not chunk_off[-1] (windows
    outside every chunk: their labels stay 0 here); the final-state draw of chunk c takes uniform n_windows + c."""
    off = np.asarray(chunk_off, np.int64)
    T = np.diff(off)
    C_ = T.size
    n = int(off[-1]) if n_windows is None else int(n_windows)
    W, Cm, alast = forward(A, off) if fwd is None else fwd
    keys = np.array([sample_key(seed, k) for k in ks], np.uint64)
    K = keys.size
    labels = np.zeros((K, n), np.int8)
    marg = np.zeros((K, n), np.float32)
    fmarg = np.zeros((K, C_), np.float32)
    live = np.flatnonzero(T > 0)
    if n == 0:
        return labels, marg, fmarg
    fw = alast[live] * end[live]
    fc = np.cumsum(fw, axis=1)
    m = live.size
    uf = uniforms(0, keys[:, None] + np.uint64(n) + live[None, :].astype(np.uint64))      # [K][m]
    s, fm = _pick(np.broadcast_to(fw, (K, m, 4)).reshape(-1, 4), np.broadcast_to(fc, (K, m, 4)).reshape(-1, 4), uf.ravel())
    s = s.reshape(K, m)
    fmarg[:, live] = fm.reshape(K, m)
    for q in range(int(T.max()) - 1, -1, -1):
        act = T[live] > q
        idx = off[live[act]] + q
        st = s[:, act]                                                                      # [K][a]
        labels[:, idx] = st
        if q == 0:
            continue
        u = uniforms(0, keys[:, None] + idx[None, :].astype(np.uint64))
        ii = np.broadcast_to(idx[None, :], st.shape)
        pr, mg = _pick(W[ii, st].reshape(-1, 4), Cm[ii, st].reshape(-1, 4), u.ravel())
        marg[:, idx] = mg.reshape(st.shape)
        s[:, act] = pr.reshape(st.shape)
    return labels, marg, fmarg


def path_probs(A, end, t0, T):
    """Brute force over the 4^T paths of the chunk at windows t0 .. t0+T-1: {path: probability}."""
    out = {}
    for path in itertools.product(range(4), repeat=T):
        w = A[t0, 0, path[0]]
        for t in range(1, T):
            w *= A[t0 + t, path[t - 1], path[t]]
        out[path] = w * end[path[-1]]
    tot = sum(out.values())
    return {p: v / tot for p, v in out.items()}


def forward_backward(A, end, chunk_off):
    """Posterior marginals [N][4] of the distribution above (normalised forward and backward vectors per window)."""
    off = np.asarray(chunk_off, np.int64)
    T = np.diff(off)
    n = int(off[-1])
    post = np.zeros((n, 4))
    if n == 0:
        return post
    _, Cm, _ = forward(A, off)
    alpha = Cm[:, :, 3]
    alpha = alpha / alpha.sum(axis=1, keepdims=True)
    live = np.flatnonzero(T > 0)
    b = end[live] / end[live].sum(axis=1, keepdims=True)
    for q in range(int(T.max()) - 1, -1, -1):
        act = T[live] > q
        idx = off[live[act]] + q
        g = alpha[idx] * b[act]
        post[idx] = g / g.sum(axis=1, keepdims=True)
        if q > 0:
            nb = np.einsum("mps,ms->mp", A[idx], b[act])
            b[act] = nb / nb.sum(axis=1, keepdims=True)
    return post
