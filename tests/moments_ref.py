"""Test-side reference of the exact count moments (hf_get_count_moments): numpy, written from the definition in
include/hmm_flagger_hip.h and not from the kernels.

A job is a window range first..last (global, inclusive), a state mask S (bit s = state s), a region filter (-1: every window) and a unit;
N = sum_t w_t 1[s_t in S] with w_t = weights(store, unit)[t], or 0 where the filter rejects window t.  Chunks are independent chains with the
first / A / end of viterbi_ref.tables (sampling_ref.rows in linear scale); a job's mean and variance are the sums over its chunk-local
parts, in chunk order.  Three routes, none of them the device's (piece products between f_a and b_b, centred by the posterior):

    brute_force   (a) every one of the 4^T paths of a tiny chunk, weighted by sampling_ref.path_probs: the distribution of N itself
    moments       (b) sum_t Var + 2 sum_{t<u} Cov from the explicit joint posterior of every pair of windows of a chunk (float64)
    moments_long  (c) the second-order jet of the forward recursion over the WHOLE chunk, sequentially, in np.longdouble, UNCENTRED:
                      mean = L'/L, var = L''/L - (L'/L)^2 (of the set or of its complement: see there)
and, to size the tolerance of the device tests,
    moments_centred   the gamma-centred recursion in float64 (the device's arithmetic in the reference's order), over the whole chunk"""
from __future__ import annotations

import numpy as np

import interval_ref as IR
import sampling_ref as S

UNITS = ("windows", "bases")


def weights(store, unit):
    """float64[N]: 1 per window, or the window's length in bases as the final bed forms it."""
    off = np.asarray(store.chunk_off, np.int64)
    w = np.ones(int(off[-1]))
    if unit == "windows":
        return w
    assert unit == "bases"
    W = int(store.window_len)
    for c in range(off.size - 1):
        k = np.arange(int(off[c + 1] - off[c]), dtype=np.int64)
        s = int(store.chunk_s[c]) + k * W
        e = np.minimum(s + W - 1, int(store.chunk_e[c]))
        w[off[c]:off[c + 1]] = e - s + 1
    return w


def _parts(chunk_off, first, last, mask, region):
    first = np.asarray(first, np.int64).ravel()
    region = np.broadcast_to(np.asarray(-1 if region is None else region, np.int64), first.shape)
    J, Cc, pa, pb, pm = IR.split(chunk_off, first, last, np.broadcast_to(np.asarray(mask, np.int64), first.shape))
    return first.size, J, Cc, pa, pb, pm, region[J]


def _sum_parts(n, J, pmean, pvar):
    mean, var = np.zeros(n), np.zeros(n)
    for j, m, v in zip(J, pmean, pvar):        # chunk order
        mean[j] += m
        var[j] += v
    return mean, var


def _in_set(pm, dtype=np.float64):
    return ((np.asarray(pm, np.int64)[:, None] >> np.arange(4)) & 1).astype(dtype)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def brute_force(A, end, chunk_off, w, reg, first, last, mask, region=None):
    """(mean, var) from the enumerated distribution of N: chunks of at most 7 windows."""
    off = np.asarray(chunk_off, np.int64)
    n, J, Cc, pa, pb, pm, pr = _parts(off, first, last, mask, region)
    cache = {}
    pmean, pvar = [], []
    for c, a, b, m, r in zip(Cc, pa, pb, pm, pr):
        t0, T = int(off[c]), int(off[c + 1] - off[c])
        assert T <= 7
        if c not in cache:
            pp = S.path_probs(A, end[c], t0, T)
            cache[c] = (np.array(list(pp.keys()), np.int64).reshape(-1, T), np.array(list(pp.values())))
        paths, prob = cache[c]
        t = np.arange(a, b + 1)
        wt = np.where((r < 0) | (reg[t] == r), w[t], 0.0)
        cnt = (((int(m) >> paths[:, a - t0:b - t0 + 1]) & 1) * wt[None, :]).sum(axis=1)
        mu = (prob * cnt).sum()
        pmean.append(mu)
        pvar.append((prob * (cnt - mu) ** 2).sum())
    return _sum_parts(n, J, pmean, pvar)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
def _pairwise(A, end_c, t0, T):
    """post [T][4] and joint [T][T][4][4] (t < u: P(s_t = p, s_u = q | data); the diagonal and t > u are left 0) of one chunk."""
    al = np.zeros((T, 4))
    v = A[t0, 0, :].copy()
    al[0] = v / v.sum()
    for k in range(1, T):
        v = al[k - 1] @ A[t0 + k]
        al[k] = v / v.sum()
    be = np.zeros((T, 4))
    be[T - 1] = end_c / end_c.sum()
    for k in range(T - 1, 0, -1):
        v = A[t0 + k] @ be[k]
        be[k - 1] = v / v.sum()
    post = al * be
    post /= post.sum(axis=1, keepdims=True)
    joint = np.zeros((T, T, 4, 4))
    for t in range(T):
        M = np.eye(4)
        for u in range(t + 1, T):
            M = M @ A[t0 + u]
            M /= M.max()
            j = al[t][:, None] * M * be[u][None, :]
            joint[t, u] = j / j.sum()
    return post, joint


def moments(A, end, chunk_off, w, reg, first, last, mask, region=None):
    """(mean, var) as sum_t w_t g_t and sum_t w_t^2 g_t (1 - g_t) + 2 sum_{t<u} w_t w_u (P(s_t in S, s_u in S) - g_t g_u)."""
    off = np.asarray(chunk_off, np.int64)
    n, J, Cc, pa, pb, pm, pr = _parts(off, first, last, mask, region)
    cache = {}
    pmean, pvar = [], []
    for c, a, b, m, r in zip(Cc, pa, pb, pm, pr):
        t0, T = int(off[c]), int(off[c + 1] - off[c])
        if c not in cache:
            cache[c] = _pairwise(A, end[c], t0, T)
        post, joint = cache[c]
        inS = _in_set([m])[0]
        t = np.arange(a, b + 1)
        wt = np.where((r < 0) | (reg[t] == r), w[t], 0.0)
        g = post[a - t0:b - t0 + 1] @ inS
        both = np.einsum("tupq,p,q->tu", joint[a - t0:b - t0 + 1, a - t0:b - t0 + 1], inS, inS)
        cov = np.triu(both - g[:, None] * g[None, :], 1)
        pmean.append((wt * g).sum())
        pvar.append((wt * wt * g * (1.0 - g)).sum() + 2.0 * (wt[:, None] * wt[None, :] * cov).sum())
    return _sum_parts(n, J, pmean, pvar)


# ---- (c) and the centred float64 recursion -------------------------------------------------------------------------------------------
def _jet(A, end, off, w, reg, Cc, pa, pb, pm, pr, dtype, post):
    """The jet over the whole chunk of every part, parts side by side with the local window index in lockstep (renormalised by the sum
    of v after every window).  post None: uncentred, d_t = w_t 1_S; else d_t = w_t (1_S - post_t . 1_S).  Returns (L'/L, var)."""
    t0 = off[Cc]
    T = off[Cc + 1] - t0
    m = Cc.size
    inS = _in_set(pm, dtype)
    AL = A.astype(dtype)
    EL = end.astype(dtype)
    wl = w.astype(dtype)
    v, v1, v2 = (np.zeros((m, 4), dtype) for _ in range(3))
    for k in range(int(T.max()) if m else 0):
        act = np.flatnonzero(T > k)
        idx = t0[act] + k
        if k == 0:
            nv = AL[idx, 0, :].copy()
            nv1, nv2 = np.zeros_like(nv), np.zeros_like(nv)
        else:
            rows = AL[idx]
            nv, nv1, nv2 = ((x[act][:, :, None] * rows).sum(axis=1) for x in (v, v1, v2))
        use = (pa[act] <= idx) & (idx <= pb[act]) & ((pr[act] < 0) | (reg[idx] == pr[act]))
        wt = np.where(use, wl[idx], dtype(0))
        centre = (post[idx].astype(dtype) * inS[act]).sum(axis=1) if post is not None else np.zeros(act.size, dtype)
        d = wt[:, None] * (inS[act] - centre[:, None])
        nv2 = nv2 + 2 * nv1 * d + nv * d * d
        nv1 = nv1 + nv * d
        s = nv.sum(axis=1)[:, None]
        v[act], v1[act], v2[act] = nv / s, nv1 / s, nv2 / s
    L = (v * EL[Cc]).sum(axis=1)
    r = (v1 * EL[Cc]).sum(axis=1) / L
    return r, (v2 * EL[Cc]).sum(axis=1) / L - r * r


def moments_long(A, end, chunk_off, w, reg, first, last, mask, region=None):
    """(c): (mean, var) in float64 from the uncentred np.longdouble recursion.  Uncentred, the variance is the difference of two numbers
    of size E[N]^2 and the recursion's own rounding error about eps sqrt(T) E[N]^2 (eps = 1.1e-19: 2e-11 windows^2 for a part of 2 500
    windows that are nearly all in S, and a negative "variance" for S = all four states).  N_S + N_(not S) is the constant sum of the part's
    weights, so Var[N_S] = Var[N_(not S)] and E[N_S] = sum w - E[N_(not S)]: every part counts S or its complement, whichever expects the
    smaller total (by the float64 posterior), which keeps that error under 1e-4 of the device tests' tolerance on their jobs."""
    off = np.asarray(chunk_off, np.int64)
    n, J, Cc, pa, pb, pm, pr = _parts(off, first, last, mask, region)
    post = S.forward_backward(A, end, off)
    cw = np.concatenate([[0.0], np.cumsum(w)])
    cwr = [np.concatenate([[0.0], np.cumsum(np.where(reg == r, w, 0.0))]) for r in range(int(reg.max()) + 1 if reg.size else 0)]
    total = np.array([(cw if r < 0 else cwr[r])[b + 1] - (cw if r < 0 else cwr[r])[a] if r < len(cwr) else 0.0 for a, b, r in zip(pa, pb, pr)])
    inS = _in_set(pm)
    half = np.array([(np.where((r < 0) | (reg[a:b + 1] == r), w[a:b + 1], 0.0) * (post[a:b + 1] @ s)).sum() for a, b, r, s in zip(pa, pb, pr, inS)])
    flip = half > 0.5 * total
    r, var = _jet(A, end, off, w, reg, Cc, pa, pb, np.where(flip, 15 & ~pm, pm), pr, np.longdouble, None)
    r = np.where(flip, total.astype(np.longdouble) - r, r)
    return _sum_parts(n, J, r.astype(np.float64), var.astype(np.float64))


def moments_centred(A, end, chunk_off, w, reg, first, last, mask, region=None):
    """The gamma-centred recursion in float64; the mean is sum_t w_t gamma_t."""
    off = np.asarray(chunk_off, np.int64)
    n, J, Cc, pa, pb, pm, pr = _parts(off, first, last, mask, region)
    post = S.forward_backward(A, end, off)
    _, var = _jet(A, end, off, w, reg, Cc, pa, pb, pm, pr, np.float64, post)
    inS = _in_set(pm)
    pmean = []
    for a, b, r, s in zip(pa, pb, pr, inS):
        t = np.arange(a, b + 1)
        pmean.append((np.where((r < 0) | (reg[t] == r), w[t], 0.0) * (post[t] @ s)).sum())
    return _sum_parts(n, J, pmean, np.maximum(var, 0.0))


# ---- the job sets of the tests --------------------------------------------------------------------------------------------------------
def jobs(store, rng, n_random, all_regions=False, piece=0, lane=0):
    """(first, last, mask, region): the whole track for all 15 masks (region -1; with all_regions also every region), single windows,
    whole chunks and their first and last windows (so every 1-window chunk), chunk-spanning ranges and n_random random ranges, with
    random masks and region filters; with piece / lane > 0 also ranges that start and end on, one before and one after a multiple of
    `piece` and of `lane` inside the longest chunk."""
    off = np.asarray(store.chunk_off, np.int64)
    N_ = int(off[-1])
    R = store.n_regions
    live = np.flatnonzero(np.diff(off) > 0)
    F, L, M, Rg = [], [], [], []

    def add(a, b, m, r=None):
        F.append(int(a)); L.append(int(b)); M.append(int(m))
        Rg.append(int(rng.integers(-1, R)) if r is None else int(r))
    for m in range(1, 16):
        add(0, N_ - 1, m, -1)
        for r in range(R if all_regions else 0):
            add(0, N_ - 1, m, r)
        t = int(rng.integers(0, N_))
        add(t, t, m)
    for c in live[:40]:
        add(off[c], off[c + 1] - 1, rng.integers(1, 16))
        add(off[c], off[c], rng.integers(1, 16))
        add(off[c + 1] - 1, off[c + 1] - 1, rng.integers(1, 16))
    for k in range(min(40, live.size - 1)):
        c0 = live[k]
        c1 = live[min(live.size - 1, k + 1 + int(rng.integers(0, 3)))]
        add(rng.integers(off[c0], off[c0 + 1]), rng.integers(off[c1], off[c1 + 1]), rng.integers(1, 16))
    for _ in range(n_random):
        a = int(rng.integers(0, N_))
        b = min(N_ - 1, a + int(rng.integers(0, 1 + int(rng.choice([4, 64, 700, 3000])))))
        add(a, b, rng.integers(1, 16))
    if piece:
        c = int(np.argmax(np.diff(off)))
        lo, hi = int(off[c]), int(off[c + 1]) - 1
        p = -(-(lo + 2) // piece) * piece                  # the first two piece boundaries well inside the chunk
        q = p + piece
        assert q + lane + 1 <= hi, "the longest chunk holds no two piece boundaries"
        for x, y in ((p, q), (p + lane, q + lane), (p - 3 * lane, p + 5 * lane)):
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    add(x + dx, y + dy, rng.integers(1, 15), -1)
                    add(x + dx, x + dx + (dy + 1), rng.integers(1, 15), -1)      # 1..3 windows from the boundary on
    return np.array(F, np.int64), np.array(L, np.int64), np.array(M, np.int64), np.array(Rg, np.int64)
