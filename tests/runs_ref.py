"""Test-side reference of the exact run moments (hf_get_run_moments): numpy, written from the definition in
include/hmm_flagger_hip.h and not from the kernels.

A job is a window range first..last (global, inclusive) and a state mask S (bit s = state s); `joined` [n_chunks] says which chunks
continue the chunk before.  For a chunk-local part [a, b]: R = 1[s_a in S] + sum_{t=a+1..b} 1[s_{t-1} not in S, s_t in S], S0 = 1[s_a in
S], E0 = 1[s_b in S]; the job's count is B = sum_j R_j - sum_{joined j} E0_j S0_{j+1}.  Chunks are independent chains with the first /
A / end of viterbi_ref.tables (sampling_ref.rows in linear scale).  Routes, none of them the device's (piece products between f_a and
b_b with a centred pair tilt):

    brute_force   (a) every one of the 4^T paths of a tiny chunk into the joint distribution of (R, S0, E0) of a part, the parts combined
                      by a dynamic programme over (count so far, E0 of the part before): the distribution of B itself, joins included
    pairwise      (b) Var(R) = sum of the variances + 2 sum of the covariances of the indicators of a part (1[s_a in S] and the pair
                      indicators), every joint probability by an explicit constrained forward product; the covariances with S0 and E0
                      likewise; the seven numbers per part feed the stitching formula (stitch)
    jet_long      (c) the UNCENTRED second-order jet over the whole part, sequentially, in np.longdouble; then stitch
and, to size the tolerance of the device tests,
    jet_centred   (d) the centred recursion in float64 (the device's arithmetic in the reference's order); then stitch

The seven numbers of a part: E[R], Var(R), s = E[S0], e = E[E0], Cov(R, E0), Cov(R, S0), Cov(S0, E0)."""
from __future__ import annotations

import numpy as np

import interval_ref as IR
import sampling_ref as S


def _bits(m):
    return ((int(m) >> np.arange(4)) & 1).astype(bool)


def part_joins(J, Cc, joined):
    """bool[m]: part k is joined to part k - 1 (same job, the next chunk, and that chunk continues the one before)."""
    J, Cc = np.asarray(J, np.int64), np.asarray(Cc, np.int64)
    out = np.zeros(J.size, bool)
    if joined is None or J.size < 2:
        return out
    jn = np.asarray(joined).astype(bool)
    out[1:] = (J[1:] == J[:-1]) & (Cc[1:] == Cc[:-1] + 1) & jn[Cc[1:]]
    return out


def stitch(n, J, Cc, seven, joined):
    """(mean, var, scale) per job from the parts' seven numbers by the stitching formula, every sum left to right; scale = the sum of
    the absolute values of the formula's variance terms (the variance is a sum of terms of both signs)."""
    join = part_joins(J, Cc, joined)
    m, mq, v, vj, vjj, sc = (np.zeros(n) for _ in range(6))
    for k in range(len(J)):
        j = J[k]
        x = seven[k]
        m[j] += x[0]
        v[j] += x[1]
        sc[j] += abs(x[1])
        if join[k]:
            y = seven[k - 1]
            q = y[3] * x[2]
            mq[j] += q
            terms = (q * (1.0 - q), -2.0 * x[2] * y[4], -2.0 * y[3] * x[5])
            vj[j] += terms[0] + terms[1] + terms[2]
            sc[j] += sum(abs(t) for t in terms)
            if join[k - 1]:
                z = seven[k - 2][3] * x[2] * y[6]
                vjj[j] += z
                sc[j] += 2.0 * abs(z)
    return m - mq, np.maximum((v + vj) + 2.0 * vjj, 0.0), sc


def groups(chunk_off, first, last, joined):
    """The number of maximal joined groups of every job's parts."""
    first = np.asarray(first, np.int64).ravel()
    J, Cc, _, _, _ = IR.split(chunk_off, first, last, np.ones(first.size, np.int64))
    join = part_joins(J, Cc, joined)
    out = np.zeros(first.size, np.int64)
    np.add.at(out, J[~join], 1)
    return out


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def brute_force(A, end, chunk_off, first, last, mask, joined=None):
    """(mean, var) from the enumerated distribution of B: chunks of at most 7 windows."""
    off = np.asarray(chunk_off, np.int64)
    first = np.asarray(first, np.int64).ravel()
    J, Cc, pa, pb, pm = IR.split(off, first, last, np.broadcast_to(np.asarray(mask, np.int64), first.shape))
    join = part_joins(J, Cc, joined)
    paths_of = {}
    mean, var = np.zeros(first.size), np.zeros(first.size)
    dist = {}
    for k in range(J.size):
        c, a, b = int(Cc[k]), int(pa[k]), int(pb[k])
        t0, T = int(off[c]), int(off[c + 1] - off[c])
        assert T <= 7
        if c not in paths_of:
            pp = S.path_probs(A, end[c], t0, T)
            paths_of[c] = (np.array(list(pp.keys()), np.int64).reshape(-1, T), np.array(list(pp.values())))
        paths, prob = paths_of[c]
        inS = _bits(pm[k])[paths[:, a - t0:b - t0 + 1]]                    # [paths][windows of the part]
        R = inS[:, 0].astype(np.int64) + (~inS[:, :-1] & inS[:, 1:]).sum(axis=1)
        trip = {}
        for r, s0, e0, p in zip(R, inS[:, 0], inS[:, -1], prob):
            key = (int(r), bool(s0), bool(e0))
            trip[key] = trip.get(key, 0.0) + p
        new = {}
        if k == 0 or J[k] != J[k - 1]:
            dist = {(0, False): 1.0}
        for (cnt, pe), p in dist.items():
            for (r, s0, e0), q in trip.items():
                key = (cnt + r - (1 if (join[k] and pe and s0) else 0), e0)
                new[key] = new.get(key, 0.0) + p * q
        dist = new
        if k + 1 == J.size or J[k + 1] != J[k]:
            cnts = np.array([key[0] for key in dist], np.float64)
            ps = np.array(list(dist.values()))
            mu = (ps * cnts).sum() / ps.sum()
            mean[J[k]] = mu
            var[J[k]] = (ps * (cnts - mu) ** 2).sum() / ps.sum()
    return mean, var


# ---- forward and backward vectors ------------------------------------------------------------------------------------------------------
def alpha_beta(A, end, chunk_off, dtype=np.float64):
    """(alpha [N][4], beta [N][4]): the forward and backward vectors of every window, each normalised to sum 1, chunks side by side."""
    off = np.asarray(chunk_off, np.int64)
    T = np.diff(off)
    n = int(off[-1])
    AL, EL = A.astype(dtype), end.astype(dtype)
    al, be = np.zeros((n, 4), dtype), np.zeros((n, 4), dtype)
    live = np.flatnonzero(T > 0)
    for k in range(int(T.max()) if live.size else 0):
        act = live[T[live] > k]
        idx = off[act] + k
        v = AL[idx, 0, :] if k == 0 else (al[idx - 1][:, :, None] * AL[idx]).sum(axis=1)
        al[idx] = v / v.sum(axis=1, keepdims=True)
    for k in range(int(T.max()) if live.size else 0):           # k windows before the chunk's last
        act = live[T[live] > k]
        idx = off[act + 1] - 1 - k
        v = EL[act] if k == 0 else (AL[idx + 1] * be[idx + 1][:, None, :]).sum(axis=2)
        be[idx] = v / v.sum(axis=1, keepdims=True)
    return al, be


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
def _pairwise_part(A, al, be, a, b, inS):
    """The seven numbers of the part [a, b] from explicit joint probabilities.  Indicators: I_a = 1[s_a in S], I_t = 1[s_{t-1} not in S,
    s_t in S] (t = a+1..b).  A constrained forward vector x (the weight of the prefixes that satisfy an event, by state of the last
    window) is carried to the right with the plain rows; every probability is x . beta / (alpha . beta) at the window where it ends,
    with x and alpha renormalised alike (x by alpha's own factor c_t)."""
    out_ = ~inS
    T = b - a + 1
    c = np.ones(T)                                              # alpha_t = alpha_{t-1} A_t / c_t
    for t in range(a + 1, b + 1):
        c[t - a] = (al[t - 1] @ A[t]).sum()
    Z = [float(al[t] @ be[t]) for t in range(a, b + 1)]

    def event(t, x_prev):
        """x after the indicator of window t, from the plain (or constrained) vector of window t - 1."""
        if t == a:
            return np.where(inS, al[a], 0.0)
        return np.where(inS, (np.where(out_, x_prev, 0.0) @ A[t]) / c[t - a], 0.0)

    p = np.zeros(T)                                             # E[I_t]
    pE = np.zeros(T)                                            # E[I_t E0]
    both = np.zeros((T, T))                                     # E[I_t I_u], t < u
    for t in range(a, b + 1):
        x = event(t, al[t - 1] if t > a else None)
        p[t - a] = x @ be[t] / Z[t - a]
        for u in range(t + 1, b + 1):
            both[t - a, u - a] = event(u, x) @ be[u] / Z[u - a]
            x = (x @ A[u]) / c[u - a]
        pE[t - a] = np.where(inS, x, 0.0) @ be[b] / Z[-1]
    ER = p.sum()
    var = (p * (1.0 - p)).sum() + 2.0 * np.triu(both - p[:, None] * p[None, :], 1).sum()
    s = p[0]
    e = float(np.where(inS, al[b], 0.0) @ be[b] / Z[-1])
    cov_RE = (pE - p * e).sum()
    cov_RS = p[0] * (1.0 - p[0]) + (both[0, 1:] - p[0] * p[1:]).sum()
    cov_SE = pE[0] - s * e
    return np.array([ER, var, s, e, cov_RE, cov_RS, cov_SE])


def pairwise(A, end, chunk_off, first, last, mask, joined=None):
    """(b): (mean, var, scale)."""
    off = np.asarray(chunk_off, np.int64)
    first = np.asarray(first, np.int64).ravel()
    J, Cc, pa, pb, pm = IR.split(off, first, last, np.broadcast_to(np.asarray(mask, np.int64), first.shape))
    al, be = alpha_beta(A, end, off)
    cache = {}
    seven = []
    for a, b, m in zip(pa, pb, pm):
        key = (int(a), int(b), int(m))
        if key not in cache:
            cache[key] = _pairwise_part(A, al, be, int(a), int(b), _bits(m))
        seven.append(cache[key])
    return stitch(first.size, J, Cc, seven, joined)


# ---- (c) and (d) -----------------------------------------------------------------------------------------------------------------------
def _jet(A, al, be, pa, pb, pm, dtype, centred):
    """The seven numbers of every part from the second-order jet over the part, parts side by side with the window index in lockstep
    (v renormalised to sum 1 after every window, the other vectors by the same factor).  centred False: the tilt is the indicator itself
    (d_a = 1_S, D_t = J); True: d_a = 1_S - gamma_a(S), D_t = J - xi_t, and E[R] = gamma_a(S) + sum_t xi_t."""
    m = pa.size
    inS = ((np.asarray(pm, np.int64)[:, None] >> np.arange(4)) & 1).astype(dtype)
    Jm = (1 - inS)[:, :, None] * inS[:, None, :]                # [m][p][s]
    AL = A.astype(dtype) if A.dtype != dtype else A
    fa, ba, bb = al[pa].astype(dtype), be[pa].astype(dtype), be[pb].astype(dtype)
    ga = fa * ba
    s0 = (ga * inS).sum(axis=1) / ga.sum(axis=1)
    gb = al[pb].astype(dtype) * bb
    e0 = (gb * inS).sum(axis=1) / gb.sum(axis=1)
    d = inS - (s0[:, None] if centred else 0)
    v, v1, v2 = fa.copy(), fa * d, fa * d * d
    u, u1 = fa * inS, fa * inS * d
    mean = s0.copy()
    Tp = pb - pa
    for k in range(1, int(Tp.max()) + 1 if m else 0):
        act = np.flatnonzero(Tp >= k)
        idx = pa[act] + k
        rows = AL[idx]
        G = rows * Jm[act]
        if centred:
            w = al[idx - 1].astype(dtype)[:, :, None] * rows * be[idx].astype(dtype)[:, None, :]
            xi = (w * Jm[act]).sum(axis=(1, 2)) / w.sum(axis=(1, 2))
            mean[act] += xi
        else:
            xi = np.zeros(act.size, dtype)
        x = xi[:, None, None]
        D1 = G - x * rows
        D2 = (1 - 2 * x) * G + x * x * rows

        def mul(vec, mat):
            return (vec[act][:, :, None] * mat).sum(axis=1)
        nv2 = mul(v2, rows) + 2 * mul(v1, D1) + mul(v, D2)
        nv1 = mul(v1, rows) + mul(v, D1)
        nu1 = mul(u1, rows) + mul(u, D1)
        nv, nu = mul(v, rows), mul(u, rows)
        sc = nv.sum(axis=1)[:, None]
        v[act], v1[act], v2[act], u[act], u1[act] = nv / sc, nv1 / sc, nv2 / sc, nu / sc, nu1 / sc
    L = (v * bb).sum(axis=1)
    r = (v1 * bb).sum(axis=1) / L
    var = (v2 * bb).sum(axis=1) / L - r * r
    cov_RE = (v1 * bb * inS).sum(axis=1) / L - r * e0
    cov_RS = (u1 * bb).sum(axis=1) / L - r * s0
    cov_SE = (u * bb * inS).sum(axis=1) / L - s0 * e0
    if not centred:
        mean = r
    return np.stack([mean, var, s0, e0, cov_RE, cov_RS, cov_SE], axis=1).astype(np.float64)


def _route(A, end, chunk_off, first, last, mask, joined, dtype, centred):
    off = np.asarray(chunk_off, np.int64)
    first = np.asarray(first, np.int64).ravel()
    J, Cc, pa, pb, pm = IR.split(off, first, last, np.broadcast_to(np.asarray(mask, np.int64), first.shape))
    al, be = alpha_beta(A, end, off, dtype)
    # equal parts once
    key, inv = np.unique(np.stack([pa, pb, pm], axis=1), axis=0, return_inverse=True)
    seven = _jet(A.astype(dtype), al, be, key[:, 0], key[:, 1], key[:, 2], dtype, centred)[inv.ravel()]
    if centred:
        seven[:, 1] = np.maximum(seven[:, 1], 0.0)
    return stitch(first.size, J, Cc, seven, joined)


def jet_long(A, end, chunk_off, first, last, mask, joined=None):
    """(c): (mean, var, scale) in float64 from the uncentred np.longdouble recursion.  Uncentred, a part's variance is the difference of
    two numbers of size E[R]^2; E[R] stays below a few hundred runs on the stores of the tests, which keeps the recursion's own rounding
    error (about 1.1e-19 sqrt(T) E[R]^2) under a tenth of the device tests' absolute term."""
    return _route(A, end, chunk_off, first, last, mask, joined, np.longdouble, False)


def jet_centred(A, end, chunk_off, first, last, mask, joined=None):
    """(d): (mean, var, scale) from the centred recursion in float64."""
    return _route(A, end, chunk_off, first, last, mask, joined, np.float64, True)


def split_store(store):
    """The store with every chunk of at least 64 windows cut into consecutive chunks of the same contig: an even chunk into n - 37 and 37
    windows, an odd one into n - 41, 1 and 40 (a one-window chunk between two joins).  The windows and their order stay, so the longest
    chunk keeps all but 41 of its windows; contig_joins of the result joins what was cut."""
    import dataclasses
    off = np.asarray(store.chunk_off, np.int64)
    wl = int(store.window_len)
    new_off, ctg, ctg_len, cs, ce = [0], [], [], [], []
    for c in range(len(store.chunk_ctg)):
        n = int(off[c + 1] - off[c])
        sizes = [n] if n < 64 else ([n - 37, 37] if c % 2 == 0 else [n - 41, 1, 40])
        s = int(store.chunk_s[c])
        for i, k in enumerate(sizes):
            e = int(store.chunk_e[c]) if i + 1 == len(sizes) else s + k * wl - 1
            new_off.append(new_off[-1] + k)
            ctg.append(store.chunk_ctg[c]); ctg_len.append(int(store.chunk_ctg_len[c])); cs.append(s); ce.append(e)
            s = e + 1
    return dataclasses.replace(store, chunk_off=np.asarray(new_off, np.int64), chunk_ctg=ctg, chunk_ctg_len=np.asarray(ctg_len, np.int32),
                               chunk_s=np.asarray(cs, np.int32), chunk_e=np.asarray(ce, np.int32))


def contig_joins(store):
    """joined [n_chunks]: chunk c carries the contig name of chunk c - 1 (the rule the final BED merges by)."""
    ctg = list(store.chunk_ctg)
    return np.array([c > 0 and ctg[c] == ctg[c - 1] for c in range(len(ctg))], bool)
