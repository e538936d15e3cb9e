"""Test-side reference of the exact breakpoint posteriors (hf_get_breakpoints, hf_get_breakpoint_profile): numpy, written from the
definition of include/hmm_flagger_hip.h and not from the kernels.

A job is a window range a < b inside one chunk and two disjoint state sets U, V (bit s = state s).  For k = a+1 .. b the event E_k is
"s_t in U for a <= t < k and s_t in V for k <= t <= b".  Chunks are chains with the first / A / end of sampling_ref.rows.  Three routes:

  (i)   masked_events: per k, a scaled float64 forward over the WHOLE chunk with a column mask per window (U on [a, k-1], V on [k, b],
        every state elsewhere): interval_ref.restricted_log_z with a mask per window.  P(E_k) = exp(log Z_k - log Z).
  (ii)  LongDouble: the chunk's forward and backward vectors once, then per job the prefix recursion L_t = L_{t-1} (A_t D_U) from
        f_a o 1_U and the suffix recursion r_{t-1} = (A_t D_V) r_t from b_b, every vector normalised with its log carried beside it, in
        np.longdouble; log P(E_k) = log(L_{k-1} . r_{k-1}) - log Z.  For long jobs.
  (iii) brute_force: every one of the 4^T paths of a chunk of T <= 7 windows.

Every route returns, per job, log P(E_k | data) for k = a+1 .. b; summary() turns that into (log_p_event, p)."""
from __future__ import annotations

import itertools

import numpy as np


def chunk_of(chunk_off, t):
    return int(np.searchsorted(np.asarray(chunk_off, np.int64), t, side="right") - 1)


def summary(log_pk):
    """(log_p_event, p[k]) of one job from its log P(E_k): p all zero and log_p_event -inf for a job without weight."""
    log_pk = np.asarray(log_pk, np.float64)
    m = log_pk.max()
    if not np.isfinite(m):
        return -np.inf, np.zeros(log_pk.size)
    x = np.exp(log_pk - m)
    s = x.sum()
    return float(m + np.log(s)), x / s


# ---- (i) ---------------------------------------------------------------------------------------------------------------------------------
def masked_log_z(A, end, t0, T, c, masks):
    """log of the weight of the paths of the chunk (windows t0 .. t0 + T - 1, end row end[c]) that keep window t0 + i inside the state
    set masks[m][i], for every row m of masks [M][T]; the forward vector renormalised to sum 1 after every window."""
    masks = np.asarray(masks, np.int64)
    M = masks.shape[0]
    inS = ((masks[:, :, None] >> np.arange(4)) & 1).astype(np.float64)
    logz = np.zeros(M)
    v = np.zeros((M, 4))
    for i in range(T):
        w = np.repeat(A[t0, 0, :][None, :], M, axis=0) if i == 0 else v @ A[t0 + i]
        w = w * inS[:, i]
        s = w.sum(axis=1)
        pos = s > 0
        with np.errstate(divide="ignore"):
            logz += np.where(pos, np.log(np.where(pos, s, 1.0)), -np.inf)
        v = np.where(pos[:, None], w / np.where(pos, s, 1.0)[:, None], 0.0)
    z = (v * end[c]).sum(axis=1)
    with np.errstate(divide="ignore"):
        logz += np.where(z > 0, np.log(np.where(z > 0, z, 1.0)), -np.inf)
    return logz


def masked_events(A, end, chunk_off, a, b, U, V):
    """float64[b - a]: log P(E_k | data), k = a+1 .. b, by route (i)."""
    off = np.asarray(chunk_off, np.int64)
    c = chunk_of(off, a)
    t0, T = int(off[c]), int(off[c + 1] - off[c])
    assert a < b < t0 + T and (U & V) == 0
    ks = np.arange(a + 1, b + 1)
    t = t0 + np.arange(T)
    masks = np.full((ks.size, T), 15, np.int64)
    masks = np.where((t[None, :] >= a) & (t[None, :] < ks[:, None]), U, masks)
    masks = np.where((t[None, :] >= ks[:, None]) & (t[None, :] <= b), V, masks)
    lz = masked_log_z(A, end, t0, T, c, np.concatenate([masks, np.full((1, T), 15, np.int64)]))
    with np.errstate(invalid="ignore"):
        return lz[:-1] - lz[-1]


# ---- (iii) -------------------------------------------------------------------------------------------------------------------------------
def brute_force(A, end, chunk_off, a, b, U, V):
    """The same by enumeration of every path of the chunk (4^T paths: tiny chunks only)."""
    off = np.asarray(chunk_off, np.int64)
    c = chunk_of(off, a)
    t0, T = int(off[c]), int(off[c + 1] - off[c])
    paths = np.array(list(itertools.product(range(4), repeat=T)), np.int64)
    w = A[t0, 0, paths[:, 0]].copy()
    for t in range(1, T):
        w *= A[t0 + t, paths[:, t - 1], paths[:, t]]
    w *= end[c][paths[:, -1]]
    inU, inV = ((U >> paths) & 1) == 1, ((V >> paths) & 1) == 1
    out = []
    for k in range(a + 1, b + 1):
        ok = np.all(inU[:, a - t0:k - t0], axis=1) & np.all(inV[:, k - t0:b - t0 + 1], axis=1)
        ps = w[ok].sum() / w.sum()
        out.append(np.log(ps) if ps > 0 else -np.inf)
    return np.array(out)


# ---- (ii) --------------------------------------------------------------------------------------------------------------------------------
def _norm(v):
    """(v / sum, log sum) along the last axis; a zero vector stays zero with log -inf."""
    s = v.sum(axis=-1)
    pos = s > 0
    with np.errstate(divide="ignore"):
        ls = np.where(pos, np.log(np.where(pos, s, 1)), -np.inf)
    return np.where(pos[..., None], v / np.where(pos, s, 1)[..., None], 0), ls


class LongDouble:
    """Route (ii): the forward and backward vectors of every chunk once (normalised, their logs beside them), then jobs in lockstep."""

    def __init__(self, A, end, chunk_off):
        LD = np.longdouble
        self.A = np.asarray(A).astype(LD)
        self.off = np.asarray(chunk_off, np.int64)
        n = self.A.shape[0]
        self.f, self.lf = np.zeros((n, 4), LD), np.zeros(n, LD)
        self.b, self.lb = np.zeros((n, 4), LD), np.zeros(n, LD)
        self.logz = np.zeros(self.off.size - 1, LD)
        for c in range(self.off.size - 1):
            t0, t1 = int(self.off[c]), int(self.off[c + 1])
            if t1 <= t0:
                continue
            v, lv = _norm(self.A[t0, 0, :].copy())
            for t in range(t0, t1):
                if t > t0:
                    v, s = _norm(v @ self.A[t])
                    lv = lv + s
                self.f[t], self.lf[t] = v, lv
            r, lr = _norm(np.asarray(end[c]).astype(LD))
            for t in range(t1 - 1, t0 - 1, -1):
                if t < t1 - 1:
                    r, s = _norm(self.A[t + 1] @ r)
                    lr = lr + s
                self.b[t], self.lb[t] = r, lr
            with np.errstate(divide="ignore"):
                self.logz[c] = self.lf[t1 - 1] + self.lb[t1 - 1] + np.log((self.f[t1 - 1] * self.b[t1 - 1]).sum())

    def events(self, first, last, U, V):
        """[log P(E_k | data), k = first[j]+1 .. last[j]] for every job j (float64 arrays)."""
        LD = np.longdouble
        first, last = np.asarray(first, np.int64), np.asarray(last, np.int64)
        U, V = np.asarray(U, np.int64), np.asarray(V, np.int64)
        m = first.size
        if m == 0:
            return []
        ln = last - first
        mx = int(ln.max())
        inU = ((U[:, None] >> np.arange(4)) & 1).astype(LD)
        inV = ((V[:, None] >> np.arange(4)) & 1).astype(LD)
        # Ls[j][i], lLs[j][i]: L_{a+i} normalised and its log, i = 0 .. ln - 1
        Ls, lLs = np.zeros((m, mx, 4), LD), np.full((m, mx), -np.inf, LD)
        v, s = _norm(self.f[first] * inU)
        lv = self.lf[first] + s
        for i in range(mx):
            act = np.flatnonzero(ln > i)
            Ls[act, i], lLs[act, i] = v[act], lv[act]
            nxt = np.flatnonzero(ln > i + 1)
            if nxt.size:
                w, s = _norm(np.einsum("mp,mps->ms", v[nxt], self.A[first[nxt] + i + 1]) * inU[nxt])
                v[nxt], lv[nxt] = w, lv[nxt] + s
        out = np.full((m, mx), -np.inf, LD)
        r, lr = self.b[last].copy(), self.lb[last].copy()
        for i in range(mx):                                   # k = last - i
            act = np.flatnonzero(ln > i)
            k = last[act] - i
            w, s = _norm(np.einsum("mps,ms->mp", self.A[k] * inV[act][:, None, :], r[act]))
            r[act], lr[act] = w, lr[act] + s
            idx = (k - 1 - first[act]).astype(np.int64)
            d = (Ls[act, idx] * r[act]).sum(axis=1)
            with np.errstate(divide="ignore"):
                out[act, idx] = lLs[act, idx] + lr[act] + np.where(d > 0, np.log(np.where(d > 0, d, 1)), -np.inf)
        cs = np.array([chunk_of(self.off, a) for a in first])
        res = []
        for j in range(m):
            with np.errstate(invalid="ignore"):
                res.append((out[j, :ln[j]] - self.logz[cs[j]]).astype(np.float64))
        return res


# ---- the checks of an index against a reference profile ---------------------------------------------------------------------------------------
def quantile_ok(p_ref, first, k, q, band):
    """A quantile k (global window index) for probability q passes iff c[k] >= q - band and c[k - 1] < q + band, c[first] = 0."""
    c = np.concatenate([[0.0], np.cumsum(p_ref)])
    i = int(k) - int(first)
    return 1 <= i < c.size and c[i] >= q - band and c[i - 1] < q + band


def mode_ok(p_ref, first, k):
    i = int(k) - int(first) - 1
    mx = float(np.max(p_ref))
    return 0 <= i < len(p_ref) and p_ref[i] >= mx - (1e-12 + 1e-9 * mx)
