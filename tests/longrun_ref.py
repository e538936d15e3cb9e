"""Test-side reference of the exact long-run probabilities (hf_get_long_run_log_probs): numpy float64, by another route than the
device's.  The device walks the pass's rows A_t between f_a and b_b with power-of-two exponents; here every chunk becomes its POSTERIOR
Markov chain first (initial distribution gamma_a, transition at window t the pair posterior over its row marginal, as in entropy_ref.py,
from the normalised forward and backward vectors of runs_ref.alpha_beta over sampling_ref.rows), and the run-length counter is carried
through that normalised chain as a probability distribution: the total stays 1, the probability of a HIT is what has been absorbed.
Across a joined chunk boundary the counter distribution is kept and the next chunk starts from its own gamma, independently.

    Chain(A, end, chunk_off).log_probs(first, last, mask, min_len, joined) -> (log_p_none, log_p_some)
    brute_force(A, end, chunk_off, first, last, mask, min_len, joined)      the same from all 4^T paths of tiny groups

Groups side by side with the position inside the group in lockstep.  The non-HIT part is renormalised to sum 1 after every window with
its log carried, the HIT part is a log carried by logaddexp: neither underflows.  Of the two logs the smaller is taken as computed and the
other as log1p(-exp(.)) of it."""
from __future__ import annotations

import numpy as np

import interval_ref as IR
import runs_ref as RR
import sampling_ref as S


def lanes(mask, min_len):
    """The lanes of the device's expanded chain: the states outside S, the counters (s, d), d = 1..L-1, four HIT lanes."""
    k = bin(int(mask)).count("1")
    return (4 - k) + k * (int(min_len) - 1) + 4


def _groups(off, first, last, joined):
    """Per group: (job, [(chunk, a, b), ..]) in job and chunk order."""
    first = np.asarray(first, np.int64).ravel()
    J, Cc, pa, pb, _ = IR.split(off, first, last, np.ones(first.size, np.int64))
    join = RR.part_joins(J, Cc, joined)
    out = []
    for k in range(len(J)):
        if not join[k]:
            out.append((int(J[k]), []))
        out[-1][1].append((int(Cc[k]), int(pa[k]), int(pb[k])))
    return out


def _finish(n, gj, ln, lh):
    """Per group (log none, log some) from the two carried logs, then the jobs: the sum of the groups' log none, and its complement."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        hit_small = lh < ln
        g_none = np.where(hit_small, np.log1p(-np.exp(np.minimum(lh, 0.0))), ln)
        g_some = np.where(hit_small, lh, np.log1p(-np.exp(np.minimum(ln, 0.0))))
        none = np.zeros(n)
        cnt = np.zeros(n, np.int64)
        one = np.full(n, -np.inf)
        for g, j in enumerate(gj):                 # chunk order
            none[j] += g_none[g]
            if g_some[g] > -np.inf:
                cnt[j] += 1
                one[j] = g_some[g]
        neg = np.minimum(none, 0.0)
        many = np.where(neg > -np.log(2.0), np.log(-np.expm1(neg)), np.log1p(-np.exp(neg)))
    return none, np.where(cnt == 0, -np.inf, np.where(cnt == 1, one, many))


class Chain:
    """The posterior Markov chain of every chunk, once per (A, end, chunk_off); then any number of job sets."""

    def __init__(self, A, end, chunk_off):
        self.off = off = np.asarray(chunk_off, np.int64)
        n = int(off[-1])
        al, be = RR.alpha_beta(A, end, off)
        g = al * be
        self.gamma = g / g.sum(axis=1, keepdims=True)
        prev = np.maximum(np.arange(n) - 1, 0)
        x = (al[prev][:, :, None] * A) * be[:, None, :]                     # [t][p][s]
        m = x.sum(axis=2, keepdims=True)
        self.P = np.where(m > 0, x / np.where(m > 0, m, 1.0), 0.0)          # rows sum to 1 (a row without weight: zeros)

    def log_probs(self, first, last, mask, min_len, joined=None):
        first = np.asarray(first, np.int64).ravel()
        n = first.size
        mask = np.broadcast_to(np.asarray(mask, np.int64), first.shape)
        min_len = np.broadcast_to(np.asarray(min_len, np.int64), first.shape)
        groups = _groups(self.off, first, last, joined)
        if not groups:
            return np.zeros(n), np.full(n, -np.inf)
        # flat windows of every group, and where a part other than the first begins
        length = np.array([sum(b - a + 1 for _, a, b in parts) for _, parts in groups], np.int64)
        order = np.argsort(-length, kind="stable")
        start = np.zeros(len(groups) + 1, np.int64)
        start[1:] = np.cumsum(length[order])
        win = np.empty(int(start[-1]), np.int64)
        bnd = np.zeros(int(start[-1]), bool)
        for r, gi in enumerate(order):
            p = int(start[r])
            for k, (_, a, b) in enumerate(groups[gi][1]):
                win[p:p + b - a + 1] = np.arange(a, b + 1)
                bnd[p] = k > 0
                p += b - a + 1
        gj = np.array([groups[gi][0] for gi in order], np.int64)
        inS = ((mask[gj][:, None] >> np.arange(4)) & 1).astype(bool)        # [G][4]
        Lg = min_len[gj]
        G = len(groups)
        D = max(int(Lg.max()) - 1, 1)
        dead = np.arange(D)[None, :] >= (Lg - 1)[:, None]                   # counter places a group does not have
        last_d = np.maximum(Lg - 2, 0)
        ln, lh = np.zeros(G), np.full(G, -np.inf)
        lens = length[order]
        # the first window
        g0 = self.gamma[win[start[:-1]]]
        out = np.where(inS, 0.0, g0)
        cnt = np.zeros((G, D, 4))
        ent = np.where(inS, g0, 0.0)
        one = Lg == 1
        with np.errstate(divide="ignore"):
            lh[one] = np.log(ent[one].sum(axis=1))
        cnt[~one, 0] = ent[~one]
        s = out.sum(axis=1) + cnt.sum(axis=(1, 2))
        with np.errstate(divide="ignore", invalid="ignore"):
            ln += np.log(s)
            sc = np.where(s > 0, s, 1.0)
        out /= sc[:, None]
        cnt /= sc[:, None, None]
        for k in range(1, int(lens[0])):
            na = int(np.searchsorted(-lens, -k, side="left"))               # groups longer than k
            idx = start[:na] + k
            t = win[idx]
            P = np.where(bnd[idx][:, None, None], self.gamma[t][:, None, :], self.P[t])       # [na][p][s]
            o, c, iS = out[:na], cnt[:na], inS[:na]
            tot = o + c.sum(axis=1)
            new_out = np.where(iS, 0.0, np.einsum("gp,gps->gs", tot, P))
            from_out = np.where(iS, np.einsum("gp,gps->gs", o, P), 0.0)
            shifted = np.where(iS[:, None, :], np.einsum("gdp,gps->gds", c, P), 0.0)
            one_k = one[:na]
            inflow = np.where(one_k, from_out.sum(axis=1), shifted[np.arange(na), last_d[:na]].sum(axis=1))
            new_cnt = np.zeros_like(c)
            new_cnt[:, 0] = np.where(one_k[:, None], 0.0, from_out)
            new_cnt[:, 1:] = shifted[:, :-1]
            new_cnt[dead[:na]] = 0.0
            with np.errstate(divide="ignore", invalid="ignore"):
                lh[:na] = np.logaddexp(lh[:na], np.log(inflow) + ln[:na])
                s = new_out.sum(axis=1) + new_cnt.sum(axis=(1, 2))
                ln[:na] += np.log(s)
                sc = np.where(s > 0, s, 1.0)
            out[:na] = new_out / sc[:, None]
            cnt[:na] = new_cnt / sc[:, None, None]
        return _finish(n, gj, ln, lh)


def log_probs(A, end, chunk_off, first, last, mask, min_len, joined=None):
    return Chain(A, end, chunk_off).log_probs(first, last, mask, min_len, joined)


def _chunk_paths(A, end_c, t0, T):
    """The weight of every path of the chunk at windows t0 .. t0+T-1, indexed by its code (window t in base-4 digit t); every row scaled
    by its largest entry first, so that no weight of a short chunk leaves the normal range."""
    w = A[t0, 0, :] / A[t0, 0, :].max()
    for t in range(1, T):
        At = A[t0 + t] / A[t0 + t].max()
        lastw = (np.arange(w.size) >> (2 * (t - 1))) & 3
        w = (w[None, :] * At[lastw, :].T).ravel()                          # code + s * 4^t
    lastw = (np.arange(w.size) >> (2 * (T - 1))) & 3
    return w * end_c[lastw]


def brute_force(A, end, chunk_off, first, last, mask, min_len, joined=None):
    """The same from the enumerated paths: chunks of at most 7 windows, groups of at most 10."""
    off = np.asarray(chunk_off, np.int64)
    first = np.asarray(first, np.int64).ravel()
    n = first.size
    mask = np.broadcast_to(np.asarray(mask, np.int64), first.shape)
    min_len = np.broadcast_to(np.asarray(min_len, np.int64), first.shape)
    groups = _groups(off, first, last, joined)
    tables = {}
    ln, lh = np.zeros(len(groups)), np.zeros(len(groups))
    for g, (j, parts) in enumerate(groups):
        prob = np.ones(1)
        T = 0
        for c, a, b in parts:
            t0, Tc = int(off[c]), int(off[c + 1] - off[c])
            assert Tc <= 7
            if (c, a, b) not in tables:
                w = _chunk_paths(A, end[c], t0, Tc)
                key = (np.arange(w.size) >> (2 * (a - t0))) & (4 ** (b - a + 1) - 1)
                tables[(c, a, b)] = np.bincount(key, weights=w, minlength=4 ** (b - a + 1))
            prob = np.multiply.outer(tables[(c, a, b)], prob).ravel()      # (the later part in the higher digits)
            T += b - a + 1
        assert T <= 10
        code = np.arange(4 ** T)
        run = np.zeros(code.size, np.int64)
        hit = np.zeros(code.size, bool)
        for t in range(T):
            inS = ((mask[j] >> ((code >> (2 * t)) & 3)) & 1).astype(bool)
            run = np.where(inS, run + 1, 0)
            hit |= run >= min_len[j]
        with np.errstate(divide="ignore"):
            ln[g] = np.log(prob[~hit].sum() / prob.sum())
            lh[g] = np.log(prob[hit].sum() / prob.sum())
    # (both sums are exact enough; the log of the larger one is taken from the smaller, as in _finish)
    return _finish(n, np.array([j for j, _ in groups], np.int64), ln, lh)
