"""Test-side reference of the exact path entropy and labelling log-probability (hf_get_path_entropy, hf_get_path_log_probs,
hf_get_entropy_profile): numpy, written from the definition in include/hmm_flagger_hip.h and not from the kernels.

A job is a window range first..last (global, inclusive); chunks are independent chains with the first / A / end of viterbi_ref.tables
(sampling_ref.rows in linear scale), and a job's value is the sum over its chunk-local parts [a, b], in chunk order.  Two routes, neither
of them the device's (a sum of per-window terms log(x / m) of the pair posterior over its row marginal):

    brute_force   (a) every one of the 4^T paths of a tiny chunk (sampling_ref.path_probs), marginalised to the sub-range: the entropy of
                      that table and the log of the labelled entry
    long_double   (b) log-partition minus expected log-weight in np.longdouble: the marginal of a sub-path is
                          f_a[y_a] prod_{t=a+1..b} A_t[y_{t-1}][y_t] b_b[y_b] / N
                      so the log-probability is that expression's log taken directly, and the entropy is
                          log N - E[log f_a[y_a]] - sum_t E[log A_t[y_{t-1}][y_t]] - E[log b_b[y_b]]
                      with the expectations under the singleton and pair posteriors of a long-double forward-backward, zeros skipped.
                      It takes log A, never log(x / m).
and, to size the tolerance of the device tests,
    chain_rule    the device's sums (marg_a + sum cond_t; log gamma_a[y_a] + sum log(x / m)) in float64, in the reference's order
    profile       (marg, cond) per window, the same way"""
from __future__ import annotations

import numpy as np

import interval_ref as IR
import runs_ref as RR
import sampling_ref as S


def _parts(chunk_off, first, last):
    first = np.asarray(first, np.int64).ravel()
    J, Cc, pa, pb, _ = IR.split(chunk_off, first, last, np.ones(first.size, np.int64))
    return first.size, J, Cc, pa, pb


def _sum_parts(n, J, vals):
    out = np.zeros(n)
    for j, v in zip(J, vals):          # chunk order
        out[j] += v
    return out


def _xlogx_sum(p):
    """- sum p log p over the last axes given, zeros skipped."""
    p = np.asarray(p)
    pos = p > 0
    return -(np.where(pos, p, 0) * np.log(np.where(pos, p, 1))).sum()


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def brute_force(A, end, chunk_off, first, last, labels=None):
    """Entropy (labels None) or the log-probability of labels[first..last], from the enumerated paths: chunks of at most 7 windows."""
    off = np.asarray(chunk_off, np.int64)
    n, J, Cc, pa, pb = _parts(off, first, last)
    cache = {}
    vals = []
    for c, a, b in zip(Cc, pa, pb):
        t0, T = int(off[c]), int(off[c + 1] - off[c])
        assert T <= 7
        if c not in cache:
            pp = S.path_probs(A, end[c], t0, T)
            cache[c] = (np.array(list(pp.keys()), np.int64).reshape(-1, T), np.array(list(pp.values())))
        paths, prob = cache[c]
        sub = paths[:, a - t0:b - t0 + 1]
        key = (sub * (4 ** np.arange(sub.shape[1]))[None, :]).sum(axis=1)
        table = np.bincount(key, weights=prob, minlength=4 ** sub.shape[1])
        if labels is None:
            vals.append(_xlogx_sum(table))
        else:
            y = np.asarray(labels[a:b + 1], np.int64)
            p = table[int((y * 4 ** np.arange(y.size)).sum())]
            vals.append(np.log(p) if p > 0 else -np.inf)
    return _sum_parts(n, J, vals)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
class LongDouble:
    """The per-window quantities of route (b), once per (A, end, chunk_off); then any number of job sets and labellings."""

    def __init__(self, A, end, chunk_off):
        LD = np.longdouble
        self.off = off = np.asarray(chunk_off, np.int64)
        n = int(off[-1])
        AL = A.astype(LD)
        al, be = RR.alpha_beta(A, end, off, LD)
        firstw = np.zeros(n, bool)
        firstw[off[:-1][np.diff(off) > 0]] = True
        prev = np.maximum(np.arange(n) - 1, 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.logA = np.log(AL)
            self.logal = np.log(al)
            self.logbe = np.log(be)
            u = al[prev][:, :, None] * AL                                  # [t][p][s] = al_{t-1}[p] A_t[p][s]
            self.logc = np.where(firstw, LD(0), np.log(u.sum(axis=(1, 2))))    # log of the forward's renormalisation at t
            xi = u * be[:, None, :]
            xi = xi / xi.sum(axis=(1, 2), keepdims=True)
            g = al * be
            self.dot = g.sum(axis=1)                                       # al_t . be_t
            g = g / self.dot[:, None]
            self.e_al = np.where(g > 0, g * np.where(g > 0, self.logal, 0), 0).sum(axis=1)      # E[log al_t[s_t]]
            self.e_be = np.where(g > 0, g * np.where(g > 0, self.logbe, 0), 0).sum(axis=1)      # E[log be_t[s_t]]
            self.e_A = np.where(xi > 0, xi * np.where(xi > 0, self.logA, 0), 0).sum(axis=(1, 2))   # E[log A_t[s_{t-1}][s_t]]
            self.e_A[firstw] = 0

    def _log_n(self, a, b):
        return self.logc[a + 1:b + 1].sum() + np.log(self.dot[b])

    def entropy(self, first, last):
        n, J, Cc, pa, pb = _parts(self.off, first, last)
        vals = [float(self._log_n(a, b) - self.e_al[a] - self.e_A[a + 1:b + 1].sum() - self.e_be[b]) for a, b in zip(pa, pb)]
        return _sum_parts(n, J, vals)

    def log_probs(self, first, last, labels):
        n, J, Cc, pa, pb = _parts(self.off, first, last)
        y = np.asarray(labels, np.int64)
        t = np.arange(y.size)
        step = self.logA[t, y[np.maximum(t - 1, 0)], y]                    # log A_t[y_{t-1}][y_t] (unused at a part's first window)
        vals = []
        with np.errstate(invalid="ignore"):
            for a, b in zip(pa, pb):
                v = self.logal[a, y[a]] + step[a + 1:b + 1].sum() + self.logbe[b, y[b]] - self._log_n(a, b)
                vals.append(float(v))
        return _sum_parts(n, J, vals)


# ---- the device's sums in float64 -----------------------------------------------------------------------------------------------------
def _local(A, end, chunk_off):
    """(gamma [N][4], x [N][4][4], m [N][4], first-window flags): the definition's per-window quantities in float64."""
    off = np.asarray(chunk_off, np.int64)
    n = int(off[-1])
    al, be = RR.alpha_beta(A, end, off)
    firstw = np.zeros(n, bool)
    firstw[off[:-1][np.diff(off) > 0]] = True
    g = al * be
    g = g / g.sum(axis=1, keepdims=True)
    prev = np.maximum(np.arange(n) - 1, 0)
    x = (al[prev][:, :, None] * A) * be[:, None, :]
    return g, x, x.sum(axis=2), firstw


def profile(A, end, chunk_off):
    """(marg [N], cond [N]) in float64; cond = marg at chunk-first windows."""
    g, x, m, firstw = _local(A, end, chunk_off)
    with np.errstate(divide="ignore", invalid="ignore"):
        marg = -np.where(g > 0, g * np.log(np.where(g > 0, g, 1)), 0).sum(axis=1)
        Z = m.sum(axis=1)
        r = np.where(x > 0, x / np.where(m > 0, m, 1)[:, :, None], 1)
        cond = -(np.where(x > 0, x, 0) / Z[:, None, None] * np.log(r)).sum(axis=(1, 2))
    return marg, np.where(firstw, marg, cond)


def chain_rule(A, end, chunk_off, first, last, labels=None):
    """Entropy (labels None) or log-probability per job as the device sums them, in float64."""
    off = np.asarray(chunk_off, np.int64)
    n, J, Cc, pa, pb = _parts(off, first, last)
    if labels is None:
        marg, cond = profile(A, end, off)
        return _sum_parts(n, J, [marg[a] + cond[a + 1:b + 1].sum() for a, b in zip(pa, pb)])
    g, x, m, _ = _local(A, end, off)
    y = np.asarray(labels, np.int64)
    t = np.arange(y.size)
    yp = y[np.maximum(t - 1, 0)]
    with np.errstate(divide="ignore", invalid="ignore"):
        xv, mv = x[t, yp, y], m[t, yp]
        step = np.where(xv > 0, np.log(np.where(xv > 0, xv / np.where(mv > 0, mv, 1), 1)), -np.inf)
        lg = np.where(g[t, y] > 0, np.log(np.where(g[t, y] > 0, g[t, y], 1)), -np.inf)
    return _sum_parts(n, J, [lg[a] + step[a + 1:b + 1].sum() for a, b in zip(pa, pb)])


# ---- the job sets and labellings of the tests ----------------------------------------------------------------------------------------
def tiny_ranges(chunk_off):
    """Every sub-range of every chunk of at most 7 windows, every small chunk with its neighbours (up to three chunks) and all small
    chunks together."""
    off = np.asarray(chunk_off, np.int64)
    small = [c for c in range(off.size - 1) if 0 < off[c + 1] - off[c] <= 7]
    F, L = [], []
    for c in small:
        for a in range(off[c], off[c + 1]):
            for b in range(a, off[c + 1]):
                F.append(a); L.append(b)
    for c in small:
        for d in (c + 1, c + 2):
            if d in small:
                F.append(off[c] + (off[c + 1] - off[c]) // 2); L.append(off[d + 1] - 1 - (off[d + 1] - off[d]) // 3)
    F.append(off[small[0]]); L.append(off[small[-1] + 1] - 1)
    return np.array(F, np.int64), np.array(L, np.int64)


def labellings(A, end, chunk_off, seed, n_drawn=3):
    """[(name, labels int64[N])]: the most probable path, paths drawn from the posterior, the four constant paths."""
    import viterbi_ref
    with np.errstate(divide="ignore"):
        vit, _ = viterbi_ref.viterbi(np.log(A), np.log(end), chunk_off)
    drawn, _, _ = S.ffbs(A, end, chunk_off, seed, list(range(n_drawn)))
    n = int(np.asarray(chunk_off)[-1])
    return ([("viterbi", vit.astype(np.int64))] + [("drawn %d" % k, drawn[k].astype(np.int64)) for k in range(n_drawn)]
            + [("constant %d" % k, np.full(n, k, np.int64)) for k in range(4)])
