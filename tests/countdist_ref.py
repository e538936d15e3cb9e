"""Test-side reference of the exact distribution of label totals (hf_get_count_distribution): numpy, by routes that are not the device's.

A job is a window range first..last (global, inclusive), a state mask S and, for the whole call, a count K.  N is the number of the
job's windows whose state lies in S; dist[j][k] = P(N = k | data) for k = 0..K and dist[j][K + 1] = P(N > K | data).  Chunks are
independent chains with the first / A / end of sampling_ref.rows; a job's parts are those of interval_ref.split.

    brute_force  (a) every one of the 4^T paths of a job of at most 10 windows in chunks of at most 7, a job over several chunks as the
                     product of its chunks' path distributions, the windows of S counted on the concatenated path
    joint        (b) np.longdouble, in the JOINT: the forward vector of the pass expanded by the counter, x[s][k], carried through the
                     rows A_t themselves with a rescaling per window and closed with the backward vector b_b; the parts convolved with
                     np.convolve.  Neither the posterior chain Q nor piece transfers nor the host's stitch are formed
    restated     (c) float64, the device's formulation: the posterior chain Q_u, gamma_a, the transfers of the pieces of the 512-window
                     grid, the chain's truncated convolutions with the running tail sum, the stitch (include/hmm_flagger_hip.h).  It
                     measures the deviation the formulation itself has from (a) and (b)."""
from __future__ import annotations

import numpy as np

import longrun_ref as LR
import runs_ref as RR

GRID = 512


def _bits(m):
    return ((int(m) >> np.arange(4)) & 1).astype(bool)


def _truncate(full, K):
    """The K + 2 bins of a distribution over 0 .. len - 1."""
    out = np.zeros(K + 2, full.dtype)
    n = min(full.size, K + 1)
    out[:n] = full[:n]
    out[K + 1] = full[K + 1:].sum()
    return out


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def fits_enumeration(chunk_off, first, last):
    """bool[n]: the job has at most 10 windows in chunks of at most 7 (route (a) applies)."""
    off = np.asarray(chunk_off, np.int64)
    first = np.asarray(first, np.int64).ravel()
    ok = np.ones(first.size, bool)
    for j, parts in LR._groups(off, first, last, None):
        (c, a, b), = parts
        if off[c + 1] - off[c] > 7:
            ok[j] = False
    ok &= (np.asarray(last, np.int64).ravel() - first + 1) <= 10
    return ok


def brute_force(A, end, chunk_off, first, last, mask, K):
    """float64[n][K + 2] from the enumerated paths."""
    off = np.asarray(chunk_off, np.int64)
    first = np.asarray(first, np.int64).ravel()
    mask = np.broadcast_to(np.asarray(mask, np.int64), first.shape)
    tables, prob, T = {}, {}, {}
    for j, parts in LR._groups(off, first, last, None):                    # (no joins: a group is a part)
        (c, a, b), = parts
        t0, Tc = int(off[c]), int(off[c + 1] - off[c])
        assert Tc <= 7
        if (c, a, b) not in tables:
            w = LR._chunk_paths(A, end[c], t0, Tc)
            key = (np.arange(w.size) >> (2 * (a - t0))) & (4 ** (b - a + 1) - 1)
            tables[(c, a, b)] = np.bincount(key, weights=w, minlength=4 ** (b - a + 1))
        prob[j] = np.multiply.outer(tables[(c, a, b)], prob.get(j, np.ones(1))).ravel()      # (the later part in the higher digits)
        T[j] = T.get(j, 0) + b - a + 1
    out = np.zeros((first.size, K + 2))
    for j in range(first.size):
        assert T[j] <= 10
        p = prob[j] / prob[j].sum()
        code = np.arange(4 ** T[j])
        cnt = np.zeros(code.size, np.int64)
        for t in range(T[j]):
            cnt += (mask[j] >> ((code >> (2 * t)) & 3)) & 1
        out[j] = _truncate(np.bincount(cnt, weights=p, minlength=T[j] + 1), K)
    return out


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
class Joint:
    """Route (b), once per (A, end, chunk_off): the normalised forward and backward vectors in long double; then any number of job sets."""

    def __init__(self, A, end, chunk_off):
        self.off = np.asarray(chunk_off, np.int64)
        self.A = A.astype(np.longdouble)
        self.al, self.be = RR.alpha_beta(A, end, self.off, dtype=np.longdouble)

    def part(self, a, b, inS, K):
        """longdouble[K + 2] of the part [a, b]: bins above K are gathered in the last one while walking (sums only)."""
        ld = np.longdouble
        B = min(b - a + 1, K + 1) + 1                                      # counts 0 .. B - 2, and "more" at B - 1
        x = np.zeros((4, B), ld)
        x[inS, 1] = self.al[a][inS]
        x[~inS, 0] = self.al[a][~inS]
        for t in range(a + 1, b + 1):
            w = self.A[t].T @ x                                            # w[q][k] = sum_p x[p][k] A_t[p][q]
            up = w[inS]
            w[inS, 1:] = up[:, :-1]
            w[inS, 0] = 0
            w[inS, B - 1] += up[:, B - 1]
            x = w / w.sum()
        d = (x * self.be[b][:, None]).sum(axis=0)
        d = d / d.sum()
        out = np.zeros(K + 2, ld)
        if B - 1 == K + 1:
            out[:] = d
        else:                                                              # T <= K: the "more" bin of the walk is the count T itself
            out[:B] = d
        return out

    def distribution(self, first, last, mask, K):
        ld = np.longdouble
        first = np.asarray(first, np.int64).ravel()
        mask = np.broadcast_to(np.asarray(mask, np.int64), first.shape)
        out = np.zeros((first.size, K + 2), ld)
        seen = set()
        for j, parts in LR._groups(self.off, first, last, None):
            (c, a, b), = parts
            d = self.part(a, b, _bits(mask[j]), K)
            if j not in seen:
                out[j] = d
                seen.add(j)
            else:
                full = np.convolve(out[j][:K + 1], d[:K + 1])
                more = out[j][K + 1] * d.sum() + out[j][:K + 1].sum() * d[K + 1]
                out[j] = _truncate(full, K)
                out[j][K + 1] += more
        return out


def joint(A, end, chunk_off, first, last, mask, K):
    return Joint(A, end, chunk_off).distribution(first, last, mask, K)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def fold(v, M, K):
    """The two sums of the header: v [.., K + 2] into M [.., K + 2] -> [.., K + 2] (leading axes broadcast).  Bin k <= K takes its terms
    in increasing j from 0.0; the tail sums r_j run downwards from M[K + 1] (np.cumsum adds in sequence)."""
    v, M = np.broadcast_arrays(np.asarray(v, np.float64), np.asarray(M, np.float64))
    out = np.zeros(v.shape)
    for j in range(K + 1):
        out[..., j:K + 1] += v[..., j:j + 1] * M[..., :K + 1 - j]
    r = np.cumsum(M[..., ::-1], axis=-1)
    for j in range(K + 2):
        out[..., K + 1] += v[..., j] * r[..., j]
    return out


class Restated:
    """Route (c), once per (A, end, chunk_off): the posterior chain Q and gamma in float64."""

    def __init__(self, A, end, chunk_off):
        self.off = np.asarray(chunk_off, np.int64)
        self.al, self.be = RR.alpha_beta(A, end, self.off)
        y = A * self.be[:, None, :]
        den = y.sum(axis=2, keepdims=True)
        self.Q = np.where(den > 0, y / np.where(den > 0, den, 1.0), 0.0)
        g = self.al * self.be
        tot = g.sum(axis=1, keepdims=True)
        self.g = np.where(tot > 0, g / np.where(tot > 0, tot, 1.0), 0.0)

    def transfer(self, t0, t1, inS, K):
        """M[p][q][k] of the windows t0 .. t1."""
        M = np.zeros((4, 4, K + 2))
        M[np.arange(4), np.arange(4), 0] = 1.0
        for u in range(t0, t1 + 1):
            W = np.einsum("pak,aq->pqk", M, self.Q[u])
            up = W[:, inS, :].copy()
            W[:, inS, 1:K + 1] = up[:, :, :K]
            W[:, inS, 0] = 0.0
            W[:, inS, K + 1] = up[:, :, K + 1] + up[:, :, K]
            M = W
        return M

    def part(self, a, b, inS, K):
        v = np.zeros((4, K + 2))
        v[inS, 1] = self.g[a][inS]
        v[~inS, 0] = self.g[a][~inS]
        t = a + 1
        while t <= b:
            e = min(b, (t // GRID + 1) * GRID - 1)
            M = self.transfer(t, e, inS, K)
            c = fold(v[:, None, :], M, K)                                  # c[p][q][k]
            v = ((c[0] + c[1]) + c[2]) + c[3]
            t = e + 1
        return v.sum(axis=0)

    def distribution(self, first, last, mask, K):
        first = np.asarray(first, np.int64).ravel()
        mask = np.broadcast_to(np.asarray(mask, np.int64), first.shape)
        out = np.zeros((first.size, K + 2))
        seen = set()
        for j, parts in LR._groups(self.off, first, last, None):
            (c, a, b), = parts
            d = self.part(a, b, _bits(mask[j]), K)
            out[j] = fold(out[j], d, K) if j in seen else d
            seen.add(j)
        return out


def restated(A, end, chunk_off, first, last, mask, K):
    return Restated(A, end, chunk_off).distribution(first, last, mask, K)


def stitch(parts, K):
    """The host's stitch over the K + 2 bins of a job's parts, in order (the sums of the header)."""
    acc = np.array(parts[0], np.float64)
    for d in parts[1:]:
        acc = fold(acc, np.asarray(d, np.float64), K)
    return acc
