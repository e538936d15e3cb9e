"""Test-side reference of the exact block-length spectrum (hf_get_run_lengths): numpy, by routes that are not the device's.

A job is a window range first..last (global, inclusive), a state mask S and, for the whole call, a length L; `joined` [n_chunks] says
which chunks continue the chunk before.  The job's parts fall into groups of joined parts (longrun_ref._groups); a run is a maximal
stretch of windows in S of a group's concatenated sequence.  spectrum[j][l - 1] = E[runs of exactly l windows], l = 1..L,
spectrum[j][L] = E[runs of more than L windows], summed over the job's groups.  Chunks are independent chains with the first / A / end
of sampling_ref.rows.

    brute_force  (a) every one of the 4^T paths of a group of at most 10 windows (chunks of at most 7), a joined group as the product of
                     its chunks' path distributions, the runs counted on the concatenated path
    joint        (b) np.longdouble, in the JOINT: a joined group is walked as ONE chain whose boundary step is the rank-one row
                     b_b[p] f_a'[s] of hf_get_long_run_log_probs; the probability that a run covers exactly the windows i..j is the
                     constrained product f_{i-1}(not S) A_i(S) prod A_SS A_{j+1}(not S) b_{j+1} over the chain's total weight, with the
                     scales of a normalised forward-backward.  Neither the posterior chain Q nor the host's stitch is formed
    restated     (c) float64, the device's formulation: the posterior chain Q_u, the start masses sigma_t, the per-part walk, the
                     stitch (include/hmm_flagger_hip.h).  It measures the deviation the formulation itself has from (a) and (b).
Routes (b) and (c) advance every start window of a group (of a part) together, one age at a time: O(windows L) per job."""
from __future__ import annotations

import numpy as np

import longrun_ref as LR
import runs_ref as RR


def _bits(m):
    return ((int(m) >> np.arange(4)) & 1).astype(bool)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
def brute_force(A, end, chunk_off, first, last, mask, L, joined=None):
    """float64[n][L + 1] from the enumerated paths: chunks of at most 7 windows, groups of at most 10."""
    off = np.asarray(chunk_off, np.int64)
    first = np.asarray(first, np.int64).ravel()
    mask = np.broadcast_to(np.asarray(mask, np.int64), first.shape)
    out = np.zeros((first.size, L + 1))
    tables = {}
    for j, parts in LR._groups(off, first, last, joined):
        prob = np.ones(1)
        T = 0
        for c, a, b in parts:
            t0, Tc = int(off[c]), int(off[c + 1] - off[c])
            assert Tc <= 7
            if (c, a, b) not in tables:
                w = LR._chunk_paths(A, end[c], t0, Tc)
                key = (np.arange(w.size) >> (2 * (a - t0))) & (4 ** (b - a + 1) - 1)
                tables[(c, a, b)] = np.bincount(key, weights=w, minlength=4 ** (b - a + 1))
            prob = np.multiply.outer(tables[(c, a, b)], prob).ravel()      # (the later part in the higher digits)
            T += b - a + 1
        assert T <= 10
        prob = prob / prob.sum()
        code = np.arange(4 ** T)
        run = np.zeros(code.size, np.int64)
        spec = np.zeros(L + 1)
        for t in range(T + 1):
            inS = ((mask[j] >> ((code >> (2 * t)) & 3)) & 1).astype(bool) if t < T else np.zeros(code.size, bool)
            ended = ~inS & (run > 0)
            np.add.at(spec, np.minimum(run[ended], L + 1) - 1, prob[ended])
            run = np.where(inS, run + 1, 0)
        out[j] += spec
    return out


def groups_fit_enumeration(chunk_off, first, last, joined=None):
    """bool[n]: every group of the job has at most 10 windows in chunks of at most 7 (route (a) applies)."""
    off = np.asarray(chunk_off, np.int64)
    first = np.asarray(first, np.int64).ravel()
    ok = np.ones(first.size, bool)
    for j, parts in LR._groups(off, first, last, joined):
        if sum(b - a + 1 for _, a, b in parts) > 10 or any(off[c + 1] - off[c] > 7 for c, _, _ in parts):
            ok[j] = False
    return ok


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
class Joint:
    """Route (b), once per (A, end, chunk_off): the normalised forward and backward vectors in long double; then any number of job sets."""

    def __init__(self, A, end, chunk_off):
        ld = np.longdouble
        self.off = off = np.asarray(chunk_off, np.int64)
        n = int(off[-1])
        self.al, self.be = RR.alpha_beta(A, end, off, dtype=ld)
        prev = np.maximum(np.arange(n) - 1, 0)
        AL = A.astype(ld)
        c = (self.al[prev][:, :, None] * AL).sum(axis=(1, 2))              # the scale of the step into t (a chunk's first window: unused)
        self.Mn = AL / np.where(c > 0, c, 1)[:, None, None]
        self.ab = (self.al * self.be).sum(axis=1)
        self.psi = self.be / np.where(self.ab > 0, self.ab, 1)[:, None]    # al_t . psi_t = 1

    def spectrum(self, first, last, mask, L, joined=None):
        ld = np.longdouble
        first = np.asarray(first, np.int64).ravel()
        mask = np.broadcast_to(np.asarray(mask, np.int64), first.shape)
        out = np.zeros((first.size, L + 1), ld)
        for j, parts in LR._groups(self.off, first, last, joined):
            inS = _bits(mask[j])
            win = np.concatenate([np.arange(a, b + 1) for _, a, b in parts])
            T = win.size
            Mn = self.Mn[win]                                              # the step INTO place u (place 0: unused)
            p = 0
            for k, (_, a, b) in enumerate(parts):
                if k > 0:                                                  # the rank-one boundary row, with its scale al_b . be_b
                    pb = parts[k - 1][2]
                    Mn[p] = np.multiply.outer(self.be[pb], self.al[a]) / self.ab[pb]
                p += b - a + 1
            phi, psi = self.al[win], self.psi[win]
            v = np.zeros((T, 4), ld)
            v[0] = phi[0] * inS
            if T > 1:
                v[1:] = np.einsum("ip,ipq->iq", phi[:-1] * ~inS, Mn[1:]) * inS
            start = np.arange(T)
            N = np.zeros(L + 1, ld)
            for d in range(1, L + 2):
                if start.size == 0:
                    break
                u = start + d - 1
                if d == L + 1:                                             # still in S at age L + 1: saturated
                    N[L] += (v * psi[u]).sum()
                    break
                if u[-1] == T - 1:                                         # open at the group's last window
                    N[d - 1] += (v[-1] * psi[T - 1]).sum()
                    start, v, u = start[:-1], v[:-1], u[:-1]
                    if start.size == 0:
                        break
                w = np.einsum("ip,ipq->iq", v, Mn[u + 1])
                N[d - 1] += (w * ~inS * psi[u + 1]).sum()
                v = w * inS
            out[j] += N
        return out


def joint(A, end, chunk_off, first, last, mask, L, joined=None):
    return Joint(A, end, chunk_off).spectrum(first, last, mask, L, joined)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def stitch_part(state, x, T, L):
    """One part into the stitch of include/hmm_flagger_hip.h: state = [o (L), O, N (L + 1)], x = (I, Lc, Rc, W, s, e)."""
    o, O, N = state
    I, Lc, Rc, W, s, e = x
    N += I
    N[:L] += o * (1.0 - s)
    N += (1.0 - O) * Lc
    if o.any():                                                            # (index k, l: lengths k + 1, l + 1 merge into k + l + 2)
        idx = np.minimum(np.add.outer(np.arange(L), np.arange(L + 1)) + 1, L)
        N += np.bincount(idx.ravel(), weights=np.multiply.outer(o, Lc).ravel(), minlength=L + 1)
    on = np.zeros(L)
    if T <= L:
        on[T - 1] += (1.0 - O) * W
        on[T:] += o[:L - T] * W
        N[L] += o[L - T:].sum() * W
    on += Rc
    return [on, e, N]


class Restated:
    """Route (c), once per (A, end, chunk_off): the posterior chain Q and the pair weights in float64."""

    def __init__(self, A, end, chunk_off):
        self.off = off = np.asarray(chunk_off, np.int64)
        n = int(off[-1])
        self.A = A
        self.al, self.be = RR.alpha_beta(A, end, off)
        y = A * self.be[:, None, :]
        den = y.sum(axis=2, keepdims=True)
        self.Q = np.where(den > 0, y / np.where(den > 0, den, 1.0), 0.0)
        prev = np.maximum(np.arange(n) - 1, 0)
        self.z = (self.al[prev][:, :, None] * A) * self.be[:, None, :]      # [t][p][s] (a chunk's first window: unused)
        g = self.al * self.be
        self.g = g / g.sum(axis=1, keepdims=True)

    def part(self, a, b, inS, L):
        """(I [L + 1], Lc [L + 1], Rc [L], W, s, e) of the part [a, b]."""
        T = b - a + 1
        z = self.z[a:b + 1]
        tot = z.sum(axis=(1, 2))
        v = np.where(tot[:, None] > 0, (z * ~inS[None, :, None]).sum(axis=1) / np.where(tot > 0, tot, 1.0)[:, None], 0.0) * inS
        v[0] = self.g[a] * inS
        I, Lc, Rc, W = np.zeros(L + 1), np.zeros(L + 1), np.zeros(L), 0.0
        start = np.arange(T)
        for d in range(1, L + 2):
            if start.size == 0:
                break
            if d == L + 1:
                sat = v.sum(axis=1)
                Lc[L] += sat[start == 0].sum()
                I[L] += sat[start != 0].sum()
                break
            if start[-1] + d - 1 == T - 1:
                if start[-1] == 0:
                    W = v[-1].sum()
                else:
                    Rc[d - 1] = v[-1].sum()
                start, v = start[:-1], v[:-1]
                if start.size == 0:
                    break
            w = np.einsum("ip,ipq->iq", v, self.Q[a + start + d])
            ex = (w * ~inS).sum(axis=1)
            Lc[d - 1] += ex[start == 0].sum()
            I[d - 1] += ex[start != 0].sum()
            v = w * inS
        return I, Lc, Rc, W, float((self.g[a] * inS).sum()), float((self.g[b] * inS).sum())

    def spectrum(self, first, last, mask, L, joined=None):
        first = np.asarray(first, np.int64).ravel()
        mask = np.broadcast_to(np.asarray(mask, np.int64), first.shape)
        out = np.zeros((first.size, L + 1))
        for j, parts in LR._groups(self.off, first, last, joined):
            inS = _bits(mask[j])
            state = [np.zeros(L), 0.0, np.zeros(L + 1)]
            for _, a, b in parts:
                state = stitch_part(state, self.part(a, b, inS, L), b - a + 1, L)
            state[2][:L] += state[0]
            out[j] += state[2]
        return out


def restated(A, end, chunk_off, first, last, mask, L, joined=None):
    return Restated(A, end, chunk_off).spectrum(first, last, mask, L, joined)
