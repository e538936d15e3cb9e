"""Test-side reference of the E-step under minimum run lengths (hf_estep_minlen): float64 numpy, written from the definition in
include/hmm_flagger_hip.h and not from the kernels.  The rows A_t and the end column come from sampling_ref.rows; F and B are the
expanded chain's forward and backward vectors of minlen_post_ref.forward_backward's recursions, kept per window here (that function
returns only their products), each window's vector divided by its largest entry: xi_adm is a ratio within one pair, so no scale
survives.

    p != s, or m_s == 1:  u_t[p][s] = F_{t-1}[(p, m_p)] A_t[p][s] B_t[(s, 1)]
    p == s, m_s > 1:      u_t[s][s] = sum_{d=2..m_s} c_d A_t[s][s] B_t[(s, d)],  c_d = F_{t-1}[(s, d-1)] (+ F_{t-1}[(s, m_s)] at d = m_s)
    xi_adm_t = u_t / sum(u_t)

The estimator accumulators are restated from SURVEY.md section 8, A12, over the pairs (w-1, w), w = 2..T-1 of every chunk, with
xi_adm_w[p][s] in the place of xi: per xi, r_c = xi p_c / sum_c p_c; x_adj = (x - alpha px) / (1 - alpha); mean: num += r_c x_adj,
den += r_c; var: num += r_c ((x_adj - mu_c)(1 - alpha))^2, den += r_c; weight: num_c += r_c, den of every component += r_c; Err as
truncated exponential: num += xi x, den += xi; transitions: count[p][s] += xi.  Element 0 is the sum of log Z_adm.

    lanes_fb(A, end, chunk_off, min_len)      -> F [N][lanes], B [N][lanes], log Z_adm [C]
    xi_adm(A, end, chunk_off, min_len)        -> xi [N][4][4] (zeros at a chunk's first window), post [N][4], log Z_adm [C]
    enumerate_pairs(weights, min_len)         -> mpf [T][4][4]: the pair marginals of a tiny chunk given admissibility, by enumeration
    stats(store, model, alpha, min_len, ...)  -> dict: vec, mag (the summed magnitudes of every element's terms), chunk [C][V], xi, lza, lz"""
from __future__ import annotations

import mpmath as mp
import numpy as np

from flagger_amd import _native as N
import minlen_ref
import sampling_ref
import viterbi_ref

PI = viterbi_ref.PI


def _norm(v):
    mx = v.max()
    return (v / mx, np.log(mx)) if mx > 0 else (v, 0.0)


def lanes_fb(A, end, chunk_off, min_len):
    m = [int(v) for v in min_len]
    ls, ld, ent, sat = minlen_ref.lanes(m)
    nl = ls.size
    off = np.asarray(chunk_off, np.int64)
    n = int(off[-1]) if off.size else 0
    F, B = np.zeros((n, nl)), np.zeros((n, nl))
    lza = np.zeros(max(off.size - 1, 0))
    for c in range(off.size - 1):
        t0, T = int(off[c]), int(off[c + 1] - off[c])
        if T <= 0:
            continue
        f = np.zeros(nl)
        f[sat] = A[t0, 0, :]
        f, logs = _norm(f)
        F[t0] = f
        for t in range(1, T):
            a = A[t0 + t]
            new = np.zeros(nl)
            for l in range(nl):
                s, d = int(ls[l]), int(ld[l])
                if d == 1:
                    v = 0.0
                    for p in range(4):
                        if not (m[s] > 1 and p == s):
                            v += f[sat[p]] * a[p, s]
                else:
                    v = f[l - 1] * a[s, s]
                    if d == m[s]:
                        v += f[l] * a[s, s]
                new[l] = v
            f, lg = _norm(new)
            logs += lg
            F[t0 + t] = f
        with np.errstate(divide="ignore"):
            lza[c] = np.log(np.sum(f * end[c][ls])) + logs
        b, _ = _norm(end[c][ls].astype(np.float64))
        B[t0 + T - 1] = b
        for t in range(T - 1, 0, -1):
            a = A[t0 + t]
            new = np.zeros(nl)
            for l in range(nl):
                s, d = int(ls[l]), int(ld[l])
                if d < m[s]:
                    new[l] = a[s, s] * b[l + 1]
                else:
                    v = a[s, s] * b[l] if m[s] > 1 else 0.0
                    for q in range(4):
                        if not (m[s] > 1 and q == s):
                            v += a[s, q] * b[ent[q]]
                    new[l] = v
            b, _ = _norm(new)
            B[t0 + t - 1] = b
    return F, B, lza


def xi_adm(A, end, chunk_off, min_len):
    m = [int(v) for v in min_len]
    ls, ld, ent, sat = minlen_ref.lanes(m)
    off = np.asarray(chunk_off, np.int64)
    n = int(off[-1]) if off.size else 0
    F, B, lza = lanes_fb(A, end, off, m)
    xi = np.zeros((n, 4, 4))
    post = np.zeros((n, 4))
    for c in range(off.size - 1):
        t0, T = int(off[c]), int(off[c + 1] - off[c])
        for t in range(T):
            g = np.zeros(4)
            np.add.at(g, ls, F[t0 + t] * B[t0 + t])
            post[t0 + t] = g / g.sum()
            if t == 0:
                continue
            a, f, b = A[t0 + t], F[t0 + t - 1], B[t0 + t]
            u = np.zeros((4, 4))
            for p in range(4):
                for s in range(4):
                    if p != s or m[s] == 1:
                        u[p, s] = f[sat[p]] * a[p, s] * b[ent[s]]
                    else:
                        v = 0.0
                        for d in range(2, m[s] + 1):
                            l = ent[s] + d - 1
                            cd = f[l - 1] + (f[l] if d == m[s] else 0.0)
                            v += cd * a[s, s] * b[l]
                        u[s, s] = v
            xi[t0 + t] = u / u.sum()
    return xi, post, lza


def enumerate_pairs(weights, min_len):
    """Pair marginals mpf[T][4][4] of minlen_ref.chunk_path_weights' list given admissibility (row 0: zeros)."""
    m = [int(v) for v in min_len]
    T = len(weights[0][0])
    zero = mp.mpf(0)
    pair = [[[zero] * 4 for _ in range(4)] for _ in range(T)]
    za = zero
    for path, w in weights:
        if not minlen_ref._path_ok(path, m):
            continue
        za += w
        for t in range(1, T):
            pair[t][path[t - 1]][path[t]] += w
    return [[[v / za for v in row] for row in mat] for mat in pair]


def stats_len(R, K):
    return 1 + R * (24 * K + 16)


def accumulate(store, model, alpha, xi, lza, K_ctx=None, adjust=True, min_frac=0.95):
    """(vec, mag, chunk [C][V]) of the estimator accumulators over the pairs (w-1, w), w = 2..T-1, with the counts xi[w][p][s]."""
    mt = model.modelType
    R = model.numberOfRegions
    K = model.maxNumberOfComps
    Kc = K if K_ctx is None else int(K_ctx)
    te = mt == N.HF_MODEL_TRUNC_EXP_GAUSSIAN
    alpha = np.asarray(alpha, np.float64)
    _, _, _, mean, var, weight = viterbi_ref._params(model)
    ncomp = [1, 1, 1, K]
    off = np.asarray(store.chunk_off, np.int64)
    C = off.size - 1
    V = stats_len(R, Kc)
    stride = 24 * Kc + 16
    chunk = np.zeros((C, V))
    cmag = np.zeros((C, V))
    chunk[:, 0] = lza
    cmag[:, 0] = np.abs(lza)
    n = int(off[-1]) if off.size else 0
    if n == 0:
        return chunk.sum(axis=0), cmag.sum(axis=0), chunk
    x = (np.asarray(store.cov, np.int64) & 0xff).astype(np.float64)
    reg = (np.asarray(store.annot, np.uint64) >> np.uint64(58)).astype(np.int64)
    bt = viterbi_ref.betas(store, adjust, min_frac)
    T = np.diff(off)
    cidx = np.repeat(np.arange(C), T)
    local = np.arange(n) - off[cidx]
    t = np.flatnonzero(local >= 2)                      # window w of the pair (w-1, w), w = 2..T-1
    ct, rt, xw, px, b = cidx[t], reg[t], x[t], x[t - 1], bt[t]

    def add(est_index, term):                           # est_index: the element's place behind a region's base, per pair
        i = 1 + rt * stride + est_index
        np.add.at(chunk, (ct, i), term)
        np.add.at(cmag, (ct, i), np.abs(term))

    def slot(s, est, which, c):
        return ((s * 3 + est) * 2 + which) * Kc + c

    for s in range(4):
        for p in range(4):
            k = xi[t, p, s]
            add(24 * Kc + p * 4 + s, k)
            if s == 0 and te:
                add(slot(0, 0, 0, 0), k * xw)
                add(slot(0, 0, 1, 0), k)
                continue
            a = alpha[p][s]
            x_adj = (xw - a * px) / (1 - a)
            nc = ncomp[s]
            pc = np.empty((nc, t.size))
            for cc in range(nc):
                mu, v = mean[rt, s, cc], var[rt, s, cc] * b
                d = xw - ((1 - a) * mu + a * px) * b
                with np.errstate(under="ignore"):
                    pc[cc] = np.maximum(weight[rt, s, cc] / np.sqrt(v * 2 * PI) * np.exp(-0.5 * d * d / v), 1e-40)
            tot = pc.sum(axis=0)
            for cc in range(nc):
                rc = k * pc[cc] / tot
                z = (x_adj - mean[rt, s, cc]) * (1 - a)
                add(slot(s, 0, 0, cc), rc * x_adj)
                add(slot(s, 0, 1, cc), rc)
                add(slot(s, 1, 0, cc), rc * z * z)
                add(slot(s, 1, 1, cc), rc)
                add(slot(s, 2, 0, cc), rc)
                for c2 in range(nc):                    # the weight estimator's denominator of every component
                    add(slot(s, 2, 1, c2), rc)
    return chunk.sum(axis=0), cmag.sum(axis=0), chunk


def stats(store, model, alpha, min_len, K_ctx=None, adjust=True, min_frac=0.95):
    A, end = sampling_ref.rows(store, model, alpha, adjust, min_frac)
    xi, post, lza = xi_adm(A, end, store.chunk_off, min_len)
    _, _, lz = lanes_fb(A, end, store.chunk_off, (1, 1, 1, 1))
    vec, mag, chunk = accumulate(store, model, alpha, xi, lza, K_ctx, adjust, min_frac)
    return {"vec": vec, "mag": mag, "chunk": chunk, "xi": xi, "post": post, "lza": lza, "lz": lz}


def close_stats(got, ref, mag, what="", rel=1e-9):
    """Every element within `rel` of its summed magnitude; prints the largest ratio first."""
    got, ref, mag = np.asarray(got), np.asarray(ref), np.asarray(mag)
    assert got.shape == ref.shape and not np.isnan(got).any(), what
    err = np.abs(got - ref)
    nz = mag > 0
    print("%s: largest deviation / summed magnitude %.3e over %d elements (bound %.0e)"
          % (what, float(np.max(err[nz] / mag[nz])) if nz.any() else 0.0, int(nz.sum()), rel))
    assert np.all(err <= rel * mag), (what, int(np.argmax(err - rel * mag)))
