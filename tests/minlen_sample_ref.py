"""Test-side reference of the admissible path sampler (hf_sample_paths_minlen): float64 numpy, written from the definition in
include/hmm_flagger_hip.h, not from the kernels.  Built on viterbi_ref.tables (exp of them, as sampling_ref.rows), minlen_ref.lanes and
sampling_ref's splitmix64 / sample_key / uniforms.

    tables(A, end, chunk_off, min_len)        the forward over the expanded chain in the linear domain, every window's vector scaled by a
                                              power of two only (sampling_ref._norm), and from it every draw's weights and left-to-right
                                              cumulative sums: with all lengths 1 the numbers sampling_ref.forward forms, bit for bit
    sample(tab, seed, ks, n_windows=None)     backward sampling by the draw rule: (labels int8[K][N], window margins float32[K][N] of the
                                              draw actually taken on the path (1 where the path takes none: a chunk's first window, a
                                              lane 1 < d < m), final margins float32[K][C]); margin = min_i |x - c_i| / c_{n-1}
    path_prob(tab, c, path)                   the product of the conditional draw probabilities of one path of chunk c, from the weights
                                              (0.0 for a path the walk cannot produce)"""
from __future__ import annotations

import numpy as np

import minlen_ref
import sampling_ref as S


def _pick(W, Cm, u):
    """The draw rule over n slots, vectorised: W, Cm [m][n], u [m] -> (choice [m], margin [m])."""
    n = W.shape[1]
    x = u * Cm[:, n - 1]
    below = x[:, None] < Cm
    choice = np.where(below.any(axis=1), np.argmax(below, axis=1), -1)
    pos = W > 0
    last_pos = np.where(pos.any(axis=1), n - 1 - np.argmax(pos[:, ::-1], axis=1), 0)
    choice = np.where(choice >= 0, choice, last_pos)
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.min(np.abs(x[:, None] - Cm), axis=1) / Cm[:, n - 1]
    return choice.astype(np.int64), margin


def _scale(v):
    """Every row of v by 2^-e, e = ilogb of its largest entry (0 when that is 0 or not finite)."""
    m = v.max(axis=-1)
    ok = (m > 0) & np.isfinite(m)
    e = np.where(ok, np.frexp(np.where(ok, m, 1.0))[1] - 1, 0)
    return np.ldexp(v, -e[..., None])


def _cumsum(w):
    """Left-to-right cumulative sums along the last axis, c_0 = w_0."""
    c = np.empty_like(w)
    c[..., 0] = w[..., 0]
    for i in range(1, w.shape[-1]):
        c[..., i] = c[..., i - 1] + w[..., i]
    return c


def tables(A, end, chunk_off, min_len):
    """dict: m, off, W4/C4 [N][s][p] (the entry lane of s: its predecessor's saturated lane), W2/C2 [N][s][2] (the saturated lane of s:
    arrived, stayed), fw/fc [C][lanes] (the final lane).  Rows of chunk-first windows stay 0."""
    m = [int(v) for v in min_len]
    ls, ld, ent, sat = minlen_ref.lanes(m)
    nl = ls.size
    off = np.asarray(chunk_off, np.int64)
    T = np.diff(off)
    n = int(off[-1]) if off.size else 0
    W4 = np.zeros((n, 4, 4)); W2 = np.zeros((n, 4, 2))
    fw = np.zeros((T.size, nl))
    live = np.flatnonzero(T > 0)
    tab = dict(m=m, off=off)
    if live.size:
        o, Tl = off[live], T[live]
        Fp = np.zeros((live.size, nl))
        Fp[:, sat] = A[o, 0, :]
        Fp = S._norm(Fp)
        inner = np.flatnonzero(ld > 1)
        ar4 = np.arange(4)
        below = np.where(np.asarray(m) > 1, sat - 1, 0)
        has_below = np.asarray(m) > 1
        for k in range(1, int(Tl.max())):
            act = np.flatnonzero(Tl > k)
            idx = o[act] + k
            At = A[idx]                                            # [a][pre][s]
            fp = Fp[act]
            # the eight values the draws read, scaled by the largest of them
            eight = _scale(np.concatenate([fp[:, sat], np.where(has_below[None, :], fp[:, below], 0.0)], axis=1))
            fs, fb = eight[:, :4], eight[:, 4:]
            w4 = fs[:, None, :] * np.transpose(At, (0, 2, 1))      # [a][s][p]
            for s in range(4):
                if m[s] > 1:
                    w4[:, s, s] = 0.0
            diag = At[:, ar4, ar4]
            W4[idx] = w4
            W2[idx] = np.stack([fb * diag, fs * diag], axis=2)
            # the forward step (hf_minlen_posterior's sums: ((v_0 + v_1) + v_2) + v_3; up + stay)
            v = fp[:, sat][:, None, :] * np.transpose(At, (0, 2, 1))
            for s in range(4):
                if m[s] > 1:
                    v[:, s, s] = 0.0
            new = np.zeros_like(fp)
            new[:, ent] = _cumsum(v)[:, :, 3]
            new[:, inner] = fp[:, inner - 1] * diag[:, ls[inner]]
            for s in range(4):
                if m[s] > 1:
                    new[:, sat[s]] = fp[:, sat[s] - 1] * diag[:, s] + fp[:, sat[s]] * diag[:, s]
            Fp[act] = S._norm(new)
        fw[live] = _scale(Fp) * end[live][:, ls]
    tab.update(W4=W4, C4=_cumsum(W4), W2=W2, C2=_cumsum(W2), fw=fw, fc=_cumsum(fw))
    return tab


def sample(tab, seed, ks, n_windows=None):
    """Samples `ks` (absolute indices), vectorised over samples and chunks."""
    m, off = np.asarray(tab["m"]), tab["off"]
    ls, ld, ent, sat = minlen_ref.lanes(tab["m"])
    T = np.diff(off)
    C_ = T.size
    n = (int(off[-1]) if off.size else 0) if n_windows is None else int(n_windows)
    keys = np.array([S.sample_key(seed, k) for k in ks], np.uint64)
    K = keys.size
    labels = np.zeros((K, n), np.int8)
    marg = np.ones((K, n), np.float32)
    fmarg = np.ones((K, C_), np.float32)
    live = np.flatnonzero(T > 0)
    if n == 0 or live.size == 0:
        return labels, marg, fmarg
    a = live.size
    nl = ls.size
    uf = S.uniforms(0, keys[:, None] + np.uint64(n) + live[None, :].astype(np.uint64))       # [K][a]
    fl, fm = _pick(np.broadcast_to(tab["fw"][live], (K, a, nl)).reshape(-1, nl), np.broadcast_to(tab["fc"][live], (K, a, nl)).reshape(-1, nl),
                   uf.ravel())
    fmarg[:, live] = fm.reshape(K, a)
    cs, cd = ls[fl].reshape(K, a), ld[fl].reshape(K, a)
    W4, C4, W2, C2 = tab["W4"], tab["C4"], tab["W2"], tab["C2"]
    for q in range(int(T.max()) - 1, -1, -1):
        act = np.flatnonzero(T[live] > q)
        idx = off[live[act]] + q
        s, d = cs[:, act], cd[:, act]                                                        # [K][a']
        labels[:, idx] = s
        if q == 0:
            continue
        u = S.uniforms(0, keys[:, None] + idx[None, :].astype(np.uint64))
        ii = np.broadcast_to(idx[None, :], s.shape)
        p4, m4 = _pick(W4[ii, s].reshape(-1, 4), C4[ii, s].reshape(-1, 4), u.ravel())
        p2, m2 = _pick(W2[ii, s].reshape(-1, 2), C2[ii, s].reshape(-1, 2), u.ravel())
        p4, m4, p2, m2 = (x.reshape(s.shape) for x in (p4, m4, p2, m2))
        entry, satd = d == 1, (d == m[s]) & (m[s] > 1)
        marg[:, idx] = np.where(entry, m4, np.where(satd, m2, 1.0))
        cs[:, act] = np.where(entry, p4, s)
        cd[:, act] = np.where(entry, m[p4], np.where(satd & (p2 == 1), d, d - 1))
    return labels, marg, fmarg


def reference(store, model, alpha, min_len, seed, ks):
    """(labels, window margins, final margins) of the whole store."""
    A, end = S.rows(store, model, alpha)
    return sample(tables(A, end, store.chunk_off, min_len), seed, ks, store.n_windows)


def path_prob(tab, c, path):
    """The probability with which `sample` draws `path` (labels of chunk c), from the weights alone."""
    m, off = tab["m"], tab["off"]
    ls, ld, ent, sat = minlen_ref.lanes(m)
    t0, T = int(off[c]), len(path)
    # the lanes of the path: the first run saturated, every later run counts from 1 up to m
    d = []
    for t, s in enumerate(path):
        if t == 0:
            d.append(m[s])
        elif s == path[t - 1]:
            d.append(min(d[-1] + 1, m[s]))
        else:
            d.append(1)
    fc = tab["fc"][c]
    tot = fc[-1]
    if not tot > 0:
        return 0.0
    pr = tab["fw"][c][ent[path[-1]] + d[-1] - 1] / tot
    for t in range(T - 1, 0, -1):
        s, p = path[t], path[t - 1]
        if d[t] == 1:
            if d[t - 1] != m[p] or not tab["C4"][t0 + t, s, 3] > 0:
                return 0.0
            pr *= tab["W4"][t0 + t, s, p] / tab["C4"][t0 + t, s, 3]
        elif d[t] == m[s]:
            if not tab["C2"][t0 + t, s, 1] > 0:
                return 0.0
            pr *= tab["W2"][t0 + t, s, 1 if d[t - 1] == m[s] else 0] / tab["C2"][t0 + t, s, 1]
    return float(pr)
