"""Test-side reference of the most-probable-path decoder (hf_viterbi): float64 numpy, log domain, written from the definitions of
include/hmm_flagger_hip.h (SURVEY.md Appendix A for the emission, transition and beta), not from the kernels.

    first[s]     = trans[r_0][4][s] * e_0[s]                 (x_prev = 0, alpha = 0)
    A_t[pre][s]  = T_t[pre][s] * e_t[pre][s],  t >= 1        (region change => 1/5; else the validity-masked, renormalised row)
    end[s]       = trans[r_{T-1}][s][4]

`reference(store, model, ...)` runs a sequential Viterbi over all chunks at once (chunks side by side, window index in lockstep) with
first-max ties (np.argmax) and returns the labels, the chunk scores and `path_log_prob(labels)` -> per-chunk log-probability of any
labelling.  `tables(...)` exposes first / log A / end for the tests."""
from __future__ import annotations

import ctypes as C

import numpy as np

from flagger_amd import _native as N

PI = 3.14159          # common.h:15 (sic)
MAXC = N.HF_MAXCOMP
NX = N.HF_NB_MAX_COVERAGE + 1 if hasattr(N, "HF_NB_MAX_COVERAGE") else 251


def betas(store, adjust=True, min_frac=0.95):
    """Appendix A.2 (hmm.c:301-316), every window; int() truncation as the reference's min/max on int arguments."""
    off = np.asarray(store.chunk_off, np.int64)
    T = np.diff(off)
    if not adjust:
        return np.ones(int(off[-1]))
    c = np.repeat(np.arange(store.n_chunks), T)
    t = np.arange(int(off[-1])) - off[c]
    s = np.asarray(store.chunk_s, np.int64)[c].astype(np.float64)
    e = np.asarray(store.chunk_e, np.int64)[c].astype(np.float64)
    ctg = np.asarray(store.chunk_ctg_len, np.int64)[c].astype(np.float64)
    W, L = float(store.window_len), int(store.avg_alignment_len)
    if L == 0:
        return np.full(t.size, 0.25)
    mid = np.minimum(np.trunc(s + W * (t + 0.5)), np.trunc((s + W * t + e) / 2))
    lo = np.maximum(mid - L + 1, np.trunc(-(1 - min_frac) * L))
    hi = np.minimum(mid, np.trunc(ctg - min_frac * L))
    b = (hi - lo) / L
    return np.where(b <= 0.25, 0.25, b)


def _params(model):
    R = model.numberOfRegions
    v = model.param_vector().reshape(R, -1)
    trans = v[:, :25].reshape(R, 5, 5)
    lam, trunc = v[:, 25], v[:, 26]
    o = 27
    mean = v[:, o:o + 4 * MAXC].reshape(R, 4, MAXC); o += 4 * MAXC
    var = v[:, o:o + 4 * MAXC].reshape(R, 4, MAXC); o += 4 * MAXC
    weight = v[:, o:o + 4 * MAXC].reshape(R, 4, MAXC)
    return trans, lam, trunc, mean, var, weight


def tables(store, model, alpha, adjust=True, min_frac=0.95):
    """(logA [N][4][4] with the chunk-first windows' first[s] in row 0 and -inf elsewhere, log end [C][4], region per window)."""
    L = N.lib()
    mt = model.modelType
    R = model.numberOfRegions
    K = model.maxNumberOfComps
    trans, lam, trunc, mean, var, weight = _params(model)
    ncomp = [1, 1, 1, K]
    off = np.asarray(store.chunk_off, np.int64)
    n = int(off[-1])
    cov_full = np.asarray(store.cov, np.float64)
    x = (np.asarray(store.cov, np.int64) & 0xff).astype(np.float64)
    reg = (np.asarray(store.annot, np.uint64) >> np.uint64(58)).astype(np.int64)
    first = np.zeros(n, bool)
    first[off[:-1][np.diff(off) > 0]] = True
    px = np.where(first, 0.0, np.concatenate([[0.0], x[:-1]]))
    bt = betas(store, adjust, min_frac)
    alpha = np.asarray(alpha, np.float64)
    E = np.empty((n, 4, 4))                      # E[t][pre][s]
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        if mt == N.HF_MODEL_NEGATIVE_BINOMIAL:
            p = model.params()
            nbE = np.ctypeslib.as_array(p.nb_E, shape=(R * 4 * NX,)).reshape(R, 4, NX)
            e = nbE[reg[:, None], np.arange(4)[None, :], x.astype(np.int64)[:, None]]          # [n][4]
            E[:] = e[:, None, :]
        else:
            for s in range(4):
                for pre in range(4):
                    a = np.where(first, 0.0, alpha[pre][s])
                    if s == 0 and mt == N.HF_MODEL_TRUNC_EXP_GAUSSIAN:          # hmm_utils.c:941-947
                        lm, b = lam[reg] / bt, bt * trunc[reg]
                        val = lm * np.exp(-lm * x) / (1 - np.exp(-lm * b))
                        E[:, pre, s] = np.where(trunc[reg] < x, 0.0, val)
                        continue
                    tot = np.zeros(n)
                    for c in range(ncomp[s]):                                     # hmm_utils.c:753-793
                        mu = ((1 - a) * mean[reg, s, c] + a * px) * bt
                        vv = var[reg, s, c] * bt
                        pc = weight[reg, s, c] / np.sqrt(vv * 2 * PI) * np.exp(-0.5 * (x - mu) ** 2 / vv)
                        tot = tot + np.where(pc < 1e-40, 1e-40, pc)
                    E[:, pre, s] = tot
        # transitions (Appendix A.4, hmm_utils.c:2229-2292; hmm.c:398 region change)
        mapq = np.asarray(store.mapq, np.float64)
        clip = np.asarray(store.clip, np.float64)
        rm, rcl = mapq / (0.1 + cov_full), clip / (0.1 + cov_full)
        valid = np.stack([np.ones(n, bool), ~(rm > L.hfm_max_high_mapq_ratio(model._h)), np.ones(n, bool),
                          ~(rm < L.hfm_min_high_mapq_ratio(model._h)), ~(rcl < L.hfm_min_highly_clipped_ratio(model._h))], axis=1)
        tr = trans[reg][:, :4, :]                                                 # [n][pre][5]
        tot = (tr * valid[:, None, :]).sum(axis=2)
        Tc = np.where(valid[:, None, :4], tr[:, :, :4] / tot[:, :, None], 0.0)
        regchg = np.concatenate([[False], reg[1:] != reg[:-1]]) & ~first
        Tc[regchg] = 1.0 / 5
        A = Tc * E
        A[first] = 0.0
        A[first, 0, :] = trans[reg[first], 4, :4] * E[first, 0, :]
        logA = np.log(A)
        last = off[1:] - 1
        nonempty = np.diff(off) > 0
        logend = np.full((store.n_chunks, 4), -np.inf)
        logend[nonempty] = np.log(trans[reg[last[nonempty]], :4, 4])
    return logA, logend


def viterbi(logA, logend, chunk_off):
    """Sequential max-sum over every chunk (side by side), ties to the lowest state: (labels int8[N], chunk scores float64[C])."""
    off = np.asarray(chunk_off, np.int64)
    T = np.diff(off)
    C_ = T.size
    n = int(off[-1])
    labels = np.zeros(n, np.int8)
    score = np.zeros(C_)
    bp = np.zeros((n, 4), np.int8)
    if n == 0:
        return labels, score
    live = np.flatnonzero(T > 0)
    delta = logA[off[live], 0, :].copy()
    with np.errstate(invalid="ignore"):
        for k in range(1, int(T.max())):
            act = T[live] > k
            idx = off[live[act]] + k
            cand = delta[act][:, :, None] + logA[idx]          # [m][pre][s]
            b = np.argmax(cand, axis=1)
            bp[idx] = b
            delta[act] = np.take_along_axis(cand, b[:, None, :], axis=1)[:, 0, :]
        fin = delta + logend[live]
        s = np.argmax(fin, axis=1)
        score[live] = fin[np.arange(live.size), s]
        for k in range(int(T.max()) - 1, -1, -1):
            act = T[live] > k
            idx = off[live[act]] + k
            st = s[act]
            labels[idx] = st
            s[act] = bp[idx, st]
    return labels, score


def path_log_prob(logA, logend, chunk_off, labels):
    """log first[s_0] + sum_t log A_t[s_{t-1}][s_t] + log end[s_{T-1}] of every chunk, for any labelling."""
    off = np.asarray(chunk_off, np.int64)
    T = np.diff(off)
    n = int(off[-1])
    lab = np.asarray(labels, np.int64)
    prev = np.concatenate([[0], lab[:-1]])
    firstw = np.zeros(n, bool)
    firstw[off[:-1][T > 0]] = True
    prev[firstw] = 0
    terms = logA[np.arange(n), prev, lab]
    out = np.zeros(T.size)
    live = np.flatnonzero(T > 0)
    with np.errstate(invalid="ignore"):
        for c in live:
            out[c] = np.sum(terms[off[c]:off[c + 1]]) + logend[c, lab[off[c + 1] - 1]]
    return out


def reference(store, model, alpha, adjust=True, min_frac=0.95):
    """(labels, chunk scores, path_log_prob) of the whole store."""
    logA, logend = tables(store, model, alpha, adjust, min_frac)
    labels, score = viterbi(logA, logend, store.chunk_off)
    return labels, score, (lambda lab: path_log_prob(logA, logend, store.chunk_off, lab))
