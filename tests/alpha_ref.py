"""Test-side reference of the alpha statistics (hf_get_alpha_stats): float64 numpy, written from the definitions of
include/hmm_flagger_hip.h and not from the kernels.  The rows A_t and the end column come from viterbi_ref.tables through
sampling_ref.rows; f (normalised to sum 1, with the scales) and b (b_{T-1} = end / scale_{T-1}, b_t = A_{t+1} b_{t+1} / scale_t) are the
reference's scaled forward and backward vectors, what hf_get_forward_backward returns.

    xi_t[p][s] = f_{t-1}[p] A_t[p][s] b_t[s] / 1e-4                       for every pair (t-1, t) of a chunk, t >= 1
    G[r][p][s] = sum_t xi_t[p][s] sum_c g_c phi_c d_c u_c / v_c
    H[r][p][s] = sum_t xi_t[p][s] sum_c g_c phi_c u_c^2 / v_c

    stats(store, model, alpha)        -> dict: G, H, Gabs (the sum of G with |d_c u_c|) [R][4][4], count [R][4][4] (sum of xi over the
                                         pairs t >= 2: the countMatrix of the statistics vector), ll (sum of log scale)
    loglik(store, model, alpha)       -> sum of log scale
    alpha_step(alpha, st, mask, lo, hi) -> the conditional maximiser alpha + G / H of every free entry with H > 0 and 10 < count, clamped
    simulate(...)                     -> a WindowStore drawn from the model definition with a known alpha"""
from __future__ import annotations

import numpy as np

import sampling_ref
import viterbi_ref
from flagger_amd import _native as N
from flagger_amd import synth

PI = viterbi_ref.PI
TERMINATION = 1e-4          # HF_TERMINATION_PROB, hf_device.h


def forward(A, chunk_off):
    """(f [N][4] normalised to sum 1, scale [N]) — chunks side by side, window index in lockstep."""
    off = np.asarray(chunk_off, np.int64)
    T = np.diff(off)
    n = int(off[-1])
    f = np.zeros((n, 4))
    sc = np.ones(n)
    if n == 0:
        return f, sc
    live = np.flatnonzero(T > 0)
    for k in range(int(T.max())):
        act = live[T[live] > k]
        idx = off[act] + k
        w = A[idx, 0, :] if k == 0 else np.einsum("mp,mps->ms", f[idx - 1], A[idx])
        s = w.sum(axis=1)
        sc[idx] = s
        f[idx] = w / s[:, None]
    return f, sc


def backward(A, end, sc, chunk_off):
    off = np.asarray(chunk_off, np.int64)
    T = np.diff(off)
    n = int(off[-1])
    b = np.zeros((n, 4))
    if n == 0:
        return b
    live = np.flatnonzero(T > 0)
    last = off[live + 1] - 1
    b[last] = end[live] / sc[last][:, None]
    for k in range(1, int(T.max())):
        act = live[T[live] > k]
        idx = off[act + 1] - 1 - k                       # window T-1-k of every chunk long enough
        b[idx] = np.einsum("mps,ms->mp", A[idx + 1], b[idx + 1]) / sc[idx][:, None]
    return b


def loglik(store, model, alpha, adjust=True, min_frac=0.95):
    A, _ = sampling_ref.rows(store, model, alpha, adjust, min_frac)
    _, sc = forward(A, store.chunk_off)
    return float(np.sum(np.log(sc)))


def stats(store, model, alpha, adjust=True, min_frac=0.95, skip_first_pair=False):
    mt = model.modelType
    R = model.numberOfRegions
    K = model.maxNumberOfComps
    alpha = np.asarray(alpha, np.float64)
    _, _, _, mean, var, weight = viterbi_ref._params(model)
    ncomp = [1, 1, 1, K]
    off = np.asarray(store.chunk_off, np.int64)
    n = int(off[-1])
    A, end = sampling_ref.rows(store, model, alpha, adjust, min_frac)
    f, sc = forward(A, off)
    b = backward(A, end, sc, off)
    out = {"G": np.zeros((R, 4, 4)), "H": np.zeros((R, 4, 4)), "Gabs": np.zeros((R, 4, 4)), "count": np.zeros((R, 4, 4)),
           "ll": float(np.sum(np.log(sc)))}
    if n == 0:
        return out
    x = (np.asarray(store.cov, np.int64) & 0xff).astype(np.float64)
    reg = (np.asarray(store.annot, np.uint64) >> np.uint64(58)).astype(np.int64)
    bt = viterbi_ref.betas(store, adjust, min_frac)
    local = np.arange(n) - np.repeat(off[:-1], np.diff(off))          # index of every window inside its chunk
    t = np.flatnonzero(local >= (2 if skip_first_pair else 1))        # window t of the pair (t-1, t)
    px = x[t - 1]
    xt, rt, btt = x[t], reg[t], bt[t]
    xi = f[t - 1][:, :, None] * A[t] * b[t][:, None, :] / TERMINATION  # [m][p][s]
    later = local[t] >= 2
    for s in range(4):
        if s == 0 and mt == N.HF_MODEL_TRUNC_EXP_GAUSSIAN:
            gterm = np.zeros((t.size, 4)); hterm = np.zeros((t.size, 4)); aterm = np.zeros((t.size, 4))
        else:
            gterm = np.empty((t.size, 4)); hterm = np.empty((t.size, 4)); aterm = np.empty((t.size, 4))
            for p in range(4):
                a = alpha[p][s]
                tot = np.zeros(t.size); g = np.zeros(t.size); h = np.zeros(t.size); ga = np.zeros(t.size)
                for c in range(ncomp[s]):
                    mu = mean[rt, s, c]
                    v = var[rt, s, c] * btt
                    d = xt - ((1 - a) * mu + a * px) * btt
                    u = btt * (px - mu)
                    with np.errstate(under="ignore"):
                        pc = weight[rt, s, c] / np.sqrt(2 * PI * v) * np.exp(-d * d / (2 * v))
                    floored = pc < 1e-40
                    pc = np.where(floored, 1e-40, pc)
                    phi = np.where(floored, 0.0, 1.0)
                    tot += pc
                    g += pc * phi * d * u / v
                    ga += pc * phi * np.abs(d * u) / v
                    h += pc * phi * u * u / v
                gterm[:, p], hterm[:, p], aterm[:, p] = g / tot, h / tot, ga / tot
        for r in range(R):
            m = rt == r
            out["G"][r, :, s] = (xi[m, :, s] * gterm[m]).sum(axis=0)
            out["H"][r, :, s] = (xi[m, :, s] * hterm[m]).sum(axis=0)
            out["Gabs"][r, :, s] = (xi[m, :, s] * aterm[m]).sum(axis=0)
            out["count"][r, :, s] = xi[m & later, :, s].sum(axis=0)
    return out


def alpha_step(alpha, st, mask, lo=0.0, hi=0.8, min_count=10.0):
    """One conditional maximisation: (new alpha, largest move)."""
    alpha = np.array(alpha, np.float64)
    G, H, cnt = st["G"].sum(axis=0), st["H"].sum(axis=0), st["count"].sum(axis=0)
    new = alpha.copy()
    for p in range(4):
        for s in range(4):
            if mask[p][s] and H[p, s] > 0 and min_count < cnt[p, s]:
                new[p, s] = min(max(alpha[p, s] + G[p, s] / H[p, s], lo), hi)
    return new, float(np.abs(new - alpha).max())


def true_model(store, model_type=N.HF_MODEL_GAUSSIAN, stay=(0.97, 0.97, 0.98, 0.97)):
    """The model `simulate` draws from, with alpha = 0: its means and variances, one collapsed component in use (the second one at
    3 x coverage with a small weight), leaving mass spread evenly."""
    from flagger_amd import hmm
    model = hmm.createModel(model_type, 2, store, np.zeros((4, 4)))
    K = N.HF_MAXCOMP
    v = model.param_vector().reshape(1, -1)
    cov = float(store.region_coverages[0])
    mu = np.array([0.1, 0.5, 1.0, 2.0]) * cov
    var = np.maximum(1.2 * mu, 2.0)
    mean_, var_, w_ = (v[0, 27 + k * 4 * K:27 + (k + 1) * 4 * K].reshape(4, K) for k in range(3))
    mean_[:, 0], var_[:, 0] = mu, var
    w_[3, 0], w_[3, 1] = 0.98, 0.02
    t = v[0, :25].reshape(5, 5)
    for s in range(4):
        t[s, :4] = (1 - stay[s]) / 3 * (1 - TERMINATION)
        t[s, s] = stay[s] * (1 - TERMINATION)
    model.set_param_vector(v.ravel())
    return model


def simulate(n_windows, chunk_windows, alpha, region_cov=20, seed=0, stay=(0.97, 0.97, 0.98, 0.97), window_len=4000):
    """A one-region WindowStore drawn from the model definition with a known alpha: a sticky hidden chain over (Err, Dup, Hap, Col) with
    means (0.1, 0.5, 1, 2) x region_cov and variance = 1.2 x mean (at least 2), x_t ~ round(N((1 - a) mu_s + a x_{t-1}, var_s)) with
    a = alpha[s_{t-1}][s_t], the first window of a chunk with a = 0.  Chunks lie in the middle of a long contig, so beta is the same
    for every window.  mapq = coverage except in Dup windows (0), so that every state passes its validity test where it occurs."""
    rng = np.random.default_rng(seed)
    alpha = np.asarray(alpha, np.float64)
    mu = np.array([0.1, 0.5, 1.0, 2.0]) * region_cov
    sd = np.sqrt(np.maximum(1.2 * mu, 2.0))
    stay = np.asarray(stay, np.float64)
    n_chunks = -(-n_windows // chunk_windows)
    cov = np.zeros(n_windows, np.uint16)
    truth = np.zeros(n_windows, np.int8)
    off = [0]
    for c in range(n_chunks):
        t0, t1 = c * chunk_windows, min(n_windows, (c + 1) * chunk_windows)
        s, xp = 2, 0.0
        for t in range(t0, t1):
            if t > t0 and rng.random() >= stay[s]:
                s_new = int(rng.choice([q for q in range(4) if q != s]))
            else:
                s_new = s
            a = alpha[s][s_new] if t > t0 else 0.0
            v = int(np.clip(np.rint(rng.normal((1 - a) * mu[s_new] + a * xp, sd[s_new])), 0, 250))
            cov[t], truth[t], s, xp = v, s_new, s_new, float(v)
        off.append(t1)
    chunk_len = chunk_windows * window_len
    lead = 20 * chunk_len
    ctg_len = lead * 2 + n_chunks * chunk_len
    cs = np.array([lead + c * chunk_len for c in range(n_chunks)], np.int32)
    ce = np.array([lead + c * chunk_len + (off[c + 1] - off[c]) * window_len - 1 for c in range(n_chunks)], np.int32)
    return synth.WindowStore(
        cov=cov, mapq=np.where(truth == 1, 0, cov).astype(np.uint16), clip=np.zeros(n_windows, np.uint16), annot=np.full(n_windows, 1, np.uint64), truth=truth,
        prediction=np.full(n_windows, -1, np.int8), chunk_off=np.asarray(off, np.int64), chunk_ctg=["sim"] * n_chunks,
        chunk_ctg_len=np.full(n_chunks, ctg_len, np.int32), chunk_s=cs, chunk_e=ce, window_len=window_len, chunk_len=chunk_len,
        region_coverages=[int(region_cov)])
