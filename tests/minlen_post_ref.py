"""Test-side reference of the posterior under minimum run lengths (hf_minlen_posterior): float64 numpy, built on the tables of
tests/viterbi_ref.py (exp of them) and written from the definition in include/hmm_flagger_hip.h, not from the kernels.

`forward_backward` runs the expanded chain of the header (lanes (s, d), d = 1..min_len[s], lane index sum_{q<s} min_len[q] + d - 1)
over every chunk side by side, forward and backward, each window's vector divided by its largest entry and the logs of the divisors
accumulated:

    F_0[(s, m_s)] = first[s], 0 elsewhere
    F_t[(s, 1)]   = sum_p F_{t-1}[(p, m_p)] A_t[p][s], p != s when m_s > 1
    F_t[(s, d)]   = F_{t-1}[(s, d-1)] A_t[s][s]                                   1 < d < m_s
    F_t[(s, m_s)] = (F_{t-1}[(s, m_s - 1)] + F_{t-1}[(s, m_s)]) A_t[s][s]          m_s > 1
    B_{T-1}       = end[s]
    B_{t-1}[(s, d)]   = A_t[s][s] B_t[(s, d+1)]                                   d < m_s
    B_{t-1}[(s, m_s)] = [m_s > 1] A_t[s][s] B_t[(s, m_s)] + sum_q A_t[s][q] B_t[(q, 1)], q != s when m_s > 1
    Z_adm = sum_lanes F_{T-1} end;  g_t[s] = sum_d F_t[(s, d)] B_t[(s, d)];  post = g_t / sum_s g_t

`enumerate_chunk` sums minlen_ref.chunk_path_weights' 4^T paths of a tiny chunk in 50 digits, filtered by admissibility: the admissible
weight sum over the full sum, and the marginals.  `tiny_case` adds them to minlen_ref.tiny_case's stores, once per process."""
from __future__ import annotations

import functools

import mpmath as mp
import numpy as np

from flagger_amd import _native as N
from test_bruteforce_cpu import Params
import minlen_ref
import viterbi_ref

mp.mp.dps = 50


def forward_backward(logA, logend, chunk_off, min_len):
    """(post float64[N][4], log Z_adm float64[C]) of every chunk; a chunk without windows has log Z_adm 0."""
    m = [int(v) for v in min_len]
    ls, ld, ent, sat = minlen_ref.lanes(m)
    nl = ls.size
    off = np.asarray(chunk_off, np.int64)
    T = np.diff(off)
    n = int(off[-1]) if off.size else 0
    post = np.zeros((n, 4))
    lz = np.zeros(T.size)
    live = np.flatnonzero(T > 0)
    if live.size == 0:
        return post, lz
    with np.errstate(divide="ignore", under="ignore"):
        A_all, end = np.exp(logA), np.exp(logend)
    Tl, o = T[live], off[live]
    Fall = np.zeros((n, nl))
    inner = np.flatnonzero(ld > 1)                  # lanes with a lane below them in the same state
    below = np.flatnonzero(ld < np.asarray(m)[ls])  # lanes with a lane above them in the same state
    ar4 = np.arange(4)

    def norm(v, logs, rows):
        mx = v.max(axis=1)
        ok = mx > 0
        v[ok] /= mx[ok, None]
        logs[rows[ok]] += np.log(mx[ok])

    # forward
    Fp = np.zeros((live.size, nl))
    Fp[:, sat] = A_all[o, 0, :]
    logs = np.zeros(live.size)
    norm(Fp, logs, np.arange(live.size))
    Fall[o] = Fp
    for k in range(1, int(Tl.max())):
        act = np.flatnonzero(Tl > k)
        idx = o[act] + k
        A = A_all[idx]                              # [a][pre][s]
        fp = Fp[act]
        S = fp[:, sat]
        new = np.zeros_like(fp)
        for s in range(4):
            acc = np.zeros(act.size)
            for p in range(4):
                if m[s] > 1 and p == s:
                    continue
                acc = acc + S[:, p] * A[:, p, s]
            new[:, ent[s]] = acc
        diag = A[:, ar4, ar4]
        new[:, inner] = fp[:, inner - 1] * diag[:, ls[inner]]
        for s in range(4):
            if m[s] > 1:
                new[:, sat[s]] += fp[:, sat[s]] * diag[:, s]
        norm(new, logs, act)
        Fp[act] = new
        Fall[idx] = new
    with np.errstate(divide="ignore"):
        lz[live] = np.log(np.sum(Fp * end[live][:, ls], axis=1)) + logs

    # backward, chunks aligned at their last windows
    Bp = end[live][:, ls].copy()
    dummy = np.zeros(live.size)

    def emit(act, idx, b):
        g = np.zeros((act.size, 4))
        np.add.at(g.T, ls, (Fall[idx] * b).T)
        post[idx] = g / g.sum(axis=1)[:, None]

    allc = np.arange(live.size)
    norm(Bp, dummy, allc)
    emit(allc, o + Tl - 1, Bp)
    for j in range(1, int(Tl.max())):
        act = np.flatnonzero(Tl > j)
        idx = o[act] + Tl[act] - 1 - j              # the window whose B is computed; the row is that of idx + 1
        A = A_all[idx + 1]
        bp = Bp[act]
        E = bp[:, ent]                              # [a][q]
        diag = A[:, ar4, ar4]
        new = np.zeros_like(bp)
        new[:, below] = diag[:, ls[below]] * bp[:, below + 1]
        for s in range(4):
            acc = diag[:, s] * bp[:, sat[s]] if m[s] > 1 else np.zeros(act.size)
            for q in range(4):
                if m[s] > 1 and q == s:
                    continue
                acc = acc + A[:, s, q] * E[:, q]
            new[:, sat[s]] = acc
        norm(new, dummy, act)
        Bp[act] = new
        emit(act, idx, new)
    return post, lz


def reference(store, model, alpha, min_len):
    """(post [N][4], log_mass [C], log Z_adm [C], log Z [C]) of the whole store."""
    logA, logend = viterbi_ref.tables(store, model, alpha)
    post, lza = forward_backward(logA, logend, store.chunk_off, min_len)
    _, lz = forward_backward(logA, logend, store.chunk_off, (1, 1, 1, 1))
    return post, lza - lz, lza, lz


def close_post(got, ref, rel=1e-9, floor=1e-250, extra_abs=0.0):
    """post within `rel` relative (plus extra_abs) where ref >= floor; elsewhere 0 <= got <= 10 * floor.  No entry is left out."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and not np.isnan(got).any()
    big = ref >= floor
    err = np.abs(got[big] - ref[big]) - extra_abs
    assert np.all(err <= rel * ref[big]), float(np.max(err / ref[big]))
    assert np.all((got[~big] >= 0.0) & (got[~big] <= 10 * floor))


# ---- enumeration ---------------------------------------------------------------------------------------------------------------

def enumerate_chunk(weights, min_len):
    """(log Z_adm, log Z, marginals mpf[T][4] given admissibility) out of minlen_ref.chunk_path_weights' list."""
    m = [int(v) for v in min_len]
    T = len(weights[0][0])
    zero = mp.mpf(0)
    marg = [[zero] * 4 for _ in range(T)]
    za, z = zero, zero
    for path, w in weights:
        z += w
        if not minlen_ref._path_ok(path, m):
            continue
        za += w
        for t in range(T):
            marg[t][path[t]] += w
    return mp.log(za), mp.log(z), [[v / za for v in row] for row in marg]


@functools.lru_cache(maxsize=None)
def tiny_case(model_type, seed, hifi):
    """(store, model, alpha, {min_len: [(log Z_adm, log Z, marginals) per chunk]}) of one of minlen_ref's tiny cases."""
    store, model, alpha, _ = minlen_ref.tiny_case(model_type, seed, hifi)
    regions = model.numberOfRegions
    K = 2 + seed % 3
    P = Params(model.param_vector(), regions, K, model_type, alpha)
    nbE = None
    if model_type == N.HF_MODEL_NEGATIVE_BINOMIAL:
        p = model.params()
        nbE = np.ctypeslib.as_array(p.nb_E, shape=(regions * 4 * viterbi_ref.NX,)).reshape(regions, 4, viterbi_ref.NX).copy()
    enum = {ml: [] for ml in minlen_ref.TINY_MIN_LENS}
    for c in range(store.n_chunks):
        w = minlen_ref.chunk_path_weights(store, c, P, model, nbE)
        for ml in minlen_ref.TINY_MIN_LENS:
            enum[ml].append(enumerate_chunk(w, ml))
    return store, model, alpha, enum


def check_against_enumeration(store, enum, min_len, post, log_mass, log_z_adm, post_rel=0.0):
    """log_mass within 1e-12 (1 + |log Z|), post within 1e-12 absolute (+ post_rel relative).  Returns the chunks with mass < 1."""
    off = store.chunk_off
    below_one = 0
    for c in range(store.n_chunks):
        lza, lz, marg = enum[min_len][c]
        tol = 1e-12 * (1 + abs(float(lz)))
        assert abs(log_mass[c] - float(lza - lz)) <= tol, (min_len, c, log_mass[c], float(lza - lz))
        assert abs(log_z_adm[c] - float(lza)) <= tol, (min_len, c, log_z_adm[c], float(lza))
        ref = np.array([[float(v) for v in row] for row in marg])
        got = post[off[c]:off[c + 1]]
        assert np.all(np.abs(got - ref) <= 1e-12 + post_rel * ref), (min_len, c, float(np.max(np.abs(got - ref))))
        below_one += (lza - lz) < mp.mpf("-1e-6")
    return below_one


# ---- chunks whose ends sit on the emission floor -------------------------------------------------------------------------------------

FLOORED = 12                          # windows at a chunk's end whose coverage is an outlier for every state
FLOORED_LENGTHS = [40, 64, 100, 24, 70]   # chunk 0: floored at its first end, 1: at its last end, 2: at both, 3: all of it, 4: 30 windows inside


@functools.lru_cache(maxsize=None)
def floored_case():
    """(store, model, alpha): a Gaussian-state model and coverage 250 in the first / last FLOORED windows of the chunks, so that every
    entry of those windows' rows is a transition probability times the emission floor of 1e-40: a walk that starts there loses 40
    decimal digits per step from its very first window."""
    from test_bruteforce_cpu import _tiny_store
    from test_viterbi_cpu import perturbed_model
    rng = np.random.default_rng(77)
    store = _tiny_store(rng, FLOORED_LENGTHS, [20])
    off = store.chunk_off
    for c, (front, back) in enumerate([(True, False), (False, True), (True, True), (True, True)]):
        if front:
            store.cov[off[c]:off[c] + FLOORED] = 250
        if back:
            store.cov[off[c + 1] - FLOORED:off[c + 1]] = 250
    store.cov[off[4] + 21:off[4] + 51] = 250               # (both walks cross it, each at its own place in its period of eight steps)
    alpha = np.zeros((4, 4))
    model = perturbed_model(store, N.HF_MODEL_GAUSSIAN, 3, alpha, rng)
    return store, model, alpha


def mp_chunk(logA, logend, chunk_off, c, min_len):
    """(log Z_adm, post mpf[T][4]) of chunk c: the header's recursions over the expanded chain in 50 digits, no scaling at all."""
    m = [int(v) for v in min_len]
    ls, ld, ent, sat = minlen_ref.lanes(m)
    nl = ls.size
    t0, T = int(chunk_off[c]), int(chunk_off[c + 1] - chunk_off[c])
    zero = mp.mpf(0)
    ex = lambda v: mp.exp(mp.mpf(float(v))) if np.isfinite(v) else zero
    A = [[[ex(logA[t0 + t, p, s]) for s in range(4)] for p in range(4)] for t in range(T)]
    end = [ex(logend[c, s]) for s in range(4)]
    F = [[zero] * nl for _ in range(T)]
    for s in range(4):
        F[0][sat[s]] = A[0][0][s]
    for t in range(1, T):
        for l in range(nl):
            s, d = int(ls[l]), int(ld[l])
            v = zero
            if d == 1:
                for p in range(4):
                    if not (m[s] > 1 and p == s):
                        v += F[t - 1][sat[p]] * A[t][p][s]
            else:
                v = F[t - 1][l - 1] * A[t][s][s]
                if d == m[s]:
                    v += F[t - 1][l] * A[t][s][s]
            F[t][l] = v
    B = [[zero] * nl for _ in range(T)]
    B[T - 1] = [end[int(ls[l])] for l in range(nl)]
    for t in range(T - 1, 0, -1):
        for l in range(nl):
            s, d = int(ls[l]), int(ld[l])
            if d < m[s]:
                B[t - 1][l] = A[t][s][s] * B[t][l + 1]
            else:
                v = A[t][s][s] * B[t][l] if m[s] > 1 else zero
                for q in range(4):
                    if not (m[s] > 1 and q == s):
                        v += A[t][s][q] * B[t][ent[q]]
                B[t - 1][l] = v
    za = sum(F[T - 1][l] * end[int(ls[l])] for l in range(nl))
    post = []
    for t in range(T):
        g = [zero] * 4
        for l in range(nl):
            g[int(ls[l])] += F[t][l] * B[t][l]
        tot = sum(g)
        post.append([v / tot for v in g])
    return mp.log(za), post
