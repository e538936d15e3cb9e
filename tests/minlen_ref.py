"""Test-side reference of the minimum-run-length Viterbi decoder (hf_viterbi_minlen): float64 numpy in the log domain, built on the
tables of tests/viterbi_ref.py and written from the definition in include/hmm_flagger_hip.h, not from the kernels.

A path of a chunk is ADMISSIBLE when every maximal run of equal state s has at least min_len[s] windows; runs that contain the chunk's
first or last window are exempt.  `viterbi_minlen` runs the expanded chain of the header (lanes (s, d), d = 1..min_len[s], lane index
sum_{q<s} min_len[q] + d - 1) over every chunk side by side, as viterbi_ref.viterbi does, with the header's tie rules:

    window 0     delta[(s, min_len[s])] = first[s], -inf elsewhere
    entry (s,1)  max over p in increasing order of delta[(p, min_len[p])] + logA_t[p][s], p != s when min_len[s] > 1, strict >
    1 < d < m    delta[(s, d-1)] + logA_t[s][s]
    d = m > 1    delta[(s, d-1)] + logA_t[s][s], then delta[(s, d)] + logA_t[s][s], strict >
    end          max over all lanes in lane order of delta + log end[s], strict >

`admissible` checks any labelling; `chunk_path_weights` / `best_admissible` enumerate all 4^T paths of a tiny chunk in 50 digits (the
tables of test_viterbi_cpu.enumerate_map) and filter them by admissibility; `tiny_case` builds the tiny stores the CPU and the GPU test
share, with their enumerations, once per process."""
from __future__ import annotations

import functools

import mpmath as mp
import numpy as np

from flagger_amd import _native as N
from flagger_amd import synth
from test_bruteforce_cpu import Params, _tiny_store, beta_of
import viterbi_ref

mp.mp.dps = 50


def lanes(min_len):
    """(state of every lane, d of every lane, entry lane per state, saturated lane per state)."""
    m = [int(v) for v in min_len]
    assert len(m) == 4 and min(m) >= 1 and sum(m) <= 64
    ls = np.repeat(np.arange(4), m)
    base = np.concatenate([[0], np.cumsum(m)[:-1]])
    ld = np.arange(sum(m)) - base[ls] + 1
    return ls, ld, base, base + np.asarray(m) - 1


def viterbi_minlen(logA, logend, chunk_off, min_len):
    """The expanded chain over every chunk (side by side): (labels int8[N], chunk scores float64[C])."""
    m = [int(v) for v in min_len]
    ls, ld, ent, sat = lanes(m)
    nl = ls.size
    off = np.asarray(chunk_off, np.int64)
    T = np.diff(off)
    n = int(off[-1]) if off.size else 0
    labels = np.zeros(n, np.int8)
    score = np.zeros(T.size)
    if n == 0:
        return labels, score
    bp_entry = np.zeros((n, 4), np.int8)       # predecessor state of every state's entry lane
    bp_stay = np.zeros((n, 4), bool)           # the saturated lane stayed (False: it arrived from d - 1)
    live = np.flatnonzero(T > 0)
    delta = np.full((live.size, nl), -np.inf)
    delta[:, sat] = logA[off[live], 0, :]
    inner = np.flatnonzero(ld > 1)             # lanes with a lane below them in the same state
    with np.errstate(invalid="ignore"):
        for k in range(1, int(T.max())):
            act = np.flatnonzero(T[live] > k)
            idx = off[live[act]] + k
            A = logA[idx]                                      # [a][pre][s]
            dl = delta[act]
            S = dl[:, sat]                                     # [a][p]
            new = np.full_like(dl, -np.inf)
            for s in range(4):
                excl = m[s] > 1
                pf = 1 if (excl and s == 0) else 0
                best = S[:, pf] + A[:, pf, s]
                arg = np.full(act.size, pf, np.int8)
                for p in range(pf + 1, 4):
                    if excl and p == s:
                        continue
                    v = S[:, p] + A[:, p, s]
                    up = v > best
                    best = np.where(up, v, best)
                    arg[up] = p
                new[:, ent[s]] = best
                bp_entry[idx, s] = arg
            diag = A[:, np.arange(4), np.arange(4)]            # [a][s]
            up = dl[:, inner - 1] + diag[:, ls[inner]]
            new[:, inner] = up
            for s in range(4):
                if m[s] > 1:
                    u = dl[:, sat[s] - 1] + diag[:, s]
                    st = dl[:, sat[s]] + diag[:, s]
                    stayed = st > u
                    new[:, sat[s]] = np.where(stayed, st, u)
                    bp_stay[idx, s] = stayed
            delta[act] = new
        fin = delta + logend[live][:, ls]
        fl = np.argmax(fin, axis=1)                            # the first largest lane
        score[live] = fin[np.arange(live.size), fl]
    cs, cd = ls[fl].copy(), ld[fl].copy()
    marr = np.asarray(m)
    for k in range(int(T.max()) - 1, -1, -1):
        act = np.flatnonzero(T[live] > k)
        idx = off[live[act]] + k
        s, d = cs[act], cd[act]
        labels[idx] = s
        if k == 0:
            break
        is_entry = d == 1
        p = bp_entry[idx, s]
        stayed = bp_stay[idx, s]
        ns = np.where(is_entry, p, s)
        nd = np.where(is_entry, marr[p], np.where((d < marr[s]) | ~stayed, d - 1, d))
        cs[act], cd[act] = ns, nd
    return labels, score


def _path_ok(path, m):
    T = len(path)
    a = 0
    while a < T:
        b = a
        while b + 1 < T and path[b + 1] == path[a]:
            b += 1
        if a > 0 and b < T - 1 and b - a + 1 < m[path[a]]:
            return False
        a = b + 1
    return True


def admissible(labels, chunk_off, min_len):
    """Per chunk: every maximal run of state s that touches neither end of the chunk has at least min_len[s] windows."""
    off = np.asarray(chunk_off, np.int64)
    m = [int(v) for v in min_len]
    lab = np.asarray(labels)
    return np.array([_path_ok(lab[off[c]:off[c + 1]].tolist(), m) for c in range(off.size - 1)], bool)


def reference(store, model, alpha, min_len):
    """(labels, chunk scores, path_log_prob, unconstrained labels) of the whole store."""
    logA, logend = viterbi_ref.tables(store, model, alpha)
    labels, score = viterbi_minlen(logA, logend, store.chunk_off, min_len)
    free, _ = viterbi_ref.viterbi(logA, logend, store.chunk_off)
    return labels, score, (lambda lab: viterbi_ref.path_log_prob(logA, logend, store.chunk_off, lab)), free


# ---- enumeration ---------------------------------------------------------------------------------------------------------------

def chunk_path_weights(store, c, P, model, nbE=None):
    """[(path, weight)] of all 4^T paths of chunk c in 50 digits; first, A_t and end as test_viterbi_cpu.enumerate_map builds them."""
    t0, T = int(store.chunk_off[c]), int(store.chunk_off[c + 1] - store.chunk_off[c])
    x = [mp.mpf(int(store.cov[t0 + t]) & 0xff) for t in range(T)]
    reg = [int(store.annot[t0 + t] >> np.uint64(58)) for t in range(T)]
    beta = [beta_of(store, c, t, True, 0.95) for t in range(T)]
    L = N.lib()
    mx, mn, mc = L.hfm_max_high_mapq_ratio(model._h), L.hfm_min_high_mapq_ratio(model._h), L.hfm_min_highly_clipped_ratio(model._h)

    def emit(t, s, px, a):
        if nbE is not None:
            return mp.mpf(float(nbE[reg[t], s, int(x[t])]))
        return P.emit(reg[t], s, x[t], px, a, beta[t])

    first = [P.trans[reg[0]][4][s] * emit(0, s, mp.mpf(0), mp.mpf(0)) for s in range(4)]
    A = [None]
    for t in range(1, T):
        cov, mapq, clip = float(int(store.cov[t0 + t])), float(int(store.mapq[t0 + t])), float(int(store.clip[t0 + t]))
        A.append([[(mp.mpf(1) / 5 if reg[t] != reg[t - 1] else P.tcond(reg[t], pre, s, cov, mapq, clip, mx, mn, mc))
                   * emit(t, s, x[t - 1], P.alpha[pre][s]) for s in range(4)] for pre in range(4)])
    end = [P.trans[reg[T - 1]][s][4] for s in range(4)]
    out = []

    def walk(path, w):                         # prefix products: 4^T / 3 multiplications more than the leaves
        if len(path) == T:
            out.append((path, w * end[path[-1]]))
            return
        t = len(path)
        for s in range(4):
            walk(path + (s,), w * A[t][path[-1]][s])

    for s in range(4):
        walk((s,), first[s])
    return out


def best_admissible(weights, min_len):
    """(best admissible path, its log-weight, the second-best admissible log-weight) out of chunk_path_weights' list."""
    m = [int(v) for v in min_len]
    best, second, arg = mp.mpf(0), mp.mpf(0), None
    for path, w in weights:
        if not _path_ok(path, m):
            continue
        if w > best:
            best, second, arg = w, best, path
        elif w > second:
            second = w
    return arg, mp.log(best), (mp.log(second) if second > 0 else mp.mpf("-inf"))


TINY_LENGTHS = [8, 7, 5, 1, 6, 3, 2, 4]
TINY_CASES = [(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 0, True), (N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 1, False),
              (N.HF_MODEL_GAUSSIAN, 2, True), (N.HF_MODEL_NEGATIVE_BINOMIAL, 4, False)]      # test_viterbi_gpu's four
TINY_MIN_LENS = [(3, 2, 2, 2), (1, 1, 1, 1)]


@functools.lru_cache(maxsize=None)
def tiny_case(model_type, seed, hifi):
    """(store, model, alpha, {min_len: [(path, log best, log second) per chunk]}) of one tiny case, computed once."""
    from test_viterbi_cpu import perturbed_model
    rng = np.random.default_rng(900 + seed)
    alpha = synth.HIFI_ALPHA if hifi else np.zeros((4, 4))
    regions = [20, 31] if seed % 2 == 0 else [25]
    store = _tiny_store(rng, TINY_LENGTHS, regions)
    K = 2 + seed % 3
    model = perturbed_model(store, model_type, K, alpha, rng)
    P = Params(model.param_vector(), len(regions), K, model_type, alpha)
    nbE = None
    if model_type == N.HF_MODEL_NEGATIVE_BINOMIAL:
        p = model.params()
        nbE = np.ctypeslib.as_array(p.nb_E, shape=(len(regions) * 4 * viterbi_ref.NX,)).reshape(len(regions), 4, viterbi_ref.NX).copy()
    enum = {ml: [] for ml in TINY_MIN_LENS}
    for c in range(store.n_chunks):
        w = chunk_path_weights(store, c, P, model, nbE)
        for ml in TINY_MIN_LENS:
            enum[ml].append(best_admissible(w, ml))
    return store, model, alpha, enum
