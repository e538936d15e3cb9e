"""The E-step under minimum run lengths over whole contigs (hf_estep_minlen_joined) and the EM over it on BASELINE configs[2],
trunc_exp_gaussian, HiFi alpha, lengths (3, 5, 1, 7) windows, joined = joined_chunks(store).  Writes what it measures to stdout (kept as
profiles/minlen_em_joined_cfg2.txt).
  python profiles/tools/minlen_em_joined_cfg2.py step        after two plain EM iterations: host wall (call .. statistics on the host,
                                                             median of 11) of hf_estep_minlen + finish, hf_minlen_posterior_joined +
                                                             finish and hf_estep_minlen_joined + finish in one process; under rocprofv3
                                                             --kernel-trace --stats this gives the kernel times of k_mle_bwd, k_mlpj_bwd,
                                                             k_mlej_bwd and the kernels around them side by side
  python profiles/tools/minlen_em_joined_cfg2.py ratio CSV   from that run's kernel_stats CSV: k_mlej_bwd's ns per window of the longest
                                                             contig against k_mle_bwd's ns per window of the longest chunk
  python profiles/tools/minlen_em_joined_cfg2.py effect      the plain fit, the per-chunk-constrained fit and the joined-constrained fit
                                                             from the same initial model (at most ITER iterations, tol 1e-3): for each
                                                             the sum over groups of log Z_adm and the joined log_mass
                                                             (hf_minlen_posterior_joined), the cost of hf_viterbi_minlen_joined's path
                                                             and the expected-correct windows of hf_get_mea_labels(joined=...); whether
                                                             the objective rose in every iteration"""
import csv, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C
import numpy as np
from flagger_amd import hmm, synth, _native as N
ML = (3, 5, 1, 7)
REPS, ITER = 11, 30
MODES = [a for a in sys.argv[1:] if a in ("step", "ratio", "effect")] or ["step", "effect"]
store = synth.config(2)
K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
T = np.diff(store.chunk_off)
joined = hmm.joined_chunks(store)
first = np.flatnonzero(~(joined & (T > 0) & (np.concatenate([[0], T[:-1]]) > 0)))       # the first chunk of every group
G = np.diff(np.concatenate([np.asarray(store.chunk_off)[first], [store.chunk_off[-1]]]))
print("windows", store.n_windows, "chunks", store.n_chunks, "longest chunk", int(T.max()), "groups", G.size, "longest group", int(G.max()),
      "K", K, "lengths", ML, flush=True)


def wall(call):
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter(); call(); ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), min(ms)


def fresh():
    return hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)


if "step" in MODES:
    model = fresh()
    em = hmm.EMList(store, model)
    for _ in range(2):
        hmm.EM_runOneIterationForList(em, model); hmm.HMM_estimateParameters(model, 1e-3); hmm.HMM_resetEstimators(model)
    L = N.lib()
    p = model.params()
    a = (C.c_int32 * 4)(*ML)
    jn = np.ascontiguousarray(joined, np.uint8)
    jp = jn.ctypes.data_as(C.POINTER(C.c_uint8))
    lp = C.c_double(0.0)
    st = np.empty(em.stats_len)
    sp = st.ctypes.data_as(C.POINTER(C.c_double))

    def con():
        N.check(L.hf_estep_minlen(em._h, p, a, None), "c"); N.check(L.hf_estep_minlen_finish(em._h, sp, C.byref(lp), None), "f")

    def postj():
        N.check(L.hf_minlen_posterior_joined(em._h, p, a, jp, None), "p"); N.check(L.hf_minlen_posterior_finish(em._h, C.byref(lp), None), "f")

    def conj():
        N.check(L.hf_estep_minlen_joined(em._h, p, a, jp, None), "c"); N.check(L.hf_estep_minlen_finish(em._h, sp, C.byref(lp), None), "f")

    con(); postj(); conj()
    for name, f in (("hf_estep_minlen + finish", con), ("hf_minlen_posterior_joined + finish", postj), ("hf_estep_minlen_joined + finish", conj)):
        print("step: %-37s median %.3f ms, min %.3f ms" % ((name,) + wall(f)), flush=True)
    print("step: forward lanes %.1f MB, xi_adm %.1f MB; sum over groups of log Z_adm %.4f, of log Z %.4f" %
          (store.n_windows * sum(ML) * 8 / 1e6, store.n_windows * 128 / 1e6, st[0], lp.value), flush=True)
    em.close()

if "ratio" in MODES:
    path = sys.argv[sys.argv.index("ratio") + 1]
    avg = {}
    for row in csv.DictReader(open(path)):
        avg[row["Name"].split("(")[0]] = float(row["AverageNs"])
    per_chunk, per_group = avg["k_mle_bwd"] / int(T.max()), avg["k_mlej_bwd"] / int(G.max())
    print("ratio: k_mle_bwd %.1f us / %d windows of the longest chunk = %.1f ns per window; k_mlej_bwd %.1f us / %d windows of the longest "
          "contig = %.1f ns per window: %.3f x" % (avg["k_mle_bwd"] / 1e3, int(T.max()), per_chunk, avg["k_mlej_bwd"] / 1e3, int(G.max()),
                                                  per_group, per_group / per_chunk), flush=True)
    if "k_mlpj_bwd" in avg:
        print("ratio: k_mlej_bwd / k_mlpj_bwd = %.3f (k_mlpj_bwd %.1f us)" % (avg["k_mlej_bwd"] / avg["k_mlpj_bwd"], avg["k_mlpj_bwd"] / 1e3), flush=True)

if "effect" in MODES:
    fits = {}
    for kind in ("plain", "per-chunk", "joined"):
        model = fresh()
        em = hmm.EMList(store, model)
        t0 = time.perf_counter()
        it, cv, obj = 0, False, []
        while it < ITER and not cv:
            if kind == "plain":
                cv = em.em_iterate(model, True, 1e-3)
            else:
                cv = em.em_iterate_minlen(model, ML, True, 1e-3, joined=joined if kind == "joined" else None)
            obj.append(model.loglikelihood)
            hmm.HMM_resetEstimators(model)
            it += 1
        dt = time.perf_counter() - t0
        hmm.EM_runOneIterationForList(em, model); hmm.HMM_resetEstimators(model)          # the final pass
        ll = model.loglikelihood
        r = em.minlen_posterior(model, ML, joined)
        v = em.viterbi(model)[2]
        vm = em.viterbi_minlen(model, ML, joined)[2]
        _, _, gain = em.mea_labels(ML, joined)
        rose = bool(np.all(np.diff(obj) > 0))
        print("effect: %-9s fit: %d iterations in %.1f ms (%.2f ms each), converged %s; objective first %.4f last %.4f, rose in every iteration: %s; "
              "final log-likelihood %.4f" % (kind, it, dt * 1e3, dt * 1e3 / it, cv, obj[0], obj[-1], rose, ll), flush=True)
        print("effect: %-9s fit: sum over groups of log Z_adm %.4f, joined log_mass %.4f; Viterbi %.4f, whole-contig constrained Viterbi %.4f, "
              "cost %.4f; expected correct windows under the contig rule %.4f" %
              (kind, float(r.chunk_log_z_adm.sum()), r.log_mass, v, vm, v - vm, gain), flush=True)
        fits[kind] = model.param_vector()
        em.close()
    R_ = fits["plain"].size // (27 + 12 * 16)
    stay = {k: f.reshape(R_, -1)[0, :25].reshape(5, 5) for k, f in fits.items()}
    print("effect: stay probabilities (Err, Dup, Hap, Col): " +
          ", ".join("%s %s" % (k, " ".join("%.6f" % t[s, s] for s in range(4))) for k, t in stay.items()), flush=True)
