"""The posterior under minimum run lengths (hf_minlen_posterior) on configs[2] after two EM iterations, with (3, 5, 1, 7) and with all
ones: host wall per call (median of 11), hf_viterbi_minlen's wall in the same process as the yardstick, and a check against the numpy
reference (tests/minlen_post_ref.py; --no-check skips it).  --only A,B,C,D runs one set of lengths.  Run under
rocprofv3 --kernel-trace --stats for the kernel times: k_dec_rows_win, k_mlp_fwd and k_mlp_bwd are the feature's three kernels."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C
import numpy as np
from flagger_amd import hmm, synth, _native as N
CHECK = "--no-check" not in sys.argv
SETS = ((3, 5, 1, 7), (1, 1, 1, 1))
if "--only" in sys.argv:
    SETS = (tuple(int(v) for v in sys.argv[sys.argv.index("--only") + 1].split(",")),)
REPS = 11
store = synth.config(2)
K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
em = hmm.EMList(store, model)
for _ in range(2):
    hmm.EM_runOneIterationForList(em, model); hmm.HMM_estimateParameters(model, 1e-3); hmm.HMM_resetEstimators(model)
T = np.diff(store.chunk_off)
print("windows", store.n_windows, "chunks", store.n_chunks, "longest chunk", int(T.max()), "K", K, flush=True)
L = N.lib()
p = model.params()
lp = C.c_double(0.0)


def wall(call):
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter(); call(); ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), min(ms)


for ml in SETS:
    a = (C.c_int32 * 4)(*ml)

    def mlv():
        N.check(L.hf_viterbi_minlen(em._h, p, a, None), "m"); N.check(L.hf_viterbi_minlen_finish(em._h, C.byref(lp), None), "f")

    def run():
        N.check(L.hf_minlen_posterior(em._h, p, a, None), "p"); N.check(L.hf_minlen_posterior_finish(em._h, C.byref(lp), None), "f")

    mlv(); run()
    wv, wp = wall(mlv), wall(run)
    print("%-14s hf_viterbi_minlen + finish: median %.3f ms, min %.3f ms" % ((str(ml) + ":",) + wv), flush=True)
    print("%-14s hf_minlen_posterior + finish: median %.3f ms, min %.3f ms; ratio of the medians %.2f" % ((str(ml) + ":",) + wp + (wp[0] / wv[0],)),
          flush=True)
    t0 = time.perf_counter(); r = em.minlen_posterior(model, ml); post = r.posterior()
    print("  EMList.minlen_posterior with the labels, the chunk values and the posterior: %.3f ms; forward lanes %.1f MB" %
          ((time.perf_counter() - t0) * 1e3, store.n_windows * sum(ml) * 8 / 1e6), flush=True)
    m = r.chunk_log_mass
    print("  log_mass total %.6f; per chunk: min %.6f, median %.6f, max %.6f; chunks below -1: %d, below -100: %d of %d" %
          (r.log_mass, float(m.min()), float(np.median(m)), float(m.max()), int(np.sum(m < -1)), int(np.sum(m < -100)), m.size), flush=True)
    vit = em.viterbi_minlen(model, ml)[0]
    print("  windows whose constrained-posterior argmax is the label of hf_viterbi_minlen: %.4f %%; of the last pass's labels: %.4f %%" %
          (100.0 * float(np.mean(r.labels == vit)), 100.0 * float(np.mean(r.labels == em.labels()))), flush=True)
    if CHECK:
        import minlen_post_ref
        rpost, rmass, rlza, _ = minlen_post_ref.reference(store, model, synth.HIFI_ALPHA, ml)
        big = rpost >= 1e-250
        print("  against the numpy reference: log_mass max deviation %.2e, log Z_adm %.2e (relative %.2e); post max relative deviation %.2e over"
              " %d entries, the other %d at most %.1e; |sum post - 1| at most %.2e" %
              (float(np.max(np.abs(m - rmass))), float(np.max(np.abs(r.chunk_log_z_adm - rlza))),
               float(np.max(np.abs(r.chunk_log_z_adm - rlza) / np.abs(rlza))), float(np.max(np.abs(post[big] - rpost[big]) / rpost[big])),
               int(big.sum()), int((~big).sum()), float(post[~big].max()) if (~big).any() else 0.0,
               float(np.max(np.abs(post.sum(axis=1) - 1)))), flush=True)
em.close()
