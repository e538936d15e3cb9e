"""Minimum-run-length Viterbi (hf_viterbi_minlen) on configs[2] after two EM iterations, with (3, 5, 1, 7) and with all ones: host wall per
call (median of 11), hf_viterbi's wall in the same process as the yardstick, and an admissibility and score check against the numpy
reference (tests/minlen_ref.py; --no-check skips it).  Run under rocprofv3 --kernel-trace --stats for the kernel times: k_mlv_rows,
k_mlv_fwd and k_mlv_back are the decoder's three kernels."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C
import numpy as np
from flagger_amd import hmm, synth, _native as N
CHECK = "--no-check" not in sys.argv
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


def vit():
    N.check(L.hf_viterbi(em._h, p, None), "v"); N.check(L.hf_viterbi_finish(em._h, C.byref(lp), None), "f")


vit()
print("hf_viterbi + finish:                       median %.3f ms, min %.3f ms" % wall(vit), flush=True)
if CHECK:
    import minlen_ref, viterbi_ref
    logA, logend = viterbi_ref.tables(store, model, synth.HIFI_ALPHA)
    free, free_ll = viterbi_ref.viterbi(logA, logend, store.chunk_off)
for ml in ((3, 5, 1, 7), (1, 1, 1, 1)):
    a = (C.c_int32 * 4)(*ml)

    def run():
        N.check(L.hf_viterbi_minlen(em._h, p, a, None), "m"); N.check(L.hf_viterbi_minlen_finish(em._h, C.byref(lp), None), "f")

    run()
    print("hf_viterbi_minlen + finish, %-14s median %.3f ms, min %.3f ms" % ((str(ml) + ":",) + wall(run)), flush=True)
    t0 = time.perf_counter(); labels, ll, tot = em.viterbi_minlen(model, ml)
    print("  EMList.viterbi_minlen with the labels: %.3f ms; log-probability %.6f" % ((time.perf_counter() - t0) * 1e3, tot), flush=True)
    if CHECK:
        ref_lab, ref_ll = minlen_ref.viterbi_minlen(logA, logend, store.chunk_off, ml)
        ok = minlen_ref.admissible(labels, store.chunk_off, ml)
        val = viterbi_ref.path_log_prob(logA, logend, store.chunk_off, labels)
        bites = int(np.sum(~minlen_ref.admissible(free, store.chunk_off, ml)))
        print("  admissible chunks %d / %d; max relative error of the chunk scores %.2e, of path_log_prob(labels) %.2e; labels equal to the"
              " reference's on %.4f %% of windows" % (int(ok.sum()), ok.size, float(np.max(np.abs(ll - ref_ll) / np.abs(ref_ll))),
                                                       float(np.max(np.abs(val - ref_ll) / np.abs(ref_ll))), 100.0 * float(np.mean(labels == ref_lab))))
        print("  the unconstrained path is inadmissible in %d chunks; cost %.6f (%.2e relative)"
              % (bites, tot - float(free_ll.sum()), abs(tot - float(free_ll.sum())) / abs(float(free_ll.sum()))), flush=True)
em.close()
