"""The admissible path sampler (hf_sample_paths_minlen) on configs[2] after two EM iterations, (3, 5, 1, 7), 64 samples: host wall per
call (median of 11), in the same process hf_sample_paths at 64 samples and hf_minlen_posterior as the yardsticks, the capacity on this
context, the share of admissible samples of either sampler, and a check against the numpy reference (tests/minlen_sample_ref.py, 8
samples; --no-check skips it).  --samples K draws another number.  Run under rocprofv3 --kernel-trace --stats for the kernel times:
k_dec_rows_win, k_mlp_fwd, k_mls_draw, k_mls_final and k_mls_back are the feature's five launches."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C
import numpy as np
from flagger_amd import hmm, synth, _native as N
CHECK = "--no-check" not in sys.argv
K_S = int(sys.argv[sys.argv.index("--samples") + 1]) if "--samples" in sys.argv else 64
ML = (3, 5, 1, 7)
REPS = 11
store = synth.config(2)
K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
em = hmm.EMList(store, model)
for _ in range(2):
    hmm.EM_runOneIterationForList(em, model); hmm.HMM_estimateParameters(model, 1e-3); hmm.HMM_resetEstimators(model)
T = np.diff(store.chunk_off)
print("windows", store.n_windows, "chunks", store.n_chunks, "longest chunk", int(T.max()), "K", K, "samples", K_S, flush=True)
L = N.lib()
p = model.params()
lp = C.c_double(0.0)
a = (C.c_int32 * 4)(*ML)


def wall(call):
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter(); call(); ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), min(ms)


def mls():
    N.check(L.hf_sample_paths_minlen(em._h, p, a, 0, K_S, 5, None), "s"); N.check(L.hf_sample_minlen_finish(em._h, None), "f")


def smp():
    N.check(L.hf_sample_paths(em._h, p, 0, K_S, 5, None), "s"); N.check(L.hf_sample_finish(em._h, None), "f")


def mlp():
    N.check(L.hf_minlen_posterior(em._h, p, a, None), "p"); N.check(L.hf_minlen_posterior_finish(em._h, C.byref(lp), None), "f")


mls(); smp(); mlp()
for name, f in (("hf_sample_paths_minlen", mls), ("hf_sample_paths", smp), ("hf_minlen_posterior", mlp)):
    print("%-24s + finish: median %.3f ms, min %.3f ms" % ((name,) + wall(f)), flush=True)
print("hf_minlen_sample_capacity %s: %d; hf_sample_capacity: %d; forward lanes %.1f MB, words and labels of %d samples %.1f MB" %
      (ML, em.minlen_sample_capacity(ML), em.sample_capacity, store.n_windows * sum(ML) * 8 / 1e6, K_S,
       store.n_windows * (2 * ((K_S + 63) // 64 * 64) + K_S) / 1e6), flush=True)
t0 = time.perf_counter(); lab = em.sample_paths_minlen(model, ML, K_S, 5)
print("EMList.sample_paths_minlen with the labels of every sample: %.3f ms" % ((time.perf_counter() - t0) * 1e3), flush=True)
free = em.sample_paths(model, K_S, 5)
import minlen_ref
adm = lambda x: np.array([minlen_ref.admissible(r, store.chunk_off, ML) for r in x[:8]])
print("admissible (sample, chunk) pairs of the first 8 samples: hf_sample_paths_minlen %d of %d, hf_sample_paths %d of %d" %
      (int(adm(lab).sum()), 8 * store.n_chunks, int(adm(free).sum()), 8 * store.n_chunks), flush=True)
if CHECK:
    import minlen_sample_ref
    ref, marg, fmarg = minlen_sample_ref.reference(store, model, synth.HIFI_ALPHA, ML, 5, range(8))
    print("against the numpy reference, 8 samples: %d of %d labels differ; smallest reference margin %.2e (window), %.2e (final)" %
          (int(np.sum(ref != lab[:8])), ref.size, float(marg.min()), float(fmarg.min())), flush=True)
em.close()
