"""Exact interval probabilities (hf_get_interval_log_probs) on BASELINE configs[2] after two EM iterations and one more full pass.
One leg per process, so that rocprofv3 --kernel-trace --stats separates them:
  python profiles/tools/intervals_cfg2.py lazy      one one-window job: the lazy re-run of the segment kernel (+ one tiny interval launch)
  python profiles/tools/intervals_cfg2.py runs      the lazy call, then all runs of the final labels, 5 times
  python profiles/tools/intervals_cfg2.py regions   the lazy call, then 10 000 random regions x 8 masks, 5 times
Prints the host wall of every call (the kernel times come from rocprofv3)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from flagger_amd import hmm, synth

leg = sys.argv[1] if len(sys.argv) > 1 else "runs"
store = synth.config(2)
K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
em = hmm.EMList(store, model)
for _ in range(2):
    hmm.EM_runOneIterationForList(em, model); hmm.HMM_estimateParameters(model, 1e-3); hmm.HMM_resetEstimators(model)
hmm.EM_runOneIterationForList(em, model)
lab = em.labels()
off = np.asarray(store.chunk_off, np.int64)
first = [0]
for c in range(store.n_chunks):
    a = int(off[c])
    for t in range(a + 1, int(off[c + 1]) + 1):
        if t == off[c + 1] or lab[t] != lab[a]:
            first.append(a); a = t
runs = np.array(first[1:], np.int64)
ends = np.append(runs[1:] - 1, store.n_windows - 1)
print("windows", store.n_windows, "chunks", store.n_chunks, "runs", runs.size, flush=True)
t0 = time.perf_counter()
em.interval_log_probs([0], [0], [1])
print("lazy call (segment kernel re-run + one job): %.3f ms" % ((time.perf_counter() - t0) * 1e3), flush=True)
if leg == "runs":
    for rep in range(5):
        t0 = time.perf_counter()
        lp = em.interval_log_probs(runs, ends, 1 << lab[runs].astype(np.int64))
        print("rep %d: %d runs: %.3f ms  (NaN %d, max %.3g, p_all < 0.5: %d)" % (rep, runs.size, (time.perf_counter() - t0) * 1e3,
              int(np.isnan(lp).sum()), float(lp.max()), int((lp < np.log(0.5)).sum())), flush=True)
elif leg == "regions":
    rng = np.random.default_rng(1)
    a = rng.integers(0, store.n_windows, 10_000)
    b = np.minimum(store.n_windows - 1, a + rng.integers(0, 64, 10_000))
    F = np.repeat(a, 8); L = np.repeat(b, 8)
    M = np.tile(np.array([1, 2, 4, 8, 14, 13, 11, 7]), 10_000)
    for rep in range(5):
        t0 = time.perf_counter()
        em.interval_log_probs(F, L, M)
        print("rep %d: 10 000 regions x 8 masks: %.3f ms" % (rep, (time.perf_counter() - t0) * 1e3), flush=True)
em.close()
