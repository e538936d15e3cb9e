"""64 posterior path samples on configs[2] after two EM iterations: host wall per call (run under rocprofv3 for kernel times)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from flagger_amd import hmm, synth, _native as N
store = synth.config(2)
K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
em = hmm.EMList(store, model)
for _ in range(2):
    hmm.EM_runOneIterationForList(em, model); hmm.HMM_estimateParameters(model, 1e-3); hmm.HMM_resetEstimators(model)
print("windows", store.n_windows, "chunks", store.n_chunks, "capacity", em.sample_capacity, flush=True)
L = N.lib()
p = model.params()
for rep in range(4):
    t0 = time.perf_counter()
    N.check(L.hf_sample_paths(em._h, p, 0, 64, 1, None), "s"); N.check(L.hf_sample_finish(em._h, None), "f")
    t1 = time.perf_counter()
    print("rep %d: hf_sample_paths + finish, 64 samples: %.3f ms" % (rep, (t1 - t0) * 1e3), flush=True)
t0 = time.perf_counter()
lab = em.sample_paths(model, 64, 1)
print("EMList.sample_paths(64) incl. label copies: %.3f ms" % ((time.perf_counter() - t0) * 1e3))
t0 = time.perf_counter(); em.viterbi(model); print("viterbi: %.3f ms" % ((time.perf_counter() - t0) * 1e3))
em.close()
