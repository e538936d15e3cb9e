"""Exact long-run probabilities (hf_get_long_run_log_probs) on BASELINE configs[2] after two EM iterations and one more full pass.
  python profiles/tools/longrun_cfg2.py     the lazy call; then, 5 times each, (a) every contig x Err, Dup, Hap, Col at the lengths
                                            (3, 5, 1, 7) windows, the chunks of a contig joined (the contig rows of `hmm_flagger
                                            --keptBlocks`), and (b) every run of the final labels with its own label and that label's
                                            length; and the same ranges and masks through hf_get_interval_log_probs as the yardstick
Prints the host wall of every call; under rocprofv3 --kernel-trace --stats the kernel times come from the trace."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from flagger_amd import hmm, synth

LENGTHS = np.array([3, 5, 1, 7])
store = synth.config(2)
K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
em = hmm.EMList(store, model)
for _ in range(2):
    hmm.EM_runOneIterationForList(em, model); hmm.HMM_estimateParameters(model, 1e-3); hmm.HMM_resetEstimators(model)
hmm.EM_runOneIterationForList(em, model)
off = np.asarray(store.chunk_off, np.int64)
n = store.n_windows
ctg = list(store.chunk_ctg)
joined = np.array([c > 0 and ctg[c] == ctg[c - 1] for c in range(len(ctg))], bool)
ranges = []
for c in range(len(ctg)):                          # (the contigs of this track are runs of consecutive chunks)
    if joined[c]:
        ranges[-1] = (ranges[-1][0], int(off[c + 1]) - 1)
    else:
        ranges.append((int(off[c]), int(off[c + 1]) - 1))
Fa = np.repeat([a for a, _ in ranges], 4); La = np.repeat([b for _, b in ranges], 4)
Ma = np.tile(1 << np.arange(4), len(ranges)); Ka = np.tile(LENGTHS, len(ranges))
lab = em.labels()
cut = np.flatnonzero((lab[1:] != lab[:-1]) | np.isin(np.arange(1, n), off))      # a run ends where the label changes or a chunk does
Fb = np.concatenate([[0], cut + 1]); Lb = np.concatenate([cut, [n - 1]])
Mb = 1 << lab[Fb].astype(np.int64); Kb = LENGTHS[lab[Fb]]
print("windows", n, "chunks", store.n_chunks, "longest chunk", int(np.diff(off).max()), "joined", int(joined.sum()), "contigs", len(ranges),
      "longest contig", int(max(b - a + 1 for a, b in ranges)), "runs of the final labels", Fb.size, flush=True)
t0 = time.perf_counter()
em.long_run_log_probs([0], [0], [1], [1])
print("lazy call (segment kernel re-run + one job): %.3f ms" % ((time.perf_counter() - t0) * 1e3), flush=True)
for name, F, L, M, Kk, jn in (("contigs x labels", Fa, La, Ma, Ka, joined), ("runs of the final labels", Fb, Lb, Mb, Kb, None)):
    for rep in range(5):
        t0 = time.perf_counter()
        none, some = em.long_run_log_probs(F, L, M, Kk, jn)
        t1 = time.perf_counter()
        iv = em.interval_log_probs(F, L, M)
        t2 = time.perf_counter()
        print("%s, rep %d: %d jobs: long runs %.3f ms, interval getter %.3f ms  (NaN %d; p_block in (0.01, 0.99): %d jobs)"
              % (name, rep, F.size, (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(np.isnan(none).sum() + np.isnan(iv).sum()),
                 int(np.sum((np.exp(some) > 0.01) & (np.exp(some) < 0.99)))), flush=True)
p = np.exp(em.long_run_log_probs(Fa, La, Ma, Ka, joined)[1]).reshape(-1, 4)
print("p_block of the first contigs (Err Dup Hap Col):", "; ".join(" ".join("%.4g" % x for x in row) for row in p[:4]), flush=True)
em.close()
