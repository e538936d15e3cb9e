"""Exact breakpoint posteriors (hf_get_breakpoints) on BASELINE configs[2] after EM to convergence and one more full pass, against the
interval getter over the same ranges, in one process:
  (a) hf_get_interval_log_probs over the jobs' ranges with mask U | V
  (b) hf_get_breakpoints over the same jobs (quantiles 0.025, 0.5, 0.975)
The jobs are those of `hmm_flagger --runBoundaries`: every two adjacent runs of the final labels whose touching windows lie in one chunk.
  python profiles/tools/breakpoints_cfg2.py            a warm call of each, then REPS calls of each, interleaved: host wall and the device
                                                       span of every call from a HIP event pair on the context's stream (a torch stream),
                                                       medians
  rocprofv3 --kernel-trace --stats ... -- python profiles/tools/breakpoints_cfg2.py      the same run for the per-kernel durations"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from flagger_amd import hmm, synth

REPS = 11
store = synth.config(2)
K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
stream = torch.cuda.Stream()
em = hmm.EMList(store, model, stream=stream.cuda_stream)
hmm.runHMMFlagger(em, model, 100, 1e-3)                      # EM to convergence; its last pass is the final inference
labels = em.labels()
off = np.asarray(store.chunk_off, np.int64)
n = store.n_windows
ctg = np.array(store.chunk_ctg)
chunk = np.searchsorted(off, np.arange(n), "right") - 1
chunk_start = np.zeros(n, bool)
chunk_start[off[:-1][np.diff(off) > 0]] = True
new_ctg = chunk_start & np.concatenate([[True], ctg[chunk[1:]] != ctg[chunk[:-1]]])
change = np.concatenate([[True], labels[1:] != labels[:-1]])
starts = np.flatnonzero(change | new_ctg)                    # the runs of final_label_runs_support.bed
ends = np.concatenate([starts[1:], [n]])
m = starts[1:]
inside = ~chunk_start[m] & (labels[m] != labels[m - 1])
c = chunk[m]
F = np.maximum(starts[:-1], off[c])[inside]
L = (np.minimum(ends[1:], off[c + 1]) - 1)[inside]
U = (1 << labels[m - 1].astype(np.int64))[inside]
V = (1 << labels[m].astype(np.int64))[inside]
print("windows %d, chunks %d, runs %d, jobs %d, candidate windows %d (longest job %d), pieces %d" % (
    n, store.n_chunks, starts.size, F.size, int((L - F).sum()), int((L - F).max()), int((L // 512 - (F + 1) // 512 + 1).sum())), flush=True)


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    t0 = time.perf_counter()
    out = call()
    wall = time.perf_counter() - t0
    e1.record(stream)
    e1.synchronize()
    return out, wall * 1e3, e0.elapsed_time(e1)


a = lambda: em.interval_log_probs(F, L, U | V)
b = lambda: em.breakpoints(F, L, U, V)
_, w, d = timed(a)
print("warm (a), with the lazy re-run of the segment kernel: host wall %.3f ms, device span %.3f ms" % (w, d), flush=True)
_, w, d = timed(b)
print("warm (b): host wall %.3f ms, device span %.3f ms" % (w, d), flush=True)
rec = {"a": [], "b": []}
for rep in range(REPS):
    for name, call in (("a", a), ("b", b)):
        out, w, d = timed(call)
        rec[name].append((w, d))
for name, what in (("a", "hf_get_interval_log_probs, mask U|V"), ("b", "hf_get_breakpoints")):
    w, d = np.array(rec[name]).T
    print("(%s) %s: %d calls: host wall median %.3f ms (min %.3f, max %.3f); device span median %.3f ms (min %.3f, max %.3f)"
          % (name, what, REPS, np.median(w), w.min(), w.max(), np.median(d), d.min(), d.max()), flush=True)
lpe, quant, mode, mode_p = out
fin = np.isfinite(lpe)
print("finite %d of %d; p_event median %.6g; mode_p median %.6g, below 0.99: %d; hi - lo in windows: median %d, max %d" % (
    int(fin.sum()), lpe.size, float(np.median(np.exp(lpe[fin]))), float(np.median(mode_p[fin])), int((mode_p[fin] < 0.99).sum()),
    int(np.median((quant[fin, 2] - quant[fin, 0]))), int((quant[fin, 2] - quant[fin, 0]).max())), flush=True)
em.close()
