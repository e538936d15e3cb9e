"""Exact path entropy and labelling log-probability (hf_get_path_entropy, hf_get_path_log_probs, hf_get_entropy_profile) on BASELINE
configs[2] after two EM iterations and one more full pass.
  python profiles/tools/entropy_cfg2.py jobs   the lazy call, then the job set of `hmm_flagger --jointEntropy` (the whole track and every
                                               contig: the entropy, the log-probability of the pass's labels, the profile's marg), 5
                                               times; then one walk each over the track (one job), 5 times; under rocprofv3
                                               --kernel-trace --stats for the kernel times
  python profiles/tools/entropy_cfg2.py cli    wall time of `hmm_flagger -n 3` without and with --jointEntropy, 3 runs each
Prints the host wall of every call (the kernel times come from rocprofv3)."""
import os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from flagger_amd import hmm, synth

leg = sys.argv[1] if len(sys.argv) > 1 else "jobs"
store = synth.config(2)
if leg == "cli":
    CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
    with tempfile.TemporaryDirectory() as d:
        binp = os.path.join(d, "cfg2.bin")
        store.write_bin(binp)
        for extra in ([], ["--jointEntropy"]):
            for rep in range(3):
                o = os.path.join(d, "o%d%d" % (len(extra), rep))
                os.mkdir(o)
                t0 = time.perf_counter()
                r = subprocess.run([CLI, "-i", binp, "-o", o, "-W", "4000", "-n", "3"] + extra, capture_output=True, text=True)
                dt = time.perf_counter() - t0
                assert r.returncode == 0, r.stderr[-2000:]
                line = [l for l in r.stderr.splitlines() if "path_uncertainty" in l]
                print("hmm_flagger -n 3 %s: %.1f ms wall%s" % (" ".join(extra), dt * 1e3, ("; " + line[0].split("] ", 2)[-1]) if line else ""), flush=True)
        print(open(os.path.join(o, "path_uncertainty.tsv")).read()[:1200])
    sys.exit(0)
K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
em = hmm.EMList(store, model)
for _ in range(2):
    hmm.EM_runOneIterationForList(em, model); hmm.HMM_estimateParameters(model, 1e-3); hmm.HMM_resetEstimators(model)
hmm.EM_runOneIterationForList(em, model)
off = np.asarray(store.chunk_off, np.int64)
n = store.n_windows
ctg = list(store.chunk_ctg)
ranges = [(0, n - 1)]
for c in range(len(ctg)):                          # (the contigs of this track are runs of consecutive chunks)
    if c > 0 and ctg[c] == ctg[c - 1]:
        ranges[-1] = (ranges[-1][0], int(off[c + 1]) - 1)
    else:
        ranges.append((int(off[c]), int(off[c + 1]) - 1))
F = np.array([a for a, _ in ranges], np.int64); L = np.array([b for _, b in ranges], np.int64)
labels = em.labels()
print("windows", n, "chunks", store.n_chunks, "scopes", len(ranges), flush=True)
t0 = time.perf_counter()
em.path_entropy([0], [0])
print("lazy call (segment kernel re-run + one job): %.3f ms" % ((time.perf_counter() - t0) * 1e3), flush=True)
for rep in range(5):
    t0 = time.perf_counter()
    h = em.path_entropy(F, L)
    t1 = time.perf_counter()
    lp = em.path_log_probs(F, L, labels)
    t2 = time.perf_counter()
    marg, _ = em.entropy_profile()
    t3 = time.perf_counter()
    print("rep %d: %d scopes: entropy %.3f ms, log-probability %.3f ms, profile %.3f ms  (all: %.6g nats, %.6g per window, window sum %.6g, labels %.6g)"
          % (rep, F.size, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, h[0], h[0] / n, marg.sum(), lp[0]), flush=True)
for rep in range(5):
    t0 = time.perf_counter()
    em.path_entropy([0], [n - 1])
    t1 = time.perf_counter()
    em.path_log_probs([0], [n - 1], labels)
    t2 = time.perf_counter()
    em.count_moments([0], [n - 1], [4])
    t3 = time.perf_counter()
    print("one walk, rep %d: entropy %.3f ms, log-probability %.3f ms, count moments %.3f ms" % (rep, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3), flush=True)
em.close()
