"""The exact block-length spectrum (hf_get_run_lengths) on BASELINE configs[2] after two EM iterations and one more full pass.
  python profiles/tools/runlen_cfg2.py walks   the lazy call, then the job set of `hmm_flagger --runLengths 64` (the whole track and every
                                               contig x Err, Dup, Hap, Col, Err+Dup+Col, chunks of a contig joined), 5 times; then, 5
                                               times each, one walk over the track (one job, Hap) of hf_get_run_lengths at L = 8 and at
                                               L = 64 and, in the same process, one walk of hf_get_run_moments; under
                                               rocprofv3 --kernel-trace --stats (no counters in that run) for the kernel times
  python profiles/tools/runlen_cfg2.py cli     wall time of `hmm_flagger -n 3` without and with --runLengths 64, 3 runs each
Prints the host wall of every call (the kernel times come from rocprofv3)."""
import os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from flagger_amd import hmm, synth

leg = sys.argv[1] if len(sys.argv) > 1 else "walks"
store = synth.config(2)
if leg == "cli":
    CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
    with tempfile.TemporaryDirectory() as d:
        binp = os.path.join(d, "cfg2.bin")
        store.write_bin(binp)
        for extra in ([], ["--runLengths", "64"]):
            for rep in range(3):
                o = os.path.join(d, "o%d%d" % (len(extra), rep))
                os.mkdir(o)
                t0 = time.perf_counter()
                r = subprocess.run([CLI, "-i", binp, "-o", o, "-W", "4000", "-n", "3"] + extra, capture_output=True, text=True)
                dt = time.perf_counter() - t0
                assert r.returncode == 0, r.stderr[-2000:]
                line = [l for l in r.stderr.splitlines() if "label_block_lengths_exact" in l]
                print("hmm_flagger -n 3 %s: %.1f ms wall%s" % (" ".join(extra), dt * 1e3, ("; " + line[0].split("] ", 2)[-1]) if line else ""), flush=True)
        rows = [l.split("\t") for l in open(os.path.join(o, "label_block_lengths_exact.tsv")).read().splitlines()]
        print("\n".join("\t".join(r) for r in rows[:1] + [r for r in rows if r[0] == "all" and r[1] == "Hap" and r[2] in ("1", "2", "3", "4", "8", "16", "32", "64", ">64")]))
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
joined = np.array([c > 0 and ctg[c] == ctg[c - 1] for c in range(len(ctg))], bool)
ranges = [(0, n - 1)]
for c in range(len(ctg)):                          # (the contigs of this track are runs of consecutive chunks)
    if joined[c]:
        ranges[-1] = (ranges[-1][0], int(off[c + 1]) - 1)
    else:
        ranges.append((int(off[c]), int(off[c + 1]) - 1))
F = np.repeat([a for a, _ in ranges], 5); L = np.repeat([b for _, b in ranges], 5)
M = np.tile([1, 2, 4, 8, 11], len(ranges))
print("windows", n, "chunks", store.n_chunks, "joined", int(joined.sum()), "scopes", len(ranges), "jobs", F.size, flush=True)
t0 = time.perf_counter()
em.run_lengths([0], [0], [1], 64)
print("lazy call (segment kernel re-run + one job): %.3f ms" % ((time.perf_counter() - t0) * 1e3), flush=True)
for rep in range(5):
    t0 = time.perf_counter()
    spec = em.run_lengths(F, L, M, 64, joined)
    print("rep %d: %d jobs at L = 64: %.3f ms  (NaN %d; all, Hap: blocks %.6g, of 1 window %.6g, of more than 64 %.6g)"
          % (rep, F.size, (time.perf_counter() - t0) * 1e3, int(np.isnan(spec).sum()), spec[2].sum(), spec[2, 0], spec[2, 64]), flush=True)
mean, _ = em.run_moments(F[:5], L[:5], M[:5], joined)
print("all: sum of the bins %s, run moments' mean %s" % (" ".join("%.10g" % x for x in spec[:5].sum(axis=1)), " ".join("%.10g" % x for x in mean)), flush=True)
for rep in range(5):
    t0 = time.perf_counter()
    em.run_lengths([0], [n - 1], [4], 8, joined)
    t1 = time.perf_counter()
    em.run_lengths([0], [n - 1], [4], 64, joined)
    t2 = time.perf_counter()
    em.run_moments([0], [n - 1], [4], joined)
    t3 = time.perf_counter()
    print("one walk, rep %d: run lengths L = 8 %.3f ms, L = 64 %.3f ms, run moments %.3f ms" % (rep, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3), flush=True)
em.close()
