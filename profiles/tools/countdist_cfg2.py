"""The exact distribution of label totals (hf_get_count_distribution) on BASELINE configs[2] after two EM iterations and one more full pass.
  python profiles/tools/countdist_cfg2.py walks    the lazy call (one one-window job), then five times: one walk over the track (one job,
                                                   Hap) of hf_get_count_distribution at K = 8 and at K = 62, of hf_get_run_lengths at
                                                   L = 64 and of hf_get_count_moments, in this order; run it under
                                                   rocprofv3 --kernel-trace --stats --output-format csv (no counters in that run)
  python profiles/tools/countdist_cfg2.py kernels DIR   the kernel times of that run from the trace under DIR: k_cd_piece / k_cd_chain
                                                   by K (their launches alternate K = 8, K = 62), k_rl_piece, k_mo_piece
  python profiles/tools/countdist_cfg2.py regions  10 000 regions of 1..64 windows x Err, Dup, Hap, Col, Err+Dup+Col at K = 62 and K = 8,
                                                   five calls each: the host wall of a call
  python profiles/tools/countdist_cfg2.py cli      wall time of `hmm_flagger -n 3 --regionProbs` (1 000 regions of 1..64 windows) without
                                                   and with --totalsDistribution 62, 3 runs each
Prints the host wall of every call (the kernel times come from rocprofv3)."""
import csv, glob, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

leg = sys.argv[1] if len(sys.argv) > 1 else "walks"
if leg == "kernels":
    rows = []
    for path in glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    def times(word):
        return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if word in r["Kernel_Name"]]
    def line(name, t):
        print("%-28s n %d  min %.1f  median %.1f  max %.1f" % (name, len(t), min(t), float(np.median(t)), max(t)) if t else "%-28s none" % name)
    piece, chain = times("k_cd_piece"), times("k_cd_chain")[1:]          # (the lazy call has no piece: its chain launch comes first)
    line("k_cd_piece  K = 8", piece[0::2]); line("k_cd_piece  K = 62", piece[1::2])
    line("k_cd_chain  K = 8", chain[0::2]); line("k_cd_chain  K = 62", chain[1::2])
    for k in ("k_rl_piece", "k_rl_chain", "k_mo_piece", "k_mo_chain"):
        line(k, times(k))
    sys.exit(0)

from flagger_amd import hmm, synth
store = synth.config(2)
off = np.asarray(store.chunk_off, np.int64)
n = store.n_windows
rng = np.random.default_rng(17)


def regions(count):
    """`count` ranges of 1..64 windows, each inside one contig (a run of chunks with one name)."""
    ctg = list(store.chunk_ctg)
    c = rng.integers(0, len(ctg), count)
    a = off[c] + (rng.random(count) * (off[c + 1] - off[c])).astype(np.int64)
    b = np.minimum(a + rng.integers(1, 65, count) - 1, n - 1)
    for i in range(count):                                               # (clip at the contig's end)
        cb = int(np.searchsorted(off, b[i], "right")) - 1
        while ctg[cb] != ctg[c[i]]:
            cb -= 1
            b[i] = off[cb + 1] - 1
    return a, b


if leg == "cli":
    CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
    a, b = regions(1000)
    with tempfile.TemporaryDirectory() as d:
        binp, bed = os.path.join(d, "cfg2.bin"), os.path.join(d, "regions.bed")
        store.write_bin(binp)
        with open(bed, "w") as f:
            for i in range(a.size):
                ca, cb = int(np.searchsorted(off, a[i], "right")) - 1, int(np.searchsorted(off, b[i], "right")) - 1
                f.write("%s\t%d\t%d\tr%d\n" % (store.chunk_ctg[ca], int(store.chunk_s[ca]) + int(a[i] - off[ca]) * 4000,
                                              int(store.chunk_s[cb]) + int(b[i] - off[cb]) * 4000 + 1, i))
        for extra in ([], ["--totalsDistribution", "62"]):
            for rep in range(3):
                o = os.path.join(d, "o%d%d" % (len(extra), rep))
                os.mkdir(o)
                t0 = time.perf_counter()
                r = subprocess.run([CLI, "-i", binp, "-o", o, "-W", "4000", "-n", "3", "--regionProbs", bed] + extra, capture_output=True, text=True)
                dt = time.perf_counter() - t0
                assert r.returncode == 0, r.stderr[-2000:]
                line = [l for l in r.stderr.splitlines() if "region_label_totals_exact" in l]
                print("hmm_flagger -n 3 --regionProbs %s: %.1f ms wall%s" % (" ".join(extra), dt * 1e3, ("; " + line[0].split("] ", 2)[-1]) if line else ""), flush=True)
        rows = open(os.path.join(o, "region_label_totals_exact.tsv")).read().splitlines()
        print("\n".join("\t".join(l.split("\t")[:14]) for l in rows[:11]))
    sys.exit(0)
K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
em = hmm.EMList(store, model)
for _ in range(2):
    hmm.EM_runOneIterationForList(em, model); hmm.HMM_estimateParameters(model, 1e-3); hmm.HMM_resetEstimators(model)
hmm.EM_runOneIterationForList(em, model)
print("windows", n, "chunks", store.n_chunks, flush=True)
t0 = time.perf_counter()
em.count_distribution([0], [0], [1], 62)
print("lazy call (segment kernel re-run + one job): %.3f ms" % ((time.perf_counter() - t0) * 1e3), flush=True)
if leg == "walks":
    for rep in range(5):
        t0 = time.perf_counter()
        d8 = em.count_distribution([0], [n - 1], [4], 8)
        t1 = time.perf_counter()
        d62 = em.count_distribution([0], [n - 1], [4], 62)
        t2 = time.perf_counter()
        em.run_lengths([0], [n - 1], [4], 64)
        t3 = time.perf_counter()
        em.count_moments([0], [n - 1], [4])
        t4 = time.perf_counter()
        print("one walk, rep %d: count distribution K = 8 %.3f ms, K = 62 %.3f ms, run lengths L = 64 %.3f ms, count moments %.3f ms  (p_gtK %.6g %.6g)"
              % (rep, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, d8[0, 9], d62[0, 63]), flush=True)
else:
    a, b = regions(10000)
    F, L, M = np.repeat(a, 5), np.repeat(b, 5), np.tile([1, 2, 4, 8, 11], a.size)
    print("regions", a.size, "jobs", F.size, "windows", int((b - a + 1).sum()), "crossing a chunk boundary",
          int(np.sum(np.searchsorted(off, a, "right") != np.searchsorted(off, b, "right"))), flush=True)
    for Kc in (62, 8):
        for rep in range(5):
            t0 = time.perf_counter()
            d = em.count_distribution(F, L, M, Kc)
            print("rep %d: %d jobs at K = %d: %.3f ms  (NaN %d, largest |sum - 1| %.3e, jobs with p_gtK > 0: %d)"
                  % (rep, F.size, Kc, (time.perf_counter() - t0) * 1e3, int(np.isnan(d).sum()), float(np.abs(d.sum(axis=1) - 1).max()), int(np.sum(d[:, -1] > 0))), flush=True)
    mean, var = em.count_moments(F, L, M)
    k = np.arange(63)
    fits = (L - F + 1) <= 62
    d = em.count_distribution(F, L, M, 62)
    print("mean of the bins against hf_get_count_moments, jobs of at most 62 windows (%d): largest deviation %.3e" % (int(fits.sum()), float(np.abs((d[fits, :63] * k).sum(axis=1) - mean[fits]).max())))
    p10 = d[:, 10:].sum(axis=1)
    print("example: P(at least 10 windows Err+Dup+Col) of the first regions of at least 32 windows:",
          " ".join("%.4g" % x for x in p10[(M == 11) & (L - F + 1 >= 32)][:8]))
em.close()
