"""The raw outputs of the five range getters with a host front of their own shape (hf_get_run_lengths, hf_get_count_distribution,
hf_get_long_run_log_probs, hf_get_run_moments, hf_get_breakpoints) on one small track, for a byte-for-byte comparison of two builds.
  python profiles/tools/rg_front_bits.py OUT      writes every output array, raw, one after the other to OUT and prints their list
Run it once per build, each in a fresh process (HF_LIBRARY_VARIANT=<name> loads flagger_amd/csrc/variants/libhmmflagger_hip.<name>.so),
and compare the files with cmp: the inputs come from fixed seeds.

The track: chunks of 7, 5, 1, 6, 3, 40 windows (the tiny store of the suite), one chunk without windows, then 300, 250 and 90: 702
windows, the ninth chunk (362..611) lies across the grid line 512.  Jobs: 200 random ranges, every chunk, every run of three and of four
consecutive chunks (the one without windows inside some of them), the whole track, 40 jobs of one window; random masks.  Each getter on
HF_ALGO_SCAN and HF_ALGO_SEQ, with joined = NULL and with joins (the chunk without windows and its successor marked, which joins
nothing), at max_len 1 and 64, max_count 1 and 62; once with the default batch caps and once with every HF_*_BATCH_* variable at 1."""
import dataclasses, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from flagger_amd import _native as N
from flagger_amd import hmm, synth

LENGTHS = [7, 5, 1, 6, 3, 40, 0, 300, 250, 90]
JOINED = np.array([0, 1, 1, 1, 0, 1, 1, 1, 1, 0], bool)
CAPS = ["HF_RL_BATCH_PIECES", "HF_RL_BATCH_PARTS", "HF_CD_BATCH_PIECES", "HF_CD_BATCH_PARTS", "HF_LR_BATCH_PIECES", "HF_LR_BATCH_PARTS"]


def track():
    rng = np.random.default_rng(5150)
    full = [n for n in LENGTHS if n]
    st = synth.synthesize([n * 1000 for n in full], 1000, 10 ** 9, [20, 31], seed=int(rng.integers(1 << 30)), avg_alignment_len=2500)
    n = st.n_windows
    st.cov = rng.integers(0, 70, size=n).astype(np.uint16)
    st.mapq = np.where(rng.random(n) < 0.5, st.cov, (st.cov * rng.random(n)).astype(np.uint16)).astype(np.uint16)
    st.clip = np.where(rng.random(n) < 0.2, st.cov, 0).astype(np.uint16)
    reg = rng.integers(0, 2, size=n).astype(np.uint64)
    st.annot = (st.annot & np.uint64((1 << 58) - 1)) | (reg << np.uint64(58))
    src = np.cumsum([n > 0 for n in LENGTHS]) - 1               # the chunk without windows: a contig of its own, no bases
    some = np.array(LENGTHS) > 0
    ctg = [st.chunk_ctg[s] if k else "empty" for s, k in zip(src, some)]
    return dataclasses.replace(st, chunk_off=np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64), chunk_ctg=ctg,
                               chunk_ctg_len=st.chunk_ctg_len[src].copy(), chunk_s=np.where(some, st.chunk_s[src], 0).astype(np.int32),
                               chunk_e=np.where(some, st.chunk_e[src], 0).astype(np.int32))


def jobs(off):
    rng = np.random.default_rng(5151)
    n, C = int(off[-1]), off.size - 1
    a = rng.integers(0, n, 200); b = rng.integers(0, n, 200)
    F, L = list(np.minimum(a, b)), list(np.maximum(a, b))
    for k in (1, 3, 4):                                          # k consecutive chunks
        for c in range(C - k + 1):
            if off[c + k] > off[c]:
                F.append(off[c]); L.append(off[c + k] - 1)
    F.append(0); L.append(n - 1)
    one = rng.integers(0, n, 40)
    F += list(one); L += list(one)
    F, L = np.array(F, np.int64), np.array(L, np.int64)
    return F, L, rng.integers(1, 16, F.size), rng.integers(1, 9, F.size)


def breakpoint_jobs(off):
    rng = np.random.default_rng(5152)
    F, L = [], []
    for c in range(off.size - 1):
        m = int(off[c + 1] - off[c])
        for _ in range(12 if m >= 2 else 0):
            a, b = sorted(rng.choice(m, 2, replace=False))
            F.append(off[c] + a); L.append(off[c] + b)
    um = rng.integers(1, 15, len(F))
    vm = np.array([int(rng.choice([v for v in range(1, 16) if not v & u])) for u in um])
    return np.array(F, np.int64), np.array(L, np.int64), um, vm


store = track()
off = np.asarray(store.chunk_off, np.int64)
F, L, M, ML = jobs(off)
BF, BL, BU, BV = breakpoint_jobs(off)
spans = np.searchsorted(off, L, "right") - np.searchsorted(off, F, "right")
assert store.n_windows == 702 and off[8] < 512 < off[9] and np.sum(spans >= 2) >= 20 and np.sum(F == L) >= 40
out, names = [], []
for algo, tag in ((N.HF_ALGO_SCAN, "scan"), (N.HF_ALGO_SEQ, "seq")):
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, 3, store, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model, algo=algo)
    hmm.EM_runOneIterationForList(em, model); hmm.HMM_estimateParameters(model, 1e-3); hmm.HMM_resetEstimators(model)
    hmm.EM_runOneIterationForList(em, model)
    for caps in ("default", "one"):
        for name in CAPS:
            if caps == "one":
                os.environ[name] = "1"
            else:
                os.environ.pop(name, None)
        def put(what, *arrays):
            for i, a in enumerate(arrays):
                names.append("%s caps=%s %s[%d] %s%s" % (tag, caps, what, i, a.dtype, list(a.shape)))
                out.append(np.ascontiguousarray(a))
        for joins, jt in ((None, "apart"), (JOINED, "joined")):
            for ml in (1, 64):
                put("run_lengths %s L=%d" % (jt, ml), em.run_lengths(F, L, M, ml, joins))
            put("long_run %s" % jt, *em.long_run_log_probs(F, L, M, ML, joins))
            put("run_moments %s" % jt, *em.run_moments(F, L, M, joins))
        for mc in (1, 62):
            put("count_distribution K=%d" % mc, em.count_distribution(F, L, M, mc))
        put("breakpoints", *em.breakpoints(BF, BL, BU, BV))
    em.close()
with open(sys.argv[1], "wb") as f:
    for a in out:
        f.write(a.tobytes())
print("\n".join(names))
print("jobs %d (of one window %d, over three chunks or more %d), breakpoint jobs %d, arrays %d, bytes %d, NaN %d"
      % (F.size, int(np.sum(F == L)), int(np.sum(spans >= 2)), BF.size, len(out), sum(a.nbytes for a in out),
         sum(int(np.isnan(a).sum()) for a in out if a.dtype == np.float64)))
