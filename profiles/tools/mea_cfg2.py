"""Maximum-expected-accuracy decoding under minimum run lengths (hf_get_mea_labels) per chunk and over whole contigs, beside
hf_viterbi_minlen in the same process, on configs[2] after two EM iterations, with (3, 5, 1, 7), the identity gain and `joined` from
the contig names: host wall per call (median of 11), the expected gains against the unconstrained bound and the final BED's own rule,
and a check against the numpy reference (tests/mea_ref.py; --no-check skips it).  Writes profiles/mea_cfg2.txt (--out PATH: elsewhere).

Kernel times: run it under rocprofv3 --kernel-trace --stats --output-format csv with --no-check --no-write, then once more with
--stats KERNEL_STATS_CSV, which only appends the rows of the kernels involved (k_mea_rows, k_mlv_rows, k_mlv_fwd, k_mlv_back) to the
file."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = arg("--out", os.path.join(ROOT, "profiles", "mea_cfg2.txt"))
if arg("--stats"):
    rows = [ln for ln in open(arg("--stats")).read().splitlines() if ln.startswith('"Name"') or "k_mlv" in ln or "k_mea" in ln]
    with open(OUT, "a") as f:
        f.write("#\n# rocprofv3 --kernel-trace --stats, a run of its own (--no-check --no-write): 12 hf_viterbi_minlen, 14 hf_get_mea_labels per chunk (one\n"
                "# of them with all lengths 1) and 13 over whole contigs (k_mlv_fwd and k_mlv_back serve all three: 39 launches each)\n")
        f.write("\n".join(rows) + "\n")
    sys.exit(0)

import ctypes as C
import numpy as np
from flagger_amd import hmm, synth, _native as N
CHECK = "--no-check" not in sys.argv
WRITE = "--no-write" not in sys.argv
REPS = 11
ML = (3, 5, 1, 7)
lines = []


def say(s):
    print(s, flush=True)
    lines.append("#   " + s)


store = synth.config(2)
K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
em = hmm.EMList(store, model)
for _ in range(2):
    hmm.EM_runOneIterationForList(em, model); hmm.HMM_estimateParameters(model, 1e-3); hmm.HMM_resetEstimators(model)
hmm.EM_runOneIterationForList(em, model); hmm.HMM_resetEstimators(model)          # the full pass the getter answers for
joined = hmm.joined_chunks(store)
off = np.asarray(store.chunk_off, np.int64)
first = np.flatnonzero(~joined)
goff = np.concatenate([off[first], off[-1:]])
say("windows %d chunks %d (longest %d) groups %d (longest %d) K %d"
    % (store.n_windows, store.n_chunks, int(np.diff(off).max()), first.size, int(np.diff(goff).max()), K))
L = N.lib()
p = model.params()
lp = C.c_double(0.0)
a = (C.c_int32 * 4)(*ML)
jn = np.ascontiguousarray(joined, np.uint8)
jp = jn.ctypes.data_as(C.POINTER(C.c_uint8))
lab = np.empty(store.n_windows, np.int8)
labp = lab.ctypes.data_as(C.POINTER(C.c_int8))
blk = np.empty(store.n_chunks)
blkp = blk.ctypes.data_as(C.POINTER(C.c_double))
tot = C.c_double(0.0)


def wall(call):
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter(); call(); ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), min(ms)


def viterbi_minlen():
    N.check(L.hf_viterbi_minlen(em._h, p, a, None), "m"); N.check(L.hf_viterbi_minlen_finish(em._h, C.byref(lp), None), "f")


def mea_chunks():
    N.check(L.hf_get_mea_labels(em._h, None, a, None, labp, blkp, C.byref(tot)), "mea")


def mea_contigs():
    N.check(L.hf_get_mea_labels(em._h, None, a, jp, labp, blkp, C.byref(tot)), "mea joined")


viterbi_minlen(); mea_chunks(); mea_contigs()
say("hf_viterbi_minlen + finish, %s:              median %.3f ms, min %.3f ms" % ((ML,) + wall(viterbi_minlen)))
say("hf_get_mea_labels per chunk, %s:             median %.3f ms, min %.3f ms (labels and scores copied to the host)" % ((ML,) + wall(mea_chunks)))
say("hf_get_mea_labels over whole contigs, %s:    median %.3f ms, min %.3f ms" % ((ML,) + wall(mea_contigs)))
pc_lab, pc_blk, pc_tot = em.mea_labels(ML)
wc_lab, wc_blk, wc_tot = em.mea_labels(ML, joined)
free_lab, _, bound = em.mea_labels((1, 1, 1, 1))
say("expected correct windows: unconstrained %.6f, per chunk rule %.6f, whole-contig rule %.6f; labels differ from posterior argmax in "
    "%d and %d windows" % (bound, pc_tot, wc_tot, int(np.sum(pc_lab != free_lab)), int(np.sum(wc_lab != free_lab))))
if CHECK:
    import mea_ref, minlen_ref, posterior_ref, viterbi_ref
    post = posterior_ref.reference(store, model, synth.HIFI_ALPHA)[0]
    logA, _ = viterbi_ref.tables(store, model, synth.HIFI_ALPHA)
    G = mea_ref.gain_rows(post, logA, off, mea_ref.IDENTITY)
    for name, boff, labels, score in (("per chunk", off, pc_lab, pc_blk), ("whole contigs", goff, wc_lab, wc_blk[first])):
        ref_lab, ref_score = mea_ref.decode(G, boff, ML)
        val = mea_ref.expected_gain(labels, post, mea_ref.IDENTITY, boff)
        n = np.diff(boff)
        say("%s: admissible blocks %d / %d, supported chunks %d / %d; largest error per window of the block scores %.2e, of the labels' "
            "gain under the reference posterior %.2e; labels equal to the reference's on %.4f %% of windows"
            % (name, int(minlen_ref.admissible(labels, boff, ML).sum()), n.size, int(mea_ref.supported(labels, post, logA, off).sum()), off.size - 1,
               float(np.max(np.abs(score - ref_score) / n)), float(np.max(np.abs(val - ref_score) / n)), 100.0 * float(np.mean(labels == ref_lab))))
    rule = mea_ref.final_bed_rule(post, off, joined, ML)
    say("the final BED's own rule (argmax, short runs to Hap, in windows): expected correct windows %.6f, supported in %d / %d chunks"
        % (float(mea_ref.expected_gain(rule, post, mea_ref.IDENTITY, goff).sum()), int(mea_ref.supported(rule, post, logA, off).sum()), off.size - 1))
em.close()
if WRITE:
    with open(OUT, "w") as f:
        f.write("# Maximum-expected-accuracy decoding under minimum run lengths (hf_get_mea_labels) beside hf_viterbi_minlen in the same process on\n"
                "# BASELINE configs[2], trunc_exp_gaussian, HiFi alpha, after two EM iterations; identity gain; joined from the contig names.\n"
                "# profiles/tools/mea_cfg2.py (host walls: call .. results on the host, median of 11)\n#\n" + "\n".join(lines) + "\n")
