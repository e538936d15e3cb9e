"""Minimum-run-length Viterbi over whole contigs (hf_viterbi_minlen_joined) against hf_viterbi_minlen in the same process on configs[2]
after two EM iterations, with (3, 5, 1, 7) and `joined` from the contig names: host wall per call (median of 11), what the whole-contig
rule costs in nats beyond the per-chunk rule, how many short runs the per-chunk labels leave inside the contigs, and a check against the
numpy reference (tests/minlen_joined_ref.py; --no-check skips it).  Writes profiles/minlen_joined_cfg2.txt (--out PATH: elsewhere).

Kernel times: run it under rocprofv3 --kernel-trace --stats --output-format csv with --no-check --no-write, then once more with
--stats KERNEL_STATS_CSV, which only appends the rows of the decoder's kernels (k_mlv_rows, k_mlv_fwd, k_mlvj_fwd, k_mlv_back) to the
file."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = arg("--out", os.path.join(ROOT, "profiles", "minlen_joined_cfg2.txt"))
if arg("--stats"):
    rows = [ln for ln in open(arg("--stats")).read().splitlines() if ln.startswith('"Name"') or "k_mlv" in ln]
    with open(OUT, "a") as f:
        f.write("#\n# rocprofv3 --kernel-trace --stats, a run of its own (--no-check --no-write): 13 per-chunk and 13 joined decodes\n")
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


def wall(call):
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter(); call(); ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), min(ms)


def per_chunk():
    N.check(L.hf_viterbi_minlen(em._h, p, a, None), "m"); N.check(L.hf_viterbi_minlen_finish(em._h, C.byref(lp), None), "f")


def whole():
    N.check(L.hf_viterbi_minlen_joined(em._h, p, a, jp, None), "j"); N.check(L.hf_viterbi_minlen_finish(em._h, C.byref(lp), None), "f")


per_chunk(); whole()
say("hf_viterbi_minlen + finish, %s:         median %.3f ms, min %.3f ms" % ((ML,) + wall(per_chunk)))
say("hf_viterbi_minlen_joined + finish, %s:  median %.3f ms, min %.3f ms" % ((ML,) + wall(whole)))
pc_lab, pc_ll, pc_tot = em.viterbi_minlen(model, ML)
lab, ll, tot = em.viterbi_minlen(model, ML, joined)


def short_inner(labels):
    n = 0
    for g in range(goff.size - 1):
        x = labels[goff[g]:goff[g + 1]]
        cut = np.flatnonzero(np.diff(x)) + 1
        s, e = np.concatenate([[0], cut]), np.concatenate([cut, [x.size]])
        inner = (s > 0) & (e < x.size)
        n += int(np.sum(inner & (e - s < np.asarray(ML)[x[s]])))
    return n


say("log-probability per chunk rule %.6f, whole-contig rule %.6f: the whole-contig rule costs %.6f nats more"
    % (pc_tot, tot, pc_tot - tot))
say("short runs inside the contigs: %d in the per-chunk labels, %d in the whole-contig labels; labels differ in %d windows"
    % (short_inner(pc_lab), short_inner(lab), int(np.sum(pc_lab != lab))))
if CHECK:
    import minlen_joined_ref as JR, minlen_ref, viterbi_ref
    logA, logend = viterbi_ref.tables(store, model, synth.HIFI_ALPHA)
    ref_lab, ref_ll, _ = JR.viterbi_minlen_joined(logA, logend, off, joined, ML)
    ok = minlen_ref.admissible(lab, goff, ML)
    val = JR.group_sums(viterbi_ref.path_log_prob(logA, logend, off, lab), off, joined)
    nz = ref_ll != 0.0
    say("admissible groups %d / %d; max relative error of the group scores %.2e, of path_log_prob(labels) %.2e; labels equal to the "
        "reference's on %.4f %% of windows" % (int(ok.sum()), ok.size, float(np.max(np.abs(ll - ref_ll)[nz] / np.abs(ref_ll[nz]))),
                                              float(np.max(np.abs(val - ref_ll)[nz] / np.abs(ref_ll[nz]))), 100.0 * float(np.mean(lab == ref_lab))))
em.close()
if WRITE:
    with open(OUT, "w") as f:
        f.write("# Minimum-run-length Viterbi over whole contigs (hf_viterbi_minlen_joined) against hf_viterbi_minlen in the same process on\n"
                "# BASELINE configs[2], trunc_exp_gaussian, HiFi alpha, after two EM iterations; joined from the contig names.\n"
                "# profiles/tools/minlen_joined_cfg2.py (host walls: launch .. finish, median of 11)\n#\n" + "\n".join(lines) + "\n")
