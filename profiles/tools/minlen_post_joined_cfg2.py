"""The posterior and the sampler under minimum run lengths over whole contigs (hf_minlen_posterior_joined,
hf_sample_paths_minlen_joined) against the per-chunk entry points in the same process on configs[2] after two EM iterations, with
(3, 5, 1, 7), `joined` from the contig names and 64 samples: host wall per call (median of 11), the masses per contig under both rules,
how many of the per-chunk sampler's (sample, contig) pairs obey the whole-contig rule, and a check of the posterior against the numpy
reference (tests/minlen_sum_joined_ref.py; --no-check skips it).  Writes profiles/minlen_post_joined_cfg2.txt (--out PATH: elsewhere).

Kernel times: run it under rocprofv3 --kernel-trace --stats --output-format csv with --no-check --no-write, then once more with
--stats KERNEL_STATS_CSV, which only appends the rows of the two decoders' kernels (k_dec_rows_win, k_mlp_*, k_mlpj_*, k_mls_*,
k_mlsj_bound) to the file."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = arg("--out", os.path.join(ROOT, "profiles", "minlen_post_joined_cfg2.txt"))
if arg("--stats"):
    rows = [ln for ln in open(arg("--stats")).read().splitlines()
            if ln.startswith('"Name"') or any(k in ln for k in ("k_dec_rows_win", "k_mlp", "k_mls"))]
    with open(OUT, "a") as f:
        f.write("#\n# rocprofv3 --kernel-trace --stats, a run of its own (--no-check --no-write): 13 calls of each of the four entry points;\n"
                "# k_dec_rows_win runs in all four, k_mls_draw / k_mls_final / k_mls_back in both samplers\n")
        f.write("\n".join(rows) + "\n")
    sys.exit(0)

import ctypes as C
import numpy as np
from flagger_amd import hmm, synth, _native as N
CHECK = "--no-check" not in sys.argv
WRITE = "--no-write" not in sys.argv
REPS = 11
ML = (3, 5, 1, 7)
K_S = 64
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
say("windows %d chunks %d (longest %d) groups %d (longest %d) K %d samples %d"
    % (store.n_windows, store.n_chunks, int(np.diff(off).max()), first.size, int(np.diff(goff).max()), K, K_S))
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


def post_chunk():
    N.check(L.hf_minlen_posterior(em._h, p, a, None), "p"); N.check(L.hf_minlen_posterior_finish(em._h, C.byref(lp), None), "f")


def post_joined():
    N.check(L.hf_minlen_posterior_joined(em._h, p, a, jp, None), "pj"); N.check(L.hf_minlen_posterior_finish(em._h, C.byref(lp), None), "f")


def smp_chunk():
    N.check(L.hf_sample_paths_minlen(em._h, p, a, 0, K_S, 5, None), "s"); N.check(L.hf_sample_minlen_finish(em._h, None), "f")


def smp_joined():
    N.check(L.hf_sample_paths_minlen_joined(em._h, p, a, jp, 0, K_S, 5, None), "sj"); N.check(L.hf_sample_minlen_finish(em._h, None), "f")


calls = (("hf_minlen_posterior", post_chunk), ("hf_minlen_posterior_joined", post_joined),
         ("hf_sample_paths_minlen", smp_chunk), ("hf_sample_paths_minlen_joined", smp_joined))
for _, f in calls:
    f()
for name, f in calls:
    say("%-30s + finish, %s: median %.3f ms, min %.3f ms" % ((name, ML) + wall(f)))
pc = em.minlen_posterior(model, ML)
pc_mass = pc.chunk_log_mass.copy()
jr = em.minlen_posterior(model, ML, joined)
post = jr.posterior()
say("log_mass of the track: per-chunk rule %.6f, whole-contig rule %.6f" % (pc.log_mass, jr.log_mass))
say("per contig (first chunk, chunks, windows, log_mass per-chunk rule, log_mass whole-contig rule):")
ends = np.concatenate([first[1:], [store.n_chunks]])
for g, (c0, c1) in enumerate(zip(first, ends)):
    say("  %-12s %4d %3d %7d %14.6f %14.6f" % (store.chunk_ctg[c0], c0, c1 - c0, goff[g + 1] - goff[g], float(np.sum(pc_mass[c0:c1])),
                                             float(jr.chunk_log_mass[c0])))


def short_inner(labels, g):
    x = labels[goff[g]:goff[g + 1]]
    cut = np.flatnonzero(np.diff(x)) + 1
    s, e = np.concatenate([[0], cut]), np.concatenate([cut, [x.size]])
    inner = (s > 0) & (e < x.size)
    return int(np.sum(inner & (e - s < np.asarray(ML)[x[s]])))


lab_pc = em.sample_paths_minlen(model, ML, K_S, 5)
lab_j = em.sample_paths_minlen(model, ML, K_S, 5, joined=joined)
sh_pc = np.array([[short_inner(row, g) for g in range(first.size)] for row in lab_pc])
sh_j = np.array([[short_inner(row, g) for g in range(first.size)] for row in lab_j])
say("(sample, contig) pairs that obey the whole-contig rule: hf_sample_paths_minlen %d of %d, hf_sample_paths_minlen_joined %d of %d"
    % (int(np.sum(sh_pc == 0)), sh_pc.size, int(np.sum(sh_j == 0)), sh_j.size))
say("short runs inside the contigs in %d samples: per-chunk sampler %d, whole-contig sampler %d" % (K_S, int(sh_pc.sum()), int(sh_j.sum())))
if CHECK:
    import minlen_sum_joined_ref as R
    ref = R.posterior(store, model, synth.HIFI_ALPHA, joined, ML)
    big = ref[0] >= 1e-250
    say("against the numpy reference: log_mass max |dev| %.2e, log Z_adm max relative %.2e, post max relative %.2e over %d entries"
        % (float(np.max(np.abs(jr.chunk_log_mass - ref[1]))), float(np.max(np.abs(jr.chunk_log_z_adm - ref[2])[first] / np.abs(ref[2][first]))),
           float(np.max(np.abs(post[big] - ref[0][big]) / ref[0][big])), int(big.sum())))
em.close()
if WRITE:
    with open(OUT, "w") as f:
        f.write("# The posterior and the sampler under minimum run lengths over whole contigs (hf_minlen_posterior_joined,\n"
                "# hf_sample_paths_minlen_joined) against the per-chunk entry points in the same process on BASELINE configs[2],\n"
                "# trunc_exp_gaussian, HiFi alpha, after two EM iterations; joined from the contig names.\n"
                "# profiles/tools/minlen_post_joined_cfg2.py (host walls: launch .. finish, median of 11)\n#\n" + "\n".join(lines) + "\n")
