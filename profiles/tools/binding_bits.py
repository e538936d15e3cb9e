"""What the Python binding (flagger_amd/hmm.py) returns and writes on one small track, for a byte-for-byte comparison of two trees.
  python profiles/tools/binding_bits.py OUT DIR    writes every returned array, raw, one after the other to OUT, then the bytes of every
                                                   file the three runHMMFlagger variants wrote under DIR, and prints the list of both
Run it once per tree, each in a fresh process, and compare the OUT files with cmp: the inputs come from fixed seeds, and the tool uses
public names only, so the same file runs in a checkout of the commit before.

The track: the grid store of tests/geometry_cases.py (case 0: trunc-exp-Gaussian, HiFi alpha, two regions; 4 173 windows in 13 chunks,
five of them joined to their predecessor), its 903 jobs with their masks and region filters, the breakpoint jobs among them (first <
last inside one chunk, the right mask the complement of the left).  Every public method of EMList, EMBatch and MultiEMList (two ranks,
loopback transport) once, with `joined` absent and present where the method takes it, and runHMMFlagger plain, under minimum run
lengths over joined chunks and with the alpha fit, four iterations each with the parameter files of every iteration.
Left out: the eight EMList methods that take raw device pointers (rank_total, copy_chunk_stats, finish_gathered, finish_exchange,
bind_chunk_stats, write_flag_row, reduce_chunks, reduce_chunks_indexed: dist.py drives them inside a process group; they convert
nothing), and the values of what differs from run to run by nature (times, capacities from free memory): those are called, and only
their keys or types are listed."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from flagger_amd import _native as N
from flagger_amd import hmm
import geometry_cases as G

OUT, DIR = sys.argv[1], sys.argv[2]
store, model0, alpha, (F, L, M, R) = G.case(0, 0)
JOINED = G.joins()
MIN_LEN = G.MINLEN_SETS[0]
off = np.asarray(store.chunk_off, np.int64)
inside = (np.searchsorted(off, F, "right") == np.searchsorted(off, L, "right")) & (F < L) & (M != 15)
BF, BL, BU, BV = F[inside], L[inside], M[inside], 15 - M[inside]
assert store.n_windows == 4173 and JOINED.sum() == 5 and F.size == 903 and BF.size == 78
out, names = [], []


def put(what, *values):
    for i, a in enumerate(values):
        a = np.array(a, order="C")                   # a copy: some results are buffers the list writes again (em_iterate's statistics)
        names.append("%s[%d] %s%s" % (what, i, a.dtype, list(a.shape)))
        out.append(a)


def note(what, value):
    names.append("%s: %s" % (what, value))


def fresh():
    return model0.copy()


def full_pass(em):
    em.launch(model0)
    return em.finish()


# ---- EMList ----
em = hmm.EMList(store, model0)
note("create_phases has a total", "total" in em.create_phases())
put("properties", [em.stats_mode, em.seg_launches, em.seg_cached_steps, em.sub_passes, em.sub_pass_windows(0)])
put("launch finish", full_pass(em))
em.check()
put("labels", em.labels())
put("posterior", em.posterior(), em.posterior(500, 30))
put("forward_backward", *em.forward_backward(1000, 100))
m = fresh()
put("em_iterate", [em.em_iterate(m, True, 1e-3)], m.estimators, m.param_vector())
put("viterbi", *em.viterbi(model0))
for joins, jt in ((None, "apart"), (JOINED, "joined")):
    kw = {} if joins is None else {"joined": joins}
    put("viterbi_minlen " + jt, *em.viterbi_minlen(model0, MIN_LEN, **kw))
    mp = em.minlen_posterior(model0, MIN_LEN, **kw)
    put("minlen_posterior " + jt, mp.labels, mp.chunk_log_mass, mp.chunk_log_z_adm, [mp.log_mass], mp.posterior(), mp.posterior(3000, 17))
    put("estep_minlen " + jt, *em.estep_minlen(model0, MIN_LEN, **kw))
    put("minlen_pair_posterior " + jt, em.minlen_pair_posterior(), em.minlen_pair_posterior(510, 8))
    put("minlen_em_chunk_stats " + jt, *em.minlen_em_chunk_stats())
    m = fresh()
    put("em_iterate_minlen " + jt, [em.em_iterate_minlen(m, MIN_LEN, True, 1e-3, **kw)], m.estimators, [em.last_log_z], m.param_vector())
    put("sample_paths_minlen " + jt, em.sample_paths_minlen(model0, MIN_LEN, 3, 41, first_sample=2, **kw))
note("sample_capacity", type(em.sample_capacity).__name__)
note("minlen_sample_capacity", type(em.minlen_sample_capacity(MIN_LEN)).__name__)
put("sample_paths", em.sample_paths(model0, 3, 41, first_sample=1))
put("pass again", full_pass(em))
gain = np.arange(16, dtype=np.float64).reshape(4, 4) / 16 + np.eye(4)
for joins, jt in ((None, "apart"), (JOINED, "joined")):
    kw = {} if joins is None else {"joined": joins}
    put("mea_labels " + jt, *em.mea_labels(MIN_LEN, **kw))
    put("mea_labels gain " + jt, *em.mea_labels(MIN_LEN, gain=gain, **kw))
    put("run_moments " + jt, *em.run_moments(F, L, M, **kw))
    put("long_run_log_probs " + jt, *em.long_run_log_probs(F, L, M, 1 + (F % 7), **kw))
    put("run_lengths " + jt, em.run_lengths(F, L, M, 9, **kw))
put("interval_log_probs", em.interval_log_probs(F, L, M), em.interval_log_probs(F[:5], 4172, 15))
put("count_moments", *em.count_moments(F, L, M), *em.count_moments(F, L, M, R, "bases"))
put("count_distribution", em.count_distribution(F, L, M, 6))
put("path_entropy", em.path_entropy(F, L))
put("path_log_probs", em.path_log_probs(F, L, em.labels()), em.path_log_probs(F, L, em.labels().astype(np.int64)))
put("entropy_profile", *em.entropy_profile(), *em.entropy_profile(100, 40))
put("breakpoints", *em.breakpoints(BF, BL, BU, BV), *em.breakpoints(BF, BL, BU, BV, probs=(0.5,)))
p, lpe = em.breakpoint_profile(int(BF[3]), int(BL[3]), int(BU[3]), int(BV[3]))
put("breakpoint_profile", p, [lpe])
em.set_alpha_stats(True)
put("alpha pass", full_pass(em), em.alpha_stats())
em.set_alpha_stats(False)
em.set_stats_mode(N.HF_STATS_CHUNKS)
put("chunk statistics mode", [em.stats_mode], full_pass(em))
em.set_stats_mode(N.HF_STATS_ROWS)
em.set_profiling(True)
em.set_profiling_stride(1)
put("profiled pass", full_pass(em))
note("kernel_ms", type(em.kernel_ms()).__name__)
note("kernel_times", sorted(em.kernel_times()))
note("kernel_time_sums", sorted(em.kernel_time_sums()))
em.set_profiling(False)

# ---- EMBatch (on the list's context) ----
m1, m2 = fresh(), fresh()
m2.set_alpha(np.zeros((4, 4)))
batch = hmm.EMBatch(em, [m1, m2])
note("batch capacity", type(batch.capacity()).__name__)
put("batch estep", *batch.estep())
put("batch size shared", [batch.size, batch.shared_models])
epoch, flags = batch.handoff(1)
put("batch handoff", [epoch], flags)
act = batch.launch(active=[1])
put("batch launch finish", act, *batch.finish(len(act)))
put("batch results", batch.labels(0), batch.labels(1), batch.posterior(0), batch.posterior(1, 40, 9))
put("EM_runBatchForList", hmm.EM_runBatchForList(batch), m1.estimators, m2.estimators)
batch.close()

# ---- MultiEMList, two ranks on one device ----
multi = hmm.MultiEMList(store, model0, 2, transport=N.HF_TRANSPORT_LOOPBACK)
put("multi run_sharded", multi.run_sharded(model0, N.HF_MODE_FULL), multi.rank_stats(0), multi.rank_stats(1), np.array(multi.shard_sizes()))
put("multi labels posterior", multi.labels(), multi.posterior(), multi.posterior(2000, 100))
put("multi viterbi", *multi.viterbi(model0))
m = fresh()
put("multi em_iterate", [multi.em_iterate(m, True, 1e-3)], m.estimators, m.param_vector())
multi.close()

# ---- runHMMFlagger ----
runs = (("plain", {}), ("minlen", {"constrainedMinLen": MIN_LEN, "constrainedJoined": JOINED}), ("alpha", {"fitAlpha": True}))
for name, kw in runs:
    d = os.path.join(DIR, name)
    os.makedirs(d)
    m = fresh()
    put("runHMMFlagger " + name, hmm.runHMMFlagger(em, m, 4, 1e-9, d, True, **kw), m.param_vector(), em.labels())
em.close()

with open(OUT, "wb") as f:
    for a in out:
        f.write(a.tobytes())
    for name, _ in runs:
        for fn in sorted(os.listdir(os.path.join(DIR, name))):
            data = open(os.path.join(DIR, name, fn), "rb").read()
            names.append("file %s/%s %d bytes" % (name, fn, len(data)))
            f.write(fn.encode() + b"\0" + data)
print("\n".join(names))
print("arrays %d, bytes %d, NaN %d" % (len(out), sum(a.nbytes for a in out), sum(int(np.isnan(a).sum()) for a in out if a.dtype == np.float64)))
