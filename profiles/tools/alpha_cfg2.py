"""The alpha statistics (hf_get_alpha_stats) and the alpha fit on BASELINE configs[2].
  python profiles/tools/alpha_cfg2.py stats   two EM iterations, then 6 x (full pass with the switch on, alpha statistics, alpha-step): the
                                              host wall of the pass and of the getter (the kernel times come from rocprofv3
                                              --kernel-trace --stats in a run of its own)
  python profiles/tools/alpha_cfg2.py cli     wall time and number of passes of `hmm_flagger`, of `hmm_flagger --fitAlpha` and of the
                                              8-candidate `--sweepAlpha` of batch_sweep.py on the same input"""
import os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from flagger_amd import hmm, synth

CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
leg = sys.argv[1] if len(sys.argv) > 1 else "stats"
store = synth.config(2)


def rows(path):
    return [l for l in open(path).read().splitlines() if l and not l.startswith("#")]


if leg == "stats":
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
    em = hmm.EMList(store, model)
    for _ in range(2):
        hmm.EM_runOneIterationForList(em, model); hmm.HMM_estimateParameters(model, 1e-3); hmm.HMM_resetEstimators(model)
    print("windows", store.n_windows, "chunks", store.n_chunks, "K", K, "statistics mode", em.stats_mode, flush=True)
    em.set_alpha_stats(True)
    for rep in range(6):
        t0 = time.perf_counter()
        hmm.EM_runOneIterationForList(em, model)
        t1 = time.perf_counter()
        st = em.alpha_stats()
        t2 = time.perf_counter()
        conv = hmm.HMM_estimateAlpha(model, st, 1e-3)
        print("rep %d: pass %.3f ms, alpha statistics %.3f ms, LL %.4f, max |G| %.4g, max move of alpha %s" %
              (rep, (t1 - t0) * 1e3, (t2 - t1) * 1e3, model.loglikelihood, float(np.abs(st[:, 0]).max()), "< 1e-3" if conv else ">= 1e-3"), flush=True)
    em.close()
else:
    from batch_sweep import alphas
    with tempfile.TemporaryDirectory() as d:
        binp = os.path.join(d, "in.bin")
        store.write_bin(binp)

        def run(name, extra):
            o = os.path.join(d, name)
            os.mkdir(o)
            t0 = time.perf_counter()
            r = subprocess.run([CLI, "-i", binp, "-o", o] + extra, capture_output=True, text=True)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-1000:]
            return o, dt

        o, dt = run("plain", [])
        ll = rows(os.path.join(o, "loglikelihood.tsv"))
        print("hmm_flagger:            %.3f s, %d passes, final log-likelihood %s" % (dt, len(ll), ll[-1].split("\t")[2]), flush=True)
        o, dt = run("fit", ["--fitAlpha"])
        ll = rows(os.path.join(o, "loglikelihood.tsv"))
        print("hmm_flagger --fitAlpha: %.3f s, %d passes (%d alpha-iterations), final log-likelihood %s" %
              (dt, len(ll), len(rows(os.path.join(o, "alpha_trace.tsv"))), ll[-1].split("\t")[2]), flush=True)
        print("alpha_fitted.tsv:\n" + open(os.path.join(o, "alpha_fitted.tsv")).read(), flush=True)
        tsvs = []
        for i, a in enumerate(alphas(8)):
            p = os.path.join(d, "a%d.tsv" % i)
            np.savetxt(p, a, fmt="%.3f", delimiter="\t")
            tsvs.append(p)
        lst = os.path.join(d, "list.txt")
        open(lst, "w").write("\n".join(tsvs) + "\n")
        o, dt = run("sweep", ["--sweepAlpha", lst])
        n = [len(rows(os.path.join(o, "alpha_%d" % (i + 1), "loglikelihood.tsv"))) for i in range(8)]
        best = max(float(rows(os.path.join(o, "alpha_%d" % (i + 1), "loglikelihood.tsv"))[-1].split("\t")[2]) for i in range(8))
        print("hmm_flagger --sweepAlpha (8 candidates): %.3f s, %d passes, best final log-likelihood %.4f" % (dt, sum(n), best), flush=True)
