"""The E-step under minimum run lengths (hf_estep_minlen) and the EM over it on BASELINE configs[2], trunc_exp_gaussian, HiFi alpha,
lengths (3, 5, 1, 7) windows.  Writes what it measures to stdout (kept as profiles/minlen_em_cfg2.txt).
  python profiles/tools/minlen_em_cfg2.py step     after two plain EM iterations: host wall (call .. statistics on the host, median of 11)
                                                   of hf_estep + hf_finish, of hf_minlen_posterior + finish and of hf_estep_minlen +
                                                   finish in one process; under rocprofv3 --kernel-trace --stats this gives the kernel
                                                   times of k_tables, k_dec_rows_win, k_mlp_fwd, k_mlp_bwd, k_mle_bwd, k_mle_tile,
                                                   k_chunk_stats and k_reduce side by side
  python profiles/tools/minlen_em_cfg2.py effect   the plain fit and the constrained fit from the same initial model (at most ITER
                                                   iterations, tol 1e-3): log_mass by hf_minlen_posterior, the cost of the constrained
                                                   Viterbi path (hf_viterbi's score minus hf_viterbi_minlen's) and the expected-accuracy
                                                   totals (hf_get_mea_labels) under both fits
  python profiles/tools/minlen_em_cfg2.py cli      wall time of `hmm_flagger` and of `hmm_flagger --lengthConstrainedEM` on the same .bin"""
import os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C
import numpy as np
from flagger_amd import hmm, synth, _native as N
ML = (3, 5, 1, 7)
REPS, ITER = 11, 30
MODES = [a for a in sys.argv[1:] if a in ("step", "effect", "cli")] or ["step", "effect", "cli"]
store = synth.config(2)
K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
T = np.diff(store.chunk_off)
print("windows", store.n_windows, "chunks", store.n_chunks, "longest chunk", int(T.max()), "K", K, "lengths", ML, flush=True)


def wall(call):
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter(); call(); ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), min(ms)


def fresh():
    return hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)


if "step" in MODES:
    model = fresh()
    em = hmm.EMList(store, model)
    for _ in range(2):
        hmm.EM_runOneIterationForList(em, model); hmm.HMM_estimateParameters(model, 1e-3); hmm.HMM_resetEstimators(model)
    L = N.lib()
    p = model.params()
    a = (C.c_int32 * 4)(*ML)
    lp = C.c_double(0.0)
    st = np.empty(em.stats_len)
    sp = st.ctypes.data_as(C.POINTER(C.c_double))

    def plain():
        N.check(L.hf_estep(em._h, p, N.HF_MODE_FULL, None), "e"); N.check(L.hf_finish(em._h, sp, None), "f")

    def post():
        N.check(L.hf_minlen_posterior(em._h, p, a, None), "p"); N.check(L.hf_minlen_posterior_finish(em._h, C.byref(lp), None), "f")

    def con():
        N.check(L.hf_estep_minlen(em._h, p, a, None), "c"); N.check(L.hf_estep_minlen_finish(em._h, sp, C.byref(lp), None), "f")

    plain(); post(); con()
    for name, f in (("hf_estep + hf_finish", plain), ("hf_minlen_posterior + finish", post), ("hf_estep_minlen + finish", con)):
        print("step: %-30s median %.3f ms, min %.3f ms" % ((name,) + wall(f)), flush=True)
    print("step: forward lanes %.1f MB, xi_adm %.1f MB; sum log Z_adm %.4f, sum log Z %.4f" %
          (store.n_windows * sum(ML) * 8 / 1e6, store.n_windows * 128 / 1e6, st[0], lp.value), flush=True)
    em.close()

if "effect" in MODES:
    fits = {}
    for kind in ("plain", "constrained"):
        model = fresh()
        em = hmm.EMList(store, model)
        t0 = time.perf_counter()
        it, cv, obj = 0, False, []
        while it < ITER and not cv:
            cv = em.em_iterate_minlen(model, ML, True, 1e-3) if kind == "constrained" else em.em_iterate(model, True, 1e-3)
            obj.append(model.loglikelihood)
            hmm.HMM_resetEstimators(model)
            it += 1
        dt = time.perf_counter() - t0
        hmm.EM_runOneIterationForList(em, model); hmm.HMM_resetEstimators(model)          # the final pass
        ll = model.loglikelihood
        r = em.minlen_posterior(model, ML)
        m = r.chunk_log_mass
        v = em.viterbi(model)[2]
        vm = em.viterbi_minlen(model, ML)[2]
        _, _, gain = em.mea_labels(ML)
        _, _, gain1 = em.mea_labels((1, 1, 1, 1))
        print("effect: %-11s fit: %d iterations in %.1f ms (%.2f ms each), converged %s; objective first %.4f last %.4f; final log-likelihood %.4f" %
              (kind, it, dt * 1e3, dt * 1e3 / it, cv, obj[0], obj[-1], ll), flush=True)
        print("effect: %-11s fit: log_mass %.4f over %d of %d chunks below -1e-6 (smallest %.4f); sum log Z_adm %.4f" %
              (kind, r.log_mass, int(np.sum(m < -1e-6)), m.size, float(m.min()), float(r.chunk_log_z_adm.sum())), flush=True)
        print("effect: %-11s fit: Viterbi %.4f, constrained Viterbi %.4f, cost %.4f; expected correct windows %.4f under the rule, %.4f without" %
              (kind, v, vm, v - vm, gain, gain1), flush=True)
        fits[kind] = model.param_vector()
        em.close()
    d = np.abs(fits["plain"] - fits["constrained"])
    R_ = d.size // (27 + 12 * 16)
    tp, tc = fits["plain"].reshape(R_, -1)[0, :25].reshape(5, 5), fits["constrained"].reshape(R_, -1)[0, :25].reshape(5, 5)
    print("effect: stay probabilities (Err, Dup, Hap, Col): plain %s, constrained %s" %
          (" ".join("%.6f" % tp[s, s] for s in range(4)), " ".join("%.6f" % tc[s, s] for s in range(4))), flush=True)

if "cli" in MODES:
    cli = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
    with tempfile.TemporaryDirectory() as tmp:
        binp = os.path.join(tmp, "in.bin")
        store.write_bin(binp)
        W = int(store.window_len)
        base = [cli, "-i", binp, "-W", str(W), "-p", str(K), "-n", str(ITER), "--minimumLengths", "%d,%d,%d" % (ML[0] * W, ML[1] * W, ML[3] * W)]
        for name, extra in (("hmm_flagger", []), ("hmm_flagger --lengthConstrainedEM", ["--lengthConstrainedEM"])):
            ws = []
            for rep in range(3):
                out = os.path.join(tmp, "out_%d_%d" % (len(extra), rep))
                os.makedirs(out)
                t0 = time.perf_counter()
                r = subprocess.run(base + extra + ["-o", out], capture_output=True, text=True)
                ws.append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr[-2000:]
            rows = [l for l in open(os.path.join(out, "loglikelihood.tsv")).read().splitlines() if not l.startswith("#")]
            em_line = [l for l in r.stderr.splitlines() if "EM+decode" in l]
            print("cli: %-34s wall median %.3f s, min %.3f s; %d rows of loglikelihood.tsv; %s" %
                  (name, float(np.median(ws)), min(ws), len(rows), em_line[-1].split("] ", 1)[-1] if em_line else ""), flush=True)
            if extra:
                print("cli: length_constrained_em.tsv, first and last rows: %s | %s" %
                      tuple(l.replace("\t", " ") for l in (lambda x: (x[1], x[-1]))(open(os.path.join(out, "length_constrained_em.tsv")).read().splitlines())), flush=True)
