"""Many models on one track, measured: (1) one batched pass of B models (hmm.EMBatch) against B passes of the single context, for
B in {1, 2, 4, 8, 16}; (2) the wall time of `hmm_flagger --sweepAlpha` over 8 alpha candidates against 8 separate `hmm_flagger`
processes on the same input.  Usage: python profiles/tools/batch_sweep.py [--scale S] [--reps R] [--cli] > profiles/batch_<name>.txt"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flagger_amd import _native as N, hmm, synth  # noqa: E402

CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")


def alphas(n):
    rng = np.random.default_rng(99)
    out = [synth.HIFI_ALPHA, np.zeros((4, 4))]
    while len(out) < n:
        out.append(rng.uniform(0.0, 0.5, (4, 4)))
    return out[:n]


def passes(store, reps):
    K = min(hmm.getBestNumberOfCollapsedComps(store), 6)
    models = [hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, a) for a in alphas(16)]
    em = hmm.EMList(store, models[0])
    print("windows %d, chunks %d, K %d, statistics mode %d, launches %d, capacity %d" %
          (store.n_windows, store.n_chunks, K, em.stats_mode, em.seg_launches, em._L.hf_batch_capacity(em._h)))
    for m in models:                                          # warm every path once
        hmm.EM_runOneIterationForList(em, m)
    print("%3s %14s %14s %8s" % ("B", "batched ms", "B x single ms", "ratio"))
    for B in (1, 2, 4, 8, 16):
        batch = hmm.EMBatch(em, models[:B])
        batch.estep()
        t0 = time.perf_counter()
        for _ in range(reps):
            batch.estep()
        tb = (time.perf_counter() - t0) / reps * 1e3
        t0 = time.perf_counter()
        for _ in range(reps):
            for m in models[:B]:
                em.launch(m)
                em.finish()
        ts = (time.perf_counter() - t0) / reps * 1e3
        print("%3d %14.3f %14.3f %8.3f" % (B, tb, ts, tb / ts))
        batch.close()
    em.close()


def sweep(store):
    with tempfile.TemporaryDirectory() as d:
        binp = os.path.join(d, "in.bin")
        store.write_bin(binp)
        tsvs = []
        for i, a in enumerate(alphas(8)):
            p = os.path.join(d, "a%d.tsv" % i)
            np.savetxt(p, a, fmt="%.3f", delimiter="\t")
            tsvs.append(p)
        lst = os.path.join(d, "list.txt")
        open(lst, "w").write("\n".join(tsvs) + "\n")
        os.mkdir(os.path.join(d, "sweep"))
        t0 = time.perf_counter()
        r = subprocess.run([CLI, "-i", binp, "-o", os.path.join(d, "sweep"), "--sweepAlpha", lst], capture_output=True, text=True)
        tsw = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-1000:]
        t0 = time.perf_counter()
        for i, p in enumerate(tsvs):
            o = os.path.join(d, "sep%d" % i)
            os.mkdir(o)
            r = subprocess.run([CLI, "-i", binp, "-o", o, "--alphaTsv", p], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-1000:]
        tsep = time.perf_counter() - t0
        print("8-candidate sweep: --sweepAlpha %.3f s, 8 separate processes %.3f s, ratio %.3f" % (tsw, tsep, tsw / tsep))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cli", action="store_true")
    a = ap.parse_args()
    store = synth.config(a.config, a.scale)
    print("configs[%d] scale %g" % (a.config, a.scale))
    passes(store, a.reps)
    if a.cli:
        sweep(store)


if __name__ == "__main__":
    main()
