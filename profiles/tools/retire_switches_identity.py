#!/usr/bin/env python
"""sha1 digests of what a pass computes, over the settings that take different paths through hf_estep / hf_finish: run once per
library (HF_LIBRARY_VARIANT=<name> loads csrc/variants/libhmmflagger_hip.<name>.so) and diff the two outputs — a change that
touches no arithmetic and no summation order leaves every line equal.  profiles/retire_switches_identity.txt is such a pair."""
import hashlib
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from flagger_amd import hmm, synth, _native as N  # noqa: E402

SWITCHES = ("HF_STATS", "HF_SUBPASSES", "HF_TOTAL")     # read by hf_create: set per context


def sha(a) -> str:
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def single(tag, store, K, model_type, env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    alpha = np.zeros((4, 4)) if model_type == hmm.MODEL_NEGATIVE_BINOMIAL else synth.HIFI_ALPHA
    model = hmm.createModel(model_type, K, store, alpha)
    em = hmm.EMList(store, model, True, 0.95)
    try:
        em.launch(model); st = em.finish().copy()
        out = [("stats", sha(st)), ("loglik", sha(st[:1])), ("labels", sha(em.labels()))]
        f, b, sc = em.forward_backward(100, 3000)
        out.append(("fwd_bwd", sha(np.concatenate([f.ravel(), b.ravel(), sc.ravel()]))))
        for _ in range(3):
            em.em_iterate(model, True, 1e-3)
        em.launch(model, N.HF_MODE_FORWARD_ONLY)
        out.append(("forward_only_after_3_steps", sha(em.finish()[:1])))
        mode = "rows" if em.stats_mode == N.HF_STATS_ROWS else "chunks"
        for what, h in out:
            print(f"{tag} [{mode}, {em.sub_passes} sub-pass(es)] {what} {h}", flush=True)
    except N.HFError as e:                       # (a setting the library refuses: the same refusal from both libraries)
        print(f"{tag} refused: {e}", flush=True)
    finally:
        em.close()
        for k in env:
            os.environ.pop(k, None)


def multi(tag, store, K):
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, synth.HIFI_ALPHA)
    m = hmm.MultiEMList(store, model, 1, True, 0.95, exchange=N.HF_EXCHANGE_RANKS, transport=N.HF_TRANSPORT_LOOPBACK)
    try:
        st = m.run_sharded(model, N.HF_MODE_FULL)
        print(f"{tag} stats {sha(st)}", flush=True)
        print(f"{tag} labels {sha(m.labels())}", flush=True)
        for _ in range(3):
            m.em_iterate(model, True, 1e-3)
        print(f"{tag} forward_only_after_3_steps {sha(m.run_sharded(model, N.HF_MODE_FORWARD_ONLY)[:1])}", flush=True)
    finally:
        m.close()


def batch(tag, store, K):
    models = []
    for k in range(3):
        alpha = np.array(synth.HIFI_ALPHA, dtype=np.float64) * (1.0 - 0.25 * k)
        models.append(hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, store, alpha))
    b = hmm.EMBatch(store, models, True, 0.95)
    try:
        st, status = b.estep()
        print(f"{tag} status {status.tolist()} shared models {b.shared_models}", flush=True)
        for k in range(3):
            print(f"{tag} model {k} stats {sha(st[k])} labels {sha(b.labels(k))}", flush=True)
    finally:
        b.close()
        b.em.close()


def main():
    print("library", N.LIB_PATH, file=sys.stderr, flush=True)
    for cfg, scale in ((2, 0.05), (2, 1.0), (4, 1.0)):
        store = synth.config(cfg, scale=scale)
        K = hmm.getBestNumberOfCollapsedComps(store)
        name = f"configs[{cfg}] x {scale} ({store.n_windows} windows, K {K})"
        types = [("trunc_exp_gaussian", hmm.MODEL_TRUNC_EXP_GAUSSIAN), ("gaussian", hmm.MODEL_GAUSSIAN)]
        if scale < 1.0:
            types.append(("negative_binomial", hmm.MODEL_NEGATIVE_BINOMIAL))
        for tname, mt in types:
            for stats in ("rows", "chunks"):
                single(f"{name} {tname} HF_STATS={stats}", store, K, mt, {"HF_STATS": stats})
        single(f"{name} trunc_exp_gaussian HF_SUBPASSES=3", store, K, hmm.MODEL_TRUNC_EXP_GAUSSIAN, {"HF_SUBPASSES": "3"})
        single(f"{name} trunc_exp_gaussian HF_TOTAL=device", store, K, hmm.MODEL_TRUNC_EXP_GAUSSIAN, {"HF_TOTAL": "device"})
        multi(f"{name} one-rank MultiEMList, ranks exchange", store, K)
        batch(f"{name} EMBatch of three", store, K)


if __name__ == "__main__":
    main()
