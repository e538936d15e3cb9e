"""Child process of tests/test_streams_gpu.py::test_torch_stream (no test in it): imports torch BEFORE the project's library, as a caller
of flagger_amd/dist.py does, runs one pass and two getters on a torch.cuda.Stream's handle — the current stream inside
`with torch.cuda.stream(s):`, fetched the way dist.py fetches it — with filler in front of every call, and the same on stream 0; compares
bitwise and prints one line "RESULT <json>"."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    if not torch.cuda.is_available():
        return {"status": "no gpu"}
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.zeros(1, device=dev)                                  # torch's runtime is up before the library loads
    import numpy as np
    from flagger_amd import _native as N
    from flagger_amd import hmm, synth
    import hip_streams as HS

    store = synth.config(2, 0.03)
    model = hmm.createModel(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 4, store, synth.HIFI_ALPHA)
    n = store.n_windows
    F, L = np.array([0, n // 3]), np.array([n - 1, n // 3 + 700])
    h = HS.hip()
    with open("/proc/self/maps") as f:
        runtimes = sorted({line.split()[-1] for line in f if "libamdhip64.so" in line})
    ts = torch.cuda.Stream(device=dev)
    out = {"status": "ok", "runtimes": runtimes, "busy_after_estep": False, "current_stream_is_the_handle": False}
    recs = []
    for use_torch in (True, False):
        with torch.cuda.stream(ts):
            s = int(torch.cuda.current_stream(dev).cuda_stream) if use_torch else 0      # dist.py: torch.cuda.current_stream(dev).cuda_stream
            if use_torch:
                out["current_stream_is_the_handle"] = s == int(ts.cuda_stream) and s != 0
            em = hmm.EMList(store, model, stream=s)
            try:
                h.delay(s)
                em.launch(model)
                if s:
                    out["busy_after_estep"] = h.stream_query(s) == HS.hipErrorNotReady
                h.delay(s)
                rec = [em.finish()]
                h.delay(s)
                rec += [em.posterior(), em.posterior(n // 2 - 300, 900)]
                h.delay(s)
                rec += [em.path_entropy(F, L)]
                h.delay(s)
                rec += [em.labels()]
                recs.append(rec)
            finally:
                em.close()
    ts.synchronize()
    out["codes_ok"] = True                                       # (the wrappers raise on any other code)
    out["compared_arrays"] = len(recs[0])
    out["equal"] = all(a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(*recs))
    return out


if __name__ == "__main__":
    print("RESULT " + json.dumps(main()), flush=True)
