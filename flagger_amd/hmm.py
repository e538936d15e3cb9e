"""Host-side mirror of the reference's HMM/EM interface for the hot path, on top of the C ABI.

Names and call order follow mobinasri/flagger (programs/submodules/hmm/hmm.h:79-113 and
programs/src/hmm_flagger.c:285-488):

    model = createModel(...)                      # hmm_flagger.c:164-237
    emList = EMList(store, model, ...)            # the list of per-chunk EM objects, hmm_flagger.c:320-330
    EM_runOneIterationForList(emList, model)      # hmm.c:739   (HIP kernels)
    converged = HMM_estimateParameters(model, tol)  # hmm.c:120
    HMM_resetEstimators(model)                    # hmm.c:129

One `EMList` is one GPU context holding every chunk of this process; with a process group the
per-chunk statistics of all ranks are all-gathered and summed in global chunk order, so the
result does not depend on the number of GPUs.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N
from .synth import WindowStore

MODEL_TRUNC_EXP_GAUSSIAN = N.HF_MODEL_TRUNC_EXP_GAUSSIAN
MODEL_GAUSSIAN = N.HF_MODEL_GAUSSIAN
MODEL_NEGATIVE_BINOMIAL = N.HF_MODEL_NEGATIVE_BINOMIAL
STATE_NAMES = ("Err", "Dup", "Hap", "Col")


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(N.p_double)


def _ptr(a: Optional[np.ndarray]):
    """The pointer the C ABI takes for the array `a`, by its dtype; None (an argument left out) stays None."""
    return None if a is None else a.ctypes.data_as(N.pointer_of[a.dtype.name])


def _unwritten(shape, dtype, fill=None) -> np.ndarray:
    """An output array for the library to write into: uninitialised, or holding `fill` where the library may leave entries alone."""
    return np.empty(shape, dtype=dtype) if fill is None else np.full(shape, fill, dtype=dtype)


# a column of state sets (bit s = state s) for _jobs: Python refuses what no uint8 holds, the library the empty set and 16..255
_MASK = (np.uint8, 0, 255, "a state mask must be 1..15")
_INT32 = (np.int32, -2 ** 31, 2 ** 31 - 1)


def _jobs(who: str, first, last, *columns) -> List[np.ndarray]:
    """The job front of the range getters: first, last (int64) and every further column (values, dtype) or (values, dtype, lo, hi,
    what) broadcast against each other, then each ravelled into a contiguous array of its dtype, in the order given.  A column with
    a range raises ValueError("<who>: <what>") where a value lies outside lo..hi; whatever passes is the library's to judge."""
    columns = ((first, np.int64), (last, np.int64)) + columns
    out = []
    for a, (_, dtype, *bounds) in zip(np.broadcast_arrays(*[np.asarray(c[0], np.int64) for c in columns]), columns):
        if bounds and a.size and (a.min() < bounds[0] or a.max() > bounds[1]):
            raise ValueError("%s: %s" % (who, bounds[2]))
        out.append(np.ascontiguousarray(a.ravel(), dtype))
    return out


def _outputs(n: int, *specs) -> List[np.ndarray]:
    """One uninitialised output array per spec for n jobs: a dtype gives shape (n,), (dtype, k) gives (n, k)."""
    return [np.empty((n,) + spec[1:], dtype=spec[0]) if isinstance(spec, tuple) else np.empty(n, dtype=spec) for spec in specs]


class HMM:
    """The model (HMM struct, hmm.h:14-25) + the pending sufficient statistics of the last E-step
    (the reference keeps them inside the model's estimator objects)."""

    def __init__(self, handle):
        self._h = handle
        self._L = N.lib()
        self.estimators: Optional[np.ndarray] = None   # reduced statistics vector of the last pass
        self.loglikelihood = 0.0

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.hfm_destroy(self._h)
            self._h = None

    @property
    def numberOfRegions(self) -> int:
        return self._L.hfm_n_regions(self._h)

    @property
    def maxNumberOfComps(self) -> int:
        return self._L.hfm_max_comps(self._h)

    @property
    def modelType(self) -> int:
        return self._L.hfm_model_type(self._h)

    def params(self) -> N.hf_params:
        p = N.hf_params()
        self._L.hfm_params(self._h, C.byref(p))
        return p

    def param_vector(self) -> np.ndarray:
        v = np.empty(self._L.hfm_param_len(self._h), dtype=np.float64)
        self._L.hfm_get_param_vector(self._h, _dptr(v))
        return v

    def set_param_vector(self, v: np.ndarray) -> None:
        v = np.ascontiguousarray(v, dtype=np.float64)
        assert v.size == self._L.hfm_param_len(self._h)
        self._L.hfm_set_param_vector(self._h, _dptr(v))

    @property
    def alpha(self) -> np.ndarray:
        """The alpha matrix alpha[preState][state] (hfm_get_alpha): float64[4][4], a copy."""
        a = np.empty((4, 4), dtype=np.float64)
        self._L.hfm_get_alpha(self._h, _dptr(a))
        return a

    def set_alpha(self, alpha) -> None:
        """hfm_set_alpha: every entry in [0, 1)."""
        a = np.ascontiguousarray(alpha, dtype=np.float64)
        if a.shape != (4, 4):
            raise ValueError("set_alpha: a 4x4 matrix")
        if self._L.hfm_set_alpha(self._h, _dptr(a)) != 0:
            raise ValueError("set_alpha: every alpha value must be in [0, 1)")

    def copy(self) -> "HMM":
        m = HMM(self._L.hfm_copy(self._h))
        m.loglikelihood = self.loglikelihood
        return m

    def unpack(self) -> dict:
        """Parameter arrays by name (tests / reporting)."""
        R, K = self.numberOfRegions, N.HF_MAXCOMP
        v = self.param_vector().reshape(R, -1)
        out = {"trans": v[:, :25].reshape(R, 5, 5).copy(), "lambda": v[:, 25].copy(), "trunc_point": v[:, 26].copy()}
        o = 27
        for name in ("mean", "var", "weight"):
            out[name] = v[:, o:o + 4 * K].reshape(R, 4, K).copy()
            o += 4 * K
        return out

    def writeTransitionTsv(self, path: str) -> None:
        if self._L.hfm_write_transition_tsv(self._h, path.encode()) != 0:
            raise OSError(f"cannot write {path}")

    def writeEmissionTsv(self, path: str) -> None:
        if self._L.hfm_write_emission_tsv(self._h, path.encode()) != 0:
            raise OSError(f"cannot write {path}")


def getAlphaMatrix(alphaTsvPath: Optional[str]) -> np.ndarray:
    """hmm_flagger.c:491-515 (None => zeros)."""
    a = np.zeros((4, 4))
    if alphaTsvPath is not None:
        rc = N.lib().hfm_read_alpha_tsv(alphaTsvPath.encode(), _dptr(a))
        if rc == -2:
            raise ValueError(f"There is at least one alpha value in '{alphaTsvPath}' not between 0 and 1.")
        if rc != 0:
            raise OSError(f"cannot read {alphaTsvPath}")
    return a


def getBestNumberOfCollapsedComps(store: WindowStore) -> int:
    """hmm_flagger.c:105-111 with the [2,10] clamp of :1012-1013."""
    cov = np.ascontiguousarray(store.cov, dtype=np.uint16)
    rc = np.asarray(store.region_coverages, dtype=np.int32)
    k = N.lib().hfm_best_collapsed_comps(_ptr(cov), cov.size, _ptr(rc), rc.size)
    if k < 0:
        raise ValueError("a region coverage of 0 in the header")
    return k


def createModel(modelType: int, numberOfCollapsedComps: int, store: WindowStore, alphaMatrix: np.ndarray,
                maxHighMapqRatio: float = 0.25, minHighMapqRatio: float = 0.75) -> HMM:
    """hmm_flagger.c:164-237 (initialRandomDev = 0)."""
    rc = np.asarray(store.region_coverages, dtype=np.int32)
    a = np.ascontiguousarray(alphaMatrix, dtype=np.float64)
    h = N.lib().hfm_create(modelType, numberOfCollapsedComps, _ptr(rc), rc.size,
                           int(store.start_only), store.avg_alignment_len, store.window_len, _dptr(a),
                           maxHighMapqRatio, minHighMapqRatio)
    if not h:
        raise ValueError("createModel: bad arguments")
    if modelType == MODEL_NEGATIVE_BINOMIAL and store.n_windows:
        # the per-x tables of the model are rebuilt on the host every iteration: only up to the largest coverage present
        N.lib().hfm_set_max_coverage(h, int(min(int((np.asarray(store.cov) & 0xff).max()), 250)))
    return HMM(h)


def _windows_struct(store: WindowStore, model: "HMM", adjustContigEnds: bool, minReadFractionAtEnds: float):
    """hf_windows over the store's arrays (+ the dict that keeps the contiguous copies alive)."""
    L = N.lib()
    k = dict(
        off=np.ascontiguousarray(store.chunk_off, np.int64), cov=np.ascontiguousarray(store.cov, np.uint16),
        mapq=np.ascontiguousarray(store.mapq, np.uint16), clip=np.ascontiguousarray(store.clip, np.uint16),
        annot=np.ascontiguousarray(store.annot, np.uint64), s=np.ascontiguousarray(store.chunk_s, np.int32),
        e=np.ascontiguousarray(store.chunk_e, np.int32), cl=np.ascontiguousarray(store.chunk_ctg_len, np.int32))
    w = N.hf_windows()
    w.n_windows, w.n_chunks = store.n_windows, store.n_chunks
    w.chunk_off, w.cov, w.mapq, w.clip, w.annot = _ptr(k["off"]), _ptr(k["cov"]), _ptr(k["mapq"]), _ptr(k["clip"]), _ptr(k["annot"])
    w.chunk_s, w.chunk_e, w.chunk_ctg_len = _ptr(k["s"]), _ptr(k["e"]), _ptr(k["cl"])
    w.window_len, w.mean_read_len = store.window_len, store.avg_alignment_len
    w.adjust_contig_ends, w.min_read_frac = int(adjustContigEnds), float(minReadFractionAtEnds)
    w.max_high_mapq_ratio = L.hfm_max_high_mapq_ratio(model._h)
    w.min_high_mapq_ratio = L.hfm_min_high_mapq_ratio(model._h)
    w.min_highly_clipped_ratio = L.hfm_min_highly_clipped_ratio(model._h)
    return w, k


class RetryPass(N.HFError):
    """HF_E_RETRY out of EMList.check(): repeat the pass and everything that consumed its statistics."""


class MultiHFError(RuntimeError):
    def __init__(self, code: int, where: str):
        self.code = code
        super().__init__(f"{where} failed with code {code}: {N.lib().hf_multi_last_error().decode(errors='replace')}")


class MultiEMList:
    """The chunk list sharded over the GPUs of this node inside ONE process (include/hmm_flagger_multi.h hf_multi: one
    host thread, stream and RCCL rank per device; one all-gather of statistics per pass).  What `hmm_flagger --gpus N`
    drives; `transport=N.HF_TRANSPORT_LOOPBACK` puts all ranks on one device (tests on a 1-GPU box)."""

    def __init__(self, store: WindowStore, model: "HMM", n_devices: int, adjustContigEnds: bool = True,
                 minReadFractionAtEnds: float = 0.95, devices: Optional[Sequence[int]] = None, algo: int = N.HF_ALGO_SCAN,
                 exchange: int = N.HF_EXCHANGE_CHUNKS, transport: int = N.HF_TRANSPORT_RCCL):
        w = self._set_up(store, model, adjustContigEnds, minReadFractionAtEnds)
        dev = (C.c_int * n_devices)(*devices) if devices is not None else None
        h = C.c_void_p()
        self._check(self._L.hf_multi_create(C.byref(w), self.n_regions, self.max_comps, n_devices, dev, algo, exchange, transport, C.byref(h)),
                    "hf_multi_create")
        self._h, self.world = h, n_devices

    # what labels() and posterior() hold where the library writes nothing: None leaves the array uninitialised (this class: every
    # window is some shard's)
    _labels_fill = _posterior_fill = None

    def _set_up(self, store: WindowStore, model: "HMM", adjustContigEnds: bool, minReadFractionAtEnds: float):
        """What either constructor needs before its hf_multi_create*: the hf_windows of the store (returned; self._keep holds its
        arrays), the layout of the statistics vector and the vector itself."""
        self._L, self.store = N.lib(), store
        w, self._keep = _windows_struct(store, model, adjustContigEnds, minReadFractionAtEnds)
        self.n_regions, self.max_comps = model.numberOfRegions, model.maxNumberOfComps
        self.stats_len = N.stats_len(self.n_regions, self.max_comps)
        self._stats = np.empty(self.stats_len, dtype=np.float64)
        return w

    @staticmethod
    def _check(rc: int, where: str) -> None:
        if rc != N.HF_OK:
            raise MultiHFError(rc, where)

    def close(self):
        if getattr(self, "_h", None):
            self._L.hf_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def run_sharded(self, model: "HMM", mode: int) -> np.ndarray:
        p = model.params()
        self._check(self._L.hf_multi_estep(self._h, C.byref(p), mode, _dptr(self._stats)), "hf_multi_estep")
        return self._stats.copy()

    def em_iterate(self, model: "HMM", do_mstep: bool = True, tol: float = 1e-3, mode: int = N.HF_MODE_FULL) -> bool:
        """Sharded EM_runOneIterationForList + exchange + HMM_estimateParameters in one native call (hf_multi_em_iterate)."""
        if getattr(self, "_stats_ptr_of", None) is not self._stats:
            self._stats_ptr, self._stats_ptr_of = _dptr(self._stats), self._stats   # (a new ctypes object per .ctypes access: 2 us of host time per call)
            self._cv = C.c_int(0)
            self._cv_ref = C.byref(self._cv)
        rc = self._L.hf_multi_em_iterate(self._h, model._h, mode, int(do_mstep), tol, self._stats_ptr, self._cv_ref)
        if rc != N.HF_OK:
            self._check(rc, "hf_multi_em_iterate")
        model.estimators = self._stats
        model.loglikelihood = float(self._stats[0])
        return bool(self._cv.value)

    def rank_stats(self, r: int) -> np.ndarray:
        out = np.empty(self.stats_len, dtype=np.float64)
        N.check(self._L.hf_multi_rank_stats(self._h, r, _dptr(out)), "hf_multi_rank_stats")
        return out

    def shard_sizes(self):
        return [(int(self._L.hf_multi_shard_chunks(self._h, r)), int(self._L.hf_multi_shard_windows(self._h, r))) for r in range(self.world)]

    def labels(self) -> np.ndarray:
        """The labels of the last full pass, int8[n_windows] (hf_multi_get_labels).  RankEMList: labels of ALL windows' positions, but
        only this rank's range is known here: the others are -1 (hf_multi_get_labels fills this rank's windows at their global
        positions).  Use local_labels() for the rank's own slice."""
        out = _unwritten(self.store.n_windows, np.int8, self._labels_fill)
        self._check(self._L.hf_multi_get_labels(self._h, _ptr(out)), "hf_multi_get_labels")
        return out

    def posterior(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Posteriors of windows first .. first + n (hf_multi_get_posterior).  RankEMList: rows of windows that other ranks hold are
        NaN."""
        n = self.store.n_windows - first if n is None else n
        out = _unwritten((n, 4), np.float64, self._posterior_fill)
        self._check(self._L.hf_multi_get_posterior(self._h, first, n, _dptr(out)), "hf_multi_get_posterior")
        return out

    def viterbi(self, model: "HMM"):
        """Most-probable-path decoding of every shard (hf_multi_viterbi): (labels, chunk_log_probs, log_prob).  RankEMList: the
        labels of other ranks' windows are -1, the scores cover every chunk."""
        p = model.params()
        lp = C.c_double(0.0)
        self._check(self._L.hf_multi_viterbi(self._h, C.byref(p), C.byref(lp)), "hf_multi_viterbi")
        labels = np.full(self.store.n_windows, -1, dtype=np.int8)
        self._check(self._L.hf_multi_get_viterbi_labels(self._h, _ptr(labels)), "hf_multi_get_viterbi_labels")
        ll = np.empty(self.store.n_chunks, dtype=np.float64)
        self._check(self._L.hf_multi_get_viterbi_chunk_log_probs(self._h, _dptr(ll)), "hf_multi_get_viterbi_chunk_log_probs")
        return labels, ll, float(lp.value)


HF_COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """Rank 0's RCCL id for `RankEMList` (include/hmm_flagger_multi.h hf_comm_unique_id); the launcher carries it to the others."""
    buf = C.create_string_buffer(HF_COMM_ID_BYTES)
    N.check(N.lib().hf_comm_unique_id(buf), "hf_comm_unique_id")
    return buf.raw


class RankEMList(MultiEMList):
    """One PROCESS per GPU (torch.distributed.run): this process is rank `rank` of `world` on `device` and holds its shard of
    the chunk list; pass + exchange (RCCL all-gather on the pass's own stream) + ordered reduction are ONE native call per
    EM pass (hf_multi_create_rank / hf_multi_estep).  Collective: every rank constructs it with the same store."""

    def __init__(self, store: WindowStore, model: "HMM", world: int, rank: int, device: int, unique_id: bytes,
                 adjustContigEnds: bool = True, minReadFractionAtEnds: float = 0.95, algo: int = N.HF_ALGO_SCAN,
                 exchange: int = N.HF_EXCHANGE_CHUNKS):
        w = self._set_up(store, model, adjustContigEnds, minReadFractionAtEnds)
        L = self._L
        if len(unique_id) != HF_COMM_ID_BYTES:
            raise ValueError("unique_id must be the %d bytes of comm_unique_id()" % HF_COMM_ID_BYTES)
        self._id = C.create_string_buffer(unique_id, HF_COMM_ID_BYTES)
        h = C.c_void_p()
        self._check(L.hf_multi_create_rank(C.byref(w), self.n_regions, self.max_comps, world, rank, device, algo, exchange, self._id, C.byref(h)),
                    "hf_multi_create_rank")
        self._h, self.world, self.rank = h, world, rank
        self.first_window = int(L.hf_multi_local_first_window(h))
        self.n_local_windows = int(L.hf_multi_local_windows(h))
        # borrowed view of the rank's context: profiling switches and kernel times (bench.py)
        self.em = EMList.__new__(EMList)
        self.em._L, self.em.store, self.em._h, self.em._borrowed = L, None, C.c_void_p(L.hf_multi_local_ctx(h)), True
        self.em.n_regions, self.em.max_comps, self.em.stats_len = self.n_regions, self.max_comps, self.stats_len

    def close(self):
        if getattr(self, "em", None) is not None:
            self.em._h = None
        super().close()

    _labels_fill, _posterior_fill = -1, np.nan       # the windows of other ranks, which the library leaves alone

    def local_labels(self) -> np.ndarray:
        """Labels of this rank's windows (global positions first_window .. first_window + n_local_windows)."""
        return self.labels()[self.first_window:self.first_window + self.n_local_windows]


class EMList:
    """All per-chunk EM objects of this process (stList<EM*> in the reference) as ONE device context:
    the windows are uploaded once and stay resident in HBM (hf_create)."""

    def __init__(self, store: WindowStore, model: HMM, adjustContigEnds: bool = True,
                 minReadFractionAtEnds: float = 0.95, device: int = 0, algo: int = N.HF_ALGO_SCAN,
                 stream: int = 0):
        L = N.lib()
        self._L = L
        self.store = store
        self.stream = C.c_void_p(stream)
        w, self._keep = _windows_struct(store, model, adjustContigEnds, minReadFractionAtEnds)
        self.n_regions, self.max_comps = model.numberOfRegions, model.maxNumberOfComps
        self.stats_len = N.stats_len(self.n_regions, self.max_comps)
        h = C.c_void_p()
        N.check(L.hf_create(C.byref(w), self.n_regions, self.max_comps, device, algo, C.byref(h)), "hf_create")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_borrowed", False):      # a view of a context something else owns (RankEMList.em)
            self._h = None
            return
        if getattr(self, "_h", None):
            self._L.hf_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set_stats_mode(self, mode: int) -> None:
        """N.HF_STATS_ROWS (default where it applies) or N.HF_STATS_CHUNKS (per-chunk vectors, needed by the multi-GPU exchange)."""
        N.check(self._L.hf_set_stats_mode(self._h, int(mode)), "hf_set_stats_mode")

    @property
    def stats_mode(self) -> int:
        return int(self._L.hf_get_stats_mode(self._h))

    @property
    def seg_launches(self) -> int:
        """1: one-launch segment kernel, 2: k_seg_prod + k_seg_fb, 0: no segment kernels (hf_seg_launches)."""
        return int(self._L.hf_seg_launches(self._h))

    @property
    def seg_cached_steps(self) -> int:
        """Row blocks a segment workgroup keeps in LDS across its three walks (hf_seg_cached_steps; 0 on a device full of segments)."""
        return int(self._L.hf_seg_cached_steps(self._h))

    @property
    def sub_passes(self) -> int:
        """Sub-passes of a full pass (hf_sub_passes: 1 unless the pair records would not fit the Infinity Cache)."""
        return int(self._L.hf_sub_passes(self._h)) if hasattr(self._L, "hf_sub_passes") else 1

    def sub_pass_windows(self, k: int = 0) -> int:
        return int(self._L.hf_sub_pass_windows(self._h, int(k)))

    def create_phases(self) -> dict:
        """{phase: ms} of this context's hf_create, in call order; the last entry is "total" (hf_create_phases)."""
        if not hasattr(self._L, "hf_create_phases"):
            return {}
        ms, names = (C.c_double * 64)(), (C.c_char_p * 64)()
        n = min(int(self._L.hf_create_phases(self._h, 64, ms, names)), 64)
        out = {}
        for i in range(n):
            k = names[i].decode()
            out[k] = out.get(k, 0.0) + float(ms[i])
        return out

    # --- E-step pieces (used directly by the multi-GPU path in dist.py) ---
    def launch(self, model: HMM, mode: int = N.HF_MODE_FULL) -> None:
        p = model.params()
        N.check(self._L.hf_estep(self._h, C.byref(p), mode, self.stream), "hf_estep")

    def finish(self) -> np.ndarray:
        out = np.empty(self.stats_len, dtype=np.float64)
        N.check(self._L.hf_finish(self._h, _dptr(out), self.stream), "hf_finish")
        return out

    def check(self) -> None:
        """hf_check: the error flags of the last pass.  HF_E_RETRY (a hand-off of the one-launch segment kernel timed out; the context has
        switched to two launches) is not an error of the data, but what the timed-out pass left behind — statistics the caller has already
        copied, reduced or all-gathered — is garbage: it is raised as `RetryPass` so that the caller repeats its WHOLE sequence
        (launch, exchange, reduction, check), as ShardedEMList.run_sharded does for all ranks together; hf_finish repeats the pass inside
        the library, where it reads the result itself.  (round 5 re-launched here and returned success over the stale copy.)"""
        rc = self._L.hf_check(self._h, self.stream)
        if rc == N.HF_E_RETRY:
            raise RetryPass(rc, "hf_check")
        N.check(rc, "hf_check")

    def rank_total(self, dst_dev_ptr: int) -> None:
        """This context's statistics vector (either statistics mode) into device memory."""
        N.check(self._L.hf_rank_total(self._h, C.c_void_p(dst_dev_ptr), self.stream), "hf_rank_total")

    def copy_chunk_stats(self, dst_dev_ptr: int) -> None:
        N.check(self._L.hf_copy_chunk_stats(self._h, C.c_void_p(dst_dev_ptr), self.stream), "hf_copy_chunk_stats")

    def finish_gathered(self, rows_dev_ptr: int, row_index_dev_ptr: int, n_chunks: int) -> np.ndarray:
        """Fixed-order sum of the all-gathered per-chunk vectors into host memory + flag check: one sync (hf_finish_gathered)."""
        if not hasattr(self, "_stats_buf"):
            self._stats_buf = np.empty(self.stats_len, dtype=np.float64)
        N.check(self._L.hf_finish_gathered(self._h, C.c_void_p(rows_dev_ptr), C.c_void_p(row_index_dev_ptr) if row_index_dev_ptr else None, n_chunks,
                                           _dptr(self._stats_buf), self.stream), "hf_finish_gathered")
        return self._stats_buf

    def finish_exchange(self, rows_dev_ptr: int, row_index_dev_ptr: int, n_rows: int, world: int, rows_per_rank: int,
                        flag_row: int) -> np.ndarray:
        """hf_finish_exchange: hf_finish_gathered + the error flags of every rank (row `flag_row` of each rank's rows)."""
        if not hasattr(self, "_stats_buf"):
            self._stats_buf = np.empty(self.stats_len, dtype=np.float64)
        rc = self._L.hf_finish_exchange(self._h, C.c_void_p(rows_dev_ptr), C.c_void_p(row_index_dev_ptr), n_rows, world,
                                        rows_per_rank, flag_row, _dptr(self._stats_buf), self.stream)
        if rc == N.HF_E_RETRY:          # every rank gets it together: the caller runs the pass again (ShardedEMList.run_sharded)
            return None
        N.check(rc, "hf_finish_exchange")
        return self._stats_buf

    def bind_chunk_stats(self, rows_dev_ptr: int) -> None:
        N.check(self._L.hf_bind_chunk_stats(self._h, C.c_void_p(rows_dev_ptr)), "hf_bind_chunk_stats")

    def write_flag_row(self, row_dev_ptr: int) -> None:
        N.check(self._L.hf_write_flag_row(self._h, C.c_void_p(row_dev_ptr), self.stream), "hf_write_flag_row")

    def reduce_chunks_indexed(self, rows_dev_ptr: int, row_index_dev_ptr: int, n_chunks: int, dst_dev_ptr: int) -> None:
        N.check(self._L.hf_reduce_chunks_indexed(self._h, C.c_void_p(rows_dev_ptr), C.c_void_p(row_index_dev_ptr) if row_index_dev_ptr else None, n_chunks,
                                                 C.c_void_p(dst_dev_ptr), self.stream), "hf_reduce_chunks_indexed")

    def reduce_chunks(self, src_dev_ptr: int, n_chunks: int, dst_dev_ptr: int) -> None:
        N.check(self._L.hf_reduce_chunks(self._h, C.c_void_p(src_dev_ptr), n_chunks, C.c_void_p(dst_dev_ptr),
                                         self.stream), "hf_reduce_chunks")

    def em_iterate(self, model: "HMM", do_mstep: bool = True, tol: float = 1e-3, mode: int = N.HF_MODE_FULL) -> bool:
        """EM_runOneIterationForList + HMM_estimateParameters in one native call (hf_em_iterate).  Leaves the
        statistics in model.estimators; returns the convergence flag of the M-step."""
        if not hasattr(self, "_stats_buf"):
            self._stats_buf = np.empty(self.stats_len, dtype=np.float64)
            self._stats_ptr = _dptr(self._stats_buf)       # (numpy builds a new ctypes object per .ctypes access: 2 us of host time per call)
            self._cv = C.c_int(0)
            self._cv_ref = C.byref(self._cv)
        rc = self._L.hf_em_iterate(self._h, model._h, mode, int(do_mstep), tol, self._stats_ptr, self._cv_ref, self.stream)
        if rc != N.HF_OK:
            N.check(rc, "hf_em_iterate")
        model.estimators = self._stats_buf
        model.loglikelihood = float(self._stats_buf[0])
        return bool(self._cv.value)

    def kernel_ms(self) -> float:
        ms = C.c_float()
        N.check(self._L.hf_last_kernel_ms(self._h, C.byref(ms)), "hf_last_kernel_ms")
        return float(ms.value)

    def set_profiling(self, kernels=True) -> None:
        """True/False: all kernels / none; or an iterable of kernel names (hf_kernel_name) to bracket with events."""
        names = [self._L.hf_kernel_name(i).decode() for i in range(N.HF_NKERNELS)]
        if kernels is True:
            mask = ((1 << N.HF_NKERNELS) - 1) | N.HF_PROF_PASS      # every kernel + the whole pass (kernel_ms)
        elif not kernels:
            mask = 0
        else:
            mask = 0
            for k in kernels:
                mask |= 1 << names.index(k)
        N.check(self._L.hf_set_profiling(self._h, mask), "hf_set_profiling")

    def set_profiling_stride(self, every_nth_pass: int) -> None:
        """Bracket the selected kernels in every n-th pass only (hf_set_profiling_stride)."""
        N.check(self._L.hf_set_profiling_stride(self._h, int(every_nth_pass)), "hf_set_profiling_stride")

    def kernel_times(self) -> dict:
        """Duration (ms) of each selected kernel in the last pass, from HIP events on the launch stream."""
        ms = (C.c_float * N.HF_NKERNELS)()
        N.check(self._L.hf_kernel_times(self._h, ms), "hf_kernel_times")
        return {self._L.hf_kernel_name(i).decode(): float(ms[i]) for i in range(N.HF_NKERNELS)}

    def kernel_time_sums(self) -> dict:
        """{kernel: (total ms, launches)} accumulated by the library since set_profiling (HIP events on the launch stream)."""
        sums = (C.c_double * N.HF_NKERNELS)()
        cnt = (C.c_int64 * N.HF_NKERNELS)()
        N.check(self._L.hf_kernel_time_sums(self._h, sums, cnt), "hf_kernel_time_sums")
        return {self._L.hf_kernel_name(i).decode(): (float(sums[i]), int(cnt[i])) for i in range(N.HF_NKERNELS)}

    # --- results ---
    def labels(self) -> np.ndarray:
        out = np.empty(self.store.n_windows, dtype=np.int8)
        N.check(self._L.hf_get_labels(self._h, _ptr(out)), "hf_get_labels")
        return out

    def posterior(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """EM_getPosterior for windows [first, first+n) — hmm.c:671-685."""
        n = self.store.n_windows - first if n is None else n
        out = np.empty((n, 4), dtype=np.float64)
        N.check(self._L.hf_get_posterior(self._h, first, n, _dptr(out)), "hf_get_posterior")
        return out

    def viterbi(self, model: HMM):
        """Most-probable-path decoding (hf_viterbi + hf_viterbi_finish): (labels, chunk_log_probs, log_prob).  The last pass's
        results (labels(), posterior(), forward_backward()) are left as they were."""
        p = model.params()
        N.check(self._L.hf_viterbi(self._h, C.byref(p), self.stream), "hf_viterbi")
        return self._decoded("viterbi")

    def _decoded(self, prefix: str):
        """(labels, chunk_log_probs, log_prob) of the launched decoder hf_<prefix>: its _finish, then hf_get_<prefix>_labels and _chunk_log_probs."""
        fin, lab, chunk = "hf_%s_finish" % prefix, "hf_get_%s_labels" % prefix, "hf_get_%s_chunk_log_probs" % prefix
        lp = C.c_double(0.0)
        N.check(getattr(self._L, fin)(self._h, C.byref(lp), self.stream), fin)
        labels = np.empty(self.store.n_windows, dtype=np.int8)
        N.check(getattr(self._L, lab)(self._h, _ptr(labels)), lab)
        ll = np.empty(self.store.n_chunks, dtype=np.float64)
        N.check(getattr(self._L, chunk)(self._h, _dptr(ll)), chunk)
        return labels, ll, float(lp.value)

    @staticmethod
    def _four_lengths(who: str, min_len) -> np.ndarray:
        """min_len as the int32[4] the C ABI takes; `who` names the caller in the refusal."""
        ml = np.asarray(min_len)
        if ml.shape != (4,):
            raise ValueError("%s: min_len holds four window counts (Err, Dup, Hap, Col)" % who)
        return np.ascontiguousarray(ml, dtype=np.int32)

    def viterbi_minlen(self, model: HMM, min_len, joined=None):
        """The most probable path among the paths whose runs have at least min_len[s] windows (states 0 Err, 1 Dup, 2 Hap, 3 Col; runs at
        a chunk's ends are exempt; hf_viterbi_minlen + hf_viterbi_minlen_finish): (labels, chunk_log_probs, log_prob).  The last pass's
        results, viterbi()'s and the sampler's are left as they were.  joined: None, or a bool array of n_chunks as for run_moments,
        joined[c] true where chunk c continues chunk c - 1 (joined_chunks(store) derives it from the contig names): the rule then holds
        over every group of joined chunks, only runs at a group's ends are exempt (hf_viterbi_minlen_joined), and chunk_log_probs holds
        a group's score in the entry of its first chunk and 0.0 in the others."""
        ml = self._four_lengths("viterbi_minlen", min_len)
        p = model.params()
        self._minlen("viterbi_minlen", C.byref(p), ml, self._joined_u8("viterbi_minlen", joined), self.stream)
        return self._decoded("viterbi_minlen")

    def _joined_u8(self, who: str, joined) -> Optional[np.ndarray]:
        """joined as the uint8[n_chunks] the C ABI takes, None (no joins) as None; `who` names the caller in the refusal."""
        if joined is None:
            return None
        jn = np.ascontiguousarray(np.asarray(joined).ravel() != 0, np.uint8)
        if jn.size != int(self._L.hf_n_chunks(self._h)):
            raise ValueError("%s: joined must have one entry per chunk" % who)
        return jn

    def _minlen(self, base: str, head, ml: np.ndarray, jn: Optional[np.ndarray], *tail) -> None:
        """The one fork of the minimum-run-length family: hf_<base>(ctx, head, min_len, *tail), or, with joins, hf_<base>_joined(ctx,
        head, min_len, joined, *tail).  head: the parameters or the model handle; ml, jn: what _four_lengths and _joined_u8 returned.
        An error names the entry point that was called."""
        name = "hf_" + base if jn is None else "hf_%s_joined" % base
        N.check(getattr(self._L, name)(self._h, head, _ptr(ml), *(() if jn is None else (_ptr(jn),)), *tail), name)

    def minlen_posterior(self, model: HMM, min_len, joined=None) -> "MinLenPosterior":
        """The posterior given that every run has at least min_len[s] windows (states 0 Err, 1 Dup, 2 Hap, 3 Col; runs at a chunk's
        ends are exempt; hf_minlen_posterior + hf_minlen_posterior_finish), and the posterior mass the rule keeps.  The last pass's
        results, viterbi()'s, viterbi_minlen()'s and the sampler's are left as they were.  joined: None, or a bool array of n_chunks
        as for viterbi_minlen: the rule then holds over every group of joined chunks (hf_minlen_posterior_joined), and
        chunk_log_mass / chunk_log_z_adm hold a group's value in the entry of its first chunk and 0.0 in the others."""
        ml = self._four_lengths("minlen_posterior", min_len)
        p = model.params()
        tot = C.c_double(0.0)
        jn = self._joined_u8("minlen_posterior", joined)
        self._mlp_run = getattr(self, "_mlp_run", 0) + 1     # (older results stop answering posterior(): the context holds one run)
        self._minlen("minlen_posterior", C.byref(p), ml, jn, self.stream)
        N.check(self._L.hf_minlen_posterior_finish(self._h, C.byref(tot), self.stream), "hf_minlen_posterior_finish")
        labels = np.empty(self.store.n_windows, dtype=np.int8)
        N.check(self._L.hf_get_minlen_posterior_labels(self._h, _ptr(labels)), "hf_get_minlen_posterior_labels")
        mass = np.empty(self.store.n_chunks, dtype=np.float64)
        lza = np.empty(self.store.n_chunks, dtype=np.float64)
        N.check(self._L.hf_get_minlen_chunk_log_mass(self._h, _dptr(mass), _dptr(lza)), "hf_get_minlen_chunk_log_mass")
        return MinLenPosterior(self, labels, mass, lza, float(tot.value))

    def estep_minlen(self, model: HMM, min_len, joined=None):
        """The E-step under minimum run lengths (hf_estep_minlen + hf_estep_minlen_finish): (stats, log_z).  stats has finish()'s
        layout and holds the expected sufficient statistics under the posterior over the paths whose runs have at least min_len[s]
        windows (runs at a chunk's ends are exempt), element 0 the sum of log Z_adm; log_z is the sum of the plain log Z of the same
        parameters.  The last pass's results, every decoder's and the next pass are left as they were.  joined: None, or a bool array
        of n_chunks as for viterbi_minlen: the rule then holds over every group of joined chunks (hf_estep_minlen_joined), element 0
        and log_z are sums over groups, and minlen_em_chunk_stats holds a group's values in the entries of its first chunk."""
        ml = self._four_lengths("estep_minlen", min_len)
        p = model.params()
        self._minlen("estep_minlen", C.byref(p), ml, self._joined_u8("estep_minlen", joined), self.stream)
        out = np.empty(self.stats_len, dtype=np.float64)
        lz = C.c_double(0.0)
        N.check(self._L.hf_estep_minlen_finish(self._h, _dptr(out), C.byref(lz), self.stream), "hf_estep_minlen_finish")
        return out, float(lz.value)

    def minlen_pair_posterior(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """xi_adm[t][p][s] = P(s_{t-1} = p, s_t = s | data, path admissible) of the last estep_minlen / em_iterate_minlen for windows
        [first, first + n): shape (n, 4, 4); zeros at a chunk's first window (hf_get_minlen_pair_posterior)."""
        n = self.store.n_windows - first if n is None else n
        out = np.empty((n, 4, 4), dtype=np.float64)
        N.check(self._L.hf_get_minlen_pair_posterior(self._h, int(first), int(n), _dptr(out)), "hf_get_minlen_pair_posterior")
        return out

    def minlen_em_chunk_stats(self):
        """(chunk_stats [n_chunks][stats_len], log_z_adm [n_chunks], log_z [n_chunks]) of the last estep_minlen / em_iterate_minlen
        (hf_get_minlen_em_chunk_stats)."""
        nc = self.store.n_chunks
        cs = np.empty((nc, self.stats_len), dtype=np.float64)
        lza = np.empty(nc, dtype=np.float64)
        lz = np.empty(nc, dtype=np.float64)
        N.check(self._L.hf_get_minlen_em_chunk_stats(self._h, _dptr(cs), _dptr(lza), _dptr(lz)), "hf_get_minlen_em_chunk_stats")
        return cs, lza, lz

    def em_iterate_minlen(self, model: "HMM", min_len, do_mstep: bool = True, tol: float = 1e-3, joined=None) -> bool:
        """em_iterate with the E-step under minimum run lengths (hf_em_iterate_minlen): the statistics in model.estimators are
        expectations over admissible paths, model.loglikelihood the objective sum of log Z_adm, self.last_log_z the plain sum of
        log Z of the parameters the step ran with; returns the convergence flag of the M-step.  joined: as for estep_minlen
        (hf_em_iterate_minlen_joined): both sums are then over the groups of joined chunks."""
        ml = self._four_lengths("em_iterate_minlen", min_len)
        stats = np.empty(self.stats_len, dtype=np.float64)
        cv, lz = C.c_int(0), C.c_double(0.0)
        self._minlen("em_iterate_minlen", model._h, ml, self._joined_u8("em_iterate_minlen", joined), int(do_mstep), tol, _dptr(stats),
                     C.byref(lz), C.byref(cv), self.stream)
        model.estimators = stats
        model.loglikelihood = float(stats[0])
        self.last_log_z = float(lz.value)
        return bool(cv.value)

    def mea_labels(self, min_len=(1, 1, 1, 1), joined=None, gain=None):
        """Maximum-expected-accuracy decoding under minimum run lengths (hf_get_mea_labels): among the labellings whose runs have at
        least min_len[s] windows (runs at a chunk's ends exempt), the one with the largest expected gain under the posterior of the
        last full pass: (labels, block_gain, total_gain).  gain: None for the identity (the expected number of correctly labelled
        windows), or a 4x4 matrix, gain[s][k] the gain of calling k when the truth is s.  joined: None, or a bool array of n_chunks
        as for viterbi_minlen: the rule then holds over every group of joined chunks, and block_gain holds a group's score in the
        entry of its first chunk and 0.0 in the others.  The last pass's results and every decoder's are left as they were."""
        ml = self._four_lengths("mea_labels", min_len)
        jn = self._joined_u8("mea_labels", joined)
        gp = None
        if gain is not None:
            g = np.asarray(gain, dtype=np.float64)
            if g.shape != (4, 4):
                raise ValueError("mea_labels: gain is a 4x4 matrix (rows: true label, columns: called label)")
            g = np.ascontiguousarray(g)
            gp = _dptr(g)
        labels = np.empty(self.store.n_windows, dtype=np.int8)
        block = np.empty(self.store.n_chunks, dtype=np.float64)
        tot = C.c_double(0.0)
        N.check(self._L.hf_get_mea_labels(self._h, gp, _ptr(ml), _ptr(jn), _ptr(labels), _dptr(block), C.byref(tot)), "hf_get_mea_labels")
        return labels, block, float(tot.value)

    @property
    def sample_capacity(self) -> int:
        """Samples one hf_sample_paths call may draw (nine tenths of the free device memory; hf_sample_capacity)."""
        cap = int(self._L.hf_sample_capacity(self._h))
        if cap < 0:
            raise N.HFError(cap, "hf_sample_capacity")
        return cap

    def sample_paths(self, model: HMM, n_samples: int, seed: int, first_sample: int = 0) -> np.ndarray:
        """Posterior path samples first_sample .. first_sample + n_samples - 1 (hf_sample_paths, in calls of at most
        sample_capacity samples): int8[n_samples][n_windows].  The last pass's results and Viterbi's are left as they were."""
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError("sample_paths: n_samples must be >= 1")
        p = model.params()
        out = np.empty((n_samples, self.store.n_windows), dtype=np.int8)
        cap = self.sample_capacity
        if cap < 1:
            raise N.HFError(N.HF_E_ARG, "hf_sample_capacity: no room for one sample")
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        return self._drawn(out, cap, "hf_sample_finish", "hf_get_sample_labels", lambda k0, n: N.check(
            self._L.hf_sample_paths(self._h, C.byref(p), int(first_sample) + k0, n, seed, self.stream), "hf_sample_paths"))

    def _drawn(self, out: np.ndarray, cap: int, finish: str, get: str, draw) -> np.ndarray:
        """`out` filled in calls of at most `cap` samples: draw(k0, n) launches those of rows k0 .. k0 + n - 1; `finish`, `get`: the sampler's."""
        for k0 in range(0, len(out), cap):
            n = min(cap, len(out) - k0)
            draw(k0, n)
            N.check(getattr(self._L, finish)(self._h, self.stream), finish)
            for k in range(n):
                N.check(getattr(self._L, get)(self._h, k, _ptr(out[k0 + k])), get)
        return out

    def minlen_sample_capacity(self, min_len) -> int:
        """Samples one hf_sample_paths_minlen call may draw at these lengths (hf_minlen_sample_capacity)."""
        ml = self._four_lengths("minlen_sample_capacity", min_len)
        cap = int(self._L.hf_minlen_sample_capacity(self._h, _ptr(ml)))
        if cap < 0:
            raise N.HFError(cap, "hf_minlen_sample_capacity")
        return cap

    def sample_paths_minlen(self, model: HMM, min_len, n_samples: int, seed: int, first_sample: int = 0, joined=None) -> np.ndarray:
        """Samples first_sample .. first_sample + n_samples - 1 of the posterior given that every run has at least min_len[s] windows
        (runs at a chunk's ends are exempt; hf_sample_paths_minlen, in calls of at most minlen_sample_capacity samples):
        int8[n_samples][n_windows], every chunk's path admissible, -1 outside chunks.  The last pass's results and every other
        decoder's are left as they were.  joined: None, or a bool array of n_chunks as for viterbi_minlen: every path is then
        admissible over its group of joined chunks (hf_sample_paths_minlen_joined)."""
        ml = self._four_lengths("sample_paths_minlen", min_len)
        jn = self._joined_u8("sample_paths_minlen", joined)
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError("sample_paths_minlen: n_samples must be >= 1")
        p = model.params()
        out = np.empty((n_samples, self.store.n_windows), dtype=np.int8)
        cap = self.minlen_sample_capacity(ml)
        if cap < 1:
            raise N.HFError(N.HF_E_ARG, "hf_minlen_sample_capacity")
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        return self._drawn(out, cap, "hf_sample_minlen_finish", "hf_get_minlen_sample_labels", lambda k0, n: self._minlen(
            "sample_paths_minlen", C.byref(p), ml, jn, int(first_sample) + k0, n, seed, self.stream))

    def interval_log_probs(self, first, last, mask) -> np.ndarray:
        """Exact interval probabilities under the model of the last full pass (hf_get_interval_log_probs): for every job i,
        log P(every window of first[i]..last[i] (inclusive) has a state in the set mask[i] (bit s = state s) | data) -> float64[n].
        Scalars broadcast against arrays.  P(some window in state k) = -expm1 of the job with mask 15 & ~(1 << k)."""
        f, l, m = _jobs("interval_log_probs", first, last, (mask, *_MASK))
        out, = _outputs(f.size, np.float64)
        N.check(self._L.hf_get_interval_log_probs(self._h, f.size, _ptr(f), _ptr(l), _ptr(m), _dptr(out)), "hf_get_interval_log_probs")
        return out

    def count_moments(self, first, last, mask, region=None, unit="windows"):
        """Exact posterior mean and variance of label totals under the model of the last full pass (hf_get_count_moments): for every
        job i, of N = sum over the windows t of first[i]..last[i] (inclusive) of w_t * [the state of t is in the set mask[i]], with
        w_t = 1 (unit "windows") or the window's length in bases (unit "bases"), and 0 where region[i] >= 0 differs from the window's
        annotation region index (region None or -1: every window) -> (mean float64[n], var float64[n]).  Scalars broadcast."""
        units = {"windows": N.HF_COUNT_WINDOWS, "bases": N.HF_COUNT_BASES}
        if unit not in units:
            raise ValueError("count_moments: unit must be 'windows' or 'bases'")
        f, l, m, r = _jobs("count_moments", first, last, (mask, *_MASK),
                           (-1 if region is None else region, *_INT32, "a region must be -1 or a region index"))
        mean, var = _outputs(f.size, np.float64, np.float64)
        N.check(self._L.hf_get_count_moments(self._h, f.size, _ptr(f), _ptr(l), _ptr(m), None if region is None else _ptr(r), units[unit],
                                             _dptr(mean), _dptr(var)), "hf_get_count_moments")
        return mean, var

    def run_moments(self, first, last, mask, joined=None):
        """Exact posterior mean and variance of block counts under the model of the last full pass (hf_get_run_moments): for every job
        i, of the number of maximal runs of windows of first[i]..last[i] (inclusive) whose state is in the set mask[i].  joined: None, or
        a bool array of n_chunks, joined[c] true where chunk c continues chunk c - 1 (a run across that boundary is one run; joined[0]
        must be false) -> (mean float64[n], var float64[n]).  Scalars broadcast."""
        f, l, m = _jobs("run_moments", first, last, (mask, *_MASK))
        jn = self._joined_u8("run_moments", joined)
        mean, var = _outputs(f.size, np.float64, np.float64)
        N.check(self._L.hf_get_run_moments(self._h, f.size, _ptr(f), _ptr(l), _ptr(m), _ptr(jn), _dptr(mean), _dptr(var)), "hf_get_run_moments")
        return mean, var

    def long_run_log_probs(self, first, last, mask, min_len, joined=None):
        """Exact long-run probabilities under the model of the last full pass (hf_get_long_run_log_probs): for every job i, whether the
        windows first[i]..last[i] (inclusive) hold a run of at least min_len[i] consecutive windows whose state is in the set mask[i]
        (the states may change inside the set).  joined: as for run_moments, a run goes on across a joined chunk boundary
        -> (log_p_none float64[n], log_p_some float64[n]): log P(no such run | data), log P(some such run | data).  Scalars broadcast."""
        f, l, m, k = _jobs("long_run_log_probs", first, last, (mask, *_MASK),
                           (min_len, *_INT32, "a length must be a positive number of windows"))
        jn = self._joined_u8("long_run_log_probs", joined)
        none, some = _outputs(f.size, np.float64, np.float64)
        N.check(self._L.hf_get_long_run_log_probs(self._h, f.size, _ptr(f), _ptr(l), _ptr(m), _ptr(k), _ptr(jn), _dptr(none), _dptr(some)),
                "hf_get_long_run_log_probs")
        return none, some

    def run_lengths(self, first, last, mask, max_len, joined=None) -> np.ndarray:
        """The exact block-length spectrum under the model of the last full pass (hf_get_run_lengths): for every job i, the expected
        number of maximal runs of windows of first[i]..last[i] (inclusive) whose state is in the set mask[i], by length: column l - 1
        the runs of exactly l windows, l = 1..max_len, column max_len the runs of more than max_len windows (max_len 1..64, one for
        the call).  joined: as for run_moments, a run goes on across a joined chunk boundary -> float64[n, max_len + 1].  Scalars
        broadcast."""
        f, l, m = _jobs("run_lengths", first, last, (mask, *_MASK))
        L = int(max_len)
        if L != max_len or not 1 <= L <= 64:                  # (refused here: the output's width comes from it)
            raise ValueError("run_lengths: max_len must be a number of windows in 1..64")
        jn = self._joined_u8("run_lengths", joined)
        out, = _outputs(f.size, (np.float64, L + 1))
        N.check(self._L.hf_get_run_lengths(self._h, f.size, _ptr(f), _ptr(l), _ptr(m), L, _ptr(jn), _dptr(out)), "hf_get_run_lengths")
        return out

    def count_distribution(self, first, last, mask, max_count) -> np.ndarray:
        """The exact distribution of label totals under the model of the last full pass (hf_get_count_distribution): for every job i,
        the posterior probability that exactly k windows of first[i]..last[i] (inclusive) have a state in the set mask[i]: column k
        for k = 0..max_count, column max_count + 1 the probability of more than max_count windows (max_count 1..62, one for the
        call) -> float64[n, max_count + 2].  Scalars broadcast."""
        f, l, m = _jobs("count_distribution", first, last, (mask, *_MASK))
        K = int(max_count)
        if K != max_count or not -2**31 <= K < 2**31:         # (unlike run_lengths' max_len, a K outside 1..62 goes on to the library)
            raise ValueError("count_distribution: max_count must be a whole number of windows (the library refuses one outside 1..62)")
        out, = _outputs(f.size, (np.float64, max(K, 0) + 2))
        N.check(self._L.hf_get_count_distribution(self._h, f.size, _ptr(f), _ptr(l), _ptr(m), K, _dptr(out)), "hf_get_count_distribution")
        return out

    def path_entropy(self, first, last) -> np.ndarray:
        """Exact path entropy under the model of the last full pass (hf_get_path_entropy): for every job i, the Shannon entropy in nats
        of the joint posterior distribution of the labels of the windows first[i]..last[i] (inclusive; chunks are independent chains)
        -> float64[n].  exp of it is the effective number of plausible labellings of the range.  Scalars broadcast."""
        f, l = _jobs("path_entropy", first, last)
        out, = _outputs(f.size, np.float64)
        N.check(self._L.hf_get_path_entropy(self._h, f.size, _ptr(f), _ptr(l), _dptr(out)), "hf_get_path_entropy")
        return out

    def path_log_probs(self, first, last, labels) -> np.ndarray:
        """Exact log-probability of a labelling under the model of the last full pass (hf_get_path_log_probs): for every job i,
        log P(the windows first[i]..last[i] (inclusive) have the labels labels[first[i]..last[i]] | data) -> float64[n], -inf where the
        labelling is impossible.  labels: n_windows values 0..3, read only inside the jobs' ranges.  Scalars broadcast."""
        f, l = _jobs("path_log_probs", first, last)
        lab = np.asarray(labels)
        if lab.ndim != 1 or lab.size != self.store.n_windows:
            raise ValueError("path_log_probs: labels must hold one label per window")
        if lab.dtype != np.int8:
            lab = np.clip(lab, -128, 127)                      # (a label outside 0..3 stays outside)
        lab = np.ascontiguousarray(lab, np.int8)
        out, = _outputs(f.size, np.float64)
        N.check(self._L.hf_get_path_log_probs(self._h, f.size, _ptr(f), _ptr(l), _ptr(lab), _dptr(out)), "hf_get_path_log_probs")
        return out

    def entropy_profile(self, first: int = 0, n: Optional[int] = None):
        """Per-window entropies under the model of the last full pass (hf_get_entropy_profile) for windows [first, first+n):
        (marg, cond), marg[i] the entropy of the window's posterior, cond[i] the entropy of its label given the label of the window
        before (marg[i] at the first window of a chunk), in nats.  The path entropy of a range inside one chunk is marg of its first
        window plus the sum of cond over the others."""
        n = self.store.n_windows - first if n is None else n
        marg, cond = np.empty(max(n, 0)), np.empty(max(n, 0))
        N.check(self._L.hf_get_entropy_profile(self._h, first, n, _dptr(marg), _dptr(cond)), "hf_get_entropy_profile")
        return marg, cond

    def breakpoints(self, first, last, left_mask, right_mask, probs=(0.025, 0.5, 0.975)):
        """Exact breakpoint posteriors under the model of the last full pass (hf_get_breakpoints): job i says that the windows
        first[i]..last[i] (inclusive, one chunk, first < last) switch once from a state in left_mask[i] to a state in right_mask[i]
        (disjoint sets, bit s = state s); k, the first window of the right side, has the posterior p_k over first+1..last.
        -> (log_p_event float64[n], the log-probability that the range switches exactly once in that way; quantiles int64[n, len(probs)],
        the smallest k whose cumulated p reaches probs[j]; mode int64[n], the k of largest p; mode_p float64[n]).  A job without weight
        gives (-inf, -1, -1, 0.0).  Scalars broadcast."""
        f, l, u, v = _jobs("breakpoints", first, last, (left_mask, *_MASK), (right_mask, *_MASK))
        q = np.ascontiguousarray(np.asarray(probs, np.float64).ravel())
        lpe, quant, mode, mode_p = _outputs(f.size, np.float64, (np.int64, q.size), np.int64, np.float64)
        N.check(self._L.hf_get_breakpoints(self._h, f.size, _ptr(f), _ptr(l), _ptr(u), _ptr(v), q.size, _dptr(q),
                                           _dptr(lpe), _ptr(quant), _ptr(mode), _dptr(mode_p)), "hf_get_breakpoints")
        return lpe, quant, mode, mode_p

    def breakpoint_profile(self, first: int, last: int, left_mask: int, right_mask: int):
        """The posterior of one breakpoint job (hf_get_breakpoint_profile): (p float64[last - first], p[i] the probability that window
        first + 1 + i is the first of the right side, given that the range switches once; log_p_event).  The values the batch call
        derives its quantiles and mode from, bit for bit."""
        if not (0 <= int(left_mask) <= 255 and 0 <= int(right_mask) <= 255):
            raise ValueError("breakpoint_profile: " + _MASK[3])
        p = np.empty(max(int(last) - int(first), 0), dtype=np.float64)
        lpe = np.empty(1, dtype=np.float64)
        N.check(self._L.hf_get_breakpoint_profile(self._h, int(first), int(last), int(left_mask), int(right_mask), _dptr(p), _dptr(lpe)),
                "hf_get_breakpoint_profile")
        return p, float(lpe[0])

    def set_alpha_stats(self, on: bool = True) -> None:
        """hf_set_alpha_stats: full passes from now on can be asked for the alpha statistics (alpha_stats)."""
        N.check(self._L.hf_set_alpha_stats(self._h, int(bool(on))), "hf_set_alpha_stats")

    def alpha_stats(self) -> np.ndarray:
        """The alpha statistics of the last full pass (hf_get_alpha_stats): float64[n_regions][2][4][4], [r][0] = G the derivative of the
        log-likelihood in alpha[pre][s], [r][1] = H the curvature of the expected complete-data log-likelihood."""
        out = np.empty(int(self._L.hf_alpha_stats_len(self._h)), dtype=np.float64)
        N.check(self._L.hf_get_alpha_stats(self._h, _dptr(out)), "hf_get_alpha_stats")
        return out.reshape(-1, 2, 4, 4)

    def forward_backward(self, first: int = 0, n: Optional[int] = None):
        n = self.store.n_windows - first if n is None else n
        f, b, sc = np.empty((n, 4)), np.empty((n, 4)), np.empty(n)
        N.check(self._L.hf_get_forward_backward(self._h, first, n, _dptr(f), _dptr(b), _dptr(sc)),
                "hf_get_forward_backward")
        return f, b, sc


def _method_of(emList, name: str, who: str, what: str):
    """emList.<name> for the wrapper `who`, or its TypeError: any list with that method will do, one without it has no <what>."""
    if not hasattr(emList, name):
        raise TypeError("%s: %s has no %s" % (who, type(emList).__name__, what))
    return getattr(emList, name)


def EM_runOneIterationForList(emList, model: HMM, threads: int = 0) -> None:
    """hmm.c:739-763.  `threads` is accepted for signature compatibility; the result never depended
    on it.  `emList` is an EMList or a dist.ShardedEMList."""
    if hasattr(emList, "run_sharded"):
        stats = emList.run_sharded(model, N.HF_MODE_FULL)
    else:
        emList.launch(model, N.HF_MODE_FULL)
        stats = emList.finish()
    model.estimators = stats
    model.loglikelihood = float(stats[0])


def EM_runOneMinLengthIterationForList(emList, model: HMM, min_len, joined=None) -> float:
    """EM_runOneIterationForList with the E-step under minimum run lengths (no counterpart in the reference): model.estimators holds the
    expected statistics under the posterior over admissible paths, model.loglikelihood the sum of log Z_adm.  Returns the plain sum of
    log Z of the same parameters.  joined[c] says that chunk c continues chunk c - 1 (joined_chunks): the rule then holds over whole
    groups of joined chunks and both sums run over the groups.  `emList`: an EMList."""
    estep_minlen = _method_of(emList, "estep_minlen", "EM_runOneMinLengthIterationForList", "E-step under minimum run lengths")
    stats, log_z = estep_minlen(model, min_len) if joined is None else estep_minlen(model, min_len, joined)
    model.estimators = stats
    model.loglikelihood = float(stats[0])
    return log_z


def EM_runForwardForList(emList, model: HMM, threads: int = 0) -> None:
    """hmm.c:790-816 — forward only; sets model.loglikelihood."""
    if hasattr(emList, "run_sharded"):
        stats = emList.run_sharded(model, N.HF_MODE_FORWARD_ONLY)
    else:
        emList.launch(model, N.HF_MODE_FORWARD_ONLY)
        stats = emList.finish()
    model.loglikelihood = float(stats[0])


def EM_runViterbiForList(emList, model: HMM):
    """Most-probable-path decoding of every chunk with the model's current parameters (no counterpart in the reference, which
    decodes by posterior argmax only): (labels: int8[n_windows], chunk_log_probs: float64[n_chunks], log_prob: float), the run's
    score being the sum of the chunk scores in list order.  `emList`: an EMList, MultiEMList or RankEMList."""
    return _method_of(emList, "viterbi", "EM_runViterbiForList", "most-probable-path decoder")(model)


def EM_runMinLengthViterbiForList(emList, model: HMM, min_len, joined=None):
    """Most-probable-path decoding under minimum run lengths (no counterpart in the reference, which relabels short runs after decoding):
    the best path among those whose runs of state s have at least min_len[s] windows, runs at a chunk's ends exempt.  Returns what
    EM_runViterbiForList returns.  joined[c] says that chunk c continues chunk c - 1 (joined_chunks): the rule then holds over whole
    groups of joined chunks and only runs at a group's ends are exempt.  `emList`: an EMList."""
    viterbi_minlen = _method_of(emList, "viterbi_minlen", "EM_runMinLengthViterbiForList", "minimum-run-length decoder")
    if joined is None:
        return viterbi_minlen(model, min_len)
    return viterbi_minlen(model, min_len, joined)


def joined_chunks(store) -> np.ndarray:
    """The `joined` array of a store: bool[n_chunks], true where chunk c carries the contig name of chunk c - 1 (the chunks of a contig
    as the final BED merges them; the rule of hmm_flagger --numBlocks)."""
    ctg = np.asarray(store.chunk_ctg)
    out = np.zeros(ctg.size, bool)
    if ctg.size > 1:
        out[1:] = ctg[1:] == ctg[:-1]
    return out


class MinLenPosterior:
    """What EMList.minlen_posterior returns: `labels` (first-max argmax of the constrained posterior, -1 outside chunks),
    `chunk_log_mass` (log P(path of the chunk admissible | data)), `chunk_log_z_adm`, `log_mass` (the sum over chunks in list order)
    and posterior(first, n), which reads the context's buffers: it answers until the list's next minlen_posterior call or close(),
    and raises RuntimeError afterwards."""

    def __init__(self, em, labels, chunk_log_mass, chunk_log_z_adm, log_mass):
        self._em = em
        self._run = em._mlp_run
        self.labels = labels
        self.chunk_log_mass = chunk_log_mass
        self.chunk_log_z_adm = chunk_log_z_adm
        self.log_mass = log_mass

    def posterior(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """P(s_t = s | data, path admissible) of windows [first, first + n)."""
        em = self._em
        if not getattr(em, "_h", None):
            raise RuntimeError("MinLenPosterior.posterior: the list is closed")
        if em._mlp_run != self._run:
            raise RuntimeError("MinLenPosterior.posterior: the list has run minlen_posterior again; its buffers hold the later run")
        n = em.store.n_windows - first if n is None else n
        out = np.empty((max(int(n), 0), 4), dtype=np.float64)
        N.check(em._L.hf_get_minlen_posterior(em._h, int(first), int(n), _dptr(out)), "hf_get_minlen_posterior")
        return out


def EM_runMinLengthPosteriorForList(emList, model: HMM, min_len, joined=None) -> MinLenPosterior:
    """The posterior under minimum run lengths (no counterpart in the reference): per-window label probabilities given that every run
    of state s has at least min_len[s] windows, runs at a chunk's ends exempt, and the posterior mass of those paths per chunk.
    joined[c] says that chunk c continues chunk c - 1 (joined_chunks): the rule then holds over whole groups of joined chunks and
    only runs at a group's ends are exempt.  `emList`: an EMList."""
    minlen_posterior = _method_of(emList, "minlen_posterior", "EM_runMinLengthPosteriorForList", "minimum-run-length posterior")
    if joined is None:
        return minlen_posterior(model, min_len)
    return minlen_posterior(model, min_len, joined)


def EM_getMaxExpectedGainLabelsForList(emList, min_len, joined=None, gain=None):
    """Maximum-expected-accuracy decoding under minimum run lengths (the exact form of what the reference's final BED approximates by
    relabelling short runs of the posterior argmax): among the labellings whose runs of state s have at least min_len[s] windows, the
    one with the largest expected gain under the posterior of the last full pass; gain None counts correctly labelled windows.
    Returns (labels: int8[n_windows], block_gain: float64[n_chunks], total_gain: float).  joined[c] says that chunk c continues chunk
    c - 1 (joined_chunks): the rule then holds over whole groups of joined chunks.  `emList`: an EMList."""
    return _method_of(emList, "mea_labels", "EM_getMaxExpectedGainLabelsForList", "maximum-expected-accuracy decoder")(min_len, joined, gain)


def EM_samplePathsForList(emList, model: HMM, n_samples: int, seed: int) -> np.ndarray:
    """Draws of whole state paths from P(path | data) with the model's current parameters (forward filtering, backward sampling; no
    counterpart in the reference): int8[n_samples][n_windows], sample k drawn from (seed, k) alone.  `emList`: an EMList."""
    return _method_of(emList, "sample_paths", "EM_samplePathsForList", "path sampler")(model, n_samples, seed)


def EM_sampleMinLengthPathsForList(emList, model: HMM, min_len, n_samples: int, seed: int, joined=None) -> np.ndarray:
    """n_samples admissible paths drawn from the posterior under minimum run lengths with the model's current parameters (no counterpart
    in the reference): int8[n_samples][n_windows], sample k drawn from (seed, k, min_len) alone.  joined[c] says that chunk c continues
    chunk c - 1 (joined_chunks): every path is then admissible over its whole group of joined chunks.  `emList`: an EMList."""
    sample_paths_minlen = _method_of(emList, "sample_paths_minlen", "EM_sampleMinLengthPathsForList", "admissible path sampler")
    if joined is None:
        return sample_paths_minlen(model, min_len, n_samples, seed)
    return sample_paths_minlen(model, min_len, n_samples, seed, joined=joined)


def EM_getIntervalLogProbsForList(emList, first, last, mask) -> np.ndarray:
    """log P(every window of first[i]..last[i] has a state in mask[i] | data) under the model of the last full pass, per job (no
    counterpart in the reference): float64[n].  `emList`: an EMList."""
    return _method_of(emList, "interval_log_probs", "EM_getIntervalLogProbsForList", "interval getter")(first, last, mask)


def EM_getCountMomentsForList(emList, first, last, mask, region=None, unit="windows"):
    """Exact posterior (mean, variance) of the number of windows (or bases) of first[i]..last[i] whose state lies in mask[i], optionally
    only those of annotation region region[i], under the model of the last full pass, per job (no counterpart in the reference):
    (float64[n], float64[n]).  `emList`: an EMList."""
    return _method_of(emList, "count_moments", "EM_getCountMomentsForList", "count-moments getter")(first, last, mask, region, unit)


def EM_getRunMomentsForList(emList, first, last, mask, joined=None):
    """Exact posterior (mean, variance) of the number of blocks (maximal runs of windows) of first[i]..last[i] whose state lies in
    mask[i], under the model of the last full pass, per job; joined[c] says that chunk c continues chunk c - 1, so that a run across
    the boundary counts once (no counterpart in the reference): (float64[n], float64[n]).  `emList`: an EMList."""
    return _method_of(emList, "run_moments", "EM_getRunMomentsForList", "run-moments getter")(first, last, mask, joined)


def EM_getLongRunLogProbsForList(emList, first, last, mask, min_len, joined=None):
    """(log P(no run), log P(some run)) of at least min_len[i] consecutive windows of first[i]..last[i] whose state lies in mask[i],
    under the model of the last full pass, per job; joined[c] says that chunk c continues chunk c - 1, so that a run goes on across the
    boundary (no counterpart in the reference): (float64[n], float64[n]).  `emList`: an EMList."""
    return _method_of(emList, "long_run_log_probs", "EM_getLongRunLogProbsForList", "long-run getter")(first, last, mask, min_len, joined)


def EM_getRunLengthsForList(emList, first, last, mask, max_len, joined=None) -> np.ndarray:
    """The expected number of blocks (maximal runs of windows) of first[i]..last[i] whose state lies in mask[i], by length 1..max_len
    and above, under the model of the last full pass, per job; joined[c] says that chunk c continues chunk c - 1, so that a run goes on
    across the boundary (no counterpart in the reference): float64[n, max_len + 1].  `emList`: an EMList."""
    return _method_of(emList, "run_lengths", "EM_getRunLengthsForList", "run-length getter")(first, last, mask, max_len, joined)


def EM_getCountDistributionForList(emList, first, last, mask, max_count) -> np.ndarray:
    """The posterior distribution of the number of windows of first[i]..last[i] whose state lies in mask[i], under the model of the
    last full pass, per job: P(N = k), k = 0..max_count, and P(N > max_count) (no counterpart in the reference):
    float64[n, max_count + 2].  `emList`: an EMList."""
    return _method_of(emList, "count_distribution", "EM_getCountDistributionForList", "count-distribution getter")(first, last, mask, max_count)


def EM_getPathEntropyForList(emList, first, last) -> np.ndarray:
    """Exact Shannon entropy (nats) of the posterior distribution over the label paths of the windows first[i]..last[i], under the model
    of the last full pass, per job (no counterpart in the reference): float64[n].  `emList`: an EMList."""
    return _method_of(emList, "path_entropy", "EM_getPathEntropyForList", "path-entropy getter")(first, last)


def EM_getPathLogProbsForList(emList, first, last, labels) -> np.ndarray:
    """log P(the windows first[i]..last[i] have the labels labels[first[i]..last[i]] | data) under the model of the last full pass, per
    job (no counterpart in the reference): float64[n].  `emList`: an EMList."""
    return _method_of(emList, "path_log_probs", "EM_getPathLogProbsForList", "path log-probability getter")(first, last, labels)


def EM_getEntropyProfileForList(emList, first: int = 0, n: Optional[int] = None):
    """(marg, cond): per window, the entropy of its posterior and the entropy of its label given the label of the window before, under
    the model of the last full pass (no counterpart in the reference).  `emList`: an EMList."""
    return _method_of(emList, "entropy_profile", "EM_getEntropyProfileForList", "entropy profile")(first, n)


def EM_getBreakpointsForList(emList, first, last, left_mask, right_mask, probs=(0.025, 0.5, 0.975)):
    """(log_p_event, quantiles, mode, mode_p) of the window at which first[i]..last[i] switches from a state of left_mask[i] to one of
    right_mask[i], given that it switches once, under the model of the last full pass, per job (no counterpart in the reference).
    `emList`: an EMList."""
    return _method_of(emList, "breakpoints", "EM_getBreakpointsForList", "breakpoint getter")(first, last, left_mask, right_mask, probs)


class EMBatch:
    """Many models over ONE window store (hf_batch_*, flagger_amd/csrc/hf_batch.h): one device context, the windows uploaded and planned
    once, and the pass state of len(models) models beside it.  Model m of a batch gets the single context's bits for the same
    parameters.  `store`: a WindowStore (a context is created from it with models[0]'s region and component layout) or an EMList
    whose context the batch then shares (the EMList itself is not touched by the batch's passes).  The context must be of the
    default algorithm with one sub-pass, and the models trunc_exp_gaussian or gaussian: else hf_batch_create raises."""

    def __init__(self, store, models: Sequence[HMM], adjustContigEnds: bool = True, minReadFractionAtEnds: float = 0.95,
                 device: int = 0, algo: int = N.HF_ALGO_SCAN, stream: int = 0):
        if len(models) < 1:
            raise ValueError("EMBatch: no models")
        L = N.lib()
        self._L = L
        self._b = None
        self.models = list(models)
        if isinstance(store, EMList):
            self.em = store
        else:
            self.em = EMList(store, self.models[0], adjustContigEnds, minReadFractionAtEnds, device=device, algo=algo, stream=stream)
        self.stream = self.em.stream
        self.stats_len = self.em.stats_len
        b = C.c_void_p()
        N.check(L.hf_batch_create(self.em._h, len(self.models), C.byref(b)), "hf_batch_create")
        self._b = b

    @property
    def size(self) -> int:
        return len(self.models)

    @property
    def shared_models(self) -> int:
        """Models of the last pass whose segment kernel ran in the shared launch (k_seg_fb_batch); the others ran their own pass."""
        return int(self._L.hf_batch_shared_models(self._b))

    def handoff(self, m: int):
        """(epoch, flags uint32[segments]) of model m: its hand-off epoch and the flag word of every chunk segment (hf_batch_handoff)."""
        epoch = C.c_uint32(0)
        n = int(self._L.hf_batch_handoff(self._b, int(m), C.byref(epoch), None, 0))
        if n < 0:
            raise N.HFError(n, "hf_batch_handoff")
        flags = np.zeros(n, dtype=np.uint32)
        n = int(self._L.hf_batch_handoff(self._b, int(m), C.byref(epoch), _ptr(flags), n))
        if n < 0:
            raise N.HFError(n, "hf_batch_handoff")
        return int(epoch.value), flags

    def capacity(self) -> int:
        """hf_batch_capacity of the underlying context: models whose pass state fits the device's free memory."""
        return int(self._L.hf_batch_capacity(self.em._h))

    def close(self):
        if getattr(self, "_b", None):
            self._L.hf_batch_destroy(self._b)
            self._b = None

    def __del__(self):
        self.close()

    def _active(self, active) -> np.ndarray:
        act = np.arange(self.size, dtype=np.int32) if active is None else np.ascontiguousarray(active, dtype=np.int32)
        if act.ndim != 1:
            raise ValueError("EMBatch: `active` is a list of model indices")
        return act

    def launch(self, models: Optional[Sequence[HMM]] = None, active=None, mode: int = N.HF_MODE_FULL) -> np.ndarray:
        """Enqueue one pass of the models `active` (default: all); models[i] (default: the batch's own) parameterises active[i]."""
        act = self._active(active)
        ms = [self.models[int(m)] for m in act] if models is None else list(models)
        if len(ms) != len(act):
            raise ValueError("EMBatch: one model per active index")
        ps = (N.hf_params * max(len(act), 1))()
        for i, m in enumerate(ms):
            ps[i] = m.params()
        self._keep = ms                                  # (the parameter views point into the models until the pass is enqueued)
        N.check(self._L.hf_batch_estep(self._b, ps, _ptr(act), len(act), mode, self.stream), "hf_batch_estep")
        return act

    def finish(self, n_active: int):
        stats = np.empty((n_active, self.stats_len), dtype=np.float64)
        status = np.zeros(n_active, dtype=np.int32)
        N.check(self._L.hf_batch_finish(self._b, _dptr(stats), _ptr(status), self.stream), "hf_batch_finish")
        return stats, status

    def estep(self, models: Optional[Sequence[HMM]] = None, active=None, mode: int = N.HF_MODE_FULL):
        """One batched pass: (stats[len(active)][V], status[len(active)]) — status[i] is model active[i]'s HF_E_* (HF_OK, HF_E_SCALE,
        HF_E_NAN, ...); a failing model does not disturb the others."""
        act = self.launch(models, active, mode)
        return self.finish(len(act))

    def labels(self, m: int) -> np.ndarray:
        out = np.empty(self.em.store.n_windows, dtype=np.int8)
        N.check(self._L.hf_batch_get_labels(self._b, int(m), _ptr(out)), "hf_batch_get_labels")
        return out

    def posterior(self, m: int, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.em.store.n_windows - first if n is None else n
        out = np.empty((n, 4), dtype=np.float64)
        N.check(self._L.hf_batch_get_posterior(self._b, int(m), int(first), int(n), _dptr(out)), "hf_batch_get_posterior")
        return out


def EM_runBatchForList(emBatch: EMBatch, models: Optional[Sequence[HMM]] = None, active=None, mode: int = N.HF_MODE_FULL) -> np.ndarray:
    """EM_runOneIterationForList for the models of a batch: one batched pass; every model whose status is HF_OK gets its statistics
    and log-likelihood (model.estimators, model.loglikelihood) as EM_runOneIterationForList would set them.  Returns the statuses."""
    act = emBatch._active(active)
    ms = [emBatch.models[int(m)] for m in act] if models is None else list(models)
    stats, status = emBatch.estep(ms, act, mode)
    for i, m in enumerate(ms):
        if status[i] == N.HF_OK:
            m.estimators = stats[i].copy()
            m.loglikelihood = float(stats[i][0])
    return status


def HMM_estimateParameters(model: HMM, convergenceTol: float) -> bool:
    """hmm.c:120-127; consumes the statistics left by EM_runOneIterationForList."""
    if model.estimators is None:
        raise RuntimeError("HMM_estimateParameters: no statistics (run EM_runOneIterationForList first)")
    st = np.ascontiguousarray(model.estimators, dtype=np.float64)
    return bool(N.lib().hfm_estimate(model._h, _dptr(st), float(convergenceTol)))


# the ten entries (pre, state) the reference's tuner frees (programs/src/tune_alpha_hmm_flagger.py), its bounds
FIT_ALPHA_ENTRIES = ((0, 0), (0, 2), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (2, 3), (3, 2), (3, 3))
FIT_ALPHA_MAX = 0.8


def alpha_free_mask(entries=FIT_ALPHA_ENTRIES) -> np.ndarray:
    m = np.zeros((4, 4), dtype=np.uint8)
    for p, s in entries:
        if not (0 <= int(p) < 4 and 0 <= int(s) < 4):
            raise ValueError("alpha entry (%r, %r): pre and state must be 0..3" % (p, s))
        m[int(p), int(s)] = 1
    return m


def HMM_estimateAlpha(model: HMM, alphaStats: np.ndarray, convergenceTol: float, entries=FIT_ALPHA_ENTRIES, lo: float = 0.0,
                      hi: float = FIT_ALPHA_MAX) -> bool:
    """hfm_estimate_alpha: one conditional maximisation of the free alpha entries from the alpha statistics of the pass whose statistics
    vector is in model.estimators (EMList.alpha_stats after EM_runOneIterationForList); True when every free entry moved by less than
    the tolerance."""
    if model.estimators is None:
        raise RuntimeError("HMM_estimateAlpha: no statistics (run EM_runOneIterationForList first)")
    st = np.ascontiguousarray(model.estimators, dtype=np.float64)
    a = np.ascontiguousarray(alphaStats, dtype=np.float64).ravel()
    if a.size != 32 * model.numberOfRegions:
        raise ValueError("HMM_estimateAlpha: alphaStats must hold 32 doubles per region")
    mask = np.ascontiguousarray(alpha_free_mask(entries).ravel())
    rc = N.lib().hfm_estimate_alpha(model._h, _dptr(a), _dptr(st), _ptr(mask), float(lo), float(hi),
                                    float(convergenceTol))
    if rc < 0:
        raise ValueError("HMM_estimateAlpha: bad argument (bounds outside [0, 1), or a negative_binomial model)")
    return bool(rc)


def HMM_resetEstimators(model: HMM) -> None:
    """hmm.c:129-134."""
    model.estimators = None


def runHMMFlagger(emList, model: HMM, numberOfIterations: int = 100, convergenceTol: float = 0.001,
                  outputDir: Optional[str] = None, writeParameterStatsPerIteration: bool = False,
                  is_writer: bool = True, fitAlpha: bool = False, fitAlphaEntries=FIT_ALPHA_ENTRIES, fitAlphaMax: float = FIT_ALPHA_MAX,
                  fitAlphaEvery: int = 2, constrainedMinLen=None, constrainedJoined=None) -> List[float]:
    """EM outer loop of hmm_flagger.c:285-488 (no --accelerate here: that loop is flagger_amd/csrc/hf_squarem.h, driven by the command line).  Returns the
    log-likelihood of every E-pass (the rows of the log-likelihood table, _RunFiles).
    constrainedMinLen (an EMList only; four window counts): the EM iterations run on the E-step under minimum run lengths
    (em_iterate_minlen), so their rows hold the objective sum of log Z_adm, and length_constrained_em.tsv holds per iteration
    log Z_adm, log Z and their difference; the final inference pass stays the plain pass with the fitted parameters.
    constrainedJoined (only with constrainedMinLen; a bool array of n_chunks, joined_chunks(store) derives it): those iterations run on
    the E-step over groups of joined chunks (em_iterate_minlen(joined=...)); the same files, the values are the sums over groups.
    fitAlpha (an EMList only): the k-th iteration, k = 1, 2, ..., is an alpha-iteration when k is a multiple of fitAlphaEvery — its pass is
    followed by HMM_estimateAlpha alone; the others are ordinary iterations (HMM_estimateParameters alone).  The run has converged when
    the latest iteration of each kind reported convergence."""
    if constrainedJoined is not None and constrainedMinLen is None:
        raise ValueError("runHMMFlagger: constrainedJoined needs constrainedMinLen")
    variant = "minlen" if constrainedMinLen is not None else "alpha" if fitAlpha else "plain"
    files = _RunFiles(outputDir if is_writer else None, writeParameterStatsPerIteration, variant)
    if variant == "minlen":
        if fitAlpha:
            raise ValueError("runHMMFlagger: constrainedMinLen cannot be combined with fitAlpha")
        step = _minlen_step(emList, model, convergenceTol, files, constrainedMinLen, constrainedJoined)
    elif variant == "alpha":
        step = _alpha_step(emList, model, convergenceTol, files, fitAlphaEntries, fitAlphaMax, int(fitAlphaEvery))
        emList.set_alpha_stats(True)
    else:
        step = _plain_step(emList, model, convergenceTol)
    try:
        with files:
            return _em_loop(emList, model, numberOfIterations, files, step)
    finally:
        if variant == "alpha":
            emList.set_alpha_stats(False)


LCEM_HEADER = "#Iteration\tLog_Z_adm\tLog_Z\tLog_mass\n"


class _RunFiles:
    """The files of one runHMMFlagger run, opened on entering and closed on leaving its `with` block: the log-likelihood table, the
    table of the variant ("minlen": length_constrained_em.tsv, "alpha": alpha_trace.tsv, "plain": none), the parameter files and,
    for "alpha", alpha_fitted.tsv.  Every name, header and row format of the run is here; without a directory nothing is written."""
    TABLES = {"plain": None, "minlen": ("length_constrained_em.tsv", LCEM_HEADER), "alpha": ("alpha_trace.tsv", "")}

    def __init__(self, outputDir: Optional[str], everyIteration: bool, variant: str):
        self.dir, self.every_iteration, self.variant = outputDir, everyIteration, variant
        self._ll = self._table = None
        self._open = contextlib.ExitStack()

    def _opened(self, name: str, header: str):
        f = self._open.enter_context(open(os.path.join(self.dir, name), "w"))
        f.write(header)
        return f

    def __enter__(self):
        try:
            if self.dir is not None:
                self._ll = self._opened("loglikelihood.tsv", "#Iteration\tEffective_Iteration\tLoglikelihood\n")
                if self.TABLES[self.variant]:
                    self._table = self._opened(*self.TABLES[self.variant])
        except BaseException:
            self._open.close()
            raise
        return self

    def __exit__(self, *exc):
        self._open.close()

    def loglikelihood(self, iteration: int, ll: float) -> None:
        if self._ll:
            self._ll.write("%d\t%d\t%.4f\n" % (iteration, iteration, ll))

    def constrained_row(self, iteration: int, log_z_adm: float, log_z: float) -> None:
        if self._table:
            self._table.write("%d\t%.4f\t%.4f\t%.4f\n" % (iteration, log_z_adm, log_z, log_z_adm - log_z))

    def alpha_trace_row(self, iteration: int, model: HMM, stats: np.ndarray) -> None:
        """The iteration, its log-likelihood, the alpha matrix the pass ran with and the alpha statistics summed over the regions."""
        if self._table:
            self._table.write("\t".join(["%d" % iteration, "%.17g" % model.loglikelihood] + ["%.17g" % v for v in model.alpha.ravel()] +
                                        ["%.17g" % v for v in stats.ravel()]) + "\n")

    def parameters(self, model: HMM, point: str) -> None:
        """transition_<point>.tsv and emission_<point>.tsv; point: "initial" (transition_initial.tsv), "iteration_<k>" or "final"."""
        if self.dir is not None:
            model.writeTransitionTsv(os.path.join(self.dir, "transition_%s.tsv" % point))
            model.writeEmissionTsv(os.path.join(self.dir, "emission_%s.tsv" % point))

    def iteration(self, model: HMM, it: int) -> None:
        if self.every_iteration:
            self.parameters(model, "iteration_%d" % it)

    def final(self, model: HMM) -> None:
        self.parameters(model, "final")
        if self.dir is not None and self.variant == "alpha":
            with open(os.path.join(self.dir, "alpha_fitted.tsv"), "w") as f:
                for row in model.alpha:
                    f.write("\t".join("%.17g" % v for v in row) + "\n")


def _em_loop(emList, model: HMM, numberOfIterations: int, files: _RunFiles, step) -> List[float]:
    """The EM outer loop, once for every variant.  step(it, record) runs iteration `it`: its pass, then record() (the pass's
    log-likelihood into the returned list and its row into the table), then whatever moves the parameters; it returns whether the
    run has converged.  The final inference pass is the plain pass with the fitted parameters (hmm_flagger.c:464)."""
    lls: List[float] = []
    it, converged = 1, False

    def record():
        lls.append(model.loglikelihood)
        files.loglikelihood(it - 1, model.loglikelihood)

    files.parameters(model, "initial")
    while it <= numberOfIterations and not converged:
        converged = step(it, record)
        HMM_resetEstimators(model)
        files.iteration(model, it)
        it += 1
    EM_runOneIterationForList(emList, model)
    record()
    files.final(model)
    return lls


def _plain_step(emList, model: HMM, tol: float):
    """An ordinary iteration: one native call where the list has the fused one (single GPU: E-step + M-step), else the pass, then
    HMM_estimateParameters."""
    fused = hasattr(emList, "em_iterate")

    def step(it, record):
        if fused:
            converged = emList.em_iterate(model, True, tol)
        else:
            EM_runOneIterationForList(emList, model)
        record()
        return converged if fused else HMM_estimateParameters(model, tol)
    return step


def _minlen_step(emList, model: HMM, tol: float, files: _RunFiles, min_len, joined):
    """An iteration on the E-step under minimum run lengths (em_iterate_minlen; `joined` is passed only where it is given)."""
    em_iterate_minlen = _method_of(emList, "em_iterate_minlen", "runHMMFlagger(constrainedMinLen=...)", "E-step under minimum run lengths")
    if model.modelType == MODEL_NEGATIVE_BINOMIAL:
        raise ValueError("constrainedMinLen: the negative_binomial model is not supported")
    joins = {} if joined is None else {"joined": joined}

    def step(it, record):
        converged = em_iterate_minlen(model, min_len, True, tol, **joins)
        record()
        files.constrained_row(it - 1, model.loglikelihood, emList.last_log_z)
        return converged
    return step


def _alpha_step(emList, model: HMM, tol: float, files: _RunFiles, entries, alphaMax: float, every: int):
    """The pass, then HMM_estimateAlpha alone in every `every`-th iteration and HMM_estimateParameters alone in the others; converged
    when the latest iteration of each kind was."""
    _method_of(emList, "alpha_stats", "runHMMFlagger(fitAlpha=True)", "alpha statistics")
    if every < 1:
        raise ValueError("fitAlphaEvery must be at least 1")
    if model.modelType == MODEL_NEGATIVE_BINOMIAL:
        raise ValueError("fitAlpha: the negative_binomial emission has no alpha")
    alpha_free_mask(entries)
    converged = {"em": False, "alpha": False}

    def step(it, record):
        EM_runOneIterationForList(emList, model)
        record()
        if it % every == 0:
            files.alpha_trace_row(it - 1, model, emList.alpha_stats().sum(axis=0))
            converged["alpha"] = HMM_estimateAlpha(model, emList.alpha_stats(), tol, entries, 0.0, alphaMax)
        else:
            converged["em"] = HMM_estimateParameters(model, tol)
        return converged["em"] and converged["alpha"]
    return step
