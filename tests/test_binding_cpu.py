"""CPU checks of the Python binding's own code (flagger_amd/hmm.py), none of which needs a device: the job front of the range getters,
the `joined` and `min_len` conversions, the exact call every EM_*ForList wrapper forwards, and the EM outer loop of runHMMFlagger in its
three variants on a scripted list: the files it writes, their text, the returned list and the order of calls.

The EM_*ForList and runHMMFlagger parts use public names only and were written against the loops as they stood before they became one:
they passed there unchanged, except test_files_are_closed_when_a_pass_raises[plain], the one intended difference (the plain loop left
loglikelihood.tsv open when a pass raised)."""
import builtins
import os
import types

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm
from test_bruteforce_cpu import _tiny_store


# ---- 1. the job front ------------------------------------------------------------------------------------------------------------
def _is_column(a, dtype, n):
    return isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == (n,) and a.flags.c_contiguous


def test_job_front_broadcasts_scalars_and_states_the_dtypes():
    f, l, m, r = hmm._jobs("who", 3, [4, 5, 6], (7, *hmm._MASK), ([-1, 0, 1], np.int32))
    assert _is_column(f, np.int64, 3) and _is_column(l, np.int64, 3) and _is_column(m, np.uint8, 3) and _is_column(r, np.int32, 3)
    assert f.tolist() == [3, 3, 3] and l.tolist() == [4, 5, 6] and m.tolist() == [7, 7, 7] and r.tolist() == [-1, 0, 1]
    f, l = hmm._jobs("who", 1, 2)                                       # all scalars: one job
    assert _is_column(f, np.int64, 1) and _is_column(l, np.int64, 1)
    f, l, m = hmm._jobs("who", [[1, 2], [3, 4]], 9, ([[1], [2]], *hmm._MASK))     # two dimensions: ravelled in C order
    assert f.tolist() == [1, 2, 3, 4] and l.tolist() == [9] * 4 and m.tolist() == [1, 1, 2, 2] and _is_column(m, np.uint8, 4)


def test_job_front_converts_what_it_is_given():
    """A non-contiguous or wrong-dtype input is converted, not refused."""
    strided = np.arange(10, dtype=np.int64)[::3]                         # 0, 3, 6, 9
    assert not strided.flags.c_contiguous or strided.strides != (8,)
    f, l, m = hmm._jobs("who", strided, np.array([9.0, 9.0, 9.0, 9.0], np.float32), (np.array([1, 2, 4, 8], np.int16), *hmm._MASK))
    assert _is_column(f, np.int64, 4) and f.tolist() == [0, 3, 6, 9] and f.strides == (8,)
    assert _is_column(l, np.int64, 4) and l.tolist() == [9] * 4
    assert _is_column(m, np.uint8, 4) and m.tolist() == [1, 2, 4, 8]


def test_job_front_mask_range():
    """-1 and 256 are refused here; 0 and 255 (and 16..254) are the library's to refuse."""
    for bad in (-1, 256, [1, -1], [3, 256]):
        with pytest.raises(ValueError, match="^getter: a state mask must be 1..15$"):
            hmm._jobs("getter", [0, 1], [1, 2], (bad, *hmm._MASK))
    f, l, m = hmm._jobs("getter", [0, 1], [1, 2], ([0, 255], *hmm._MASK))
    assert m.tolist() == [0, 255] and m.dtype == np.uint8
    with pytest.raises(ValueError, match="^getter: a region$"):           # a column's own range and words
        hmm._jobs("getter", 0, 1, (1, *hmm._MASK), (2 ** 31, np.int32, -2 ** 31, 2 ** 31 - 1, "a region"))
    assert hmm._jobs("getter", 0, 1, (-2 ** 31, np.int32, -2 ** 31, 2 ** 31 - 1, "a region"))[2].tolist() == [-2 ** 31]
    with pytest.raises(ValueError, match="^getter: a state mask must be 1..15$"):   # the columns are checked in the order given
        hmm._jobs("getter", 0, 1, (256, *hmm._MASK), (2 ** 31, np.int32, -2 ** 31, 2 ** 31 - 1, "a region"))


def test_job_front_and_outputs_of_an_empty_job_list():
    f, l, m = hmm._jobs("who", [], [], ([], *hmm._MASK))
    assert _is_column(f, np.int64, 0) and _is_column(l, np.int64, 0) and _is_column(m, np.uint8, 0)
    f, l, m = hmm._jobs("who", [], 5, (300, *hmm._MASK))                 # (no job: nothing to refuse, as before)
    assert f.size == l.size == m.size == 0
    a, b, c = hmm._outputs(0, np.float64, (np.int64, 3), np.int64)
    assert a.shape == (0,) and b.shape == (0, 3) and c.shape == (0,)


def test_outputs():
    a, b, c = hmm._outputs(5, np.float64, (np.int64, 3), (np.float64, 0))
    assert (a.shape, a.dtype) == ((5,), np.float64) and (b.shape, b.dtype) == ((5, 3), np.int64) and c.shape == (5, 0)
    assert all(x.flags.c_contiguous and x.flags.writeable for x in (a, b, c))


def test_pointer_of_an_array_follows_its_dtype():
    for dtype, p in ((np.int8, N.p_int8), (np.uint8, N.p_uint8), (np.int32, N.p_int32), (np.int64, N.p_int64), (np.float64, N.p_double)):
        a = np.arange(3).astype(dtype)
        q = hmm._ptr(a)
        assert isinstance(q, p) and q[2] == 2
    assert hmm._ptr(None) is None
    with pytest.raises(KeyError):
        hmm._ptr(np.zeros(2, np.float32))


# ---- 2. joined and min_len -------------------------------------------------------------------------------------------------------
def _bare_list(n_chunks):
    em = hmm.EMList.__new__(hmm.EMList)
    em._L, em._h, em._borrowed = types.SimpleNamespace(hf_n_chunks=lambda h: n_chunks), 1, True
    return em


def test_joined_u8():
    em = _bare_list(4)
    jn = em._joined_u8("who", [0, 7, -1, 0.5])
    assert jn.dtype == np.uint8 and jn.tolist() == [0, 1, 1, 1] and jn.flags.c_contiguous
    assert em._joined_u8("who", np.array([[False, True], [True, False]])).tolist() == [0, 1, 1, 0]
    assert em._joined_u8("who", None) is None                            # no joins: the C ABI's NULL
    for bad in ([0, 1, 0], [0] * 5, []):
        with pytest.raises(ValueError, match="^who: joined must have one entry per chunk$"):
            em._joined_u8("who", bad)


def test_four_lengths():
    ml = hmm.EMList._four_lengths("who", (1, 2.0, np.int64(3), 4))
    assert ml.dtype == np.int32 and ml.tolist() == [1, 2, 3, 4] and ml.flags.c_contiguous
    assert hmm.EMList._four_lengths("who", np.arange(8)[::2]).tolist() == [0, 2, 4, 6]
    for bad in ((1, 2, 3), (1, 2, 3, 4, 5), 3, [[1, 2, 3, 4]]):
        with pytest.raises(ValueError, match="^who: min_len holds four window counts"):
            hmm.EMList._four_lengths("who", bad)


def test_minlen_fork_names_the_entry_point_it_calls():
    """hf_<base> or hf_<base>_joined, the joined pointer directly after min_len, and that name in the error."""
    calls = []

    def entry(name, rc):
        def f(*args):
            calls.append((name, args))
            return rc
        return f
    em = _bare_list(2)
    em._L = types.SimpleNamespace(hf_n_chunks=lambda h: 2, hf_x=entry("hf_x", 0), hf_x_joined=entry("hf_x_joined", 0), hf_y_joined=entry("hf_y_joined", -1),
                                  hf_last_error=lambda: b"scripted")
    ml, jn = em._four_lengths("who", (1, 2, 3, 4)), em._joined_u8("who", [0, 1])
    em._minlen("x", "head", ml, None, "t0", "t1")
    em._minlen("x", "head", ml, jn, "t0", "t1")
    (n0, a0), (n1, a1) = calls
    assert n0 == "hf_x" and a0[0] == 1 and a0[1] == "head" and a0[3:] == ("t0", "t1") and isinstance(a0[2], N.p_int32) and a0[2][3] == 4
    assert n1 == "hf_x_joined" and a1[:2] == (1, "head") and a1[4:] == ("t0", "t1") and isinstance(a1[3], N.p_uint8) and a1[3][1] == 1
    real, N._lib = N._lib, em._L                      # (HFError reads the library's last error text)
    try:
        with pytest.raises(N.HFError, match="^hf_y_joined failed with code -1: scripted$"):
            em._minlen("y", "head", ml, jn)
    finally:
        N._lib = real


# ---- 3. EM_*ForList --------------------------------------------------------------------------------------------------------------
class Recorder:
    """Answers every method name; records (name, positional, keyword) of each call."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def method(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            return (np.array([-3.5, 1.0]), -2.25) if name == "estep_minlen" else ("result of", name)
        return method


MODEL, ML, J, F, L, M, K, U, V, LAB = "model", "min_len", "joined", "first", "last", "mask", "k", "left", "right", "labels"
PROBS = (0.025, 0.5, 0.975)
# (wrapper, its arguments after the list, keyword arguments) -> (method, positional, keyword) exactly as forwarded
FORWARDS = [
    ("EM_runOneMinLengthIterationForList", (MODEL, ML), {}, ("estep_minlen", (MODEL, ML), {})),
    ("EM_runOneMinLengthIterationForList", (MODEL, ML, J), {}, ("estep_minlen", (MODEL, ML, J), {})),
    ("EM_runOneMinLengthIterationForList", (MODEL, ML), {"joined": J}, ("estep_minlen", (MODEL, ML, J), {})),
    ("EM_runViterbiForList", (MODEL,), {}, ("viterbi", (MODEL,), {})),
    ("EM_runMinLengthViterbiForList", (MODEL, ML), {}, ("viterbi_minlen", (MODEL, ML), {})),
    ("EM_runMinLengthViterbiForList", (MODEL, ML, J), {}, ("viterbi_minlen", (MODEL, ML, J), {})),
    ("EM_runMinLengthPosteriorForList", (MODEL, ML), {}, ("minlen_posterior", (MODEL, ML), {})),
    ("EM_runMinLengthPosteriorForList", (MODEL, ML), {"joined": J}, ("minlen_posterior", (MODEL, ML, J), {})),
    ("EM_getMaxExpectedGainLabelsForList", (ML,), {}, ("mea_labels", (ML, None, None), {})),
    ("EM_getMaxExpectedGainLabelsForList", (ML, J, "gain"), {}, ("mea_labels", (ML, J, "gain"), {})),
    ("EM_samplePathsForList", (MODEL, 3, 7), {}, ("sample_paths", (MODEL, 3, 7), {})),
    ("EM_sampleMinLengthPathsForList", (MODEL, ML, 3, 7), {}, ("sample_paths_minlen", (MODEL, ML, 3, 7), {})),
    ("EM_sampleMinLengthPathsForList", (MODEL, ML, 3, 7, J), {}, ("sample_paths_minlen", (MODEL, ML, 3, 7), {"joined": J})),
    ("EM_getIntervalLogProbsForList", (F, L, M), {}, ("interval_log_probs", (F, L, M), {})),
    ("EM_getCountMomentsForList", (F, L, M), {}, ("count_moments", (F, L, M, None, "windows"), {})),
    ("EM_getCountMomentsForList", (F, L, M, 1), {"unit": "bases"}, ("count_moments", (F, L, M, 1, "bases"), {})),
    ("EM_getRunMomentsForList", (F, L, M), {}, ("run_moments", (F, L, M, None), {})),
    ("EM_getRunMomentsForList", (F, L, M, J), {}, ("run_moments", (F, L, M, J), {})),
    ("EM_getLongRunLogProbsForList", (F, L, M, K), {}, ("long_run_log_probs", (F, L, M, K, None), {})),
    ("EM_getLongRunLogProbsForList", (F, L, M, K, J), {}, ("long_run_log_probs", (F, L, M, K, J), {})),
    ("EM_getRunLengthsForList", (F, L, M, 8), {}, ("run_lengths", (F, L, M, 8, None), {})),
    ("EM_getRunLengthsForList", (F, L, M, 8), {"joined": J}, ("run_lengths", (F, L, M, 8, J), {})),
    ("EM_getCountDistributionForList", (F, L, M, 5), {}, ("count_distribution", (F, L, M, 5), {})),
    ("EM_getPathEntropyForList", (F, L), {}, ("path_entropy", (F, L), {})),
    ("EM_getPathLogProbsForList", (F, L, LAB), {}, ("path_log_probs", (F, L, LAB), {})),
    ("EM_getEntropyProfileForList", (), {}, ("entropy_profile", (0, None), {})),
    ("EM_getEntropyProfileForList", (5, 9), {}, ("entropy_profile", (5, 9), {})),
    ("EM_getBreakpointsForList", (F, L, U, V), {}, ("breakpoints", (F, L, U, V, PROBS), {})),
    ("EM_getBreakpointsForList", (F, L, U, V, (0.5,)), {}, ("breakpoints", (F, L, U, V, (0.5,)), {})),
]
WRAPPERS = sorted({row[0] for row in FORWARDS})


def test_the_table_names_every_wrapper_that_looks_a_method_up():
    """Every EM_*ForList but the two that run a pass by launch / finish or run_sharded, and the batch's."""
    public = {n for n in dir(hmm) if n.startswith("EM_") and n.endswith("ForList")}
    assert public - set(WRAPPERS) == {"EM_runOneIterationForList", "EM_runForwardForList", "EM_runBatchForList"}
    assert len(WRAPPERS) == 17


@pytest.mark.parametrize("name", WRAPPERS)
def test_wrapper_refuses_a_list_without_the_method(name):
    args = next(row[1] for row in FORWARDS if row[0] == name)
    with pytest.raises(TypeError, match="^%s: object has no " % name):
        getattr(hmm, name)(object(), *args)


@pytest.mark.parametrize("name,args,kwargs,forwarded", FORWARDS, ids=["%s-%d" % (r[0], i) for i, r in enumerate(FORWARDS)])
def test_wrapper_forwards_exactly(name, args, kwargs, forwarded):
    rec = Recorder()
    model = types.SimpleNamespace()
    args = tuple(model if a is MODEL else a for a in args)
    method, pos, kw = forwarded
    got = getattr(hmm, name)(rec, *args, **kwargs)
    assert rec.calls == [(method, tuple(model if a is MODEL else a for a in pos), kw)]
    if method == "estep_minlen":
        assert got == -2.25 and model.loglikelihood == -3.5 and model.estimators.tolist() == [-3.5, 1.0]
    else:
        assert got == ("result of", method)


# ---- 4. runHMMFlagger ------------------------------------------------------------------------------------------------------------
LLS = [-100.25, -90.5, -85.125, -80.0625, -79.5]
LOG_Z = [-99.0, -88.25, -84.0, -79.0, -78.0]
ALPHA_STATS = np.arange(64, dtype=np.float64).reshape(2, 2, 4, 4)      # two regions: the trace holds their sum, 32 + 2 i


class ScriptedList:
    """A list without a fused iteration: every pass takes the next scripted log-likelihood; pass number `raise_at` (1-based) raises."""

    def __init__(self, stats_len, raise_at=None):
        self.calls, self.n, self.stats_len, self.raise_at = [], 0, stats_len, raise_at

    def _next(self):
        self.n += 1
        if self.n == self.raise_at:
            raise RuntimeError("scripted failure")
        return LLS[self.n - 1]

    def run_sharded(self, model, mode):
        self.calls.append(("run_sharded", mode))
        stats = np.zeros(self.stats_len)
        stats[0] = self._next()
        return stats


class FusedList(ScriptedList):
    def __init__(self, stats_len, converge_at, raise_at=None):
        super().__init__(stats_len, raise_at)
        self.converge_at = converge_at

    def em_iterate(self, model, *args, **kwargs):
        self.calls.append(("em_iterate", args, kwargs))
        model.loglikelihood = self._next()
        model.estimators = np.zeros(self.stats_len)
        return self.n >= self.converge_at


class MinLenList(ScriptedList):
    def __init__(self, stats_len, converge_at, raise_at=None):
        super().__init__(stats_len, raise_at)
        self.converge_at = converge_at

    def em_iterate_minlen(self, model, *args, **kwargs):
        self.calls.append(("em_iterate_minlen", args, kwargs))
        model.loglikelihood = self._next()
        self.last_log_z = LOG_Z[self.n - 1]
        return self.n >= self.converge_at


class AlphaList(ScriptedList):
    def set_alpha_stats(self, on=True):
        self.calls.append(("set_alpha_stats", on))

    def alpha_stats(self):
        self.calls.append(("alpha_stats",))
        return ALPHA_STATS.copy()


@pytest.fixture
def model():
    store = _tiny_store(np.random.default_rng(77), [7, 5], [20, 31])
    return hmm.createModel(N.HF_MODEL_GAUSSIAN, 2, store, np.zeros((4, 4)))


@pytest.fixture
def m_steps(monkeypatch):
    """HMM_estimateParameters / HMM_estimateAlpha scripted: they record their call and answer from `answers` (name -> list of flags)."""
    log, answers = [], {"HMM_estimateParameters": [], "HMM_estimateAlpha": []}
    for name in answers:
        def scripted(model, *args, _name=name):
            log.append((_name,) + tuple(a for a in args if not isinstance(a, np.ndarray)))
            return answers[_name].pop(0)
        monkeypatch.setattr(hmm, name, scripted)
    return log, answers


def _stats_len(model):
    return N.stats_len(model.numberOfRegions, model.maxNumberOfComps)


def _files(d):
    return sorted(os.listdir(d))


def _params(*points):
    return ["%s_%s.tsv" % (kind, p) for kind in ("emission", "transition") for p in points]


LL_HEADER = "#Iteration\tEffective_Iteration\tLoglikelihood\n"


def test_plain_loop_fused(model, m_steps, tmp_path):
    em = FusedList(_stats_len(model), converge_at=2)
    got = hmm.runHMMFlagger(em, model, 5, 0.01, str(tmp_path), True)
    assert got == [-100.25, -90.5, -85.125]
    assert em.calls == [("em_iterate", (True, 0.01), {}), ("em_iterate", (True, 0.01), {}), ("run_sharded", N.HF_MODE_FULL)]
    assert m_steps[0] == [] and model.estimators is not None and model.loglikelihood == -85.125
    assert _files(tmp_path) == sorted(["loglikelihood.tsv"] + _params("initial", "iteration_1", "iteration_2", "final"))
    assert (tmp_path / "loglikelihood.tsv").read_text() == LL_HEADER + "0\t0\t-100.2500\n1\t1\t-90.5000\n2\t2\t-85.1250\n"


def test_plain_loop_unfused(model, m_steps, tmp_path):
    log, answers = m_steps
    answers["HMM_estimateParameters"] = [False, False, True]
    em = ScriptedList(_stats_len(model))
    em.calls = log                                                      # one shared record of the order
    got = hmm.runHMMFlagger(em, model, 5, 0.01, str(tmp_path), True)
    assert got == [-100.25, -90.5, -85.125, -80.0625]
    assert log == [("run_sharded", N.HF_MODE_FULL), ("HMM_estimateParameters", 0.01)] * 3 + [("run_sharded", N.HF_MODE_FULL)]
    assert _files(tmp_path) == sorted(["loglikelihood.tsv"] + _params("initial", "iteration_1", "iteration_2", "iteration_3", "final"))
    assert (tmp_path / "loglikelihood.tsv").read_text() == LL_HEADER + "0\t0\t-100.2500\n1\t1\t-90.5000\n2\t2\t-85.1250\n3\t3\t-80.0625\n"


def test_plain_loop_stops_at_the_iteration_limit_and_writes_nothing_without_a_directory(model, m_steps, tmp_path):
    em = FusedList(_stats_len(model), converge_at=99)
    assert hmm.runHMMFlagger(em, model, 2, 0.01, None, True) == [-100.25, -90.5, -85.125]
    em = FusedList(_stats_len(model), converge_at=99)
    assert hmm.runHMMFlagger(em, model, 2, 0.01, str(tmp_path), True, is_writer=False) == [-100.25, -90.5, -85.125]
    assert _files(tmp_path) == []
    em = FusedList(_stats_len(model), converge_at=99)
    assert hmm.runHMMFlagger(em, model, 1, 0.01, str(tmp_path), False) == [-100.25, -90.5]
    assert _files(tmp_path) == sorted(["loglikelihood.tsv"] + _params("initial", "final"))
    assert (tmp_path / "loglikelihood.tsv").read_text() == LL_HEADER + "0\t0\t-100.2500\n1\t1\t-90.5000\n"


@pytest.mark.parametrize("joined", [None, "joins"])
def test_minimum_run_length_loop(model, m_steps, tmp_path, joined):
    em = MinLenList(_stats_len(model), converge_at=3)
    got = hmm.runHMMFlagger(em, model, 5, 0.01, str(tmp_path), True, constrainedMinLen=(1, 2, 3, 4), constrainedJoined=joined)
    assert got == [-100.25, -90.5, -85.125, -80.0625]
    step = ("em_iterate_minlen", ((1, 2, 3, 4), True, 0.01), {} if joined is None else {"joined": "joins"})
    assert em.calls == [step, step, step, ("run_sharded", N.HF_MODE_FULL)]
    assert m_steps[0] == [] and em.last_log_z == -84.0
    assert _files(tmp_path) == sorted(["loglikelihood.tsv", "length_constrained_em.tsv"] +
                                      _params("initial", "iteration_1", "iteration_2", "iteration_3", "final"))
    assert (tmp_path / "loglikelihood.tsv").read_text() == LL_HEADER + "0\t0\t-100.2500\n1\t1\t-90.5000\n2\t2\t-85.1250\n3\t3\t-80.0625\n"
    assert (tmp_path / "length_constrained_em.tsv").read_text() == (
        "#Iteration\tLog_Z_adm\tLog_Z\tLog_mass\n0\t-100.2500\t-99.0000\t-1.2500\n1\t-90.5000\t-88.2500\t-2.2500\n2\t-85.1250\t-84.0000\t-1.1250\n")


def test_alpha_fitting_loop(model, m_steps, tmp_path):
    log, answers = m_steps
    answers["HMM_estimateParameters"] = [False, True]                   # iterations 1 and 3
    answers["HMM_estimateAlpha"] = [True]                               # iteration 2
    em = AlphaList(_stats_len(model))
    em.calls = log                                                      # one shared record of the order
    got = hmm.runHMMFlagger(em, model, 9, 0.01, str(tmp_path), True, fitAlpha=True, fitAlphaEntries=((0, 0), (2, 2)), fitAlphaMax=0.5,
                            fitAlphaEvery=2)
    assert got == [-100.25, -90.5, -85.125, -80.0625]
    run = ("run_sharded", N.HF_MODE_FULL)
    assert log == [("set_alpha_stats", True), run, ("HMM_estimateParameters", 0.01), run, ("alpha_stats",), ("alpha_stats",),
                   ("HMM_estimateAlpha", 0.01, ((0, 0), (2, 2)), 0.0, 0.5), run, ("HMM_estimateParameters", 0.01), run,
                   ("set_alpha_stats", False)]
    assert _files(tmp_path) == sorted(["loglikelihood.tsv", "alpha_trace.tsv", "alpha_fitted.tsv"] +
                                      _params("initial", "iteration_1", "iteration_2", "iteration_3", "final"))
    assert (tmp_path / "loglikelihood.tsv").read_text() == LL_HEADER + "0\t0\t-100.2500\n1\t1\t-90.5000\n2\t2\t-85.1250\n3\t3\t-80.0625\n"
    assert (tmp_path / "alpha_trace.tsv").read_text() == (
        "1\t-90.5\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t"
        "32\t34\t36\t38\t40\t42\t44\t46\t48\t50\t52\t54\t56\t58\t60\t62\t64\t66\t68\t70\t72\t74\t76\t78\t80\t82\t84\t86\t88\t90\t92\t94\n")
    assert (tmp_path / "alpha_fitted.tsv").read_text() == "0\t0\t0\t0\n" * 4


def test_refusals_of_the_loop(model):
    em = FusedList(_stats_len(model), converge_at=1)
    with pytest.raises(ValueError, match="constrainedJoined needs constrainedMinLen"):
        hmm.runHMMFlagger(em, model, constrainedJoined=[0])
    with pytest.raises(ValueError, match="cannot be combined with fitAlpha"):
        hmm.runHMMFlagger(em, model, constrainedMinLen=(1, 1, 1, 1), fitAlpha=True)
    with pytest.raises(TypeError, match=r"^runHMMFlagger\(constrainedMinLen=...\): FusedList has no E-step under minimum run lengths$"):
        hmm.runHMMFlagger(em, model, constrainedMinLen=(1, 1, 1, 1))
    with pytest.raises(TypeError, match=r"^runHMMFlagger\(fitAlpha=True\): FusedList has no alpha statistics$"):
        hmm.runHMMFlagger(em, model, fitAlpha=True)
    alpha = AlphaList(_stats_len(model))
    with pytest.raises(ValueError, match="fitAlphaEvery must be at least 1"):
        hmm.runHMMFlagger(alpha, model, fitAlpha=True, fitAlphaEvery=0)
    with pytest.raises(ValueError, match="pre and state must be 0..3"):
        hmm.runHMMFlagger(alpha, model, fitAlpha=True, fitAlphaEntries=((4, 0),))
    assert em.calls == [] and alpha.calls == []                         # refused before anything ran


@pytest.mark.parametrize("variant", ["plain", "minlen", "alpha"])
def test_files_are_closed_when_a_pass_raises(model, m_steps, tmp_path, monkeypatch, variant):
    """The pass of iteration 2 raises: every file the loop opened is closed on the way out, and the alpha variant has switched the alpha
    statistics off again.  [plain] is the one intended difference to the three separate loops: that one left its file open."""
    opened = []
    real_open = builtins.open

    def recording_open(path, *args, **kwargs):
        f = real_open(path, *args, **kwargs)
        if str(path).startswith(str(tmp_path)):
            opened.append(f)
        return f
    monkeypatch.setattr(builtins, "open", recording_open)
    log, answers = m_steps
    answers["HMM_estimateParameters"] = [False]
    kwargs = {}
    if variant == "plain":
        em = FusedList(_stats_len(model), converge_at=99, raise_at=2)
    elif variant == "minlen":
        em, kwargs = MinLenList(_stats_len(model), converge_at=99, raise_at=2), {"constrainedMinLen": (1, 2, 3, 4)}
    else:
        em, kwargs = AlphaList(_stats_len(model), raise_at=2), {"fitAlpha": True}
    with pytest.raises(RuntimeError, match="scripted failure") as info:
        hmm.runHMMFlagger(em, model, 5, 0.01, str(tmp_path), True, **kwargs)
    assert info.traceback                                               # (the frames, and what they opened, are still alive here)
    assert len(opened) == (1 if variant == "plain" else 2)
    assert all(f.closed for f in opened)
    assert (tmp_path / "loglikelihood.tsv").read_text() == LL_HEADER + "0\t0\t-100.2500\n"
    if variant == "alpha":
        assert em.calls[0] == ("set_alpha_stats", True) and em.calls[-1] == ("set_alpha_stats", False)
