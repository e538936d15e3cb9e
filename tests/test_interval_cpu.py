"""CPU checks of the exact interval probabilities' ground: the numpy reference (tests/interval_ref.py) against brute-force path
enumeration, the C ABI entry point (declared, exported, bound), and the command line's --runConfidence / --regionProbs options
(prefixes, help text, checks made before the input is read)."""
import os
import re
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm
from test_cli_prefix_cpu import ADDED, CLI, REFERENCE, unique_prefixes
from test_sampling_cpu import _tiny
import interval_ref as IR
import sampling_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm_flagger_hip.h")
NEW = {"runConfidence": 0, "regionProbs": 1}
BUILD = {**REFERENCE, **{n: 1 for n in ADDED}, "viterbi": 0, "sweepAlpha": 1, "uncertaintySamples": 1, "uncertaintySeed": 1}


def _all_jobs(off):
    n = int(off[-1])
    first, last, mask = [], [], []
    for a in range(n):
        for b in range(a, n):
            for m in range(1, 16):
                first.append(a); last.append(b); mask.append(m)
    return np.array(first), np.array(last), np.array(mask)


@pytest.mark.parametrize("model_type,seed", [(N.HF_MODEL_TRUNC_EXP_GAUSSIAN, 0), (N.HF_MODEL_GAUSSIAN, 1),
                                             (N.HF_MODEL_NEGATIVE_BINOMIAL, 2)])
def test_reference_equals_path_enumeration(model_type, seed):
    """Every interval (chunk-spanning ones included) and every mask of a tiny store."""
    store, model, alpha = _tiny(seed, model_type, [4, 3, 1, 5])
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    first, last, mask = _all_jobs(off)
    ref = IR.log_probs(A, end, off, first, last, mask)
    bf = IR.brute_force(A, end, off, first, last, mask)
    assert np.array_equal(np.isneginf(ref), np.isneginf(bf))
    fin = np.isfinite(bf)
    assert np.allclose(np.exp(ref[fin]), np.exp(bf[fin]), rtol=1e-12, atol=0)
    assert np.all(ref[mask == 15] == 0.0) or np.allclose(ref[mask == 15], 0.0, atol=1e-13)
    assert np.all(ref <= 1e-12)


def test_reference_complement_and_chunk_split():
    """P(some window in k) = -expm1(log_p of the mask without k) lies in [0, 1]; a job equals the sum of its chunk-local parts."""
    store, model, alpha = _tiny(4, N.HF_MODEL_TRUNC_EXP_GAUSSIAN, [30, 20, 1, 12])
    A, end = S.rows(store, model, alpha)
    off = np.asarray(store.chunk_off, np.int64)
    n = int(off[-1])
    lp = IR.log_probs(A, end, off, [0] * 4, [n - 1] * 4, [15 & ~(1 << k) for k in range(4)])
    p_any = -np.expm1(lp)
    assert np.all((p_any >= 0) & (p_any <= 1))
    whole = IR.log_probs(A, end, off, [5], [n - 3], [6])[0]
    J, Cc, pa, pb, pm = IR.split(off, [5], [n - 3], [6])
    parts = IR.log_probs(A, end, off, pa, pb, pm)
    assert len(parts) == 4 and abs(whole - parts.sum()) <= 1e-12 * abs(whole)


def test_declared_exported_and_bound():
    """The getter is declared in the public header, exported by the library and bound in _native."""
    text = open(HEADER).read()
    assert re.search(r"int\s+hf_get_interval_log_probs\s*\(\s*hf_ctx\s*\*\s*ctx\s*,\s*int64_t\s+n\s*,", text)
    f = getattr(N.lib(), "hf_get_interval_log_probs")
    assert f.restype is not None and len(f.argtypes) == 6
    assert hasattr(hmm.EMList, "interval_log_probs") and hasattr(hmm, "EM_getIntervalLogProbsForList")


# ---- command line --------------------------------------------------------------------------------------------------------------
def test_new_options_move_no_unique_prefix():
    for before in (list(REFERENCE), list(BUILD)):
        now = dict(unique_prefixes(list(BUILD) + list(NEW)))
        lost = [(p, n) for p, n in unique_prefixes(before) if now.get(p) != n]
        assert not lost, lost


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_the_binary_resolves_every_shortest_prefix(tmp_path):
    names = {**BUILD, **NEW}
    shortest = {}
    for p, n in unique_prefixes(list(names)):
        if n not in shortest or len(p) < len(shortest[n]):
            shortest[n] = p
    for n, p in shortest.items():
        args = [CLI, "--" + p] + ([str(tmp_path / "x.bed")] if names[n] else []) + ["-o", str(tmp_path)]
        r = subprocess.run(args, capture_output=True, text=True)
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and "undefined option" not in r.stderr, (p, r.stderr[-300:])


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_help_names_both_options():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--runConfidence" in r.stderr + r.stdout and "--regionProbs" in r.stderr + r.stdout


def _run(tmp_path, extra):
    args = [CLI, "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path)] + extra
    r = subprocess.run(args, capture_output=True, text=True)
    return r, [l for l in r.stderr.splitlines() if l.strip()]


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--sweepAlpha", "list.txt"]])
@pytest.mark.parametrize("opt", [["--runConfidence"], ["--regionProbs", "REGIONS"]])
def test_refused_combinations(tmp_path, extra, opt):
    """Refused before the input is read: the input named here does not exist, so only the refusal can be the error."""
    (tmp_path / "regions.bed").write_text("ctg1\t0\t100\n")
    opt = [str(tmp_path / "regions.bed") if x == "REGIONS" else x for x in opt]
    r, lines = _run(tmp_path, opt + extra)
    assert r.returncode != 0
    assert len(lines) == 1 and ("--runConfidence" in lines[0] or "--regionProbs" in lines[0]), r.stderr[-500:]


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
@pytest.mark.parametrize("content,where", [(None, "cannot read"), ("ctg1\t0\n", "line 1"), ("# c\n\nctg1\t10\t5\n", "line 3"),
                                           ("track x\nctg1\ta\t5\n", "line 2"), ("ctg1\t-1\t5\n", "line 1"),
                                           ("browser y\nctg1\t0\t5\tg1\nctg2\t7\t7\n", "line 3")])
def test_region_file_checked_before_the_input(tmp_path, content, where):
    path = tmp_path / "regions.bed"
    if content is not None:
        path.write_text(content)
    r, lines = _run(tmp_path, ["--regionProbs", str(path)])
    assert r.returncode != 0
    assert len(lines) == 1 and "--regionProbs" in lines[0] and where in lines[0], r.stderr[-500:]


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_a_good_region_file_passes_to_the_input_check(tmp_path):
    path = tmp_path / "regions.bed"
    path.write_text("#ctg\tstart\tend\n\ntrack name=x\nctg1\t0\t100\tgeneA\textra\nctg2\t5\t6\n")
    r, lines = _run(tmp_path, ["--regionProbs", str(path), "--runConfidence"])
    assert r.returncode != 0
    assert "--regionProbs" not in r.stderr and "--runConfidence" not in r.stderr, r.stderr[-500:]
