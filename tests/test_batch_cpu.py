"""Many models on one track without a GPU: the --sweepAlpha option keeps every unique prefix of the reference's options, the binary
resolves it, and a bad list stops the command before the input is read or a device is touched.  Also the batch ABI's refusals that need
no device."""
import ctypes as C
import os
import subprocess

import pytest

from flagger_amd import _native as N
from test_cli_prefix_cpu import REFERENCE, ADDED, unique_prefixes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NOW = ADDED + ["viterbi", "sweepAlpha"]
needs_cli = pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")


def test_sweep_alpha_shadows_no_prefix_of_a_reference_option():
    ref = unique_prefixes(list(REFERENCE))
    now = dict(unique_prefixes(list(REFERENCE) + NOW))
    lost = [(p, n) for p, n in ref if now.get(p) != n]
    assert not lost, lost
    assert now["alpha"] == "alphaTsv"


@needs_cli
def test_the_binary_resolves_sweep(tmp_path):
    r = subprocess.run([CLI, "--sweep", str(tmp_path / "no_such_list")], capture_output=True, text=True)
    assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and "undefined option" not in r.stderr, r.stderr[-300:]
    r = subprocess.run([CLI, "--alpha", "x", "--sweep", "y"], capture_output=True, text=True)
    assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr, r.stderr[-300:]


def _run(tmp_path, extra):
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    args = [CLI, "-i", os.path.join(GOLDEN, "small_em.bin"), "-o", str(out)] + extra
    return subprocess.run(args, capture_output=True, text=True)


def _refused(r, needle):
    assert r.returncode != 0
    assert needle in r.stderr, r.stderr[-600:]
    # stopped at the list check: the input was not parsed and no device was brought up
    assert "Parsing/Creating coverage chunks" not in r.stderr, r.stderr[-600:]


@needs_cli
def test_empty_list(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("# nothing but a comment\n\n   \n")
    _refused(_run(tmp_path, ["--sweepAlpha", str(lst)]), "names no alpha TSV")


@needs_cli
def test_missing_list(tmp_path):
    _refused(_run(tmp_path, ["--sweepAlpha", str(tmp_path / "absent.txt")]), "cannot read the --sweepAlpha list")


@needs_cli
def test_missing_tsv(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text(os.path.join(GOLDEN, "alpha_hifi.tsv") + "\n" + str(tmp_path / "absent.tsv") + "\n")
    _refused(_run(tmp_path, ["--sweepAlpha", str(lst)]), "cannot read " + str(tmp_path / "absent.tsv"))


@needs_cli
def test_malformed_tsv(tmp_path):
    bad = tmp_path / "bad.tsv"
    bad.write_text("0\t0\t0\t0\n0\t1.5\t0\t0\n0\t0\t0\t0\n0\t0\t0\t0\n")
    lst = tmp_path / "list.txt"
    lst.write_text("# candidates\n" + os.path.join(GOLDEN, "alpha_hifi.tsv") + "\n\n" + str(bad) + "\n")
    _refused(_run(tmp_path, ["--sweepAlpha", str(lst)]), "not between 0 and 1")


@needs_cli
def test_together_with_alpha_tsv(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text(os.path.join(GOLDEN, "alpha_hifi.tsv") + "\n")
    _refused(_run(tmp_path, ["--sweepAlpha", str(lst), "--alphaTsv", os.path.join(GOLDEN, "alpha_hifi.tsv")]), "exclude each other")


def test_batch_abi_refuses_without_a_context():
    L = N.lib()
    assert L.hf_batch_capacity(None) == 0
    b = C.c_void_p()
    assert L.hf_batch_create(None, 4, C.byref(b)) == N.HF_E_ARG
    assert not b.value
    assert L.hf_batch_size(None) == 0
    L.hf_batch_destroy(None)
    st = (C.c_double * 4)()
    status = (C.c_int32 * 1)()
    assert L.hf_batch_finish(None, st, status, None) == N.HF_E_ARG
    assert L.hf_batch_get_labels(None, 0, None) == N.HF_E_ARG
    assert L.hf_batch_get_posterior(None, 0, 0, 0, None) == N.HF_E_ARG
    assert L.hf_batch_handoff(None, 0, None, None, 0) == N.HF_E_ARG
