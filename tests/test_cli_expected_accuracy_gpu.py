"""hmm_flagger --expectedAccuracy chunks|contigs and --expectedGains on the GPU: the final BED is hfio_write_final_bed of the library's
labels (hf_get_mea_labels through EMList.mea_labels on the same input and parameters), expected_accuracy.tsv parses and adds up, and
every other file of the run is byte-identical to the run without the option."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flagger_amd import _native as N
from flagger_amd import hmm, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flagger_amd", "csrc", "hmm_flagger")
MINLEN_ARGS = ["--minimumLengths", "20000,40000,20000"]    # with -W 4000: 5, 10, 1, 5 windows
WINDOWS = (5, 10, 1, 5)
BED_LENS = (20000, 40000, 0, 20000)
GAINS = np.array([[1.0, 0.0, 0.25, 0.0], [0.0, 1.5, -0.5, 0.25], [0.125, 0.0, 1.0, 0.0], [0.0, 0.5, 0.0, 2.0]])


def _cli(args, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([CLI] + args + ["-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r


def _bed_from_labels(binp, labels, path, lens, track="final_hmm_flagger"):
    L = N.lib()
    tab = L.hfio_load(str(binp).encode(), 0, 0)
    assert tab
    lens = (C.c_int32 * 4)(*lens)
    lab = np.ascontiguousarray(labels, np.int8)
    assert L.hfio_write_final_bed(tab, lab.ctypes.data_as(C.POINTER(C.c_int8)), str(path).encode(), track.encode(), lens) == 0
    L.hfio_destroy(tab)


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """A small input as test_cli_gpu synthesizes them (two contigs in three chunks and one, 1050 windows; at these lengths posterior
    argmax is inadmissible, the reference says), the fixed-parameter run without the option, and a context of the library whose last
    pass is the command line's final pass."""
    d = tmp_path_factory.mktemp("mea_cli")
    store = synth.synthesize([3_000_000, 1_200_000], 4000, 1_000_000, [20, 30], seed=8)
    binp = d / "in.bin"
    store.write_bin(str(binp))
    K = hmm.getBestNumberOfCollapsedComps(store)
    args = ["-i", str(binp), "-W", "4000", "-n", "0", "-P", "-p", str(K)] + MINLEN_ARGS
    _cli(args, d / "plain")
    st = synth.WindowStore.read_bin(str(binp))
    assert st.window_len == 4000
    model = hmm.createModel(hmm.MODEL_TRUNC_EXP_GAUSSIAN, K, st, np.zeros((4, 4)))
    em = hmm.EMList(st, model)
    em.launch(model, N.HF_MODE_FULL)
    em.finish()
    yield d, binp, args, st, em
    em.close()


def _table(path):
    rows = path.read_text().splitlines()
    assert rows[0] == "#scope\twindows\tgain_argmax\tgain_final_bed_rule\tgain_decoded\tfinal_bed_rule_supported"
    out = []
    for r in rows[1:]:
        f = r.split("\t")
        assert len(f) == 6 and f[5] in ("0", "1")
        out.append((f[0], int(f[1]), float(f[2]), float(f[3]), float(f[4]), int(f[5])))
    return out


@pytest.mark.parametrize("mode,gains", [("chunks", None), ("contigs", None), ("contigs", GAINS)], ids=["chunks", "contigs", "contigs-gains"])
def test_final_labels_table_and_untouched_files(base, mode, gains):
    d, binp, args, st, em = base
    out = d / (mode + ("_gains" if gains is not None else ""))
    extra = ["--expectedAccuracy", mode]
    if gains is not None:
        gp = d / "gains.tsv"
        gp.write_text("".join("\t".join(repr(float(v)) for v in row) + "\n" for row in gains))
        extra += ["--expectedGains", str(gp)]
    _cli(args + extra, out)
    # the final BED: the library's labels
    joined = hmm.joined_chunks(st) if mode == "contigs" else None
    labels, block, total = em.mea_labels(WINDOWS, joined, gains)
    _bed_from_labels(binp, labels, d / "ref.bed", BED_LENS)
    assert (out / "final_flagger_prediction.bed").read_text() == (d / "ref.bed").read_text()
    # expected_accuracy.tsv: one row per contig, then the track, which is their sum
    rows = _table(out / "expected_accuracy.tsv")
    ctgs = list(dict.fromkeys(st.chunk_ctg))
    assert [r[0] for r in rows] == [str(c) for c in ctgs] + ["track"]
    track = rows[-1]
    assert track[1] == sum(r[1] for r in rows[:-1]) == int(st.chunk_off[-1] - st.chunk_off[0])
    for col in (2, 3, 4):
        tot = 0.0
        for r in rows[:-1]:
            tot += r[col]
        assert track[col] == tot, col
    assert track[5] == min(r[5] for r in rows[:-1])
    assert track[4] <= track[2]                             # gain_decoded <= gain_argmax: the rule costs something on this input
    wmax = 1.0 if gains is None else np.abs(gains).max()
    for r in rows[:-1]:                                     # per contig to rounding (a contig the rule leaves alone sums the same terms in another order)
        assert r[4] <= r[2] + 1e-9 * r[1] * wmax, r
        assert r[3] <= r[2] + 1e-9 * r[1] * wmax, r
    assert abs(track[4] - total) <= 1e-9 * track[1] * wmax
    # every other file is the plain run's, -P's posterior BED included
    plain = d / "plain"
    names = sorted(os.listdir(plain))
    assert sorted(set(os.listdir(out)) - set(names)) == ["expected_accuracy.tsv"]
    assert "posterior_prediction_final.bed" in names and "loglikelihood.tsv" in names
    for n in names:
        if n == "final_flagger_prediction.bed" or n.startswith("prediction_summary_final"):
            continue
        assert (plain / n).read_bytes() == (out / n).read_bytes(), n


def test_the_rule_bites_on_this_input(base):
    """The lengths of the test change labels: what the option writes differs from the plain run's final BED."""
    d, binp, args, st, em = base
    labels, block, total = em.mea_labels(WINDOWS)
    free, _, bound = em.mea_labels((1, 1, 1, 1))
    assert not np.array_equal(labels, free) and total < bound
