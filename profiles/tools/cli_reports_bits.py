#!/usr/bin/env python3
"""Every output file of hmm_flagger from two builds, byte for byte: the report writers of hf_cli_reports.h against the parent commit's.

    python profiles/tools/cli_reports_bits.py PARENT_CLI NEW_CLI OUT_ROOT [--record FILE]

PARENT_CLI and NEW_CLI are the two hmm_flagger binaries (each beside its own libhmmflagger_hip.so).  Every run of the matrix below is made
three times into OUT_ROOT/<input>/<run>/{parent, parent_again, new}: the parent twice, to show that every file is reproducible at all,
then the new build.  Every file of the three directories is compared (a file that one of them lacks counts as different); stderr is not
looked at.  One line per run and file goes to FILE (default profiles/cli_reports_ab.txt): `same`, or `DIFFERS` with the first differing
line, and `NOT REPRODUCIBLE` where the parent's two runs differ; then the counts.  Exit status 1 when anything differs.
Each run is a child process under `timeout -k 10 120`; the first one that does not exit with 0 ends the tool with that status, and
nothing is started after it.

Inputs: (a) synth.config(1, 0.5), the store of tests/test_cli_combined_gpu.py: one contig, one chunk.  (b) three contigs of 3, 2 and 1
chunks (800 + 575 + 225 windows of 4 kb, two annotation regions), the chunks reordered to A0 A1 B0 A2 B1 C0: contig A is split by a
chunk of B, so it has two chunk runs, and A2 is joined to nothing.
The region BED, built from the first run's files as the combined test builds it: a run of the final labels, a region of one window, an
unknown contig, a region of two runs; on (b) also a region across the boundary of A1 and A2 (two chunks that are not adjacent).
Runs (all with -W 4000 -n 4 -P): `probe` --uncertaintySamples alone; `all` every late option with --minimumLengths; `merged` the same
with --mergedChunks; `runlengths` --runLengths without --minimumLengths (no kept file); `mea_chunks` / `mea_contigs` --expectedAccuracy
with some late options behind it (their final labels are the decoder's); `viterbi_whole` --viterbi --enforceMinimumLengths
--wholeContigs with every late option (--expectedAccuracy does not combine with --viterbi)."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flagger_amd import synth

MIN = ["--minimumLengths", "12000,20000,28000"]


def store_b():
    st = synth.synthesize([3_200_000, 2_300_000, 900_000], 4000, 1_000_000, [20, 28], seed=4242, region_run_bases=(100_000, 600_000))
    assert list(st.chunk_ctg) == ["ctg0"] * 3 + ["ctg1"] * 2 + ["ctg2"]
    st = st.subset_chunks([0, 1, 3, 2, 4, 5])
    assert list(st.chunk_ctg) == ["ctg0", "ctg0", "ctg1", "ctg0", "ctg1", "ctg2"] and st.n_windows == 1600
    return st


def late(bed):
    return ["--uncertaintySamples", "4", "--runConfidence", "--regionProbs", bed, "--exactTotals", "--numBlocks", "--runLengths", "6", "--jointEntropy",
            "--runBoundaries", "--keptBlocks", "--totalsDistribution", "8", "--constrainedPosterior", "--admissibleSamples", "4"]


def matrix(bed):
    some = ["--runConfidence", "--regionProbs", bed, "--exactTotals", "--numBlocks", "--keptBlocks", "--jointEntropy"]
    return [("all", MIN + late(bed)), ("merged", MIN + late(bed) + ["--mergedChunks"]), ("runlengths", ["--runLengths", "6"]),
            ("mea_chunks", MIN + ["--expectedAccuracy", "chunks"] + some), ("mea_contigs", MIN + ["--expectedAccuracy", "contigs"] + some),
            ("viterbi_whole", MIN + ["--viterbi", "--enforceMinimumLengths", "--wholeContigs"] + late(bed))]


def run(cli, args, out):
    os.makedirs(out, exist_ok=True)
    with open(out + ".stderr", "w") as err:
        rc = subprocess.run(["timeout", "-k", "10", "120", cli] + args + ["-o", out], stdout=err, stderr=err).returncode
    if rc != 0:
        print("exit status %d: %s %s -o %s (stderr: %s.stderr)" % (rc, cli, " ".join(args), out, out), flush=True)
        sys.exit(rc)


def first_difference(a, b):
    la, lb = a.split(b"\n"), b.split(b"\n")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            return "line %d: %r | %r" % (i + 1, x[:120], y[:120])
    return "line %d: one file ends" % (min(len(la), len(lb)) + 1)


def rows(path):
    return [l.split("\t") for l in open(path).read().splitlines() if not l.startswith("#")]


def regions_bed(probe, path, extra):
    runs, w0 = rows(os.path.join(probe, "final_label_runs_support.bed")), rows(os.path.join(probe, "posterior_prediction_final.bed"))[0]
    r0 = runs[len(runs) // 2]
    regions = [(r0[0], r0[1], r0[2], "run"), (w0[0], w0[1], str(int(w0[1]) + 1), None), ("no_such_contig", "0", "100", "x"),
               (runs[0][0], runs[0][1], runs[1][2], "two")] + extra
    with open(path, "w") as f:
        f.write("#ctg\tstart\tend\n" + "".join("\t".join([c, s, e] + ([n] if n else [])) + "\n" for c, s, e, n in regions))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("out")
    ap.add_argument("--record", default=os.path.join(ROOT, "profiles", "cli_reports_ab.txt"))
    a = ap.parse_args()
    builds = (("parent", os.path.abspath(a.parent)), ("parent_again", os.path.abspath(a.parent)), ("new", os.path.abspath(a.new)))
    lines, files, unstable, differs, seen = [], 0, 0, 0, set()
    inputs = (("a", synth.config(1, 0.5), []), ("b", store_b(), [("ctg0", "1900000", "2100000", "split")]))
    for name, store, extra in inputs:
        root = os.path.join(os.path.abspath(a.out), name)
        os.makedirs(root, exist_ok=True)
        binp, bed = os.path.join(root, "in.bin"), os.path.join(root, "regions.bed")
        store.write_bin(binp)
        base = ["-i", binp, "-W", "4000", "-n", "4", "-P"]
        for rname, opts in [("probe", MIN + ["--uncertaintySamples", "4"])] + matrix(bed):
            for bname, cli in builds:
                run(cli, base + opts, os.path.join(root, rname, bname))
            if rname == "probe":
                regions_bed(os.path.join(root, rname, "parent"), bed, extra)
            d = {b: os.path.join(root, rname, b) for b, _ in builds}
            for f in sorted(set().union(*(os.listdir(p) for p in d.values()))):
                data = [open(os.path.join(p, f), "rb").read() if os.path.exists(os.path.join(p, f)) else None for p in d.values()]
                files += 1
                seen.add(f)
                verdict = "same"
                if data[0] != data[1]:
                    unstable += 1
                    verdict = "NOT REPRODUCIBLE (the parent twice: %s)" % ("a file is missing" if None in data[:2] else first_difference(data[0], data[1]))
                elif data[0] != data[2]:
                    differs += 1
                    verdict = "DIFFERS  %s" % ("a file is missing" if data[2] is None else first_difference(data[0], data[2]))
                lines.append("%s/%s/%s\t%d bytes\t%s" % (name, rname, f, len(data[0] or b""), verdict))
                print(lines[-1], flush=True)
    tail = "%d files of %d runs on 2 inputs (%d file names), %d NOT REPRODUCIBLE, %d DIFFERS" % (files, len(matrix("")) + 1, len(seen), unstable, differs)
    print(tail)
    with open(a.record, "w") as f:
        f.write("# profiles/tools/cli_reports_bits.py (its head comment has the inputs and the runs): the parent commit's hmm_flagger twice and\n"
                "# this build's once, every file of every run directory byte for byte, on one MI355X\n" + "\n".join(lines) + "\n" + tail + "\n"
                "file names: " + " ".join(sorted(seen)) + "\n")
    return 1 if unstable or differs else 0


if __name__ == "__main__":
    sys.exit(main())
