"""The range getters' job cutter (flagger_amd/csrc/hf_jobs.h: parts per chunk, pieces on the global 512 grid, device batches under two
caps) on the host alone: `make jobcut_check` compiles it with the host compiler under the address and undefined-behaviour sanitizers
into a stand-alone program, which prints every job's parts, pieces and batch.  The jobs are the 903 of the grid store
(tests/geometry_cases.py), on its chunk list and on that list with chunks without windows in front, behind, two in a row and between
two chunks; the caps are the getters' own and tiny ones that split the call into many batches.  Against geometry_cases.pieces_of and
geometry_cases._batches, the statements of the two rules that tests/test_geometry_gpu.py checks the device results by."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import geometry_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flagger_amd", "csrc")


def _caps():
    text = open(os.path.join(CSRC, "hf_estep.hip")).read()
    caps = {}
    for name in ("HF_IV_BATCH_PIECES", "HF_IV_BATCH_PARTS", "HF_MO_BATCH_PIECES", "HF_MO_BATCH_PARTS"):
        m = re.search(r"#ifndef\s+%s\s+#define\s+%s\s+\(1\s*<<\s*(\d+)\)\s+#endif" % (name, name), text)      # (overridable)
        assert m, name
        caps[name] = 1 << int(m.group(1))
    return caps


@pytest.fixture(scope="module")
def program():
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx) or not shutil.which("make"):
        pytest.skip("no host compiler")
    subprocess.run(["make", "-s", "-C", CSRC, "jobcut_check", "CXX=" + cxx], check=True)
    return os.path.join(CSRC, "jobcut_check")


def _off_with_empty_chunks():
    """G.OFF with the chunks without windows of G.with_empty_chunks: in front, between two chunks, two in a row, behind."""
    off = []
    for c, o in enumerate(G.OFF):
        off += [o] * (1 + G.EMPTY_BEFORE.count(c))
    assert len(off) == len(G.OFF) + len(G.EMPTY_BEFORE) and off[0] == off[1] == 0 and off[-1] == off[-2] == G.N_WINDOWS
    assert sorted(set(off)) == G.OFF and max(off.count(o) for o in off) == 3
    return off


def _jobs():
    F, L = np.meshgrid(G.POINTS, G.POINTS, indexing="ij")
    keep = F <= L
    assert keep.sum() == 903
    return F[keep], L[keep]


@pytest.mark.parametrize("caps", ["interval", "moments", (7, 5), (1, 1 << 20), (1 << 20, 1)], ids=str)
@pytest.mark.parametrize("empty", [False, True], ids=["grid", "empty-chunks"])
def test_cutter_equals_the_stated_rules(program, tmp_path, empty, caps):
    if isinstance(caps, str):
        c = _caps()
        caps = (c["HF_IV_BATCH_PIECES"], c["HF_IV_BATCH_PARTS"]) if caps == "interval" else (c["HF_MO_BATCH_PIECES"], c["HF_MO_BATCH_PARTS"])
    off = np.asarray(_off_with_empty_chunks() if empty else G.OFF, np.int64)
    F, L = _jobs()
    path = tmp_path / "jobs.txt"
    path.write_text("%d %d\n%d\n%s\n%d\n%s\n" % (caps[0], caps[1], off.size, " ".join(map(str, off)), F.size,
                                               "\n".join("%d %d" % fl for fl in zip(F, L))))
    r = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]               # (a sanitizer report ends the program with an error)
    rows = np.array(r.stdout.split(), np.int64).reshape(-1, 7)
    job, part, piece = (rows[rows[:, 0] == k, 1:] for k in range(3))
    # 1. a part per chunk touched and the pieces of pieces_of, job by job and in the order asked
    parts_ref, pieces_ref = G.pieces_of(off, F, L)
    assert np.array_equal(job[:, 0], np.arange(F.size))
    assert np.array_equal(job[:, 2], parts_ref) and np.array_equal(job[:, 3], pieces_ref)
    assert np.array_equal(np.bincount(part[:, 0], minlength=F.size), parts_ref)
    assert np.array_equal(np.bincount(piece[:, 0], minlength=F.size), pieces_ref)
    # 2. the batches
    starts = np.flatnonzero(np.diff(job[:, 1], prepend=-1))
    assert np.array_equal(job[starts, 1], np.arange(starts.size))
    assert list(starts) == G._batches(parts_ref, pieces_ref, caps[0], caps[1])
    if caps[0] < 100:
        assert starts.size > 100
    # the parts of a job: consecutive chunk-local ranges from first to last, in chunks that have windows
    pj, pc, pa, pb, p0, p1 = part.T
    assert np.all(off[pc] <= pa) and np.all(pa <= pb) and np.all(pb < off[pc + 1])
    head = np.diff(pj, prepend=-1) != 0
    tail = np.diff(pj, append=-1) != 0
    assert np.array_equal(pa[head], F) and np.array_equal(pb[tail], L)
    assert np.all(pa[1:][~head[1:]] == pb[:-1][~head[1:]] + 1) and np.all(np.diff(pc)[~head[1:]] > 0)
    assert np.all((pa == off[pc]) | head) and np.all((pb == off[pc + 1] - 1) | tail)
    # 3. the pieces: inside the interior (a, b] of their part, inside one 512-block of the global grid, tiling the interior in order
    qj, qc, qt, qn, qg, qk = piece.T
    k_global = np.cumsum(np.ones(part.shape[0], np.int64)) - 1          # a part's row; qk and p0 / p1 count inside the batch
    batch_of_part = job[pj, 1]
    first_part_of_batch = np.flatnonzero(np.diff(batch_of_part, prepend=-1))
    row = first_part_of_batch[job[qj, 1]] + qk                          # the row of every piece's part
    assert np.array_equal(pj[row], qj) and np.array_equal(pc[row], qc)
    assert np.all(p0[row] <= qg) and np.all(qg < p1[row]) and np.array_equal(np.bincount(row, minlength=part.shape[0]), p1 - p0)
    qe = qt + qn - 1
    assert np.all(qn >= 1) and np.all(pa[row] < qt) and np.all(qe <= pb[row])
    assert np.all(qt // G.PIECE == qe // G.PIECE)
    has = p1 > p0
    assert np.array_equal(has, pb > pa)
    firsts = np.flatnonzero(np.diff(row, prepend=-1))
    lasts = np.flatnonzero(np.diff(row, append=-1))
    assert np.array_equal(row[firsts], k_global[has]) and np.array_equal(qt[firsts], pa[has] + 1) and np.array_equal(qe[lasts], pb[has])
    inner = np.diff(row) == 0
    assert np.all(qt[1:][inner] == qe[:-1][inner] + 1) and np.all(np.diff(qg)[inner] == 1)
    assert np.all(qt[1:][inner] % G.PIECE == 0)                          # every cut lies on the grid
