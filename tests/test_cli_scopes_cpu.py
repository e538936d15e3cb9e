"""The command line's chunk-list rules (flagger_amd/csrc/hf_cli_scopes.h: which chunks are joined, what continues what, the groups, the
scopes "all" + every contig with their chunk runs and window ranges) on the host alone: `make scopes_check` compiles them with the host
compiler under the address and undefined-behaviour sanitizers into a stand-alone program that prints all of it for one chunk list.
Against the rules written out here from the header's comments."""
import os
import shutil
import subprocess

import pytest

import geometry_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flagger_amd", "csrc")


@pytest.fixture(scope="module")
def program():
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx) or not shutil.which("make"):
        pytest.skip("no host compiler")
    subprocess.run(["make", "-s", "-C", CSRC, "scopes_check", "CXX=" + cxx], check=True)
    return os.path.join(CSRC, "scopes_check")


def _merge(pairs):
    out = []
    for a, b in pairs:
        if out and out[-1][1] == a:
            out[-1] = (out[-1][0], b)
        else:
            out.append((a, b))
    return out


def _rules(off, names):
    """The statements of hf_cli_scopes.h and of chunk_continues (hf_jobs.h), each on its own."""
    C = len(names)
    has = [off[c + 1] > off[c] for c in range(C)]
    joined = [int(c > 0 and names[c] == names[c - 1]) for c in range(max(C, 1))]
    continues = [c > 0 and bool(joined[c]) and has[c] and has[c - 1] for c in range(C)]
    group_end = []
    for c0 in range(C):
        c1 = c0 + 1
        while c1 < C and continues[c1]:
            c1 += 1
        group_end.append(c1)
    order = list(dict.fromkeys(names))                      # first appearance
    scopes = [("all", [(0, C)] if C else [], [(off[0], off[C])] if C and off[C] > off[0] else [])]
    for n in order:
        at = [c for c in range(C) if names[c] == n]
        scopes.append((n, _merge((c, c + 1) for c in at), _merge((off[c], off[c + 1]) for c in at if has[c])))
    # ("all": the merged ranges of every chunk that has windows are the one range, as the header says)
    assert scopes[0][2] == _merge((off[c], off[c + 1]) for c in range(C) if has[c])
    return dict(joined=joined, names=[s[0] for s in scopes], scope_of_chunk=[1 + order.index(n) for n in names],
                runs=[s[1] for s in scopes], ranges=[s[2] for s in scopes], group_end=group_end)


def _grid_with_empty_chunks(own_names):
    """The grid store's chunk list (contigs by G.JOINED) with the chunks without windows of G.with_empty_chunks: in front, between the two
    chunks 5 and 6 of one contig, two in a row, behind.  own_names: each is a contig of its own, as there; else it carries the name of the
    chunk it stands in front of (behind the last: of the last), so that `joined` alone would let a run go on through it."""
    ctg, k = [], -1
    for c in range(len(G.OFF) - 1):
        k += c not in G.JOINED
        ctg.append("ctg%d" % k)
    off, names = [], []
    for c in range(len(G.OFF)):
        for _ in range(G.EMPTY_BEFORE.count(c)):
            off.append(G.OFF[c])
            names.append("empty_%d" % len(names) if own_names else ctg[min(c, len(ctg) - 1)])
        off.append(G.OFF[c])
        if c < len(ctg):
            names.append(ctg[c])
    assert len(names) == len(ctg) + len(G.EMPTY_BEFORE) == len(off) - 1 and off[0] == off[1] == 0 and off[-1] == off[-2] == G.N_WINDOWS
    return off, names


CASES = {
    "no-chunks": ([0], []),
    "one-chunk": ([0, 7], ["A"]),
    "AABB": ([0, 3, 8, 9, 20], ["A", "A", "B", "B"]),
    "ABA": ([0, 3, 8, 12], ["A", "B", "A"]),
    "prefix-names": ([0, 2, 4, 6, 8], ["ctg1", "ctg10", "ctg1", "ctg10"]),
    "only-chunk-empty": ([0, 5, 5, 9], ["A", "B", "C"]),
    "all-empty": ([0, 0, 0], ["A", "A"]),
    "grid-empty-own-contigs": _grid_with_empty_chunks(True),
    "grid-empty-same-contig": _grid_with_empty_chunks(False),
}


@pytest.mark.parametrize("case", list(CASES), ids=str)
def test_scopes_equal_the_stated_rules(program, tmp_path, case):
    off, names = CASES[case]
    path = tmp_path / "chunks.txt"
    path.write_text("%d\n%s\n%s\n" % (len(names), " ".join(map(str, off)), " ".join(names)))
    r = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]               # (a sanitizer report ends the program with an error)
    want = _rules(off, names)
    got = dict(runs={}, ranges={})
    for line in r.stdout.splitlines():
        key, *v = line.split()
        if key in ("runs", "ranges"):
            x = list(map(int, v[1:]))
            got[key][int(v[0])] = list(zip(x[0::2], x[1::2]))
        else:
            got[key] = v if key == "names" else list(map(int, v))
    for key in ("runs", "ranges"):
        got[key] = [got[key][i] for i in range(len(got["names"]))]
    assert got == want
    # what the cases are here for
    if case == "ABA":
        assert got["names"] == ["all", "A", "B"] and got["joined"] == [0, 0, 0] and got["runs"][1] == [(0, 1), (2, 3)] and got["ranges"][1] == [(0, 3), (8, 12)]
    if case == "prefix-names":
        assert got["names"] == ["all", "ctg1", "ctg10"] and got["scope_of_chunk"] == [1, 2, 1, 2]
    if case == "only-chunk-empty":
        assert got["names"][2] == "B" and got["runs"][2] == [(1, 2)] and got["ranges"][2] == [] and got["ranges"][0] == [(0, 9)]
    if case == "grid-empty-same-contig":
        # the chunk without windows between chunks 5 and 6 (list positions 6, 7, 8): joined on both sides, continued by neither, so the
        # group ends in front of it while the contig's window range goes on through it
        assert got["joined"][7:9] == [1, 1] and got["group_end"][6] == 7 and got["group_end"][7] == 8
        assert (G.OFF[3], G.OFF[8]) in got["ranges"][got["scope_of_chunk"][7]]
