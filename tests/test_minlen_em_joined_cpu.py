"""CPU checks of the ground of the E-step under minimum run lengths over groups of joined chunks: the numpy reference the GPU tests
rely on (tests/minlen_em_joined_ref.py) against 50-digit enumeration of a group's admissible paths, the boundary pair included, against
the joined posterior reference (tests/minlen_sum_joined_ref.py), and, with all four lengths 1, where J_t has rank 1 and a group
factorises into its chunks, against the per-chunk reference (tests/minlen_em_ref.py)."""
import numpy as np
import pytest

from flagger_amd import _native as N
import minlen_em_joined_ref as EJ
import minlen_em_ref as E
import minlen_joined_ref as JR
import minlen_ref
import minlen_sum_joined_ref as R
import sampling_ref
import viterbi_ref

ONES = (1, 1, 1, 1)
STAT_CASES = [c for c in minlen_ref.TINY_CASES if c[0] != N.HF_MODEL_NEGATIVE_BINOMIAL]   # (the statistics have no such path)


@pytest.mark.parametrize("case", minlen_ref.TINY_CASES)
def test_pair_marginals_against_group_enumeration(case):
    """Groups of 5, 6, 7 and 9 windows under (3, 2, 2, 2) and all ones: every pair marginal inside a group, the pair across a joined
    boundary included, within 1e-12 of the enumeration; zeros at the group's first window."""
    store, model, alpha, _ = minlen_ref.tiny_case(*case)
    A, end = sampling_ref.rows(store, model, alpha)
    off = np.asarray(store.chunk_off)
    weights = R.tiny_chunk_weights(*case)
    checked = bites = 0
    worst = 0.0
    for joined in JR.TINY_JOINS:
        bound = EJ.boundary_windows(off, joined)
        for ml in minlen_ref.TINY_MIN_LENS:
            xi, _, lza = EJ.xi_adm(A, end, off, joined, ml)
            per_chunk = E.xi_adm(A, end, off, ml)[0]
            _, gf, gl = JR.group_offsets(off, joined)
            for a, b in zip(gf.tolist(), gl.tolist()):
                if a == b:
                    assert np.array_equal(xi[off[a]:off[a + 1]], per_chunk[off[a]:off[a + 1]])    # a group of one chunk
                    continue
                pairs = EJ.enumerate_group_pairs([weights[c] for c in range(a, b + 1)], ml)
                want = np.array([[[float(v) for v in row] for row in mat] for mat in pairs])
                got = xi[off[a]:off[b + 1]]
                dev = float(np.max(np.abs(got - want)))
                worst = max(worst, dev)
                assert dev <= 1e-12, (joined, ml, a, dev)
                assert np.all(got[0] == 0.0)
                inner = [t for t in bound if off[a] < t < off[b + 1]]
                assert len(inner) == b - a
                for t in inner:                              # the boundary pair is a distribution, not zeros
                    assert abs(xi[t].sum() - 1.0) <= 1e-12
                inside = np.ones(got.shape[0], bool)
                inside[[0] + [int(t - off[a]) for t in inner]] = False
                bites += not np.allclose(got[inside], per_chunk[off[a]:off[b + 1]][inside], rtol=0, atol=1e-6)
                assert np.all(lza[a + 1:b + 1] == 0.0)
                checked += 1
    print("largest |xi - enumeration| %.3e; groups whose inner pairs the join changes by more than 1e-6: %d" % (worst, bites))
    assert checked == 8                                      # 2 patterns x 2 length sets x 2 groups of more than one chunk
    assert bites >= 1, "no join changes a pair marginal: the tests could not tell the two rules apart"


@pytest.mark.parametrize("case", minlen_ref.TINY_CASES)
@pytest.mark.parametrize("min_len", minlen_ref.TINY_MIN_LENS + [(3, 5, 1, 7), (2, 1, 1, 3)])
def test_marginal_identities(case, min_len):
    """sum_p xi_t[p][s] = post_joined[t][s] and sum_s xi_t[p][s] = post_joined[t-1][p], post_joined and log Z_adm those of
    minlen_sum_joined_ref, for every window but a group's first."""
    store, model, alpha, _ = minlen_ref.tiny_case(*case)
    A, end = sampling_ref.rows(store, model, alpha)
    logA, logend = viterbi_ref.tables(store, model, alpha)
    off = np.asarray(store.chunk_off)
    for joined in JR.TINY_JOINS:
        xi, post_own, lza_own = EJ.xi_adm(A, end, off, joined, min_len)
        post, _, lza, _ = R.posterior_tables(logA, logend, off, joined, min_len)
        assert np.all(np.abs(post_own - post) <= 1e-12)
        assert np.all(np.abs(lza_own - lza) <= 1e-12 * (1 + np.abs(lza)))
        goff = JR.group_offsets(off, joined)[0]
        first = np.zeros(store.n_windows, bool)
        first[goff[:-1]] = True
        t = np.flatnonzero(~first)
        assert np.all(np.abs(xi[t].sum(axis=1) - post[t]) <= 1e-12)
        assert np.all(np.abs(xi[t].sum(axis=2) - post[t - 1]) <= 1e-12)
        assert np.all(xi[first] == 0.0)


@pytest.mark.parametrize("case", STAT_CASES)
def test_all_ones_factorises_into_the_chunks(case):
    """With all lengths 1, J_t = end (x) first has rank 1: xi inside the chunks, the statistics and the sum of log Z_adm are the
    per-chunk reference's to 1e-12 relative, and at a joined chunk-first window xi[t] = post[t-1] (x) post[t]."""
    store, model, alpha, _ = minlen_ref.tiny_case(*case)
    off = np.asarray(store.chunk_off)
    pc = E.stats(store, model, alpha, ONES)
    for joined in JR.TINY_JOINS:
        jn = EJ.stats(store, model, alpha, joined, ONES)
        bound = jn["bound"]
        assert bound.size == int(np.sum(joined))
        inside = np.ones(store.n_windows, bool)
        inside[bound] = False
        assert np.all(np.abs(jn["xi"][inside] - pc["xi"][inside]) <= 1e-12 * pc["xi"][inside])
        assert np.all(np.abs(jn["post"] - pc["post"]) <= 1e-12 * pc["post"])
        for t in bound:
            want = pc["post"][t - 1][:, None] * pc["post"][t][None, :]
            assert np.all(np.abs(jn["xi"][t] - want) <= 1e-12 * want), t
        assert abs(jn["lza"].sum() - pc["lza"].sum()) <= 1e-12 * abs(pc["lza"].sum())
        assert np.array_equal(jn["lza"], jn["lz"])
        E.close_stats(jn["vec"], pc["vec"], pc["mag"], "all ones, joined against per chunk", rel=1e-12)
        _, gf, gl = JR.group_offsets(off, joined)
        for a, b in zip(gf.tolist(), gl.tolist()):          # a group's value in its first chunk's entry, 0.0 in the others
            assert abs(jn["lza"][a] - pc["lza"][a:b + 1].sum()) <= 1e-12 * abs(pc["lza"][a:b + 1].sum())
            assert np.all(jn["lza"][a + 1:b + 1] == 0.0) and np.all(jn["chunk"][a + 1:b + 1, 0] == 0.0)


@pytest.mark.parametrize("case", STAT_CASES)
def test_no_join_is_the_per_chunk_reference(case):
    store, model, alpha, _ = minlen_ref.tiny_case(*case)
    for ml in minlen_ref.TINY_MIN_LENS:
        pc = E.stats(store, model, alpha, ml)
        for joined in (None, np.zeros(store.n_chunks, bool)):
            jn = EJ.stats(store, model, alpha, joined, ml)
            assert jn["bound"].size == 0
            for k in ("vec", "chunk", "xi", "post", "lza", "lz"):
                assert np.array_equal(jn[k], pc[k]), k


def test_the_statistics_never_see_a_boundary_pair():
    """The pairs of the statistics are those of the original chunks: changing xi at the joined chunk-first windows (and at the window
    behind each, the reference's skipped first pair of a chunk) changes no element."""
    case = STAT_CASES[0]
    store, model, alpha, _ = minlen_ref.tiny_case(*case)
    joined = JR.TINY_JOINS[1]
    ml = (3, 2, 2, 2)
    jn = EJ.stats(store, model, alpha, joined, ml)
    xi = jn["xi"].copy()
    off = np.asarray(store.chunk_off)
    T = np.diff(off)
    for c in range(store.n_chunks):
        xi[off[c]:off[c] + min(2, T[c])] = 7.0
    vec, _, chunk = E.accumulate(store, model, alpha, xi, jn["lza"])
    assert np.array_equal(vec, jn["vec"]) and np.array_equal(chunk, jn["chunk"])
