"""CPU checks of the ground of the whole-contig posterior and sampler under minimum run lengths (hf_minlen_posterior_joined,
hf_sample_paths_minlen_joined): the numpy reference the GPU tests rely on (tests/minlen_sum_joined_ref.py) against 50-digit enumeration
of every joined group of the tiny stores (mass, log Z_adm, marginals, the draw rule's path probabilities), the draw code by a chi-square
test at the level of test_minlen_sample_cpu.py, the exact cases, and the command line's --mergedChunks option (prefixes, help text,
refusals before the input is read)."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from test_cli_prefix_cpu import CLI, REFERENCE, unique_prefixes
from test_minlen_joined_cpu import EARLIER as BEFORE_WHOLE, OPTION as WHOLE
import minlen_joined_ref as JR
import minlen_post_ref as PR
import minlen_ref
import minlen_sample_ref as SR
import minlen_sum_joined_ref as R
import sampling_ref as S
import viterbi_ref

EARLIER = BEFORE_WHOLE + [WHOLE]
OPTION = "mergedChunks"
ONES = (1, 1, 1, 1)


# ---- 1. the reference against enumeration ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", minlen_ref.TINY_CASES)
def test_numpy_reference_against_group_enumeration(case):
    """Groups of 5, 6, 7 and 9 windows under (3, 2, 2, 2) and all ones: mass, log Z_adm and post within 1e-12; the product of the
    conditional draw probabilities is weight / Z_adm for every admissible path and sums to 1 within 1e-12."""
    store, model, alpha, _ = minlen_ref.tiny_case(*case)
    logA, logend = viterbi_ref.tables(store, model, alpha)
    A, end = S.rows(store, model, alpha)
    off = store.chunk_off
    checked = bites = 0
    worst = 0.0
    for joined in JR.TINY_JOINS:
        for ml in minlen_ref.TINY_MIN_LENS:
            post, mass, lza, lz = R.posterior_tables(logA, logend, off, joined, ml)
            checked += R.check_against_enumeration(store, case, joined, ml, post, mass, lza)
            if ml == ONES:
                assert np.all(np.abs(mass) <= 1e-12 * (1 + np.abs(lz)))
            pc_mass = PR.forward_backward(logA, logend, off, ml)[1] - PR.forward_backward(logA, logend, off, ONES)[1]
            bound = JR.group_sums(pc_mass, off, joined)
            bites += int(np.sum(mass < bound - 1e-6))
            tab = R.sample_tables(A, end, off, joined, ml)
            for a, b, _, _, _, paths in R.tiny_groups(*case)[(joined, ml)]:
                if paths is None:
                    continue
                tot = 0.0
                for path, pr_ref in paths.items():
                    pr = SR.path_prob(tab, a, path)
                    worst = max(worst, abs(pr - float(pr_ref)))
                    assert abs(pr - float(pr_ref)) <= 1e-12, (joined, ml, a, path, pr, float(pr_ref))
                    tot += pr
                assert abs(tot - 1.0) <= 1e-12, (joined, ml, a, tot)
    print("largest |product of draw probabilities - weight / Z_adm| %.3e; groups whose mass the join lowers: %d" % (worst, bites))
    assert checked == 8                                      # 2 patterns x 2 length sets x 2 groups of more than one chunk
    assert bites >= 1, "no join lowers a mass: the tests could not tell the two rules apart"


def test_the_draw_code_samples_the_group_distribution():
    """20 000 reference samples of one group of 3 + 4 windows under (3, 2, 2, 2): every one admissible over the group, and Pearson's
    chi-square of the path frequencies against enumeration (paths of expected count below 5 pooled into one cell) is at most
    dof + 5 sqrt(2 dof), the level of test_minlen_sample_cpu.py.  Random flat rows with zeros among them, as there."""
    min_len = (3, 2, 2, 2)
    T, cut = 7, 3
    rng = np.random.default_rng(31415)
    A = rng.uniform(0.05, 1.0, (T, 4, 4)) * (rng.uniform(size=(T, 4, 4)) > 0.1)
    A[0, 1:] = 0.0
    A[cut, 1:] = 0.0                                         # chunk-first rows: first[s] in row 0
    end = rng.uniform(0.1, 1.0, (2, 4))
    off, joined = [0, cut, T], [0, 1]
    tab = R.sample_tables(A, end, off, joined, min_len)
    n_s = 20_000
    labels = SR.sample(tab, 4242, range(n_s))[0]
    assert all(minlen_ref._path_ok(row.tolist(), list(min_len)) for row in np.unique(labels, axis=0))
    per_chunk = SR.sample(SR.tables(A, end, off, min_len), 4242, range(2000))[0]
    assert not all(minlen_ref._path_ok(row.tolist(), list(min_len)) for row in np.unique(per_chunk, axis=0))   # the join does bite here
    code = lambda path: sum(int(s) * 4 ** (T - 1 - i) for i, s in enumerate(path))
    expect = np.zeros(4 ** T)
    for path in itertools.product(range(4), repeat=T):
        if minlen_ref._path_ok(path, list(min_len)):
            w = A[0, 0, path[0]] * end[0, path[cut - 1]] * A[cut, 0, path[cut]] * end[1, path[-1]]
            for t in range(1, T):
                if t != cut:
                    w *= A[t, path[t - 1], path[t]]
            expect[code(path)] = w
    expect *= n_s / expect.sum()
    counts = np.bincount((labels.astype(np.int64) * (4 ** np.arange(T - 1, -1, -1))).sum(axis=1), minlength=4 ** T).astype(np.float64)
    assert np.all(counts[expect == 0] == 0)
    big = expect >= 5
    cells_o = np.append(counts[big], counts[~big].sum())
    cells_e = np.append(expect[big], expect[~big].sum())
    keep = cells_e > 0
    chi2 = float(np.sum((cells_o[keep] - cells_e[keep]) ** 2 / cells_e[keep]))
    dof = int(keep.sum()) - 1
    print("chi-square %.2f over %d cells (dof %d, bound %.2f)" % (chi2, int(keep.sum()), dof, dof + 5 * np.sqrt(2 * dof)))
    assert dof >= 100
    assert chi2 <= dof + 5 * np.sqrt(2 * dof), (chi2, dof)


# ---- 2. exact cases ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", minlen_ref.TINY_CASES)
def test_exact_cases_of_the_reference(case):
    store, model, alpha, _ = minlen_ref.tiny_case(*case)
    logA, logend = viterbi_ref.tables(store, model, alpha)
    A, end = S.rows(store, model, alpha)
    off = store.chunk_off
    for ml in minlen_ref.TINY_MIN_LENS:
        post, lza = PR.forward_backward(logA, logend, off, ml)
        lz = PR.forward_backward(logA, logend, off, ONES)[1]
        smp = SR.sample(SR.tables(A, end, off, ml), 3, range(16))
        for none in (None, np.zeros(store.n_chunks, bool)):
            got = R.posterior_tables(logA, logend, off, none, ml)
            assert np.array_equal(got[0], post) and np.array_equal(got[2], lza) and np.array_equal(got[1], lza - lz)
            assert np.array_equal(R.group_chunk_offsets(off, none), np.asarray(off))
            for x, y in zip(SR.sample(R.sample_tables(A, end, off, none, ml), 3, range(16)), smp):
                assert np.array_equal(x, y)
        for joined in JR.TINY_JOINS:
            jp, jmass, jlza, jlz = R.posterior_tables(logA, logend, off, joined, ml)
            bound = JR.group_sums(lza - lz, off, joined)
            assert np.all(jmass <= bound + 1e-12 * (1 + np.abs(lz).sum())), (ml, joined, jmass - bound)
            zsum = JR.group_sums(lz, off, joined)
            assert np.all(np.abs(jlz - zsum) <= 1e-12 * (1 + np.abs(zsum))), (ml, joined, jlz - zsum)
            inner = sorted(set(range(store.n_chunks)) - set(JR.group_first_chunks(off, joined).tolist()))
            assert np.all(jmass[inner] == 0.0) and np.all(jlza[inner] == 0.0)
            assert np.all(np.abs(jp.sum(axis=1) - 1.0) <= 4 * np.finfo(float).eps)
            labels = SR.sample(R.sample_tables(A, end, off, joined, ml), 3, range(16))[0]
            assert all(R.admissible_over_groups(row, off, joined, ml) for row in labels)


def test_a_chunk_without_windows_ends_a_group():
    off = [0, 3, 3, 5, 9, 9]
    assert R.group_chunk_offsets(off, [0, 1, 1, 1, 1]).tolist() == [0, 3, 3, 9, 9, 9]
    assert R.group_chunk_offsets(off, None).tolist() == off
    assert R.group_chunk_offsets([0, 2, 4, 7, 9], [0, 1, 1, 0]).tolist() == [0, 7, 7, 7, 9]
    rng = np.random.default_rng(5)
    A = rng.uniform(0.05, 1.0, (9, 4, 4))
    for t in (0, 3, 5):
        A[t, 1:] = 0.0
    end = rng.uniform(0.1, 1.0, (5, 4))
    Aj, endj, goff = R.joined_rows(A, end, off, [0, 1, 1, 1, 1])
    assert np.array_equal(Aj[3], A[3])                       # chunk 2 follows a chunk without windows: its first row stays
    assert np.array_equal(Aj[5], end[2][:, None] * A[5, 0][None, :]) and np.array_equal(endj[2], end[3])
    with np.errstate(divide="ignore"):
        post, mass, lza, lz = R.posterior_tables(np.log(A), np.log(end), off, [0, 1, 1, 1, 1], (2, 2, 2, 2))
    assert mass[1] == 0.0 and mass[3] == 0.0 and mass[4] == 0.0 and lza[3] == 0.0


# ---- 3. the command line's option ---------------------------------------------------------------------------------------------------

def test_option_keeps_every_reference_prefix_and_every_earlier_one():
    ref = unique_prefixes(list(REFERENCE))
    now = dict(unique_prefixes(list(REFERENCE) + EARLIER + [OPTION]))
    lost = [(p, n) for p, n in ref if now.get(p) != n]
    assert not lost, lost
    before = dict(unique_prefixes(list(REFERENCE) + EARLIER))
    assert {p: n for p, n in before.items() if now.get(p) != n} == {}
    assert before.get("wh") == WHOLE and before.get("cons") == "constrainedPosterior" and before.get("ad") == "admissibleSamples"
    assert "m" not in before and "me" not in before          # --m was ambiguous already, nothing started with --me
    assert now.get("me") == OPTION


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("HF_LOOPBACK_RANKS", None)
    e.update(env or {})
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=e)


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_help_mentions_the_option():
    r = _run(["--help"])
    assert "--" + OPTION in r.stderr + r.stdout and "log_mass_per_chunk_rule" in r.stderr + r.stdout


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_the_binary_resolves_the_prefixes(tmp_path):
    for p in ("--me", "--merged", "--" + OPTION):
        r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), p])
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr, (p, r.stderr[-300:])
        assert "--mergedChunks needs --constrainedPosterior or --admissibleSamples" in r.stderr, (p, r.stderr[-300:])
    for p, name in (("--wh", "--wholeContigs"), ("--cons", "--constrainedPosterior"), ("--en", "--enforceMinimumLengths")):
        r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), p, "--gpus", "2"])
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and name in r.stderr, (p, r.stderr[-300:])


POST = ["--constrainedPosterior", "--minimumLengths", "1,2,3"]
SAMP = ["--admissibleSamples", "4", "--minimumLengths", "1,2,3"]


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
@pytest.mark.parametrize("extra,env,needle", [
    ([], {}, "needs --constrainedPosterior or --admissibleSamples"),
    (["--viterbi", "--enforceMinimumLengths", "--minimumLengths", "1,2,3"], {}, "needs --constrainedPosterior or --admissibleSamples"),
    (["--constrainedPosterior"], {}, "needs --minimumLengths"),
    (POST + ["--gpus", "2"], {}, "one GPU"),
    (POST, {"HF_LOOPBACK_RANKS": "2"}, "one GPU"),
    (POST + ["--sweepAlpha", "x"], {}, "one GPU"),
    (SAMP + ["--gpus", "2"], {}, "one GPU"),
    (SAMP, {"HF_LOOPBACK_RANKS": "2"}, "one GPU"),
    (SAMP + ["--sweepAlpha", "x"], {}, "one GPU"),
    (["--constrainedPosterior", "-W", "1000", "--minimumLengths", "30000,20000,13001"], {}, "30,20,1,14"),
])
def test_refusals_come_before_the_input_is_read(tmp_path, extra, env, needle):
    """The input named here does not exist, so only the refusal can be the error."""
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--" + OPTION] + extra, env)
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert r.returncode != 0
    assert len(lines) == 1 and "--" + OPTION in lines[0].replace(", --", " --") and needle in lines[0], r.stderr[-500:]


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
@pytest.mark.parametrize("extra", [POST, SAMP, POST + ["--admissibleSamples", "4"]])
def test_the_option_with_what_it_needs_passes_the_option_checks(tmp_path, extra):
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--" + OPTION] + extra)
    assert r.returncode != 0 and OPTION not in r.stderr


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_refusals_without_the_option_keep_their_text(tmp_path):
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--constrainedPosterior"])
    assert "Error: --constrainedPosterior needs --minimumLengths." in r.stderr
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path)] + SAMP + ["--gpus", "2"])
    assert "Error: --admissibleSamples runs on one GPU" in r.stderr
