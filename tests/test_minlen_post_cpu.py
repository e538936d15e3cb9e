"""CPU checks of the ground of the posterior under minimum run lengths: the numpy reference the GPU tests rely on
(tests/minlen_post_ref.py) against mpmath enumeration of all admissible paths, and the command line's --constrainedPosterior option
(prefixes, help text, refusals before the input is read)."""
import os
import subprocess

import numpy as np
import pytest

from test_cli_prefix_cpu import CLI, REFERENCE, unique_prefixes
from test_minlen_cpu import EARLIER as BEFORE_MINLEN
import minlen_post_ref
import minlen_ref
import viterbi_ref

# the additions of this build before this option, in the order they came (hf_cli.cpp long_options)
EARLIER = BEFORE_MINLEN + ["keptBlocks", "enforceMinimumLengths"]
OPTION = "constrainedPosterior"


@pytest.mark.parametrize("model_type,seed,hifi", minlen_ref.TINY_CASES)
def test_numpy_reference_against_path_enumeration(model_type, seed, hifi):
    store, model, alpha, enum = minlen_post_ref.tiny_case(model_type, seed, hifi)
    for min_len in minlen_ref.TINY_MIN_LENS:
        post, mass, lza, lz = minlen_post_ref.reference(store, model, alpha, min_len)
        below_one = minlen_post_ref.check_against_enumeration(store, enum, min_len, post, mass, lza)
        T = np.diff(store.chunk_off)
        assert np.all(np.abs(mass[T <= 2]) <= 1e-12 * (1 + np.abs(lz[T <= 2])))           # one or two windows: every path is admissible
        if min_len == (3, 2, 2, 2):
            assert below_one >= 1, "the rule removes no mass in any chunk of this case: the test would pass vacuously"
        else:
            assert below_one == 0


@pytest.mark.parametrize("model_type,seed,hifi", minlen_ref.TINY_CASES)
def test_all_ones_is_the_plain_forward_backward(model_type, seed, hifi):
    """Mass 1 in every chunk, and the posterior of the plain 4-state chain (written here on its own, in logs)."""
    store, model, alpha, _ = minlen_ref.tiny_case(model_type, seed, hifi)
    logA, logend = viterbi_ref.tables(store, model, alpha)
    post, mass, lza, lz = minlen_post_ref.reference(store, model, alpha, (1, 1, 1, 1))
    assert np.array_equal(lza, lz) and np.all(mass == 0.0)
    off = store.chunk_off
    with np.errstate(divide="ignore"):
        for c in range(store.n_chunks):
            A, T = logA[off[c]:off[c + 1]], int(off[c + 1] - off[c])
            f = np.empty((T, 4)); b = np.empty((T, 4))
            f[0] = A[0, 0]
            for t in range(1, T):
                f[t] = np.logaddexp.reduce(f[t - 1][:, None] + A[t], axis=0)
            b[T - 1] = logend[c]
            for t in range(T - 1, 0, -1):
                b[t - 1] = np.logaddexp.reduce(A[t] + b[t][None, :], axis=1)
            g = f + b
            want = np.exp(g - np.logaddexp.reduce(g, axis=1)[:, None])
            assert np.all(np.abs(post[off[c]:off[c + 1]] - want) <= 1e-12), c
            z = np.logaddexp.reduce(f[T - 1] + logend[c])
            assert abs(lz[c] - z) <= 1e-12 * (1 + abs(z))


def test_posterior_rows_sum_to_one_and_respect_impossible_states():
    """A chain whose Dup state cannot be left before two windows and never entered at window 3: a hand-checkable chunk."""
    A = np.full((4, 4, 4), 0.25)
    A[0] = 0.0
    A[0, 0, :] = 0.25
    A[3, :, 1] = 0.0                                       # nobody enters or stays in Dup at window 3
    with np.errstate(divide="ignore"):
        logA, logend = np.log(A), np.log(np.full((1, 4), 0.5))
    post, lza = minlen_post_ref.forward_backward(logA, logend, [0, 4], (1, 2, 1, 1))
    assert np.all(np.abs(post.sum(axis=1) - 1) <= 4e-16)
    assert post[3, 1] == 0.0
    # Dup at window 2 would be a run that ends at window 2 (window 3 is not Dup): it must have begun at window 0 or 1.  By hand: paths
    # with s_3 != Dup, weight 4^-4 / 2 each; admissible = all but those with an interior Dup run of one window, i.e. s_1 = Dup alone
    # (s_0, s_2 != Dup: 3 * 3 * 3 paths) or s_2 = Dup alone (s_1 != Dup, s_3 != Dup: 4 * 3 * 3 paths)
    n_all, n_bad = 4 * 4 * 4 * 3, 27 + 36
    assert abs(lza[0] - np.log((n_all - n_bad) * 0.25 ** 4 * 0.5)) <= 1e-14


def test_option_keeps_every_reference_prefix_and_every_earlier_one():
    ref = unique_prefixes(list(REFERENCE))
    now = dict(unique_prefixes(list(REFERENCE) + EARLIER + [OPTION]))
    lost = [(p, n) for p, n in ref if now.get(p) != n]
    assert not lost, lost
    before = dict(unique_prefixes(list(REFERENCE) + EARLIER))
    assert {p: n for p, n in before.items() if now.get(p) != n} == {}
    # --c, --co and --con were ambiguous among the reference's options already
    assert "con" not in before and now.get("cons") == OPTION and now.get("cont") == "contigsList" and now.get("conv") == "convergenceTol"


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("HF_LOOPBACK_RANKS", None)
    e.update(env or {})
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=e)


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_help_mentions_the_option():
    r = _run(["--help"])
    assert "--" + OPTION in r.stderr + r.stdout


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_the_binary_resolves_the_prefixes(tmp_path):
    for p in ("--cons", "--constrained", "--" + OPTION):
        r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), p])
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and "--constrainedPosterior needs --minimumLengths" in r.stderr, p
    for p, name in (("--cont", "x"), ("--conv", "0.5"), ("--col", "3")):
        r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), p, name])
        assert "ambiguous" not in r.stderr and "unrecognized" not in r.stderr and OPTION not in r.stderr, (p, r.stderr[-300:])
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--enforceMinimumLengths"])
    assert "--enforceMinimumLengths needs --viterbi" in r.stderr


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
@pytest.mark.parametrize("extra,env,needle", [
    ([], {}, "needs --minimumLengths"),
    (["--minimumLengths", "1,2,3", "--gpus", "2"], {}, "one GPU"),
    (["--minimumLengths", "1,2,3"], {"HF_LOOPBACK_RANKS": "2"}, "one GPU"),
    (["--minimumLengths", "1,2,3", "--sweepAlpha", "x"], {}, "one GPU"),
    (["-W", "1000", "--minimumLengths", "30000,20000,13001"], {}, "30,20,1,14"),
])
def test_refusals_come_before_the_input_is_read(tmp_path, extra, env, needle):
    """The input named here does not exist, so only the refusal can be the error."""
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--" + OPTION] + extra, env)
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert r.returncode != 0
    assert len(lines) == 1 and "--" + OPTION in lines[0] and needle in lines[0], r.stderr[-500:]


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_lengths_within_the_lane_budget_pass_the_option_checks(tmp_path):
    """30 + 20 + 1 + 13 = 64 windows: not refused; the run stops at the missing input."""
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--" + OPTION, "-W", "1000", "--minimumLengths", "30000,20000,13000"])
    assert r.returncode != 0 and OPTION not in r.stderr


@pytest.mark.parametrize("min_len", [(3, 5, 1, 7), (1, 1, 1, 1)])
def test_reference_on_chunk_ends_at_the_emission_floor(min_len):
    """Twelve windows at a chunk's first end, last end or both whose rows are the 1e-40 emission floor times a transition probability:
    the numpy reference against the header's recursions in 50 digits without any scaling."""
    store, model, alpha = minlen_post_ref.floored_case()
    logA, logend = viterbi_ref.tables(store, model, alpha)
    off = store.chunk_off
    k = minlen_post_ref.FLOORED
    floor = np.log(1e-40)
    assert logA[off[0] + 1:off[0] + k].max() <= floor and logA[off[2] - k:off[2]].max() <= floor        # the rows do sit on the floor
    assert logA[off[0], 0].max() <= floor and logA[off[0] + k:off[1]].max() > -60
    post, mass, lza, lz = minlen_post_ref.reference(store, model, alpha, min_len)
    assert np.all(np.isfinite(lza)) and np.all(lza < -1000)
    for c in range(store.n_chunks):
        want_lza, want_post = minlen_post_ref.mp_chunk(logA, logend, off, c, min_len)
        assert abs(lza[c] - float(want_lza)) <= 1e-12 * (1 + abs(float(want_lza))), (c, lza[c], want_lza)
        want = np.array([[float(v) for v in row] for row in want_post])
        assert np.all(np.abs(post[off[c]:off[c + 1]] - want) <= 1e-12), c
    if min_len == (1, 1, 1, 1):
        assert np.all(mass == 0.0)
    else:
        assert np.all(mass[:3] < -100)


@pytest.mark.skipif(not os.path.exists(CLI), reason="hmm_flagger not built")
def test_the_lane_budget_refusal_names_both_options_when_both_are_given(tmp_path):
    r = _run(["-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path), "--" + OPTION, "--viterbi", "--enforceMinimumLengths", "-W", "1000",
              "--minimumLengths", "30000,20000,13001"])
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert r.returncode != 0 and len(lines) == 1
    assert "--enforceMinimumLengths" in lines[0] and "--" + OPTION in lines[0] and "30,20,1,14" in lines[0]
