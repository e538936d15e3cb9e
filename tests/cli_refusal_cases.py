"""The refusals of the `hmm_flagger` command line, and which of two wins: the cases of tests/test_cli_refusals_cpu.py.

A TRIGGER is one way to provoke one refusal: options (name, value) and environment variables, on top of `-i <missing file> -o .`.  Every
option that check_options holds in its table appears in each of its roles: a bad argument, a missing --viterbi or --minimumLengths,
--gpus 2, --sweepAlpha x, HF_LOOPBACK_RANKS=2 (for the options up to --jointEntropy and for --fitAlpha that last one is NOT refused: the
command goes on to the loader, which does not find the input).  The cases are every trigger alone, and every pair of triggers that can
stand on one command line (no option or variable with two values); a pair carries the first trigger's options first.

tests/golden/cli_refusals.json holds exit status and stderr (timestamps replaced) of every case as a binary built from `parent_commit`
gave them.  A pair stores 0 or 1 where it equals that member's single case, and the text itself only where it equals neither.

    python tests/cli_refusal_cases.py --record BINARY [COMMIT]     write the golden file from BINARY
    python tests/cli_refusal_cases.py --check BINARY               replay every case against BINARY; exit status 1 on a difference
"""
import itertools
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_refusals.json")
BASE = [("-i", "no_such_input.cov"), ("-o", ".")]
MINLEN = ("--minimumLengths", "1,2,3")
OVER_BUDGET = [("-W", "1000"), ("--minimumLengths", "30000,20000,13001")]     # 30, 20, 1, 14 windows: 65 in sum, above 64


def _trigger(name, options=(), env=None, drop=()):
    return {"name": name, "options": list(options), "env": dict(env or {}), "drop": set(drop)}


def _one_gpu_roles(name, options):
    """The three ways to leave the single GPU, for an option that is otherwise well-formed."""
    return [_trigger(name + ":gpus2", options + [("--gpus", "2")]),
            _trigger(name + ":sweep", options + [("--sweepAlpha", "x")]),
            _trigger(name + ":loopback", options, {"HF_LOOPBACK_RANKS": "2"})]


def triggers():
    t = [_trigger("uncertaintySamples:bad", [("--uncertaintySamples", "x")]),
         _trigger("uncertaintySeed:bad", [("--uncertaintySeed", "-1")])]
    t += _one_gpu_roles("uncertaintySamples", [("--uncertaintySamples", "5")])
    t += _one_gpu_roles("runConfidence", [("--runConfidence", None)])
    t += _one_gpu_roles("regionProbs", [("--regionProbs", "no_such_regions.bed")])
    for o in ("runBoundaries", "exactTotals", "numBlocks", "jointEntropy"):
        t += _one_gpu_roles(o, [("--" + o, None)])
    t += [_trigger("fitAlphaEntries:bad", [("--fitAlpha", None), ("--fitAlphaEntries", "0,4")]),
          _trigger("fitAlphaMax:bad", [("--fitAlpha", None), ("--fitAlphaMax", "2")]),
          _trigger("fitAlphaEvery:bad", [("--fitAlpha", None), ("--fitAlphaEvery", "0")]),
          _trigger("fitAlpha:missing", [("--fitAlphaEvery", "3")]),
          _trigger("fitAlpha:accelerate", [("--fitAlpha", None), ("--accelerate", None)]),
          _trigger("fitAlpha:nb", [("--fitAlpha", None), ("-m", "negative_binomial")])]
    t += _one_gpu_roles("fitAlpha", [("--fitAlpha", None)])
    t += [_trigger("gpus:65", [("--gpus", "65")]),
          _trigger("gpus:with_loopback", [("--gpus", "1")], {"HF_LOOPBACK_RANKS": "2"})]
    t += [_trigger("enforceMinimumLengths:no_viterbi", [("--enforceMinimumLengths", None)])]
    t += _one_gpu_roles("enforceMinimumLengths", [("--enforceMinimumLengths", None), ("--viterbi", None)])
    for o, arg in (("keptBlocks", None), ("constrainedPosterior", None), ("admissibleSamples", "4")):
        t += [_trigger(o + ":no_minlen", [("--" + o, arg)])]
        t += _one_gpu_roles(o, [("--" + o, arg), MINLEN])
    t += [_trigger("admissibleSamples:bad", [("--admissibleSamples", "0"), MINLEN]),
          _trigger("input:missing", drop=["-i"]),
          _trigger("outputDir:missing", drop=["-o"]),
          _trigger("convergenceTol:bad", [("-t", "1.5")]),
          _trigger("preset:bad", [("-x", "sanger")]),
          _trigger("modelType:bad", [("-m", "poisson")]),
          _trigger("windowLen:0", [("-W", "0")]),
          _trigger("initialRandomDev:0.6", [("-D", "0.6")]),
          _trigger("lanes:expanded_chain", [("--enforceMinimumLengths", None), ("--viterbi", None)] + OVER_BUDGET),
          _trigger("lanes:keptBlocks", [("--keptBlocks", None), ("-W", "1000"), ("--minimumLengths", "59000,0,0")])]
    assert len({x["name"] for x in t}) == len(t)
    return t


def _compatible(a, b):
    va, vb = dict(a["options"]), dict(b["options"])
    return all(va[k] == vb[k] for k in va.keys() & vb.keys()) and all(a["env"][k] == b["env"][k] for k in a["env"].keys() & b["env"].keys())


def cases():
    """name -> (options, env, drop); the singles first, then the pairs as `first+second`."""
    t = triggers()
    out = {x["name"]: (x["options"], x["env"], x["drop"]) for x in t}
    for a, b in itertools.combinations(t, 2):
        if _compatible(a, b):
            options = a["options"] + [o for o in b["options"] if o not in a["options"]]
            out[a["name"] + "+" + b["name"]] = (options, {**a["env"], **b["env"]}, a["drop"] | b["drop"])
    return out


_STAMP = re.compile(r"\[\d{4}-\d\d-\d\d \d\d:\d\d:\d\d\]")


def run_case(binary, case, cwd):
    options, env, drop = case
    argv = [binary]
    for name, value in [o for o in BASE if o[0] not in drop] + options:
        argv += [name] if value is None else [name, value]
    full_env = {k: v for k, v in os.environ.items() if k != "HF_LOOPBACK_RANKS"}
    full_env.update(env)
    r = subprocess.run(argv, capture_output=True, text=True, cwd=cwd, env=full_env, timeout=120)
    return {"status": r.returncode, "stderr": _STAMP.sub("[TIME]", r.stderr)}


def run_all(binary):
    binary = os.path.abspath(binary)
    cs = cases()
    with tempfile.TemporaryDirectory() as cwd, ThreadPoolExecutor(max_workers=4) as pool:
        return dict(zip(cs, pool.map(lambda c: run_case(binary, c, cwd), cs.values())))


def record(binary, commit):
    got = run_all(binary)
    singles = {k: v for k, v in got.items() if "+" not in k}
    pairs = {}
    for k, v in got.items():
        if "+" in k:
            members = [singles[m] for m in k.split("+")]
            pairs[k] = members.index(v) if v in members else v
    with open(GOLDEN, "w") as f:
        json.dump({"parent_commit": commit, "singles": singles, "pairs": pairs}, f, indent=0, sort_keys=True)
        f.write("\n")
    return len(singles), len(pairs)


def expected():
    with open(GOLDEN) as f:
        g = json.load(f)
    out = dict(g["singles"])
    for k, v in g["pairs"].items():
        out[k] = g["singles"][k.split("+")[v]] if isinstance(v, int) else v
    return out


def check(binary):
    """The cases whose status or stderr differ from the golden file: [(name, expected, got)]; a case the file lacks counts."""
    want, got = expected(), run_all(binary)
    assert set(want) == set(got), sorted(set(want) ^ set(got))[:10]
    return [(k, want[k], got[k]) for k in want if want[k] != got[k]]


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--record":
        commit = sys.argv[3] if len(sys.argv) > 3 else subprocess.run(
            ["git", "rev-parse", "HEAD"], capture_output=True, text=True, check=True, cwd=os.path.dirname(GOLDEN)).stdout.strip()
        print("recorded %d singles and %d pairs" % record(sys.argv[2], commit))
    elif len(sys.argv) == 3 and sys.argv[1] == "--check":
        bad = check(sys.argv[2])
        for name, want, got in bad[:20]:
            print(name, "\n  expected", want, "\n  got     ", got)
        print("%d cases differ" % len(bad))
        sys.exit(1 if bad else 0)
    else:
        sys.exit(__doc__)
