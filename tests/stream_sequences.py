"""Mixed call orders for tests/test_streams_gpu.py: a seeded generator in pure Python (random.Random only), so that what the committed
seeds cover can be checked without a GPU (tests/test_streams_cpu.py).

An operation is a string: a pass ("pass_a", "pass_b": full passes with two models; "forward": a forward-only pass), a switch ("flip": the
other statistics mode, scan contexts only; "alpha_on" / "alpha_off": hf_set_alpha_stats), a decoder with parameters other than the last
pass's ("viterbi", "sample", "viterbi_minlen"), or one of GETTERS.

There are two GENERATIONS of sequences.  What rnd.choice draws depends on the tuple it draws from, so the getters and decoders a seed
was chosen with are pinned to it: generation 1 is the ten getters and two decoders the first four seeds were committed with (their
lists never change: tests/test_streams_cpu.py holds a digest of them), generation 2 adds the breakpoint and long-run getters and the
minimum-length decoder.  The seeds of generation 2 were chosen on the CPU: with the tuples extended in the order below, random sets of
four seeds below 1000 were drawn until `coverage` met the conditions of test_streams_cpu.test_committed_seeds_cover_every_getter for all
thirteen getters and every operation occurred.  At lengths 40 and 48 no set did in 20 000 draws (thirteen getters need more getter
calls than ten); at length 64 such a search ends within a few hundred draws (random.Random(0).sample(range(1000), 4): the 328th), and
the set below is one that an earlier search of this kind met after 183."""
import random

GETTERS = ("labels", "posterior", "forward_backward", "interval_log_probs", "count_moments", "run_moments", "path_entropy",
           "path_log_probs", "entropy_profile", "alpha_stats", "breakpoints", "breakpoint_profile", "long_run_log_probs")
PASSES = ("pass_a", "pass_b", "forward")
DECODERS = ("viterbi", "sample", "viterbi_minlen")
SWITCHES = ("flip", "alpha_on", "alpha_off")
# generation -> (getters, decoders, length, seeds)
GENERATIONS = {
    1: (GETTERS[:10], DECODERS[:2], 40, (148, 97, 63, 0)),
    2: (GETTERS, DECODERS, 64, (812, 661, 955, 426)),
}
LENGTH = GENERATIONS[1][2]
SEEDS = GENERATIONS[1][3]


def sequence(seed: int, generation: int = 1, length=None):
    """`length` operations (default: the generation's) from `seed`, drawn from the generation's getters and decoders.  After a full pass
    or a decoder the next operation is a getter four times in five: those are the orders in which a getter builds its lazy state, or
    finds another model's tables on the device."""
    getters, decoders, gen_length, _ = GENERATIONS[generation]
    length = gen_length if length is None else length
    rnd = random.Random(seed)
    ops = ["alpha_on" if rnd.random() < 0.7 else "alpha_off", rnd.choice(("pass_a", "pass_b"))]
    while len(ops) < length:
        last = ops[-1]
        x = rnd.random()
        if last in ("pass_a", "pass_b") or last in decoders:
            kind = "getter" if x < 0.8 else rnd.choice(("pass", "decoder", "switch"))
        else:
            kind = "getter" if x < 0.5 else ("pass" if x < 0.68 else ("decoder" if x < 0.9 else "switch"))
        if kind == "getter":
            ops.append(rnd.choice(getters))
        elif kind == "pass":
            ops.append(rnd.choice(("pass_a", "pass_b", "pass_a", "pass_b", "forward")))
        elif kind == "decoder":
            ops.append(rnd.choice(decoders))
        else:
            ops.append(rnd.choice(("flip", "alpha_on", "alpha_on", "alpha_off")))
    return ops


def replay(ops):
    """(op, state) for every operation, `state` the bookkeeping a test needs before it runs the operation: the last pass ("pass_a",
    "pass_b", "forward" or None), the switches as they stood when that pass ran (`pass_alpha`, `pass_flipped`) and as they stand now
    (`alpha`, `flipped`), whether hf_get_alpha_stats answers (`alpha_answers`: the last pass was a full one with the statistics switched
    on, and they have not been switched off since — switching them off drops them), whether a getter has run since the last pass, and
    the operation before this one."""
    st = dict(last_pass=None, pass_alpha=False, pass_flipped=False, alpha=False, flipped=False, alpha_answers=False,
              getter_since_pass=False, prev=None)
    for op in ops:
        yield op, dict(st)
        if op in PASSES:
            st.update(last_pass=op, pass_alpha=st["alpha"], pass_flipped=st["flipped"], getter_since_pass=False,
                      alpha_answers=st["alpha"] and op != "forward")
        elif op == "flip":
            st["flipped"] = not st["flipped"]
        elif op == "alpha_on":
            st["alpha"] = True
        elif op == "alpha_off":
            st["alpha"] = False
            st["alpha_answers"] = False
        elif op in GETTERS:
            st["getter_since_pass"] = True
        st["prev"] = op


def coverage(seeds=None, generation: int = 1, length=None):
    """Per getter kind of the generation, over the sequences of `seeds` (default: the generation's): how often it runs after a full
    pass, as the first getter after a full pass, directly after a decoder (the last pass a full one), and after a forward-only pass.
    "alpha_stats" counts only where the statistics were switched on when the pass ran and have not been switched off since (elsewhere
    it answers HF_E_ARG)."""
    getters, decoders, _, gen_seeds = GENERATIONS[generation]
    cov = {g: dict(after_full=0, first_after_full=0, after_decoder=0, after_forward=0) for g in getters}
    for seed in gen_seeds if seeds is None else seeds:
        for op, st in replay(sequence(seed, generation, length)):
            if op not in getters:
                continue
            if st["last_pass"] == "forward":
                cov[op]["after_forward"] += 1
            if st["last_pass"] not in ("pass_a", "pass_b"):
                continue
            if op == "alpha_stats" and not st["alpha_answers"]:
                continue
            cov[op]["after_full"] += 1
            if not st["getter_since_pass"]:
                cov[op]["first_after_full"] += 1
            if st["prev"] in decoders:
                cov[op]["after_decoder"] += 1
    return cov
