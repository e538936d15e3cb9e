"""Mixed call orders for tests/test_streams_gpu.py: a seeded generator in pure Python (random.Random only), so that what the committed
seeds cover can be checked without a GPU (tests/test_streams_cpu.py).

An operation is a string: a pass ("pass_a", "pass_b": full passes with two models; "forward": a forward-only pass), a switch ("flip": the
other statistics mode, scan contexts only; "alpha_on" / "alpha_off": hf_set_alpha_stats), a decoder with parameters other than the last
pass's ("viterbi", "sample"), or one of GETTERS."""
import random

GETTERS = ("labels", "posterior", "forward_backward", "interval_log_probs", "count_moments", "run_moments", "path_entropy",
           "path_log_probs", "entropy_profile", "alpha_stats")
PASSES = ("pass_a", "pass_b", "forward")
DECODERS = ("viterbi", "sample")
SWITCHES = ("flip", "alpha_on", "alpha_off")
LENGTH = 40
SEEDS = (148, 97, 63, 0)


def sequence(seed: int, length: int = LENGTH):
    """`length` operations from `seed`.  After a full pass or a decoder the next operation is a getter four times in five: those are
    the orders in which a getter builds its lazy state, or finds another model's tables on the device."""
    rnd = random.Random(seed)
    ops = ["alpha_on" if rnd.random() < 0.7 else "alpha_off", rnd.choice(("pass_a", "pass_b"))]
    while len(ops) < length:
        last = ops[-1]
        x = rnd.random()
        if last in ("pass_a", "pass_b") or last in DECODERS:
            kind = "getter" if x < 0.8 else rnd.choice(("pass", "decoder", "switch"))
        else:
            kind = "getter" if x < 0.5 else ("pass" if x < 0.68 else ("decoder" if x < 0.9 else "switch"))
        if kind == "getter":
            ops.append(rnd.choice(GETTERS))
        elif kind == "pass":
            ops.append(rnd.choice(("pass_a", "pass_b", "pass_a", "pass_b", "forward")))
        elif kind == "decoder":
            ops.append(rnd.choice(DECODERS))
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


def coverage(seeds=SEEDS):
    """Per getter kind, over the sequences of `seeds`: how often it runs after a full pass, as the first getter after a full pass,
    directly after a decoder (the last pass a full one), and after a forward-only pass.  "alpha_stats" counts only where the statistics
    were switched on when the pass ran and have not been switched off since (elsewhere it answers HF_E_ARG)."""
    cov = {g: dict(after_full=0, first_after_full=0, after_decoder=0, after_forward=0) for g in GETTERS}
    for seed in seeds:
        for op, st in replay(sequence(seed)):
            if op not in GETTERS:
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
            if st["prev"] in DECODERS:
                cov[op]["after_decoder"] += 1
    return cov
