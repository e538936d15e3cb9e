"""Mixed call orders for tests/test_streams_gpu.py: a seeded generator in pure Python (random.Random only), so that what the committed
seeds cover can be checked without a GPU (tests/test_streams_cpu.py).

An operation is a string: a pass ("pass_a", "pass_b": full passes with two models; "forward": a forward-only pass), a switch ("flip": the
other statistics mode, scan contexts only; "alpha_on" / "alpha_off": hf_set_alpha_stats), a decoder with parameters other than the last
pass's ("viterbi", "sample", "viterbi_minlen", from generation 3 the three of MINLEN_DECODERS and in generation 4 the two of
JOINED_DECODERS), or one of GETTERS.

There are four GENERATIONS of sequences.  What rnd.choice draws depends on the tuple it draws from, so the getters and decoders a seed
was chosen with are pinned to it: generation 1 is the ten getters and two decoders the first four seeds were committed with (their
lists never change: tests/test_streams_cpu.py holds a digest of them), generation 2 adds the breakpoint and long-run getters and the
minimum-length decoder.  The seeds of generation 2 were chosen on the CPU: with the tuples extended in the order below, random sets of
four seeds below 1000 were drawn until `coverage` met the conditions of test_streams_cpu.test_committed_seeds_cover_every_getter for all
thirteen getters and every operation occurred.  At lengths 40 and 48 no set did in 20 000 draws (thirteen getters need more getter
calls than ten); at length 64 such a search ends within a few hundred draws (random.Random(0).sample(range(1000), 4): the 328th), and
the set below is one that an earlier search of this kind met after 183.

Generation 3 adds the three newest decoders (MINLEN_DECODERS) to the thirteen getters and three decoders of generation 2.  These carry
state from call to call: hf_viterbi_minlen_joined shares its decoder state with hf_viterbi_minlen, and the forward lanes of
hf_minlen_posterior and hf_sample_paths_minlen and the sampler's per-sample slab grow with a call's arguments and never shrink.  So
in generation 3 the arguments of a decoder call come from its ORDINAL, the number of earlier calls of the same decoder in the sequence
(`decoder_arguments`): the minimum lengths from LENS_CYCLE (16, 64, 4, 64 and 7 lanes: the buffer grows, then serves narrower calls),
the sample count of "sample_minlen" from SAMPLE_CYCLE (padded to 64, 128, 64, 64 words per window) and the joined vector of
"viterbi_minlen_joined" from JOIN_CYCLE (`join_vector`).  Its seeds were chosen on the CPU as those of generation 2 were:
random.Random(0).sample(range(1000), 4) was drawn until the set was disjoint from the seeds of generations 1 and 2 and met, at length
64, the getter conditions above and the conditions of test_streams_cpu.test_generation_3_covers_the_decoders (`decoder_coverage`:
every decoder twice, each new decoder after a forward-only pass and three times in one sequence, both orders on the shared state, for
each buffer one call that grows it and two that do not, three join kinds).  The 328th draw, (586, 294, 195, 107), meets the getter
conditions with the six decoders too, but each of the three buffers has only ONE call in its sequences that does not grow it; the
first draw that meets everything is the 3071st, the set below (the seventh disjoint set that meets the getter conditions).

Generation 4 adds the two whole-contig entry points of JOINED_DECODERS: hf_minlen_posterior_joined runs in hf_minlen_posterior's state
and hf_sample_paths_minlen_joined in hf_sample_paths_minlen's (STATES), as hf_viterbi_minlen_joined runs in hf_viterbi_minlen's.  A
buffer belongs to the STATE: the forward lanes and the per-sample slab grow with whichever of a state's two entry points asks for more
and then serve the narrower calls of both, and each of the two states takes a further buffer, "grp" (the groups of a call as a chunk
list), on its first joined call.  `decoder_arguments` therefore counts `grows` per state.  The new decoders take LENS_CYCLE by their
own ordinals, JOIN_CYCLE one entry ahead of "viterbi_minlen_joined" (ordinal + 1: all, random, zeros, null — a sequence then holds
joined calls of different entry points with different vectors), and "sample_minlen_joined" its sample count from
JOINED_SAMPLE_CYCLE (padded to 64, 192, 64, 64 words per window: three wavefront groups, then narrower calls in them).  The seeds
were chosen as those of generation 3 were: random.Random(0).sample(range(1000), 4) was drawn until the set was disjoint from the seeds
of generations 1 to 3 and met the getter conditions and those of test_streams_cpu.test_generation_4_covers_the_decoders
(`state_coverage`: all eight decoders twice; each new one after a forward-only pass, three times in one sequence and with three join
kinds; both orders of the two entry points of each of the three states; per buffer of a state one call that grows it and two that do
not; per buffer and entry point a call narrower than what the OTHER entry point left in the buffer).  At length 64 no set did in
20 000 draws; at length 80 the 1268th draw is the set below."""
import random

GETTERS = ("labels", "posterior", "forward_backward", "interval_log_probs", "count_moments", "run_moments", "path_entropy",
           "path_log_probs", "entropy_profile", "alpha_stats", "breakpoints", "breakpoint_profile", "long_run_log_probs")
PASSES = ("pass_a", "pass_b", "forward")
DECODERS = ("viterbi", "sample", "viterbi_minlen")
MINLEN_DECODERS = ("minlen_posterior", "sample_minlen", "viterbi_minlen_joined")
JOINED_DECODERS = ("minlen_posterior_joined", "sample_minlen_joined")      # a tuple of its own, appended: rnd.choice of generation 3 is pinned
SWITCHES = ("flip", "alpha_on", "alpha_off")
# generation -> (getters, decoders, length, seeds)
GENERATIONS = {
    1: (GETTERS[:10], DECODERS[:2], 40, (148, 97, 63, 0)),
    2: (GETTERS, DECODERS, 64, (812, 661, 955, 426)),
    3: (GETTERS, DECODERS + MINLEN_DECODERS, 64, (207, 692, 582, 391)),
    4: (GETTERS, DECODERS + MINLEN_DECODERS + JOINED_DECODERS, 80, (879, 717, 395, 670)),
}
# generation 3: the n-th call of a decoder in a sequence (from 0) takes entry n % len of these
LENS_CYCLE = ((3, 5, 1, 7), (16, 16, 16, 16), (1, 1, 1, 1), (61, 1, 1, 1), (2, 1, 1, 3))      # 16, 64, 4, 64 and 7 lanes
SAMPLE_CYCLE = (8, 65, 3, 64)                                  # samples per call of "sample_minlen"
JOIN_CYCLE = ("null", "all", "random", "zeros")                # the joined vector of "viterbi_minlen_joined" (join_vector)
JOIN_SEED = 20261020
JOINED_SAMPLE_CYCLE = (8, 130, 3, 64)                          # samples per call of "sample_minlen_joined"
JOIN_PHASE = {"viterbi_minlen_joined": 0, "minlen_posterior_joined": 1, "sample_minlen_joined": 1}      # decoder -> its start in JOIN_CYCLE
MINLEN_USERS = ("viterbi_minlen",) + MINLEN_DECODERS           # the decoders that take minimum lengths (to generation 3)
SHARED_STATE = ("viterbi_minlen", "viterbi_minlen_joined")     # two entry points, one decoder state
BUFFERS = {"minlen_posterior": ("fwd",), "sample_minlen": ("fwd", "samples")}      # decoder -> its buffers that grow and never shrink
# decoder -> the state of the context it runs in: two entry points each, the per-chunk one first
STATES = {"viterbi_minlen": "mlv", "viterbi_minlen_joined": "mlv", "minlen_posterior": "mlp", "minlen_posterior_joined": "mlp",
          "sample_minlen": "mls", "sample_minlen_joined": "mls"}
STATE_BUFFERS = {"mlp": ("fwd",), "mls": ("fwd", "samples")}   # state -> its buffers that grow with a call's arguments and never shrink
ALL_DECODERS = DECODERS + MINLEN_DECODERS + JOINED_DECODERS
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


def join_vector(kind, n_chunks):
    """The joined vector of JOIN_CYCLE's entry `kind` for a track of n_chunks chunks: None ("null": a NULL pointer) or a list of 0/1
    with [0] = 0.  "all": every chunk continues its predecessor, one group spans the track; "random": Bernoulli(1/2), seeded;
    "zeros": nothing is joined.  The vectors are synthetic (the ABI takes any vector)."""
    if kind == "null":
        return None
    if kind == "all":
        return [0] + [1] * (n_chunks - 1) if n_chunks else []
    if kind == "zeros":
        return [0] * n_chunks
    assert kind == "random"
    rnd = random.Random(JOIN_SEED)
    return [0 if c == 0 else int(rnd.random() < 0.5) for c in range(n_chunks)]


def _decoder_calls(ops, generation):
    """(op, args, grows, narrower) for every operation: decoder_arguments' three, and for a decoder the tuple of its state's buffers in
    which this call is narrower than what the state's OTHER entry point left there (that one grew the buffer last, to more than this
    call asks for)."""
    count, size, owner, cut = {}, {}, {}, set()
    for op in ops:
        if op not in ALL_DECODERS:
            yield op, None, (), ()
            continue
        n = count.get(op, 0)
        count[op] = n + 1
        args, grows, narrower = {"ordinal": n}, [], []
        if op in STATES:
            args["min_len"] = LENS_CYCLE[n % len(LENS_CYCLE) if generation >= 3 else 0]
        if op == "sample_minlen":
            args["n_samples"] = SAMPLE_CYCLE[n % len(SAMPLE_CYCLE)]
        if op == "sample_minlen_joined":
            args["n_samples"] = JOINED_SAMPLE_CYCLE[n % len(JOINED_SAMPLE_CYCLE)]
        if op in JOIN_PHASE:
            args["join"] = JOIN_CYCLE[(n + JOIN_PHASE[op]) % len(JOIN_CYCLE)]
        state = STATES.get(op)
        for b in STATE_BUFFERS.get(state, ()):
            want = sum(args["min_len"]) if b == "fwd" else args["n_samples"]
            if want > size.get((state, b), 0):
                size[state, b], owner[state, b] = want, op
                grows.append(b)
            elif want < size[state, b] and owner[state, b] != op:
                narrower.append(b)
        if op in JOINED_DECODERS and state not in cut:         # the state's first joined call takes "grp"
            cut.add(state)
            grows.append("grp")
        yield op, args, tuple(grows), tuple(narrower)


def decoder_arguments(ops, generation: int = 3):
    """(op, args, grows) for every operation.  For a decoder, `args` is a dict: "ordinal" (the number of earlier calls of the same decoder
    in `ops`), and what the decoder takes of "min_len", "n_samples" (sample_minlen: SAMPLE_CYCLE, sample_minlen_joined:
    JOINED_SAMPLE_CYCLE) and "join" (an entry of JOIN_CYCLE, from the decoder's JOIN_PHASE on); `grows` is the tuple of the buffers
    this call grows.  They belong to the decoder's STATE (STATE_BUFFERS), whichever of the state's two entry points is called: "fwd"
    when the lengths have more lanes than those of every earlier call in the state, "samples" when it asks for more samples than every
    earlier call in the state (the state's first call grows all of them: it allocates them), and "grp" in the state's first call of
    an entry point of JOINED_DECODERS.  Below generation 3 "viterbi_minlen" takes LENS_CYCLE[0] in every call.  For any other
    operation `args` is None and `grows` is ()."""
    for op, args, grows, _ in _decoder_calls(ops, generation):
        yield op, args, grows


def decoder_coverage(seeds=None, generation: int = 3):
    """What the decoder calls of the sequences of `seeds` (default: the generation's) cover, from the generator alone:
    "calls": decoder -> calls over all sequences; "after_forward": decoder -> calls while the last pass is a forward-only one;
    "most_in_one": decoder -> the most calls within one sequence; "minlen_then_joined" / "joined_then_minlen": how often, among the
    calls on the shared state in one sequence (other operations may lie between them), a "viterbi_minlen" is followed by a
    "viterbi_minlen_joined" and the reverse; "grows" / "reuses": (decoder, buffer) -> calls that grow the buffer / that do not;
    "joins": the entries of JOIN_CYCLE used."""
    decoders = GENERATIONS[generation][1]
    cov = dict(calls={d: 0 for d in decoders}, after_forward={d: 0 for d in decoders}, most_in_one={d: 0 for d in decoders},
               minlen_then_joined=0, joined_then_minlen=0, grows={(d, b): 0 for d in BUFFERS for b in BUFFERS[d]},
               reuses={(d, b): 0 for d in BUFFERS for b in BUFFERS[d]}, joins=set())
    for seed in GENERATIONS[generation][3] if seeds is None else seeds:
        ops = sequence(seed, generation)
        shared = None
        for (op, st), (_, args, grows) in zip(replay(ops), decoder_arguments(ops, generation)):
            if args is None:
                continue
            cov["calls"][op] += 1
            cov["after_forward"][op] += st["last_pass"] == "forward"
            cov["most_in_one"][op] = max(cov["most_in_one"][op], args["ordinal"] + 1)
            if op in SHARED_STATE:
                if shared is not None and shared != op:
                    cov["minlen_then_joined" if op == "viterbi_minlen_joined" else "joined_then_minlen"] += 1
                shared = op
            for b in BUFFERS.get(op, ()):
                cov["grows" if b in grows else "reuses"][(op, b)] += 1
            if "join" in args:
                cov["joins"].add(args["join"])
    return cov


def state_coverage(seeds=None, generation: int = 4):
    """What the decoder calls of the sequences of `seeds` (default: the generation's) cover, per STATE, from the generator alone:
    "calls", "after_forward", "most_in_one": as decoder_coverage's; "joins": decoder -> the entries of JOIN_CYCLE it is called with;
    "orders": (state, earlier entry point, later entry point) -> how often, among the calls in that state in one sequence (other
    operations may lie between them), the one is followed by the other; "grows" / "reuses": (state, buffer) -> calls in the state
    that grow the buffer / that do not; "narrower": (state, buffer, decoder) -> calls of the decoder with less than what the state's
    other entry point left in the buffer; "first_joined": state -> calls that take "grp"."""
    decoders = GENERATIONS[generation][1]
    pairs = {}
    for d in decoders:
        if d in STATES:
            pairs.setdefault(STATES[d], []).append(d)
    cov = dict(calls={d: 0 for d in decoders}, after_forward={d: 0 for d in decoders}, most_in_one={d: 0 for d in decoders},
               joins={d: set() for d in decoders if d in JOIN_PHASE},
               orders={(s, a, b): 0 for s, p in pairs.items() for a in p for b in p if a != b},
               grows={(s, b): 0 for s in STATE_BUFFERS for b in STATE_BUFFERS[s]}, reuses={(s, b): 0 for s in STATE_BUFFERS for b in STATE_BUFFERS[s]},
               narrower={(s, b, d): 0 for s in STATE_BUFFERS for b in STATE_BUFFERS[s] for d in pairs.get(s, ())},
               first_joined={s: 0 for s in STATE_BUFFERS})
    for seed in GENERATIONS[generation][3] if seeds is None else seeds:
        ops = sequence(seed, generation)
        last = {}
        for (op, st), (_, args, grows, narrower) in zip(replay(ops), _decoder_calls(ops, generation)):
            if args is None:
                continue
            cov["calls"][op] += 1
            cov["after_forward"][op] += st["last_pass"] == "forward"
            cov["most_in_one"][op] = max(cov["most_in_one"][op], args["ordinal"] + 1)
            if "join" in args:
                cov["joins"][op].add(args["join"])
            state = STATES.get(op)
            if state is None:
                continue
            if last.get(state, op) != op:
                cov["orders"][state, last[state], op] += 1
            last[state] = op
            for b in STATE_BUFFERS.get(state, ()):
                cov["grows" if b in grows else "reuses"][state, b] += 1
                cov["narrower"][state, b, op] += b in narrower
            if "grp" in grows:
                cov["first_joined"][state] += 1
    return cov
