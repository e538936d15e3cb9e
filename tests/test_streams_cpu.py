"""What the committed call orders of tests/test_streams_gpu.py cover (tests/stream_sequences.py), on the generator alone: every getter
kind runs at least twice after a full pass, at least once as the FIRST getter after a full pass (its lazy state is built then), at
least once directly after a decoder call with other parameters, and — for the refusals — at least once after a forward-only pass.
This holds for each generation of sequences by itself: for the ten getters of the first over its seeds, and for all thirteen getters
over the seeds of the second alone, over those of the third alone, and over those of the fourth alone.

Generation 3 adds the three decoders that carry state from call to call (hf_minlen_posterior, hf_sample_paths_minlen,
hf_viterbi_minlen_joined), with arguments that change from call to call (stream_sequences.decoder_arguments).  For its committed seeds
the generator alone shows: every one of the six decoders at least twice; each new decoder after a forward-only pass, and three times
within one sequence; hf_viterbi_minlen and hf_viterbi_minlen_joined, which share their state, in both orders; for each buffer that
grows and never shrinks a call that grows it and two that run in it narrower; three kinds of joined vector.

Generation 4 adds hf_minlen_posterior_joined and hf_sample_paths_minlen_joined, which run in the states of hf_minlen_posterior and
hf_sample_paths_minlen: buffers belong to the state, so `grows` is counted per state (test_decoder_arguments_per_state), and the
conditions on its seeds are per state too (test_generation_4_covers_the_decoders).  Generations 2 and 3 are pinned by digests, and
generation 3's arguments by a digest of decoder_arguments' output."""
import hashlib
import json

import stream_sequences as SQ

GENS = sorted(SQ.GENERATIONS)
# sha256 of json.dumps of the four lists of generation 1, computed at the commit before the second generation was added
GENERATION_1_DIGEST = "6ec2eb0113304e64909753fbb9f77679807ef5142128e2cd98f557c75c994049"
# ... of generation 2, computed at the commit before the third generation was added
GENERATION_2_DIGEST = "cfe3109ad41025538fc2df9a07ae10a96d7d46c5efa387711191474a632d5957"
# ... of generation 3, and of [[list(x) for x in decoder_arguments(ops, 3)] for its four lists], computed at the commit before the fourth
GENERATION_3_DIGEST = "bf34ea6f0e6b37fccca0177b0adb5d40285eb7e5b429bc29e413d700b8b09acf"
GENERATION_3_ARGUMENTS_DIGEST = "2b02656ee578cda898329139d7c62169d527abbb17e041671e482d4b3cf29697"


def test_generations():
    g1, d1, l1, s1 = SQ.GENERATIONS[1]
    g2, d2, l2, s2 = SQ.GENERATIONS[2]
    assert (SQ.SEEDS, SQ.LENGTH) == (s1, l1) == ((148, 97, 63, 0), 40)
    assert len(g1) == 10 and d1 == ("viterbi", "sample")
    assert g2 == SQ.GETTERS == g1 + ("breakpoints", "breakpoint_profile", "long_run_log_probs")
    assert d2 == SQ.DECODERS == ("viterbi", "sample", "viterbi_minlen")
    assert len(s2) == 4 and l2 <= 64 and not set(s1) & set(s2)


def test_the_first_generation_is_what_it_was():
    seqs = [SQ.sequence(s) for s in SQ.SEEDS]
    assert seqs == [SQ.sequence(s, 1) for s in SQ.GENERATIONS[1][3]]
    assert hashlib.sha256(json.dumps(seqs).encode()).hexdigest() == GENERATION_1_DIGEST


def test_the_second_generation_is_what_it_was():
    seqs = [SQ.sequence(s, 2) for s in SQ.GENERATIONS[2][3]]
    assert hashlib.sha256(json.dumps(seqs).encode()).hexdigest() == GENERATION_2_DIGEST
    for ops in seqs:                                       # below generation 3 the minimum-length decoder keeps its one set of lengths
        assert all(args["min_len"] == (3, 5, 1, 7) and grows == () for op, args, grows in SQ.decoder_arguments(ops, 2) if op == "viterbi_minlen")


def test_generation_3():
    g3, d3, l3, s3 = SQ.GENERATIONS[3]
    assert g3 == SQ.GETTERS and d3 == SQ.DECODERS + SQ.MINLEN_DECODERS and l3 == 64 and len(s3) == 4
    assert SQ.MINLEN_DECODERS == ("minlen_posterior", "sample_minlen", "viterbi_minlen_joined")
    assert not set(s3) & (set(SQ.GENERATIONS[1][3]) | set(SQ.GENERATIONS[2][3]))
    assert SQ.LENS_CYCLE == ((3, 5, 1, 7), (16, 16, 16, 16), (1, 1, 1, 1), (61, 1, 1, 1), (2, 1, 1, 3))
    assert [sum(m) for m in SQ.LENS_CYCLE] == [16, 64, 4, 64, 7] and all(min(m) >= 1 for m in SQ.LENS_CYCLE)
    assert SQ.SAMPLE_CYCLE == (8, 65, 3, 64) and [-(-k // 64) * 64 for k in SQ.SAMPLE_CYCLE] == [64, 128, 64, 64]
    assert SQ.JOIN_CYCLE == ("null", "all", "random", "zeros")


def test_the_third_generation_is_what_it_was():
    seqs = [SQ.sequence(s, 3) for s in SQ.GENERATIONS[3][3]]
    assert hashlib.sha256(json.dumps(seqs).encode()).hexdigest() == GENERATION_3_DIGEST
    args = [[list(x) for x in SQ.decoder_arguments(ops, 3)] for ops in seqs]
    assert hashlib.sha256(json.dumps(args).encode()).hexdigest() == GENERATION_3_ARGUMENTS_DIGEST
    assert args == [[list(x) for x in SQ.decoder_arguments(ops)] for ops in seqs]


def test_generation_4():
    g4, d4, l4, s4 = SQ.GENERATIONS[4]
    assert g4 == SQ.GETTERS and len(g4) == 13 and l4 in (64, 80, 96) and len(s4) == 4
    assert d4 == SQ.DECODERS + SQ.MINLEN_DECODERS + SQ.JOINED_DECODERS == SQ.ALL_DECODERS and len(d4) == 8
    assert SQ.JOINED_DECODERS == ("minlen_posterior_joined", "sample_minlen_joined")
    assert not set(s4) & (set(SQ.GENERATIONS[1][3]) | set(SQ.GENERATIONS[2][3]) | set(SQ.GENERATIONS[3][3]))
    assert SQ.JOINED_SAMPLE_CYCLE == (8, 130, 3, 64) and [-(-k // 64) * 64 for k in SQ.JOINED_SAMPLE_CYCLE] == [64, 192, 64, 64]
    assert SQ.JOIN_PHASE["viterbi_minlen_joined"] == 0 and all(SQ.JOIN_PHASE[d] % len(SQ.JOIN_CYCLE) != 0 for d in SQ.JOINED_DECODERS)
    assert sorted(SQ.STATES.values()) == ["mlp"] * 2 + ["mls"] * 2 + ["mlv"] * 2 and set(SQ.STATES) == set(d4) - {"viterbi", "sample"}
    assert (SQ.STATES["minlen_posterior_joined"], SQ.STATES["sample_minlen_joined"]) == (SQ.STATES["minlen_posterior"], SQ.STATES["sample_minlen"])
    assert SQ.STATE_BUFFERS == {SQ.STATES[d]: b for d, b in SQ.BUFFERS.items()}


def test_join_vectors():
    assert SQ.join_vector("null", 10) is None
    assert SQ.join_vector("all", 10) == [0] + [1] * 9 and SQ.join_vector("zeros", 10) == [0] * 10
    r = SQ.join_vector("random", 10)
    assert r == SQ.join_vector("random", 10) and len(r) == 10 and r[0] == 0 and set(r) == {0, 1}
    assert r not in (SQ.join_vector("all", 10), SQ.join_vector("zeros", 10))
    for kind in SQ.JOIN_CYCLE[1:]:
        assert SQ.join_vector(kind, 1) == [0] and SQ.join_vector(kind, 0) == []


def test_decoder_arguments():
    ops = ["alpha_on", "pass_a"] + ["sample_minlen"] * 5 + ["labels"] + ["minlen_posterior"] * 6 + ["viterbi_minlen_joined"] * 5 + \
        ["viterbi", "viterbi_minlen", "viterbi_minlen", "sample"]
    out = list(SQ.decoder_arguments(ops))
    assert [o for o, _, _ in out] == ops and out[0][1:] == (None, ()) and out[7][1:] == (None, ())
    smp, post, join = out[2:7], out[8:14], out[14:19]
    assert [a["ordinal"] for _, a, _ in smp] == [0, 1, 2, 3, 4]
    assert [a["n_samples"] for _, a, _ in smp] == [8, 65, 3, 64, 8] and [a["min_len"] for _, a, _ in smp] == list(SQ.LENS_CYCLE)
    assert [g for _, _, g in smp] == [("fwd", "samples"), ("fwd", "samples"), (), (), ()]
    assert [a["min_len"] for _, a, _ in post] == list(SQ.LENS_CYCLE) + [SQ.LENS_CYCLE[0]] and all("n_samples" not in a and "join" not in a for _, a, _ in post)
    assert [g for _, _, g in post] == [("fwd",), ("fwd",), (), (), (), ()]
    assert [a["join"] for _, a, _ in join] == ["null", "all", "random", "zeros", "null"] and all(g == () for _, _, g in join)
    assert out[19][1] == {"ordinal": 0} and out[22][1] == {"ordinal": 0}
    assert [a["min_len"] for _, a, _ in out[20:22]] == list(SQ.LENS_CYCLE[:2])             # a count of its own per decoder
    assert [a["min_len"] for _, a, _ in list(SQ.decoder_arguments(ops, 2))[20:22]] == [SQ.LENS_CYCLE[0]] * 2
    # 64 lanes after 16 grow the lanes; a narrower call after a wider one does not, whatever lay between
    ops = ["minlen_posterior", "sample_minlen", "minlen_posterior", "forward", "minlen_posterior", "sample_minlen"]
    assert [g for _, _, g in SQ.decoder_arguments(ops)] == [("fwd",), ("fwd", "samples"), ("fwd",), (), (), ("fwd", "samples")]


def test_decoder_arguments_per_state():
    """The buffers belong to the state: a joined call after a wider per-chunk call grows nothing, and the reverse; "grp" is taken in the
    state's first joined call alone."""
    ops = ["minlen_posterior", "minlen_posterior_joined", "minlen_posterior_joined", "minlen_posterior", "minlen_posterior_joined",
           "labels", "sample_minlen_joined", "sample_minlen_joined", "sample_minlen", "sample_minlen", "sample_minlen_joined", "sample_minlen",
           "viterbi_minlen_joined", "sample_minlen_joined"]
    out = list(SQ._decoder_calls(ops, 4))
    assert [(o, a, g) for o, a, g, _ in out] == list(SQ.decoder_arguments(ops, 4)) and out[5] == ("labels", None, (), ())
    post, smp = out[:5], out[6:12] + out[13:]
    assert [sum(a["min_len"]) for _, a, _, _ in post] == [16, 16, 64, 64, 4]              # an ordinal of its own per decoder
    assert [a.get("join") for _, a, _, _ in post] == [None, "all", "random", None, "zeros"]
    assert [g for _, _, g, _ in post] == [("fwd",), ("grp",), ("fwd",), (), ()]
    assert [n for _, _, _, n in post] == [(), (), (), (), ()]                            # (the 4 lanes run in the joined call's own 64)
    assert [a["n_samples"] for _, a, _, _ in smp] == [8, 130, 8, 65, 3, 3, 64]
    assert [sum(a["min_len"]) for _, a, _, _ in smp] == [16, 64, 16, 64, 4, 4, 64]
    assert [a.get("join") for _, a, _, _ in smp] == ["all", "random", None, None, "zeros", None, "null"]
    assert [g for _, _, g, _ in smp] == [("fwd", "samples", "grp"), ("fwd", "samples"), (), (), (), (), ()]
    assert [n for _, _, _, n in smp] == [(), (), ("fwd", "samples"), ("samples",), (), ("fwd", "samples"), ()]
    assert out[12][1]["join"] == "null" and out[12][2:] == ((), ())                      # the joined Viterbi run keeps its phase, and has no such buffer
    # the reverse: the per-chunk entry point grows, the joined one runs narrower in what it left, and still takes "grp"
    ops = ["sample_minlen", "sample_minlen", "sample_minlen_joined", "minlen_posterior", "minlen_posterior", "minlen_posterior_joined"]
    out = list(SQ._decoder_calls(ops, 4))
    assert [g for _, _, g, _ in out] == [("fwd", "samples"), ("fwd", "samples"), ("grp",), ("fwd",), ("fwd",), ("grp",)]
    assert [n for _, _, _, n in out] == [(), (), ("fwd", "samples"), (), (), ("fwd",)]
    # generation 3's names alone: what the count per decoder gave
    ops = ["minlen_posterior", "sample_minlen", "minlen_posterior", "forward", "minlen_posterior", "sample_minlen"]
    assert [g for _, _, g in SQ.decoder_arguments(ops, 4)] == [("fwd",), ("fwd", "samples"), ("fwd",), (), (), ("fwd", "samples")]


def test_generation_4_covers_the_decoders():
    cov = SQ.state_coverage()
    assert cov == SQ.state_coverage(SQ.GENERATIONS[4][3], 4)
    assert sorted(cov["calls"]) == sorted(SQ.ALL_DECODERS) and len(cov["calls"]) == 8
    for d, n in cov["calls"].items():
        assert n >= 2, (d, n)
    for d in SQ.JOINED_DECODERS:
        assert cov["after_forward"][d] >= 1, d
        assert cov["most_in_one"][d] >= 3, d
        assert len(cov["joins"][d]) >= 3 and cov["joins"][d] <= set(SQ.JOIN_CYCLE), (d, cov["joins"][d])
    # both orders of the two entry points of every shared state, within a sequence
    assert sorted({s for s, _, _ in cov["orders"]}) == ["mlp", "mls", "mlv"] and len(cov["orders"]) == 6
    for key, n in cov["orders"].items():
        assert n >= 1, key
    assert sorted(cov["grows"]) == [("mlp", "fwd"), ("mls", "fwd"), ("mls", "samples")] == sorted(cov["reuses"])
    for buf in cov["grows"]:
        assert cov["grows"][buf] >= 1 and cov["reuses"][buf] >= 2, (buf, cov["grows"][buf], cov["reuses"][buf])
    # per buffer and entry point: a call narrower than what the OTHER entry point left in the buffer
    assert len(cov["narrower"]) == 6 and {d for _, _, d in cov["narrower"]} == {"minlen_posterior", "sample_minlen"} | set(SQ.JOINED_DECODERS)
    for key, n in cov["narrower"].items():
        assert n >= 1, key
    assert all(n >= 1 for n in cov["first_joined"].values())
    # the sample axis: 130 samples (three wavefront groups) are drawn, and a narrower call of either entry point follows in that slab
    for seed in SQ.GENERATIONS[4][3]:
        sizes = [(op, a["n_samples"]) for op, a, _ in SQ.decoder_arguments(SQ.sequence(seed, 4), 4) if a and "n_samples" in a]
        if ("sample_minlen_joined", 130) in sizes:
            after = sizes[sizes.index(("sample_minlen_joined", 130)) + 1:]
            if any(op == "sample_minlen" for op, _ in after):
                break
    else:
        raise AssertionError("no sequence runs hf_sample_paths_minlen in the slab a joined call of 130 samples left")


def test_state_coverage_counts():
    """state_coverage on generation 3, whose sequences hold no call of the new entry points: its counts are decoder_coverage's."""
    cov, old = SQ.state_coverage(generation=3), SQ.decoder_coverage()
    assert cov["calls"] == old["calls"] and cov["after_forward"] == old["after_forward"] and cov["most_in_one"] == old["most_in_one"]
    assert cov["joins"] == {"viterbi_minlen_joined": old["joins"]} and cov["first_joined"] == {"mlp": 0, "mls": 0}
    assert cov["orders"] == {("mlv", "viterbi_minlen", "viterbi_minlen_joined"): old["minlen_then_joined"],
                             ("mlv", "viterbi_minlen_joined", "viterbi_minlen"): old["joined_then_minlen"]}
    for (d, b), n in old["grows"].items():
        assert cov["grows"][SQ.STATES[d], b] == n and cov["reuses"][SQ.STATES[d], b] == old["reuses"][d, b]
    assert all(n == 0 for n in cov["narrower"].values())


def test_generation_3_covers_the_decoders():
    cov = SQ.decoder_coverage()
    assert cov == SQ.decoder_coverage(SQ.GENERATIONS[3][3], 3)
    assert sorted(cov["calls"]) == sorted(SQ.DECODERS + SQ.MINLEN_DECODERS) and len(cov["calls"]) == 6
    for d, n in cov["calls"].items():
        assert n >= 2, (d, n)
    for d in SQ.MINLEN_DECODERS:
        assert cov["after_forward"][d] >= 1, d
        assert cov["most_in_one"][d] >= 3, d               # one grow and one narrower reuse on a single context
    assert cov["minlen_then_joined"] >= 1 and cov["joined_then_minlen"] >= 1
    assert sorted(cov["grows"]) == [("minlen_posterior", "fwd"), ("sample_minlen", "fwd"), ("sample_minlen", "samples")]
    for buf in cov["grows"]:
        assert cov["grows"][buf] >= 1 and cov["reuses"][buf] >= 2, (buf, cov["grows"][buf], cov["reuses"][buf])
    assert len(cov["joins"]) >= 3 and cov["joins"] <= set(SQ.JOIN_CYCLE)
    # within one sequence: a call that grows the buffer, later one with fewer lanes (samples) in the buffer the wider call left
    for d, b in cov["grows"]:
        key = (lambda a: sum(a["min_len"])) if b == "fwd" else (lambda a: a["n_samples"])
        found = False
        for seed in SQ.GENERATIONS[3][3]:
            sizes = [(key(a), b in g) for op, a, g in SQ.decoder_arguments(SQ.sequence(seed, 3)) if op == d]
            found |= any(grew and i > 0 and any(n < size for n, _ in sizes[i + 1:]) for i, (size, grew) in enumerate(sizes))
        assert found, (d, b)


def test_decoder_coverage_counts():
    """decoder_coverage on generation 2, whose sequences hold no call it could miscount: no new decoder, no shared state in two orders."""
    cov = SQ.decoder_coverage(generation=2)
    assert sorted(cov["calls"]) == sorted(SQ.DECODERS) and all(n >= 1 for n in cov["calls"].values())
    assert cov["minlen_then_joined"] == 0 == cov["joined_then_minlen"] and cov["joins"] == set()
    assert all(n == 0 for n in list(cov["grows"].values()) + list(cov["reuses"].values()))
    n = sum(op == "viterbi_minlen" for s in SQ.GENERATIONS[2][3] for op in SQ.sequence(s, 2))
    assert cov["calls"]["viterbi_minlen"] == n


def test_sequences_are_reproducible_and_of_the_stated_length():
    for gen in GENS:
        getters, decoders, length, seeds = SQ.GENERATIONS[gen]
        for seed in seeds:
            ops = SQ.sequence(seed, gen)
            assert ops == SQ.sequence(seed, gen) and len(ops) == length
            assert set(ops) <= set(getters + SQ.PASSES + decoders + SQ.SWITCHES)
        assert len({tuple(SQ.sequence(s, gen)) for s in seeds}) == len(seeds)


def test_every_operation_occurs():
    for gen in GENS:
        getters, decoders, _, seeds = SQ.GENERATIONS[gen]
        seen = set()
        for seed in seeds:
            seen |= set(SQ.sequence(seed, gen))
        assert seen == set(getters + SQ.PASSES + decoders + SQ.SWITCHES)


def test_committed_seeds_cover_every_getter():
    for gen in GENS:
        cov = SQ.coverage(generation=gen)
        assert sorted(cov) == sorted(SQ.GENERATIONS[gen][0])
        for g, c in cov.items():
            assert c["after_full"] >= 2, (g, c)
            assert c["first_after_full"] >= 1, (g, c)
            assert c["after_decoder"] >= 1, (g, c)
            assert c["after_forward"] >= 1, (g, c)
        if gen == 1:
            assert cov == SQ.coverage()


def test_replay_bookkeeping():
    ops = ["alpha_on", "pass_a", "viterbi", "labels", "flip", "alpha_off", "posterior", "forward", "labels"]
    st = [s for _, s in SQ.replay(ops)]
    assert st[1]["last_pass"] is None and st[1]["alpha"]
    assert st[3]["last_pass"] == "pass_a" and st[3]["prev"] == "viterbi" and not st[3]["getter_since_pass"] and st[3]["pass_alpha"]
    assert st[3]["alpha_answers"] and not st[6]["alpha_answers"] and not st[8]["alpha_answers"]
    assert st[6]["getter_since_pass"] and st[6]["flipped"] and not st[6]["pass_flipped"] and not st[6]["alpha"] and st[6]["pass_alpha"]
    assert st[8]["last_pass"] == "forward" and not st[8]["getter_since_pass"] and st[8]["pass_flipped"] and not st[8]["pass_alpha"]
    # the minimum-length decoder in front of a getter: a decoder is no pass and no getter
    ops = ["alpha_on", "pass_b", "breakpoints", "viterbi_minlen", "long_run_log_probs", "pass_a", "viterbi_minlen", "breakpoint_profile"]
    st = [s for _, s in SQ.replay(ops)]
    assert st[3]["prev"] == "breakpoints" and st[3]["getter_since_pass"]
    assert st[4]["prev"] == "viterbi_minlen" and st[4]["last_pass"] == "pass_b" and st[4]["getter_since_pass"] and st[4]["alpha_answers"]
    assert st[7]["prev"] == "viterbi_minlen" and st[7]["last_pass"] == "pass_a" and not st[7]["getter_since_pass"]
    cov = {g: 0 for g in SQ.GETTERS}
    for op, s in SQ.replay(ops):
        if op in SQ.GETTERS and s["prev"] in SQ.DECODERS:
            cov[op] += 1
    assert cov["long_run_log_probs"] == 1 and cov["breakpoint_profile"] == 1 and cov["breakpoints"] == 0
    # the decoders of generation 3: no pass, no getter, whatever their arguments
    ops = ["alpha_off", "pass_a", "minlen_posterior", "posterior", "sample_minlen", "viterbi_minlen_joined", "forward", "sample_minlen",
           "labels", "viterbi_minlen_joined", "alpha_on", "pass_b", "viterbi_minlen", "alpha_stats"]
    st = [s for _, s in SQ.replay(ops)]
    assert st[3]["prev"] == "minlen_posterior" and st[3]["last_pass"] == "pass_a" and not st[3]["getter_since_pass"]
    assert st[5]["prev"] == "sample_minlen" and st[5]["getter_since_pass"] and st[6]["prev"] == "viterbi_minlen_joined"
    assert st[7]["last_pass"] == "forward" and st[8]["prev"] == "sample_minlen" and not st[8]["getter_since_pass"]
    assert st[9]["last_pass"] == "forward" and st[9]["getter_since_pass"]
    assert st[13]["prev"] == "viterbi_minlen" and st[13]["alpha_answers"] and not st[13]["getter_since_pass"]
    assert [op for op, s in SQ.replay(ops) if s["last_pass"] == "forward" and op in SQ.MINLEN_DECODERS] == ["sample_minlen", "viterbi_minlen_joined"]
