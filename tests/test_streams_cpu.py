"""What the committed call orders of tests/test_streams_gpu.py cover (tests/stream_sequences.py), on the generator alone: every getter
kind runs at least twice after a full pass, at least once as the FIRST getter after a full pass (its lazy state is built then), at
least once directly after a decoder call with other parameters, and — for the refusals — at least once after a forward-only pass.
This holds for each generation of sequences by itself: for the ten getters of the first over its seeds, and for all thirteen getters
over the seeds of the second alone."""
import hashlib
import json

import stream_sequences as SQ

GENS = sorted(SQ.GENERATIONS)
# sha256 of json.dumps of the four lists of generation 1, computed at the commit before the second generation was added
GENERATION_1_DIGEST = "6ec2eb0113304e64909753fbb9f77679807ef5142128e2cd98f557c75c994049"


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
