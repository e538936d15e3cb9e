"""What the committed call orders of tests/test_streams_gpu.py cover (tests/stream_sequences.py), on the generator alone: every getter
kind runs at least twice after a full pass, at least once as the FIRST getter after a full pass (its lazy state is built then), at
least once directly after a decoder call with other parameters, and — for the refusals — at least once after a forward-only pass."""
import stream_sequences as SQ


def test_sequences_are_reproducible_and_of_the_stated_length():
    for seed in SQ.SEEDS:
        ops = SQ.sequence(seed)
        assert ops == SQ.sequence(seed) and len(ops) == SQ.LENGTH
        assert set(ops) <= set(SQ.GETTERS + SQ.PASSES + SQ.DECODERS + SQ.SWITCHES)
    assert len({tuple(SQ.sequence(s)) for s in SQ.SEEDS}) == len(SQ.SEEDS)


def test_every_operation_occurs():
    seen = set()
    for seed in SQ.SEEDS:
        seen |= set(SQ.sequence(seed))
    assert seen == set(SQ.GETTERS + SQ.PASSES + SQ.DECODERS + SQ.SWITCHES)


def test_committed_seeds_cover_every_getter():
    cov = SQ.coverage()
    assert sorted(cov) == sorted(SQ.GETTERS)
    for g, c in cov.items():
        assert c["after_full"] >= 2, (g, c)
        assert c["first_after_full"] >= 1, (g, c)
        assert c["after_decoder"] >= 1, (g, c)
        assert c["after_forward"] >= 1, (g, c)


def test_replay_bookkeeping():
    ops = ["alpha_on", "pass_a", "viterbi", "labels", "flip", "alpha_off", "posterior", "forward", "labels"]
    st = [s for _, s in SQ.replay(ops)]
    assert st[1]["last_pass"] is None and st[1]["alpha"]
    assert st[3]["last_pass"] == "pass_a" and st[3]["prev"] == "viterbi" and not st[3]["getter_since_pass"] and st[3]["pass_alpha"]
    assert st[3]["alpha_answers"] and not st[6]["alpha_answers"] and not st[8]["alpha_answers"]
    assert st[6]["getter_since_pass"] and st[6]["flipped"] and not st[6]["pass_flipped"] and not st[6]["alpha"] and st[6]["pass_alpha"]
    assert st[8]["last_pass"] == "forward" and not st[8]["getter_since_pass"] and st[8]["pass_flipped"] and not st[8]["pass_alpha"]
