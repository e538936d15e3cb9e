"""The reference of maximum-expected-accuracy decoding under minimum run lengths (tests/mea_ref.py) against enumeration of all 4^T
labellings on the tiny stores, per chunk and over joined groups, and its exact case: lengths 1 with the identity are posterior argmax."""
import numpy as np
import pytest

import mea_ref
import minlen_ref

ONES = (1, 1, 1, 1)


def _blocks(store, joined):
    if joined is None:
        return np.asarray(store.chunk_off, np.int64)
    return mea_ref.group_off(store.chunk_off, joined)[0]


@pytest.mark.parametrize("model_type,seed,hifi", minlen_ref.TINY_CASES)
@pytest.mark.parametrize("min_len", minlen_ref.TINY_MIN_LENS)
@pytest.mark.parametrize("joined", [None, mea_ref.TINY_JOINED], ids=["chunks", "joined"])
def test_reference_equals_enumeration(model_type, seed, hifi, min_len, joined):
    store, model, alpha, post, logA = mea_ref.tiny(model_type, seed, hifi)
    boff = _blocks(store, joined)
    if joined is not None:
        assert np.diff(boff).tolist() == [8, 7, 5 + 1, 6, 3 + 2, 4]                    # two groups of two chunks among the blocks
    for W in mea_ref.TINY_GAINS:
        G = mea_ref.gain_rows(post, logA, store.chunk_off, W)
        labels, score = mea_ref.decode(G, boff, min_len)
        assert minlen_ref.admissible(labels, boff, min_len).all()
        assert mea_ref.supported(labels, post, logA, store.chunk_off).all()
        val = mea_ref.expected_gain(labels, post, W, boff)
        clear = 0
        for b in range(boff.size - 1):
            path, best, second = mea_ref.enumerate_block(G, int(boff[b]), int(boff[b + 1]), min_len)
            T = int(boff[b + 1] - boff[b])
            tol = 1e-12 * T * np.abs(W).max()
            assert abs(score[b] - best) <= tol and abs(val[b] - best) <= tol, (b, score[b], val[b], best)
            if best - second > 1e-9:
                assert np.array_equal(labels[boff[b]:boff[b + 1]], path), (b, labels[boff[b]:boff[b + 1]], path)
                clear += 1
        assert clear >= (boff.size - 1) // 2


def test_two_chunk_group_is_one_block():
    off, gchunk = mea_ref.group_off([0, 8, 15, 20, 21, 27, 30, 32, 36], mea_ref.TINY_JOINED)
    assert off.tolist() == [0, 8, 15, 21, 27, 32, 36] and gchunk.tolist() == [0, 1, 2, 4, 5, 7]
    # a chunk without windows ends a group whatever the entries say
    off, gchunk = mea_ref.group_off([0, 4, 4, 9], [0, 1, 1])
    assert off.tolist() == [0, 4, 4, 9] and gchunk.tolist() == [0, 1, 2]


@pytest.mark.parametrize("model_type,seed,hifi", minlen_ref.TINY_CASES)
def test_lengths_one_with_the_identity_are_posterior_argmax(model_type, seed, hifi):
    store, model, alpha, post, logA = mea_ref.tiny(model_type, seed, hifi)
    for joined in (None, mea_ref.TINY_JOINED):
        boff = _blocks(store, joined)
        # support ignored: exactly the per-window argmax, first largest
        G = mea_ref.gain_rows(post, logA, store.chunk_off, mea_ref.IDENTITY, support=False)
        labels, score = mea_ref.decode(G, boff, ONES)
        srt = np.sort(post, axis=1)
        clear = srt[:, 3] - srt[:, 2] > 1e-9
        assert clear.mean() >= 0.9
        assert np.array_equal(labels[clear], np.argmax(post, axis=1)[clear])
        want = np.array([post.max(axis=1)[boff[b]:boff[b + 1]].sum() for b in range(boff.size - 1)])
        assert np.all(np.abs(score - want) <= 1e-12 * np.diff(boff))
        # with support: never above it, and equal wherever the argmax labelling is supported
        Gs = mea_ref.gain_rows(post, logA, store.chunk_off, mea_ref.IDENTITY)
        ls, ss = mea_ref.decode(Gs, boff, ONES)
        assert np.all(ss <= score + 1e-12 * np.diff(boff))
        sup = mea_ref.supported(np.argmax(post, axis=1), post, logA, store.chunk_off)
        if sup.all():
            assert np.all(np.abs(ss - score) <= 1e-12 * np.diff(boff))


def test_final_bed_rule_in_windows():
    post = np.zeros((10, 4))
    lab = [2, 0, 0, 2, 2, 1, 1, 1, 3, 2]
    post[np.arange(10), lab] = 1.0
    out = mea_ref.final_bed_rule(post, [0, 5, 10], None, (3, 3, 1, 2))
    assert out.tolist() == [2, 2, 2, 2, 2, 1, 1, 1, 2, 2]
    out = mea_ref.final_bed_rule(post, [0, 5, 10], None, (2, 4, 1, 1))
    assert out.tolist() == [2, 0, 0, 2, 2, 2, 2, 2, 3, 2]
    # joined: the run of Dup goes on across the chunk boundary
    lab = [2, 0, 0, 1, 1, 1, 1, 2, 3, 2]
    post[:] = 0.0
    post[np.arange(10), lab] = 1.0
    assert mea_ref.final_bed_rule(post, [0, 5, 10], None, (1, 3, 1, 1)).tolist() == [2, 0, 0, 2, 2, 2, 2, 2, 3, 2]
    assert mea_ref.final_bed_rule(post, [0, 5, 10], [0, 1], (1, 3, 1, 1)).tolist() == lab
