"""ASMK query expansion on the host: the twin (tests/asmk_expand_numpy.py) against itself at the corners of the
definition, the arguments of `ASMKExpansion`, the overflow guard, and the effect of the expansion on the grouped corpus."""
import numpy as np
import pytest

import asmk_expand_numpy as xt
import asmk_numpy as tw
from pvsim import ASMKExpansion, asmk

B, W, K = 64, 2, 12


def _sig(rng):
    return rng.randint(0, 1 << 32, W, dtype=np.uint64).astype(np.uint32)


def _file(db):
    return tw.invert(db, K)


@pytest.fixture(scope="module")
def small():
    """five images over twelve words; the query shares the words 1, 4, 7 with some of them and holds 9 alone"""
    rng = np.random.RandomState(1901)
    words = [[0, 1, 4, 7], [1, 4, 5, 11], [4, 5, 7, 11], [], [0, 5, 10]]
    db = [(np.array(w, np.int32), np.array([_sig(rng) for _ in w], np.uint32).reshape(len(w), W)) for w in words]
    query = (np.array([1, 4, 7, 9], np.int32), np.array([_sig(rng) for _ in range(4)], np.uint32))
    wt = rng.randint(1, 1024, K).astype(np.int32)
    return db, query, wt


def _expand(small, members, votes, query_vote=2, h_max=B, min_support=2, query=None):
    db, q, wt = small
    q = q if query is None else query
    out, counts, sums = xt.expand([q], *_file(db), np.array([members], np.int32), np.array([votes], np.int32), query_vote, h_max,
                                  min_support, wt)
    assert counts[0] == len(out[0][0]) and sums[0] == tw.weight_sum(out[0][0], wt)      # sum is the weight sum of the output
    assert (np.diff(out[0][0]) > 0).all()
    return out[0]


def test_no_member_is_the_identity(small):
    _, q, _ = small
    for members, votes in (([], []), ([-1, -1, -1], [0, 0, 0])):
        for min_support in (0, 1, 2):
            w, s = _expand(small, members, votes, min_support=min_support)
            assert np.array_equal(w, q[0]) and np.array_equal(s, q[1])
    beyond = (np.array([-3, 1, 4, 12, 40], np.int32), np.concatenate([q[1][:1], q[1][:2], q[1][:2]]))
    w, s = _expand(small, [], [], query=beyond)                                          # query words outside [0, K) are dropped
    assert np.array_equal(w, [1, 4]) and np.array_equal(s, beyond[1][1:3])


def test_min_support_zero_adds_no_word(small):
    _, q, _ = small
    w, _ = _expand(small, [0, 1, 2, 4], [1, 1, 1, 1], min_support=0)
    assert np.array_equal(w, q[0])
    w1, _ = _expand(small, [0, 1, 2, 4], [1, 1, 1, 1], min_support=1)
    assert np.array_equal(w1, [0, 1, 4, 5, 7, 9, 10, 11])                                # every word a member holds
    w2, _ = _expand(small, [0, 1, 2, 4], [1, 1, 1, 1], min_support=2)
    assert np.array_equal(w2, [0, 1, 4, 5, 7, 9, 11])                                    # 10 is held once
    w5, _ = _expand(small, [0, 1, 2, 4], [1, 1, 1, 1], min_support=5)
    assert np.array_equal(w5, q[0])                                                      # more than there are members


def test_one_member_without_gate_and_query_vote_copies_its_bits(small):
    db, q, _ = small
    w, s = _expand(small, [1], [7], query_vote=0, h_max=B, min_support=0)
    assert np.array_equal(w, q[0])
    assert np.array_equal(s[0], db[1][1][0]) and np.array_equal(s[1], db[1][1][1])       # words 1 and 4: image 1's signatures
    assert np.array_equal(s[2], q[1][2]) and np.array_equal(s[3], q[1][3])               # 7 and 9: image 1 holds neither
    w, s = _expand(small, [1], [7], query_vote=0, h_max=0, min_support=0)                # the gate shuts image 1 out
    assert np.array_equal(s, q[1])


def test_the_gate_uses_the_original_signature(small):
    db, q, _ = small
    h = [tw.popcount(np.bitwise_xor(db[i][1][list(db[i][0]).index(4)], q[1][1])) for i in (0, 1, 2)]
    assert len(set(h)) == 3
    mid = sorted(h)[1]
    _, s = _expand(small, [0, 1, 2], [1, 1, 1], query_vote=1, h_max=mid, min_support=0)
    voters = [i for i, hd in zip((0, 1, 2), h) if hd <= mid]
    want = []
    for t in range(B):
        tally = (2 * xt.bit(q[1][1], t) - 1) + sum(2 * xt.bit(db[i][1][list(db[i][0]).index(4)], t) - 1 for i in voters)
        want.append(1 if tally > 0 else 0 if tally < 0 else xt.bit(q[1][1], t))
    assert np.array_equal(s[1], xt.pack(want))


def test_ties(small):
    db, q, wt = small
    ones, zeros = np.full(W, 0xFFFFFFFF, np.uint32), np.zeros(W, np.uint32)
    mixed = np.array([0x0F0F0F0F, 0xFFFF0000], np.uint32)
    tied = [(np.array([3], np.int32), ones[None].copy()), (np.array([3], np.int32), zeros[None].copy())]
    q3 = (np.array([3], np.int32), mixed[None].copy())
    # a query word: two members cancel, query_vote 0 -> every tally is 0 and the query's bits stay
    out, _, _ = xt.expand([q3], *tw.invert(tied, K), np.array([[0, 1]], np.int32), np.array([[5, 5]], np.int32), 0, B, 0, wt)
    assert np.array_equal(out[0][1][0], mixed)
    # ... and with query_vote 5 against one member of vote 5 that disagrees everywhere
    inv = np.bitwise_not(mixed)
    out, _, _ = xt.expand([q3], *tw.invert([(np.array([3], np.int32), inv[None].copy())], K), np.array([[0]], np.int32),
                          np.array([[5]], np.int32), 5, B, 0, wt)
    assert np.array_equal(out[0][1][0], mixed)
    # a new word: the two members cancel on every bit -> all ones (the z >= 0 rule)
    none = (np.zeros(0, np.int32), np.zeros((0, W), np.uint32))
    out, counts, _ = xt.expand([none], *tw.invert(tied, K), np.array([[0, 1]], np.int32), np.array([[5, 5]], np.int32), 2, B, 2, wt)
    assert counts[0] == 1 and np.array_equal(out[0][0], [3]) and np.array_equal(out[0][1][0], ones)


def test_members_and_votes_follow_the_lists():
    idx = np.array([[7, 2, -1, 5], [3, -1, -1, -1], [-1, -1, -1, -1]], np.int64)
    for scheme, want_votes in (("flat", [[1, 1, 1, 0, 0], [1, 0, 0, 0, 0], [0] * 5]), ("linear", [[4, 2, 5, 0, 0], [5, 0, 0, 0, 0], [0] * 5])):
        members, votes = ASMKExpansion(n=5, scheme=scheme).members_of(idx)
        assert members.dtype == np.int32 and votes.dtype == np.int32
        assert members.tolist() == [[2, 5, 7, -1, -1], [3, -1, -1, -1, -1], [-1] * 5] and votes.tolist() == want_votes
        tm, tv = xt.members_and_votes(idx, 5, scheme)
        assert np.array_equal(tm, members) and np.array_equal(tv, votes)
    members, _ = ASMKExpansion(n=2).members_of(idx)                                      # only the first n slots
    assert members.tolist() == [[2, 7], [3, -1], [-1, -1]]
    with pytest.raises(ValueError, match="twice"):
        ASMKExpansion(n=3).members_of(np.array([[4, 4, 1]]))


def test_expansion_arguments():
    e = ASMKExpansion()
    assert (e.n, e.h_max, e.min_support, e.query_vote, e.scheme, e.passes) == (10, None, 2, 2, "flat", 1)
    assert e.resolve_h_max(128) == 32 and e.resolve_h_max(32) == 8
    lin = ASMKExpansion(n=7, scheme="linear")
    assert lin.query_vote == 7 and ASMKExpansion(n=7, scheme="linear", query_vote=0).query_vote == 0
    assert ASMKExpansion(h_max=0).resolve_h_max(32) == 0 and ASMKExpansion(h_max=64).resolve_h_max(64) == 64
    with pytest.raises(ValueError, match="exceeds"):
        ASMKExpansion(h_max=64).resolve_h_max(32)
    assert "min_support=2" in repr(e)
    for bad in (dict(n=0), dict(n=33), dict(n=True), dict(n=2.0), dict(h_max=-1), dict(h_max=129), dict(h_max=1.5), dict(min_support=-1),
                dict(min_support=34), dict(min_support=None), dict(query_vote=-1), dict(query_vote=65536), dict(query_vote=1.0),
                dict(scheme="average"), dict(scheme=None), dict(passes=0), dict(passes=True), dict(passes=1.0)):
        with pytest.raises(ValueError):
            ASMKExpansion(**bad)


def test_member_arrays_are_checked_before_any_device_work():
    ok_m, ok_v = np.array([[1, 4, -1]], np.int32), np.array([[1, 9, 0]], np.int32)
    m, v = asmk._check_members(ok_m, ok_v, 1, 5)
    assert m.dtype == np.int32 and np.array_equal(m, ok_m) and np.array_equal(v, ok_v)
    for members, votes, N in (([[4, 1, -1]], [[1, 1, 0]], 5), ([[1, 1, -1]], [[1, 1, 0]], 5), ([[-1, 1, 4]], [[0, 1, 1]], 5),
                              ([[1, 5, -1]], [[1, 1, 0]], 5), ([[1, 4, -1]], [[1, 0, 0]], 5), ([[1, 4, -1]], [[1, 1024, 0]], 5),
                              ([[1, 4, -2]], [[1, 1, 0]], 5), ([[1, 4]], [[1, 1, 0]], 5), ([list(range(33))], [[1] * 33], 40)):
        with pytest.raises(ValueError):
            asmk._check_members(np.array(members), np.array(votes), 1, N)


def test_overflow_guard_names_the_remedy():
    e = ASMKExpansion(n=7, min_support=3)
    asmk.check_expanded_sums(np.array([0, (1 << 32) - 1], np.int64), e)
    asmk.check_expanded_sums(np.zeros(0, np.int64), e)
    with pytest.raises(ValueError, match=r"query 1 .*2\^32.*min_support \(now 3\).*n \(now 7\)"):
        asmk.check_expanded_sums(np.array([5, 1 << 32, 7], np.int64), e)


MEASURED = {11: (0.937, 0.995), 12: (0.936, 0.991), 13: (0.934, 0.990)}    # plain and expanded mAP of the definition


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_expansion_lifts_map_on_the_grouped_corpus(seed):
    """members: the top 5 of the plain ranking, votes 1, query_vote 2, h_max 8, min_support 2; mAP over the full ranking of the 144
    images.  The gains measured on the definition are 0.058, 0.055 and 0.056; the margin of 0.03 is about half of them, so the
    assertion trips when the expansion stops adding the agreed words, and not on a change in the last digit."""
    cent, images, group, queries, qgroup = xt.grouped_corpus(seed)
    db, qe = tw.entries(images, cent), tw.entries(queries, cent)
    wt, sel, N = tw.word_weights(db, len(cent), True), tw.selectivity(32, 3.0, 0.0), len(db)
    assert N == 144 and len(qe) == 24
    plain = xt.mean_average_precision(tw.rank(tw.scores(qe, db, wt, sel), N)[0], group, qgroup)
    expanded = xt.mean_average_precision(xt.rank_expanded(qe, db, wt, sel, N, n=5, h_max=8, min_support=2, query_vote=2)[0], group, qgroup)
    print(f"seed {seed}: plain mAP {plain:.4f}, expanded {expanded:.4f}")
    assert (round(plain, 3), round(expanded, 3)) == MEASURED[seed]                       # the generator and the twin are the issue's
    assert expanded >= plain + 0.03
    if seed == 11:                                                                       # without new words the gain is gone
        bare = xt.mean_average_precision(xt.rank_expanded(qe, db, wt, sel, N, n=5, h_max=8, min_support=0, query_vote=2)[0], group, qgroup)
        assert bare < plain + 0.03
