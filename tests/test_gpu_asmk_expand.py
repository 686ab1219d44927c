"""GPU tests of the ASMK query expansion (csrc/asmk_expand.hip, pvsim.ASMKExpansion, pvsim.ASMKIndex): the entry
point against its NumPy twin (tests/asmk_expand_numpy.py) on random inverted files, and the ranking with `expand=` against the twin
of the index.  Everything is integers or bit patterns: np.array_equal throughout.  Outputs are allocated over a fill pattern, so
what the device must leave alone is checked as well."""
import numpy as np
import pytest

import asmk_expand_numpy as xt
import asmk_numpy as tw
import asmk_update_numpy as up

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 0x5A
FILL32 = np.uint32(0x5A5A5A5A)
DESC_F32 = 0


def _up(ctx, a):
    a = np.ascontiguousarray(a)
    return ctx.buffer(max(a.nbytes, 16)).upload(a) if a.nbytes else ctx.buffer(16)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _flat(ents, W):
    off = np.zeros(len(ents) + 1, np.int64)
    np.cumsum([len(e[0]) for e in ents], out=off[1:])
    words = np.concatenate([e[0] for e in ents]).astype(np.int32) if ents else np.zeros(0, np.int32)
    sigs = np.concatenate([e[1].reshape(-1, W) for e in ents]).astype(np.uint32) if ents else np.zeros((0, W), np.uint32)
    return off, words, sigs


def _rand_sigs(rng, n, W):
    return rng.randint(0, 1 << 32, (n, W), dtype=np.uint64).astype(np.uint32)


def _flip(rng, sig, flips):
    s = sig.copy()
    for _ in range(flips):
        s[rng.randint(0, len(s))] ^= np.uint32(1) << np.uint32(rng.randint(0, 32))
    return s


def _without(ent, words):
    keep = ~np.isin(ent[0], words)
    return ent[0][keep], ent[1][keep]


def _with(ent, word, sig):
    w = np.append(ent[0], word).astype(np.int32)
    order = np.argsort(w, kind="stable")
    return w[order], np.concatenate([ent[1], sig[None]])[order]


class _File:
    """an inverted file (tests/asmk_update_numpy.py inverts the slots that hold exactly the entries) with its weights, resident"""

    def __init__(self, ctx, ents, K, W, wt):
        self.ctx, self.K, self.W, self.N, self.wt = ctx, K, W, len(ents), np.ascontiguousarray(wt, dtype=np.int32)
        off, words, sigs = _flat(ents, W)
        self.host = up.invert(off, np.diff(off).astype(np.int32), words, sigs, K)
        self.bufs = [_up(ctx, a) for a in (*self.host, self.wt)]

    def run(self, queries, members, votes, query_vote, h_max, min_support, cap, tile=0, sig_shift=0):
        """-> (out_word (nq, cap), out_sig (nq, cap, W), count (nq,), sum (nq,)) as the device leaves them over the fill pattern"""
        ctx, W, nq = self.ctx, self.W, len(queries)
        off, words, sigs = _flat(queries, W)
        members, votes = np.ascontiguousarray(members, dtype=np.int32), np.ascontiguousarray(votes, dtype=np.int32)
        d_in = [_up(ctx, a) for a in (words, sigs, members, votes)]
        d_out = [ctx.buffer(max(nq * cap, 4) * 4).fill_bytes(FILL), ctx.buffer(max(nq * cap, 4) * 4 * W + 16).fill_bytes(FILL),
                 ctx.buffer(max(nq, 4) * 4).fill_bytes(FILL), ctx.buffer(max(nq, 2) * 8).fill_bytes(FILL)]
        b = self.bufs
        try:
            ctx.asmk_expand_dev(nq, off, d_in[0].ptr, d_in[1].ptr, 32 * W, self.K, b[0].ptr, b[1].ptr, b[2].ptr, self.N, members.shape[1],
                                d_in[2].ptr, d_in[3].ptr, query_vote, h_max, min_support, b[3].ptr, cap, d_out[0].ptr,
                                d_out[1].ptr + sig_shift, d_out[2].ptr, d_out[3].ptr, tile)
            return (d_out[0].download((max(nq * cap, 4),), np.int32)[:nq * cap].reshape(nq, cap),
                    d_out[1].download((max(nq * cap, 4) * W,), np.uint32)[:nq * cap * W].reshape(nq, cap, W),
                    d_out[2].download((max(nq, 4),), np.int32), d_out[3].download((max(nq, 2),), np.int64))
        finally:
            for x in d_in + d_out:
                x.free()

    def check(self, queries, members, votes, query_vote, h_max, min_support, tiles=(0,), cap=None):
        """the device against the twin, for every tile; -> the twin's (entries, counts)"""
        nq = len(queries)
        want, counts, sums = xt.expand(queries, *self.host, members, votes, query_vote, h_max, min_support, self.wt)
        cap = int(counts.max(initial=0)) + 3 if cap is None else cap
        for tile in tiles:
            ow, os_, cnt, sm = self.run(queries, members, votes, query_vote, h_max, min_support, cap, tile)
            assert np.array_equal(cnt[:nq], counts) and np.array_equal(sm[:nq], sums), tile          # always the true values
            assert (cnt[nq:].view(np.uint32) == FILL32).all() and (sm[nq:].view(np.uint8) == FILL).all()
            for q in range(nq):
                c = min(int(counts[q]), cap)
                assert np.array_equal(ow[q, :c], want[q][0][:c]) and np.array_equal(os_[q, :c], want[q][1][:c]), (tile, q)
                assert (ow[q, c:].view(np.uint32) == FILL32).all() and (os_[q, c:] == FILL32).all(), (tile, q)   # nothing beyond
        return want, counts

    def close(self):
        for b in self.bufs:
            b.free()


def _members(rows, R):
    """lists of ids -> (members (nq, R) ascending with -1 padding, flat votes)"""
    m, v = np.full((len(rows), R), -1, np.int32), np.zeros((len(rows), R), np.int32)
    for q, ids in enumerate(rows):
        ids = sorted(ids)[:R]
        m[q, :len(ids)], v[q, :len(ids)] = ids, 1
    return m, v


# ------------------------------------------------------------------------------------------------ the entry point
KS, WS, RS = [1, 5, 257, 65536], [1, 2, 3, 4], [0, 1, 10, 32]
CASES = [(K, W, RS[(ik + iw) % 4]) for ik, K in enumerate(KS) for iw, W in enumerate(WS)]      # every K with every B and every R


@pytest.mark.parametrize("K,W,R", CASES)
def test_expand_matches_the_twin(gpu_ctx, K, W, R):
    rng = np.random.RandomState(1990 + K % 1000 + 7 * W + R)
    N, B = 200, 32 * W
    E = {1: 150, 5: 600}.get(K, 4000)
    ents = up.make_slots(rng, N, E, K, W, "random")[4]
    hollow, stranger, tie_a, tie_b = 17, 23, 40, 90
    ents[hollow] = (np.zeros(0, np.int32), np.zeros((0, W), np.uint32))                        # a member with no entries
    if not len(ents[N - 1][0]):                                 # K = 1: the last image holds the word as well
        ents[N - 1] = (ents[1][0].copy(), ents[1][1].copy())
    wa, wb = (100, 200) if K >= 257 else (None, None)
    if wa is not None:                                          # planted ties: two members alone hold wa and wb, with opposite bits
        ents = [_without(e, [wa, wb]) for e in ents]
        sa, sb = _rand_sigs(rng, 1, W)[0], _rand_sigs(rng, 1, W)[0]
        ents[tie_a], ents[tie_b] = _with(_with(ents[tie_a], wa, sa), wb, sb), _with(_with(ents[tie_b], wa, ~sa), wb, ~sb)
    if K == 65536:
        assert 0 in ents[0][0] and 65535 in ents[0][0]                                          # the words at both ends are held
    base = [0, N - 1, hollow, stranger, tie_a, tie_b] + [int(i) for i in rng.permutation(np.arange(1, N - 1)) if i not in (hollow, stranger, tie_a, tie_b)]
    ids = base[:R]
    # query 0: half of the words of the members 0 and N - 1 with signatures near theirs, random words, none of the stranger's, wa but
    # not wb, word 0 but not word K - 1 at the largest K, and a word beyond K at the end
    q0 = {}
    for i in (0, N - 1):
        for w, s in zip(*ents[i]):
            if rng.randint(0, 2):
                q0[int(w)] = _flip(rng, s, rng.randint(0, B // 3))
    for w in rng.randint(0, K, 12):
        q0.setdefault(int(w), _rand_sigs(rng, 1, W)[0])
    if K > 5:
        for w in list(ents[stranger][0]) + [wb, K - 1]:
            q0.pop(w, None)
        assert len(ents[stranger][0]) and not set(q0) & set(ents[stranger][0].tolist())         # a member sharing no query word
    if wa is not None:
        q0[wa] = _rand_sigs(rng, 1, W)[0]
    if K == 65536:
        q0[0] = _flip(rng, ents[0][1][0], 2)
    q0[K + 5] = _rand_sigs(rng, 1, W)[0]
    words0 = np.array(sorted(q0), np.int32)
    queries = [(words0, np.array([q0[int(w)] for w in words0], np.uint32).reshape(-1, W)),
               (np.zeros(0, np.int32), np.zeros((0, W), np.uint32)),                            # an empty query
               (np.concatenate([[-2], np.sort(rng.permutation(K)[:min(K, 9)])]).astype(np.int32), _rand_sigs(rng, min(K, 9) + 1, W))]
    members, flat = _members([ids, ids, ids[:R // 2]], R)                                       # the last one padded with -1
    if R >= 10:
        assert {0, N - 1, hollow, stranger, tie_a, tie_b} <= set(members[0].tolist()) and (members[2] == -1).any()
    varied = np.where(members >= 0, rng.randint(1, 1024, members.shape), 0).astype(np.int32)
    f = _File(gpu_ctx, ents, K, W, rng.randint(0, 1024, K))
    try:
        word_off, ent_img = f.host[0], f.host[1]
        if R >= 1:                                               # member 0 is first in a list, member N - 1 last in one
            assert any(ent_img[word_off[w]] == 0 for w in ents[0][0])
        if R >= 2:
            assert any(ent_img[word_off[w + 1] - 1] == N - 1 for w in ents[N - 1][0])
        want, counts = f.check(queries, members, flat, 2, B // 4, 1, tiles=(64, 256, 0))
        if K == 65536 and R >= 1:                                # word 0 is a query word, word 65535 a new one
            assert want[0][0][0] == 0 and want[0][0][-1] == 65535 and want[1][0][-1] == 65535
        if R >= 1:
            assert counts[1] > 0                                 # the empty query gains the words of its members
        f.check(queries, members, flat, 2, 0, 0)
        f.check(queries, members, varied, 0, B, R)
        f.check(queries, members, flat, 1, B, R + 1)
        f.check(queries, members, np.where(members >= 0, 1023, 0), 65535, B // 4, 1)            # the largest votes
        full, counts = f.check(queries, members, flat, 0, B, 2)
        if wa is not None and R >= 10:                           # both ties: the query's bits stay, the new word is all ones
            at = {int(w): s for w, s in zip(*full[0])}
            assert np.array_equal(at[wa], q0[wa]) and (at[wb] == 0xFFFFFFFF).all() and wb not in q0
        if counts.max() >= 2:                                    # cap below count: the first cap entries, the true count and sum
            f.check(queries, members, flat, 0, B, 2, tiles=(64, 0), cap=int(counts.max()) // 2)
        f.check(queries, members, flat, 0, B, 2, cap=1)
    finally:
        f.close()


def test_a_long_list_and_members_at_its_ends(gpu_ctx):
    """word 2 is held by the images 0 .. 699 of 800: the members 0 and 699 stand first and last in a list of 700 entries"""
    rng = np.random.RandomState(1991)
    K, W, N, B = 5, 4, 800, 128
    ents = []
    for i in range(N):
        words = np.array(sorted(set(([2] if i < 700 else []) + [int(w) for w in rng.permutation(K)[:rng.randint(0, 3)] if w != 2])), np.int32)
        ents.append((words, _rand_sigs(rng, len(words), W)))
    f = _File(gpu_ctx, ents, K, W, rng.randint(1, 1024, K))
    try:
        assert f.host[0][3] - f.host[0][2] == 700
        queries = [(np.array([2], np.int32), _flip(rng, ents[699][1][list(ents[699][0]).index(2)], 5)[None]),
                   (np.array([0, 4], np.int32), _rand_sigs(rng, 2, W))]
        members, votes = _members([[0, 350, 699, 799], [699, 0]], 4)
        for h_max, min_support in ((B // 4, 1), (B, 2), (0, 0)):
            f.check(queries, members, votes, 2, h_max, min_support, tiles=(64, 0))
    finally:
        f.close()


@pytest.mark.parametrize("nq", [0, 1, 130])
def test_query_counts(gpu_ctx, nq):
    """no query; one; more than the 128 whose offsets one launch carries"""
    rng = np.random.RandomState(1992 + nq)
    K, W, N, R = 257, 2, 200, 3
    ents = up.make_slots(rng, N, 4000, K, W, "random")[4]
    f = _File(gpu_ctx, ents, K, W, rng.randint(0, 1024, K))
    try:
        queries = []
        for _ in range(nq):
            words = np.sort(rng.permutation(K)[:rng.randint(0, 7)]).astype(np.int32)
            queries.append((words, _rand_sigs(rng, len(words), W)))
        members, votes = _members([rng.permutation(N)[:rng.randint(0, R + 1)].tolist() for _ in range(nq)], R)
        f.check(queries, members.reshape(nq, R), votes.reshape(nq, R), 2, 64, 2, tiles=(64, 0))
    finally:
        f.close()


def test_expand_refuses_bad_arguments(gpu_ctx):
    rng = np.random.RandomState(1993)
    K, W, N = 9, 4, 6
    ents = up.make_slots(rng, N, 20, K, W, "random")[4]
    queries = [(np.array([1, 3], np.int32), _rand_sigs(rng, 2, W))]
    members, votes = _members([[0, 4]], 2)
    f = _File(gpu_ctx, ents, K, W, np.ones(K, np.int32))
    try:
        f.run(queries, members, votes, 2, 32, 2, 8)
        for kw in (dict(query_vote=-1), dict(query_vote=65536), dict(h_max=-1), dict(h_max=129), dict(min_support=-1), dict(min_support=34),
                   dict(cap=-1), dict(tile=32), dict(tile=100), dict(tile=4160), dict(sig_shift=4)):
            args = dict(query_vote=2, h_max=32, min_support=2, cap=8, tile=0, sig_shift=0)
            args.update(kw)
            with pytest.raises(ValueError):
                f.run(queries, members, votes, args["query_vote"], args["h_max"], args["min_support"], args["cap"], args["tile"], args["sig_shift"])
        with pytest.raises(ValueError):
            f.run(queries, *_members([list(range(6))], 33), 2, 32, 2, 8)
        f.K = 0
        with pytest.raises(ValueError):
            f.run(queries, members, votes, 2, 32, 2, 8)
    finally:
        f.close()


# ------------------------------------------------------------------------------------------------ end to end
def _index(ctx, cent, db, wt, bits, frozen=False):
    """an ASMKIndex over float32 rows from the twin's own arrays"""
    from pvsim import ASMKIndex
    K = len(cent)
    gamma = np.array([tw.gamma(x[0], wt) for x in db], F)
    return ASMKIndex([f"im{i}" for i in range(len(db))], cent, *tw.invert(db, K), gamma, wt, tw.selectivity(bits, 3.0, 0.0), bits,
                     desc_kind=DESC_F32, ctx=ctx, frozen=frozen)


def _same_lists(got, want):
    kk = want[0].shape[1]
    return (np.array_equal(got[0][:, :kk], want[0]) and np.array_equal(_bits(got[1][:, :kk]), _bits(want[1]))
            and (got[0][:, kk:] == -1).all() and np.isneginf(got[1][:, kk:]).all())


@pytest.fixture(scope="module")
def grouped():
    cent, images, group, queries, qgroup = xt.grouped_corpus(seed=11)
    for x in images + queries:
        assert tw.labels_and_gap(x, cent)[1] > 1e-3
    db, qe = tw.entries(images, cent), tw.entries(queries, cent)
    return cent, images, queries, db, qe, tw.word_weights(db, len(cent), True)


@pytest.mark.parametrize("passes", [1, 2])
def test_rank_rows_with_expansion_on_the_grouped_corpus(gpu_ctx, grouped, passes):
    from pvsim import ASMKExpansion
    cent, images, queries, db, qe, wt = grouped
    sel = tw.selectivity(32, 3.0, 0.0)
    index = _index(gpu_ctx, cent, db, wt, 32)
    try:
        plain = index.rank_rows(queries, 10)
        assert _same_lists(plain, tw.rank(tw.scores(qe, db, wt, sel), 10))
        again = index.rank_rows(queries, 10, expand=None)                                       # None is today's path
        assert np.array_equal(plain[0], again[0]) and np.array_equal(_bits(plain[1]), _bits(again[1]))
        got = index.rank_rows(queries, 10, expand=ASMKExpansion(n=5, h_max=8, min_support=2, passes=passes))
        want = xt.rank_expanded(qe, db, wt, sel, 10, n=5, h_max=8, min_support=2, passes=passes)
        assert _same_lists(got, want)
        assert not np.array_equal(got[0], plain[0])                                             # the expansion moved something
        if passes == 1:
            lin = index.rank_rows(queries[:3], 10, expand=ASMKExpansion(n=5, h_max=8, min_support=2, scheme="linear"))
            assert _same_lists(lin, xt.rank_expanded(qe[:3], db, wt, sel, 10, n=5, h_max=8, min_support=2, scheme="linear"))
            # expand_entries: the entries themselves, in the layout of query_entries
            idx5 = tw.rank(tw.scores(qe, db, wt, sel), 5)[0]
            e = ASMKExpansion(n=5, h_max=8, min_support=2)
            members, votes = e.members_of(idx5)
            off, words, sigs = index.expand_entries(*_flat(qe, 1), members, votes, e)
            x, counts, _ = xt.expand(qe, *tw.invert(db, len(cent)), members, votes, 2, 8, 2, wt)
            assert np.array_equal(np.diff(off), counts) and np.array_equal(words, _flat(x, 1)[1]) and np.array_equal(sigs, _flat(x, 1)[2])
            with pytest.raises(TypeError):
                index.rank_rows(queries[:1], 5, expand="flat")
    finally:
        index.close()


def test_expansion_on_a_frozen_index_after_add_and_remove(gpu_ctx):
    from pvsim import ASMKExpansion
    cent, images, queries, _ = tw.planted_corpus()
    for x in images + queries:
        assert tw.labels_and_gap(x, cent)[1] > 1e-3
    db, qe = tw.entries(images, cent), tw.entries(queries[:12], cent)
    wt, sel = tw.word_weights(db, len(cent), True), tw.selectivity(32, 3.0, 0.0)
    e = ASMKExpansion(n=5, h_max=8, min_support=2)
    index = _index(gpu_ctx, cent, db[:90], wt, 32, frozen=True)
    try:
        assert _same_lists(index.rank_rows(queries[:12], 8, expand=e), xt.rank_expanded(qe, db[:90], wt, sel, 8, n=5, h_max=8, min_support=2))
        index.add([f"im{i}" for i in range(90, 96)], images[90:])
        gone = [0, 41, 93]
        index.remove([f"im{i}" for i in gone])
        left = [i for i in range(96) if i not in gone]
        assert index.paths == [f"im{i}" for i in left]
        for passes in (1, 2):
            got = index.rank_rows(queries[:12], 8, expand=ASMKExpansion(n=5, h_max=8, min_support=2, passes=passes))
            assert _same_lists(got, xt.rank_expanded(qe, [db[i] for i in left], wt, sel, 8, n=5, h_max=8, min_support=2, passes=passes))
    finally:
        index.close()


def test_expand_verified_with_a_hand_made_ranking(gpu_ctx):
    """the members are the first n paths of `ranked` with enough inliers, in that order for the linear votes"""
    import dsift_numpy as dtw
    from pvsim import ASMKExpansion, ASMKIndex
    from pvsim.features import KeypointSIFT
    from pvsim.verify import LocalFeatureIndex
    rng = np.random.RandomState(1850)
    K = 30
    proto = rng.randint(0, 80, (K, 128)).astype(np.uint8)
    cent = tw.rootsift(proto)
    images = [np.clip(proto[rng.randint(0, K, n)].astype(np.int64) + rng.randint(-2, 3, (n, 128)), 0, 255).astype(np.uint8)
              for n in [4, 1, 7, 25, 40, 3, 12, 30, 18, 9, 22, 5]]
    values = [tw.rootsift(r) for r in images]
    for x in values:
        assert tw.labels_and_gap(x, cent)[1] > 1e-3
    db = tw.entries(values, cent)
    wt, sel = tw.word_weights(db, K), tw.selectivity(128, 3.0, 0.0)
    query_image = np.clip(np.floor(dtw.texture(160, 200, 31, channels=1) + 0.5), 0, 255).astype(np.uint8)
    local = LocalFeatureIndex.from_arrays(images, [np.zeros((len(r), 6), F) for r in images], [f"im{i}" for i in range(12)], ctx=gpu_ctx)
    index = ASMKIndex.build(local, cent, extractor=KeypointSIFT(ctx=gpu_ctx))
    try:
        assert np.array_equal(index.wt, wt)
        off, words, sigs = index._image_entries([query_image], 1)                               # the query as the index sees it
        assert len(words) >= 3
        qe = [(words, sigs)]
        ranked = [("im7", 0.9, 12), ("im3", 0.8, 2), ("im4", 0.7, 9), ("im9", 0.6, 4), ("im1", 0.5, 0)]
        e = ASMKExpansion(n=2, min_support=1, scheme="linear")
        got = index.expand_verified(query_image, ranked, k=5, expand=e, min_inliers=4)
        want = xt.rank_expanded(qe, db, wt, sel, 5, n=2, h_max=32, min_support=1, scheme="linear", members=np.array([[4, 7]], np.int32),
                                votes=np.array([[1, 2]], np.int32))
        assert [p for p, _ in got] == [f"im{i}" for i in want[0][0]]
        assert np.array_equal(_bits(np.array([s for _, s in got], F)), _bits(want[1][0]))
        assert index.expand_verified(query_image, ranked, k=3, expand=e, min_inliers=50) == [(p, s) for p, s, _ in ranked[:3]]
        with pytest.raises(KeyError):
            index.expand_verified(query_image, [("nowhere", 1.0, 9)], k=3, expand=e)
        hits = index.retrieve(query_image, k=4, expand=ASMKExpansion(n=3, min_support=2))
        want = xt.rank_expanded(qe, db, wt, sel, 4, n=3, h_max=32, min_support=2)
        assert [p for p, _ in hits] == [f"im{i}" for i in want[0][0]]
    finally:
        index.close()
        local.close()
