"""NumPy twin of the ASMK query expansion (include/pvsim.h): the entries of a query, refined by the majority vote
of the signatures its members store for the same words and extended by the words enough members hold.

Written from the definition in the header, not from the kernel: plain loops over words, members and bits in Python integers; a list
is searched by walking it.  The device and pvsim.asmk must agree with this byte for byte.  Also here: the ranking flow of
`ASMKIndex.rank_*(..., expand=)` restated on the twin of the index (tests/asmk_numpy.py), the grouped corpus on which the
expansion's effect is measured, and mean average precision."""
import numpy as np

import asmk_numpy as tw

SCALE = 1023
MAX_MEMBERS = 32


def bit(sig, t):
    """bit t of a signature: uint32 word t / 32, position t % 32"""
    return (int(sig[t // 32]) >> (t % 32)) & 1


def pack(bits_list):
    out = np.zeros(len(bits_list) // 32, np.uint32)
    for t, b in enumerate(bits_list):
        if b:
            out[t // 32] |= np.uint32(1) << np.uint32(t % 32)
    return out


def members_of_row(members_row):
    """the members of a query: the ids before the first negative value"""
    out = []
    for i in members_row:
        if int(i) < 0:
            break
        out.append(int(i))
    return out


def stored_entries(word_off, ent_img, members):
    """{word: [(r, p)]}: member r's id stands at position p of the word's list; r ascending.  One walk over the file."""
    rank = {i: r for r, i in enumerate(members)}
    stored = {}
    if rank:
        img = np.asarray(ent_img).tolist()
        off = np.asarray(word_off).tolist()
        for w in range(len(off) - 1):
            for p in range(off[w], off[w + 1]):
                if img[p] in rank:
                    stored.setdefault(w, []).append((rank[img[p]], p))
    return {w: sorted(hits) for w, hits in stored.items()}


def expand_query(q_words, q_sigs, word_off, ent_img, ent_sig, members_row, votes_row, query_vote, h_max, min_support, wt):
    """one query -> (words int32 (count,) ascending, sigs uint32 (count, W), sum: Python int of 1023 wt[w] over the output)"""
    K, B = len(word_off) - 1, 32 * np.asarray(ent_sig).shape[1]
    assert 0 <= query_vote <= 65535 and 0 <= h_max <= B and 0 <= min_support <= MAX_MEMBERS + 1
    members = members_of_row(members_row)
    assert len(members) <= MAX_MEMBERS and all(a < b for a, b in zip(members, members[1:]))
    assert all(1 <= int(votes_row[r]) <= SCALE for r in range(len(members)))
    assert all(int(a) < int(b) for a, b in zip(q_words, q_words[1:]))
    where = {int(w): e for e, w in enumerate(q_words)}
    out_words, out_sigs, total = [], [], 0
    stored = stored_entries(word_off, ent_img, members)
    for w in sorted(set(stored) | {w for w in where if 0 <= w < K}):          # any other word has an empty M(w) and is no query word
        M = stored.get(w, [])
        if w in where:
            q_w = q_sigs[where[w]]
            voters = [(r, p) for r, p in M if tw.popcount(np.bitwise_xor(ent_sig[p], q_w)) <= h_max]   # the ORIGINAL signature
            new = []
            for t in range(B):
                tally = query_vote * (2 * bit(q_w, t) - 1) + sum(int(votes_row[r]) * (2 * bit(ent_sig[p], t) - 1) for r, p in voters)
                new.append(1 if tally > 0 else 0 if tally < 0 else bit(q_w, t))
        elif min_support >= 1 and len(M) >= min_support:
            new = [1 if sum(int(votes_row[r]) * (2 * bit(ent_sig[p], t) - 1) for r, p in M) >= 0 else 0 for t in range(B)]
        else:
            continue
        out_words.append(w)
        out_sigs.append(pack(new))
        total += SCALE * int(wt[w])
    W = B // 32
    return (np.array(out_words, np.int32), np.array(out_sigs, np.uint32).reshape(len(out_words), W), total)


def expand(q_entries, word_off, ent_img, ent_sig, members, votes, query_vote, h_max, min_support, wt):
    """q_entries: list of (words, sigs); members, votes: (nq, R) -> (list of (words, sigs), counts int64 (nq,), sums int64 (nq,))"""
    out, counts, sums = [], [], []
    for q, (qw, qs) in enumerate(q_entries):
        w, s, total = expand_query(qw, qs, word_off, ent_img, ent_sig, members[q], votes[q], query_vote, h_max, min_support, wt)
        out.append((w, s))
        counts.append(len(w))
        sums.append(total)
    return out, np.array(counts, np.int64), np.array(sums, np.int64)


# ------------------------------------------------------------------------------------------------ the ranking flow
def members_and_votes(idx, n, scheme="flat"):
    """ranked lists (nq, >= 0 slots, -1 where a slot is empty) -> (members (nq, n), votes (nq, n)): the filled slots among the first n,
    ids ascending, -1 behind them; "flat": vote 1; "linear": the member at rank j votes n - j"""
    nq = len(idx)
    members, votes = np.full((nq, n), -1, np.int32), np.zeros((nq, n), np.int32)
    for q in range(nq):
        pairs = sorted((int(i), 1 if scheme == "flat" else n - j) for j, i in enumerate(idx[q][:n]) if int(i) >= 0)
        for r, (i, v) in enumerate(pairs):
            members[q, r], votes[q, r] = i, v
    return members, votes


def rank_expanded(q_entries, db_entries, wt, sel, k, n, h_max, min_support, query_vote=None, scheme="flat", passes=1, members=None,
                  votes=None):
    """rank to depth n, expand by the lists' images, rank to depth k; `passes` > 1 repeats from the lists of the expanded query and
    always expands the original entries.  -> (idx, val) of tw.rank"""
    K, N = len(wt), len(db_entries)
    query_vote = (2 if scheme == "flat" else n) if query_vote is None else query_vote
    word_off, ent_img, ent_sig = tw.invert(db_entries, K)
    if members is None:
        idx, _ = tw.rank(tw.scores(q_entries, db_entries, wt, sel), min(n, N))
        members, votes = members_and_votes(idx, n, scheme)
    for p in range(passes):
        x, _, sums = expand(q_entries, word_off, ent_img, ent_sig, members, votes, query_vote, h_max, min_support, wt)
        assert all(int(s) == tw.weight_sum(e[0], wt) for s, e in zip(sums, x))
        last = p == passes - 1
        idx, val = tw.rank(tw.scores(x, db_entries, wt, sel), min(k if last else n, N))
        if not last:
            members, votes = members_and_votes(idx, n, scheme)
    return idx, val


# ------------------------------------------------------------------------------------------------ the grouped corpus
def grouped_corpus(seed=11, D=32, K=256, groups=24, views=6, feats=40, per_view=14, clutter=25, nq_feats=8, q_clutter=20, noise=0.25):
    """`groups` objects of `feats` features near lattice centroids; every object is seen in `views` images that each show `per_view`
    of its features (jittered) among `clutter` rows, and once more in a query of `nq_feats` features among `q_clutter` rows: two
    views of an object share few words, which is what query expansion is for.
    -> (centroids, images, group of every image, queries, group of every query)"""
    rng = np.random.RandomState(seed)
    cent = set()
    while len(cent) < K:
        cent.add(tuple((rng.randint(0, 2, D) * 4).tolist()))
    cent = np.array(sorted(cent), np.float32)

    def near(words):
        return (cent[words] + rng.randint(-1, 2, (len(words), D))).astype(np.float32)

    def jitter(x):
        move = rng.random_sample(x.shape) < noise
        return (x + move * rng.choice([-1.0, 1.0], x.shape)).astype(np.float32)

    images, group, queries, qgroup = [], [], [], []
    for g in range(groups):
        obj = near(rng.randint(0, K, feats))
        for v in range(views):
            pick = np.sort(rng.permutation(feats)[:per_view])
            images.append(np.concatenate([jitter(obj[pick]), near(rng.randint(0, K, clutter))]))
            group.append(g)
        pick = np.sort(rng.permutation(feats)[:nq_feats])
        queries.append(np.concatenate([jitter(obj[pick]), near(rng.randint(0, K, q_clutter))]))
        qgroup.append(g)
    return cent, images, np.array(group), queries, np.array(qgroup)


def mean_average_precision(idx, group, qgroup):
    """idx (nq, N): full rankings; an image is relevant iff it is in the query's group"""
    aps = []
    for q in range(len(idx)):
        rel = group[idx[q]] == qgroup[q]
        hits = np.cumsum(rel)
        aps.append(float((hits[rel] / (np.flatnonzero(rel) + 1.0)).mean()) if rel.any() else 0.0)
    return float(np.mean(aps))
