"""CPU tests of the NumPy twin of k-reciprocal re-ranking (tests/reciprocal_numpy.py): the planted facts on
hand-made lists, the identities the definitions promise, and the quality measurement on the two planted corpora.  The GPU tests
(tests/test_gpu_reciprocal.py) hold the device to this twin bit for bit, so what is checked here by hand is what the device does."""
import numpy as np

import diffusion_numpy as dn
import reciprocal_numpy as tw

E_ = -1                                     # an empty slot

# 8 rows, kg = 6, k1 = 6 (k1h = 3).  Row 0 lists 1, 2, 3 (who list it back) and 5 (who does not).  H(1) = {1, 0, 2, 4} and
# H(2) = {2, 0, 1, 6} share 3 of their 4 ids with B(0) = {0, 1, 2, 3}: 9 > 8, they join, and 4 and 6 are not in row 0.  H(3) =
# {3, 0, 7} shares 2 of 3: 6 > 6 fails by one element.  Row 5 lists 6 and 7, who do not list it: no reciprocal slot.
HAND = np.array([[1, 2, 3, 5, E_, E_],
                 [0, 2, 4, E_, E_, E_],
                 [0, 1, 6, E_, E_, E_],
                 [0, 7, E_, E_, E_, E_],
                 [1, E_, E_, E_, E_, E_],
                 [6, 7, E_, E_, E_, E_],
                 [2, E_, E_, E_, E_, E_],
                 [3, E_, E_, E_, E_, E_]], np.int32)
HAND_SIM = np.where(HAND >= 0, np.float32(0.9) - np.float32(0.1) * np.arange(6, dtype=np.float32)[None, :], np.float32(0)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_planted_facts_on_hand_made_lists():
    db = tw.database(HAND, HAND_SIM, k1=6, k2=1, gamma=2)
    assert db["mask1"][0] == 0b0111 and db["maskh"][0] == 0b0111                   # the one-sided neighbour 5 is in neither
    assert db["mask1"][1] == 0b111 and tw.h_set(1, db["nbr"], db["maskh"]) == {1, 0, 2, 4}
    assert tw.h_set(2, db["nbr"], db["maskh"]) == {2, 0, 1, 6} and tw.h_set(3, db["nbr"], db["maskh"]) == {3, 0, 7}
    B, E = tw.expanded_set(0, [1, 2, 3], db["nbr"], db["maskh"])
    assert B == {0, 1, 2, 3} and E == {0, 1, 2, 3, 4, 6}                            # H(3) fails by one element: 7 stays out
    assert db["members"][0].tolist() == [1, 1, 1, 0, 0, 0] and db["dropped"][0] == 2  # 4 and 6 are dropped and counted
    assert db["mask1"][5] == 0 and not db["members"][5].any() and db["dropped"][5] == 0   # the isolated row
    assert db["v0"][5] == 1.0 and not db["v"][5].any() and db["w0"][5] == 1.0 and db["ws"][5] == 1.0
    a = [float(np.float32(x)) ** 2 for x in HAND_SIM[0, :3]]                        # gamma = 2: one product
    s = ((0.0 + 1.0) + a[0]) + a[1]
    s = s + a[2]
    assert db["v0"][0] == 1.0 / s and db["v"][0].tolist() == [a[0] / s, a[1] / s, a[2] / s, 0.0, 0.0, 0.0]
    assert np.array_equal(_bits(db["w"]), _bits(db["v"])) and np.array_equal(_bits(db["w0"]), _bits(db["v0"]))     # k2 = 1
    # row 4 lists 1 alone and 1 lists it back at slot 2 < 6: B(4) = {4, 1}; H(1) shares {1, 4} of 4 ids: 6 > 8 fails
    assert db["members"][4].tolist() == [1, 0, 0, 0, 0, 0] and db["dropped"][4] == 0


def test_local_expansion_by_hand():
    db = tw.database(HAND, HAND_SIM, k1=6, k2=3, gamma=2)
    v, v0, nbr = db["v"], db["v0"], db["nbr"]
    # row 4: sources 4, then nbr[4][0] = 1 (slot 1 holds -1 and is skipped); support {4, 1}
    assert db["w0"][4] == ((0.0 + v0[4]) + v[1, 2]) / 3.0                            # V_1[4] = v[1][2]
    assert db["w"][4, 0] == ((0.0 + v[4, 0]) + v0[1]) / 3.0 and not db["w"][4, 1:].any()
    assert db["ws"][4] == (0.0 + db["w0"][4]) + db["w"][4, 0]
    # row 0, slot 3 holds 5, who is no member: sources 0, 1, 2 hold nothing for it
    assert db["w"][0, 3] == 0.0
    # ... but a slot that is no member of its own row can still receive weight: 2 sits in rows 0 and 1, the sources of row 0
    assert db["w"][0, 1] == (((0.0 + v[0, 1]) + v[1, 1]) + v0[2]) / 3.0


def test_query_rules_by_hand():
    lists = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, E_]], np.int32)      # 0..3 a clique; 4 lists 0 and 1 one-sided
    sim = np.array([[.9, .8, .7], [.9, .8, .6], [.8, .8, .5], [.7, .6, .5], [.4, .3, 0]], np.float32)
    db = tw.database(lists, sim, k1=3, k2=1, gamma=1)
    thr = sim[:, 2]                                                                   # sim[g][k1 - 1]
    qidx = np.array([[0, 1, 2, 4], [0, 1, 2, 4], [4, 0, E_, 0]], np.int64)
    qval = np.array([[thr[0], np.nextafter(thr[1], np.float32(0)), .9, .9],           # exactly on the threshold: in; one ulp below: out
                     [.1, .1, .1, .1],
                     [.9, thr[0], 0, .95]], np.float32)
    wq, sq, dropped, flags = tw.query(db, qidx, qval)
    # query 0: B = {0, 2}; H(0) = {0, 1, 2} (k1h = 2) shares 2 of 3 and fails, H(2) = {2, 0, 1} too; row 4's slot 2 holds -1
    assert flags[0].tolist() == [1, 0, 1, 0] and dropped[0] == 0
    s = (0.0 + float(thr[0])) + float(np.float32(.9))
    assert wq[0].tolist() == [float(thr[0]) / s, 0.0, float(np.float32(.9)) / s, 0.0] and sq[0] == (0.0 + wq[0, 0]) + wq[0, 2]
    # query 1: below every threshold: no member, every weight +0, J = +0 and the score is lambda * cosine
    assert not flags[1].any() and sq[1] == 0.0
    sc = tw.score(db, qidx, qval, wq, sq, 4, 0.25)
    assert sc[1].tolist() == [0.75 * 0.0 + 0.25 * float(np.float32(.1))] * 4
    # query 2: 0 sits in slots 1 and 3: the first counts, the reciprocity test is on slot 1 alone
    assert flags[2].tolist() == [0, 1, 0, 0] and wq[2, 1] == wq[2, 3] == 1.0 and wq[2, 2] == 0.0
    idx, val, rep = tw.rerank(db, qidx, qval, 4, 4, 1.0)                             # lambda = 1: the first ranking, ties by position
    assert np.array_equal(idx[0], qidx[0][np.lexsort((np.arange(4), -qval[0].astype(np.float64)))])
    assert val[1].tolist() == [float(np.float32(.1))] * 4 and idx[1].tolist() == [0, 1, 2, 4]


def test_scores_by_hand():
    lists = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, E_]], np.int32)
    sim = np.array([[.9, .8, .7], [.9, .8, .6], [.8, .8, .5], [.7, .6, .5], [.4, .3, 0]], np.float32)
    db = tw.database(lists, sim, k1=3, k2=2, gamma=3)
    qidx = np.array([[1, 0, 3]], np.int64)
    qval = np.array([[.95, .9, .55]], np.float32)
    wq, sq, dropped, flags = tw.query(db, qidx, qval)
    sc = tw.score(db, qidx, qval, wq, sq, 2, 0.3)
    w, w0, ws = db["w"], db["w0"], db["ws"]
    m = 0.0 + min(wq[0, 0], w0[1])                                                    # candidate 1: self, then its slots 0 (id 0), 1 (id 2: not in the list), 2 (id 3)
    m = m + min(wq[0, 1], w[1, 0])
    m = m + min(wq[0, 2], w[1, 2])
    J = m / ((sq[0] + ws[1]) - m)
    assert sc[0, 0] == 0.7 * J + 0.3 * float(np.float32(.95)) and 0 < J <= 1
    assert sc.shape == (1, 2)                                                         # kr < kq


def test_helps_on_the_blobs_corpus_and_is_recorded_on_the_curves():
    """32 blobs x 32 rows in 64-d at spread 1.6, 256 queries, seed 0; kg = 40, k1 = 20, k2 = 6, kq = kr = 80, gamma = 3, lambda = 0.3.
    Measured with the twin: precision@20 0.6713 plain, 0.8961 re-ranked (gain 0.2248), 0.8434 with k2 = 1; the dense algorithm of
    the paper with the same weights, no truncation and the whole database re-ranked reaches 0.9090 (recorded, no threshold); 9.5 %
    of the members are dropped by the truncation.  On the curves corpus of diffusion_numpy: 0.7619 plain, 0.8303 re-ranked, 0.8631
    dense (diffusion reaches 1.0000 there: the two methods mend different failures).  The run is deterministic; the asserted margin
    of half the measured gain only guards against later edits of the generator.  The plain ranking is the baseline, never the code
    under test."""
    X, lab, Q, ql = tw.blobs(seed=0)
    assert X.shape == (1024, 64) and Q.shape == (256, 64) and X.dtype == np.float32
    nbr, sim = tw.lists(X, 40)
    qi, qv = tw.cosine_rank(Q, X, 80)
    qv = qv.astype(np.float32)
    plain = tw.precision(qi[:, :20], lab, ql)
    got = {}
    for k2 in (6, 1):
        db = tw.database(nbr, sim, 20, k2, 3)
        idx, val, rep = tw.rerank(db, qi, qv, 20, 80, 0.3)
        got[k2] = tw.precision(idx, lab, ql)
        assert (np.diff(val, axis=1) <= 0).all() and all(len(set(r)) == 20 for r in idx.tolist())
    frac = db["dropped"].sum() / (db["dropped"].sum() + db["members"].sum())
    dense = tw.precision(tw.dense_rerank(X, Q, 20), lab, ql)
    print(f"blobs precision@20: plain {plain:.4f}, re-ranked {got[6]:.4f}, k2 = 1 {got[1]:.4f}, dense {dense:.4f}, dropped {frac:.3f}")
    assert got[6] >= plain + 0.112
    assert got[6] >= got[1]
    X, lab, Q, ql = dn.curves(seed=0)
    nbr, sim = tw.lists(X, 40)
    qi, qv = tw.cosine_rank(Q, X, 80)
    idx = tw.rerank(tw.database(nbr, sim, 20, 6, 3), qi, qv.astype(np.float32), 20, 80, 0.3)[0]
    print(f"curves precision@20: plain {tw.precision(qi[:, :20], lab, ql):.4f}, re-ranked {tw.precision(idx, lab, ql):.4f}, "
          f"dense {tw.precision(tw.dense_rerank(X, Q, 20), lab, ql):.4f}")
