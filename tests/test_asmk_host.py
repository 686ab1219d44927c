"""Host tests of the ASMK* index: the NumPy twin against itself (inverted file = pair loop), the integer
weights of pvsim.asmk against the twin, the guards, persistence, and retrieval quality on a planted corpus.  No device is needed."""
import numpy as np
import pytest

import asmk_numpy as tw
from pvsim import asmk, compact
from pvsim.asmk import ASMKIndex

F = np.float32


def _random_entries(rng, n_images, K, W, lo=0, hi=12):
    out = []
    for _ in range(n_images):
        words = np.sort(rng.permutation(K)[:rng.randint(lo, hi + 1)]).astype(np.int32)
        out.append((words, rng.randint(0, 1 << 32, (len(words), W), dtype=np.uint64).astype(np.uint32)))
    return out


def _flat(ents, W):
    off = np.zeros(len(ents) + 1, np.int64)
    np.cumsum([len(e[0]) for e in ents], out=off[1:])
    words = np.concatenate([e[0] for e in ents]) if ents else np.zeros(0, np.int32)
    sigs = np.concatenate([e[1].reshape(-1, W) for e in ents]) if ents else np.zeros((0, W), np.uint32)
    return off, words.astype(np.int32), sigs.astype(np.uint32)


# ------------------------------------------------------------------------------------------------ the twin against itself
@pytest.mark.parametrize("bits", [32, 64, 96, 128])
def test_inverted_file_score_equals_pair_loop(bits):
    rng = np.random.RandomState(100 + bits)
    K, W = 40, bits // 32
    db = _random_entries(rng, 30, K, W)
    db[3] = (np.zeros(0, np.int32), np.zeros((0, W), np.uint32))              # an image without entries
    qs = _random_entries(rng, 5, K, W) + [db[7], (np.zeros(0, np.int32), np.zeros((0, W), np.uint32))]
    wt, sel = tw.word_weights(db, K), tw.selectivity(bits, 3.0, 0.0)
    word_off, ent_img, ent_sig = tw.invert(db, K)
    gdb = np.array([tw.gamma(x[0], wt) for x in db], F)
    a = tw.scores(qs, db, wt, sel)
    b = tw.scores_inverted(qs, word_off, ent_img, ent_sig, len(db), wt, sel, gdb)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (a[:, 3].view(np.uint32) == 0).all() and (a[-1].view(np.uint32) == 0).all()
    assert a.max() > 0
    # entries are sorted by (word, image)
    for w in range(K):
        part = ent_img[word_off[w]:word_off[w + 1]]
        assert (np.diff(part) > 0).all()


def test_self_score_is_one():
    """acc = sum 1023 wt = s exactly; score = (fl(s) g) g with g = fl(1 / sqrt(s)): the conversion, g (twice) and the two products
    each add at most 2^-24 relative, so |score - 1| <= 5 * 2^-24 (1 + small)."""
    rng = np.random.RandomState(5)
    for bits, tau in ((32, 0.0), (128, 0.9)):
        db = _random_entries(rng, 20, 50, bits // 32, lo=1)
        wt, sel = tw.word_weights(db, 50), tw.selectivity(bits, 3.0, tau)
        s = tw.scores(db, db, wt, sel)
        assert np.abs(np.diag(s).astype(np.float64) - 1.0).max() <= 5.5 * 2.0 ** -24
        assert (s <= 1.0 + 5.5 * 2.0 ** -24).all()


def test_all_zero_selectivity_gives_plus_zero():
    rng = np.random.RandomState(6)
    db = _random_entries(rng, 10, 20, 1, lo=1)
    wt = tw.word_weights(db, 20)
    s = tw.scores(db, db, wt, np.zeros(33, np.int32))
    assert (s.view(np.uint32) == 0).all()
    # tau close to one keeps h = 0 alone
    sel = tw.selectivity(32, 3.0, 0.99)
    assert sel[0] == 1023 and not sel[1:].any()


def test_selectivity_and_weights_match_the_twin():
    for bits in (32, 64, 96, 128):
        for alpha, tau in ((3.0, 0.0), (1.0, 0.25), (2.5, 0.5), (0.5, 0.0)):
            a, b = asmk.selectivity(bits, alpha, tau), tw.selectivity(bits, alpha, tau)
            assert a.dtype == np.int32 and np.array_equal(a, b)
            assert a[0] == 1023 and (np.diff(a) <= 0).all() and not a[bits // 2:].any()
    rng = np.random.RandomState(7)
    K = 300
    db = _random_entries(rng, 64, K, 1, hi=40)
    off, words, sigs = _flat(db, 1)
    word_off, ent_img, ent_sig = asmk.invert(off, words, sigs, K)
    t_off, t_img, t_sig = tw.invert(db, K)
    assert np.array_equal(word_off, t_off) and np.array_equal(ent_img, t_img) and np.array_equal(ent_sig, t_sig)
    for idf in (True, False):
        wt = asmk.word_weights(np.diff(word_off), len(db), idf)
        assert wt.dtype == np.int32 and np.array_equal(wt, tw.word_weights(db, K, idf))
        g = asmk.gammas(off, words, wt)
        assert np.array_equal(g.view(np.uint32), np.array([tw.gamma(x[0], wt) for x in db], F).view(np.uint32))
    # a word every image holds: ln 1 = 0 is clipped to 1; a word one image of many holds is clipped to 1023 only beyond e^16 images
    assert asmk.word_weights([5, 0, 1], 5).tolist() == [1, 0, int(np.rint(64 * np.log(5.0)))]
    for bad in (dict(bits=48), dict(bits=32, alpha=0), dict(bits=32, tau=1.0), dict(bits=32, tau=-0.1)):
        with pytest.raises(ValueError):
            asmk.selectivity(**bad)


def test_random_projection_is_seeded_and_orthonormal():
    for bits, dim in ((64, 128), (32, 20), (32, 2), (128, 128)):
        p = asmk.random_projection(bits, dim, 3)
        assert p.dtype == F and p.shape == (bits, dim)
        assert np.array_equal(p, tw.random_projection(bits, dim, 3)) and not np.array_equal(p, asmk.random_projection(bits, dim, 4))
        g = p.astype(np.float64) @ p.astype(np.float64).T if bits <= dim else p.astype(np.float64).T @ p.astype(np.float64)
        assert np.abs(g - np.eye(len(g))).max() < 1e-6


def test_signature_bit_layout_and_centroid_row():
    cent = np.zeros((2, 32), F)
    cent[1] = 4
    x = np.zeros((3, 32), F)
    x[0] = cent[1]                          # on its centroid: V = +0 everywhere -> all ones
    x[1, :] = -1
    x[1, 5] = 1                             # word 0: bits 5 and 31 alone
    x[2, 31] = 2
    words, sigs = tw.image_entries(x, np.array([1, 0, 0]), cent)
    assert words.tolist() == [0, 1]
    assert sigs[1, 0] == 0xFFFFFFFF
    assert sigs[0, 0] == (1 << 5) | (1 << 31)
    with pytest.raises(NotImplementedError):
        tw.image_entries(np.zeros((8193, 32), F), np.zeros(8193, np.int32), cent)


# ------------------------------------------------------------------------------------------------ guards, persistence
def _index(n_images=6, K=65536, bits=32, wt_value=1023):
    W = bits // 32
    words = np.arange(n_images, dtype=np.int32)                     # image i holds word i
    off = np.arange(n_images + 1, dtype=np.int64)
    sigs = np.arange(n_images * W, dtype=np.uint32).reshape(n_images, W)
    word_off, ent_img, ent_sig = asmk.invert(off, words, sigs, K)
    wt = np.full(K, wt_value, np.int32)
    cent = np.zeros((K, bits), F)
    return ASMKIndex([f"img{i}" for i in range(n_images)], cent, word_off, ent_img, ent_sig, asmk.gammas(off, words, wt), wt,
                     asmk.selectivity(bits), bits)


def test_overflow_guard_raises_before_any_device_work():
    index = _index()
    n = 4105                                                         # 4105 * 1023 * 1023 >= 2^32 > 4104 * 1023 * 1023
    assert 4104 * 1023 * 1023 < 1 << 32 <= n * 1023 * 1023
    words = np.arange(n, dtype=np.int32)
    with pytest.raises(ValueError, match="overflow"):
        index.rank_entries(np.array([0, n], np.int64), words, np.zeros((n, 1), np.uint32), 3)
    with pytest.raises(ValueError):
        tw.check_query(words, index.wt)
    tw.check_query(words[:4104], index.wt)
    assert asmk._weight_sums(np.array([0, 4104], np.int64), words[:4104], index.wt)[0] < 1 << 32
    with pytest.raises(ValueError):
        index.rank_entries(np.array([0, 0], np.int64), words[:0], np.zeros((0, 1), np.uint32), 0)


def test_save_load_round_trip_and_foreign_files(tmp_path):
    index = _index(n_images=5, K=17, bits=64)
    p = str(tmp_path / "a.npz")
    index.save(p)
    back = ASMKIndex.load(p)
    for name in ("centroids", "word_off", "ent_img", "ent_sig", "gamma_db", "wt", "sel"):
        a, b = getattr(index, name), getattr(back, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert back.paths == index.paths and len(back) == 5 and back.bits == 64 and back.projection is None
    assert (back.alpha, back.tau, back.idf, back.desc_kind) == (index.alpha, index.tau, index.idf, index.desc_kind)
    assert np.array_equal(back.list_sizes(), np.diff(index.word_off)) and back.list_sizes().sum() == 5
    with pytest.raises(ValueError):
        compact.load_arrays(p)                                           # the compact loaders refuse it
    with pytest.raises(ValueError):
        compact.load_arrays(p, kind="ivf_compact_index")
    other = str(tmp_path / "c.npz")
    compact.save_arrays(other, ["x"], np.zeros((1, 2), np.uint8), np.ones(1, F), np.zeros((2, 4, 1), F))
    with pytest.raises(ValueError, match="ASMK"):
        ASMKIndex.load(other)                                            # and it refuses theirs
    # integer paths (LocalFeatureIndex.from_arrays without names) survive
    index._paths = list(range(5))
    index.save(p)
    assert ASMKIndex.load(p).paths == [0, 1, 2, 3, 4]


def test_add_and_remove_name_a_rebuild():
    index = _index(K=8)
    for call in (index.add, index.remove):
        with pytest.raises(NotImplementedError, match="rebuild"):
            call(["x"])


def test_constructor_checks_its_arrays():
    index = _index(K=8)
    args = dict(paths=index.paths, centroids=index.centroids, word_off=index.word_off, ent_img=index.ent_img, ent_sig=index.ent_sig,
                gamma_db=index.gamma_db, wt=index.wt, sel=index.sel, bits=32)
    ASMKIndex(**args)
    for change in (dict(bits=64), dict(word_off=index.word_off[:-1]), dict(gamma_db=index.gamma_db[:-1]), dict(ent_img=index.ent_img + 1),
                   dict(wt=index.wt[:-1]), dict(projection=np.zeros((32, 31), F))):
        with pytest.raises(ValueError):
            ASMKIndex(**{**args, **change})


# ------------------------------------------------------------------------------------------------ quality
def _recall_at_1(score, truth):
    return float((tw.rank(score, 1)[0][:, 0] == truth).mean())


def test_planted_corpus_recall():
    """D = B = 32, K = 64 lattice centroids, 96 images of 20..59 rows, 48 queries (half of an image's rows, a fifth of the
    coordinates moved by +-1, plus 20 clutter rows).  The selective kernel must find the planted image for >= 95 % of the
    queries and must not fall below the same score with a flat selectivity (word overlap alone)."""
    cent, images, queries, truth = tw.planted_corpus(seed=7)
    for x in images + queries:
        assert tw.labels_and_gap(x, cent)[1] > 1e-3
    db, qs = tw.entries(images, cent), tw.entries(queries, cent)
    wt = tw.word_weights(db, len(cent))
    asmk_recall = _recall_at_1(tw.scores(qs, db, wt, tw.selectivity(32, 3.0, 0.0)), truth)
    flat_recall = _recall_at_1(tw.scores(qs, db, wt, np.full(33, 1023, np.int32)), truth)
    print(f"planted corpus: recall@1 ASMK* {asmk_recall:.3f}, flat selectivity {flat_recall:.3f}")
    assert asmk_recall >= 0.95
    assert asmk_recall >= flat_recall
