"""Host tests of ASMK maintenance: the NumPy twin of the four device entry points (tests/asmk_update_numpy.py)
against np.argsort(kind="stable"), pvsim.asmk.invert, np.delete and list concatenation; the frozen state of an index, its guards and
its persistence; and retrieval quality with weights learnt on a part of the corpus.  No device is needed."""
import numpy as np
import pytest

import asmk_numpy as tw
import asmk_update_numpy as up
from pvsim import asmk
from pvsim.asmk import ASMKIndex

F = np.float32


def _slots(rng, n, K, W, max_rows=9, empty=(), bad_words=False, all_words=None):
    """entries in slots as pvs_asmk_aggregate_dev leaves them: image i owns rows_i slots and fills the first count_i with ascending
    distinct words; the rest holds 0xFF bytes.  -> (offsets, count, word, sig, per-image list of (words, sigs))"""
    rows = [0 if i in empty else int(rng.randint(1, max_rows + 1)) for i in range(n)]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(rows, out=off[1:])
    total = int(off[-1])
    word = np.full(total, -1, np.int32)                                     # 0xFFFFFFFF
    sig = np.full((total, W), 0xFFFFFFFF, np.uint32)
    count, ents = np.zeros(n, np.int32), []
    for i in range(n):
        c = min(rows[i], K, int(rng.randint(0, rows[i] + 1))) if rows[i] else 0
        w = np.sort(rng.permutation(K)[:c]).astype(np.int32)
        if all_words is not None and rows[i]:
            w = np.unique(np.append(w[:max(rows[i] - 1, 0)], all_words)).astype(np.int32)
        c = len(w)
        s = rng.randint(0, 1 << 32, (c, W), dtype=np.uint64).astype(np.uint32)
        word[off[i]:off[i] + c], sig[off[i]:off[i] + c], count[i] = w, s, c
        ents.append((w, s))
    if bad_words and total:
        for i in range(n):                                                   # a word of -1 and a word of K: dropped
            if count[i] >= 2:
                word[off[i]], word[off[i] + count[i] - 1] = -1, K
                ents[i] = (ents[i][0][1:-1], ents[i][1][1:-1])
    return off, count, word, sig, ents


def _reference(ents, K, W, img_base=0):
    """np.argsort(kind="stable") on the compacted entries, as pvsim.asmk.invert sorts them"""
    ent_off = np.zeros(len(ents) + 1, np.int64)
    np.cumsum([len(e[0]) for e in ents], out=ent_off[1:])
    words = np.concatenate([e[0] for e in ents]).astype(np.int32) if ents else np.zeros(0, np.int32)
    sigs = np.concatenate([e[1].reshape(-1, W) for e in ents]).astype(np.uint32) if ents else np.zeros((0, W), np.uint32)
    word_off, img, sig = asmk.invert(ent_off, words, sigs, K)
    return word_off, img + np.int32(img_base), sig


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("K,W,tile", [(1, 1, 256), (2, 2, 0), (255, 3, 256), (256, 4, 512), (257, 1, 256), (1000, 4, 256), (65536, 2, 512)])
def test_twin_invert_equals_stable_argsort(K, W, tile):
    rng = np.random.RandomState(K + W)
    off, count, word, sig, ents = _slots(rng, 40, K, W, max_rows=40, empty=(0, 1, 17, 39), bad_words=K > 2)
    assert off[-1] > 2 * 256                                                 # the test's own input: more than two tiles of 256
    got = up.invert(off, count, word, sig, K, 1000, tile)
    want = _reference(ents, K, W, 1000)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert all(np.array_equal(g, w) for g, w in zip(up.invert(off, count, word, sig, K, 1000, 0), want))   # every tile, the same arrays
    assert all(np.array_equal(g, w) for g, w in zip(up.invert(off, count, word, sig, K), tw.invert(ents, K)))  # the twin of the index
    assert np.array_equal(up.weight_sums(off, count, word, np.arange(K) % 1024),
                          asmk._weight_sums(*_flat_entries(ents), np.arange(K) % 1024))


def _flat_entries(ents):
    ent_off = np.zeros(len(ents) + 1, np.int64)
    np.cumsum([len(e[0]) for e in ents], out=ent_off[1:])
    return ent_off, np.concatenate([e[0] for e in ents]).astype(np.int32) if ents else np.zeros(0, np.int32)


def test_twin_invert_edges():
    W = 2
    for n, rows in ((0, []), (1, [0]), (3, [0, 0, 0]), (1, [1])):
        off = np.zeros(n + 1, np.int64)
        np.cumsum(rows, out=off[1:])
        total = int(off[-1])
        word_off, img, sig = up.invert(off, np.array(rows, np.int32), np.zeros(total, np.int32), np.ones((total, W), np.uint32), 5)
        assert word_off.tolist() == [0] + [total] * 5 and img.tolist() == [0] * total and sig.shape == (total, W)
    # one word held by every image: its list crosses tiles of 256 in image order
    rng = np.random.RandomState(3)
    off, count, word, sig, ents = _slots(rng, 40, 300, W, max_rows=40, all_words=[299])
    word_off, img, _ = up.invert(off, count, word, sig, 300, 0, 256)
    assert off[-1] > 768 and img[word_off[299]:word_off[300]].tolist() == [i for i in range(40) if off[i + 1] > off[i]]
    # the tile the host chooses
    assert [up.resolve_tile(t, e) for t, e in ((10, 0), (10, 1), (10, 300), (10, 1 << 20), ((1 << 31) - 1, 256))] == [4096, 256, 512, 65536, 32768]


@pytest.mark.parametrize("K,W", [(1, 1), (7, 2), (300, 3), (300, 4)])
def test_twin_insert_and_remove_equal_a_rebuild(K, W):
    rng = np.random.RandomState(50 + K + W)
    ents = _slots(rng, 23, K, W, max_rows=6, empty=(4,))[4]
    if K == 300:                                                             # every list state: old empty, new empty, both, neither
        ents = [(e[0][e[0] % 4 != (1 if i < 15 else 2)], e[1][e[0] % 4 != (1 if i < 15 else 2)]) for i, e in enumerate(ents)]
        ents = [(e[0][e[0] % 4 != 3], e[1][e[0] % 4 != 3]) for e in ents]
    old, new = ents[:15], ents[15:]
    a, b, whole = _reference(old, K, W), _reference(new, K, W, 15), _reference(ents, K, W)
    got = up.insert(*a, *b)
    assert all(np.array_equal(g, w) for g, w in zip(got, whole))
    assert all(np.array_equal(g, w) for g, w in zip(up.insert(*_reference([], K, W), *whole), whole))      # into an empty file
    assert all(np.array_equal(g, w) for g, w in zip(up.insert(*whole, *_reference([], K, W)), whole))      # an empty batch
    for gone in ([], list(range(23)), [0], [22], list(range(0, 23, 2)), [3, 4, 11]):
        keep = np.ones(23, np.uint8)
        keep[gone] = 0
        got = up.remove(*whole, keep, up.keep_positions(keep))
        want = _reference([e for i, e in enumerate(ents) if keep[i]], K, W)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), gone
        # the same through np.delete on the stored arrays
        dead = np.flatnonzero(~keep[whole[1]].astype(bool))
        assert np.array_equal(got[2], np.delete(whole[2], dead, axis=0))
        assert np.array_equal(got[1], up.keep_positions(keep)[np.delete(whole[1], dead)])


# ------------------------------------------------------------------------------------------------ frozen state
def _index(n_images=6, K=16, bits=32):
    W = bits // 32
    words = np.arange(n_images, dtype=np.int32)                              # image i holds word i
    off = np.arange(n_images + 1, dtype=np.int64)
    sigs = np.arange(n_images * W, dtype=np.uint32).reshape(n_images, W)
    word_off, ent_img, ent_sig = asmk.invert(off, words, sigs, K)
    wt = asmk.word_weights(np.diff(word_off), n_images)
    return ASMKIndex([f"img{i}" for i in range(n_images)], np.zeros((K, bits), F), word_off, ent_img, ent_sig, asmk.gammas(off, words, wt),
                     wt, asmk.selectivity(bits), bits)


def test_weights_are_checked_before_device_work():
    cent = np.zeros((16, 128), F)
    for bad in (np.zeros(15, np.int32), np.zeros((16, 1), np.int32), np.zeros(16, F), np.full(16, 1024, np.int32), np.full(16, -1, np.int32),
                np.zeros(16, bool), [0.5] * 16):
        with pytest.raises(ValueError, match="weight"):
            ASMKIndex.build(None, cent, weights=bad)                          # no LocalFeatureIndex is touched
    assert asmk.check_weights(np.arange(16, dtype=np.int64) * 68, 16).dtype == np.int32
    with pytest.raises(ValueError, match="on_device"):
        ASMKIndex.build(None, cent, on_device=1)


def test_freeze_bounds_and_the_default_changes_nothing():
    index = _index()
    assert index.frozen is False and (index.wt[6:] == 0).all() and (index.wt[:6] > 0).all()
    for bad in (-1, 1024, 1.0, True, None, "0"):
        with pytest.raises(ValueError, match="unseen_weight"):
            index.freeze(bad)
    assert index.frozen is False
    before = index.wt.copy()
    assert index.freeze() is index and index.frozen is True and np.array_equal(index.wt, before)
    with pytest.raises(AttributeError):
        index.frozen = False
    other = _index().freeze(unseen_weight=64)
    assert np.array_equal(other.wt[:6], before[:6]) and (other.wt[6:] == 64).all() and other.wt.dtype == np.int32


def test_unfrozen_index_names_a_rebuild_for_any_arguments():
    index = _index()
    for call, args, kwargs in ((index.add, (), {}), (index.add, (["x"],), {}), (index.add, (1, 2, 3), {"nonsense": 4}),
                               (index.remove, (), {}), (index.remove, (["nowhere"], 5), {"x": 1}), (index.remove, (object(),), {})):
        with pytest.raises(NotImplementedError, match="rebuild") as e:
            call(*args, **kwargs)
        assert "freeze()" in str(e.value) and "weights=" in str(e.value)
    with pytest.raises(NotImplementedError, match="rebuild"):
        del index["img0"]


def test_frozen_index_checks_paths_before_device_work():
    index = _index().freeze()
    row = np.zeros((1, 32), np.uint8)
    with pytest.raises(ValueError, match="already"):
        index.add(["new", "img3"], [row, row])
    with pytest.raises(ValueError, match="already"):
        index.add(["new", "new"], [row, row])
    with pytest.raises(ValueError):
        index.add(["new"], [row, row])
    with pytest.raises(NotImplementedError, match="8192"):
        index.add(["new"], [np.zeros((8193, 32), np.uint8)])
    with pytest.raises(KeyError):
        index.remove(["img1", "nowhere"])
    with pytest.raises(ValueError, match="twice"):
        index.remove(["img1", "img2", "img1"])
    with pytest.raises(KeyError):
        del index["nowhere"]
    assert index.add([], []) is index and index.remove([]) is index         # empty updates touch no device
    assert index._dev is None and index.paths == [f"img{i}" for i in range(6)] and len(index.ent_img) == 6


def test_frozen_key_round_trips(tmp_path):
    index = _index()
    p, q = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    index.save(p)
    assert ASMKIndex.load(p).frozen is False
    index.freeze().save(q)
    back = ASMKIndex.load(q)
    assert back.frozen is True and np.array_equal(back.wt, index.wt) and np.array_equal(back.ent_img, index.ent_img)
    with np.load(q, allow_pickle=False) as z:
        assert z["params"].shape == (5,) and bool(z["frozen"]) is True
        legacy = {k: z[k] for k in z.files if k != "frozen"}
    np.savez(p, **legacy)                                                    # a file from before the key existed
    assert ASMKIndex.load(p).frozen is False


# ------------------------------------------------------------------------------------------------ quality
def test_planted_corpus_recall_with_frozen_weights():
    """weights from the first 64 of the 96 images, all 96 indexed with them: recall@1 must reach the bound of
    test_asmk_host.py::test_planted_corpus_recall"""
    cent, images, queries, truth = tw.planted_corpus(seed=7)
    db, qs = tw.entries(images, cent), tw.entries(queries, cent)
    wt, full = tw.word_weights(db[:64], len(cent)), tw.word_weights(db, len(cent))
    score = tw.scores(qs, db, wt, tw.selectivity(32, 3.0, 0.0))
    recall = float((tw.rank(score, 1)[0][:, 0] == truth).mean())
    print(f"planted corpus, weights of 64 images: recall@1 {recall:.3f}; {int((wt != full).sum())} of {len(wt)} weights differ")
    assert (wt != full).any()
    assert recall >= 0.95
